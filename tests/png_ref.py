"""Reference for the PNG encoder (include/gs2m_png.h): numpy and pure Python, no GPU.

    filter_stream(image)            the row-filter rule, byte for byte
    segments(H, W, CH)              the segmentation and the stored worst case
    adler32_combine(a1, a2, len2)   Adler-32 of a concatenation from the parts'
    parse_png(data)                 chunk walk with CRC check -> IHDR fields and the zlib stream
    strict_inflate(stream, lens)    a bit-level inflater that holds the stream to the contract of section 17
    png_container / BitWriter / write_dynamic_block   what the tests build their own files and streams with
"""
import struct
import zlib

import numpy as np

SEGMENT_BYTES = 32768
MAX_STRIDE = 65536
ADLER = 65521
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOR_TYPE = {1: 0, 3: 2, 4: 6}


class InflateError(ValueError):
    pass


# ---- row filter --------------------------------------------------------------------------------------------------------------

def _as_hwc(image):
    a = np.asarray(image)
    if a.ndim == 2:
        a = a[:, :, None]
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] in (1, 3, 4), (a.dtype, a.shape)
    return a


def filter_rows(image):
    """-> (H, 1 + W CH) uint8: per row the filter byte and the filtered bytes.  The five PNG filters (bytes left of the row and the
    row above row 0 are 0), each priced at sum(v < 128 ? v : 256 - v); the cheapest wins, ties go to the lowest filter number."""
    a = _as_hwc(image)
    H, W, CH = a.shape
    rows = a.reshape(H, W * CH).astype(np.int32)
    out = np.empty((H, 1 + W * CH), np.uint8)
    zero = np.zeros(W * CH, np.int32)
    for y in range(H):
        x = rows[y]
        b = rows[y - 1] if y > 0 else zero
        left = np.concatenate([np.zeros(CH, np.int32), x[:-CH]]) if W > 1 else zero
        c = (np.concatenate([np.zeros(CH, np.int32), b[:-CH]]) if W > 1 else zero)
        p = left + b - c
        pa, pb, pc = np.abs(p - left), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, b, c))
        cands = [x & 255, (x - left) & 255, (x - b) & 255, (x - ((left + b) >> 1)) & 255, (x - paeth) & 255]
        costs = [int(np.where(v < 128, v, 256 - v).sum()) for v in cands]
        best = costs.index(min(costs))
        out[y, 0] = best
        out[y, 1:] = cands[best]
    return out


def filter_stream(image):
    """the filtered stream of an image: H records [filter byte][W CH filtered bytes], as bytes"""
    return filter_rows(image).tobytes()


# ---- the tests' images ---------------------------------------------------------------------------------------------------------

def make_image(kind, H, W, seed=0):
    """Seeded test images: "a" an RGB gradient plus noise of +-6, "b" RGBA: a disc of "a" on zeros with alpha 0 / 255, "c" the red
    channel of "a" (one channel), "d" the constant 137 (RGB), "noise" uniform random RGB."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    grad = np.stack([x * 255 // max(W - 1, 1), y * 255 // max(H - 1, 1), (x + y) * 255 // max(W + H - 2, 1)], axis=2)
    a = np.clip(grad + rng.integers(-6, 7, size=(H, W, 3)), 0, 255).astype(np.uint8)
    if kind == "a":
        return a
    if kind == "b":
        inside = (x - W / 2) ** 2 + (y - H / 2) ** 2 <= (0.4 * min(H, W)) ** 2
        out = np.zeros((H, W, 4), np.uint8)
        out[inside, :3] = a[inside]
        out[inside, 3] = 255
        return out
    if kind == "c":
        return np.ascontiguousarray(a[:, :, :1])
    if kind == "d":
        return np.full((H, W, 3), 137, np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    raise ValueError(kind)


# ---- segments ----------------------------------------------------------------------------------------------------------------

def stored_bytes(n):
    return n + 5 * ((n + 65534) // 65535)


def segments(H, W, CH):
    """-> dict: stride, rows_per_segment, n_segments, lengths (bytes of each segment), max_stream_bytes (every segment stored);
    ValueError for the sizes the encoder refuses."""
    if H < 1 or W < 1 or CH not in (1, 3, 4):
        raise ValueError("bad shape")
    stride = 1 + W * CH
    if stride > MAX_STRIDE or H * stride > 2 ** 31 - 1:
        raise ValueError("unsupported size")
    rps = max(1, SEGMENT_BYTES // stride)
    n = (H + rps - 1) // rps
    lengths = [(min(H, (s + 1) * rps) - s * rps) * stride for s in range(n)]
    return dict(stride=stride, rows_per_segment=rps, n_segments=n, lengths=lengths,
                max_stream_bytes=2 + sum(stored_bytes(x) for x in lengths) + 5 * (n - 1) + 4)


# ---- Adler-32 ----------------------------------------------------------------------------------------------------------------

def adler32_combine(adler1, adler2, len2):
    """zlib.adler32(x + y) from zlib.adler32(x), zlib.adler32(y) and len(y)"""
    a1, b1 = adler1 & 0xFFFF, adler1 >> 16
    a2, b2 = adler2 & 0xFFFF, adler2 >> 16
    a = (a1 + a2 - 1) % ADLER
    b = (b1 + b2 + len2 * (a1 - 1)) % ADLER
    return (b << 16) | a


# ---- container ---------------------------------------------------------------------------------------------------------------

def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def png_container(W, H, CH, zstream):
    """the tests' own container writer: signature, IHDR, one IDAT, IEND"""
    return (PNG_SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, COLOR_TYPE[CH], 0, 0, 0)) + _chunk(b"IDAT", zstream)
            + _chunk(b"IEND", b""))


def parse_png(data):
    """-> dict(width, height, bit_depth, color_type, compression, filter, interlace, chunks=[names], zlib=the IDAT bytes joined);
    ValueError on a bad signature, a bad CRC, a truncated chunk, bytes behind IEND or a missing IHDR / IDAT / IEND."""
    if data[:8] != PNG_SIGNATURE:
        raise ValueError("bad signature")
    pos, names, idat, hdr = 8, [], [], None
    while pos < len(data):
        if pos + 12 > len(data):
            raise ValueError("truncated chunk")
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind = data[pos + 4:pos + 8]
        if pos + 12 + n > len(data):
            raise ValueError("truncated chunk")
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if crc != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise ValueError(f"bad CRC in {kind!r}")
        names.append(kind.decode("latin1"))
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        pos += 12 + n
        if kind == b"IEND":
            break
    if pos != len(data):
        raise ValueError("bytes behind IEND")
    if hdr is None or not idat or names[0] != "IHDR" or names[-1] != "IEND":
        raise ValueError(f"chunks {names}")
    return dict(width=hdr[0], height=hdr[1], bit_depth=hdr[2], color_type=hdr[3], compression=hdr[4], filter=hdr[5], interlace=hdr[6],
                chunks=names, zlib=b"".join(idat))


# ---- strict inflate ------------------------------------------------------------------------------------------------------------

def check_code_lengths(lengths, limit, kind):
    """Holds a set of code lengths to the contract; `kind`: "codelen" (limit 7, complete), "litlen" (limit 15, complete, symbol 256
    present) or "dist" (limit 15; complete, or no length at all, or a single length of 1).  Raises InflateError."""
    lengths = list(lengths)
    if any(l > limit for l in lengths):
        raise InflateError(f"{kind}: a code length above {limit}")
    used = [l for l in lengths if l > 0]
    kraft = sum(1 << (limit - l) for l in used)
    full = 1 << limit
    if kind == "dist":
        if not used or used == [1]:
            return
        if kraft != full:
            raise InflateError("dist: malformed distance code (neither complete, nor empty, nor a single code of one bit)")
        return
    if kraft > full:
        raise InflateError(f"{kind}: over-subscribed code")
    if kraft < full:
        raise InflateError(f"{kind}: incomplete code")
    if kind == "litlen" and (len(lengths) <= 256 or lengths[256] == 0):
        raise InflateError("litlen: the end-of-block symbol has no code")


def _decode_table(lengths, maxbits):
    """peek of `maxbits` bits (LSB first) -> symbol << 4 | length; 0 where no code matches"""
    lengths = np.asarray(lengths, np.int64)
    table = np.zeros(1 << maxbits, np.int64)
    code = 0
    for l in range(1, maxbits + 1):
        code <<= 1
        for sym in np.nonzero(lengths == l)[0]:
            rev = int(format(code, f"0{l}b")[::-1], 2)
            table[rev::1 << l] = (int(sym) << 4) | l
            code += 1
    return table.tolist()


_FIXED = None


def _fixed_tables():
    global _FIXED
    if _FIXED is None:
        lit = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
        _FIXED = (_decode_table(lit, 15), _decode_table([5] * 32, 15))
    return _FIXED


class _Bits:
    def __init__(self, data, pos):
        self.data, self.pos, self.buf, self.cnt = data, pos, 0, 0

    def need(self, n):
        while self.cnt < n:
            chunk = self.data[self.pos:self.pos + 4]
            if not chunk:
                raise InflateError("the stream ends inside a block")
            self.buf |= int.from_bytes(chunk, "little") << self.cnt
            self.pos += len(chunk)
            self.cnt += 8 * len(chunk)

    def take(self, n):
        if n == 0:
            return 0
        self.need(n)
        v = self.buf & ((1 << n) - 1)
        self.buf >>= n
        self.cnt -= n
        return v

    def align(self):
        """drop the bits up to the byte boundary -> the byte position; the buffer is emptied"""
        drop = self.cnt % 8
        pad = self.buf & ((1 << drop) - 1)
        self.buf >>= drop
        self.cnt -= drop
        byte = self.pos - self.cnt // 8
        self.pos, self.buf, self.cnt = byte, 0, 0
        return byte, pad

    def at_byte_boundary(self):
        return self.cnt % 8 == 0

    def byte_pos(self):
        return self.pos - self.cnt // 8


def strict_inflate(stream, segment_lengths):
    """Inflates a zlib stream whose deflate data is cut into segments of `segment_lengths` output bytes, and holds it to the
    contract: -> (output bytes, tokens), tokens a list of ints (literals) and (length, distance) pairs.  Raises InflateError on
      * a code length above 15, or above 7 for the code-length code (check_code_lengths; the bit format itself cannot carry them);
      * an over-subscribed or incomplete literal/length (or code-length) code; a missing end-of-block code;
      * a distance code that is neither complete, nor empty, nor a single code of one bit; a match where there is no distance code;
      * a distance that reaches before the current segment's first byte;
      * a segment that does not end, after exactly its planned number of bytes, in an empty stored block at a byte boundary
        (BFINAL 0, BTYPE 0, LEN 0) -- or, for the last one, in a block with the final bit; a final bit or an empty stored block
        anywhere else;
      * trailing garbage, a bad zlib header, a wrong Adler-32."""
    data = bytes(stream)
    if len(data) < 6:
        raise InflateError("the stream is shorter than a zlib wrapper")
    if (data[0] & 15) != 8 or (data[0] >> 4) > 7 or ((data[0] << 8) | data[1]) % 31 != 0 or (data[1] & 0x20):
        raise InflateError("bad zlib header")
    seg_ends = np.cumsum(np.asarray(segment_lengths, np.int64)).tolist()
    if not seg_ends or any(l < 1 for l in segment_lengths):
        raise InflateError("segment lengths")
    bits = _Bits(data, 2)
    out = bytearray()
    tokens = []
    seg, seg_start = 0, 0
    done = False
    while not done:
        seg_end = seg_ends[seg]
        last_seg = seg == len(seg_ends) - 1
        final = bits.take(1)
        btype = bits.take(2)
        if btype == 3:
            raise InflateError("block type 3")
        if btype == 0:
            byte, _ = bits.align()
            if byte + 4 > len(data):
                raise InflateError("the stream ends inside a block")
            ln, nln = struct.unpack("<HH", data[byte:byte + 4])
            if ln ^ nln != 0xFFFF:
                raise InflateError("stored block: LEN / NLEN")
            if ln == 0:
                raise InflateError("an empty stored block inside a segment")
            if byte + 4 + ln > len(data):
                raise InflateError("the stream ends inside a block")
            out += data[byte + 4:byte + 4 + ln]
            tokens.extend(data[byte + 4:byte + 4 + ln])
            bits.pos = byte + 4 + ln
        else:
            if btype == 1:
                lit_table, dist_table = _fixed_tables()
                have_dist = True
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                if hlit > 286 or hdist > 30:
                    raise InflateError("too many length or distance symbols")
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = bits.take(3)
                check_code_lengths(cl, 7, "codelen")
                cl_table = _decode_table(cl, 7)
                lens = []
                while len(lens) < hlit + hdist:
                    try:
                        bits.need(7)
                    except InflateError:
                        pass  # the last bytes of the stream: the test below sees a code that runs past them
                    e = cl_table[bits.buf & 127]
                    if e == 0 or (e & 15) > bits.cnt:
                        raise InflateError("the stream ends inside a block")
                    bits.take(e & 15)
                    sym = e >> 4
                    if sym < 16:
                        lens.append(sym)
                    elif sym == 16:
                        if not lens:
                            raise InflateError("repeat code without a previous length")
                        lens.extend([lens[-1]] * (3 + bits.take(2)))
                    elif sym == 17:
                        lens.extend([0] * (3 + bits.take(3)))
                    else:
                        lens.extend([0] * (11 + bits.take(7)))
                if len(lens) != hlit + hdist:
                    raise InflateError("a repeat code runs past the last length")
                check_code_lengths(lens[:hlit], 15, "litlen")
                check_code_lengths(lens[hlit:], 15, "dist")
                have_dist = any(lens[hlit:])
                lit_table = _decode_table(lens[:hlit], 15)
                dist_table = _decode_table(lens[hlit:], 15) if have_dist else None
            # the block's symbols (locals: this loop is the hot one)
            buf, cnt, pos = bits.buf, bits.cnt, bits.pos
            n_data = len(data)
            while True:
                if cnt < 48:
                    chunk = data[pos:pos + 4]
                    buf |= int.from_bytes(chunk, "little") << cnt
                    pos += len(chunk)
                    cnt += 8 * len(chunk)
                e = lit_table[buf & 0x7FFF]
                l = e & 15
                if l == 0 or l > cnt:
                    raise InflateError("the stream ends inside a block" if pos >= n_data else "invalid literal/length code")
                buf >>= l
                cnt -= l
                sym = e >> 4
                if sym < 256:
                    out.append(sym)
                    tokens.append(sym)
                    continue
                if sym == 256:
                    break
                if sym > 285:
                    raise InflateError("invalid literal/length symbol")
                eb = LEN_EXTRA[sym - 257]
                length = LEN_BASE[sym - 257] + (buf & ((1 << eb) - 1))
                buf >>= eb
                cnt -= eb
                if not have_dist:
                    raise InflateError("a match in a block without a distance code")
                e = dist_table[buf & 0x7FFF]
                l = e & 15
                if l == 0 or l > cnt:
                    raise InflateError("invalid distance code")
                buf >>= l
                cnt -= l
                dsym = e >> 4
                if dsym > 29:
                    raise InflateError("invalid distance symbol")
                eb = DIST_EXTRA[dsym]
                dist = DIST_BASE[dsym] + (buf & ((1 << eb) - 1))
                buf >>= eb
                cnt -= eb
                if cnt < 0:
                    raise InflateError("the stream ends inside a block")
                if dist > len(out) - seg_start:
                    raise InflateError("a distance reaches before the segment's first byte")
                if dist == 1:
                    out += out[-1:] * length
                else:
                    for _ in range(length):
                        out.append(out[-dist])
                tokens.append((length, dist))
            if cnt < 0:
                raise InflateError("the stream ends inside a block")
            bits.buf, bits.cnt, bits.pos = buf, cnt, pos
        # ---- the end of a block
        if len(out) > seg_end:
            raise InflateError("a block crosses the planned end of its segment")
        if len(out) < seg_end:
            if final:
                raise InflateError("the final bit inside a segment")
            continue
        if last_seg:
            if not final:
                raise InflateError("the last block lacks the final bit")
            done = True
        else:
            if final:
                raise InflateError("the final bit in front of the last segment")
            if bits.take(1) != 0 or bits.take(2) != 0:
                raise InflateError("a segment does not end in an empty stored block")
            byte, _ = bits.align()
            if data[byte:byte + 4] != b"\x00\x00\xff\xff":
                raise InflateError("a segment does not end in an empty stored block")
            bits.pos = byte + 4
            seg += 1
            seg_start = len(out)
    byte, _ = bits.align()
    if byte + 4 > len(data):
        raise InflateError("the Adler-32 is missing")
    if byte + 4 < len(data):
        raise InflateError("trailing garbage")
    if struct.unpack(">I", data[byte:byte + 4])[0] != (zlib.adler32(bytes(out)) & 0xFFFFFFFF):
        raise InflateError("wrong Adler-32")
    return bytes(out), tokens


# ---- a bit writer, for the streams the tests make by hand ----------------------------------------------------------------------

class BitWriter:
    def __init__(self):
        self.out, self.buf, self.cnt = bytearray(), 0, 0

    def bits(self, value, n):
        """n bits of value, LSB first (headers, extra bits)"""
        self.buf |= (value & ((1 << n) - 1)) << self.cnt
        self.cnt += n
        while self.cnt >= 8:
            self.out.append(self.buf & 255)
            self.buf >>= 8
            self.cnt -= 8

    def code(self, code, n):
        """a Huffman code of n bits, most significant bit first"""
        self.bits(int(format(code, f"0{n}b")[::-1], 2) if n else 0, n)

    def align(self):
        if self.cnt:
            self.bits(0, 8 - self.cnt)

    def raw(self, data):
        self.align()
        self.out += data

    def done(self):
        self.align()
        return bytes(self.out)


def canonical_codes(lengths):
    """{symbol: (code, length)} of the canonical Huffman code of `lengths` (no completeness check)"""
    codes, code = {}, 0
    for l in range(1, max(list(lengths) + [0]) + 1):
        code <<= 1
        for sym, sl in enumerate(lengths):
            if sl == l:
                codes[sym] = (code, l)
                code += 1
    return codes


def write_dynamic_block(bw, lit_lengths, dist_lengths, tokens, final, cl_lengths=None, end_of_block=True):
    """One BTYPE 2 block: `lit_lengths` (257 .. 286 entries), `dist_lengths` (1 .. 30 entries), tokens as strict_inflate
    returns them.  The header spells every length out with the code-length symbols 0 .. 15 under `cl_lengths` (default: 4 bits
    each, a complete code).  Nothing is checked: the tests write malformed blocks with it."""
    cl = list(cl_lengths) if cl_lengths is not None else [4] * 16 + [0, 0, 0]
    clc = canonical_codes(cl)
    bw.bits(1 if final else 0, 1)
    bw.bits(2, 2)
    bw.bits(len(lit_lengths) - 257, 5)
    bw.bits(len(dist_lengths) - 1, 5)
    bw.bits(19 - 4, 4)
    for s in CL_ORDER:
        bw.bits(cl[s], 3)
    for l in list(lit_lengths) + list(dist_lengths):
        bw.code(*clc[l])
    lc, dc = canonical_codes(lit_lengths), canonical_codes(dist_lengths)
    for t in tokens:
        if isinstance(t, int):
            bw.code(*lc[t])
            continue
        length, dist = t
        k = 28 if length == 258 else max(i for i in range(28) if LEN_BASE[i] <= length)
        bw.code(*lc[257 + k])
        bw.bits(length - LEN_BASE[k], LEN_EXTRA[k])
        j = max(i for i in range(30) if DIST_BASE[i] <= dist)
        if j in dc:  # (a block written without the distance code carries no distance: malformed on purpose)
            bw.code(*dc[j])
            bw.bits(dist - DIST_BASE[j], DIST_EXTRA[j])
    if end_of_block:
        bw.code(*lc[256])
