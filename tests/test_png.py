"""The PNG encoder's reference (tests/png_ref.py) checked against Pillow and zlib, and the host-only part of the product
(gs2m_png_plan, the container, the CPU refusal): no GPU."""
import ctypes
import io
import zlib

import numpy as np
import pytest

import png_ref as R

KINDS = ("a", "b", "c", "d")


def _zlib_segments(data, lengths, strategy=zlib.Z_RLE, level=6):
    """zlib's own stream cut into independent segments: a full flush (an empty stored block, the window reset) behind each"""
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    out, pos = b"", 0
    for i, n in enumerate(lengths):
        out += co.compress(data[pos:pos + n])
        out += co.flush(zlib.Z_FULL_FLUSH if i < len(lengths) - 1 else zlib.Z_FINISH)
        pos += n
    return out


# ---- the filter restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(96, 160), (5, 5), (1, 7), (7, 1), (1, 1)])
def test_pillow_decodes_the_filtered_stream_to_the_image(kind, shape):
    from PIL import Image
    img = R.make_image(kind, *shape)
    H, W, CH = img.shape
    rows = R.filter_rows(img)
    assert rows.shape == (H, 1 + W * CH) and set(rows[:, 0].tolist()) <= {0, 1, 2, 3, 4}
    data = R.png_container(W, H, CH, zlib.compress(R.filter_stream(img)))
    with Image.open(io.BytesIO(data)) as im:
        im.load()
        assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[CH] and im.size == (W, H)
        assert np.array_equal(np.asarray(im).reshape(H, W, CH), img)
    hdr = R.parse_png(data)
    assert (hdr["width"], hdr["height"], hdr["bit_depth"], hdr["color_type"], hdr["interlace"]) == (W, H, 8, R.COLOR_TYPE[CH], 0)
    assert zlib.decompress(hdr["zlib"]) == rows.tobytes()


def test_the_generator_exercises_all_five_filters():
    used = {k: set(R.filter_rows(R.make_image(k, 96, 160))[:, 0].tolist()) for k in KINDS}
    assert set().union(*used.values()) == {0, 1, 2, 3, 4}, used


def test_filter_choice_takes_the_cheapest_and_the_lowest_number_on_ties():
    zero = np.zeros((3, 4, 3), np.uint8)
    assert R.filter_rows(zero)[:, 0].tolist() == [0, 0, 0]  # every filter costs 0
    const = np.full((3, 4, 1), 200, np.uint8)
    assert R.filter_rows(const)[:, 0].tolist() == [1, 2, 2]  # row 0: Sub 56 (Paeth ties it); below: Up 0 (Paeth ties it)
    assert R.filter_rows(const)[0, 1:].tolist() == [200, 0, 0, 0]


def test_parse_png_rejects_a_bad_crc_and_trailing_bytes():
    img = R.make_image("c", 5, 5)
    data = R.png_container(5, 5, 1, zlib.compress(R.filter_stream(img)))
    R.parse_png(data)
    bad = bytearray(data)
    bad[40] ^= 1
    with pytest.raises(ValueError):
        R.parse_png(bytes(bad))
    with pytest.raises(ValueError):
        R.parse_png(data + b"\0")
    with pytest.raises(ValueError):
        R.parse_png(b"\0" + data[1:])


# ---- Adler-32 and segments ---------------------------------------------------------------------------------------------------

def test_adler32_combine_over_random_splits():
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, 200000, dtype=np.uint8).tobytes() + b"\xff" * 70000
    for _ in range(20):
        cuts = sorted(rng.integers(0, len(data) + 1, rng.integers(1, 9)).tolist())
        parts = [data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])]
        acc = zlib.adler32(parts[0])
        for p in parts[1:]:
            acc = R.adler32_combine(acc, zlib.adler32(p), len(p))
        assert acc == zlib.adler32(data), cuts


def test_segments():
    s = R.segments(96, 160, 3)
    assert (s["stride"], s["rows_per_segment"], s["n_segments"], s["lengths"]) == (481, 68, 2, [68 * 481, 28 * 481])
    assert R.segments(96, 160, 1)["n_segments"] == 1
    s = R.segments(3, 8200, 4)
    assert (s["stride"], s["rows_per_segment"], s["n_segments"]) == (32801, 1, 3)
    assert R.segments(600, 800, 3)["n_segments"] == 47 and R.segments(600, 800, 4)["n_segments"] == 60
    with pytest.raises(ValueError):
        R.segments(2, 16384, 4)  # stride 65537
    s = R.segments(2, 65535, 1)  # the longest record: 65536 bytes, two stored blocks
    assert s["lengths"] == [65536, 65536] and s["max_stream_bytes"] == 2 + 2 * (65536 + 10) + 5 + 4
    with pytest.raises(ValueError):
        R.segments(2 ** 31 // 4 + 1, 1, 3)


@pytest.mark.parametrize("shape", [(96, 160, 3), (96, 160, 4), (96, 160, 1), (1, 1, 3), (7, 1, 3), (3, 8200, 4), (600, 800, 3), (600, 800, 4),
                                   (2, 65535, 1), (1200, 1600, 3), (100000, 2, 1)])
def test_plan_through_ctypes_equals_the_reference(shape):
    import gs2m_png
    H, W, CH = shape
    want = R.segments(H, W, CH)
    got = gs2m_png.plan(H, W, CH, 3)
    assert {k: got[k] for k in ("stride", "rows_per_segment", "n_segments", "max_stream_bytes")} == {k: want[k] for k in ("stride", "rows_per_segment", "n_segments", "max_stream_bytes")}
    assert got["workspace_bytes"] >= 3 * (H * want["stride"] + want["max_stream_bytes"]) and got["workspace_bytes"] % 256 == 0
    assert gs2m_png.plan(H, W, CH, 1)["n_segments"] == got["n_segments"]  # segmentation does not depend on N


def test_plan_refuses_what_the_contract_refuses():
    import gs2m_native as N
    L = N.lib()
    out = [ctypes.c_longlong(-7) for _ in range(4)]
    refs = [ctypes.byref(o) for o in out]
    assert L.gs2m_png_plan(2, 16384, 4, 1, *refs) == -4          # stride 65537
    assert L.gs2m_png_plan(2, 65535, 1, 1, *refs) == 0           # stride 65536
    assert L.gs2m_png_plan(2 ** 31 // 4 + 1, 1, 3, 1, *[ctypes.byref(ctypes.c_longlong()) for _ in range(4)]) == -4  # H stride > 2^31 - 1
    for H, W, CH, n in ((0, 4, 3, 1), (4, 0, 3, 1), (4, 4, 2, 1), (4, 4, 5, 1), (4, 4, 3, 0), (-1, 4, 3, 1)):
        fresh = [ctypes.c_longlong(-7) for _ in range(4)]
        assert L.gs2m_png_plan(H, W, CH, n, *[ctypes.byref(o) for o in fresh]) == -1, (H, W, CH, n)
        assert all(o.value == -7 for o in fresh)
    assert L.gs2m_png_plan(4, 4, 3, 1, None, None, None, None) == 0  # every output is optional


def test_the_module_refuses_cpu_tensors():
    import torch
    import gs2m_png
    img = torch.zeros(4, 4, 3, dtype=torch.uint8)
    for fn in (gs2m_png.filter_rows, gs2m_png.encode, gs2m_png.encode_streams):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(img)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gs2m_png.save([img], ["x.png"])
    with pytest.raises(ValueError):
        gs2m_png.Writer("gpu")


def test_container_is_a_png_pillow_reads():
    from PIL import Image
    import gs2m_png
    img = R.make_image("b", 9, 11)
    data = gs2m_png.container(11, 9, 4, zlib.compress(R.filter_stream(img)))
    assert data == R.png_container(11, 9, 4, zlib.compress(R.filter_stream(img)))
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), img)


# ---- strict_inflate ------------------------------------------------------------------------------------------------------------

def _payload():
    return R.filter_stream(R.make_image("b", 96, 160)), R.segments(96, 160, 4)["lengths"]


@pytest.mark.parametrize("strategy, level", [(zlib.Z_RLE, 6), (zlib.Z_HUFFMAN_ONLY, 6), (zlib.Z_DEFAULT_STRATEGY, 0), (zlib.Z_FIXED, 6),
                                             (zlib.Z_DEFAULT_STRATEGY, 9)])
def test_strict_inflate_equals_zlib_on_zlib_made_streams(strategy, level):
    data, lengths = _payload()
    for lens in ([len(data)], lengths):
        if level == 0:  # (a compressobj closes a level-0 stream with an empty final stored block, which the contract has no place for)
            if len(lens) > 1:
                continue
            z = zlib.compress(data, 0)
        else:
            z = _zlib_segments(data, lens, strategy, level)
        out, tokens = R.strict_inflate(z, lens)
        assert out == zlib.decompress(z) == data
        assert sum(1 if isinstance(t, int) else t[0] for t in tokens) == len(data)
        if strategy == zlib.Z_RLE:
            assert all(isinstance(t, int) or t[1] == 1 for t in tokens) and any(not isinstance(t, int) for t in tokens)
        if strategy == zlib.Z_HUFFMAN_ONLY or level == 0:
            assert all(isinstance(t, int) for t in tokens)


LIT = [0] * 286
for _s in (65, 66, 256, 257):  # 'A', 'B', end of block, length 3: four codes of two bits
    LIT[_s] = 2
TOKENS = [65, 66, (3, 1), 65, (3, 1)]
PLAIN = b"ABBBBAAAA"


def _hand_stream(blocks, plain=PLAIN, adler=None, tail=b""):
    bw = R.BitWriter()
    bw.raw(b"\x78\x01")
    for write in blocks:
        write(bw)
    bw.raw(struct_adler(plain if adler is None else adler))
    return bw.done() + tail


def struct_adler(data):
    return (zlib.adler32(data) & 0xFFFFFFFF).to_bytes(4, "big")


def _sync(bw):
    bw.bits(0, 3)
    bw.raw(b"\x00\x00\xff\xff")


def test_strict_inflate_accepts_the_hand_made_streams_it_is_tested_with():
    """the well-formed twins of the corrupted streams below, zlib agreeing"""
    for dist, tokens, plain in (([1], TOKENS, PLAIN), ([0], [65, 66, 66], b"ABB"), ([1, 1], TOKENS, PLAIN)):
        z = _hand_stream([lambda bw: R.write_dynamic_block(bw, LIT, dist, tokens, True)], plain)
        assert R.strict_inflate(z, [len(plain)]) == (plain, tokens)
        assert zlib.decompress(z) == plain
    two = _hand_stream([lambda bw: R.write_dynamic_block(bw, LIT, [1], TOKENS, False), _sync,
                        lambda bw: R.write_dynamic_block(bw, LIT, [0], [66, 65], True)], PLAIN + b"BA")
    assert R.strict_inflate(two, [9, 2])[0] == zlib.decompress(two) == PLAIN + b"BA"


def _rejects(z, lengths, what):
    with pytest.raises(R.InflateError, match=what):
        R.strict_inflate(z, lengths)


def test_strict_inflate_rejects_each_kind_of_malformed_stream():
    dyn = lambda **kw: (lambda bw: R.write_dynamic_block(bw, kw.pop("lit", LIT), kw.pop("dist", [1]), kw.pop("tokens", TOKENS), kw.pop("final", True), **kw))
    # code lengths above the limits: the bit format cannot carry them (3 bits per code-length length, symbols 0 .. 15), the check is there
    with pytest.raises(R.InflateError, match="above 15"):
        R.check_code_lengths([16, 1], 15, "litlen")
    with pytest.raises(R.InflateError, match="above 7"):
        R.check_code_lengths([8, 1], 7, "codelen")
    over = list(LIT); over[67] = 2
    _rejects(_hand_stream([dyn(lit=over)]), [9], "over-subscribed")
    under = list(LIT); under[257] = 3
    _rejects(_hand_stream([dyn(lit=under, tokens=[65, 66, 66])], b"ABB"), [3], "incomplete")
    _rejects(_hand_stream([dyn(cl_lengths=[4] * 15 + [0] * 4)]), [9], "codelen: incomplete")
    no_eob = [0] * 286
    for s in (65, 66, 257, 258):
        no_eob[s] = 2
    _rejects(_hand_stream([dyn(lit=no_eob, end_of_block=False)]), [9], "end-of-block")
    _rejects(_hand_stream([dyn(dist=[2])]), [9], "malformed distance code")       # one code of two bits
    _rejects(_hand_stream([dyn(dist=[1, 2])]), [9], "malformed distance code")    # incomplete, two codes
    _rejects(_hand_stream([dyn(dist=[0])]), [9], "without a distance code")       # a match, no distance code
    # a distance that reaches before the segment: the second segment opens with a match
    _rejects(_hand_stream([dyn(final=False), _sync, dyn(tokens=[(3, 1), 65])], PLAIN + b"AAAA"), [9, 4], "before the segment")
    _rejects(_hand_stream([dyn(tokens=[(3, 1), 65])], b"\0\0\0A"), [4], "before the segment")
    # segment ends
    _rejects(_hand_stream([dyn(final=False), dyn(tokens=[66, 65])], PLAIN + b"BA"), [9, 2], "empty stored block")  # no sync block
    _rejects(_hand_stream([dyn(final=False), _sync, dyn(tokens=[66, 65])], PLAIN + b"BA"), [8, 3], "crosses")       # not at the planned byte
    _rejects(_hand_stream([dyn(final=False), _sync, dyn(tokens=[66, 65], final=False), _sync, dyn(tokens=[65])], PLAIN + b"BAA"), [9, 3],
             "empty stored block inside")
    _rejects(_hand_stream([dyn(final=True), _sync, dyn(tokens=[66, 65])], PLAIN + b"BA"), [9, 2], "final bit in front")
    _rejects(_hand_stream([dyn(final=False)]), [9], "final bit")                   # the last block lacks it
    _rejects(_hand_stream([dyn()], tail=b"\0"), [9], "trailing garbage")
    _rejects(_hand_stream([dyn()], adler=b"ABBBBAAAB"), [9], "Adler")
    _rejects(_hand_stream([dyn()])[:-2], [9], "Adler-32 is missing")
    _rejects(b"\x78\x02" + _hand_stream([dyn()])[2:], [9], "zlib header")
    # and a zlib stream with one bit flipped in its last block's data or trailer never passes as it is
    data, lengths = _payload()
    z = bytearray(_zlib_segments(data, lengths))
    z[-1] ^= 1
    _rejects(bytes(z), lengths, "Adler")
