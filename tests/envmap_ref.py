"""numpy restatement of the environment-map stage (include/gs2m_envmap.h), straight from the formulas: the Radiance
RGBE codec with a writer for run-length coded, flat and mixed files, the scan, and the lat-long -> cube-map conversion in a chosen
float type (float64: the reference; float32: the yardstick of what fp32 arithmetic costs)."""
import numpy as np

ROW_FLAT, ROW_RLE = 0, 1
OK, INVALID = 0, -1
TRUNCATED, ZERO_CODE, OVERRUN, TRAILING, OLD_RLE = -10, -11, -12, -13, -14
TOP = 255.0 * 2.0 ** 119  # the largest value of the format


# ---- codec ---------------------------------------------------------------------------------------------------------------------

def rgbe_to_float(rgbe):
    """(..., 4) uint8 -> (..., 3) float32: e == 0 -> 0, else m 2^(e - 136); exact."""
    rgbe = np.asarray(rgbe, dtype=np.uint8)
    e = rgbe[..., 3:4].astype(np.int64)
    val = np.ldexp(rgbe[..., :3].astype(np.float64), e - 136)
    out = np.where(e == 0, 0.0, val).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), np.where(e == 0, 0.0, val))  # exact in fp32
    return out


def float_to_rgbe(image):
    """(..., 3) float32 -> (..., 4) uint8, as gs2m_hdr_encode: negatives and NaN -> 0, +inf -> the largest finite fp32, components limited
    to 255 2^119; v = max < 1e-32 -> 0 0 0 0; else (f, e) = frexp(v), bytes trunc(c 2^(8 - e)) and e + 128."""
    c = np.asarray(image, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        c = np.where(c > 0.0, c, 0.0)  # NaN, negatives, -inf
    c = np.minimum(c, float(np.finfo(np.float32).max))
    c = np.minimum(c, TOP)
    v = c.max(axis=-1)
    _, e = np.frexp(v)
    m = np.floor(np.ldexp(c, (8 - e)[..., None])).astype(np.int64)
    assert m.max(initial=0) <= 255
    out = np.concatenate([m, (e + 128)[..., None]], axis=-1)
    out = np.where((v < float(np.float32(1e-32)))[..., None], 0, out)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def rle_plane(vals):
    """One channel plane -> its new-style RLE coding: runs of at least 4 equal bytes become run codes of at most 127 (longer runs are
    split), everything else literals of at most 128."""
    vals = [int(v) for v in vals]
    out, lit, i, n = bytearray(), [], 0, len(vals)

    def flush():
        while lit:
            out.append(min(len(lit), 128))
            out.extend(lit[:128])
            del lit[:128]

    while i < n:
        j = i
        while j < n and vals[j] == vals[i]:
            j += 1
        if j - i >= 4:
            flush()
            run = j - i
            while run > 0:
                k = min(run, 127)
                out.extend((128 + k, vals[i]))
                run -= k
        else:
            lit.extend(vals[i:j])
        i = j
    flush()
    return bytes(out)


def write_pixels(rgbe, kinds="rle"):
    """(H, W, 4) uint8 -> the pixel bytes; `kinds`: "rle", "flat", "mixed" (alternating, RLE first) or one of the two per row.  A row
    whose width new-style RLE cannot carry (W < 8 or W > 32767) is written flat."""
    rgbe = np.asarray(rgbe, dtype=np.uint8)
    h, w, _ = rgbe.shape
    if isinstance(kinds, str):
        kinds = [("rle", "flat")[r % 2] if kinds == "mixed" else kinds for r in range(h)]
    out = bytearray()
    for r in range(h):
        if kinds[r] == "rle" and 8 <= w <= 32767:
            out.extend((2, 2, w >> 8, w & 255))
            for c in range(4):
                out.extend(rle_plane(rgbe[r, :, c]))
        else:
            out.extend(rgbe[r].tobytes())
    return bytes(out)


def hdr_file(pixels, w, h, magic=b"#?RADIANCE", lines=(b"FORMAT=32-bit_rle_rgbe",), resolution=None):
    res = resolution if resolution is not None else f"-Y {h} +X {w}".encode()
    return magic + b"\n" + b"".join(ln + b"\n" for ln in lines) + b"\n" + res + b"\n" + pixels


def scan(pixels, W, H):
    """gs2m_hdr_scan: -> (code, table (H, 5) int64 of {kind, o0 .. o3}; rows behind a refused one are zero)."""
    b, n = bytes(pixels), len(pixels)
    table = np.zeros((max(H, 1), 5), dtype=np.int64)
    if W < 1 or H < 1:
        return INVALID, table
    pos = 0
    for row in range(H):
        rle = 8 <= W <= 32767 and n - pos >= 4 and b[pos] == 2 and b[pos + 1] == 2 and (b[pos + 2] << 8 | b[pos + 3]) == W
        if not rle:
            if n - pos < 4 * W:
                return TRUNCATED, table
            px = np.frombuffer(b, np.uint8, 4 * W, pos).reshape(W, 4)
            if ((px[:, 0] == 1) & (px[:, 1] == 1) & (px[:, 2] == 1)).any():
                return OLD_RLE, table
            table[row] = (ROW_FLAT, pos, pos + 1, pos + 2, pos + 3)
            pos += 4 * W
            continue
        table[row, 0] = ROW_RLE
        pos += 4
        for c in range(4):
            table[row, 1 + c] = pos
            x = 0
            while x < W:
                if pos >= n:
                    return TRUNCATED, table
                code = b[pos]
                if code == 0:
                    return ZERO_CODE, table
                k = code - 128 if code > 128 else code
                if x + k > W:
                    return OVERRUN, table
                nxt = pos + (2 if code > 128 else 1 + k)
                if nxt > n:
                    return TRUNCATED, table
                x, pos = x + k, nxt
    return (OK if pos == n else TRAILING), table


def expand(pixels, W, H):
    """-> (H, W, 4) uint8 of an accepted file."""
    code, table = scan(pixels, W, H)
    assert code == OK, code
    b = bytes(pixels)
    out = np.zeros((H, W, 4), dtype=np.uint8)
    for row in range(H):
        kind, offs = table[row, 0], table[row, 1:]
        for c in range(4):
            if kind == ROW_FLAT:
                out[row, :, c] = np.frombuffer(b, np.uint8, 4 * W, offs[0])[c::4]
                continue
            pos, x = int(offs[c]), 0
            while x < W:
                code = b[pos]
                if code > 128:
                    out[row, x:x + code - 128, c] = b[pos + 1]
                    x, pos = x + code - 128, pos + 2
                else:
                    out[row, x:x + code, c] = np.frombuffer(b, np.uint8, code, pos + 1)
                    x, pos = x + code, pos + 1 + code
    return out


def decode(pixels, W, H):
    return rgbe_to_float(expand(pixels, W, H))


def sample_rgbe(w, h, seed=0):
    """(h, w, 4) uint8 with long and short runs, and the edge values: e = 0 (with non-zero mantissas), e = 255, e = 1, mantissas 255 and 0"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    for r in range(h):
        x = 0
        while x < w:  # runs of assorted lengths in every plane, 127 and longer among them
            k = int(rng.choice([1, 2, 3, 4, 5, 9, 126, 127, 128, 129, 260]))
            for c in range(4):
                if rng.random() < 0.6:
                    img[r, x:x + k, c] = rng.integers(0, 256)
            x += k
    edge = np.array([[7, 9, 200, 0], [255, 255, 255, 255], [255, 0, 1, 1], [0, 0, 0, 128], [255, 128, 127, 136], [1, 2, 3, 9], [3, 1, 1, 5]], dtype=np.uint8)
    flat = img.reshape(-1, 4)
    flat[:min(len(edge), len(flat))] = edge[:len(flat)]
    flat[(flat[:, 0] == 1) & (flat[:, 1] == 1) & (flat[:, 2] == 1), 2] = 2  # no old-style repeat markers
    return img


# ---- conversion ----------------------------------------------------------------------------------------------------------------

def cube_to_dir(f, x, y):
    """pbr/light.py cube_to_dir"""
    one = np.ones_like(x)
    return ((one, -y, -x), (-one, -y, x), (x, one, y), (x, -one, -y), (x, -y, one), (-x, -y, -one))[f]


def latlong_dirs(hs, ws, dtype=np.float64):
    """(hs, ws, 3): the directions of a lat-long image's pixel centres; export_envmap's reflvec at its own resolution."""
    theta = ((np.arange(hs, dtype=dtype) + 0.5) / hs * np.pi)[:, None]
    phi = (((np.arange(ws, dtype=dtype) + 0.5) * 2 / ws - 1) * np.pi)[None, :]
    return np.stack(np.broadcast_arrays(np.sin(theta) * np.sin(phi), np.cos(theta), -np.sin(theta) * np.cos(phi)), axis=-1)


def export_dirs(res):
    """(res[0], res[1], 3): CubemapLight.export_envmap's own sample directions (its linspace grids, not the pixel centres)"""
    gy = np.linspace(0.0 + 1.0 / res[0], 1.0 - 1.0 / res[0], res[0])[:, None] * np.pi
    gx = np.linspace(-1.0 + 1.0 / res[1], 1.0 - 1.0 / res[1], res[1])[None, :] * np.pi
    return np.stack(np.broadcast_arrays(np.sin(gy) * np.sin(gx), np.cos(gy), -np.sin(gy) * np.cos(gx)), axis=-1)


def sample_taps(hs, ws, R, S, angle=0.0, dtype=np.float64):
    """The taps of every sub-sample: -> (w, (y0, y1, x0, x1), (tu, tv)), arrays of shape (6, R, S, R, S) indexed [f, r, a, c, b]."""
    T = dtype
    pi, one, half = T(np.pi), T(1), T(0.5)
    k = np.arange(R * S, dtype=np.int64)
    coord = (-one + (2 * k + 1).astype(T) / T(R * S)).astype(T)
    y, x = np.meshgrid(coord, coord, indexing="ij")
    inv = (one / np.sqrt((one + x * x) + y * y)).astype(T)
    w = ((inv * inv) * inv).astype(T)
    ca, sa = T(np.cos(np.float64(angle))), T(np.sin(np.float64(angle)))
    ws_, hs_ = T(ws), T(hs)
    W6, idx, frac = [], [], []
    for f in range(6):
        dx, dy, dz = (np.asarray(c, dtype=T) * inv for c in cube_to_dir(f, x, y))
        rx, rz = ca * dx - sa * dz, sa * dx + ca * dz
        theta = np.arccos(np.clip(dy, -one, one)).astype(T)
        phi = np.arctan2(rx, -rz).astype(T)
        u = ((phi / pi + one) * half * ws_ - half).astype(T)
        v = (theta / pi * hs_ - half).astype(T)
        uf, vf = np.floor(u), np.floor(v)
        iu, iv = uf.astype(np.int64), vf.astype(np.int64)
        idx.append((np.clip(iv, 0, hs - 1), np.clip(iv + 1, 0, hs - 1), iu % ws, (iu + 1) % ws))
        frac.append(((u - uf).astype(T), (v - vf).astype(T)))
        W6.append(w)
    shape = (6, R, S, R, S)
    pack = lambda arrs: np.stack(arrs).reshape(shape)
    return (pack(W6), tuple(pack([i[k] for i in idx]) for k in range(4)), tuple(pack([fr[k] for fr in frac]) for k in range(2)))


def latlong_to_cubemap(src, R, S, angle=0.0, scale=1.0, dtype=np.float64):
    """gs2m_latlong_to_cubemap in `dtype` arithmetic: (Hs, Ws, 3) -> (6, R, R, 3)."""
    T = dtype
    src = np.asarray(src).astype(T)
    hs, ws, _ = src.shape
    w, (y0, y1, x0, x1), (tu, tv) = sample_taps(hs, ws, R, S, angle, T)
    tu, tv = tu[..., None], tv[..., None]
    a00, a01, a10, a11 = src[y0, x0], src[y0, x1], src[y1, x0], src[y1, x1]
    top = a00 + tu * (a01 - a00)
    bot = a10 + tu * (a11 - a10)
    L = (top + tv * (bot - top)).astype(T)
    wl = (w[..., None] * L).astype(T)
    acc, wsum = np.zeros((6, R, R, 3), dtype=T), np.zeros((6, R, R), dtype=T)
    for a in range(S):  # the sub-samples added in (a, b) order
        for b in range(S):
            acc = (acc + wl[:, :, a, :, b]).astype(T)
            wsum = (wsum + w[:, :, a, :, b]).astype(T)
    return (T(scale) * (acc / wsum[..., None])).astype(T)


def texel_dirs(R, dtype=np.float64):
    """(6, R, R, 3) unit directions of the texel centres"""
    c = -1 + (2 * np.arange(R, dtype=dtype) + 1) / R
    y, x = np.meshgrid(c, c, indexing="ij")
    d = np.stack([np.stack(cube_to_dir(f, x, y), axis=-1) for f in range(6)])
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def rotate_y(d, angle):
    """R_y(angle) d: x' = cos x + sin z, z' = -sin x + cos z"""
    c, s = np.cos(angle), np.sin(angle)
    return np.stack((c * d[..., 0] + s * d[..., 2], d[..., 1], -s * d[..., 0] + c * d[..., 2]), axis=-1)


def radiance(d):
    """A fixed positive polynomial of degree 2 in the direction: (..., 3) -> (..., 3) RGB."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack((1.5 + 0.5 * x + 0.3 * y * z + 0.4 * x * x,
                     1.2 - 0.4 * y + 0.3 * x * z + 0.5 * z * z,
                     1.0 + 0.3 * z - 0.2 * x * y + 0.6 * y * y), axis=-1)


def relative_distance(a, b):
    """max |a - b| / max |b|: the distance the conversion's tolerance is stated in"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def conversion_cases():
    """[(source (Hs, Ws, 3) float32, R, S, angle, scale)]: random positive sources times one 1e4 spike"""
    cases = []
    for k, (ws, hs) in enumerate(((16, 8), (37, 19), (64, 32))):
        rng = np.random.default_rng(100 + k)
        src = rng.uniform(0.05, 2.0, (hs, ws, 3)).astype(np.float32)
        src[int(rng.integers(hs)), int(rng.integers(ws))] *= np.float32(1e4)
        for R in (16, 32):
            for S in (1, 2, 4):
                for angle in (0.0, 1.0):
                    for scale in (1.0, 0.25):
                        cases.append((src, R, S, angle, scale))
    return cases
