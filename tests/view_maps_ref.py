"""numpy restatement of include/gs2m_maps.h: what csrc/view_maps.hip has to compute, written independently of
gs2m_render.py.  tests/test_view_maps.py holds it to the reference's own outputs (tests/golden/ref_view_maps.npz) and to
np.percentile; tests/test_view_maps_gpu.py holds the kernels to it."""
import os

import numpy as np

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_view_maps.npz")
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def magma_table():
    """matplotlib's (magma(arange(256))[:, :3] * 255).astype(uint8), as recorded in the golden file"""
    return golden()["magma_table"]


# ---- order statistics --------------------------------------------------------------------------------------------------------

def sort_keys(x):
    """the order-preserving unsigned key of every float32: sign flipped for x >= +0, all bits flipped below; NaN = 0xFFFFFFFF"""
    bits = np.ascontiguousarray(x, dtype=F32).reshape(-1).view(np.uint32)
    key = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)
    key[(bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0xFFFFFFFF)
    return key


def unkey(key):
    key = np.asarray(key, dtype=np.uint32)
    return np.where(key & np.uint32(0x80000000), key ^ np.uint32(0x80000000), ~key).astype(np.uint32).view(F32)


def order_stats(x, ranks):
    """-> (the values a sort of x puts at `ranks` as float32, the number of NaN / Inf).  The sort is of the integer keys, so
    it has one answer: -0.0 directly below +0.0 (numpy's float sort calls them equal and leaves their order to its algorithm)."""
    x = np.asarray(x, dtype=F32).reshape(-1)
    return unkey(np.sort(sort_keys(x))[np.asarray(ranks, dtype=np.int64)]), int(np.count_nonzero(~np.isfinite(x)))


def percentile_plan(n, q):
    """(rank of previous, rank of next, fp32 weight) of numpy's 'linear' percentile q of n float32 values: the quantile, the
    virtual index (n - 1) quantile and the weight are float32 there"""
    quantile = F32(q) / F32(100)
    virtual = F32(n - 1) * quantile
    if virtual >= n - 1:
        prev = nxt = n - 1
        gamma = F32(np.float64(virtual) + 1.0)  # numpy: previous = next = -1, gamma = virtual - (-1)
    else:
        prev = int(np.floor(virtual))
        nxt = prev + 1
        gamma = F32(np.float64(virtual) - prev)
    return prev, nxt, gamma


def lerp(a, b, t):
    """numpy's _lerp on float32 scalars"""
    a, b, t = F32(a), F32(b), F32(t)
    d = b - a
    return b - d * (F32(1) - t) if t >= 0.5 else a + d * t


def percentile(x, q):
    n = np.asarray(x).size
    p, nx, t = percentile_plan(n, q)
    (a, b), _ = order_stats(x, (p, nx))
    return lerp(a, b, t)


# ---- depth image -------------------------------------------------------------------------------------------------------------

def depth_image(depth, lower=1, upper=99):
    """save_depth_map's stored array: (H, W, 4) uint8, every step float32"""
    d = np.asarray(depth, dtype=F32)
    with np.errstate(over="ignore"):
        lo, hi = percentile(d, lower), percentile(d, upper)
        x = (np.minimum(np.maximum(d, lo), hi) - lo) / F32(hi - lo + F32(1e-8))
    assert x.dtype == F32
    idx = np.minimum((x * F32(256)).astype(np.int64), 255)
    out = np.full(d.shape + (4,), 255, np.uint8)
    out[..., :3] = magma_table()[idx]
    return out


# ---- image packing -----------------------------------------------------------------------------------------------------------

def quant_round(v):
    """torchvision save_image: clamp(0, 1) * 255 + 0.5, clamp(0, 255), truncate -- float32"""
    v = np.asarray(v, dtype=F32)
    return np.minimum(np.maximum(np.minimum(np.maximum(v, F32(0)), F32(1)) * F32(255) + F32(0.5), F32(0)), F32(255)).astype(np.uint8)


def quant_trunc(v):
    """map_to_rgba: (v * 255).byte() for v in [0, 1]; saturating outside"""
    v = np.asarray(v, dtype=F32)
    return np.minimum(np.maximum(v * F32(255), F32(0)), F32(255)).astype(np.uint8)


def normal_values(n_hw3, rot=None):
    """convert_normal_for_save before quantisation: (H, W, 3) float32 in, float32 out"""
    n = np.asarray(n_hw3, dtype=F32)
    length = np.maximum(np.sqrt((n * n).sum(-1, dtype=F32, keepdims=True)), F32(1e-12))
    v = n / length
    if rot is not None:
        v = (v @ np.asarray(rot, dtype=F32)) * np.array([1, -1, -1], F32)
    return (v * F32(0.5) + F32(0.5)).astype(F32)


def srgb_values(v):
    """pbr linear_to_srgb, float32"""
    v = np.asarray(v, dtype=F32)
    eps = np.finfo(F32).eps
    return np.where(v <= F32(0.0031308), F32(323 / 25) * v, (F32(211) * np.maximum(v, eps) ** F32(5 / 12) - F32(11)) / F32(200)).astype(F32)


def pack_values(src, layout="chw", mask=None, background=None, srgb=False, normal=False, rot=None):
    """the float32 (H, W, 3) values gs2m_pack_image quantises: steps 1 to 3 of the header"""
    s = np.asarray(src, dtype=F32)
    v = s.transpose(1, 2, 0) if layout == "chw" else s
    if v.shape[2] == 1:
        v = np.repeat(v, 3, axis=2)
    if normal:
        v = normal_values(v, rot)
    if srgb:
        v = srgb_values(v)
    if mask is not None:
        m = np.asarray(mask, dtype=F32).reshape(v.shape[:2])[..., None] > F32(0.5)
        v = np.where(m, np.minimum(np.maximum(v, F32(0)), F32(1)), np.asarray(background, dtype=F32)[None, None, :])
    return np.ascontiguousarray(v, dtype=F32)


def pack_image(src, layout="chw", quant="round", alpha=None, channels=None, **kw):
    """(H, W, 3 | 4) uint8"""
    v = pack_values(src, layout, **kw)
    rgb = quant_trunc(v) if quant == "trunc" else quant_round(v)
    channels = (4 if alpha is not None else 3) if channels is None else channels
    if channels == 3:
        return rgb
    a = quant_trunc(np.asarray(alpha, dtype=F32).reshape(v.shape[:2])) if alpha is not None else np.full(v.shape[:2], 255, np.uint8)
    return np.concatenate([rgb, a[..., None]], axis=2)


def boundary_distance(v, quant):
    """distance of the pre-quantisation value, on the 0 .. 255 scale, from the nearest point where the byte changes"""
    s = np.asarray(v, dtype=np.float64) * 255.0 + (0.5 if quant == "round" else 0.0)
    return np.abs(s - np.rint(s))


def assert_bytes_close(got, ref, values, quant, what):
    """The rule for the modes whose fp32 rounding is not pinned (pow, sqrt, the 3x3 product): every byte within 1 of the
    reference's, and every byte that differs must come from a value within 1e-4 (255 times a few fp32 ulps) of a quantisation
    boundary.  `values`: the reference's pre-quantisation (H, W, 3) values.  No counted budget.  -> the number that differ."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.uint8, (what, got.shape, ref.shape)
    diff = got[..., :3].astype(np.int64) - ref[..., :3].astype(np.int64)
    assert np.abs(diff).max(initial=0) <= 1, f"{what}: a byte differs by {np.abs(diff).max()}"
    dist = boundary_distance(values, quant)[diff != 0]
    assert (dist <= 1e-4).all(), f"{what}: {int((dist > 1e-4).sum())} differing bytes away from a boundary, farthest {dist.max():.3e}"
    if got.shape[-1] == 4:
        assert np.array_equal(got[..., 3], ref[..., 3]), f"{what}: alpha differs"
    return int(np.count_nonzero(diff))
