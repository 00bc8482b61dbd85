"""The kernels of csrc/loss_ops.hip alone, through the C entry points of include/gs2m_loss.h, against the numpy restatements
of tests/loss_ref.py (checked without a GPU by tests/test_loss_ref.py):

  (a) exact sums    dyadic inputs: every term a small multiple of 2^-8 .. 2^-11, every float32 partial an integer below 2^24
                    units (asserted on the inputs, per workgroup), so the reduction must return the integer sum pushed through
                    the kernel's last line, compared with ==; sizes on each side of the reducing grid 262144, of its unrolled
                    trip 1048576 and of the 256 workgroup chunks; one planted term at the chunk and trip edges;
  (b) float64       the continuous inputs of test_losses_gpu._frames; bound (n_thread + 6 + 15 + c) 2^-24 sum|term| from the
                    operation counts (loss_ref.C_*), never from the kernels;
  (c) per element   bitwise against the *_exact float32 expressions, or within c 2^-24 sum|terms of the element| where an
                    expf is involved; every element, no exception budget;
  (d) decisions     sgn(0), the clamp's edges, -0, NaN, sobel == normal, edge == min / max, min == max, ncc at 0.9f, noise at
                    1, angle at the threshold, radii == max_radii, tied scales;
  (e) edge gradient bitwise, min / max planted at the chunk edges;  (f) the random subset as one definite list;
  (g) the workspace hand-off between every pair of reducing kernels.

Every output lives in a canary-filled buffer with guard bytes before, between and after the arrays; the guards and the arrays
a call must not write are checked after every call, the ticket word and the words behind the partials after every reduction.

Largest err / bound measured on the MI355X (printed by the cases of (b) and (c); the bound is 1):

    kernel / output        largest   case
    image_loss (l1, dn, out0)  0.0816   5x4, no edge, no weight map: l1
    tv_fwd                 0.0396   7x9, C 3, absolute, weight map
    tv_bwd                 0.2633   1080x1920, C 2, squared, weight map
    plane_fwd              0.0508   n 257, activated scales
    plane_bwd (raw)        0.5603   n 2073600
    ncc_tail               0.0110   n 257
    mv_geo_fwd             0.0466   n 1025
    w_ncc                  0.6874   n 2073600
    mv_geo_bwd             0.4182   n 2073600, d_noise
    affine_mean            0.0547   n 1025
    image decisions        0.2787   d_image with the NaN pixel
  every bitwise comparison ((a), (c), (e), (f), (g)) held on every element; nothing in csrc/loss_ops.hip had to change.
"""
import functools
import math

import numpy as np
import pytest
import torch

import loss_ref as R
from test_losses_gpu import _frames

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
U = R.U
RB, LG, RU, WS_K = 1024, 256, 4, 4        # the reducing launches' workgroup, grid, unroll; partials the workspace holds
GRID = LG * RB
CANARY, GUARD = 0xA5, 256
OK, INVALID = 0, -1
TREE = 6 + 15                               # shuffle steps of a wave's sum + the adds of the 16 wave partials

FRAMES = [(511, 513), (512, 512), (481, 545), (6, 87381), (512, 1024), (3, 174763), (1023, 1025), (1024, 1024), (17, 61681),
          (3, 3), (3, 86), (5, 4), (16, 16), (1080, 1920)]
COUNTS = [h * w for h, w in FRAMES[:9]] + [524287, 1, 3, 1023, 1024, 1025, 258, 1080 * 1920]


def _lib():
    import gs2m_native
    return gs2m_native.lib()


def _stream():
    import gs2m_native
    return gs2m_native.stream_ptr()


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def P(t):
    return None if t is None else t.data_ptr()


_DT = {"f32": (torch.float32, 4), "u8": (torch.uint8, 1), "i64": (torch.int64, 8), "i32": (torch.int32, 4)}


class Outs:
    """named arrays of any type in one canary-filled byte buffer: GUARD bytes before, between and after them"""

    def __init__(self, **spec):
        self.off, pos = {}, GUARD
        for name, (n, dt) in spec.items():
            nb = n * _DT[dt][1]
            self.off[name] = (pos, nb, _DT[dt][0])
            pos += (nb + 15) // 16 * 16 + GUARD
        self.buf = torch.full((pos,), CANARY, dtype=torch.uint8, device="cuda")

    def ptr(self, name):
        return self.buf.data_ptr() + self.off[name][0]

    def get(self, name):
        o, nb, dt = self.off[name]
        return self.buf[o:o + nb].view(dt)

    def np(self, name):
        return self.get(name).cpu().numpy()

    def fill(self, name, values):
        self.get(name).copy_(dev(values).reshape(-1))

    def intact(self, written):
        """every guard byte, and every array not in `written`, still holds the canary"""
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        for name in written:
            o, nb, _ = self.off[name]
            keep[o:o + nb] = False
        return bool((self.buf[keep] == CANARY).all())


@functools.lru_cache(maxsize=None)
def _ws():
    """the reducing kernels' workspace: zeroed once, handed from call to call"""
    return torch.zeros(_lib().gs2m_loss_workspace_bytes() // 4, dtype=torch.int32, device="cuda")


def _ws_clean():
    """the ticket word reads 0 and so does every word behind the WS_K * LG partials"""
    return bool((_ws()[WS_K * LG:] == 0).all())


def call(name, *args, rc=OK):
    got = getattr(_lib(), name)(*args, _stream())
    torch.cuda.synchronize()
    assert got == rc, (name, got)
    if name.endswith("_forward") or name in ("gs2m_edge_gradient", "gs2m_affine_mean"):
        if name != "gs2m_mv_take_forward":
            assert _ws_clean(), f"{name} left the ticket or the words behind the partials non-zero"


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def assert_bits(got, want, what):
    got, want = np.ravel(np.asarray(got)), np.ravel(np.asarray(want, dtype=F32))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    assert not bad.any(), (what, "elements that differ bitwise", int(bad.sum()), "first", np.argwhere(bad)[0], got[bad][:3], want[bad][:3])


_worst = {}


def ratio(err, bound, what):
    """largest err / bound over the elements (0 / 0 = 0); printed, the largest per kernel kept for the record"""
    err, bound = np.atleast_1d(np.asarray(err, dtype=F64)), np.atleast_1d(np.asarray(bound, dtype=F64))
    assert np.isfinite(err).all() and np.isfinite(bound).all(), what
    r = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))
    key = what.split(":")[0]
    _worst[key] = max(_worst.get(key, 0.0), r)
    print(f"{what}: err / bound {r:.4f}   (largest so far for {key}: {_worst[key]:.4f})")
    return r


# ---------------------------------------------------------------- the entry points
def edge_gradient(gt, W, H, rc=OK):
    o = Outs(edge=(H * W, "f32"), minmax=(2, "f32"))
    call("gs2m_edge_gradient", W, H, P(gt), o.ptr("edge"), o.ptr("minmax"), P(_ws()), rc=rc)
    assert o.intact(("edge", "minmax") if rc == OK else ())
    return o.np("edge").reshape(H, W), o.np("minmax")


def image_fwd(W, H, image, gt, hwc=0, mask=None, bg=None, normal=None, sobel=None, edge=None, mm=None, wm=None, w_l1=0.8, w_dn=0.015):
    o = Outs(rgb=(3 * H * W, "f32"), out=(3, "f32"))
    call("gs2m_image_loss_forward", W, H, P(image), hwc, P(mask), P(bg), P(gt), P(normal), P(sobel), P(edge), P(mm), P(wm), w_l1, w_dn,
         o.ptr("rgb"), o.ptr("out"), P(_ws()))
    assert o.intact(("rgb", "out"))
    return o.np("rgb").reshape(3, H, W), o.np("out")


def image_bwd(W, H, image, gt, hwc=0, mask=None, normal=None, sobel=None, edge=None, mm=None, wm=None, w_l1=0.8, w_dn=0.015, g_loss=None, g_rgb=None):
    """d_normal / d_sobel pointers are always given: without a normal map they must stay untouched"""
    n = 3 * H * W
    o = Outs(d_image=(n, "f32"), d_normal=(n, "f32"), d_sobel=(n, "f32"))
    call("gs2m_image_loss_backward", W, H, P(image), hwc, P(mask), P(gt), P(normal), P(sobel), P(edge), P(mm), P(wm), w_l1, w_dn, P(g_loss), P(g_rgb),
         o.ptr("d_image"), o.ptr("d_normal"), o.ptr("d_sobel"))
    assert o.intact(("d_image", "d_normal", "d_sobel") if normal is not None else ("d_image",)), "wrote outside its arrays (or into d_normal / d_sobel without a normal map)"
    di = o.np("d_image").reshape((H, W, 3) if hwc else (3, H, W))
    return (di, o.np("d_normal").reshape(3, H, W), o.np("d_sobel").reshape(3, H, W)) if normal is not None else (di, None, None)


def tv_fwd(W, H, C, gt, pred, wm, norm1, weight):
    o = Outs(out=(1, "f32"))
    call("gs2m_tv_loss_forward", W, H, C, P(gt), P(pred), P(wm), norm1, weight, o.ptr("out"), P(_ws()))
    assert o.intact(("out",))
    return o.np("out")[0]


def tv_bwd(W, H, C, gt, pred, wm, norm1, weight, g):
    o = Outs(d=(C * H * W, "f32"))
    call("gs2m_tv_loss_backward", W, H, C, P(gt), P(pred), P(wm), norm1, weight, P(g), o.ptr("d"))
    assert o.intact(("d",))
    return o.np("d").reshape(C, H, W)


def geo_fwd(n, noise, angle, valid, thr, decay, factor, weight):
    o = Outs(out=(3, "f32"), pixel_valid=(n, "u8"), w_ncc=(n, "f32"))
    call("gs2m_mv_geo_loss_forward", n, P(noise), P(angle), P(valid), thr, decay, factor, weight, o.ptr("out"), o.ptr("pixel_valid"), o.ptr("w_ncc"), P(_ws()))
    assert o.intact(("out", "pixel_valid", "w_ncc"))
    return o.np("out"), o.np("pixel_valid"), o.np("w_ncc")


def geo_bwd(n, noise, angle, valid, thr, decay, factor, weight, out, g):
    o = Outs(d_noise=(n, "f32"), d_angle=(n, "f32"))
    call("gs2m_mv_geo_loss_backward", n, P(noise), P(angle), P(valid), thr, decay, factor, weight, P(out), P(g), o.ptr("d_noise"), o.ptr("d_angle"))
    assert o.intact(("d_noise", "d_angle"))
    return o.np("d_noise"), o.np("d_angle")


def ncc_fwd(n, ncc, w):
    o = Outs(out=(2, "f32"))
    call("gs2m_ncc_tail_forward", n, P(ncc), P(w), o.ptr("out"), P(_ws()))
    assert o.intact(("out",))
    return o.np("out")


def ncc_bwd(n, ncc, w, out, g):
    o = Outs(d=(n, "f32"))
    call("gs2m_ncc_tail_backward", n, P(ncc), P(w), P(out), P(g), o.ptr("d"))
    assert o.intact(("d",))
    return o.np("d")


def affine_mean(n, x, a, b):
    o = Outs(out=(1, "f32"))
    call("gs2m_affine_mean", n, P(x), a, b, o.ptr("out"), P(_ws()))
    assert o.intact(("out",))
    return o.np("out")[0]


def plane_fwd(Pn, scaling, raw, vis, weight):
    o = Outs(out=(2, "f32"))
    call("gs2m_plane_loss_forward", Pn, P(scaling), raw, P(vis), weight, o.ptr("out"), P(_ws()))
    assert o.intact(("out",))
    return o.np("out")


def plane_bwd(Pn, scaling, raw, vis, weight, out, g):
    o = Outs(d=(3 * Pn, "f32"))
    call("gs2m_plane_loss_backward", Pn, P(scaling), raw, P(vis), weight, P(out), P(g), o.ptr("d"))
    assert o.intact(("d",))
    return o.np("d").reshape(Pn, 3)


def subset_thin(n, mask, k, seed, cap):
    o = Outs(idx=(cap, "i64"), counts=(2, "i32"), blocks=((n + 1023) // 1024, "i32"))
    call("gs2m_subset_thin", n, P(mask), k, seed, o.ptr("idx"), cap, o.ptr("counts"), o.ptr("blocks"))
    assert o.intact(("idx", "counts", "blocks"))
    return o.np("idx"), o.np("counts")


def subset_remove(m, k, seed, idx):
    o = Outs(out=(k, "i64"))
    call("gs2m_subset_remove", m, k, seed, P(idx), o.ptr("out"))
    assert o.intact(("out",))
    return o.np("out")


# ---------------------------------------------------------------- how the sums are dealt to the workgroups
def wg_sums_strided(units):
    """per-workgroup sums of a grid-stride reduction: element i belongs to workgroup (i // RB) % LG"""
    u = np.abs(np.asarray(units, dtype=np.int64).reshape(-1))
    pad = (-u.size) % GRID
    return np.pad(u, (0, pad)).reshape(-1, LG, RB).sum(axis=(0, 2))


def wg_sums_chunked(units):
    """per-workgroup sums where workgroup b owns the contiguous pixels [b * ceil(n / 256), (b + 1) * ceil(n / 256))"""
    u = np.abs(np.asarray(units, dtype=np.int64).reshape(-1))
    chunk = -(-u.size // LG)
    return np.pad(u, (0, chunk * LG - u.size)).reshape(LG, chunk).sum(axis=1)


def assert_exactly_summable(units, chunked, what):
    s = (wg_sums_chunked if chunked else wg_sums_strided)(units)
    assert int(s.max()) < 2 ** 24, (what, "a workgroup's partial would leave the integers float32 holds exactly", int(s.max()))


def plant_indices(n):
    """0, n - 1, the first and last index of a few workgroup chunks, of the workgroup blocks and of the grid's trips"""
    chunk = -(-n // LG)
    cand = {0, n - 1, RB - 1, RB, GRID - 1, GRID, RU * GRID - 1}
    for b in (1, 2, 128, 255):
        cand |= {b * chunk - 1, b * chunk}
    cand |= {(n // chunk) * chunk - 1, (n // chunk) * chunk}     # the last, short chunk
    return sorted(p for p in cand if 0 <= p < n)


# ================================================================ (a) exact sums
def _dyadic_frame(H, W, seed):
    rng = np.random.default_rng(seed)
    z = {}
    z["image_i"] = rng.integers(-64, 321, (3, H, W))        # 1/256 grid on [-0.25, 1.25]
    z["gt_i"] = rng.integers(0, 257, (3, H, W))
    z["normal_i"], z["sobel_i"] = rng.integers(-32, 33, (3, H, W)), rng.integers(-32, 33, (3, H, W))
    z["wm_i"] = rng.integers(0, 3, (H, W))                  # {0, 1/2, 1}
    z["edge_sel"] = rng.integers(0, 3, (H, W))              # edge in {mn, (mn + mx) / 2, mx}: the weight is 1, 1/4, 0
    return z


def _image_exact_case(H, W, z, with_edge, with_wm):
    """-> device inputs, the two integer term arrays (units 2^-8 and 2^-11)"""
    HW = H * W
    f = lambda a: dev((a / 256.0).astype(F32))
    edge = np.array([0.25, 0.5, 0.75], dtype=F32)[z["edge_sel"]]
    l1_units = np.abs(np.clip(z["image_i"], 0, 256) - z["gt_i"])
    w4 = np.array([4, 1, 0])[z["edge_sel"]]
    w4[0, :] = w4[-1, :] = 4
    w4[:, 0] = w4[:, -1] = 4
    w4 = w4 if with_edge else np.full((H, W), 4)
    wm2 = z["wm_i"] if with_wm else np.full((H, W), 2)
    dn_units = np.abs(z["sobel_i"] - z["normal_i"]).sum(0) * w4 * wm2
    args = dict(image=f(z["image_i"]), gt=f(z["gt_i"]), normal=f(z["normal_i"]), sobel=f(z["sobel_i"]),
                edge=dev(edge) if with_edge else None, mm=dev(np.array([0.25, 0.75], dtype=F32)) if with_edge else None,
                wm=dev((z["wm_i"] / 2.0).astype(F32)) if with_wm else None)
    return args, l1_units, dn_units


def _image_expected(S0, S1, HW, w_l1=0.8, w_dn=0.015):
    l1, dn = F32((S0 / 256.0) / (3.0 * HW)), F32((S1 / 2048.0) / float(HW))
    return np.array([F32(w_l1) * l1 + F32(w_dn) * dn, l1, dn], dtype=F32)


@pytest.mark.parametrize("H,W", FRAMES + [(1, 1)], ids=lambda v: str(v))
def test_image_loss_sums_are_exact(H, W):
    HW = H * W
    z = _dyadic_frame(H, W, seed=HW)
    for with_edge, with_wm in ((True, True), (False, False)) if H >= 3 and W >= 3 else ((False, True),):
        a, l1_u, dn_u = _image_exact_case(H, W, z, with_edge, with_wm)
        assert_exactly_summable(l1_u.sum(0), False, "l1")
        assert_exactly_summable(dn_u, False, "dn")
        rgb, out = image_fwd(W, H, **a)
        assert_bits(out, _image_expected(int(l1_u.sum()), int(dn_u.sum()), HW), ("image loss", H, W, with_edge, with_wm))
        assert_bits(rgb, (np.clip(z["image_i"], 0, 256) / 256.0).astype(F32), "rgb")
    # one planted term, zeros elsewhere: |0.5 - 0| in channel 1 and |0.25 - 0| in the Sobel map's channel 2
    image, gt, normal, sobel = (torch.zeros(3, HW, device="cuda") for _ in range(4))
    for p in plant_indices(HW):
        image[1, p], sobel[2, p] = 0.5, 0.25
        _, out = image_fwd(W, H, image, gt, normal=normal, sobel=sobel)
        image[1, p], sobel[2, p] = 0.0, 0.0
        assert_bits(out, _image_expected(128, 64 * 8, HW), ("planted at", p, "of", HW))


def _tv_units(pred_i, wm_i, norm1):
    """integer terms of the vertical and the horizontal pairs, booked at the pair's upper / left pixel: units 2^-10"""
    C, H, W = pred_i.shape
    f = (lambda d: np.abs(d)) if norm1 else (lambda d: d * d)
    wsum_h = (wm_i[1:] + wm_i[:-1]) if wm_i is not None else np.full((H - 1, W), 4)
    wsum_w = (wm_i[:, 1:] + wm_i[:, :-1]) if wm_i is not None else np.full((H, W - 1), 4)
    th, tw = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    th[:-1] = f(pred_i[:, 1:] - pred_i[:, :-1]).sum(0) * wsum_h
    tw[:, :-1] = f(pred_i[:, :, 1:] - pred_i[:, :, :-1]).sum(0) * wsum_w
    return th, tw


def _tv_expected(Sh, Sw, C, H, W, weight):
    return F32(weight) * (F32((Sh / 1024.0) / (float(C) * (H - 1) * W)) + F32((Sw / 1024.0) / (float(C) * H * (W - 1))))


@pytest.mark.parametrize("H,W", FRAMES, ids=lambda v: str(v))
def test_tv_sums_are_exact(H, W):
    """a constant ground truth: the damping is expf(-0) = 1; pred on the 1/256 grid (absolute) or the 1/16 grid (squared)"""
    HW = H * W
    rng = np.random.default_rng(HW + 1)
    gt = torch.full((3, H, W), 0.5, device="cuda")
    wm_i = rng.integers(0, 3, (H, W))
    for C, norm1, weighted in ((3, 1, True), (1, 0, False), (2, 0, True), (4, 1, True), (5, 0, False)):
        pred_i = rng.integers(0, 257 if norm1 else 17, (C, H, W))
        pred = dev((pred_i / (256.0 if norm1 else 16.0)).astype(F32))
        th, tw = _tv_units(pred_i, wm_i if weighted else None, norm1)
        for t in (th, tw):
            assert_exactly_summable(t, C <= 3, "tv")
        got = tv_fwd(W, H, C, gt, pred, dev((wm_i / 2.0).astype(F32)) if weighted else None, norm1, 0.37)
        assert_bits(got, _tv_expected(int(th.sum()), int(tw.sum()), C, H, W, 0.37), ("tv", H, W, C, norm1, weighted))
    # one planted pixel of value 1 among zeros: one term per neighbour, each 1 (1024 units)
    for C in (3, 4):
        pred = torch.zeros(C, HW, device="cuda")
        for p in plant_indices(HW):
            y, x = divmod(p, W)
            pred[C - 1, p] = 1.0
            got = tv_fwd(W, H, C, gt, pred, None, 1, 1.0)
            pred[C - 1, p] = 0.0
            assert_bits(got, _tv_expected(1024 * ((y > 0) + (y < H - 1)), 1024 * ((x > 0) + (x < W - 1)), C, H, W, 1.0), ("planted at", p, "of", HW, "C", C))


@pytest.mark.parametrize("n", COUNTS)
def test_plane_ncc_geo_and_mean_sums_are_exact(n):
    rng = np.random.default_rng(n)
    # plane loss: scales on the 1/256 grid, raw = 0
    sc_i = rng.integers(1, 257, (n, 3))
    vis = rng.random(n) < 0.8
    units = np.where(vis, sc_i.min(1), 0)
    assert_exactly_summable(units, False, "plane")
    cnt = int(vis.sum())
    out = plane_fwd(n, dev((sc_i / 256.0).astype(F32)), 0, dev(vis), 0.25)
    assert_bits(out, [F32(0.25) * F32((int(units.sum()) / 256.0) / max(cnt, 1)), F32(cnt)], ("plane", n))
    # ncc tail: ncc and w on the 1/16 grid, signed terms
    ncc_i, w_i = rng.integers(-16, 17, n), rng.integers(0, 17, n)
    m = ncc_i <= 14                                  # 15 / 16 = 0.9375 and 1 are not below 0.9f
    units = np.where(m, ncc_i * w_i, 0)
    assert_exactly_summable(units, False, "ncc")
    out = ncc_fwd(n, dev((ncc_i / 16.0).astype(F32)), dev((w_i / 16.0).astype(F32)))
    assert_bits(out, [F32((int(units.sum()) / 256.0) / max(int(m.sum()), 1)), F32(int(m.sum()))], ("ncc_tail", n))
    # geometric means: decay = 0 (the weight is expf(-0) = 1), factor 1/2
    nz_i, an_i = rng.integers(0, 384, n), rng.integers(0, 256, n)
    valid = rng.random(n) < 0.7
    pv, av = valid & (nz_i < 256), valid & (an_i < 128)
    u0, u1 = np.where(pv, nz_i, 0), np.where(av & pv, an_i, 0)       # geo_w is 0 outside pixel_valid; units 2^-8 and 2^-9
    assert_exactly_summable(u0, False, "geo noise")
    assert_exactly_summable(u1, False, "geo angle")
    noise = (nz_i / 256.0).astype(F32)
    out, pvk, w_ncc = geo_fwd(n, dev(noise), dev((an_i / 256.0).astype(F32)), dev(valid), 0.5, 0.0, 0.5, 0.05)
    n0, n1 = int(pv.sum()), int(av.sum())
    want = F32(0.05) * (F32((int(u0.sum()) / 256.0) / max(n0, 1)) + F32((int(u1.sum()) / 512.0) / max(n1, 1)))
    assert_bits(out, [want, F32(n0), F32(n1)], ("mv_geo", n))
    assert np.array_equal(pvk, pv.astype(np.uint8))
    ref = np.where(pv, np.exp(-noise.astype(F64)), 0.0)
    assert bool((np.abs(w_ncc - ref) <= R.gamma(R.C_W_NCC) * ref).all()) and not w_ncc[~pv].any()
    # affine mean: every n mod 4, the float4 body and the scalar tail
    for nn in sorted({n, max(n - 1, 1), max(n - 2, 1), max(n - 3, 1)}):
        x_i = rng.integers(0, 257, nn)
        assert_exactly_summable(x_i, False, "mean")
        got = affine_mean(nn, dev((x_i / 256.0).astype(F32)), 0.2, -0.2)
        assert_bits(got, F32(0.2) + F32(-0.2) * F32((int(x_i.sum()) / 256.0) / float(nn)), ("affine_mean", nn))
    # one planted term among zeros
    sc, vz = torch.ones(n, 3, device="cuda"), torch.zeros(n, dtype=torch.bool, device="cuda")
    x, ncc, w = torch.zeros(n, device="cuda"), torch.ones(n, device="cuda"), torch.ones(n, device="cuda")
    nz, an, va = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.ones(n, dtype=torch.bool, device="cuda")
    for p in plant_indices(n):
        sc[p, 1], vz[p], x[p], ncc[p], nz[p], an[p] = 0.375, True, 0.625, 0.5, 0.75, 0.25
        assert_bits(plane_fwd(n, sc, 0, vz, 1.0), [0.375, 1.0], ("plane planted", p, n))
        assert_bits(affine_mean(n, x, 0.0, 1.0), F32(0.625 / float(n)), ("mean planted", p, n))
        assert_bits(ncc_fwd(n, ncc, w), [0.5, 1.0], ("ncc planted", p, n))
        want = F32(1.0) * (F32(0.75 / float(n)) + F32(0.25 / float(n)))
        assert_bits(geo_fwd(n, nz, an, va, 0.5, 0.0, 1.0, 1.0)[0], [want, F32(n), F32(n)], ("geo planted", p, n))
        sc[p, 1], vz[p], x[p], ncc[p], nz[p], an[p] = 1.0, False, 0.0, 1.0, 0.0, 0.0


def test_small_means_below_one_float4():
    for n in (1, 2, 3, 4, 5, 6, 7):
        x = np.arange(1, n + 1, dtype=F32) / F32(8)
        assert_bits(affine_mean(n, dev(x), 1.0, -1.0), F32(1.0) + F32(-1.0) * F32(float(x.astype(F64).sum()) / n), n)


# ================================================================ (b) continuous inputs against float64
def _np_frames(H, W, seed):
    return [t.cpu().numpy() for t in _frames(H, W, seed, dev="cpu")]


@pytest.mark.parametrize("H,W", [(1080, 1920), (481, 545), (77, 333), (5, 4)])
def test_image_loss_within_the_derived_bound(H, W):
    image, gt, normal, sobel, _, wm = _np_frames(H, W, seed=H + W)
    HW = H * W
    edge = R.edge_exact(gt)
    mm = np.array([edge[1:-1, 1:-1].min(), edge[1:-1, 1:-1].max()], dtype=F32)
    npix = -(-HW // GRID)
    for with_edge, with_wm in ((True, False), (True, True), (False, True), (False, False)):
        ref = R.image_loss_f64(image, 0, None, None, gt, normal, sobel, edge if with_edge else None, mm, wm if with_wm else None, 0.8, 0.015)
        rgb, out = image_fwd(W, H, dev(image), dev(gt), normal=dev(normal), sobel=dev(sobel), edge=dev(edge) if with_edge else None,
                             mm=dev(mm) if with_edge else None, wm=dev(wm) if with_wm else None)
        assert_bits(rgb, ref["rgb"], "rgb")
        b1 = (3 * npix + TREE + R.C_L1 + R.C_OUT) * U * ref["l1"]          # a thread adds three terms per pixel
        # the weight's own error is absolute, |dw| <= C_DN_W u sqrt(w): not relative to a term that w makes small
        D = np.abs(sobel.astype(F64) - normal).sum(0)
        sq = np.sqrt(R.dn_weight(H, W, edge, mm, None)) * (wm[0] if with_wm else 1.0) if with_edge else 0.0
        b2 = (npix + TREE + R.C_DN + R.C_OUT) * U * ref["dn"] + R.C_DN_W * U * float(np.mean(sq * D))
        b0 = float(F32(0.8)) * b1 + float(F32(0.015)) * b2 + R.C_OUT0 * U * ref["out0"]
        tag = f"image_loss: {H}x{W} edge {int(with_edge)} wm {int(with_wm)}"
        assert ratio(abs(out[1] - ref["l1"]), b1, tag + " l1") <= 1
        assert ratio(abs(out[2] - ref["dn"]), b2, tag + " dn") <= 1
        assert ratio(abs(out[0] - ref["out0"]), b0, tag + " out0") <= 1


@pytest.mark.parametrize("H,W", [(1080, 1920), (481, 545), (7, 9), (2, 2)])
def test_tv_within_the_derived_bound(H, W):
    _, gt, _, _, _, wm = _np_frames(H, W, seed=H * 7 + W)
    HW = H * W
    g = dev(np.array([0.7], dtype=F32))
    for C, norm1, weighted in ((1, 0, False), (3, 1, False), (3, 1, True), (2, 0, True), (4, 1, True), (5, 0, False)):
        pred = np.random.default_rng(HW + C).random((C, H, W), dtype=F32)
        w = wm if weighted else None
        val, mh, mw = R.tv_f64(gt, pred, w, bool(norm1), 0.37)
        n_thread = C * (-(-(-(-HW // LG)) // RB) if C <= 3 else -(-HW // GRID))
        c = R.C_TV + (R.C_TV_WM if weighted else 0)
        bound = float(F32(0.37)) * (n_thread + TREE + c + 1) * U * (mh + mw) + 2 * U * val     # the two casts; the add and the product
        got = tv_fwd(W, H, C, dev(gt), dev(pred), dev(w), norm1, 0.37)
        tag = f"tv_fwd: {H}x{W} C {C} norm1 {norm1} wm {int(weighted)}"
        assert ratio(abs(got - val), bound, tag) <= 1
        d, mag = R.tv_bwd_f64(gt, pred, w, bool(norm1), 0.37, 0.7)
        gotd = tv_bwd(W, H, C, dev(gt), dev(pred), dev(w), norm1, 0.37, g)
        assert ratio(np.abs(gotd - d), R.gamma(R.C_TV_BWD + (R.C_TV_WM if weighted else 0)) * mag, tag.replace("tv_fwd", "tv_bwd")) <= 1


@pytest.mark.parametrize("n", [1080 * 1920, 1_000_000, 1025, 257])
def test_plane_ncc_geo_and_mean_within_the_derived_bound(n):
    rng = np.random.default_rng(n)
    per = -(-n // GRID)
    raw = (rng.standard_normal((n, 3)) - 4.0).astype(F32)
    vis = rng.random(n) < 0.85
    g = dev(np.array([3.0], dtype=F32))
    for is_raw, sc in ((1, raw), (0, np.exp(raw.astype(F64)).astype(F32))):
        val, cnt = R.plane_f64(sc, is_raw, vis, 0.01)
        out = plane_fwd(n, dev(sc), is_raw, dev(vis), 0.01)
        assert out[1] == cnt
        assert ratio(abs(out[0] - val), (per + TREE + (R.C_PLANE_RAW if is_raw else R.C_PLANE) + 2) * U * val, f"plane_fwd: n {n} raw {is_raw}") <= 1
        outd = dev(np.array([out[0], cnt], dtype=F32))
        d = plane_bwd(n, dev(sc), is_raw, dev(vis), 0.01, outd, g)
        if is_raw:
            ref = R.plane_bwd_f64(sc, 1, vis, 0.01, cnt, 3.0)
            assert np.array_equal(d != 0, ref != 0)
            assert ratio(np.abs(d - ref), R.gamma(R.C_PLANE_BWD_RAW) * np.abs(ref), f"plane_bwd: n {n} raw") <= 1
        else:
            assert_bits(d, R.plane_bwd_exact(sc, vis, 0.01, cnt, 3.0), "plane backward")
    ncc, w = (rng.random(n) * 2 - 1).astype(F32), rng.random(n).astype(F32)
    val, cnt = R.ncc_tail_f64(ncc, w)
    out = ncc_fwd(n, dev(ncc), dev(w))
    assert out[1] == cnt
    mean_abs = float(np.abs(ncc.astype(F64) * w)[ncc < R.NCC_LIMIT].sum()) / max(cnt, 1)
    assert ratio(abs(out[0] - val), (per + TREE + R.C_NCC + 1) * U * mean_abs, f"ncc_tail: n {n}") <= 1
    assert_bits(ncc_bwd(n, dev(ncc), dev(w), dev(np.array([out[0], cnt], dtype=F32)), dev(np.array([0.3], dtype=F32))), R.d_ncc_exact(ncc, w, cnt, F32(0.3)), "d_ncc")
    noise, angle, valid = (rng.random(n) * 1.5).astype(F32), (rng.random(n) * 0.6).astype(F32), rng.random(n) < 0.7
    thr, decay, factor, weight = F32(0.3), F32(0.5), F32(2.0), F32(0.05)
    r = R.mv_geo_f64(noise, angle, valid, thr, decay, factor, weight)
    out, pv, w_ncc = geo_fwd(n, dev(noise), dev(angle), dev(valid), thr, decay, factor, weight)
    assert out[1] == r["n0"] and out[2] == r["n1"] and np.array_equal(pv, r["pixel_valid"].astype(np.uint8))
    bound = float(weight) * ((per + TREE + R.C_GEO_NOISE + float(decay) + 1) * U * r["pixel_loss"] + (per + TREE + R.C_GEO_ANGLE + float(decay) + 1) * U * r["angle_loss"]) + 2 * U * r["out0"]
    assert ratio(abs(out[0] - r["out0"]), bound, f"mv_geo_fwd: n {n}") <= 1
    assert ratio(np.abs(w_ncc - r["w_ncc"]), R.gamma(R.C_W_NCC) * r["w_ncc"], f"w_ncc: n {n}") <= 1
    dn_, da_ = R.mv_geo_bwd_f64(noise, angle, valid, thr, decay, factor, weight, 1.3)
    gn, ga = geo_bwd(n, dev(noise), dev(angle), dev(valid), thr, decay, factor, weight, dev(np.array([out[0], r["n0"], r["n1"]], dtype=F32)), dev(np.array([1.3], dtype=F32)))
    assert ratio(np.abs(gn - dn_), R.gamma(R.C_GEO_DNOISE + float(decay)) * np.abs(dn_), f"mv_geo_bwd: n {n} d_noise") <= 1
    assert ratio(np.abs(ga - da_), R.gamma(R.C_GEO_DANGLE + float(decay)) * np.abs(da_), f"mv_geo_bwd: n {n} d_angle") <= 1
    x = rng.random(n).astype(F32)
    val = R.affine_mean_f64(x, 0.2, -0.2)
    bound = 0.2 * (-(-(n // 4) // GRID) + 1 + TREE + R.C_MEAN) * U * float(x.astype(F64).mean()) + R.C_MEAN_OUT * U * 0.2
    assert ratio(abs(affine_mean(n, dev(x), 0.2, -0.2) - val), bound, f"affine_mean: n {n}") <= 1


# ================================================================ (c) per-element outputs, every element
@pytest.mark.parametrize("H,W", [(77, 333), (270, 481), (5, 4), (1, 1)])
def test_image_loss_backward_is_the_written_expression_bit_for_bit(H, W):
    image, gt, normal, sobel, Rr, wm = _np_frames(H, W, seed=H - W)
    HW = H * W
    have_edge = H >= 3 and W >= 3
    edge = R.edge_exact(gt) if have_edge else None
    mm = np.array([edge[1:-1, 1:-1].min(), edge[1:-1, 1:-1].max()], dtype=F32) if have_edge and HW > 9 else np.array([0.0, 1.0], dtype=F32)
    mask = np.random.default_rng(3).random((H, W)) < 0.7
    bg = np.array([0.2, 1.0, 0.0], dtype=F32)
    g_loss, g_rgb = np.array([1.7], dtype=F32), (Rr * 1e-3).astype(F32)
    for hwc in (0, 1):
        img = np.ascontiguousarray(image.transpose(1, 2, 0)) if hwc else image
        for use_mask in (False, True):
            for gl, gr in ((g_loss, g_rgb), (None, g_rgb), (g_loss, None), (None, None)):
                for dn, with_edge, with_wm in ((True, True, False), (True, False, True), (True, True, True), (False, False, False)):
                    with_edge = with_edge and have_edge
                    kw = dict(hwc=hwc, mask=mask if use_mask else None, normal=normal if dn else None, sobel=sobel if dn else None,
                              edge=edge if with_edge else None, mm=mm if with_edge else None, wm=wm if with_wm and dn else None)
                    want = R.image_loss_bwd_exact(img, hwc, kw["mask"], gt, kw["normal"], kw["sobel"], kw["edge"], mm, kw["wm"], 0.8, 0.015,
                                                  None if gl is None else gl[0], gr)
                    got = image_bwd(W, H, dev(img), dev(gt), **{k: (v if k == "hwc" else dev(v)) for k, v in kw.items()}, g_loss=dev(gl), g_rgb=dev(gr))
                    for a, b, name in zip(got, want, ("d_image", "d_normal", "d_sobel")):
                        if b is not None:
                            assert_bits(a, b, (name, H, W, hwc, use_mask, gl is not None, gr is not None, dn, with_edge, with_wm))
            # the forward's rgb through the mask and the background, and its sums against float64
            ref = R.image_loss_f64(img, hwc, mask if use_mask else None, bg, gt, None, None, None, None, None, 1.0, 0.0)
            rgb, out = image_fwd(W, H, dev(img), dev(gt), hwc=hwc, mask=dev(mask) if use_mask else None, bg=dev(bg) if use_mask else None, w_l1=1.0, w_dn=0.0)
            assert_bits(rgb, ref["rgb"], ("rgb", hwc, use_mask))
            assert abs(out[1] - ref["l1"]) <= (3 * -(-HW // GRID) + TREE + R.C_L1 + R.C_OUT) * U * ref["l1"] and out[2] == 0


@pytest.mark.parametrize("H,W", [(9, 2047), (45, 46), (2, 2), (2, 1025), (300, 7)])
def test_tv_backward_every_element(H, W):
    """block counts 72, 9, 1, 9, 9 (rounded up to a multiple of 8 by the launch): the dealt-out blocks beyond the frame"""
    _, gt, _, _, _, wm = _np_frames(H, W, seed=H + 3 * W)
    g = dev(np.array([0.7], dtype=F32))
    for C, norm1, weighted in ((3, 1, True), (1, 0, False), (5, 0, True), (4, 1, False)):
        pred = np.random.default_rng(H * W + C).random((C, H, W), dtype=F32)
        pred[:, ::3, ::2] = pred[:, :1, :1]          # equal neighbours: sgn(0)
        w = wm if weighted else None
        d, mag = R.tv_bwd_f64(gt, pred, w, bool(norm1), 0.37, 0.7)
        got = tv_bwd(W, H, C, dev(gt), dev(pred), dev(w), norm1, 0.37, g)
        assert ratio(np.abs(got - d), R.gamma(R.C_TV_BWD + (R.C_TV_WM if weighted else 0)) * mag, f"tv_bwd: {H}x{W} C {C} norm1 {norm1} wm {int(weighted)}") <= 1


@pytest.mark.parametrize("n", [1, 255, 256, 257, 300_001])
def test_take_and_statistics_are_exact(n):
    rng = np.random.default_rng(n)
    H, W = 97, 3119
    idx = np.sort(rng.choice(H * W, n, replace=False)).astype(np.int64)
    if n > 2:
        idx[0], idx[-1] = 0, H * W - 1
    nm, dm, wmap = rng.random((3, H, W), dtype=F32), rng.random((H, W), dtype=F32), rng.random((H, W), dtype=F32)
    t_idx, t_nm, t_dm = dev(idx), dev(nm), dev(dm)
    for wsrc in (wmap, None):
        o = Outs(pixels=(2 * n, "f32"), normals=(3 * n, "f32"), dists=(n, "f32"), w=(n, "f32"))
        t_w = dev(wsrc)
        call("gs2m_mv_take_forward", n, P(t_idx), W, H, P(t_nm), P(t_dm), P(t_w), o.ptr("pixels"), o.ptr("normals"), o.ptr("dists"), o.ptr("w"))
        assert o.intact(("pixels", "normals", "dists", "w"))
        for name, want in zip(("pixels", "normals", "dists", "w"), R.mv_take_exact(idx, W, H, nm, dm, wsrc)):
            assert_bits(o.np(name), want.reshape(-1), name)
    d_n, d_d = rng.standard_normal((n, 3)).astype(F32), rng.standard_normal(n).astype(F32)
    o = Outs(dn=(3 * H * W, "f32"), dd=(H * W, "f32"))
    o.get("dn").zero_(); o.get("dd").zero_()
    t_dn, t_dd = dev(d_n), dev(d_d)
    call("gs2m_mv_take_backward", n, P(t_idx), W, H, P(t_dn), P(t_dd), o.ptr("dn"), o.ptr("dd"))
    assert o.intact(("dn", "dd"))
    wn, wd = R.mv_take_bwd_exact(idx, W, H, d_n, d_d)
    assert_bits(o.np("dn"), wn.reshape(-1), "d_normal_map")
    assert_bits(o.np("dd"), wd.reshape(-1), "d_dist_map")
    # the statistics, in place; invisible rows and unobserved radii keep their bits
    vg = rng.standard_normal((n, 4)).astype(F32)
    vis, observe, radii = rng.random(n) < 0.8, rng.integers(0, 3, n).astype(np.int32), rng.integers(0, 200, n).astype(np.int32)
    acc, ab, den, mr = rng.random(n, dtype=F32), rng.random(n, dtype=F32), rng.integers(0, 50, n).astype(F32), (rng.random(n) * 100).astype(F32)
    mr[::5] = radii[::5]                              # radii == max_radii
    for with_radii in (True, False):
        o = Outs(acc=(n, "f32"), ab=(n, "f32"), den=(n, "f32"), mr=(n, "f32"))
        for name, v in (("acc", acc), ("ab", ab), ("den", den)) + ((("mr", mr),) if with_radii else ()):
            o.fill(name, v)
        t_vg, t_vis, t_ob, t_ra = dev(vg), dev(vis), dev(observe), dev(radii)
        call("gs2m_densification_stats", n, P(t_vg), P(t_vis), P(t_ob) if with_radii else None, P(t_ra) if with_radii else None,
             o.ptr("acc"), o.ptr("ab"), o.ptr("den"), o.ptr("mr") if with_radii else None)
        assert o.intact(("acc", "ab", "den") + (("mr",) if with_radii else ()))
        want = R.densification_exact(vg, vis, observe, radii, acc, ab, den, mr if with_radii else None)
        for name, wv in zip(("acc", "ab", "den", "mr"), want):
            if wv is not None:
                assert_bits(o.np(name), wv, name)
        ref = R.densification_f64(vg, vis, observe, radii, acc, ab, den, mr if with_radii else None)
        assert bool((np.abs(o.np("acc") - ref[0]) <= 4 * U * np.abs(ref[0])).all()) and np.array_equal(o.np("den"), ref[2].astype(F32))


# ================================================================ (d) decisions, planted on purpose
def test_image_loss_decisions_against_float64_autograd():
    H, W = 16, 16
    image, gt, normal, sobel, Rr, wm = _np_frames(H, W, seed=99)
    nxt = lambda v, to: np.nextafter(F32(v), F32(to))
    plant = [0.0, 1.0, -0.0, nxt(0, -1), nxt(1, 2), nxt(0, 1), nxt(1, 0)]
    for j, v in enumerate(plant):
        image[j % 3, 2, 1 + j] = v
    image[:, 3, 1:6] = gt[:, 3, 1:6]                   # render == gt inside [0, 1]: sgn(0)
    gt[0, 2, 1], gt[1, 2, 2] = 0.0, 1.0                # ... and at the clamp's two ends
    sobel[0, 5, 5] = normal[0, 5, 5]                   # sobel == normal in one channel, and in all
    sobel[:, 6, 6] = normal[:, 6, 6]
    edge = R.edge_exact(gt)
    mm = np.array([edge[1:-1, 1:-1].min(), edge[1:-1, 1:-1].max()], dtype=F32)   # the argmin / argmax pixels have edge == mn / mx
    g_rgb, g_loss = (Rr * 1e-3).astype(F32), np.array([1.7], dtype=F32)
    for nan_pixel in (False, True):
        if nan_pixel:
            image[1, 8, 8] = np.nan
        x, n, s = (torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in (image, normal, sobel))
        t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
        rgb = x.clamp(0, 1)
        wt = t64(R.dn_weight(H, W, edge, mm, wm))
        assert float(wt.min()) == 0.0 and int((wt[1:-1, 1:-1] == t64(wm)[0, 1:-1, 1:-1]).sum()) >= 1, "edge == mx and edge == mn are both in the frame"
        l1, dn = (rgb - t64(gt)).abs().mean(), (wt * (s - n).abs().sum(0)).mean()
        (float(F32(1.7)) * (float(F32(0.8)) * l1 + float(F32(0.015)) * dn) + (rgb * t64(g_rgb)).sum()).backward()
        kw = dict(normal=dev(normal), sobel=dev(sobel), edge=dev(edge), mm=dev(mm), wm=dev(wm))
        rgbk, out = image_fwd(W, H, dev(image), dev(gt), **kw)
        assert_bits(rgbk, R.rgb_exact(image), "rgb")
        assert np.array_equal(np.isnan(rgbk), np.isnan(image)) and rgbk[2 % 3, 2, 3] == 0 and np.signbit(rgbk[2, 2, 3]), "-0 stays -0, NaN passes"
        di, dnk, dsk = image_bwd(W, H, dev(image), dev(gt), **kw, g_loss=dev(g_loss), g_rgb=dev(g_rgb))
        k1, k2 = 1.7 * 0.8 / (3 * H * W), 1.7 * 0.015 / (H * W)
        sel = ~np.isnan(image)     # at the NaN pixel the kernel's 0 (torch.clamp's gradient mask is false there) is asserted below
        assert ratio(np.abs(di - x.grad.numpy())[sel], (4 * U * (np.abs(g_rgb) + k1))[sel], f"decisions: d_image nan {int(nan_pixel)}") <= 1
        assert ratio(np.abs(dsk - s.grad.numpy()), R.C_DN_BWD * U * k2 * np.ones_like(dsk), f"decisions: d_sobel nan {int(nan_pixel)}") <= 1
        assert ratio(np.abs(dnk - n.grad.numpy()), R.C_DN_BWD * U * k2 * np.ones_like(dnk), f"decisions: d_normal nan {int(nan_pixel)}") <= 1
        want = R.image_loss_bwd_exact(image, 0, None, gt, normal, sobel, edge, mm, wm, 0.8, 0.015, g_loss[0], g_rgb)
        for a, b, name in zip((di, dnk, dsk), want, ("d_image", "d_normal", "d_sobel")):
            assert_bits(a, b, name)
        # what the decisions must give, spelled out
        assert di[0, 2, 4] == 0 and di[1, 2, 5] == 0, "just outside [0, 1]: no gradient, not even the D-SSIM term's"
        assert bool((di[:, 3, 1:6] == g_rgb[:, 3, 1:6]).all()), "render == gt: sgn(0) = 0, only the D-SSIM term's gradient"
        assert di[0, 2, 1] == g_rgb[0, 2, 1] and di[1, 2, 2] == g_rgb[1, 2, 2], "0 == gt and 1 == gt at the clamp's ends: inside, sgn(0)"
        assert dsk[0, 5, 5] == 0 and dsk[1, 5, 5] != 0 and not dsk[:, 6, 6].any() and not dnk[:, 6, 6].any()
        if nan_pixel:
            assert np.isnan(out[0]) and np.isnan(out[1]) and np.isfinite(out[2]) and di[1, 8, 8] == 0 and np.isfinite(di).all()
        else:
            ref = R.image_loss_f64(image, 0, None, None, gt, normal, sobel, edge, mm, wm, 0.8, 0.015)
            assert abs(out[1] - ref["l1"]) <= (3 + TREE + 2) * U * ref["l1"] and abs(out[2] - ref["dn"]) <= (1 + TREE + R.C_DN + R.C_DN_W + 1) * U * float(np.abs(sobel.astype(F64) - normal).sum(0).mean())


def test_a_constant_ground_truth_gives_nan_only_in_the_depth_normal_term():
    """mn == mx: the reference's (g - g.min()) / (g.max() - g.min()) is 0 / 0 inside; the L1 term and d_image do not see it"""
    H, W = 12, 20
    image, _, normal, sobel, Rr, _ = _np_frames(H, W, seed=4)
    gt = np.full((3, H, W), 0.375, dtype=F32)
    edge, mm = edge_gradient(dev(gt), W, H)
    assert not edge.any() and mm[0] == 0 and mm[1] == 0
    assert np.isnan(R.image_loss_f64(image, 0, None, None, gt, normal, sobel, edge, mm, None, 0.8, 0.015)["dn"])
    kw = dict(normal=dev(normal), sobel=dev(sobel), edge=dev(edge), mm=dev(mm))
    _, out = image_fwd(W, H, dev(image), dev(gt), **kw)
    ref = R.image_loss_f64(image, 0, None, None, gt, None, None, None, None, None, 0.8, 0.0)
    assert np.isnan(out[2]) and np.isnan(out[0]) and abs(out[1] - ref["l1"]) <= (3 + TREE + 2) * U * ref["l1"]
    di, dnk, dsk = image_bwd(W, H, dev(image), dev(gt), **kw, g_loss=dev(np.array([1.0], dtype=F32)), g_rgb=None)
    assert np.isfinite(di).all() and np.isnan(dsk[:, 1:-1, 1:-1]).all() and np.isfinite(dsk[:, 0]).all()
    assert_bits(di, R.image_loss_bwd_exact(image, 0, None, gt, None, None, None, None, None, 0.8, 0.015, 1.0, None)[0], "d_image")


def test_ncc_and_geo_thresholds():
    lim = F32(0.9)
    lo, hi = np.nextafter(lim, F32(0)), np.nextafter(lim, F32(1))
    ncc = np.array([lo, lim, hi, 0.5, -0.25, 1.0, lo, hi], dtype=F32)
    w = np.array([1, 1, 1, 0.5, 2, 1, 0.25, 4], dtype=F32)
    val, cnt = R.ncc_tail_f64(ncc, w)
    assert cnt == 4
    out = ncc_fwd(8, dev(ncc), dev(w))
    assert out[1] == 4 and abs(out[0] - val) <= (1 + TREE + R.C_NCC + 1) * U * float(np.abs(ncc.astype(F64) * w)[ncc < lim].sum()) / 4
    d = ncc_bwd(8, dev(ncc), dev(w), dev(out), dev(np.array([2.0], dtype=F32)))
    assert_bits(d, R.d_ncc_exact(ncc, w, 4, 2.0), "d_ncc")
    assert [bool(v) for v in d != 0] == [True, False, False, True, True, False, True, False]
    assert_bits(ncc_fwd(3, dev(np.array([lim, hi, 1.0], dtype=F32)), dev(w[:3])), [0.0, 0.0], "an empty NCC mask")
    # noise at 1 and its neighbours, angle at the threshold; inf / NaN noise (and angle) on invalid pixels
    one, thr = F32(1), F32(0.3)
    noise = np.array([np.nextafter(one, F32(0)), one, np.nextafter(one, F32(2)), 0.5, np.inf, np.nan, 0.25, np.inf, 0.5], dtype=F32)
    angle = np.array([0.1, 0.1, 0.1, np.nextafter(thr, F32(0)), 0.1, 0.1, thr, np.nan, np.nextafter(thr, F32(1))], dtype=F32)
    valid = np.array([1, 1, 1, 1, 0, 0, 1, 0, 1], dtype=bool)
    for decay in (F32(0.0), F32(0.5)):
        r = R.mv_geo_f64(noise, angle, valid, thr, decay, F32(2.0), F32(0.05))
        assert r["n0"] == 4 and r["n1"] == 4 and np.isfinite(r["out0"])
        out, pv, w_ncc = geo_fwd(9, dev(noise), dev(angle), dev(valid), thr, decay, 2.0, 0.05)
        assert out[1] == 4 and out[2] == 4 and list(pv) == [1, 0, 0, 1, 0, 0, 1, 0, 1]
        assert abs(out[0] - r["out0"]) <= (1 + TREE + R.C_GEO_ANGLE + 1 + 3) * U * r["out0"]
        assert bool((np.abs(w_ncc - r["w_ncc"]) <= R.gamma(R.C_W_NCC) * r["w_ncc"]).all()) and np.isfinite(w_ncc).all()
        dn_, da_ = R.mv_geo_bwd_f64(noise, angle, valid, thr, decay, F32(2.0), F32(0.05), 1.3)
        gn, ga = geo_bwd(9, dev(noise), dev(angle), dev(valid), thr, decay, 2.0, 0.05, dev(out), dev(np.array([1.3], dtype=F32)))
        assert np.isfinite(gn).all() and np.isfinite(ga).all()
        assert bool((np.abs(gn - dn_) <= R.gamma(R.C_GEO_DNOISE + 1) * np.abs(dn_)).all()) and bool((np.abs(ga - da_) <= R.gamma(R.C_GEO_DANGLE + 1) * np.abs(da_)).all())
        assert [bool(v) for v in ga != 0] == [True, False, False, True, False, False, False, False, False], "angle_valid, and geo_w = 0 outside pixel_valid"
    # no valid pixel at all: empty sets count 1
    assert_bits(geo_fwd(9, dev(noise), dev(angle), dev(np.zeros(9, dtype=bool)), thr, 0.5, 2.0, 0.05)[0], [0.0, 0.0, 0.0], "nothing valid")


def test_tied_scales_send_the_whole_weight_to_the_first_minimum():
    """three equal scales: every Gaussian right after create_from_pcd.  The reference takes sort(...)[..., 0] (tie order
    unspecified): required is that exactly one tied minimum gets the whole weight; this project's rule is the first one"""
    base = np.array([[1, 1, 2], [1, 2, 1], [2, 1, 1], [1, 1, 1], [3, 2, 1], [1, 2, 3], [2, 1, 3]], dtype=F32) * F32(0.125)
    rows = np.concatenate([base, -base, np.tile(base[3:4], (300, 1))])
    Pn = rows.shape[0]
    for vis in (np.ones(Pn, dtype=bool), np.zeros(Pn, dtype=bool), np.arange(Pn) % 2 == 0):
        for raw in (0, 1):
            val, cnt = R.plane_f64(rows, raw, vis, 0.5)
            out = plane_fwd(Pn, dev(rows), raw, dev(vis), 0.5)
            mins = rows.astype(F64).min(1)
            mabs = float(np.abs(np.exp(mins) if raw else mins)[vis].sum()) / max(cnt, 1)
            assert out[1] == cnt and abs(out[0] - val) <= (2 + TREE + R.C_PLANE_RAW + 2) * U * 0.5 * mabs
            if cnt == 0:
                assert_bits(out, [0.0, 0.0], "an empty filter")
            d = plane_bwd(Pn, dev(rows), raw, dev(vis), 0.5, dev(out), dev(np.array([3.0], dtype=F32)))
            assert bool(((d != 0).sum(1) == vis).all()), "exactly one entry per visible row, none elsewhere"
            assert np.array_equal(np.argmax(d != 0, axis=1)[vis], R.first_minimum(rows)[vis]), "the first tied minimum"
            if raw:
                ref = R.plane_bwd_f64(rows, 1, vis, 0.5, cnt, 3.0)
                assert bool((np.abs(d - ref) <= R.gamma(R.C_PLANE_BWD_RAW) * np.abs(ref)).all())
            else:
                assert_bits(d, R.plane_bwd_exact(rows, vis, 0.5, cnt, 3.0), "d_scaling")
                assert abs(float(d.astype(F64).sum()) - 0.5 * 3.0 * (1 if cnt else 0)) <= 4 * U * 1.5, "the rows' weights add up to g * weight"


def test_statistics_decisions():
    n = 8
    vg = np.zeros((n, 4), dtype=F32)
    vg[:, 0], vg[:, 3] = 3.0, -2.0
    vg[:, 1] = 4.0
    vis = np.array([1, 1, 1, 1, 0, 0, 1, 1], dtype=bool)
    observe = np.array([1, 0, 2, 1, 1, 0, -1, 1], dtype=np.int32)
    radii = np.array([7, 9, 5, 6, 99, 99, 99, 0], dtype=np.int32)
    mr = np.array([7, 1, 6, 5, 1, 1, 1, 0], dtype=F32)         # equal, unobserved, larger, smaller, invisible x2, observe < 0, zero
    for all_vis in (None, True, False):
        v = vis if all_vis is None else np.full(n, all_vis)
        o = Outs(acc=(n, "f32"), ab=(n, "f32"), den=(n, "f32"), mr=(n, "f32"))
        for name, val in (("acc", np.ones(n, F32)), ("ab", np.ones(n, F32)), ("den", np.zeros(n, F32)), ("mr", mr)):
            o.fill(name, val)
        t_vg, t_v, t_ob, t_ra = dev(vg), dev(v), dev(observe), dev(radii)
        call("gs2m_densification_stats", n, P(t_vg), P(t_v), P(t_ob), P(t_ra), o.ptr("acc"), o.ptr("ab"), o.ptr("den"), o.ptr("mr"))
        assert o.intact(("acc", "ab", "den", "mr"))
        want = R.densification_exact(vg, v, observe, radii, np.ones(n, F32), np.ones(n, F32), np.zeros(n, F32), mr)
        for name, wv in zip(("acc", "ab", "den", "mr"), want):
            assert_bits(o.np(name), wv, name)
        if all_vis is None:
            assert list(o.np("mr")) == [7, 1, 6, 6, 1, 1, 1, 0] and list(o.np("acc")) == [6, 6, 6, 6, 1, 1, 6, 6] and list(o.np("ab")[:2]) == [3, 3]


# ================================================================ (e) edge gradient
EDGE_FRAMES = [(511, 513), (512, 512), (481, 545), (6, 87381), (3, 174763), (1023, 1025), (17, 61681), (3, 3), (3, 200), (200, 3), (5, 4)]


@pytest.mark.parametrize("H,W", EDGE_FRAMES, ids=lambda v: str(v))
def test_edge_gradient_bitwise_and_extrema_at_the_chunk_edges(H, W):
    gt = _np_frames(H, W, seed=H + 5 * W)[1]
    want = R.edge_exact(gt)
    edge, mm = edge_gradient(dev(gt), W, H)
    assert_bits(edge, want, "edge")
    assert not edge[0].any() and not edge[-1].any() and not edge[:, 0].any() and not edge[:, -1].any()
    inner = want[1:-1, 1:-1]
    assert_bits(mm, [inner.min(), inner.max()], "minmax")
    # planted extrema.  Maximum: a flat frame, channel 1 raised to 0.75 right of p and lowered to 0 left of it: p alone has
    # strength 0.75 / 3 = 0.25 (its other neighbours see a step of 0.5 or 0.25).  Minimum: a ramp along x of slope 2^-20
    # (strength 2^-19 at every interior pixel), p's two horizontal neighbours set equal: p alone has strength 0.
    HW, chunk = H * W, -(-H * W // LG)
    interior = lambda p: 0 < p // W < H - 1 and 0 < p % W < W - 1
    cand = {W + 1, 2 * W - 2, HW - 2 * W + 1, HW - W - 2}                 # the first and the last interior pixel, and the ends of their rows
    for b in (1, 2, 255):
        cand |= {b * chunk - 2, b * chunk - 1, b * chunk, b * chunk + 1}   # the last and the first pixel of a workgroup's chunk
    cand |= {RB - 1, RB, RU * RB - 1, RU * RB}
    cand |= {(H // 2) * W + 1, (H // 2) * W + W - 2, W + W // 2, HW - 2 * W + W // 2}   # next to each border
    pix = sorted(p for p in cand if 0 <= p < HW and interior(p))
    flat = torch.full((3, HW), 0.25, device="cuda")
    ramp = dev((np.arange(W, dtype=F32)[None, None, :] * F32(2.0 ** -20) * np.ones((3, H, 1), dtype=F32)).reshape(3, HW))
    n_inner = (H - 2) * (W - 2)
    for p in pix:
        flat[1, p + 1], flat[1, p - 1] = 0.75, 0.0
        e, m = edge_gradient(flat, W, H)
        if HW <= 20000:
            assert_bits(e, R.edge_exact(flat.cpu().numpy().reshape(3, H, W)), ("edge, planted maximum", p))
        flat[1, p + 1], flat[1, p - 1] = 0.25, 0.25
        assert e.reshape(-1)[p] == F32(0.25) and int((e == F32(0.25)).sum()) == 1 and float(e.max()) == 0.25, p
        assert_bits(m, [0.25 if n_inner == 1 else e[1:-1, 1:-1].min(), 0.25], ("the maximum planted at", p))
        assert n_inner < 12 or m[0] == 0
        keep = ramp[:, p - 1].clone(), ramp[:, p + 1].clone()
        ramp[:, p - 1] = ramp[:, p + 1] = 0.5
        e, m = edge_gradient(ramp, W, H)
        if HW <= 20000:
            assert_bits(e, R.edge_exact(ramp.cpu().numpy().reshape(3, H, W)), ("edge, planted minimum", p))
        ramp[:, p - 1], ramp[:, p + 1] = keep
        inner = e[1:-1, 1:-1]
        assert e.reshape(-1)[p] == 0 and int((inner == 0).sum()) == 1, p
        assert_bits(m, [0.0, inner.max()], ("the minimum planted at", p))
        assert n_inner == 1 or m[1] >= F32(2.0 ** -19)


# ================================================================ (f) the random subset, exactly
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 1080 * 1920, 1024 * 1025 + 3])
def test_subset_thin_is_the_restated_list(n):
    rng = np.random.default_rng(n)
    masks = {"all": np.ones(n, dtype=bool), "none": np.zeros(n, dtype=bool), "one": np.arange(n) == (n * 2) // 3, "70%": rng.random(n) < 0.7}
    for label, mask in masks.items():
        count = int(mask.sum())
        for k in sorted({1, max(count // 7, 1), max(count, 1), count + 5}):
            seed = int(rng.integers(0, 2 ** 63))
            want, cnt = R.subset_thin(mask, k, seed)
            assert cnt == count
            if k >= count:
                assert want.shape[0] == count, "p = 1"
            m = want.shape[0]
            for cap in sorted({m + 3, max(m // 2, 1)}):
                idx, counts = subset_thin(n, dev(mask), k, seed, cap)
                assert counts[0] == count and counts[1] == m, (label, k, cap, counts, m)
                kept = min(m, cap)
                assert np.array_equal(idx[:kept], want[:kept]), (label, n, k, cap)
                assert bool((idx[kept:].view(np.uint8) == CANARY).all()), "words beyond the survivors keep the canary"


@pytest.mark.parametrize("k", [1, 2, 100, 10_000, 102_400])
def test_subset_remove_is_the_restated_list(k):
    rng = np.random.default_rng(k)
    for e in sorted({1, 2, max(k // 100, 1), max(k // 3, 1)}):
        m = k + e
        idx = np.sort(rng.choice(4 * m + 10, m, replace=False)).astype(np.int64)
        for rep in range(3):
            seed = int(rng.integers(0, 2 ** 63))
            got = subset_remove(m, k, seed, dev(idx))
            assert bool((np.diff(got) > 0).all()) and bool(np.isin(got, idx).all()), "distinct, increasing, survivors"
            assert np.array_equal(got, R.subset_remove(m, k, seed, idx)), (m, k, seed)


def test_subset_remove_where_two_strata_floor_to_one_position():
    """neighbouring strata can give removed_i == removed_(i+1): the keys removed_i - i then step down by one; the output must
    still be k distinct survivors in increasing order, and the list the bisection in those keys gives"""
    m, k = 1234, 1000
    idx = np.arange(m, dtype=np.int64) * 3 + 1
    found = 0
    for seed in range(1, 400):
        rem = R.subset_removed(m, k, seed)
        if bool((np.diff(rem) > 0).all()):
            continue
        found += 1
        got = subset_remove(m, k, seed, dev(idx))
        assert bool((np.diff(got) > 0).all()) and bool(np.isin(got, idx).all()), seed
        assert np.array_equal(got, R.subset_remove(m, k, seed, idx)), seed
        if found == 5:
            break
    assert found == 5


# ================================================================ (g) the workspace hand-off
def _reducers():
    """(name, call) of every reducing kernel on fixed continuous inputs -> the bits of its outputs"""
    H, W, n = 123, 457, 300_007
    image, gt, normal, sobel, _, wm = (dev(t) for t in _np_frames(H, W, seed=8))
    edge_np = R.edge_exact(gt.cpu().numpy())
    edge, mm = dev(edge_np), dev(np.array([edge_np[1:-1, 1:-1].min(), edge_np[1:-1, 1:-1].max()], dtype=F32))
    rng = np.random.default_rng(8)
    sc, vis = dev((rng.standard_normal((n, 3)) - 4).astype(F32)), dev(rng.random(n) < 0.8)
    ncc, w = dev((rng.random(n) * 2 - 1).astype(F32)), dev(rng.random(n).astype(F32))
    noise, angle, valid = dev((rng.random(n) * 1.5).astype(F32)), dev((rng.random(n) * 0.6).astype(F32)), dev(rng.random(n) < 0.7)
    pred5 = dev(rng.random((5, H, W), dtype=F32))
    b = lambda *arrs: b"".join(np.ascontiguousarray(a).tobytes() for a in arrs)
    return [("mv_geo", lambda: b(*geo_fwd(n, noise, angle, valid, 0.3, 0.5, 2.0, 0.05))),
            ("image", lambda: b(image_fwd(W, H, image, gt, normal=normal, sobel=sobel, edge=edge, mm=mm, wm=wm)[1])),
            ("edge", lambda: b(*edge_gradient(gt, W, H))),
            ("plane", lambda: b(plane_fwd(n, sc, 1, vis, 0.01))),
            ("tv3", lambda: b(tv_fwd(W, H, 3, gt, pred5[:3].contiguous(), wm, 1, 0.37))),
            ("tv5", lambda: b(tv_fwd(W, H, 5, gt, pred5, None, 0, 1.0))),
            ("ncc", lambda: b(ncc_fwd(n, ncc, w))),
            ("mean", lambda: b(affine_mean(n - 1, w, 0.2, -0.2)))]


def test_every_reducer_after_every_other_on_one_workspace():
    red = _reducers()
    alone = {}
    for name, f in red:
        runs = [f() for _ in range(3)]
        assert runs[0] == runs[1] == runs[2], (name, "three repeats differ")
        alone[name] = runs[0]
    for first, f1 in red:            # mv_geo (four partials) in front of every kernel with two or one, and every other order
        for second, f2 in red:
            assert f1() == alone[first], (first, "before", second)
            assert f2() == alone[second], (second, "right after", first)
    assert _ws_clean()


def test_refusals_write_nothing():
    gt = torch.rand(3, 8, 8, device="cuda")
    for W, H in ((2, 8), (8, 2), (1, 524287)):
        edge_gradient(gt, W, H, rc=INVALID)
    o = Outs(out=(1, "f32"))
    call("gs2m_tv_loss_forward", 1, 8, 3, P(gt), P(gt), None, 1, 1.0, o.ptr("out"), P(_ws()), rc=INVALID)
    call("gs2m_affine_mean", 0, P(gt), 0.0, 1.0, o.ptr("out"), P(_ws()), rc=INVALID)
    call("gs2m_affine_mean", 5, P(gt) + 4, 0.0, 1.0, o.ptr("out"), P(_ws()), rc=INVALID)
    call("gs2m_subset_remove", 5, 5, 1, P(gt), o.ptr("out"), rc=INVALID)
    assert o.intact(())
