"""tests/loss_ref.py checked without a GPU, before tests/test_loss_kernels_gpu.py holds the kernels of csrc/loss_ops.hip to it:
the float64 restatements against the PyTorch expressions of gs2m_losses.py evaluated in float64 (values, and gradients through
autograd) and against the reference's own recorded outputs (tests/golden/ref_losses.npz), the float32 `*_exact` expressions
against the float64 ones within a few ulp, and the integer restatement of the random subset against what it must return."""
import os
import types

import numpy as np
import pytest
import torch

import gs2m_losses as L
import loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _frames(H, W, seed):
    """the continuous inputs of tests/test_losses_gpu._frames, as numpy"""
    g = torch.Generator().manual_seed(seed)
    image = torch.randn(3, H, W, generator=g) * 0.45 + 0.5
    gt = torch.rand(3, H, W, generator=g)
    normal = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0)
    sobel = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0)
    wm = torch.rand(1, H, W, generator=g)
    return [t.numpy() for t in (image, gt, normal, sobel, wm)]


def _t64(x):
    return torch.tensor(np.asarray(x), dtype=torch.float64)


def _rel(a, b):
    """relative difference of two scalars; two NaN (a frame with one interior pixel: 0 / 0 in the reference too) agree"""
    a, b = float(a.detach()) if torch.is_tensor(a) else float(a), float(b.detach()) if torch.is_tensor(b) else float(b)
    if np.isnan(a) and np.isnan(b):
        return 0.0
    return abs(a - b) / max(abs(b), 1e-300)


def _maxdiff(a, b):
    """largest difference of two arrays whose NaN sit at the same places"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return float(np.nanmax(np.abs(a - b), initial=0.0))


SIZES = [(24, 32), (3, 3), (5, 4), (3, 86), (37, 19)]


@pytest.mark.parametrize("H,W", SIZES)
def test_f64_equals_the_pytorch_expressions_in_float64(H, W):
    image, gt, normal, sobel, wm = _frames(H, W, seed=H * 100 + W)
    rgb = R.rgb_exact(image)
    assert np.array_equal(rgb, torch.tensor(image).clamp(0, 1).numpy())
    assert _rel(R.l1_f64(rgb, gt), L.l1_loss(_t64(rgb), _t64(gt))) < 1e-12
    # the edge weight: normalised strength, then (1 - .).clamp(0, 1) ** 2; from the raw strength and its min / max as the kernels get it
    assert _maxdiff(R.img_grad_weight_f64(gt), L.image_gradient_weight(_t64(gt)).numpy()) < 1e-12
    raw = R.img_grad_f64(gt)
    w = R.edge_weight_f64(np.pad(raw, 1), raw.min(), raw.max())
    assert _maxdiff(w, L.edge_weights(_t64(gt)).numpy()) < 1e-12
    assert _maxdiff(w, np.clip(1.0 - R.img_grad_weight_f64(gt), 0, 1) ** 2) < 1e-12
    for weight_map in (None, wm):
        got = R.depth_normal_f64(normal, sobel, R.dn_weight(H, W, np.pad(raw, 1), (raw.min(), raw.max()), weight_map))
        want = L.depth_normal_loss(_t64(normal), _t64(sobel), _t64(gt), weight_map=None if weight_map is None else _t64(weight_map))
        assert _rel(got, want) < 1e-12
    assert _rel(R.depth_normal_f64(normal, sobel, R.dn_weight(H, W, None, None, wm)), (_t64(wm)[0] * (_t64(sobel) - _t64(normal)).abs().sum(0)).mean()) < 1e-12
    full = R.image_loss_f64(image, 0, None, None, gt, normal, sobel, np.pad(raw, 1).astype(F32), (F32(raw.min()), F32(raw.max())), wm, 0.8, 0.015)
    assert _rel(full["out0"], float(F32(0.8)) * full["l1"] + float(F32(0.015)) * full["dn"]) < 1e-15
    # total variation, value and gradient
    g = torch.Generator().manual_seed(H + W)
    for C, norm1, weighted in ((1, False, False), (3, True, False), (3, True, True), (2, False, True), (4, True, True), (5, False, False)):
        pred = torch.rand(C, H, W, generator=g).numpy()
        p = _t64(pred).requires_grad_(True)
        want = L.tv_loss(_t64(gt), p, norm1=norm1, weight_map=_t64(wm) if weighted else None)
        got = R.tv_f64(gt, pred, wm if weighted else None, norm1, 0.37)
        assert _rel(got[0], float(F32(0.37)) * float(want.detach())) < 1e-12 and _rel(got[1] + got[2], want) < 1e-12
        (want * float(F32(0.37)) * float(F32(0.7))).backward()
        d, mag = R.tv_bwd_f64(gt, pred, wm if weighted else None, norm1, 0.37, 0.7)
        assert np.abs(d - p.grad.numpy()).max() <= 1e-12 * max(mag.max(), 1e-300)
        assert bool((np.abs(d) <= mag * (1 + 1e-12)).all())


@pytest.mark.parametrize("P,frac", [(200, 0.6), (1, 1.0), (257, 0.0), (1025, 0.9)])
def test_plane_f64_equals_plane_loss_in_float64(P, frac):
    g = torch.Generator().manual_seed(P)
    raw = (torch.randn(P, 3, generator=g) - 3.0).numpy()
    vis = (torch.rand(P, generator=g) < frac).numpy()
    r = _t64(raw).requires_grad_(True)
    want = L.plane_loss(torch.tensor(vis), types.SimpleNamespace(get_scaling=torch.exp(r)))
    got, n = R.plane_f64(raw, 1, vis, 0.25)
    assert n == int(vis.sum()) and abs(got - 0.25 * float(want)) <= 1e-12 * abs(float(want))
    act = np.exp(raw.astype(np.float64)).astype(F32)
    assert abs(R.plane_f64(act, 0, vis)[0] - float(L.plane_loss(torch.tensor(vis), types.SimpleNamespace(get_scaling=_t64(act))))) <= 1e-12 * abs(got) + 0.0
    (want * 0.25 * 3.0).backward()
    d = R.plane_bwd_f64(raw, 1, vis, 0.25, n, 3.0)
    assert np.abs(d - r.grad.numpy()).max() <= 1e-12 * max(np.abs(d).max(), 1e-300)
    # the float32 expression of the non-raw backward: one value, at the first minimum
    ex = R.plane_bwd_exact(act, vis, 0.25, n, 3.0)
    f = R.plane_bwd_f64(act, 0, vis, 0.25, n, 3.0)
    assert np.array_equal(ex != 0, f != 0) and np.abs(ex - f).max() <= 3 * R.U * np.abs(f).max()


def test_ties_go_to_the_first_minimum_as_torch_min_does():
    rows = np.array([[1, 1, 2], [1, 2, 1], [2, 1, 1], [1, 1, 1], [3, 2, 1], [0.5, 0.5, 0.5]], dtype=F32)
    assert list(R.first_minimum(rows)) == [0, 0, 1, 0, 2, 0]
    assert list(R.first_minimum(rows)) == list(torch.tensor(rows).min(dim=-1).indices.numpy())
    s = _t64(rows).requires_grad_(True)
    L.plane_loss(torch.ones(6, dtype=torch.bool), types.SimpleNamespace(get_scaling=s)).backward()
    assert np.array_equal(s.grad.numpy(), R.plane_bwd_f64(rows, 0, np.ones(6, bool), 1.0, 6, 1.0))
    assert np.array_equal((R.plane_bwd_exact(rows, np.ones(6, bool), 1.0, 6, 1.0) != 0).sum(1), np.ones(6))


def test_f64_equals_the_recorded_outputs_of_the_reference():
    """tests/golden/ref_losses.npz: the reference's own l1_loss, _get_img_grad_weight, depth_normal_loss, tv_loss, plane_loss
    in float32; 2e-5 is what those float32 values allow"""
    z = dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_losses.npz")))
    close = lambda a, b: abs(float(a) - float(b)) <= 2e-5 * max(1.0, abs(float(b)))
    rgb = R.rgb_exact(z["img"])
    assert close(R.l1_f64(rgb, z["gt"]), z["l1"])
    assert np.abs(R.img_grad_weight_f64(z["gt"]) - z["img_grad_weight"]).max() <= 2e-5
    raw = R.img_grad_f64(z["gt"])
    H, W = z["gt"].shape[1:]
    edge, mm = np.pad(raw, 1), (raw.min(), raw.max())
    assert close(R.depth_normal_f64(z["normal"], z["sobel"], R.dn_weight(H, W, edge, mm, None)), z["depth_normal"])
    assert close(R.depth_normal_f64(z["normal"], z["sobel"], R.dn_weight(H, W, edge, mm, z["wm"])), z["depth_normal_wm"])
    assert close(R.tv_f64(z["gt"], z["pred1"], None, False)[0], z["tv_l2_c1"])
    assert close(R.tv_f64(z["gt"], z["pred3"], None, True)[0], z["tv_l1_c3"])
    assert close(R.tv_f64(z["gt"], z["pred3"], z["wm"], True)[0], z["tv_l1_c3_wm"])
    assert close(R.plane_f64(z["raw_scale"], 1, z["vis"])[0], z["plane"])
    assert R.plane_f64(z["raw_scale"], 1, np.zeros_like(z["vis"]))[0] == float(z["plane_none_visible"]) == 0.0


@pytest.mark.parametrize("H,W", SIZES)
def test_exact_agrees_with_f64_within_a_few_ulp(H, W):
    image, gt, normal, sobel, wm = _frames(H, W, seed=H + 7 * W)
    # edge strength: three differences, two adds, one quotient -> 6 roundings of values below 1
    e = R.edge_exact(gt)
    assert e.dtype == F32 and e.shape == (H, W)
    assert np.abs(e[1:-1, 1:-1] - R.img_grad_f64(gt)).max() <= 6 * R.U
    assert not e[0].any() and not e[-1].any() and not e[:, 0].any() and not e[:, -1].any()
    if H > 3 or W > 3:
        mn, mx = e[1:-1, 1:-1].min(), e[1:-1, 1:-1].max()
        w32, w64 = R.edge_weight_exact(e, mn, mx), R.edge_weight_f64(e, mn, mx)
        assert w32.dtype == F32 and np.abs(w32 - w64).max() <= 8 * R.U
        assert bool((w32[0] == 1).all()) and bool((w32[:, -1] == 1).all())
    else:
        mn, mx = F32(0.0), F32(1.0)
    # the backward of the image loss against float64 autograd of the same expression
    for hwc in (0, 1):
        img = np.ascontiguousarray(image.transpose(1, 2, 0)) if hwc else image
        mask = (np.arange(H * W).reshape(H, W) % 3 != 0) if hwc else None
        bg = np.array([0.2, 1.0, 0.0], dtype=F32) if hwc else None
        g_rgb = (image * 1e-3).astype(F32)
        di, dn, ds = R.image_loss_bwd_exact(img, hwc, mask, gt, normal, sobel, e, (mn, mx), wm, 0.8, 0.015, 1.7, g_rgb)
        x, n, s = (_t64(t).requires_grad_(True) for t in (img, normal, sobel))
        rgb = x.permute(2, 0, 1).clamp(0, 1) if hwc else x.clamp(0, 1)
        if hwc:
            rgb = torch.where(torch.tensor(mask)[None], rgb, _t64(bg)[:, None, None])
        assert np.array_equal(rgb.detach().numpy().astype(F32), R.rgb_exact(img, hwc, mask, bg))
        wt = torch.tensor(R.dn_weight(H, W, e, (mn, mx), wm))
        loss = float(F32(0.8)) * L.l1_loss(rgb, _t64(gt)) + float(F32(0.015)) * (wt * (s - n).abs().sum(0)).mean()
        (float(F32(1.7)) * loss + (rgb * _t64(g_rgb)).sum()).backward()
        assert di.shape == img.shape and di.dtype == F32
        tol = 4 * R.U * (np.abs(g_rgb).max() + 1.7 * 0.8 / (3 * H * W))
        assert np.abs(di - x.grad.numpy()).max() <= tol
        assert np.abs(ds - s.grad.numpy()).max() <= 12 * R.U * 1.7 * 0.015 / (H * W) and np.array_equal(dn, -ds)
        assert np.abs(dn - n.grad.numpy()).max() <= 12 * R.U * 1.7 * 0.015 / (H * W)
    # no upstream gradients at all: zeros
    di, dn, ds = R.image_loss_bwd_exact(image, 0, None, gt, None, None, None, None, None, 0.8, 0.0, None, None)
    assert not di.any() and dn is None and ds is None


def test_ncc_tail_mv_geo_and_statistics_restatements():
    g = torch.Generator().manual_seed(11)
    n = 3000
    ncc = (torch.rand(n, generator=g) * 2 - 1).numpy()
    ncc[:3] = [np.nextafter(F32(0.9), F32(0)), F32(0.9), np.nextafter(F32(0.9), F32(1))]
    w = torch.rand(n, generator=g).numpy()
    c, wt = _t64(ncc).requires_grad_(True), _t64(w)
    m = torch.tensor(ncc) < 0.9          # the float32 comparison of the reference
    want = (c * wt)[m].mean()
    loss, cnt = R.ncc_tail_f64(ncc, w)
    assert cnt == int(m.sum()) == int((ncc[3:] < 0.9).sum()) + 1 and _rel(loss, want) < 1e-12
    (want * float(F32(0.3))).backward()
    d = R.d_ncc_exact(ncc, w, cnt, 0.3)
    assert d.dtype == F32 and np.abs(d - c.grad.numpy()).max() <= 2 * R.U * np.abs(c.grad.numpy()).max() and d[1] == 0 and d[2] == 0 and d[0] != 0
    assert R.ncc_tail_f64(np.ones(5, F32), np.ones(5, F32)) == (0.0, 0)
    # the geometric part: the reference's lines with float64 tensors
    noise = (torch.rand(n, generator=g) * 1.5).numpy()
    angle = (torch.rand(n, generator=g) * 0.6).numpy()
    valid = (torch.rand(n, generator=g) < 0.7).numpy()
    noise[~valid] = np.where(np.arange((~valid).sum()) % 2 == 0, np.inf, np.nan).astype(F32)
    thr, decay, factor, weight = F32(0.3), F32(0.5), F32(2.0), F32(0.05)
    nz, an = _t64(np.where(valid, noise, 0.0)).requires_grad_(True), _t64(angle).requires_grad_(True)
    v = torch.tensor(valid)
    angle_valid = v & (torch.tensor(angle) < float(thr))
    pixel_valid = v & (torch.tensor(np.where(valid, noise, 7.0)) < 1.0)
    geo_weights = torch.exp(-nz * float(decay)).detach()
    geo_weights[~pixel_valid] = 0
    ref = float(weight) * ((geo_weights * nz)[pixel_valid].mean() + (geo_weights * (float(factor) * an))[angle_valid].mean())
    r = R.mv_geo_f64(noise, angle, valid, thr, decay, factor, weight)
    assert r["n0"] == int(pixel_valid.sum()) and r["n1"] == int(angle_valid.sum()) and _rel(r["out0"], ref) < 1e-12
    assert np.isfinite(r["out0"]) and np.array_equal(r["pixel_valid"], pixel_valid.numpy())
    (ref * float(F32(1.3))).backward()
    dnz, dan = R.mv_geo_bwd_f64(noise, angle, valid, thr, decay, factor, weight, 1.3)
    assert np.abs(dnz - nz.grad.numpy()).max() <= 1e-12 * np.abs(dnz).max() and np.abs(dan - an.grad.numpy()).max() <= 1e-12 * np.abs(dan).max()
    # statistics
    P = 500
    vg = torch.randn(P, 4, generator=g).numpy()
    vis = (torch.rand(P, generator=g) < 0.8).numpy()
    observe = torch.randint(0, 3, (P,), generator=g, dtype=torch.int32).numpy()
    radii = torch.randint(0, 200, (P,), generator=g, dtype=torch.int32).numpy()
    acc, ab, den, mr = (torch.rand(P, generator=g).numpy() * s for s in (1, 1, 1, 100))
    mr[:50] = radii[:50]
    ex, hi = R.densification_exact(vg, vis, observe, radii, acc, ab, den, mr), R.densification_f64(vg, vis, observe, radii, acc, ab, den, mr)
    for a, b in zip(ex[:2], hi[:2]):
        assert a.dtype == F32 and np.abs(a - b).max() <= 4 * R.U * np.abs(b).max()
    assert np.array_equal(ex[2], hi[2].astype(F32)) and np.array_equal(ex[3], hi[3].astype(F32))
    assert np.array_equal(ex[3][~vis], mr[~vis]) and np.array_equal(ex[0][~vis], acc[~vis])
    assert R.densification_exact(vg, vis, None, None, acc, ab, den, None)[3] is None
    # mv_take and its backward are copies
    H, W = 9, 13
    idx = np.array([0, 5, 13, 116, 57], dtype=np.int64)
    nm, dm = torch.rand(3, H, W, generator=g).numpy(), torch.rand(H, W, generator=g).numpy()
    px, nr, ds, ww = R.mv_take_exact(idx, W, H, nm, dm, None)
    assert px.tolist() == [[0, 0], [5, 0], [0, 1], [12, 8], [5, 4]] and np.array_equal(nr[3], nm[:, 8, 12]) and ds[4] == dm[4, 5] and bool((ww == 1).all())
    bn, bd = R.mv_take_bwd_exact(idx, W, H, nr, ds)
    assert np.array_equal(bn[:, 8, 12], nm[:, 8, 12]) and bd[4, 5] == dm[4, 5] and int((bd != 0).sum()) == 5


def test_the_mix_is_splitmix64():
    """the first outputs of splitmix64 seeded with 0 (Vigna's reference implementation): state += golden, then the finaliser;
    subset_mix adds the golden constant itself, so mix(j * golden) is output j + 1"""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    golden = 0x9E3779B97F4A7C15
    got = [int(R.subset_mix(np.uint64((j * golden) & R.MASK64))) for j in range(3)]
    assert got == want
    i = np.arange(5, dtype=np.uint64)
    py = [(7 ^ (int(k) * 0xD1342543DE82EF95)) & R.MASK64 for k in i]
    assert [int(x) for x in R.subset_bits(7, i)] == [int(R.subset_mix(np.uint64(v))) for v in py]


@pytest.mark.parametrize("n,frac,k", [(1, 1.0, 1), (1023, 1.0, 100), (1024, 0.7, 100), (1025, 0.0, 10), (5000, 0.7, 5000), (200_000, 0.7, 3000),
                                      (200_000, 1.0, 20_000), (1024 * 1025 + 3, 0.7, 100_000), (50_000, 0.0002, 5)])
def test_subset_returns_exactly_min_k_count_distinct_set_indices_in_order(n, frac, k):
    rng = np.random.default_rng(n + k)
    mask = rng.random(n) < frac
    done = 0
    for s in range(4):
        seed1, seed2 = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 63))
        surv, count = R.subset_thin(mask, k, seed1)
        assert count == int(mask.sum()) and bool(mask[surv].all()) and bool((np.diff(surv) > 0).all())
        if k >= count:
            assert surv.shape[0] == count, "p = 1: every set element survives"
        m = surv.shape[0]
        if m > k and 4 * (m - k) <= m:
            rem = R.subset_removed(m, k, seed2)
            assert bool((np.diff(rem) >= 0).all()) and rem[0] >= 0 and rem[-1] <= m - 1, "one removal per stratum, in order"
            if bool((np.diff(rem) > 0).all()):   # (two neighbouring strata can floor to one position: then one survivor more is skipped)
                assert np.array_equal(R.subset_remove(m, k, seed2, surv), surv[np.setdiff1d(np.arange(m), rem)])
        out = R.random_subset(mask, k, seed1, seed2)
        if out is None:
            continue
        done += 1
        assert out.dtype == np.int64 and out.shape[0] == min(k, count)
        assert bool((np.diff(out) > 0).all()) and bool(mask[out].all())
    if k >= 1000 or k >= mask.sum():   # (a small k out of a long list removes more than a quarter: the caller's plain path)
        assert done >= 3, "the two steps apply to nearly every draw"


def test_bisection_counts_on_sorted_keys_and_keeps_k_distinct_survivors_on_tied_strata():
    rng = np.random.default_rng(2)
    key = np.sort(rng.integers(0, 50, 37))
    j = np.arange(-2, 55)
    assert np.array_equal(R.bisect_right(key, j), np.searchsorted(key, j, side="right"))
    assert np.array_equal(R.bisect_right(key[:1], j), np.searchsorted(key[:1], j, side="right"))
    m, k, tied = 1234, 1000, 0
    idx = np.arange(m, dtype=np.int64) * 3 + 1
    for seed in range(1, 200):
        rem = R.subset_removed(m, k, seed)
        tied += int(not (np.diff(rem) > 0).all())
        out = R.subset_remove(m, k, seed, idx)
        assert out.shape[0] == k and bool((np.diff(out) > 0).all()) and bool(np.isin(out, idx).all())
    assert tied >= 5, "m / e = 5.27: neighbouring strata do floor to one position now and then"


def test_thinning_is_uniform_enough_to_be_the_right_bits():
    """u = (bits >> 40) 2^-24 is uniform on the 2^-24 grid: the share below p is p within 5 sigma"""
    n, k = 400_000, 40_000
    surv, count = R.subset_thin(np.ones(n, bool), k, 12345)
    p = float(R.subset_p(k, n))
    assert count == n and abs(surv.shape[0] - p * n) < 5 * np.sqrt(n * p * (1 - p))
    assert p == float((F32(k) + F32(4) * np.sqrt(F32(k))) / F32(n)) and R.subset_p(5, 3) == 1 and R.subset_p(1, 0) == 1
