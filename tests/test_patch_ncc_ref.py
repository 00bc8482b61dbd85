"""The float64 arbiters of tests/patch_ncc_ref.py against OUTPUTS OF THE REFERENCE's own photometric chain
(tests/golden/ref_patch_ncc.npz, written by tests/golden/make_patch_ncc_golden.py), the recorded yardstick ratios that K is
derived from, and the conditions the GPU tests' scenes must meet, asserted from the float64 margins alone: flip-band shares and
the presence of every named edge.  CPU only."""
import os

import numpy as np
import pytest
import torch

import patch_ncc_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_patch_ncc.npz")


def _golden():
    z = np.load(GOLD)
    rc, nc = R.RefCam.from_numbers(z["ref_cam"]), R.RefCam.from_numbers(z["near_cam"])
    return z, rc, nc, float(z["ncc_scale"]), int(z["patch"])


def test_restatement_and_op_by_op_reproduce_the_reference_chain():
    """The reference's float32 run sums the RAW moments (grey values ~0.5: sums of ~12 for 49 taps), so its own rounding is
    6 float32 roundings of the largest raw moment in each of cross and the two variances; carried through the quotient that is
    the tolerance per sample -- it comes from the golden's number format and terms, not from the code under test.  The masks are
    compared where the float64 value is further from the threshold than that."""
    import gs2m_mvs as MV
    z, rc, nc, scale, patch = _golden()
    assert z["ref_gray"].shape == (18, 24) and len(z["dists"]) == 48 and 0 < z["mask"].sum() < 48 and 0 < z["std_mask"].sum() < 48
    M, b, Kinv = R.homography_constants(rc, nc, scale)
    args = (z["pixels"], z["normals"], z["dists"], z["ref_gray"], z["near_gray"], M, b, Kinv, scale, patch)
    f = R.chain(*args, dtype=np.float64)
    t = R.restate(*[torch.tensor(np.asarray(a, np.float64)) for a in args[:8]], scale, patch)
    raw_moment = np.maximum((f.rv ** 2).sum(1), (f.bv ** 2).sum(1))
    d = 6 * 2 * R.U * raw_moment
    cc = f.cross ** 2 / f.D
    tol = 2 * np.abs(f.cross) * d / f.D + cc * (f.ref_var + f.nea_var) * d / f.D + 4 * R.U
    for name, x in (("restate", t.ncc.numpy()), ("chain", f.ncc)):
        err = np.abs(x - z["ncc"].reshape(-1).astype(np.float64))
        print(name, "ncc to golden: worst err / tol", (err / tol).max(), "worst err", err.max())
        assert (err <= tol).all(), (name, (err / tol).max())
    clear = np.abs(f.ncc - 0.9) > tol
    assert clear.sum() >= 40 and np.array_equal(t.mask.numpy()[clear], z["mask"].reshape(-1)[clear])
    sw_clear = np.abs(np.sqrt(f.ref_var) - 0.01) > d / (2 * np.sqrt(f.ref_var))
    assert sw_clear.sum() >= 40 and np.array_equal(t.switch.numpy()[sw_clear], z["std_mask"].reshape(-1)[sw_clear])
    assert np.abs(t.ncc.numpy() - z["ncc_gray"].reshape(-1)).max() <= tol.max()
    # the Sobel magnitudes: sqrt(gx^2 + gy^2 + 1e-6) >= 1e-3 with |gx| <= 4 -- raw moments of at most 49 x 32; same rule
    s = f.sobel
    ds = 6 * 2 * R.U * np.maximum((f.gr ** 2).sum(1), (f.gv ** 2).sum(1))
    tol_s = 2 * np.abs(s.cross) * ds / s.D + s.cross ** 2 / s.D * (s.ref_var + s.nea_var) * ds / s.D + 4 * R.U
    err = np.abs(t.ncc_grad.numpy() - z["ncc_grad"].reshape(-1))
    print("ncc_grad to golden: worst err / tol", (err / tol_s).max())
    assert (err <= tol_s).all()
    # gs2m_mvs.patch_ncc_torch, the project's op-by-op formulation, in float32 (the golden's own precision) and in float64
    cam, near = R.project_camera(rc, z["ref_gray"]), R.project_camera(nc, z["near_gray"])
    pix, n, dd = (torch.tensor(z[k]) for k in ("pixels", "normals", "dists"))
    a, ma = MV.patch_ncc_torch(pix, n, dd, cam, near, scale, patch)
    assert (np.abs(a.numpy().reshape(-1) - z["ncc"].reshape(-1)) <= 2 * tol).all() and np.array_equal(ma.numpy().reshape(-1)[clear], z["mask"].reshape(-1)[clear])
    a64, _ = MV.patch_ncc_torch(pix, n, dd, cam, near, scale, patch, dtype=torch.float64)
    assert np.abs(a64.numpy().reshape(-1) - t.ncc.numpy()).max() <= 1e-6, "both float64 formulations (the constants differ by their float32 rounding)"
    g, gg, sm = MV.patch_ncc_torch(pix, n, dd, cam, near, scale, patch, roughness=True)
    assert (np.abs(gg.numpy().reshape(-1) - z["ncc_grad"].reshape(-1)) <= 2 * tol_s).all()
    assert np.array_equal(sm.numpy().reshape(-1)[sw_clear], z["std_mask"].reshape(-1)[sw_clear])


@pytest.mark.parametrize("name,patch", [("production", 1), ("production", 4), ("borders", 8), ("thrown", 3), ("half", 3)])
def test_hand_chain_equals_autograd(name, patch):
    """The numpy chain at float64 (the source of every error-scale term, with the backward written out as the kernel's header
    states it) against the torch restatement with autograd: values and gradients to float64 rounding, outside the flip band
    (on a cell line autograd takes one side)."""
    r = R.reference(name, patch)
    a, b = R.outputs_of(r.f64), R.outputs_of(r.t)
    ok = ~r.k["flip_grad"]
    for k in a:
        x, y = a[k][ok], b[k][ok]
        fin = np.isfinite(y)
        assert np.abs(x[fin] - y[fin]).max() <= 1e-9 * max(1.0, np.abs(y[fin]).max()), k
    assert r.t.ncc.dtype == torch.float64 and r.f64.ncc.dtype == np.float64 and r.y32.ncc.dtype == np.float32 and r.y32.d_normals.dtype == np.float32


def test_recorded_yardstick_ratios_hold_and_K_is_three_times_them():
    worst = R.measure(verbose=False)
    for k, (reg, stiff) in worst.items():
        print(k, "regular", reg, "stiff", stiff, "recorded", R.RATIO[k])
        assert reg <= R.RATIO[k][0] and stiff <= R.RATIO[k][1], (k, reg, stiff)
        assert reg >= 0.5 * R.RATIO[k][0], "the recorded ratio is the measured one, not a generous one"
        assert R.K[k] == (3 * R.RATIO[k][0], 3 * max(R.RATIO[k]))
    gw = R.grid_measure()
    for k, v in gw.items():
        print(k, v, R.RATIO[k])
        assert 0.5 * R.RATIO[k][0] <= v <= R.RATIO[k][0]
    assert max(R.K["ncc"]) <= R.BAND and max(R.K["ref_var"]) <= R.BAND, "a threshold's band covers what the bound allows"


@pytest.mark.parametrize("name,patch", R.cases())
def test_flip_band_shares(name, patch):
    """At most 1 % of a scene's samples on the mask's and on the switch's threshold, at most 2 % left out of the gradients.  The
    identity scene is exempt from the gradient share by construction (b = 0: every tap of an integer pixel is ON a cell line, and
    the gradients are exactly 0 anyway: asserted as such on the GPU); the degenerate scene's eight degenerate samples are counted
    apart."""
    r = R.reference(name, patch)
    k, n = r.k, len(r.k["stiff"])
    base = ~k["nonfinite"]
    if name == "degenerate":
        base[r.scene.bad] = False
    print(name, patch, "mask", int((k["flip_mask"] & base).sum()), "switch", int((k["flip_switch"] & base).sum()), "grad", int((k["flip_grad"] & base).sum()), "of", n)
    assert (k["flip_mask"] & base).sum() <= 0.01 * n
    if patch <= 3:   # (the roughness variant, the only reader of the switch, takes no larger patch)
        assert (k["flip_switch"] & base).sum() <= 0.01 * n
    if name != "identity":
        assert (k["flip_grad"] & base).sum() <= 0.02 * n
    # outside the bands the float32 yardstick decides as float64 does
    ym, ys = r.y32.ncc < 0.9, np.sqrt(r.y32.ref_var) < 0.01
    assert np.array_equal(ym[~k["flip_mask"] & base], r.t.mask.numpy()[~k["flip_mask"] & base])
    assert np.array_equal(ys[~k["flip_switch"] & base], r.t.switch.numpy()[~k["flip_switch"] & base])


def test_every_named_edge_is_present():
    w, h = 32, 24
    r = R.reference("production", 3)
    s = r.scene
    frac = (s.pixels != np.round(s.pixels)).any(1)
    assert len(s.dists) == 1001 and 20 <= frac.sum() <= 60 and (s.d_ncc == 0).sum() >= 100 and (r.k["stiff"].sum() <= 0.05 * 1001)
    assert (r.t.mask.numpy().sum() >= 20) and ((~r.t.mask.numpy()).sum() >= 20), "both sides of ncc < 0.9"
    r = R.reference("half", 3)
    assert r.scene.ref_gray.shape == (24, 32) and (r.scene.pixels % 2 == 1).any(1).sum() >= 100 and r.scene.pixels.max() > 32
    r = R.reference("borders", 8)
    f = r.f64
    sides = {"left": f.px.min(1) < 0, "right": f.px.max(1) > w - 1, "top": f.py.min(1) < 0, "bottom": f.py.max(1) > h - 1}
    for k, v in sides.items():
        assert v.sum() >= 8, k
    for a, b in (("left", "top"), ("right", "top"), ("left", "bottom"), ("right", "bottom")):
        assert (sides[a] & sides[b]).sum() >= 1, (a, b)
    assert (f.px.min(1) <= -1).sum() >= 4, "taps beyond the padding limit"
    r = R.reference("thrown", 3)
    f = r.f64
    out = ~((f.qx > -1) & (f.qx < w) & (f.qy > -1) & (f.qy < h))
    cnt = {"(-1, 0)": ((f.qx > -1) & (f.qx < 0) & ~out).any(1).sum(), "(w-1, w)": ((f.qx > w - 1) & (f.qx < w) & ~out).any(1).sum(),
           "y (-1, 0)": ((f.qy > -1) & (f.qy < 0) & ~out).any(1).sum(), "y (h-1, h)": ((f.qy > h - 1) & (f.qy < h) & ~out).any(1).sum(),
           "partly": (out.any(1) & ~out.all(1)).sum(), "wholly": out.all(1).sum(), "inside": (~out.any(1)).sum()}
    print(cnt)
    assert all(v >= 4 for v in cnt.values()), cnt
    whole = out.all(1)
    assert (r.t.ncc.detach().numpy()[whole] == 1.0).all() and (r.t.d_normals[whole] == 0).all() and (r.t.d_dists[whole] == 0).all()
    r = R.reference("flat", 3)
    kind = r.scene.kind
    assert (r.f64.ref_var[kind == 0] == 0).all() and (r.t.ncc.detach().numpy()[kind == 0] == 1.0).all() and (r.t.d_normals[kind == 0] == 0).all()
    assert r.k["stiff"][kind == 0].all() and r.k["stiff"][kind == 1].all() and (kind == 1).sum() == 80 and (~r.k["stiff"][kind == 2]).sum() >= 40
    assert r.t.switch.numpy()[kind < 2].all() and (~r.t.switch.numpy()[kind == 2]).sum() >= 40
    assert (r.f64.D[kind == 1] < R.STIFF_D * 1e-8).all() and (r.f64.ref_var[kind == 1] > 0).all()
    r = R.reference("identity", 3)
    assert (r.scene.b == 0).all() and (r.f64.raw < R.STIFF_CORR).all() and r.k["stiff"].all() and (r.t.d_normals == 0).all() and (r.t.d_dists == 0).all()
    r = R.reference("degenerate", 3)
    bad = r.scene.bad
    assert r.k["stiff"][np.delete(bad, 4)].all()   # (n . r = 0 is degenerate only in name: h = M p there)
    assert r.k["nonfinite"][bad].sum() >= 2 and (~r.k["nonfinite"][bad]).sum() >= 3
    assert (~r.k["stiff"][np.setdiff1d(np.arange(64), bad)]).sum() >= 40
    hz = r.f64.h[2]
    assert ((np.sign(hz).min(1) < 0) & (np.sign(hz).max(1) > 0))[bad].sum() >= 2, "hz through 0 inside the patch"
    assert (np.abs(r.f64.s[bad[4], 24]) < 1e-7), "n . r = 0 at the patch centre"
    assert set(np.sign(r.scene.dists[bad[:4]]).tolist()) >= {1.0, -1.0, 0.0}


def test_grid_restatement_is_grid_sample_and_carries_the_edges():
    """grid_restate against torch's own op in float64 at the finite positions (value and both gradients), a NaN position as the
    clip at 0 with zero position gradient, and the populations of the grid cases."""
    import torch.nn.functional as F
    for C, (H, W) in ((3, (37, 53)), (2, (1, 9)), (1, (9, 1)), (4, (1, 1))):
        img, grid, d_out = R.grid_case(C, H, W)
        r = R.grid_reference(img, grid, d_out)
        fin = np.isfinite(grid).all(1)
        ti, tg = torch.tensor(img.astype(np.float64), requires_grad=True), torch.tensor(grid[fin].astype(np.float64), requires_grad=True)
        o = F.grid_sample(ti[None], tg.view(1, -1, 1, 2), mode="bilinear", padding_mode="border", align_corners=True)[0, :, :, 0].permute(1, 0)
        (o * torch.tensor(d_out[fin].astype(np.float64))).sum().backward()
        assert np.abs(o.detach().numpy() - r.out[fin]).max() <= 1e-12
        okg = ~r.flip[fin]
        assert np.abs(tg.grad.numpy() - r.d_grid[fin])[okg].max() <= 1e-12
        nan = np.isnan(grid)
        assert nan.any() and (r.d_grid[nan] == 0).all()
        i = int(np.nonzero(nan[:, 0] & ~nan[:, 1])[0][0])
        alt = grid.copy(); alt[i, 0] = -1.0
        assert np.array_equal(R.grid_reference(img, alt, d_out).out[i], r.out[i]), "NaN in x: the value of the clip at 0"
        if (H, W) == (37, 53):
            raw = r.raw
            assert (raw[:, 0] < 0).sum() > 50 and (raw[:, 0] > W - 1).sum() > 50 and (raw[:, 1] < 0).sum() > 50 and (raw[:, 1] > H - 1).sum() > 50
            assert (np.abs(grid) == 1).any(1).sum() >= 5 and r.flip.sum() >= 10 and r.flip.sum() <= 0.05 * len(grid)
            assert (d_out == 0).all(1).sum() >= 100


def test_exact_lattice_sums_fit_float32():
    """The exact-lattice case: positions on multiples of 1/16 pixel of a 33 x 17 image, values and upstream gradients k 2^-10.
    Every product g w is a multiple of 2^-18 (weights: multiples of 2^-8), and sum |k| per texel stays below 2^24 in those units,
    so every partial sum in any order is exact in float32 and the result is order independent."""
    img, grid, d_out = R.lattice_case(3)
    raw, pos, _ = R.grid_positions(grid, 33, 17)
    assert np.array_equal(pos * 16, np.round(pos * 16)) and np.array_equal(img * 1024, np.round(img * 1024)) and np.array_equal(d_out * 1024, np.round(d_out * 1024))
    x32 = (grid[:, 0] + np.float32(1)) * np.float32(0.5) * np.float32(32)
    assert np.array_equal(x32.astype(np.float64), np.where(raw[:, 0] > 0, raw[:, 0], raw[:, 0])), "the float32 un-normalisation is exact on the lattice"
    absum = R.dense_scatter(torch.tensor(np.abs(d_out).astype(np.float64)), torch.tensor(pos), 33, 17).numpy()
    assert absum.max() * 2.0 ** 18 < 2.0 ** 24
    r = R.grid_reference(img, grid, d_out)
    assert np.array_equal(r.d_img.astype(np.float32).astype(np.float64), r.d_img), "the float64 sums are float32 numbers"


def test_low_texture_switch_is_on_for_a_variance_that_rounded_below_zero():
    """gs2m_mvs._low_texture, the switch of patch_ncc_roughness: sqrt(-1e-9) is NaN and NaN < 0.01 is False, so without the clamp a
    textureless patch whose float32 variance rounded below zero would switch the gradient NCC OFF."""
    import gs2m_mvs as MV
    rv = torch.tensor([-1e-9, -0.0, 0.0, 9.9e-5, 1.01e-4, 0.3], dtype=torch.float32)
    assert MV._low_texture(rv).tolist() == [True, True, True, True, False, False]
    assert not bool((torch.sqrt(rv[:1]) < 0.01).any()), "what the unclamped expression gives"
