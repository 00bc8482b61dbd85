"""The multi-view geometry kernels of csrc/mvs.hip alone (geo_eval, mv_geo_kernel<false>, mv_geo_kernel<true> with float atomics,
mv_geo_kernel<true, SCATTER_MAX>, mv_geo_scatter_kernel, det_finalize_kernel) against the float64 arbiter of tests/mv_geo_ref.py
(pinned to the reference's own chain by tests/test_mv_geo_ref.py), per element, on scenes with unequal views, partial blocks and
waves, and every edge class of the chain (the populations are asserted on the CPU, from float64 margins, in test_mv_geo_ref.py).

The rule of every comparison: within a conditioning group (regular / stiff, mv_geo_ref.classify) the kernel's largest error
against float64 is at most 3 x the largest error of gs2m_mvs.mv_geo_torch (float32 op by op, CPU) against float64 on the same
inputs, plus a floor of 4 float32 ulps of the group's largest |float64 value|.  The kernel is never bounded by its own output.
Pixels in the flip band (at most 1 % of a scene, asserted on the CPU) are left out of `valid` and of the gradients; noise and
angle are continuous across every decision and are checked for all pixels.

Measured on an MI355X, largest error against float64, kernel / op-by-op (of the group's largest |value|); deterministic mode,
upstream scale 1 -- the float-atomic mode and the scales 1e-11 and 3e7 give the same relative figures:
  general, regular group: noise 1.22e-5 / 1.11e-5 px (of 0.74), angle 9.36e-6 / 9.36e-6 rad (both at the clamp, where float32's
    1 - 1e-6 is 3e-8 off), d_depth 6.6e-6 / 5.6e-6 (of 4.3), d_normal 8.7e-6 / 3.9e-5 (of 5.7), d_depth_n 2.3e-5 / 1.9e-5 (of 8.5),
    d_normal_n 6.9e-5 / 1.1e-4 (of 5.4);
  general, stiff group: noise 1.0e-4 / 1.3e-4 (of 647), d_depth 2.8e-2 / 9.1e-2 (of 1.4e4), d_normal 14 / 156 (of 2.4e8: the
    1 / 1e-8 of the normalisation at a zero-length normal), d_normal_n 395 / 395 (of 1.4e8);
  one wave: angle 4.3e-7 / 2.2e-7, d_depth 4.7e-8 / 3.3e-8 (of 0.12), d_normal 1.6e-6 / 1.0e-6 (of 2.0), d_normal_n 8.7e-7 / 5.0e-7 (of 1.1);
  contention: d_depth 5.5e-6 / 3.2e-6 (of 5.8), d_normal 6.9e-6 / 1.9e-5 (of 5.1), d_depth_n 2.1e-5 / 6.5e-5 (of 26), d_normal_n
    5.3e-5 / 7.2e-5 (of 6.9); fixed-point sums within 0.49 ulp of the exact sum of the kernel's own 3015 float32 contributions per
    texel, the float atomics within 58.5 ulp;
  identity (all stiff: |noise| <= 7e-7 px): noise 3.6e-6 / 9.3e-6 px, angle 1.6e-6 / 1.6e-6, d_normal 8.3e-6 / 1.0e-5 (of 3.6).
"""

import pytest
import torch

import mv_geo_ref as R

pytestmark = pytest.mark.gpu
NAMES = ("d_depth", "d_normal", "d_depth_n", "d_normal_n")
FLOOR = 4 * R.EPS32


def _launch(s, d_noise, d_angle, det=True):
    """One forward + backward of the kernels on scene `s` with the given upstream gradients (CPU tensors) -> noise, angle, valid,
    [d_depth, d_normal, d_depth_n, d_normal_n] on the CPU."""
    import gs2m_mvs as MV
    rc, nc = s.ref.project_camera("cuda"), s.near.project_camera("cuda")
    leaves = [t.cuda().requires_grad_(True) for t in (s.depth, s.normal, s.depth_n, s.normal_n)]
    try:
        MV.set_deterministic(det)
        noise, angle, valid = MV.mv_geo(*leaves, rc, nc, s.occlusion)
        torch.autograd.backward([noise, angle], [d_noise.cuda(), d_angle.cuda()])
    finally:
        MV.set_deterministic(True)
    return noise.detach().cpu(), angle.detach().cpu(), valid.cpu(), [t.grad.cpu() for t in leaves]


def _run(name, det=True, scale=1.0):
    s = R.scene(name)
    return _launch(s, s.d_noise * scale, s.d_angle * scale, det)


def _three_times(label, got, op, truth, exclude, stiff):
    """The 3 x rule, per conditioning group."""
    a, b = R.grouped_errors(got, truth, exclude, stiff), R.grouped_errors(op, truth, exclude, stiff)
    ok = torch.isfinite(truth.reshape(-1))
    assert torch.isfinite(got.reshape(-1)[ok]).all(), f"{label}: not finite where float64 is"
    for grp in ("regular", "stiff"):
        (ea, scale, n, worst), (eb, _, _, _) = a[grp], b[grp]
        print(f"{label:34s} {grp:8s} n={n:5d} kernel {ea:.3e} op-by-op {eb:.3e} scale {scale:.3e}")
        assert ea <= 3 * eb + FLOOR * scale, (label, grp, ea, eb, scale, "worst element", worst)


def _check(name, out, scale=1.0, label=""):
    r = R.reference(name, scale)
    f, op, k = r.f64, r.op, r.k
    noise, angle, valid, grads = out
    n = valid.numel()
    label = f"{name} {label}"
    # forward: valid exactly outside the flip band (whose share is asserted again), noise and angle for ALL pixels
    assert int(k["flip_bwd"].sum()) <= 0.01 * n
    assert torch.equal(valid[~k["flip"]], f.valid[~k["flip"]]), f"{label}: valid differs outside the flip band"
    none = torch.zeros(n, dtype=torch.bool)
    _three_times(f"{label} noise", noise, op.noise, f.noise.detach(), none, k["stiff"])
    _three_times(f"{label} angle", angle, op.angle, f.angle.detach(), none, k["stiff"])
    # backward: per element against float64 autograd; the neighbour's maps against the float64 dense scatter of the float64 contributions
    truth = [f.grads[0], f.grads[1], r.scatter[:1], r.scatter[1:]]
    excl = [k["flip_bwd"], k["flip_bwd"][None].expand(3, -1), r.texel_flip, r.texel_flip[None].expand(3, -1, -1)]
    stiff = [k["stiff"], k["stiff"][None].expand(3, -1), r.texel_stiff, r.texel_stiff[None].expand(3, -1, -1)]
    for nm, g, o, t, e, st in zip(NAMES, grads, op.grads, truth, excl, stiff):
        _three_times(f"{label} {nm}", g, o, t, e, st)
    # exact zeros (upstream: d_noise is 0 on every 5th pixel, d_angle on every 7th)
    gn0, ga0 = r.upstream[0] == 0, r.upstream[1] == 0
    dn, dd = grads[1].reshape(3, -1), grads[0].reshape(-1)
    dead_angle = ga0 | k["clamp binds"]
    assert bool((dn[:, dead_angle] == 0).all()), f"{label}: the reference normal's gradient where d_angle is 0 or the clamp binds"
    assert bool((dd[gn0 & (dead_angle | k["zero reference normal"])] == 0).all()), f"{label}: d_depth where nothing flows"
    return r


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "float_atomics"])
@pytest.mark.parametrize("name", R.SCENES)
def test_forward_and_backward_per_element_against_float64(name, det):
    """Every scene in both scatter modes: `valid` exactly outside the flip band, noise / angle for all pixels, the four gradients per
    element (upstream gradients random, of both signs, not masked by valid), finite wherever float64 is -- depth 0 and points behind
    the neighbour's near limit included -- and exact zeros where nothing flows.  Figures: the module docstring."""
    assert torch.cuda.is_available()
    _check(name, _run(name, det), label="det" if det else "float")


@pytest.mark.parametrize("scale", [1e-11, 3e7])
@pytest.mark.parametrize("name", ["general", "contention"])
def test_error_does_not_depend_on_the_gradient_magnitude(name, scale):
    """Upstream gradients x 1e-11 and x 3e7 (a mean-reduced loss; an unreduced one): the same rule with the float64 and op-by-op
    results OF THAT SCALE -- the fixed-point scale follows the call's largest contribution, so the relative error must not move."""
    assert torch.cuda.is_available()
    _check(name, _run(name, True, scale), scale=scale, label=f"x{scale:g}")


def _masked_run(name, noise_mask, angle_mask, det=True):
    s = R.scene(name)
    return s, _launch(s, s.d_noise * noise_mask, s.d_angle * angle_mask, det)


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "float_atomics"])
def test_exact_zeros_of_the_scattered_gradients(det):
    """What reaches the neighbour's maps is a sum over pixels, so its exact zeros are checked with upstream gradients confined to one
    class: (a) d_angle on the pixels where the clamp binds or the reference normal has zero length, d_noise = 0 -> nothing reaches
    depth, neighbour depth or neighbour normal (dL/dnraw is exactly 0 in both classes), and the reference normal gets exactly 0
    where the clamp binds.  At a zero-length reference normal float64 autograd does NOT give that normal 0: x / (|x| + 1e-8) has the
    derivative 1 / 1e-8 at 0, so the gradient is d_angle x (-n_s) x 1e8 -- the kernel must give that value (bound: the float32 error
    of q, ~1e-4 px, times the normal map's slope, < 0.3 / px).  (b) d_noise alone -> both normal gradients exactly 0."""
    assert torch.cuda.is_available()
    r = R.reference("general")
    k = r.k
    cls = (k["clamp binds"] | k["zero reference normal"]).float()
    s, (_, _, _, g) = _masked_run("general", torch.zeros_like(cls), cls, det)
    assert int(k["clamp binds"].sum()) >= 8 and int(k["zero reference normal"].sum()) >= 8
    assert all(bool((g[i] == 0).all()) for i in (0, 2, 3)), [float(g[i].abs().max()) for i in (0, 2, 3)]
    dn = g[1].reshape(3, -1)
    assert bool((dn[:, ~k["zero reference normal"]] == 0).all())
    f = R.evaluate((s.depth, s.normal, s.depth_n, s.normal_n), s.ref, s.near, s.occlusion, s.d_noise * 0, s.d_angle * cls)
    zr = k["zero reference normal"]
    t = f.grads[1].reshape(3, -1)[:, zr]
    assert t.abs().max().item() > 1e6 and (dn[:, zr].double() - t).abs().max().item() <= 1e-4 * t.abs().max().item()
    s, (_, _, _, g) = _masked_run("general", torch.ones_like(cls), torch.zeros_like(cls), det)
    assert bool((g[1] == 0).all()) and bool((g[3] == 0).all()) and bool((g[0] != 0).any()) and bool((g[2] != 0).any())


def _ulp(x):
    return torch.where(x == 0, torch.zeros_like(x), torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-300))) - 23))


def test_contention_sums_are_one_rounding_of_the_kernels_own_contributions():
    """3015 samples on the same four texels of a 2 x 2 neighbour.  The kernel's own float32 contributions are measured, not
    restated: one backward per pixel with the upstream gradient of that pixel alone (float-atomic mode; a single addition into
    zero is exact), 16 values each.  Their exact sum (float64: 3015 terms of 24 bits) is what the fixed-point path claims to round
    ONCE per texel: |deterministic - exact| <= 1 ulp of the sum + the fixed-point quantum (2^-47 of the largest contribution) per
    sample; and, as in the grid test, err_det <= 1.5 err_float + tiny.  This checks the parked footprint (x0 | y0 << 15 | bx << 30 |
    by << 31), its unpacking, the headroom for 4 x 3015 additions and the integer sums for value."""
    assert torch.cuda.is_available()
    import gs2m_mvs as MV
    import gs2m_native as N
    s = R.scene("contention")
    n, dev = s.ref.W * s.ref.H, torch.device("cuda")
    rc, nc = s.ref.project_camera("cuda"), s.near.project_camera("cuda")
    consts = MV._relative_pose(rc, nc)
    maps = [t.cuda().contiguous() for t in (s.depth, s.normal, s.depth_n, s.normal_n)]
    gn, ga = s.d_noise.cuda(), s.d_angle.cuda()
    one_n, one_a = torch.zeros_like(gn), torch.zeros_like(ga)
    dd, dnm = torch.empty_like(maps[0]), torch.empty_like(maps[1])
    out, own = torch.zeros(16, device=dev), torch.zeros(n, 16, device=dev)
    try:
        MV.set_deterministic(False)
        for i in range(n):
            one_n[i], one_a[i] = gn[i], ga[i]
            out.zero_()
            N.launch("gs2m_mv_geo_backward", dev, s.ref.W, s.ref.H, 2, 2, *[m.data_ptr() for m in maps], *consts, float(s.occlusion),
                     one_n.data_ptr(), one_a.data_ptr(), dd.data_ptr(), dnm.data_ptr(), out[:4].data_ptr(), out[4:].data_ptr())
            own[i] = out
            one_n[i], one_a[i] = 0.0, 0.0
    finally:
        MV.set_deterministic(True)
    own = own.cpu().double()
    assert int((own != 0).any(dim=1).sum()) > 0.7 * n, "most samples reach the four texels"
    exact = own.sum(dim=0)
    det = torch.cat([g.reshape(-1) for g in _run("contention", True)[3][2:]]).double()
    flt = torch.cat([g.reshape(-1) for g in _run("contention", False)[3][2:]]).double()
    quantum = n * 2.0 ** -47 * own.abs().max().item()
    err_det, err_flt = (det - exact).abs(), (flt - exact).abs()
    print("contention: err_det / ulp", (err_det / _ulp(exact)).max().item(), "err_float / ulp", (err_flt / _ulp(exact)).max().item())
    assert bool((err_det <= _ulp(exact) + quantum).all()), (err_det / _ulp(exact)).max().item()
    assert err_det.max().item() <= 1.5 * err_flt.max().item() + 1e-30
    # and against the float64 scatter of the float64 contributions, with the yardstick of float32 contributions: 3 x the op-by-op error
    r = R.reference("contention")
    ref = torch.cat([r.scatter[:1].reshape(-1), r.scatter[1:].reshape(-1)])
    op = torch.cat([g.reshape(-1) for g in r.op.grads[2:]]).double()
    assert (det - ref).abs().max().item() <= 3 * (op - ref).abs().max().item() + FLOOR * ref.abs().max().item()


def test_all_zero_upstream_gradient_then_a_normal_call():
    """maxbits stays 0: both neighbour gradients exactly zero (no shift is derived from an empty maximum that could poison the sums),
    and the next call on the same workspace is right."""
    assert torch.cuda.is_available()
    s = R.scene("general")
    z = torch.zeros_like(s.d_noise)
    _, _, _, g = _launch(s, z, z, True)
    assert all(bool((x == 0).all()) for x in g)
    _check("general", _run("general", True), label="after zero")


def test_workspace_stays_zero_between_calls_of_different_shapes():
    """One stream, in this order: general -> contention -> grid_sample_border backward (4 channels, 9 x 7) -> one wave -> general.  The
    64-bit sums are shared by mv_geo and grid_sample_border and must be all-zero between calls: every result is compared with float64,
    and the second general run equals the first bit for bit (integer sums left over, or a workspace regrown without clearing, show)."""
    assert torch.cuda.is_available()
    import torch.nn.functional as F
    import gs2m_mvs as MV
    assert MV.is_deterministic()
    first = _run("general")
    _check("general", first, label="ws 1")
    _check("contention", _run("contention"), label="ws 2")
    g = torch.Generator().manual_seed(21)
    img = torch.randn(4, 7, 9, generator=g)
    grid = torch.rand(500, 2, generator=g) * 2.4 - 1.2
    G = torch.randn(500, 4, generator=g)
    a = img.cuda().requires_grad_(True)
    (MV.grid_sample_border(a, grid.cuda()) * G.cuda()).sum().backward()
    b = img.double().requires_grad_(True)
    (F.grid_sample(b[None], grid.double().view(1, -1, 1, 2), mode="bilinear", padding_mode="border", align_corners=True)[0, :, :, 0].permute(1, 0) * G.double()).sum().backward()
    assert (a.grad.cpu().double() - b.grad).abs().max().item() <= 4e-6 * b.grad.abs().max().item()   # (the existing grid test's bound)
    _check("one_wave", _run("one_wave"), label="ws 4")
    again = _run("general")
    _check("general", again, label="ws 5")
    for x, y in zip(first[3], again[3]):
        assert torch.equal(x, y)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]) and torch.equal(first[2], again[2])


@pytest.mark.parametrize("name", ["general", "contention"])
def test_deterministic_mode_is_bitwise_reproducible(name):
    """Three runs on the partial-block scene (3015 = 11 x 256 + 199) and on the contention scene: identical bits."""
    assert torch.cuda.is_available()
    a = [_run(name)[3] for _ in range(3)]
    for b in a[1:]:
        for x, y in zip(a[0], b):
            assert torch.equal(x, y)
