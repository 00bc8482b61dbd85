"""patch_ncc_kernel<false / true> and patch_ncc_rough_kernel of csrc/mvs.hip alone, every sample compared with the float64
arbiter of tests/patch_ncc_ref.py (pinned to the reference's own chain by tests/test_patch_ncc_ref.py, which also asserts the
flip-band shares and the edge populations of every scene used here).

The rule: |got - f64| <= K e_i for every sample outside the band of the compared quantity, for the value and each gradient
component, with no exception budget; e_i is the sample's own first-order float32 error scale and K is 3 x the float32
yardstick's worst ratio (patch_ncc_ref.RATIO) -- never derived from the kernel.  The entry points are called through ctypes
with over-allocated, sentinel-filled outputs: nothing beyond N may change.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import patch_ncc_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
PAD = 40


def _carr(a):
    return (C.c_float * len(a))(*[float(x) for x in a])


def _inputs(s, n=None, normals=None, dists=None):
    n = len(s.dists) if n is None else n
    t = lambda a: torch.tensor(np.ascontiguousarray(a[:n]), dtype=torch.float32).cuda()
    return dict(N=n, pixels=t(s.pixels), normals=t(s.normals if normals is None else normals), dists=t(s.dists if dists is None else dists),
                rg=torch.tensor(s.ref_gray).cuda(), ng=torch.tensor(s.near_gray).cuda(), h=s.ref_gray.shape[0], w=s.ref_gray.shape[1],
                consts=(_carr(s.M), _carr(s.b), _carr(s.Kinv)), scale=float(s.ncc_scale), d_ncc=t(s.d_ncc))


def _buf(n, k=1):
    return torch.full((n + PAD, k) if k > 1 else (n + PAD,), SENTINEL, device="cuda")


def _call(name, i, patch, tail, scale=None, w=None, h=None, N=None, null=None):
    """Calls the entry point without raising -> return code.  `null`: name of a pointer argument passed as NULL."""
    import gs2m_native as NV
    ptr = {k: i[k].data_ptr() for k in ("pixels", "normals", "dists", "rg", "ng")}
    consts = list(i["consts"])
    if null in ("M", "b", "Kinv"):
        consts[("M", "b", "Kinv").index(null)] = None
    elif null is not None and null in ptr:
        ptr[null] = None
    fn = getattr(NV.lib(), name)
    rc = fn(i["N"] if N is None else N, ptr["pixels"], ptr["normals"], ptr["dists"], ptr["rg"], ptr["ng"], i["w"] if w is None else w, i["h"] if h is None else h,
            *consts, i["scale"] if scale is None else scale, patch, *tail, NV.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _forward(i, patch):
    out = _buf(i["N"])
    assert _call("gs2m_patch_ncc_forward", i, patch, (out.data_ptr(),)) == 0
    assert bool((out[i["N"]:] == SENTINEL).all()), "forward wrote beyond N"
    return out[:i["N"]].cpu().numpy()


def _backward(i, patch, d_ncc=None):
    dn, dd = _buf(i["N"], 3), _buf(i["N"])
    g = i["d_ncc"] if d_ncc is None else d_ncc
    assert _call("gs2m_patch_ncc_backward", i, patch, (g.data_ptr(), dn.data_ptr(), dd.data_ptr())) == 0
    assert bool((dn[i["N"]:] == SENTINEL).all()) and bool((dd[i["N"]:] == SENTINEL).all()), "backward wrote beyond N"
    return dn[:i["N"]].cpu().numpy(), dd[:i["N"]].cpu().numpy()


def _rough(i, patch):
    a, b, c = _buf(i["N"]), _buf(i["N"]), _buf(i["N"])
    assert _call("gs2m_patch_ncc_roughness", i, patch, (a.data_ptr(), b.data_ptr(), c.data_ptr())) == 0
    assert all(bool((x[i["N"]:] == SENTINEL).all()) for x in (a, b, c)), "roughness wrote beyond N"
    return a[:i["N"]].cpu().numpy(), b[:i["N"]].cpu().numpy(), c[:i["N"]].cpu().numpy()


def _assert_bounds(r, got, n, label):
    worst = R.compare(r, got, n)
    print(label, {k: tuple(round(x, 4) for x in v) for k, v in worst.items()})
    for k, (reg, stiff) in worst.items():
        assert reg <= 1.0 and stiff <= 1.0, (label, k, "worst err / (K e_i): regular, stiff", reg, stiff)
    truth = R.outputs_of(r.t)
    for k, x in got.items():   # finite wherever float64 is
        fin = np.isfinite(truth[k][:n])
        assert np.isfinite(np.asarray(x).reshape(truth[k][:n].shape)[fin]).all(), (label, k)


def _check(name, patch, n=None):
    r = R.reference(name, patch)
    s = r.scene
    i = _inputs(s, n)
    n = i["N"]
    ncc = _forward(i, patch)
    dn, dd = _backward(i, patch)
    _assert_bounds(r, {"ncc": ncc, "d_normals": dn, "d_dists": dd}, n, f"{name} patch {patch} N {n}")
    ok = ~(r.k["flip_mask"] | r.k["nonfinite"])[:n]
    assert np.array_equal((ncc < 0.9)[ok], r.t.mask.numpy()[:n][ok]), "the mask outside its band"
    assert (ncc >= 0).all() and (ncc <= 2).all()
    zero = (s.d_ncc[:n] == 0)
    assert (dn[zero] == 0).all() and (dd[zero] == 0).all(), "upstream gradient 0: gradients exactly 0"
    return r, ncc, dn, dd


@pytest.mark.parametrize("n", R.COUNTS)
@pytest.mark.parametrize("patch", R.PATCHES)
def test_production_every_sample_every_patch_size_and_count(patch, n):
    """Patch 0, 1, 2 (idle lanes), 3 (lane 7 idle), 4 (nine rows: a second trip of the row loop for lane 0), 8 (seventeen rows:
    three trips); N = 1 (one group in a workgroup), 15, 16 (exactly one workgroup), 17 and 1001 (a partial last workgroup: the
    tail clamp and the `live` stores); integer pixels and a few fractional ones (the last forty samples)."""
    assert torch.cuda.is_available()
    _check("production", patch, n)


@pytest.mark.parametrize("name,patch", [(nm, p) for nm, p in R.cases() if nm not in ("production", "degenerate")])
def test_scene(name, patch):
    """half: ncc_scale 2, half-resolution images, full-resolution odd pixels.  borders: reference patches over every side and corner.
    thrown: warped patches partly outside (taps in (-1, 0) and (w-1, w)) and wholly outside: exactly 1.0 and exactly zero
    gradients.  flat: a constant reference patch gives exactly 1.0 and zero gradients, contrast 1e-4 is in the stiff class.
    identity: same camera, same image: perfect correlation against the absolute bound K e_i, gradients exactly 0 (b = 0)."""
    assert torch.cuda.is_available()
    r, ncc, dn, dd = _check(name, patch)
    f = r.f64
    if name == "thrown":
        h, w = r.scene.near_gray.shape
        whole = (~((f.qx > -1) & (f.qx < w) & (f.qy > -1) & (f.qy < h))).all(1)
        pos_clear = np.minimum(np.abs(np.stack([f.qx + 1, f.qx - w, f.qy + 1, f.qy - h])).min(0) - r.e["eq"].max(-1), 1).min(1) > 0
        whole &= pos_clear   # no tap within its float32 position error of the padding limit
        assert whole.sum() >= 30 and (ncc[whole] == 1.0).all() and (dn[whole] == 0).all() and (dd[whole] == 0).all()
    if name == "flat":
        const = r.scene.kind == 0
        assert (ncc[const] == 1.0).all() and (dn[const] == 0).all() and (dd[const] == 0).all()
    if name == "identity":
        assert (dn == 0).all() and (dd == 0).all() and (ncc < 0.01).all()


def test_degenerate_planes_do_not_leak_into_other_samples():
    """d tiny, negative, +0 and -0; n . r = 0; hz through 0 inside the patch.  Where the float64 value / gradient is finite the
    kernel's is finite and within the (stiff) bound, where it is not nothing is asserted; and every OTHER sample of the call is
    bit-equal to a call in which the degenerate samples were replaced by benign ones: nothing leaks through the eight-lane sums."""
    assert torch.cuda.is_available()
    r = R.reference("degenerate", 3)
    s = r.scene
    i = _inputs(s)
    ncc, (dn, dd) = _forward(i, 3), _backward(i, 3)
    _assert_bounds(r, {"ncc": ncc, "d_normals": dn, "d_dists": dd}, i["N"], "degenerate")
    j = _inputs(s, normals=s.benign[0], dists=s.benign[1])
    ncc2, (dn2, dd2) = _forward(j, 3), _backward(j, 3)
    other = np.setdiff1d(np.arange(len(s.dists)), s.bad)
    for a, b in ((ncc, ncc2), (dn, dn2), (dd, dd2)):
        assert np.array_equal(a[other].view(np.uint32), b[other].view(np.uint32))
    assert np.isfinite(ncc2).all() and np.isfinite(dn2).all()


@pytest.mark.parametrize("name,patch", [("production", 0), ("production", 1), ("production", 2), ("production", 3), ("half", 3), ("borders", 3), ("flat", 3),
                                        ("thrown", 3), ("identity", 3)])
def test_roughness_variant_per_sample(name, patch):
    """ncc_gray, ncc_grad (3x3 Sobel magnitudes, zero padded at the patch border) and ref_var per sample; the low-texture switch
    equals the arbiter's outside its band; on constant and near-constant patches ref_var >= 0 and the switch is on."""
    assert torch.cuda.is_available()
    r = R.reference(name, patch)
    i = _inputs(r.scene)
    g, gg, rv = _rough(i, patch)
    _assert_bounds(r, {"ncc": g, "ncc_grad": gg, "ref_var": rv}, i["N"], f"roughness {name} patch {patch}")
    ok = ~(r.k["flip_switch"] | r.k["nonfinite"])
    with np.errstate(invalid="ignore"):
        assert np.array_equal((np.sqrt(rv) < 0.01)[ok], r.t.switch.numpy()[ok])
    if name == "flat":
        flat = r.scene.kind < 2
        print("flat: smallest ref_var", rv[flat].min())
        assert (rv[flat] >= 0).all() and (np.sqrt(rv[flat]) < 0.01).all()


def test_roughness_wrapper_switch_size_check_and_patch_limit():
    """gs2m_mvs.patch_ncc_roughness: the switch is on for constant and near-constant patches (ref_var clamped at 0 before the
    square root), grey images of different sizes are refused as _PatchNCC.forward refuses them, and patch 4 returns
    GS2M_ERR_UNSUPPORTED leaving the outputs untouched."""
    assert torch.cuda.is_available()
    import gs2m_mvs as MV
    r = R.reference("flat", 3)
    s = r.scene
    cam, near = R.project_camera(s.ref, s.ref_gray, "cuda"), R.project_camera(s.near, s.near_gray, "cuda")
    t = lambda a: torch.tensor(a).cuda()
    g, gg, sw = MV.patch_ncc_roughness(t(s.pixels), t(s.normals), t(s.dists), cam, near, 1.0, 3)
    assert bool(sw.reshape(-1)[torch.tensor(s.kind < 2).cuda()].all())
    ok = torch.tensor(~(r.k["flip_switch"] | r.k["nonfinite"]))
    assert torch.equal(sw.reshape(-1).cpu()[ok], r.t.switch[ok])
    small = R.project_camera(s.near, s.near_gray[:-1, :-2].copy(), "cuda")
    with pytest.raises(AssertionError, match="same size"):
        MV.patch_ncc_roughness(t(s.pixels), t(s.normals), t(s.dists), cam, small, 1.0, 3)
    with pytest.raises(AssertionError, match="same size"):
        MV._PatchNCC.apply(t(s.pixels), t(s.normals), t(s.dists), cam.gray_image, small.gray_image, t(s.M), t(s.b), t(s.Kinv), 1.0, 3)
    i = _inputs(s)
    a, b, c = _buf(i["N"]), _buf(i["N"]), _buf(i["N"])
    assert _call("gs2m_patch_ncc_roughness", i, 4, (a.data_ptr(), b.data_ptr(), c.data_ptr())) == -4
    assert all(bool((x == SENTINEL).all()) for x in (a, b, c))


def test_refusals_return_their_code_and_write_nothing():
    """patch -1 and 9, ncc_scale 0, negative and NaN, w or h 0, NULL pointers: GS2M_ERR_INVALID_ARG from all three entry points
    (patch 9 in the roughness variant: GS2M_ERR_UNSUPPORTED, as for every patch above 3), outputs untouched."""
    assert torch.cuda.is_available()
    i = _inputs(R.scene("production"), 17)
    outs = {"gs2m_patch_ncc_forward": lambda: [_buf(17)], "gs2m_patch_ncc_backward": lambda: [_buf(17, 3), _buf(17)],
            "gs2m_patch_ncc_roughness": lambda: [_buf(17), _buf(17), _buf(17)]}
    bad = [dict(patch=-1), dict(patch=9), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(w=0), dict(h=0), dict(N=-1)]
    bad += [dict(null=k) for k in ("pixels", "normals", "dists", "rg", "ng", "M", "b", "Kinv")]
    for name, mk in outs.items():
        for kw in bad:
            o = mk()
            tail = ([i["d_ncc"].data_ptr()] if "backward" in name else []) + [x.data_ptr() for x in o]
            kw = dict(kw)
            patch = kw.pop("patch", 3)
            want = -4 if ("roughness" in name and patch > 3) else -1   # (the roughness variant stages at most 7 x 7: GS2M_ERR_UNSUPPORTED first)
            assert _call(name, i, patch, tail, **kw) == want, (name, kw, patch)
            assert all(bool((x == SENTINEL).all()) for x in o), (name, kw)
        o = mk()   # a NULL output
        tail = ([i["d_ncc"].data_ptr()] if "backward" in name else []) + [None] + [x.data_ptr() for x in o[1:]]
        assert _call(name, i, 3, tail) == -1 and all(bool((x == SENTINEL).all()) for x in o)
    dn, dd = _buf(17, 3), _buf(17)
    assert _call("gs2m_patch_ncc_backward", i, 3, (None, dn.data_ptr(), dd.data_ptr())) == -1 and bool((dn == SENTINEL).all())


def test_autograd_path_equals_the_entry_points():
    """gs2m_mvs._PatchNCC (what multi_view_loss calls) hands the same bits back as the raw entry points."""
    assert torch.cuda.is_available()
    import gs2m_mvs as MV
    s = R.scene("production")
    i = _inputs(s)
    n, d = i["normals"].clone().requires_grad_(True), i["dists"].clone().requires_grad_(True)
    t = lambda a: torch.tensor(a)
    ncc = MV._PatchNCC.apply(i["pixels"], n, d, i["rg"][None], i["ng"][None], t(s.M), t(s.b), t(s.Kinv), 1.0, 3)
    (ncc.reshape(-1) * i["d_ncc"]).sum().backward()
    dn, dd = _backward(i, 3)
    assert np.array_equal(ncc.detach().cpu().numpy().reshape(-1), _forward(i, 3)) and np.array_equal(n.grad.cpu().numpy(), dn) and np.array_equal(d.grad.cpu().numpy(), dd)
