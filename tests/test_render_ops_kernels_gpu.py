"""The ten kernels of csrc/render_ops.hip alone, through the C entry points (include/gs2m_raster.h, include/gs2m_pbr.h), against
the float64 arbiter of tests/render_ops_ref.py (checked without a GPU by tests/test_render_ops_ref.py).  Every output lives in a
canary-filled buffer with guard bytes before, between and after the arrays (`Outs` of test_loss_kernels_gpu.py); the guards and
the arrays a call must not write are checked after every call.  Every element is compared with its own error scale -- the
first-order propagation of one rounding per float32 operation through the reference's formulas, never taken from a kernel --
or bitwise where the output is a copy, a selection or one fixed float32 expression.  Nothing is excepted but the rows of the
flip band, which test_render_ops_ref.py caps at 1 % and keeps clear of every planted case.

Largest err / bound measured on the MI355X (printed by every comparison; the bound is 1):

    kernel / output                 largest   case
    pack_fwd distance               0.6711   P 513, z_depth, no blend_metallic
    pack_fwd normal                 0.3562   P 513, plane distance
    pack_bwd d_xyz                  0.9795   P 255, z_depth
    pack_bwd d_rot                  0.1590   P 513, z_depth
    gbuffer_fwd local_normal        0.8137   17x16
    gbuffer_fwd depth               0.4921   16x18, plane distance
    gbuffer_post_bwd                0.8833   33x17, z_depth, dl and dd given
    gbuffer_maps_bwd                0.9977   35x50, z_depth, no pointer NULL
    sobel_fwd                       0.5371   33x17, general
    sobel_bwd d_depth               0.0131   35x50, general
    sobel_bwd d_alpha               0.4561   35x50, general
    pbr_inputs normals              0.7454   35x50
    pbr_inputs roughness            0.7053   35x50
    pbr_inputs metallic estimate    0.8326   35x50
    activate_fwd scales             0.6476   P 257
    activate_fwd rotations          0.6811   P 513
    activate_fwd opacities .. metallic_a   0.7061   P 513, metallic_a
    activate_bwd scales             0.9799   P 256
    activate_bwd rotations          0.5261   P 255
    activate_bwd opacities .. metallic_a   0.7720   P 513, albedo_a
  The ratios next to 1 belong to outputs that are ONE rounded operation, where the scale is that single rounding: d_xyz with
  z_depth is ddist * V[a][2], d_buffer[1] of gbuffer_maps with z_depth is dd + d_distance, d_scaling is g * y.  The smallest,
  sobel d_depth, is dominated by the scale of the camera-to-world rotation: C_ADJ = 16 roundings per entry are allowed for the
  adjugate inverse and every stencil term carries them three times over, while the kernel's inverse of a rotation is good to
  about one.  Every bitwise comparison (copies, the mask, the border, the clamp and its backward, exp and sigmoid against torch,
  the direct gradients of gbuffer_maps, the second run of the sobel backward) held on every element.

Sensitivity, each edit made once in a scratch copy of csrc/render_ops.hip and run against this file:
    pack_features_bwd without e.sgn             test_pack_features_general_scene (P >= 255), test_pack_features_planted_rows (d_rot)
    pack_features_bwd without - e.q[a] * qdq    test_pack_features_general_scene (every P), test_pack_features_planted_rows (d_rot)
    argmin with <= for the tie                  test_pack_features_planted_rows (the tied rows' normal)
    one + / - swapped in the sobel gather       test_sobel_normal at every size with an interior (d_depth)
    pbr_inputs_bwd with an exclusive clamp edge test_pbr_inputs at every size with the planted albedo edges
    gbuffer_post_bwd without de * rr[j]         test_gbuffer_post_and_maps, plane distance, at every size

Nothing in the kernels of csrc/render_ops.hip had to change; the entry points gs2m_pack_features_forward / _backward now refuse
`rotations` / dL_drotations that are not 16-byte aligned and feature rows that are not 8-byte aligned (GS2M_ERR_UNSUPPORTED), as
gs2m_activate_* already did; the refusal is tested below and no misaligned pointer ever reaches a kernel.
"""
import numpy as np
import pytest
import torch

import render_ops_ref as R
from test_loss_kernels_gpu import CANARY, Outs, assert_bits, dev

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
OK, INVALID, UNSUPPORTED = 0, -1, -4
P_SIZES = [1, 255, 256, 257, 513]
MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]       # (z_depth, blend_metallic)


def _lib():
    import gs2m_native
    return gs2m_native.lib()


def call(name, *args, rc=OK):
    import gs2m_native
    got = getattr(_lib(), name)(*args, gs2m_native.stream_ptr())
    torch.cuda.synchronize()
    assert got == rc, (name, got, "expected", rc)


def ptr(t):
    return None if t is None else t.data_ptr()


_worst = {}


def within(got, ref, what, keep=None):
    """every element of `got` within its own error scale of the float64 value: ref = (value, scale)"""
    val, scale = ref
    got = np.asarray(got, dtype=F64).reshape(val.shape)
    assert np.isfinite(got).all() and np.isfinite(val).all() and np.isfinite(scale).all(), what
    err = np.abs(got - val)
    if keep is not None:
        err, scale = err[keep], scale[keep]
    r = float(np.max(np.where(err == 0, 0.0, err / np.maximum(scale, 1e-300)), initial=0.0))
    key = what.split(":")[0]
    if r >= _worst.get(key, (-1.0, ""))[0]:
        _worst[key] = (r, what)
    print(f"{what}: err / bound {r:.4f}   (largest so far for {key}: {_worst[key][0]:.4f} in {_worst[key][1]})")
    assert r <= 1, (what, r)


# ================================================================ pack_features
def pack_fwd(sc, view, campos, z, bm, rc=OK, n=None, shift=None):
    n = sc["xyz"].shape[0] if n is None else n
    t = {k: dev(sc[k]) for k in ("xyz", "scales", "rot", "albedo", "roughness", "metallic")}
    tv, tc = dev(view), dev(campos)
    o = Outs(features=(10 * max(n, 1) + 4, "f32"))
    a = [ptr(t[k]) for k in ("xyz", "scales", "rot", "albedo", "roughness", "metallic")] + [ptr(tc), ptr(tv)]
    f = o.ptr("features")
    if shift is not None:
        if shift == "features":
            f += 4
        elif isinstance(shift, int):
            a[shift] = None
        else:
            a[2] += 4
    call("gs2m_pack_features_forward", n, *a, z, bm, f, rc=rc)
    assert o.intact(("features",) if rc == OK and n > 0 else ())
    if rc != OK or n <= 0:
        return None
    return o.np("features")[:10 * n].reshape(n, 10)


def pack_bwd(sc, view, campos, z, bm, rc=OK, n=None, shift=None):
    n = sc["xyz"].shape[0] if n is None else n
    t = {k: dev(sc[k]) for k in ("xyz", "scales", "rot", "dF")}
    tv, tc = dev(view), dev(campos)
    m = max(n, 1)
    o = Outs(d_xyz=(3 * m, "f32"), d_rot=(4 * m + 4, "f32"), d_albedo=(3 * m, "f32"), d_roughness=(m, "f32"), d_metallic=(m, "f32"))
    a = [ptr(t["xyz"]), ptr(t["scales"]), ptr(t["rot"]), ptr(tc), ptr(tv)]
    g = ptr(t["dF"])
    outs = [o.ptr(k) for k in ("d_xyz", "d_rot", "d_albedo", "d_roughness", "d_metallic")]
    if shift == "rot":
        a[2] += 4
    elif shift == "dF":
        g += 4                                                   # refused before any launch: never dereferenced
    elif shift == "d_rot":
        outs[1] += 4
    elif isinstance(shift, int):
        if shift < 5:
            a[shift] = None
        elif shift == 5:
            g = None
        else:
            outs[shift - 6] = None
    call("gs2m_pack_features_backward", n, *a, z, bm, g, *outs, rc=rc)
    names = ("d_xyz", "d_rot", "d_albedo", "d_roughness", "d_metallic")
    assert o.intact(names if rc == OK and n > 0 else ())
    if rc != OK or n <= 0:
        return None
    return {k: o.np(k)[:c * n].reshape(n, c) for k, c in zip(names, (3, 4, 3, 1, 1))}


def _check_pack(sc, view, campos, z, bm, tag):
    ref = R.PackRef(sc["xyz"], sc["scales"], sc["rot"], sc["albedo"], sc["roughness"], sc["metallic"], campos, view, z, bm)
    keep = ~ref.band
    f = pack_fwd(sc, view, campos, z, bm)
    assert_bits(f[:, 0], np.ones(ref.P, dtype=F32), "channel 0 is exactly 1")
    assert_bits(f[:, 5:8], sc["albedo"], "albedo copy")
    assert_bits(f[:, 8], sc["roughness"].reshape(-1), "roughness copy")
    assert_bits(f[:, 9], sc["metallic"].reshape(-1) if bm else np.zeros(ref.P, dtype=F32), "metallic copy, or exactly 0 without blend_metallic")
    within(f[:, 1], (ref.features[:, 1], ref.features_scale[:, 1]), f"pack_fwd distance: {tag}", keep)
    within(f[:, 2:5], (ref.features[:, 2:5], ref.features_scale[:, 2:5]), f"pack_fwd normal: {tag}", keep)
    b = pack_bwd(sc, view, campos, z, bm)
    want = ref.backward(sc["dF"])
    within(b["d_xyz"], want["d_xyz"], f"pack_bwd d_xyz: {tag}", keep)
    within(b["d_rot"], want["d_rot"], f"pack_bwd d_rot: {tag}", keep)
    assert_bits(b["d_albedo"], sc["dF"][:, 5:8], "d_albedo")
    assert_bits(b["d_roughness"], sc["dF"][:, 8], "d_roughness")
    assert_bits(b["d_metallic"], sc["dF"][:, 9] if bm else np.zeros(ref.P, dtype=F32), "d_metallic: exactly 0 without blend_metallic")
    return ref, f, b


@pytest.mark.parametrize("z,bm", MODES)
@pytest.mark.parametrize("n", P_SIZES)
def test_pack_features_general_scene(n, z, bm):
    cam = R.general_camera()
    _check_pack(R.pack_scene(n, R.PACK_SEEDS[n]), cam["view"], cam["campos"], z, bm, f"P {n} z {z} bm {bm}")


@pytest.mark.parametrize("z,bm", MODES)
def test_pack_features_planted_rows(z, bm):
    sc = R.pack_planted()
    view, campos = R.identity_camera(R.PLANTED_CAMPOS)
    ref, f, b = _check_pack(sc, view, campos, z, bm, f"planted z {z} bm {bm}")
    assert not ref.band.any()
    for name, i in sc["rows"].items():
        if sc["expect"][name] is None:
            continue
        k, flip, dot = sc["expect"][name]
        want = np.zeros(3)
        want[k] = -1.0 if flip else 1.0
        if name == "dot-0":
            want[k] = -1.0                                       # R = diag(1, -1, -1): column 1 is -e1, and -0 does not flip it
        assert np.array_equal(f[i, 2:5].astype(F64), want), (name, f[i, 2:5], "first minimal index, flip only below zero")
        if not z:
            assert f[i, 1] == abs(dot), name
    if not z:
        for name in ("dot+0", "dot-0"):
            i = sc["rows"][name]
            assert not b["d_xyz"][i].any(), "s = 0: ddist * 0, no gradient to xyz"


# ================================================================ gbuffer_post / gbuffer_maps
def gbuf_fwd(W, H, buf, rays, view, z, rc=OK):
    N = max(W * H, 1) if W > 0 and H > 0 else 1
    tb, tr, tv = dev(buf), dev(rays), dev(view)
    o = Outs(mask=(N, "u8"), ln=(3 * N, "f32"), depth=(N, "f32"))
    call("gs2m_gbuffer_post_forward", W, H, ptr(tb), ptr(tr), ptr(tv), z, o.ptr("mask"), o.ptr("ln"), o.ptr("depth"), rc=rc)
    assert o.intact(("mask", "ln", "depth") if rc == OK else ())
    return o.np("mask"), o.np("ln").reshape(3, N), o.np("depth")


def gbuf_bwd(W, H, buf, rays, view, z, dl, dd, direct=None, rc=OK):
    """direct None: gs2m_gbuffer_post_backward (channels 0 and 5..9 must keep their canaries); else the six upstream gradients
    (alpha, distance, normal, albedo, roughness, metallic; None = NULL) of gs2m_gbuffer_maps_backward (all ten written)"""
    N = W * H
    tb, tr, tv, tl, td = dev(buf), dev(rays), dev(view), dev(dl), dev(dd)
    o = Outs(d=(10 * N, "f32"))
    if direct is None:
        call("gs2m_gbuffer_post_backward", W, H, ptr(tb), ptr(tr), ptr(tv), z, ptr(tl), ptr(td), o.ptr("d"), rc=rc)
    else:
        tg = [dev(g) for g in direct]
        call("gs2m_gbuffer_maps_backward", W, H, ptr(tb), ptr(tr), ptr(tv), z, ptr(tl), ptr(td), *[ptr(g) for g in tg], o.ptr("d"), rc=rc)
    assert o.intact(("d",) if rc == OK else ())
    off, nb, _ = o.off["d"]
    raw = o.buf[off:off + nb].view(10, 4 * N)
    if direct is None and rc == OK:
        assert bool((raw[[0, 5, 6, 7, 8, 9]] == CANARY).all()), "gbuffer_post_backward wrote a channel it does not own"
    return o.np("d").reshape(10, N)


@pytest.mark.parametrize("z", [0, 1])
@pytest.mark.parametrize("H,W", R.PIXEL_SIZES)
def test_gbuffer_post_and_maps(H, W, z):
    cam = R.general_camera(W, H)
    buf, rays, planted = R.gbuffer_scene(H, W, H * 100 + W, cam)
    N = H * W
    rays_k = None if z else rays
    ref = R.GBufRef(buf, rays_k, cam["view"], z)
    tag = f"{H}x{W} z {z}"
    mask, ln, depth = gbuf_fwd(W, H, buf, rays_k, cam["view"], z)
    assert np.array_equal(mask, ref.mask.astype(np.uint8)), "the mask is exact: 0 or 1, off for any zero channel, -0 included"
    within(ln, ref.local_normal, f"gbuffer_fwd local_normal: {tag}")
    within(depth, ref.depth, f"gbuffer_fwd depth: {tag}")
    if z:
        assert_bits(depth, buf.reshape(10, N)[1], "z_depth: the distance channel itself")
    rng = np.random.default_rng(N + z)
    dl, dd = rng.standard_normal((3, N)).astype(F32), rng.standard_normal(N).astype(F32)
    for use_l, use_d in ((1, 1), (1, 0), (0, 1), (0, 0)):
        a, b = dl if use_l else None, dd if use_d else None
        d = gbuf_bwd(W, H, buf, rays_k, cam["view"], z, a, b)
        within(d[1:5], ref.backward(a, b), f"gbuffer_post_bwd: {tag} dl {use_l} dd {use_d}")
    # gbuffer_maps_backward: each of the eight upstream gradients NULL in turn, all NULL, none NULL
    up = [rng.standard_normal((c, N)).astype(F32) for c in (1, 1, 3, 3, 1, 1)]       # alpha, distance, normal, albedo, roughness, metallic
    for null in [None, "all"] + list(range(8)):
        gone = lambda k: null == "all" or null == k
        a, b = None if gone(0) else dl, None if gone(1) else dd
        direct = [None if gone(2 + k) else up[k] for k in range(6)]
        d = gbuf_bwd(W, H, buf, rays_k, cam["view"], z, a, b, direct)
        chan = lambda g, c: np.zeros((c, N), dtype=F32) if g is None else g
        ten = np.concatenate([chan(g, c) for g, c in zip(direct, (1, 1, 3, 3, 1, 1))])
        assert_bits(d[0], ten[0], "d_alpha slice")
        assert_bits(d[5:], ten[5:], "albedo / roughness / metallic slices")
        per_channel = [None, None if direct[1] is None else direct[1][0]] + [None if direct[2] is None else direct[2][c] for c in range(3)]
        within(d[1:5], ref.backward(a, b, per_channel), f"gbuffer_maps_bwd: {tag} null {null}")
    # zero (not NULL) dl and dd: the direct gradients come through bit for bit
    d = gbuf_bwd(W, H, buf, rays_k, cam["view"], z, np.zeros((3, N), dtype=F32), np.zeros(N, dtype=F32), up)
    assert_bits(d, np.concatenate(up), "direct gradients with zero dl and dd")


# ================================================================ sobel_normal
def sobel_fwd(W, H, sc, cam, rc=OK, fx=None, fy=None):
    N = max(W * H, 1) if W > 0 and H > 0 else 1
    t = [dev(sc[k]) for k in ("depth", "alpha", "bg")]
    tv = dev(cam["view"])
    o = Outs(out=(3 * N, "f32"))
    call("gs2m_sobel_normal_forward", W, H, *[ptr(x) for x in t], ptr(tv), cam["fx"] if fx is None else fx, cam["fy"] if fy is None else fy, cam["cx"], cam["cy"],
         o.ptr("out"), rc=rc)
    assert o.intact(("out",) if rc == OK else ())
    return o.np("out")


def sobel_bwd(W, H, sc, cam, rc=OK, fx=None):
    N = max(W * H, 1) if W > 0 and H > 0 else 1
    t = [dev(sc[k]) for k in ("depth", "alpha", "bg")]
    tv, tg = dev(cam["view"]), dev(sc["g"])
    o = Outs(d_depth=(N, "f32"), d_alpha=(N, "f32"))
    call("gs2m_sobel_normal_backward", W, H, *[ptr(x) for x in t], ptr(tv), cam["fx"] if fx is None else fx, cam["fy"], cam["cx"], cam["cy"], ptr(tg),
         o.ptr("d_depth"), o.ptr("d_alpha"), rc=rc)
    assert o.intact(("d_depth", "d_alpha") if rc == OK else ())
    return o.np("d_depth"), o.np("d_alpha")


@pytest.mark.parametrize("kind", ["general", "constant"])
@pytest.mark.parametrize("H,W", R.PIXEL_SIZES)
def test_sobel_normal(H, W, kind):
    """the rotated camera of test_render_ops_gpu.py; the tile edge of the backward (16) on, one before and one after the frame's
    edge; first and last interior rows and columns; W or H below 3: all border"""
    cam = R.general_camera(W, H)
    sc = R.sobel_scene(H, W, H * 100 + W, kind)
    ref = R.SobelRef(sc["depth"], sc["alpha"], sc["bg"], cam["view"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    assert not ref.band.any()
    tag = f"{H}x{W} {kind}"
    out = sobel_fwd(W, H, sc, cam).reshape(3, H, W)
    within(out, ref.out, f"sobel_fwd: {tag}")
    border = ~ref.interior
    assert_bits(out[:, border], ref.border_exact()[:, border], "the border is exactly bg (1 - alpha)")
    dd, da = sobel_bwd(W, H, sc, cam)
    (dv, ds), d_alpha = ref.backward(sc["g"])
    within(dd, (dv, ds), f"sobel_bwd d_depth: {tag}")
    within(da, d_alpha, f"sobel_bwd d_alpha: {tag}")
    if H < 3 or W < 3:
        assert_bits(dd, np.zeros(H * W, dtype=F32), "all border: d_depth is exactly 0")
    dd2, da2 = sobel_bwd(W, H, sc, cam)
    assert_bits(dd2, dd, "the gather form is bitwise reproducible")
    assert_bits(da2, da, "d_alpha, second run")
    if "zero_cross" in sc["planted"]:
        v, u = sc["planted"]["zero_cross"]
        assert not ref.side[v - 1, u - 1] and abs(dd.reshape(H, W)[v, u - 1]) > 1e6, "the 1e-12 branch was taken"


# ================================================================ pbr_inputs
def pbr_fwd(W, H, sc, learnt, alpha=True, rc=OK):
    N = W * H
    t = [dev(sc[k]) for k in ("normal", "albedo", "roughness")]
    ta, tm = dev(sc["alpha"]) if alpha else None, dev(sc["metallic"]) if learnt else None
    o = Outs(normals=(3 * N, "f32"), albedo=(3 * N, "f32"), roughness=(N, "f32"), metallic=(N, "f32"))
    call("gs2m_pbr_inputs_forward", W, H, *[ptr(x) for x in t], ptr(ta), ptr(tm), 0.04, 1.0, *[o.ptr(k) for k in ("normals", "albedo", "roughness", "metallic")], rc=rc)
    names = ("normals", "albedo", "roughness", "metallic")
    assert o.intact(names if rc == OK else ())
    return {k: o.np(k) for k in names}


@pytest.mark.parametrize("learnt", [False, True])
@pytest.mark.parametrize("H,W", R.PIXEL_SIZES)
def test_pbr_inputs(H, W, learnt):
    sc = R.pbr_scene(H, W, H + W)
    N = H * W
    ref = R.PbrRef(sc["normal"], sc["albedo"], sc["roughness"], sc["alpha"], sc["metallic"] if learnt else None, 0.04, 1.0)
    assert not ref.band.any()
    tag = f"{H}x{W} learnt {int(learnt)}"
    for alpha in (True, False) if learnt else (True,):
        got = pbr_fwd(W, H, sc, learnt, alpha)
        within(got["normals"].reshape(N, 3), ref.normals, f"pbr_inputs normals: {tag}")      # pixel-major
        assert_bits(got["normals"].reshape(N, 3)[~ref.nonzero], sc["normal"].T[~ref.nonzero], "a zero normal (or one whose squares underflow) passes as it is")
        assert_bits(got["albedo"], ref.albedo, "albedo: clamp and transposition")
        within(got["roughness"], ref.roughness, f"pbr_inputs roughness: {tag}")
        if learnt:
            assert_bits(got["metallic"], sc["metallic"], "a learnt metallic map is copied")
        else:
            within(got["metallic"], ref.metallic, f"pbr_inputs metallic estimate: {tag}")
    if not learnt:
        pbr_fwd(W, H, sc, False, alpha=False, rc=INVALID)       # neither a metallic map nor an alpha map to estimate it from
    tam, tg = dev(sc["albedo"]), dev(sc["g"])
    o = Outs(d=(3 * N, "f32"))
    call("gs2m_pbr_inputs_backward", W, H, ptr(tam), ptr(tg), o.ptr("d"))
    assert o.intact(("d",))
    assert_bits(o.np("d"), ref.backward_exact(sc["g"]), "clamp backward: passes at the inclusive edges, 0 outside")


# ================================================================ activate
ACT_OUT = ("scales", "rotations", "opacities", "albedo_a", "roughness_a", "metallic_a")


def act_fwd(n, raw, present, rc=OK, shift=False):
    t = [dev(raw[k]) if present[k] else None for k in range(6)]
    o = Outs(**{nm: (raw[k].size + 4, "f32") for k, nm in enumerate(ACT_OUT)})
    a = [ptr(x) for x in t]
    if shift:
        a[1] += 4
    call("gs2m_activate_forward", n, *a, *[o.ptr(nm) for nm in ACT_OUT], rc=rc)
    assert o.intact([nm for k, nm in enumerate(ACT_OUT) if present[k]] if rc == OK and n > 0 else ())
    return [o.np(nm)[:raw[k].size].reshape(raw[k].shape) if present[k] else None for k, nm in enumerate(ACT_OUT)]


def act_bwd(n, raw, y, g, present, rc=OK, shift=False):
    names = ("d_scaling", "d_rotation", "d_opacity", "d_albedo", "d_roughness", "d_metallic")
    tr = dev(raw[1]) if present[1] else None
    ty = [dev(y[k]) if present[k] and k != 1 else None for k in range(6)]
    tg = [dev(g[k]) if present[k] else None for k in range(6)]
    o = Outs(**{nm: (raw[k].size + 4, "f32") for k, nm in enumerate(names)})
    r = ptr(tr)
    if shift:
        r += 4
    call("gs2m_activate_backward", n, r, *[ptr(ty[k]) for k in (0, 2, 3, 4, 5)], *[ptr(x) for x in tg], *[o.ptr(nm) if present[k] else None for k, nm in enumerate(names)], rc=rc)
    assert o.intact([nm for k, nm in enumerate(names) if present[k]] if rc == OK and n > 0 else ())
    return [o.np(nm)[:raw[k].size].reshape(raw[k].shape) if present[k] else None for k, nm in enumerate(names)]


@pytest.mark.parametrize("n", P_SIZES)
def test_activate(n):
    raw, g, planted = R.activate_scene(n, n)
    ref = R.ActivateRef(*raw)
    assert not planted or not ref.band.any()
    fns = [torch.exp, None, torch.sigmoid, torch.sigmoid, torch.sigmoid, torch.sigmoid]
    combos = [[True] * 6] + [[j == k for j in range(6)] for k in range(6)] + [[j != k for j in range(6)] for k in range(6)]
    for ci, present in enumerate(combos):
        y = act_fwd(n, raw, present)
        for k in range(6):
            if not present[k]:
                continue
            if k != 1:
                assert_bits(y[k], fns[k](dev(raw[k])).cpu().numpy(), f"output {k} equals the float32 torch op bit for bit")
            keep = None if k < 2 else raw[k] >= -87.0             # expf(-x) overflows float32 beyond: 1 / inf = 0, as torch gives
            within(y[k], (ref.out[k][0].reshape(raw[k].shape), ref.out[k][1].reshape(raw[k].shape)), f"activate_fwd {ACT_OUT[k]}: P {n} combination {ci}", keep)
        d = act_bwd(n, raw, y, g, present)
        for k in range(6):
            if present[k]:
                bv, bs = ref.backward(k, g[k], y[k])
                within(d[k], (bv.reshape(raw[k].shape), bs.reshape(raw[k].shape)), f"activate_bwd {ACT_OUT[k]}: P {n} combination {ci}")
        if ci == 0 and planted:
            for name, want in (("sig+20", None), ("sig-20", None), ("sig+90", 1.0), ("sig-90", 0.0)):
                i = planted[name]
                for k in (2, 3, 4, 5):
                    assert 0.0 <= y[k][i].min() and y[k][i].max() <= 1.0 and (want is None or (y[k][i] == want).all()), (name, k)
                    assert np.isfinite(d[k][i]).all() and (want is None or not d[k][i].any()), "a saturated sigmoid passes no gradient"
            assert not y[1][planted["q_zero"]].any() and y[1][planted["q_at_eps"]][1] == 1.0


# ================================================================ refusals: nothing is launched, nothing is written
def test_refusals():
    cam = R.general_camera()
    sc = R.pack_scene(5, 3)
    for z, bm in MODES[:2]:
        for k in range(8):
            pack_fwd(sc, cam["view"], cam["campos"], z, bm, rc=INVALID, shift=k)              # each required pointer NULL in turn
        for k in range(11):
            pack_bwd(sc, cam["view"], cam["campos"], z, bm, rc=INVALID, shift=k)
    pack_fwd(sc, cam["view"], cam["campos"], 0, 1, rc=INVALID, n=-1)
    pack_bwd(sc, cam["view"], cam["campos"], 0, 1, rc=INVALID, n=-1)
    pack_fwd(sc, cam["view"], cam["campos"], 0, 1, n=0)                                        # P = 0: OK, nothing written
    pack_bwd(sc, cam["view"], cam["campos"], 0, 1, n=0)
    # alignment: refused before any launch
    pack_fwd(sc, cam["view"], cam["campos"], 0, 1, rc=UNSUPPORTED, shift="rot")
    pack_fwd(sc, cam["view"], cam["campos"], 0, 1, rc=UNSUPPORTED, shift="features")
    for s in ("rot", "dF", "d_rot"):
        pack_bwd(sc, cam["view"], cam["campos"], 0, 1, rc=UNSUPPORTED, shift=s)
    raw, g, _ = R.activate_scene(5, 1)
    act_fwd(5, raw, [True] * 6, rc=UNSUPPORTED, shift=True)
    act_bwd(5, raw, raw, g, [True] * 6, rc=UNSUPPORTED, shift=True)
    act_fwd(0, raw, [True] * 6)
    act_bwd(0, raw, raw, g, [True] * 6)
    act_fwd(-1, raw, [True] * 6, rc=INVALID)
    act_bwd(-1, raw, raw, g, [True] * 6, rc=INVALID)
    # frames
    H, W = 4, 5
    camp = R.general_camera(W, H)
    buf, rays, _ = R.gbuffer_scene(H, W, 1, camp)
    for w, h in ((0, H), (W, 0), (-1, H), (W, -3)):
        gbuf_fwd(w, h, buf, rays, camp["view"], 0, rc=INVALID)
    gbuf_fwd(W, H, buf, None, camp["view"], 0, rc=INVALID)                                     # rays are required without z_depth
    gbuf_fwd(W, H, None, rays, camp["view"], 0, rc=INVALID)
    gbuf_fwd(W, H, buf, rays, None, 0, rc=INVALID)
    dl, dd = np.ones((3, H * W), dtype=F32), np.ones(H * W, dtype=F32)
    for direct in (None, [None] * 6):
        gbuf_bwd(W, H, buf, None, camp["view"], 0, dl, dd, direct, rc=INVALID)
        gbuf_bwd(W, H, None, rays, camp["view"], 0, dl, dd, direct, rc=INVALID)
        gbuf_bwd(W, H, buf, rays, None, 1, dl, dd, direct, rc=INVALID)
    ss = R.sobel_scene(H, W, 2)
    sobel_fwd(W, H, ss, camp, rc=INVALID, fx=0.0)
    sobel_fwd(W, H, ss, camp, rc=INVALID, fy=0.0)
    sobel_bwd(W, H, ss, camp, rc=INVALID, fx=0.0)
    sobel_fwd(0, H, ss, camp, rc=INVALID)
    sobel_bwd(W, -1, ss, camp, rc=INVALID)
    for k in ("depth", "alpha", "bg"):
        sobel_fwd(W, H, {**ss, k: None}, camp, rc=INVALID)
        sobel_bwd(W, H, {**ss, k: None}, camp, rc=INVALID)
    sobel_bwd(W, H, {**ss, "g": None}, camp, rc=INVALID)
    ps = R.pbr_scene(H, W, 3)
    for k in ("normal", "albedo", "roughness"):
        pbr_fwd(W, H, {**ps, k: None}, True, rc=INVALID)
