"""tests/render_ops_ref.py checked without a GPU, before tests/test_render_ops_kernels_gpu.py holds the kernels of
csrc/render_ops.hip to it: the float64 arbiter against this project's float32 PyTorch formulation on the CPU (values and
gradients, to float32 accuracy), its hand-written backward passes against float64 autograd and against central differences,
every planted decision on its intended side with a margin of exactly 0 or exactly the planted value, and the flip band of the
general scenes: at most 1 % of the elements, no planted case in it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import render_ops_ref as R

F32, F64 = np.float32, np.float64


def _t32(x, grad=False):
    return torch.tensor(np.asarray(x, dtype=F32), requires_grad=grad)


def _rel(a, b, floor=1.0):
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    return float(np.abs(a - b).max(initial=0.0)) / max(floor, float(np.abs(b).max(initial=0.0)))


def _pack(sc, cam, z_depth, blend):
    return R.PackRef(sc["xyz"], sc["scales"], sc["rot"], sc["albedo"], sc["roughness"], sc["metallic"], cam["campos"], cam["view"], z_depth, blend)


def _torch_features(xyz, scales, rot, albedo, roughness, metallic, campos, view, z_depth, blend):
    """_torch_features of tests/test_render_ops_gpu.py on plain tensors (get_normals: gs2m_scene.GaussianParams)"""
    import gs2m_scene
    k = torch.argmin(scales, dim=-1, keepdim=True)
    normals = torch.bmm(gs2m_scene.build_rotation(rot), torch.zeros_like(scales).scatter(1, k, 1).unsqueeze(-1)).squeeze(-1)
    flip = torch.sum(normals * (campos[None] - xyz), dim=-1) < 0.0
    normals = torch.where(flip[:, None], -normals, normals)
    normals = normals / normals.norm(dim=1, keepdim=True)
    cn = normals @ view[:3, :3]
    cp = xyz @ view[:3, :3] + view[3, :3]
    f = torch.zeros((xyz.shape[0], 10), dtype=xyz.dtype)
    f[:, 0] = 1.0
    f[:, 1] = cp[:, 2] if z_depth else (cn * cp).sum(dim=-1).abs()
    f[:, 2:5] = normals
    f[:, 5:8] = albedo
    f[:, 8:9] = roughness
    if blend:
        f[:, 9:10] = metallic
    return f


@pytest.mark.parametrize("P", [257, 513])
@pytest.mark.parametrize("z_depth,blend", [(False, False), (True, True)])
def test_pack_features_arbiter(P, z_depth, blend):
    cam = R.general_camera()
    sc = R.pack_scene(P, R.PACK_SEEDS[P])
    ref = _pack(sc, cam, z_depth, blend)
    keep = ~ref.band
    # against the float32 PyTorch formulation
    ts = [_t32(sc[n], True) for n in ("xyz", "scales", "rot", "albedo", "roughness", "metallic")]
    f32 = _torch_features(*ts, _t32(cam["campos"]), _t32(cam["view"]), z_depth, blend)
    (f32 * _t32(sc["dF"])).sum().backward()
    assert _rel(f32.detach().numpy()[keep], ref.features[keep]) < 2e-6
    b = ref.backward(sc["dF"])
    assert _rel(ts[0].grad.numpy()[keep], b["d_xyz"][0][keep]) < 2e-5 and _rel(ts[2].grad.numpy()[keep], b["d_rot"][0][keep]) < 2e-5
    # the written-out backward against float64 autograd; autograd against central differences
    gx, gr = ref.backward_f64(sc["dF"])
    assert _rel(b["d_xyz"][0], gx) < 1e-12 and _rel(b["d_rot"][0], gr) < 1e-11
    dF = R.f64(sc["dF"])[:, 1:5]
    loss = lambda x, r: float((ref.torch_forward(R.t64(x), R.t64(r)) * R.t64(dF)).sum())
    x0, r0 = R.f64(sc["xyz"]), R.f64(sc["rot"])
    for i, j in ((0, 0), (P // 2, 1), (P - 1, 2), (3, 3)):
        h = 1e-6
        rp, rm = r0.copy(), r0.copy()
        rp[i, j] += h; rm[i, j] -= h
        assert abs((loss(x0, rp) - loss(x0, rm)) / (2 * h) - gr[i, j]) <= 1e-6 * max(1.0, abs(gr[i, j]))
        if j < 3:
            xp, xm = x0.copy(), x0.copy()
            xp[i, j] += h; xm[i, j] -= h
            assert abs((loss(xp, r0) - loss(xm, r0)) / (2 * h) - gx[i, j]) <= 1e-6 * max(1.0, abs(gx[i, j]))
    # error scales: positive where something is computed, zero on the copies
    assert (ref.features_scale[:, [0, 5, 6, 7, 8, 9]] == 0).all() and (ref.features_scale[:, 2:5] > 0).all()
    assert (ref.features_scale[:, 2:5] < 64 * R.U).all(), "a unit normal carries a few dozen roundings at most"


@pytest.mark.parametrize("P", sorted(R.PACK_SEEDS))
def test_pack_features_flip_band_is_small(P):
    ref = _pack(R.pack_scene(P, R.PACK_SEEDS[P]), R.general_camera(), False, True)
    assert int(ref.band.sum()) <= 0.01 * P, (P, int(ref.band.sum()))
    assert 0 < ref.flip.sum() < P or P == 1, "both sides of the flip occur"


def test_pack_features_planted_rows():
    sc = R.pack_planted()
    view, campos = R.identity_camera(R.PLANTED_CAMPOS)
    ref = _pack(sc, dict(view=view, campos=campos), False, True)
    assert not ref.band.any(), "no planted row lies in the flip band"
    for name, i in sc["rows"].items():
        exp = sc["expect"][name]
        if exp is None:
            continue
        k, flip, dot = exp
        assert ref.k[i] == k and bool(ref.flip[i]) == flip and ref.dot[i] == dot and ref.s[i] == -abs(dot), name     # s = n . (p - c): the flipped normal faces the camera
    # exact in float32 as well: the same dot from the float32 operations, bit for bit, its sign of zero included
    x, r = sc["xyz"], sc["rot"]
    i = sc["rows"]["dot-0"]
    m = np.array([F32(2) * (r[i, 1] * r[i, 2] - r[i, 0] * r[i, 3]), F32(1) - F32(2) * (r[i, 1] * r[i, 1] + r[i, 3] * r[i, 3]), F32(2) * (r[i, 2] * r[i, 3] + r[i, 0] * r[i, 1])], dtype=F32)
    v = campos - x[i]
    d = m[0] * v[0] + m[1] * v[1] + m[2] * v[2]
    assert d == 0 and np.signbit(d) and not d < 0, "-0: not flipped"
    i = sc["rows"]["dot+0"]
    v = campos - x[i]
    d = F32(1) * v[0] + F32(0) * v[1] + F32(0) * v[2]
    assert d == 0 and not np.signbit(d)
    # s = 0: no gradient through |s|
    b = ref.backward(sc["dF"])
    for name in ("dot+0", "dot-0"):
        assert not b["d_xyz"][0][sc["rows"][name]].any()
    # the two sides of the flip mirror each other
    f, bk = sc["rows"]["front"], sc["rows"]["back"]
    assert ref.features[f, 2] == 1.0 and ref.features[bk, 2] == -1.0 and ref.features[f, 1] == ref.features[bk, 1] == 0.5
    # a quaternion of norm 1e-3 / 1e3: the same normal as the unit one, the gradient scaled by 1 / norm
    gx, gr = ref.backward_f64(sc["dF"])
    assert _rel(b["d_rot"][0], gr, floor=1e-30) < 1e-9 and np.abs(gr[sc["rows"]["qn1e-3"]]).max() > 100 * np.abs(gr[sc["rows"]["qn1e3"]]).max()
    for name in ("qn1e-3", "qn1e3"):
        i = sc["rows"][name]
        assert abs(np.dot(gr[i], R.f64(sc["rot"][i]))) <= 1e-12 * np.abs(gr[i]).max() * np.abs(sc["rot"][i]).max() * 4, "the gradient is orthogonal to the quaternion"


def _torch_post(b, rays, view, H, W, z_depth):
    """torch_post of tests/test_render_ops_gpu.py"""
    normal_map = b[2:5]
    mask = (normal_map != 0).all(0, keepdim=True)
    ln = normal_map.permute(1, 2, 0).reshape(-1, 3) @ view[:3, :3]
    depth = b[1:2]
    if not z_depth:
        depth = b[1:2] / -(torch.sum(ln * rays, dim=-1).view(1, H, W) + 1e-8)
    return mask, ln.reshape(H, W, 3).permute(2, 0, 1), depth


@pytest.mark.parametrize("z_depth", [False, True])
@pytest.mark.parametrize("H,W", [(2, 5), (17, 16), (35, 50)])
def test_gbuffer_arbiter(H, W, z_depth):
    cam = R.general_camera(W, H)
    buf, rays, planted = R.gbuffer_scene(H, W, H * 100 + W, cam)
    ref = R.GBufRef(buf, None if z_depth else rays, cam["view"], z_depth)
    rng = np.random.default_rng(1)
    dl, dd = rng.standard_normal((3, H * W)).astype(F32), rng.standard_normal(H * W).astype(F32)
    b = _t32(buf, True)
    m, l, d = _torch_post(b, _t32(rays), _t32(cam["view"]), H, W, z_depth)
    ((l * _t32(dl).view(3, H, W)).sum() + (d * _t32(dd).view(1, H, W)).sum()).backward()
    assert np.array_equal(m.numpy().reshape(-1), ref.mask)
    for name in ("one_zero", "minus_zero", "all_zero", "two_zero"):
        assert not ref.mask[planted[name]]
    assert ref.mask[planted["small_denom"]] and ref.mask[6:].all()
    sd = planted["small_denom"]
    if not z_depth:
        assert 2.0 ** -11 < abs(ref.e.v[sd]) < 2.0 ** -8 and ref.depth[1][sd] > 100 * np.median(ref.depth[1]), "stiff: compared on its own scale"
    keep = np.ones(H * W, dtype=bool)
    keep[sd] = False                                             # the float32 yardstick is useless there; the scale is not
    assert _rel(l.detach().numpy().reshape(3, -1), ref.local_normal[0]) < 1e-6 and _rel(d.detach().numpy().reshape(-1)[keep], ref.depth[0][keep]) < 1e-4
    gv, gs = ref.backward(dl, dd)
    g64 = ref.backward_f64(dl.reshape(3, -1), dd)
    assert _rel(gv, g64[1:5], floor=1e-30) < 1e-12
    assert not g64[0].any() and not g64[5:].any()
    g32 = b.grad.numpy().reshape(10, -1)
    assert _rel(g32[1:5][:, keep], gv[:, keep]) < 1e-3
    err = np.abs(g32[1:5] - gv)
    assert (err <= 64 * gs + 1e-30).all(), "the float32 autograd result lies within a few dozen error scales, the stiff pixel included"
    # one zero channel changes the mask only: the local normal and its gradient are those of the other two channels
    oz = planted["one_zero"]
    want = R.f64(buf.reshape(10, -1)[2:5, oz]) @ R.f64(cam["view"])[:3, :3]
    assert np.abs(ref.local_normal[0][:, oz] - want).max() < 1e-15
    # central differences on a handful of elements
    bb = R.f64(buf).reshape(10, -1)
    def loss(x, p):                                              # pixels are independent: pixel p's share of the loss
        ln, dep, _ = R._gbuf_chain(R._Torch, R.t64(x[1]), [R.t64(x[2]), R.t64(x[3]), R.t64(x[4])], None if z_depth else [R.t64(rays[:, j]) for j in range(3)], cam["view"], z_depth)
        return float((torch.stack(ln) * R.t64(dl))[:, p].sum() + (dep * R.t64(dd))[p])
    for c, p in ((1, 0), (2, 7), (3, H * W - 1), (4, 8)):
        h = 1e-6
        xp, xm = bb.copy(), bb.copy()
        xp[c, p] += h; xm[c, p] -= h
        assert abs((loss(xp, p) - loss(xm, p)) / (2 * h) - g64[c, p]) <= 1e-5 * max(1.0, abs(g64[c, p]))


@pytest.mark.parametrize("H,W", R.PIXEL_SIZES)
def test_sobel_arbiter(H, W):
    import gs2m_scene
    cam = R.general_camera(W, H)
    sc = R.sobel_scene(H, W, H * 100 + W)
    k = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    ref = R.SobelRef(sc["depth"], sc["alpha"], sc["bg"], cam["view"], *k)
    assert not ref.band.any(), "no norm near 1e-12 in the general scene, and the planted zero is decided"
    # the cancelled form equals the reference's formulation in float64
    out64 = R.sobel_f64(R.t64(sc["depth"]), R.t64(sc["alpha"]), R.f64(sc["bg"]), cam["view"], *ref.k).numpy()
    assert _rel(ref.out[0], out64) < 1e-12
    gd, ga = ref.backward_f64(sc["g"])
    (dv, ds), (av, as_) = ref.backward(sc["g"])
    assert _rel(dv, gd, floor=1e-30) < 1e-9 and _rel(av, ga) < 1e-12
    if H < 3 or W < 3:
        assert not dv.any() and not ds.any() and not gd.any()
        return
    if "zero_cross" in sc["planted"]:
        v, u = sc["planted"]["zero_cross"]
        assert ref.len.v[v - 1, u - 1] == 0 and not ref.side[v - 1, u - 1] and ref.margin[v - 1, u - 1] == -R.EPS
        assert not out64[:, v, u].any() or sc["alpha"][v, u] != 1
        assert np.abs(gd[v, u - 1]) > 1e6, "the 1e-12 branch: the gradient of the neighbours is g alpha / 1e-12"
    # against the float32 PyTorch formulation (gs2m_scene.normal_from_depth_image), away from the planted zero
    d32, a32 = _t32(sc["depth"], True), _t32(sc["alpha"], True)
    K = torch.tensor([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1]]).float()
    nrm = gs2m_scene.normal_from_depth_image(d32, K, _t32(cam["view"]).t().contiguous())
    out32 = (nrm * a32[..., None] + _t32(sc["bg"])[None, None] * (1 - a32[..., None])).permute(2, 0, 1)
    keep = np.ones((H, W), dtype=bool)
    if "zero_cross" in sc["planted"]:
        keep[1:4, 0:5] = False
    assert _rel(out32.detach().numpy()[:, keep], ref.out[0][:, keep]) < 1e-4
    (out32 * _t32(sc["g"])).sum().backward()
    assert _rel(a32.grad.numpy()[keep], av[keep]) < 1e-4
    far = keep.copy()
    if "zero_cross" in sc["planted"]:
        far[0:5, 0:6] = False
    assert _rel(d32.grad.numpy()[far], dv[far]) < 2e-3
    # central differences through the reference's formulation
    loss = lambda d, a: float((R.sobel_f64(R.t64(d), R.t64(a), R.f64(sc["bg"]), cam["view"], *ref.k) * R.t64(sc["g"])).sum())
    d0, a0 = R.f64(sc["depth"]), R.f64(sc["alpha"])
    for v, u in ((0, 0), (H - 1, W - 1), (1, 1), (H // 2, W - 2), (H - 2, W // 2)):
        if not far[v, u]:
            continue
        h = 1e-6
        dp, dm = d0.copy(), d0.copy()
        dp[v, u] += h; dm[v, u] -= h
        assert abs((loss(dp, a0) - loss(dm, a0)) / (2 * h) - gd[v, u]) <= 1e-5 * max(1.0, abs(gd[v, u]))
        ap, am = a0.copy(), a0.copy()
        ap[v, u] += h; am[v, u] -= h
        assert abs((loss(d0, ap) - loss(d0, am)) / (2 * h) - ga[v, u]) <= 1e-6 * max(1.0, abs(ga[v, u]))


def test_sobel_adjugate_matches_inverse():
    """the camera-to-world rotation: the inverse the arbiter takes equals the transpose (a rotation) to float32 accuracy"""
    cam = R.general_camera()
    A = R.f64(cam["view"])[:3, :3].T
    assert np.abs(np.linalg.inv(A) - A.T).max() < 4 * R.U and abs(np.linalg.det(A) - 1) < 8 * R.U
    assert np.abs(A - np.eye(3)).max() > 0.1, "rotated, not axis-aligned"


@pytest.mark.parametrize("H,W", [(2, 5), (16, 18), (35, 50)])
@pytest.mark.parametrize("learnt", [False, True])
def test_pbr_inputs_arbiter(H, W, learnt):
    sc = R.pbr_scene(H, W, H + W)
    ref = R.PbrRef(sc["normal"], sc["albedo"], sc["roughness"], sc["alpha"], sc["metallic"] if learnt else None, 0.04, 1.0)
    # the unfused preparation of pbr_render (pbr/__init__.py) in float32
    nm = _t32(sc["normal"]).view(3, H, W)
    nm = torch.where(torch.norm(nm, dim=0, keepdim=True) > 0, F.normalize(nm, dim=0, p=2), nm)
    am = _t32(sc["albedo"], True)
    alb = am.view(3, H, W).clamp(0, 1)
    ro = _t32(sc["roughness"]).view(1, H, W)
    met = _t32(sc["metallic"]).view(1, H, W) if learnt else _t32(sc["alpha"]).view(1, H, W) * (1.0 - ro).clamp(0, 1)
    rough = ro * (1.0 - 0.04) + 0.04
    assert not ref.band.any()
    assert _rel(nm.permute(1, 2, 0).reshape(-1, 3).numpy(), ref.normals[0]) < 2e-6
    assert np.array_equal(alb.detach().permute(1, 2, 0).reshape(-1, 3).numpy(), ref.albedo)
    assert _rel(rough.reshape(-1).numpy(), ref.roughness[0]) < 2e-7
    if learnt:
        assert np.array_equal(met.reshape(-1).numpy(), ref.metallic_exact)
    else:
        assert _rel(met.reshape(-1).numpy(), ref.metallic[0]) < 2e-7 and ref.metallic[0].min() == 0 and (ref.metallic[0] <= sc["alpha"]).all()
    (alb.permute(1, 2, 0).reshape(-1, 3) * _t32(sc["g"])).sum().backward()
    assert np.array_equal(am.grad.numpy(), ref.backward_exact(sc["g"]))
    p = sc["planted"]
    N = ref.normals[0]
    assert not N[p["zero_normal"]].any() and not ref.nonzero[p["zero_normal"]]
    assert not ref.nonzero[p["underflow"]] and np.array_equal(N[p["underflow"]], R.f64(sc["normal"][:, p["underflow"]])), "squares underflow: passes as it is"
    assert ref.nonzero[p["below_eps"]] and not ref.side[p["below_eps"]] and abs(np.linalg.norm(N[p["below_eps"]]) - 0.5) < 1e-6
    assert ref.side[p["at_eps"]] and ref.margin[p["at_eps"]] == 0 and N[p["at_eps"], 0] == 1.0
    g = ref.backward_exact(sc["g"])
    assert np.array_equal(g[:, p["albedo_edges"]], sc["g"][p["albedo_edges"]]) and not g[:, p["albedo_outside"]].any(), "inclusive edges, 0 outside"


@pytest.mark.parametrize("P", [1, 255, 257])
def test_activate_arbiter(P):
    raw, g, planted = R.activate_scene(P, P)
    ref = R.ActivateRef(*raw)
    fns = [torch.exp, F.normalize, torch.sigmoid, torch.sigmoid, torch.sigmoid, torch.sigmoid]
    for k in range(6):
        x = _t32(raw[k], True)
        y = fns[k](x)
        (y * _t32(g[k])).sum().backward()
        y32 = y.detach().numpy()
        assert _rel(y32, ref.out[k][0].reshape(y32.shape)) < 1e-6
        bv, bs = ref.backward(k, g[k], y32)
        g64 = ref.backward_f64(k, g[k])
        scale = max(1.0, float(np.abs(g64).max()))
        assert np.abs(x.grad.numpy() - bv).max() <= 2e-6 * scale
        assert np.abs(bv - g64).max() <= (1e-11 if k == 1 else 1e-6) * scale, "from the saved float32 activation: float32 accuracy for exp / sigmoid"
        xs = R.f64(raw[k])
        for i in ((0, 0), (P - 1, xs.shape[1] - 1)):
            if k == 1 and planted and i[0] in (planted["q_zero"], planted["q_below"], planted["q_at_eps"], planted["q_large"]):
                continue
            if k >= 2 and planted and i[0] < len(R.ACT_PLANTED):
                continue
            h = 1e-6
            xp, xm = xs.copy(), xs.copy()
            xp[i] += h; xm[i] -= h
            f = lambda a: float((ref.forward_f64(k, R.t64(a)) * R.t64(g[k])).sum())
            assert abs((f(xp) - f(xm)) / (2 * h) - g64[i]) <= 1e-5 * max(1.0, abs(g64[i]))
    if planted:
        assert not ref.band.any()
        z, b, e, L = (planted[n] for n in ("q_zero", "q_below", "q_at_eps", "q_large"))
        assert ref.zero[z] and not ref.side[z] and not ref.side[b] and ref.side[e] and ref.margin[e] == 0 and ref.side[L]
        assert not ref.out[1][0][z].any() and abs(np.linalg.norm(ref.out[1][0][b]) - 0.5) < 1e-6 and ref.out[1][0][e][1] == 1.0
        d = ref.backward(1, g[1])[0]
        assert np.allclose(d[z], R.f64(g[1][z]) / R.EPS) and np.allclose(d[b], R.f64(g[1][b]) / R.EPS), "below the clamp: g / eps"
        assert abs(d[e][1]) <= 1e-3 * np.abs(d[e]).max(), "at the clamp's edge the norm's gradient passes: the radial part is projected out"
