"""The per-vertex bake and the PBR mesh views on the GPU (csrc/mesh_bake.hip, csrc/mesh_view.hip) against the fp64 restatement of
tests/mesh_bake_ref.py: sums and weights, the bitwise identities, argument handling, the G-buffer and the RGB resolve, a round trip
G-buffer -> bake, shade_views_pbr against the unfused shading, and the two command lines.  All data is synthetic."""
import os

import numpy as np
import pytest
import torch

import gs2m_mesh_bake as MB
import gs2m_mesh_cull as K
import gs2m_mesh_view as MVW
import gs2m_native as N
import mesh_bake_ref as B
import mesh_view_ref as MV

pytestmark = pytest.mark.gpu

INVALID = "invalid argument"


def _cuda(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def _accumulate(c, views, channels, sums=None, weights=None, masked=True, with_normals=True, n_verts=None):
    """one call of gs2m_meshbake_accumulate on views[a:b] of the case -> (sums, weights) device tensors"""
    a, b = views
    V = len(c["verts"]) if n_verts is None else n_verts
    v, nrm, m = _cuda(c["verts"][:V]), _cuda(c["normals"][:V]), _cuda(c["w2c"][a:b])
    depth, maps, mask = _cuda(c["depth"][a:b]), _cuda(c["maps"][a:b, :channels]), _cuda(c["mask"][a:b])
    acc = 0 if sums is None else 1
    sums = torch.full((V, channels), 7.0, dtype=torch.float64, device="cuda") if sums is None else sums.clone()
    weights = torch.full((V,), 7.0, dtype=torch.float64, device="cuda") if weights is None else weights.clone()
    N.launch("gs2m_meshbake_accumulate", v.device, V, N.ptr(v), N.ptr(nrm) if with_normals else None, b - a, N.ptr(m), c["fx"], c["fy"], c["cx"],
             c["cy"], c["W"], c["H"], N.ptr(depth), channels, N.ptr(maps), N.ptr(mask) if masked else None, c["eps"], acc, N.ptr(sums), N.ptr(weights))
    torch.cuda.synchronize()
    return sums, weights


def _close(got, want, rel):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= rel * np.abs(want)))


@pytest.mark.parametrize("channels,masked,with_normals", [(5, True, True), (1, True, True), (5, False, True), (5, True, False)])
def test_sums_and_weights_against_the_restatement(channels, masked, with_normals):
    c = B.bake_case()
    want_s, want_w, use, _ = B.bake_reference(channels, masked, with_normals)
    s, w = _accumulate(c, (0, 3), channels, masked=masked, with_normals=with_normals)
    s, w = s.cpu().numpy(), w.cpu().numpy()
    assert np.array_equal(w > 0, want_w > 0)
    assert _close(w, want_w, 1e-12) and _close(s, want_s, 1e-12)
    # the contributing (vertex, view) pairs: each view alone
    for k in range(3):
        _, wk = _accumulate(c, (k, k + 1), channels, masked=masked, with_normals=with_normals)
        assert np.array_equal(wk.cpu().numpy() > 0, use[:, k]), k
    # resolve: seen and the values
    fb = [0.25 + 0.1 * k for k in range(channels)]
    out, seen, _ = _resolve(torch.as_tensor(want_s).cuda(), torch.as_tensor(want_w).cuda(), 0.3, fb)
    want_out, want_seen = B.resolve(want_s, want_w, 0.3, fb)
    assert np.array_equal(seen.cpu().numpy(), want_seen) and want_seen.any() and not want_seen.all()
    assert np.array_equal(out.cpu().numpy()[~want_seen], want_out[~want_seen])
    assert np.abs(out.cpu().numpy()[want_seen] - want_out[want_seen]).max() <= 1.2e-7  # one rounding to fp32 of a value in [0, 1]


def _resolve(sums, weights, min_weight, fallback):
    import ctypes as C
    V, ch = sums.shape
    out = torch.empty((V, ch), dtype=torch.float32, device="cuda")
    seen = torch.empty(V, dtype=torch.uint8, device="cuda")
    N.launch("gs2m_meshbake_resolve", sums.device, V, ch, N.ptr(sums), N.ptr(weights), float(min_weight), (C.c_float * ch)(*fallback), N.ptr(out),
             N.ptr(seen))
    return out, seen.bool(), weights


def test_bitwise_identities():
    c = B.bake_case()
    s, w = _accumulate(c, (0, 3), 5)
    s2, w2 = _accumulate(c, (0, 3), 5)
    assert torch.equal(s, s2) and torch.equal(w, w2)  # two runs
    for k in (1, 2):  # the views split over two calls
        sa, wa = _accumulate(c, (0, k), 5)
        sb, wb = _accumulate(c, (k, 3), 5, sa, wa)
        assert torch.equal(s, sb) and torch.equal(w, wb), k
    # through the Python API: the mesh's depth comes from the rasterizer there
    args = (_cuda(c["verts"]), _cuda(c["tris"]), _cuda(c["w2c"]), c["fx"], c["fy"], c["cx"], c["cy"], _cuda(c["maps"]), _cuda(c["mask"]))
    one = MB.bake_vertex_attributes(*args, view_batch=1, min_weight=0.2, fallback=(1, 2, 3, 4, 5))
    three = MB.bake_vertex_attributes(*args, view_batch=3, min_weight=0.2, fallback=(1, 2, 3, 4, 5))
    for a, b in zip(one, three):
        assert torch.equal(a, b)
    assert one[0].dtype == torch.float32 and one[1].dtype == torch.bool and one[2].dtype == torch.float64
    assert one[1].any() and not one[1].all() and (one[0][~one[1]] == torch.tensor([1, 2, 3, 4, 5.0], device="cuda")).all()


def test_argument_handling():
    c = B.bake_case()
    V = len(c["verts"])
    # no view: the buffers are still zeroed; NULL normals; no vertex
    s, w = _accumulate(c, (0, 0), 5)
    assert (s == 0).all() and (w == 0).all()
    s, w = _accumulate(c, (0, 3), 5, with_normals=False)
    assert (w == w.round()).all() and w.max() >= 2  # every view weighs 1
    _accumulate(c, (0, 3), 5, n_verts=0)
    v, m = _cuda(c["verts"]), _cuda(c["w2c"])
    depth, maps = _cuda(c["depth"]), _cuda(c["maps"])
    sums, weights = torch.full((V, 9), 7.0, dtype=torch.float64, device="cuda"), torch.full((V,), 7.0, dtype=torch.float64, device="cuda")

    def call(C=5, W=c["W"], H=c["H"], fx=c["fx"], fy=c["fy"]):
        N.launch("gs2m_meshbake_accumulate", v.device, V, N.ptr(v), None, 3, N.ptr(m), fx, fy, c["cx"], c["cy"], W, H, N.ptr(depth), C, N.ptr(maps),
                 None, c["eps"], 0, N.ptr(sums), N.ptr(weights))

    for bad in (dict(C=0), dict(C=9), dict(W=0), dict(H=0), dict(fx=0.0), dict(fy=0.0)):
        with pytest.raises(RuntimeError, match=INVALID):
            call(**bad)
    torch.cuda.synchronize()
    assert (sums == 7.0).all() and (weights == 7.0).all()  # nothing was launched
    with pytest.raises(RuntimeError, match=INVALID):
        _resolve(sums, weights, 0.0, [0.0] * 9)  # nine channels
    with pytest.raises(RuntimeError, match="1 to 8"):
        MB.bake_vertex_attributes(v, _cuda(c["tris"]), m, c["fx"], c["fy"], c["cx"], c["cy"], torch.zeros((3, 9, c["H"], c["W"]), device="cuda"))


def _bake(c, maps, views, owner=None, sums=None, weights=None, masked=True, with_normals=True):
    """one accumulate over views[a:b] of the case with `maps` (3, C, H, W): gs2m_meshbake_accumulate, or with `owner`
    gs2m_texbake_accumulate on the vertices as its points -> (sums, weights)"""
    a, b = views
    V, ch = len(c["verts"]), maps.shape[1]
    v, nrm, m = _cuda(c["verts"]), _cuda(c["normals"]), _cuda(c["w2c"][a:b])
    depth, x, mask = _cuda(c["depth"][a:b]), _cuda(maps[a:b]), _cuda(c["mask"][a:b])
    acc = 0 if sums is None else 1
    sums = torch.full((V, ch), 7.0, dtype=torch.float64, device="cuda") if sums is None else sums.clone()
    weights = torch.full((V,), 7.0, dtype=torch.float64, device="cuda") if weights is None else weights.clone()
    head = (V, N.ptr(v), N.ptr(nrm) if with_normals else None)
    tail = (b - a, N.ptr(m), c["fx"], c["fy"], c["cx"], c["cy"], c["W"], c["H"], N.ptr(depth), ch, N.ptr(x), N.ptr(mask) if masked else None,
            c["eps"], acc, N.ptr(sums), N.ptr(weights))
    if owner is None:
        N.launch("gs2m_meshbake_accumulate", v.device, *head, *tail)
    else:
        N.launch("gs2m_texbake_accumulate", v.device, *head, N.ptr(owner), *tail)
    torch.cuda.synchronize()
    return sums, weights


@pytest.mark.parametrize("with_normals", [True, False])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("channels", [1, 5, 8])
def test_the_texel_bake_of_owned_points_is_the_vertex_bake(channels, masked, with_normals):
    """gs2m_texbake_accumulate with the vertices as its points and every point owned gives the sums and weights of
    gs2m_meshbake_accumulate bit for bit, in a first call and in an accumulating one; a point without an owner has zeros and
    changes no other row.  gs2m_texbake_resolve without attributes, every point owned and one row as wide as the call, is
    gs2m_meshbake_resolve."""
    import ctypes as C
    c = B.bake_case()
    V = len(c["verts"])
    maps = np.concatenate([c["maps"], c["maps"][:, 2::-1]], axis=1)[:, :channels]  # eight planes from the case's five
    kw = dict(masked=masked, with_normals=with_normals)
    owned = torch.zeros(V, dtype=torch.int32, device="cuda")
    holes = owned.clone()
    holes[::3] = -1
    first = {}
    for name, owner in (("vertex", None), ("owned", owned), ("holes", holes)):
        first[name] = _bake(c, maps, (0, 2), owner, **kw)
    assert (first["vertex"][1] > 0).any()
    total = {}
    for name, owner in (("vertex", None), ("owned", owned), ("holes", holes)):
        total[name] = _bake(c, maps, (2, 3), owner, *first[name], **kw)
    for stage in (first, total):
        for k in range(2):
            assert torch.equal(stage["owned"][k], stage["vertex"][k])
            assert (stage["holes"][k][::3] == 0).all()
            keep = torch.ones(V, dtype=torch.bool, device="cuda")
            keep[::3] = False
            assert torch.equal(stage["holes"][k][keep], stage["vertex"][k][keep])
    # resolve
    s, w = total["vertex"]
    fb = [0.25 + 0.1 * k for k in range(channels)]
    out, seen, _ = _resolve(s, w, 0.3, fb)
    tout = torch.full((V, channels), -3.0, dtype=torch.float32, device="cuda")
    tseen = torch.full((V,), 9, dtype=torch.uint8, device="cuda")
    N.launch("gs2m_texbake_resolve", s.device, V, channels, V, 0, N.ptr(s), N.ptr(w), 0.3, (C.c_float * channels)(*fb), N.ptr(owned), 0, None, None,
             0, None, N.ptr(tout), N.ptr(tseen))
    assert seen.any() and not seen.all()
    assert torch.equal(tout, out) and torch.equal(tseen.bool(), seen)


# ---- G-buffer and resolve ------------------------------------------------------------------------------------------------------

def _ulps(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("ss", [1, 3])
@pytest.mark.parametrize("shading", ["smooth", "flat"])
def test_gbuffer_and_resolve_against_the_restatement(ss, shading):
    c = B.gbuffer_case()
    k = [c[n] for n in ("fx", "fy", "cx", "cy")]
    vis = MV.visibility(c["verts"], c["tris"], c["w2c"], *k, c["H"], c["W"], ss)
    tri = vis["tri"].copy()
    covered = np.argwhere(tri[0] >= 0)
    assert {0, 1, 2} <= set(np.unique(tri)) and (tri < 0).any()
    j, i = covered[len(covered) // 2]
    tri[0, j, i] = len(c["tris"])  # a key whose index is not below n_tris: an empty sample
    keys = (vis["zbits"].astype(np.int64) << 32) | np.where(tri >= 0, tri, 0xFFFFFFFF)
    keys = np.where(tri >= 0, keys, -1)
    normals = MVW.vertex_normals(_cuda(c["verts"]), _cuda(c["tris"]))[0] if shading == "smooth" else None
    g = MVW.mesh_gbuffer(_cuda(c["verts"]), _cuda(c["tris"]), _cuda(c["w2c"]), *k, c["H"], c["W"], _cuda(keys).reshape(-1), _cuda(c["albedo"]),
                         _cuda(c["roughness"]), _cuda(c["metallic"]), ss, normals)
    want = B.gbuffer(c["verts"], c["tris"], c["w2c"], *k, c["H"], c["W"], ss, tri, c["albedo"], c["roughness"], c["metallic"], shading)
    assert np.array_equal(g["coverage"].cpu().numpy(), want["coverage"]) and want["coverage"][0, j, i] == 0
    for name in ("normal", "view_dir", "albedo", "roughness", "metallic"):
        got = g[name].cpu().numpy().reshape(want[name].shape)
        assert _ulps(got, want[name]).max() <= 2, name
        assert (got[want["coverage"] == 0] == 0).all(), name
    n = g["normal"].cpu().numpy()[want["coverage"] == 1].astype(np.float64)
    d = g["view_dir"].cpu().numpy()[want["coverage"] == 1].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6 and np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-6
    assert ((n * d).sum(axis=1) >= -1e-6).all()  # the normal faces the eye
    # resolve: the same linear input on both sides, so identical bytes
    rng = np.random.default_rng(ss)
    rgb = rng.uniform(-0.1, 1.1, want["coverage"].shape + (3,)).astype(np.float32)
    bg = rng.random((1, c["H"], c["W"], 3)).astype(np.float32)
    for srgb in (False, True):
        got = MVW.resolve_rgb(_cuda(rgb), g["coverage"], ss, srgb).cpu().numpy()
        ref = B.resolve_rgb(rgb, want["coverage"], ss, srgb)
        assert np.array_equal(got, ref) and (ref[..., 3] == 255).any() and ((ref[..., 3] > 0) & (ref[..., 3] < 255)).any() == (ss > 1)
        got = MVW.resolve_rgb(_cuda(rgb), g["coverage"], ss, srgb, _cuda(bg)).cpu().numpy()
        ref = B.resolve_rgb(rgb, want["coverage"], ss, srgb, bg)
        assert (got[..., 3] == 255).all() and np.array_equal(got, ref)
        empty = want["coverage"].reshape(1, c["H"], ss, c["W"], ss).any(axis=(2, 4)) == 0
        assert np.array_equal(got[empty][:, :3], np.floor(255.0 * bg.astype(np.float64)[empty] + 0.5).astype(np.uint8))


def test_round_trip_gbuffer_to_bake():
    """affine vertex attributes on a plane, seen fronto-parallel: the G-buffer's maps are affine in the pixel coordinates, and the
    bake brings back the vertex values"""
    g = np.linspace(-1.0, 1.0, 16)
    X, Y = np.meshgrid(g, g)
    verts = np.stack([X.ravel(), Y.ravel(), np.full(256, 3.0)], axis=1)
    idx = np.arange(256).reshape(16, 16)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    tris = np.concatenate([np.stack([a, b, c], axis=1), np.stack([c, b, d], axis=1)]).astype(np.int32)  # normals towards -z: the cameras
    x, y = verts[:, 0], verts[:, 1]
    att = np.stack([0.5 + 0.3 * x + 0.1 * y, 0.5 - 0.2 * x + 0.25 * y, 0.5 + 0.1 * x - 0.35 * y, 0.6 + 0.15 * x + 0.2 * y, 0.3 - 0.1 * x + 0.1 * y],
                   axis=1).astype(np.float32)
    assert att.min() >= 0 and att.max() <= 1
    H, W, fx, fy, cx, cy = 48, 52, 45.0, 45.0, 26.0, 24.0  # the grid's vertices are 2 pixels apart
    w2c = []
    for th, (tx, ty) in zip((0.0, 0.2, -0.3, 0.5), ((0.04, -0.03), (-0.1, 0.05), (0.12, 0.08), (-0.05, -0.11))):
        M = np.eye(4)
        M[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
        M[:2, 3] = (tx, ty)
        w2c.append(M)
    w2c = np.stack(w2c)
    v, f, m = _cuda(verts), _cuda(tris), _cuda(w2c)
    vis = MVW.visibility_buffer(v, f, m, fx, fy, cx, cy, H, W, 1)
    gb = MVW.mesh_gbuffer(v, f, m, fx, fy, cx, cy, H, W, vis.reshape(-1), _cuda(att[:, :3]), _cuda(att[:, 3]), _cuda(att[:, 4]), 1,
                          MVW.vertex_normals(v, f)[0])
    maps = torch.cat([gb["albedo"], gb["roughness"], gb["metallic"]], dim=3).permute(0, 3, 1, 2).contiguous()
    cover = gb["coverage"].float()
    # texel (i, j) of the maps is the ray through (i + 0.5, j + 0.5): texel centres sit at integers for the principal point moved by half a pixel
    values, seen, weights = MB.bake_vertex_attributes(v, f, m, fx, fy, cx - 0.5, cy - 0.5, maps, cover, min_weight=1e-3)
    values, seen, cov = values.cpu().numpy(), seen.cpu().numpy(), cover.cpu().numpy() > 0.5
    # the vertices whose four taps are covered in some view, in the mask and in the mesh's own depth for these intrinsics
    depth = K.render_mesh_depth(v, f, m, fx, fy, cx - 0.5, cy - 0.5, H, W).cpu().numpy()
    cov = cov & (depth > 0)
    expect = np.zeros(256, bool)
    for k, M in enumerate(w2c):
        cam = verts @ M[:3, :3].T + M[:3, 3]
        u, w_ = fx * cam[:, 0] / cam[:, 2] + cx - 0.5, fy * cam[:, 1] / cam[:, 2] + cy - 0.5
        x0, y0 = np.floor(u).astype(int), np.floor(w_).astype(int)
        ok = (x0 >= 0) & (y0 >= 0) & (x0 + 1 < W) & (y0 + 1 < H)
        x0, y0 = np.clip(x0, 0, W - 2), np.clip(y0, 0, H - 2)
        expect |= ok & cov[k, y0, x0] & cov[k, y0, x0 + 1] & cov[k, y0 + 1, x0] & cov[k, y0 + 1, x0 + 1]
    interior = np.zeros((16, 16), bool)
    interior[1:-1, 1:-1] = True
    assert expect[interior.ravel()].all() and expect.sum() >= 14 * 14
    assert seen[expect].all()
    assert np.abs(values[seen].astype(np.float64) - att[seen].astype(np.float64)).max() <= 1e-5
    assert (weights.cpu().numpy()[seen] > 0.85).all()  # a view from 3 away of a point at most 1.6 off its axis: cos > 0.88


# ---- PBR views -----------------------------------------------------------------------------------------------------------------

def _pbr_scene():
    import gs2m_envmap as E
    verts, tris = B.icosahedron()
    rng = np.random.default_rng(12)
    w2c = MV.random_views(2, 6, radius=3.0, jitter=0.05)
    light = E.EnvLight((torch.rand((6, 64, 64, 3), generator=torch.Generator().manual_seed(5)) * 1.5).cuda())
    k = dict(fx=30.0, fy=30.5, cx=16.2, cy=11.9)
    return verts, tris, w2c, light, k, rng.random((12, 3)).astype(np.float32), rng.random(12).astype(np.float32), rng.random(12).astype(np.float32)


@pytest.mark.parametrize("gamma,background", [(False, "none"), (True, "none"), (True, "env")])
def test_shade_views_pbr_against_the_unfused_shading(gamma, background):
    from pbr import pbr_shading
    verts, tris, w2c, light, k, alb, rough, metal = _pbr_scene()
    H, W, ss = 24, 32, 2
    v, f, m = _cuda(verts), _cuda(tris), _cuda(w2c)
    args = (v, f, m, k["fx"], k["fy"], k["cx"], k["cy"], H, W)
    got = MVW.shade_views_pbr(*args, light, _cuda(alb), _cuda(rough), _cuda(metal), ss=ss, shading="smooth", gamma=gamma, background=background)
    assert got.shape == (2, H, W, 4) and got.dtype == torch.uint8
    assert torch.equal(got, MVW.shade_views_pbr(*args, light, _cuda(alb), _cuda(rough), _cuda(metal), ss=ss, shading="smooth", gamma=gamma,
                                                background=background, view_batch=1))
    # the oracle: the same G-buffer samples, the unfused shading, the restatement's resolve
    vis = MVW.visibility_buffer(*args, ss)
    g = MVW.mesh_gbuffer(*args, vis.reshape(-1), _cuda(alb), _cuda(rough), _cuda(metal), ss, MVW.vertex_normals(v, f)[0])
    rgb = []
    with torch.no_grad():
        light.cubemap.build_mips()
        for n in range(2):
            ones = torch.ones_like(g["roughness"][n])
            rgb.append(pbr_shading(light.cubemap, g["normal"][n], g["view_dir"][n], g["albedo"][n], g["roughness"][n], metallic=g["metallic"][n],
                                   occlusion=ones, irradiance=torch.zeros_like(ones), brdf_lut=light.brdf_lut)["render_rgb"].reshape(H * ss, W * ss, 3))
        bg = None
        if background == "env":
            from gs2m_relight import environment_behind
            bg = torch.stack([environment_behind(light, d, gamma) for d in MVW.pixel_view_dirs(m, k["fx"], k["fy"], k["cx"], k["cy"], H, W)]).cpu().numpy()
    want = B.resolve_rgb(torch.stack(rgb).cpu().numpy(), g["coverage"].cpu().numpy(), ss, gamma, bg)
    got = got.cpu().numpy()
    assert np.array_equal(got[..., 3], want[..., 3])
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
    alpha = got[..., 3]
    if background == "none":
        assert (alpha == 255).any() and (alpha == 0).any() and ((alpha > 0) & (alpha < 255)).any()
        assert got[alpha == 255][:, :3].std() > 5  # a lit, coloured surface
    else:
        assert (alpha == 255).all()


# ---- command lines -------------------------------------------------------------------------------------------------------------

def test_command_lines(tmp_path):
    import gs2m_envmap as E
    import gs2m_mesh as M
    import gs2m_train as T
    from gs2m_model import GaussianModel
    from PIL import Image
    W, H = 48, 32
    scene = tmp_path / "scene"
    T.export_colmap_dataset(str(scene), T.synthetic_scene(2000, 3, W, H, seed=1))
    ply = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_small.ply")
    verts, tris = B.icosahedron()
    verts = 0.8 * verts + np.array([0.0, -0.8, 6.0])  # where the scene's cameras look
    import types
    M.write_mesh(tmp_path / "mesh.ply", types.SimpleNamespace(vertices=verts, triangles=tris, vertex_colors=np.zeros((12, 3))))
    out = tmp_path / "material.ply"
    r = MB.main(["--ply", ply, "-s", str(scene), "--mesh", str(tmp_path / "mesh.ply"), "-o", str(out), "--metallic"])
    assert r["n_views"] == 3 and r["n_vertices"] == 12
    # the same in-process
    cams, _, _, _, _ = T.load_colmap_dataset(str(scene), resolution=1)
    model = GaussianModel(3)
    model.load_ply(ply)
    mesh = M.read_mesh(tmp_path / "mesh.ply")
    values, seen, _ = MB.bake_materials(model, cams, mesh, metallic=True)
    MB.write_material_mesh(tmp_path / "again.ply", mesh.vertices, mesh.triangles, values, seen)
    assert out.read_bytes() == (tmp_path / "again.ply").read_bytes()
    back = MB.read_material_mesh(out)
    assert np.array_equal(back["vertices"], mesh.vertices) and np.array_equal(back["triangles"], mesh.triangles)
    assert np.array_equal(back["seen"], seen.cpu().numpy())
    # the material mesh under a light
    light = E.EnvLight((0.2 + torch.rand((6, 64, 64, 3), generator=torch.Generator().manual_seed(2))).cuda())
    hdr = E.save_light_hdr(light, str(tmp_path / "tiny.hdr"), res=(16, 32))
    res = MVW.main(["--ply-path", str(out), "-s", str(scene), "--out-dir", str(tmp_path / "visual"), "--rendering", "--colour", "pbr", "--envmap", hdr,
                    "--env-res", "64", "--env-samples", "2", "--env-rotation", "20", "--exposure", "0.5", "--gamma", "--shading", "smooth"])
    assert len(res["views"]) == 3
    for p in res["views"]:
        with Image.open(p) as img:
            a = np.asarray(img)
        assert a.shape == (H, W, 4) and (a[..., 3] == 255).any() and (a[..., 3] == 0).any() and a[a[..., 3] == 255][:, :3].max() > 0
    res = MVW.main(["--ply-path", str(out), "-s", str(scene), "--out-dir", str(tmp_path / "visual_env"), "--rendering", "--render_view_idx", "0", "--colour",
                    "pbr", "--envmap", hdr, "--env-res", "64", "--background", "env"])
    with Image.open(res["views"][0]) as img:
        a = np.asarray(img)
    with Image.open(tmp_path / "visual" / "views" / os.path.basename(res["views"][0])) as img:
        behind = np.asarray(img)[..., 3] == 0  # where the first run saw no mesh: the environment
    assert a.shape == (H, W, 4) and (a[..., 3] == 255).all() and behind.any() and a[behind][:, :3].min() > 0
    # a plain mesh is refused with a clear message; without --colour pbr nothing changes
    with pytest.raises(RuntimeError, match="material mesh"):
        MVW.main(["--ply-path", str(tmp_path / "mesh.ply"), "-s", str(scene), "--out-dir", str(tmp_path / "x"), "--rendering", "--colour", "pbr", "--envmap", hdr])
    grey = MVW.main(["--ply-path", str(out), "-s", str(scene), "--out-dir", str(tmp_path / "grey"), "--rendering"])
    plain = MVW.main(["--ply-path", str(tmp_path / "mesh.ply"), "-s", str(scene), "--out-dir", str(tmp_path / "grey2"), "--rendering"])
    for p, q in zip(grey["views"], plain["views"]):
        assert open(p, "rb").read() == open(q, "rb").read()
