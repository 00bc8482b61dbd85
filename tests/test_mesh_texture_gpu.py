"""The triangle atlas, the texel bake and the glTF export on the GPU (csrc/mesh_atlas.hip, csrc/mesh_bake.hip,
gs2m_mesh_texture.py) against the fp64 restatement of tests/mesh_texture_ref.py.  All data is synthetic.

Tolerances: the integer side (class, cell, half, histogram, size, owner, interior) and the fp32 UVs are held to equality;
barycentric points, normals, sums and weights to 1e-12 relative (the bound tests/test_mesh_bake_gpu.py uses for the same
arithmetic: what a division or square root of another library may differ by); resolved fp32 values to 1 ulp; linear and ORM
bytes to the restatement's packing of the device's own fp32 values; sRGB bytes to 1, and to equality outside the 1e-6 band of
mesh_texture_ref.srgb_band."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import gs2m_mesh_texture as MT
import gs2m_native as N
import mesh_bake_ref as B
import mesh_texture_ref as T

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = "invalid argument", "unsupported size"


def _cuda(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def _mesh(verts, tris):
    return types.SimpleNamespace(vertices=_cuda(verts, torch.float64), triangles=_cuda(tris, torch.int32))


def _close(got, want, rel):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= rel * np.abs(want)))


def _check_atlas(a, want):
    assert a.hist == want["hist"] and (a.width, a.height) == (want["width"], want["height"]) and a.bases == want["base"]
    assert np.array_equal(a.cells.cpu().numpy(), want["cells"])
    assert np.array_equal(a.order.cpu().numpy(), want["order"])
    assert np.array_equal(a.cells[:, 2].cpu().numpy(), 8 << want["cls"])
    assert np.array_equal(a.uvs.cpu().numpy(), want["uvs"])  # exact in fp32


def _check_texels(a, verts, normals, tris, want_atlas):
    want = T.texels(verts, normals, tris, want_atlas)
    owner, interior, points, tn = MT.atlas_texels(a, None if normals is None else _cuda(normals))
    assert np.array_equal(owner.cpu().numpy(), want["owner"])
    assert np.array_equal(interior.cpu().numpy(), want["interior"])
    assert _close(points.cpu().numpy(), want["points"], 1e-12) and _close(tn.cpu().numpy(), want["normals"], 1e-12)
    return want


@pytest.mark.parametrize("name", T.SMALL_SHAPES)
def test_small_shapes_against_the_restatement(name):
    verts, tris, density = T.small_shape(name)
    want = T.build(verts, tris, density)
    a = MT.build_atlas(_mesh(verts, tris), density=density)
    _check_atlas(a, want)
    assert MT.atlas_count(a.vertices, a.triangles, density) == (want["hist"], want["width"], want["height"])
    tex = _check_texels(a, verts, None, tris, want)
    if name == "one":
        assert (tex["owner"] >= 0).sum() == 36 and (a.width, a.height) == (8, 8)       # half 1 is empty
    if name == "four":
        assert (a.width, a.height) == (16, 8)
    if name == "clamped":
        assert a.hist[5] == 1
    if name == "zero_area":
        assert a.hist[0] == 2
    if name == "second_half":
        assert a.height == a.width == 64


def test_empty_mesh():
    a = MT.build_atlas(_mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int32)), density=3.0)
    assert a.hist == [0] * 6 and (a.width, a.height) == (0, 0)
    owner, interior, points, tn = MT.atlas_texels(a)
    assert owner.numel() == 0 and points.numel() == 0
    b = MT.TextureBaker(a, 5)
    values, seen, weights = b.finish()
    assert values.shape == (0, 0, 5) and seen.numel() == 0
    with pytest.raises(RuntimeError, match="no triangle"):
        MT.export_glb("unused.glb", a, None)


def test_icosphere_atlas_and_texels():
    c = T.sphere_case()
    a = MT.build_atlas(_mesh(c["verts"], c["tris"]), density=c["density"])
    _check_atlas(a, c["atlas"])
    assert sum(h > 0 for h in a.hist) == 2
    _check_texels(a, c["verts"], c["normals"], c["tris"], c["atlas"])
    _check_texels(a, c["verts"], None, c["tris"], c["atlas"])
    # a band of rows is the same rows
    full = MT.atlas_texels(a, _cuda(c["normals"]))
    band = MT.atlas_texels(a, _cuda(c["normals"]), row0=40, n_rows=17)
    for x, y in zip(full, band):
        assert torch.equal(x[40:57], y)


def _device_case(c):
    a = MT.build_atlas(_mesh(c["verts"], c["tris"]), density=c["density"])
    # the restatement's own texels (test_icosphere_atlas_and_texels compares the device's with them): the bake is then held to
    # the restatement on identical inputs
    x = c["tex"]
    return a, _cuda(x["owner"], torch.int32).reshape(-1), _cuda(x["points"]).reshape(-1, 3), _cuda(x["normals"]).reshape(-1, 3)


def _accumulate(c, dev, views, channels, sums=None, weights=None, masked=True, with_normals=True, fill=None):
    a, owner, points, tn = dev
    lo, hi = views
    n = len(owner)
    m, depth = _cuda(c["w2c"][lo:hi]), _cuda(c["depth"][lo:hi])
    maps, mask = _cuda(c["maps"][lo:hi, :channels]), _cuda(c["mask"][lo:hi])
    acc = 0 if sums is None else 1
    sums = torch.full((n, channels), 7.0, dtype=torch.float64, device="cuda") if sums is None else sums.clone()
    weights = torch.full((n,), 7.0, dtype=torch.float64, device="cuda") if weights is None else weights.clone()
    N.launch("gs2m_texbake_accumulate", points.device, n, N.ptr(points), N.ptr(tn) if with_normals else None, N.ptr(owner), hi - lo, N.ptr(m),
             c["fx"], c["fy"], c["cx"], c["cy"], c["W"], c["H"], N.ptr(depth), channels, N.ptr(maps), N.ptr(mask) if masked else None, c["eps"],
             acc, N.ptr(sums), N.ptr(weights))
    torch.cuda.synchronize()
    return sums, weights


def _resolve(dev, sums, weights, min_weight, fallback, attributes=None):
    a, owner, _, _ = dev
    n, ch = sums.shape
    out = torch.full((n, ch), -3.0, dtype=torch.float32, device="cuda")
    seen = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    N.launch("gs2m_texbake_resolve", sums.device, n, ch, a.width, 0, N.ptr(sums), N.ptr(weights), float(min_weight), (C.c_float * ch)(*fallback),
             N.ptr(owner), len(a.triangles), N.ptr(a.triangles), N.ptr(a.cells), len(a.vertices), N.ptr(attributes), N.ptr(out), N.ptr(seen))
    return out, seen


def _ulps(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("channels,masked,with_normals", [(5, True, True), (3, False, True), (5, True, False)])
def test_sums_weights_resolve_and_pack_against_the_restatement(channels, masked, with_normals):
    c = T.sphere_case()
    dev = _device_case(c)
    want_s, want_w, use, _ = T.sphere_reference(channels, masked, with_normals)
    s, w = _accumulate(c, dev, (0, 5), channels, masked=masked, with_normals=with_normals)
    sn, wn = s.cpu().numpy(), w.cpu().numpy()
    assert np.array_equal(wn > 0, want_w > 0) and (want_w > 0).any()
    assert _close(wn, want_w, 1e-12) and _close(sn, want_s, 1e-12)
    empty = c["tex"]["owner"].reshape(-1) < 0
    assert empty.any() and (sn[empty] == 0).all() and (wn[empty] == 0).all()
    for k in range(5):  # the contributing (texel, view) pairs: each view alone
        _, wk = _accumulate(c, dev, (k, k + 1), channels, masked=masked, with_normals=with_normals)
        assert np.array_equal(wk.cpu().numpy() > 0, use[:, k]), k
    # resolve, with the per-vertex attributes behind the texels no view reached
    fb = [0.2 + 0.1 * k for k in range(channels)]
    att = np.random.default_rng(5).random((len(c["verts"]), channels)).astype(np.float32)
    for attributes in (None, att):
        out, seen = _resolve(dev, s, w, 0.3, fb, None if attributes is None else _cuda(attributes))
        want_out, want_seen = T.resolve(c["tex"], c["tris"], sn, wn, 0.3, fb, attributes)
        assert np.array_equal(seen.cpu().numpy().astype(bool), want_seen) and want_seen.any() and (~want_seen & ~empty).any()
        assert _ulps(out.cpu().numpy(), want_out).max() <= 1.0
        assert np.array_equal(out.cpu().numpy()[empty], np.tile(np.float32(fb), (empty.sum(), 1)))
    values = out.reshape(c["atlas"]["height"], c["atlas"]["width"], channels)
    vn = values.cpu().numpy()
    lin, orm = MT.pack_textures(values, srgb=False)
    want_lin, want_orm = T.pack(vn, srgb=False)
    assert np.array_equal(lin.cpu().numpy(), want_lin)
    assert (orm is None and want_orm is None) or np.array_equal(orm.cpu().numpy(), want_orm)
    enc, _ = MT.pack_textures(values, srgb=True)
    want_enc, _ = T.pack(vn, srgb=True)
    d = np.abs(enc.cpu().numpy().astype(int) - want_enc.astype(int))
    assert d.max() <= 1 and (d[T.srgb_band(vn) >= 1e-6] == 0).all()


def test_bitwise_identities():
    c = T.sphere_case()
    dev = _device_case(c)
    s, w = _accumulate(c, dev, (0, 5), 5)
    s2, w2 = _accumulate(c, dev, (0, 5), 5)
    assert torch.equal(s, s2) and torch.equal(w, w2)  # two runs
    for k in (1, 3):  # the views split over two calls
        sa, wa = _accumulate(c, dev, (0, k), 5)
        sb, wb = _accumulate(c, dev, (k, 5), 5, sa, wa)
        assert torch.equal(s, sb) and torch.equal(w, wb), k
    # through the Python API (the mesh's depth comes from the rasterizer there): view_batch 1 against 8
    a = dev[0]
    args = (_cuda(c["w2c"]), c["fx"], c["fy"], c["cx"], c["cy"], _cuda(c["maps"]), _cuda(c["mask"]))
    one = MT.bake_texel_attributes(a, *args, view_batch=1, min_weight=0.2, fallback=(1, 2, 3, 4, 5))
    eight = MT.bake_texel_attributes(a, *args, view_batch=8, min_weight=0.2, fallback=(1, 2, 3, 4, 5))
    for x, y in zip(one, eight):
        assert torch.equal(x, y)
    assert one[0].dtype == torch.float32 and one[1].dtype == torch.bool and one[1].any() and not one[1].all()
    # a workspace full of ones: the atlas does not depend on what the workspace held
    v, f = a.vertices, a.triangles
    ws = MT.workspace_for("gs2m_atlas_workspace_bytes", v.device, len(f))
    ws.fill_(0xFF)
    cells, uvs, order = torch.empty_like(a.cells), torch.empty_like(a.uvs), torch.empty_like(a.order)
    hist, bases, dims = (C.c_longlong * 6)(), (C.c_longlong * 6)(), (C.c_int * 2)()
    N.launch("gs2m_atlas_build", v.device, len(v), len(f), N.ptr(v), N.ptr(f), c["density"], N.ptr(ws), N.ptr(cells), N.ptr(uvs), N.ptr(order), hist,
             bases, dims)
    assert torch.equal(cells, a.cells) and torch.equal(uvs, a.uvs) and torch.equal(order, a.order) and list(hist) == a.hist


def test_errors_leave_the_outputs_untouched():
    verts, tris, density = T.small_shape("four")
    v, f = _cuda(verts, torch.float64), _cuda(tris, torch.int32)
    ws = MT.workspace_for("gs2m_atlas_workspace_bytes", v.device, len(f))
    cells = torch.full((len(f), 4), -7, dtype=torch.int32, device="cuda")
    uvs = torch.full((len(f), 3, 2), -7.0, dtype=torch.float32, device="cuda")
    order = torch.full((len(f),), -7, dtype=torch.int32, device="cuda")
    hist, bases, dims = (C.c_longlong * 6)(*[-7] * 6), (C.c_longlong * 6)(*[-7] * 6), (C.c_int * 2)(-7, -7)

    def build(vv=v, ff=f, d=density, nv=None):
        N.launch("gs2m_atlas_build", v.device, len(vv) if nv is None else nv, len(ff), N.ptr(vv), N.ptr(ff), d, N.ptr(ws), N.ptr(cells),
                 N.ptr(uvs), N.ptr(order), hist, bases, dims)

    bad_v = v.clone()
    bad_v[4, 1] = float("nan")
    inf_v = v.clone()
    inf_v[0, 0] = float("inf")
    bad_f = f.clone()
    bad_f[2, 1] = len(v)
    neg_f = f.clone()
    neg_f[0, 0] = -1
    for kw in (dict(vv=bad_v), dict(vv=inf_v), dict(ff=bad_f), dict(ff=neg_f), dict(d=0.0), dict(d=-1.0), dict(d=float("nan")),
               dict(d=float("inf"))):
        with pytest.raises(RuntimeError, match=INVALID):
            build(**kw)
    # wider than 16384: 8200 triangles of side 256 are 4100 cells of 1024 units, more than 4^11
    big_v, _, _ = T.small_shape("second_half")
    n = 8200
    bv = _cuda(np.tile(big_v[:3], (n, 1)) * 1000.0, torch.float64)
    bf = _cuda(np.arange(3 * n).reshape(n, 3), torch.int32)
    ws_big = MT.workspace_for("gs2m_atlas_workspace_bytes", v.device, n)
    h2, d2 = (C.c_longlong * 6)(*[-7] * 6), (C.c_int * 2)(-7, -7)
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        N.launch("gs2m_atlas_count", v.device, len(bv), n, N.ptr(bv), N.ptr(bf), 1.0, N.ptr(ws_big), h2, d2)
    torch.cuda.synchronize()
    assert (cells == -7).all() and (uvs == -7).all() and (order == -7).all()
    assert list(hist) == [-7] * 6 and list(bases) == [-7] * 6 and list(dims) == [-7, -7] and list(h2) == [-7] * 6 and list(d2) == [-7, -7]
    # texels: a histogram that is not this mesh's, a size that is not the histogram's, rows beyond the atlas
    a = MT.build_atlas(_mesh(verts, tris), density=density)
    owner = torch.full((a.height, a.width), -7, dtype=torch.int32, device="cuda")
    interior = torch.full((a.height, a.width), 7, dtype=torch.uint8, device="cuda")
    points = torch.full((a.height, a.width, 3), -7.0, dtype=torch.float64, device="cuda")
    tn = points.clone()

    def texels(hist=a.hist, width=a.width, height=a.height, row0=0, n_rows=a.height):
        N.launch("gs2m_atlas_texels", v.device, len(v), N.ptr(v), None, len(f), N.ptr(f), N.ptr(a.order), (C.c_longlong * 6)(*hist), width, height,
                 row0, n_rows, N.ptr(owner), N.ptr(interior), N.ptr(points), N.ptr(tn))

    for kw in (dict(hist=[3, 0, 0, 0, 0, 0]), dict(hist=[-1, 5, 0, 0, 0, 0]), dict(width=8), dict(height=16), dict(row0=1), dict(row0=-1),
               dict(n_rows=-1)):
        with pytest.raises(RuntimeError, match=INVALID):
            texels(**kw)
    # bake, resolve and pack
    sums = torch.full((a.height * a.width, 5), 7.0, dtype=torch.float64, device="cuda")
    weights = torch.full((a.height * a.width,), 7.0, dtype=torch.float64, device="cuda")
    m = _cuda(np.eye(4)[None])
    img = torch.zeros((1, 5, 4, 4), device="cuda")
    MT.atlas_texels(a)  # (a valid call in between)
    own, _, pts, _ = MT.atlas_texels(a)

    def accumulate(C_=5, W=4, H=4, fx=5.0, eps=0.1):
        N.launch("gs2m_texbake_accumulate", v.device, a.height * a.width, N.ptr(pts), None, N.ptr(own), 1, N.ptr(m), fx, 5.0, 2.0, 2.0, W, H,
                 N.ptr(img[:, 0]), C_, N.ptr(img), None, eps, 0, N.ptr(sums), N.ptr(weights))

    for kw in (dict(C_=0), dict(C_=9), dict(W=0), dict(H=0), dict(fx=0.0), dict(eps=float("nan"))):
        with pytest.raises(RuntimeError, match=INVALID):
            accumulate(**kw)
    out = torch.full((a.height * a.width, 5), -7.0, dtype=torch.float32, device="cuda")
    seen = torch.full((a.height * a.width,), 7, dtype=torch.uint8, device="cuda")
    for ch, width, mw in ((0, a.width, 0.1), (9, a.width, 0.1), (5, 0, 0.1), (5, a.width, float("nan"))):
        with pytest.raises(RuntimeError, match=INVALID):
            N.launch("gs2m_texbake_resolve", v.device, a.height * a.width, ch, width, 0, N.ptr(sums), N.ptr(weights), mw, (C.c_float * 9)(), N.ptr(own),
                     len(f), N.ptr(f), N.ptr(a.cells), len(v), None, N.ptr(out), N.ptr(seen))
    base = torch.full((a.height, a.width, 3), 7, dtype=torch.uint8, device="cuda")
    for ch, orm in ((4, base), (3, base), (5, None)):
        with pytest.raises(RuntimeError, match=INVALID):
            N.launch("gs2m_texture_pack", v.device, a.height * a.width, ch, N.ptr(out), 1, N.ptr(base), None if orm is None else N.ptr(orm))
    torch.cuda.synchronize()
    assert (owner == -7).all() and (interior == 7).all() and (points == -7).all() and (tn == -7).all()
    assert (sums == 7).all() and (weights == 7).all() and (out == -7).all() and (seen == 7).all() and (base == 7).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------

def test_texture_size_lands_under_its_target():
    c = T.sphere_case()
    for target in (256, 700):
        a = MT.build_atlas(_mesh(c["verts"], c["tris"]), texture_size=target)
        assert a.width <= target and a.rung is not None
        nxt = MT.base_density(a.vertices, a.triangles) * 2.0 ** ((a.rung + 1) / MT.LADDER)
        assert MT.atlas_count(a.vertices, a.triangles, nxt)[1] > target
        assert a.density == MT.base_density(a.vertices, a.triangles) * 2.0 ** (a.rung / MT.LADDER)
    with pytest.raises(RuntimeError, match="does not fit"):
        MT.build_atlas(_mesh(c["verts"], c["tris"]), texture_size=64)  # 160 cells of side 8 are 128 wide
    with pytest.raises(ValueError, match="one of"):
        MT.build_atlas(_mesh(c["verts"], c["tris"]))


def _plane_views(c):
    """four views of the tilted plane and the affine field as they see it"""
    k = T.FRAME
    n = np.array([-0.3, 0.2, 1.0])  # z = 3 + 0.3 x - 0.2 y
    w2c = np.stack([T.R.look_at(e, [0.0, 0.0, 3.0]) for e in ([0.0, 0.0, 0.0], [0.8, 0.3, 0.2], [-0.7, -0.5, 0.1], [0.2, 0.9, 0.3])])
    return w2c, T.affine_maps(w2c, k["H"], k["W"], k["fx"], k["fy"], k["cx"], k["cy"], n, 3.0)


def test_glb_reproduces_the_affine_field_and_both_png_routes_agree(tmp_path):
    c = T.plane_case()
    k = T.FRAME
    verts, tris = c["verts"], c["tris"]
    a = MT.build_atlas(_mesh(verts, tris), density=c["density"])
    w2c, maps = _plane_views(c)
    # (texels along the plane's border see a z-buffer that fades to 0 there and fail the depth test: they read the vertices)
    values, seen, _ = MT.bake_texel_attributes(a, _cuda(w2c), k["fx"], k["fy"], k["cx"], k["cy"], _cuda(maps), view_batch=3,
                                               attributes=_cuda(T.affine_field(verts).astype(np.float32)))
    owner = MT.atlas_texels(a)[0].cpu().numpy() >= 0
    assert seen.cpu().numpy()[owner].mean() > 0.8
    base, orm = MT.pack_textures(values, srgb=False)
    host = MT.export_glb(tmp_path / "host.glb", a, base, orm, textures_dir=str(tmp_path / "tex"))
    MT.export_glb(tmp_path / "device.glb", a, base, orm, device_png=True)
    g, gd = MT.read_glb(tmp_path / "host.glb"), MT.read_glb(tmp_path / "device.glb")
    assert (tmp_path / "host.glb").read_bytes() == host and len(g["images"]) == 2
    px = [MT.decode_png(b) for b in g["images"]]
    assert np.array_equal(px[0], base.cpu().numpy()) and np.array_equal(px[1], orm.cpu().numpy())
    for x, y in zip(px, [MT.decode_png(b) for b in gd["images"]]):
        assert np.array_equal(x, y)  # --device-png decodes to the same pixels
    assert np.array_equal(MT.decode_png((tmp_path / "tex" / "base_color.png").read_bytes()), px[0])
    assert np.array_equal(g["uvs"], a.uvs.reshape(-1, 2).cpu().numpy()) and np.array_equal(g["indices"], np.arange(3 * len(tris)))
    assert np.array_equal(g["positions"], verts[tris].reshape(-1, 3).astype(np.float32))
    # random surface points: the glb's textures at their UVs against the field.  The views sample the field at pixel centres and
    # the bake interpolates those bilinearly: a perspective view bends an affine field by less than 2e-4 over a pixel here.
    rng = np.random.default_rng(4)
    t = rng.integers(0, len(tris), 400)
    l = rng.dirichlet(np.ones(3), 400)
    p = (l[:, :, None] * verts[tris[t]]).sum(1)
    uv = (l[:, :, None] * g["uvs"].reshape(-1, 3, 2)[t].astype(np.float64)).sum(1)
    tex = np.concatenate([px[0], px[1][..., 1:]], axis=2).astype(np.float64) / 255.0
    got, _, _ = T.sample_bilinear(tex, uv)
    assert np.abs(got - T.affine_field(p)).max() <= 1.0 / 255.0 + 1e-6


def test_unseen_texels_read_the_vertex_values():
    c = T.plane_case()
    k = T.FRAME
    verts, tris = c["verts"], c["tris"]
    a = MT.build_atlas(_mesh(verts, tris), density=c["density"])
    w2c, maps = _plane_views(c)
    field = T.affine_field(verts).astype(np.float32)
    baker = MT.TextureBaker(a, 5)
    baker.add(_cuda(w2c), k["fx"], k["fy"], k["cx"], k["cy"], _cuda(maps))
    assert (baker.weights > 0).any()
    values, seen, _ = baker.finish(min_weight=1e9, fallback=(9, 9, 9, 9, 9), attributes=_cuda(field))  # no texel has that weight
    assert not seen.any()
    owner = MT.atlas_texels(a)[0].cpu().numpy()
    want, _ = T.resolve(c["tex"], tris, np.zeros((owner.size, 5)), np.zeros(owner.size), 1e9, (9, 9, 9, 9, 9), field)
    assert _ulps(values.cpu().numpy().reshape(-1, 5), want).max() <= 1.0
    assert (values.cpu().numpy()[owner < 0] == 9).all()
    # an affine field interpolates exactly: a bilinear lookup whose taps are interior texels gives it back before packing (a skirt
    # texel holds the value of a point ON the triangle, not the field's continuation: tests/test_mesh_texture.py bounds that)
    rng = np.random.default_rng(6)
    t = rng.integers(0, len(tris), 300)
    l = rng.dirichlet(np.ones(3), 300)
    uv = (l[:, :, None] * a.uvs.cpu().numpy().astype(np.float64)[t]).sum(1)
    got, taps, w = T.sample_bilinear(values.cpu().numpy(), uv)
    interior = MT.atlas_texels(a)[1].cpu().numpy()
    inner = (interior[taps[..., 0], taps[..., 1]] | (w == 0)).all(1)
    err = np.abs(got - T.affine_field((l[:, :, None] * verts[tris[t]]).sum(1))).max(1)
    assert inner.mean() > 0.5 and err[inner].max() <= 2e-6  # fp32 texels, fp32 uvs


def test_mesh_command_line_takes_texture_size(tmp_path):
    """gs2m_mesh.py: without the flag the files are what they were and no .glb appears; with it tsdf_textured.glb holds the
    post-processed mesh, or the simplified one when the run made it, and the other files are the same bytes."""
    import gs2m_mesh as M
    import gs2m_train as Tr
    from gs2m_model import GaussianModel
    Tr.export_colmap_dataset(str(tmp_path / "scene"), Tr.synthetic_scene(8000, 4, 96, 64, seed=1))
    import test_mesh_gpu as TM
    truth, _ = TM._truth_and_cams(8000, 1, 96, 64)
    model = GaussianModel(3)
    model.parameterize((truth._xyz, truth._features_dc, truth._features_rest, truth._scaling, truth._rotation, truth._opacity,
                        truth._albedo, truth._roughness, truth._metallic))
    model.active_sh_degree = 3
    model.save_ply(str(tmp_path / "model.ply"))
    base = ["--ply", str(tmp_path / "model.ply"), "-s", str(tmp_path / "scene"), "--voxel_size", "0.16"]
    plain, tex, both = tmp_path / "plain", tmp_path / "tex", tmp_path / "both"
    M.main(base + ["-o", str(plain)])
    M.main(base + ["-o", str(tex), "--texture-size", "512"])
    M.main(base + ["-o", str(both), "--texture-size", "512", "--simplify-cell", "0.48"])
    assert not (plain / "tsdf_textured.glb").exists() and not (tex / "tsdf_simplified.ply").exists()
    assert (plain / "config.json").read_bytes() == (tex / "config.json").read_bytes()
    for name in ("tsdf_mesh.ply", "tsdf_post.ply"):  # the same surface (as sets: the extraction does not promise an order)
        m0, m1 = M.read_mesh(plain / name), M.read_mesh(tex / name)
        assert len(m0.triangles) == len(m1.triangles)
        assert np.array_equal(np.unique(np.asarray(m0.vertices), axis=0), np.unique(np.asarray(m1.vertices), axis=0)), name
    for out, source in ((tex, "tsdf_post.ply"), (both, "tsdf_simplified.ply")):
        g = MT.read_glb(out / "tsdf_textured.glb")
        mesh = M.read_mesh(out / source)
        assert len(mesh.triangles) > 0 and len(g["positions"]) == 3 * len(mesh.triangles)
        assert np.array_equal(g["positions"], np.asarray(mesh.vertices, np.float32)[np.asarray(mesh.triangles)].reshape(-1, 3))
        px = [MT.decode_png(b) for b in g["images"]]
        assert len(px) == 2 and px[0].shape[1] <= 512 and px[0].shape == px[1].shape
    assert len(M.read_mesh(both / "tsdf_simplified.ply").triangles) < len(M.read_mesh(both / "tsdf_post.ply").triangles)


def test_command_line(tmp_path):
    import os
    import gs2m_mesh as M
    import gs2m_train as Tr
    from gs2m_model import GaussianModel
    W, H = 48, 32
    scene = tmp_path / "scene"
    Tr.export_colmap_dataset(str(scene), Tr.synthetic_scene(2000, 3, W, H, seed=1))
    ply = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_small.ply")
    verts, tris = B.icosahedron()
    verts = 0.8 * verts + np.array([0.0, -0.8, 6.0])  # where the scene's cameras look
    M.write_mesh(tmp_path / "mesh.ply", types.SimpleNamespace(vertices=verts, triangles=tris, vertex_colors=np.full((12, 3), 0.25)))
    out = tmp_path / "asset.glb"
    r = MT.main(["--ply", ply, "-s", str(scene), "--mesh", str(tmp_path / "mesh.ply"), "-o", str(out), "--texture-size", "128", "--metallic"])
    assert r["n_views"] == 3 and r["width"] <= 128 and r["n_seen"] > 0
    g = MT.read_glb(out)
    assert len(g["positions"]) == 60 and len(g["images"]) == 2
    assert g["json"]["materials"][0]["pbrMetallicRoughness"]["metallicRoughnessTexture"] == {"index": 1}
    # the same in-process
    cams, _, _, _, _ = Tr.load_colmap_dataset(str(scene), resolution=1)
    model = GaussianModel(3)
    model.load_ply(ply)
    mesh = M.read_mesh(tmp_path / "mesh.ply")
    again = MT.texture_mesh(model, cams, mesh, tmp_path / "again.glb", texture_size=128, metallic=True)
    assert (tmp_path / "again.glb").read_bytes() == out.read_bytes() and again["density"] == r["density"]
    px = MT.decode_png(g["images"][1])
    assert px.shape == (r["height"], r["width"], 3) and (px[..., 0] == 255).all()
    # a plain colour bake: one texture, linear bytes, through the device's PNG encoder
    r3 = MT.main(["--ply", ply, "-s", str(scene), "--mesh", str(tmp_path / "mesh.ply"), "-o", str(tmp_path / "rgb.glb"), "--density",
                  str(r["density"]), "--rgb", "--linear", "--device-png"])
    g3 = MT.read_glb(tmp_path / "rgb.glb")
    assert len(g3["images"]) == 1 and (r3["width"], r3["height"]) == (r["width"], r["height"])
    assert "metallicRoughnessTexture" not in g3["json"]["materials"][0]["pbrMetallicRoughness"]
    assert np.array_equal(g3["uvs"], g["uvs"])
    # a material mesh: texels no view reached read its per-vertex albedo, roughness and metallic, not constants
    import gs2m_mesh_bake as MB
    vals = np.random.default_rng(3).random((12, 5)).astype(np.float32)
    MB.write_material_mesh(tmp_path / "material.ply", verts, tris, vals)
    src, vertex_values = MT.read_source_mesh(tmp_path / "material.ply")
    assert vertex_values.shape == (12, 5) and np.array_equal(vertex_values[:, 3:], vals[:, 3:])
    assert np.abs(vertex_values[:, :3] - vals[:, :3]).max() <= 0.5 / 255 + 1e-7 and MT.read_source_mesh(tmp_path / "mesh.ply")[1] is None
    rm = MT.texture_mesh(model, cams, src, tmp_path / "m.glb", density=r["density"], metallic=True, linear=True, min_weight=1e9,
                         vertex_values=vertex_values)
    assert rm["n_seen"] == 0
    orm = MT.decode_png(MT.read_glb(tmp_path / "m.glb")["images"][1]).astype(np.float64) / 255.0
    a = MT.build_atlas(src, density=r["density"])
    own, inner = (x.cpu().numpy() for x in MT.atlas_texels(a)[:2])
    t = own[inner]
    lo, hi = vals[tris[t]][..., 3:].min(1), vals[tris[t]][..., 3:].max(1)  # an interior texel lies within its corners' values
    assert ((orm[inner][:, 1:] >= lo - 0.5 / 255 - 1e-6) & (orm[inner][:, 1:] <= hi + 0.5 / 255 + 1e-6)).all()
    assert np.ptp(orm[inner][:, 1]) > 0.2
    rc = MT.main(["--ply", ply, "-s", str(scene), "--mesh", str(tmp_path / "material.ply"), "-o", str(tmp_path / "mc.glb"), "--density",
                  str(r["density"]), "--metallic"])
    assert rc["width"] == r["width"]
