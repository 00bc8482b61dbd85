"""The LBVH, the any-hit traversal and the ambient occlusion on the GPU (csrc/mesh_bvh.hip, gs2m_mesh_bvh.py, gs2m_mesh_ao.py) against the numpy
restatement of tests/mesh_ao_ref.py.  Everything is held to equality: the traversal's answer is defined as the brute-force
loop's, the AO count as the restatement's, and the tree's invariants are read back from the buffer.  All data is synthetic."""
import functools
import types

import numpy as np
import pytest
import torch

import gs2m_mesh_ao as AO
import gs2m_mesh_bvh as BV
import gs2m_native as N
import mesh_ao_ref as A

pytestmark = pytest.mark.gpu

INVALID = "invalid argument"


def _cuda(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


@functools.lru_cache(maxsize=None)
def _scene(name):
    v, f = A.MESHES[name]()
    return v, f, BV.build_bvh(_cuda(v, torch.float64), _cuda(f, torch.int32))


def _device_occluded(bvh, r):
    return BV.occluded(bvh, _cuda(r["origins"]), _cuda(r["dirs"]), r["tmin"], r["tmax"],
                       None if r["skip"] is None else _cuda(r["skip"], torch.int32)).cpu().numpy()


@pytest.mark.parametrize("name", list(A.MESHES))
def test_bvh_invariants_and_two_builds(name):
    v, f, bvh = _scene(name)
    lo, hi, links = bvh.nodes()
    A.check_bvh(lo, hi, links, v, f)
    again = BV.build_bvh(_cuda(v, torch.float64), _cuda(f, torch.int32))
    m = 64 * max(2 * len(f) - 1, 0)
    assert torch.equal(bvh.buffer[:m], again.buffer[:m])
    if name in ("identical257", "collinear200", "n1000"):   # ties are split by position: no chain
        assert A.depth(links, len(f)) <= 2 * int(np.ceil(np.log2(len(f)))) + (0 if name == "identical257" else 12)
    if name == "identical257":
        assert A.depth(links, 257) == 9 and links[256:, 0].tolist() == list(range(257))   # equal codes stay in triangle order
    if name == "dead100":                                   # the dead sort behind the live
        live = A.live_triangles(v, f)
        assert not live[links[99 + int(live.sum()):, 0]].any() and live[links[99:99 + int(live.sum()), 0]].all()


@pytest.mark.parametrize("name", [m for m in A.MESHES if m != "n0"])
def test_occluded_equals_the_brute_force(name):
    v, f, bvh = _scene(name)
    families = [(k, A.ray_family(k, v, f, 1000)) for k in A.FAMILIES if not (name == "n1" and k == "skip")]
    if name == "grid":
        families += [(k, A.grid_family(k, 1000)) for k in A.GRID_FAMILIES]
    for fam, r in families:
        want = A.occluded(v, f, r["origins"], r["dirs"], r["tmin"], r["tmax"], r["skip"])
        assert 0.1 <= want.mean() <= 0.9, (fam, want.mean())    # the reference alone has both outcomes
        got = _device_occluded(bvh, r)
        assert np.array_equal(got, want), (fam, np.nonzero(got != want)[0][:8])


@pytest.mark.parametrize("n_rays", [1, 63, 64, 65])
@pytest.mark.parametrize("name", ["n1", "n2", "n3", "n65", "identical257", "dead100", "grid"])
def test_occluded_ray_counts(name, n_rays):
    """the wave's tail on tiny and degenerate trees: every count with and without a skip list (the 1000 are the test above)"""
    v, f, bvh = _scene(name)
    for fam in ("random", "grazing") + (() if name == "n1" else ("skip",)):
        want, got = [], []
        for seed in range(24 if n_rays == 1 else 2):   # one ray says little: two dozen calls of one ray each
            r = A.ray_family(fam, v, f, n_rays, seed=seed)
            want.append(A.occluded(v, f, r["origins"], r["dirs"], r["tmin"], r["tmax"], r["skip"]))
            got.append(_device_occluded(bvh, r))
        want, got = np.concatenate(want), np.concatenate(got)
        assert want.any() and not want.all() and np.array_equal(got, want), fam


def test_empty_and_dead_meshes_occlude_nothing():
    o, d = _cuda(np.random.default_rng(0).random((65, 3))), _cuda(np.random.default_rng(1).standard_normal((65, 3)))
    v, f, bvh = _scene("n0")
    assert not BV.occluded(bvh, o, d).any()
    vd = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 1, 0]])
    fd = np.array([[0, 1, 2], [0, 1, 5], [-1, 0, 1]], np.int32)
    dead = BV.build_bvh(_cuda(vd), _cuda(fd))
    A.check_bvh(*dead.nodes(), vd, fd)
    assert not BV.occluded(dead, o, d).any()
    vis, ao = AO.ambient_occlusion(dead, o, d, rays=64, tables=2, radius=1.0, bias=0.0)
    assert (vis == 64).all() and (ao == 1).all()
    # a ray with a NaN misses everything, whatever the tree
    v, f, bvh = _scene("n64")
    bad = d.clone()
    bad[::2, 1] = float("nan")
    assert not BV.occluded(bvh, o, bad)[::2].any()


def _ao_case(v, f, pts, nrm, skip, K, R, radius, bias, seed=0, index0=0):
    bvh = BV.build_bvh(_cuda(v, torch.float64), _cuda(f, torch.int32))
    if radius is None:
        diag = BV.live_diagonal(bvh.vertices, bvh.triangles)
        assert diag == float(np.linalg.norm(v.max(0) - v.min(0)))
        radius_ref, bias_ref = 0.25 * diag, 1e-4 * diag
    else:
        radius_ref, bias_ref = radius, bias
    unit = BV.unit_rows(_cuda(nrm, torch.float64)).cpu().numpy()   # the caller's part of the contract, as the wrapper does it
    got, ao = AO.ambient_occlusion(bvh, _cuda(pts), _cuda(nrm), None if skip is None else _cuda(skip, torch.int32), rays=K, tables=R,
                                   radius=radius, bias=bias, seed=seed, index0=index0)
    want = A.ambient_occlusion(v, f, pts, unit, skip, AO.direction_table(K, R, seed), bias_ref, radius_ref, index0, seed)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ao.cpu().numpy(), (want / K).astype(np.float32))
    return want


@pytest.mark.parametrize("K, R, radius", [(1, 1, None), (64, 16, None), (100, 16, np.inf), (64, 1, np.inf), (100, 1, 0.3)])
def test_ao_open_box_equals_the_restatement(K, R, radius):
    v, f = A.open_box()
    rng = np.random.default_rng(K)
    pts = np.concatenate([0.05 + 0.9 * rng.random((37, 2)), np.zeros((37, 1))], 1)
    nrm = np.tile([0.0, 0.0, 1.0], (37, 1))
    want = _ao_case(v, f, pts, nrm, None, K, R, radius, None if radius is None else 1e-4)
    if K >= 64 and radius == np.inf:   # under the lid (x < 0.5) it is darker than under the opening
        assert want[pts[:, 0] < 0.4].mean() < want[pts[:, 0] > 0.6].mean()


def test_ao_height_field_with_skip_equals_the_restatement():
    v, f = A.height_field()
    assert len(f) == 500
    which = np.arange(0, 500, 7)
    pts, nrm, owner = A.face_points(v, f, which)
    nrm = np.where(nrm[:, 2:3] < 0, -nrm, nrm)
    want = _ao_case(v, f, pts, nrm, owner, 64, 16, None, None, seed=3)
    assert want.min() < 64 and want.max() > 32
    # bias 0: only the skip keeps a point's own triangle out of its rays
    assert _ao_case(v, f, pts, nrm, owner, 64, 16, 0.5, 0.0).min() > 0


def test_ao_fixed_cases_splits_and_repeats():
    table_K = 64
    plane = (np.array([[-5, -5, 0], [5, -5, 0], [5, 5, 0], [-5, 5, 0.0]]), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    rng = np.random.default_rng(4)
    pts = np.concatenate([rng.random((33, 2)) * 4 - 2, np.zeros((33, 1))], 1)
    up = np.tile([0.0, 0.0, 1.0], (33, 1))
    assert (_ao_case(*plane, pts, up, None, table_K, 16, np.inf, 1e-4) == table_K).all()     # a plane alone
    v, f = A.closed_box()
    inside = 0.1 + 0.8 * rng.random((33, 3))
    nrm = A.unit_rows(rng.standard_normal((33, 3)))
    nrm[5], nrm[6], nrm[7] = 0.0, (np.nan, 0.0, 1.0), (np.inf, 0.0, 0.0)
    skip = np.full(33, 11, np.int32)
    skip[9] = -1
    inside[11, 2] = np.nan
    want = _ao_case(v, f, inside, nrm, skip, table_K, 16, np.inf, 1e-4)
    open_ = [5, 6, 7, 9, 11]
    assert (want[open_] == table_K).all() and (np.delete(want, open_) < table_K).all()
    closed = _ao_case(v, f, inside[12:], nrm[12:], None, table_K, 16, np.inf, 1e-4)
    assert (closed == 0).all()                                                                # inside a closed box
    # two calls split at an odd point, with index0, are one call; two runs are the same bits
    bvh = BV.build_bvh(_cuda(v, torch.float64), _cuda(f, torch.int32))
    p, n, s = _cuda(inside), _cuda(nrm), _cuda(skip)
    kw = dict(rays=100, tables=16, radius=0.7, bias=1e-4, seed=9)
    whole = AO.ambient_occlusion(bvh, p, n, s, index0=1000, **kw)[0]
    a = AO.ambient_occlusion(bvh, p[:13], n[:13], s[:13], index0=1000, **kw)[0]
    b = AO.ambient_occlusion(bvh, p[13:], n[13:], s[13:], index0=1013, **kw)[0]
    assert torch.equal(torch.cat([a, b]), whole) and torch.equal(AO.ambient_occlusion(bvh, p, n, s, index0=1000, **kw)[0], whole)
    assert int(whole.min()) < int(whole.max())


def _overhang():
    """a unit quad in z = 0 and a triangle hanging over its x < 0.5 half at z = 0.2"""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [-0.2, -0.2, 0.2], [0.5, -0.2, 0.2], [-0.2, 1.6, 0.2]], np.float64)
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 6, 5]], np.int32)
    return v, f


def test_texel_and_vertex_occlusion_under_an_overhang():
    import gs2m_mesh_texture as MT
    v, f = _overhang()
    mesh = types.SimpleNamespace(vertices=_cuda(v), triangles=_cuda(f, torch.int32))
    atlas = MT.build_atlas(mesh, density=12.0)
    K = 64
    visible, owner = AO.texel_occlusion(atlas, rays=K, tables=16, radius=np.inf, bias=1e-6, seed=2, band_texels=3 * atlas.width)
    whole, _ = AO.texel_occlusion(atlas, rays=K, tables=16, radius=np.inf, bias=1e-6, seed=2)
    assert torch.equal(visible, whole)                                         # the bands do not show
    own, pts, nrm = AO.texel_points(atlas)
    assert torch.equal(own, owner)
    unit = BV.unit_rows(nrm.reshape(-1, 3)).cpu().numpy()
    want = A.ambient_occlusion(v, f, pts.reshape(-1, 3).cpu().numpy(), unit, owner.reshape(-1).cpu().numpy(), AO.direction_table(K, 16, 2),
                               1e-6, np.inf, 0, 2)
    assert np.array_equal(visible.reshape(-1).cpu().numpy(), want)
    o, p, vis = owner.cpu().numpy(), pts.cpu().numpy(), visible.cpu().numpy()
    floor = (o == 0) | (o == 1)
    under, clear = floor & (p[..., 0] < 0.1) & (p[..., 1] > 0.2) & (p[..., 1] < 0.5), floor & (p[..., 0] > 0.8)
    assert under.sum() >= 3 and clear.sum() > 5 and vis[under].max() < vis[clear].min()
    assert (vis[o < 0] == K).all() and (o < 0).any()
    values = torch.rand((atlas.height, atlas.width, 5), device="cuda")
    base, orm = MT.pack_textures(values)
    before = orm.clone()
    AO.apply_occlusion(orm, owner, visible, K)
    got = orm.cpu().numpy()
    assert np.array_equal(got, A.occlusion_bytes(before.cpu().numpy(), o, vis, K))
    assert np.array_equal(got[..., 1:], before.cpu().numpy()[..., 1:]) and (got[o < 0][:, 0] == 255).all()
    assert got[under][:, 0].max() < got[clear][:, 0].min()
    # the vertices: those of the quad under the overhang (x = 0) are darker than those beside it
    vv, ao = AO.vertex_occlusion(mesh, rays=K, tables=16, radius=np.inf, bias=1e-6)
    from gs2m_mesh_view import vertex_normals
    vn = vertex_normals(mesh.vertices, mesh.triangles)[0].cpu().numpy()
    want_v = A.ambient_occlusion(v, f, v, vn, None, AO.direction_table(K, 16, 0), 1e-6, np.inf)
    assert np.array_equal(vv.cpu().numpy(), want_v) and np.array_equal(ao.cpu().numpy(), (want_v / K).astype(np.float32))
    assert max(want_v[0], want_v[3]) < min(want_v[1], want_v[2])


def test_command_line_ao(tmp_path):
    import os
    import gs2m_mesh as M
    import gs2m_mesh_texture as MT
    import gs2m_train as Tr
    scene = tmp_path / "scene"
    Tr.export_colmap_dataset(str(scene), Tr.synthetic_scene(2000, 3, 48, 32, seed=1))
    ply = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_small.ply")
    v, f = _overhang()
    v = 1.2 * (v - [0.5, 0.5, 0.0]) + np.array([0.0, -0.8, 6.0])   # where the scene's cameras look
    M.write_mesh(tmp_path / "mesh.ply", types.SimpleNamespace(vertices=v, triangles=f, vertex_colors=np.full((len(v), 3), 0.25)))
    common = ["--ply", ply, "-s", str(scene), "--mesh", str(tmp_path / "mesh.ply"), "--density", "20", "--metallic"]
    MT.main(common + ["-o", str(tmp_path / "plain.glb")])
    MT.main(common + ["-o", str(tmp_path / "ao.glb"), "--ao", "--ao-rays", "32", "--ao-radius", "2.0"])
    plain, ao = MT.read_glb(tmp_path / "plain.glb"), MT.read_glb(tmp_path / "ao.glb")
    assert not plain["occlusion"] and ao["occlusion"] and ao["json"]["materials"][0]["occlusionTexture"] == {"index": 1}
    p0, p1 = MT.decode_png(plain["images"][1]), MT.decode_png(ao["images"][1])
    assert (p0[..., 0] == 255).all() and len(np.unique(p1[..., 0])) > 2 and np.array_equal(p0[..., 1:], p1[..., 1:])
    assert plain["images"][0] == ao["images"][0]
    # without --ao the document is the one the writer has always written: these values were fixed before the flag existed
    doc = plain["json"]
    assert doc["materials"] == [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 1.0, "roughnessFactor": 1.0,
                                                          "metallicRoughnessTexture": {"index": 1}}}]
    assert doc["textures"] == [{"sampler": 0, "source": 0}, {"sampler": 0, "source": 1}] and len(doc["images"]) == 2
    assert list(doc) == ["asset", "scene", "scenes", "nodes", "meshes", "materials", "textures", "samplers", "images", "accessors", "bufferViews",
                         "buffers"] and len(doc["accessors"]) == 4 and len(doc["bufferViews"]) == 6
    ao_doc = dict(ao["json"], materials=[{k: x for k, x in ao["json"]["materials"][0].items() if k != "occlusionTexture"}])
    ao_doc["bufferViews"], ao_doc["buffers"] = doc["bufferViews"][:5] + ao_doc["bufferViews"][5:], doc["buffers"]
    assert ao_doc["bufferViews"][5]["byteOffset"] == doc["bufferViews"][5]["byteOffset"]
    assert {k: x for k, x in ao_doc.items() if k not in ("bufferViews", "buffers")} == {k: x for k, x in doc.items() if k not in ("bufferViews", "buffers")}
    # without --ao nothing of the feature runs: the file is the one texture_mesh writes with the keyword left out
    cams, _, _, _, _ = Tr.load_colmap_dataset(str(scene), resolution=1)
    from gs2m_model import GaussianModel
    model = GaussianModel(3)
    model.load_ply(ply)
    MT.texture_mesh(model, cams, M.read_mesh(tmp_path / "mesh.ply"), tmp_path / "again.glb", density=20.0, metallic=True)
    assert (tmp_path / "again.glb").read_bytes() == (tmp_path / "plain.glb").read_bytes()
    # --rgb has no ORM image of its own: one of roughness 1, metallic 0 carries the occlusion
    MT.main(common[:-1] + ["-o", str(tmp_path / "rgb.glb"), "--rgb", "--ao", "--ao-rays", "32", "--ao-radius", "2.0"])
    rgb = MT.read_glb(tmp_path / "rgb.glb")
    px = MT.decode_png(rgb["images"][1])
    assert rgb["occlusion"] and (px[..., 1] == 255).all() and (px[..., 2] == 0).all() and np.array_equal(px[..., 0], p1[..., 0])


def test_views_of_the_occlusion_are_grey(tmp_path):
    """gs2m_mesh_view.py --colour ao: a PLY's occlusion property, one traced on the fly, and a .glb's ORM R channel, drawn unlit"""
    import gs2m_mesh as M
    import gs2m_mesh_bake as MB
    import gs2m_mesh_texture as MT
    import gs2m_mesh_view as G
    import gs2m_train as Tr
    from PIL import Image
    scene = tmp_path / "scene"
    Tr.export_colmap_dataset(str(scene), Tr.synthetic_scene(2000, 3, 48, 32, seed=1))
    v, f = _overhang()
    v = 1.2 * (v - [0.5, 0.5, 0.0]) + np.array([0.0, -0.8, 6.0])
    mesh = types.SimpleNamespace(vertices=_cuda(v), triangles=_cuda(f, torch.int32))
    ao = np.linspace(0.1, 0.9, len(v)).astype(np.float32)
    MB.write_material_mesh(tmp_path / "material.ply", v, f, np.full((len(v), 5), 0.5, np.float32), None, ao)
    M.write_mesh(tmp_path / "plain.ply", types.SimpleNamespace(vertices=v, triangles=f, vertex_colors=np.full((len(v), 3), 0.25)))
    views = G.read_colmap_views(str(scene))
    w2c = _cuda(np.stack([x["w2c"] for x in views]), torch.float64)
    k = views[0]

    def draw(args, out):
        r = G.main(args + ["-s", str(scene), "--rendering", "--colour", "ao", "--out-dir", str(tmp_path / out)])
        px = np.stack([np.asarray(Image.open(p)) for p in r["views"]])
        covered = px[..., 3] > 0
        assert covered.any() and (px[..., 0] == px[..., 1])[covered].all() and (px[..., 1] == px[..., 2])[covered].all()
        return px, covered

    # the property, as shade_views draws vertex colours with no light
    px, covered = draw(["--ply-path", str(tmp_path / "material.ply")], "a")
    col = _cuda(np.repeat(ao[:, None], 3, 1))
    want = G.shade_views(mesh.vertices, mesh.triangles, w2c, k["fx"], k["fy"], k["cx"], k["cy"], k["height"], k["width"], colors=col, ambient=1.0,
                         diffuse=0.0).cpu().numpy()
    assert np.array_equal(px, want) and len(np.unique(px[..., 0][covered])) > 3
    # no property: traced here
    px, covered = draw(["--ply-path", str(tmp_path / "plain.ply")], "b")
    traced = AO.vertex_occlusion(mesh)[1]
    want = G.shade_views(mesh.vertices, mesh.triangles, w2c, k["fx"], k["fy"], k["cx"], k["cy"], k["height"], k["width"],
                         colors=traced[:, None].expand(-1, 3).contiguous(), ambient=1.0, diffuse=0.0).cpu().numpy()
    assert np.array_equal(px, want) and float(traced.min()) < float(traced.max())
    # a .glb: the ORM's R channel; one without an occlusionTexture is refused
    atlas = MT.build_atlas(mesh, density=20.0)
    values = torch.full((atlas.height, atlas.width, 5), 0.5, device="cuda")
    base, orm = MT.pack_textures(values)
    MT.export_glb(tmp_path / "plain.glb", atlas, base, orm)
    visible, owner = AO.texel_occlusion(atlas, rays=32, radius=2.0)
    AO.apply_occlusion(orm, owner, visible, 32)
    MT.export_glb(tmp_path / "ao.glb", atlas, base, orm, occlusion=True)
    px, covered = draw(["--glb", str(tmp_path / "ao.glb")], "c")
    tex = G.read_textured_mesh(tmp_path / "ao.glb", torch.device("cuda"))
    grey = tex["orm"][..., :1].expand(-1, -1, 3).contiguous()
    want = G.shade_views_textured(tex["vertices"], tex["triangles"], tex["uvs"], w2c, k["fx"], k["fy"], k["cx"], k["cy"], k["height"], k["width"],
                                  grey, None, False, ambient=1.0, diffuse=0.0).cpu().numpy()
    assert np.array_equal(px, want) and len(np.unique(px[..., 0][covered])) > 2
    with pytest.raises(RuntimeError, match="occlusionTexture"):
        G.main(["--glb", str(tmp_path / "plain.glb"), "-s", str(scene), "--rendering", "--colour", "ao", "--out-dir", str(tmp_path / "d")])


def test_bake_and_simplify_carry_the_occlusion(tmp_path):
    """gs2m_mesh_bake.py --ao writes the vertex pass as a property; gs2m_mesh_simplify.py carries it as a sixth channel, the
    seen-weighted mean of each cell"""
    import os
    import gs2m_mesh as M
    import gs2m_mesh_bake as MB
    import gs2m_mesh_simplify as MS
    import gs2m_train as Tr
    scene = tmp_path / "scene"
    Tr.export_colmap_dataset(str(scene), Tr.synthetic_scene(2000, 3, 48, 32, seed=1))
    ply = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_small.ply")
    v, f = A.height_field()
    v = 0.8 * (v - [1.25, 0.5, 0.0]) + np.array([0.0, -0.8, 6.0])
    M.write_mesh(tmp_path / "mesh.ply", types.SimpleNamespace(vertices=v, triangles=f, vertex_colors=np.full((len(v), 3), 0.25)))
    common = ["--ply", ply, "-s", str(scene), "--mesh", str(tmp_path / "mesh.ply")]
    MB.main(common + ["-o", str(tmp_path / "plain.ply")])
    MB.main(common + ["-o", str(tmp_path / "ao.ply"), "--ao", "--ao-rays", "32", "--ao-radius", "0.5"])
    plain, ao = MB.read_material_mesh(tmp_path / "plain.ply"), MB.read_material_mesh(tmp_path / "ao.ply")
    assert "occlusion" not in plain and b"occlusion" not in (tmp_path / "plain.ply").read_bytes()[:600]
    for key in plain:
        assert np.array_equal(plain[key], ao[key]), key
    mesh = M.read_mesh(tmp_path / "mesh.ply")
    want = AO.vertex_occlusion(mesh, rays=32, radius=0.5)[1].cpu().numpy()
    assert np.array_equal(ao["occlusion"], want) and want.min() < want.max()
    # through the simplification: nine channels, the sixth of the material ones the occlusion
    loaded, values, seen = MS.load(tmp_path / "ao.ply")
    seen = (np.arange(len(seen)) % 3 != 0).astype(np.float32)       # a third unseen, so the weights matter
    out, info = M.simplify_mesh_gpu(loaded, cell=0.2, attributes=values, weights=seen)
    vmap = np.asarray(info["vertex_map"].cpu() if torch.is_tensor(info["vertex_map"]) else info["vertex_map"])
    got = np.asarray(info["attributes"].cpu() if torch.is_tensor(info["attributes"]) else info["attributes"])
    assert got.shape[1] == 6 and 0 < len(got) < len(values)
    checked = 0
    for c in range(len(got)):
        members = np.nonzero(vmap == c)[0]
        w = seen[members].astype(np.float64)
        x = values[members, 5].astype(np.float64)
        mean = (w * x).sum() / w.sum() if w.sum() > 0 else x.mean()
        assert abs(got[c, 5] - mean) <= 2.0 ** -23 * abs(mean), c   # fp64 sums rounded once to fp32
        checked += len(members) > 1
    assert checked > 10
    MB.write_material_mesh(tmp_path / "shuffled.ply", loaded.vertices, loaded.triangles, values[:, :5], seen, values[:, 5])
    r = MS.main(["--ply-path", str(tmp_path / "shuffled.ply"), "-o", str(tmp_path / "simple.ply"), "--cell", "0.2"])
    simple = MB.read_material_mesh(tmp_path / "simple.ply")
    assert r["material"] and np.array_equal(simple["occlusion"], got[:, 5]) and np.array_equal(simple["roughness"], got[:, 3])


def test_mesh_command_line_takes_ao(tmp_path):
    """gs2m_mesh.py --texture-size N --ao: tsdf_textured.glb carries the occlusion; --ao alone is refused"""
    import gs2m_mesh as M
    import gs2m_mesh_texture as MT
    import gs2m_train as Tr
    import test_mesh_gpu as TM
    from gs2m_model import GaussianModel
    Tr.export_colmap_dataset(str(tmp_path / "scene"), Tr.synthetic_scene(8000, 4, 96, 64, seed=1))
    truth, _ = TM._truth_and_cams(8000, 1, 96, 64)
    model = GaussianModel(3)
    model.parameterize((truth._xyz, truth._features_dc, truth._features_rest, truth._scaling, truth._rotation, truth._opacity,
                        truth._albedo, truth._roughness, truth._metallic))
    model.active_sh_degree = 3
    model.save_ply(str(tmp_path / "model.ply"))
    base = ["--ply", str(tmp_path / "model.ply"), "-s", str(tmp_path / "scene"), "--voxel_size", "0.16", "--texture-size", "512"]
    M.main(base + ["-o", str(tmp_path / "tex")])
    M.main(base + ["-o", str(tmp_path / "ao"), "--ao"])
    tex, ao = MT.read_glb(tmp_path / "tex" / "tsdf_textured.glb"), MT.read_glb(tmp_path / "ao" / "tsdf_textured.glb")
    assert not tex["occlusion"] and ao["occlusion"] and tex["images"][0] == ao["images"][0]
    p0, p1 = MT.decode_png(tex["images"][1]), MT.decode_png(ao["images"][1])
    assert (p0[..., 0] == 255).all() and len(np.unique(p1[..., 0])) > 2 and np.array_equal(p0[..., 1:], p1[..., 1:])
    with pytest.raises(SystemExit):
        M.main(base[:-2] + ["-o", str(tmp_path / "bad"), "--ao"])


def test_error_paths():
    v, f, bvh = _scene("n64")
    o = _cuda(np.zeros((4, 3)))
    d = _cuda(np.ones((4, 3)))
    hit = torch.zeros(4, dtype=torch.uint8, device="cuda")
    vis = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    tab = _cuda(AO.direction_table(4, 2))
    P = lambda t: None if t is None else t.data_ptr()
    tree = (P(bvh.buffer), bvh.buffer.numel(), len(bvh.vertices), P(bvh.vertices), len(bvh.triangles), P(bvh.triangles))

    def bad(name, *args):
        with pytest.raises(RuntimeError, match=INVALID):
            N.launch(name, o.device, *args)

    occ = lambda tree=tree, n=4, oo=o, dd=d, tmin=0.0, tmax=1.0, h=hit: tree + (n, P(oo), P(dd), tmin, tmax, None, P(h))
    ao = lambda tree=tree, n=4, pp=o, nn=d, R=2, K=4, t=tab, bias=0.0, radius=1.0, out=vis: tree + (n, P(pp), P(nn), None, R, K, P(t), bias,
                                                                                                   radius, 0, 0, P(out))
    N.launch("gs2m_bvh_occluded", o.device, *occ())
    N.launch("gs2m_bvh_ao", o.device, *ao())
    vis.fill_(-7)
    hit.fill_(9)
    small = (tree[0], tree[1] - 1) + tree[2:]
    for t in (small, (None,) + tree[1:], tree[:3] + (None,) + tree[4:], tree[:5] + (None,), (tree[0], tree[1], -1) + tree[3:],
              tree[:4] + (-1, tree[5])):
        bad("gs2m_bvh_occluded", *occ(tree=t))
        bad("gs2m_bvh_ao", *ao(tree=t))
        bad("gs2m_bvh_build", *(t[2:] + t[:2]))
    for kw in (dict(n=-1), dict(oo=None), dict(dd=None), dict(h=None), dict(tmin=float("nan")), dict(tmax=float("nan"))):
        bad("gs2m_bvh_occluded", *occ(**kw))
    for kw in (dict(n=-1), dict(pp=None), dict(nn=None), dict(out=None), dict(t=None), dict(K=0), dict(R=0), dict(K=-3),
               dict(bias=float("nan")), dict(radius=float("nan"))):
        bad("gs2m_bvh_ao", *ao(**kw))
    orm = torch.full((4, 3), 3, dtype=torch.uint8, device="cuda")
    own = torch.zeros(4, dtype=torch.int32, device="cuda")
    for args in ((-1, P(own), P(vis), 4, P(orm)), (4, None, P(vis), 4, P(orm)), (4, P(own), None, 4, P(orm)), (4, P(own), P(vis), 0, P(orm)),
                 (4, P(own), P(vis), 4, None)):
        bad("gs2m_texture_occlusion", *args)
    import ctypes as C
    assert N.lib().gs2m_bvh_bytes(-1, C.byref(C.c_longlong())) == -1 and N.lib().gs2m_bvh_bytes(4, None) == -1
    torch.cuda.synchronize()
    assert (vis == -7).all() and (hit == 9).all() and (orm == 3).all()   # nothing was launched
    again = BV.build_bvh(bvh.vertices, bvh.triangles)
    assert torch.equal(again.buffer[:64 * 127], bvh.buffer[:64 * 127])
