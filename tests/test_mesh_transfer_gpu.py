"""The closest-hit query and the detail transfer on the GPU (csrc/mesh_bvh.hip, gs2m_mesh_bvh.closest, gs2m_mesh_transfer.py) against
the numpy restatement of tests/mesh_transfer_ref.py.  Everything is held to equality with no exception budget: the traversal's
answer is defined as the brute-force loop's in all four outputs, the transfer's as the restatement's.  All data is synthetic."""
import functools
import types

import numpy as np
import pytest
import torch

import gs2m_mesh_bvh as BV
import gs2m_mesh_transfer as T
import gs2m_native as N
import mesh_ao_ref as A
import mesh_transfer_ref as R
from test_mesh_ao_gpu import INVALID, _cuda, _overhang

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _scene(name):
    v, f = R.layered_grid() if name == "layered" else A.MESHES[name]()
    return v, f, BV.build_bvh(_cuda(v, torch.float64), _cuda(f, torch.int32))


def _device_closest(bvh, r, skip=None, facing=0):
    got = BV.closest(bvh, _cuda(r["origins"]), _cuda(r["dirs"]), r["tmin"], r["tmax"], None if skip is None else _cuda(skip, torch.int32), facing)
    return tuple(x.cpu().numpy() for x in got)


def _same(got, want, what):
    for k, name in enumerate(("tri", "t", "uv")):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, name, np.nonzero(got[k] != want[k])[0][:8])


@pytest.mark.parametrize("name", list(A.MESHES))
def test_closest_equals_the_brute_force(name):
    v, f, bvh = _scene(name)
    if name == "n0":
        rng = np.random.default_rng(0)
        r = dict(origins=rng.random((65, 3)), dirs=rng.standard_normal((65, 3)), tmin=0.0, tmax=np.inf)
        for facing in (0, 1, -1):
            _same(_device_closest(bvh, r, None, facing), R.closest(v, f, r["origins"], r["dirs"], facing=facing), facing)
        return
    rays, tables, cases = {}, {}, 0
    for facing in (0, 1, -1):
        for with_skip in (False, True):
            for fam in R.BALANCED.get((name, facing, with_skip), ()):
                if fam not in rays:
                    rays[fam] = r = A.grid_family(fam, 1000) if fam in A.GRID_FAMILIES else A.ray_family(fam, v, f, 1000)
                    tables[fam] = R.triangle_table(v, f, r["origins"], r["dirs"], r["tmin"], r["tmax"])
                r, (ok, t, u, w, det) = rays[fam], tables[fam]
                skip = R.nearest_skip(r, R.answer(ok, t, u, w)[0]) if with_skip else None
                want = R.answer(R.select(ok, det, skip, facing), t, u, w)
                assert 0.1 <= (want[0] >= 0).mean() <= 0.9, (fam, facing, with_skip)   # the reference alone has both outcomes
                _same(_device_closest(bvh, r, skip, facing), want, (fam, facing, with_skip))
                cases += 1
    assert cases == sum(len(fams) for key, fams in R.BALANCED.items() if key[0] == name) >= 18


@pytest.mark.parametrize("n_rays", [1, 63, 64, 65])
@pytest.mark.parametrize("name", ["n1", "n2", "n3", "n65", "identical257", "dead100", "grid"])
def test_closest_ray_counts(name, n_rays):
    """the wave's tail on tiny and degenerate trees: every count with and without a skip list (the 1000 are the test above)"""
    v, f, bvh = _scene(name)
    for fam in ("random", "grazing") + (() if name == "n1" else ("skip",)):
        want, got = [], []
        for seed in range(24 if n_rays == 1 else 2):   # one ray says little: two dozen calls of one ray each
            r = A.ray_family(fam, v, f, n_rays, seed=seed)
            want.append(R.closest(v, f, r["origins"], r["dirs"], r["tmin"], r["tmax"], r["skip"])[:3])
            got.append(_device_closest(bvh, r, r["skip"]))
        want, got = [np.concatenate(x) for x in zip(*want)], [np.concatenate(x) for x in zip(*got)]
        assert (want[0] >= 0).any() and not (want[0] >= 0).all(), fam
        _same(got, want, fam)


def test_ties_take_the_smaller_index():
    """dyadic axis-aligned rays onto the lattice vertices and edges of the grid, and onto two coplanar layers of it: at least 100
    rays whose best t two or more candidates share, and the device returns the smaller index on each"""
    for name in ("grid", "layered"):
        v, f, bvh = _scene(name)
        r = R.tie_family(1000)
        for facing in (0, 1, -1):
            want = R.closest(v, f, r["origins"], r["dirs"], facing=facing)
            if facing == 0:
                assert (want[3] >= 2).sum() >= 100 and 0.1 <= (want[0] >= 0).mean() <= 0.9
                if name == "layered":
                    assert (want[3][want[0] >= 0] >= 2).all() and (want[0] < len(f) // 2).all()
            _same(_device_closest(bvh, r, None, facing), want, (name, facing))
            tied = want[3] >= 2
            assert np.array_equal(_device_closest(bvh, r, None, facing)[0][tied], want[0][tied])
        # with the winner skipped the next index of the tie takes over
        want = R.closest(v, f, r["origins"], r["dirs"])
        second = R.closest(v, f, r["origins"], r["dirs"], skip=want[0])
        assert (second[0][want[3] >= 2] > want[0][want[3] >= 2]).all() and np.array_equal(second[1][want[3] >= 2], want[1][want[3] >= 2])
        _same(_device_closest(bvh, r, want[0]), second, name)


def test_nan_rays_and_dead_meshes_find_nothing():
    rng = np.random.default_rng(0)
    o, d = rng.random((65, 3)), rng.standard_normal((65, 3))
    vd = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 1, 0]])
    fd = np.array([[0, 1, 2], [0, 1, 5], [-1, 0, 1]], np.int32)
    dead = BV.build_bvh(_cuda(vd), _cuda(fd))
    tri, t, uv = BV.closest(dead, _cuda(o), _cuda(d))
    assert (tri == -1).all() and torch.isposinf(t).all() and (uv == 0).all()
    v, f, bvh = _scene("n64")
    bad = d.copy()
    bad[::2, 1] = np.nan
    tri, t, uv = BV.closest(bvh, _cuda(o), _cuda(bad))
    assert (tri[::2] == -1).all() and torch.isposinf(t[::2]).all() and (uv[::2] == 0).all()
    _same((tri.cpu().numpy(), t.cpu().numpy(), uv.cpu().numpy()), R.closest(v, f, o, bad), "nan")


# ---- transfer ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _transfer_scene():
    import gs2m_mesh_texture as MT
    from gs2m_mesh_view import vertex_normals
    v, f = A.height_field()
    assert len(f) == 500
    lv, lf = R.tilted_plane()
    atlas = MT.build_atlas(types.SimpleNamespace(vertices=_cuda(lv), triangles=_cuda(lf, torch.int32)), density=12.0)
    owner, points, normals = (x.cpu().numpy() for x in T.texel_rays(atlas))
    rng = np.random.default_rng(5)
    att = rng.random((len(v), 5)).astype(np.float32)
    low = rng.random((len(lv), 5)).astype(np.float32)
    sn = vertex_normals(_cuda(v), _cuda(f, torch.int32))[0].cpu().numpy()
    return dict(v=v, f=f, atlas=atlas, owner=owner.reshape(-1), points=points.reshape(-1, 3), normals=normals.reshape(-1, 3), att=att, low=low, sn=sn)


def _mesh(v, f):
    return types.SimpleNamespace(vertices=v, triangles=f)


def _flat(x):
    x = x.cpu().numpy()
    return x.reshape(-1, x.shape[-1]) if x.ndim == 3 else x.reshape(-1)


def test_transfer_texels_equal_the_restatement():
    s = _transfer_scene()
    a, D = s["atlas"], R.TRANSFER_DISTANCE
    owned = s["owner"] >= 0
    assert a.width * a.height <= 20000 and owned.sum() >= 150
    # the texel normals are the interpolated vertex normals (sums in units of 2^-32), unit: here the plane's
    assert np.abs(s["normals"][owned] - A.unit_rows(np.array([-R.TRANSFER_SLOPE, 0.0, 1.0]))).max() <= 1e-8
    assert np.abs(np.sqrt(A.dot(s["normals"][owned], s["normals"][owned])) - 1.0).max() <= 1e-15
    fill = np.concatenate([_flat(T._fill(a, 5, _cuda(s["low"]))), np.zeros((a.width * a.height, 3), np.float32)], 1)
    want = R.transfer(s["v"], s["f"], s["points"], s["normals"], s["owner"], D, False, fill, s["att"], s["sn"], True)
    counts = np.bincount(want[3][owned], minlength=4)
    assert counts[0] == 0 and (counts[1:] >= 0.1 * owned.sum()).all(), counts          # forward, backward and miss: a tenth each
    values, hit, offset = T.transfer_texels(a, _mesh(s["v"], s["f"]), s["att"], distance=D, normal=True, attributes=s["low"])
    assert values.shape == (a.height, a.width, 8) and values.dtype == torch.float32 and hit.dtype == torch.int32 and offset.dtype == torch.float64
    assert np.array_equal(_flat(hit), want[1]) and np.array_equal(_flat(offset), want[2]) and np.array_equal(_flat(values), want[0])
    # missed and unowned texels keep the pre-filled row: the low mesh's own values interpolated, the fallback, a zero normal
    kept = want[1] < 0
    assert np.array_equal(_flat(values)[kept], fill[kept]) and (offset.reshape(-1).cpu().numpy()[kept] == 0).all()
    assert (fill[~owned, :5] == np.array(T.FALLBACK, np.float32)).all() and (fill[owned & kept, :5] != np.array(T.FALLBACK, np.float32)).any()
    assert (np.sign(want[2][want[3] == 2]) >= 0).all() and (want[2][want[3] == 3] <= 0).all() and np.abs(want[2]).max() <= D
    # bands of three rows, one call and a second run: the same bits
    for kw in (dict(band_texels=3 * a.width), dict(), dict(bvh=BV.build_bvh(_cuda(s["v"]), _cuda(s["f"], torch.int32)))):
        again = T.transfer_texels(a, _mesh(s["v"], s["f"]), s["att"], distance=D, normal=True, attributes=s["low"], **kw)
        assert all(torch.equal(x, y) for x, y in zip(again, (values, hit, offset)))
    # face normals, no attributes: three planes, cross(e1, e2) of the hit triangle
    flat = T.transfer_texels(a, _mesh(s["v"], s["f"]), None, distance=D, normal=True, smooth=False)
    want_flat = R.transfer(s["v"], s["f"], s["points"], s["normals"], s["owner"], D, False, np.zeros((len(owned), 3), np.float32), None, None, True)
    assert flat[0].shape == (a.height, a.width, 3) and np.array_equal(_flat(flat[0]), want_flat[0]) and np.array_equal(_flat(flat[1]), want[1])
    assert (want_flat[0][want[1] >= 0][:, 2] > 0).all()
    # attributes alone, and the default distance: 0.02 of the low mesh's diagonal
    lv = R.tilted_plane()[0]
    default = 0.02 * BV.live_diagonal(a.vertices, a.triangles)
    assert abs(default - 0.02 * float(np.linalg.norm(lv.max(0) - lv.min(0)))) <= 1e-15
    only = T.transfer_texels(a, _mesh(s["v"], s["f"]), s["att"], attributes=s["low"])
    want_only = R.transfer(s["v"], s["f"], s["points"], s["normals"], s["owner"], default, False, fill[:, :5], s["att"])
    assert np.array_equal(_flat(only[0]), want_only[0]) and np.array_equal(_flat(only[1]), want_only[1]) and np.array_equal(_flat(only[2]), want_only[2])
    with pytest.raises(RuntimeError, match="nothing to transfer"):
        T.transfer_texels(a, _mesh(s["v"], s["f"]), None)


def test_transfer_two_sided_against_a_half_flipped_source():
    s = _transfer_scene()
    a, D = s["atlas"], R.TRANSFER_DISTANCE
    half = R.half_flipped(s["f"])
    fill = np.zeros((a.width * a.height, 8), np.float32)
    fill[:, :5] = _flat(T._fill(a, 5, None))
    got, want = {}, {}
    for two in (False, True):
        got[two] = T.transfer_texels(a, _mesh(s["v"], half), s["att"], distance=D, two_sided=two, normal=True, smooth=False)
        want[two] = R.transfer(s["v"], half, s["points"], s["normals"], s["owner"], D, two, fill, s["att"], None, True)
        assert np.array_equal(_flat(got[two][0]), want[two][0]) and np.array_equal(_flat(got[two][1]), want[two][1])
        assert np.array_equal(_flat(got[two][2]), want[two][2])
    assert not torch.equal(got[False][1], got[True][1]) and int((got[True][1] >= 0).sum()) > int((got[False][1] >= 0).sum())
    flipped = np.zeros(len(half), bool)
    flipped[::2] = True
    hit1, hit2 = want[False][1], want[True][1]
    assert not flipped[hit1[hit1 >= 0]].any() and flipped[hit2[hit2 >= 0]].any()
    assert (want[True][0][hit2 >= 0][:, 7][flipped[hit2[hit2 >= 0]]] < 0).all()      # a flipped triangle's cross(e1, e2) points down


def test_transfer_points_stride_owner_and_splits():
    """the entry point on loose points: a stride beyond the columns it writes, no owner list, skipped points, and a split of the
    points over two calls"""
    s = _transfer_scene()
    pts, nrm = R.tilted_plane_samples(601)
    nrm[7], nrm[8, 0], pts[9, 2], pts[10, 1] = 0.0, np.nan, np.nan, np.inf
    owner = np.zeros(601, np.int32)
    owner[11::50] = -1
    bvh = BV.build_bvh(_cuda(s["v"]), _cuda(s["f"], torch.int32))
    fill = np.random.default_rng(1).random((601, 11)).astype(np.float32)
    kw = dict(distance=R.TRANSFER_DISTANCE, source_values=_cuda(s["att"]), source_normals=_cuda(s["sn"]), normal=True)
    for own in (owner, None):
        want = R.transfer(s["v"], s["f"], pts, nrm, own, R.TRANSFER_DISTANCE, False, fill, s["att"], s["sn"], True)
        assert (np.bincount(want[3], minlength=4) >= (4 if own is None else 10)).all()
        values = _cuda(fill)
        hit, offset = T.transfer(bvh, _cuda(pts), _cuda(nrm), values, None if own is None else _cuda(own), **kw)
        assert np.array_equal(values.cpu().numpy(), want[0]) and np.array_equal(hit.cpu().numpy(), want[1]) and np.array_equal(offset.cpu().numpy(), want[2])
        assert np.array_equal(want[0][:, 8:], fill[:, 8:]) and np.array_equal(want[0][want[1] < 0], fill[want[1] < 0])
        parts = _cuda(fill)
        h1, o1 = T.transfer(bvh, _cuda(pts[:333]), _cuda(nrm[:333]), parts[:333], None if own is None else _cuda(own[:333]), **kw)
        h2, o2 = T.transfer(bvh, _cuda(pts[333:]), _cuda(nrm[333:]), parts[333:], None if own is None else _cuda(own[333:]), **kw)
        assert torch.equal(parts, values) and torch.equal(torch.cat([h1, h2]), hit) and torch.equal(torch.cat([o1, o2]), offset)
    # a source without a triangle: every point misses
    empty = BV.build_bvh(_cuda(s["v"]), _cuda(s["f"][:0], torch.int32))
    values = _cuda(fill)
    hit, offset = T.transfer(empty, _cuda(pts), _cuda(nrm), values, None, distance=1.0, normal=True)
    assert (hit == -1).all() and (offset == 0).all() and np.array_equal(values.cpu().numpy(), fill)


# ---- command lines ------------------------------------------------------------------------------------------------------------------

def _strip(x0, x1, y0, y1, z, n=4):
    """2 n n triangles of the rectangle [x0, x1] x [y0, y1] at height z, wound to +z"""
    x, y = np.meshgrid(x0 + (x1 - x0) * np.arange(n + 1) / n, y0 + (y1 - y0) * np.arange(n + 1) / n, indexing="ij")
    v = np.stack([x, y, np.full_like(x, z)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    q = (i * (n + 1) + j).reshape(-1)
    return v, np.concatenate([np.stack([q, q + n + 1, q + 1], 1), np.stack([q + 1, q + n + 1, q + n + 2], 1)]).astype(np.int32)


def test_command_line_transfer(tmp_path):
    import gs2m_mesh as M
    import gs2m_mesh_bake as MB
    import gs2m_mesh_texture as MT
    lv, lf = _overhang()
    sv, sf = _strip(-0.5, 1.5, -0.5, 0.5, 0.01)                  # the source covers the y < 0.5 half of the quad, just above it
    low_values = np.tile(np.array([0.8, 0.8, 0.8, 1.0, 0.0], np.float32), (len(lv), 1))
    src_values = np.tile(np.array([0.2, 0.4, 0.6, 0.25, 0.75], np.float32), (len(sv), 1))
    MB.write_material_mesh(tmp_path / "low.ply", lv, lf, low_values)
    MB.write_material_mesh(tmp_path / "high.ply", sv, sf, src_values, None, np.full(len(sv), 0.5, np.float32))   # its occlusion is not carried
    common = ["--mesh", str(tmp_path / "low.ply"), "--source", str(tmp_path / "high.ply"), "--density", "20", "--distance", "0.05", "--linear"]
    r = T.main(common + ["-o", str(tmp_path / "a.glb")])
    g = MT.read_glb(tmp_path / "a.glb")
    assert len(g["images"]) == 2 and g["normal_image"] is None and g["tangents"] is None and not g["occlusion"]
    base, orm = MT.decode_png(g["images"][0]), MT.decode_png(g["images"][1])
    # what the tool saw: the meshes as the files hold them
    low, _ = MT.read_source_mesh(tmp_path / "low.ply")
    atlas = MT.build_atlas(low, density=20.0)
    owner, points, _ = (x.cpu().numpy() for x in T.texel_rays(atlas))
    _, hit, offset = T.transfer_texels(atlas, MT.read_source_mesh(tmp_path / "high.ply")[0], src_values, distance=0.05)
    hit, offset = hit.cpu().numpy(), offset.cpu().numpy()
    floor = (owner == 0) | (owner == 1)
    under, beside = floor & (points[..., 1] < 0.45), floor & (points[..., 1] > 0.55)
    assert under.sum() > 20 and beside.sum() > 20 and (hit[under] >= 0).all() and (hit[beside] < 0).all() and (hit[owner == 2] < 0).all()
    assert (base[hit >= 0] == [51, 102, 153]).all() and (base[(hit < 0) & (owner >= 0)] == 204).all() and (base[owner < 0] == 128).all()
    assert (orm[hit >= 0][:, 1:] == [64, 191]).all() and (orm[(hit < 0) & (owner >= 0)][:, 1:] == [255, 0]).all() and (orm[..., 0] == 255).all()
    assert r["n_hit"] == int((hit >= 0).sum()) and r["n_owned"] == int((owner >= 0).sum()) and 0.1 < r["hit_share"] < 0.9
    assert r["max_offset"] == float(np.abs(offset).max()) and abs(r["max_offset"] - 0.01) < 1e-6 and r["distance"] == 0.05
    # --normal-map: a normalTexture and tangents; flat over a flat source, so every texel encodes +z
    T.main(common + ["-o", str(tmp_path / "n.glb"), "--normal-map", "--flat-normals", "--textures-dir", str(tmp_path / "tex")])
    n = MT.read_glb(tmp_path / "n.glb")
    assert "normalTexture" in n["json"]["materials"][0] and "TANGENT" in n["json"]["meshes"][0]["primitives"][0]["attributes"]
    assert n["tangents"] is not None and n["images"] == g["images"] and sorted(p.name for p in (tmp_path / "tex").iterdir()) == [
        "base_color.png", "metallic_roughness.png", "normal.png"]
    px = MT.decode_png(n["normal_image"])
    assert np.abs(px[floor].astype(int) - [128, 128, 255]).max() <= 1
    # --ao on the low mesh, as gs2m_mesh_texture.py traces it; a coloured PLY without materials gives a base colour only
    T.main(common + ["-o", str(tmp_path / "ao.glb"), "--ao", "--ao-rays", "32", "--ao-radius", "2.0"])
    ao = MT.read_glb(tmp_path / "ao.glb")
    p1 = MT.decode_png(ao["images"][1])
    assert ao["occlusion"] and ao["images"][0] == g["images"][0] and np.array_equal(p1[..., 1:], orm[..., 1:]) and len(np.unique(p1[..., 0])) > 2
    M.write_mesh(tmp_path / "plain.ply", types.SimpleNamespace(vertices=sv, triangles=sf, vertex_colors=np.full((len(sv), 3), 0.2)))
    T.main(common[:2] + ["--source", str(tmp_path / "plain.ply")] + common[4:] + ["-o", str(tmp_path / "c.glb")])
    c = MT.read_glb(tmp_path / "c.glb")
    assert len(c["images"]) == 1 and (MT.decode_png(c["images"][0])[hit >= 0] == 51).all()


def test_texture_tool_takes_its_normal_map_from_a_source_mesh(tmp_path):
    import os
    import gs2m_mesh as M
    import gs2m_mesh_texture as MT
    import gs2m_train as Tr
    from gs2m_model import GaussianModel
    scene = tmp_path / "scene"
    Tr.export_colmap_dataset(str(scene), Tr.synthetic_scene(2000, 3, 48, 32, seed=1))
    ply = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_small.ply")
    place = lambda v: 1.2 * (v - [0.5, 0.5, 0.0]) + np.array([0.0, -0.8, 6.0])   # where the scene's cameras look
    lv, lf = _overhang()
    sv, sf = _strip(-0.5, 1.5, -0.5, 1.5, 0.01, n=6)
    sv[:, 2] += 0.01 * np.sin(9.0 * sv[:, 0]) * np.cos(7.0 * sv[:, 1])            # ripples the quad does not have
    M.write_mesh(tmp_path / "mesh.ply", types.SimpleNamespace(vertices=place(lv), triangles=lf, vertex_colors=np.full((len(lv), 3), 0.25)))
    M.write_mesh(tmp_path / "high.ply", types.SimpleNamespace(vertices=place(sv), triangles=sf, vertex_colors=np.full((len(sv), 3), 0.25)))
    common = ["--ply", ply, "-s", str(scene), "--mesh", str(tmp_path / "mesh.ply"), "--density", "20", "--metallic"]
    MT.main(common + ["-o", str(tmp_path / "plain.glb")])
    MT.main(common + ["-o", str(tmp_path / "views.glb"), "--normal-map"])
    MT.main(common + ["-o", str(tmp_path / "source.glb"), "--normal-map-from", str(tmp_path / "high.ply")])
    with pytest.raises(SystemExit):
        MT.main(common + ["-o", str(tmp_path / "both.glb"), "--normal-map", "--normal-map-from", str(tmp_path / "high.ply")])
    plain, views, source = (MT.read_glb(tmp_path / k) for k in ("plain.glb", "views.glb", "source.glb"))
    assert plain["normal_image"] is None and source["normal_image"] is not None and source["tangents"] is not None
    assert source["images"] == plain["images"]                                    # the colour bake is the views', unchanged
    a, b = MT.decode_png(source["normal_image"]), MT.decode_png(views["normal_image"])
    assert a.shape == b.shape and not np.array_equal(a, b) and len(np.unique(a.reshape(-1, 3), axis=0)) > 3
    assert np.array_equal(source["tangents"], views["tangents"])
    # without the flag nothing of the feature runs: the file is the one texture_mesh writes with the keyword left out
    cams, _, _, _, _ = Tr.load_colmap_dataset(str(scene), resolution=1)
    model = GaussianModel(3)
    model.load_ply(ply)
    MT.texture_mesh(model, cams, M.read_mesh(tmp_path / "mesh.ply"), tmp_path / "again.glb", density=20.0, metallic=True)
    assert (tmp_path / "again.glb").read_bytes() == (tmp_path / "plain.glb").read_bytes()
    with pytest.raises(ValueError):
        MT.texture_mesh(model, cams, M.read_mesh(tmp_path / "mesh.ply"), tmp_path / "bad.glb", density=20.0, normal_map=True,
                        normal_source=M.read_mesh(tmp_path / "high.ply"))


# ---- errors ---------------------------------------------------------------------------------------------------------------------------

def test_error_paths():
    v, f, bvh = _scene("n64")
    o, d = _cuda(np.zeros((4, 3))), _cuda(np.ones((4, 3)))
    tri = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    t = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    uv = torch.full((4, 2), -7.0, dtype=torch.float64, device="cuda")
    values = torch.full((4, 8), -7.0, dtype=torch.float32, device="cuda")
    hit = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    off = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    att = torch.zeros((len(v), 5), dtype=torch.float32, device="cuda")
    sn = torch.ones((len(v), 3), dtype=torch.float64, device="cuda")
    P = lambda x: None if x is None else x.data_ptr()
    tree = (P(bvh.buffer), bvh.buffer.numel(), len(bvh.vertices), P(bvh.vertices), len(bvh.triangles), P(bvh.triangles))

    def bad(name, *args):
        with pytest.raises(RuntimeError, match=INVALID):
            N.launch(name, o.device, *args)

    clo = lambda tree=tree, n=4, oo=o, dd=d, tmin=0.0, tmax=1.0, facing=0, a=tri, b=t, c=uv: tree + (n, P(oo), P(dd), tmin, tmax, None, facing,
                                                                                                  P(a), P(b), P(c))
    tra = lambda tree=tree, n=4, pp=o, nn=d, dist=1.0, ch=5, at=att, nr=sn, wn=1, stride=8, val=values, h=hit, of=off: tree + (
        n, P(pp), P(nn), None, dist, 0, ch, P(at), P(nr), wn, stride, P(val), P(h), P(of))
    # the calls as they stand are valid, and so are a missing offset, missing source normals and no channel at all
    N.launch("gs2m_bvh_closest", o.device, *clo())
    N.launch("gs2m_mesh_transfer", o.device, *tra())
    N.launch("gs2m_mesh_transfer", o.device, *tra(of=None, nr=None))
    N.launch("gs2m_mesh_transfer", o.device, *tra(ch=0, at=None, wn=0, stride=0, val=None))
    torch.cuda.synchronize()
    for x in (tri, t, uv, values, hit, off):
        x.fill_(-7)
    small = (tree[0], tree[1] - 1) + tree[2:]
    for tr in (small, (None,) + tree[1:], tree[:3] + (None,) + tree[4:], tree[:5] + (None,), (tree[0], tree[1], -1) + tree[3:],
               tree[:4] + (-1, tree[5])):
        bad("gs2m_bvh_closest", *clo(tree=tr))
        bad("gs2m_mesh_transfer", *tra(tree=tr))
    for kw in (dict(n=-1), dict(oo=None), dict(dd=None), dict(a=None), dict(b=None), dict(c=None), dict(tmin=float("nan")),
               dict(tmax=float("nan")), dict(facing=2), dict(facing=-2), dict(facing=7)):
        bad("gs2m_bvh_closest", *clo(**kw))
    for kw in (dict(n=-1), dict(pp=None), dict(nn=None), dict(val=None), dict(h=None), dict(dist=float("nan")), dict(dist=-1.0),
               dict(dist=-float("inf")), dict(ch=-1), dict(at=None), dict(stride=7), dict(ch=6, stride=8), dict(ch=0, at=None, stride=2)):
        bad("gs2m_mesh_transfer", *tra(**kw))
    torch.cuda.synchronize()
    for x in (tri, t, uv, values, hit, off):
        assert (x == -7).all()                                                     # nothing was launched
    again = BV.build_bvh(bvh.vertices, bvh.triangles)
    assert torch.equal(again.buffer[:64 * 127], bvh.buffer[:64 * 127])
    # the wrappers' own checks
    with pytest.raises(RuntimeError, match="no CPU path"):
        BV.closest(bvh, torch.zeros(4, 3, dtype=torch.float64), d)
    with pytest.raises(RuntimeError, match="3 origins for 4"):
        BV.closest(bvh, o[:3], d)
    with pytest.raises(RuntimeError, match="float32"):
        T.transfer(bvh, o, d, values.double(), distance=1.0, normal=True)
