"""The restatement of the per-vertex bake (tests/mesh_bake_ref.py) checked on its own, the margins of the GPU test's scene, and the
material PLY.  No GPU."""
import numpy as np
import pytest

import mesh_bake_ref as B
import tnt_cull_ref as R


def test_an_affine_map_sampled_bilinearly_is_the_affine_value():
    H, W = 9, 13
    j, i = np.mgrid[0:H, 0:W]
    A = (0.25 + 0.5 * i - 0.125 * j).astype(np.float32)  # exact in fp32
    rng = np.random.default_rng(0)
    u, v = rng.uniform(0, W - 1, 500), rng.uniform(0, H - 1, 500)
    u[:3], v[:3] = (0.0, W - 1.0, 4.0), (H - 1.0, 0.0, 3.0)
    assert np.abs(R.bilinear(A, u, v) - (0.25 + 0.5 * u - 0.125 * v)).max() <= 1e-12


def test_each_edge_case_vertex_is_classified_as_the_contract_says():
    c = B.bake_case()
    k = {n: c[n] for n in ("fx", "fy", "cx", "cy")}
    r = B.bake_view(c["verts"], c["normals"], c["w2c"][0], **k, depth=c["depth"][0], maps=c["maps"][0], mask=c["mask"][0], eps=c["eps"])
    e = c["edge"]
    got = lambda name, key: bool(r[key][e[name]])
    assert not got("outside", "inside") and r["z"][e["outside"]] > 0
    assert not got("behind", "inside") and r["z"][e["behind"]] <= 0
    i = e["corner"]
    assert r["u"][i] == c["W"] - 1 and r["v"][i] == c["H"] - 1 and got("corner", "inside") and got("corner", "use")
    # its sample is the corner texel alone
    assert np.array_equal(r["a"][i], c["maps"][0][:, c["H"] - 1, c["W"] - 1].astype(np.float64))
    i = e["occluded"]
    assert got("occluded", "inside") and r["d"][i] > 0 and r["z"][i] > r["d"][i] + c["eps"] and not got("occluded", "front") and not got("occluded", "use")
    assert got("depth0", "inside") and r["d"][e["depth0"]] == 0 and got("depth0", "front") and got("depth0", "use")
    assert got("backfacing", "inside") and got("backfacing", "front") and not got("backfacing", "lit") and not got("backfacing", "use")
    assert got("grazing", "inside") and got("grazing", "front") and r["w"][e["grazing"]] == 0 and not got("grazing", "use")
    i = e["masked_zero_weight"]
    x0, y0 = int(r["u"][i]), int(np.floor(r["v"][i]))
    assert r["u"][i] == x0 and (c["mask"][0, y0:y0 + 2, x0 + 1] == 0).all() and got("masked_zero_weight", "unmasked") and got("masked_zero_weight", "use")
    i = e["masked_tap"]
    x0, y0 = int(np.floor(r["u"][i])), int(np.floor(r["v"][i]))
    assert c["mask"][0, y0, x0] == 0 and r["u"][i] > x0 and r["v"][i] > y0 and got("masked_tap", "inside") and got("masked_tap", "front")
    assert not got("masked_tap", "unmasked") and not got("masked_tap", "use")


def test_the_scene_has_about_300_vertices_and_every_kind_of_view():
    c = B.bake_case()
    assert 290 <= len(c["verts"]) <= 320 and c["w2c"].shape == (3, 4, 4) and c["maps"].shape == (3, 5, 16, 24)
    _, weights, use, _ = B.bake_reference(5)
    assert use.any(axis=0).all() and 0.25 < use.mean() < 0.95  # every view contributes, and none to every vertex
    # the occluder hides about a third of the patch's vertices from view 0
    r = B.bake_view(c["verts"][:144], None, c["w2c"][0], c["fx"], c["fy"], c["cx"], c["cy"], c["depth"][0], c["maps"][0])
    assert r["inside"].all() and 30 <= (~r["front"]).sum() <= 70
    assert (weights > 0).sum() > 150


@pytest.mark.parametrize("channels,masked,with_normals", [(5, True, True), (1, True, True), (5, False, True), (5, True, False)])
def test_no_decision_of_the_gpu_scene_lies_near_its_threshold(channels, masked, with_normals):
    """the two sides can then differ only in rounding, never in a decision (an exact hit, distance 0, is the same exact value on
    both sides)"""
    _, _, _, margin = B.bake_reference(channels, masked, with_normals)
    assert margin.min() >= B.MARGIN, margin.min()


def test_split_accumulation_gives_the_same_bits_in_the_restatement():
    c = B.bake_case()
    k = [c[n] for n in ("fx", "fy", "cx", "cy")]
    s, w, _, _ = B.bake_reference(5)
    s1, w1, _, _ = B.accumulate(c["verts"], c["normals"], c["w2c"][:1], *k, c["depth"][:1], c["maps"][:1], c["mask"][:1], c["eps"])
    s2, w2, _, _ = B.accumulate(c["verts"], c["normals"], c["w2c"][1:], *k, c["depth"][1:], c["maps"][1:], c["mask"][1:], c["eps"], s1, w1)
    assert np.array_equal(s, s2) and np.array_equal(w, w2)


def test_material_ply_round_trip(tmp_path):
    import gs2m_mesh as M
    import gs2m_mesh_bake as MB
    rng = np.random.default_rng(4)
    v = rng.normal(size=(37, 3)).astype(np.float32)
    t = rng.integers(0, 37, (50, 3)).astype(np.int32)
    values = rng.random((37, 5)).astype(np.float32)
    values[0, :3], values[1, :3] = (0.0, 1.0, 0.5), (1.5, -0.2, 127.5 / 255.0)  # clipped; a tie goes to even, as write_mesh rounds
    seen = rng.random(37) > 0.3
    path = tmp_path / "m.ply"
    MB.write_material_mesh(path, v, t, values, seen)
    back = MB.read_material_mesh(path)
    want = np.clip(np.rint(values[:, :3].astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    assert np.array_equal(back["vertices"], v) and np.array_equal(back["triangles"], t)
    assert np.array_equal(back["roughness"], values[:, 3]) and np.array_equal(back["metallic"], values[:, 4])
    assert np.array_equal(back["seen"], seen) and np.array_equal(back["albedo"], want.astype(np.float32) / 255.0)
    assert tuple(want[1]) == (255, 0, 128)
    mesh = M.read_mesh(path)  # the existing reader: the albedo as vertex colours
    assert np.array_equal(mesh.vertices, v) and np.array_equal(mesh.triangles, t)
    assert np.array_equal(mesh.vertex_colors, want.astype(np.float32) / 255.0)
    # a plain mesh is refused with the absent properties named
    import types
    M.write_mesh(tmp_path / "plain.ply", types.SimpleNamespace(vertices=v, triangles=t, vertex_colors=values[:, :3]))
    with pytest.raises(ValueError, match="roughness, metallic"):
        MB.read_material_mesh(tmp_path / "plain.ply")


def test_resolve_of_the_restatement():
    sums = np.array([[2.0, 4.0], [1.0, 1.0], [0.0, 0.0], [3e-4, 3e-4]])
    weights = np.array([2.0, 1e-3, 0.0, 5e-4])
    out, seen = B.resolve(sums, weights, 1e-3, (9.0, 8.0))
    assert seen.tolist() == [True, True, False, False]
    assert np.array_equal(out, np.array([[1.0, 2.0], [1000.0, 1000.0], [9.0, 8.0], [9.0, 8.0]], np.float32))
    out, seen = B.resolve(sums, weights, 0.0, (9.0, 8.0))  # min_weight 0: a weight of 0 is still not seen
    assert seen.tolist() == [True, True, False, True]
