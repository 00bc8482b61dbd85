"""csrc/mesh_depth.hip through gs2m_mesh_cull.py against the float64 restatement tests/tnt_cull_ref.py: the depth
rasterizer pixel by pixel on every path (a lane, a wave, a row of workgroups), exact ties, triangle-order independence, refused
indices; the votes vertex by vertex, accumulation, the min_views rule; the cull end to end, the command line and the evaluator's
--visibility-cull.  All data is synthetic."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tnt_cull_ref as R  # noqa: E402
import gs2m_mesh_cull as K  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


def _render(c, tris=None, views=None):
    w2c = c["w2c"] if views is None else c["w2c"][views]
    return K.render_mesh_depth(_dev(c["verts"], torch.float64), _dev(c["tris"] if tris is None else tris, torch.int32),
                               _dev(w2c, torch.float64), c["fx"], c["fy"], c["cx"], c["cy"], c["H"], c["W"], c["near"], c["far"]).cpu().numpy()


def _ulps(a, b):
    """the distance of positive float32 values in units of the last place"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("name", sorted(R.depth_cases()))
def test_depth_matches_the_restatement(name):
    """every decided pixel: empty exactly where the restatement is, else within 1 fp32 ulp of its value (both are roundings of
    fp64 values that differ far below half an ulp)"""
    c = R.depth_cases()[name]
    want, und = R.depth_reference(name)
    got = _render(c)
    assert got.shape == want.shape and got.dtype == np.float32
    ok = ~und
    print(name, "pixels", got.size, "covered", int((want > 0).sum()), "undecided", int(und.sum()),
          "largest ulp distance", int(_ulps(got, want)[ok & (want > 0) & (got > 0)].max(initial=0)))
    assert np.array_equal((got > 0)[ok], (want > 0)[ok]), np.argwhere(ok & ((got > 0) != (want > 0)))[:10]
    both = ok & (want > 0)
    assert (_ulps(got, want)[both] <= 1).all()
    assert (got[got > 0] >= np.float32(c["near"])).all() and (got <= np.float32(c["far"])).all()


def test_views_of_a_call_do_not_leak_into_each_other():
    c = R.depth_cases()["views3"]
    whole = _render(c)
    for k in range(len(c["w2c"])):
        assert np.array_equal(whole[k].view(np.uint32), _render(c, views=[k])[0].view(np.uint32)), k
    assert not np.array_equal(whole[0], whole[1])


def test_exact_ties_are_covered():
    v, t, cov = R.tie_case()
    got = K.render_mesh_depth(_dev(v, torch.float64), _dev(t, torch.int32), _dev(R.IDENT, torch.float64), R.TIE["fx"], R.TIE["fy"],
                              R.TIE["cx"], R.TIE["cy"], R.TIE["H"], R.TIE["W"]).cpu().numpy()[0]
    assert np.array_equal(got > 0, cov)
    assert np.array_equal(got[cov], np.full(cov.sum(), 4.0, np.float32))


@pytest.mark.parametrize("name", ["soup", "soup_big", "views3", "overlap", "quad"])
def test_reversed_triangle_order_gives_the_same_bits(name):
    c = R.depth_cases()[name]
    a, b = _render(c), _render(c, tris=c["tris"][::-1])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.view(np.uint32), _render(c).view(np.uint32))  # and so do two runs


def test_out_of_range_index_is_refused():
    c = R.depth_cases()["soup"]
    for bad in (len(c["verts"]), -1, 2 ** 31 - 1):
        t = c["tris"].copy()
        t[len(t) // 2, 1] = bad
        with pytest.raises(RuntimeError, match="invalid argument"):
            _render(c, tris=t)
    torch.cuda.synchronize()  # nothing is left behind: the next call is served
    want, und = R.depth_reference("soup")
    got = _render(c)
    assert np.array_equal((got > 0)[~und], (want > 0)[~und])
    with pytest.raises(RuntimeError, match="invalid argument"):  # near has to be positive
        K.render_mesh_depth(_dev(c["verts"], torch.float64), _dev(c["tris"], torch.int32), _dev(c["w2c"], torch.float64),
                            c["fx"], c["fy"], c["cx"], c["cy"], c["H"], c["W"], near=0.0)


def test_empty_inputs():
    c = R.depth_cases()["quad"]
    none = K.render_mesh_depth(_dev(c["verts"], torch.float64), torch.zeros((0, 3), dtype=torch.int32, device="cuda"),
                               _dev(c["w2c"], torch.float64), c["fx"], c["fy"], c["cx"], c["cy"], 5, 7)
    assert none.shape == (1, 5, 7) and not none.any()
    noview = K.render_mesh_depth(_dev(c["verts"], torch.float64), _dev(c["tris"], torch.int32),
                                 torch.zeros((0, 4, 4), dtype=torch.float64, device="cuda"), c["fx"], c["fy"], c["cx"], c["cy"], 5, 7)
    assert noview.shape == (0, 5, 7)


# ---- votes ----

def _votes(c, views=slice(None), out=None):
    return K.visibility_votes(_dev(c["verts"], torch.float64), _dev(c["w2c"][views], torch.float64), c["fx"], c["fy"], c["cx"], c["cy"],
                              _dev(c["depth"][views], torch.float32), out=out)


def test_votes_on_given_depth_maps_are_exact():
    c = R.vote_case()
    got = _votes(c).cpu().numpy()
    ok = ~c["undecided"]
    assert got.dtype == np.int32 and np.array_equal(got[ok], c["votes"][ok]), np.nonzero(ok & (got != c["votes"]))[0][:10]
    for k in range(len(c["w2c"])):  # view by view
        one = _votes(c, slice(k, k + 1)).cpu().numpy()
        okk = ~c["views"][k]["undecided"]
        assert np.array_equal(one[okk] != 0, c["views"][k]["vote"][okk]), k


def test_accumulate_over_two_batches_equals_one_call():
    c = R.vote_case()
    whole = _votes(c)
    acc = torch.zeros_like(whole)
    assert _votes(c, slice(0, 2), out=acc) is acc
    _votes(c, slice(2, None), out=acc)
    assert torch.equal(acc, whole)


def test_vertex_exactly_on_the_frames_border_votes():
    k = dict(fx=4.0, fy=4.0, cx=2.0, cy=2.0)
    at = lambda u, v, z: [(u - 2.0) / 4.0 * z, (v - 2.0) / 4.0 * z, z]  # noqa: E731
    verts = np.array([at(0.0, 1.0, 1.5), at(1.0, 0.0, 1.5), at(-0.25, 1.0, 1.5)])  # u = 0 and v = 0 exactly: the numerators are 0
    got = K.visibility_votes(_dev(verts, torch.float64), _dev(np.eye(4)[None], torch.float64), depth=torch.zeros((1, 5, 7), device="cuda"), **k)
    assert got.tolist() == [1, 1, 0]


def test_min_views_19_20_21():
    """21 views of an empty 9 x 9 depth map (every inside vertex is in front): three vertices inside 19, 20 and 21 of them"""
    k = dict(fx=4.0, fy=4.0, cx=4.0, cy=4.0)
    w2c = np.tile(np.eye(4), (21, 1, 1))
    verts = np.array([[1.0, 0.0, 2.0], [0.5, 0.0, 2.0], [0.0, 0.0, 2.0]])  # u = 6, 5, 4 in the 19 views that are the identity
    w2c[0, 0, 3] = -2.25  # u - 4.5: 1.5, 0.5, -0.5: view 0 loses the third
    w2c[1, 0, 3] = -2.75  # u - 5.5: 0.5, -0.5, -1.5: view 1 loses the second and the third
    want = R.votes(verts, w2c, depth=np.zeros((21, 9, 9), np.float32), **k)
    assert want[0].tolist() == [21, 20, 19] and not want[1].any()
    votes = K.visibility_votes(_dev(verts, torch.float64), _dev(w2c, torch.float64), depth=torch.zeros((21, 9, 9), device="cuda"), **k)
    assert votes.tolist() == [21, 20, 19]
    assert K.keep_flags(votes, 20).tolist() == [1, 1, 0] and K.keep_flags(votes, 21).tolist() == [1, 0, 0]
    assert K.keep_flags(votes, 19).tolist() == [1, 1, 1] and K.keep_flags(votes, 22).tolist() == [0, 0, 0]


# ---- the cull ----

def _cull(c, **kw):
    return K.cull_mesh_by_visibility(_dev(c["verts"], torch.float64), _dev(c["tris"], torch.int32), _dev(c["w2c"], torch.float64),
                                     c["fx"], c["fy"], c["cx"], c["cy"], c["H"], c["W"], eps=c["eps"], min_views=c["min_views"], **kw)


@pytest.mark.parametrize("view_batch", [None, 1, 4, 100])
def test_cull_matches_the_restatement(view_batch):
    c = R.cull_case()
    cv, cf, votes = _cull(c, view_batch=view_batch)
    assert np.array_equal(votes.cpu().numpy(), c["votes"])
    assert np.array_equal(cv.cpu().numpy(), c["culled_verts"]) and np.array_equal(cf.cpu().numpy(), c["culled_tris"])
    assert cv.dtype == torch.float64 and cf.dtype == torch.int32 and votes.dtype == torch.int32


def test_cull_carries_colours_and_drops_unreferenced_vertices():
    c = R.cull_case()
    col = np.random.default_rng(0).random((len(c["verts"]), 3))
    cv, cf, cc, votes = _cull(c, colors=_dev(col, torch.float64))
    assert np.array_equal(cc.cpu().numpy(), col[c["used"]]) and np.array_equal(cv.cpu().numpy(), c["verts"][c["used"]])
    kept_by_votes = c["votes"] >= c["min_views"]
    assert (kept_by_votes & ~c["used"]).any(), "the case holds kept vertices that no kept face names"
    assert np.array_equal(np.unique(cf.cpu().numpy()), np.arange(len(cv)))


def _write_log(path, poses):
    with open(path, "w") as f:
        for k, p in enumerate(poses):
            f.write(f"{k} {k} {k + 1}\n" + "\n".join(" ".join(repr(float(x)) for x in row) for row in p) + "\n")


def test_cli_writes_the_culled_mesh(tmp_path):
    import gs2m_mesh as M
    c = R.cull_case()
    verts = c["verts"].astype(np.float32)  # what the PLY holds; the restatement follows on the same values
    M.write_mesh(tmp_path / "m.ply", types.SimpleNamespace(vertices=verts, triangles=c["tris"], vertex_colors=np.zeros((len(verts), 3))))
    c2w = np.linalg.inv(c["w2c"])
    gl = c2w.copy()
    gl[:, :3, 1:3] *= -1
    _write_log(tmp_path / "t.log", c2w)
    np.save(tmp_path / "t_gl.npy", gl)
    k = {n: c[n] for n in ("fx", "fy", "cx", "cy")}
    depth, upix = R.render_depth(verts, c["tris"], np.linalg.inv(c2w), H=c["H"], W=c["W"], **k)
    tot, und = R.votes(verts, np.linalg.inv(c2w), depth=depth, eps=c["eps"], tol=10 * R.VOTE_TOL, undecided_pixels=upix, **k)
    assert not und.any(), "rounding the vertices to float32 left the case decided"
    wv, wt, _ = R.cull_mesh(verts, c["tris"], tot, c["min_views"])
    common = ["--ply-path", str(tmp_path / "m.ply"), "--width", str(c["W"]), "--height", str(c["H"]), "--eps", str(c["eps"]),
              "--min-views", str(c["min_views"])] + [x for n in k for x in ("--" + n, repr(float(k[n])))]
    r = K.main(["--traj-path", str(tmp_path / "t.log")] + common)
    assert r["out"] == str(tmp_path / "m_cull.ply") and os.path.exists(r["out"])
    got = M.read_mesh(r["out"])
    assert np.array_equal(got.vertices, wv.astype(np.float32)) and np.array_equal(got.triangles, wt)
    assert 0 < r["n_triangles_kept"] == len(wt) < r["n_triangles"]
    r2 = K.main(["--traj-path", str(tmp_path / "t_gl.npy"), "--opengl", "--out", str(tmp_path / "other.ply")] + common)
    other = M.read_mesh(r2["out"])
    assert np.array_equal(other.vertices, got.vertices) and np.array_equal(other.triangles, got.triangles)


def test_evaluator_visibility_cull(tmp_path):
    """gs2m_tnt_eval.py --visibility-cull: the mesh is culled with the evaluation's own trajectory, written beside the results,
    and fewer points are scored; without the flag nothing changes"""
    import json
    import gs2m_mesh as M
    import gs2m_tnt_eval as E
    from test_tnt_eval_gpu import _write_gt_ply
    rng = np.random.default_rng(4)
    v, t = R.bumpy_sphere(40, 60, seed=1)
    vi, ti = R.bumpy_sphere(20, 30, seed=2, radius=0.4)  # an inner shell no camera sees
    verts, tris = np.concatenate([v, vi]).astype(np.float32), np.concatenate([t, ti + len(v)])
    gt = v[rng.integers(0, len(v), 20000)] + rng.normal(0, 1e-3, (20000, 3))
    data = tmp_path / "Barn"
    data.mkdir()
    _write_gt_ply(data / "Barn.ply", gt, rng)
    sq = [[-2, 0, -2], [2, 0, -2], [2, 0, 2], [-2, 0, 2]]
    (data / "Barn.json").write_text(json.dumps({"class_name": "SelectionPolygonVolume", "orthogonal_axis": "Y", "axis_min": -2.0,
                                                "axis_max": 2.0, "bounding_polygon": sq, "version_major": 1, "version_minor": 0}))
    poses = np.linalg.inv(R.ring_views(72, radius=3.5, height=0.5))  # cameras around the mesh, looking at it
    np.savetxt(data / "Barn_trans.txt", np.eye(4))
    _write_log(data / "Barn_COLMAP_SfM.log", poses)
    _write_log(tmp_path / "est.log", poses)
    runs = {}
    for name, extra in (("plain", []), ("culled", ["--visibility-cull"])):
        d = tmp_path / name
        d.mkdir()
        M.write_mesh(d / "mesh.ply", types.SimpleNamespace(vertices=verts, triangles=tris, vertex_colors=np.zeros((len(verts), 3))))
        runs[name] = E.main(["--dataset-dir", str(data), "--traj-path", str(tmp_path / "est.log"), "--ply-path", str(d / "mesh.ply"),
                             "--no-clouds"] + extra)
    plain, culled = runs["plain"], runs["culled"]
    assert "visibility_cull" not in plain and not os.path.exists(tmp_path / "plain" / "evaluation" / "culled_mesh.ply")
    assert plain["n_vertices"] == len(verts) and plain["n_triangles"] == len(tris)
    info = culled["visibility_cull"]
    out = M.read_mesh(tmp_path / "culled" / "evaluation" / "culled_mesh.ply")
    assert len(out.vertices) == info["n_vertices_kept"] == culled["n_vertices"] and len(out.triangles) == info["n_triangles_kept"]
    assert 0 < info["n_vertices_kept"] < len(verts)
    assert culled["n_source"] < plain["n_source"] and culled["n_source_scored"] != plain["n_source_scored"]
    # the inner shell (radii up to 0.54; the outer surface's start at 0.65) is gone: it is what no camera sees
    assert (np.linalg.norm(out.vertices, axis=1) > 0.6).all() and (np.linalg.norm(vi, axis=1) < 0.6).all()
