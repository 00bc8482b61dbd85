"""The mesh visibility cull without a GPU: the numpy restatement tests/tnt_cull_ref.py held to the definitions --
an analytic plane's depth, coverage against a barycentric point-in-triangle test, the bilinear sample against torch's
grid_sample on the CPU, the vote rule case by case -- the share of undecided pixels and vertices of every input the GPU tests
use, and the command line's defaults against the reference's constants."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tnt_cull_ref as R  # noqa: E402


def test_depth_of_an_analytic_plane():
    """a frame-filling triangle in the plane n . x = h of a tilted camera: z at pixel (i, j) is h / (n . r)"""
    H, W = 9, 11
    k = R.intrinsics(H, W)
    n, h = np.array([0.2, -0.1, 1.0]), 3.0
    corners = np.array([[-40.0, -40.0], [50.0, -35.0], [0.0, 60.0]])
    cam = np.array([[x, y, (h - n[0] * x - n[1] * y) / n[2]] for x, y in corners])
    M = R.look_at([0.3, -0.2, 0.1], [0.5, 0.1, 4.0])
    world = (cam - M[:3, 3]) @ M[:3, :3]  # M is rigid: x_world = R^T (x_cam - t)
    depth, und = R.render_depth(world, [[0, 1, 2]], M[None], H=H, W=W, **k)
    r = R.pixel_rays(H, W, **k)
    want = (h / (r @ n)).reshape(H, W)
    assert not und.any() and (depth[0] > 0).all()
    assert np.abs(depth[0] - want).max() <= 4e-7 * want.max()  # fp32 rounding of values near 3


def test_coverage_matches_a_barycentric_test():
    rng = np.random.default_rng(0)
    H, W = 24, 31
    k = R.intrinsics(H, W)
    r = R.pixel_rays(H, W, **k)
    for _ in range(40):
        z = rng.uniform(1.0, 5.0, 3)
        uv = rng.uniform([-4, -4], [W + 4, H + 4], (3, 2))
        v = np.array([R._unproject(k, uv[q, 0], uv[q, 1], z[q]) for q in range(3)])
        depth, und = R.render_depth(v, [[0, 1, 2]], R.IDENT, H=H, W=W, **k)
        # barycentric coordinates of every centre in the projected triangle
        j, i = np.mgrid[0:H, 0:W]
        P = np.stack([i.ravel() + 0.5, j.ravel() + 0.5], 1)
        T = np.array([uv[1] - uv[0], uv[2] - uv[0]]).T
        l12 = np.linalg.solve(T, (P - uv[0]).T).T
        lam = np.column_stack([1 - l12.sum(1), l12])
        inside = (lam > 1e-7).all(1).reshape(H, W)
        outside = (lam < -1e-7).any(1).reshape(H, W)
        assert (depth[0] > 0)[inside].all() and not (depth[0] > 0)[outside].any()
        assert und[0][~inside & ~outside].all() or not (~inside & ~outside).any()
        # and the depth is the perspective-correct one: 1 / z is affine in the image
        zi = 1.0 / (lam @ (1.0 / z))
        got = depth[0].ravel()[inside.ravel()]
        assert np.abs(got - zi[inside.ravel()]).max() <= 1e-6 * 5.0
    assert r.shape == (H * W, 3)


def test_tie_case_is_exact():
    v, t, cov = R.tie_case()
    depth, und = R.render_depth(v, t, R.IDENT, R.TIE["fx"], R.TIE["fy"], R.TIE["cx"], R.TIE["cy"], R.TIE["H"], R.TIE["W"])
    assert np.array_equal(depth[0] > 0, cov) and np.array_equal(depth[0][cov], np.full(cov.sum(), 4.0, np.float32))
    assert und[0][1, 1] and und[0][1, 5] and und[0][4, 1]  # the corners are ties, and the restatement says so


def test_bilinear_matches_grid_sample():
    rng = np.random.default_rng(1)
    H, W = 7, 9
    D = rng.uniform(1.0, 3.0, (H, W)).astype(np.float32)
    D[2:4, 3:6] = 0.0  # neighbours that are 0 enter the average as 0
    u = np.concatenate([rng.uniform(0, W - 1, 500), [0.0, W - 1.0, 0.0, W - 1.0, 3.0, 2.5, np.nextafter(W - 1.0, 0)]])
    v = np.concatenate([rng.uniform(0, H - 1, 500), [0.0, 0.0, H - 1.0, H - 1.0, 2.0, 1.5, np.nextafter(H - 1.0, 0)]])
    got = R.bilinear(D, u, v)
    grid = torch.from_numpy(np.stack([u / (W - 1) * 2.0 - 1.0, v / (H - 1) * 2.0 - 1.0], -1))[None, None]
    want = torch.nn.functional.grid_sample(torch.from_numpy(D.astype(np.float64))[None, None], grid, mode="bilinear",
                                           padding_mode="border", align_corners=True)[0, 0, 0].numpy()
    assert np.abs(got - want).max() <= 1e-12
    assert got[500] == D[0, 0] and got[501] == D[0, W - 1] and got[503] == D[H - 1, W - 1] and got[504] == 0.0


def test_vote_rule_case_by_case():
    H, W = 5, 7
    k = dict(fx=4.0, fy=4.0, cx=2.0, cy=2.0)
    D = np.full((H, W), 2.0, np.float32)
    D[:, 4:] = 0.0
    at = lambda u, v, z: [(u - 2.0) / 4.0 * z, (v - 2.0) / 4.0 * z, z]  # noqa: E731
    cases = [(at(1.0, 1.0, 1.5), True),             # in front of the surface
             (at(1.0, 1.0, 2.004), True),           # within eps behind it
             (at(1.0, 1.0, 2.006), False),          # beyond eps
             (at(5.5, 1.0, 9.0), True),             # over empty pixels: always in front
             (at(3.5, 1.0, 1.004), True),           # half surface, half empty: d = 1, z < 1.005
             (at(3.5, 1.0, 1.006), False),
             (at(-0.5, 1.0, 1.5), False), (at(6.5, 1.0, 1.5), False), (at(1.0, -0.5, 1.5), False), (at(1.0, 4.5, 1.5), False),
             (at(1.0, 1.0, -1.5), False),           # behind the camera (it projects inside the frame)
             ([np.nan, 0.0, 1.0], False)]
    r = R.view_votes([c[0] for c in cases], np.eye(4), depth=D, **k)
    assert r["vote"].tolist() == [c[1] for c in cases]
    assert not r["undecided"][:-1].any()
    tot, _ = R.votes([c[0] for c in cases], np.stack([np.eye(4)] * 3), depth=np.stack([D] * 3), **k)
    assert tot.tolist() == [3 * c[1] for c in cases]
    # u = 0 exactly (the numerator is exactly 0) is inside, and a margin of 0 is reported as undecided
    edge = R.view_votes([at(0.0, 1.0, 1.5)], np.eye(4), depth=D, **k)
    assert edge["u"][0] == 0.0 and edge["vote"][0] and edge["undecided"][0]


def test_cull_mesh_drops_unreferenced_vertices():
    v = np.arange(18.0).reshape(6, 3)
    t = np.array([[0, 1, 2], [2, 3, 4], [1, 2, 5]])
    cv, ct, used = R.cull_mesh(v, t, [20, 25, 20, 19, 30, 21])
    assert used.tolist() == [True, True, True, False, False, True]  # 4 is kept by its votes but no kept face names it
    assert np.array_equal(cv, v[[0, 1, 2, 5]]) and ct.tolist() == [[0, 1, 2], [1, 2, 3]]


@pytest.mark.parametrize("name", sorted(R.depth_cases()))
def test_undecided_pixels_stay_under_the_cap(name):
    depth, und = R.depth_reference(name)
    assert und.mean() <= R.UNDECIDED_CAP, (name, und.mean())


def test_depth_cases_are_what_their_names_say():
    cov = {n: int((R.depth_reference(n)[0] > 0).sum()) for n in R.depth_cases()}
    assert cov["no_centre"] == 0 and cov["one_centre"] == 1 and cov["behind"] == 0
    for n in ("fills_frame_1x1", "fills_frame_7x5", "fills_frame_64", "fills_frame_65x129"):
        assert cov[n] == R.depth_cases()[n]["H"] * R.depth_cases()[n]["W"]
    assert 0 < cov["crossing"] < 64 * 64 and 0 < cov["crossing_65x129"] < 65 * 129
    d = R.depth_reference("near_far")[0]
    assert cov["near_far"] > 0 and d[d > 0].min() >= 15.0 and d.max() <= 20.0  # only the third triangle, cut at far
    # the quad: no hole along the shared diagonal (every centre inside the outline is covered)
    c = R.depth_cases()["quad"]
    whole = R.render_depth(c["verts"], [[0, 1, 2], [0, 2, 3]], c["w2c"], c["fx"], c["fy"], c["cx"], c["cy"], 64, 64)[0] > 0
    halves = [R.render_depth(c["verts"], [f], c["w2c"], c["fx"], c["fy"], c["cx"], c["cy"], 64, 64)[0] > 0 for f in ([0, 1, 2], [0, 2, 3])]
    assert np.array_equal(whole, halves[0] | halves[1]) and cov["quad"] == whole.sum() > 2000


def test_undecided_vertices_stay_under_the_cap():
    c = R.vote_case()
    assert c["undecided"].mean() <= R.UNDECIDED_CAP
    kinds = c["views"][0]
    assert (c["votes"] == 0).any() and (c["votes"] == len(c["w2c"])).any()
    assert (~kinds["inside"]).sum() > 100 and (kinds["inside"] & ~kinds["front"]).sum() > 100 and (kinds["inside"] & (kinds["d"] == 0)).sum() > 10
    cc = R.cull_case()
    assert 0 < len(cc["culled_verts"]) < len(cc["verts"]) and 0 < len(cc["culled_tris"]) < len(cc["tris"])


def test_cli_defaults_are_the_reference_constants():
    import gs2m_mesh_cull as K
    a = K.parser().parse_args(["--traj-path", "t.log", "--ply-path", "m.ply"])
    assert (a.width, a.height) == (1920, 1080)
    assert (a.fx, a.fy, a.cx, a.cy) == (1163.8678928442187, 1172.793101201448, 962.3120628412543, 542.0667209577691)
    assert (a.near, a.far, a.eps, a.min_views) == (0.01, 20.0, 0.005, 20) and not a.opengl and a.out == ""
    assert (R.NEAR, R.FAR, R.EPS, R.MIN_VIEWS) == (K.NEAR, K.FAR, K.EPS, K.MIN_VIEWS)
    # --opengl flips the y and z columns of the camera-to-world pose before it is inverted
    c2w = np.linalg.inv(R.look_at([1.0, 2.0, 3.0], [0.0, 0.0, 0.0]))
    gl = c2w.copy()
    gl[:3, 1:3] *= -1
    assert np.allclose(K.world_to_camera(gl[None], opengl=True)[0], R.look_at([1.0, 2.0, 3.0], [0.0, 0.0, 0.0]), atol=1e-12)


def test_cpu_tensors_are_refused():
    import gs2m_mesh_cull as K
    v, f, m = torch.zeros(3, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.int32), torch.eye(4, dtype=torch.float64)[None]
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.render_mesh_depth(v, f, m, 1.0, 1.0, 0.5, 0.5, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.visibility_votes(v, m, 1.0, 1.0, 0.5, 0.5, torch.zeros(1, 1, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.cull_mesh_by_visibility(v, f, m, 1.0, 1.0, 0.5, 0.5, 1, 1)
