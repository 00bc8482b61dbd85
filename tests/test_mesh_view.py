"""The float64 restatement of the mesh visualisation (tests/mesh_view_ref.py) against values worked out by hand,
the host side of gs2m_mesh_view.py (the turntable, the cameras.json reader), and the condition every input of the GPU tests has
to meet: few undecided pixels, few loose bytes.  No GPU."""
import json
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mesh_view_ref as V  # noqa: E402
import tnt_cull_ref as R  # noqa: E402

K = dict(fx=20.0, fy=20.0, cx=8.0, cy=8.0, H=16, W=16)  # the quad of V.quad() covers the columns and rows 3 .. 12


def _byte(lin):
    return math.floor(255.0 * float(V.srgb_encode(lin)) + 0.5)


def test_quad_seen_head_on():
    """on the optical axis cos = 1: floor(255 srgb(0.7 * 1.0) + 0.5); off it the ray leans, so the test looks along the axis:
    a 1 x 1 frame whose only ray is (0, 0, 1)"""
    v, t = V.quad()
    out = V.shade(v, t, R.IDENT, 1.0, 1.0, 0.5, 0.5, 1, 1, ss=1)
    assert out["rgba"][0, 0, 0].tolist() == [_byte(0.7)] * 3 + [255] and _byte(0.7) == 218
    assert out["tri_id"][0, 0, 0] in (0, 1) and out["depth"][0, 0, 0] == np.float32(2.0)
    # a frame of 16 x 16: everything inside is lit by at least the cosine at the quad's corner and at most 1
    out = V.shade(v, t, R.IDENT, ss=2, **K)
    inside = out["rgba"][0, 4:12, 4:12]
    assert (inside[..., 3] == 255).all() and (inside[..., :3] <= _byte(0.7)).all()
    assert (inside[..., :3] >= _byte(0.7 * (0.15 + 0.85 / math.sqrt(1 + 2 * 0.25 ** 2)))).all()
    assert (out["rgba"][0, :2] == 0).all() and (out["tri_id"][0, :2] == -1).all() and (out["depth"][0, :2] == 0).all()


def test_quad_tilted_by_60_degrees():
    """the normal at 60 degrees to the axis' ray: ambient + diffuse / 2"""
    v, t = V.quad()
    c, s = math.cos(math.pi / 3), math.sin(math.pi / 3)
    tilt = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    v = (v - [0, 0, 2.0]) @ tilt.T + [0, 0, 2.0]
    for srgb in (True, False):
        out = V.shade(v, t, R.IDENT, 1.0, 1.0, 0.5, 0.5, 1, 1, ss=1, srgb=srgb)
        lin = 0.7 * (0.15 + 0.85 * 0.5)
        want = _byte(lin) if srgb else math.floor(255.0 * lin + 0.5)
        assert out["rgba"][0, 0, 0].tolist() == [want] * 3 + [255]
    both = V.shade(v, t[:1], R.IDENT, 1.0, 1.0, 0.5, 0.5, 1, 1, ss=1), V.shade(v, t[:1, ::-1], R.IDENT, 1.0, 1.0, 0.5, 0.5, 1, 1, ss=1)
    assert np.array_equal(both[0]["rgba"], both[1]["rgba"]), "two-sided: the winding does not matter"


def test_barycentrics_reproduce_a_linear_ramp():
    rng = np.random.default_rng(0)
    v, t = V.quad()
    v = v + rng.normal(0, 0.2, v.shape)  # a skew quad: two triangles in different planes
    g = np.array([0.3, -0.2, 0.1])
    colors = (0.5 + v @ g)[:, None] * np.ones(3)  # linear in world space
    vis = V.visibility(v, t, R.IDENT, ss=2, **K)
    p = np.nonzero(vis["tri"][0].ravel() >= 0)[0]
    tt = t[vis["tri"][0].ravel()[p]]
    ray = R.pixel_rays(32, 32, 40.0, 40.0, 16.0, 16.0)[p]
    l0, l1, l2 = V.barycentrics(v[tt[:, 0]], v[tt[:, 1]], v[tt[:, 2]], ray)
    assert len(p) > 300 and np.allclose((l0 + l1) + l2, 1.0, rtol=0, atol=1e-14)
    assert (np.minimum(np.minimum(l0, l1), l2) > -1e-12).all()
    hit = l0[:, None] * v[tt[:, 0]] + l1[:, None] * v[tt[:, 1]] + l2[:, None] * v[tt[:, 2]]
    assert np.allclose(hit / hit[:, 2:], ray, atol=1e-12), "the interpolated point lies on the sample's ray"
    # the ramp through the shader: ambient 1, diffuse 0 leaves the albedo alone
    out = V.shade(v, t, R.IDENT, ss=1, colors=colors.astype(np.float32), ambient=1.0, diffuse=0.0, srgb=False, **K)
    vis1 = V.visibility(v, t, R.IDENT, ss=1, **K)
    p1 = np.nonzero(vis1["tri"][0].ravel() >= 0)[0]
    t1 = t[vis1["tri"][0].ravel()[p1]]
    r1 = R.pixel_rays(16, 16, K["fx"], K["fy"], K["cx"], K["cy"])[p1]
    m0, m1, m2 = V.barycentrics(v[t1[:, 0]], v[t1[:, 1]], v[t1[:, 2]], r1)
    point = m0[:, None] * v[t1[:, 0]] + m1[:, None] * v[t1[:, 1]] + m2[:, None] * v[t1[:, 2]]
    want = np.floor(255.0 * np.clip(0.5 + point @ g, 0, 1) + 0.5)
    got = out["rgba"][0].reshape(-1, 4)[p1, 0]
    assert np.abs(got.astype(np.int64) - want).max() <= 1  # (the colours were rounded to float32)


@pytest.mark.parametrize("ss", [2, 3, 4])
def test_alpha_at_a_straight_edge_counts_the_covered_samples(ss):
    """a half plane x <= x_e in front of an 8 x 1 frame, fx = 1: the samples of pixel 3 with centre left of x_e are covered"""
    for frac in (0.1, 0.3, 0.55, 0.8):
        xe = 3.0 + frac
        z = 2.0
        v, t = R._tri([-50.0, -40.0, z], [(xe - 4.0) * z, -40.0, z], [(xe - 4.0) * z, 40.0, z])
        v = np.concatenate([v, [[-50.0, 40.0, z]]])
        t = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
        out = V.shade(v, t, R.IDENT, 1.0, 1.0, 4.0, 0.5, 1, 8, ss=ss)
        centres = 3.0 + (np.arange(ss) + 0.5) / ss
        m = ss * int((centres < xe).sum())
        assert out["rgba"][0, 0, :, 3].tolist() == [255, 255, 255, math.floor(255.0 * m / ss ** 2 + 0.5), 0, 0, 0, 0], (ss, frac)


def test_vertex_normal_sums_of_a_cube_are_exact():
    v, t, axes = V.cube()
    want = [[0, 0, 0] for _ in v]
    for tri, (axis, sign) in zip(t.tolist(), axes):
        for i in tri:
            want[i][axis] += sign * 2 ** 32  # Python integers
    sums, deg, normals = V.vertex_normal_sums(v, t)
    assert sums.tolist() == want and deg.sum() == 36
    s = np.array(want, np.float64)
    assert np.array_equal(normals, s / np.sqrt((s * s).sum(1))[:, None])
    # a zero-area triangle and one with a bad index add nothing
    t2 = np.concatenate([t, [[0, 0, 5], [1, 2, len(v)], [3, -1, 4]]]).astype(np.int32)
    assert np.array_equal(V.vertex_normal_sums(v, t2)[0], sums)
    assert np.array_equal(V.vertex_normal_sums(v, t[::-1])[0], sums)


def test_turntable():
    import gs2m_mesh_view as G
    w2c = R.look_at([1.0, 0.5, -3.0], [0.1, 0.0, 0.2])
    m = G.turntable(w2c, 120)
    assert m.shape == (120, 4, 4) and m.dtype == np.float64
    assert np.array_equal(m[0], w2c), "frame 0: the identity rotation"
    assert np.allclose(G.turntable(w2c, 12), m[::10], atol=1e-15)
    again = G.turntable(w2c, 120, shift=(0.1, -0.2, 0.3))
    T = np.eye(4)
    T[:3, 3] = (0.1, -0.2, 0.3)
    assert np.allclose(again[0], w2c @ T, atol=1e-15)
    # periodic over the frame count: frame f + frames is frame f
    for f in (1, 7, 59):
        ax, ay = 0.4 * math.sin(2 * math.pi * (f + 120) / 120), 0.6 * math.sin(4 * math.pi * (f + 120) / 120)
        rot = np.linalg.inv(w2c) @ m[f]
        Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
        Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
        assert np.allclose(rot[:3, :3], Ry @ Rx, atol=1e-12) and np.allclose(rot[:3, 3], 0, atol=1e-12)
    assert np.allclose(m[30, :3, :3], w2c[:3, :3] @ np.array([[1, 0, 0], [0, math.cos(0.4), -math.sin(0.4)], [0, math.sin(0.4), math.cos(0.4)]]), atol=1e-12)


def test_cameras_json_round_trip(tmp_path):
    import gs2m_mesh_view as G
    w2c = R.look_at([2.0, -1.0, 0.5], [0.0, 0.1, 0.0])
    c2w = np.linalg.inv(w2c)
    rec = [{"id": 0, "img_name": "rect_001_3_r5000.png", "width": 1554, "height": 1162, "position": c2w[:3, 3].tolist(),
            "rotation": [row.tolist() for row in c2w[:3, :3]], "fy": 2892.33, "fx": 2883.5}]
    (tmp_path / "cameras.json").write_text(json.dumps(rec))
    (view,) = G.read_cameras_json(tmp_path / "cameras.json")
    assert view["name"] == "rect_001_3_r5000.png" and (view["width"], view["height"]) == (1554, 1162)
    assert (view["fx"], view["fy"], view["cx"], view["cy"]) == (2883.5, 2892.33, 777.0, 581.0)
    assert np.allclose(view["w2c"], w2c, atol=1e-13)
    half = G.scaled(view, 4)
    assert (half["width"], half["height"]) == (388, 290) and half["fx"] == 2883.5 * 388 / 1554 and half["cy"] == 581.0 * 290 / 1162
    a = G.parser().parse_args(["--ply-path", "m.ply", "--cameras", "c.json"])
    assert (a.ss, a.shading, a.colour, a.view_idx, a.frames, a.resolution) == (2, "flat", "grey", 23, 120, 1)


CASES = [(n, ss) for n, c in sorted(V.view_cases().items()) for ss in c["ss"]]


@pytest.mark.parametrize("name,ss", CASES)
def test_gpu_inputs_are_decided(name, ss):
    """a condition on the inputs: at most 1 % of the pixels undecided, at most 1 % of the bytes loose, in every mode the GPU
    tests run the case in"""
    for shading, colour, srgb in (("flat", "grey", True), ("smooth", "vertex", True), ("smooth", "grey", False)):
        ref = V.reference(name, ss, shading, colour, srgb)
        und, loose = ref["undecided"].mean(), ref["loose"][~ref["undecided"]].mean() if (~ref["undecided"]).any() else 0.0
        print(name, ss, shading, colour, srgb, "undecided", und, "loose", loose, "covered", (ref["rgba"][..., 3] > 0).mean())
        assert und <= V.CAP and loose <= V.CAP


def test_duplicates_and_cli_inputs():
    c = V.duplicates_case()
    vis = V.visibility(c["verts"], c["tris"], c["w2c"], c["fx"], c["fy"], c["cx"], c["cy"], c["H"], c["W"], 1)
    tri = vis["tri"][0]
    assert set(np.unique(tri).tolist()) == {-1, 0, 1, 2}, "the duplicate of the higher index never wins"
    assert vis["undecided"][0][tri == 1].all(), "an exact tie is an undecided sample of the restatement"
    assert (tri == 1).sum() > 100 and (tri == 2).sum() > 20 and (tri == 0).sum() > 20
    v, t, records = V.cli_mesh()
    assert len(t) == 200 and len(records) == 4
