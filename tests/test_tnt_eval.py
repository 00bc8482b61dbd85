"""Tanks and Temples evaluation, the parts that need no GPU: the numpy restatement (tests/tnt_eval_ref.py) against the
reference's own get_f1_score_histo2 (tests/golden/ref_tnt_eval.npz), the product's readers and scene table against the
golden, the trajectory alignment, the crop rule on a hand-made polygon, and gs2m_mesh's --tnt preset."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tnt_eval_ref as R  # noqa: E402
import gs2m_tnt_eval as E  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "ref_tnt_eval.npz"))
SCORE_CASES = ("random", "edges", "empty", "truck", "ignatius")


@pytest.mark.parametrize("name", SCORE_CASES)
def test_restated_score_equals_the_reference(name):
    tau = float(GOLD[f"{name}/tau"])
    p, r, f, es, cs, et, ct = R.score(GOLD[f"{name}/distance1"], GOLD[f"{name}/distance2"], tau)
    assert np.array_equal(np.array([p, r, f], np.float64), GOLD[f"{name}/prf"])
    for got, key in ((es, "edges_source"), (cs, "cum_source"), (et, "edges_target"), (ct, "cum_target")):
        assert np.array_equal(np.asarray(got), GOLD[f"{name}/{key}"]), key


def test_values_from_five_tau_on_are_alike():
    """the product reports +inf from 5 tau on: nothing the score derives can tell"""
    tau = float(GOLD["edges/tau"])
    d1, d2 = GOLD["edges/distance1"], GOLD["edges/distance2"]
    a = R.score(d1, d2, tau)
    b = R.score(np.where(d1 >= 5 * tau, np.inf, d1), np.where(d2 >= 5 * tau, np.inf, d2), tau)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_readers_and_scene_table(tmp_path):
    table = json.load(open(os.path.join(HERE, "golden", "ref_tnt_scenes.json")))["scenes_tau"]
    assert E.SCENES_TAU == table
    log = tmp_path / "t.log"
    log.write_bytes(GOLD["log/text"].tobytes())
    poses = E.read_trajectory_log(log)
    assert np.array_equal(poses, GOLD["log/poses"])
    assert np.array_equal(E.read_trajectory(str(log)), poses)
    np.save(tmp_path / "t.npy", poses)
    assert np.array_equal(E.read_trajectory(str(tmp_path / "t.npy")), poses)
    (tmp_path / "t.json").write_text("{}")
    with pytest.raises(ValueError, match="auto_orient_and_center_poses"):
        E.read_trajectory(str(tmp_path / "t.json"))
    vol = {"class_name": "SelectionPolygonVolume", "orthogonal_axis": "y", "axis_min": -1.5, "axis_max": 2.0, "version_major": 1,
           "bounding_polygon": [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 2.0]]}
    (tmp_path / "v.json").write_text(json.dumps(vol))
    v = E.read_crop_volume(tmp_path / "v.json")
    assert v["orthogonal_axis"] == "Y" and v["axis_min"] == -1.5 and v["axis_max"] == 2.0
    assert np.array_equal(v["bounding_polygon"], np.asarray(vol["bounding_polygon"]))


def _similarity(seed, scale):
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    T = np.eye(4)
    T[:3, :3] = scale * Q
    T[:3, 3] = rng.normal(0, 2, 3)
    return T


def _poses(centres):
    P = np.tile(np.eye(4), (len(centres), 1, 1))
    P[:, :3, 3] = centres
    return P


@pytest.mark.parametrize("align", [E.align_trajectories, R.align_trajectories], ids=["product", "restatement"])
def test_align_trajectories_recovers_a_similarity(align):
    rng = np.random.default_rng(0)
    T = _similarity(1, 1.7)
    gt_trans = _similarity(2, 0.9)
    x = rng.normal(0, 3, (200, 3))
    y_world = R.transform(x, T)                             # where the estimated centres belong
    y = R.transform(y_world, np.linalg.inv(gt_trans))       # the reference trajectory before gt_trans
    got = align(_poses(x), _poses(y), gt_trans)
    assert np.abs(got - T).max() <= 1e-12 * np.abs(T).max(), np.abs(got - T).max()
    # 20 % gross outliers: every one lands at least 0.3 sqrt(3) 1.7 = 0.88 from its partner, four times the 0.2 bound, and the
    # same fit comes out (the clean pairs alone give it).  The trimmed refit is no RANSAC: it needs the all-pairs fit to leave
    # the clean pairs within 0.2, which offsets of this size (2 % of the cloud's variance) do; DESIGN.md section 11 says so.
    bad = rng.choice(200, 40, replace=False)
    xo = x.copy()
    xo[bad] += rng.choice([-1.0, 1.0], (40, 3)) * rng.uniform(0.3, 0.6, (40, 3))
    got_o = align(_poses(xo), _poses(y), gt_trans)
    clean = np.setdiff1d(np.arange(200), bad)
    assert np.array_equal(got_o, align(_poses(x[clean]), _poses(y[clean]), gt_trans))
    assert np.abs(got_o - T).max() <= 1e-12 * np.abs(T).max(), np.abs(got_o - T).max()
    with pytest.raises(ValueError):
        align(_poses(x[:4]), _poses(y[:4]), gt_trans)


def test_crop_restatement_on_a_concave_polygon():
    """an L-shaped polygon in the (x, z) plane, orthogonal axis Y.  u = x, v = z: an edge crosses when exactly one end lies
    strictly below p.z, and counts when its node is strictly left of p.x -- so a point on a left or lower edge is outside
    or inside as this rule says, not by closure"""
    L = [[0, 0, 0], [4, 0, 0], [4, 0, 2], [2, 0, 2], [2, 0, 4], [0, 0, 4]]
    vol = {"orthogonal_axis": "Y", "axis_min": -1.0, "axis_max": 1.0, "bounding_polygon": np.asarray(L, float)}
    cases = [
        ((1.0, 0.0, 1.0), True),    # inside the foot
        ((3.0, 0.0, 1.0), True),
        ((1.0, 0.0, 3.0), True),    # inside the leg
        ((3.0, 0.0, 3.0), False),   # the notch
        ((5.0, 0.0, 1.0), False),
        ((-1.0, 0.0, 1.0), False),
        ((1.0, 1.0, 1.0), True),    # on axis_max: closed
        ((1.0, -1.0, 1.0), True),   # on axis_min: closed
        ((1.0, 1.0000001, 1.0), False),
        ((0.0, 0.0, 1.0), False),   # on the left edge x = 0: its node is not strictly below p.x
        ((4.0, 0.0, 1.0), True),    # on the right edge x = 4: one crossing (x = 0) strictly left
        ((2.0, 0.0, 3.0), True),    # on the notch's vertical edge x = 2
        ((1.0, 0.0, 0.0), False),   # on the bottom edge z = 0: no end strictly below
        ((1.0, 0.0, 4.0), True),    # on the top edge z = 4: the vertical edges x = 0 cross (0 < 4, 4 >= 4)
        ((3.0, 0.0, 2.0), True),    # on the notch's horizontal edge z = 2
        ((0.0, 0.0, 0.0), False),   # vertices
        ((4.0, 0.0, 0.0), False),
        ((4.0, 0.0, 2.0), True),
        ((2.0, 0.0, 2.0), True),
        ((2.0, 0.0, 4.0), True),
        ((0.0, 0.0, 4.0), False),
    ]
    pts = np.array([c[0] for c in cases], float)
    want = np.array([c[1] for c in cases])
    got = R.crop_flags(pts, vol)
    assert np.array_equal(got, want), [(c[0], bool(g)) for c, g in zip(cases, got) if g != c[1]]
    # the same polygon seen along X and Z
    for axis in ("X", "Z"):
        # X: (u, v, w) = (y, z, x), so old (x, y, z) -> (y, x, z); Z: (u, v, w) = (x, y, z), so old (x, y, z) -> (x, z, y)
        P = np.asarray(L, float)
        if axis == "X":
            poly, q = P[:, [1, 0, 2]], pts[:, [1, 0, 2]]
        else:
            poly, q = P[:, [0, 2, 1]], pts[:, [0, 2, 1]]
        v2 = {"orthogonal_axis": axis.lower(), "axis_min": -1.0, "axis_max": 1.0, "bounding_polygon": poly}
        assert np.array_equal(R.crop_flags(q, v2), want), axis


def test_restatement_voxel_and_uniform_downsample():
    p = np.array([[0.0, 0.0, 0.0], [0.1, 0.1, 0.1], [1.0, 0.0, 0.0], [0.2, 0.0, 0.2], [1.1, 0.2, 0.1]])
    # lo = -0.25: voxels floor((p + 0.25) / 0.5) = (0, 0, 0) for rows 0, 1, 3 and (2, 0, 0) for rows 2, 4
    out = R.voxel_downsample(p, 0.5)
    assert np.array_equal(out, np.array([((p[0] + p[1]) + p[3]) / 3.0, (p[2] + p[4]) / 2.0]))
    big = np.arange(30, dtype=float).reshape(10, 3)
    assert np.array_equal(R.uniform_downsample(big, limit=4), big[::2])   # round(2.5) = 2: Python's round
    assert np.array_equal(R.uniform_downsample(big, limit=3), big[::3])
    assert R.uniform_downsample(big, limit=10) is not None and len(R.uniform_downsample(big, limit=10)) == 10


def test_mesh_tnt_preset(tmp_path):
    import gs2m_mesh as M
    src = tmp_path / "data"
    src.mkdir()
    base = ["--ply", "x.ply", "-s", str(src)]
    a, b = M.parse_args(base + ["-o", str(tmp_path / "Barn"), "--tnt"])
    assert (a.max_depth, a.voxel_size, a.sdf_trunc, a.num_clusters, b) == (3.0, 0.002, 4.0 * 0.002, 1, None)
    a, b = M.parse_args(base + ["-o", str(tmp_path / "Courthouse"), "--tnt"])
    assert a.max_depth == 4.5
    a, b = M.parse_args(base + ["-o", str(tmp_path / "out"), "--tnt", "--scene", "Truck"])
    assert a.max_depth == 3.0
    (src / "transforms.json").write_text(json.dumps({"frames": []}))
    a, b = M.parse_args(base + ["-o", str(tmp_path / "Barn"), "--tnt"])
    assert b is None and a.voxel_size == 0.002
    aabb = [[-1.0, 1.5], [-2.0, 2.096], [0.0, 1.0]]
    (src / "transforms.json").write_text(json.dumps({"aabb_range": aabb}))
    a, b = M.parse_args(base + ["-o", str(tmp_path / "Barn"), "--tnt"])
    assert np.array_equal(b, np.asarray(aabb)) and a.voxel_size == 4.096 / 2048 and a.sdf_trunc == 4.0 * a.voxel_size
    with pytest.raises(SystemExit):
        M.parse_args(base + ["-o", str(tmp_path / "Barn"), "--tnt", "--dtu"])
    a, b = M.parse_args(base + ["-o", str(tmp_path / "Barn"), "--dtu"])
    assert (a.max_depth, a.voxel_size, a.sdf_trunc, a.num_clusters, b) == (5.0, 0.002, 0.008, 1, None)
    a, b = M.parse_args(base + ["-o", str(tmp_path / "Barn")])
    assert (a.max_depth, a.voxel_size, a.sdf_trunc, b) == (-1.0, -1.0, -1.0, None)
