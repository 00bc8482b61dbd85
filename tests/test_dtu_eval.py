"""DTU mesh evaluation on the CPU: the numpy / scikit-learn restatement (tests/dtu_eval_ref.py) against the reference's own
evaluator (tests/golden/ref_dtu_eval.npz, tests/golden/make_dtu_eval_golden.py), the seeded shuffle, the KD-tree's radius
rule, the loaders and the command line's refusals.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dtu_eval_ref as R  # noqa: E402
import gs2m_dtu_eval as E  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "ref_dtu_eval.npz")
CASES = ("mc", "edges", "nan")


def golden_case(name):
    z = np.load(GOLDEN)
    c = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}
    for k in ("res", "thresh", "patch", "max_dist", "vis", "mean_d2s", "mean_s2d", "overall"):
        c[k] = float(c[k])
    c["seed"] = int(c["seed"])
    return c


def ref_eval(c):
    return R.evaluate(c["vertices"], c["triangles"], c["stl"], c["obs_mask"], c["bb"], c["res"], c["plane"], c["thresh"], c["patch"],
                      c["max_dist"], c["seed"], c["vis"])


def _close(a, b, rel=1e-12):
    if np.isnan(b):
        return np.isnan(a)
    return abs(a - b) <= rel * abs(b)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_evaluator(name):
    c = golden_case(name)
    r = ref_eval(c)
    assert np.array_equal(r["down"], c["d2s_points"]), "thinned cloud in shuffled order"
    assert np.array_equal(r["d2s_colors"], c["d2s_colors"])
    assert np.array_equal(r["s2d_colors"], c["s2d_colors"])
    for k in ("mean_d2s", "mean_s2d", "overall"):
        assert _close(r[k], c[k]), (k, r[k], c[k])


def test_golden_cases_cover_the_contract():
    c = golden_case("edges")
    V, F = c["vertices"], c["triangles"]
    p0, p1, p2 = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    v1, v2 = p1 - p0, p2 - p0
    area2 = np.linalg.norm(np.cross(v1, v2), axis=1)
    assert (area2 == 0).sum() >= 2
    l1, l2 = np.linalg.norm(v1, axis=1), np.linalg.norm(v2, axis=1)
    ok = area2 > 0
    thr = c["thresh"] * np.sqrt(l1[ok] * l2[ok] / area2[ok])
    n1, n2 = np.floor(l1[ok] / thr), np.floor(l2[ok] / thr)
    assert ((n1 == 0) | (n2 == 0)).any() and (n1 * n2 / 2 > 500).sum() >= 2
    assert len(np.setdiff1d(np.arange(len(V)), F)) >= 6, "unreferenced vertices"
    r = ref_eval(c)
    assert len(r["cloud"]) > len(V) + 2000
    assert np.isnan(golden_case("nan")["mean_d2s"]) and not np.isnan(golden_case("nan")["mean_s2d"])
    m = golden_case("mc")
    rm = ref_eval(m)
    assert 0 < rm["inbound"].sum() < len(rm["down"]) and 0 < rm["obs"].sum() < rm["inbound"].sum()
    assert 0 < rm["above"].sum() < len(m["stl"])


def test_seeded_shuffle_is_the_permutation():
    """step 3: rng.shuffle(a, axis=0) moves the rows as a[rng.permutation(len(a))] does, for the same seed"""
    for seed in (0, 1, 7, 12345):
        for n in (1, 2, 17, 1000, 65537):
            a = np.random.default_rng(99).random((n, 3))
            b = a.copy()
            np.random.default_rng(seed).shuffle(b, axis=0)
            assert np.array_equal(b, a[E.shuffle_order(n, seed)])


def test_kd_tree_radius_rule_is_the_squared_form():
    """step 4: scikit-learn's KD-tree counts q as a neighbour exactly when (dx dx + dy dy) + dz dz <= r r, boundary included"""
    import sklearn.neighbors as skln
    rng = np.random.default_rng(3)
    r = 0.2
    base = rng.uniform(-50, 50, (200, 3))
    # points at distance r (in every rounding of it) along random directions, and on the axes
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = np.concatenate([base, base + r * d, base + r * d * (1 + 1e-16), base + [r, 0, 0], base - [0, r, 0],
                          np.array([[0.0, 0, 0], [0.2, 0, 0], [0.4, 0, 0], [0.6000000000000001, 0, 0]])])
    tree = skln.KDTree(pts)
    got = tree.query_radius(pts, r=r)
    for q in range(len(pts)):
        dd = pts - pts[q]
        want = np.nonzero((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2] <= r * r)[0]
        assert np.array_equal(np.sort(got[q]), want), q
    keep = R.thin(pts, r)
    assert np.array_equal(keep, R.thin_sequential(pts, r, np.arange(len(pts))))


def test_world_transform_matches_the_contract():
    S = np.eye(4, dtype=np.float32)
    S[0, 0] = S[1, 1] = S[2, 2] = np.float32(301.7)
    S[:3, 3] = np.float32([-12.3, 45.6, 612.9])
    v = np.random.default_rng(0).uniform(-1, 1, (100, 3)).astype(np.float32).astype(np.float64)
    w = R.world_transform(v, S)
    assert np.array_equal(w, v * float(S[0, 0]) + np.array([float(x) for x in S[:3, 3]]))


def test_mat_and_ply_loaders_round_trip(tmp_path):
    from scipy.io import savemat
    c = golden_case("mc")
    scan = 24
    os.makedirs(tmp_path / "ObsMask")
    os.makedirs(tmp_path / "Points" / "stl")
    mask = c["obs_mask"].copy()
    mask[1, 2, 3] = 1
    mask[3, 2, 1] = 0  # an axis swap would show
    savemat(str(tmp_path / "ObsMask" / f"ObsMask{scan}_10.mat"), {"ObsMask": mask, "BB": c["bb"], "Res": np.array([[c["res"]]])})
    savemat(str(tmp_path / "ObsMask" / f"Plane{scan}.mat"), {"P": c["plane"].reshape(1, 4)})
    E.write_point_cloud(tmp_path / "Points" / "stl" / f"stl{scan:03}_total.ply", c["stl"])
    gt = E.load_dtu_ground_truth(str(tmp_path), scan)
    assert gt["obs_mask"].flags.c_contiguous and gt["obs_mask"].dtype == np.uint8
    assert np.array_equal(gt["obs_mask"], mask)
    assert gt["bb"].dtype == np.float32 and np.array_equal(gt["bb"], c["bb"].astype(np.float32))
    assert gt["res"] == c["res"] and np.array_equal(gt["plane"], c["plane"])
    assert gt["stl"].dtype == np.float64 and np.array_equal(gt["stl"], c["stl"])
    # the mesh writer's fp32 PLY reads back widened, faces kept; colours of a written cloud are rounded to uchar
    import gs2m_mesh as M
    mesh = M.TriangleMesh(c["vertices"].astype(np.float32), c["triangles"])
    M.write_mesh(tmp_path / "m.ply", mesh)
    v, f = E.read_ply(tmp_path / "m.ply")
    assert v.dtype == np.float64 and np.array_equal(v, c["vertices"].astype(np.float32).astype(np.float64))
    assert np.array_equal(f, c["triangles"])
    col = c["d2s_colors"]
    E.write_point_cloud(tmp_path / "vis.ply", c["d2s_points"], col)
    data = open(tmp_path / "vis.ply", "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    a = np.frombuffer(data, np.dtype([("p", "<f8", (3,)), ("c", "u1", (3,))]), len(col), end)
    assert np.array_equal(a["p"], c["d2s_points"]) and np.array_equal(a["c"], np.rint(col * 255).astype(np.uint8))
    with open(tmp_path / "ascii.ply", "w") as fh:
        fh.write("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n0 0 0\n")
    with pytest.raises(ValueError, match="binary little-endian"):
        E.read_ply(tmp_path / "ascii.ply")


def test_cli_refuses_mask_cull(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        E.main(["--input_ply", str(tmp_path / "m.ply"), "--ref_dir", str(tmp_path / "scan24"), "--dtu_dir", str(tmp_path), "--mask_cull"])
    assert e.value.code != 0
    assert "--mask_cull is not supported" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        E.main(["--input_ply", str(tmp_path / "m.ply"), "--ref_dir", str(tmp_path / "notascan"), "--dtu_dir", str(tmp_path)])
