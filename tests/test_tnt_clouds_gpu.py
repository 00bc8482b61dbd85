"""The Tanks and Temples clouds on the GPU (csrc/tnt_clouds.hip through gs2m_tnt_eval): the k-nearest-neighbour search through
its index output, exactly the brute-force set and order; the normals against exact planes and the float64 arbiter
(tests/tnt_clouds_ref.py); the colours against matplotlib's hot_r byte for byte; the two PLY files end to end."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tnt_clouds_ref as CR  # noqa: E402
import gs2m_eval_util as U  # noqa: E402
import gs2m_tnt_eval as E  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (1, 20, 32)


def _dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64)).cuda()


def _knn(p, k, cell=None):
    nrm, idx = E.knn_normals(_dev(p), k, return_index=True, cell=cell)
    return nrm.cpu().numpy(), idx.cpu().numpy()


def _check_search(p, cell=None, ks=KS):
    want = CR.knn_brute(p, max(ks))
    for k in ks:
        nrm, idx = _knn(p, k, cell)
        assert idx.shape == (len(p), k) and np.array_equal(idx, want[:, :k]), (len(p), k, cell)
        assert np.isfinite(nrm).all() and np.abs(np.linalg.norm(nrm, axis=1) - 1).max() <= 1e-15 * 4
    return want


def test_surface_is_the_evaluators_own_downsample():
    raw, s = CR.surface_raw()
    assert np.array_equal(E.voxel_downsample(raw, s).cpu().numpy(), CR.surface())


@pytest.mark.parametrize("n", CR.SIZES)
def test_search_on_the_surface(n):
    p = CR.surface()[:n]
    want = CR.surface_knn(n)
    for k in KS:
        _, idx = _knn(p, k)
        assert np.array_equal(idx, want[:, :k]), (n, k)
        assert (idx[:, min(k, n):] == -1).all() and (idx[:, :min(k, n)] >= 0).all()


def test_search_inside_one_cell():
    p = np.random.default_rng(1).uniform(0.1, 0.9, (300, 3))
    _check_search(p, cell=1.0)
    _check_search(p[:7], cell=1.0)


def test_search_across_empty_cells():
    """two clusters 60 cells apart, the small one with fewer points than k: its queries cross the empty cells and end at the box"""
    rng = np.random.default_rng(2)
    p = np.concatenate([rng.uniform(0, 1, (10, 3)), rng.uniform(0, 2, (490, 3)) + 30.0])
    p = p[rng.permutation(len(p))]
    want = _check_search(p, cell=0.5)
    small = np.nonzero(p[:, 0] < 5)[0]
    assert (p[want[small, 19], 0] > 5).all(), "the 20th neighbour of a small-cluster point lies in the other cluster"
    _check_search(np.concatenate([p, -p]) * 0.25, cell=0.5, ks=(20,))  # cells of negative coordinates, 16 cells apart


@pytest.mark.parametrize("cell", [None, 1.0, 2.5, 0.75])
def test_search_on_the_lattice(cell):
    """8 x 8 x 8 integer points: the 20th neighbour is one of many at its distance, so the tie rule decides the set; with
    cell = 1.0 every point sits on a cell's face"""
    p = CR.lattice()
    want = _check_search(p, cell=cell)
    d2 = ((p[want[:, 19]] - p) ** 2).sum(1)
    d2_next = ((p[want[:, 20]] - p) ** 2).sum(1)
    assert (d2 == d2_next).mean() > 0.2, "ties at the cut"
    _check_search(p[np.random.default_rng(3).permutation(len(p))], cell=cell, ks=(20,))


def test_k_out_of_range_is_refused():
    p = _dev(CR.lattice(3, 3, 3))
    for k in (0, 33):
        with pytest.raises(RuntimeError, match="invalid argument"):
            E.knn_normals(p, k)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.knn_normals(CR.lattice(3, 3, 3), 20)
    with pytest.raises(RuntimeError, match="unsupported size"):  # a box of more cells than the walk may cross
        E.knn_normals(p, 20, cell=1e-5)
    for x in (np.nan, np.inf, -np.inf):
        bad = CR.lattice(3, 3, 3)
        bad[5, 1] = x
        with pytest.raises(RuntimeError, match="invalid argument"):
            E.knn_normals(_dev(bad), 20, cell=1.0)


def _plane(a, b, o=(0.0, 0.0, 0.0), m=12):
    """m x m points o + i a + j b, i, j whole: exact in float64 for whole a, b, o"""
    i, j = np.meshgrid(np.arange(float(m)), np.arange(float(m)), indexing="ij")
    return np.asarray(o) + i.reshape(-1, 1) * np.asarray(a, float) + j.reshape(-1, 1) * np.asarray(b, float)


# (a, b, the normal under the sign rule): z = x + 2 y and its mirror image z = -x - 2 y, whose unflipped normals point to
# opposite sides of z = 0; planes that hold the z axis, where the first non-zero component decides; the coordinate planes
PLANES = [((1, 0, 1), (0, 1, 2), (-1, -2, 1)), ((1, 0, -1), (0, 1, -2), (1, 2, 1)), ((0, 1, 2), (1, 0, 1), (-1, -2, 1)),
          ((2, 1, -3), (1, -1, 1), (2, 5, 3)), ((1, 1, 0), (0, 0, 1), (1, -1, 0)), ((1, -1, 0), (0, 0, 1), (1, 1, 0)),
          ((-1, 1, 0), (0, 0, -1), (1, 1, 0)), ((0, 1, 0), (0, 0, 1), (1, 0, 0)), ((1, 0, 0), (0, 0, 1), (0, 1, 0)),
          ((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((0, -1, 0), (-1, 0, 0), (0, 0, 1))]


@pytest.mark.parametrize("a,b,want", PLANES)
def test_normals_of_exact_planes(a, b, want):
    want = np.asarray(want, float) / np.linalg.norm(want)
    assert abs(np.dot(want, a)) < 1e-15 and abs(np.dot(want, b)) < 1e-15
    for o in ((0, 0, 0), (-7, 3, -5)):
        nrm, _ = _knn(_plane(a, b, o), 20)
        err = CR.sine_cross(nrm, np.broadcast_to(want, nrm.shape))
        print("plane", a, b, "largest |n x n_true|:", err.max())
        assert err.max() <= 1e-12
        assert CR.sign_rule_holds(nrm)
        # Where the true normal has no z component the computed one may carry a rounding-sized z of either sign, and the rule
        # speaks about the computed z: the side is then held only where the zeros are exact (a coordinate plane).
        if want[2] != 0 or np.count_nonzero(want) == 1:
            assert (nrm @ want > 0).all(), "the side the sign rule names"


def test_normals_of_the_lattice_planes():
    """two z = const sheets of the lattice, 40 apart: every neighbour set lies in its own sheet"""
    p = np.concatenate([CR.lattice(8, 8, 1), CR.lattice(8, 8, 1) + [0, 0, 40.0]])
    nrm, idx = _knn(p, 20, cell=2.0)
    assert np.array_equal(idx, CR.knn_brute(p, 20))
    assert (p[idx][:, :, 2] == p[:, None, 2]).all()
    assert CR.sine_cross(nrm, np.broadcast_to([0.0, 0.0, 1.0], nrm.shape)).max() <= 1e-12 and (nrm[:, 2] > 0).all()


@pytest.mark.parametrize("offset", [0.0, 1e4])
def test_normals_on_the_surface_match_the_arbiter(offset):
    """|n x n_ref| <= 1e-9 wherever the arbiter's eigenvalue gap (l1 - l0) / l2 is at least 1e-3 (tests/test_tnt_clouds.py holds
    the excluded share to 1 % for the arbiter alone).  An fp64 eigenvector's angle error is about 2^-53 l2 / gap, 1e-13 here;
    the bound leaves four decades for the covariance's own rounding.  Moved by 1e4 the cloud's raw second moments are 1e12
    times its variances: a covariance that is not centred loses every digit there."""
    p = CR.surface()[:5000] + offset
    index = CR.surface_knn(5000)[:, :20] if offset == 0.0 else CR.knn_brute(p, 20)
    nrm, idx = _knn(p, 20)
    assert np.array_equal(idx, index)
    ref, w = CR.normals_ref(p, index)
    keep = CR.gap(w) >= CR.GAP_MIN
    err = CR.sine_cross(nrm, ref)
    print("offset", offset, "compared:", int(keep.sum()), "of", len(p), "largest |n x n_ref|:", err[keep].max())
    assert (~keep).mean() <= CR.EXCLUDED_MAX
    assert err[keep].max() <= 1e-9
    assert CR.sign_rule_holds(nrm) and np.abs(np.linalg.norm(nrm, axis=1) - 1).max() <= 4e-16


def test_degenerate_neighbourhoods():
    for n in (1, 2):
        nrm, idx = _knn(CR.surface()[:n], 20)
        assert np.array_equal(nrm, np.tile([0.0, 0.0, 1.0], (n, 1)))
    line = np.arange(30.0).reshape(-1, 1) * np.array([1.0, 2.0, 3.0])
    same = np.tile([[0.5, -2.0, 7.0]], (25, 1))
    for p in (line, line * 0.1 + 3.3, same):
        nrm, _ = _knn(p, 20)
        assert np.isfinite(nrm).all()
        assert np.abs(np.linalg.norm(nrm, axis=1) - 1).max() <= 4e-16
    assert np.array_equal(_knn(same, 20)[0], np.tile([0.0, 0.0, 1.0], (25, 1))), "a zero covariance: the fallback"
    assert np.abs(_knn(line, 20)[0] @ np.array([1.0, 2.0, 3.0])).max() <= 1e-12, "perpendicular to the line"
    assert len(E.knn_normals(torch.zeros((0, 3), dtype=torch.float64, device="cuda"))) == 0


@pytest.mark.parametrize("m", [0.03, 0.015, 0.075, 0.009, 1.0])
def test_colours_are_hot_r(m):
    d = CR.color_probe(m)
    got = E.distance_colors(_dev(d), m).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, CR.hot_r_bytes(d, m))
    with pytest.raises(RuntimeError, match="invalid argument"):
        E.distance_colors(_dev(np.concatenate([d, [np.nan]])), m)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(RuntimeError, match="invalid argument"):
            E.distance_colors(_dev(d), bad)


def _read_cloud(file):
    data = open(file, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    n = int([ln for ln in data[:end].decode().split("\n") if ln.startswith("element vertex")][0].split()[2])
    a = np.frombuffer(data, np.dtype([(k, "<f8") for k in ("x", "y", "z", "nx", "ny", "nz")] + [(k, "u1") for k in ("red", "green", "blue")]), n, end)
    assert len(data) == end + 51 * n
    return (np.stack([a[k] for k in "xyz"], 1), np.stack([a[k] for k in ("nx", "ny", "nz")], 1),
            np.stack([a[k] for k in ("red", "green", "blue")], 1))


def test_evaluate_scene_writes_the_two_clouds(tmp_path):
    from test_tnt_eval_gpu import _trajectories, icp_scene
    sc = icp_scene()
    est, ref, gt_trans = _trajectories(sc)
    tau = sc["tau"]
    run = lambda out, **kw: E.evaluate_scene(sc["V"], sc["F"], sc["gt"], sc["volume"], tau, est, ref, gt_trans, scene="Barn",  # noqa: E731
                                             out_dir=str(tmp_path / out), details=True, **kw)
    r, r0 = run("with", plot=True), run("without", clouds=False)
    for k in ("precision", "recall", "fscore", "n_source_scored", "n_target_scored", "transformation"):
        assert r[k] == r0[k], k
    for f in ("Barn.precision.txt", "Barn.recall.txt", "Barn.prf_tau_plotstr.txt"):
        assert open(tmp_path / "with" / f, "rb").read() == open(tmp_path / "without" / f, "rb").read(), f
    for k in r["arrays"]:
        assert np.array_equal(r["arrays"][k], r0["arrays"][k]), k
    assert not list((tmp_path / "without").glob("*.ply")) and "clouds" not in json.load(open(tmp_path / "without" / "results.json"))["ms"]
    assert json.load(open(tmp_path / "with" / "results.json"))["ms"]["clouds"] > 0
    table = CR.hot_r_bytes(np.arange(256) / 256.0, 1.0)  # row k of the table, through matplotlib
    for name, pts, dist, count in (("precision", "source", "distance1", "n_source_scored"), ("recall", "target", "distance2", "n_target_scored")):
        p, nrm, rgb = _read_cloud(tmp_path / "with" / f"Barn.{name}.ply")
        assert len(p) == r[count] > 1000
        assert np.array_equal(p, r["arrays"][pts])
        d = r["arrays"][dist]
        rows = np.minimum((np.minimum(d, 3 * tau) / (3 * tau) * 256).astype(np.int64), 255)
        assert np.array_equal(rgb, table[rows]) and np.array_equal(rgb, CR.hot_r_bytes(d, 3 * tau))
        assert (rgb[np.isinf(d)] == table[255]).all(), "from 5 tau on the distances are +inf: the cap's colour"
        assert np.abs(np.linalg.norm(nrm, axis=1) - 1).max() <= 4e-16 and CR.sign_rule_holds(nrm)
        assert np.array_equal(nrm, r["clouds"][name]["normals"].cpu().numpy()) and r["clouds"][name]["normals"].is_cuda
        assert np.array_equal(U.read_ply(tmp_path / "with" / f"Barn.{name}.ply")[0], p)
    stem = "PR_Barn_@d_th_0_0100"
    assert (tmp_path / "with" / (stem + ".png")).stat().st_size > 1000 and (tmp_path / "with" / (stem + ".pdf")).stat().st_size > 1000
    assert not list((tmp_path / "without").glob("PR_*"))
