"""Tanks and Temples evaluation on the GPU (csrc/tnt_eval.hip and mesh_eval.hip through gs2m_tnt_eval) against the numpy
restatement (tests/tnt_eval_ref.py): every step bit for bit, one ICP evaluation's sums, ICP and registration end to end,
the score from the GPU's transform, determinism, and the CLI on a dataset folder written here.  All data is synthetic."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tnt_eval_ref as R  # noqa: E402
import gs2m_dtu_eval as D  # noqa: E402
import gs2m_tnt_eval as E  # noqa: E402

pytestmark = pytest.mark.gpu

# The summation-order floor of the registration's final 4 x 4 on the scene below: the largest element-wise difference between
# the restatement run with numpy's pairwise sums and with math.fsum (DESIGN.md §11 records it and how it was taken).  The
# allowance for the GPU's fixed-order sums is 16 times that.
SUM_ORDER_FLOOR = 6.661338147750939e-15
T_ALLOWANCE = 16 * SUM_ORDER_FLOOR


def _np(t):
    return t.cpu().numpy()


def _random_mesh(seed, n_verts, n_tris, scale):
    rng = np.random.default_rng(seed)
    return rng.uniform(-scale, scale, (n_verts, 3)), rng.integers(0, n_verts, (n_tris, 3)).astype(np.int32)


def _similarity(deg, scale, t, axis=(0.3, -0.5, 0.8)):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = scale * (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K))
    T[:3, 3] = t
    return T


CONVEX = [[-0.8, -0.7], [0.9, -0.6], [1.0, 0.5], [0.1, 0.95], [-0.9, 0.6]]
CONCAVE = [[-0.9, -0.9], [0.9, -0.9], [0.9, -0.1], [0.0, -0.1], [0.0, 0.4], [0.9, 0.4], [0.9, 0.9], [-0.9, 0.9], [-0.3, 0.0]]


def _volume(axis, poly2, scale, lo, hi):
    u, v, w = R.AXES[axis]
    P = np.zeros((len(poly2), 3))
    P[:, u], P[:, v] = np.asarray(poly2)[:, 0] * scale, np.asarray(poly2)[:, 1] * scale
    return {"orthogonal_axis": axis, "axis_min": lo * scale, "axis_max": hi * scale, "bounding_polygon": P}


@pytest.mark.parametrize("seed,scale", [(0, 1.0), (1, 37.5), (2, 0.004)])
def test_points_transform_and_crop_match_the_restatement(seed, scale):
    V, F = _random_mesh(seed, 700, 1500, scale)
    cloud = _np(E.mesh_points(V, F))
    assert np.array_equal(cloud, R.mesh_points(V, F))
    F_bad = F.copy()
    F_bad[17, 1] = len(V)
    with pytest.raises(RuntimeError, match="invalid argument"):
        E.mesh_points(V, F_bad)
    T = _similarity(20.0 + seed, 1.3, np.array([0.2, -0.1, 0.05]) * scale)
    moved = _np(E.transform(cloud, T))
    assert np.array_equal(moved, R.transform(cloud, T))
    bad = T.copy()
    bad[3, 0] = 1e-9
    with pytest.raises(RuntimeError, match="invalid argument"):
        E.transform(cloud, bad)
    rng = np.random.default_rng(seed + 10)
    for axis in ("X", "Y", "Z"):
        for poly in (CONVEX, CONCAVE):
            vol = _volume(axis, poly, scale, -0.5, 0.6)
            u, v, w = R.AXES[axis]
            P = vol["bounding_polygon"]
            special = []
            for k in range(len(P)):  # the polygon's vertices, edge midpoints, and points level with a vertex
                a, b = P[k], P[(k + 1) % len(P)]
                for q in (a, 0.5 * (a + b), a + np.eye(3)[u] * 0.3 * scale, a - np.eye(3)[u] * 0.3 * scale):
                    for h in (vol["axis_min"], vol["axis_max"], 0.0, np.nextafter(vol["axis_max"], np.inf)):
                        p = q.copy()
                        p[w] = h
                        special.append(p)
            pts = np.concatenate([moved, rng.uniform(-scale, scale, (3000, 3)), np.asarray(special)])
            want = R.crop_flags(pts, vol)
            got = _np(E.crop_flags(pts, vol))
            assert np.array_equal(got != 0, want), (axis, len(poly))
            assert 0 < want.sum() < len(pts)
            assert np.array_equal(_np(E.crop(pts, vol)), pts[want])
    # a polygon of more edges than one launch takes (a 300-gon), and one that is refused
    ang = np.linspace(0, 2 * np.pi, 300, endpoint=False)
    ring = np.stack([np.cos(ang) * (0.7 + 0.2 * np.sin(7 * ang)), np.sin(ang) * (0.7 + 0.2 * np.sin(7 * ang))], axis=1)
    vol = _volume("Y", ring, scale, -0.9, 0.9)
    pts = rng.uniform(-scale, scale, (20000, 3))
    assert np.array_equal(_np(E.crop_flags(pts, vol)) != 0, R.crop_flags(pts, vol))
    with pytest.raises(ValueError):
        E.crop_flags(pts, _volume("Y", np.zeros((1025, 2)), scale, -1, 1))


@pytest.mark.parametrize("seed,n,scale,s", [(0, 20000, 1.0, 0.07), (1, 150000, 25.0, 0.4), (2, 60000, 0.01, 0.0000066)])
def test_voxel_downsample_matches_the_restatement(seed, n, scale, s):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-scale, scale, (n, 3))
    pts[: n // 10] = rng.normal(0, 0.3 * s, (n // 10, 3)) + 0.37 * scale      # a voxel or two holding thousands of points
    lo = pts.min(0) - s * 0.5
    # points exactly on voxel faces: lo + k s for whole k, on one, two and three axes
    k = rng.integers(1, 20, (300, 3)).astype(float)
    on = lo + k * s
    on[:100, 1:] = rng.uniform(-scale, scale, (100, 2))
    on[100:200, 2] = rng.uniform(-scale, scale, 100)
    pts = np.concatenate([pts, np.clip(on, pts.min(0), pts.max(0))])
    pts = pts[rng.permutation(len(pts))]
    want = R.voxel_downsample(pts, s)
    got = _np(E.voxel_downsample(pts, s))
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    if seed == 2:  # 3 x 12 bits: the key needs both words
        assert np.floor((pts.max(0) - lo) / s).max() >= 2 ** 11
    with pytest.raises(RuntimeError, match="invalid argument"):
        E.voxel_downsample(pts, (pts.max() - pts.min()) / 2 ** 21 / 1.5)
    assert len(E.voxel_downsample(np.zeros((0, 3)), s)) == 0
    for bad in (np.nan, np.inf, -np.inf):  # one such coordinate among finite points is refused, not averaged in
        q = pts.copy()
        q[len(q) // 3, seed % 3] = bad
        with pytest.raises(RuntimeError, match="invalid argument"):
            E.voxel_downsample(q, s)


def test_uniform_downsample_by_a_stubbed_limit():
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(10000, 3))
    # n / limit = 2.5 -> 2 (Python's round: half to even), 3.33 -> 3, 1.0001 -> 1, 3.5002 -> 4
    for limit, k in ((4000, 2), (3000, 3), (9999, 1), (2857, 4)):
        assert int(round(len(pts) / float(limit))) == k
        want = R.uniform_downsample(pts, limit)
        assert np.array_equal(want, pts[::k])
        got = _np(E.uniform_downsample(pts, limit))
        assert np.array_equal(got, want), limit
    assert len(R.uniform_downsample(pts, 4000)) == 5000
    assert np.array_equal(_np(E.uniform_downsample(pts[:9999], 3000)), pts[:9999:3])  # n not a multiple of k
    assert np.array_equal(_np(E.uniform_downsample(pts[:7000], 2000)), pts[:7000:4])  # 3.5 -> 4
    assert np.array_equal(_np(E.uniform_downsample(pts, 10000)), pts)


@pytest.mark.parametrize("seed,nq,nt,scale", [(0, 3000, 2500, 1.0), (1, 5000, 4000, 50.0), (2, 2000, 6000, 0.02)])
def test_nearest_index_matches_brute_force(seed, nq, nt, scale):
    rng = np.random.default_rng(seed)
    t = rng.uniform(-scale, scale, (nt, 3))
    t[nt // 2: nt // 2 + 300] = t[:300]                      # exact duplicates: the lowest index wins
    t[-50:] = t[7]
    q = np.concatenate([rng.uniform(-1.2 * scale, 1.2 * scale, (nq, 3)), t[:200], t[nt // 2: nt // 2 + 100]])
    # a lattice: many queries at exactly the same distance from several targets
    g = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"), -1).reshape(-1, 3) * (scale / 8)
    t = np.concatenate([t, g])
    q = np.concatenate([q, g + scale / 16, g])
    for md in (0.05 * scale, 0.3 * scale, 3.0 * scale):
        idx, dist = E.nearest(q, t, md)
        widx, wdist = R.nearest(q, t, md)
        assert np.array_equal(_np(idx), widx), md
        assert np.array_equal(_np(dist), wdist), md
        assert np.array_equal(D.nearest_distances(q, t, md), wdist), "the distance-only call gives the same distances"
    assert (widx >= 0).all() and (R.nearest(q, t, 0.05 * scale)[0] < 0).any()
    idx, dist = E.nearest(q, np.zeros((0, 3)), 1.0)
    assert (_np(idx) == -1).all() and np.isinf(_np(dist)).all()


def test_histogram_counts_match_numpy():
    rng = np.random.default_rng(5)
    for tau in (0.01, 0.003, 0.025):
        edges = np.arange(0, 5 * tau, tau / 100)
        d = np.concatenate([rng.gamma(2.0, 0.5 * tau, 200000), edges, [edges[-1], 5 * tau, np.nextafter(edges[-1], 0), np.inf, np.inf],
                            np.nextafter(edges[1:40], 0), np.nextafter(edges[1:40], 1)])
        assert np.array_equal(E.histogram(d, edges), R.histogram(d, edges))
        assert E.histogram(d, edges).sum() == (d <= edges[-1]).sum()


def _radius(th, ph):
    return 1 + 0.25 * np.sin(3 * th + 0.5) * np.cos(2 * ph) + 0.15 * np.cos(5 * ph + 1.0) * np.sin(th) ** 2 + 0.1 * np.sin(4 * th) * np.sin(ph + 0.3)


def surface(th, ph):
    """a closed bumpy surface without symmetry (polar angle th, azimuth ph): relief in every direction, so that point-to-point
    ICP does not slide (on a gentle height field it takes hundreds of iterations)"""
    r = _radius(th, ph)
    return np.stack([r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph), r * np.cos(th)], -1)


def icp_scene(n_gt=150000, nt=121, nph=241, tau=0.01, seed=0):
    """-> dict: a grid mesh of `surface` moved by the inverse of a known similarity (2 degrees, 1 % scale, a few tau), ground truth
    of random surface points with scanner-like noise (tau / 10), a concave crop polygon along Z that cuts part of it away"""
    rng = np.random.default_rng(seed)
    th, ph = np.meshgrid(np.linspace(0.05, np.pi - 0.05, nt), np.linspace(0, 2 * np.pi, nph), indexing="ij")
    V = surface(th, ph).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nt - 1), np.arange(nph - 1), indexing="ij")
    a = (i * nph + j).ravel()
    F = np.concatenate([np.stack([a, a + nph, a + 1], 1), np.stack([a + 1, a + nph, a + nph + 1], 1)]).astype(np.int32)
    offset = _similarity(2.0, 1.01, np.array([0.03, -0.02, 0.025]))
    V_moved = R.transform(V, np.linalg.inv(offset))
    gt = surface(np.arccos(rng.uniform(-0.998, 0.998, n_gt)), rng.uniform(0, 2 * np.pi, n_gt)) + rng.normal(0, tau / 10, (n_gt, 3))
    poly = np.array([[-1.4, -1.4], [1.4, -1.3], [1.3, 0.2], [0.5, 0.3], [1.35, 0.6], [1.4, 1.4], [-1.2, 1.4], [-0.9, 0.1]])
    vol = {"orthogonal_axis": "Z", "axis_min": -1.1, "axis_max": 1.2, "bounding_polygon": np.concatenate([poly, np.zeros((len(poly), 1))], 1)}
    return {"V": V_moved, "F": F, "gt": gt, "volume": vol, "tau": tau, "offset": offset}


def corner_error(T, sc):
    """how far T o offset^-1 moves the corners of the ground truth's box from where they are"""
    lo, hi = sc["gt"].min(0), sc["gt"].max(0)
    c = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    return np.linalg.norm(R.transform(R.transform(c, np.linalg.inv(sc["offset"])), T) - c, axis=1).max()


def test_one_icp_evaluation():
    sc = icp_scene(n_gt=30000)
    src = R.crop(R.mesh_points(sc["V"], sc["F"]), sc["volume"])
    tgt = R.crop(sc["gt"], sc["volume"])
    for thr in (80 * sc["tau"], 2 * sc["tau"]):
        idx, _ = E.nearest(src, tgt, thr)
        widx, _ = R.nearest(src, tgt, thr, kdtree=True)
        assert np.array_equal(_np(idx), widx), "the correspondence set"
        m, w = E.icp_moments(src, tgt, idx), R.icp_moments(src, tgt, widx)
        assert m["c"] == w["c"] and 3 < m["c"]
        got = np.concatenate([[m["sum_d2"]], m["mx"] * m["c"], m["my"] * m["c"], m["sigma"].ravel() * m["c"], [m["sx2"] * m["c"]]])
        want = np.concatenate([[w["sum_d2"]], w["mx"] * w["c"], w["my"] * w["c"], w["sigma"].ravel() * w["c"], [w["sx2"] * w["c"]]])
        rel = np.abs(got - want) / w["terms"]
        print("icp sums: thr", thr, "c", m["c"], "largest error relative to the sum of |terms|:", rel.max())
        assert (rel <= 1e-12).all(), rel
    none = E.icp_moments(src, tgt, np.full(len(src), -1))
    assert none["c"] == 0 and none["sum_d2"] == 0.0
    stale = widx.copy()  # an index array against a smaller target cloud
    with pytest.raises(RuntimeError, match="invalid argument"):
        E.icp_moments(src, tgt[: widx.max()], stale)


# n = 0; below one workgroup; not a multiple of 256; beyond 256 x 256, so that a thread adds more than one pair
@pytest.mark.parametrize("n", [0, 100, 1000, 70001, 200000])
def test_icp_moments_sum_in_the_fixed_order(n):
    """All 17 outputs and the count of gs2m_tnt_icp_moments are, to the bit, those of the numpy restatement of the fixed order."""
    rng = np.random.default_rng(n)
    nt = 5000
    tgt = rng.normal(0, 1, (nt, 3)) * 10.0 ** rng.uniform(-3, 1, (nt, 1)) + np.array([3.0, -1.0, 0.5])
    idx = rng.integers(0, nt, n)
    idx[rng.random(n) < 0.2] = -1  # queries without a partner
    src = tgt[idx] + rng.normal(0, 0.05, (n, 3))
    m = E.icp_moments(src, tgt, idx)
    got = np.concatenate([[m["sum_d2"]], m["mx"], m["my"], m["sigma"].ravel(), [m["sx2"]]])
    c, want = R.icp_moments_fixed_order(src, tgt, idx)
    w = R.icp_moments(src, tgt, idx)
    loose = np.concatenate([[w["sum_d2"]], w["mx"], w["my"], w["sigma"].ravel(), [w["sx2"]]])
    print("icp moments: n", n, "count", m["c"], c, "outputs that differ from numpy's own sums:", int((got != loose).sum()))
    assert m["c"] == c == int((idx >= 0).sum())
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.nonzero(got != want)[0]


def test_icp_and_registration_end_to_end():
    sc = icp_scene()
    src = R.mesh_points(sc["V"], sc["F"])
    T0 = np.eye(4)
    # one ICP stage on its own
    s, t = R.voxel_downsample(R.crop(src, sc["volume"]), sc["tau"]), R.voxel_downsample(R.crop(sc["gt"], sc["volume"]), sc["tau"])
    Tg, fg, rg, ig = E.icp(s, t, 80 * sc["tau"], 20)
    Tr, fr, rr, ir = R.icp(s, t, 80 * sc["tau"], 20, kdtree=True)
    print("icp: iterations", ig, ir, "fitness", fg, fr, "rmse", rg, rr, "max |dT|", np.abs(Tg - Tr).max())
    assert ig == ir and abs(fg - fr) <= 1e-12 and abs(rg - rr) <= 1e-12
    assert np.abs(Tg - Tr).max() <= T_ALLOWANCE
    # the three stages
    T, stages = E.register(src, sc["gt"], T0, sc["volume"], sc["tau"])
    Tw, wstages = R.register(src, sc["gt"], T0, sc["volume"], sc["tau"], kdtree=True)
    print("register: iterations", [st["iterations"] for st in stages], [st["iterations"] for st in wstages],
          "max |dT|", np.abs(T - Tw).max(), "allowance", T_ALLOWANCE, "corner error", corner_error(T, sc), corner_error(Tw, sc))
    assert [st["iterations"] for st in stages] == [st["iterations"] for st in wstages]
    assert [(st["n_source"], st["n_target"]) for st in stages] == [(st["n_source"], st["n_target"]) for st in wstages]
    assert np.abs(T - Tw).max() <= T_ALLOWANCE
    assert corner_error(T, sc) <= sc["tau"] / 10
    # the score from the GPU's transform, handed to the restatement
    g = E.evaluate(src, sc["gt"], T, sc["volume"], sc["tau"], details=True)
    w = R.evaluate(src, sc["gt"], T, sc["volume"], sc["tau"], kdtree=True)
    assert np.array_equal(g["arrays"]["distance1"], w["distance1"]) and np.array_equal(g["arrays"]["distance2"], w["distance2"])
    for k in ("precision", "recall", "fscore", "n_source", "n_target"):
        assert g[k] == w[k], k
    for k in ("edges", "cum_source", "cum_target"):
        assert np.array_equal(g[k], w[k]), k
    assert g["fscore"] > 0.5, g["fscore"]  # aligned: 0.93 in the restatement; off by a few tau it falls towards 0


def _trajectories(sc, n=40, seed=1):
    """camera poses around the scene; the estimated ones live in the mesh's frame (offset^-1 of the true ones)"""
    rng = np.random.default_rng(seed)
    gt_trans = _similarity(33.0, 0.8, np.array([0.5, 0.2, -0.3]), axis=(0.1, 0.9, 0.2))
    centres = rng.uniform([-3, -3, -1], [3, 3, 2], (n, 3))
    est = np.tile(np.eye(4), (n, 1, 1))
    est[:, :3, 3] = R.transform(centres, np.linalg.inv(sc["offset"]))
    ref = np.tile(np.eye(4), (n, 1, 1))
    ref[:, :3, 3] = R.transform(centres, np.linalg.inv(gt_trans))
    return est, ref, gt_trans


def test_two_runs_are_bitwise_equal(tmp_path):
    sc = icp_scene()
    est, ref, gt_trans = _trajectories(sc)
    # a coarse start: the trajectories carry the offset up to a small error
    est[:, :3, 3] += np.random.default_rng(2).normal(0, 0.01, (len(est), 3))
    runs = []
    for k in range(2):
        out = tmp_path / f"run{k}"
        r = E.evaluate_scene(sc["V"], sc["F"], sc["gt"], sc["volume"], sc["tau"], est, ref, gt_trans, scene="Barn", out_dir=str(out),
                             details=True)
        j = json.load(open(out / "results.json"))
        runs.append((r, j))
    (a, ja), (b, jb) = runs
    for k in ja:
        if k not in ("ms", "stages"):
            assert ja[k] == jb[k], k
    for sa, sb in zip(ja["stages"], jb["stages"]):
        assert {k: v for k, v in sa.items() if k != "ms"} == {k: v for k, v in sb.items() if k != "ms"}
    for k in a["arrays"]:
        assert np.array_equal(a["arrays"][k], b["arrays"][k]), k
    for k in ("cum_source", "cum_target"):
        assert np.array_equal(a[k], b[k])
    assert a["fscore"] > 0.5


def _write_gt_ply(path, pts, rng):
    """a vertex-only binary PLY with normals and colours beside the coordinates, as the scans have"""
    a = np.zeros(len(pts), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                                     ("red", "u1"), ("green", "u1"), ("blue", "u1")]))
    for k, n in enumerate("xyz"):
        a[n] = pts[:, k]
    a["nz"], a["red"] = 1.0, rng.integers(0, 255, len(pts))
    head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(pts)}\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(a.tobytes())


def test_cli_end_to_end(tmp_path):
    import gs2m_mesh as M
    sc = icp_scene()
    rng = np.random.default_rng(4)
    data = tmp_path / "Barn"
    data.mkdir()
    _write_gt_ply(data / "Barn.ply", sc["gt"], rng)
    vol = sc["volume"]
    (data / "Barn.json").write_text(json.dumps({"class_name": "SelectionPolygonVolume", "orthogonal_axis": "Z", "axis_min": vol["axis_min"],
                                                "axis_max": vol["axis_max"], "bounding_polygon": vol["bounding_polygon"].tolist(),
                                                "version_major": 1, "version_minor": 0}))
    est, ref, gt_trans = _trajectories(sc)
    np.savetxt(data / "Barn_trans.txt", gt_trans)

    def write_log(path, poses):
        with open(path, "w") as f:
            for k, p in enumerate(poses):
                f.write(f"{k} {k} {k + 1}\n" + "\n".join(" ".join(f"{x:.12f}" for x in row) for row in p) + "\n")

    write_log(data / "Barn_COLMAP_SfM.log", ref)
    write_log(tmp_path / "est.log", est)
    mesh_dir = tmp_path / "mesh"
    mesh_dir.mkdir()
    import types
    M.write_mesh(mesh_dir / "tsdf_post.ply", types.SimpleNamespace(vertices=sc["V"].astype(np.float32), triangles=sc["F"],
                                                                  vertex_colors=np.zeros((len(sc["V"]), 3), np.float32)))
    r = E.main(["--dataset-dir", str(data), "--traj-path", str(tmp_path / "est.log"), "--ply-path", str(mesh_dir / "tsdf_post.ply")])
    out = mesh_dir / "evaluation"
    j = json.load(open(out / "results.json"))
    for k in ("precision", "recall", "fscore", "tau", "stages", "transformation", "ms"):
        assert k in j, k
    assert j["tau"] == 0.01 and len(j["stages"]) == 3 and np.asarray(j["transformation"]).shape == (4, 4)
    prf = np.loadtxt(out / "Barn.prf_tau_plotstr.txt")
    assert np.array_equal(prf, np.array([j["precision"], j["recall"], j["fscore"], 0.01, 5.0]))
    assert np.array_equal(np.loadtxt(out / "Barn.precision.txt"), r["cum_source"])
    assert np.array_equal(np.loadtxt(out / "Barn.recall.txt"), r["cum_target"])
    # the F-score against the restatement's score stage on what the CLI read, with the CLI's transform
    verts, tris = E.read_ply(mesh_dir / "tsdf_post.ply")
    gt, _ = E.read_ply(data / "Barn.ply")
    w = R.evaluate(R.mesh_points(verts, tris), gt, np.asarray(j["transformation"]), vol, 0.01, kdtree=True)
    for k in ("precision", "recall", "fscore"):
        assert j[k] == w[k], k
    assert j["fscore"] > 0.5
    with pytest.raises(SystemExit):
        E.main(["--dataset-dir", str(data), "--traj-path", str(tmp_path / "est.log"), "--ply-path", str(mesh_dir / "tsdf_post.ply"),
                "--scene", "Shed"])
