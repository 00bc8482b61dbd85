"""DTU mesh evaluation on the GPU (csrc/mesh_eval.hip through gs2m_dtu_eval): against the reference's own evaluator
(tests/golden/ref_dtu_eval.npz) and the numpy / scikit-learn restatement (tests/dtu_eval_ref.py) bit for bit, thinning under
adversarial orders, determinism, an analytic plane, and the synthetic surface scene scored end to end through the CLI."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dtu_eval_ref as R  # noqa: E402
import gs2m_dtu_eval as E  # noqa: E402
from test_dtu_eval import CASES, golden_case  # noqa: E402

pytestmark = pytest.mark.gpu


def _close(a, b, rel=1e-12):
    if np.isnan(b):
        return np.isnan(a)
    return abs(a - b) <= rel * abs(b)


def _gpu_eval(c, **kw):
    return E.evaluate_mesh(c["vertices"], c["triangles"], c["stl"], c["obs_mask"], c["bb"], c["res"], c["plane"], c["thresh"],
                           c["patch"], c["max_dist"], c["seed"], visualize_threshold=c["vis"], details=True, **kw)


@pytest.mark.parametrize("name", CASES)
def test_matches_the_reference_evaluator(name):
    c = golden_case(name)
    g = _gpu_eval(c)
    a = g["arrays"]
    assert np.array_equal(a["down"], c["d2s_points"]), "thinned cloud in shuffled order"
    assert np.array_equal(a["d2s_colors"], c["d2s_colors"])
    assert np.array_equal(a["s2d_colors"], c["s2d_colors"])
    for k in ("mean_d2s", "mean_s2d", "overall"):
        assert _close(g[k], c[k]), (k, g[k], c[k])


def _random_mesh(seed, n_tris, scale):
    rng = np.random.default_rng(seed)
    V = rng.uniform(-scale, scale, (n_tris + 40, 3))
    F = rng.integers(0, n_tris + 20, (n_tris, 3)).astype(np.int32)  # the last 20 vertices unreferenced
    F[:5, 2] = F[:5, 1]  # zero area
    # small triangles around random vertices, as a fine mesh has
    small = rng.integers(0, len(V), (n_tris, 1))
    Vs = np.concatenate([V, V[small[:, 0]] + rng.normal(0, 0.3, (n_tris, 3)), V[small[:, 0]] + rng.normal(0, 0.3, (n_tris, 3))])
    Fs = np.stack([small[:, 0], len(V) + np.arange(n_tris), len(V) + n_tris + np.arange(n_tris)], axis=1).astype(np.int32)
    return Vs, np.concatenate([F, Fs])


@pytest.mark.parametrize("seed,n_tris,scale,thresh", [(0, 30, 3.0, 0.2), (1, 200, 6.0, 0.25), (2, 500, 2.0, 0.1)])
def test_steps_match_the_restatement(seed, n_tris, scale, thresh):
    V, F = _random_mesh(seed, n_tris, scale)
    cloud = E.sample_mesh_points(V, F, thresh).cpu().numpy()
    assert np.array_equal(cloud, R.sample_mesh(V, F, thresh)), "sampled points"
    order = E.shuffle_order(len(cloud), seed)
    sh = cloud[order]
    assert np.array_equal(E.gather(cloud, order).cpu().numpy(), sh)
    keep = E.radius_downsample(sh, thresh)
    assert np.array_equal(keep, R.thin(sh, thresh)), "keep mask"
    keep_o = E.radius_downsample(cloud, thresh, order)
    assert np.array_equal(keep_o[order], keep), "keep mask through an order"
    down = sh[keep]
    rng = np.random.default_rng(seed + 100)
    bb = np.array([[-0.6 * scale, -0.7 * scale, -0.5 * scale], [0.55 * scale, 0.6 * scale, 0.45 * scale]]) + rng.normal(0, 0.01, (2, 3))
    res = 0.37 * scale / 8
    dims = (np.floor((bb[1] - bb[0]) / res).astype(int) + 1)
    mask = (rng.random(dims) < 0.7).astype(np.uint8)
    fl = E.mask_flags(down, mask, bb, res, 0.1 * scale).cpu().numpy()
    inb, obs = R.mask_flags(down, mask, bb, res, 0.1 * scale)
    assert np.array_equal(fl & 1 != 0, inb) and np.array_equal(fl & 2 != 0, obs), "inbound / mask flags"
    assert 0 < obs.sum() < inb.sum() < len(down)
    stl = rng.uniform(-scale, scale, (3000, 3))
    for q, t, md in ((down[obs], stl, 0.3 * scale), (stl, down[inb], 0.05 * scale), (stl, down[inb], 20.0)):
        d = E.nearest_distances(q, t, md)
        r = R.nearest(q, t, md)
        fin = np.isfinite(r)
        assert np.array_equal(np.isinf(d), ~fin), "+inf exactly where >= max_dist"
        assert np.array_equal(d[fin], r[fin]), "distances bit for bit"
        m, n = E.masked_mean(d, md)
        assert n == fin.sum() and _close(m, R.masked_mean(r, md))
    P = np.array([0.3, -0.2, 1.0, 0.1])
    assert np.array_equal(E.above_plane(stl, P).cpu().numpy() != 0, R.above_plane(stl, P))


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


# n = 0; below one workgroup; not a multiple of 256; beyond 256 x 256, so that a thread adds more than one element
FIXED_ORDER_SIZES = [0, 100, 1000, 70001, 200000]


@pytest.mark.parametrize("n", FIXED_ORDER_SIZES)
def test_masked_mean_sums_in_the_fixed_order(n):
    """The sum and the count of gs2m_eval_masked_mean are, to the bit, those of the numpy restatement of the fixed order."""
    import ctypes as C
    import gs2m_native as N
    rng = np.random.default_rng(n)
    md = 20.0
    d = rng.uniform(0, 25, n) * 10.0 ** rng.uniform(-9, 0, n)  # magnitudes apart: the order of the additions shows
    d[rng.random(n) < 0.1] = np.inf
    d[rng.random(n) < 0.05] = md
    dev = torch.device("cuda")
    t = torch.as_tensor(d).to(dev)
    wb = C.c_longlong()
    N.check(N.lib().gs2m_eval_scan_workspace_bytes(0, C.byref(wb)), "gs2m_eval_scan_workspace_bytes")
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    tot, cnt = C.c_double(), C.c_longlong()
    N.launch("gs2m_eval_masked_mean", dev, n, N.ptr(t), md, N.ptr(ws), C.byref(tot), C.byref(cnt))
    want, want_n = R.masked_sum_fixed_order(d, md)
    print("masked mean: n", n, "count", cnt.value, want_n, "sum", tot.value.hex(), want.hex(), "numpy's sum", float(d[d < md].sum()).hex())
    assert cnt.value == want_n
    assert _bits(tot.value) == _bits(want)
    m, c = E.masked_mean(d, md)
    assert c == want_n and (_bits(m) == _bits(want / want_n) if want_n else math.isnan(m))


def test_thinning_adversarial_orders():
    r = 0.2
    # a chain spaced 0.9 r visited in index order: every other point is kept, one decision per round at worst
    chain = np.zeros((3001, 3))
    chain[:, 0] = 0.9 * r * np.arange(3001)
    keep = E.radius_downsample(chain, r)
    assert np.array_equal(keep, R.thin_sequential(chain, r, np.arange(len(chain))))
    assert keep.sum() == 1501
    rev = np.arange(len(chain))[::-1]
    assert np.array_equal(E.radius_downsample(chain, r, rev), R.thin_sequential(chain, r, rev))
    # clusters of exact duplicates and near-duplicates, in a shuffled order
    rng = np.random.default_rng(4)
    centres = rng.uniform(-2, 2, (60, 3))
    pts = np.concatenate([np.repeat(centres, 25, axis=0), centres[:, None].repeat(10, 1).reshape(-1, 3) + rng.normal(0, 0.05, (600, 3))])
    order = rng.permutation(len(pts))
    keep = E.radius_downsample(pts, r, order)
    assert np.array_equal(keep, R.thin_sequential(pts, r, order))


def test_two_runs_are_bitwise_equal():
    c = golden_case("mc")
    a, b = _gpu_eval(c), _gpu_eval(c)
    for k in ("mean_d2s", "mean_s2d", "overall"):
        assert np.array_equal(np.float64(a[k]), np.float64(b[k]))
    for k in a["arrays"]:
        assert np.array_equal(a["arrays"][k], b["arrays"][k]), k


def test_analytic_offset_plane():
    """a square of two right triangles delta above a planar STL grid of step thresh / 2: every sample (p0 + thresh (i + 0.5) along
    the legs) and vertex lies over a grid node, so d2s is delta; s2d adds the STL beyond the square's border, bounded exactly"""
    delta, half, thresh = 0.75, 40.0, 0.2
    V = np.array([[-half, -half, delta], [half, -half, delta], [half, half, delta], [-half, half, delta]])
    F = np.array([[0, 1, 3], [2, 3, 1]], np.int32)  # right angle at the first vertex of each
    g = np.arange(-500, 501) * 0.1
    gx, gy = np.meshgrid(g, g)
    stl = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], axis=1)
    bb = np.array([[-60.0, -60.0, -5.0], [60.0, 60.0, 5.0]])
    mask = np.ones((121, 121, 11), np.uint8)
    r = E.evaluate_mesh(V, F, stl, mask, bb, 1.0, np.array([0.0, 0.0, 1.0, 1.0]), thresh, 60, 20, seed=3)
    assert abs(r["mean_d2s"] - delta) <= 1e-9, r["mean_d2s"]
    assert r["n_d2s_used"] == r["n_in_obs"] > 50000
    # in-plane distance e of every STL point to the square; the thinned points cover the square to within thresh + a sample step
    e = np.hypot(np.maximum(np.abs(stl[:, 0]) - half, 0), np.maximum(np.abs(stl[:, 1]) - half, 0))
    lo, hi = np.sqrt(delta ** 2 + e ** 2).mean(), np.sqrt(delta ** 2 + (e + 2 * thresh) ** 2).mean()
    assert lo - 1e-9 <= r["mean_s2d"] <= hi, (lo, r["mean_s2d"], hi)
    assert r["mean_s2d"] > delta + 1.0  # the border effect is there


def _surface_points(n, centre, scale, t):
    k = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * k / n)
    th = np.pi * (1 + 5 ** 0.5) * k
    sph = np.asarray(centre) + 1.5 * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)
    m = n  # the disc (radius 3, y = 1.5) at about the sphere's density
    rr = 3.0 * np.sqrt((np.arange(m) + 0.5) / m)
    aa = np.pi * (1 + 5 ** 0.5) * np.arange(m)
    disc = np.stack([rr * np.cos(aa), np.full(m, 1.5), rr * np.sin(aa)], axis=1) + [centre[0], 0.0, centre[2]]
    return np.concatenate([sph, disc]) * scale + t


def test_end_to_end_synthetic_surface_through_the_cli(tmp_path):
    import gs2m_mesh as M
    from test_mesh_gpu import _truth_and_cams
    truth, cams = _truth_and_cams(40_000, 10, 320, 240)
    voxel = 0.01
    depths = M.render_views(truth, cams, str(tmp_path / "renders"))
    vol = M.fuse_depths(depths, cams, tmp_path / "renders", 12.0, voxel, 4 * voxel)
    post = M.post_process_mesh(vol.extract_triangle_mesh(), 1)
    M.write_mesh(tmp_path / "tsdf_post.ply", post)
    # DTU layout: the scene in millimetres through scale_mat_0, ground truth on the analytic surface
    scale, t = 20.0, np.array([10.0, -20.0, 300.0])
    S = np.eye(4, dtype=np.float32)
    S[0, 0] = S[1, 1] = S[2, 2] = scale
    S[:3, 3] = t
    ref = tmp_path / "scan7"
    os.makedirs(ref)
    np.savez(ref / "cameras.npz", scale_mat_0=S, world_mat_0=np.eye(4, dtype=np.float32))
    from scipy.io import savemat
    dtu = tmp_path / "dtu"
    os.makedirs(dtu / "ObsMask")
    os.makedirs(dtu / "Points" / "stl")
    centre = (0.0, 0.0, 6.0)
    stl = _surface_points(200_000, centre, scale, t)
    E.write_point_cloud(dtu / "Points" / "stl" / "stl007_total.ply", stl)
    bb = np.stack([stl.min(0) - 5, stl.max(0) + 5])
    res = 2.0
    dims = np.floor((bb[1] - bb[0]) / res).astype(int) + 1
    savemat(str(dtu / "ObsMask" / "ObsMask7_10.mat"), {"ObsMask": np.ones(dims, np.uint8), "BB": bb, "Res": np.array([[res]])})
    # s2d over the part of the sphere the cameras see (world y below 1.2 scene units: the disc and the contact are left out)
    ycut = 1.2 * scale + t[1]
    savemat(str(dtu / "ObsMask" / "Plane7.mat"), {"P": np.array([[0.0, -1.0, 0.0, ycut]])})
    out = tmp_path / "eval"
    E.main(["--input_ply", str(tmp_path / "tsdf_post.ply"), "--ref_dir", str(ref), "--dtu_dir", str(dtu), "--out_dir", str(out)])
    r = json.load(open(out / "results.json"))
    for k in ("mean_d2s", "mean_s2d", "overall"):
        assert k in r and math.isfinite(r[k]), r
    voxel_mm = voxel * scale
    assert r["overall"] <= 3 * voxel_mm and r["mean_d2s"] <= 3 * voxel_mm and r["mean_s2d"] <= 3 * voxel_mm, r
    assert os.path.exists(out / "vis_007_d2s.ply") and os.path.exists(out / "vis_007_s2d.ply")
    print("end to end:", {k: r[k] for k in ("mean_d2s", "mean_s2d", "overall", "n_down", "n_in_obs", "n_stl_above", "ms")})
