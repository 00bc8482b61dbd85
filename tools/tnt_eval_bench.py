"""The Tanks and Temples evaluation timed on a TnT-shaped synthetic job: tools/mesh_bench.py's scene (the radius-1.5 sphere and
the ground disc, 49 orbit views) fused and extracted as the mesh, `--gt` ground-truth points on the analytic surface with
scanner-like noise (tau / 10), a camera trajectory that carries a known similarity error (2 degrees, 1 % scale, a few tau)
into the initial transform, and a concave crop polygon along Y.  One warm-up evaluation, then a timed one; prints one JSON
line: the GPU stage times (load, the three registration stages with their iterations, score, clouds -- the 20-neighbour normals
and the distance colours of the two scored clouds; each ends with a device synchronisation), the point counts, the scores, how far the recovered transform leaves analytic surface points from the
surface (the scene is symmetric about its vertical axis, so the offset's rotation about that axis cannot be observed and
stays in the transform: the transform itself is not compared with the identity), and the CPU
restatement's (tests/tnt_eval_ref.py: numpy + scipy's cKDTree -- NOT the reference's evaluator, which needs Open3D) time on the
stated fraction of the job, and the host formulation of the clouds stage (scipy's cKDTree.query(k=20) on all cores and numpy's
batched eigh, standing in for Open3D's estimate_normals) for `--cpu-points` queries of each scored cloud against the whole
cloud.  There is no reference timing to compare with: no threshold.  All data is synthetic.

    python tools/tnt_eval_bench.py [--views 49] [--voxel 0.004] [--tau 0.01] [--gt 4000000]

`--cell-probe` times something else and renders nothing: one nearest pass shaped like the first two registration stages (the
ground truth downsampled at tau / threshold 80 tau, and at tau / 2 / threshold 20 tau; the queries are the same cloud moved by
the offset, plus 1 % of queries scattered far from the surface) for grid cells of 0.5 to 8 times gs2m_dtu_eval.grid_cell's
edge, one line per cell: near-surface queries, the far ones, all (DESIGN.md section 11's cell-size table).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-2m_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gs2m_tnt_eval as E  # noqa: E402
from dtu_eval_bench import surface_points  # noqa: E402


def similarity(deg, scale, t, axis=(0.3, -0.5, 0.8)):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = scale * (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K))
    T[:3, 3] = t
    return T


def cell_probe(tau, n_gt):
    rng = np.random.default_rng(0)
    gt_full = surface_points(n_gt, 1.0, np.zeros(3)) + rng.normal(0, tau / 10, (n_gt, 3))
    off = similarity(2.0, 1.01, np.array([3.0, -2.0, 2.5]) * tau)

    def timed(grid, q, thr):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index, _ = grid.query(q, thr)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), int((index >= 0).sum())

    for vox, thr in ((tau, 80 * tau), (tau / 2, 20 * tau)):
        gt = E.voxel_downsample(gt_full, vox)
        near = E.transform(gt, off)
        far = torch.as_tensor(np.random.default_rng(1).uniform(-4, 10, (len(near) // 100, 3))).cuda()
        both = torch.cat([near, far])
        base = E.grid_cell(gt, thr)
        for mult in (0.5, 1.0, 2.0, 4.0, 8.0):
            grid = E.TargetGrid(gt, thr, cell=base * mult)
            grid.query(both, thr)  # warm-up
            (t_all, matched), (t_near, _), (t_far, _) = timed(grid, both, thr), timed(grid, near, thr), timed(grid, far, thr)
            print(json.dumps({"voxel": vox, "threshold": thr, "targets": int(len(gt)), "cell": round(base * mult, 5), "x": mult,
                              "near_ms": round(t_near, 2), "far_ms": round(t_far, 2), "all_ms": round(t_all, 2), "matched": matched}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--voxel", type=float, default=0.004)
    ap.add_argument("--tau", type=float, default=0.01)
    ap.add_argument("--gt", type=int, default=4_000_000)
    ap.add_argument("--cpu-points", type=int, default=200_000)
    ap.add_argument("--cell-probe", action="store_true", help="time nearest passes for several grid cells instead (see above)")
    a = ap.parse_args()
    tau = a.tau
    if a.cell_probe:
        return cell_probe(tau, a.gt)
    import gs2m_mesh as M
    import mesh_bench as MB
    cams, depths, colors = MB.scene(200_000, a.views, a.width, a.height)
    lo, hi = M._depth_aabb(depths, cams, 10.0, torch.device("cuda"))
    L, tr = 16 * a.voxel, 4 * a.voxel
    _, mesh, _, _ = MB.fuse(cams, depths, colors, a.voxel, 10.0, 4096, lo - tr - L, hi + tr + L)
    del depths, colors
    rng = np.random.default_rng(0)
    gt = surface_points(a.gt, 1.0, np.zeros(3)) + rng.normal(0, tau / 10, (a.gt, 3))
    # the trajectory: a ring of camera centres; the estimated ones are off by the known similarity, so the initial transform
    # moves the (correctly placed) mesh by it and the registration has to take it back
    off = similarity(2.0, 1.01, np.array([3.0, -2.0, 2.5]) * tau)
    ang = np.linspace(0, 2 * np.pi, 60, endpoint=False)
    centres = np.stack([6 * np.cos(ang), -0.8 + 0.5 * np.sin(3 * ang), 6 + 6 * np.sin(ang)], axis=1)
    ref = np.tile(np.eye(4), (60, 1, 1))
    ref[:, :3, 3] = centres
    est = ref.copy()
    est[:, :3, 3] = (centres - off[:3, 3]) @ np.linalg.inv(off[:3, :3]).T
    r8 = np.array([2.9, 2.7, 2.9, 1.6, 2.8, 2.9, 2.6, 2.9])  # a concave octagon around the scene's axis, in (x, z)
    pa = np.linspace(0, 2 * np.pi, 8, endpoint=False)
    vol = {"orthogonal_axis": "Y", "axis_min": -2.0, "axis_max": 1.6,
           "bounding_polygon": np.stack([r8 * np.cos(pa), np.zeros(8), 6.0 + r8 * np.sin(pa)], axis=1)}
    run = lambda: E.evaluate_scene(mesh.vertices, mesh.triangles, gt, vol, tau, est, ref, np.eye(4), scene="synthetic", clouds=True)  # noqa: E731
    run()
    torch.cuda.reset_peak_memory_stats()
    r = run()
    peak = torch.cuda.max_memory_allocated()
    T = np.asarray(r["transformation"])
    # the mesh is in place, so T should map the surface onto itself: distance of moved surface points to the sphere / the disc
    q = surface_points(20000, 1.0, np.zeros(3)) @ T[:3, :3].T + T[:3, 3]
    d_sph = np.abs(np.linalg.norm(q - np.array([0.0, 0.0, 6.0]), axis=1) - 1.5)
    d_disc = np.hypot(np.maximum(np.hypot(q[:, 0], q[:, 2] - 6.0) - 3.0, 0.0), q[:, 1] - 1.5)
    off_surface = np.minimum(d_sph, d_disc)
    # the CPU restatement on a fraction of the same job
    import tnt_eval_ref as R
    part = gt[: a.cpu_points]
    t0 = time.perf_counter()
    down = R.voxel_downsample(R.crop(part, vol), tau / 2)
    t_down = time.perf_counter() - t0
    tgt = E.voxel_downsample(E.crop(gt, vol), tau / 2).cpu().numpy()
    t0 = time.perf_counter()
    R.nearest(down, tgt, 5 * tau, kdtree=True)
    t_nn = time.perf_counter() - t0
    # the clouds stage's host formulation on a part of the same clouds
    from scipy.spatial import cKDTree
    host = {}
    for name, c in r["clouds"].items():
        pts = c["points"].cpu().numpy()
        q = pts[: a.cpu_points]
        t0 = time.perf_counter()
        _, idx = cKDTree(pts).query(q, k=20, workers=-1)
        t_knn = time.perf_counter() - t0
        t0 = time.perf_counter()
        nb = pts[idx]
        nb = nb - nb.mean(axis=1, keepdims=True)
        np.linalg.eigh(np.einsum("nki,nkj->nij", nb, nb))
        t_eig = time.perf_counter() - t0
        host[name] = {"points": len(pts), "queries": len(q), "tree_and_knn_ms": round(1e3 * t_knn, 1), "eigh_ms": round(1e3 * t_eig, 1)}
    print(json.dumps({
        "workload": f"{a.views} views {a.width}x{a.height}, voxel {a.voxel}, synthetic surface scene, tau {tau}, {a.gt} ground-truth points, "
                    "initial transform off by 2 degrees / 1 % / a few tau",
        "gpu_ms": r["ms"], "gpu_ms_total": round(sum(r["ms"].values()), 3), "peak_device_bytes": int(peak),
        "stages": [{k: s[k] for k in ("method", "iterations", "fitness", "rmse", "n_source", "n_target", "ms")} for s in r["stages"]],
        "counts": {k: r[k] for k in ("n_vertices", "n_triangles", "n_source", "n_gt", "n_gt_cropped", "n_source_scored", "n_target_scored")},
        "scores": {k: r[k] for k in ("precision", "recall", "fscore")},
        "surface_to_surface_under_T": {"mean": float(off_surface.mean()), "max": float(off_surface.max()), "tau": tau},
        "clouds_host_formulation_not_open3d": host,
        "cpu_restatement_not_the_reference": {"gt_points": len(part), "of": a.gt, "crop_voxel_ms": round(1e3 * t_down, 1),
                                              "nearest_queries": len(down), "nearest_targets": len(tgt), "nearest_ms": round(1e3 * t_nn, 1)}}))


if __name__ == "__main__":
    main()
