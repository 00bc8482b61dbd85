"""Tanks and Temples evaluation of a mesh on the GPU (csrc/tnt_eval.hip, csrc/mesh_eval.hip; include/gs2m_tnt.h, gs2m_eval.h).

The score GS-2M reports for Barn and Truck: the reference's scripts/eval_tnt/run.py (precision / recall / F-score), as
DESIGN.md §11 writes the contract down.  The mesh becomes a cloud (vertices and triangle centres), is aligned to the
ground-truth scan -- the camera trajectories give the initial similarity, three ICP refinements with scaling follow -- and
both clouds are cropped to the scene's polygon volume, voxel-downsampled and scored by their nearest-neighbour distances.
Transform, crop, downsampling, nearest neighbours, the ICP moment sums and the histograms run in HIP kernels, all in fp64;
the 3 x 3 similarity update is numpy on the host.  Every buffer is a torch tensor owned here.  Where Open3D decides what the
reference computes, the contract is Open3D's behaviour as read, unpinned: Open3D is not part of this stack.

    python gs-2m_amd/gs2m_tnt_eval.py --dataset-dir TNT/Barn --traj-path TNT/Barn/Barn_COLMAP_SfM.log --ply-path tsdf_post.ply
writes evaluation/{results.json, Barn.precision.txt, Barn.recall.txt, Barn.prf_tau_plotstr.txt, Barn.precision.ply,
Barn.recall.ply} beside the ply: the two scored clouds, each point with its 20-neighbour normal and hot_r of its distance to the
other cloud, capped at 3 tau (csrc/tnt_clouds.hip; --no-clouds skips them).  --plot adds plot.py's PR_<scene>_@d_th_0_<tau>.png
and .pdf (matplotlib, on the host).
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np
import torch

import gs2m_native as N
from gs2m_eval_util import (TargetGrid, compact as _compact, device as _dev, grid_cell, masked_mean, points as _points,  # noqa: F401
                            ptr as _ptr, read_ply, triangles_i32, workspace as _ws, workspace_for, write_point_cloud)

# scripts/eval_tnt/config.py: the distance threshold tau of every scene
SCENES_TAU = {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003, "Meetingroom": 0.01,
              "Truck": 0.005}
MAX_POINT_NUMBER = 4e6  # registration.py: clouds above it are thinned by rows for the last ICP stage
PLOT_STRETCH = 5
KNN = 20            # evaluation.py: estimate_normals(KDTreeSearchParamKNN(knn=20))
COLOR_STRETCH = 3   # evaluation.py: write_color_distances(..., 3 * threshold)
_AXES = {"X": 0, "Y": 1, "Z": 2}


# ---- the steps, on device tensors ----------------------------------------------------------------------------------------

def mesh_points(vertices, triangles, device=None):
    """The source cloud: the vertices in file order, then ((p0 + p1) + p2) / 3 of every triangle.  -> (V + F, 3) tensor."""
    dev = _dev(device)
    v = _points(vertices, dev)
    f = triangles_i32(triangles, dev)
    cloud = torch.empty((len(v) + len(f), 3), dtype=torch.float64, device=dev)
    ws = _ws(8, dev)
    N.launch("gs2m_tnt_mesh_points", dev, len(v), _ptr(v), len(f), _ptr(f), _ptr(ws), _ptr(cloud))
    return cloud


def _mat16(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    return (C.c_double * 16)(*[float(x) for x in T.reshape(-1)])


def transform(points, T, out=None, device=None):
    """x' = ((T00 x + T01 y) + T02 z) + T03 per row of the 4 x 4 `T` (last row (0, 0, 0, 1)).  out: may be `points` itself."""
    dev = _dev(device)
    p = _points(points, dev)
    out = torch.empty_like(p) if out is None else out
    N.launch("gs2m_tnt_transform", dev, len(p), _ptr(p), _mat16(T), _ptr(out))
    return out


def _volume(volume):
    axis = str(volume["orthogonal_axis"]).upper()
    if axis not in _AXES:
        raise ValueError(f"gs2m_tnt_eval: orthogonal_axis {volume['orthogonal_axis']!r} is not X, Y or Z")
    poly = np.ascontiguousarray(np.asarray(volume["bounding_polygon"], np.float64).reshape(-1, 3))
    if len(poly) > 1024:
        raise ValueError(f"gs2m_tnt_eval: a bounding polygon of {len(poly)} vertices (at most 1024 are taken)")
    return _AXES[axis], float(volume["axis_min"]), float(volume["axis_max"]), poly


def crop_flags(points, volume, device=None):
    """1 per point inside the SelectionPolygonVolume `volume` (dict: orthogonal_axis, axis_min, axis_max, bounding_polygon).
    -> uint8 tensor."""
    dev = _dev(device)
    p = _points(points, dev)
    axis, lo, hi, poly = _volume(volume)
    flags = torch.empty(len(p), dtype=torch.uint8, device=dev)
    N.launch("gs2m_tnt_crop_flags", dev, len(p), _ptr(p), axis, lo, hi, len(poly), poly.ctypes.data_as(C.c_void_p), _ptr(flags))
    return flags


def crop(points, volume, device=None):
    dev = _dev(device)
    p = _points(points, dev)
    return _compact(p, crop_flags(p, volume, dev), 0, dev).clone()


def voxel_downsample(points, s, device=None):
    """One point per occupied voxel of edge `s`: the mean of its members, summed in input order; voxels in ascending
    (ix, iy, iz) order."""
    dev = _dev(device)
    p = _points(points, dev)
    ws = workspace_for("gs2m_tnt_voxel_workspace_bytes", dev, len(p))
    out = torch.empty_like(p)
    cnt = C.c_longlong()
    N.launch("gs2m_tnt_voxel_downsample", dev, len(p), _ptr(p), float(s), _ptr(ws), _ptr(out), C.byref(cnt))
    return out[:cnt.value].clone()


def uniform_downsample(points, limit=MAX_POINT_NUMBER, device=None):
    """registration.py's "uniform" method: above `limit` points every k-th row, k = int(round(n / limit)); else the cloud."""
    dev = _dev(device)
    p = _points(points, dev)
    if not len(p) > limit:
        return p
    k = int(round(len(p) / float(limit)))
    out = torch.empty(((len(p) + k - 1) // k, 3), dtype=torch.float64, device=dev)
    N.launch("gs2m_tnt_stride_gather", dev, len(p), _ptr(p), k, _ptr(out))
    return out


def nearest(queries, targets, max_dist, cell=None, device=None):
    """For every query the index (in the targets' given order; the lowest among equals) and the distance of its nearest target
    where that is < max_dist; else -1 and +inf.  -> (index, dist) tensors."""
    return TargetGrid(targets, max_dist, cell, device).query(queries, max_dist)


def icp_moments(source, targets, index, device=None):
    """One ICP evaluation's sums over the pairs with index >= 0, in a fixed order on the device.
    -> dict(c, sum_d2, mx, my, sigma, sx2)."""
    dev = _dev(device)
    x, t = _points(source, dev), _points(targets, dev)
    idx = torch.as_tensor(index).to(dev, torch.int64).contiguous()
    ws = workspace_for("gs2m_tnt_icp_workspace_bytes", dev)
    cnt, out = C.c_longlong(), (C.c_double * 17)()
    N.launch("gs2m_tnt_icp_moments", dev, len(x), _ptr(x), len(t), _ptr(t), _ptr(idx), _ptr(ws), C.byref(cnt), out)
    o = np.array(out[:], np.float64)
    return {"c": cnt.value, "sum_d2": float(o[0]), "mx": o[1:4].copy(), "my": o[4:7].copy(), "sigma": o[7:16].reshape(3, 3).copy(),
            "sx2": float(o[16])}


def umeyama_update(m):
    """The similarity (4 x 4) of Open3D's TransformationEstimationPointToPoint(with_scaling=True) from the moments:
    U D V^T = svd(Sigma), S = diag(1, 1, sign(det U det V)), R = U S V^T, scale = trace(D S) / sx2, t = my - scale R mx."""
    U, D, Vt = np.linalg.svd(m["sigma"])
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    scale = float((D * np.diag(S)).sum()) / m["sx2"]
    T = np.eye(4)
    T[:3, :3] = scale * R
    T[:3, 3] = m["my"] - scale * (R @ m["mx"])
    return T


def icp(source, target, thr, max_itr, device=None):
    """registration_icp, point to point with scaling, from the identity, criteria (1e-6, 1e-6, max_itr).  The target grid is
    built once; the moved source stays on the device.  -> (T (4, 4) numpy, fitness, rmse, iterations)."""
    dev = _dev(device)
    src = _points(source, dev).clone()
    grid = TargetGrid(target, thr, device=dev)

    def evaluate_once():
        index, _ = grid.query(src, thr)
        m = icp_moments(src, grid.targets, index, dev)
        c = m["c"]
        return m, (c / len(src) if c else 0.0), (math.sqrt(m["sum_d2"] / c) if c else 0.0)

    T = np.eye(4)
    m, fitness, rmse = evaluate_once()
    it = 0
    for _ in range(int(max_itr)):
        if m["c"] < 3:
            break
        upd = umeyama_update(m)
        T = upd @ T
        transform(src, upd, out=src, device=dev)  # the update moves the already-moved cloud, as Open3D does
        prev = (fitness, rmse)
        m, fitness, rmse = evaluate_once()
        it += 1
        if abs(fitness - prev[0]) < 1e-6 and abs(rmse - prev[1]) < 1e-6:
            break
    return T, fitness, rmse, it


class GroundTruth:
    """The ground-truth scan cropped once to the volume and kept on the device, with its voxel downsamples by edge."""

    def __init__(self, points, volume, device=None):
        self.dev = _dev(device)
        self.n_raw = len(points)
        self.cropped = crop(points, volume, self.dev)
        self._voxels = {}

    def voxels(self, s):
        if s not in self._voxels:
            self._voxels[s] = voxel_downsample(self.cropped, s, self.dev)
        return self._voxels[s]


def _gt(gt, volume, dev):
    return gt if isinstance(gt, GroundTruth) else GroundTruth(gt, volume, dev)


def register(source, gt, T0, volume, tau, limit=MAX_POINT_NUMBER, device=None):
    """run.py's three refinements, each from the one before: voxel tau / threshold 80 tau, voxel tau / 2 / threshold 20 tau,
    uniform / threshold 2 tau; 20 iterations each.  gt: points or a GroundTruth.  -> (T (4, 4) numpy, [per stage: dict])."""
    dev = _dev(device)
    src0 = _points(source, dev)
    g = _gt(gt, volume, dev)
    T = np.asarray(T0, np.float64).reshape(4, 4).copy()
    stages = []
    for kind, vox, thr in (("voxel", tau, 80 * tau), ("voxel", tau / 2.0, 20 * tau), ("uniform", None, 2 * tau)):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        s = crop(transform(src0, T, device=dev), volume, dev)
        if kind == "voxel":
            s, t = voxel_downsample(s, vox, dev), g.voxels(vox)
        else:
            s, t = uniform_downsample(s, limit, dev), uniform_downsample(g.cropped, limit, dev)
        Ti, fit, rmse, it = icp(s, t, thr, 20, dev)
        T = Ti @ T
        torch.cuda.synchronize(dev)
        stages.append({"method": kind, "voxel": vox, "threshold": thr, "iterations": it, "fitness": fit, "rmse": rmse,
                       "n_source": int(len(s)), "n_target": int(len(t)), "ms": round(1e3 * (time.perf_counter() - t0), 3)})
    return T, stages


def fit_similarity(x, y):
    """The update of `umeyama_update` fitted to the pairs x[i] -> y[i] (host, numpy: a few hundred camera centres)."""
    x, y = np.asarray(x, np.float64).reshape(-1, 3), np.asarray(y, np.float64).reshape(-1, 3)
    mx, my = x.sum(0) / len(x), y.sum(0) / len(y)
    a, b = x - mx, y - my
    sigma = (b[:, :, None] * a[:, None, :]).sum(0) / len(x)
    return umeyama_update({"sigma": sigma, "sx2": float((a * a).sum()) / len(x), "mx": mx, "my": my})


def _host_transform(p, T):
    return p @ T[:3, :3].T + T[:3, 3]


def align_trajectories(est, gt, gt_trans=None, dist=0.2, min_pairs=6, max_rounds=20):
    """The initial similarity from the camera centres est[i] <-> gt_trans gt[i] (poses (n, 4, 4)).  The reference draws an
    unseeded RANSAC (distance 0.2, 6 points); here, deterministically: fit all pairs, keep those within `dist` of their
    partner under the fit, refit, until the kept set stands still (at most `max_rounds` fits)."""
    x = np.asarray(est, np.float64).reshape(-1, 4, 4)[:, :3, 3]
    y = np.asarray(gt, np.float64).reshape(-1, 4, 4)[:, :3, 3]
    if gt_trans is not None:
        y = _host_transform(y, np.asarray(gt_trans, np.float64).reshape(4, 4))
    if len(x) != len(y):
        raise ValueError(f"gs2m_tnt_eval: {len(x)} estimated poses for {len(y)} reference poses (the correspondence is i <-> i)")
    keep = np.ones(len(x), bool)
    T = None
    for _ in range(max_rounds):
        if keep.sum() < min_pairs:
            raise ValueError(f"gs2m_tnt_eval: only {int(keep.sum())} camera pairs agree within {dist}; {min_pairs} are needed")
        T = fit_similarity(x[keep], y[keep])
        new = np.linalg.norm(_host_transform(x, T) - y, axis=1) < dist
        if np.array_equal(new, keep):
            break
        keep = new
    return T


def histogram(dist, edges, device=None):
    """numpy.histogram's counts of `dist` for the given `edges` (right-open bins, the last one closed), counted on the device.
    -> int64 numpy."""
    dev = _dev(device)
    d = torch.as_tensor(dist).to(dev, torch.float64).contiguous()
    e = torch.as_tensor(np.asarray(edges, np.float64)).to(dev).contiguous()
    counts = torch.zeros(max(len(e) - 1, 1), dtype=torch.int64, device=dev)
    N.launch("gs2m_tnt_histogram", dev, len(d), _ptr(d), len(e), _ptr(e), _ptr(counts))
    return counts[:len(e) - 1].cpu().numpy()


def _device_tensor(t, name, who):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{who}: `{name}` must be a tensor on a HIP device; there is no CPU path")
    return t


def knn_normals(points, k=KNN, device=None, return_index=False, cell=None):
    """estimate_normals(KDTreeSearchParamKNN(knn=k)) of the cloud `points` ((n, 3) device tensor): per point the unit
    eigenvector of the smallest eigenvalue of its k nearest neighbours' covariance (the point itself among them, ties to the
    lower index; include/gs2m_tnt.h states the rules and the fixed sign).  cell: the grid's edge (default: grid_cell over the
    cloud's extent).  -> (n, 3) fp64 device tensor; with `return_index` also the (n, k) int64 neighbour indices in (d2, index)
    order, -1 beyond min(k, n)."""
    dev = _dev(device)
    p = _points(_device_tensor(points, "points", "knn_normals"), dev)
    n = len(p)
    if not 1 <= int(k) <= 32:  # the library's own refusal, whatever the cloud
        N.launch("gs2m_tnt_knn_normals", dev, n, None, 1.0, None, int(k), None, None, None)
    normals = torch.empty((n, 3), dtype=torch.float64, device=dev)
    index = torch.empty((n, int(k)), dtype=torch.int64, device=dev) if return_index else None
    if n:
        if not cell:
            lo, hi = torch.aminmax(p, dim=0)
            ext = float((hi - lo).max())
            cell = grid_cell(p, ext) if ext > 0 and math.isfinite(ext) else 1.0
        grid = TargetGrid(p, cell, cell=cell, device=dev)
        ws = workspace_for("gs2m_tnt_knn_normals_workspace_bytes", dev, n)
        N.launch("gs2m_tnt_knn_normals", dev, n, _ptr(p), float(cell), _ptr(grid.grid), int(k), _ptr(ws), _ptr(normals), _ptr(index))
    return (normals, index) if return_index else normals


def distance_colors(dist, max_distance, device=None):
    """write_color_distances' colours: hot_r(min(d, max_distance) / max_distance) as matplotlib indexes its 256 entries, each
    channel round(c * 255).  dist: (n,) device tensor (+inf takes the cap's colour; NaN is refused).  -> (n, 3) uint8 device
    tensor."""
    dev = _dev(device)
    d = _device_tensor(dist, "dist", "distance_colors").to(dev, torch.float64).reshape(-1).contiguous()
    rgb = torch.empty((len(d), 3), dtype=torch.uint8, device=dev)
    ws = _ws(8, dev)
    N.launch("gs2m_tnt_distance_colors", dev, len(d), _ptr(d), float(max_distance), _ptr(ws), _ptr(rgb))
    return rgb


def evaluate(source, gt, T, volume, tau, details=False, device=None, clouds=False):
    """EvaluateHisto: source moved by T, both clouds cropped and voxel-downsampled at tau / 2, distances capped at 5 tau (+inf
    there: every number below treats values from 5 tau on alike).  -> dict(precision, recall, fscore, n_source, n_target,
    edges, cum_source, cum_target); with `details` also the clouds and distances (numpy); with `clouds` also "clouds": the
    precision cloud (the source, coloured by distance1) and the recall cloud (the target, by distance2) as device tensors:
    dict(precision / recall: dict(points, normals, colors)), colours capped at 3 tau."""
    dev = _dev(device)
    g = _gt(gt, volume, dev)
    s = voxel_downsample(crop(transform(source, T, device=dev), volume, dev), tau / 2.0, dev)
    t = g.voxels(tau / 2.0)
    cap = PLOT_STRETCH * tau
    _, d1 = TargetGrid(t, cap, device=dev).query(s, cap)
    _, d2 = TargetGrid(s, cap, device=dev).query(t, cap)
    edges = np.arange(0, tau * PLOT_STRETCH, tau / 100)
    if len(s) and len(t):
        precision = float(masked_mean(d1, tau, dev)[1]) / float(len(s))
        recall = float(masked_mean(d2, tau, dev)[1]) / float(len(t))
        fscore = 2 * recall * precision / (recall + precision) if recall + precision != 0 else 0.0
        cum1 = np.cumsum(histogram(d1, edges, dev)).astype(float) / len(s)
        cum2 = np.cumsum(histogram(d2, edges, dev)).astype(float) / len(t)
    else:
        precision = recall = fscore = 0
        edges = cum1 = cum2 = np.array([0])
    out = {"precision": precision, "recall": recall, "fscore": fscore, "n_source": int(len(s)), "n_target": int(len(t)),
           "edges": edges, "cum_source": cum1, "cum_target": cum2}
    if details:
        out["arrays"] = {"source": s.cpu().numpy(), "target": t.cpu().numpy(), "distance1": d1.cpu().numpy(), "distance2": d2.cpu().numpy()}
    if clouds:  # after everything above, which it leaves as it is; timed on its own
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        # a voxel downsample at tau / 2 leaves about one point per tau / 2 of surface: cells of three spacings hold the 20
        # neighbours within the first shell for most points
        out["clouds"] = {name: {"points": p, "normals": knn_normals(p, KNN, dev, cell=1.5 * tau),
                                "colors": distance_colors(d, COLOR_STRETCH * tau, dev)}
                         for name, p, d in (("precision", s, d1), ("recall", t, d2))}
        torch.cuda.synchronize(dev)
        out["clouds_ms"] = 1e3 * (time.perf_counter() - t0)
    return out


def rotation_y(theta):
    """run_tnt.py's pre-rotation of the Truck mesh: about y through the origin"""
    c, s = math.cos(theta), math.sin(theta)
    return np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], np.float64)


def plot_graph(scene, fscore, tau, edges, cum_source, cum_target, out_dir, stretch=PLOT_STRETCH):
    """plot.py's plot_graph: precision (red) and recall (blue) in per cent over the distance, tau dashed, as
    PR_<scene>_@d_th_0_<tau * 10000, four digits>.png and .pdf in out_dir.  matplotlib is imported here, with the Agg backend.
    -> (png, pdf)."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig = plt.figure(figsize=(14, 7))
    ax = fig.add_subplot(111)
    ax.plot(np.asarray(edges)[1:], np.asarray(cum_source) * 100, c="red", label="precision", linewidth=2.0)
    ax.plot(np.asarray(edges)[1:], np.asarray(cum_target) * 100, c="blue", label="recall", linewidth=2.0)
    ax.grid(True)
    ax.set_title("Precision and Recall: " + scene + ", " + "%02.2f f-score" % (fscore * 100))
    ax.axvline(x=tau, c="black", ls="dashed", linewidth=2.0)
    ax.set_ylabel("# of points (%)", fontsize=15)
    ax.set_xlabel("Meters", fontsize=15)
    ax.axis([0, tau * stretch, 0, 100])
    box = ax.get_position()
    ax.set_position([box.x0, box.y0, box.width * 0.8, box.height])
    ax.legend(loc="center left", bbox_to_anchor=(1, 0.5), fontsize="medium")
    stem = os.path.join(out_dir, "PR_{0}_@d_th_0_{1}".format(scene, "%04d" % (tau * 10000)))
    fig.savefig(stem + ".png", format="png", bbox_inches="tight")
    fig.savefig(stem + ".pdf", format="pdf", bbox_inches="tight")
    plt.close(fig)
    return stem + ".png", stem + ".pdf"


def evaluate_scene(vertices, triangles, gt_points, volume, tau, est_traj, gt_traj, gt_trans, scene="scene", out_dir=None,
                   rotate_y=0.0, details=False, device=None, clouds=None, plot=False):
    """run.py's run_evaluation.  vertices (V, 3), triangles (F, 3): the mesh; gt_points (M, 3); volume: the crop (dict);
    est_traj, gt_traj: (n, 4, 4) poses; gt_trans (4, 4).  -> dict(precision, recall, fscore, tau, counts, the stages, the final
    transformation, times in ms; cum_source / cum_target; with `details` the arrays); out_dir: the reference's files:
    results.json, the three .txt files, with `clouds` (default: when there is an out_dir) <scene>.precision.ply and
    <scene>.recall.ply, with `plot` plot_graph's figure.  ms["clouds"]: the normals and colours on the device (the score's time
    does not hold them); writing the two files is host time and is not in it."""
    dev = _dev(device)
    times = {}
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    v = _points(vertices, dev)
    if rotate_y:
        v = transform(v, rotation_y(rotate_y), device=dev)
    source = mesh_points(v, triangles, dev)
    g = GroundTruth(gt_points, volume, dev)
    T0 = align_trajectories(est_traj, gt_traj, gt_trans)
    torch.cuda.synchronize(dev)
    times["load"] = round(1e3 * (time.perf_counter() - t0), 3)
    T, stages = register(source, g, T0, volume, tau, device=dev)
    for k, st in enumerate(stages):
        times[f"register{k}"] = st["ms"]
    t0 = time.perf_counter()
    clouds = out_dir is not None if clouds is None else bool(clouds)
    r = evaluate(source, g, T, volume, tau, details, dev, clouds)
    torch.cuda.synchronize(dev)
    times["score"] = round(1e3 * (time.perf_counter() - t0) - r.get("clouds_ms", 0.0), 3)
    if clouds:
        times["clouds"] = round(r["clouds_ms"], 3)
    out = {"precision": r["precision"], "recall": r["recall"], "fscore": r["fscore"], "tau": tau, "scene": scene,
           "n_vertices": int(len(v)), "n_triangles": int(len(triangles)), "n_source": int(len(source)), "n_gt": int(g.n_raw),
           "n_gt_cropped": int(len(g.cropped)), "n_source_scored": r["n_source"], "n_target_scored": r["n_target"],
           "stages": stages, "initial_transformation": T0.tolist(), "transformation": T.tolist(), "ms": times}
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "results.json"), "w") as f:
            json.dump(out, f, indent=2)
        np.savetxt(os.path.join(out_dir, f"{scene}.recall.txt"), r["cum_target"])
        np.savetxt(os.path.join(out_dir, f"{scene}.precision.txt"), r["cum_source"])
        np.savetxt(os.path.join(out_dir, f"{scene}.prf_tau_plotstr.txt"), np.array([r["precision"], r["recall"], r["fscore"], tau, PLOT_STRETCH]))
        if clouds:
            for name, c in r["clouds"].items():
                write_point_cloud(os.path.join(out_dir, f"{scene}.{name}.ply"), c["points"].cpu().numpy(),
                                  c["colors"].cpu().numpy() / 255.0, c["normals"].cpu().numpy())
        if plot:
            plot_graph(scene, r["fscore"], tau, r["edges"], r["cum_source"], r["cum_target"], out_dir)
    out["edges"], out["cum_source"], out["cum_target"] = r["edges"], r["cum_source"], r["cum_target"]
    if details:
        out["arrays"] = r["arrays"]
    if clouds:
        out["clouds"] = r["clouds"]
    return out


# ---- files -------------------------------------------------------------------------------------------------------------------

def read_trajectory_log(file):
    """The .log trajectory format (trajectory_io.py): per pose a line of integers, then the four rows of the 4 x 4 matrix.
    -> (n, 4, 4) fp64."""
    poses = []
    with open(str(file), "r") as f:
        lines = f.read().split("\n")
    k = 0
    while k < len(lines) and lines[k] != "":
        rows = lines[k + 1:k + 5]
        if len(rows) < 4:
            raise ValueError(f"{file}: the pose after line {k + 1} is cut short")
        poses.append([[float(x) for x in row.split()] for row in rows])
        k += 5
    return np.array(poses, np.float64).reshape(-1, 4, 4)


def read_trajectory(file):
    """run.py's three trajectory forms: .log, .npy ((n, 4, 4)); the .json form is refused."""
    file = str(file)
    if file.endswith(".npy"):
        return np.asarray(np.load(file), np.float64).reshape(-1, 4, 4)
    if file.endswith(".json"):
        raise ValueError(f"{file}: a .json trajectory needs the reference's auto_orient_and_center_poses, which is not provided here; "
                         "convert it to the .log or .npy form")
    return read_trajectory_log(file)


def read_crop_volume(file):
    """Open3D's SelectionPolygonVolume JSON -> dict(orthogonal_axis, axis_min, axis_max, bounding_polygon (m, 3)); other keys
    are ignored."""
    with open(str(file)) as f:
        d = json.load(f)
    axis = str(d["orthogonal_axis"]).upper()
    if axis not in _AXES:
        raise ValueError(f"{file}: orthogonal_axis {d['orthogonal_axis']!r} is not X, Y or Z")
    return {"orthogonal_axis": axis, "axis_min": float(d["axis_min"]), "axis_max": float(d["axis_max"]),
            "bounding_polygon": np.asarray(d["bounding_polygon"], np.float64).reshape(-1, 3)}


def visibility_cull(vertices, triangles, c2w, out_ply=None, device=None, **options):
    """The mesh culled against the camera-to-world poses `c2w` (gs2m_mesh_cull.cull_mesh_by_visibility; options: its keyword
    arguments, by default the Tanks and Temples frame and constants), written to `out_ply` when given.
    -> (vertices, triangles) device tensors, dict(the counts before and after)."""
    import types
    import gs2m_mesh as M
    import gs2m_mesh_cull as K
    dev = _dev(device)
    v, f = _points(vertices, dev), triangles_i32(triangles, dev)
    o = dict(fx=K.TNT_FX, fy=K.TNT_FY, cx=K.TNT_CX, cy=K.TNT_CY, H=K.TNT_HEIGHT, W=K.TNT_WIDTH)
    o.update(options)
    cv, cf, _ = K.cull_mesh_by_visibility(v, f, torch.as_tensor(K.world_to_camera(c2w)).to(dev), **o)
    if out_ply is not None:
        os.makedirs(os.path.dirname(os.path.abspath(out_ply)), exist_ok=True)
        M.write_mesh(out_ply, types.SimpleNamespace(vertices=cv.cpu().numpy(), triangles=cf.cpu().numpy(), vertex_colors=np.zeros((len(cv), 3))))
    return cv, cf, {"n_vertices": int(len(v)), "n_triangles": int(len(f)), "n_vertices_kept": int(len(cv)), "n_triangles_kept": int(len(cf))}


# ---- command line: run.py ------------------------------------------------------------------------------------------------

def main(argv=None):
    ap = argparse.ArgumentParser(description="Tanks and Temples precision / recall / F-score of a mesh (scripts/eval_tnt/run.py)")
    ap.add_argument("--dataset-dir", required=True, help="the scene folder: X.ply, X.json, X_trans.txt, X_COLMAP_SfM.log")
    ap.add_argument("--traj-path", required=True, help="the reconstruction's camera trajectory (.log or .npy)")
    ap.add_argument("--ply-path", required=True, help="the mesh to evaluate (binary PLY)")
    ap.add_argument("--out-dir", default="", help="default: evaluation/ beside the ply")
    ap.add_argument("--scene", default="", help="default: the dataset folder's name")
    ap.add_argument("--tau", type=float, default=None, help="the distance threshold (default: the scene's)")
    ap.add_argument("--rotate-y", type=float, default=0.0, help="rotate the mesh about y first (run_tnt.py: pi / 8 for Truck)")
    ap.add_argument("--no-clouds", action="store_true", help="do not write <scene>.precision.ply and <scene>.recall.ply")
    ap.add_argument("--plot", action="store_true", help="write the precision / recall figure (png and pdf; needs matplotlib)")
    ap.add_argument("--visibility-cull", action="store_true", help="cull the mesh against --traj-path's cameras first (gs2m_mesh_cull.py with "
                    "its defaults: the Tanks and Temples frame, 20 views) and write culled_mesh.ply beside the results")
    a = ap.parse_args(argv)
    scene = a.scene or os.path.basename(os.path.normpath(a.dataset_dir))
    if a.tau is None and scene not in SCENES_TAU:
        ap.error(f"scene {scene!r} is not one of {sorted(SCENES_TAU)}: give --tau")
    tau = a.tau if a.tau is not None else SCENES_TAU[scene]
    out_dir = a.out_dir.strip() or os.path.join(os.path.dirname(a.ply_path), "evaluation")
    verts, tris = read_ply(a.ply_path)
    culled = None
    if a.visibility_cull:
        verts, tris, culled = visibility_cull(verts, tris, read_trajectory(a.traj_path), os.path.join(out_dir, "culled_mesh.ply"))
    gt, _ = read_ply(os.path.join(a.dataset_dir, scene + ".ply"))
    r = evaluate_scene(verts, tris, gt, read_crop_volume(os.path.join(a.dataset_dir, scene + ".json")), tau,
                       read_trajectory(a.traj_path), read_trajectory_log(os.path.join(a.dataset_dir, scene + "_COLMAP_SfM.log")),
                       np.loadtxt(os.path.join(a.dataset_dir, scene + "_trans.txt")), scene=scene, out_dir=out_dir, rotate_y=a.rotate_y,
                       clouds=not a.no_clouds, plot=a.plot)
    if culled is not None:
        r["visibility_cull"] = culled
    print(f"[>] {scene}: tau {tau:.3f} precision {r['precision']:.4f} recall {r['recall']:.4f} f-score {r['fscore']:.4f}")
    return r


if __name__ == "__main__":
    main()
