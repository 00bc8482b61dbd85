"""DTU Chamfer evaluation of a mesh on the GPU (csrc/mesh_eval.hip, include/gs2m_eval.h).

The score GS-2M reports for its extracted mesh: the reference's scripts/eval_dtu/evaluate_single_scene.py (the scale-matrix
step, without --mask_cull) followed by eval.py in mesh mode, as DESIGN.md §10 writes the contract down.  The mesh is sampled
on every triangle, shuffled with a seeded numpy generator, thinned to `downsample_density`, cut to the observation mask and
scored against the ground-truth STL points in both directions.  Sampling, thinning, the filters and the nearest-neighbour
distances run in HIP kernels, all in fp64; every buffer is a torch tensor owned here.

    python gs-2m_amd/gs2m_dtu_eval.py --input_ply tsdf_post.ply --ref_dir DTU/scan24 --dtu_dir Offical_DTU_Dataset --out_dir OUT
writes OUT/results.json (mean_d2s, mean_s2d, overall, plus counts, seed and stage times) and OUT/vis_XXX_{d2s,s2d}.ply.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np
import torch

import gs2m_native as N
from gs2m_eval_util import (TargetGrid, compact as _compact, device as _dev, grid_cell, masked_mean, points as _points,  # noqa: E402,F401
                            ptr as _ptr, read_ply, triangles_i32, workspace_for, write_point_cloud)


# ---- the steps, on device tensors ----------------------------------------------------------------------------------------

def world_transform(vertices, scale_mat, device=None):
    """evaluate_single_scene.py's step without --mask_cull: v * S[0, 0] + S[:3, 3] in fp64, S the float32 scale_mat_0."""
    dev = _dev(device)
    S = np.asarray(scale_mat, dtype=np.float32).reshape(4, 4)
    v = _points(vertices, dev)
    out = torch.empty_like(v)
    t = (C.c_double * 3)(*[float(x) for x in S[:3, 3]])
    N.launch("gs2m_eval_transform", dev, len(v), _ptr(v), float(S[0, 0]), t, _ptr(out))
    return out


def sample_mesh_points(vertices, triangles, thresh=0.2, device=None):
    """eval.py's mesh-mode cloud: the vertices (all of them, in file order), then the samples of every triangle in triangle
    order.  -> (V + S, 3) fp64 tensor on the device."""
    dev = _dev(device)
    v = _points(vertices, dev)
    f = triangles_i32(triangles, dev)
    nv, nt = len(v), len(f)
    tri_ws = workspace_for("gs2m_eval_sample_workspace_bytes", dev, nt, 0, only=0)
    rows = C.c_longlong()
    N.launch("gs2m_eval_sample_rows", dev, nv, _ptr(v), nt, _ptr(f), float(thresh), _ptr(tri_ws), C.byref(rows))
    row_ws = workspace_for("gs2m_eval_sample_workspace_bytes", dev, nt, rows.value, only=1)
    ns = C.c_longlong()
    N.launch("gs2m_eval_sample_count", dev, nt, rows.value, _ptr(tri_ws), _ptr(row_ws), C.byref(ns))
    cloud = torch.empty((nv + ns.value, 3), dtype=torch.float64, device=dev)
    N.launch("gs2m_eval_sample_emit", dev, nv, _ptr(v), nt, _ptr(f), rows.value, _ptr(tri_ws), _ptr(row_ws), ns.value, _ptr(cloud))
    return cloud


def shuffle_order(n, seed=0):
    """The row order of the shuffle: numpy's default_rng(seed).permutation(n), which is the order rng.shuffle(a, axis=0)
    applies (tests/test_dtu_eval.py checks that)."""
    return np.random.default_rng(seed).permutation(n)


def gather(points, order, device=None):
    dev = _dev(device)
    p = _points(points, dev)
    o = torch.as_tensor(np.asarray(order, dtype=np.int64) if not torch.is_tensor(order) else order).to(dev, torch.int64).contiguous()
    if len(o) != len(p):
        raise ValueError(f"gs2m_dtu_eval: order has {len(o)} entries for {len(p)} points")
    out = torch.empty_like(p)
    N.launch("gs2m_eval_gather", dev, len(p), _ptr(p), _ptr(o), _ptr(out))
    return out


def _thin(p, radius, rank, dev):
    keep = torch.empty(len(p), dtype=torch.uint8, device=dev)
    rounds = C.c_int()
    ws = workspace_for("gs2m_eval_thin_workspace_bytes", dev, len(p))
    N.launch("gs2m_eval_thin", dev, len(p), _ptr(p), _ptr(rank), float(radius), _ptr(ws), _ptr(keep), C.byref(rounds))
    return keep, rounds.value


def radius_downsample(points, radius, order=None, device=None):
    """eval.py's thinning: visiting the points in `order` (default: index order), a point not yet removed is kept and removes
    every point within `radius` ((dx dx + dy dy) + dz dz <= radius^2).  -> keep mask (n,) bool, numpy, indexed like `points`."""
    dev = _dev(device)
    p = _points(points, dev)
    rank = None
    if order is not None:
        order = np.asarray(order, dtype=np.int64)
        if len(order) != len(p) or not np.array_equal(np.sort(order), np.arange(len(p))):
            raise ValueError("gs2m_dtu_eval: order must be a permutation of the points")
        r = np.empty(len(p), np.int64)
        r[order] = np.arange(len(p))
        rank = torch.as_tensor(r.astype(np.int32)).to(dev).contiguous()
    keep, _ = _thin(p, radius, rank, dev)
    return keep.cpu().numpy().astype(bool)


def mask_bounds(bb, patch):
    """The inbound box as eval.py forms it: BB cast to float32, lo = f32(BB0 - patch), hi = f32(BB1 + 2 patch)."""
    BB = np.asarray(bb).astype(np.float32).reshape(2, 3)
    lo = (BB[:1] - np.float32(patch)).astype(np.float32)[0]
    hi = (BB[1:] + np.float32(patch * 2)).astype(np.float32)[0]
    return lo.astype(np.float64), hi.astype(np.float64), BB[0].astype(np.float64)


def mask_flags(points, obs_mask, bb, res, patch=60.0, device=None):
    """bit 0: inbound, bit 1: inbound and inside the observation mask (axis order (x, y, z), C-contiguous). -> uint8 tensor."""
    dev = _dev(device)
    p = _points(points, dev)
    lo, hi, bb0 = mask_bounds(bb, patch)
    m = torch.as_tensor(np.ascontiguousarray(np.asarray(obs_mask) != 0, dtype=np.uint8)).to(dev).contiguous()
    dims = (C.c_int * 3)(*[int(x) for x in np.asarray(obs_mask).shape])
    flags = torch.empty(len(p), dtype=torch.uint8, device=dev)
    dd = lambda a: (C.c_double * 3)(*[float(x) for x in a])  # noqa: E731
    N.launch("gs2m_eval_filter", dev, len(p), _ptr(p), dd(lo), dd(hi), dd(bb0), float(np.asarray(res, np.float64).reshape(-1)[0]), _ptr(m),
             dims, _ptr(flags))
    return flags


def above_plane(points, plane, device=None):
    dev = _dev(device)
    p = _points(points, dev)
    P = (C.c_double * 4)(*[float(x) for x in np.asarray(plane, np.float64).reshape(-1)[:4]])
    flags = torch.empty(len(p), dtype=torch.uint8, device=dev)
    N.launch("gs2m_eval_above_plane", dev, len(p), _ptr(p), P, _ptr(flags))
    return flags


def nearest_distances(queries, targets, max_dist, cell=None, device=None):
    """The distance of every query to its nearest target point where that is < max_dist, +inf elsewhere.  -> numpy fp64."""
    dev = _dev(device)
    return TargetGrid(targets, max_dist, cell, dev).distances(queries, max_dist).cpu().numpy()


# ---- colours of the two visualisation clouds -------------------------------------------------------------------------------

def vis_colors(n, index, dist, max_dist, vis_dist):
    """eval.py's rule: blue outside the evaluated set `index`; evaluated points red * a + white * (1 - a), a = min(d, vis) / vis;
    green at or beyond max_dist.  -> (n, 3) fp64."""
    col = np.tile(np.array([[0.0, 0.0, 1.0]]), (n, 1))
    d = np.asarray(dist, np.float64).reshape(-1, 1)
    a = np.minimum(d, vis_dist) / vis_dist
    col[index] = np.array([[1.0, 0.0, 0.0]]) * a + np.array([[1.0, 1.0, 1.0]]) * (1 - a)
    col[index[d[:, 0] >= max_dist]] = np.array([0.0, 1.0, 0.0])
    return col


# ---- the whole evaluation --------------------------------------------------------------------------------------------------

def evaluate_mesh(vertices, triangles, stl, obs_mask, bb, res, plane, downsample_density=0.2, patch_size=60, max_dist=20, seed=0,
                  vis_dir=None, scan=None, visualize_threshold=10.0, scale_mat=None, details=False, device=None):
    """eval.py's mesh mode on the GPU.  vertices (V, 3) in world coordinates (or mesh coordinates with `scale_mat`, which
    applies evaluate_single_scene.py's transform), triangles (F, 3), stl (M, 3) ground-truth points, obs_mask (X, Y, Z),
    bb (2, 3), res, plane (4,).  -> dict: mean_d2s, mean_s2d, overall, counts, seed, stage times in ms; with `details` also
    the intermediate arrays (numpy).  vis_dir: writes vis_{scan:03}_d2s.ply and vis_{scan:03}_s2d.ply there."""
    dev = _dev(device)
    thresh = float(downsample_density)
    times = {}

    def stage(name, t0):
        torch.cuda.synchronize(dev)
        times[name] = round(1e3 * (time.perf_counter() - t0), 3)
        return time.perf_counter()

    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    v = world_transform(vertices, scale_mat, dev) if scale_mat is not None else _points(vertices, dev)
    cloud = sample_mesh_points(v, triangles, thresh, dev)
    t0 = stage("sample", t0)
    order = shuffle_order(len(cloud), seed)
    shuffled = gather(cloud, order, dev)
    t0 = stage("shuffle", t0)
    keep, rounds = _thin(shuffled, thresh, None, dev)
    down = _compact(shuffled, keep, 0, dev)
    t0 = stage("thin", t0)
    flags = mask_flags(down, obs_mask, bb, res, patch_size, dev)
    data_in = _compact(down, flags, 0, dev)
    data_in_obs = _compact(down, flags, 1, dev)
    t0 = stage("filter", t0)
    stl_t = _points(stl, dev)
    d2s = TargetGrid(stl_t, max_dist, device=dev).distances(data_in_obs, max_dist)
    mean_d2s, n_d2s = masked_mean(d2s, max_dist, dev)
    t0 = stage("d2s", t0)
    above = above_plane(stl_t, plane, dev)
    stl_above = _compact(stl_t, above, 0, dev)
    s2d = TargetGrid(data_in, max_dist, device=dev).distances(stl_above, max_dist)
    mean_s2d, n_s2d = masked_mean(s2d, max_dist, dev)
    stage("s2d", t0)
    out = {"mean_d2s": mean_d2s, "mean_s2d": mean_s2d, "overall": (mean_d2s + mean_s2d) / 2,
           "n_vertices": int(len(v)), "n_triangles": int(len(triangles)), "n_cloud": int(len(cloud)), "n_down": int(len(down)),
           "n_in": int(len(data_in)), "n_in_obs": int(len(data_in_obs)), "n_stl": int(len(stl_t)), "n_stl_above": int(len(stl_above)),
           "n_d2s_used": n_d2s, "n_s2d_used": n_s2d, "thin_rounds": rounds, "seed": seed, "downsample_density": thresh,
           "patch_size": patch_size, "max_dist": max_dist, "ms": times}
    if vis_dir is not None or details:
        fl = flags.cpu().numpy()
        idx_obs = np.nonzero(fl & 2)[0]
        ab = above.cpu().numpy()
        d2s_np, s2d_np = d2s.cpu().numpy(), s2d.cpu().numpy()
        down_np, stl_np = down.cpu().numpy(), stl_t.cpu().numpy()
        d_col = vis_colors(len(down_np), idx_obs, d2s_np, max_dist, visualize_threshold)
        s_col = vis_colors(len(stl_np), np.nonzero(ab)[0], s2d_np, max_dist, visualize_threshold)
        if vis_dir is not None:
            os.makedirs(vis_dir, exist_ok=True)
            tag = f"{int(scan):03}" if scan is not None else "000"
            write_point_cloud(os.path.join(vis_dir, f"vis_{tag}_d2s.ply"), down_np, d_col)
            write_point_cloud(os.path.join(vis_dir, f"vis_{tag}_s2d.ply"), stl_np, s_col)
        if details:
            out["arrays"] = {"cloud": cloud.cpu().numpy(), "order": order, "keep": keep.cpu().numpy().astype(bool), "down": down_np,
                             "flags": fl, "dist_d2s": d2s_np, "above": ab.astype(bool), "dist_s2d": s2d_np,
                             "d2s_colors": d_col, "s2d_colors": s_col}
    return out


# ---- files -------------------------------------------------------------------------------------------------------------------

def load_dtu_ground_truth(dtu_dir, scan):
    """The DTU evaluation files of `scan`: Points/stl/stl{scan:03}_total.ply, ObsMask/ObsMask{scan}_10.mat (ObsMask, BB, Res)
    and ObsMask/Plane{scan}.mat (P).  -> dict(stl (M, 3) fp64, obs_mask uint8 C-contiguous indexed [x, y, z], bb (2, 3) float32,
    res float, plane (4,) fp64)."""
    from scipy.io import loadmat
    m = loadmat(os.path.join(dtu_dir, "ObsMask", f"ObsMask{scan}_10.mat"))
    stl, _ = read_ply(os.path.join(dtu_dir, "Points", "stl", f"stl{scan:03}_total.ply"))
    plane = loadmat(os.path.join(dtu_dir, "ObsMask", f"Plane{scan}.mat"))["P"]
    return {"stl": stl, "obs_mask": np.ascontiguousarray(m["ObsMask"] != 0, dtype=np.uint8), "bb": m["BB"].astype(np.float32),
            "res": float(np.asarray(m["Res"], np.float64).reshape(-1)[0]), "plane": np.asarray(plane, np.float64).reshape(-1)}


def load_scale_mat(ref_dir):
    """cameras.npz's scale_mat_0 as float32 (evaluate_single_scene.py takes scale_mats[0])."""
    return np.load(os.path.join(ref_dir, "cameras.npz"))["scale_mat_0"].astype(np.float32)


# ---- command line: evaluate_single_scene.py + eval.py --------------------------------------------------------------------

def main(argv=None):
    ap = argparse.ArgumentParser(description="DTU Chamfer distance of a mesh (evaluate_single_scene.py + eval.py, mesh mode)")
    ap.add_argument("--input_ply", required=True, help="the mesh to evaluate (binary PLY)")
    ap.add_argument("--ref_dir", required=True, help="the scan folder (cameras.npz; the scan id from its name, e.g. scan24)")
    ap.add_argument("--dtu_dir", default="Offical_DTU_Dataset", help="the DTU ground-truth folder (Points/, ObsMask/)")
    ap.add_argument("--out_dir", default="", help="default: the input's folder")
    ap.add_argument("--mask_cull", action="store_true", help="not supported")
    ap.add_argument("--downsample_density", type=float, default=0.2)
    ap.add_argument("--patch_size", type=float, default=60)
    ap.add_argument("--max_dist", type=float, default=20)
    ap.add_argument("--visualize_threshold", type=float, default=10)
    ap.add_argument("--seed", type=int, default=0, help="the shuffle's seed (the reference's shuffle is unseeded)")
    ap.add_argument("--no_vis", action="store_true", help="skip the two coloured clouds")
    a = ap.parse_args(argv)
    if a.mask_cull:
        ap.error("--mask_cull is not supported (it needs mask dilation); the reference's run_dtu.py does not use it")
    ref_dir = os.path.normpath(a.ref_dir)
    name = os.path.basename(ref_dir)
    try:
        scan = int(name.replace("scan", ""))
    except ValueError:
        ap.error(f"--ref_dir {a.ref_dir}: the folder name must be scan<id>")
    out_dir = a.out_dir or os.path.dirname(os.path.abspath(a.input_ply))
    os.makedirs(out_dir, exist_ok=True)
    verts, tris = read_ply(a.input_ply)
    gt = load_dtu_ground_truth(a.dtu_dir, scan)
    r = evaluate_mesh(verts, tris, gt["stl"], gt["obs_mask"], gt["bb"], gt["res"], gt["plane"], a.downsample_density, a.patch_size,
                      a.max_dist, a.seed, vis_dir=None if a.no_vis else out_dir, scan=scan, visualize_threshold=a.visualize_threshold,
                      scale_mat=load_scale_mat(ref_dir))
    r["scan"] = scan
    print(f"[>] Average Chamfer distance: {r['overall']:.2f} (d2s {r['mean_d2s']:.4f}, s2d {r['mean_s2d']:.4f})")
    with open(os.path.join(out_dir, "results.json"), "w") as f:
        json.dump(r, f, indent=True)
    return r


if __name__ == "__main__":
    main()
