"""DTU Chamfer evaluation of a mesh on the GPU (csrc/mesh_eval.hip, csrc/mesh_cull.hip, include/gs2m_eval.h).

The score GS-2M reports for its extracted mesh: the reference's scripts/eval_dtu/evaluate_single_scene.py (the scale-matrix
step, and with --mask_cull the culling against the dilated object masks) followed by eval.py in mesh mode, as DESIGN.md §10
writes the contract down.  The mesh is sampled
on every triangle, shuffled with a seeded numpy generator, thinned to `downsample_density`, cut to the observation mask and
scored against the ground-truth STL points in both directions.  Sampling, thinning, the filters and the nearest-neighbour
distances run in HIP kernels, all in fp64; every buffer is a torch tensor owned here.

    python gs-2m_amd/gs2m_dtu_eval.py --input_ply tsdf_post.ply --ref_dir DTU/scan24 --dtu_dir Offical_DTU_Dataset --out_dir OUT
writes OUT/results.json (mean_d2s, mean_s2d, overall, plus counts, seed and stage times) and OUT/vis_XXX_{d2s,s2d}.ply.
With --mask_cull (needs ref_dir/images, ref_dir/mask) the mesh is culled first and OUT/culled_mesh.ply is written too.
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


# ---- mask culling (DESIGN.md §10 "Mask culling") ---------------------------------------------------------------------------

CULL_RADIUS = 24
CULL_IMAGE_SIZE = (1600, 1200)  # (Wn, Hn): the size the reference normalises pixel coordinates by, whatever the masks' size


def decompose_projection(P):
    """P (3, 4) -> K (3, 3) upper triangular with K[0, 0] > 0 and K[1, 1] > 0, R a rotation with K R = P[:, :3], and the camera
    centre C = -P[:, :3]^-1 P[:, 3]; computed in fp64.  K[2, 2] carries the sign of det P[:, :3]."""
    P = np.asarray(P, np.float64).reshape(3, 4)
    A = P[:, :3]
    J = np.eye(3)[::-1]
    Q, U = np.linalg.qr((J @ A).T)  # J A = U^T Q^T, so A = (J U^T J) (J Q^T)
    K, R = J @ U.T @ J, J @ Q.T
    sg = np.where(np.diag(K) < 0, -1.0, 1.0)
    K, R = K * sg[None, :], R * sg[:, None]
    if np.linalg.det(R) < 0:
        K[:, 2], R[2, :] = -K[:, 2], -R[2, :]
    return K, R, -np.linalg.solve(A, P[:, 3])


def view_matrices(world_mats, scale_mats):
    """The (n_views, 4, 4) float32 matrices the vertex test multiplies with: P = (world_mat @ scale_mat)[:3, :4] in float32,
    decomposed; intrinsics = K / K[2, 2] in a 4 x 4 float32, pose = [R^T | C] in a 4 x 4 float32, M = intrinsics @ inverse(pose),
    inverted and multiplied in float32."""
    out = []
    for Wm, Sm in zip(world_mats, scale_mats):
        P = (np.asarray(Wm, np.float32).reshape(4, 4) @ np.asarray(Sm, np.float32).reshape(4, 4))[:3, :4]
        K, R, Cc = decompose_projection(P)
        intr, pose = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
        intr[:3, :3] = (K / K[2, 2]).astype(np.float32)
        pose[:3, :3], pose[:3, 3] = R.T.astype(np.float32), Cc.astype(np.float32)
        out.append(intr @ np.linalg.inv(pose))
    return np.stack(out).astype(np.float32) if out else np.zeros((0, 4, 4), np.float32)


def read_mask_png(path):
    """The blue channel of an 8-bit PNG as (H, W) uint8 (what cv2.imread(path)[:, :, 0] gives: alpha dropped, greyscale and
    palette files expanded).  A file with more than 8 bits per channel is refused."""
    from PIL import Image
    with open(str(path), "rb") as f:
        head = f.read(26)
    if len(head) < 26 or head[:8] != b"\x89PNG\r\n\x1a\n" or head[12:16] != b"IHDR":
        raise ValueError(f"{path}: not a PNG file")
    depth, ctype = head[24], head[25]
    if depth != 8 and ctype != 3:  # a palette's entries are 8 bits per channel whatever the index width
        raise ValueError(f"{path}: {depth} bits per channel: only 8-bit masks are read")
    with Image.open(str(path)) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, 2])


def load_cull_inputs(ref_dir):
    """The culling inputs of a scan folder: cameras.npz (world_mat_i, scale_mat_i for the n images of images/*.png) and
    mask/*.png sorted by path, mask i for camera i.  -> (M (n, 4, 4) float32, [n masks (H, W) uint8])."""
    import glob
    n = len(glob.glob(os.path.join(ref_dir, "images", "*.png")))
    cams = np.load(os.path.join(ref_dir, "cameras.npz"))
    M = view_matrices([cams[f"world_mat_{k}"] for k in range(n)], [cams[f"scale_mat_{k}"] for k in range(n)])
    paths = sorted(glob.glob(os.path.join(ref_dir, "mask", "*.png")))
    if len(paths) < n:
        raise ValueError(f"{ref_dir}: {len(paths)} masks for {n} images")
    return M, [read_mask_png(q) for q in paths[:n]]


class DilatedMasks:
    """n dilated masks on the device, one bit per pixel: packed (n, H, ceil(W / 64)) int64, bit x & 63 of word x >> 6."""

    def __init__(self, packed, height, width):
        self.packed, self.height, self.width = packed, int(height), int(width)

    def __len__(self):
        return len(self.packed)

    def unpack(self):
        """-> (n, H, W) bool, numpy"""
        w = self.packed.cpu().numpy().view(np.uint64)
        bits = (w[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
        return bits.reshape(len(w), self.height, 64 * w.shape[2])[:, :, :self.width].astype(bool)


def _mask_stack(masks, dev):
    if torch.is_tensor(masks):
        t = masks
    elif isinstance(masks, np.ndarray) and masks.ndim == 3:
        t = torch.as_tensor(np.ascontiguousarray(masks))
    else:
        ms = [np.asarray(m) for m in masks]
        if any(m.ndim != 2 or m.shape != ms[0].shape for m in ms):
            raise ValueError("gs2m_dtu_eval: the masks must be 2-D and of one size")
        t = torch.as_tensor(np.stack(ms)) if ms else None
    if t is None or t.ndim != 3 or t.shape[1] < 1 or t.shape[2] < 1:
        raise ValueError("gs2m_dtu_eval: masks must be (n, H, W) with H, W >= 1 (no mask at all has no size: pass an empty (0, H, W) array)")
    if t.dtype != torch.uint8:
        t = (t != 0).to(torch.uint8)
    return t.to(dev).contiguous()


def dilate_masks(masks, radius=CULL_RADIUS, device=None):
    """masks: n arrays (H, W) or one (n, H, W) array or tensor, non-zero = foreground.  -> DilatedMasks: each mask dilated by the
    disk dx^2 + dy^2 <= radius^2 (scipy.ndimage.binary_dilation with that structure, bit for bit)."""
    dev = _dev(device)
    m = _mask_stack(masks, dev)
    n, H, W = (int(x) for x in m.shape)
    nbytes = C.c_longlong()
    N.check(N.lib().gs2m_eval_dilate_bytes(n, H, W, C.byref(nbytes)), "gs2m_eval_dilate_bytes")
    packed = torch.empty((n, H, (W + 63) // 64), dtype=torch.int64, device=dev)
    assert packed.numel() * 8 == nbytes.value
    N.launch("gs2m_eval_dilate_disk", dev, n, H, W, _ptr(m), int(radius), _ptr(packed))
    return DilatedMasks(packed, H, W)


def cull_flags(vertices, M, dilated, image_size=CULL_IMAGE_SIZE, device=None):
    """keep flag per vertex (uint8 tensor): 1 when no view sees the vertex outside its dilated mask.  M: view_matrices' array."""
    dev = _dev(device)
    v = _points(vertices, dev)
    Mt = torch.as_tensor(np.ascontiguousarray(np.asarray(M, np.float32).reshape(-1, 4, 4))).to(dev)
    if len(Mt) != len(dilated):
        raise ValueError(f"gs2m_dtu_eval: {len(Mt)} view matrices for {len(dilated)} masks")
    keep = torch.empty(len(v), dtype=torch.uint8, device=dev)
    N.launch("gs2m_eval_cull_flags", dev, len(v), _ptr(v), len(Mt), _ptr(Mt), dilated.height, dilated.width, _ptr(dilated.packed),
             int(image_size[0]), int(image_size[1]), _ptr(keep))
    return keep


def cull_triangles(keep, triangles, device=None):
    """The triangles whose three vertices are kept, in order, renumbered to the kept vertices' positions (kept vertices stay
    whether referenced or not).  -> (F', 3) int32 device tensor."""
    dev = _dev(device)
    f = triangles_i32(triangles, dev)
    out = torch.empty_like(f)
    ws = workspace_for("gs2m_eval_cull_workspace_bytes", dev, len(keep), len(f))
    tot = (C.c_longlong * 2)()
    N.launch("gs2m_eval_cull_triangles", dev, len(keep), _ptr(keep), len(f), _ptr(f), _ptr(ws), _ptr(out), tot)
    return out[:tot[1]].clone()


def cull_mesh(vertices, triangles, M, masks, radius=CULL_RADIUS, image_size=CULL_IMAGE_SIZE, device=None, times=None):
    """evaluate_single_scene.py's --mask_cull step on the device.  masks: as dilate_masks takes them, or a DilatedMasks.
    -> (vertices (V', 3) fp64, triangles (F', 3) int32), device tensors, in the mesh's own coordinates.  times: a dict that
    receives the ms of the three kernels' stages (dilate, flags, compact), each ended by a device synchronisation; they start
    once the vertices and the masks are on the device ("flags" includes the upload of the view matrices, a few kB)."""
    dev = _dev(device)
    t0 = 0.0

    def lap(name):
        nonlocal t0
        if times is not None:
            torch.cuda.synchronize(dev)
            times[name] = round(1e3 * (time.perf_counter() - t0), 3)
            t0 = time.perf_counter()

    v = _points(vertices, dev)
    if not isinstance(masks, DilatedMasks):
        masks = _mask_stack(masks, dev)
    if times is not None:  # the laps start with the vertices and the masks on the device
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
    dil = masks if isinstance(masks, DilatedMasks) else dilate_masks(masks, radius, dev)
    lap("dilate")
    keep = cull_flags(v, M, dil, image_size, dev)
    lap("flags")
    f = cull_triangles(keep, triangles, dev)
    out = _compact(v, keep, 0, dev).clone()
    lap("compact")
    return out, f


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
                  vis_dir=None, scan=None, visualize_threshold=10.0, scale_mat=None, details=False, device=None, cull=None,
                  cull_radius=CULL_RADIUS, culled_ply=None):
    """eval.py's mesh mode on the GPU.  vertices (V, 3) in world coordinates (or mesh coordinates with `scale_mat`, which
    applies evaluate_single_scene.py's transform), triangles (F, 3), stl (M, 3) ground-truth points, obs_mask (X, Y, Z),
    bb (2, 3), res, plane (4,).  -> dict: mean_d2s, mean_s2d, overall, counts, seed, stage times in ms; with `details` also
    the intermediate arrays (numpy).  vis_dir: writes vis_{scan:03}_d2s.ply and vis_{scan:03}_s2d.ply there.
    cull: (M, masks) as load_cull_inputs returns them: the mesh (in its own coordinates) is culled against the masks dilated
    by `cull_radius` before the world transform; adds the stage time `cull` and n_vertices_culled / n_triangles_culled (the
    numbers removed).  culled_ply: the culled mesh in world coordinates is written there."""
    dev = _dev(device)
    thresh = float(downsample_density)
    times = {}

    def stage(name, t0):
        torch.cuda.synchronize(dev)
        times[name] = round(1e3 * (time.perf_counter() - t0), 3)
        return time.perf_counter()

    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    culled = None
    if cull is not None:
        n_v0, n_f0 = len(vertices), len(triangles)
        vertices, triangles = cull_mesh(vertices, triangles, cull[0], cull[1], cull_radius, device=dev)
        culled = {"n_vertices_culled": n_v0 - len(vertices), "n_triangles_culled": n_f0 - len(triangles)}
        t0 = stage("cull", t0)
    v = world_transform(vertices, scale_mat, dev) if scale_mat is not None else _points(vertices, dev)
    if culled_ply is not None:
        from gs2m_mesh import TriangleMesh, write_mesh
        torch.cuda.synchronize(dev)
        t_write = time.perf_counter()
        write_mesh(culled_ply, TriangleMesh(v.cpu().numpy(), triangles_i32(triangles, dev).cpu().numpy(), np.zeros((len(v), 3))))
        t0 += time.perf_counter() - t_write  # the file is no part of the "sample" stage, the world transform is, as without it
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
    if culled is not None:
        out.update(culled)
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
    ap.add_argument("--mask_cull", action="store_true", help="cull the mesh against ref_dir's object masks (dilated by 24 pixels) first; "
                    "writes culled_mesh.ply")
    ap.add_argument("--downsample_density", type=float, default=0.2)
    ap.add_argument("--patch_size", type=float, default=60)
    ap.add_argument("--max_dist", type=float, default=20)
    ap.add_argument("--visualize_threshold", type=float, default=10)
    ap.add_argument("--seed", type=int, default=0, help="the shuffle's seed (the reference's shuffle is unseeded)")
    ap.add_argument("--no_vis", action="store_true", help="skip the two coloured clouds")
    a = ap.parse_args(argv)
    ref_dir = os.path.normpath(a.ref_dir)
    name = os.path.basename(ref_dir)
    try:
        scan = int(name.replace("scan", ""))
    except ValueError:
        ap.error(f"--ref_dir {a.ref_dir}: the folder name must be scan<id>")
    if a.mask_cull:  # before anything is read: the scan folder must hold what the culling needs
        import glob
        missing = [what for what in ("cameras.npz", "images/*.png", "mask/*.png") if not glob.glob(os.path.join(ref_dir, *what.split("/")))]
        if missing:
            ap.error(f"--mask_cull is not supported without cameras.npz, images/*.png and mask/*.png in --ref_dir: {a.ref_dir} holds no "
                     f"{', '.join(missing)}")
    out_dir = a.out_dir or os.path.dirname(os.path.abspath(a.input_ply))
    os.makedirs(out_dir, exist_ok=True)
    verts, tris = read_ply(a.input_ply)
    gt = load_dtu_ground_truth(a.dtu_dir, scan)
    r = evaluate_mesh(verts, tris, gt["stl"], gt["obs_mask"], gt["bb"], gt["res"], gt["plane"], a.downsample_density, a.patch_size,
                      a.max_dist, a.seed, vis_dir=None if a.no_vis else out_dir, scan=scan, visualize_threshold=a.visualize_threshold,
                      scale_mat=load_scale_mat(ref_dir), cull=load_cull_inputs(ref_dir) if a.mask_cull else None,
                      culled_ply=os.path.join(out_dir, "culled_mesh.ply") if a.mask_cull else None)
    r["scan"] = scan
    if a.mask_cull:
        r["mask_cull"] = True
    print(f"[>] Average Chamfer distance: {r['overall']:.2f} (d2s {r['mean_d2s']:.4f}, s2d {r['mean_s2d']:.4f})")
    with open(os.path.join(out_dir, "results.json"), "w") as f:
        json.dump(r, f, indent=True)
    return r


if __name__ == "__main__":
    main()
