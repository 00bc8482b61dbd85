"""TSDF fusion + marching cubes timed on a DTU-shaped job: the synthetic surface scene (gs2m_synth.make_surface_scene: a
radius-1.5 sphere and a ground disc) seen by 49 orbit cameras at 1600 x 1200, voxel 0.002, sdf_trunc 4 voxels.  The depth
and colour of every view are rendered first (not timed); one full fusion + extraction warms up and sizes the block pool;
the timed run then fuses into a fresh volume whose pool already holds every block (no growth), synchronising the device
around each step.  Prints one JSON line: ms per integrated view (touch / allocate with its host read of the counts, then
integrate), ms per extraction (both passes and the read-back of the mesh), blocks, V, F.
Post-processing stage: the mesh is extracted once more onto the device (not timed); post_process_mesh_gpu runs once to warm
up and is then timed, the device synchronised around it (its own read-backs of the counts included, no read-back of the
mesh); --host-post also times the host post_process_mesh on the same mesh, once (it is slow), and compares the two results.
Adds ms_post_device, C (clusters), kept_V / kept_F, the two workspace sizes and, with --host-post, ms_post_host and the ratio.

    python tools/mesh_bench.py [--views 49] [--width 1600] [--height 1200] [--voxel 0.002] [--host-post]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-2m_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gs2m_mesh as M  # noqa: E402
import gs2m_synth as S  # noqa: E402
from gaussian_renderer import render  # noqa: E402
from gs2m_scene import Camera, GaussianParams, PipelineParams, inverse_sigmoid  # noqa: E402


def scene(n_true, n_views, W, H):
    sc = S.make_surface_scene(n_true, seed=0)
    t = {k: v.cuda() for k, v in sc.items()}
    truth = GaussianParams(t["points"], t["shs"][:, :1].contiguous(), t["shs"][:, 1:].contiguous(), torch.log(t["scales"]),
                           t["rotations"], inverse_sigmoid(t["opacities"]),
                           *(inverse_sigmoid(torch.full((n_true, c), 0.5, device="cuda")) for c in (3, 1, 1)))
    cams = [Camera(c, "cuda") for c in S.orbit_cameras(n_views, W, H, radius=6.0, centre=(0.0, -0.8, 6.0), fx=1.1 * W)]
    depths, colors = [], []
    with torch.no_grad():
        for cam in cams:
            out = render(cam, truth, PipelineParams(), torch.zeros(3, device="cuda"), material_stage=True)
            depths.append(M.quantize_depth_mm(out["depth_map"].squeeze(0).float()).contiguous())
            colors.append(out["render"].clamp(0, 1).mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).contiguous())
    return cams, depths, colors


def fuse(cams, depths, colors, voxel, max_depth, capacity, lo, hi):
    vol = M.TSDFVolume(voxel, 4 * voxel, max_depth, lo, hi, capacity=capacity)
    t_int = []
    for cam, d, c in zip(cams, depths, colors):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vol.integrate(d, c, cam.Fx, cam.Fy, cam.Cx, cam.Cy, M._view_w2c(cam))
        torch.cuda.synchronize()
        t_int.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mesh = vol.extract_triangle_mesh()
    torch.cuda.synchronize()
    return vol, mesh, t_int, time.perf_counter() - t0


def post_stage(vol, host_mesh, num_clusters, host_post):
    """The post-processing of the volume's mesh: the device path timed after a warm-up, the host path once on request."""
    dmesh = vol.extract_triangle_mesh(to_host=False)
    V, F = len(dmesh.vertices), len(dmesh.triangles)
    cluster_bytes, compact_bytes = M.post_workspace_bytes(V, F)
    _, sizes = M.cluster_connected_triangles_gpu(dmesh)  # the cluster count for the report (and a first warm-up)
    M.post_process_mesh_gpu(dmesh, num_clusters)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    post = M.post_process_mesh_gpu(dmesh, num_clusters)
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    out = {"ms_post_device": round(1e3 * t_dev, 3), "C": int(len(sizes)), "largest_cluster": int(sizes.max()) if len(sizes) else 0,
           "kept_V": int(len(post.vertices)), "kept_F": int(len(post.triangles)), "post_cluster_ws_bytes": cluster_bytes,
           "post_compact_ws_bytes": compact_bytes}
    if host_post:
        print(f"[mesh_bench] device post-processing {1e3 * t_dev:.1f} ms; the host function on V = {V}, F = {F} ...", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        ref = M.post_process_mesh(host_mesh, num_clusters)
        t_host = time.perf_counter() - t0
        got = post.cpu()
        same = all(np.array_equal(getattr(got, k), getattr(ref, k)) for k in ("vertices", "triangles", "vertex_colors"))
        out.update({"ms_post_host": round(1e3 * t_host, 1), "post_host_over_device": round(t_host / t_dev, 1), "post_equal": bool(same)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--voxel", type=float, default=0.002)
    ap.add_argument("--max-depth", type=float, default=10.0)
    ap.add_argument("--true-gaussians", type=int, default=200_000)
    ap.add_argument("--num-clusters", type=int, default=1)
    ap.add_argument("--host-post", action="store_true", help="also time the host post_process_mesh on the same mesh, once")
    a = ap.parse_args()
    cams, depths, colors = scene(a.true_gaussians, a.views, a.width, a.height)
    lo, hi = M._depth_aabb(depths, cams, a.max_depth, torch.device("cuda"))
    L, tr = 16 * a.voxel, 4 * a.voxel
    lo, hi = lo - tr - L, hi + tr + L
    vol, mesh, _, _ = fuse(cams, depths, colors, a.voxel, a.max_depth, 4096, lo, hi)  # warm-up; sizes the pool
    vol2, mesh2, t_int, t_ext = fuse(cams, depths, colors, a.voxel, a.max_depth, vol.n_blocks, lo, hi)
    assert vol2.n_blocks == vol.n_blocks and np.array_equal(mesh.triangles, mesh2.triangles)
    del mesh, vol
    post = post_stage(vol2, mesh2, a.num_clusters, a.host_post)
    print(json.dumps({
        "workload": f"{a.views} views {a.width}x{a.height}, voxel {a.voxel}, trunc {tr}, synthetic surface scene",
        "ms_per_view": round(1e3 * float(np.mean(t_int)), 3), "ms_per_view_median": round(1e3 * float(np.median(t_int)), 3),
        "ms_extract": round(1e3 * t_ext, 3), "blocks": vol2.n_blocks, "domain_blocks": vol2.dom[3] * vol2.dom[4] * vol2.dom[5],
        "pool_mib": round(vol2.n_blocks * 4096 * 20 / 2 ** 20, 1), "V": int(len(mesh2.vertices)), "F": int(len(mesh2.triangles)),
        "ignored_points": vol2.ignored_points, **post}))


if __name__ == "__main__":
    main()
