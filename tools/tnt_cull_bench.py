"""The mesh visibility cull timed on a TnT-shaped synthetic job: tools/mesh_bench.py's scene (the radius-1.5 sphere and the ground
disc) fused and extracted as the mesh at `--voxel`, then rendered and voted on from `--views` cameras of the Tanks and Temples
frame (1920 x 1080, the reference's intrinsics): an orbit around the scene, every eighth camera moved up to the sphere's wall,
where triangles fill many pixels.  For each view-batch size of `--batches` one warm-up pass and one timed pass over all views;
prints one JSON line: ms per view of the rasterizer and of the votes, triangles and vertices per second, the share of
(triangle, view) pairs that went to the cooperative paths (a wave; a row of workgroups), the rasterizer's triangle and vertex
bytes per second beside the HBM figure, and the cull's counts.  Nothing has measured this before: no threshold.  All data is
synthetic.

    python tools/tnt_cull_bench.py [--views 48] [--voxel 0.004] [--batches 1,2,4,8,16]
"""
import argparse
import ctypes as C
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

import gs2m_mesh_cull as K  # noqa: E402
import gs2m_native as N  # noqa: E402
from gs2m_eval_util import workspace_for  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12  # bytes / s: the MI355X's specified peak and a measured float4 copy


def cameras(n, centre=(0.0, -0.8, 6.0), sphere=(0.0, 0.0, 6.0)):
    from tnt_cull_ref import look_at
    out = []
    for k in range(n):
        a = 2 * np.pi * k / n
        d = np.array([np.cos(a), -0.15, np.sin(a)])
        if k % 8 == 7:  # next to the wall: 0.25 from the sphere's surface, looking along it
            eye = np.asarray(sphere) + 1.75 * d / np.linalg.norm(d)
            out.append(look_at(eye, eye + np.array([-np.sin(a), 0.1, np.cos(a)])))
        else:
            out.append(look_at(np.asarray(centre) + 5.0 * d, sphere))
    return np.stack(out)


def rasterize(v, f, w2c, depth, a):
    """one call of the rasterizer with its own workspace -> (wave entries, workgroup entries) summed over the call's views"""
    ws = workspace_for("gs2m_meshdepth_workspace_bytes", v.device, len(f), len(w2c))
    N.launch("gs2m_meshdepth_render", v.device, len(v), v.data_ptr(), len(f), f.data_ptr(), len(w2c), w2c.data_ptr(), K.TNT_FX, K.TNT_FY,
             K.TNT_CX, K.TNT_CY, a.width, a.height, K.NEAR, K.FAR, ws.data_ptr(), depth.data_ptr())
    # the workspace's layout (csrc/mesh_raster.h, carve_raster): the flag, then the views' two counters, each array padded to 256 bytes
    counts = ws[256:256 + 8 * len(w2c)].view(torch.int32).reshape(-1, 2).sum(0).tolist()
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=48)
    ap.add_argument("--width", type=int, default=K.TNT_WIDTH)
    ap.add_argument("--height", type=int, default=K.TNT_HEIGHT)
    ap.add_argument("--voxel", type=float, default=0.004)
    ap.add_argument("--fuse-views", type=int, default=49)
    ap.add_argument("--batches", default="1,2,4,8,16")
    a = ap.parse_args()
    import gs2m_mesh as M
    import mesh_bench as MB
    cams, depths, colors = MB.scene(200_000, a.fuse_views, 1600, 1200)
    lo, hi = M._depth_aabb(depths, cams, 10.0, torch.device("cuda"))
    L, tr = 16 * a.voxel, 4 * a.voxel
    _, mesh, _, _ = MB.fuse(cams, depths, colors, a.voxel, 10.0, 4096, lo - tr - L, hi + tr + L)
    del depths, colors
    dev = torch.device("cuda")
    v = torch.as_tensor(np.asarray(mesh.vertices, np.float64)).to(dev).contiguous()
    f = torch.as_tensor(np.asarray(mesh.triangles, np.int32)).to(dev).contiguous()
    w2c = torch.as_tensor(cameras(a.views)).to(dev).contiguous()
    n_tris, n_verts, frame = len(f), len(v), a.width * a.height
    rows = []
    for b in [int(x) for x in a.batches.split(",")]:
        depth = torch.empty((b, a.height, a.width), dtype=torch.float32, device=dev)
        votes = torch.zeros(n_verts, dtype=torch.int32, device=dev)
        for timed in (False, True):
            votes.zero_()
            t_r = t_v = 0.0
            coop = [0, 0]
            for k in range(0, a.views, b):
                part = w2c[k:k + b]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c = rasterize(v, f, part, depth, a)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                K.visibility_votes(v, part, K.TNT_FX, K.TNT_FY, K.TNT_CX, K.TNT_CY, depth[:len(part)], K.EPS, out=votes)
                torch.cuda.synchronize()
                t_r, t_v = t_r + t1 - t0, t_v + time.perf_counter() - t1
                coop = [coop[0] + c[0], coop[1] + c[1]]
        calls = -(-a.views // b)
        # what the small-triangle path has to read: per call every triangle's three indices and its three fp64 vertices
        mesh_bytes = calls * n_tris * (12 + 72)
        rows.append({"view_batch": b, "raster_ms_per_view": round(1e3 * t_r / a.views, 3), "votes_ms_per_view": round(1e3 * t_v / a.views, 3),
                     "triangle_views_per_s": round(n_tris * a.views / t_r), "vertex_views_per_s": round(n_verts * a.views / t_v),
                     "wave_share": coop[0] / (n_tris * a.views), "workgroup_share": coop[1] / (n_tris * a.views),
                     "raster_mesh_bytes_per_s": round(mesh_bytes / t_r), "of_hbm_peak": round(mesh_bytes / t_r / HBM_PEAK, 4),
                     "of_hbm_copy": round(mesh_bytes / t_r / HBM_COPY, 4), "covered_pixels_last_view": int((depth[len(part) - 1] > 0).sum())})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cv, cf, tot = K.cull_mesh_by_visibility(v, f, w2c, K.TNT_FX, K.TNT_FY, K.TNT_CX, K.TNT_CY, a.height, a.width)
    torch.cuda.synchronize()
    t_cull = time.perf_counter() - t0
    print(json.dumps({"workload": f"{a.views} views {a.width}x{a.height}, voxel {a.voxel}, synthetic surface scene, every eighth camera at the wall",
                      "n_triangles": n_tris, "n_vertices": n_verts, "frame_pixels": frame, "batches": rows,
                      "cull_ms_default_batch": round(1e3 * t_cull, 2), "kept_vertices": int(len(cv)), "kept_triangles": int(len(cf)),
                      "votes_histogram_0_10_20_max": [int((tot == 0).sum()), int(((tot > 0) & (tot < 10)).sum()), int(((tot >= 10) & (tot < 20)).sum()),
                                                      int((tot >= 20).sum())],
                      "hbm_peak_bytes_per_s": HBM_PEAK, "hbm_copy_bytes_per_s": HBM_COPY}))


if __name__ == "__main__":
    main()
