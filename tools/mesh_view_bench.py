"""The mesh visualisation timed on tools/tnt_cull_bench.py's scene: the synthetic surface scene extracted at `--voxel` (7.7 M
triangles at the default) seen from `--views` cameras of the Tanks and Temples frame (1920 x 1080), every eighth camera at the
sphere's wall.  For ss in 1, 2 and view batches of 1 and 8: one warm-up pass and one timed pass over all views of the visibility
pass alone and of the shade pass alone (flat and smooth, on the visibility buffer of the batch); and, in the same run,
gs2m_meshdepth_render on the same inputs, with the ratio of the ss = 1 visibility pass to it (what the 64-bit keys cost).
Writes profiles/mesh_view_bench.json and prints it as one JSON line.  Nothing has measured this before: no threshold.  All data
is synthetic.

    python tools/mesh_view_bench.py [--views 48] [--voxel 0.004]
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

import gs2m_mesh_cull as K  # noqa: E402
import gs2m_mesh_view as G  # noqa: E402
import gs2m_native as N  # noqa: E402


def timed(fn, batches):
    """fn(batch) over the batches, once to warm up and once on the clock -> seconds"""
    for on in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in batches:
            fn(b)
        torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=48)
    ap.add_argument("--width", type=int, default=K.TNT_WIDTH)
    ap.add_argument("--height", type=int, default=K.TNT_HEIGHT)
    ap.add_argument("--voxel", type=float, default=0.004)
    ap.add_argument("--fuse-views", type=int, default=49)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_view_bench.json"))
    a = ap.parse_args()
    import gs2m_mesh as M
    import mesh_bench as MB
    from tnt_cull_bench import cameras
    cams, depths, colors = MB.scene(200_000, a.fuse_views, 1600, 1200)
    lo, hi = M._depth_aabb(depths, cams, 10.0, torch.device("cuda"))
    L, tr = 16 * a.voxel, 4 * a.voxel
    _, mesh, _, _ = MB.fuse(cams, depths, colors, a.voxel, 10.0, 4096, lo - tr - L, hi + tr + L)
    del depths, colors
    dev = torch.device("cuda")
    v = torch.as_tensor(np.asarray(mesh.vertices, np.float64)).to(dev).contiguous()
    f = torch.as_tensor(np.asarray(mesh.triangles, np.int32)).to(dev).contiguous()
    w2c = torch.as_tensor(cameras(a.views)).to(dev).contiguous()
    k = (K.TNT_FX, K.TNT_FY, K.TNT_CX, K.TNT_CY)
    H, W = a.height, a.width
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    normals, _ = G.vertex_normals(v, f)
    torch.cuda.synchronize()
    t_normals = time.perf_counter() - t0
    rows = []
    depth_ms = {}
    for batch in (1, 8):
        parts = [w2c[i:i + batch] for i in range(0, a.views, batch)]
        dbuf = torch.empty(batch * H * W, dtype=torch.float32, device=dev)
        depth_ms[batch] = 1e3 * timed(lambda p: K.render_mesh_depth(v, f, p, *k, H, W, out=dbuf), parts) / a.views
        for ss in (1, 2):
            buf = torch.empty(batch * H * W * ss * ss, dtype=torch.int64, device=dev)
            rgba = torch.empty((batch, H, W, 4), dtype=torch.uint8, device=dev)
            t_vis = timed(lambda p: G.visibility_buffer(v, f, p, *k, H, W, ss=ss, out=buf), parts)
            row = {"view_batch": batch, "ss": ss, "visibility_ms_per_view": round(1e3 * t_vis / a.views, 3)}
            if ss == 1:
                row["meshdepth_ms_per_view"] = round(depth_ms[batch], 3)
                row["visibility_over_meshdepth"] = round(1e3 * t_vis / a.views / depth_ms[batch], 3)
            for name, nrm in (("flat", None), ("smooth", normals)):
                # the buffer holds the last batch's keys; every batch shades them (the same work per view)
                def shade(p):
                    N.launch("gs2m_meshview_shade", dev, len(v), v.data_ptr(), len(f), f.data_ptr(), len(p), p.data_ptr(), *k, W, H, ss,
                             buf.data_ptr(), None if nrm is None else nrm.data_ptr(), None, 0.7, 0.7, 0.7, 0.15, 0.85, 1, rgba.data_ptr(), None, None)
                row[f"shade_{name}_ms_per_view"] = round(1e3 * timed(shade, [parts[-1]] * len(parts)) / (len(parts[-1]) * len(parts)), 3)
            row["covered_pixels_last_view"] = int((rgba[len(parts[-1]) - 1, ..., 3] > 0).sum())
            rows.append(row)
            del buf, rgba
    out = {"workload": f"{a.views} views {W}x{H}, voxel {a.voxel}, synthetic surface scene, every eighth camera at the wall",
           "n_triangles": int(len(f)), "n_vertices": int(len(v)), "frame_pixels": W * H, "vertex_normals_ms": round(1e3 * t_normals, 3), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
