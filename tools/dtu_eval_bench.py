"""The DTU evaluation timed on a DTU-shaped synthetic job: tools/mesh_bench.py's scene (the radius-1.5 sphere and the ground
disc, 49 orbit views) fused and extracted, the mesh scaled to millimetres by `--scale` (as scale_mat_0 does), and about
2.5 M ground-truth points on the analytic surface.  One warm-up evaluation, then a timed one; prints one JSON line of the
GPU stage times (sample, shuffle, thin, filter, d2s, s2d; each ends with a device synchronisation), the point counts, and
the CPU restatement's (tests/dtu_eval_ref.py: numpy + scikit-learn) time on the stated fraction of the job: the thinning
on the first `--cpu-points` shuffled points, the d2s query of as many points against the full STL tree.

    python tools/dtu_eval_bench.py [--views 49] [--voxel 0.004] [--scale 40] [--stl 2500000] [--mask-cull]

--mask-cull adds the culling against object masks to the job: a ring of `--views` cameras around the sphere (tests/dtu_cull_ref.py's,
at the frame size), an elliptic silhouette per view at the frame size, dilated by 24 pixels.  The evaluation then reports its `cull`
stage, and `cull_ms` holds the times of the three kernel stages (dilate, flags, compact) of one more culling on its own, the bytes
per second of the dilation against one byte in and one bit out per pixel, and the host route this replaces:
scipy.ndimage.binary_dilation of one mask, timed once and multiplied by the views.
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

import gs2m_dtu_eval as E  # noqa: E402
import gs2m_mesh as M  # noqa: E402
import mesh_bench as MB  # noqa: E402


def surface_points(n, scale, t, centre=(0.0, 0.0, 6.0)):
    """n points on the sphere and the disc (area-proportional), in millimetres"""
    a_s, a_d = 4 * np.pi * 1.5 ** 2, np.pi * 3.0 ** 2
    ns = int(n * a_s / (a_s + a_d))
    k = np.arange(ns) + 0.5
    phi, th = np.arccos(1 - 2 * k / ns), np.pi * (1 + 5 ** 0.5) * k
    sph = np.asarray(centre) + 1.5 * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)
    m = n - ns
    rr, aa = 3.0 * np.sqrt((np.arange(m) + 0.5) / m), np.pi * (1 + 5 ** 0.5) * np.arange(m)
    disc = np.stack([rr * np.cos(aa) + centre[0], np.full(m, 1.5), rr * np.sin(aa) + centre[2]], axis=1)
    return np.concatenate([sph, disc]) * scale + t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--voxel", type=float, default=0.004)
    ap.add_argument("--scale", type=float, default=40.0, help="millimetres per scene unit")
    ap.add_argument("--stl", type=int, default=2_500_000)
    ap.add_argument("--cpu-points", type=int, default=100_000)
    ap.add_argument("--mask-cull", action="store_true", help="cull the mesh against synthetic silhouette masks first")
    a = ap.parse_args()
    cams, depths, colors = MB.scene(200_000, a.views, a.width, a.height)
    lo, hi = M._depth_aabb(depths, cams, 10.0, torch.device("cuda"))
    L, tr = 16 * a.voxel, 4 * a.voxel
    vol, mesh, _, _ = MB.fuse(cams, depths, colors, a.voxel, 10.0, 4096, lo - tr - L, hi + tr + L)
    t = np.array([10.0, -20.0, 300.0])
    S = np.eye(4, dtype=np.float32)
    S[0, 0] = S[1, 1] = S[2, 2] = a.scale
    S[:3, 3] = t
    stl = surface_points(a.stl, a.scale, t)
    res = 4.0
    bb = np.stack([stl.min(0) - 5, stl.max(0) + 5])
    mask = np.ones(np.floor((bb[1] - bb[0]) / res).astype(int) + 1, np.uint8)
    plane = np.array([0.0, -1.0, 0.0, 1.2 * a.scale + t[1]])
    cull, cull_ms = None, None
    if a.mask_cull:
        import dtu_cull_ref as CR
        size = (a.width, a.height)
        world, _ = CR.ring_cameras(a.views, a.scale, tuple(np.array([0.0, 0.0, 6.0]) * a.scale + t), size)
        masks = np.stack([CR.ellipse_mask(a.height, a.width, k % 3) for k in range(a.views)])
        cull = (E.view_matrices(world, [S] * a.views), masks)
    run = lambda: E.evaluate_mesh(mesh.vertices, mesh.triangles, stl, mask, bb, res, plane, scale_mat=S, cull=cull)  # noqa: E731
    run()
    r = run()
    verts_mesh, tris_mesh = mesh.vertices, mesh.triangles
    if a.mask_cull:
        dv, dt, dm = E._points(mesh.vertices, "cuda"), E.triangles_i32(mesh.triangles, "cuda"), torch.as_tensor(cull[1]).cuda()
        E.cull_mesh(dv, dt, cull[0], dm, image_size=size)
        cull_ms = {}
        cv, ct = E.cull_mesh(dv, dt, cull[0], dm, image_size=size, times=cull_ms)  # the inputs already on the device
        px = a.views * a.width * a.height
        cull_ms["dilate_min_traffic_GBps"] = round(px * 1.125 / (cull_ms["dilate"] * 1e-3) / 1e9, 1)
        from scipy import ndimage
        t0 = time.perf_counter()
        host = ndimage.binary_dilation(cull[1][0] != 0, structure=CR.disk(E.CULL_RADIUS))
        cull_ms["host_dilate_one_mask"] = round(1e3 * (time.perf_counter() - t0), 1)
        cull_ms["host_dilate_all_views"] = round(cull_ms["host_dilate_one_mask"] * a.views, 1)
        assert np.array_equal(host, E.dilate_masks(dm[:1]).unpack()[0])
        verts_mesh, tris_mesh = cv.cpu().numpy(), ct.cpu().numpy()
    # the CPU restatement on a fraction of the same job
    import dtu_eval_ref as R
    verts = R.world_transform(np.asarray(verts_mesh, np.float64), S)
    cloud = E.sample_mesh_points(verts, tris_mesh).cpu().numpy()
    sh = cloud[E.shuffle_order(len(cloud), 0)][: a.cpu_points]
    t0 = time.perf_counter()
    keep = R.thin(sh, 0.2)
    t_thin = time.perf_counter() - t0
    t0 = time.perf_counter()
    R.nearest(sh[keep], stl, 20.0)
    t_d2s = time.perf_counter() - t0
    print(json.dumps({
        "workload": f"{a.views} views {a.width}x{a.height}, voxel {a.voxel} ({a.voxel * a.scale:.3f} mm), synthetic surface scene x {a.scale} mm, "
                    f"{a.stl} STL points",
        "gpu_ms": r["ms"], "gpu_ms_total": round(sum(r["ms"].values()), 3),
        **({"cull_ms": cull_ms, "culled": {k: r[k] for k in ("n_vertices_culled", "n_triangles_culled")}} if a.mask_cull else {}),
        "counts": {k: r[k] for k in ("n_vertices", "n_triangles", "n_cloud", "n_down", "n_in", "n_in_obs", "n_stl", "n_stl_above",
                                     "thin_rounds")},
        "means": {k: r[k] for k in ("mean_d2s", "mean_s2d", "overall")},
        "cpu_restatement": {"points": len(sh), "of_cloud": len(cloud), "thin_ms": round(1e3 * t_thin, 1),
                            "d2s_ms": round(1e3 * t_d2s, 1), "d2s_queries": int(keep.sum())}}))


if __name__ == "__main__":
    main()
