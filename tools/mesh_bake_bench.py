"""The per-vertex bake and one PBR mesh view timed on tools/tnt_cull_bench.py's scene: tools/mesh_bench.py's sphere and ground disc
fused from 49 views at 1600 x 1200 and extracted at `--voxel`, then (a) five random attribute planes per view baked onto the
mesh's vertices from the same 49 cameras -- the z-buffer of the mesh included, and the accumulate kernel alone -- (b) the same bake
written with torch.nn.functional.grid_sample (align_corners=True, border padding) and torch arithmetic on the same depth maps, and
(c) one PBR view of the material mesh at 1600 x 1200, ss = 2.  Each figure is the median of `--repeats` timed passes after one
warm-up, bracketed by synchronisations; writes profiles/mesh_bake_bench.json and prints it.  Nothing has measured this before: no
threshold.  All data is synthetic.

    python tools/mesh_bake_bench.py [--views 49] [--voxel 0.004] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-2m_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import gs2m_mesh_bake as MB  # noqa: E402
import gs2m_mesh_cull as K  # noqa: E402
import gs2m_mesh_view as MV  # noqa: E402
import gs2m_native as N  # noqa: E402

W, H, C = 1600, 1200, 5


def timed(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out), min(out), max(out)


def torch_bake(v, normals, w2c, k, depth, maps, mask, eps):
    """the bake of one batch of views with grid_sample: the same tests, fp32 sampling, fp64 sums -> (sums (V, C), weights (V,))"""
    fx, fy, cx, cy = k
    n = len(w2c)
    cam = torch.einsum("nij,vj->nvi", w2c[:, :3, :3], v) + w2c[:, None, :3, 3]
    z = cam[..., 2] + 1e-8
    u, t = (fx * cam[..., 0] + cx * cam[..., 2]) / z, (fy * cam[..., 1] + cy * cam[..., 2]) / z
    inside = (u >= 0) & (u <= W - 1) & (t >= 0) & (t <= H - 1) & (z > 0)
    grid = torch.stack([2 * u / (W - 1) - 1, 2 * t / (H - 1) - 1], dim=-1).float()[:, None]  # (n, 1, V, 2)
    planes = torch.cat([depth[:, None], mask[:, None], maps], dim=1)
    s = F.grid_sample(planes, grid, mode="bilinear", padding_mode="border", align_corners=True)[:, :, 0].double()  # (n, 2 + C, V)
    d, m, a = s[:, 0], s[:, 1], s[:, 2:]
    front = torch.where(d > 0, z < d + eps, torch.ones_like(inside))
    centre = -torch.einsum("nji,nj->ni", w2c[:, :3, :3], w2c[:, :3, 3])
    e = centre[:, None] - v[None]
    w = ((normals[None] * e).sum(-1) / (normals.norm(dim=-1)[None] * e.norm(dim=-1))).clamp(min=0)
    w = torch.where(inside & front & (m >= 1.0), w, torch.zeros_like(w))
    return torch.einsum("nv,ncv->vc", w, a), w.sum(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--voxel", type=float, default=0.004)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--view-batch", type=int, default=K.VIEW_BATCH)
    a = ap.parse_args()
    import gs2m_envmap as E
    import gs2m_mesh as M
    import mesh_bench as MBench
    cams, depths, colors = MBench.scene(200_000, a.views, W, H)
    lo, hi = M._depth_aabb(depths, cams, 10.0, torch.device("cuda"))
    L, tr = 16 * a.voxel, 4 * a.voxel
    _, mesh, _, _ = MBench.fuse(cams, depths, colors, a.voxel, 10.0, 4096, lo - tr - L, hi + tr + L)
    del depths, colors
    dev = torch.device("cuda")
    v = torch.as_tensor(np.asarray(mesh.vertices, np.float64)).to(dev).contiguous()
    f = torch.as_tensor(np.asarray(mesh.triangles, np.int32)).to(dev).contiguous()
    w2c = torch.stack([c.world_view_transform.transpose(0, 1).to(torch.float64) for c in cams]).contiguous()
    k = (float(cams[0].Fx), float(cams[0].Fy), float(cams[0].Cx) - 0.5, float(cams[0].Cy) - 0.5)
    gen = torch.Generator(device=dev).manual_seed(0)
    b = a.view_batch
    maps = torch.rand((b, C, H, W), generator=gen, device=dev)  # one batch's planes, reused for every batch: 49 views' would be 1.9 GB
    mask = (torch.rand((b, H, W), generator=gen, device=dev) > 0.05).float()
    normals = MV.vertex_normals(v, f)[0]
    n_verts, n_tris = len(v), len(f)

    def bake_all():
        baker = MB.Baker(v, f, C)
        for s in range(0, a.views, b):
            part = w2c[s:s + b]
            baker.add(part, *k, maps[:len(part)], mask[:len(part)])
        return baker.finish()

    t_bake = timed(bake_all, a.repeats)
    values, seen, weights = bake_all()
    # the accumulate kernel alone and the grid_sample form, on one batch's depth maps
    part = w2c[:b]
    depth = K.render_mesh_depth(v, f, part, *k, H, W)
    sums = torch.zeros((n_verts, C), dtype=torch.float64, device=dev)
    wsum = torch.zeros(n_verts, dtype=torch.float64, device=dev)

    def kernel_only():
        N.launch("gs2m_meshbake_accumulate", dev, n_verts, v.data_ptr(), normals.data_ptr(), len(part), part.data_ptr(), *k, W, H, depth.data_ptr(), C,
                 maps.data_ptr(), mask.data_ptr(), K.EPS, 0, sums.data_ptr(), wsum.data_ptr())

    t_kernel = timed(kernel_only, a.repeats)
    t_torch = timed(lambda: torch_bake(v, normals, part, k, depth, maps, mask, K.EPS), a.repeats)
    ts, tw = torch_bake(v, normals, part, k, depth, maps, mask, K.EPS)
    both = (wsum > 0) & (tw > 0)
    agree = float(((wsum > 0) == (tw > 0)).double().mean())
    diff = float(((sums[both] / wsum[both, None]) - (ts[both] / tw[both, None])).abs().max()) if both.any() else None
    # one PBR view
    light = E.EnvLight(torch.rand((6, 64, 64, 3), generator=gen, device=dev))
    alb, rough, metal = values[:, :3].contiguous(), values[:, 3].contiguous(), values[:, 4].contiguous()
    kv = (float(cams[0].Fx), float(cams[0].Fy), float(cams[0].Cx), float(cams[0].Cy))
    t_view = timed(lambda: MV.shade_views_pbr(v, f, w2c[:1], *kv, H, W, light, alb, rough, metal, ss=2), a.repeats)
    ms = lambda t: {"median_ms": round(t[0], 3), "min_ms": round(t[1], 3), "max_ms": round(t[2], 3)}
    result = {"workload": f"{a.views} views {W}x{H}, C = {C}, voxel {a.voxel}, synthetic surface scene", "n_vertices": n_verts, "n_triangles": n_tris,
              "view_batch": b, "repeats": a.repeats, "seen_vertices": int(seen.sum()),
              "bake_all_views_with_depth": ms(t_bake), "bake_ms_per_view_with_depth": round(t_bake[0] / a.views, 3),
              "accumulate_kernel_one_batch": ms(t_kernel), "accumulate_kernel_ms_per_view": round(t_kernel[0] / len(part), 3),
              "vertex_views_per_s": round(n_verts * len(part) / (1e-3 * t_kernel[0])),
              "grid_sample_one_batch": ms(t_torch), "grid_sample_ms_per_view": round(t_torch[0] / len(part), 3),
              "grid_sample_over_kernel": round(t_torch[0] / t_kernel[0], 2), "seen_agreement_with_grid_sample": agree,
              "max_abs_difference_to_grid_sample": diff, "pbr_view_1600x1200_ss2": ms(t_view)}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_bake_bench.json"), "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
