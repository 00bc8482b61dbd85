"""The closest-hit query and the detail transfer timed on tools/mesh_texture_bench.py's mesh: the fused sphere-and-disc surface
is the source, its simplification at 8 voxels with an atlas at most 2048 wide the target.  Timed: the BVH build over the source,
gs2m_bvh_closest beside gs2m_bvh_occluded on the SAME rays (the owned texels' forward rays: any-hit is the natural floor, the
ratio of the two is the finding), transfer_texels end to end (five channels and the normal), and as the only other formulation
available a brute-force torch expression -- every ray against every source triangle -- on a subset of the texels, whose answers
are compared with the library's.  Each figure is the median of `--repeats` timed passes after one warm-up, host clock between
synchronisations; writes profiles/mesh_transfer_bench.json (or --out) and prints it.  Nothing has measured this before: no
threshold.  All data is synthetic.

    python tools/mesh_transfer_bench.py [--views 49] [--voxel 0.004] [--repeats 5] [--size 2048] [--subset 2048]
"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-2m_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import gs2m_mesh_bvh as BV  # noqa: E402
import gs2m_mesh_texture as MT  # noqa: E402
import gs2m_mesh_transfer as T  # noqa: E402
from mesh_bake_bench import H, W, timed  # noqa: E402


def torch_closest(verts, tris, origins, dirs, tmax, facing, chunk=2):
    """(tri (n,) int64, -1 for a miss; t (n,) float64) of the header's Candidate, Facing and Answer paragraphs by every ray against
    every triangle in torch fp64 operators (no contract on contraction: a yardstick, compared up to a count)"""
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    p = verts[tris.long()]
    a, e1, e2 = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    out_tri, out_t = [], []
    for s in range(0, len(origins), chunk):
        o, d = origins[s:s + chunk, None], dirs[s:s + chunk, None]                    # (c, 1, 3)
        P = torch.linalg.cross(d.expand(-1, len(a), -1), e2.expand(len(o), -1, -1))
        det = dot(e1, P)
        Tv = o - a
        u = dot(Tv, P) / det
        Q = torch.linalg.cross(Tv, e1.expand(len(o), -1, -1))
        v = dot(d, Q) / det
        t = dot(e2, Q) / det
        ok = (det != 0) & torch.isfinite(det) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= tmax)
        ok &= (det > 0) if facing > 0 else (det < 0) if facing < 0 else ok
        t = torch.where(ok, t, torch.full_like(t, float("inf")))
        best = t.min(1)                                                               # the first index among equal values is not
        out_t.append(best.values)                                                    # promised by torch: ties are counted apart
        out_tri.append(torch.where(ok.any(1), best.indices, torch.full_like(best.indices, -1)))
    return torch.cat(out_tri), torch.cat(out_t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--voxel", type=float, default=0.004)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--subset", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_transfer_bench.json"))
    a = ap.parse_args()
    import gs2m_mesh as M
    import mesh_bench as MBench
    cams, depths, colors = MBench.scene(200_000, a.views, W, H)
    lo, hi = M._depth_aabb(depths, cams, 10.0, torch.device("cuda"))
    L, tr = 16 * a.voxel, 4 * a.voxel
    _, mesh, _, _ = MBench.fuse(cams, depths, colors, a.voxel, 10.0, 4096, lo - tr - L, hi + tr + L)
    del depths, colors
    dev = torch.device("cuda")
    full = M.DeviceMesh.from_mesh(mesh, dev)
    simple = M.simplify_mesh_gpu(full, cell=8 * a.voxel)
    source = types.SimpleNamespace(vertices=full.vertices.to(torch.float64).contiguous(), triangles=full.triangles.to(torch.int32).contiguous())
    low = types.SimpleNamespace(vertices=simple.vertices.to(torch.float64).contiguous(), triangles=simple.triangles.to(torch.int32).contiguous())
    atlas = MT.build_atlas(low, texture_size=a.size)
    distance = T.DISTANCE_SHARE * BV.live_diagonal(atlas.vertices, atlas.triangles)
    ms = lambda t: {"median_ms": round(t[0], 3), "min_ms": round(t[1], 3), "max_ms": round(t[2], 3)}
    result = {"workload": f"source: voxel {a.voxel}; target: its simplification at 8 voxels, atlas {atlas.width} x {atlas.height}; default distance, "
                          "one-sided, synthetic surface scene", "source_vertices": len(source.vertices), "source_triangles": len(source.triangles),
              "target_vertices": len(low.vertices), "target_triangles": len(low.triangles), "distance": distance, "repeats": a.repeats}
    bvh = BV.build_bvh(source.vertices, source.triangles)
    result["build"] = ms(timed(lambda: BV.build_bvh(source.vertices, source.triangles), a.repeats))
    result["bvh_bytes"] = bvh.buffer.numel()
    # the two queries on the same rays: the owned texels' forward rays, made once, outside the clock
    owner, points, normals = T.texel_rays(atlas)
    keep = owner.reshape(-1) >= 0
    origins, dirs = points.reshape(-1, 3)[keep].contiguous(), normals.reshape(-1, 3)[keep].contiguous()
    n = len(origins)
    result.update(n_texels=owner.numel(), n_owned=n)
    blocked = BV.occluded(bvh, origins, dirs, 0.0, distance)
    tri, t_hit, _ = BV.closest(bvh, origins, dirs, 0.0, distance)
    t0 = timed(lambda: BV.occluded(bvh, origins, dirs, 0.0, distance), a.repeats)
    t1 = timed(lambda: BV.closest(bvh, origins, dirs, 0.0, distance), a.repeats)
    result["occluded"] = dict(ms(t0), rays_per_s=round(n / (t0[0] * 1e-3)), hit_share=round(float(blocked.double().mean()), 4))
    result["closest"] = dict(ms(t1), rays_per_s=round(n / (t1[0] * 1e-3)), hit_share=round(float((tri >= 0).double().mean()), 4))
    result["closest_over_occluded"] = round(t1[0] / t0[0], 3)
    result["hit_masks_differ_off_tmin"] = int(((tri >= 0) != blocked)[t_hit != 0].sum())
    # the transfer end to end: fill, texel points, both rays, interpolation, in bands
    values = torch.rand((len(source.vertices), 5), device=dev)
    out = T.transfer_texels(atlas, source, values, normal=True, bvh=bvh)
    result["transfer_texels_end_to_end"] = ms(timed(lambda: T.transfer_texels(atlas, source, values, normal=True, bvh=bvh), a.repeats))
    hit, offset = out[1].reshape(-1)[keep], out[2].reshape(-1)[keep]
    result.update(transfer_hit_share=round(float((hit >= 0).double().mean()), 4), transfer_backward_share=round(float((offset < 0).double().mean()), 4),
                  transfer_max_offset=float(offset.abs().max()))
    # the yardstick: a subset of the rays, every ray against every source triangle in torch operators
    pick = torch.linspace(0, n - 1, min(a.subset, n), device=dev).long()
    brute_tri, brute_t = torch_closest(source.vertices, source.triangles, origins[pick], dirs[pick], distance, 0)
    t = timed(lambda: torch_closest(source.vertices, source.triangles, origins[pick], dirs[pick], distance, 0), max(1, a.repeats // 2))
    result["torch_brute_force_subset"] = dict(ms(t), rays=len(pick), rays_per_s=round(len(pick) / (t[0] * 1e-3)))
    result["torch_t_differ"] = int((brute_t != t_hit[pick]).sum())
    result["torch_tri_differ"] = int((brute_tri != tri[pick].long()).sum())
    result["speedup_per_ray_over_torch"] = round(result["closest"]["rays_per_s"] / result["torch_brute_force_subset"]["rays_per_s"], 1)
    text = json.dumps(result, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
