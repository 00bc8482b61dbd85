"""The mesh ray casting timed on tools/mesh_texture_bench.py's mesh: the fused sphere-and-disc surface simplified at 8 voxels with
an atlas at most 2048 wide.  Timed: the BVH build, the ambient occlusion of every texel at K = 64 (gs2m_bvh_ao: one wave per point), and
the vertex pass.  The yardstick is the same `visible`
counts formed by a brute-force torch expression of the triangle test -- every ray against every triangle -- for a subset of
4096 owned texels on the same GPU, scaled per ray; its counts are compared with the library's.  Each figure is the median of
`--repeats` timed passes after one warm-up, host clock between synchronisations; writes profiles/mesh_ao_bench.json (or --out)
and prints it.  Nothing has measured this before: no threshold.  All data is synthetic.

    python tools/mesh_ao_bench.py [--views 49] [--voxel 0.004] [--repeats 5] [--size 2048] [--rays 64]
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

import gs2m_mesh_ao as AO  # noqa: E402
import gs2m_mesh_bvh as BV  # noqa: E402
import gs2m_mesh_texture as MT  # noqa: E402
from mesh_bake_bench import H, W, timed  # noqa: E402

SUBSET = 4096


def torch_visible(verts, tris, origins, dirs, skip, radius, chunk=16):
    """visible (n,) of rays dirs (n, K, 3) from origins (n, 3), each point skipping triangle skip[n], by the header's triangle
    test of every ray against every triangle, in torch fp64 operators (no contract on contraction: a yardstick, compared up to
    a count)"""
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    p = verts[tris.long()]
    a, e1, e2 = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    ids = torch.arange(len(tris), device=verts.device)
    out = []
    for s in range(0, len(origins), chunk):
        o, d = origins[s:s + chunk, None, None], dirs[s:s + chunk, :, None]           # (c, 1, 1, 3), (c, K, 1, 3)
        P = torch.linalg.cross(d, e2.expand(d.shape[0], d.shape[1], -1, -1))
        det = dot(e1, P)
        T = o - a
        u = dot(T, P) / det
        Q = torch.linalg.cross(T, e1.expand(T.shape[0], 1, -1, -1))
        v = dot(d, Q) / det
        t = dot(e2, Q) / det
        hit = (det != 0) & torch.isfinite(det) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > 0) & (t <= radius)
        hit &= ids[None, None] != skip[s:s + chunk, None, None]
        out.append((~hit.any(2)).sum(1))
    return torch.cat(out).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--voxel", type=float, default=0.004)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_ao_bench.json"))
    a = ap.parse_args()
    import gs2m_mesh as M
    import mesh_bench as MBench
    cams, depths, colors = MBench.scene(200_000, a.views, W, H)
    lo, hi = M._depth_aabb(depths, cams, 10.0, torch.device("cuda"))
    L, tr = 16 * a.voxel, 4 * a.voxel
    _, mesh, _, _ = MBench.fuse(cams, depths, colors, a.voxel, 10.0, 4096, lo - tr - L, hi + tr + L)
    del depths, colors
    dev = torch.device("cuda")
    simple = M.simplify_mesh_gpu(M.DeviceMesh.from_mesh(mesh, dev), cell=8 * a.voxel)
    mesh = types.SimpleNamespace(vertices=simple.vertices.to(torch.float64).contiguous(), triangles=simple.triangles.to(torch.int32).contiguous())
    atlas = MT.build_atlas(mesh, texture_size=a.size)
    K = a.rays
    ms = lambda t: {"median_ms": round(t[0], 3), "min_ms": round(t[1], 3), "max_ms": round(t[2], 3)}
    result = {"workload": f"voxel {a.voxel} simplified at 8 voxels, atlas {atlas.width} x {atlas.height}, K = {K}, 16 tables, default radius and bias, "
                          "synthetic surface scene", "n_vertices": len(mesh.vertices), "n_triangles": len(mesh.triangles), "repeats": a.repeats}
    bvh = BV.build_bvh(mesh.vertices, mesh.triangles)
    result["build"] = ms(timed(lambda: BV.build_bvh(mesh.vertices, mesh.triangles), a.repeats))
    result["bvh_bytes"] = bvh.buffer.numel()
    # the traversal alone: the texels' points are made once, outside the clock
    owner, points, normals = AO.texel_points(atlas)
    owner, points, normals = owner.reshape(-1), points.reshape(-1, 3).contiguous(), normals.reshape(-1, 3).contiguous()
    n_owned = int((owner >= 0).sum())
    sampler = AO._Sampler(bvh, K, AO.TABLES, None, None, 0)
    result.update(radius=sampler.radius, bias=sampler.bias, n_texels=len(owner), n_owned=n_owned, rays=n_owned * K)
    visible = sampler.visible(points, normals, owner)
    t = timed(lambda: sampler.visible(points, normals, owner), a.repeats)
    result["texels"] = dict(ms(t), rays_per_s=round(n_owned * K / (t[0] * 1e-3)))
    result["mean_ao_owned"] = round(float(visible[owner >= 0].double().mean()) / K, 4)
    result["texel_occlusion_end_to_end"] = ms(timed(lambda: AO.texel_occlusion(atlas, rays=K, bvh=bvh), a.repeats))
    # the vertex pass, its normals included
    t = timed(lambda: AO.vertex_occlusion(mesh, rays=K, bvh=bvh), a.repeats)
    result["vertices"] = dict(ms(t), rays_per_s=round(len(mesh.vertices) * K / (t[0] * 1e-3)))
    # the yardstick: a subset of owned texels, every ray against every triangle in torch operators
    pick = torch.nonzero(owner >= 0).reshape(-1)
    pick = pick[torch.linspace(0, len(pick) - 1, min(SUBSET, len(pick)), device=dev).long()]
    unit = BV.unit_rows(normals[pick])
    table = sampler.dirs
    x = (pick + sampler.seed) & 0xFFFFFFFF                 # mix32 of the header, index0 = 0
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    r = (x ^ (x >> 16)) % AO.TABLES
    sg = torch.copysign(torch.ones_like(unit[:, 2]), unit[:, 2])
    q = -1.0 / (sg + unit[:, 2])
    bb = (unit[:, 0] * unit[:, 1]) * q
    Tn = torch.stack([1.0 + ((sg * unit[:, 0]) * unit[:, 0]) * q, sg * bb, -(sg * unit[:, 0])], 1)
    Bn = torch.stack([bb, sg + (unit[:, 1] * unit[:, 1]) * q, -unit[:, 1]], 1)
    l = table[r]
    dirs = (Tn[:, None] * l[..., 0:1] + Bn[:, None] * l[..., 1:2]) + unit[:, None] * l[..., 2:3]
    origins = points[pick] + unit * sampler.bias
    brute = torch_visible(mesh.vertices, mesh.triangles, origins, dirs, owner[pick], sampler.radius)
    t = timed(lambda: torch_visible(mesh.vertices, mesh.triangles, origins, dirs, owner[pick], sampler.radius), max(1, a.repeats // 2))
    result["torch_brute_force_subset"] = dict(ms(t), points=len(pick), rays_per_s=round(len(pick) * K / (t[0] * 1e-3)))
    result["torch_counts_differ"] = int((brute != visible[pick]).sum())
    result["speedup_per_ray_over_torch"] = round(result["texels"]["rays_per_s"] / result["torch_brute_force_subset"]["rays_per_s"], 1)
    text = json.dumps(result, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
