"""The textured-mesh export timed on tools/mesh_bake_bench.py's scene: the fused sphere-and-disc mesh simplified at 8 voxels, an
atlas at 2048 and at 4096, five random attribute planes per view baked into its texels from 49 cameras at 1600 x 1200, resolve
and pack, the two PNG routes and the .glb.  The yardstick is the same bake of one batch of views written with
torch.nn.functional.grid_sample (mesh_bake_bench.torch_bake) on the same GPU.  Each figure is the median of `--repeats` timed
passes after one warm-up, host clock between synchronisations; writes profiles/mesh_texture_bench.json (or --out) and prints it.
Nothing has measured this before: no threshold.  All data is synthetic.

    python tools/mesh_texture_bench.py [--views 49] [--voxel 0.004] [--repeats 5] [--sizes 2048 4096]
"""
import argparse
import json
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-2m_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import gs2m_mesh_cull as K  # noqa: E402
import gs2m_mesh_texture as MT  # noqa: E402
import gs2m_native as N  # noqa: E402
from mesh_bake_bench import C, H, W, timed, torch_bake  # noqa: E402

VERTEX_BAKE_RATE = 6.2e10  # vertex-views per second of gs2m_meshbake_accumulate (profiles/mesh_bake_bench.json)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--voxel", type=float, default=0.004)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--view-batch", type=int, default=K.VIEW_BATCH)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_texture_bench.json"))
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
    w2c = torch.stack([c.world_view_transform.transpose(0, 1).to(torch.float64) for c in cams]).contiguous()
    k = (float(cams[0].Fx), float(cams[0].Fy), float(cams[0].Cx) - 0.5, float(cams[0].Cy) - 0.5)
    gen = torch.Generator(device=dev).manual_seed(0)
    b = a.view_batch
    maps = torch.rand((b, C, H, W), generator=gen, device=dev)  # one batch's planes, reused for every batch
    mask = (torch.rand((b, H, W), generator=gen, device=dev) > 0.05).float()
    ms = lambda t: {"median_ms": round(t[0], 3), "min_ms": round(t[1], 3), "max_ms": round(t[2], 3)}
    result = {"workload": f"{a.views} views {W}x{H}, C = {C}, voxel {a.voxel} simplified at 8 voxels, synthetic surface scene",
              "n_vertices": len(mesh.vertices), "n_triangles": len(mesh.triangles), "view_batch": b, "repeats": a.repeats,
              "vertex_bake_vertex_views_per_s": VERTEX_BAKE_RATE, "sizes": {}}
    for size in a.sizes:
        atlas = MT.build_atlas(mesh, texture_size=size)
        t_search = timed(lambda: MT.build_atlas(mesh, texture_size=size), a.repeats)
        t_build = timed(lambda: MT.build_atlas(mesh, density=atlas.density), a.repeats)
        normals = __import__("gs2m_mesh_view").vertex_normals(atlas.vertices, atlas.triangles)[0]
        t_texels = timed(lambda: MT.atlas_texels(atlas, normals), a.repeats)

        def bake_all():
            baker = MT.TextureBaker(atlas, C)
            for s in range(0, a.views, b):
                part = w2c[s:s + b]
                baker.add(part, *k, maps[:len(part)], mask[:len(part)])
            return baker

        t_bake = timed(bake_all, a.repeats)
        baker = bake_all()
        t_resolve = timed(lambda: MT.pack_textures(baker.finish()[0]), a.repeats)
        values, seen, _ = baker.finish()
        base, orm = MT.pack_textures(values)
        # the accumulate kernel alone and the grid_sample form, on one batch's depth maps
        part = w2c[:b]
        depth = K.render_mesh_depth(atlas.vertices, atlas.triangles, part, *k, H, W)
        owned = baker.owner.reshape(-1) >= 0
        n, n_owned = baker.n, int(owned.sum())
        sums, wsum = torch.zeros((n, C), dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
        pts, nrm = baker.points.reshape(-1, 3), baker.normals.reshape(-1, 3)

        def kernel_only():
            N.launch("gs2m_texbake_accumulate", dev, n, pts.data_ptr(), nrm.data_ptr(), baker.owner.data_ptr(), len(part), part.data_ptr(), *k, W, H,
                     depth.data_ptr(), C, maps.data_ptr(), mask.data_ptr(), K.EPS, 0, sums.data_ptr(), wsum.data_ptr())

        t_kernel = timed(kernel_only, a.repeats)
        po, no = pts[owned].contiguous(), nrm[owned].contiguous()
        t_torch = timed(lambda: torch_bake(po, no, part, k, depth, maps, mask, K.EPS), a.repeats)
        t_png_host = timed(lambda: MT.encode_png([base, orm], False), a.repeats)
        t_png_dev = timed(lambda: MT.encode_png([base, orm], True), a.repeats)
        pngs = MT.encode_png([base, orm], True)
        geo = MT.unwelded(atlas)
        with tempfile.TemporaryDirectory() as d:
            t_glb = timed(lambda: MT.write_glb(os.path.join(d, "a.glb"), *geo, pngs), a.repeats)
        result["sizes"][str(size)] = {
            "width": atlas.width, "height": atlas.height, "density": atlas.density, "hist": atlas.hist, "owned_texels": n_owned, "texels": n,
            "seen_texels": int(seen.sum()), "atlas_search": ms(t_search), "atlas_build": ms(t_build), "texel_generation": ms(t_texels),
            "bake_all_views_with_depth_and_texels": ms(t_bake), "bake_ms_per_view": round(t_bake[0] / a.views, 3),
            "accumulate_kernel_one_batch": ms(t_kernel), "accumulate_kernel_ms_per_view": round(t_kernel[0] / len(part), 3),
            "owned_texel_views_per_s": round(n_owned * len(part) / (1e-3 * t_kernel[0])),
            "grid_sample_one_batch_owned_texels": ms(t_torch), "grid_sample_over_kernel": round(t_torch[0] / t_kernel[0], 2),
            "resolve_and_pack": ms(t_resolve), "png_host_two_images": ms(t_png_host), "png_device_two_images": ms(t_png_dev),
            "glb_write": ms(t_glb)}
        del baker, sums, wsum, pts, nrm, po, no, values, seen, base, orm
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
