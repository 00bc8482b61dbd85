"""The textured-mesh export timed on tools/mesh_bake_bench.py's scene: the fused sphere-and-disc mesh simplified at 8 voxels, an
atlas at 2048 and at 4096, five random attribute planes per view baked into its texels from 49 cameras at 1600 x 1200, resolve
and pack, the two PNG routes and the .glb; and the normal-map path of DESIGN.md §23: the same accumulate with eight planes, the
tangent-space conversion beside the same conversion in torch operators (`torch_normals`), and one 1600 x 1200 view at ss = 2 through
the textured G-buffer beside the vertex-attribute G-buffer.  The yardstick is the same bake of one batch of views written with
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


def torch_normals(owner, tn, tris, uvs, verts, values):
    """gs2m_texture_normals for owned texels with usable frames, formed with torch operators: the yardstick -> (n, 3) uint8"""
    t = tris[owner.long()].long()
    a, b, c = verts[t[:, 0]], verts[t[:, 1]], verts[t[:, 2]]
    uv = uvs[owner.long()].double()
    e1, e2 = b - a, c - a
    d1, d2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
    det = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
    du = (e1 * d2[:, 1:2] - e2 * d1[:, 1:2]) / det[:, None]
    nf = torch.linalg.cross(e1, e2)
    n = torch.nn.functional.normalize(tn, dim=1)
    n = torch.where(((n * nf).sum(1) > 0)[:, None], n, torch.nn.functional.normalize(nf, dim=1))
    T = torch.nn.functional.normalize(du - n * (n * du).sum(1, keepdim=True), dim=1)
    B = -torch.linalg.cross(n, T)
    w = torch.nn.functional.normalize(values.double(), dim=1)
    m = torch.stack([(w * T).sum(1), (w * B).sum(1), (w * n).sum(1).clamp_min(0.0)], 1)
    m = torch.nn.functional.normalize(m, dim=1)
    return torch.floor(255.0 * (0.5 * m + 0.5) + 0.5).to(torch.uint8)


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
        # the normal-map path: eight planes through the same kernel, the conversion, and the textured G-buffer
        maps8 = torch.rand((b, 8, H, W), generator=gen, device=dev)
        sums8 = torch.zeros((n, 8), dtype=torch.float64, device=dev)

        def kernel_eight():
            N.launch("gs2m_texbake_accumulate", dev, n, pts.data_ptr(), nrm.data_ptr(), baker.owner.data_ptr(), len(part), part.data_ptr(), *k, W, H,
                     depth.data_ptr(), 8, maps8.data_ptr(), mask.data_ptr(), K.EPS, 0, sums8.data_ptr(), wsum.data_ptr())

        t_kernel8 = timed(kernel_eight, a.repeats)
        t_kernel_again = timed(kernel_only, a.repeats)
        del maps8
        values8 = torch.cat([values.reshape(-1, C), torch.nn.functional.normalize(nrm.float() + 0.3 * torch.randn((n, 3), generator=gen, device=dev), dim=1)], 1)
        values8 = values8.reshape(atlas.height, atlas.width, 8).contiguous()
        del sums8
        nmap = torch.empty((n, 3), dtype=torch.uint8, device=dev)
        flat_owner = baker.owner.reshape(-1)

        def normals_kernel():
            N.launch("gs2m_texture_normals", dev, n, flat_owner.data_ptr(), nrm.data_ptr(), len(atlas.triangles), atlas.triangles.data_ptr(),
                     atlas.uvs.data_ptr(), len(atlas.vertices), atlas.vertices.data_ptr(), 8, 5, values8.data_ptr(), nmap.data_ptr(), None)

        t_normals = timed(normals_kernel, a.repeats)
        oo, on_, ov = flat_owner[owned].contiguous(), nrm[owned].contiguous(), values8.reshape(-1, 8)[owned][:, 5:].contiguous()
        t_normals_torch = timed(lambda: torch_normals(oo, on_, atlas.triangles, atlas.uvs, atlas.vertices, ov), a.repeats)
        agree = float((torch_normals(oo, on_, atlas.triangles, atlas.uvs, atlas.vertices, ov).int() - nmap[owned].int()).abs().le(1).all(1).float().mean())
        del oo, on_, ov
        import gs2m_mesh_view as MVW
        one, ss = w2c[:1], 2
        vis = MVW.visibility_buffer(atlas.vertices, atlas.triangles, one, *k, H, W, ss)
        nv = len(atlas.vertices)
        alb, rough, metal = torch.rand((nv, 3), generator=gen, device=dev), torch.rand(nv, generator=gen, device=dev), torch.rand(nv, generator=gen, device=dev)
        tex_base = torch.randint(0, 256, (atlas.height, atlas.width, 3), generator=gen, device=dev, dtype=torch.uint8)
        tex_orm = torch.randint(0, 256, (atlas.height, atlas.width, 3), generator=gen, device=dev, dtype=torch.uint8)
        tex_nm = nmap.reshape(atlas.height, atlas.width, 3)
        vn = MVW.vertex_normals(atlas.vertices, atlas.triangles)[0]
        t_gbuf = timed(lambda: MVW.mesh_gbuffer(atlas.vertices, atlas.triangles, one, *k, H, W, vis.reshape(-1), alb, rough, metal, ss, vn), a.repeats)
        t_gbuf_tex = timed(lambda: MVW.mesh_gbuffer_textured(atlas.vertices, atlas.triangles, atlas.uvs, one, *k, H, W, vis.reshape(-1), tex_base, tex_orm,
                                                             tex_nm, True, ss, vn), a.repeats)
        t_gbuf_tex_plain = timed(lambda: MVW.mesh_gbuffer_textured(atlas.vertices, atlas.triangles, atlas.uvs, one, *k, H, W, vis.reshape(-1), tex_base,
                                                                   tex_orm, None, True, ss, vn), a.repeats)
        covered = int((vis != -1).sum())
        del vis, tex_base, tex_orm, tex_nm, nmap, values8
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
            "glb_write": ms(t_glb),
            "normal_map": {
                "accumulate_kernel_one_batch_c8": ms(t_kernel8), "accumulate_kernel_one_batch_c5_same_run": ms(t_kernel_again),
                "c8_over_c5": round(t_kernel8[0] / t_kernel_again[0], 3),
                "texture_normals": ms(t_normals), "texture_normals_torch_operators_owned_texels": ms(t_normals_torch),
                "torch_over_kernel": round(t_normals_torch[0] / t_normals[0], 2), "bytes_within_one_of_torch": agree,
                "gbuffer_view": f"{W}x{H} ss=2, {covered} covered samples",
                "gbuffer_vertex_attributes": ms(t_gbuf), "gbuffer_textured_with_normal_map": ms(t_gbuf_tex),
                "gbuffer_textured_without_normal_map": ms(t_gbuf_tex_plain), "textured_over_vertex": round(t_gbuf_tex[0] / t_gbuf[0], 3)}}
        del baker, sums, wsum, pts, nrm, po, no, values, seen, base, orm
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
