"""The mesh bake and mesh view paths give the bytes they gave when tests/golden/mesh_paths_digests.json was recorded: SHA-256
digests of the raw bytes of every output of the vertex bake, the texel bake with its packing, the visibility buffer, the shaded
views, both G-buffers, the RGB resolve and the PBR views, on an icosphere and a flat quad in frames of a few tens of pixels.

The golden file pins the arithmetic of csrc/mesh_bake.hip and csrc/mesh_view.hip and of the Python around them on the MI355X: a
digest that differs is a change of behaviour, not of the golden file.  Run as a script with --record, this file prints that JSON.
All data is synthetic."""
import hashlib
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(os.path.dirname(HERE), "gs-2m_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402

import gs2m_mesh_bake as MB  # noqa: E402
import gs2m_mesh_texture as MT  # noqa: E402
import gs2m_mesh_view as MVW  # noqa: E402
import mesh_texture_ref as T  # noqa: E402
import mesh_view_ref as MV  # noqa: E402
import tnt_cull_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "mesh_paths_digests.json")
H, W = 30, 40
K = (44.0, 44.5, 19.7, 14.6)  # fx, fy, cx, cy
FALLBACK = (0.1, 0.2, 0.3, 0.4, 0.5, 0.0, 0.0, 0.0)


def _cuda(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _scenes():
    """name -> (verts, tris, w2c): the level-2 icosphere of mesh_texture_ref from four cameras, the quad of mesh_view_ref (wound
    towards the cameras) from three"""
    v, f = T.icosphere(2)
    sphere = (0.9 * v + np.array([0.0, 0.0, 3.2]), f,
              np.stack([R.look_at(e, [0.0, 0.0, 3.2]) for e in ([0.0, 0.0, 0.0], [2.2, 0.3, 1.2], [-2.0, -0.4, 1.5], [0.4, 2.3, 2.0])]))
    qv, qf = MV.quad(z=2.0, half=0.5)
    quad = (qv, np.ascontiguousarray(qf[:, ::-1]),
            np.stack([R.look_at(e, [0.0, 0.0, 2.0]) for e in ([0.0, 0.0, 0.0], [0.5, 0.2, 0.3], [-0.4, -0.3, 0.2])]))
    return {"sphere": sphere, "quad": quad}


def _pbr_textured(args, light, ss, tex):
    """shade_views_pbr with the materials read from the texture set `tex`, smooth with the set's own vertex normals"""
    return MVW.shade_views_pbr(*args, light, ss=ss, shading="smooth", gamma=True, background="env", textures=tex)


def digests():
    """-> {name: SHA-256 of the output's raw bytes}"""
    import gs2m_envmap as E
    out = {}

    def put(name, t):
        assert name not in out
        out[name] = _sha(t)

    for seed, (scene, (verts, tris, w2c)) in enumerate(sorted(_scenes().items())):
        rng = np.random.default_rng(40 + seed)
        v, f, m = _cuda(verts, torch.float64), _cuda(tris, torch.int32), _cuda(w2c, torch.float64)
        n = len(m)
        maps = rng.random((n, 8, H, W)).astype(np.float32)
        maps[:, 5:] = 2.0 * maps[:, 5:] - 1.0  # the normal planes
        maps, mask = _cuda(maps), _cuda((rng.random((n, H, W)) > 0.1).astype(np.float32))
        att = _cuda(rng.random((len(verts), 8)).astype(np.float32))

        # vertex bake: C = 5, mask and normals, the views over two calls
        b = MB.Baker(v, f, 5)
        b.add(m[:2], *K, maps[:2, :5], mask[:2])
        b.add(m[2:], *K, maps[2:, :5], mask[2:])
        put(f"{scene}/vertex_bake/sums", b.sums)
        put(f"{scene}/vertex_bake/weights", b.weights)
        values, seen, _ = b.finish(0.3, FALLBACK[:5])
        put(f"{scene}/vertex_bake/values", values)
        put(f"{scene}/vertex_bake/seen", seen)
        values, seen, weights = MB.bake_vertex_attributes(v, f, m, *K, maps[:, :5], mask, view_batch=3, min_weight=0.3)
        put(f"{scene}/bake_vertex_attributes/values", values)
        put(f"{scene}/bake_vertex_attributes/seen", seen)
        put(f"{scene}/bake_vertex_attributes/weights", weights)

        # texel bake: the five planes and a normal's three
        atlas = MT.build_atlas(types.SimpleNamespace(vertices=v, triangles=f), density=21.0)
        tb = MT.TextureBaker(atlas, 8)
        tb.add(m[:2], *K, maps[:2], mask[:2])
        tb.add(m[2:], *K, maps[2:], mask[2:])
        put(f"{scene}/texel_bake/sums", tb.sums)
        put(f"{scene}/texel_bake/weights", tb.weights)
        plain, seen, _ = tb.finish(0.3, FALLBACK)
        put(f"{scene}/texel_bake/values", plain)
        put(f"{scene}/texel_bake/seen", seen)
        values, seen, _ = tb.finish(0.3, FALLBACK, att)
        put(f"{scene}/texel_bake/values_from_vertices", values)
        put(f"{scene}/texel_bake/seen_from_vertices", seen)
        five, seen5, w5 = MT.bake_texel_attributes(atlas, m, *K, maps[:, :5], mask, view_batch=3, min_weight=0.3, attributes=att[:, :5].contiguous())
        put(f"{scene}/bake_texel_attributes/values", five)
        put(f"{scene}/bake_texel_attributes/seen", seen5)
        put(f"{scene}/bake_texel_attributes/weights", w5)
        edge = values.clone()  # values no packing can use, in the first texels: every byte of the NaN texel is 0
        edge[0, 0], edge[0, 1], edge[0, 2], edge[0, 3] = float("nan"), float("inf"), float("-inf"), 1.5
        for srgb in (True, False):
            base, orm = MT.pack_textures(edge, srgb=srgb)
            assert (base[0, 0] == 0).all() and (orm[0, 0, 1:] == 0).all() and orm[0, 0, 0] == 255
            put(f"{scene}/pack_textures/srgb{int(srgb)}/base", base)
            put(f"{scene}/pack_textures/srgb{int(srgb)}/orm", orm)
        base3, none = MT.pack_textures(five[..., :3].contiguous())
        assert none is None
        put(f"{scene}/pack_textures/three/base", base3)
        nmap, tangent = MT.pack_normal_map(atlas, values, return_tangent=True)
        put(f"{scene}/pack_normal_map/bytes", nmap)
        put(f"{scene}/pack_normal_map/tangent", tangent)

        # views
        args = (v, f, m, *K, H, W)
        vn = MVW.vertex_normals(v, f)[0]
        put(f"{scene}/vertex_normals", vn)
        vis = {ss: MVW.visibility_buffer(*args, ss) for ss in (1, 2)}
        for ss in (1, 2):
            put(f"{scene}/visibility/ss{ss}", vis[ss])
        for shading, colors in (("flat", None), ("smooth", att[:, :3].contiguous())):
            for name, t in zip(("rgba", "depth", "tri_id"), MVW.shade_views(*args, ss=2, shading=shading, colors=colors, return_aux=True)):
                put(f"{scene}/shade_views/{shading}/{name}", t)
        put(f"{scene}/shade_views/batched", MVW.shade_views(*args, ss=3, view_batch=2))
        alb, rough, metal = att[:, :3].contiguous(), att[:, 3].contiguous(), att[:, 4].contiguous()
        for ss, normals in ((1, None), (2, vn)):
            g = MVW.mesh_gbuffer(*args, vis[ss].reshape(-1), alb, rough, metal, ss, normals)
            for name in sorted(g):
                put(f"{scene}/mesh_gbuffer/ss{ss}/{name}", g[name])
        th, tw = atlas.height, atlas.width
        tex_base, tex_orm = (_cuda(rng.integers(0, 256, (th, tw, 3), dtype=np.uint8)) for _ in range(2))
        for with_nm in (False, True):
            for with_orm in (False, True):
                g = MVW.mesh_gbuffer_textured(v, f, atlas.uvs, m, *K, H, W, vis[2].reshape(-1), tex_base, tex_orm if with_orm else None,
                                              nmap if with_nm else None, True, 2, vn)
                for name in sorted(g):
                    put(f"{scene}/mesh_gbuffer_textured/nm{int(with_nm)}_orm{int(with_orm)}/{name}", g[name])
        g = MVW.mesh_gbuffer_textured(v, f, atlas.uvs, m, *K, H, W, vis[1].reshape(-1), tex_base, None, nmap, False, 1, None)
        for name in sorted(g):
            put(f"{scene}/mesh_gbuffer_textured/flat_linear/{name}", g[name])
        rgb = _cuda(rng.uniform(-0.1, 1.1, (n, 2 * H, 2 * W, 3)).astype(np.float32))
        cover = MVW.mesh_gbuffer(*args, vis[2].reshape(-1), alb, rough, metal, 2, vn)["coverage"]
        put(f"{scene}/resolve_rgb/plain", MVW.resolve_rgb(rgb, cover, 2, True))
        put(f"{scene}/resolve_rgb/background", MVW.resolve_rgb(rgb, cover, 2, True, _cuda(rng.random((n, H, W, 3)).astype(np.float32))))
        put(f"{scene}/shade_views_textured", MVW.shade_views_textured(v, f, atlas.uvs, m, *K, H, W, tex_base, nmap, True, ss=2, normals=vn))
        put(f"{scene}/shade_views_textured/flat_batched",
            MVW.shade_views_textured(v, f, atlas.uvs, m, *K, H, W, tex_base, None, False, ss=2, view_batch=3))

        # under the small light of test_mesh_bake_gpu.test_shade_views_pbr_against_the_unfused_shading
        light = E.EnvLight((torch.rand((6, 64, 64, 3), generator=torch.Generator().manual_seed(5)) * 1.5).cuda())
        put(f"{scene}/shade_views_pbr/vertex", MVW.shade_views_pbr(*args, light, alb, rough, metal, ss=2, shading="smooth", gamma=True, view_batch=3))
        tex = dict(uvs=atlas.uvs, base_color=tex_base, orm=tex_orm, normal_map=nmap, srgb=True, normals=vn)
        put(f"{scene}/shade_views_pbr/textured", _pbr_textured(args, light, 2, tex))
    return out


def test_same_bytes_as_recorded():
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = digests()
    assert sorted(got) == sorted(want)  # no entry left out, none added
    assert [k for k in sorted(want) if got[k] != want[k]] == []


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_mesh_paths_same_bits_gpu.py --record")
    print(json.dumps(digests(), indent=1, sort_keys=True))
