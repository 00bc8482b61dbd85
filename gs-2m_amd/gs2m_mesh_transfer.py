"""Detail transfer between two meshes of one surface: a high-to-low bake (csrc/mesh_bvh.hip; include/gs2m_meshtransfer.h,
include/gs2m_meshao.h).

The mesh pipeline ends in the full TSDF mesh, which carries the vertex bake's albedo, roughness and metallic, and its simplified
copy, which is what is exported.  `transfer_texels` casts, for every texel of the simplified mesh's atlas, a short ray along the
texel's normal, forth and back, against a hierarchy of the SOURCE mesh (`gs2m_mesh_bvh.build_bvh`, the closest-hit query), and
copies what the source has where the nearer ray meets it: its vertex values, and with `normal=True` its geometric normal, which
`gs2m_mesh_texture.pack_normal_map` turns into the tangent-space normal map of the detail the simplification removed.  Texturing a
simplified mesh this way needs the two PLY files and nothing else: no model, no dataset.  Every ray is traced by the library, on
device tensors owned here; there is no CPU path.

    python gs-2m_amd/gs2m_mesh_transfer.py --mesh LOW.ply --source HIGH.ply -o asset.glb (--texture-size N | --density D) \\
        [--distance X] [--two-sided] [--normal-map] [--flat-normals] [--linear] [--device-png] [--textures-dir DIR] [--ao ...]

A material source (gs2m_mesh_bake.py's PLY) gives base colour, roughness and metallic; any other coloured PLY a base colour
only.  A source's `occlusion` property is NOT carried: it was traced against the source's geometry at its vertices; --ao traces
it anew on the mesh that is exported, at its texels.
"""
import argparse
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np
import torch

import gs2m_native as N
from gs2m_eval_util import ptr as _ptr
from gs2m_mesh_bake import FALLBACK
from gs2m_mesh_bvh import BAND_TEXELS, OWNER_ROWS, Bvh, atlas_normals, bands, build_bvh, checked_rows, live_diagonal, texels, unit_rows
from gs2m_mesh_cull import _mesh_on_device, _on_device

DISTANCE_SHARE = 0.02   # of the diagonal of the target's live vertices' bounding box: how far a ray is followed, each way


def transfer(bvh, points, normals, values, owner=None, distance=0.0, two_sided=False, source_values=None, source_normals=None,
             normal=False):
    """gs2m_mesh_transfer on device tensors.  bvh: the SOURCE mesh's (build_bvh); points, normals (n, 3) float64, the normals unit
    already; values (n, stride) float32, contiguous, written IN PLACE: columns 0 .. C - 1 of a point whose rays met the source get
    source_values (V_src, C) float32 interpolated there, with normal=True columns C .. C + 2 source_normals (V_src, 3) float64
    interpolated, or for None the hit triangle's cross(e1, e2); every other element stays.  owner (n,) int32: negative = no point
    here.  -> (hit (n,) int32: the source triangle or -1; offset (n,) float64: the signed distance along the normal, 0 for a miss)"""
    who = "transfer"
    p, n, ow = checked_rows(who, OWNER_ROWS, points, normals, owner)
    att = None if source_values is None else N.f32(source_values, "source_values", who=who)
    if att is not None and (att.dim() != 2 or len(att) != len(bvh.vertices)):
        raise RuntimeError(f"{who}: `source_values` must have shape ({len(bvh.vertices)}, C), got {tuple(att.shape)}")
    channels = 0 if att is None else int(att.shape[1])
    sn = None if source_normals is None else _on_device(source_normals, "source_normals", who, torch.float64, (3,))
    if sn is not None and len(sn) != len(bvh.vertices):
        raise RuntimeError(f"{who}: {len(sn)} source normals for {len(bvh.vertices)} source vertices")
    if (not torch.is_tensor(values) or values.device != p.device or values.dtype != torch.float32 or not values.is_contiguous()
            or values.dim() != 2 or len(values) != len(p)):
        raise RuntimeError(f"{who}: `values` must be a contiguous ({len(p)}, stride) float32 tensor on {p.device}")
    hit = torch.full((len(p),), -1, dtype=torch.int32, device=p.device)
    offset = torch.zeros(len(p), dtype=torch.float64, device=p.device)
    N.launch("gs2m_mesh_transfer", p.device, *bvh.args(), len(p), _ptr(p), _ptr(n), _ptr(ow), float(distance), int(bool(two_sided)), channels,
             _ptr(att), _ptr(sn), int(bool(normal)), int(values.shape[1]), _ptr(values), _ptr(hit), _ptr(offset))
    return hit, offset


def texel_rays(atlas, vertex_normals=None, row0=0, n_rows=None):
    """Where the transfer's rays start and run, for rows row0 .. row0 + n_rows of the atlas: the texels as points of the low mesh
    and its interpolated vertex normals (gs2m_mesh_bvh.texels), normalised as gs2m_mesh_bvh.unit_rows does
    -> (owner (n, W) int32, points (n, W, 3), normals (n, W, 3) float64)"""
    owner, points, tn = texels(atlas, vertex_normals, row0, n_rows)
    return owner, points, unit_rows(tn.reshape(-1, 3)).reshape(tn.shape).contiguous()


def _fill(atlas, channels, attributes):
    """What a texel bake that saw no view resolves to: owned texels interpolate `attributes` (V, channels), the low mesh's own
    vertex values; without them, and on empty texels, the fallback -> (H, W, channels) float32"""
    from gs2m_mesh_texture import TextureBaker
    fallback = list(FALLBACK[:channels]) if channels in (3, 5) else None
    return TextureBaker(atlas, channels, use_normals=False).finish(fallback=fallback, attributes=attributes)[0]


def transfer_texels(atlas, source_mesh, source_values=None, distance=None, two_sided=False, normal=False, smooth=True, bvh=None,
                    band_texels=BAND_TEXELS, attributes=None):
    """The source mesh's vertex values, and with normal=True its normals, at the texels of `atlas` (gs2m_mesh_texture.build_atlas
    of the LOW mesh).  source_mesh: anything with .vertices and .triangles; source_values (V_src, C) float32 or None (C = 0);
    distance: how far each of a texel's two rays is followed, default 0.02 of the diagonal of the low mesh's live vertices' box
    (a parameter's default, not a tolerance); two_sided: also accept source triangles that face away from the texel's normal;
    smooth: interpolate the source's vertex normals (gs2m_mesh_view.vertex_normals), else the hit triangle's face normal, in
    neither case normalised; bvh: build_bvh of the source, where the caller has it.  The C value planes start as a texel bake
    without a view resolves them -- `attributes` (V_low, C), the low mesh's own vertex values, interpolated, else the fallback --
    and the three normal planes start at zero, which pack_normal_map encodes flat: a texel whose rays find nothing keeps those.
    The atlas goes through the library in bands of whole rows; the result does not depend on the band.
    -> (values (H, W, C [+ 3]) float32, hit (H, W) int32: the source triangle or -1, offset (H, W) float64)"""
    who = "transfer_texels"
    a = atlas
    dev = a.vertices.device
    if bvh is None:
        bvh = build_bvh(*_mesh_on_device(source_mesh, dev, who))
    elif not isinstance(bvh, Bvh):
        raise RuntimeError(f"{who}: `bvh` must be build_bvh's of the source mesh")
    att = None if source_values is None else N.f32(torch.as_tensor(source_values).to(dev), "source_values", who=who)
    channels = 0 if att is None else int(att.shape[-1])
    if channels == 0 and not normal:
        raise RuntimeError(f"{who}: nothing to transfer: no `source_values` and normal=False")
    distance = DISTANCE_SHARE * live_diagonal(a.vertices, a.triangles) if distance is None else float(distance)
    sn = None
    if normal and smooth and len(bvh.triangles):
        from gs2m_mesh_view import vertex_normals
        sn = vertex_normals(bvh.vertices, bvh.triangles)[0]
    planes = []
    if channels:
        low = None if attributes is None else N.f32(torch.as_tensor(attributes).to(dev), "attributes", (len(a.vertices), channels), who=who)
        planes.append(_fill(a, channels, low))
    if normal:
        planes.append(torch.zeros((a.height, a.width, 3), dtype=torch.float32, device=dev))
    values = torch.cat(planes, 2).contiguous()
    hit = torch.full((a.height, a.width), -1, dtype=torch.int32, device=dev)
    offset = torch.zeros((a.height, a.width), dtype=torch.float64, device=dev)
    vn = atlas_normals(a)
    for row0, n in bands(a, band_texels):
        owner, points, normals = texel_rays(a, vn, row0, n)
        band = values[row0:row0 + n].reshape(n * a.width, -1)            # a view: whole rows of a contiguous tensor
        h, o = transfer(bvh, points.reshape(-1, 3), normals.reshape(-1, 3), band, owner.reshape(-1), distance, two_sided, att, sn, normal)
        hit[row0:row0 + n], offset[row0:row0 + n] = h.reshape(n, a.width), o.reshape(n, a.width)
    return values, hit, offset


# ---- command line ------------------------------------------------------------------------------------------------------------

def parser():
    ap = argparse.ArgumentParser(description="Texture a simplified mesh from the full mesh it came from and write a glTF 2.0 binary: "
                                 "a high-to-low bake of vertex colours, materials and the normal map, with no model and no dataset")
    ap.add_argument("--mesh", required=True, help="the LOW mesh that is textured and exported (binary PLY), e.g. tsdf_simplified.ply")
    ap.add_argument("--source", required=True, help="the HIGH mesh whose detail is transferred (binary PLY): a material mesh "
                    "(gs2m_mesh_bake.py's) gives base colour, roughness and metallic, any other coloured PLY a base colour only; "
                    "an `occlusion` property is not carried (see --ao)")
    ap.add_argument("--output", "-o", required=True, help="the .glb to write")
    size = ap.add_mutually_exclusive_group(required=True)
    size.add_argument("--texture-size", type=int, metavar="N", help="the atlas is at most N texels wide (the densest rung that fits)")
    size.add_argument("--density", type=float, metavar="D", help="texels per world unit")
    ap.add_argument("--distance", type=float, default=None, metavar="X",
                    help=f"how far a texel's rays are followed along its normal, each way (default: {DISTANCE_SHARE} of the low mesh's "
                    "bounding-box diagonal)")
    ap.add_argument("--two-sided", action="store_true", help="also accept source triangles that face away from the texel's normal")
    ap.add_argument("--normal-map", action="store_true",
                    help="also transfer the source's normals into a tangent-space normal map: TANGENT and normalTexture in the .glb")
    ap.add_argument("--flat-normals", action="store_true", help="with --normal-map: the source's face normals, not its smooth vertex normals")
    ap.add_argument("--linear", action="store_true", help="store the base colour without the sRGB transfer")
    ap.add_argument("--textures-dir", default=None, metavar="DIR",
                    help="also write base_color.png and metallic_roughness.png (with --normal-map: normal.png) there")
    from gs2m_mesh_bake import add_ao_arguments
    add_ao_arguments(ap, "traced on the LOW mesh at its texels, into the R channel of the ORM image and an occlusionTexture in the .glb "
                     "(a source without materials: an ORM image of roughness 1, metallic 0)")
    from gs2m_png import add_png_argument
    add_png_argument(ap)
    return ap


def _vertex_values(mesh, values, channels):
    """What a mesh read by read_source_mesh carries per vertex, as (V, channels) float32 numpy with channels 5 (albedo rgb,
    roughness, metallic) or 3; a mesh with colours alone gets roughness 1 and metallic 0; None for one without colours"""
    if values is None:
        colours = getattr(mesh, "vertex_colors", None)
        if colours is None or len(colours) != len(mesh.vertices):
            return None
        c = np.asarray(colours, np.float32).reshape(-1, 3)
        values = np.concatenate([c, np.broadcast_to(np.asarray(FALLBACK[3:], np.float32), (len(c), 2))], 1)
    return np.ascontiguousarray(np.asarray(values, np.float32)[:, :channels])


def transfer_mesh(mesh, source, output, source_values=None, vertex_values=None, density=None, texture_size=None, distance=None,
                  two_sided=False, normal_map=False, flat_normals=False, linear=False, device_png=False, textures_dir=None, ao=False,
                  ao_rays=64, ao_radius=None, device="cuda"):
    """Atlas of `mesh`, transfer from `source`, pack and export in one call.  source_values (V_src, 5) for a material source, None
    for the source's vertex colours (a base colour only); vertex_values: the same of the low mesh, which texels without a hit
    keep.  -> dict(out, width, height, density, distance, n_texels, n_owned, n_hit, hit_share, max_offset)"""
    from gs2m_mesh_texture import build_atlas, export_glb, pack_normal_map, pack_textures
    channels = 5 if source_values is not None else 3
    src = _vertex_values(source, source_values, channels)
    if src is None:
        raise RuntimeError("transfer_mesh: the source mesh has neither materials nor vertex colours: nothing to transfer")
    atlas = build_atlas(mesh, density=density, texture_size=texture_size, device=device)
    values, hit, offset = transfer_texels(atlas, source, src, distance=distance, two_sided=two_sided, normal=normal_map,
                                          smooth=not flat_normals, attributes=_vertex_values(mesh, vertex_values, channels))
    base, orm = pack_textures(values, srgb=not linear)
    extra = {"normal_map": pack_normal_map(atlas, values)} if normal_map else {}
    if ao:
        from gs2m_mesh_ao import apply_occlusion, texel_occlusion
        if orm is None:
            orm = torch.tensor([255, 255, 0], dtype=torch.uint8, device=base.device).repeat(atlas.height, atlas.width, 1).contiguous()
        visible, owner = texel_occlusion(atlas, rays=ao_rays, radius=ao_radius)
        apply_occlusion(orm, owner, visible, ao_rays)
        extra["occlusion"] = True
    export_glb(output, atlas, base, orm, device_png=device_png, textures_dir=textures_dir, **extra)
    owned = texel_rays(atlas)[0] >= 0
    n_owned, n_hit = int(owned.sum()), int((hit >= 0).sum())
    share = n_hit / n_owned if n_owned else 0.0
    max_offset = float(offset.abs().max()) if offset.numel() else 0.0
    used = DISTANCE_SHARE * live_diagonal(atlas.vertices, atlas.triangles) if distance is None else float(distance)
    print(f"[>] atlas {atlas.width} x {atlas.height} at {atlas.density:.6g} texels per unit: {n_hit} of {n_owned} owned texels "
          f"({100.0 * share:.2f} %) met the source within {used:.6g}, largest |offset| {max_offset:.6g} -> {output}")
    return {"out": str(output), "width": atlas.width, "height": atlas.height, "density": atlas.density, "distance": used,
            "n_texels": atlas.width * atlas.height, "n_owned": n_owned, "n_hit": n_hit, "hit_share": share, "max_offset": max_offset}


def main(argv=None):
    a = parser().parse_args(argv)
    from gs2m_mesh_texture import read_source_mesh
    mesh, vertex_values = read_source_mesh(a.mesh)
    source, source_values = read_source_mesh(a.source)
    return transfer_mesh(mesh, source, a.output, source_values=source_values, vertex_values=vertex_values, density=a.density,
                         texture_size=a.texture_size, distance=a.distance, two_sided=a.two_sided, normal_map=a.normal_map,
                         flat_normals=a.flat_normals, linear=a.linear, device_png=a.device_png, textures_dir=a.textures_dir,
                         **({"ao": True, "ao_rays": a.ao_rays, "ao_radius": a.ao_radius} if a.ao else {}))


if __name__ == "__main__":
    main()
