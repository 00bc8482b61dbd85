"""Textured mesh export: a triangle atlas, the per-view maps of a trained model baked into its texels, and a glTF 2.0 binary
(csrc/mesh_atlas.hip, csrc/mesh_bake.hip; include/gs2m_atlas.h, include/gs2m_meshbake.h).

Every triangle gets a right-isosceles chart of its own in a power-of-two cell; the layout is a function of the mesh and of one
number, the density in texels per world unit (`build_atlas`; `texture_size` picks the density from a target width).  Every texel
is a point of its triangle; the views are averaged onto the texels exactly as gs2m_mesh_bake.py averages them onto vertices
(`TextureBaker`, `bake_textures`), packed into a base-colour and an occlusion-roughness-metallic image (`pack_textures`) and
written with the unwelded mesh as one .glb (`export_glb`, `write_glb`; `read_glb` reads it back).  Everything up to the PNG
files runs on device tensors owned here; there is no CPU path.

    python gs-2m_amd/gs2m_mesh_texture.py --ply point_cloud.ply -s SCENE --mesh tsdf_simplified.ply -o asset.glb \\
        (--texture-size N | --density D) [--metallic] [--rgb] [--linear] [--normal-map | --normal-map-from SOURCE.ply] [--device-png]
        [--textures-dir DIR]

With --normal-map the views' world-space normals are baked beside the materials and encoded per texel in the tangent frame of its
triangle (`pack_normal_map`; csrc/tangent_frame.h): the .glb then carries a TANGENT accessor and a normalTexture.
With --normal-map-from the colours are still baked from the views, but the normal map's three planes are the geometry of
SOURCE.ply -- the full mesh this one was simplified from -- found by a ray along each texel's normal
(gs2m_mesh_transfer.transfer_texels).
"""
import argparse
import ctypes as C
import io
import json
import os
import struct
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np
import torch

import gs2m_native as N
from gs2m_eval_util import ptr as _ptr
from gs2m_eval_util import workspace_for
from gs2m_mesh_bake import FALLBACK, MAX_CHANNELS, MIN_WEIGHT, _Bake, bake_runs, bake_slices
from gs2m_mesh_cull import EPS, FAR, NEAR, VIEW_BATCH, _mesh_on_device, _on_device

CLASSES = 6
MAX_WIDTH = 16384
LADDER = 4            # rungs per doubling of the density
MAX_RUNGS = 4 * 40
BASE_TRIANGLES = 4096


class Atlas:
    """The layout of one mesh: width, height, density, hist and bases (lists of 6), and the device tensors vertices (V, 3)
    float64, triangles (F, 3) int32, cells (F, 4) int32 = origin x, y, side, half, uvs (F, 3, 2) float32, order (F,) int32."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def atlas_count(vertices, triangles, density):
    """-> (hist [6], width, height) of the atlas at `density`, without building it.  RuntimeError ("unsupported size") beyond
    a width of 16384."""
    v = _on_device(vertices, "vertices", "atlas_count", torch.float64, (3,))
    f = _on_device(triangles, "triangles", "atlas_count", torch.int32, (3,))
    ws = workspace_for("gs2m_atlas_workspace_bytes", v.device, len(f))
    hist, dims = (C.c_longlong * CLASSES)(), (C.c_int * 2)()
    N.launch("gs2m_atlas_count", v.device, len(v), len(f), _ptr(v), _ptr(f), float(density), _ptr(ws), hist, dims)
    return list(hist), int(dims[0]), int(dims[1])


def base_density(vertices, triangles):
    """One texel per shortest non-degenerate edge of the first 4096 triangles: the ladder's rung 0."""
    f = triangles[:BASE_TRIANGLES].long()
    if len(f) == 0:
        return 1.0
    p = vertices[f]
    e = torch.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 1], p[:, 0] - p[:, 2]], 1).norm(dim=2).reshape(-1)
    e = e[(e > 0) & torch.isfinite(e)]
    return 1.0 / float(e.min()) if len(e) else 1.0


def target_density(vertices, triangles, texture_size):
    """The density of the ladder base * 2^(k / 4) (base: base_density) that bisection with gs2m_atlas_count finds: the last rung
    whose atlas is at most `texture_size` wide; the next rung's is wider.  -> (density, k)"""
    base, n = base_density(vertices, triangles), int(texture_size)
    if n < 8:
        raise RuntimeError(f"build_atlas: a texture of width {n} holds no cell; 8 at least")

    def fits(k):
        try:
            return atlas_count(vertices, triangles, base * 2.0 ** (k / LADDER))[1] <= n
        except RuntimeError as e:
            if "unsupported size" in str(e):
                return False
            raise

    lo = 0
    while not fits(lo):  # down to a rung that fits
        lo -= LADDER
        if lo < -MAX_RUNGS:
            raise RuntimeError(f"build_atlas: the mesh does not fit a texture of width {n} at any density")
    hi = lo + LADDER
    while fits(hi):      # up to one that does not
        lo, hi = hi, hi + LADDER
        if hi > MAX_RUNGS:
            raise RuntimeError(f"build_atlas: no density up to base * 2^{MAX_RUNGS // LADDER} fills a texture of width {n}")
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return base * 2.0 ** (lo / LADDER), lo


def build_atlas(mesh, density=None, texture_size=None, device="cuda"):
    """The atlas of `mesh` (anything with .vertices and .triangles) at `density` texels per world unit, or at the density
    `target_density` finds for a texture at most `texture_size` wide (one of the two).  -> Atlas"""
    who = "build_atlas"
    if (density is None) == (texture_size is None):
        raise ValueError(f"{who}: give one of `density` and `texture_size`")
    v, f = _mesh_on_device(mesh, device, who)
    rung = None
    if density is None:
        density, rung = target_density(v, f, texture_size)
    dev, F = v.device, len(f)
    ws = workspace_for("gs2m_atlas_workspace_bytes", dev, F)
    cells = torch.empty((F, 4), dtype=torch.int32, device=dev)
    uvs = torch.empty((F, 3, 2), dtype=torch.float32, device=dev)
    order = torch.empty(F, dtype=torch.int32, device=dev)
    hist, bases, dims = (C.c_longlong * CLASSES)(), (C.c_longlong * CLASSES)(), (C.c_int * 2)()
    N.launch("gs2m_atlas_build", dev, len(v), F, _ptr(v), _ptr(f), float(density), _ptr(ws), _ptr(cells), _ptr(uvs), _ptr(order), hist, bases,
             dims)
    return Atlas(vertices=v, triangles=f, density=float(density), rung=rung, width=int(dims[0]), height=int(dims[1]), hist=list(hist),
                 bases=list(bases), cells=cells, uvs=uvs, order=order)


def atlas_texels(atlas, normals=None, row0=0, n_rows=None):
    """Rows row0 .. row0 + n_rows of the atlas as points of the surface -> (owner (n, W) int32, -1 where empty; interior (n, W)
    bool; points (n, W, 3) float64; normals (n, W, 3) float64).  normals: the (V, 3) vertex normals, or None for face normals."""
    a = atlas
    dev = a.vertices.device
    n = a.height - row0 if n_rows is None else int(n_rows)
    owner = torch.empty((n, a.width), dtype=torch.int32, device=dev)
    interior = torch.empty((n, a.width), dtype=torch.uint8, device=dev)
    points = torch.empty((n, a.width, 3), dtype=torch.float64, device=dev)
    tn = torch.empty((n, a.width, 3), dtype=torch.float64, device=dev)
    nrm = None if normals is None else _on_device(normals, "normals", "atlas_texels", torch.float64, (3,))
    N.launch("gs2m_atlas_texels", dev, len(a.vertices), _ptr(a.vertices), _ptr(nrm), len(a.triangles), _ptr(a.triangles), _ptr(a.order),
             (C.c_longlong * CLASSES)(*a.hist), a.width, a.height, int(row0), n, _ptr(owner), _ptr(interior), _ptr(points), _ptr(tn))
    return owner, interior.bool(), points, tn


class TextureBaker(_Bake):
    """The running sums of a texel bake: `add` takes a batch of views with their maps, `finish` resolves -- gs2m_mesh_bake.Baker
    with the atlas's texels in the place of the vertices.  The views may come in any grouping; the result depends only on their
    order."""
    who, entry = "TextureBaker", "gs2m_texbake_accumulate"

    def __init__(self, atlas, channels, eps=EPS, use_normals=True, near=NEAR, far=FAR):
        super().__init__(atlas.vertices, atlas.triangles, atlas.width * atlas.height, channels, eps, near, far)
        self.atlas, self.use_normals = atlas, bool(use_normals)
        vn = None
        if use_normals and len(atlas.triangles):
            from gs2m_mesh_view import vertex_normals
            vn = vertex_normals(atlas.vertices, atlas.triangles)[0]
        self.owner, self.interior, self.points, self.normals = atlas_texels(atlas, vn)

    def _points(self):
        return _ptr(self.points), _ptr(self.normals) if self.use_normals else None, _ptr(self.owner)

    def finish(self, min_weight=MIN_WEIGHT, fallback=None, attributes=None):
        """attributes: (V, C) float32 per-vertex values that owned texels no view reached interpolate, or None for the fallback.
        -> (values (H, W, C) float32, seen (H, W) bool, weights (H, W) float64)"""
        a = self.atlas
        att = None
        if attributes is not None:
            att = N.f32(attributes, "attributes", (len(a.vertices), self.channels), who="TextureBaker.finish")
        return self._resolve("gs2m_texbake_resolve", (a.height, a.width), min_weight, fallback, (max(a.width, 1), 0),
                             (_ptr(self.owner), len(a.triangles), _ptr(a.triangles), _ptr(a.cells), len(a.vertices), _ptr(att))
                             ) + (self.weights.reshape(a.height, a.width),)


def bake_texel_attributes(atlas, w2c, fx, fy, cx, cy, maps, mask=None, eps=EPS, use_normals=True, view_batch=None, min_weight=MIN_WEIGHT,
                          fallback=None, attributes=None, near=NEAR, far=FAR):
    """Per-texel averages of the views' attribute maps: gs2m_mesh_bake.bake_vertex_attributes for the texels of `atlas`.  The
    result does not depend on `view_batch`, bit for bit.  -> (values (H, W, C) float32, seen (H, W) bool, weights (H, W) float64)"""
    new = lambda channels: TextureBaker(atlas, channels, eps, use_normals, near, far)
    return bake_slices("bake_texel_attributes", new, w2c, fx, fy, cx, cy, maps, mask, view_batch).finish(min_weight, fallback, attributes)


def rgb_maps(gaussians, view, normal=False):
    """One view's plain render and its foreground (alpha >= 0.5) -> (maps (3, H, W) float32, mask (H, W) float32); normal: three
    more planes, gs2m_mesh_bake.unit_normal_planes of the render's normal_map"""
    from gaussian_renderer import render
    from gs2m_scene import PipelineParams
    dev = gaussians.get_xyz.device
    with torch.no_grad():
        pkg = render(view, gaussians, PipelineParams(), torch.zeros(3, device=dev))
        rgb = pkg["render"].clamp(0.0, 1.0).to(torch.float32)
        if normal:
            from gs2m_mesh_bake import unit_normal_planes
            rgb = torch.cat([rgb, unit_normal_planes(pkg["normal_map"])])
        return rgb.contiguous(), (pkg["alpha_map"].reshape(rgb.shape[-2:]) >= 0.5).to(torch.float32)


def bake_textures(gaussians, views, mesh, atlas, metallic=False, rgb=False, eps=EPS, use_normals=True, view_batch=None,
                  min_weight=MIN_WEIGHT, fallback=None, attributes=None, near=NEAR, far=FAR, normal_map=False):
    """The model's albedo, roughness and metallic (gs2m_mesh_bake.material_maps), or with rgb=True its plain render, in the texels
    of `atlas` (build_atlas(mesh, ...)).  Views are baked in runs of up to `view_batch` that share size and intrinsics, with the
    principal-point shift of gs2m_mesh_bake.bake_runs.  Texels no view reached take `attributes` (V, C) interpolated, else `fallback`.
    normal_map: three more planes, the views' unit world-space normals averaged like the others (for pack_normal_map; the mean is
    not unit); `attributes` and `fallback` keep their 5 or 3 columns and are padded with zeros there, so that a texel no view
    reached carries a zero normal and encodes flat.
    -> (values (H, W, 5 or 3, + 3 with normal_map) float32, seen (H, W) bool, weights (H, W) float64)"""
    from gs2m_mesh_bake import material_maps
    materials = 3 if rgb else 5
    channels = materials + (3 if normal_map else 0)
    fallback = list(FALLBACK[:materials] if fallback is None else fallback)
    if normal_map:
        fallback = fallback + [0.0, 0.0, 0.0]
        if attributes is not None:
            att = N.f32(attributes, "attributes", (len(atlas.vertices), materials), who="bake_textures")
            attributes = torch.cat([att, torch.zeros((len(att), 3), dtype=torch.float32, device=att.device)], 1).contiguous()
    baker = TextureBaker(atlas, channels, eps, use_normals, near, far)
    maps_of = lambda view: rgb_maps(gaussians, view, normal_map) if rgb else material_maps(gaussians, view, metallic, normal_map)
    bake_runs(baker, views, maps_of, view_batch)
    return baker.finish(min_weight, fallback, attributes)


def pack_textures(values, srgb=True):
    """values (H, W, 5) or (H, W, 3) float32 -> (base colour (H, W, 3) uint8, sRGB-encoded unless srgb=False; ORM (H, W, 3) uint8:
    255, roughness, metallic -- None for three channels).  The three normal planes of a bake with normal_map=True (6 or 8 channels)
    are left to pack_normal_map."""
    x = N.f32(values, "values", who="pack_textures")
    if x.dim() == 3 and x.shape[2] in (6, 8):  # a bake with normal planes: they are pack_normal_map's
        x = x[..., :x.shape[2] - 3].contiguous()
    if x.dim() != 3 or x.shape[2] not in (3, 5):
        raise RuntimeError(f"pack_textures: `values` must have shape (H, W, 3) or (H, W, 5), got {tuple(x.shape)}")
    H, W, ch = x.shape
    base = torch.empty((H, W, 3), dtype=torch.uint8, device=x.device)
    orm = torch.empty((H, W, 3), dtype=torch.uint8, device=x.device) if ch == 5 else None
    N.launch("gs2m_texture_pack", x.device, H * W, ch, _ptr(x), int(bool(srgb)), _ptr(base), _ptr(orm))
    return base, orm


def texel_normals(atlas):
    """The texels' interpolated normals as the bake sees them (TextureBaker with use_normals) -> (owner (H, W) int32, normals
    (H, W, 3) float64)"""
    vn = None
    if len(atlas.triangles):
        from gs2m_mesh_view import vertex_normals
        vn = vertex_normals(atlas.vertices, atlas.triangles)[0]
    owner, _, _, tn = atlas_texels(atlas, vn)
    return owner, tn


def pack_normal_map(atlas, values, offset=None, return_tangent=False):
    """values (H, W, C) float32 of a bake of `atlas` whose planes offset .. offset + 2 (default: the last three) hold the baked
    world-space normal -> the tangent-space normal map (H, W, 3) uint8 (include/gs2m_meshbake.h, the Normals paragraph: each
    texel's frame is built at its interpolated vertex normal); return_tangent: also the (H, W, 3) float64 values before packing."""
    who = "pack_normal_map"
    x = N.f32(values, "values", who=who)
    if x.dim() != 3 or not 3 <= x.shape[2] <= MAX_CHANNELS or tuple(x.shape[:2]) != (atlas.height, atlas.width):
        raise RuntimeError(f"{who}: `values` must have shape ({atlas.height}, {atlas.width}, 3 .. {MAX_CHANNELS}), got {tuple(x.shape)}")
    ch = int(x.shape[2])
    offset = ch - 3 if offset is None else int(offset)
    owner, tn = texel_normals(atlas)
    dev = x.device
    out = torch.empty((atlas.height, atlas.width, 3), dtype=torch.uint8, device=dev)
    tangent = torch.empty((atlas.height, atlas.width, 3), dtype=torch.float64, device=dev) if return_tangent else None
    N.launch("gs2m_texture_normals", dev, atlas.height * atlas.width, _ptr(owner), _ptr(tn), len(atlas.triangles), _ptr(atlas.triangles),
             _ptr(atlas.uvs), len(atlas.vertices), _ptr(atlas.vertices), ch, offset, _ptr(x), _ptr(out), _ptr(tangent))
    return (out, tangent) if return_tangent else out


# ---- glTF 2.0 binary -------------------------------------------------------------------------------------------------------

GLB_MAGIC, GLB_JSON, GLB_BIN = 0x46546C67, 0x4E4F534A, 0x004E4942
_FLOAT, _UINT, _ARRAY_BUFFER, _ELEMENT_BUFFER = 5126, 5125, 34962, 34963


def _pad(b, fill):
    return b + fill * (-len(b) % 4)


def write_glb(file, positions, normals, uvs, indices, images, tangents=None, normal_image=None, occlusion=False):
    """One mesh, one primitive: positions, normals (n, 3) and uvs (n, 2) float32, indices (m,) uint32, images = the PNG files
    (bytes) of the base-colour texture and, optionally, of the metallic-roughness texture, embedded as buffer views.  Buffer
    views and chunks are aligned to 4 bytes; POSITION carries min / max.  tangents (n, 4) float32 and normal_image (a PNG file),
    both or neither: the TANGENT accessor (xyz and the handedness w) and the material's normalTexture; they come after everything
    else in the buffer, and without them the file is byte for byte what it was before they existed.  occlusion: the second
    image's R channel is the ambient occlusion: the material's occlusionTexture names the texture of the
    metallicRoughnessTexture, glTF's ORM packing (two images then); without it, again, the bytes of before.
    -> the bytes written."""
    pos = np.ascontiguousarray(positions, "<f4").reshape(-1, 3)
    nrm = np.ascontiguousarray(normals, "<f4").reshape(-1, 3)
    uv = np.ascontiguousarray(uvs, "<f4").reshape(-1, 2)
    idx = np.ascontiguousarray(indices, "<u4").reshape(-1)
    images = [bytes(b) for b in images]
    if not (len(pos) == len(nrm) == len(uv)) or len(pos) == 0 or len(idx) == 0 or len(idx) % 3 or not 1 <= len(images) <= 2:
        raise ValueError("write_glb: n positions, normals and uvs (n > 0), 3 m indices and one or two images")
    if int(idx.max()) >= len(pos):
        raise ValueError("write_glb: an index names no vertex")
    if (tangents is None) != (normal_image is None):
        raise ValueError("write_glb: `tangents` and `normal_image` come together")
    if occlusion and len(images) != 2:
        raise ValueError("write_glb: the occlusion is the R channel of the second image")
    blobs = [pos.tobytes(), nrm.tobytes(), uv.tobytes(), idx.tobytes()] + images
    if tangents is not None:
        tan = np.ascontiguousarray(tangents, "<f4").reshape(-1, 4)
        if len(tan) != len(pos):
            raise ValueError("write_glb: one tangent per vertex")
        blobs += [tan.tobytes(), bytes(normal_image)]
    views, body = [], b""
    for k, b in enumerate(blobs):
        view = {"buffer": 0, "byteOffset": len(body), "byteLength": len(b)}
        if k < 4 or (tangents is not None and k == len(blobs) - 2):
            view["target"] = _ELEMENT_BUFFER if k == 3 else _ARRAY_BUFFER
        views.append(view)
        body = _pad(body + b, b"\0")
    accessors = [
        {"bufferView": 0, "componentType": _FLOAT, "count": len(pos), "type": "VEC3", "min": [float(x) for x in pos.min(0)],
         "max": [float(x) for x in pos.max(0)]},
        {"bufferView": 1, "componentType": _FLOAT, "count": len(nrm), "type": "VEC3"},
        {"bufferView": 2, "componentType": _FLOAT, "count": len(uv), "type": "VEC2"},
        {"bufferView": 3, "componentType": _UINT, "count": len(idx), "type": "SCALAR"},
    ]
    pbr = {"baseColorTexture": {"index": 0}, "metallicFactor": 1.0 if len(images) == 2 else 0.0, "roughnessFactor": 1.0}
    if len(images) == 2:
        pbr["metallicRoughnessTexture"] = {"index": 1}
    doc = {
        "asset": {"version": "2.0", "generator": "gs2m_mesh_texture"},
        "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [{"mesh": 0}],
        "meshes": [{"primitives": [{"attributes": {"POSITION": 0, "NORMAL": 1, "TEXCOORD_0": 2}, "indices": 3, "material": 0, "mode": 4}]}],
        "materials": [{"pbrMetallicRoughness": pbr}],
        "textures": [{"sampler": 0, "source": k} for k in range(len(images))],
        "samplers": [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}],  # linear, clamp to edge: level 0 only
        "images": [{"bufferView": 4 + k, "mimeType": "image/png"} for k in range(len(images))],
        "accessors": accessors, "bufferViews": views, "buffers": [{"byteLength": len(body)}],
    }
    if occlusion:
        doc["materials"][0]["occlusionTexture"] = {"index": 1}
    if tangents is not None:
        n = len(images)
        accessors.append({"bufferView": 4 + n, "componentType": _FLOAT, "count": len(tan), "type": "VEC4"})
        doc["meshes"][0]["primitives"][0]["attributes"]["TANGENT"] = 4
        doc["materials"][0]["normalTexture"] = {"index": n}
        doc["textures"].append({"sampler": 0, "source": n})
        doc["images"].append({"bufferView": 5 + n, "mimeType": "image/png"})
    text = _pad(json.dumps(doc, separators=(",", ":")).encode("utf-8"), b" ")
    total = 12 + 8 + len(text) + 8 + len(body)
    data = struct.pack("<III", GLB_MAGIC, 2, total) + struct.pack("<II", len(text), GLB_JSON) + text + struct.pack("<II", len(body), GLB_BIN) + body
    with open(str(file), "wb") as f:
        f.write(data)
    return data


def read_glb(file):
    """What write_glb wrote -> dict(positions, normals (n, 3) float32, uvs (n, 2) float32, indices (m,) uint32, images: list of
    PNG files as bytes -- the base colour and, where the material has one, the metallic-roughness texture --, tangents (n, 4)
    float32 or None, normal_image: the normal map's PNG file or None, occlusion: whether the material has an occlusionTexture
    (the R channel of images[1]), json: the document).  ValueError for anything but a version-2 .glb of one mesh with one primitive."""
    with open(str(file), "rb") as f:
        data = f.read()
    if len(data) < 20 or struct.unpack_from("<III", data, 0)[:2] != (GLB_MAGIC, 2) or struct.unpack_from("<I", data, 8)[0] != len(data):
        raise ValueError(f"{file}: not a glTF 2.0 binary")
    n, kind = struct.unpack_from("<II", data, 12)
    if kind != GLB_JSON or 20 + n + 8 > len(data):
        raise ValueError(f"{file}: the first chunk is not JSON")
    doc = json.loads(data[20:20 + n].decode("utf-8"))
    m, kind = struct.unpack_from("<II", data, 20 + n)
    if kind != GLB_BIN or 28 + n + m != len(data):
        raise ValueError(f"{file}: the second chunk is not the binary buffer")
    body = data[28 + n:]
    if len(doc.get("meshes", ())) != 1 or len(doc["meshes"][0]["primitives"]) != 1:
        raise ValueError(f"{file}: one mesh with one primitive is read")

    def view(k):
        v = doc["bufferViews"][k]
        return body[v.get("byteOffset", 0):v.get("byteOffset", 0) + v["byteLength"]]

    def accessor(k, dtype, cols):
        a = doc["accessors"][k]
        if a["componentType"] != {"<f4": _FLOAT, "<u4": _UINT}[dtype] or a["type"] != {1: "SCALAR", 2: "VEC2", 3: "VEC3", 4: "VEC4"}[cols]:
            raise ValueError(f"{file}: accessor {k} is not what write_glb writes")
        x = np.frombuffer(view(a["bufferView"]), dtype, a["count"] * cols, a.get("byteOffset", 0))
        return x.reshape(-1, cols) if cols > 1 else x

    prim = doc["meshes"][0]["primitives"][0]
    att = prim["attributes"]
    images = [view(i["bufferView"]) for i in doc.get("images", ())]
    normal_image = None
    material = doc.get("materials", [{}])[prim.get("material", 0)]
    if "normalTexture" in material:
        source = doc["textures"][material["normalTexture"]["index"]]["source"]
        normal_image = images[source]
        images = [b for k, b in enumerate(images) if k != source]
    return dict(positions=accessor(att["POSITION"], "<f4", 3), normals=accessor(att["NORMAL"], "<f4", 3), uvs=accessor(att["TEXCOORD_0"], "<f4", 2),
                indices=accessor(prim["indices"], "<u4", 1), images=images, tangents=accessor(att["TANGENT"], "<f4", 4) if "TANGENT" in att else None,
                normal_image=normal_image, occlusion="occlusionTexture" in material, json=doc)


def decode_png(data):
    """PNG bytes -> (H, W, CH) uint8, through Pillow"""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as img:
        return np.asarray(img).copy()


def encode_png(images, device_png=False):
    """(H, W, 3) uint8 device tensors -> PNG files as bytes: gs2m_png on the device, else Pillow"""
    if device_png:
        import gs2m_png
        return gs2m_png.encode(list(images))
    from PIL import Image
    out = []
    for t in images:
        buf = io.BytesIO()
        Image.fromarray(t.cpu().numpy()).save(buf, format="PNG")
        out.append(buf.getvalue())
    return out


def _corner_normals(atlas):
    """-> (p (F, 3, 3) the corners, n (F, 3, 3) their unit normals as `unwelded` documents them), float64 device tensors"""
    from gs2m_mesh_view import vertex_normals
    f = atlas.triangles.long()
    p = atlas.vertices[f]                                  # (F, 3, 3)
    vn = vertex_normals(atlas.vertices, atlas.triangles)[0][f]
    face = torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])[:, None].expand(-1, 3, -1)
    n = torch.where((vn != 0).any(2, keepdim=True) & torch.isfinite(vn).all(2, keepdim=True), vn, face)
    length = n.norm(dim=2, keepdim=True)
    n = torch.where((length > 0) & torch.isfinite(length), n / length, torch.tensor([0.0, 0.0, 1.0], dtype=n.dtype, device=n.device))
    return p, n


def unwelded(atlas):
    """The primitive of the export: 3 F vertices, each triangle with corners of its own -> (positions (3F, 3) float32, unit normals
    (3F, 3) float32: the smooth vertex normals, the face normal where there is none, +z for a zero-area triangle; uvs (3F, 2)
    float32; indices (3F,) uint32), numpy."""
    p, n = _corner_normals(atlas)
    return (p.reshape(-1, 3).float().cpu().numpy(), n.reshape(-1, 3).float().cpu().numpy(), atlas.uvs.reshape(-1, 2).cpu().numpy(),
            np.arange(3 * len(p), dtype=np.uint32))


def unwelded_tangents(atlas):
    """The TANGENT accessor of `unwelded`'s vertices: per corner the T of the Tangent frame paragraph (include/gs2m_meshbake.h)
    of its triangle at that corner's own normal, and the handedness w = -1 -> (3F, 4) float32 numpy.  A corner without a frame (a
    zero-area triangle) gets (1, 0, 0, -1).  The frame replaces a normal that opposes its face by the face's: there T is
    perpendicular to the face normal, not to the NORMAL accessor's."""
    p, n = _corner_normals(atlas)
    uv = atlas.uvs.to(torch.float64)
    dot = lambda a, b: ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2])[..., None]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    d1, d2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
    det = (d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1])[:, None]
    du = ((e1 * d2[:, 1:2] - e2 * d1[:, 1:2]) / det)[:, None]            # (F, 1, 3)
    nf = torch.linalg.cross(e1, e2)
    uf = (nf / dot(nf, nf).sqrt())[:, None]
    n = torch.where(dot(n, nf[:, None]) > 0, n, uf.expand(-1, 3, -1))
    t = du - n * dot(n, du)
    t = t / dot(t, t).sqrt()
    ok = torch.isfinite(t).all(2, keepdim=True) & (det != 0)[:, None]
    t = torch.where(ok, t, torch.tensor([1.0, 0.0, 0.0], dtype=t.dtype, device=t.device))
    out = torch.cat([t, torch.full_like(t[..., :1], -1.0)], 2)
    return out.reshape(-1, 4).float().cpu().numpy()


def export_glb(file, atlas, base_color, orm=None, device_png=False, textures_dir=None, normal_map=None, occlusion=False):
    """The mesh of `atlas` with its textures (pack_textures's images, and pack_normal_map's as `normal_map`: then with tangents)
    as one .glb; textures_dir: also the PNG files.  occlusion: the R channel of `orm` holds the ambient occlusion
    (gs2m_mesh_ao.apply_occlusion): the material gets an occlusionTexture."""
    if len(atlas.triangles) == 0:
        raise RuntimeError("export_glb: the mesh has no triangle")
    pngs = encode_png([base_color] + ([orm] if orm is not None else []) + ([normal_map] if normal_map is not None else []), device_png)
    names = ["base_color.png"] + (["metallic_roughness.png"] if orm is not None else []) + (["normal.png"] if normal_map is not None else [])
    if textures_dir:
        os.makedirs(textures_dir, exist_ok=True)
        for name, b in zip(names, pngs):
            with open(os.path.join(textures_dir, name), "wb") as f:
                f.write(b)
    more = {"occlusion": True} if occlusion else {}
    if normal_map is None:
        return write_glb(file, *unwelded(atlas), pngs, **more)
    return write_glb(file, *unwelded(atlas), pngs[:-1], tangents=unwelded_tangents(atlas), normal_image=pngs[-1], **more)


# ---- command line ------------------------------------------------------------------------------------------------------------

def parser():
    ap = argparse.ArgumentParser(description="Bake a trained model into the texture atlas of its mesh and write a glTF 2.0 binary")
    ap.add_argument("--ply", required=True, help="the model's point_cloud.ply")
    ap.add_argument("--source-path", "--source_path", "-s", required=True, help="COLMAP-format dataset (or NeRF-synthetic with --blender)")
    ap.add_argument("--mesh", required=True, help="the mesh to texture (binary PLY), e.g. tsdf_simplified.ply")
    ap.add_argument("--output", "-o", required=True, help="the .glb to write")
    size = ap.add_mutually_exclusive_group(required=True)
    size.add_argument("--texture-size", type=int, metavar="N", help="the atlas is at most N texels wide (the densest rung that fits)")
    size.add_argument("--density", type=float, metavar="D", help="texels per world unit")
    ap.add_argument("--metallic", action="store_true", help="the model's metallic map (default: estimated from the roughness)")
    ap.add_argument("--rgb", action="store_true", help="bake the plain render into a base colour only (a model without materials)")
    ap.add_argument("--linear", action="store_true", help="store the base colour without the sRGB transfer")
    normal = ap.add_mutually_exclusive_group()
    normal.add_argument("--normal-map", action="store_true",
                        help="also bake the views' normals into a tangent-space normal map: TANGENT and normalTexture in the .glb")
    normal.add_argument("--normal-map-from", default=None, metavar="SOURCE.ply",
                        help="the normal map from the geometry of SOURCE.ply, the full mesh --mesh was simplified from, instead of the "
                        "views' rendered normals (gs2m_mesh_transfer.py); the colours are baked from the views as without it")
    ap.add_argument("--textures-dir", default=None, metavar="DIR",
                    help="also write base_color.png and metallic_roughness.png (with --normal-map: normal.png) there")
    ap.add_argument("--blender", action="store_true")
    ap.add_argument("--split", choices=("train", "test"), default="train")
    ap.add_argument("--resolution", "-r", type=int, default=1)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--eps", type=float, default=EPS, help="a texel is in front when z < depth + eps")
    ap.add_argument("--min-weight", type=float, default=MIN_WEIGHT, help="summed cosines a texel needs to count as seen")
    ap.add_argument("--view-batch", type=int, default=VIEW_BATCH)
    from gs2m_mesh_bake import add_ao_arguments
    add_ao_arguments(ap, "the R channel of the ORM image and an occlusionTexture in the .glb (with --rgb: an ORM image of roughness 1, metallic 0)")
    from gs2m_ingest import add_ingest_arguments
    from gs2m_png import add_png_argument
    add_ingest_arguments(ap)
    add_png_argument(ap)
    return ap


def read_source_mesh(file):
    """The mesh to texture and what its vertices carry -> (mesh, vertex_values): for a material mesh (gs2m_mesh_bake.py's, or a
    simplified one) vertex_values is (V, 5) float32 albedo rgb, roughness, metallic -- the vertex bake's output; for any other PLY
    it is None and the mesh's vertex colours stand in."""
    import types
    import gs2m_mesh as M
    from gs2m_mesh_bake import read_material_mesh
    try:
        m = read_material_mesh(file)
    except ValueError:
        return M.read_mesh(file), None
    values = np.concatenate([m["albedo"], m["roughness"][:, None], m["metallic"][:, None]], axis=1).astype(np.float32)
    return types.SimpleNamespace(vertices=m["vertices"], triangles=m["triangles"], vertex_colors=m["albedo"]), values


def texture_mesh(model, cams, mesh, output, density=None, texture_size=None, metallic=False, rgb=False, linear=False, device_png=False,
                 textures_dir=None, eps=EPS, min_weight=MIN_WEIGHT, view_batch=None, vertex_values=None, normal_map=False, ao=False,
                 ao_rays=64, ao_radius=None, normal_source=None):
    """Atlas, bake, pack and export in one call -> dict(out, width, height, density, n_views, n_texels, n_seen).  Texels no view
    reached interpolate `vertex_values` (V, 5): albedo rgb, roughness, metallic, the vertex bake's output; without them the mesh's
    vertex colours, taken as they are for the linear albedo (a PLY says nothing of their transfer), with roughness 1 and metallic 0;
    a mesh without colours leaves the fallback.  normal_map: the views' normals too, as a tangent-space normal map.  ao: ambient
    occlusion traced against the mesh at every texel (gs2m_mesh_ao.texel_occlusion: ao_rays rays followed for ao_radius) into the
    R channel of the ORM image -- with rgb=True, which has none, one of roughness 1 and metallic 0 is made for it.
    normal_source: a mesh (the full one `mesh` was simplified from) whose geometric normals, found along each texel's normal by
    gs2m_mesh_transfer.transfer_texels with its defaults, make the normal map in the place of the views' (not with normal_map)."""
    if normal_map and normal_source is not None:
        raise ValueError("texture_mesh: `normal_map` bakes the views' normals, `normal_source` transfers a mesh's: give one of the two")
    atlas = build_atlas(mesh, density=density, texture_size=texture_size, device=model.get_xyz.device)
    colours = getattr(mesh, "vertex_colors", None)
    attributes = None
    if vertex_values is not None:
        x = torch.as_tensor(np.asarray(vertex_values, np.float32)).to(atlas.vertices.device).reshape(len(atlas.vertices), 5)
        attributes = x[:, :3].contiguous() if rgb else x.contiguous()
    elif colours is not None and len(colours) == len(atlas.vertices):
        c = torch.as_tensor(np.asarray(colours, np.float32)).to(atlas.vertices.device).reshape(-1, 3)
        attributes = c if rgb else torch.cat([c, torch.tensor(FALLBACK[3:], device=c.device).expand(len(c), 2)], 1).contiguous()
    values, seen, _ = bake_textures(model, cams, mesh, atlas, metallic=metallic, rgb=rgb, eps=eps, view_batch=view_batch,
                                    min_weight=min_weight, attributes=attributes, **({"normal_map": True} if normal_map else {}))
    base, orm = pack_textures(values, srgb=not linear)
    extra = {"normal_map": pack_normal_map(atlas, values)} if normal_map else {}
    if normal_source is not None:
        from gs2m_mesh_transfer import transfer_texels
        extra["normal_map"] = pack_normal_map(atlas, transfer_texels(atlas, normal_source, normal=True)[0])
    if ao:
        from gs2m_mesh_ao import apply_occlusion, texel_occlusion
        if orm is None:
            orm = torch.tensor([255, 255, 0], dtype=torch.uint8, device=base.device).repeat(atlas.height, atlas.width, 1).contiguous()
        visible, owner = texel_occlusion(atlas, rays=ao_rays, radius=ao_radius)
        apply_occlusion(orm, owner, visible, ao_rays)
        extra["occlusion"] = True
    export_glb(output, atlas, base, orm, device_png=device_png, textures_dir=textures_dir, **extra)
    print(f"[>] {len(cams)} views: atlas {atlas.width} x {atlas.height} at {atlas.density:.6g} texels per unit, "
          f"{int(seen.sum())} of {atlas.width * atlas.height} texels seen -> {output}")
    return {"out": str(output), "width": atlas.width, "height": atlas.height, "density": atlas.density, "n_views": len(cams),
            "n_texels": atlas.width * atlas.height, "n_seen": int(seen.sum())}


def main(argv=None):
    a = parser().parse_args(argv)
    import gs2m_mesh as M
    import gs2m_train as T
    from gs2m_model import GaussianModel
    if a.blender:
        cams, _, _, _, _ = T.load_blender_dataset(a.source_path, "transforms_test.json" if a.split == "test" else "transforms_train.json")
    else:
        from gs2m_ingest import ingest_keywords
        cams, _, _, _, _ = T.load_colmap_dataset(a.source_path, resolution=a.resolution, **ingest_keywords(a))
        if a.split == "test":
            cams = cams[::8]
    model = GaussianModel(a.sh_degree)
    model.load_ply(a.ply)
    mesh, vertex_values = read_source_mesh(a.mesh)
    return texture_mesh(model, cams, mesh, a.output, vertex_values=vertex_values, density=a.density, texture_size=a.texture_size, metallic=a.metallic, rgb=a.rgb,
                        linear=a.linear, device_png=a.device_png, textures_dir=a.textures_dir, eps=a.eps, min_weight=a.min_weight,
                        view_batch=a.view_batch, normal_map=a.normal_map, **({"ao": True, "ao_rays": a.ao_rays, "ao_radius": a.ao_radius} if a.ao else {}),
                        **({"normal_source": M.read_mesh(a.normal_map_from)} if a.normal_map_from else {}))


if __name__ == "__main__":
    main()
