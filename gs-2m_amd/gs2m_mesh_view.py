"""Shaded views and turntable frames of a mesh on the GPU (csrc/mesh_view.hip; include/gs2m_meshview.h).

The reference's scripts/vis_dtu.py and scripts/vis_shiny.py, which need Blender and Cycles, as DESIGN.md §16 writes the contract
down: the mesh is rasterized into a visibility buffer (nearest triangle per sample, the z-buffer rasterizer of the visibility
cull), shaded grey with a light at the camera (a Lambert term above an ambient floor), resolved over ss x ss samples per pixel and
encoded as straight-alpha sRGB bytes.  Everything is fp64 on device tensors owned here; there is no CPU path.

    python gs-2m_amd/gs2m_mesh_view.py --ply-path M.ply --cameras MODEL/cameras.json --rendering --still --animation
    python gs-2m_amd/gs2m_mesh_view.py --ply-path M.ply -s SCENE -r 2 --rendering --shading smooth --colour vertex
    python gs-2m_amd/gs2m_mesh_view.py --ply-path MATERIAL.ply -s SCENE --rendering --colour pbr --envmap studio.hdr [--background env]
    python gs-2m_amd/gs2m_mesh_view.py --glb ASSET.glb -s SCENE --rendering --colour texture [--shading smooth]
    python gs-2m_amd/gs2m_mesh_view.py --glb ASSET.glb -s SCENE --rendering --colour pbr --envmap studio.hdr
    python gs-2m_amd/gs2m_mesh_view.py (--ply-path M.ply | --glb ASSET.glb) -s SCENE --rendering --colour ao
(the third: a material mesh of gs2m_mesh_bake.py under an environment map; the last two: the textured .glb of
gs2m_mesh_texture.py, its base colour under the headlight or its materials under an environment map, with its normal map where
it has one; the last: the ambient occlusion as grey, unlit -- a PLY's `occlusion` property (gs2m_mesh_bake.py --ao) or,
without one, gs2m_mesh_ao.vertex_occlusion on the fly; a .glb's occlusionTexture (gs2m_mesh_texture.py --ao))
write views/<stem>.png, still.png, frames/000.png .. 119.png, anim.gif and anim.webp under --out-dir (default: visual/ beside the
mesh's directory).
"""
import argparse
import json
import math
import os
import sys
import types

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np
import torch

import gs2m_native as N
from gs2m_eval_util import device as _dev, ptr as _ptr, workspace_for
from gs2m_mesh_cull import FAR, NEAR, _mesh_args, _mesh_on_device, _on_device

VIS_BUDGET = 512 << 20  # bytes of visibility buffer a batch of views may take
BASE, AMBIENT, DIFFUSE = (0.7, 0.7, 0.7), 0.15, 0.85
STILL_SIZE, FRAMES, FPS, VIEW_IDX = 600, 120, 24, 23


def vertex_normals(vertices, triangles):
    """Open3D's compute_vertex_normals: per vertex the sum of its triangles' unit normals, kept exactly as int64 in units of
    2^-32, and that sum normalised.  -> (normals (V, 3) fp64, sums (V, 3) int64), device tensors."""
    who = "vertex_normals"
    v = _on_device(vertices, "vertices", who, torch.float64, (3,))
    f = _on_device(triangles, "triangles", who, torch.int32, (3,))
    sums = torch.empty((len(v), 3), dtype=torch.int64, device=v.device)
    normals = torch.empty((len(v), 3), dtype=torch.float64, device=v.device)
    ws = workspace_for("gs2m_meshview_normals_workspace_bytes", v.device)
    N.launch("gs2m_meshview_normals", v.device, len(v), _ptr(v), len(f), _ptr(f), _ptr(ws), _ptr(sums), _ptr(normals))
    return normals, sums


def _check_frame(H, W, ss, who):
    """what the library would refuse, before a buffer is sized by it -> (H, W, ss) as int"""
    if int(ss) != ss or not 1 <= int(ss) <= 4:
        raise RuntimeError(f"{who}: invalid argument: `ss` must be 1, 2, 3 or 4, got {ss!r}")
    H, W, ss = int(H), int(W), int(ss)
    if H < 1 or W < 1 or H * ss * W * ss > 2 ** 31 - 1:
        raise RuntimeError(f"{who}: invalid argument: a frame of {W} x {H} at ss = {ss} is empty or has more than 2^31 - 1 samples")
    return H, W, ss


def visibility_buffer(vertices, triangles, w2c, fx, fy, cx, cy, H, W, ss=1, near=NEAR, far=FAR, out=None):
    """The nearest triangle through every sample: (n_views, H ss, W ss) int64 on the device whose bits are the unsigned key
    (bits of the fp32 z << 32) | triangle index, all ones (-1) where there is none.  The sample frame has the intrinsics
    (ss fx, ss fy, ss cx, ss cy).  out: an int64 buffer of at least n_views H W ss^2 elements to render into."""
    who = "visibility_buffer"
    v, f, m = _mesh_args(vertices, triangles, w2c, who)
    H, W, ss = _check_frame(H, W, ss, who)
    dev, n, count = v.device, len(m), len(m) * H * W * ss * ss
    if out is None:
        vis = torch.empty(count, dtype=torch.int64, device=dev)
    else:
        if not torch.is_tensor(out) or out.device != dev or out.dtype != torch.int64 or not out.is_contiguous() or out.numel() < count:
            raise RuntimeError(f"{who}: `out` must be a contiguous int64 tensor of at least {count} elements on {dev}")
        vis = out.reshape(-1)[:count]
    ws = workspace_for("gs2m_meshview_workspace_bytes", dev, len(f), n)
    N.launch("gs2m_meshview_visibility", dev, len(v), _ptr(v), len(f), _ptr(f), n, _ptr(m), float(fx), float(fy), float(cx), float(cy),
             W, H, ss, float(near), float(far), _ptr(ws), _ptr(vis))
    return vis.view(n, H * ss, W * ss)


def shade_views(vertices, triangles, w2c, fx, fy, cx, cy, H, W, ss=2, shading="flat", colors=None, base=BASE, ambient=AMBIENT,
                diffuse=DIFFUSE, srgb=True, view_batch=None, return_aux=False, near=NEAR, far=FAR):
    """Shaded RGBA views of the mesh: (n_views, H, W, 4) uint8 on the device, straight alpha = the covered share of the pixel's
    ss x ss samples.  shading: "flat" (the face normal) or "smooth" (vertex normals interpolated).  colors: (V, 3) vertex colours
    in [0, 1] as the albedo instead of `base`.  The views go through the rasterizer `view_batch` at a time (default: as many as
    keep the visibility buffer under 512 MiB) into one reused buffer.  return_aux: also depth (n, H, W) float32 and tri_id
    (n, H, W) int32 of each pixel's centre sample, 0 and -1 where it is empty."""
    who = "shade_views"
    v, f, m = _mesh_args(vertices, triangles, w2c, who)
    H, W, ss = _check_frame(H, W, ss, who)
    if shading not in ("flat", "smooth"):
        raise RuntimeError(f"{who}: `shading` must be 'flat' or 'smooth', got {shading!r}")
    col = None if colors is None else _on_device(colors, "colors", who, torch.float32, (3,))
    if col is not None and len(col) != len(v):
        raise RuntimeError(f"{who}: {len(col)} colours for {len(v)} vertices")
    base = [float(x) for x in base]
    if len(base) != 3:
        raise RuntimeError(f"{who}: `base` must hold three values")
    dev, n = v.device, len(m)
    normals = vertex_normals(v, f)[0] if shading == "smooth" else None
    rgba = torch.empty((n, H, W, 4), dtype=torch.uint8, device=dev)
    depth = torch.empty((n, H, W), dtype=torch.float32, device=dev) if return_aux else None
    tri_id = torch.empty((n, H, W), dtype=torch.int32, device=dev) if return_aux else None
    # (with no view one call still checks the arguments and the indices)
    for k, part, vis in _view_batches(v, f, m, fx, fy, cx, cy, H, W, ss, near, far, 8 * H * W * ss * ss, view_batch, max(n, 1)):
        N.launch("gs2m_meshview_shade", dev, len(v), _ptr(v), len(f), _ptr(f), len(part), _ptr(part), float(fx), float(fy), float(cx),
                 float(cy), W, H, ss, _ptr(vis), _ptr(normals), _ptr(col), base[0], base[1], base[2], float(ambient), float(diffuse),
                 1 if srgb else 0, _ptr(rgba[k]), None if depth is None else _ptr(depth[k]), None if tri_id is None else _ptr(tri_id[k]))
    return (rgba, depth, tri_id) if return_aux else rgba


GBUFFER_BYTES = 8 + 4 * 14 + 1  # per sample: the key, the G-buffer and the shaded sample, the coverage


def _view_batches(v, f, m, fx, fy, cx, cy, H, W, ss, near, far, per_view, view_batch, stop=None):
    """The views `m` through the rasterizer `view_batch` at a time (default: as many as keep `per_view` bytes each under
    VIS_BUDGET) into one reused visibility buffer -> (the batch's slice of the views, its w2c, its visibility buffer), one
    batch after the other.  stop: the views end there (default: at len(m))."""
    n = len(m)
    batch = int(view_batch) if view_batch else max(1, VIS_BUDGET // max(per_view, 1))
    batch = max(1, min(batch, max(n, 1)))
    buf = torch.empty(batch * H * W * ss * ss, dtype=torch.int64, device=v.device)
    for k in range(0, n if stop is None else stop, batch):
        part = m[k:k + batch]
        yield slice(k, k + batch), part, visibility_buffer(v, f, part, fx, fy, cx, cy, H, W, ss, near, far, out=buf)


def _check_vis(vis, who, dev, n, H, W, ss):
    if not torch.is_tensor(vis) or vis.device != dev or vis.dtype != torch.int64 or not vis.is_contiguous() or vis.numel() != n * H * W * ss * ss:
        raise RuntimeError(f"{who}: `vis` must be the contiguous int64 visibility buffer of {n} views of {W * ss} x {H * ss} samples on {dev}")


GBUFFER_PLANES = (("normal", 3), ("view_dir", 3), ("albedo", 3), ("roughness", 1), ("metallic", 1))


def _new_gbuffer(dev, n, H, W, ss):
    """-> (the G-buffer dict of n views, uninitialised; its six pointers in the order of the C entries)"""
    shape = (n, H * ss, W * ss)
    g = {name: torch.empty(shape + (c,), dtype=torch.float32, device=dev) for name, c in GBUFFER_PLANES}
    g["coverage"] = torch.empty(shape, dtype=torch.uint8, device=dev)
    return g, tuple(_ptr(t) for t in g.values())


def mesh_gbuffer(vertices, triangles, w2c, fx, fy, cx, cy, H, W, vis, albedo, roughness, metallic, ss=1, normals=None):
    """The G-buffer of the samples of `vis` (visibility_buffer of the same mesh, views, frame and ss): dict(normal, view_dir,
    albedo: (n, H ss, W ss, 3) float32; roughness, metallic: (n, H ss, W ss, 1) float32; coverage: (n, H ss, W ss) uint8), on the
    device.  normal and view_dir (surface to eye) are unit vectors in world space, the normal facing the eye; albedo (V, 3),
    roughness (V,) and metallic (V,) are float32 vertex arrays interpolated by the sample's barycentrics.  normals: (V, 3) fp64
    vertex normals for smooth shading, None for flat.  An empty sample is 0 throughout."""
    who = "mesh_gbuffer"
    v, f, m = _mesh_args(vertices, triangles, w2c, who)
    H, W, ss = _check_frame(H, W, ss, who)
    dev, n = v.device, len(m)
    a = _on_device(albedo, "albedo", who, torch.float32, (3,))
    r = _on_device(roughness, "roughness", who, torch.float32, ())
    k = _on_device(metallic, "metallic", who, torch.float32, ())
    if not len(a) == len(r) == len(k) == len(v):
        raise RuntimeError(f"{who}: {len(a)} albedo, {len(r)} roughness and {len(k)} metallic values for {len(v)} vertices")
    _check_vis(vis, who, dev, n, H, W, ss)
    nrm = None if normals is None else _on_device(normals, "normals", who, torch.float64, (3,))
    g, outputs = _new_gbuffer(dev, n, H, W, ss)
    N.launch("gs2m_meshview_gbuffer", dev, len(v), _ptr(v), len(f), _ptr(f), n, _ptr(m), float(fx), float(fy), float(cx), float(cy), W, H, ss,
             _ptr(vis), _ptr(nrm), _ptr(a), _ptr(r), _ptr(k), *outputs)
    return g


def _image(t, name, who, dev, like=None):
    """a (th, tw, 3) uint8 texture on `dev`, of the size of `like` when given"""
    if not torch.is_tensor(t) or t.device != dev or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.numel() == 0:
        raise RuntimeError(f"{who}: `{name}` must be a (th, tw, 3) uint8 tensor on {dev}")
    if like is not None and t.shape != like.shape:
        raise RuntimeError(f"{who}: `{name}` is {tuple(t.shape)}, the base colour {tuple(like.shape)}")
    return t.contiguous()


def mesh_gbuffer_textured(vertices, triangles, uvs, w2c, fx, fy, cx, cy, H, W, vis, base_color, orm=None, normal_map=None, srgb=True,
                          ss=1, normals=None):
    """mesh_gbuffer with the materials read from textures (include/gs2m_meshview.h, the Textured paragraph): uvs (F, 3, 2) float32
    per triangle corner, v from the top row; base_color, orm, normal_map: (th, tw, 3) uint8 device tensors of one size, orm and
    normal_map optional (roughness 1 and metallic 0; the geometric normal).  srgb: the base colour is sRGB-encoded and is decoded.
    normal_map is tangent-space, in the frame gs2m_mesh_texture.pack_normal_map encodes in.  -> the same dict."""
    who = "mesh_gbuffer_textured"
    v, f, m = _mesh_args(vertices, triangles, w2c, who)
    H, W, ss = _check_frame(H, W, ss, who)
    dev, n = v.device, len(m)
    uv = N.f32(uvs, "uvs", (len(f), 3, 2), who=who)
    base = _image(base_color, "base_color", who, dev)
    o = None if orm is None else _image(orm, "orm", who, dev, base)
    nm = None if normal_map is None else _image(normal_map, "normal_map", who, dev, base)
    _check_vis(vis, who, dev, n, H, W, ss)
    nrm = None if normals is None else _on_device(normals, "normals", who, torch.float64, (3,))
    g, outputs = _new_gbuffer(dev, n, H, W, ss)
    N.launch("gs2m_meshview_gbuffer_textured", dev, len(v), _ptr(v), len(f), _ptr(f), _ptr(uv), n, _ptr(m), float(fx), float(fy), float(cx),
             float(cy), W, H, ss, _ptr(vis), _ptr(nrm), int(base.shape[1]), int(base.shape[0]), _ptr(base), 1 if srgb else 0, _ptr(o), _ptr(nm),
             *outputs)
    return g


def shade_views_textured(vertices, triangles, uvs, w2c, fx, fy, cx, cy, H, W, base_color, normal_map=None, texture_srgb=True, ss=2,
                         normals=None, ambient=AMBIENT, diffuse=DIFFUSE, srgb=True, view_batch=None, near=NEAR, far=FAR):
    """shade_views for a textured mesh: the headlight Lambert shade, ambient + diffuse |dot(normal, view_dir)|, on the texture's
    base colour, per sample of the textured G-buffer and resolved by resolve_rgb -> (n_views, H, W, 4) uint8, straight alpha.
    normals: (V, 3) fp64 vertex normals for smooth shading, None for flat."""
    who = "shade_views_textured"
    v, f, m = _mesh_args(vertices, triangles, w2c, who)
    H, W, ss = _check_frame(H, W, ss, who)
    rgba = torch.empty((len(m), H, W, 4), dtype=torch.uint8, device=v.device)
    for k, part, vis in _view_batches(v, f, m, fx, fy, cx, cy, H, W, ss, near, far, GBUFFER_BYTES * H * W * ss * ss, view_batch):
        g = mesh_gbuffer_textured(v, f, uvs, part, fx, fy, cx, cy, H, W, vis.reshape(-1), base_color, None, normal_map, texture_srgb, ss, normals)
        cos = (g["normal"] * g["view_dir"]).sum(-1, keepdim=True).abs()
        rgba[k] = resolve_rgb(g["albedo"] * (float(ambient) + float(diffuse) * cos), g["coverage"], ss, srgb)
    return rgba


def resolve_rgb(rgb, coverage, ss, srgb=False, background=None):
    """Per-sample linear RGB (n, H ss, W ss, 3) float32 and coverage bytes (n, H ss, W ss) -> (n, H, W, 4) uint8: the mean over a
    pixel's covered samples, optionally sRGB-encoded, straight alpha = the covered share.  background: (n, H, W, 3) float32 in the
    output's encoding, composited under the alpha; the alpha byte is then 255."""
    who = "resolve_rgb"
    rgb = N.f32(rgb, "rgb", who=who)
    if rgb.dim() != 4 or rgb.shape[3] != 3 or int(ss) < 1 or rgb.shape[1] % int(ss) or rgb.shape[2] % int(ss):
        raise RuntimeError(f"{who}: `rgb` must have shape (n, H ss, W ss, 3) with ss = {ss}, got {tuple(rgb.shape)}")
    n, H, W = int(rgb.shape[0]), int(rgb.shape[1]) // int(ss), int(rgb.shape[2]) // int(ss)
    H, W, ss = _check_frame(H, W, ss, who)
    if not torch.is_tensor(coverage) or coverage.device != rgb.device or coverage.dtype != torch.uint8 or coverage.numel() * 3 != rgb.numel():
        raise RuntimeError(f"{who}: `coverage` must be a uint8 tensor of shape {tuple(rgb.shape[:3])} on {rgb.device}")
    bg = None if background is None else N.f32(background, "background", (n, H, W, 3), who=who)
    out = torch.empty((n, H, W, 4), dtype=torch.uint8, device=rgb.device)
    N.launch("gs2m_meshview_resolve_rgb", rgb.device, n, W, H, ss, _ptr(rgb), _ptr(coverage.contiguous()), 1 if srgb else 0, _ptr(bg), _ptr(out))
    return out


def pixel_view_dirs(w2c, fx, fy, cx, cy, H, W):
    """The unit directions surface -> eye along the rays through the pixel centres, in world space: (n, H, W, 3) float32, what
    gs2m_relight.environment_behind takes."""
    m = torch.as_tensor(w2c).to(torch.float64).reshape(-1, 4, 4)
    j, i = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=m.device), torch.arange(W, dtype=torch.float64, device=m.device), indexing="ij")
    r = torch.stack([(i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, torch.ones_like(i)], dim=-1)
    world = torch.einsum("nck,hwc->nhwk", m[:, :3, :3], r)
    return (-world / world.norm(dim=-1, keepdim=True)).to(torch.float32)


def shade_views_pbr(vertices, triangles, w2c, fx, fy, cx, cy, H, W, light, albedo=None, roughness=None, metallic=None, ss=2,
                    shading="smooth", gamma=False, background="none", view_batch=None, near=NEAR, far=FAR, textures=None):
    """Views of a material mesh under an environment light: (n_views, H, W, 4) uint8 on the device.  light: anything with
    `.cubemap` (a CubemapLight) and `.brdf_lut`, e.g. gs2m_envmap.EnvLight.  The materials are either albedo (V, 3), roughness
    (V,), metallic (V,), float32 vertex attributes, or `textures`: dict(uvs, base_color, and optionally orm, normal_map, srgb
    (default True): what mesh_gbuffer_textured takes; normals: the mesh's own (V, 3) vertex normals, e.g. a .glb's, that smooth
    shading then uses instead of vertex_normals).  Per batch of views: the visibility buffer, the G-buffer of its samples, the
    project's fused split-sum shading (pbr_shading_fused) on every sample, and the resolve over ss x ss samples; gamma:
    sRGB-encode the resolved colour.  background "none": straight alpha = the covered share of the pixel; "env": the environment
    along the pixel's ray (gs2m_relight.environment_behind) under the alpha, which is then 255."""
    from pbr import pbr_shading_fused
    who = "shade_views_pbr"
    v, f, m = _mesh_args(vertices, triangles, w2c, who)
    H, W, ss = _check_frame(H, W, ss, who)
    if shading not in ("flat", "smooth"):
        raise RuntimeError(f"{who}: `shading` must be 'flat' or 'smooth', got {shading!r}")
    if background not in ("none", "env"):
        raise RuntimeError(f"{who}: `background` must be 'none' or 'env', got {background!r}")
    t = textures
    if (t is None) == (albedo is None and roughness is None and metallic is None):
        raise RuntimeError(f"{who}: give the materials as `albedo`, `roughness` and `metallic`, or as `textures`")
    normals = None
    if shading == "smooth":
        normals = t["normals"] if t is not None and t.get("normals") is not None else vertex_normals(v, f)[0]
    rgba = torch.empty((len(m), H, W, 4), dtype=torch.uint8, device=v.device)
    with torch.no_grad():
        light.cubemap.build_mips()
        for k, part, vis in _view_batches(v, f, m, fx, fy, cx, cy, H, W, ss, near, far, GBUFFER_BYTES * H * W * ss * ss, view_batch):
            if t is not None:
                g = mesh_gbuffer_textured(v, f, t["uvs"], part, fx, fy, cx, cy, H, W, vis.reshape(-1), t["base_color"], t.get("orm"),
                                          t.get("normal_map"), t.get("srgb", True), ss, normals)
            else:
                g = mesh_gbuffer(v, f, part, fx, fy, cx, cy, H, W, vis.reshape(-1), albedo, roughness, metallic, ss, normals)
            rgb = pbr_shading_fused(light.cubemap, g["normal"], g["view_dir"], g["albedo"], g["roughness"], metallic=g["metallic"],
                                    brdf_lut=light.brdf_lut, gamma=False)["render_rgb"]
            bg = None
            if background == "env":
                from gs2m_relight import environment_behind
                dirs = pixel_view_dirs(part, fx, fy, cx, cy, H, W)
                bg = torch.stack([environment_behind(light, d, gamma) for d in dirs]).contiguous()
            rgba[k] = resolve_rgb(rgb.reshape(len(part), H * ss, W * ss, 3), g["coverage"], ss, gamma, bg)
    return rgba


def turntable(w2c, frames=FRAMES, shift=(0.0, 0.0, 0.0)):
    """The rocking animation of vis_dtu.py's export_anim as cameras: the mesh, moved by `shift`, turns about its x axis by
    0.4 sin(2 pi f / frames) and then about its y axis by 0.6 sin(4 pi f / frames) (Euler XYZ); composed into the camera:
    w2c @ T(shift) @ Ry @ Rx.  w2c: (4, 4) world-to-camera.  -> (frames, 4, 4) float64 numpy."""
    w = np.asarray(torch.as_tensor(w2c).detach().cpu().numpy() if torch.is_tensor(w2c) else w2c, np.float64).reshape(4, 4)
    T = np.eye(4)
    T[:3, 3] = np.asarray(shift, np.float64)
    out = np.empty((int(frames), 4, 4), np.float64)
    for k in range(int(frames)):
        ax, ay = 0.4 * math.sin(2.0 * math.pi * k / frames), 0.6 * math.sin(4.0 * math.pi * k / frames)
        Rx, Ry = np.eye(4), np.eye(4)
        Rx[1:3, 1:3] = [[math.cos(ax), -math.sin(ax)], [math.sin(ax), math.cos(ax)]]
        Ry[0, 0], Ry[0, 2], Ry[2, 0], Ry[2, 2] = math.cos(ay), math.sin(ay), -math.sin(ay), math.cos(ay)
        out[k] = w @ T @ Ry @ Rx
    return out


# ---- files -------------------------------------------------------------------------------------------------------------------

def read_cameras_json(path):
    """MODEL/cameras.json, the reference's camera_to_JSON records -> a list of dict(name, width, height, fx, fy, cx, cy, w2c):
    `rotation` and `position` are the camera-to-world pose (OpenCV convention), the principal point is the frame's centre."""
    with open(str(path)) as f:
        records = json.load(f)
    views = []
    for r in records:
        c2w = np.eye(4)
        c2w[:3, :3], c2w[:3, 3] = np.asarray(r["rotation"], np.float64).reshape(3, 3), np.asarray(r["position"], np.float64).reshape(3)
        w, h = int(r["width"]), int(r["height"])
        views.append(dict(name=str(r["img_name"]), width=w, height=h, fx=float(r["fx"]), fy=float(r["fy"]), cx=0.5 * w, cy=0.5 * h,
                          w2c=np.linalg.inv(c2w)))
    return views


def read_colmap_views(folder):
    """SCENE/sparse/0 through the readers gs2m_train.load_colmap_dataset is built on (images sorted by name; no image is opened)
    -> the same list as read_cameras_json."""
    import gs2m_colmap as C
    sparse = os.path.join(str(folder), "sparse", "0")
    intr = C.read_intrinsics_binary(os.path.join(sparse, "cameras.bin"))
    infos = sorted(C.colmap_cameras(C.read_extrinsics_binary(os.path.join(sparse, "images.bin")), intr), key=lambda c: c.image_name)
    views = []
    for info in infos:
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = np.asarray(info.R, np.float64).T, np.asarray(info.T, np.float64)
        views.append(dict(name=str(info.image_name), width=int(info.width), height=int(info.height), fx=float(info.Fx), fy=float(info.Fy),
                          cx=0.5 * info.width, cy=0.5 * info.height, w2c=w2c))
    return views


def scaled(view, n):
    """-r N: the frame at (w // N, h // N), the intrinsics scaled by the same two ratios"""
    w, h = view["width"] // n, view["height"] // n
    sx, sy = w / view["width"], h / view["height"]
    return dict(view, width=w, height=h, fx=view["fx"] * sx, fy=view["fy"] * sy, cx=view["cx"] * sx, cy=view["cy"] * sy)


def write_gif(frames, path, fps=FPS):
    """(n, H, W, 4) uint8 numpy -> a looping GIF as vis_dtu.py's convert_gif makes it: pixels of alpha 0 are transparent, the
    others opaque; one adaptive palette of 255 colours from the first frame, whose black entry (else entry 0) is the transparent
    index; every frame replaces the one before (disposal 2)."""
    from PIL import Image
    rgb = [Image.fromarray(np.where(f[..., 3:] == 0, 0, f[..., :3]).astype(np.uint8), "RGB") for f in frames]
    source = rgb[0].convert("P", palette=Image.ADAPTIVE, colors=255)
    pal = source.getpalette()
    black = [k for k in range(len(pal) // 3) if pal[3 * k:3 * k + 3] == [0, 0, 0]]
    index = black[0] if black else 0
    out = []
    for im, f in zip(rgb, frames):
        q = im.quantize(palette=source)
        q.paste(index, mask=Image.fromarray(np.where(f[..., 3] == 0, 255, 0).astype(np.uint8), "L"))
        out.append(q)
    out[0].save(str(path), save_all=True, append_images=out[1:], optimize=True, duration=int(1000 / fps), loop=0, transparency=index, disposal=2)


def write_webp(frames, path, fps=FPS):
    """an animated WebP of the RGBA frames where the installed Pillow can write one -> whether it was written"""
    from PIL import Image, features
    if not features.check("webp"):
        return False
    ims = [Image.fromarray(f, "RGBA") for f in frames]
    ims[0].save(str(path), save_all=True, append_images=ims[1:], format="WEBP", duration=int(1000 / fps), loop=0)
    return True


def read_textured_mesh(file, device):
    """A .glb of gs2m_mesh_texture.write_glb as device tensors -> dict(vertices (V, 3) float64, triangles (F, 3) int32, uvs
    (F, 3, 2) float32, normals (V, 3) float64: the NORMAL accessor, base_color, orm, normal_map: (th, tw, 3) uint8, the last two
    None where the file has none).  The PNGs are decoded on the host (gs2m_mesh_texture.decode_png)."""
    import gs2m_mesh_texture as MT
    g = MT.read_glb(file)
    idx = np.asarray(g["indices"], np.int64).reshape(-1, 3)

    def image(data):
        px = MT.decode_png(data)
        if px.ndim != 3 or px.shape[2] < 3 or px.dtype != np.uint8:
            raise ValueError(f"{file}: a texture is not 8-bit RGB")
        return torch.as_tensor(np.ascontiguousarray(px[..., :3])).to(device)

    images = [image(b) for b in g["images"]]
    if not images:
        raise ValueError(f"{file}: no base-colour texture")
    return dict(vertices=torch.as_tensor(np.asarray(g["positions"], np.float64)).to(device),
                triangles=torch.as_tensor(idx.astype(np.int32)).to(device),
                uvs=torch.as_tensor(np.ascontiguousarray(np.asarray(g["uvs"], np.float32)[idx])).to(device),
                normals=torch.as_tensor(np.asarray(g["normals"], np.float64)).to(device), base_color=images[0],
                orm=images[1] if len(images) > 1 else None, normal_map=None if g["normal_image"] is None else image(g["normal_image"]))


def view_files(a):
    """The command line's work.  -> dict(out_dir, views: the PNGs written, still, frames, gif, webp)."""
    import gs2m_mesh as M
    dev = _dev(None)
    glb = getattr(a, "glb", "") or ""
    if glb:
        return _view_files(a, dev, None, read_textured_mesh(glb, dev))
    if a.colour == "texture":
        raise RuntimeError("--colour texture needs --glb FILE")
    if not a.ply_path:
        raise RuntimeError("give the mesh: --ply-path FILE or --glb FILE")
    return _view_files(a, dev, M.read_mesh(a.ply_path), None)


def _view_files(a, dev, mesh, tex):
    if tex is not None:
        if a.colour not in ("texture", "pbr", "ao"):
            raise RuntimeError("--glb is drawn with --colour texture or --colour pbr, or its occlusion with --colour ao")
        v, f = tex["vertices"], tex["triangles"]
        if a.colour == "ao":  # the occlusion as a linear grey base colour, drawn unlit
            from gs2m_mesh_texture import read_glb
            if tex["orm"] is None or not read_glb(a.glb)["occlusion"]:
                raise RuntimeError(f"{a.glb}: --colour ao needs a .glb with an occlusionTexture (gs2m_mesh_texture.py --ao writes one)")
            tex = dict(tex, base_color=tex["orm"][..., :1].expand(-1, -1, 3).contiguous(), normal_map=None)
    else:
        v, f = _mesh_on_device(mesh, dev, "view_files")
    col = None
    if a.colour == "vertex":
        if mesh.vertex_colors is None:
            raise RuntimeError(f"{a.ply_path}: --colour vertex needs a mesh with vertex colours")
        col = torch.as_tensor(np.asarray(mesh.vertex_colors, np.float32).reshape(-1, 3)).to(dev)
    if a.colour == "ao" and tex is None:  # the file's occlusion property, else traced here
        from gs2m_mesh_bake import read_material_mesh
        try:
            ao = read_material_mesh(a.ply_path).get("occlusion")
        except ValueError:
            ao = None
        if ao is None:
            from gs2m_mesh_ao import vertex_occlusion
            ao = vertex_occlusion(types.SimpleNamespace(vertices=v, triangles=f), device=dev)[1]
        col = torch.as_tensor(np.asarray(ao.cpu() if torch.is_tensor(ao) else ao, np.float32)).to(dev).reshape(-1, 1).expand(-1, 3).contiguous()
    unlit = {"ambient": 1.0, "diffuse": 0.0} if a.colour == "ao" else {}
    views = read_cameras_json(a.cameras) if a.cameras else read_colmap_views(a.source_path)
    if not views:
        raise RuntimeError("no camera to render from")
    out_dir = a.out_dir or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(a.glb if tex is not None else a.ply_path))), "visual")
    os.makedirs(out_dir, exist_ok=True)
    result = dict(out_dir=out_dir, views=[], still=None, frames=[], gif=None, webp=None)
    from gs2m_png import Writer
    writer = Writer("device" if getattr(a, "device_png", False) else "host")  # the PNGs; the GIF and the WebP stay on Pillow

    material = light = None
    if a.colour == "pbr":
        import gs2m_relight as RL
        from gs2m_envmap import EnvLight
        from gs2m_mesh_bake import read_material_mesh
        if not a.envmap:
            raise RuntimeError("--colour pbr needs --envmap FILE.hdr")
        srgb_tex = not getattr(a, "linear_texture", False)
        if tex is not None:
            material = dict(textures=dict(tex, srgb=srgb_tex))
        else:
            try:
                mm = read_material_mesh(a.ply_path)
            except ValueError as e:
                raise RuntimeError(f"--colour pbr needs a material mesh (gs2m_mesh_bake.py writes one): {e}") from None
            material = {k: torch.as_tensor(mm[k]).to(dev) for k in ("albedo", "roughness", "metallic")}
        light = EnvLight.from_hdr(a.envmap, a.env_res, a.env_samples, math.radians(a.env_rotation), a.exposure, device=dev)
        RL._check(light, "env", "normal")  # the light's size, as the relighting checks it

    def shade(w2c, k, H, W):
        m = torch.as_tensor(np.ascontiguousarray(w2c)).to(dev)
        if material is not None:
            return shade_views_pbr(v, f, m, k["fx"], k["fy"], k["cx"], k["cy"], H, W, light, ss=a.ss, shading=a.shading, gamma=a.gamma,
                                   background=a.background, **material)
        if tex is not None:
            return shade_views_textured(v, f, tex["uvs"], m, k["fx"], k["fy"], k["cx"], k["cy"], H, W, tex["base_color"], tex["normal_map"],
                                        not getattr(a, "linear_texture", False) and a.colour != "ao", ss=a.ss,
                                        normals=tex["normals"] if a.shading == "smooth" else None, **unlit)
        return shade_views(v, f, m, k["fx"], k["fy"], k["cx"], k["cy"], H, W, ss=a.ss, shading=a.shading, colors=col, **unlit)

    if a.rendering:
        os.makedirs(os.path.join(out_dir, "views"), exist_ok=True)
        chosen = [scaled(x, a.resolution) for x in (views if a.render_view_idx < 0 else [views[a.render_view_idx]])]
        groups = {}
        for x in chosen:  # one batched call per frame size and intrinsics
            groups.setdefault((x["height"], x["width"], x["fx"], x["fy"], x["cx"], x["cy"]), []).append(x)
        for (H, W, *_), members in groups.items():
            images = shade(np.stack([x["w2c"] for x in members]), members[0], H, W)
            for x, image in zip(members, images):
                path = os.path.join(out_dir, "views", x["name"].split(".")[0] + ".png")
                writer.put(image, path)
                result["views"].append(path)
            writer.flush()
    if a.still or a.animation:
        # a 600 x 600 frame, the first view's focal lengths scaled to it as the frame of the first view is
        first, ref = views[0], views[min(a.view_idx, len(views) - 1)]
        k = dict(fx=first["fx"] * STILL_SIZE / first["width"], fy=first["fy"] * STILL_SIZE / first["height"], cx=0.5 * STILL_SIZE, cy=0.5 * STILL_SIZE)
        T = np.eye(4)
        T[:3, 3] = a.shift
        if a.still:
            result["still"] = os.path.join(out_dir, "still.png")
            writer.put(shade((ref["w2c"] @ T)[None], k, STILL_SIZE, STILL_SIZE)[0], result["still"])
            writer.flush()
        if a.animation:
            os.makedirs(os.path.join(out_dir, "frames"), exist_ok=True)
            images = shade(turntable(ref["w2c"], a.frames, a.shift), k, STILL_SIZE, STILL_SIZE)
            for n, image in enumerate(images):
                result["frames"].append(os.path.join(out_dir, "frames", f"{n:03d}.png"))
                writer.put(image, result["frames"][-1])
            writer.flush()
            host = images.cpu().numpy()
            result["gif"] = os.path.join(out_dir, "anim.gif")
            write_gif(host, result["gif"])
            webp = os.path.join(out_dir, "anim.webp")
            result["webp"] = webp if write_webp(host, webp) else None
    return result


def parser():
    ap = argparse.ArgumentParser(description="Shaded views and turntable frames of a mesh (scripts/vis_dtu.py, scripts/vis_shiny.py)")
    ap.add_argument("--ply-path", default="", help="the mesh (binary PLY), e.g. MODEL/train/ours_30000/mesh/tsdf_post.ply")
    ap.add_argument("--glb", default="", metavar="FILE",
                    help="instead of --ply-path: a textured .glb of gs2m_mesh_texture.py, drawn with --colour texture or --colour pbr")
    ap.add_argument("--linear-texture", action="store_true", help="the .glb's base colour was written with --linear")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--cameras", default="", help="MODEL/cameras.json")
    src.add_argument("--source-path", "-s", default="", help="a COLMAP-format dataset")
    ap.add_argument("--resolution", "-r", type=int, default=1, help="--rendering at (w // N, h // N)")
    ap.add_argument("--rendering", action="store_true", help="views/<stem>.png from every camera")
    ap.add_argument("--render_view_idx", type=int, default=-1, help="--rendering from this camera alone")
    ap.add_argument("--still", action="store_true", help="still.png, 600 x 600, from the camera --view-idx")
    ap.add_argument("--animation", action="store_true", help="frames/, anim.gif and anim.webp: the mesh rocking in front of --view-idx")
    ap.add_argument("--view-idx", type=int, default=VIEW_IDX)
    ap.add_argument("--frames", type=int, default=FRAMES, help=argparse.SUPPRESS)  # for the tests
    ap.add_argument("--shift", type=float, nargs=3, default=(0.0, 0.0, 0.0), metavar=("X", "Y", "Z"), help="moves the mesh (still, animation)")
    ap.add_argument("--shading", choices=("flat", "smooth"), default="flat")
    ap.add_argument("--colour", choices=("grey", "vertex", "pbr", "texture", "ao"), default="grey",
                    help="pbr: a material mesh (gs2m_mesh_bake.py), or the textures of --glb, shaded under --envmap; the options below "
                         "belong to it.  texture: the base colour of --glb under the headlight.  ao: the ambient occlusion as grey, unlit: a PLY's "
                         "occlusion property or one traced here, a .glb's occlusionTexture")
    ap.add_argument("--envmap", default="", help="lat-long Radiance file (.hdr), as gs2m_relight.py takes it")
    ap.add_argument("--env-res", type=int, default=512, help="cube-map resolution: a power of two >= 64")
    ap.add_argument("--env-samples", type=int, default=None, help="S x S taps per texel, 1 .. 16")
    ap.add_argument("--env-rotation", type=float, default=0.0, help="degrees about +y")
    ap.add_argument("--exposure", type=float, default=0.0, help="stops: the radiance is scaled by 2^EV")
    ap.add_argument("--gamma", action="store_true", help="sRGB-encode the shaded colour")
    ap.add_argument("--background", choices=("none", "env"), default="none", help="env: the environment along the view ray behind the mesh")
    ap.add_argument("--ss", type=int, default=2, help="samples per pixel and axis, 1 .. 4")
    ap.add_argument("--out-dir", default="", help="default: visual/ beside the mesh's directory")
    from gs2m_png import add_png_argument
    add_png_argument(ap)
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    if bool(a.ply_path) == bool(a.glb):
        ap.error("one of --ply-path and --glb is required")
    r = view_files(a)
    print(f"[>] {len(r['views'])} views, {'a still, ' if r['still'] else ''}{len(r['frames'])} frames -> {r['out_dir']}")
    return r


if __name__ == "__main__":
    main()
