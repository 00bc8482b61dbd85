"""Material mesh: the per-view BRDF maps of a trained model baked onto the vertices of its mesh (csrc/mesh_bake.hip;
include/gs2m_meshbake.h).

As DESIGN.md §20 writes the contract down: every vertex is projected into every view; a view counts where the vertex lies inside
the frame, is not behind the mesh's own z-buffer (z < depth + eps, the visibility cull's test), all its bilinear taps are
foreground, and the surface faces the camera; the views' bilinear samples are averaged with the cosine between the vertex normal
and the direction to the camera as the weight.  Everything is fp64 on device tensors owned here; there is no CPU path.

    python gs-2m_amd/gs2m_mesh_bake.py --ply point_cloud.ply -s SCENE --mesh tsdf_post.ply -o tsdf_material.ply [--metallic]
writes the mesh with albedo as its vertex colour and the float properties roughness and metallic (and a byte `seen`: 0 where no view
reached the vertex and the fallback stands).  gs2m_mesh_view.py --colour pbr shades it under an environment map.
"""
import argparse
import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np
import torch

import gs2m_native as N
from gs2m_eval_util import ptr as _ptr
from gs2m_mesh_cull import EPS, FAR, NEAR, VIEW_BATCH, _mesh_on_device, _on_device, render_mesh_depth

MAX_CHANNELS = 8
MIN_WEIGHT = 1e-3                          # a vertex seen only at a grazing angle keeps the fallback
FALLBACK = (0.5, 0.5, 0.5, 1.0, 0.0)        # albedo, roughness, metallic of a vertex no view reached
CHANNELS = ("albedo_r", "albedo_g", "albedo_b", "roughness", "metallic")


class _Bake:
    """What the vertex bake and the texel bake (gs2m_mesh_texture.TextureBaker) share: the running sums and weights of `n` points,
    the reused depth buffer of the mesh `v`, `f`, the checks of `maps` and `mask`, the accumulate launch and the fallback of
    `finish`.  A subclass names itself in `who` and its accumulate entry in `entry`, says in `_points` where its points, normals
    and owner are, and shapes the result in `finish`."""
    who = entry = None

    def __init__(self, v, f, n, channels, eps, near, far):
        self.v, self.f, self.n, self.channels = v, f, int(n), int(channels)
        if not 1 <= self.channels <= MAX_CHANNELS:
            raise RuntimeError(f"{self.who}: invalid argument: {channels} channels; 1 to {MAX_CHANNELS}")
        self.eps, self.near, self.far = float(eps), float(near), float(far)
        self.sums = torch.zeros((self.n, self.channels), dtype=torch.float64, device=v.device)
        self.weights = torch.zeros(self.n, dtype=torch.float64, device=v.device)
        self._depth = None

    def _points(self):
        """the entry's arguments between the number of points and the number of views"""
        raise NotImplementedError

    def add(self, w2c, fx, fy, cx, cy, maps, mask=None):
        """w2c (n, 4, 4); maps (n, C, H, W) float32; mask (n, H, W) float32 or bool, or None: device tensors."""
        who = f"{self.who}.add"
        m = _on_device(w2c, "w2c", who, torch.float64, (4, 4))
        a = N.f32(maps, "maps", who=who)
        if a.dim() != 4 or a.shape[0] != len(m) or a.shape[1] != self.channels:
            raise RuntimeError(f"{who}: `maps` must have shape ({len(m)}, {self.channels}, H, W), got {tuple(a.shape)}")
        H, W = int(a.shape[2]), int(a.shape[3])
        k = None
        if mask is not None:
            k = N.f32(mask.float() if torch.is_tensor(mask) and mask.dtype in (torch.bool, torch.uint8) else mask, "mask", who=who)
            if k.numel() != len(m) * H * W:
                raise RuntimeError(f"{who}: `mask` {tuple(k.shape)} does not match ({len(m)}, {H}, {W})")
        if self._depth is None or self._depth.numel() < len(m) * H * W:
            self._depth = torch.empty(len(m) * H * W, dtype=torch.float32, device=self.v.device)
        depth = render_mesh_depth(self.v, self.f, m, fx, fy, cx, cy, H, W, self.near, self.far, out=self._depth)
        N.launch(self.entry, self.v.device, self.n, *self._points(), len(m), _ptr(m), float(fx), float(fy), float(cx), float(cy), W, H,
                 _ptr(depth), self.channels, _ptr(a), _ptr(k), self.eps, 1, _ptr(self.sums), _ptr(self.weights))

    def _resolve(self, entry, shape, min_weight, fallback, head=(), tail=()):
        """-> (values `shape` + (C,) float32, seen `shape` bool) of entry(n, C, *head, sums, weights, min_weight, fallback, *tail,
        values, seen)"""
        fb = [0.0] * self.channels if fallback is None else [float(x) for x in fallback]
        if len(fb) != self.channels:
            raise RuntimeError(f"{self.who}.finish: {len(fb)} fallback values for {self.channels} channels")
        out = torch.empty(tuple(shape) + (self.channels,), dtype=torch.float32, device=self.v.device)
        seen = torch.empty(tuple(shape), dtype=torch.uint8, device=self.v.device)
        N.launch(entry, self.v.device, self.n, self.channels, *head, _ptr(self.sums), _ptr(self.weights), float(min_weight),
                 (C.c_float * self.channels)(*fb), *tail, _ptr(out), _ptr(seen))
        return out, seen.bool()


class Baker(_Bake):
    """The running sums of a bake: `add` takes a batch of views with their maps, `finish` resolves.  The views may come in any
    grouping; the result depends only on their order."""
    who, entry = "Baker", "gs2m_meshbake_accumulate"

    def __init__(self, vertices, triangles, channels, eps=EPS, use_normals=True, near=NEAR, far=FAR):
        v = _on_device(vertices, "vertices", self.who, torch.float64, (3,))
        f = _on_device(triangles, "triangles", self.who, torch.int32, (3,))
        super().__init__(v, f, len(v), channels, eps, near, far)
        self.normals = None
        if use_normals:
            from gs2m_mesh_view import vertex_normals
            self.normals = vertex_normals(self.v, self.f)[0]

    def _points(self):
        return _ptr(self.v), _ptr(self.normals)

    def finish(self, min_weight=MIN_WEIGHT, fallback=None):
        """-> (values (V, C) float32, seen (V,) bool, weights (V,) float64)"""
        return self._resolve("gs2m_meshbake_resolve", (self.n,), min_weight, fallback) + (self.weights,)


def bake_slices(who, new_baker, w2c, fx, fy, cx, cy, maps, mask, view_batch):
    """The views of one size and one set of intrinsics through new_baker(C), `view_batch` at a time (default 8) -> the baker"""
    m = _on_device(w2c, "w2c", who, torch.float64, (4, 4))
    a = N.f32(maps, "maps", who=who)
    if a.dim() != 4 or a.shape[0] != len(m):
        raise RuntimeError(f"{who}: `maps` must have shape (n_views, C, H, W) with n_views = {len(m)}, got {tuple(a.shape)}")
    baker = new_baker(a.shape[1])
    batch = max(1, min(int(view_batch or VIEW_BATCH), max(len(m), 1)))
    for k in range(0, len(m), batch):
        baker.add(m[k:k + batch], fx, fy, cx, cy, a[k:k + batch], None if mask is None else mask[k:k + batch])
    return baker


def bake_vertex_attributes(vertices, triangles, w2c, fx, fy, cx, cy, maps, mask=None, eps=EPS, use_normals=True, view_batch=None,
                           min_weight=MIN_WEIGHT, fallback=None, near=NEAR, far=FAR):
    """Per-vertex averages of the views' attribute maps.  vertices (V, 3), triangles (F, 3), w2c (n, 4, 4) world-to-camera (OpenCV
    convention), maps (n, C, H, W) float32 with 1 <= C <= 8, mask (n, H, W) foreground or None: device tensors; fx, fy, cx, cy the
    pinhole intrinsics of every view.  The mesh's depth is rendered `view_batch` views at a time (default 8) and the sums are
    accumulated across the batches: the result does not depend on the batch size, bit for bit.  use_normals: weigh a view by the
    cosine between the vertex normal and the direction to its camera (and drop back-facing views); else every view weighs 1.
    -> (values (V, C) float32, `fallback` (default 0) where not seen; seen (V,) bool: weight >= min_weight and > 0; weights (V,)
    float64), on the device."""
    new = lambda channels: Baker(vertices, triangles, channels, eps, use_normals, near, far)
    return bake_slices("bake_vertex_attributes", new, w2c, fx, fy, cx, cy, maps, mask, view_batch).finish(min_weight, fallback)


def unit_normal_planes(normal_map):
    """A render's world-space normal_map (3, H, W) normalised per pixel, zero where its length is zero or not finite: the three
    planes a normal-map bake appends to a view's maps."""
    n = normal_map.to(torch.float32)
    length = n.norm(dim=0, keepdim=True)
    return torch.where((length > 0) & torch.isfinite(length), n / length, torch.zeros_like(n))


def material_maps(gaussians, view, metallic=False, normal=False):
    """One view's five material planes and its mask, as gs2m_render.py stores them before the 8-bit packing: the clamped albedo,
    and the roughness and metallic shading_inputs_fused hands to the shading (with `metallic` the model's blended metallic map,
    else the estimate from the roughness that gs2m_render.py stores under metallic/).
    normal: three more planes, unit_normal_planes of the render's normal_map (gs2m_mesh_texture.bake_textures(normal_map=True)).
    -> (maps (5 or 8, H, W) float32, mask (H, W) float32) on the device."""
    from gaussian_renderer import render
    from gs2m_scene import PipelineParams
    from pbr import shading_inputs_fused
    dev = gaussians.get_xyz.device
    with torch.no_grad():
        pkg = render(view, gaussians, PipelineParams(), torch.zeros(3, device=dev), material_stage=True, blend_metallic=metallic)
        h, w = pkg["normal_map"].shape[-2:]
        _, albedo, rough, metal = shading_inputs_fused(pkg["normal_map"], pkg["albedo_map"], pkg["roughness_map"], pkg["alpha_map"],
                                                       pkg["metallic_map"] if metallic else None, 0.04, 1.0)
        maps = torch.empty((8 if normal else 5, h, w), dtype=torch.float32, device=dev)
        maps[0:3] = pkg["albedo_map"].clamp(0.0, 1.0)
        maps[3] = rough.reshape(h, w)
        maps[4] = metal.reshape(h, w)
        if normal:
            maps[5:8] = unit_normal_planes(pkg["normal_map"])
        return maps, pkg["normal_mask"].to(torch.float32).reshape(h, w)


def bake_materials(gaussians, views, mesh, metallic=False, eps=EPS, use_normals=True, view_batch=None, min_weight=MIN_WEIGHT,
                   fallback=FALLBACK, near=NEAR, far=FAR):
    """The model's albedo, roughness and metallic on the vertices of `mesh` (anything with .vertices and .triangles).  Every view is
    rendered with render(..., material_stage=True, blend_metallic=metallic), the render's normal_mask is the foreground, and the
    views are baked in runs of up to `view_batch` (default 8) that share size and intrinsics; nothing leaves the device between
    render and bake.  -> (values (V, 5) float32: albedo rgb, roughness, metallic; seen (V,) bool; weights (V,) float64)."""
    baker = Baker(*_mesh_on_device(mesh, gaussians.get_xyz.device, "bake_materials"), 5, eps, use_normals, near, far)
    bake_runs(baker, views, lambda view: material_maps(gaussians, view, metallic), view_batch)
    return baker.finish(min_weight, fallback)


def bake_runs(baker, views, maps_of, view_batch=None):
    """Adds `views` (cameras of the trainer) to `baker` in runs of up to `view_batch` (default 8) that share size and intrinsics;
    maps_of(view) -> (maps (C, H, W), mask (H, W)) of one view."""
    batch = max(1, int(view_batch or VIEW_BATCH))
    run, key = [], None

    def flush():
        if run:
            # the rasterizer's pixel (i, j) is the ray through (i + 0.5, j + 0.5) of a frame whose principal point is (Cx, Cy), and the
            # bake's texel centres are at integers: the maps are looked up with the principal point (Cx - 0.5, Cy - 0.5)
            _, _, fx, fy, cx, cy = key
            baker.add(torch.stack([r[0] for r in run]), fx, fy, cx - 0.5, cy - 0.5, torch.stack([r[1] for r in run]), torch.stack([r[2] for r in run]))
            run.clear()

    for view in views:
        k = (int(view.image_height), int(view.image_width), float(view.Fx), float(view.Fy), float(view.Cx), float(view.Cy))
        if k != key or len(run) == batch:
            flush()
            key = k
        maps, mask = maps_of(view)
        run.append((view.world_view_transform.transpose(0, 1).to(torch.float64), maps, mask))
    flush()


# ---- files -------------------------------------------------------------------------------------------------------------------

_PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                        ("roughness", "<f4"), ("metallic", "<f4"), ("seen", "u1")])
_PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def _host(t, dtype):
    return np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype)


def write_material_mesh(file, vertices, triangles, values, seen=None, occlusion=None):
    """Binary little-endian PLY: float x y z, uchar red green blue (albedo * 255 rounded to nearest, as gs2m_mesh.write_mesh
    rounds), float roughness, float metallic, uchar seen, int32 face lists.  values (V, 5): albedo rgb, roughness, metallic.
    gs2m_mesh.read_mesh reads the file as a mesh whose vertex colours are the albedo.  occlusion (V,): the ambient occlusion of
    gs2m_mesh_ao.vertex_occlusion (1 = open) as a float property `occlusion` after `seen`; without it the file is byte for byte
    what it was before the property existed."""
    v = _host(vertices, np.float32).reshape(-1, 3)
    t = _host(triangles, np.int32).reshape(-1, 3)
    a = _host(values, np.float32).reshape(-1, 5)
    s = np.ones(len(v), np.uint8) if seen is None else _host(seen, np.uint8).reshape(-1)
    if len(a) != len(v) or len(s) != len(v):
        raise ValueError(f"write_material_mesh: {len(a)} values and {len(s)} flags for {len(v)} vertices")
    ao = None if occlusion is None else _host(occlusion, np.float32).reshape(-1)
    if ao is not None and len(ao) != len(v):
        raise ValueError(f"write_material_mesh: {len(ao)} occlusion values for {len(v)} vertices")
    va = np.zeros(len(v), _PLY_VERTEX if ao is None else np.dtype(_PLY_VERTEX.descr + [("occlusion", "<f4")]))
    if ao is not None:
        va["occlusion"] = ao
    for k, n in enumerate("xyz"):
        va[n] = v[:, k]
    for k, n in enumerate(("red", "green", "blue")):
        va[n] = np.clip(np.rint(a[:, k].astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    va["roughness"], va["metallic"], va["seen"] = a[:, 3], a[:, 4], s
    fa = np.zeros(len(t), _PLY_FACE)
    fa["n"] = 3
    fa["v"] = t
    head = ("ply\nformat binary_little_endian 1.0\ncomment gs2m_mesh_bake material mesh\n"
            f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            "property float roughness\nproperty float metallic\nproperty uchar seen\n" + ("" if ao is None else "property float occlusion\n") +
            f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(str(file), "wb") as f:
        f.write(head.encode("ascii"))
        f.write(va.tobytes())
        f.write(fa.tobytes())


def read_material_mesh(file):
    """-> dict(vertices (V, 3) float32, triangles (F, 3) int32, albedo (V, 3) float32 = the bytes / 255, roughness (V,) float32,
    metallic (V,) float32, seen (V,) bool, and occlusion (V,) float32 where the file has the property).  ValueError, naming what is absent, for a PLY without the material properties."""
    from gs2m_mesh import _ply_columns, _ply_elements
    out = {}
    for name, a, is_list in _ply_elements(file):
        if is_list and name == "face":
            out["triangles"] = a["v"].astype(np.int32)
        elif not is_list and name == "vertex":
            missing = [k for k in ("x", "y", "z", "red", "green", "blue", "roughness", "metallic") if k not in (a.dtype.names or ())]
            if missing:
                raise ValueError(f"{file}: not a material mesh: the vertex properties {', '.join(missing)} are absent "
                                 "(gs2m_mesh_bake.py writes them)")
            out["vertices"], out["albedo"] = _ply_columns(a, "xyz"), _ply_columns(a, ("red", "green", "blue"), 255.0)
            out["roughness"], out["metallic"] = a["roughness"].astype(np.float32), a["metallic"].astype(np.float32)
            out["seen"] = a["seen"].astype(bool) if "seen" in a.dtype.names else np.ones(len(a), bool)
            if "occlusion" in a.dtype.names:
                out["occlusion"] = a["occlusion"].astype(np.float32)
    if "vertices" not in out:
        raise ValueError(f"{file}: no vertex element")
    out.setdefault("triangles", np.zeros((0, 3), np.int32))
    return out


# ---- command line ------------------------------------------------------------------------------------------------------------

def parser():
    ap = argparse.ArgumentParser(description="Bake a trained material model's albedo, roughness and metallic onto the vertices of its mesh")
    ap.add_argument("--ply", required=True, help="the model's point_cloud.ply")
    ap.add_argument("--source-path", "--source_path", "-s", required=True, help="COLMAP-format dataset (or NeRF-synthetic with --blender)")
    ap.add_argument("--mesh", required=True, help="the mesh to bake onto (binary PLY), e.g. tsdf_post.ply")
    ap.add_argument("--output", "-o", required=True, help="the material mesh to write")
    ap.add_argument("--metallic", action="store_true", help="the model's metallic map (default: estimated from the roughness)")
    ap.add_argument("--blender", action="store_true")
    ap.add_argument("--split", choices=("train", "test"), default="train",
                    help="test: transforms_test.json (--blender) or every 8th COLMAP image")
    ap.add_argument("--resolution", "-r", type=int, default=1)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--eps", type=float, default=EPS, help="a vertex is in front when z < depth + eps")
    ap.add_argument("--min-weight", type=float, default=MIN_WEIGHT, help="summed cosines a vertex needs to count as seen")
    ap.add_argument("--view-batch", type=int, default=VIEW_BATCH)
    add_ao_arguments(ap, "a float `occlusion` vertex property")
    from gs2m_ingest import add_ingest_arguments
    add_ingest_arguments(ap)
    return ap


def add_ao_arguments(ap, what):
    """--ao, --ao-rays, --ao-radius of the tools that can trace ambient occlusion (gs2m_mesh_ao.py)"""
    ap.add_argument("--ao", action="store_true", help=f"trace ambient occlusion against the mesh: {what}")
    ap.add_argument("--ao-rays", type=int, default=64, metavar="K", help="rays per point")
    ap.add_argument("--ao-radius", type=float, default=None, metavar="X",
                    help="how far a ray is followed (default: a quarter of the mesh's bounding-box diagonal)")


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
    mesh = M.read_mesh(a.mesh)
    values, seen, _ = bake_materials(model, cams, mesh, a.metallic, eps=a.eps, view_batch=a.view_batch, min_weight=a.min_weight)
    occlusion = None
    if a.ao:
        from gs2m_mesh_ao import vertex_occlusion
        occlusion = vertex_occlusion(mesh, rays=a.ao_rays, radius=a.ao_radius, device=model.get_xyz.device)[1]
    write_material_mesh(a.output, mesh.vertices, mesh.triangles, values, seen, occlusion)
    print(f"[>] {len(cams)} views: {int(seen.sum())} of {len(seen)} vertices seen -> {a.output}")
    return {"out": a.output, "n_views": len(cams), "n_vertices": int(len(seen)), "n_seen": int(seen.sum())}


if __name__ == "__main__":
    main()
