"""Ambient occlusion of a mesh (csrc/mesh_bvh.hip; include/gs2m_meshao.h).

Against a hierarchy of the mesh (gs2m_mesh_bvh.build_bvh), `ambient_occlusion` counts, per point, how many of K cosine-weighted
directions about its normal leave the neighbourhood unblocked.  `vertex_occlusion` works at the vertices of a mesh,
`texel_occlusion` at the texels of an atlas, whose counts `apply_occlusion` writes into the R channel of the ORM image.  The
direction tables are data, made on the host (`direction_table`); every ray is traced by the library, on device tensors owned
here; there is no CPU path.
"""
import math
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np
import torch

import gs2m_native as N
from gs2m_eval_util import ptr as _ptr
from gs2m_mesh_bvh import BAND_TEXELS, SKIP_ROWS, atlas_normals, bands, build_bvh, checked_rows, live_diagonal, texels, unit_rows
from gs2m_mesh_bvh import Bvh, closest, occluded  # noqa: F401  (the ray casting lived here before gs2m_mesh_bvh.py: callers of then find it still)
from gs2m_mesh_bvh import unit_rows as _unit  # noqa: F401  (likewise)
from gs2m_mesh_cull import _mesh_on_device, _on_device

RAYS, TABLES = 64, 16
RADIUS_SHARE, BIAS_SHARE = 0.25, 1e-4   # of the diagonal of the live vertices' bounding box


def direction_table(rays, tables, seed=0):
    """(tables, rays, 3) float64 numpy: `rays` cosine-weighted directions of the hemisphere about +z, stratified -- one per cell of
    an nu x nv grid over the unit square (nu nv >= rays, the first `rays` cells of a permutation), jittered in its cell, through
    Malley's map (a uniform disk sample lifted to the hemisphere) -- and `tables` copies of that set, copy r rotated about z by a
    jittered share of the full turn.  Rows are renormalised in fp64: unit to 1e-15.  Computed on the host: the table is data."""
    K, R = int(rays), int(tables)
    if K < 1 or R < 1:
        raise ValueError("direction_table: `rays` and `tables` must be at least 1")
    rng = np.random.default_rng([int(seed), K, R])
    nu = int(math.ceil(math.sqrt(K)))
    nv = (K + nu - 1) // nu
    cells = rng.permutation(nu * nv)[:K]
    u = ((cells % nu) + rng.random(K)) / nu
    v = ((cells // nu) + rng.random(K)) / nv
    r, phi = np.sqrt(u), 2.0 * np.pi * v
    z = np.sqrt(np.maximum(1.0 - u, 0.0))
    z = np.maximum(z, 1e-3)  # l_z > 0: no ray runs in the tangent plane
    base = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)
    ang = 2.0 * np.pi * (np.arange(R) + np.concatenate([[0.0], rng.random(R - 1)])) / R
    c, s = np.cos(ang)[:, None], np.sin(ang)[:, None]
    out = np.stack([c * base[None, :, 0] - s * base[None, :, 1], s * base[None, :, 0] + c * base[None, :, 1],
                    np.broadcast_to(base[None, :, 2], (R, K))], 2)
    for _ in range(2):
        out = out / np.sqrt((out * out).sum(2, keepdims=True))
    return np.ascontiguousarray(out, np.float64)


class _Sampler:
    """The resolved parameters of an ambient-occlusion pass and its direction table on the device"""

    def __init__(self, bvh, rays, tables, radius, bias, seed):
        diag = live_diagonal(bvh.vertices, bvh.triangles) if radius is None or bias is None else 0.0
        self.bvh, self.rays, self.tables, self.seed = bvh, int(rays), int(tables), int(seed)
        self.radius = RADIUS_SHARE * diag if radius is None else float(radius)
        self.bias = BIAS_SHARE * diag if bias is None else float(bias)
        self.dirs = torch.as_tensor(direction_table(rays, tables, seed)).to(bvh.vertices.device)

    def visible(self, points, normals, skip, index0=0):
        p, n, sk = checked_rows("ambient_occlusion", SKIP_ROWS, points, normals, skip)
        n = unit_rows(n).contiguous()
        out = torch.full((len(p),), self.rays, dtype=torch.int32, device=p.device)
        N.launch("gs2m_bvh_ao", p.device, *self.bvh.args(), len(p), _ptr(p), _ptr(n), _ptr(sk), self.tables, self.rays, _ptr(self.dirs),
                 self.bias, self.radius, int(index0), self.seed, _ptr(out))
        return out


def ambient_occlusion(bvh, points, normals, skip=None, rays=RAYS, tables=TABLES, radius=None, bias=None, seed=0, index0=0):
    """Per point the number of `rays` cosine-weighted directions about its normal that reach `radius` unblocked.  points, normals
    (n, 3) device tensors (the normals are normalised here, in fp64); skip (n,) int32: the triangle a point lies on, which its
    rays ignore, negative for "no point here" (such a point gets `rays`).  radius, bias default to 0.25 and 1e-4 of the diagonal
    of the live vertices' bounding box; radius may be inf.  Point p uses table mix32(index0 + p + seed) % tables.
    -> (visible (n,) int32, ao (n,) float32 = visible / rays)"""
    vis = _Sampler(bvh, rays, tables, radius, bias, seed).visible(points, normals, skip, index0)
    return vis, (vis.to(torch.float64) / int(rays)).to(torch.float32)


def vertex_occlusion(mesh, rays=RAYS, tables=TABLES, radius=None, bias=None, seed=0, device="cuda", bvh=None):
    """Ambient occlusion at the vertices of `mesh` (anything with .vertices and .triangles) along its vertex normals
    (gs2m_mesh_view.vertex_normals), no triangle skipped -> (visible (V,) int32, ao (V,) float32)"""
    from gs2m_mesh_view import vertex_normals
    v, f = _mesh_on_device(mesh, device, "vertex_occlusion")
    bvh = build_bvh(v, f) if bvh is None else bvh
    return ambient_occlusion(bvh, v, vertex_normals(v, f)[0], None, rays, tables, radius, bias, seed)


def texel_points(atlas, row0=0, n_rows=None, vertex_normals=None):
    """What texel_occlusion traces from, for rows row0 .. row0 + n_rows of the atlas (gs2m_mesh_bvh.texels) -> (owner (n, W) int32,
    points (n, W, 3), normals (n, W, 3) float64): the normal is the owner's face normal turned to the side of the texel's
    interpolated vertex normal, so that a coarse mesh does not shadow itself through its own shading normals"""
    owner, points, tn = texels(atlas, vertex_normals, row0, n_rows)
    if len(atlas.triangles) == 0:
        return owner, points, torch.zeros_like(tn)
    f = atlas.triangles.long()[owner.clamp(min=0).long()]                 # (n, W, 3)
    inside = ((f >= 0) & (f < len(atlas.vertices))).all(-1, keepdim=True)
    p = atlas.vertices[f.clamp(0, max(len(atlas.vertices) - 1, 0))]       # (n, W, 3, 3)
    face = torch.linalg.cross(p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 0, :])
    side = ((face[..., 0] * tn[..., 0] + face[..., 1] * tn[..., 1]) + face[..., 2] * tn[..., 2])[..., None]
    face = torch.where(side < 0, -face, face)
    return owner, points, torch.where(inside, face, torch.zeros_like(face))


def texel_occlusion(atlas, rays=RAYS, tables=TABLES, radius=None, bias=None, seed=0, bvh=None, band_texels=BAND_TEXELS):
    """Ambient occlusion at the texels of `atlas` (gs2m_mesh_texture.build_atlas), each texel skipping its own triangle, empty
    texels left at `rays`; the atlas goes through the library in bands of whole rows, texel index = index0 + p, so the result does
    not depend on the band -> (visible (H, W) int32, owner (H, W) int32)"""
    a = atlas
    bvh = build_bvh(a.vertices, a.triangles) if bvh is None else bvh
    sampler = _Sampler(bvh, rays, tables, radius, bias, seed)
    vn = atlas_normals(a)
    vis, own = [], []
    for row0, n_rows in bands(a, band_texels):
        owner, points, normals = texel_points(a, row0, n_rows, vn)
        vis.append(sampler.visible(points.reshape(-1, 3), normals.reshape(-1, 3), owner.reshape(-1), row0 * a.width).reshape(owner.shape))
        own.append(owner)
    if not vis:
        z = torch.zeros((0, a.width), dtype=torch.int32, device=a.vertices.device)
        return z, z.clone()
    return torch.cat(vis), torch.cat(own)


def apply_occlusion(orm, owner, visible, rays):
    """R of the ORM image (H, W, 3) uint8 <- floor(255 visible / rays + 0.5) at owned texels, in place; G, B and empty texels stay"""
    who = "apply_occlusion"
    if not torch.is_tensor(orm) or not orm.is_cuda or orm.dtype != torch.uint8 or not orm.is_contiguous() or orm.shape[-1] != 3:
        raise RuntimeError(f"{who}: `orm` must be a contiguous (H, W, 3) uint8 tensor on a HIP device; there is no CPU path")
    ow = _on_device(owner, "owner", who, torch.int32, ())
    vi = _on_device(visible, "visible", who, torch.int32, ())
    if not len(ow) == len(vi) == orm.numel() // 3:
        raise RuntimeError(f"{who}: {len(ow)} owners and {len(vi)} counts for {orm.numel() // 3} texels")
    N.launch("gs2m_texture_occlusion", orm.device, len(ow), _ptr(ow), _ptr(vi), int(rays), _ptr(orm))
    return orm

