"""Ray casting against a mesh and ambient occlusion (csrc/mesh_bvh.hip; include/gs2m_meshao.h).

A bounding-volume hierarchy over the mesh is built on the device (`build_bvh`); `occluded` answers "is this segment blocked?" for
explicit rays and `closest` "which triangle does it meet first, and where?" (its user: gs2m_mesh_transfer.py); `ambient_occlusion` counts, per point, how many of K cosine-weighted directions about its normal leave the
neighbourhood unblocked.  `vertex_occlusion` works at the vertices of a mesh, `texel_occlusion` at the texels of an atlas, whose
counts `apply_occlusion` writes into the R channel of the ORM image.  The direction tables are data, made on the host
(`direction_table`); every ray is traced by the library, on device tensors owned here; there is no CPU path.
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
from gs2m_eval_util import workspace_for
from gs2m_mesh_cull import _mesh_on_device, _on_device

RAYS, TABLES = 64, 16
RADIUS_SHARE, BIAS_SHARE = 0.25, 1e-4   # of the diagonal of the live vertices' bounding box
BAND_TEXELS = 1 << 20                   # texels per call of texel_occlusion


class Bvh:
    """The hierarchy of one mesh: `buffer` (uint8, the library's layout: include/gs2m_meshao.h) and the mesh it was built over,
    vertices (V, 3) float64 and triangles (F, 3) int32, all on one device."""

    def __init__(self, buffer, vertices, triangles):
        self.buffer, self.vertices, self.triangles = buffer, vertices, triangles

    def nodes(self):
        """The 2 F - 1 nodes as numpy: (lo (m, 3), hi (m, 3) float64, links (m, 4) int32 = left, right, miss, parent)"""
        m = max(2 * len(self.triangles) - 1, 0)
        raw = self.buffer[:64 * m].cpu().numpy().reshape(m, 64)
        box = raw[:, :48].copy().view(np.float64).reshape(m, 6)
        return box[:, :3], box[:, 3:], raw[:, 48:].copy().view(np.int32).reshape(m, 4)

    def _args(self):
        return (_ptr(self.buffer), self.buffer.numel(), len(self.vertices), _ptr(self.vertices), len(self.triangles), _ptr(self.triangles))


def build_bvh(vertices, triangles):
    """The hierarchy of the mesh vertices (V, 3), triangles (F, 3), device tensors -> Bvh.  F = 0 is valid: nothing is hit."""
    who = "build_bvh"
    v = _on_device(vertices, "vertices", who, torch.float64, (3,))
    f = _on_device(triangles, "triangles", who, torch.int32, (3,))
    buf = workspace_for("gs2m_bvh_bytes", v.device, len(f))
    N.launch("gs2m_bvh_build", v.device, len(v), _ptr(v), len(f), _ptr(f), _ptr(buf), buf.numel())
    return Bvh(buf, v, f)


def _rays(who, origins, dirs, skip):
    """The checked device tensors of a ray query -> (origins, dirs, skip or None)"""
    o = _on_device(origins, "origins", who, torch.float64, (3,))
    d = _on_device(dirs, "dirs", who, torch.float64, (3,))
    if len(o) != len(d):
        raise RuntimeError(f"{who}: {len(o)} origins for {len(d)} directions")
    sk = None if skip is None else _on_device(skip, "skip", who, torch.int32, ())
    if sk is not None and len(sk) != len(o):
        raise RuntimeError(f"{who}: {len(sk)} skip ids for {len(o)} rays")
    return o, d, sk


def occluded(bvh, origins, dirs, tmin=0.0, tmax=math.inf, skip=None):
    """Per ray: does origin + t dir, tmin < t <= tmax, hit a triangle other than skip[ray]?  origins, dirs (n, 3); skip (n,) int32
    triangle ids (negative: none) or None -> (n,) bool on the device."""
    o, d, sk = _rays("occluded", origins, dirs, skip)
    hit = torch.zeros(len(o), dtype=torch.uint8, device=o.device)
    N.launch("gs2m_bvh_occluded", o.device, *bvh._args(), len(o), _ptr(o), _ptr(d), float(tmin), float(tmax), _ptr(sk), _ptr(hit))
    return hit.bool()


def closest(bvh, origins, dirs, tmin=0.0, tmax=math.inf, skip=None, facing=0):
    """Per ray the nearest triangle other than skip[ray] that origin + t dir meets with tmin <= t <= tmax (closed at both ends: a
    ray that starts on the surface finds it), the smallest index among equal t.  facing: 0 both sides, +1 only the side the
    triangle's cross(e1, e2) points out of, -1 only the other.  -> (tri (n,) int32, -1 for a miss; t (n,) float64, inf for a miss;
    uv (n, 2) float64: the hit point is (1 - u - v) a + u b + v c) on the device."""
    o, d, sk = _rays("closest", origins, dirs, skip)
    tri = torch.full((len(o),), -1, dtype=torch.int32, device=o.device)
    t = torch.full((len(o),), math.inf, dtype=torch.float64, device=o.device)
    uv = torch.zeros((len(o), 2), dtype=torch.float64, device=o.device)
    N.launch("gs2m_bvh_closest", o.device, *bvh._args(), len(o), _ptr(o), _ptr(d), float(tmin), float(tmax), _ptr(sk), int(facing), _ptr(tri),
             _ptr(t), _ptr(uv))
    return tri, t, uv


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


def live_diagonal(vertices, triangles):
    """The diagonal of the bounding box of the vertices that live triangles (indices in range, finite corners) reference; 0.0
    without one"""
    v, f = vertices, triangles.long()
    if len(f) == 0 or len(v) == 0:
        return 0.0
    ok = ((f >= 0) & (f < len(v))).all(1)
    f = f[ok]
    ok = torch.isfinite(v[f.reshape(-1)]).reshape(len(f), -1).all(1)
    p = v[f[ok].reshape(-1)]
    if len(p) == 0:
        return 0.0
    return float((p.max(0).values - p.min(0).values).norm())


def _unit(n):
    """Rows of n normalised in torch fp64; a zero or non-finite row stays as it is (the library gives such a point K)"""
    length = ((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).sqrt()[:, None]
    return torch.where((length > 0) & torch.isfinite(length), n / length, n)


class _Sampler:
    """The resolved parameters of an ambient-occlusion pass and its direction table on the device"""

    def __init__(self, bvh, rays, tables, radius, bias, seed):
        diag = live_diagonal(bvh.vertices, bvh.triangles) if radius is None or bias is None else 0.0
        self.bvh, self.rays, self.tables, self.seed = bvh, int(rays), int(tables), int(seed)
        self.radius = RADIUS_SHARE * diag if radius is None else float(radius)
        self.bias = BIAS_SHARE * diag if bias is None else float(bias)
        self.dirs = torch.as_tensor(direction_table(rays, tables, seed)).to(bvh.vertices.device)

    def visible(self, points, normals, skip, index0=0):
        who = "ambient_occlusion"
        p = _on_device(points, "points", who, torch.float64, (3,))
        n = _unit(_on_device(normals, "normals", who, torch.float64, (3,))).contiguous()
        if len(p) != len(n):
            raise RuntimeError(f"{who}: {len(p)} points for {len(n)} normals")
        sk = None if skip is None else _on_device(skip, "skip", who, torch.int32, ())
        if sk is not None and len(sk) != len(p):
            raise RuntimeError(f"{who}: {len(sk)} skip ids for {len(p)} points")
        out = torch.full((len(p),), self.rays, dtype=torch.int32, device=p.device)
        N.launch("gs2m_bvh_ao", p.device, *self.bvh._args(), len(p), _ptr(p), _ptr(n), _ptr(sk), self.tables, self.rays, _ptr(self.dirs),
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


def texel_points(atlas, row0=0, n_rows=None):
    """What texel_occlusion traces from, for rows row0 .. row0 + n_rows of the atlas -> (owner (n, W) int32, points (n, W, 3),
    normals (n, W, 3) float64): the normal is the owner's face normal turned to the side of the texel's interpolated vertex
    normal, so that a coarse mesh does not shadow itself through its own shading normals"""
    from gs2m_mesh_texture import atlas_texels
    from gs2m_mesh_view import vertex_normals
    vn = vertex_normals(atlas.vertices, atlas.triangles)[0] if len(atlas.triangles) else None
    owner, _, points, tn = atlas_texels(atlas, vn, row0, n_rows)
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
    rows = max(1, int(band_texels) // max(a.width, 1))
    vis, own = [], []
    for row0 in range(0, a.height, rows):
        owner, points, normals = texel_points(a, row0, min(rows, a.height - row0))
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

