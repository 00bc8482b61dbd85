"""Ray casting against a mesh (csrc/mesh_bvh.hip; include/gs2m_meshao.h).

A bounding-volume hierarchy over the mesh is built on the device (`build_bvh`); `occluded` answers "is this segment blocked?" for
explicit rays and `closest` "which triangle does it meet first, and where?".  What the users of the hierarchy share is here too:
the check of their per-row arguments (`checked_rows`), `unit_rows`, `live_diagonal`, and the walk over the texels of an atlas
(`bands`, `texels`).  The users: gs2m_mesh_ao.py (ambient occlusion) and gs2m_mesh_transfer.py (detail transfer).  Every ray is
traced by the library, on device tensors owned here; there is no CPU path.
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
from gs2m_mesh_cull import _on_device

BAND_TEXELS = 1 << 20                   # texels of an atlas per call of the library


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

    def args(self):
        """The leading arguments of every query of the library"""
        return (_ptr(self.buffer), self.buffer.numel(), len(self.vertices), _ptr(self.vertices), len(self.triangles), _ptr(self.triangles))


def build_bvh(vertices, triangles):
    """The hierarchy of the mesh vertices (V, 3), triangles (F, 3), device tensors -> Bvh.  F = 0 is valid: nothing is hit."""
    who = "build_bvh"
    v = _on_device(vertices, "vertices", who, torch.float64, (3,))
    f = _on_device(triangles, "triangles", who, torch.int32, (3,))
    buf = workspace_for("gs2m_bvh_bytes", v.device, len(f))
    N.launch("gs2m_bvh_build", v.device, len(v), _ptr(v), len(f), _ptr(f), _ptr(buf), buf.numel())
    return Bvh(buf, v, f)


# what checked_rows calls a query's three per-row arguments, and the nouns of its messages: "N <first> for M <second>",
# "N <ids> for M <rows>"
RAY_ROWS = (("origins", "dirs", "skip"), ("origins", "directions", "skip ids", "rays"))
SKIP_ROWS = (("points", "normals", "skip"), ("points", "normals", "skip ids", "points"))
OWNER_ROWS = (("points", "normals", "owner"), ("points", "normals", "owners", "points"))


def checked_rows(who, words, first, second, ids=None):
    """The checked device tensors of a query's rows: `first`, `second` (n, 3) float64 and `ids` (n,) int32 or None, of equal
    length; words: RAY_ROWS, SKIP_ROWS or OWNER_ROWS -> (first, second, ids or None)"""
    names, nouns = words
    a = _on_device(first, names[0], who, torch.float64, (3,))
    b = _on_device(second, names[1], who, torch.float64, (3,))
    if len(a) != len(b):
        raise RuntimeError(f"{who}: {len(a)} {nouns[0]} for {len(b)} {nouns[1]}")
    i = None if ids is None else _on_device(ids, names[2], who, torch.int32, ())
    if i is not None and len(i) != len(a):
        raise RuntimeError(f"{who}: {len(i)} {nouns[2]} for {len(a)} {nouns[3]}")
    return a, b, i


def occluded(bvh, origins, dirs, tmin=0.0, tmax=math.inf, skip=None):
    """Per ray: does origin + t dir, tmin < t <= tmax, hit a triangle other than skip[ray]?  origins, dirs (n, 3); skip (n,) int32
    triangle ids (negative: none) or None -> (n,) bool on the device."""
    o, d, sk = checked_rows("occluded", RAY_ROWS, origins, dirs, skip)
    hit = torch.zeros(len(o), dtype=torch.uint8, device=o.device)
    N.launch("gs2m_bvh_occluded", o.device, *bvh.args(), len(o), _ptr(o), _ptr(d), float(tmin), float(tmax), _ptr(sk), _ptr(hit))
    return hit.bool()


def closest(bvh, origins, dirs, tmin=0.0, tmax=math.inf, skip=None, facing=0):
    """Per ray the nearest triangle other than skip[ray] that origin + t dir meets with tmin <= t <= tmax (closed at both ends: a
    ray that starts on the surface finds it), the smallest index among equal t.  facing: 0 both sides, +1 only the side the
    triangle's cross(e1, e2) points out of, -1 only the other.  -> (tri (n,) int32, -1 for a miss; t (n,) float64, inf for a miss;
    uv (n, 2) float64: the hit point is (1 - u - v) a + u b + v c) on the device."""
    o, d, sk = checked_rows("closest", RAY_ROWS, origins, dirs, skip)
    tri = torch.full((len(o),), -1, dtype=torch.int32, device=o.device)
    t = torch.full((len(o),), math.inf, dtype=torch.float64, device=o.device)
    uv = torch.zeros((len(o), 2), dtype=torch.float64, device=o.device)
    N.launch("gs2m_bvh_closest", o.device, *bvh.args(), len(o), _ptr(o), _ptr(d), float(tmin), float(tmax), _ptr(sk), int(facing), _ptr(tri),
             _ptr(t), _ptr(uv))
    return tri, t, uv


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


def unit_rows(n):
    """Rows of n normalised in torch fp64; a zero or non-finite row stays as it is (the library casts no ray from such a point)"""
    length = ((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).sqrt()[:, None]
    return torch.where((length > 0) & torch.isfinite(length), n / length, n)


def bands(atlas, band_texels=BAND_TEXELS):
    """The atlas in bands of whole rows, at most band_texels texels each and one row at the least -> (row0, n_rows) of each"""
    rows = max(1, int(band_texels) // max(atlas.width, 1))
    for row0 in range(0, atlas.height, rows):
        yield row0, min(rows, atlas.height - row0)


def atlas_normals(atlas):
    """The vertex normals of the atlas's mesh (gs2m_mesh_view.vertex_normals), which a walk over `bands` computes once; None
    for a mesh without a triangle"""
    if not len(atlas.triangles):
        return None
    from gs2m_mesh_view import vertex_normals
    return vertex_normals(atlas.vertices, atlas.triangles)[0]


def texels(atlas, vertex_normals=None, row0=0, n_rows=None):
    """Rows row0 .. row0 + n_rows of the atlas as points of its mesh (gs2m_mesh_texture.atlas_texels, what the texel bake sees)
    -> (owner (n, W) int32, -1 where empty; points (n, W, 3); the interpolated vertex normals (n, W, 3) float64, not normalised).
    vertex_normals: atlas_normals(atlas), where the caller has them."""
    from gs2m_mesh_texture import atlas_texels
    owner, _, points, tn = atlas_texels(atlas, atlas_normals(atlas) if vertex_normals is None else vertex_normals, row0, n_rows)
    return owner, points, tn
