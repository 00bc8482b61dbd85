"""numpy restatement of the closest-hit query of include/gs2m_meshao.h (Candidate, Facing, Answer) and of
include/gs2m_meshtransfer.h: the brute-force loop over all triangles with the closed range, the facing rule, the skip, the dead
triangles and the (t, index) order, and the transfer's two rays, its choice and its interpolation with the one rounding to float.
fp64, one ufunc per operation of the headers, so the device gives the same bits.  The products, the meshes and the ray families are
those of tests/mesh_ao_ref.py; the traversal has no restatement: its answer is defined as the loop's."""
import numpy as np

import mesh_ao_ref as A


def triangle_table(vertices, triangles, origins, dirs, tmin=0.0, tmax=np.inf):
    """Every ray against every triangle, the Candidate paragraph with facing = 0 and no skip -> (ok (n_rays, F) bool; t, u, v,
    det (n_rays, F) float64, defined where ok).  `select` narrows ok by facing and skip, `answer` picks the winner: a test that
    needs several facings of one set of rays pays for the products once."""
    ok, t, u, v, det = A.triangle_table(vertices, triangles, origins, dirs)
    return ok & A.in_range(t, tmin, tmax, True), t, u, v, det


def select(ok, det, skip=None, facing=0):
    """The Facing paragraph and the skip rule on a copy of triangle_table's ok"""
    if facing not in (0, 1, -1):
        raise ValueError("facing")
    ok = ok.copy()
    with np.errstate(all="ignore"):
        if facing > 0:
            ok &= det > 0
        elif facing < 0:
            ok &= det < 0
    return A.without_skipped(ok, skip)


def answer(ok, t, u, v):
    """The Answer paragraph -> (tri (n,) int32, t (n,) float64, uv (n, 2) float64, ties (n,) int: how many candidates share the
    best t)"""
    n = len(ok)
    tri, best, uv, ties = np.full(n, -1, np.int32), np.full(n, np.inf), np.zeros((n, 2)), np.zeros(n, np.int64)
    if ok.shape[1] == 0:
        return tri, best, uv, ties
    tt = np.where(ok, t, np.inf)
    low = tt.min(1)
    first = ok & (tt == low[:, None])          # the candidates at the smallest t; argmax: the smallest index among them
    ties = first.sum(1)
    hit = np.nonzero(ok.any(1))[0]
    k = first[hit].argmax(1)
    tri[hit], best[hit] = k, t[hit, k]
    uv[hit, 0], uv[hit, 1] = u[hit, k], v[hit, k]
    return tri, best, uv, ties


def closest(vertices, triangles, origins, dirs, tmin=0.0, tmax=np.inf, skip=None, facing=0):
    """gs2m_bvh_closest by the loop over all triangles -> answer's four"""
    ok, t, u, v, det = triangle_table(vertices, triangles, origins, dirs, tmin, tmax)
    return answer(select(ok, det, skip, facing), t, u, v)


def transfer(vertices, triangles, points, normals, owner, distance, two_sided, values, attributes=None, src_normals=None,
             want_normal=False):
    """gs2m_meshtransfer.h on a copy of values (n, stride) float32 -> (values, hit (n,) int32, offset (n,) float64, outcome (n,)
    int8: 0 skipped, 1 miss, 2 forward, 3 backward)"""
    v, f = np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(triangles).reshape(-1, 3).astype(np.int64)
    p, n = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    out = np.array(values, np.float32).copy()
    assert out.ndim == 2 and len(out) == len(p)
    hit, offset, outcome = np.full(len(p), -1, np.int32), np.zeros(len(p)), np.zeros(len(p), np.int8)
    with np.errstate(all="ignore"):
        nn = A.dot(n, n)
    walk = (nn > 0) & np.isfinite(nn) & np.isfinite(p).all(1)
    if owner is not None:
        walk &= np.asarray(owner).reshape(-1) >= 0
    rows = np.nonzero(walk)[0]
    if len(rows) == 0:
        return out, hit, offset, outcome
    ft, tf, uvf, _ = closest(v, f, p[rows], n[rows], 0.0, distance, None, 0 if two_sided else -1)
    bt, tb, uvb, _ = closest(v, f, p[rows], -n[rows], 0.0, distance, None, 0 if two_sided else 1)
    back = (bt >= 0) & ((ft < 0) | (tb < tf))
    tri = np.where(back, bt, ft)
    uv = np.where(back[:, None], uvb, uvf)
    outcome[rows] = np.where(tri < 0, 1, np.where(back, 3, 2))
    got = tri >= 0
    rows, tri, uv, back, tf, tb = rows[got], tri[got], uv[got], back[got], tf[got], tb[got]
    hit[rows] = tri
    offset[rows] = np.where(back, -tb, tf)
    i0, i1, i2 = f[tri, 0], f[tri, 1], f[tri, 2]
    u, w2 = uv[:, 0:1], uv[:, 1:2]
    w = (1.0 - u) - w2
    mix = lambda x: ((w * x[i0].astype(np.float64) + u * x[i1].astype(np.float64)) + w2 * x[i2].astype(np.float64)).astype(np.float32)
    channels = 0
    if attributes is not None:
        att = np.asarray(attributes, np.float32)
        channels = att.shape[1]
        out[rows, :channels] = mix(att)
    if want_normal:
        if src_normals is not None:
            out[rows, channels:channels + 3] = mix(np.asarray(src_normals, np.float64))
        else:
            out[rows, channels:channels + 3] = A.cross(v[i1] - v[i0], v[i2] - v[i0]).astype(np.float32)
    return out, hit, offset, outcome


# ---- scenes and ray families of the closest-hit tests -------------------------------------------------------------------------

def layered_grid(m=8):
    """A.grid_mesh with every triangle a second time, in reversed order: two coplanar layers, so every hit has a twin at the same
    t whose index is larger, and the twin comes first in half of the tree's leaves"""
    v, f = A.grid_mesh(m)
    return v, np.concatenate([f, f[::-1]]).astype(np.int32)


def tie_family(n, seed=0, m=8):
    """Axis-aligned dyadic rays onto the floor (z = 0.5) and the wall (x = 0.5) of the grid, aimed at lattice vertices, at
    points of lattice edges (the diagonals included) and into the interior: up to six triangles meet at a vertex, two at an edge,
    and the arithmetic is exact, so they share their t to the bit"""
    rng = np.random.default_rng([seed, n, 77])
    g = 4 * m                                                    # a quarter of a cell
    a, b = rng.integers(-g // 4, g + g // 4 + 1, n) / g, rng.integers(-g // 4, g + g // 4 + 1, n) / g   # a quarter falls beside the mesh
    on_diagonal = rng.random(n) < 0.25                           # x + y on a lattice line: the quads' diagonals
    b = np.where(on_diagonal, np.round((a + b) * m) / m - a, b)
    start = rng.choice([0.0, 1.0, 0.25, 2.0], n)
    sign = np.where(start < 0.5, 1.0, -1.0)
    floor = rng.random(n) < 0.5
    o = np.where(floor[:, None], np.stack([a, b, start], 1), np.stack([start, a, b], 1))
    d = np.where(floor[:, None], np.stack([0 * a, 0 * a, sign], 1), np.stack([sign, 0 * a, 0 * a], 1)) * rng.choice([0.5, 1.0, 2.0], (n, 1))
    return dict(origins=o, dirs=d, tmin=0.0, tmax=np.inf, skip=None)


# The transfer scene: the source is A.height_field() (z between -0.15 and 0.2, wound to +z), the target a tilted plane through it.
# The plane's height and the distance are chosen so that the source lies above the plane within the distance, below it within the
# distance, and further away than the distance over comparable shares of the plane (test_transfer_scene_has_every_outcome).
TRANSFER_HEIGHT, TRANSFER_SLOPE, TRANSFER_DISTANCE = 0.025, 0.04, 0.06


def tilted_plane(nx=4, ny=2):
    """2 nx ny triangles of the plane z = TRANSFER_HEIGHT + TRANSFER_SLOPE (x - 1.25) over [0.1, 2.4] x [0.1, 0.9], wound to +z"""
    x, y = np.meshgrid(0.1 + 2.3 * np.arange(nx + 1) / nx, 0.1 + 0.8 * np.arange(ny + 1) / ny, indexing="ij")
    v = np.stack([x, y, TRANSFER_HEIGHT + TRANSFER_SLOPE * (x - 1.25)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    q = (i * (ny + 1) + j).reshape(-1)
    f = np.concatenate([np.stack([q, q + ny + 1, q + 1], 1), np.stack([q + 1, q + ny + 1, q + ny + 2], 1)]).astype(np.int32)
    return v, f


def tilted_plane_samples(n, seed=0):
    """n random points of that plane and its unit normal -> (points, normals)"""
    rng = np.random.default_rng([seed, n])
    xy = np.stack([0.1 + 2.3 * rng.random(n), 0.1 + 0.8 * rng.random(n)], 1)
    return (np.concatenate([xy, TRANSFER_HEIGHT + TRANSFER_SLOPE * (xy[:, :1] - 1.25)], 1),
            A.unit_rows(np.tile([-TRANSFER_SLOPE, 0.0, 1.0], (n, 1))))


def half_flipped(triangles):
    """every second triangle wound the other way"""
    f = np.array(triangles, np.int32)
    f[::2] = f[::2][:, [0, 2, 1]]
    return f


def nearest_skip(r, nearest):
    """The skip list of a family's "with skip" run: the family's own where it has one, else each ray's nearest triangle under
    facing 0 (`nearest`: answer's tri), so that the second one decides"""
    return np.asarray(r["skip"] if r["skip"] is not None else nearest, np.int32)


# (mesh, facing, with skip) -> the families of A.FAMILIES / A.GRID_FAMILIES, at 1000 rays, whose hit share under the restatement
# alone lies in 0.1 .. 0.9: every combination of mesh, family, facing and skip was measured on the CPU and the ones that hold the
# bound are listed (tests/test_mesh_transfer.py checks each entry; the GPU test runs them all).  The meshes' winding is random, so
# +1 and -1 roughly halve the hits of 0, and a skipped nearest triangle leaves the tiny meshes and the grazing rays with too few.
BALANCED = {
    ("n1", 0, False): ('random', 'axis1', 'axis2', 'short', 'far', 'grazing'),
    ("n1", 1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'grazing'),
    ("n1", -1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'grazing'),
    ("n2", 0, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n2", 0, True): ('random', 'far', 'skip'),
    ("n2", 1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n2", -1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n2", 1, True): ('skip',),
    ("n3", 0, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n3", 1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n3", -1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n3", 0, True): ('axis2', 'far', 'skip'),
    ("n64", 0, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n64", 0, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip'),
    ("n64", 1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n64", 1, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip'),
    ("n64", -1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n64", -1, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip'),
    ("n65", 0, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n65", 0, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip'),
    ("n65", 1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n65", 1, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip'),
    ("n65", -1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n65", -1, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip'),
    ("n1000", 0, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n1000", 0, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n1000", 1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n1000", 1, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n1000", -1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("n1000", -1, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("identical257", 0, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("identical257", 0, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("identical257", 1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("identical257", 1, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("identical257", -1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("identical257", -1, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("collinear200", 0, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("collinear200", 0, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip'),
    ("collinear200", 1, False): ('random', 'axis1', 'short', 'far', 'skip', 'grazing'),
    ("collinear200", 1, True): ('random', 'axis1', 'short', 'far', 'skip'),
    ("collinear200", -1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("collinear200", -1, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip'),
    ("dead100", 0, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("dead100", 0, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip'),
    ("dead100", 1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("dead100", 1, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip'),
    ("dead100", -1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing'),
    ("dead100", -1, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip'),
    ("grid", 0, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing', 'faces', 'tmax'),
    ("grid", 0, True): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'tmax'),
    ("grid", 1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing', 'faces'),
    ("grid", 1, True): ('random', 'axis1', 'far', 'skip'),
    ("grid", -1, False): ('random', 'axis1', 'axis2', 'short', 'far', 'skip', 'grazing', 'faces', 'tmax'),
    ("grid", -1, True): ('random', 'far', 'skip', 'tmax'),
}
