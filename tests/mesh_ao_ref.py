"""numpy restatement of include/gs2m_meshao.h: the triangle test, the brute-force any-hit loop, mix32, the Duff frame, the
ambient-occlusion count and the ORM byte.  fp64, one ufunc per operation of the header (numpy fuses nothing), so the device gives
the same bits.  The traversal has no restatement: its answer is defined as the loop's."""
import numpy as np


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def triangle_tuv(o, d, a, b, c):
    """The Triangle paragraph up to t, broadcasting: o, d (..., 3) rays against a, b, c (..., 3) corners -> (ok: what det, u and v
    say, before any range of t; t, u, v, det, computed whatever ok says)"""
    o, d, a, b, c = (np.asarray(x, np.float64) for x in (o, d, a, b, c))
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        P = cross(d, e2)
        det = dot(e1, P)
        ok = (det != 0) & np.isfinite(det)
        T = o - a
        u = dot(T, P) / det
        ok &= (u >= 0) & (u <= 1)
        Q = cross(T, e1)
        v = dot(d, Q) / det
        ok &= (v >= 0) & (u + v <= 1)
        t = dot(e2, Q) / det
    return ok, t, u, v, det


def in_range(t, tmin, tmax, closed):
    """tmin < t <= tmax of the any-hit query; closed: tmin <= t <= tmax of the closest-hit query"""
    with np.errstate(all="ignore"):
        return ((t >= tmin) if closed else (t > tmin)) & (t <= tmax)


def triangle_hits(o, d, a, b, c, tmin, tmax):
    """The Triangle paragraph, broadcasting -> bool"""
    ok, t = triangle_tuv(o, d, a, b, c)[:2]
    return ok & in_range(t, tmin, tmax, False)


def hit_parameter(o, d, a, b, c):
    """t of the Triangle paragraph (whatever u and v say), for building rays that end exactly on a triangle"""
    return triangle_tuv(o, d, a, b, c)[1]


def live_triangles(vertices, triangles):
    """The Dead paragraph -> (F,) bool"""
    v, f = np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(triangles).reshape(-1, 3).astype(np.int64)
    ok = ((f >= 0) & (f < len(v))).all(1)
    fin = np.zeros(len(f), bool)
    if len(v):
        fin[ok] = np.isfinite(v[f[ok]]).all((1, 2))
    return ok & fin


def triangle_table(vertices, triangles, origins, dirs):
    """triangle_tuv of every ray against every triangle -> (ok (n_rays, F) bool, false for a dead triangle; t, u, v, det
    (n_rays, F) float64, NaN for a dead triangle)"""
    v, f = np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(triangles).reshape(-1, 3).astype(np.int64)
    o, d = np.asarray(origins, np.float64).reshape(-1, 3), np.asarray(dirs, np.float64).reshape(-1, 3)
    live = live_triangles(v, f)
    ok = np.zeros((len(o), len(f)), bool)
    t, u, w, det = (np.full((len(o), len(f)), np.nan) for _ in range(4))
    if not live.any() or len(o) == 0:
        return ok, t, u, w, det
    p = v[f[live]]
    for r0 in range(0, len(o), 128):
        s = slice(r0, r0 + 128)
        ok[s, live], t[s, live], u[s, live], w[s, live], det[s, live] = triangle_tuv(o[s, None], d[s, None], p[None, :, 0], p[None, :, 1],
                                                                                     p[None, :, 2])
    return ok, t, u, w, det


def hit_matrix(vertices, triangles, origins, dirs, tmin=0.0, tmax=np.inf):
    """(n_rays, F) bool: ray i hits the live triangle j"""
    ok, t = triangle_table(vertices, triangles, origins, dirs)[:2]
    return ok & in_range(t, tmin, tmax, False)


def without_skipped(ok, skip):
    """The skip rule on a table (n_rays, F) bool, in place: ray i does not see triangle skip[i]; an id that names no triangle
    skips nothing"""
    if skip is not None:
        sk = np.asarray(skip).reshape(-1)
        rows = np.nonzero((sk >= 0) & (sk < ok.shape[1]))[0]
        ok[rows, sk[rows]] = False
    return ok


def occluded(vertices, triangles, origins, dirs, tmin=0.0, tmax=np.inf, skip=None):
    """The Occluded paragraph by the loop over all triangles -> (n_rays,) bool"""
    return without_skipped(hit_matrix(vertices, triangles, origins, dirs, tmin, tmax), skip).any(1)


def mix32(x):
    x = np.asarray(x).astype(np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x.astype(np.uint32)


def duff_frame(n):
    """The AO paragraph's frame of unit normals n (..., 3) -> (T, B)"""
    n = np.asarray(n, np.float64)
    with np.errstate(all="ignore"):
        s = np.copysign(1.0, n[..., 2])
        a = -1.0 / (s + n[..., 2])
        b = (n[..., 0] * n[..., 1]) * a
        T = np.stack([1.0 + ((s * n[..., 0]) * n[..., 0]) * a, s * b, -(s * n[..., 0])], -1)
        B = np.stack([b, s + (n[..., 1] * n[..., 1]) * a, -n[..., 1]], -1)
    return T, B


def ao_rays(points, normals, table, bias, index0=0, seed=0):
    """-> (origins (n, 3), dirs (n, K, 3)) of the AO paragraph; table (R, K, 3)"""
    p, n = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    table = np.asarray(table, np.float64)
    R = table.shape[0]
    r = mix32((np.arange(len(p), dtype=np.int64) + int(index0) + int(seed)) & 0xFFFFFFFF) % np.uint32(R)
    l = table[r.astype(np.int64)]                                       # (n, K, 3)
    T, B = duff_frame(n)
    with np.errstate(all="ignore"):
        d = (T[:, None, :] * l[:, :, 0:1] + B[:, None, :] * l[:, :, 1:2]) + n[:, None, :] * l[:, :, 2:3]
        o = p + n * bias
    return o, d


def ambient_occlusion(vertices, triangles, points, normals, skip, table, bias, radius, index0=0, seed=0):
    """visible (n,) int32 of the AO paragraph; normals are unit already (the caller's part)"""
    p, n = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    K = np.asarray(table).shape[1]
    out = np.full(len(p), K, np.int32)
    with np.errstate(all="ignore"):
        nn = dot(n, n)
    walk = (nn > 0) & np.isfinite(nn) & np.isfinite(p).all(1)
    sk = None
    if skip is not None:
        sk = np.asarray(skip).reshape(-1)
        walk &= sk >= 0
    o, d = ao_rays(p, n, table, bias, index0, seed)
    for i in np.nonzero(walk)[0]:
        hit = occluded(vertices, triangles, np.broadcast_to(o[i], (K, 3)), d[i], 0.0, radius, None if sk is None else np.full(K, sk[i]))
        out[i] = K - int(hit.sum())
    return out


def occlusion_bytes(orm, owner, visible, K):
    """The Occlusion paragraph on a copy of orm (n, 3) uint8"""
    out = np.array(orm, np.uint8).reshape(-1, 3).copy()
    own = np.asarray(owner).reshape(-1) >= 0
    out[own, 0] = np.floor(255.0 * (np.asarray(visible, np.float64).reshape(-1)[own] / float(K)) + 0.5).astype(np.uint8)
    return out.reshape(np.shape(orm))


def check_bvh(lo, hi, links, vertices, triangles):
    """The invariants of the Layout paragraph on nodes read back from the buffer; raises AssertionError naming the first broken"""
    v, f = np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(triangles).reshape(-1, 3).astype(np.int64)
    n = len(f)
    assert len(lo) == len(hi) == len(links) == max(2 * n - 1, 0)
    if n == 0:
        return
    assert not np.isnan(lo).any() and not np.isnan(hi).any(), "a NaN box coordinate"
    live = live_triangles(v, f)
    leaves = links[n - 1:]
    assert sorted(leaves[:, 0].tolist()) == list(range(n)), "every triangle in exactly one leaf"
    assert (leaves[:, 1] == -1).all()
    empty = ~(lo[:, 0] <= hi[:, 0])
    for i in range(n):
        t, x = leaves[i, 0], n - 1 + i
        if live[t]:
            p = v[f[t]]
            assert (lo[x] == p.min(0)).all() and (hi[x] == p.max(0)).all(), f"leaf {x} is not the box of triangle {t}"
        else:
            assert empty[x] and np.isposinf(lo[x]).all() and np.isneginf(hi[x]).all(), f"the dead triangle {t} has a box"
    assert links[0, 3] == -1
    for x in range(n - 1):
        l, r = links[x, 0], links[x, 1]
        assert 0 <= l < 2 * n - 1 and 0 <= r < 2 * n - 1 and l != r
        assert links[l, 3] == x and links[r, 3] == x, f"parent links of node {x}"
        assert (lo[x] == np.minimum(lo[l], lo[r])).all() and (hi[x] == np.maximum(hi[l], hi[r])).all(), f"node {x} is not the union of its children"
    # following "box hit" everywhere: every node once in depth-first order, every leaf once, the end within 2 n steps
    node, seen_leaves, steps = 0, [], 0
    while node != -1:
        assert 0 <= node < 2 * n - 1 and steps < 2 * n, "the walk does not end"
        steps += 1
        if node >= n - 1:
            seen_leaves.append(node)
            node = links[node, 2]
        else:
            node = links[node, 0]
    assert steps == 2 * n - 1 and sorted(seen_leaves) == list(range(n - 1, 2 * n - 1)), "the walk misses a leaf"
    # a box miss at every internal node skips exactly its subtree
    for x in range(n - 1):
        m, y = links[x, 2], x
        while y < n - 1:
            y = links[y, 1]                       # the rightmost leaf of x
        assert links[y, 2] == m, f"miss link of node {x}"


def depth(links, n):
    """the longest root-to-leaf path in edges"""
    if n <= 1:
        return 0
    d = np.zeros(2 * n - 1, np.int64)
    best, stack = 0, [0]
    while stack:
        x = stack.pop()
        if x >= n - 1:
            best = max(best, int(d[x]))
            continue
        for c in links[x, :2]:
            d[c] = d[x] + 1
            stack.append(int(c))
    return best


# ---- the scenes and ray families the CPU and the GPU tests share ----------------------------------------------------------

def random_mesh(n, seed=0):
    """n triangles with centres in the unit cube, the size falling with n so that a ray through the cube meets about one"""
    rng = np.random.default_rng([seed, n])
    size = 0.6 / max(n, 1) ** (1.0 / 3.0) + 0.04
    c = rng.random((n, 1, 3))
    v = (c + size * rng.standard_normal((n, 3, 3))).reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def grid_mesh(m=8):
    """An axis-aligned floor (z = 0.5) and wall (x = 0.5) of m x m quads each over the unit square, every coordinate a multiple of
    1 / m: flat node boxes, and triangle edges that rays of dyadic coordinates meet exactly"""
    k = np.arange(m + 1) / m
    a, b = np.meshgrid(k, k, indexing="ij")
    floor = np.stack([a, b, np.full_like(a, 0.5)], -1).reshape(-1, 3)
    wall = np.stack([np.full_like(a, 0.5), a, b], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    q = (i * (m + 1) + j).reshape(-1)
    quads = np.concatenate([np.stack([q, q + m + 1, q + 1], 1), np.stack([q + 1, q + m + 1, q + m + 2], 1)])
    return np.concatenate([floor, wall]), np.concatenate([quads, quads + len(floor)]).astype(np.int32)


def dead_mesh(seed=0):
    """100 triangles: 85 live random ones and, spread among them, 5 with an index out of range, 5 with a corner that is not finite
    and 5 of zero area"""
    v, f = random_mesh(100, seed + 7)
    v = np.concatenate([v, [[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [-np.inf, 0.0, 0.0]]])
    f = f.copy()
    nv = len(v)
    for k, t in enumerate(range(3, 100, 20)):
        f[t, k % 3] = (-1, nv, nv + 7, 2 ** 31 - 1, -2 ** 31)[k]
        f[t + 5, (k + 1) % 3] = nv - 3 + k % 3
        f[t + 11] = (f[t + 11, 0], f[t + 11, 0], f[t + 11, 1]) if k % 2 else (f[t + 11, 0],) * 3
    return v, f


def identical_mesh(n=257):
    v = np.array([[0.2, 0.2, 0.5], [0.8, 0.3, 0.5], [0.4, 0.9, 0.6]])
    return v, np.tile(np.arange(3, dtype=np.int32), (n, 1))


def collinear_mesh(n=200):
    """n small triangles whose centroids lie on one line (two Morton axes constant)"""
    x = (np.arange(n) / n)[:, None, None]
    base = np.array([[0.0, -0.02, -0.01], [0.0, 0.02, -0.01], [0.0, 0.0, 0.02]])[None]
    v = (base + np.array([0.0, 0.5, 0.5]) + x * np.array([1.0, 0.0, 0.0])).reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


MESHES = {"n0": lambda: random_mesh(0), "n1": lambda: random_mesh(1), "n2": lambda: random_mesh(2), "n3": lambda: random_mesh(3),
          "n64": lambda: random_mesh(64), "n65": lambda: random_mesh(65), "n1000": lambda: random_mesh(1000),
          "identical257": identical_mesh, "collinear200": collinear_mesh, "dead100": dead_mesh, "grid": grid_mesh}


def _targets(v, f, n, rng):
    """n points on random live triangles"""
    live = np.nonzero(live_triangles(v, f))[0]
    t = live[rng.integers(0, len(live), n)]
    w = rng.dirichlet(np.ones(3), n)
    return (v[f[t]] * w[:, :, None]).sum(1), t


def ray_family(name, v, f, n, seed=0):
    """-> dict(origins, dirs, tmin, tmax, skip) of the family `name` for the mesh (v, f), which has a live triangle: about half
    of the rays are aimed at a point of the mesh, half are not"""
    rng = np.random.default_rng([seed, n, sum(map(ord, name))])
    v, f = np.asarray(v, np.float64), np.asarray(f)
    aim, _ = _targets(v, f, n, rng)
    aimed = rng.random(n) < 0.5
    lo, hi = np.nanmin(np.where(np.isfinite(v), v, np.nan), 0), np.nanmax(np.where(np.isfinite(v), v, np.nan), 0)
    ext = float(np.max(hi - lo)) + 1e-3
    away = lo + (hi - lo) * rng.random((n, 3)) + ext * rng.standard_normal((n, 3))
    out = dict(tmin=0.0, tmax=np.inf, skip=None)
    if name in ("random", "skip"):          # origins inside the root box and near it
        o = lo + (hi - lo) * (rng.random((n, 3)) * 1.5 - 0.25)
        goal = np.where(aimed[:, None], aim, away)
        d = (goal - o) * (0.5 + 2.0 * rng.random((n, 1)))
        if name == "skip":                   # the nearest hit is skipped: the second one decides
            m = hit_matrix(v, f, o, d)
            p = v[np.clip(f, 0, len(v) - 1)]
            with np.errstate(all="ignore"):
                t = hit_parameter(o[:, None], d[:, None], p[None, :, 0], p[None, :, 1], p[None, :, 2])
            t = np.where(m, t, np.inf)
            out["skip"] = np.where(m.any(1), t.argmin(1), -1).astype(np.int32)
    elif name == "short":                    # a finite tmax that cuts some of the hits off
        o = lo + (hi - lo) * (rng.random((n, 3)) * 1.5 - 0.25)
        d = np.where(aimed[:, None], aim, away) - o
        d *= rng.choice([0.8, 1.25], (n, 1))  # the aimed point lies at t = 1.25 or 0.8
        out["tmax"] = 1.0
    elif name == "far":                      # origins far outside the root box
        u = rng.standard_normal((n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        o = np.where(aimed[:, None], aim, away) - u * (10.0 ** rng.uniform(2, 6, (n, 1))) * ext
        d = u * rng.uniform(0.5, 2.0, (n, 1))
    elif name in ("axis1", "axis2"):         # one, two zero direction components
        zero = np.zeros((n, 3), bool)
        k = rng.integers(0, 3, n)
        zero[np.arange(n), k] = True
        if name == "axis2":
            zero[np.arange(n), (k + 1 + rng.integers(0, 2, n)) % 3] = True
        step = np.where(zero, 0.0, rng.choice([-1.0, 1.0], (n, 3)) * rng.uniform(0.2, 2.0, (n, 3)) * ext)
        goal = np.where(aimed[:, None], aim, lo + (hi - lo) * (rng.random((n, 3)) * 1.6 - 0.3))
        o, d = goal - step, step * rng.uniform(0.5, 3.0, (n, 1))
    elif name == "grazing":                  # nearly in the plane of the triangle aimed at: |det| is 1e-13 .. 1e-7 of its products
        _, t = _targets(v, f, n, rng)
        p = v[f[t]]
        safe = lambda x: x / np.maximum(np.sqrt(dot(x, x)), 1e-300)[..., None]
        edge = np.sqrt(dot(p[:, 1] - p[:, 0], p[:, 1] - p[:, 0]))[:, None] + 1e-3 * ext
        nrm = safe(cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]))
        along = safe((p[:, 1] - p[:, 0]) * rng.uniform(-1, 1, (n, 1)) + (p[:, 2] - p[:, 0]) * rng.uniform(-1, 1, (n, 1)))
        w = rng.dirichlet(np.ones(3), n)
        w = np.where(aimed[:, None], w, w * 1.6 - 0.2)   # the others pass near the triangle's edges, inside or outside
        goal = (p * w[:, :, None]).sum(1)
        d = (along + nrm * rng.choice([-1.0, 1.0], (n, 1)) * 10.0 ** rng.uniform(-13, -7, (n, 1))) * edge * rng.uniform(0.1, 0.5, (n, 1))
        o = goal - d * rng.uniform(0.5, 1.5, (n, 1))     # the plane is crossed at t = 0.5 .. 1.5; tmax = 1
        out["tmax"] = 1.0
    else:
        raise KeyError(name)
    out.update(origins=np.ascontiguousarray(o), dirs=np.ascontiguousarray(d))
    return out


def grid_family(name, n, seed=0, m=8):
    """Families of dyadic rays for grid_mesh(m), whose arithmetic under the triangle test is exact.
    faces: rays lying in the floor's plane z = 0.5 -- a face of every floor node box -- or offset from it by an ulp or 2^-40, along
    the grid lines or across them; they hit nothing of the floor (det == 0) and meet the wall on the edges of its triangles.
    tmax: rays from z = 0.25 whose floor hit lies at t = 1 exactly (tmax = 1), just beyond it, or before it."""
    rng = np.random.default_rng([seed, n, len(name)])
    g = 64
    if name == "faces":
        o = np.stack([rng.integers(-g // 2, g + g // 2, n) / g, rng.integers(-g // 4, g + g // 4, n) / g, np.full(n, 0.5)], 1)
        o[:, 2] += rng.choice([0.0, 0.0, 2.0 ** -53, -2.0 ** -53, 2.0 ** -40, -2.0 ** -40], n)
        d = np.stack([rng.integers(-8, 9, n) / 8.0, rng.integers(-8, 9, n) / 8.0, np.zeros(n)], 1)
        axis = rng.random(n) < 0.4
        d[axis, 1] = 0.0                                      # along x: grazing the floor quads' edges when o_y is on a grid line
        d[(d[:, 0] == 0) & (d[:, 1] == 0), 0] = 1.0
        return dict(origins=o, dirs=d, tmin=0.0, tmax=np.inf, skip=None)
    if name == "tmax":
        o = np.stack([rng.integers(-g // 4, g + g // 4, n) / g, rng.integers(-g // 4, g + g // 4, n) / g, np.full(n, 0.25)], 1)
        d = np.stack([rng.integers(-16, 17, n) / 64.0, rng.integers(-16, 17, n) / 64.0,
                      rng.choice([0.25, 0.25, 0.25 - 2.0 ** -12, 0.5], n)], 1)
        return dict(origins=o, dirs=d, tmin=0.0, tmax=1.0, skip=None)
    raise KeyError(name)


FAMILIES = ("random", "axis1", "axis2", "short", "far", "skip", "grazing")
GRID_FAMILIES = ("faces", "tmax")


def open_box():
    """12 triangles: a unit floor, four walls of height 0.5 and a lid over half of the top (x < 0.5)"""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, .5], [1, 0, .5], [1, 1, .5], [0, 1, .5], [.5, 0, .5], [.5, 1, .5]], np.float64)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5], [2, 3, 7], [2, 7, 6], [3, 0, 4], [3, 4, 7],
                  [4, 8, 9], [4, 9, 7]], np.int32)
    return v, f


def closed_box():
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.float64)
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5], [2, 3, 7], [2, 7, 6],
                  [3, 0, 4], [3, 4, 7]], np.int32)
    return v, f


def height_field(nx=25, ny=10, seed=3):
    """2 nx ny = 500 triangles of a bumpy height field over [0, nx] x [0, ny] / 10"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx + 1) / 10.0, np.arange(ny + 1) / 10.0, indexing="ij")
    z = 0.15 * np.sin(5.0 * x) * np.cos(4.0 * y) + 0.05 * rng.random(x.shape)
    v = np.stack([x, y, z], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    q = (i * (ny + 1) + j).reshape(-1)
    f = np.concatenate([np.stack([q, q + ny + 1, q + 1], 1), np.stack([q + 1, q + ny + 1, q + ny + 2], 1)]).astype(np.int32)
    return v, f


def unit_rows(n):
    n = np.asarray(n, np.float64)
    return n / np.sqrt(dot(n, n))[..., None]


def face_points(v, f, which):
    """The centroids and unit face normals of the triangles `which` -> (points, normals, owner)"""
    p = v[f[which]]
    n = cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return p.mean(1), unit_rows(n), np.asarray(which, np.int32)
