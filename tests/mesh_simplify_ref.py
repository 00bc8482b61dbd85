"""fp64 numpy restatement of the mesh simplification contract (include/gs2m_simplify.h): vertex clustering on a lattice with
quadric placement.  Not a test module: tests/test_mesh_simplify.py checks it on its own, tests/test_mesh_simplify_gpu.py holds
the HIP kernels to it.

`simplify_ref` returns, besides the outputs, the per-cell margins of the two decisions a last-bit difference could flip, and
takes the placement routine as a parameter: `place_eigh` (numpy.linalg.eigh) or `place_jacobi` (the header's fixed-sweep
cyclic Jacobi written out, expression for expression as the kernel evaluates it).  The tolerance of the GPU comparison is
measured between those two (ULP_MEASURED, ULP_BOUND below)."""
import numpy as np

SWEEPS = 8                 # GS2M_SIMPLIFY_SWEEPS
EIG_CUT = 1e-3             # Lindstrom's constant
MAX_AXIS_CELLS = 1 << 21   # GS2M_SIMPLIFY_MAX_AXIS_CELLS
LONG_SEG = 256
MARGIN = 1e-6              # a decision closer than this to its threshold could flip with a last-bit difference

# The largest difference between the two placements (eigh / written-out Jacobi) over every scene of `gpu_scenes()`, in fp32
# ulps of the coordinate after the final rounding, as tests/test_mesh_simplify.py measures and asserts it; the GPU test's bound
# is four times that and at least 1 ulp (a single rounding tie can flip).
ULP_MEASURED = 0.0
ULP_BOUND = max(1.0, 4.0 * ULP_MEASURED)


# ---- the fixed summation order ----

def fixed_order_sum(e):
    """e (n, Q) fp64 -> (Q,): the header's order.  n <= 256: sixteen strided partials from 0.0, folded 8, 4, 2, 1; longer:
    256 strided partials, runs of 64 folded 32 .. 1, the four results as (w0 + w1) + (w2 + w3)."""
    e = np.asarray(e, dtype=np.float64)
    n, q = e.shape
    width = 16 if n <= LONG_SEG else 256
    rows = -(-n // width) if n else 0
    pad = np.zeros((rows * width, q))
    pad[:n] = e
    pad = pad.reshape(rows, width, q)
    valid = (np.arange(rows * width).reshape(rows, width) < n)
    r = np.zeros((width, q))
    for k in range(rows):  # left to right; a lane past the end adds nothing (not even +0.0)
        r = np.where(valid[k][:, None], r + pad[k], r)
    if width == 16:
        for o in (8, 4, 2, 1):
            r[:o] = r[:o] + r[o:2 * o]
        return r[0].copy()
    w = r.reshape(4, 64, q).copy()
    for o in (32, 16, 8, 4, 2, 1):
        w[:, :o] = w[:, :o] + w[:, o:2 * o]
    return (w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])


# ---- placement ----

def place_jacobi(A, b, m, cell):
    """A (C, 3, 3), b (C, 3), m (C, 3) -> x (C, 3), l (C, 3), fallback (C,), xq (C, 3) the unclamped solution (m where
    lmax <= 0).  The kernel's arithmetic, vectorised over the cells."""
    a = np.array(A, dtype=np.float64)
    C = len(a)
    u = np.tile(np.eye(3), (C, 1, 1))
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                apq = a[:, p, q].copy()
                on = apq != 0.0
                theta = np.where(on, (a[:, q, q] - a[:, p, p]) / np.where(on, 2.0 * apq, 1.0), 0.0)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = np.where(on, 1.0 / np.sqrt(t * t + 1.0), 1.0)
                s = np.where(on, t * c, 0.0)
                c, s, on3 = c[:, None], s[:, None], on[:, None]
                x, y = a[:, :, p].copy(), a[:, :, q].copy()
                a[:, :, p] = np.where(on3, c * x - s * y, x)
                a[:, :, q] = np.where(on3, s * x + c * y, y)
                x, y = a[:, p, :].copy(), a[:, q, :].copy()
                a[:, p, :] = np.where(on3, c * x - s * y, x)
                a[:, q, :] = np.where(on3, s * x + c * y, y)
                x, y = u[:, :, p].copy(), u[:, :, q].copy()
                u[:, :, p] = np.where(on3, c * x - s * y, x)
                u[:, :, q] = np.where(on3, s * x + c * y, y)
    l = np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1)
    return _solve(A, b, m, cell, l, u)


def place_eigh(A, b, m, cell):
    l, u = np.linalg.eigh(np.asarray(A, dtype=np.float64))
    return _solve(A, b, m, cell, l, u)


def _solve(A, b, m, cell, l, u):
    A, b, m = np.asarray(A, np.float64), np.asarray(b, np.float64), np.asarray(m, np.float64)
    lmax = l.max(axis=1)
    pos = lmax > 0.0
    with np.errstate(all="ignore"):
        inv = np.where(l > EIG_CUT * lmax[:, None], 1.0 / l, 0.0)
        r = -b - ((A[:, :, 0] * m[:, 0:1] + A[:, :, 1] * m[:, 1:2]) + A[:, :, 2] * m[:, 2:3])
        y = ((u[:, 0, :] * r[:, 0:1] + u[:, 1, :] * r[:, 1:2]) + u[:, 2, :] * r[:, 2:3]) * inv
        z = m + ((u[:, :, 0] * y[:, 0:1] + u[:, :, 1] * y[:, 1:2]) + u[:, :, 2] * y[:, 2:3])
    z = np.where(pos[:, None], z, m)
    inside = np.all(np.abs(z) <= 0.5 * cell, axis=1)
    x = np.where((pos & inside)[:, None], z, m)
    return x, l, ~(pos & inside), z


def ulp_diff(a, b):
    """|a - b| in fp32 ulps of the larger magnitude, elementwise (a, b fp32)."""
    a32, b32 = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ulp = np.spacing(np.maximum(np.abs(a32), np.abs(b32))).astype(np.float64)
    return np.abs(a32.astype(np.float64) - b32.astype(np.float64)) / ulp


def vertex_ulps(a, b):
    """a, b (n, 3) fp32 positions -> (n, 3): |a - b| in fp32 ulps of the vertex's coordinate magnitude, the largest |coordinate|
    of the vertex in either array (the solve mixes the axes: an error does not shrink with the one coordinate it lands on)."""
    a32, b32 = np.asarray(a, np.float32).reshape(-1, 3), np.asarray(b, np.float32).reshape(-1, 3)
    mag = np.maximum(np.abs(a32).max(axis=1), np.abs(b32).max(axis=1))
    ulp = np.spacing(mag).astype(np.float64)[:, None]
    return np.abs(a32.astype(np.float64) - b32.astype(np.float64)) / ulp


# ---- the contract ----

def cells_of(vertices, cell):
    """-> (cell id per vertex, absolute index (C, 3) int64 per cell): cells numbered in increasing (ix, iy, iz)."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    if not np.all(np.isfinite(v)):
        raise ValueError("mesh_simplify_ref: a non-finite vertex (GS2M_ERR_INVALID_ARG)")
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError("mesh_simplify_ref: cell must be finite and positive (GS2M_ERR_INVALID_ARG)")
    idx = np.floor(v.astype(np.float64) / float(cell))
    if len(v) and np.any(idx.max(axis=0) - idx.min(axis=0) + 1 > MAX_AXIS_CELLS):
        raise OverflowError("mesh_simplify_ref: more than 2^21 cells along an axis (GS2M_ERR_UNSUPPORTED)")
    idx = idx.astype(np.int64)
    uniq, inverse = np.unique(idx, axis=0, return_inverse=True)
    return inverse.reshape(-1).astype(np.int64), uniq


def _kept_triangles(ct):
    """ct (F, 3) cells per corner -> the indices of the emitted triangles, in input order."""
    distinct = (ct[:, 0] != ct[:, 1]) & (ct[:, 1] != ct[:, 2]) & (ct[:, 0] != ct[:, 2])
    cand = np.nonzero(distinct)[0]
    if len(cand) == 0:
        return cand
    _, first = np.unique(np.sort(ct[cand], axis=1), axis=0, return_index=True)  # the first occurrence: the smallest index
    return np.sort(cand[first])


def count_ref(vertices, triangles, cell):
    """-> (surviving vertices, emitted triangles)."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if len(t) == 0 or len(vertices) == 0:
        return 0, 0
    vcell, _ = cells_of(vertices, cell)
    ct = vcell[t]
    kept = _kept_triangles(ct)
    return int(len(np.unique(ct[kept]))), int(len(kept))


def simplify_ref(vertices, triangles, cell, attributes=None, weights=None, placement=place_eigh):
    """The whole contract.  -> dict: vertices (n, 3) fp32, positions64 (n, 3) fp64 before the rounding, triangles (m, 3) int32,
    vertex_map (V,) int32, attributes (n, nch) fp32 or None, weight (n,) fp32, totals; per CELL (before the compaction):
    fallback (took the mean), margin_eig = min_i |l_i / lmax - 1e-3| (inf where lmax <= 0), margin_box = min_k (cell / 2 -
    |x_k|) / cell of the unclamped solution (negative: rejected), survives."""
    v32 = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V, F = len(v32), len(t)
    nch = 0 if attributes is None else np.asarray(attributes).reshape(V, -1).shape[1]
    if V == 0 or F == 0:
        return dict(vertices=np.zeros((0, 3), np.float32), positions64=np.zeros((0, 3)), triangles=np.zeros((0, 3), np.int32),
                    vertex_map=np.full(V, -1, np.int32), attributes=None if attributes is None else np.zeros((0, nch), np.float32),
                    weight=np.zeros(0, np.float32), totals=(0, 0), fallback=np.zeros(0, bool), margin_eig=np.zeros(0),
                    margin_box=np.zeros(0), survives=np.zeros(0, bool))
    if t.min() < 0 or t.max() >= V:
        raise IndexError("mesh_simplify_ref: a triangle id outside [0, V) (GS2M_ERR_INVALID_ARG)")
    cell = float(cell)
    vcell, cidx = cells_of(v32, cell)
    C = len(cidx)
    centre = (cidx.astype(np.float64) + 0.5) * cell
    v64 = v32.astype(np.float64)
    w64 = np.ones(V) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    a64 = None if attributes is None else np.asarray(attributes, dtype=np.float32).reshape(V, nch).astype(np.float64)

    # vertices of a cell in increasing input index
    vorder = np.argsort(vcell, kind="stable")
    vstart = np.searchsorted(vcell[vorder], np.arange(C + 1))
    # a slot per distinct cell of a triangle, by cell and then by triangle
    ct = vcell[t]
    valid = np.stack([np.ones(F, bool), ct[:, 1] != ct[:, 0], (ct[:, 2] != ct[:, 0]) & (ct[:, 2] != ct[:, 1])], axis=1)
    skey = np.where(valid, ct, C).reshape(-1)
    sorder = np.argsort(skey, kind="stable")
    sstart = np.searchsorted(skey[sorder], np.arange(C + 1))

    m = np.zeros((C, 3))
    A = np.zeros((C, 3, 3))
    b = np.zeros((C, 3))
    wsum = np.zeros(C)
    attr = np.zeros((C, nch))
    for c in range(C):
        vs = vorder[vstart[c]:vstart[c + 1]]
        n = len(vs)
        s = fixed_order_sum(np.concatenate([v64[vs] - centre[c], w64[vs, None]], axis=1))
        m[c] = s[:3] / float(n)
        wsum[c] = s[3]
        for ch in range(nch):
            sa = fixed_order_sum(np.stack([w64[vs] * a64[vs, ch], a64[vs, ch]], axis=1))
            attr[c, ch] = sa[1] / float(n) if s[3] == 0.0 else sa[0] / s[3]
        ts = sorder[sstart[c]:sstart[c + 1]] // 3
        if len(ts):
            p = v64[t[ts]] - centre[c]  # (k, corner, axis)
            e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
            nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
            ok = ln > 0.0
            lns = np.where(ok, ln, 1.0)
            d = -((nx * p[:, 0, 0] + ny * p[:, 0, 1]) + nz * p[:, 0, 2])
            terms = np.stack([nx * nx / lns, nx * ny / lns, nx * nz / lns, ny * ny / lns, ny * nz / lns, nz * nz / lns,
                              nx * d / lns, ny * d / lns, nz * d / lns], axis=1)
            # a triangle with len == 0 keeps its place in the order and adds nothing (+0.0 here: the same partials up to
            # the sign of a zero, which nothing downstream tells apart)
            q = fixed_order_sum(np.where(ok[:, None], terms, 0.0))
            A[c] = [[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]]
            b[c] = q[6:9]

    x, l, fallback, z = placement(A, b, m, cell)
    lmax = l.max(axis=1)
    with np.errstate(all="ignore"):
        margin_eig = np.where(lmax > 0.0, np.min(np.abs(l / lmax[:, None] - EIG_CUT), axis=1), np.inf)
    margin_box = np.where(lmax > 0.0, np.min(0.5 * cell - np.abs(z), axis=1) / cell, np.inf)
    pos64 = centre + x

    kept = _kept_triangles(ct)
    survives = np.zeros(C, bool)
    survives[ct[kept].reshape(-1)] = True
    newid = np.cumsum(survives) - 1
    vmap = np.where(survives[vcell], newid[vcell], -1).astype(np.int32)
    out_w = np.where(wsum == 0.0, 0.0, wsum)
    return dict(vertices=pos64[survives].astype(np.float32), positions64=pos64[survives],
                triangles=newid[ct[kept]].astype(np.int32).reshape(-1, 3), vertex_map=vmap,
                attributes=None if attributes is None else attr[survives].astype(np.float32),
                weight=out_w[survives].astype(np.float32), totals=(int(survives.sum()), int(len(kept))),
                fallback=fallback, margin_eig=margin_eig, margin_box=margin_box, survives=survives)


def decision_distance(ref):
    """Per cell: how close its two decisions came to their thresholds: min(margin_eig, |margin_box|)."""
    return np.minimum(ref["margin_eig"], np.abs(ref["margin_box"]))


# ---- scenes ----

def box_mesh(n, lo=(-1.013, -1.009, -1.021), size=2.0):
    """A box with every face subdivided n x n, vertices shared: 6 n^2 + 2 of them; outward triangles."""
    g = np.arange(n + 1)
    I, J, K = np.meshgrid(g, g, g, indexing="ij")
    on = (I == 0) | (I == n) | (J == 0) | (J == n) | (K == 0) | (K == n)
    ids = np.full((n + 1,) * 3, -1, np.int64)
    ids[on] = np.arange(int(on.sum()))
    ijk = np.stack([I[on], J[on], K[on]], axis=1)
    lo32 = np.asarray(lo, dtype=np.float32).astype(np.float64)
    verts = (lo32 + ijk * (size / n)).astype(np.float32)
    tris = []
    a, bb = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a, bb = a.reshape(-1), bb.reshape(-1)
    for axis in range(3):
        for side in (0, n):
            def vid(da, db):
                c = [None, None, None]
                c[axis] = np.full(len(a), side)
                c[(axis + 1) % 3] = a + da
                c[(axis + 2) % 3] = bb + db
                return ids[c[0], c[1], c[2]]
            q00, q10, q11, q01 = vid(0, 0), vid(1, 0), vid(1, 1), vid(0, 1)
            t1, t2 = np.stack([q00, q10, q11], 1), np.stack([q00, q11, q01], 1)
            f = np.concatenate([t1, t2])
            tris.append(f if side == n else f[:, ::-1])
    return verts, np.concatenate(tris).astype(np.int32)


def box_planes(n, lo=(-1.013, -1.009, -1.021), size=2.0):
    """The fp32 coordinates of the box's six planes as the vertices carry them: (lo (3,), hi (3,)) fp64."""
    v, _ = box_mesh(n, lo, size)
    return v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)


def icosphere(level, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """Level 0 is the icosahedron; every level splits each triangle in four.  10 * 4^level + 2 vertices."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p],
                  [p, 0, -1], [p, 0, 1], [-p, 0, -1], [-p, 0, 1]], dtype=np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
                  [9, 8, 1]], dtype=np.int64)
    for _ in range(level):
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        ue, inv = np.unique(e, axis=0, return_inverse=True)
        mid = v[ue[:, 0]] + v[ue[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        base = len(v)
        v = np.concatenate([v, mid])
        inv = inv.reshape(-1)
        F = len(f)
        ab, bc, ca = base + inv[:F], base + inv[F:2 * F], base + inv[2 * F:]
        f = np.concatenate([np.stack([f[:, 0], ab, ca], 1), np.stack([f[:, 1], bc, ab], 1), np.stack([f[:, 2], ca, bc], 1),
                            np.stack([ab, bc, ca], 1)])
    return (v * radius + np.asarray(centre)).astype(np.float32), f.astype(np.int32)


def plane_grid(n=40, origin=(0.031, 0.047, 0.402), du=(0.011, 0.002, 0.001), dv=(-0.001, 0.012, 0.003)):
    """n x n vertices on a tilted plane, 2 (n - 1)^2 triangles."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = (np.asarray(origin) + i.reshape(-1, 1) * np.asarray(du) + j.reshape(-1, 1) * np.asarray(dv)).astype(np.float32)
    idx = (i * n + j)
    q00, q10, q11, q01 = idx[:-1, :-1].reshape(-1), idx[1:, :-1].reshape(-1), idx[1:, 1:].reshape(-1), idx[:-1, 1:].reshape(-1)
    t = np.concatenate([np.stack([q00, q10, q11], 1), np.stack([q00, q11, q01], 1)]).astype(np.int32)
    return v, t


def scene_attributes(V, nch=5, seed=7):
    """nch channels in [0, 1) and 0 / 1 weights, a pure function of (V, nch, seed)."""
    rng = np.random.default_rng(seed)
    return rng.random((V, nch), dtype=np.float32), (rng.random(V) < 0.6).astype(np.float32)


_SCENES = {}


def gpu_scenes():
    """name -> (vertices, triangles, cell): the scenes the GPU test compares with the restatement.  Built once."""
    if not _SCENES:
        b8, b24 = box_mesh(8), box_mesh(24)
        i3, i6 = icosphere(3), icosphere(6)
        _SCENES.update({
            "box8": (b8[0], b8[1], 0.31),
            "box24_a": (b24[0], b24[1], 0.23),
            "box24_b": (b24[0], b24[1], 0.31),
            "ico3": (i3[0], i3[1], 0.37),
            "ico6": (i6[0], i6[1], 0.11),
        })
    return _SCENES


_REFS = {}


def gpu_scene_ref(name, placement=place_eigh):
    """simplify_ref of a scene of gpu_scenes() with its test attributes and weights, computed once and shared."""
    key = (name, placement.__name__)
    if key not in _REFS:
        v, t, cell = gpu_scenes()[name]
        a, w = scene_attributes(len(v))
        _REFS[key] = simplify_ref(v, t, cell, a, w, placement)
    return _REFS[key]
