"""The mesh visualisation (include/gs2m_meshview.h) restated in float64 numpy, brute force over (triangle, sample),
and the synthetic inputs the tests of it share.  Coverage, depth and the notion of an undecided sample are tnt_cull_ref's, applied
to the sample frame (H ss, W ss) with the intrinsics (ss fx, ss fy, ss cx, ss cy).

What two correct evaluations of the contract may settle differently is reported beside the values:
  sample  undecided as tnt_cull_ref.render_depth says (an edge value near zero, a triangle seen edge-on, z at near or far), or
          when two triangles of different indices have covering fp32 z within TIE_ULPS units of the last place of the minimum;
  pixel   undecided when one of its ss x ss samples is;
  byte    loose when 255 enc -- for the alpha byte 255 m / ss^2 -- lies within LOOSE of a half-integer: it may differ by 1.
An input may hold at most CAP undecided pixels and CAP loose bytes (tests/test_mesh_view.py asserts that of every input)."""
import functools

import numpy as np

import tnt_cull_ref as R

TIE_ULPS = 4
LOOSE = 1e-6
CAP = 0.01
BASE, AMBIENT, DIFFUSE = (0.7, 0.7, 0.7), 0.15, 0.85
_NONE = np.int64(1) << 40  # above every fp32 bit pattern: no triangle


def _cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)


def _rdot(u, v):
    """row by row: (u0 v0 + u1 v1) + u2 v2"""
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def srgb_encode(x):
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(np.maximum(x, 0.0031308), 1.0 / 2.4) - 0.055)


def visibility(verts, tris, w2c, fx, fy, cx, cy, H, W, ss=1, near=R.NEAR, far=R.FAR, chunk=64):
    """-> dict(zbits (n, H ss, W ss) uint32, 0xFFFFFFFF where empty; tri (n, H ss, W ss) int64, the lowest index among the
    triangles of the smallest fp32 z, -1 where empty; undecided (n, H ss, W ss) bool)"""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    w2c = np.asarray(w2c, np.float64).reshape(-1, 4, 4)
    Hs, Ws, k = H * ss, W * ss, (ss * fx, ss * fy, ss * cx, ss * cy)
    depth, und = R.render_depth(verts, tris, w2c, *k, Hs, Ws, near, far)
    r = R.pixel_rays(Hs, Ws, *k)
    zbits = np.empty((len(w2c), Hs * Ws), np.uint32)
    tri = np.empty((len(w2c), Hs * Ws), np.int64)
    tie = np.empty((len(w2c), Hs * Ws), bool)
    with np.errstate(all="ignore"):
        for v, M in enumerate(w2c):
            cam = R.to_camera(verts, M)
            b1, b2, t1 = np.full(Hs * Ws, _NONE), np.full(Hs * Ws, _NONE), np.full(Hs * Ws, -1, np.int64)
            for t0 in range(0, len(tris), chunk):
                t = tris[t0:t0 + chunk]
                a, b, c = cam[t[:, 0]], cam[t[:, 1]], cam[t[:, 2]]
                n = _cross(b - a, c - a)
                valid = np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1) & (n != 0).any(1)
                if not valid.any():
                    continue
                idx = t0 + np.nonzero(valid)[0]
                a, b, c, n = a[valid], b[valid], c[valid], n[valid]
                w = [R._dot(_cross(p, q), r) for p, q in ((b, c), (c, a), (a, b))]
                pos = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)
                neg = (w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0)
                covered = (pos | neg) & ~((w[0] == 0) & (w[1] == 0) & (w[2] == 0))
                z = _rdot(n, a)[:, None] / R._dot(n, r)
                sample = covered & (z >= near) & (z <= far)
                bits = np.where(sample, np.where(sample, z, 1.0).astype(np.float32).view(np.uint32).astype(np.int64), _NONE)
                m1 = bits.min(axis=0)
                m2 = np.partition(bits, 1, axis=0)[1] if len(bits) > 1 else np.full_like(m1, _NONE)
                first = idx[bits.argmin(axis=0)]  # the lowest index of the chunk's minimum: idx ascends
                b2 = np.minimum(np.maximum(b1, m1), np.minimum(b2, m2))
                t1 = np.where(m1 < b1, first, t1)
                b1 = np.minimum(b1, m1)
            zbits[v] = np.where(b1 < _NONE, b1, 0xFFFFFFFF).astype(np.uint32)
            tri[v] = np.where(b1 < _NONE, t1, -1)
            tie[v] = (b1 < _NONE) & (b2 - b1 <= TIE_ULPS)
    shape = (len(w2c), Hs, Ws)
    zbits, und = zbits.reshape(shape), und | tie.reshape(shape)
    ok = ~und
    assert np.array_equal(np.where(zbits == 0xFFFFFFFF, 0, zbits)[ok], depth.view(np.uint32)[ok]), "the two restatements disagree"
    return dict(zbits=zbits, tri=tri.reshape(shape), undecided=und)


def vertex_normal_sums(verts, tris):
    """-> (sums (V, 3) int64 in units of 2^-32, deg (V,) the valid triangles at each vertex, normals (V, 3) fp64)"""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    sums, deg = np.zeros((len(verts), 3), np.int64), np.zeros(len(verts), np.int64)
    good = ((tris >= 0) & (tris < len(verts))).all(axis=1)
    t = tris[good]
    with np.errstate(all="ignore"):
        a, b, c = verts[t[:, 0]], verts[t[:, 1]], verts[t[:, 2]]
        n = _cross(b - a, c - a)
        u = n / np.sqrt(_rdot(n, n))[:, None]
        use = (n != 0).any(axis=1) & np.isfinite(u).all(axis=1)
        q = np.rint(u[use] * 4294967296.0).astype(np.int64)
        for k in range(3):
            np.add.at(sums, t[use, k], q)
            np.add.at(deg, t[use, k], 1)
        s = sums.astype(np.float64)
        normals = np.where((sums != 0).any(axis=1)[:, None], s / np.sqrt(_rdot(s, s))[:, None], 0.0)
    return sums, deg, normals


def barycentrics(a, b, c, ray):
    """rows of camera-space vertices and rays -> (l0, l1, l2)"""
    e0, e1, e2 = _rdot(_cross(b, c), ray), _rdot(_cross(c, a), ray), _rdot(_cross(a, b), ray)
    s = (e0 + e1) + e2
    return e0 / s, e1 / s, e2 / s


def shade(verts, tris, w2c, fx, fy, cx, cy, H, W, ss=2, shading="flat", colors=None, base=BASE, ambient=AMBIENT, diffuse=DIFFUSE,
          srgb=True, near=R.NEAR, far=R.FAR, vis=None):
    """-> dict(rgba (n, H, W, 4) uint8, depth (n, H, W) float32, tri_id (n, H, W) int32, undecided (n, H, W) bool,
    loose (n, H, W, 4) bool).  vis: visibility(...) of the same arguments, when the caller has it already."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    w2c = np.asarray(w2c, np.float64).reshape(-1, 4, 4)
    vis = vis or visibility(verts, tris, w2c, fx, fy, cx, cy, H, W, ss, near, far)
    Hs, Ws = H * ss, W * ss
    r = R.pixel_rays(Hs, Ws, ss * fx, ss * fy, ss * cx, ss * cy)
    vn = vertex_normal_sums(verts, tris)[2] if shading == "smooth" else None
    col = None if colors is None else np.asarray(colors, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(w2c)
    rgba, loose = np.zeros((n, H, W, 4), np.uint8), np.zeros((n, H, W, 4), bool)
    with np.errstate(all="ignore"):
        for v, M in enumerate(w2c):
            cam = R.to_camera(verts, M)
            p = np.nonzero(vis["tri"][v].ravel() >= 0)[0]
            t = tris[vis["tri"][v].ravel()[p]]
            a, b, c, ray = cam[t[:, 0]], cam[t[:, 1]], cam[t[:, 2]], r[p]
            l0, l1, l2 = barycentrics(a, b, c, ray)
            N = _cross(b - a, c - a)
            if vn is not None:
                rot = np.stack([(M[d, 0] * vn[:, 0] + M[d, 1] * vn[:, 1]) + M[d, 2] * vn[:, 2] for d in range(3)], axis=1)
                S = (l0[:, None] * rot[t[:, 0]] + l1[:, None] * rot[t[:, 1]]) + l2[:, None] * rot[t[:, 2]]
                ok = (vn[t] != 0).any(axis=2).all(axis=1) & np.isfinite(S).all(axis=1) & (S != 0).any(axis=1)
                N = np.where(ok[:, None], S, N)
            cos = np.abs(_rdot(N, ray)) / np.sqrt(_rdot(N, N) * _rdot(ray, ray))
            alb = np.tile(np.asarray(base, np.float64), (len(p), 1)) if col is None else \
                (l0[:, None] * col[t[:, 0]] + l1[:, None] * col[t[:, 1]]) + l2[:, None] * col[t[:, 2]]
            lin = np.zeros((Hs * Ws, 3))
            lin[p] = np.minimum(np.maximum(alb * (ambient + diffuse * cos)[:, None], 0.0), 1.0)
            lin, cov = lin.reshape(Hs, Ws, 3), (vis["tri"][v] >= 0)
            total, m = np.zeros((H, W, 3)), np.zeros((H, W), np.int64)
            for k in range(ss * ss):  # the pixel's samples in row-major order (an empty one adds 0.0: nothing)
                sy, sx = divmod(k, ss)
                total = total + np.where(cov[sy::ss, sx::ss, None], lin[sy::ss, sx::ss], 0.0)
                m += cov[sy::ss, sx::ss]
            mean = total / np.maximum(m, 1)[..., None]
            val = np.concatenate([255.0 * (srgb_encode(mean) if srgb else mean), (255.0 * m / (ss * ss))[..., None]], axis=2) + 0.5
            rgba[v] = np.where((m > 0)[..., None], np.floor(val), 0).astype(np.uint8)
            loose[v] = (m > 0)[..., None] & (np.abs(val - np.rint(val)) < LOOSE)
    c = ss // 2
    ztop, tcen = vis["zbits"][:, c::ss, c::ss], vis["tri"][:, c::ss, c::ss]
    depth = np.where(tcen >= 0, ztop, 0).astype(np.uint32).view(np.float32)
    und = vis["undecided"].reshape(n, H, ss, W, ss).any(axis=(2, 4))
    return dict(rgba=rgba, depth=depth, tri_id=tcen.astype(np.int32), undecided=und, loose=loose)


# ---- synthetic inputs ------------------------------------------------------------------------------------------------------

def random_views(n, seed, radius=3.0, jitter=0.3):
    """cameras at random places on a shell around the origin, looking near it"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        d = rng.normal(size=3)
        out.append(R.look_at(radius * d / np.linalg.norm(d), rng.normal(0, jitter, 3)))
    return np.stack(out)


def quad(z=2.0, half=0.5):
    """a square in the plane z of the identity camera, two triangles"""
    v = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], np.float64)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def cube():
    """the unit cube, 12 triangles wound outwards -> (verts, tris, the outward axis and sign of each triangle)"""
    v = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    quads = [((0, 1, 3, 2), (0, -1)), ((4, 6, 7, 5), (0, 1)), ((0, 4, 5, 1), (1, -1)), ((2, 3, 7, 6), (1, 1)), ((0, 2, 6, 4), (2, -1)), ((1, 5, 7, 3), (2, 1))]
    t, axes = [], []
    for (a, b, c, d), ax in quads:
        t += [[a, b, c], [a, c, d]]
        axes += [ax, ax]
    return v, np.array(t, np.int32), axes


@functools.lru_cache(maxsize=None)
def view_cases():
    """name -> dict(verts, tris, w2c, H, W, fx, fy, cx, cy, near, far, ss: the factors the case runs at, colors (V, 3) float32):
    every input of the GPU tests that are held to the restatement.  Built once; leave the arrays unchanged."""
    D = R.depth_cases()
    cases = {}

    def add(name, c, ss):
        colors = np.random.default_rng(len(cases)).random((len(c["verts"]), 3)).astype(np.float32)
        cases[name] = dict(c, ss=tuple(ss), colors=colors)

    def new(vt, H, W, w2c=R.IDENT, **k):
        return dict(verts=vt[0], tris=vt[1], w2c=np.asarray(w2c, np.float64), H=H, W=W, near=R.NEAR, far=R.FAR, **(k or R.intrinsics(H, W)))

    add("frame_1x1", D["fills_frame_1x1"], (1, 2, 3, 4))
    # the lane path: a soup of sub-pixel triangles in a 37 x 29 frame (at ss = 3 still boxes of a few samples)
    add("soup_37x29", new(R.soup(800, 7, size=0.04, spread=1.0), 29, 37, w2c=random_views(1, 11, radius=2.6)), (1, 3))
    # the wave path: boxes of 18, 4096 (ss = 1) and 72 (ss = 2) samples; soup_big's boxes lie between the two thresholds
    add("box_9x2", D["box_9x2"], (1, 2))
    add("box_64x64", D["box_64x64"], (1,))
    add("soup_big", D["soup_big"], (1,))
    # the workgroup path: one triangle over a whole 96 x 80 frame, 7680 samples at ss = 1
    add("fill_96x80", new(R._tri([-30, -30, 2.0], [30, -25, 3.0], [0, 40, 2.5]), 80, 96), (1, 2))
    add("crossing", D["crossing"], (1, 2))
    add("rejected_among_good", D["rejected_among_good"], (1, 3))  # zero-area and non-finite triangles among good ones
    # a closed surface from three random cameras: shared vertices (smooth normals), silhouettes, every ss
    add("mesh3", new(R.bumpy_sphere(8, 12, seed=5), 33, 41, w2c=random_views(3, 3)), (1, 2, 3, 4))
    add("mesh1", new(R.bumpy_sphere(8, 12, seed=5), 33, 41, w2c=random_views(1, 4)), (2,))
    return cases


def duplicates_case():
    """two coplanar duplicates (triangles 1 and 3 name the same three vertices) behind a nearer triangle 2 that hides part of
    them, and a farther triangle 0: where the duplicates are the nearest surface the key holds index 1"""
    k = R.intrinsics(29, 37)
    v = np.array([R._unproject(k, 3.2, 2.1, 3.0), R._unproject(k, 33.7, 4.3, 3.3), R._unproject(k, 17.4, 27.2, 2.8),  # the duplicated one
                  R._unproject(k, 1.3, 1.2, 5.0), R._unproject(k, 35.6, 2.1, 5.0), R._unproject(k, 18.1, 28.3, 5.0),  # behind
                  R._unproject(k, 10.2, 8.3, 2.0), R._unproject(k, 20.9, 9.1, 2.0), R._unproject(k, 15.3, 17.7, 2.0)])  # in front
    t = np.array([[3, 4, 5], [0, 1, 2], [6, 7, 8], [0, 1, 2]], np.int32)
    return dict(verts=v, tris=t, w2c=R.IDENT, H=29, W=37, near=R.NEAR, far=R.FAR, **k)


@functools.lru_cache(maxsize=None)
def reference(name, ss, shading="flat", colour="grey", srgb=True):
    """the restatement of view_cases()[name] at `ss`; the visibility is computed once per (name, ss)"""
    c = view_cases()[name]
    return shade(c["verts"], c["tris"], c["w2c"], c["fx"], c["fy"], c["cx"], c["cy"], c["H"], c["W"], ss, shading,
                 c["colors"] if colour == "vertex" else None, srgb=srgb, near=c["near"], far=c["far"], vis=reference_visibility(name, ss))


@functools.lru_cache(maxsize=None)
def reference_visibility(name, ss):
    c = view_cases()[name]
    return visibility(c["verts"], c["tris"], c["w2c"], c["fx"], c["fy"], c["cx"], c["cy"], c["H"], c["W"], ss, c["near"], c["far"])


@functools.lru_cache(maxsize=None)
def cli_mesh():
    """a 200-triangle closed surface and four cameras around it as cameras.json records at 40 x 30"""
    v, t = R.bumpy_sphere(11, 10, seed=9)
    assert len(t) == 200
    w2c = random_views(4, 21, radius=3.5, jitter=0.1)
    records = []
    for k, M in enumerate(w2c):
        c2w = np.linalg.inv(M)
        records.append({"id": k, "img_name": f"view_{k:02d}", "width": 40, "height": 30, "position": c2w[:3, 3].tolist(),
                        "rotation": c2w[:3, :3].tolist(), "fx": 43.7 + k * 0.0, "fy": 44.1})
    return v.astype(np.float32), t, records
