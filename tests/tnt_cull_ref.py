"""The mesh visibility cull (include/gs2m_visibility.h) restated in float64 numpy, brute force over
(triangle, pixel) and (vertex, view), and the synthetic inputs the tests of it share.

The restatement also reports what is UNDECIDED, i.e. what two correct fp64 evaluations of the definitions may settle differently:
  pixel   some (valid) triangle has an edge value within EDGE_TOL of zero there -- the value divided by the lengths of the three
          vectors in the product -- while its other two do not disagree in sign (beyond the same tolerance); or a covering
          triangle is seen edge-on (|dot(n, r)| < EDGE_ON |n| |r|); or a covering sample lies within RANGE_TOL (relative) of near
          or far.
  vertex  in some view one of its comparisons (u and v against the frame, z against 0, z against d + eps) has a margin below
          VOTE_TOL, relative to the size of the quantities compared.
Decided elements have to match the kernels; undecided ones are left out, and an input may hold at most UNDECIDED_CAP of them."""
import functools

import numpy as np

EDGE_TOL = 1e-9
EDGE_ON = 1e-6
RANGE_TOL = 1e-9
VOTE_TOL = 1e-7
UNDECIDED_CAP = 0.01
NEAR, FAR, EPS, MIN_VIEWS = 0.01, 20.0, 0.005, 20


def to_camera(p, M):
    """c_k = ((M[k][0] x + M[k][1] y) + M[k][2] z) + M[k][3] for points p (n, 3) -> (n, 3)"""
    p, M = np.asarray(p, np.float64), np.asarray(M, np.float64)
    return np.stack([((M[k, 0] * p[:, 0] + M[k, 1] * p[:, 1]) + M[k, 2] * p[:, 2]) + M[k, 3] for k in range(3)], axis=1)


def _dot(u, r):
    """(u0 r0 + u1 r1) + u2 r2 of u (T, 3) with r (P, 3) -> (T, P)"""
    return (u[:, 0, None] * r[None, :, 0] + u[:, 1, None] * r[None, :, 1]) + u[:, 2, None] * r[None, :, 2]


def pixel_rays(H, W, fx, fy, cx, cy):
    """the ray through the centre of pixel (i, j), row major over (j, i) -> (H W, 3)"""
    j, i = np.mgrid[0:H, 0:W]
    return np.stack([(i.ravel() + 0.5 - cx) / fx, (j.ravel() + 0.5 - cy) / fy, np.ones(H * W)], axis=1)


def render_depth(verts, tris, w2c, fx, fy, cx, cy, H, W, near=NEAR, far=FAR, chunk=128):
    """-> depth (n_views, H, W) float32 (0: nothing), undecided (n_views, H, W) bool"""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    w2c = np.asarray(w2c, np.float64).reshape(-1, 4, 4)
    r = pixel_rays(H, W, fx, fy, cx, cy)
    rl = np.linalg.norm(r, axis=1)
    depth = np.zeros((len(w2c), H * W), np.float32)
    und = np.zeros((len(w2c), H * W), bool)
    with np.errstate(all="ignore"):
        for k, M in enumerate(w2c):
            cam = to_camera(verts, M)
            best = np.full(H * W, np.inf)
            for t0 in range(0, len(tris), chunk):
                t = tris[t0:t0 + chunk]
                a, b, c = cam[t[:, 0]], cam[t[:, 1]], cam[t[:, 2]]
                n = np.cross(b - a, c - a)
                valid = np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1) & (n != 0).any(1)
                if not valid.any():
                    continue
                a, b, c, n = a[valid], b[valid], c[valid], n[valid]
                w = [_dot(np.cross(u, v), r) for u, v in ((b, c), (c, a), (a, b))]
                pos = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)
                neg = (w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0)
                covered = (pos | neg) & ~((w[0] == 0) & (w[1] == 0) & (w[2] == 0))
                den = _dot(n, r)
                z = ((n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]) + n[:, 2] * a[:, 2])[:, None] / den
                sample = covered & (z >= near) & (z <= far)
                best = np.minimum(best, np.where(sample, z, np.inf).min(axis=0))
                # undecided: an edge value near zero whose two companions do not disagree
                la, lb, lc = (np.linalg.norm(x, axis=1)[:, None] for x in (a, b, c))
                wn = [w[0] / (lb * lc * rl), w[1] / (lc * la * rl), w[2] / (la * lb * rl)]
                for e in range(3):
                    p, q = wn[(e + 1) % 3], wn[(e + 2) % 3]
                    disagree = ((p > EDGE_TOL) & (q < -EDGE_TOL)) | ((p < -EDGE_TOL) & (q > EDGE_TOL))
                    und[k] |= (~(np.abs(wn[e]) >= EDGE_TOL) & ~disagree).any(axis=0)
                edge_on = np.abs(den) < EDGE_ON * np.linalg.norm(n, axis=1)[:, None] * rl
                at_range = (np.abs(z - near) <= RANGE_TOL * near) | (np.abs(z - far) <= RANGE_TOL * far)
                und[k] |= (covered & (edge_on | at_range)).any(axis=0)
            depth[k] = np.where(np.isfinite(best), best, 0.0).astype(np.float32)
    return depth.reshape(len(w2c), H, W), und.reshape(len(w2c), H, W)


def bilinear(depth, u, v):
    """the contract's sample of depth (H, W) at texel coordinates u, v (n,), all within the frame -> (n,) fp64"""
    D = np.asarray(depth, np.float64)
    H, W = D.shape
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    tx, ty = u - x0, v - y0
    right, below = x0 + 1 < W, y0 + 1 < H
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    d00, d01 = D[y0, x0], np.where(right, D[y0, x1], 0.0)
    d10, d11 = np.where(below, D[y1, x0], 0.0), np.where(right & below, D[y1, x1], 0.0)
    return ((d00 * ((1 - tx) * (1 - ty)) + d01 * (tx * (1 - ty))) + d10 * ((1 - tx) * ty)) + d11 * (tx * ty)


def view_votes(verts, M, fx, fy, cx, cy, depth, eps=EPS, tol=VOTE_TOL):
    """one view -> dict(vote, undecided, inside, front, u, v, z, d) over the vertices"""
    p = np.asarray(verts, np.float64).reshape(-1, 3)
    M = np.asarray(M, np.float64)
    H, W = depth.shape
    with np.errstate(all="ignore"):
        c = to_camera(p, M)
        z = c[:, 2] + 1e-8
        u, v = (fx * c[:, 0] + cx * c[:, 2]) / z, (fy * c[:, 1] + cy * c[:, 2]) / z
        inside = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & (z > 0)
        uc, vc = np.where(inside, u, 0.0), np.where(inside, v, 0.0)
        d = bilinear(depth, uc, vc)
        front = np.where(d > 0, z < d + eps, True)
        # margins, each relative to the size of what is compared
        zs = (np.abs(M[2, 0] * p[:, 0]) + np.abs(M[2, 1] * p[:, 1])) + np.abs(M[2, 2] * p[:, 2]) + np.abs(M[2, 3]) + 1e-8
        und = ~(np.abs(z) >= tol * zs)
        for x, hi in ((u, W - 1), (v, H - 1)):
            s = max(hi, 1)
            und |= ~(np.abs(x) >= tol * s) | ~(np.abs(x - hi) >= tol * s)
        und |= inside & (d > 0) & ~(np.abs(z - (d + eps)) >= tol * np.maximum(np.abs(z), np.abs(d + eps)))
    return {"vote": inside & front, "undecided": und, "inside": inside, "front": front, "u": u, "v": v, "z": z, "d": d}


def votes(verts, w2c, fx, fy, cx, cy, depth, eps=EPS, tol=VOTE_TOL, undecided_pixels=None):
    """-> votes (V,) int32, undecided (V,) bool.  undecided_pixels (n_views, H, W): a vertex whose sample reads one of them is
    undecided too (depth maps that come out of the rasterizer)."""
    n = len(np.asarray(verts).reshape(-1, 3))
    tot, und = np.zeros(n, np.int32), np.zeros(n, bool)
    for k, (M, D) in enumerate(zip(np.asarray(w2c, np.float64).reshape(-1, 4, 4), depth)):
        r = view_votes(verts, M, fx, fy, cx, cy, D, eps, tol)
        tot += r["vote"]
        und |= r["undecided"]
        if undecided_pixels is not None:
            H, W = D.shape
            ins = r["inside"]
            x0, y0 = np.floor(np.where(ins, r["u"], 0.0)).astype(np.int64), np.floor(np.where(ins, r["v"], 0.0)).astype(np.int64)
            x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
            U = undecided_pixels[k]
            und |= ins & (U[y0, x0] | U[y0, x1] | U[y1, x0] | U[y1, x1])
    return tot, und


def cull_mesh(verts, tris, vote_counts, min_views=MIN_VIEWS):
    """the vertices with enough votes, the faces whose three vertices are kept, then only the vertices those faces name:
    -> (vertices, triangles int32 renumbered, the final vertex mask)"""
    keep = np.asarray(vote_counts) >= min_views
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    faces = t[keep[t].all(axis=1)] if len(t) else t
    used = np.zeros(len(keep), bool)
    used[faces.ravel()] = True
    new_id = np.cumsum(used) - 1
    return np.asarray(verts)[used], new_id[faces].astype(np.int32), used


# ---- synthetic inputs ------------------------------------------------------------------------------------------------------

def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """world-to-camera (4, 4), OpenCV convention (z forward, y down), of a camera at `eye` looking at `target`"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    zc = (target - eye) / np.linalg.norm(target - eye)
    xc = np.cross(-np.asarray(up, np.float64), zc)
    xc /= np.linalg.norm(xc)
    R = np.stack([xc, np.cross(zc, xc), zc])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, -R @ eye
    return M


def ring_views(n, radius=4.0, height=0.7, target=(0.0, 0.0, 0.0), phase=0.2):
    return np.stack([look_at([radius * np.cos(a), height * np.sin(2 * a), radius * np.sin(a)], target)
                     for a in phase + 2 * np.pi * np.arange(n) / max(n, 1)]) if n else np.zeros((0, 4, 4))


def intrinsics(H, W, fov=1.1):
    """a pinhole whose principal point is off the frame's centre by a fraction of a pixel"""
    f = 0.5 * max(W, H) / np.tan(0.5 * fov)
    return dict(fx=f, fy=f * 1.01, cx=0.5 * W + 0.13, cy=0.5 * H - 0.21)


def soup(n_tris, seed, size=0.05, spread=1.2):
    """n small triangles scattered through a ball around the origin (no shared vertices)"""
    rng = np.random.default_rng(seed)
    centre = rng.normal(size=(n_tris, 1, 3))
    centre *= spread * rng.random((n_tris, 1, 1)) ** (1 / 3) / np.linalg.norm(centre, axis=2, keepdims=True)
    v = (centre + rng.normal(0, size, (n_tris, 3, 3))).reshape(-1, 3)
    return v, np.arange(3 * n_tris, dtype=np.int32).reshape(-1, 3)


def bumpy_sphere(n_lat, n_lon, seed=0, radius=1.0):
    """a closed surface with relief: a latitude-longitude grid without its poles, the seam closed"""
    rng = np.random.default_rng(seed)
    th = np.pi * (np.arange(n_lat) + 0.5) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    T, P = np.meshgrid(th, ph, indexing="ij")
    r = radius * (1 + 0.25 * np.sin(3 * T + 0.5) * np.cos(2 * P) + 0.1 * np.cos(5 * P + 1.0) * np.sin(T) ** 2)
    v = (r[..., None] * np.stack([np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)], -1)).reshape(-1, 3)
    v += rng.normal(0, 1e-3, v.shape)
    idx = np.arange(n_lat * n_lon).reshape(n_lat, n_lon)
    a, b, c, d = idx[:-1], np.roll(idx, -1, 1)[:-1], idx[1:], np.roll(idx, -1, 1)[1:]
    t = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)])
    return v, t.astype(np.int32)


def _tri(*p):
    return np.asarray(p, np.float64).reshape(-1, 3), np.arange(len(p), dtype=np.int32).reshape(-1, 3)


def _unproject(k, i, j, z):
    """the point at depth z on the ray through frame position (i, j) (pixel centres at half integers) of the identity camera"""
    return [(i - k["cx"]) / k["fx"] * z, (j - k["cy"]) / k["fy"] * z, z]


def _box_triangle(k, x0, y0, bw, bh, z, skew=0.0):
    """a right triangle in the plane z whose pixel box under the rasterizer's rule -- columns floor(u_min - 0.5 - 1e-6) to
    ceil(u_max - 0.5 + 1e-6), rows alike, clamped to the frame -- is the columns [x0, x0 + bw) and the rows [y0, y0 + bh):
    its corners sit three quarters of a pixel inside that box (bw, bh >= 2)"""
    return _tri(_unproject(k, x0 + 0.75, y0 + 0.75, z), _unproject(k, x0 + bw - 0.75, y0 + 0.75, z), _unproject(k, x0 + 0.75 + skew, y0 + bh - 0.75, z))


IDENT = np.eye(4)[None]


@functools.lru_cache(maxsize=None)
def depth_cases():
    """name -> dict(verts, tris, w2c, H, W, fx, fy, cx, cy, near, far): every input of the GPU depth tests.  Built once; leave
    the arrays unchanged."""
    cases = {}

    def add(name, vt, H, W, w2c=IDENT, near=NEAR, far=FAR, **k):
        k = k or intrinsics(H, W)
        cases[name] = dict(verts=vt[0], tris=vt[1], w2c=np.asarray(w2c, np.float64), H=H, W=W, near=near, far=far, **k)

    k75, k64, k65 = intrinsics(5, 7), intrinsics(64, 64), intrinsics(129, 65)
    # covers no centre: a sliver between the centres of pixels (2, 2) and (3, 2)
    add("no_centre", _tri(_unproject(k75, 2.6, 2.2, 2.0), _unproject(k75, 2.9, 2.3, 2.0), _unproject(k75, 2.7, 2.8, 2.0)), 5, 7)
    add("one_centre", _tri(_unproject(k75, 3.1, 2.2, 2.0), _unproject(k75, 3.9, 2.3, 2.5), _unproject(k75, 3.4, 2.9, 3.0)), 5, 7)
    big = _tri([-30, -30, 2.0], [30, -25, 3.0], [0, 40, 2.5])
    add("fills_frame_1x1", big, 1, 1)
    add("fills_frame_7x5", big, 5, 7)
    add("fills_frame_64", big, 64, 64)
    add("fills_frame_65x129", big, 129, 65)
    add("behind", _tri([-1, -1, -2.0], [1, -1, -3.0], [0, 1, -2.5]), 64, 64)
    add("crossing", _tri([-0.8, -0.3, 3.0], [0.9, -0.2, 2.0], [0.1, 0.4, -1.5]), 64, 64)
    add("crossing_65x129", _tri([-0.8, -0.3, -1.0], [0.9, -0.2, 2.0], [0.1, 1.4, 2.5]), 129, 65)
    v = np.array([[-1, -1, 25.0], [1, -1, 26.0], [0, 1, 25.5], [-0.001, -0.001, 0.004], [0.001, -0.001, 0.005], [0, 0.001, 0.0045],
                  [-1, -1, 15.0], [1, -1, 30.0], [0, 1, 18.0]])
    add("near_far", (v, np.arange(9, dtype=np.int32).reshape(3, 3)), 64, 64)
    v = np.array([[-1, -1, 3.0], [1, -1, 3.0], [0, 1, 3.5], [0.2, 0.2, 2.0], [0.4, 0.4, 2.0], [0.6, 0.6, 2.0],  # collinear
                  [0.1, 0.1, 2.5], [np.nan, 0, 2.0], [0.5, -0.5, 2.0], [0.3, 0.3, 1.0]])
    t = np.array([[0, 1, 2], [3, 4, 5], [6, 6, 8], [7, 8, 9], [9, 9, 9]], np.int32)
    add("rejected_among_good", (v, t), 64, 64)
    v = np.array([[-1, -1, 3.0], [1, -1, 3.2], [0, 1, 3.4], [-0.5, -0.8, 2.0], [0.9, 0.1, 4.5], [-0.2, 0.7, 2.6]])
    add("overlap", (v, np.arange(6, dtype=np.int32).reshape(2, 3)), 64, 64)
    q = np.array([_unproject(k64, 5.3, 4.2, 2.0), _unproject(k64, 50.7, 6.1, 2.4), _unproject(k64, 55.2, 58.6, 3.0), _unproject(k64, 7.9, 52.3, 2.2)])
    add("quad", (q, np.array([[0, 1, 2], [0, 2, 3]], np.int32)), 64, 64)
    # the clamped box against the two thresholds of the rasterizer: 16 pixels (a lane / a wave) and 4096 (a wave / a workgroup row)
    add("box_4x4", _box_triangle(k64, 10, 20, 4, 4, 2.0), 64, 64)
    add("box_9x2", _box_triangle(k64, 10, 20, 9, 2, 2.0), 64, 64)
    # 17 x 1: a box of one row only exists at the frame's edge (rows -1 .. 0 clamped to row 0); it holds no centre
    add("box_17x1_edge", _tri(_unproject(k64, 10.75, -0.3, 2.0), _unproject(k64, 26.25, -0.3, 2.0), _unproject(k64, 10.75, 0.4, 2.0)), 64, 64)
    add("box_64x64", _box_triangle(k65, 0, 30, 64, 64, 2.0, skew=0.31), 129, 65)
    add("box_65x64", _box_triangle(k65, 0, 30, 65, 64, 2.0, skew=0.31), 129, 65)
    add("soup", soup(3000, 1), 129, 65, w2c=ring_views(1))
    add("soup_big", soup(600, 2, size=0.3), 64, 64, w2c=ring_views(1, radius=2.0))
    add("views3", soup(1500, 3, size=0.12), 64, 64, w2c=ring_views(3, radius=1.0))  # the cameras sit inside the soup
    return cases


TIE = dict(fx=4.0, fy=4.0, cx=2.0, cy=2.0, H=5, W=7)


def tie_case():
    """Small dyadic numbers, every product exact in fp64.  The identity camera, fx = fy = 4, cx = cy = 2: the centre of pixel
    (i, j) has the ray ((i - 1.5) / 4, (j - 1.5) / 4, 1).  One triangle in the plane z = 4 with its corners on the rays of the
    centres (1, 1), (5, 1) and (1, 4): the centres on its three edges and at its three corners are covered, the neighbours
    beyond them are not.  -> (verts, tris, the expected coverage (5, 7) bool)"""
    ray = lambda i, j: [(i - 1.5), (j - 1.5), 4.0]  # noqa: E731  (z = 4 times the ray)
    v, t = _tri(ray(1, 1), ray(5, 1), ray(1, 4))
    cov = np.zeros((5, 7), bool)
    for j in range(5):
        for i in range(7):
            # inside or on: i >= 1, j >= 1, (i - 1) / 4 + (j - 1) / 3 <= 1, in integers
            cov[j, i] = i >= 1 and j >= 1 and 3 * (i - 1) + 4 * (j - 1) <= 12
    return v, t, cov


@functools.lru_cache(maxsize=None)
def depth_reference(name):
    c = depth_cases()[name]
    return render_depth(c["verts"], c["tris"], c["w2c"], c["fx"], c["fy"], c["cx"], c["cy"], c["H"], c["W"], c["near"], c["far"])


def random_depth(n, H, W, seed):
    """depth maps with smooth relief and holes (zero regions)"""
    rng = np.random.default_rng(seed)
    j, i = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.float32)
    for k in range(n):
        d = 3.0 + 0.8 * np.sin(0.23 * i + k) * np.cos(0.17 * j - k) + rng.normal(0, 0.02, (H, W))
        d[((i - rng.uniform(0, W)) ** 2 + (j - rng.uniform(0, H)) ** 2) < (0.3 * min(H, W)) ** 2] = 0.0
        d[rng.random((H, W)) < 0.03] = 0.0
        out[k] = d
    return out


@functools.lru_cache(maxsize=None)
def vote_case(n_views=3, H=64, W=65, n=6000, seed=5):
    """Vertices thrown against given depth maps: through the frustum around the maps' depth, behind the camera, off the frame,
    a shade inside and outside the frame's border, a shade in front of and behind d + eps, and over holes.
    -> dict(verts, w2c, depth, votes, undecided, views: the per-view details, the intrinsics)"""
    rng = np.random.default_rng(seed)
    k = intrinsics(H, W)
    w2c = ring_views(n_views, radius=0.5, height=0.1, target=(0.0, 0.0, 5.0))
    depth = random_depth(n_views, H, W, seed + 1)
    c2w0 = np.linalg.inv(w2c[0])
    pts = []
    u, v = rng.uniform(-8, W + 7, n), rng.uniform(-8, H + 7, n)
    z = rng.uniform(1.5, 4.5, n)
    z[: n // 10] = -z[: n // 10]
    pts.append(np.stack([(u - k["cx"]) / k["fx"] * z, (v - k["cy"]) / k["fy"] * z, z], 1))
    m = 400
    side = rng.integers(0, 4, m)
    off = np.where(rng.random(m) < 0.5, -1e-4, 1e-4)  # a ten-thousandth of a pixel inside or outside the border
    ub = np.where(side == 0, off, np.where(side == 1, W - 1 + off, rng.uniform(1, W - 2, m)))
    vb = np.where(side == 2, off, np.where(side == 3, H - 1 + off, rng.uniform(1, H - 2, m)))
    zb = rng.uniform(2.0, 3.0, m)
    pts.append(np.stack([(ub - k["cx"]) / k["fx"] * zb, (vb - k["cy"]) / k["fy"] * zb, zb], 1))
    # just in front of and just behind d + eps of view 0
    us, vs = rng.uniform(0, W - 1, m), rng.uniform(0, H - 1, m)
    d = bilinear(depth[0], us, vs)
    zs = np.where(d > 0, d + EPS + np.where(rng.random(m) < 0.5, -1e-5, 1e-5), rng.uniform(1.0, 6.0, m))  # over a hole: any depth
    pts.append(np.stack([(us - k["cx"]) / k["fx"] * zs, (vs - k["cy"]) / k["fy"] * zs, zs], 1))
    cam = np.concatenate(pts)
    verts = cam @ c2w0[:3, :3].T + c2w0[:3, 3]
    verts[7] = np.nan
    views = [view_votes(verts, w2c[q], k["fx"], k["fy"], k["cx"], k["cy"], depth[q]) for q in range(n_views)]
    tot, und = votes(verts, w2c, k["fx"], k["fy"], k["cx"], k["cy"], depth)
    return dict(verts=verts, w2c=w2c, depth=depth, votes=tot, undecided=und, views=views, H=H, W=W, **k)


@functools.lru_cache(maxsize=None)
def cull_case(n_views=9, H=48, W=64, n_lat=16, n_lon=24, min_views=3, eps=0.1):
    """A closed bumpy surface inside a ring of cameras, plus an inner shell no camera sees: rendered and voted on by the
    restatement, the undecided vertices (and the faces naming them) taken out, and that mesh's cull.  eps is wide: in so small
    a frame the half pixel between rendering and sampling moves the sampled depth by more than the reference's 0.005.
    -> dict(verts, tris, w2c, intrinsics, min_views, eps, votes, culled_verts, culled_tris)"""
    k = intrinsics(H, W, fov=0.9)
    w2c = ring_views(n_views, radius=3.2, height=0.8)
    vo, to = bumpy_sphere(n_lat, n_lon, seed=3)
    vi, ti = bumpy_sphere(n_lat // 2, n_lon // 2, seed=4, radius=0.5)
    verts, tris = np.concatenate([vo, vi]), np.concatenate([to, ti + len(vo)])
    for _ in range(4):  # taking vertices out changes the surface: until nothing is undecided any more
        depth, upix = render_depth(verts, tris, w2c, k["fx"], k["fy"], k["cx"], k["cy"], H, W)
        # the rasterizer's depth may differ from this one by an fp32 ulp (6e-8 relative): ten times VOTE_TOL covers it
        tot, und = votes(verts, w2c, k["fx"], k["fy"], k["cx"], k["cy"], depth, eps, tol=10 * VOTE_TOL, undecided_pixels=upix)
        if not und.any():
            break
        new_id = np.cumsum(~und) - 1
        tris = new_id[tris[(~und)[tris].all(axis=1)]].astype(np.int32)
        verts = verts[~und]
    assert not und.any()
    cv, ct, used = cull_mesh(verts, tris, tot, min_views)
    return dict(verts=verts, tris=tris, w2c=w2c, H=H, W=W, min_views=min_views, eps=eps, votes=tot, depth=depth, culled_verts=cv,
                culled_tris=ct, used=used, **k)
