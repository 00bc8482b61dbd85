"""The per-vertex attribute bake (include/gs2m_meshbake.h) and the G-buffer and RGB resolve of the mesh views
(include/gs2m_meshview.h) restated in float64 numpy, operation for operation, and the synthetic inputs the tests of them share.
Not collected.

Both sides evaluate the same IEEE fp64 expressions; what could still differ is the last place of a division or a square root taken
by another library.  A decision (inside, front, mask, w > 0) can only come out differently where its operands lie within such a
rounding of the threshold, so every view of a vertex reports `margin`: the smallest non-zero distance of a compared value from its
threshold.  A distance of exactly 0 is allowed: the edge-case vertices sit on their thresholds by construction, with operands for
which both sides compute the same exact value.  tests/test_mesh_bake.py asserts margin >= MARGIN for the GPU test's scene."""
import functools

import numpy as np

import mesh_view_ref as MV
import tnt_cull_ref as R

MARGIN = 1e-9
EPS = 0.005


def _rdot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def camera_centre(M):
    return np.array([-((M[0, k] * M[0, 3] + M[1, k] * M[1, 3]) + M[2, k] * M[2, 3]) for k in range(3)])


def taps(u, v, H, W):
    """-> x0, y0, tx, ty, the four tap weights (w00, w01, w10, w11) and whether each tap lies in the frame"""
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    tx, ty = u - x0, v - y0
    right, below = x0 + 1 < W, y0 + 1 < H
    w = ((1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty)
    return x0, y0, tx, ty, w, (np.ones_like(right), right, below, right & below)


def bake_view(verts, normals, M, fx, fy, cx, cy, depth, maps, mask=None, eps=EPS):
    """one view -> dict(use (V,) bool: the view contributes; w (V,); a (V, C); inside, front, unmasked, lit (V,) bool; margin (V,))"""
    p = np.asarray(verts, np.float64).reshape(-1, 3)
    M = np.asarray(M, np.float64)
    maps = np.asarray(maps, np.float32)
    C, H, W = maps.shape
    V = len(p)
    with np.errstate(all="ignore"):
        c = R.to_camera(p, M)
        z = c[:, 2] + 1e-8
        u, v = (fx * c[:, 0] + cx * c[:, 2]) / z, (fy * c[:, 1] + cy * c[:, 2]) / z
        inside = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & (z > 0)
        margin = np.full(V, np.inf)

        def near(d, where=None):
            d = np.abs(d)
            d = np.where((d > 0) & (np.ones(V, bool) if where is None else where), d, np.inf)
            np.minimum(margin, d, out=margin)

        for x, hi in ((u, W - 1), (v, H - 1)):
            near(x), near(x - hi)
        near(z)
        uc, vc = np.where(inside, u, 0.0), np.where(inside, v, 0.0)
        d = R.bilinear(depth, uc, vc)
        front = np.where(d > 0, z < d + eps, True)
        near(z - (d + eps), inside & (d > 0))
        near(d, inside)
        x0, y0, tx, ty, tw, exists = taps(uc, vc, H, W)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        unmasked = np.ones(V, bool)
        if mask is not None:
            K = np.asarray(mask, np.float32)
            for (yy, xx), w_k, ex in zip(((y0, x0), (y0, x1), (y1, x0), (y1, x1)), tw, exists):
                counts = ex & (w_k != 0)
                unmasked &= ~counts | (K[yy, xx] >= np.float32(0.5))
                near(w_k, inside & ex)
                near(K[yy, xx].astype(np.float64) - 0.5, inside & counts)
        if normals is None:
            w = np.ones(V)
            lit = np.ones(V, bool)
        else:
            N = np.asarray(normals, np.float64).reshape(-1, 3)
            e = camera_centre(M)[None] - p
            w = np.maximum(0.0, _rdot(N, e) / np.sqrt(_rdot(N, N) * _rdot(e, e)))
            ok = np.isfinite(N).all(axis=1) & (N != 0).any(axis=1)
            w = np.where(ok, w, 0.0)
            lit = w > 0  # NaN fails
            near(_rdot(N, e) / np.sqrt(_rdot(N, N) * _rdot(e, e)), ok)
        a = np.stack([R.bilinear(maps[k], uc, vc) for k in range(C)], axis=1)
        use = inside & front & unmasked & lit
    return dict(use=use, w=w, a=a, inside=inside, front=front, unmasked=unmasked, lit=lit, margin=margin, u=u, v=v, z=z, d=d)


def accumulate(verts, normals, w2c, fx, fy, cx, cy, depth, maps, mask=None, eps=EPS, sums=None, weights=None):
    """-> (sums (V, C), weights (V,), use (V, n_views) bool, margin (V, n_views)); sums, weights: the values to start from"""
    p = np.asarray(verts, np.float64).reshape(-1, 3)
    w2c = np.asarray(w2c, np.float64).reshape(-1, 4, 4)
    C = np.asarray(maps).shape[1]
    sums = np.zeros((len(p), C)) if sums is None else np.array(sums, np.float64)
    weights = np.zeros(len(p)) if weights is None else np.array(weights, np.float64)
    use, margin = np.zeros((len(p), len(w2c)), bool), np.full((len(p), len(w2c)), np.inf)
    for k, M in enumerate(w2c):
        r = bake_view(p, normals, M, fx, fy, cx, cy, depth[k], maps[k], None if mask is None else mask[k], eps)
        u = r["use"]
        sums[u] = sums[u] + r["w"][u, None] * r["a"][u]
        weights[u] = weights[u] + r["w"][u]
        use[:, k], margin[:, k] = u, r["margin"]
    return sums, weights, use, margin


def resolve(sums, weights, min_weight, fallback):
    seen = (weights >= min_weight) & (weights > 0)
    with np.errstate(all="ignore"):
        out = np.where(seen[:, None], (sums / weights[:, None]).astype(np.float32), np.asarray(fallback, np.float32)[None])
    return out.astype(np.float32), seen


# ---- G-buffer and resolve ------------------------------------------------------------------------------------------------------

def gbuffer(verts, tris, w2c, fx, fy, cx, cy, H, W, ss, tri, albedo, roughness, metallic, shading="smooth"):
    """tri (n, H ss, W ss) int64: the triangle of each sample's key, -1 where empty; an index >= len(tris), or a triangle that names
    a vertex out of range, is an empty sample.  -> dict of float32 arrays (normal, view_dir, albedo (.., 3); roughness, metallic
    (..,)) and coverage uint8, each rounded once from the fp64 value."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    w2c = np.asarray(w2c, np.float64).reshape(-1, 4, 4)
    Hs, Ws = H * ss, W * ss
    rays = R.pixel_rays(Hs, Ws, ss * fx, ss * fy, ss * cx, ss * cy)
    vn = MV.vertex_normal_sums(verts, tris)[2] if shading == "smooth" else None
    att = np.concatenate([np.asarray(albedo, np.float32).reshape(-1, 3), np.asarray(roughness, np.float32).reshape(-1, 1),
                          np.asarray(metallic, np.float32).reshape(-1, 1)], axis=1).astype(np.float64)
    n = len(w2c)
    out = np.zeros((n, Hs * Ws, 11), np.float32)
    cov = np.zeros((n, Hs * Ws), np.uint8)
    with np.errstate(all="ignore"):
        for v, M in enumerate(w2c):
            cam = R.to_camera(verts, M)
            key = np.asarray(tri[v]).ravel()
            ok = (key >= 0) & (key < len(tris))
            t_all = tris[np.where(ok, key, 0)]
            ok &= ((t_all >= 0) & (t_all < len(verts))).all(axis=1)
            p = np.nonzero(ok)[0]
            t = t_all[p]
            a, b, c, ray = cam[t[:, 0]], cam[t[:, 1]], cam[t[:, 2]], rays[p]
            l0, l1, l2 = MV.barycentrics(a, b, c, ray)
            N = MV._cross(b - a, c - a)
            if vn is not None:
                rot = np.stack([(M[d, 0] * vn[:, 0] + M[d, 1] * vn[:, 1]) + M[d, 2] * vn[:, 2] for d in range(3)], axis=1)
                S = (l0[:, None] * rot[t[:, 0]] + l1[:, None] * rot[t[:, 1]]) + l2[:, None] * rot[t[:, 2]]
                good = (vn[t] != 0).any(axis=2).all(axis=1) & np.isfinite(S).all(axis=1) & (S != 0).any(axis=1)
                N = np.where(good[:, None], S, N)
            N = np.where((MV._rdot(N, ray) > 0)[:, None], -N, N)
            back = -ray
            world = lambda x: np.stack([(M[0, k] * x[:, 0] + M[1, k] * x[:, 1]) + M[2, k] * x[:, 2] for k in range(3)], axis=1)
            Nw, Vw = world(N), world(back)
            val = np.concatenate([Nw / np.sqrt(MV._rdot(Nw, Nw))[:, None], Vw / np.sqrt(MV._rdot(Vw, Vw))[:, None],
                                  (l0[:, None] * att[t[:, 0]] + l1[:, None] * att[t[:, 1]]) + l2[:, None] * att[t[:, 2]]], axis=1)
            out[v, p] = val.astype(np.float32)
            cov[v, p] = 1
    s = (n, Hs, Ws)
    return dict(normal=out[..., 0:3].reshape(s + (3,)), view_dir=out[..., 3:6].reshape(s + (3,)), albedo=out[..., 6:9].reshape(s + (3,)),
                roughness=out[..., 9].reshape(s), metallic=out[..., 10].reshape(s), coverage=cov.reshape(s))


def resolve_rgb(rgb, coverage, ss, srgb=False, background=None):
    """rgb (n, H ss, W ss, 3) float32, coverage (n, H ss, W ss) -> (n, H, W, 4) uint8"""
    rgb = np.asarray(rgb, np.float32).astype(np.float64)
    cov = np.asarray(coverage) != 0
    n, Hs, Ws, _ = rgb.shape
    H, W = Hs // ss, Ws // ss
    lin = np.minimum(np.maximum(np.where(np.isnan(rgb), 0.0, rgb), 0.0), 1.0)
    total, m = np.zeros((n, H, W, 3)), np.zeros((n, H, W), np.int64)
    for k in range(ss * ss):
        sy, sx = divmod(k, ss)
        total = total + np.where(cov[:, sy::ss, sx::ss, None], lin[:, sy::ss, sx::ss], 0.0)
        m += cov[:, sy::ss, sx::ss]
    mean = total / np.maximum(m, 1)[..., None]
    enc = np.where((m > 0)[..., None], MV.srgb_encode(mean) if srgb else mean, 0.0)
    a = m / float(ss * ss)
    out = np.zeros((n, H, W, 4), np.uint8)
    if background is not None:
        bg = np.asarray(background, np.float32).astype(np.float64)
        bg = np.minimum(np.maximum(np.where(np.isnan(bg), 0.0, bg), 0.0), 1.0)
        out[..., :3] = np.floor(255.0 * (a[..., None] * enc + (1.0 - a)[..., None] * bg) + 0.5).astype(np.uint8)
        out[..., 3] = 255
    else:
        val = np.concatenate([255.0 * enc, (255.0 * a)[..., None]], axis=3) + 0.5
        out = np.where((m > 0)[..., None], np.floor(val), 0).astype(np.uint8)
    return out


# ---- synthetic inputs ------------------------------------------------------------------------------------------------------

BAKE_FRAME = dict(H=16, W=24, fx=20.0, fy=20.0, cx=12.0, cy=8.0)
EDGE_NAMES = ("outside", "behind", "corner", "occluded", "depth0", "backfacing", "grazing", "masked_zero_weight", "masked_tap")


def _solve(f, x, target, span=4096):
    """the double nearest x (within `span` places) at which f(x) == target exactly"""
    lo = hi = x
    for _ in range(span):
        for cand in (lo, hi):
            if f(cand) == target:
                return cand
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    raise AssertionError("no exact solution nearby")


@functools.lru_cache(maxsize=None)
def bake_case():
    """The small scene of the GPU test.  A 12 x 12 grid patch at z = 3 facing the cameras, an occluder quad at z = 2 in front of its
    left third, and one isolated vertex per edge case of view 0 (the identity camera), EDGE_NAMES in order, at the end.
    -> dict(verts, tris, normals, w2c (3), H, W, fx, fy, cx, cy, depth (3, H, W) float32: the restatement's z-buffer, maps (3, 5, H, W)
    float32, mask (3, H, W) float32, eps, edge: name -> vertex index).  Built once; leave the arrays unchanged."""
    k = BAKE_FRAME
    g = np.linspace(-1.0, 1.0, 12)
    X, Y = np.meshgrid(g, g)
    patch = np.stack([X.ravel(), Y.ravel(), np.full(144, 3.0)], axis=1)
    idx = np.arange(144).reshape(12, 12)
    quads = np.stack([idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()], axis=1)
    tris = np.concatenate([quads[:, [0, 2, 1]], quads[:, [0, 3, 2]]])  # wound so that the face normals point to -z: the cameras
    # a second, finer layer of loose vertices on the patch (no triangles of their own): ~150 more samples between the grid's
    rng = np.random.default_rng(3)
    loose = np.stack([rng.uniform(-0.95, 0.95, 150), rng.uniform(-0.95, 0.95, 150), np.full(150, 3.0)], axis=1)
    occ = np.array([[-1.1, -1.2, 2.0], [-0.35, -1.2, 2.0], [-0.35, 1.2, 2.0], [-1.1, 1.2, 2.0]])
    n0 = 144 + 150
    tris = np.concatenate([tris, [[n0, n0 + 2, n0 + 1], [n0, n0 + 3, n0 + 2]]]).astype(np.int32)
    proj_u = lambda x, z: (k["fx"] * x + k["cx"] * z) / (z + 1e-8)
    proj_v = lambda y, z: (k["fy"] * y + k["cy"] * z) / (z + 1e-8)
    guess = lambda t, f, c, z: (t * (z + 1e-8) - c * z) / f
    xc = _solve(lambda x: proj_u(x, 2.5), guess(k["W"] - 1, k["fx"], k["cx"], 2.5), float(k["W"] - 1))
    yc = _solve(lambda y: proj_v(y, 2.5), guess(k["H"] - 1, k["fy"], k["cy"], 2.5), float(k["H"] - 1))
    xz = _solve(lambda x: proj_u(x, 3.0), guess(21.0, k["fx"], k["cx"], 3.0), 21.0)  # u = 21 exactly: the right taps weigh 0
    edge = np.array([[3.0, 0.0, 3.0],        # outside the frame
                     [0.0, 0.0, -1.0],       # z <= 0
                     [xc, yc, 2.5],          # u = W - 1, v = H - 1
                     [-0.8, 0.1, 3.5],       # behind the occluder and the patch by more than eps
                     [1.45, 0.07, 3.0],      # nothing rendered around it: d = 0, front
                     [1.4, 0.5, 3.0],        # its normal points away
                     [1.45, -0.5, 3.0],      # its normal is at a right angle to the ray: w = 0
                     [xz, -0.77, 3.0],       # u = 21: the masked taps at x = 22 weigh 0
                     [1.25, 0.93, 3.0]])     # a masked tap of non-zero weight
    verts = np.concatenate([patch, loose, occ, edge])
    normals = np.tile([0.0, 0.0, -1.0], (len(verts), 1))
    e0 = len(verts) - len(edge)
    names = {n: e0 + i for i, n in enumerate(EDGE_NAMES)}
    normals[names["backfacing"]] = (0.0, 0.0, 1.0)
    normals[names["grazing"]] = (3.0, 0.0, -1.45)
    w2c = np.stack([np.eye(4), R.look_at([0.6, 0.2, -0.3], [0.05, 0.0, 3.0]), R.look_at([-0.5, -0.3, 0.2], [0.0, 0.1, 3.0])])
    depth, _ = R.render_depth(verts, tris, w2c, k["fx"], k["fy"], k["cx"], k["cy"], k["H"], k["W"])
    maps = rng.random((3, 5, k["H"], k["W"])).astype(np.float32)
    mask = (rng.random((3, k["H"], k["W"])) > 0.06).astype(np.float32)
    r = bake_view(verts, None, w2c[0], k["fx"], k["fy"], k["cx"], k["cy"], depth[0], maps[0])
    fl = lambda i, key: int(np.floor(r[key][names[i]]))
    for n in ("corner", "depth0", "backfacing", "grazing", "masked_zero_weight", "masked_tap"):  # their taps in view 0 are foreground ...
        x0, y0 = fl(n, "u"), fl(n, "v")
        mask[0, y0:y0 + 2, x0:x0 + 2] = 1.0
    x0, y0 = fl("masked_zero_weight", "u"), fl("masked_zero_weight", "v")
    mask[0, y0:y0 + 2, x0 + 1] = 0.0          # ... but these two, of weight 0,
    mask[0, fl("masked_tap", "v"), fl("masked_tap", "u")] = 0.0  # and this one, of weight > 0
    return dict(verts=verts, tris=tris, normals=normals, w2c=w2c, depth=depth, maps=maps, mask=mask, eps=EPS, edge=names, **k)


@functools.lru_cache(maxsize=None)
def bake_reference(channels=5, masked=True, with_normals=True):
    c = bake_case()
    return accumulate(c["verts"], c["normals"] if with_normals else None, c["w2c"], c["fx"], c["fy"], c["cx"], c["cy"], c["depth"],
                      c["maps"][:, :channels], c["mask"] if masked else None, c["eps"])


@functools.lru_cache(maxsize=None)
def gbuffer_case():
    """Two triangles sharing an edge, and one crossing the camera plane, in a 16 x 12 frame from a slightly turned camera; vertex
    attributes in [0, 1].  -> dict(verts, tris, w2c (1), H, W, fx, fy, cx, cy, albedo, roughness, metallic)"""
    k = R.intrinsics(12, 16)
    verts = np.array([[-0.6, -0.5, 2.0], [0.5, -0.45, 2.3], [0.55, 0.5, 2.1], [-0.5, 0.55, 1.9],   # the pair
                      [-0.9, 0.2, 1.5], [0.1, 0.35, 1.2], [-0.3, 0.1, -0.5]])                      # crosses z = 0
    tris = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]], np.int32)
    rng = np.random.default_rng(8)
    w2c = R.look_at([0.1, -0.05, 0.0], [0.0, 0.02, 2.0])[None]
    return dict(verts=verts, tris=tris, w2c=w2c, H=12, W=16, albedo=rng.random((7, 3)).astype(np.float32),
                roughness=rng.random(7).astype(np.float32), metallic=rng.random(7).astype(np.float32), **k)


def icosahedron():
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
                  [-t, 0, -1], [-t, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int32)
    return v / np.linalg.norm(v[0]), f
