"""The triangle atlas (include/gs2m_atlas.h) and the texel bake (include/gs2m_meshbake.h, second half) restated in
float64 numpy, operation for operation, with the synthetic scenes the tests of them share.  The per-view part is
tests/mesh_bake_ref.py's.  Not collected.  The arrays of the cached scenes are shared: leave them unchanged."""
import functools

import numpy as np

import mesh_bake_ref as B
import mesh_view_ref as MV
import tnt_cull_ref as R

CLASSES = 6
MAX_WIDTH = 16384


# ---- layout --------------------------------------------------------------------------------------------------------------------

def tri_class(verts, tris, density):
    p = np.asarray(verts, np.float64)[np.asarray(tris, np.int64)]
    e = np.zeros(len(p))
    for c in range(3):
        d = p[:, (c + 1) % 3] - p[:, c]
        e = np.maximum(e, np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))
    want = e * density
    k = np.full(len(p), CLASSES - 1)
    for c in range(CLASSES - 2, -1, -1):
        k[float((8 << c) - 4) >= want] = c
    return k


def class_margin(verts, tris, density):
    """the smallest non-zero relative distance of e * density from a class threshold (exactly on it is allowed, as in
    mesh_bake_ref: such operands are exact on both sides)"""
    p = np.asarray(verts, np.float64)[np.asarray(tris, np.int64)]
    if not len(p):
        return np.inf
    e = np.max([np.linalg.norm(p[:, (c + 1) % 3] - p[:, c], axis=1) for c in range(3)], axis=0) * density
    d = np.abs(np.stack([e / float((8 << c) - 4) - 1.0 for c in range(CLASSES - 1)]))
    return d[d > 0].min()


def morton_decode(m):
    x = y = 0
    for b in range(32):
        x |= ((m >> (2 * b)) & 1) << b
        y |= ((m >> (2 * b + 1)) & 1) << b
    return x, y


def morton_encode(x, y):
    m = 0
    for b in range(16):
        m |= ((int(x) >> b) & 1) << (2 * b) | ((int(y) >> b) & 1) << (2 * b + 1)
    return m


def layout(hist):
    """-> dict(start, base (lists of 6), total, width, height); ValueError beyond MAX_WIDTH"""
    start, base, n, units = [0] * CLASSES, [0] * CLASSES, 0, 0
    for k in range(CLASSES - 1, -1, -1):
        start[k], base[k] = n, units
        n += int(hist[k])
        units += ((int(hist[k]) + 1) // 2) * 4 ** k
    width = height = 0
    if units:
        j = 0
        while 4 ** j < units:
            j += 1
        width = 8 << j
        if width > MAX_WIDTH:
            raise ValueError("unsupported size")
        height = width // 2 if j >= 1 and 2 * units <= 4 ** j else width
    return dict(hist=[int(h) for h in hist], start=start, base=base, total=units, width=width, height=height)


def cell_origin(L, k, cell):
    ux, uy = morton_decode(L["base"][k] + cell * 4 ** k)
    return 8 * ux, 8 * uy


def corners(side, half):
    Lc = side - 4
    if half == 0:
        return [(1, 1), (1 + Lc, 1), (1, 1 + Lc)]
    return [(side - 1, side - 1), (side - 1 - Lc, side - 1), (side - 1, side - 1 - Lc)]


def build(verts, tris, density):
    """-> dict(cls (F,), cells (F, 4), uvs (F, 3, 2) float32, order (F,), + layout's keys)"""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    cls = tri_class(verts, tris, density)
    L = layout(np.bincount(cls, minlength=CLASSES))
    order = np.argsort(CLASSES - 1 - cls, kind="stable")
    cells, uvs = np.zeros((len(tris), 4), np.int64), np.zeros((len(tris), 3, 2), np.float32)
    for q, t in enumerate(order):
        k = cls[t]
        rank = q - L["start"][k]
        ox, oy = cell_origin(L, k, rank // 2)
        side, half = 8 << k, rank % 2
        cells[t] = (ox, oy, side, half)
        for c, (x, y) in enumerate(corners(side, half)):
            uvs[t, c] = (np.float32(np.float64(ox + x) / np.float64(L["width"])), np.float32(np.float64(oy + y) / np.float64(L["height"])))
    return dict(cls=cls, cells=cells, uvs=uvs, order=order, **L)


def owners(L, order):
    """The texel side alone: -> owner (H, W) int64 (-1: empty), side, half, li, lj (H, W) -- through the Morton code of the
    texel's unit and the bases, as the device finds them"""
    H, W = L["height"], L["width"]
    owner = np.full((H, W), -1, np.int64)
    side, half, li, lj = (np.zeros((H, W), np.int64) for _ in range(4))
    for uy in range(H // 8):
        for ux in range(W // 8):
            m = morton_encode(ux, uy)
            if m >= L["total"]:
                continue
            k = CLASSES - 1
            for c in range(CLASSES - 2, -1, -1):
                if L["hist"][c] > 0 and m >= L["base"][c]:
                    k = c
            cell = (m - L["base"][k]) >> (2 * k)
            ox, oy = cell_origin(L, k, cell)
            s = 8 << k
            j, i = np.mgrid[8 * uy - oy:8 * uy - oy + 8, 8 * ux - ox:8 * ux - ox + 8]
            h = (i + j > s - 1).astype(np.int64)
            rank = 2 * cell + h
            ok = rank < L["hist"][k]
            blk = (slice(8 * uy, 8 * uy + 8), slice(8 * ux, 8 * ux + 8))
            owner[blk] = np.where(ok, np.asarray(order, np.int64)[np.minimum(L["start"][k] + rank, len(order) - 1)], -1)
            side[blk], half[blk], li[blk], lj[blk] = s, h, i, j
    return owner, side, half, li, lj


def bary(side, half, li, lj):
    """-> (l (.., 3), interior) of the Texel paragraph; arrays of one shape"""
    Lc = (side - 4).astype(np.float64)
    a = 2 * np.where(half == 1, side - 1 - li, li) - 1
    b = 2 * np.where(half == 1, side - 1 - lj, lj) - 1
    interior = (a >= 0) & (b >= 0) & (a + b <= 2 * (side - 4))
    with np.errstate(all="ignore"):
        l1, l2 = (a * 0.5) / Lc, (b * 0.5) / Lc
        l = np.stack([(1.0 - l1) - l2, l1, l2], axis=-1)
        l = np.where(l > 0.0, l, 0.0)
        l = l / ((l[..., 0] + l[..., 1]) + l[..., 2])[..., None]
    return l, interior


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def _mix(l, xa, xb, xc):
    return (l[..., 0:1] * xa + l[..., 1:2] * xb) + l[..., 2:3] * xc


def texels(verts, normals, tris, atlas):
    """-> dict(owner (H, W), interior (H, W) bool, points, normals (H, W, 3), l (H, W, 3))"""
    verts = np.asarray(verts, np.float64)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    owner, side, half, li, lj = owners(atlas, atlas["order"])
    own = owner >= 0
    t = tris[np.where(own, owner, 0)] if len(tris) else np.zeros(owner.shape + (3,), np.int64)
    l, interior = bary(np.where(own, side, 8), half, li, lj)
    with np.errstate(all="ignore"):
        a, b, c = (verts[t[..., k]] for k in range(3)) if len(tris) else (np.zeros(owner.shape + (3,)),) * 3
        p = _mix(l, a, b, c)
        face = _cross(b - a, c - a)
        N = face
        if normals is not None:
            vn = np.asarray(normals, np.float64)
            S = _mix(l, vn[t[..., 0]], vn[t[..., 1]], vn[t[..., 2]])
            good = np.isfinite(S).all(-1) & (S != 0).any(-1)
            N = np.where(good[..., None], S, face)
    z = np.zeros(3)
    return dict(owner=owner, interior=interior & own, points=np.where(own[..., None], p, z), normals=np.where(own[..., None], N, z),
                l=np.where(own[..., None], l, z))


# ---- bake ----------------------------------------------------------------------------------------------------------------------

def accumulate(tex, w2c, fx, fy, cx, cy, depth, maps, mask=None, eps=B.EPS, with_normals=True):
    """the texels as points through mesh_bake_ref.accumulate -> (sums (HW, C), weights (HW,), use (HW, n_views), margin)"""
    own = tex["owner"].reshape(-1) >= 0
    p, n = tex["points"].reshape(-1, 3), tex["normals"].reshape(-1, 3)
    s, w, use, margin = B.accumulate(p, n if with_normals else None, w2c, fx, fy, cx, cy, depth, maps, mask, eps)
    s[~own], w[~own], use[~own], margin[~own] = 0.0, 0.0, False, np.inf
    return s, w, use, margin


def resolve(tex, tris, sums, weights, min_weight, fallback, attributes=None):
    """-> (out (HW, C) float32, seen (HW,))"""
    own = tex["owner"].reshape(-1) >= 0
    weights = np.where(own, weights, 0.0)
    seen = (weights >= min_weight) & (weights > 0)
    fb = np.asarray(fallback, np.float32)
    with np.errstate(all="ignore"):
        out = np.where(seen[:, None], (sums / weights[:, None]).astype(np.float32), fb[None]).astype(np.float32)
    if attributes is not None:
        X = np.asarray(attributes, np.float32).astype(np.float64)
        t = np.asarray(tris, np.int64).reshape(-1, 3)[np.where(own, tex["owner"].reshape(-1), 0)]
        v = _mix(tex["l"].reshape(-1, 3), X[t[:, 0]], X[t[:, 1]], X[t[:, 2]]).astype(np.float32)
        out = np.where((own & ~seen)[:, None], v, out)
    return out, seen


def srgb_band(values):
    """|255 enc(x) + 0.5 - nearest integer| of the base-colour channels: where it is below 1e-6 a last-place difference of pow
    may move the byte"""
    x = np.clip(np.nan_to_num(np.asarray(values, np.float32)[..., :3].astype(np.float64), nan=0.0), 0.0, 1.0)
    y = 255.0 * MV.srgb_encode(x) + 0.5
    return np.abs(y - np.rint(y))


def pack(values, srgb=True):
    """values (.., 3 or 5) float32 -> (base (.., 3) uint8, orm (.., 3) uint8 or None)"""
    v = np.asarray(values, np.float32).astype(np.float64)
    x = np.where(v > 0.0, np.where(v < 1.0, v, 1.0), 0.0)
    base = np.floor(255.0 * (MV.srgb_encode(x[..., :3]) if srgb else x[..., :3]) + 0.5).astype(np.uint8)
    orm = None
    if v.shape[-1] == 5:
        orm = np.stack([np.full(v.shape[:-1], 255.0), np.floor(255.0 * x[..., 3] + 0.5), np.floor(255.0 * x[..., 4] + 0.5)], axis=-1).astype(np.uint8)
    return base, orm


def sample_bilinear(tex, uv):
    """tex (H, W, C); uv (n, 2) with v from the top row; texel (i, j) has its centre at (i + 0.5, j + 0.5) -> (values (n, C), taps:
    (n, 4, 2) the (row, column) of the four taps, weights (n, 4))"""
    H, W = tex.shape[:2]
    x, y = uv[:, 0] * W - 0.5, uv[:, 1] * H - 0.5
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    tx, ty = x - x0, y - y0
    taps = np.stack([np.stack([y0, x0], 1), np.stack([y0, x0 + 1], 1), np.stack([y0 + 1, x0], 1), np.stack([y0 + 1, x0 + 1], 1)], 1)
    w = np.stack([(1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty], 1)
    tc = np.stack([np.clip(taps[..., 0], 0, H - 1), np.clip(taps[..., 1], 0, W - 1)], -1)
    vals = (np.asarray(tex, np.float64)[tc[..., 0], tc[..., 1]] * w[..., None]).sum(1)
    return vals, taps, w


# ---- scenes --------------------------------------------------------------------------------------------------------------------

def icosphere(level=2):
    v, f = B.icosahedron()
    for _ in range(level):
        mid, nv, nf = {}, list(v), []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = nv[a] + nv[b]
                mid[key] = len(nv)
                nv.append(p / np.linalg.norm(p))
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        v, f = np.array(nv), np.array(nf, np.int32)
    return np.asarray(v, np.float64), np.asarray(f, np.int32)


FRAME = dict(H=48, W=64, fx=70.0, fy=70.0, cx=31.5, cy=23.5)
AFFINE = np.array([[0.11, 0.05, -0.07, 0.45], [-0.06, 0.12, 0.04, 0.5], [0.05, -0.03, 0.1, 0.4], [0.08, 0.02, 0.06, 0.35],
                   [-0.04, 0.09, -0.05, 0.55]])  # channel c at world point p: AFFINE[c, :3] . p + AFFINE[c, 3]


def affine_field(p):
    return p @ AFFINE[:, :3].T + AFFINE[:, 3]


def affine_maps(w2c, H, W, fx, fy, cx, cy, plane_n, plane_d):
    """The affine field on the plane {p: plane_n . p = plane_d} as every view sees it, per pixel centre at integer coordinates
    (the bake's convention) -> (n, 5, H, W) float32.  A perspective view of an affine field on a plane is not affine in the
    image, so a bilinear tap is exact only to the pixel's size: use it where the tolerance says so."""
    out = np.zeros((len(w2c), 5, H, W), np.float32)
    j, i = np.mgrid[0:H, 0:W]
    for v, M in enumerate(w2c):
        Rm, t = M[:3, :3], M[:3, 3]
        ray = np.stack([(i - cx) / fx, (j - cy) / fy, np.ones_like(i, np.float64)], -1) @ Rm  # world directions
        o = -Rm.T @ t
        s = (plane_d - o @ plane_n) / (ray @ plane_n)
        p = o + s[..., None] * ray
        out[v] = np.moveaxis(affine_field(p), -1, 0)
    return out


@functools.lru_cache(maxsize=None)
def sphere_case():
    """The GPU scene: a level-2 icosphere of radius 0.9 around (0, 0, 3.2) (320 triangles: 120 of side 16 and 200 of side 32 at this density), five
    views on a ring, random 64 x 48 maps and a mask with holes; the restatement's own z-buffer.
    -> dict(verts, tris, normals, w2c, depth, maps, mask, density, atlas, tex, **FRAME)"""
    v, f = icosphere(2)
    verts = 0.9 * v + np.array([0.0, 0.0, 3.2])
    k = FRAME
    eyes = [[0.0, 0.0, 0.0], [2.2, 0.3, 1.2], [-2.0, -0.4, 1.5], [0.4, 2.3, 2.0], [0.3, -0.2, 6.4]]
    w2c = np.stack([R.look_at(e, [0.0, 0.0, 3.2]) for e in eyes])
    depth, _ = R.render_depth(verts, f, w2c, k["fx"], k["fy"], k["cx"], k["cy"], k["H"], k["W"])
    rng = np.random.default_rng(11)
    maps = rng.random((len(w2c), 5, k["H"], k["W"])).astype(np.float32)
    mask = (rng.random((len(w2c), k["H"], k["W"])) > 0.05).astype(np.float32)
    normals = MV.vertex_normal_sums(verts, f)[2]
    density = 42.0
    atlas = build(verts, f, density)
    tex = texels(verts, normals, f, atlas)
    return dict(verts=verts, tris=f, normals=normals, w2c=w2c, depth=depth, maps=maps, mask=mask, density=density, atlas=atlas, tex=tex,
                eps=B.EPS, **k)


@functools.lru_cache(maxsize=None)
def sphere_reference(channels=5, masked=True, with_normals=True):
    c = sphere_case()
    return accumulate(c["tex"], c["w2c"], c["fx"], c["fy"], c["cx"], c["cy"], c["depth"], c["maps"][:, :channels],
                      c["mask"] if masked else None, c["eps"], with_normals)


@functools.lru_cache(maxsize=None)
def plane_case():
    """A tilted plane of 6 x 6 quads (72 triangles) facing the origin, inside FRAME from there -> dict(verts, tris, density,
    atlas, tex)"""
    X, Y = np.meshgrid(np.linspace(-1.0, 1.0, 7), np.linspace(-0.7, 0.7, 7))
    verts = np.stack([X.ravel(), Y.ravel(), 3.0 + 0.3 * X.ravel() - 0.2 * Y.ravel()], 1)
    idx = np.arange(49).reshape(7, 7)
    q = np.stack([idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()], 1)
    tris = np.concatenate([q[:, [0, 2, 1]], q[:, [0, 3, 2]]]).astype(np.int32)
    density = 40.0
    atlas = build(verts, tris, density)
    tex = texels(verts, None, tris, atlas)
    return dict(verts=verts, tris=tris, density=density, atlas=atlas, tex=tex)


SMALL_SHAPES = ("one", "two", "three", "four", "six_classes", "clamped", "zero_area", "second_half")


@functools.lru_cache(maxsize=None)
def small_shape(name):
    """-> (verts (V, 3), tris (F, 3) int32, density)"""
    def fan(n, edge):  # n separate right triangles with legs `edge`
        v = np.concatenate([[[3.0 * t, 0.0, 1.0], [3.0 * t + edge, 0.0, 1.0], [3.0 * t, edge, 1.0]] for t in range(n)])
        return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    if name in ("one", "two", "three", "four"):
        n = SMALL_SHAPES.index(name) + 1
        return fan(n, 0.5) + (4.0,)       # longest edge 0.707 * 4 = 2.83 texels: side 8
    if name == "six_classes":
        v = np.concatenate([[[10.0 * k, 0.0, 0.0], [10.0 * k + 0.7 * (8 << k) - 2.0, 0.0, 0.0], [10.0 * k, 1.0, 0.5]] for k in range(6)])
        return v / 1.0, np.arange(18, dtype=np.int32).reshape(6, 3)[[2, 5, 0, 3, 1, 4]], 1.0
    if name == "clamped":
        v, f = fan(2, 0.5)
        v[1, 0] = 400.0                   # an edge of 400 texels at density 1
        return v, f, 1.0
    if name == "zero_area":
        v = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [2.0, 0.0, 1.0], [5.0, 5.0, 5.0]])
        return v, np.array([[0, 1, 2], [3, 3, 3], [0, 1, 3]], np.int32), 2.0
    if name == "second_half":
        return fan(70, 0.5) + (4.0,)      # 35 cells: 4^3 = 64 units, 35 > 32 -> the full square; fan(64, ..) would give half
    raise KeyError(name)
