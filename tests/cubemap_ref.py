"""TEST INFRASTRUCTURE ONLY.  Float64 reference of the specular cube-map prefilter (csrc/cubemap.hip), one column or one
row of the weight matrix at a time, on top of oracle/cubemap_oracle.py (texel directions, areas, the GGX weight):

    forward  raw[o, :3] = sum_t W[o, t] x[t],  raw[o, 3] = sum_t W[o, t];      backward  grad[t] = sum_o W[o, t] G[o]

so a column W[:, t] is what a one-texel input probe produces and a row W[o, :] what a one-texel gradient probe produces.
Every pair (o, t) also gets a class against the cone test `d >= cos_cut` and every accepted pair a bound on its weight.

The band.  u = 2^-24 is the unit roundoff of fp32.  The kernel forms, for both texels of a pair,

    fx = org + step * x,  org = 1/N - 1,  step = 2/N        error <= u/N + u (org) + 4u (step * x: the rounding of step,
                                                            2u/N, times x < N, and of the product, < 2) + u (the sum) <= 7u
    d  = ((p1 + p2) + p3) * (ro * rt),  p_i products of face-point components,  ro, rt = rsq((fx fx + fy fy) + 1)

(a) The face coordinates: a point (fx, fy, 1) moved by at most sqrt(2) 7u turns its unit direction by at most 9.9u
    (|P| >= 1), and a turn dn of one direction, being orthogonal to it, changes d = n_o . n_t by at most |dn| sin(theta):
    together 19.8u sin(theta) + (9.9u)^2.
(b) Three products (u |p_i| each), two adds (u |p1 + p2|, u |D|): by Cauchy-Schwarz each of the three sums of magnitudes
    is at most |P_o| |P_t|, so after the scaling by ro rt ~ 1 / (|P_o| |P_t|) they cost 3u.
(c) rsq's argument carries 3u relative (two squares, two adds), which the root halves, and the instruction is good to
    1 ulp = 2u: 3.5u for each of ro and rt; the two multiplies u each: 9u |d| <= 9u.

    E_d(d) = (12 + 20 sqrt(1 - d^2)) u,   taken 1 % up for the second-order terms, + 1e-13

At most 32.3u = 1.93e-6: inside the 2e-6 of test_cubemap_gpu.py for every cone, and 12u = 7.2e-7 for the sub-texel lobes,
whose pairs sit at sin(theta) ~ 1e-2.  A pair is IN when d - E_d(d) >= cos_cut, OUT when d + E_d(d) < cos_cut, RIM
otherwise; cos_cut and the roughness are the fp32 values the C call receives (`f32`).

The weight of an IN pair.  w = max(d, 0) a2 / (pi den^2) area / 4 with den = 1 + (1 + d)(a2 - 1) / 2, a2 = roughness^4.
  den   takes E_d (1 - a2) / 2 from d and u (1 + 3 a2 + den) of its own (the rounding of 1 + d, of (a2 - 1) / 2 -- a2 itself
        is three roundings from the roughness -- and of the fma): e_den; w moves by (1 - e_den / den)^-2 - 1, to first order
        (E_d + 2u (1 + 3 a2)) / den.  This is the term that lets a sub-texel lobe resolve its self weight to a percent only.
  d     as a factor: E_d times the rest of the weight (absolute, d may be small in a wide cone).
  c     = 12: a2 / pi 4.5u (r r, alpha alpha, the constant, the division), den den u, rcp 1 ulp = 2u, two multiplies 2u
        for k, the product of the two axis factors u, k area u.  The backward multiplies by the area at the end: same count.
  area  the fp32 table holds atanf((k + 1) / h) - atanf(k / h): each atanf is taken as good to ATANF_ULP ulp of its value
        plus u / 2 for its rounded argument, the difference rounds once; relative to the small difference that is ~3u N,
        per axis (`axis_error`).  tests/test_cubemap_kernels_gpu.py holds the table itself to the same figure.

    |dw| <= 1.01 (w ((1 - e_den / den)^-2 - 1 + 12u + area_rel) + (w / d) E_d)

A probe puts one non-zero term into each sum, so nothing else enters; the dense tests add n u sum |w x| for a sum of n terms
in any order.
"""
import functools

import numpy as np

from oracle import cubemap_oracle as O

U = 2.0 ** -24
OUT, RIM, IN = 0, 1, 2
C_W = 12.0
ATANF_ULP = 2.0


def f32(v):
    """the value a C `float` parameter receives"""
    return float(np.float32(v))


@functools.lru_cache(maxsize=None)
def _geo(N):
    return O.texel_dirs(N), O.texel_areas(N)


def texel_areas(N):
    return _geo(N)[1]


def diffuse_matrix(N):
    return O.diffuse_matrix(N)


def err_d(d):
    return (12.0 + 20.0 * np.sqrt(np.maximum(1.0 - d * d, 0.0))) * U * 1.01 + 1e-13


def _ulp32(v):
    v = np.abs(np.asarray(v, dtype=np.float64))
    return np.where(v > 0, 2.0 ** (np.floor(np.log2(np.maximum(v, 1e-300))) - 23), 0.0)


@functools.lru_cache(maxsize=None)
def axis_table(N):
    """(ax, err): the float64 axis factors area(x, y) = ax[x] ax[y] and the bound on the fp32 table's error"""
    if N <= 1:
        return np.ones(N), np.zeros(N)
    H = N // 2
    k = np.abs(np.arange(N) - H).astype(np.float64)
    hi, lo = np.arctan((k + 1) / H), np.arctan(k / H)
    ax = hi - lo
    err = (ATANF_ULP * _ulp32(hi) + 0.5 * U) + np.where(k > 0, ATANF_ULP * _ulp32(lo) + 0.5 * U, 0.0) + U * ax
    return ax, err


@functools.lru_cache(maxsize=None)
def area_rel(N):
    """per texel of one face, tiled over the six: relative bound on the fp32 area ax[x] * ax[y]"""
    ax, err = axis_table(N)
    r = err / ax
    return np.tile((r[:, None] + r[None, :] + U).reshape(-1), 6)


class Pairs:
    """One row or column of W restricted to the pairs that are not surely outside the cone: `idx` the other texel of each
    pair, `d`, `cls` (RIM / IN), `w` the float64 weight (whatever the class), `bound` on |dw|; `self_idx` the fixed texel."""

    def __init__(self, T, self_idx, idx, d, cls, w, bound):
        self.T, self.self_idx, self.idx, self.d, self.cls, self.w, self.bound = T, self_idx, idx, d, cls, w, bound

    def dense(self, what="w"):
        """the 6 N^2 vector: weights of the pairs the float64 cone test accepts (`w`, as the oracle's matrix has them)"""
        out = np.zeros(self.T)
        out[self.idx] = getattr(self, what)
        return out

    @property
    def n_in(self):
        return int((self.cls == IN).sum())

    @property
    def n_rim(self):
        return int((self.cls == RIM).sum())


def pairs_flat(N, roughness, cos_cut, fixed, column, both=False):
    """The pairs of several rows (or columns) at once, as flat arrays: (k, idx, d, cls, w, bound), `k` the position in
    `fixed` of the pair's fixed texel, sorted by k.  `both`: (k, idx, d, cls, w_row, bound_row, w_col, bound_col) -- the
    pair geometry is symmetric, only the area belongs to the input texel."""
    dirs, areas = _geo(N)
    fixed = np.asarray(fixed, dtype=np.int64).reshape(-1)
    dots = dirs[fixed] @ dirs.T
    k, idx = np.nonzero(dots + err_d(dots) >= cos_cut)      # everything else is OUT
    d = dots[k, idx]
    a = fixed[k]
    Hv = dirs[idx] + dirs[a]
    Hv /= np.maximum(np.linalg.norm(Hv, axis=-1, keepdims=True), 1e-300)
    # V_o . H (den = 1 - vh^2 (1 - a2) amplifies the last bit of vh by 1 / den); o is the varying texel of a column
    vh = np.clip(np.einsum("pc,pc->p", dirs[idx] if column else dirs[a], Hv), 0.0, 1.0)
    a2 = roughness ** 4
    den = (vh * a2 - vh) * vh + 1.0
    coef = a2 / (den * den * np.pi)
    Ed = err_d(d)
    cls = np.where(d - Ed >= cos_cut, IN, RIM)
    x = (Ed * (1.0 - a2) / 2.0 + U * (1.0 + 3.0 * a2 + den)) / den
    rel = np.where(x < 0.9, (1.0 - np.minimum(x, 0.9)) ** -2 - 1.0, np.inf) + C_W * U

    def weigh(t):                                           # t: the input texel, which carries the area
        area = areas[t]
        w = np.maximum(d, 0.0) * coef * area / 4.0
        return w, 1.01 * (w * (rel + area_rel(N)[t]) + coef * area / 4.0 * Ed)
    if both:
        return (k, idx, d, cls) + weigh(idx) + weigh(a)
    return (k, idx, d, cls) + weigh(a if column else idx)


def _pairs(N, roughness, cos_cut, a, column):
    _, idx, d, cls, w, bound = pairs_flat(N, roughness, cos_cut, [a], column)
    return Pairs(6 * N * N, a, idx, d, cls, w, bound)


def column_pairs(N, roughness, cos_cut, t):
    return _pairs(N, roughness, cos_cut, t, True)


def row_pairs(N, roughness, cos_cut, o):
    return _pairs(N, roughness, cos_cut, o, False)


def _accepted(p, cos_cut):
    out = np.zeros(p.T)
    keep = p.d >= cos_cut
    out[p.idx[keep]] = p.w[keep]
    return out


def specular_column(N, roughness, cos_cut, t):
    """W[:, t] in float64 (the oracle's matrix column: zero where d < cos_cut)"""
    return _accepted(column_pairs(N, roughness, cos_cut, t), cos_cut)


def specular_row(N, roughness, cos_cut, o):
    """W[o, :] in float64"""
    return _accepted(row_pairs(N, roughness, cos_cut, o), cos_cut)


# ------------------------------------------------------------------------------------------------ the culling boxes
def _to_face_frame(s, v):
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return [(-z, -y, x), (z, -y, -x), (x, z, y), (x, -z, -y), (x, -y, z), (-x, -y, -z)][s]


def _cone_range(u, cz, sin_t, N):
    """numpy restatement of cone_range: (lo, hi) per element, empty as lo > hi"""
    rho = np.sqrt(u * u + cz * cz)
    full = sin_t >= rho * 0.999
    rs = np.where(full, 1.0, rho)
    psi, delta = np.arctan2(u, cz), np.arcsin(np.minimum(sin_t / rs, 1.0)) + 1e-4
    lim = 1.5607963
    a0, a1 = psi - delta, psi + delta
    empty = (a1 < -lim) | (a0 > lim)
    a0, a1 = np.tan(np.maximum(a0, -lim)), np.tan(np.minimum(a1, lim))
    empty |= (a0 > 1.0) | (a1 < -1.0)
    lo = np.maximum(np.floor((np.maximum(a0, -1.0) + 1.0) * (0.5 * N)).astype(np.int64) - 1, 0)
    hi = np.minimum(np.floor((np.minimum(a1, 1.0) + 1.0) * (0.5 * N)).astype(np.int64) + 1, N - 1)
    lo, hi = np.where(full, 0, lo), np.where(full, N - 1, hi)
    return np.where(empty & ~full, 1, lo), np.where(empty & ~full, 0, hi)


def union_box(N, cos_cut, tile, face):
    """(X0, X1, Y0, Y1) of the union of the 64 cone boxes of workgroup `tile` of specular_tile_kernel (the source face is
    tile // (N / 8)^2) on face `face`, or None when no output of the tile reaches the face.  Only used to prove that a test
    shape contains the boxes it is meant to contain."""
    tiles = N // 8
    os_, tt = divmod(tile, tiles * tiles)
    lane = np.arange(64)
    ox, oy = (tt % tiles) * 8 + (lane & 7), (tt // tiles) * 8 + (lane >> 3)
    V = _geo(N)[0][(os_ * N + oy) * N + ox]
    if cos_cut <= 0.70710678:
        return 0, N - 1, 0, N - 1
    sin_t = np.sqrt(max(1.0 - cos_cut * cos_cut, 0.0))
    cx, cy, cz = _to_face_frame(face, V)
    x0, x1 = _cone_range(cx, cz, sin_t, N)
    y0, y1 = _cone_range(cy, cz, sin_t, N)
    ok = (cz > -sin_t) & ~(np.maximum(np.abs(cx), np.abs(cy)) - cz > 1.41421356 * sin_t + 2e-3) & (x0 <= x1) & (y0 <= y1)
    if not ok.any():
        return None
    return int(x0[ok].min()), int(x1[ok].max()), int(y0[ok].min()), int(y1[ok].max())


# ------------------------------------------------------------------------------------------------ shapes and probes
# (N, roughness, NDF cutoff, route, aligned): gs2m_specular_cubemap_route's numbering; aligned 0: `out` 4 bytes off
TPO1, TPO16, TPO64, TILE8, TILE4 = range(5)
SHAPES = [
    (1, 0.5, 0.99, TPO1, 1), (2, 0.5, 0.99, TPO1, 1), (3, 0.3, 0.99, TPO1, 1), (5, 0.3, 0.99, TPO1, 1),
    (24, 0.08, 0.99, TPO1, 1),
    (16, 1.0, 0.99, TPO64, 1), (16, 1.0, 0.5, TPO64, 1), (32, 0.5, 0.99, TPO64, 1),
    (40, 0.3, 0.99, TPO16, 1), (63, 0.2, 0.99, TPO16, 1), (65, 0.3, 0.99, TPO16, 1),
    (40, 0.7, 0.99, TPO64, 1),
    (64, 0.385, 0.99, TILE8, 1), (72, 0.3, 0.99, TILE8, 1), (104, 0.25, 0.99, TILE8, 1),
    (112, 0.25, 0.99, TILE4, 1), (128, 0.27, 0.99, TILE4, 1), (256, 0.155, 0.99, TILE4, 1),
    (256, 0.24, 0.99, TILE4, 1),
    (512, 0.04, 0.99, TPO1, 1),
    (64, 0.385, 0.99, TPO64, 0), (128, 0.27, 0.99, TPO16, 0),
]
SUB_TEXEL = {(512, 0.04), (24, 0.08)}      # rim share capped at 25 %, every other shape at 5 %
WIDE_SEGMENT = (256, 0.24)                 # has a union box wider than one 64-texel LDS segment
FEW_ROWS = (64, 0.385)                     # split 8, has a union box with fewer than 8 rows


def shape_id(s):
    return f"{s[0]}-{s[1]}-{s[2]}" + ("" if s[4] else "-unaligned")


def cos_cut_of(roughness, cutoff):
    """the fp32 cosine the C call receives (render_utils.ndf_cutoff: no GPU needed)"""
    import render_utils as RU
    return f32(RU.ndf_cutoff(roughness, cutoff))


def probe_texels(N, seed=0):
    """Probe texels of a level, in groups of three (one per colour channel): the four corners, the four edge midpoints
    and the centre of face 4, the texel across the face edge from each of the eight on faces 0, 1, 2 and 3 (a +y and a -y
    face among them: to_face_frame permutes differently there), and 12 seeded random ones."""
    M, m, c = N - 1, N // 2, N // 2
    def tx(s, y, x):
        return (s * N + y) * N + x
    on4 = [(0, 0), (0, M), (M, 0), (M, M), (0, m), (M, m), (m, 0), (m, M), (c, c)]
    t = [tx(4, y, x) for y, x in on4]
    # face 4 = (fx, -fy, 1): its x = +1 edge meets face 0 = (1, -fy, -fx) at fx0 = -1 (column 0, same row); x = -1 meets
    # face 1 at its column M; y = 0 (world +y) meets face 2 = (fx, 1, fy) at its row M; y = M meets face 3 at its row 0
    t += [tx(0, 0, 0), tx(0, M, 0), tx(0, m, 0), tx(1, 0, M), tx(1, M, M), tx(1, m, M),
          tx(2, M, 0), tx(2, M, M), tx(2, M, m), tx(3, 0, 0), tx(3, 0, M), tx(3, 0, m), tx(5, c, c), tx(2, c, c), tx(1, c, c)]
    rng = np.random.RandomState(1000 * N + seed)
    t += [int(v) for v in rng.randint(0, 6 * N * N, 12)]
    t = [int(v) for v in t]
    assert len(t) % 3 == 0
    return [t[k:k + 3] for k in range(0, len(t), 3)]
