"""numpy fp64 restatement of the undistortion contract (gs-2m_amd/csrc/undistort_model.h, include/gs2m_undistort.h, DESIGN.md
section 24): the distortion models, the Newton inverse, the undistorted camera, the image warp and the observation transform.

Every function mirrors the header LINE BY LINE: the same order of operations, only + - * / and comparisons on IEEE doubles
(np.float64 scalars in the iteration, elementwise arrays in the warp; numpy fuses nothing), so the results are the bits the host
and the device compute.  The contract is this project's own, modelled on COLMAP's image_undistorter; nothing of COLMAP's pins it.
"""
import numpy as np

MAX_ITER = 100
EPS = np.float64(1e-12)
MODEL_IDS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4, "OPENCV_FISHEYE": 5, "FULL_OPENCV": 6, "FOV": 7,
             "SIMPLE_RADIAL_FISHEYE": 8, "RADIAL_FISHEYE": 9, "THIN_PRISM_FISHEYE": 10}
N_PARAMS = {0: 3, 1: 4, 2: 4, 3: 5, 4: 8, 6: 12}  # the supported models
F = np.float64


class Model:
    """undistort_unpack: COLMAP's parameters -> {fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6}, rational, identity"""

    def __init__(self, model, params):
        if model not in N_PARAMS:
            raise ValueError(f"refused model {model}")
        p = [F(v) for v in params]
        assert len(p) == N_PARAMS[model]
        single = model in (0, 2, 3)
        self.fx = p[0]
        self.fy = p[0] if single else p[1]
        self.cx = p[1] if single else p[2]
        self.cy = p[2] if single else p[3]
        self.k1 = self.k2 = self.p1 = self.p2 = self.k3 = self.k4 = self.k5 = self.k6 = F(0.0)
        self.rational = model == 6
        if model == 2:
            self.k1 = p[3]
        if model == 3:
            self.k1, self.k2 = p[3], p[4]
        if model in (4, 6):
            self.k1, self.k2, self.p1, self.p2 = p[4], p[5], p[6], p[7]
        if model == 6:
            self.k3, self.k4, self.k5, self.k6 = p[8], p[9], p[10], p[11]
        self.identity = all(k == 0.0 for k in (self.k1, self.k2, self.p1, self.p2, self.k3, self.k4, self.k5, self.k6))


def finite(x):
    with np.errstate(all="ignore"):
        return (x - x) == 0.0


def distort_jac(m, u, v):
    """undistort_distort_jac; u, v: np.float64 scalars or arrays.  -> (pu, pv, j00, j01, j11)"""
    if m.identity:
        return u, v, F(1.0) + 0 * u, 0 * u, F(1.0) + 0 * u
    with np.errstate(all="ignore"):
        u2 = u * u
        v2 = v * v
        uv = u * v
        r2 = u2 + v2
        r4 = r2 * r2
        if m.rational:
            r6 = r4 * r2
            num = ((1.0 + m.k1 * r2) + m.k2 * r4) + m.k3 * r6
            den = ((1.0 + m.k4 * r2) + m.k5 * r4) + m.k6 * r6
            rad = num / den - 1.0
            dn = (m.k1 + (2.0 * m.k2) * r2) + (3.0 * m.k3) * r4
            dd = (m.k4 + (2.0 * m.k5) * r2) + (3.0 * m.k6) * r4
            g = (dn * den - num * dd) / (den * den)
        else:
            rad = m.k1 * r2 + m.k2 * r4
            g = m.k1 + (2.0 * m.k2) * r2
        du = (u * rad + (2.0 * m.p1) * uv) + m.p2 * (r2 + 2.0 * u2)
        dv = (v * rad + (2.0 * m.p2) * uv) + m.p1 * (r2 + 2.0 * v2)
        pu = u + du
        pv = v + dv
        j00 = (((1.0 + rad) + (2.0 * u2) * g) + (2.0 * m.p1) * v) + (6.0 * m.p2) * u
        j01 = ((2.0 * uv) * g + (2.0 * m.p1) * u) + (2.0 * m.p2) * v
        j11 = (((1.0 + rad) + (2.0 * v2) * g) + (2.0 * m.p2) * u) + (6.0 * m.p1) * v
    return pu, pv, j00, j01, j11


def distort(m, u, v):
    return distort_jac(m, u, v)[:2]


def undistort(m, tu, tv):
    """undistort_undistort on np.float64 scalars.  -> (u, v, converged)"""
    tu, tv = F(tu), F(tv)
    u, v = tu, tv
    if m.identity:
        return u, v, True
    with np.errstate(all="ignore"):
        for _ in range(MAX_ITER):
            pu, pv, j00, j01, j11 = distort_jac(m, u, v)
            fu = pu - tu
            fv = pv - tv
            det = j00 * j11 - j01 * j01
            if not finite(det) or det == 0.0:
                return u, v, False
            su = (j11 * fu - j01 * fv) / det
            sv = (j00 * fv - j01 * fu) / det
            nu = u - su
            nv = v - sv
            if not finite(nu) or not finite(nv):
                return u, v, False
            u, v = nu, nv
            au = -su if su < 0.0 else su
            av = -sv if sv < 0.0 else sv
            if (au if au > av else av) <= EPS:
                return u, v, True
    return u, v, False


def point(m, q, x, y):
    """undistort_point: a distorted observation (pixels) -> the PINHOLE camera q = (fx, fy, cx, cy).  -> (ox, oy, converged)"""
    with np.errstate(all="ignore"):
        u, v, ok = undistort(m, (F(x) - m.cx) / m.fx, (F(y) - m.cy) / m.fy)
        return F(q[0]) * u + F(q[2]), F(q[1]) * v + F(q[3]), ok


def points(model, params, pinhole4, xy):
    """gs2m_undistort_points: xy (n, 2) -> (xy_out (n, 2) float64, failed count)"""
    m = Model(model, params)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    out = np.empty_like(xy)
    failed = 0
    for i in range(len(xy)):
        out[i, 0], out[i, 1], ok = point(m, pinhole4, xy[i, 0], xy[i, 1])
        failed += not ok
    return out, failed


def _scale(c, size, lo_min, lo_max, hi_min, hi_max, blank, min_scale, max_scale):
    with np.errstate(all="ignore"):
        a0, a1 = c / (c - lo_min), ((size - 0.5) - c) / (hi_max - c)
        b0, b1 = c / (c - lo_max), ((size - 0.5) - c) / (hi_min - c)
        min_s = a0 if a0 < a1 else a1
        max_s = b0 if b0 > b1 else b1
        s = 1.0 / (min_s * blank + max_s * (1.0 - blank))
    return min_scale if not (s >= min_scale) else (max_scale if s > max_scale else s)


def camera(model, w, h, params, blank=0.0, min_scale=0.2, max_scale=2.0, stats=None):
    """undistort_camera_rule.  -> (out_w, out_h, np.float64[4]) or None where the entry point returns GS2M_ERR_INVALID_ARG.
    `stats`: a dict that receives the number of border samples and of failed ones."""
    blank, min_scale, max_scale = F(blank), F(min_scale), F(max_scale)
    if model not in N_PARAMS or w < 1 or h < 1 or len(params) != N_PARAMS[model]:
        return None
    m = Model(model, params)
    if not all(finite(F(p)) for p in params) or not m.fx > 0.0 or not m.fy > 0.0:
        return None
    if not (0.0 <= blank <= 1.0) or not min_scale > 0.0 or not max_scale >= min_scale or not finite(max_scale):
        return None
    if not max_scale * F(max(w, h)) <= 2147483647.0:
        return None
    if m.identity:
        return w, h, np.array([m.fx, m.fy, m.cx, m.cy])
    q = (m.fx, m.fy, m.cx, m.cy)
    sides = {"left": [], "right": [], "top": [], "bottom": []}
    n = bad = 0
    for y in range(h):
        for side, x in (("left", 0.5), ("right", F(w) - 0.5)):
            px, _, ok = point(m, q, x, F(y) + 0.5)
            n, bad = n + 1, bad + (not ok)
            if ok:
                sides[side].append(px)
    for x in range(w):
        for side, y in (("top", 0.5), ("bottom", F(h) - 0.5)):
            _, py, ok = point(m, q, F(x) + 0.5, y)
            n, bad = n + 1, bad + (not ok)
            if ok:
                sides[side].append(py)
    if stats is not None:
        stats.update(samples=n, failed=bad)
    if not all(sides.values()):
        return None
    sx = _scale(m.cx, F(w), min(sides["left"]), max(sides["left"]), min(sides["right"]), max(sides["right"]), blank, min_scale, max_scale)
    sy = _scale(m.cy, F(h), min(sides["top"]), max(sides["top"]), min(sides["bottom"]), max(sides["bottom"]), blank, min_scale, max_scale)
    ow, oh = max(1, int(sx * F(w))), max(1, int(sy * F(h)))
    return ow, oh, np.array([m.fx, m.fy, (m.cx * F(ow)) / F(w), (m.cy * F(oh)) / F(h)])


def source_positions(model, params, pinhole4, ow, oh):
    """undistort_source_position for every output pixel.  -> (sx, sy) float64 (oh, ow)"""
    m = Model(model, params)
    q = [F(v) for v in pinhole4]
    x = np.arange(ow, dtype=np.float64)[None, :] + np.zeros((oh, 1))
    y = np.arange(oh, dtype=np.float64)[:, None] + np.zeros((1, ow))
    if m.identity and (q[0], q[1], q[2], q[3]) == (m.fx, m.fy, m.cx, m.cy):
        return x, y
    with np.errstate(all="ignore"):
        u = ((x + 0.5) - q[2]) / q[0]
        v = ((y + 0.5) - q[3]) / q[1]
        pu, pv = distort(m, u, v)
        return (m.fx * pu + m.cx) - 0.5, (m.fy * pv + m.cy) - 0.5


def images(model, params, src, pinhole4, ow, oh):
    """gs2m_undistort_images_u8: src (n, h, w, ch) uint8 -> (dst (n, oh, ow, ch) uint8, valid (oh, ow) uint8)"""
    src = np.asarray(src)
    n, h, w, ch = src.shape
    sx, sy = source_positions(model, params, pinhole4, ow, oh)
    with np.errstate(all="ignore"):
        inside = (sx >= 0.0) & (sx <= F(w - 1)) & (sy >= 0.0) & (sy <= F(h - 1))
    sx, sy = np.where(inside, sx, 0.0), np.where(inside, sy, 0.0)
    x0, y0 = sx.astype(np.int64), sy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    tx, ty = (sx - x0.astype(np.float64))[None, :, :, None], (sy - y0.astype(np.float64))[None, :, :, None]
    wx0, wy0 = 1.0 - tx, 1.0 - ty
    s = src.astype(np.float64)
    p00, p01, p10, p11 = s[:, y0, x0], s[:, y0, x1], s[:, y1, x0], s[:, y1, x1]
    v = wy0 * (wx0 * p00 + tx * p01) + ty * (wx0 * p10 + tx * p11)
    b = np.minimum((v + 0.5).astype(np.int64), 255)
    dst = np.where(inside[None, :, :, None], b, 0).astype(np.uint8)
    return dst, np.where(inside, 255, 0).astype(np.uint8)


# ---- the affine-field test's source image and bound ---------------------------------------------------------------------------
def affine_field_source(model, params, w, h, coeffs):
    """An intensity field I(u, v) = a + b u + c v on the UNDISTORTED normalised plane, seen by the distorted camera: source pixel
    (x, y) holds I(undistort of its centre).  -> (unrounded float64 (h, w), uint8 (1, h, w, 1)); every sample must converge."""
    m = Model(model, params)
    a, b, c = coeffs
    f = np.empty((h, w))
    for y in range(h):
        for x in range(w):
            u, v, ok = undistort(m, (F(x) + 0.5 - m.cx) / m.fx, (F(y) + 0.5 - m.cy) / m.fy)
            assert ok
            f[y, x] = a + b * u + c * v
    assert f.min() >= 0.0 and f.max() <= 255.0
    return f, np.floor(f + 0.5).astype(np.uint8)[None, :, :, None]


def bilinear_bound(field):
    """|warped byte - I(output pixel)| for the affine-field test.  The warped value is the bilinear interpolant of the ROUNDED source
    samples, rounded again: 0.5 for each rounding (the interpolant is a convex combination, so it inherits the samples' 0.5), plus
    the interpolation error of f = I o undistort on a unit cell, at most (max |f_xx| + max |f_yy|) / 8.  The second derivatives are
    taken from the second differences of the unrounded source field at unit spacing -- each is f'' at some point of its three-sample
    span -- with a factor 2 for their variation inside a cell (the coefficient sets of the tests are mild: the third derivative over
    one pixel is a small fraction of the second), plus 1e-9 for the fp64 arithmetic."""
    dxx = np.abs(field[:, 2:] - 2.0 * field[:, 1:-1] + field[:, :-2]).max() if field.shape[1] > 2 else 0.0
    dyy = np.abs(field[2:, :] - 2.0 * field[1:-1, :] + field[:-2, :]).max() if field.shape[0] > 2 else 0.0
    return 1.0 + 2.0 * (dxx + dyy) / 8.0 + 1e-9
