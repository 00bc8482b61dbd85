"""The loss tail of one training iteration (include/gs2m_loss.h, csrc/loss_ops.hip) restated in plain numpy, from the
comments of loss_ops.hip and the reference's utils/loss_utils.py -- not from the kernels' loops.  Three kinds:

  *_f64    the operation in float64 on the float32 inputs, as the reference project writes it (l1_loss :24-25, plane_loss
           :72-78, depth_normal_loss :111-117, _get_img_grad_weight :119-131, the masked means of multi_view_loss :277-291
           and :344-346, tv_loss :536-557, add_densification_stats with the radius update of train.py:223-225);
  *_exact  outputs that are one fixed float32 expression per element: the same expression in np.float32, in the written
           order.  The library is built with -ffp-contract=off, `/` and sqrtf are correctly rounded: these match bit for bit;
  subset_* the counter-based random subset as integers (np.uint64).

The constants C_* count the float32 roundings inside ONE term of a sum (or one element of an output), in units of
u = 2^-24, each next to the expression it counts; expf is allowed 1 ulp = 2 u, as the device library documents.
tests/test_loss_ref.py holds this file to the PyTorch expressions of gs2m_losses.py and to the reference's recorded outputs."""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24                      # unit roundoff of float32
NCC_LIMIT = F32(0.9)                # `ncc < 0.9f`


def f64(x):
    return np.asarray(x, dtype=F64)


def _sgn32(d):
    """torch.sgn: 0 at 0 (and at NaN, whose two comparisons are both false)"""
    return (d > 0).astype(F32) - (d < 0).astype(F32)


def gamma(c):
    """c roundings compounded: c u / (1 - c u)"""
    return c * U / (1.0 - c * U)


# ---------------------------------------------------------------- image loss: clamp / mask, L1, depth-normal term
def chw(image, hwc):
    return np.ascontiguousarray(np.transpose(image, (2, 0, 1))) if hwc else image


def rgb_exact(image, hwc=0, mask=None, background=None):
    """clamp(image, 0, 1) as (3, H, W), `background` where mask is 0; NaN passes the clamp (torch.clamp), -0 stays -0"""
    x = chw(np.asarray(image, dtype=F32), hwc)
    with np.errstate(invalid="ignore"):
        r = np.where(x < 0, F32(0), np.where(x > 1, F32(1), x)).astype(F32)
    if mask is not None:
        r = np.where(np.asarray(mask).reshape(1, *x.shape[1:]) != 0, r, np.asarray(background, dtype=F32).reshape(3, 1, 1)).astype(F32)
    return r


def l1_f64(a, b):
    """l1_loss: torch.abs(network_output - gt).mean()"""
    return np.abs(f64(a) - f64(b)).mean()


def img_grad_f64(gt):
    """_get_img_grad_weight up to its normalisation: (H-2, W-2), the larger of the two channel-mean absolute central differences"""
    g = f64(gt)
    gx = np.abs(g[:, 1:-1, 2:] - g[:, 1:-1, :-2]).mean(0)
    gy = np.abs(g[:, :-2, 1:-1] - g[:, 2:, 1:-1]).mean(0)
    return np.maximum(gx, gy)


def img_grad_weight_f64(gt):
    """_get_img_grad_weight: min-max normalised over the interior, zero on the one-pixel border"""
    g = img_grad_f64(gt)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (g - g.min()) / (g.max() - g.min())
    return np.pad(g, 1)


def edge_exact(gt):
    """the edge strength as float32: ((|d0| + |d1|) + |d2|) / 3 per axis, right - left and top - bottom, the larger of the two;
    0 on the border -> (H, W)"""
    g = np.asarray(gt, dtype=F32)
    ax = [np.abs(g[c, 1:-1, 2:] - g[c, 1:-1, :-2]) for c in range(3)]
    ay = [np.abs(g[c, :-2, 1:-1] - g[c, 2:, 1:-1]) for c in range(3)]
    gx, gy = ((ax[0] + ax[1]) + ax[2]) / F32(3), ((ay[0] + ay[1]) + ay[2]) / F32(3)
    e = np.maximum(gx, gy)
    assert e.dtype == F32
    return np.pad(e, 1)


def _interior(H, W):
    m = np.zeros((H, W), dtype=bool)
    m[1:-1, 1:-1] = True
    return m


def edge_weight_f64(edge, mn, mx):
    """(1 - normalised edge strength).clamp(0, 1) ** 2 from the raw strength and its interior min / max; 1 on the border
    (where the padded normalised strength is 0).  mn == mx: NaN inside, as the reference's 0 / 0."""
    e = f64(edge)
    with np.errstate(invalid="ignore", divide="ignore"):
        gn = np.where(_interior(*e.shape), (e - F64(mn)) / (F64(mx) - F64(mn)), 0.0)
    return np.clip(1.0 - gn, 0.0, 1.0) ** 2


def edge_weight_exact(edge, mn, mx):
    e, mn, mx = np.asarray(edge, dtype=F32), F32(mn), F32(mx)
    with np.errstate(invalid="ignore", divide="ignore"):
        gn = np.where(_interior(*e.shape), (e - mn) / (mx - mn), F32(0)).astype(F32)
        t = F32(1) - gn
        w = np.where(t < 0, F32(0), np.where(t > 1, F32(1), t)).astype(F32)
    return w * w


def dn_weight(H, W, edge, minmax, weight_map, exact=False):
    """the per-pixel weight of the depth-normal term: the edge weight (1 without `edge`) times weight_map when given"""
    if exact:
        w = edge_weight_exact(edge, minmax[0], minmax[1]) if edge is not None else np.ones((H, W), dtype=F32)
        return w * np.asarray(weight_map, dtype=F32).reshape(H, W) if weight_map is not None else w
    w = edge_weight_f64(edge, minmax[0], minmax[1]) if edge is not None else np.ones((H, W))
    return w * f64(weight_map).reshape(H, W) if weight_map is not None else w


# roundings inside one term of the L1 sum |r - g|: the subtraction                                                    -> 1
C_L1 = 1
# one term of the depth-normal sum w * ((d0 + d1) + d2): three subtractions (each relative to its own |d|: 1 in all), two
# adds, the product, w * w and the product with weight_map                                                            -> 6
C_DN = 6
# the edge weight's own error is absolute, not relative to the term it makes small: gn = (e - mn) / (mx - mn) carries 3 u gn,
# 1 - gn one more u, and d (t t) = 2 t dt with t = sqrt(w) <= 1  ->  |dw| <= 8 u sqrt(w)
C_DN_W = 8
# one element of d_sobel = ((g w_dn) / HW) w sgn: the two roundings of the factor, the product, the weight's 8 + 1 (w <= 1) -> 12
C_DN_BWD = 12
# the last lines: (float)(s / n): 1, w_l1 * l1 and w_dn * dn: 1 each, their sum: 1
C_OUT = 1
C_OUT0 = 3


def depth_normal_f64(normal, sobel, w):
    """depth_normal_loss with the weights given: (weights * (sobel - normal).abs().sum(0)).mean()"""
    return (w * np.abs(f64(sobel) - f64(normal)).sum(0)).mean()


def image_loss_f64(image, hwc, mask, background, gt, normal, sobel, edge, minmax, weight_map, w_l1, w_dn):
    """-> dict: rgb (float32, exact), l1, dn, out0 = w_l1 l1 + w_dn dn (the weights as the float32 values the call receives)"""
    rgb = rgb_exact(image, hwc, mask, background)
    _, H, W = rgb.shape
    out = {"rgb": rgb, "l1": l1_f64(rgb, gt), "dn": 0.0}
    if normal is not None:
        out["dn"] = depth_normal_f64(normal, sobel, dn_weight(H, W, edge, minmax, weight_map))
    out["out0"] = F64(F32(w_l1)) * out["l1"] + F64(F32(w_dn)) * out["dn"]
    return out


def image_loss_bwd_exact(image, hwc, mask, gt, normal, sobel, edge, minmax, weight_map, w_l1, w_dn, g_loss, g_rgb):
    """d_image (in the image's layout), d_normal, d_sobel as float32 in the written order:
         k1 = (g w_l1) / (3 HW);  up = g_rgb + k1 sgn(clamp(x) - gt);  d_image = up inside [0, 1] and the mask, else 0
         k2 = ((g w_dn) / HW) w;  d_sobel = k2 sgn(sobel - normal);  d_normal = -d_sobel
       g_loss / g_rgb None: 0"""
    x = chw(np.asarray(image, dtype=F32), hwc)
    _, H, W = x.shape
    HW = F32(H * W)
    g = F32(0) if g_loss is None else F32(g_loss)
    gt = np.asarray(gt, dtype=F32)
    k1 = g * F32(w_l1) / (F32(3) * HW)
    with np.errstate(invalid="ignore"):
        cl = np.where(x < 0, F32(0), np.where(x > 1, F32(1), x)).astype(F32)
        up = (np.asarray(g_rgb, dtype=F32) if g_rgb is not None else np.zeros_like(x)) + k1 * _sgn32(cl - gt)
        passes = (x >= 0) & (x <= 1)
    if mask is not None:
        passes = passes & (np.asarray(mask).reshape(1, H, W) != 0)
    d_image = np.where(passes, up, F32(0)).astype(F32)
    if hwc:
        d_image = np.ascontiguousarray(np.transpose(d_image, (1, 2, 0)))
    if normal is None:
        return d_image, None, None
    w = dn_weight(H, W, edge, minmax, weight_map, exact=True)
    with np.errstate(invalid="ignore"):
        k2 = g * F32(w_dn) / HW * w
        d_sobel = (k2[None] * _sgn32(np.asarray(sobel, dtype=F32) - np.asarray(normal, dtype=F32))).astype(F32)
    return d_image, -d_sobel, d_sobel


# ---------------------------------------------------------------- plane loss
# one term: min is exact; raw: expf -> 2
C_PLANE = 0
C_PLANE_RAW = 2
# one element of the raw backward k exp(s): g * weight 1, / n 1, expf 2, the product 1                                -> 5
C_PLANE_BWD_RAW = 5


def plane_f64(scaling, raw, visible, weight=1.0):
    """plane_loss: mean over the visible Gaussians of sort(scale)[..., 0], 0.0 when none is visible; raw: scale = exp(scaling)
    -> (weight * loss, count)"""
    s = f64(scaling)
    s = np.exp(s) if raw else s
    vis = np.asarray(visible) != 0
    n = int(vis.sum())
    if n == 0:
        return 0.0, 0
    return F64(F32(weight)) * np.sort(s[vis], axis=-1)[..., 0].mean(), n


def first_minimum(scaling):
    """index of the FIRST of the tied minima of each row: torch.min(dim=-1) of gs2m_losses.plane_loss, this project's rule"""
    return np.argmin(np.asarray(scaling), axis=-1)


def plane_bwd_exact(scaling, visible, weight, n, g):
    """non-raw d_scaling as float32: (g weight) / max(n, 1) at the first minimum of every visible row, 0 elsewhere"""
    s = np.asarray(scaling, dtype=F32)
    n = F32(n)
    k = (F32(g) * F32(weight)) / (n if n > 1 else F32(1))
    d = np.zeros_like(s)
    rows = np.nonzero(np.asarray(visible) != 0)[0]
    d[rows, first_minimum(s[rows])] = k
    return d


def plane_bwd_f64(scaling, raw, visible, weight, n, g):
    s = f64(scaling)
    k = F64(F32(g)) * F64(F32(weight)) / max(float(n), 1.0)
    d = np.zeros_like(s)
    rows = np.nonzero(np.asarray(visible) != 0)[0]
    m = first_minimum(np.asarray(scaling)[rows])
    d[rows, m] = k * (np.exp(s[rows, m]) if raw else 1.0)
    return d


# ---------------------------------------------------------------- total variation
# one term (|d| or d d) * w: d 1 (squared: its relative error doubles, and the square rounds: 3), the damping
# exp(-((e0 + e1) + e2) / 3): the argument's roundings are ABSOLUTE errors of the exponent -- three differences, two adds and
# the quotient, each at most u times a partial sum <= 3 max|gt difference| <= 3 for gt in [0, 1] -> 6 * 3 u of relative error
# in the worst case (counted as 6: the partial sums are means of three values below 1, |arg| <= 1) -- expf 2, the product 1;
# with a weight map: the add, the halving (exact) and the product                                                     -> 2
C_TV = 3 + 6 + 2 + 1
C_TV_WM = 2
# one of the (up to four) terms of a backward element  k * w * dd(d):  g = g_loss * weight 1, the double product cast to
# float 1, the quotient 1, the pair weight 6 + 2 (+ 2), k * w 1, d 1, 2 d exact, the product 1; the running sum of four: 3
C_TV_BWD = 1 + 1 + 1 + 8 + 1 + 1 + 1 + 3


def _tv_pairs(gt, pred, weight_map, norm1):
    g, p = f64(gt), f64(pred)
    rgb_grad_h = np.exp(-np.abs(g[:, 1:, :] - g[:, :-1, :]).mean(0, keepdims=True))
    rgb_grad_w = np.exp(-np.abs(g[:, :, 1:] - g[:, :, :-1]).mean(0, keepdims=True))
    dh, dw = p[:, 1:, :] - p[:, :-1, :], p[:, :, 1:] - p[:, :, :-1]
    if weight_map is not None:
        wm = f64(weight_map).reshape(1, *g.shape[1:])
        rgb_grad_h = rgb_grad_h * ((wm[:, 1:, :] + wm[:, :-1, :]) / 2.0)
        rgb_grad_w = rgb_grad_w * ((wm[:, :, 1:] + wm[:, :, :-1]) / 2.0)
    return dh, dw, rgb_grad_h, rgb_grad_w


def tv_f64(gt, pred, weight_map=None, norm1=True, weight=1.0):
    """weight * tv_loss(gt, pred, norm1, weight_map) -> (value, mean of the vertical terms, mean of the horizontal terms)"""
    dh, dw, eh, ew = _tv_pairs(gt, pred, weight_map, norm1)
    lh = (np.abs(dh) if norm1 else dh ** 2) * eh
    lw = (np.abs(dw) if norm1 else dw ** 2) * ew
    return F64(F32(weight)) * (lh.mean() + lw.mean()), lh.mean(), lw.mean()


def tv_bwd_f64(gt, pred, weight_map, norm1, weight, g_loss):
    """d (g_loss * weight * tv_loss) / d pred -> (gradient, sum over the element's up to four terms of their magnitudes)"""
    dh, dw, eh, ew = _tv_pairs(gt, pred, weight_map, norm1)
    g = F64(F32(g_loss)) * F64(F32(weight))
    th = g / dh.size * eh * (np.sign(dh) if norm1 else 2.0 * dh)
    tw = g / dw.size * ew * (np.sign(dw) if norm1 else 2.0 * dw)
    d, mag = np.zeros_like(f64(pred)), np.zeros_like(f64(pred))
    d[:, 1:, :] += th; d[:, :-1, :] -= th; d[:, :, 1:] += tw; d[:, :, :-1] -= tw
    mag[:, 1:, :] += np.abs(th); mag[:, :-1, :] += np.abs(th); mag[:, :, 1:] += np.abs(tw); mag[:, :, :-1] += np.abs(tw)
    return d, mag


# ---------------------------------------------------------------- multi-view loss: the geometric masked means, the NCC tail
# one term gw * nz: the exponent's product nz * decay 1 (an absolute error u nz decay <= u decay of the exponent), expf 2,
# the product 1; the angle term gw * (factor * an): one more product
C_GEO_NOISE = 4     # plus `decay`, added where the bound is formed
C_GEO_ANGLE = 5
# one element of the backward: g_loss * weight 1, gw as above 3 (+ decay), g * gw 1, (* factor 1,) / n 1
C_GEO_DNOISE = 6
C_GEO_DANGLE = 7
C_W_NCC = 2         # expf(-noise)


def mv_geo_masks(noise, angle, valid, angle_threshold):
    """pixel_valid = valid & (noise < 1), angle_valid = valid & (angle < threshold): float32 comparisons, exact"""
    ok = np.asarray(valid) != 0
    with np.errstate(invalid="ignore"):
        return ok & (np.asarray(noise, dtype=F32) < F32(1)), ok & (np.asarray(angle, dtype=F32) < F32(angle_threshold))


def mv_geo_f64(noise, angle, valid, angle_threshold, decay, factor, weight):
    """-> dict: out0 = weight (pixel_loss + angle_loss), n0, n1, pixel_valid, w_ncc (float64), the two term arrays"""
    pv, av = mv_geo_masks(noise, angle, valid, angle_threshold)
    nz, an = f64(noise), f64(angle)
    with np.errstate(invalid="ignore", over="ignore"):
        gw = np.where(pv, np.exp(-np.where(pv, nz, 0.0) * F64(F32(decay))), 0.0)    # geo_weights[~pixel_valid] = 0
        t0 = np.where(pv, gw * np.where(pv, nz, 0.0), 0.0)
        t1 = np.where(av, gw * (F64(F32(factor)) * np.where(av, an, 0.0)), 0.0)
        w_ncc = np.where(pv, np.exp(-np.where(pv, nz, 0.0)), 0.0)
    n0, n1 = int(pv.sum()), int(av.sum())
    pixel_loss = t0[pv].mean() if n0 > 0 else 0.0
    angle_loss = t1[av].mean() if n1 > 0 else 0.0
    return dict(out0=F64(F32(weight)) * (pixel_loss + angle_loss), pixel_loss=pixel_loss, angle_loss=angle_loss, n0=n0, n1=n1,
                pixel_valid=pv, angle_valid=av, w_ncc=w_ncc, gw=gw, t0=t0, t1=t1)


def mv_geo_bwd_f64(noise, angle, valid, angle_threshold, decay, factor, weight, g_loss):
    """geo_w is detached: d_noise = g geo_w / n0 (0 outside pixel_valid, where geo_w is 0), d_angle = g geo_w factor / n1 on angle_valid"""
    r = mv_geo_f64(noise, angle, valid, angle_threshold, decay, factor, weight)
    g = F64(F32(g_loss)) * F64(F32(weight))
    return g * r["gw"] / max(r["n0"], 1), np.where(r["angle_valid"], g * r["gw"] * F64(F32(factor)) / max(r["n1"], 1), 0.0)


C_NCC = 1           # one term ncc * w


def ncc_tail_f64(ncc, w):
    """(ncc * w)[ncc < 0.9].mean(), 0.0 when the mask is empty -> (loss, count)"""
    c = np.asarray(ncc, dtype=F32)
    with np.errstate(invalid="ignore"):
        m = c < NCC_LIMIT
    n = int(m.sum())
    return ((f64(c) * f64(w))[m].mean() if n > 0 else 0.0), n


def d_ncc_exact(ncc, w, n, g_loss):
    """(g w) / max(n, 1) where ncc < 0.9f, else 0, as float32"""
    c = np.asarray(ncc, dtype=F32)
    n = F32(n)
    with np.errstate(invalid="ignore"):
        return np.where(c < NCC_LIMIT, F32(g_loss) * np.asarray(w, dtype=F32) / (n if n > 1 else F32(1)), F32(0)).astype(F32)


def mv_take_exact(idx, W, H, normal_map, dist_map, w_map):
    """-> pixels (n, 2) = (x, y), normals (n, 3), dists (n), w (n; ones without w_map): copies"""
    idx = np.asarray(idx, dtype=np.int64)
    pixels = np.stack([(idx % W).astype(F32), (idx // W).astype(F32)], axis=1)
    normals = np.asarray(normal_map, dtype=F32).reshape(3, -1)[:, idx].T.copy()
    dists = np.asarray(dist_map, dtype=F32).reshape(-1)[idx]
    w = np.asarray(w_map, dtype=F32).reshape(-1)[idx] if w_map is not None else np.ones(idx.shape[0], dtype=F32)
    return pixels, normals, dists, w


def mv_take_bwd_exact(idx, W, H, d_normals, d_dists):
    idx = np.asarray(idx, dtype=np.int64)
    dn, dd = np.zeros((3, H * W), dtype=F32), np.zeros(H * W, dtype=F32)
    dn[:, idx] = np.asarray(d_normals, dtype=F32).T
    dd[idx] = np.asarray(d_dists, dtype=F32)
    return dn.reshape(3, H, W), dd.reshape(H, W)


# one term of affine_mean's sum is a float4: (x + y) + (z + w)                                                         -> 2
C_MEAN = 2
# a + b * (float)(s / n): the cast, the product, the sum
C_MEAN_OUT = 3


def affine_mean_f64(x, a, b):
    return F64(F32(a)) + F64(F32(b)) * f64(x).mean()


# ---------------------------------------------------------------- densification statistics
def densification_exact(vg, visible, observe, radii, accum, accum_abs, denom, max_radii):
    """add_densification_stats + the radius update, as float32: accum += sqrt(gx gx + gy gy), accum_abs += sqrt(gz gz + gw gw),
    denom += 1 where visible; max_radii = max(max_radii, radii) where visible and observe > 0 -> the four updated arrays"""
    v = np.asarray(vg, dtype=F32)
    vis = np.asarray(visible) != 0
    acc, ab, den = (np.asarray(t, dtype=F32).copy() for t in (accum, accum_abs, denom))
    acc[vis] = (acc + np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]))[vis]
    ab[vis] = (ab + np.sqrt(v[:, 2] * v[:, 2] + v[:, 3] * v[:, 3]))[vis]
    den[vis] = (den + F32(1))[vis]
    mr = None
    if max_radii is not None:
        mr = np.asarray(max_radii, dtype=F32).copy()
        m = vis & (np.asarray(observe) > 0)
        mr[m] = np.maximum(mr, np.asarray(radii).astype(F32))[m]
    return acc, ab, den, mr


def densification_f64(vg, visible, observe, radii, accum, accum_abs, denom, max_radii):
    """the same as the reference writes it: torch.norm(grad[filter, :2], dim=-1) ..., torch.max(max_radii[mask], radii[mask])"""
    v = f64(vg)
    vis = np.asarray(visible) != 0
    acc, ab, den = f64(accum).copy(), f64(accum_abs).copy(), f64(denom).copy()
    acc[vis] += np.linalg.norm(v[vis, :2], axis=-1)
    ab[vis] += np.linalg.norm(v[vis, 2:], axis=-1)
    den[vis] += 1
    mr = None
    if max_radii is not None:
        mr = f64(max_radii).copy()
        m = vis & (np.asarray(observe) > 0)
        mr[m] = np.maximum(mr[m], f64(radii)[m])
    return acc, ab, den, mr


# ---------------------------------------------------------------- the random subset, as integers
MASK64 = (1 << 64) - 1
_GOLD, _M1, _M2, _STEP = (np.uint64(c) for c in (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0xD1342543DE82EF95))


def subset_mix(x):
    """splitmix64's finaliser on np.uint64 (arithmetic modulo 2^64)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + _GOLD
        x = (x ^ (x >> np.uint64(30))) * _M1
        x = (x ^ (x >> np.uint64(27))) * _M2
    return x ^ (x >> np.uint64(31))


def subset_bits(seed, i):
    """the 64 random bits of element i: mix(seed ^ i * 0xD1342543DE82EF95)"""
    i = np.asarray(i, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return subset_mix(np.uint64(seed & MASK64) ^ (i * _STEP))


def subset_p(k, count):
    """min((k + 4 sqrt(k)) / max(count, 1), 1) in float32"""
    return min((F32(k) + F32(4) * np.sqrt(F32(k))) / F32(max(int(count), 1)), F32(1))


def subset_thin(mask, k, seed):
    """-> (the surviving indices in increasing order (int64), the set count): element i survives when set and
    u = (bits >> 40) 2^-24 < p"""
    mask = np.asarray(mask).reshape(-1) != 0
    count = int(mask.sum())
    i = np.nonzero(mask)[0]
    u = (subset_bits(seed, i) >> np.uint64(40)).astype(F32) * F32(2.0 ** -24)
    return i[u < subset_p(k, count)].astype(np.int64), count


def subset_removed(m, k, seed):
    """removed_i = min(m - 1, floor((i + U_i) m / e)), U_i = (bits >> 11) 2^-53, in float64; e = m - k"""
    e = m - k
    i = np.arange(e, dtype=np.int64)
    u = (subset_bits(seed, i) >> np.uint64(11)).astype(F64) * 2.0 ** -53
    return np.minimum(np.floor((i.astype(F64) + u) * (F64(m) / F64(e))).astype(np.int64), m - 1)


def bisect_right(key, j):
    """searchsorted(right=True) as the plain bisection it is -- lo = 0, hi = len, mid = (lo + hi) >> 1, `key[mid] <= j` moves lo --
    for every j at once.  On sorted keys: the number of keys <= j."""
    key, j = np.asarray(key, dtype=np.int64), np.asarray(j, dtype=np.int64)
    lo, hi = np.zeros(j.shape, dtype=np.int64), np.full(j.shape, key.shape[0], dtype=np.int64)
    while bool((lo < hi).any()):
        act = lo < hi
        mid = (lo + hi) >> 1
        le = key[np.minimum(mid, key.shape[0] - 1)] <= j
        lo, hi = np.where(act & le, mid + 1, lo), np.where(act & ~le, mid, hi)
    return lo


def subset_remove(m, k, seed, idx):
    """out[j] = idx[j + #{i < e : removed_i - i <= j}] (searchsorted right=True in the keys removed_i - i): the k survivors that
    are kept, in order.  Two neighbouring strata can floor to the same position (m / e not an integer); the keys then step down by
    one there and `the count` is what the bisection returns: one of the two survivors next to that position is skipped as well.
    Either way k distinct survivors in increasing order come out -- what tests assert next to the list itself."""
    key = subset_removed(m, k, seed) - np.arange(m - k, dtype=np.int64)
    j = np.arange(k, dtype=np.int64)
    return np.asarray(idx, dtype=np.int64)[j + bisect_right(key, j)]


def random_subset(mask, k, seed1, seed2):
    """both steps -> exactly min(k, count) distinct set indices in increasing order, or None where the two steps do not
    apply (the thinning came out short while set elements remain, or more than a quarter of the survivors would go)"""
    idx, count = subset_thin(mask, k, seed1)
    m = idx.shape[0]
    if m <= k:
        return idx if m == min(k, count) else None
    if 4 * (m - k) > m:
        return None
    return subset_remove(m, k, seed2, idx)
