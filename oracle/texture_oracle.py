"""TEST INFRASTRUCTURE ONLY -- never imported by the product (gs-2m_amd/).

numpy (float64) restatement of the three `nvdiffrast.torch.texture` modes the reference uses, following
submodules/nvdiffrast/nvdiffrast/common/textureCUDA.cu: face selection and face coordinates (indexCubeMap :99-121),
texel-space coordinates and the four-texel footprint (indexTextureLinear :362-470), continuation of the footprint
across cube edges (wrapCubeMap :47-92 -- restated geometrically: the texel centre is folded around the edge, and the
neighbour texel is found by SEARCH over the neighbouring face, not by the index algebra the kernel uses), the corner
texel as the average of the other three (fetchQuad :590-607), level selection from the bias alone (calculateMipLevel
:575-589) and the blend of the two levels (:776-779).  Parity unpinned in the strict sense (no golden vectors in the
reference; nvdiffrast is CUDA only): besides this restatement the tests rely on properties that hold for any correct
implementation -- continuity across edges and corners, exactness at texel centres, constants, and the adjoint
identity for the backward."""
import numpy as np

_FACE_POINT = {0: lambda X, Y: (1.0, -Y, -X), 1: lambda X, Y: (-1.0, -Y, X), 2: lambda X, Y: (X, 1.0, Y),
               3: lambda X, Y: (X, -1.0, -Y), 4: lambda X, Y: (X, -Y, 1.0), 5: lambda X, Y: (-X, -Y, -1.0)}


def cube_index(d):
    """direction (3,) -> (face, u, v) with u, v in [0, 1], or None for a non-finite result."""
    x, y, z = (float(np.float32(c)) for c in d)
    ax, ay, az = abs(x), abs(y), abs(z)
    if az > max(ax, ay):
        f, c, s, t = 4, z, x, y
    elif ay > ax:
        f, c, s, t = 2, y, x, z
    else:
        f, c, s, t = 0, x, z, y
    if c < 0:
        f += 1
    with np.errstate(all="ignore"):
        m = np.float64(0.5) / np.float64(abs(c))
        u = s * (-m if f in (0, 5) else m) + 0.5
        v = t * (-m if f != 2 else m) + 0.5
    if not (np.isfinite(u) and np.isfinite(v)):
        return None
    return f, min(max(u, 0.0), 1.0), min(max(v, 0.0), 1.0)


_FOLD = {}


def fold(f, ix, iy, w):
    """texel (ix, iy) of face f, possibly one texel outside -> (face, x, y) on the cube, or None at a corner.
    Memoised on (f, ix, iy, w); the neighbour is still found by search (`_fold_search`)."""
    key = (f, ix, iy, w)
    if key not in _FOLD:
        _FOLD[key] = _fold_search(f, ix, iy, w)
    return _FOLD[key]


def _fold_search(f, ix, iy, w):
    ox, oy = not 0 <= ix < w, not 0 <= iy < w
    if not ox and not oy:
        return f, ix, iy
    if ox and oy:
        return None
    X, Y = (2 * ix + 1 - w) / w, (2 * iy + 1 - w) / w          # face coordinates of the texel centre, one beyond +-1
    p = list(_FACE_POINT[f](X, Y))
    major = f >> 1
    a = [k for k in range(3) if k != major and abs(p[k]) > 1.0][0]
    over = abs(p[a]) - 1.0
    p[major] -= np.sign(p[major]) * over                       # bend the overshoot around the edge
    p[a] = np.sign(p[a])
    g = 2 * a + (1 if p[a] < 0 else 0)
    c = (2 * np.arange(w) + 1 - w) / w                         # the texel of face g whose centre is that point:
    jy, jx = np.meshgrid(c, c, indexing="ij")                  # every texel centre of g at once
    q = _FACE_POINT[g](jx, jy)
    e = sum((np.broadcast_to(qa, jx.shape) - pa) ** 2 for qa, pa in zip(q, p))
    by, bx = np.unravel_index(np.argmin(e), e.shape)
    assert e[by, bx] < 1e-18
    return g, int(bx), int(by)


def footprint_slots(d, w):
    """The four corners of the footprint in the order (u0 v0, u1 v0, u0 v1, u1 v1): [(texel or None, weight)] with
    the weight of a missing corner texel already handed to the other three in thirds, or None (non-finite)."""
    r = cube_index(d)
    if r is None:
        return None
    f, u, v = r
    u, v = u * w - 0.5, v * w - 0.5
    iu0, iv0 = int(np.floor(u)), int(np.floor(v))
    fu, fv = u - iu0, v - iv0
    tex = [fold(f, iu0 + (k & 1), iv0 + (k >> 1), w) for k in range(4)]
    wt = [(1 - fu) * (1 - fv), fu * (1 - fv), (1 - fu) * fv, fu * fv]
    if any(t is None for t in tex):
        miss = [k for k in range(4) if tex[k] is None][0]
        share = wt[miss] / 3.0
        wt = [w_ + share for w_ in wt]
    return list(zip(tex, wt))


def footprint_cube(d, w):
    fp = footprint_slots(d, w)
    return None if fp is None else [(t, w_) for t, w_ in fp if t is not None]


def level_split(b, nlevels):
    """bias (or None: 'linear' on level 0) -> [(level, blend factor)], one or two entries."""
    if b is None:
        return [(0, 1.0)]
    fl = min(max(float(np.float32(b)), 0.0), float(nlevels - 1))
    l0 = int(np.floor(fl))
    if fl > 0:
        return [(l0, 1.0 - (fl - l0)), (min(l0 + 1, nlevels - 1), fl - l0)]
    return [(l0, 1.0)]


def cube_sample(levels, dirs, bias=None):
    """levels: list of (6, w, w, C) arrays; dirs (n, 3); bias (n,) or None -> (n, C) float64."""
    levels = [np.asarray(l, dtype=np.float64) for l in levels]
    out = np.zeros((len(dirs), levels[0].shape[-1]))
    for i, d in enumerate(dirs):
        for lv, a in level_split(None if bias is None else bias[i], len(levels)):
            fp = footprint_cube(d, levels[lv].shape[1])
            if fp is None:
                continue
            for (f, x, y), w_ in fp:
                out[i] += a * w_ * levels[lv][f, y, x]
    return out


def cube_contributions(widths, dirs, bias=None):
    """Every (pixel, level part, corner) of the lookups as flat arrays: `level`, `texel` (x + w (y + w face), -1 where
    nothing is addressed: non-finite direction, missing corner, unused second part), `weight`, `scale` (the level
    blend factor), each of shape (n, 2, 4) -- the order in which a pixel walks its up to eight texels."""
    n = len(dirs)
    level, texel = np.zeros((n, 2, 4), dtype=np.int64), np.full((n, 2, 4), -1, dtype=np.int64)
    weight, scale = np.zeros((n, 2, 4)), np.zeros((n, 2, 4))
    for i, d in enumerate(dirs):
        for part, (lv, a) in enumerate(level_split(None if bias is None else bias[i], len(widths))):
            if a == 0.0:
                continue                                        # bias exactly on a level: the second part has no share
            w = widths[lv]
            fp = footprint_slots(d, w)
            if fp is None:
                continue
            for k, (t, w_) in enumerate(fp):
                if t is not None:
                    level[i, part, k], texel[i, part, k] = lv, t[1] + w * (t[2] + w * t[0])
                    weight[i, part, k], scale[i, part, k] = w_, a
    return level, texel, weight, scale


def _scatter(shapes, level, texel, coef, dy):
    """sum the contributions coef * dy[pixel] into float64 tensors of `shapes` (one per level, channels last); with
    S = sum |scale dy| per texel and channel and cnt = number of contributions per texel.  A pixel whose dy is zero in every channel
    contributes nothing and is not counted."""
    dy = np.asarray(dy, dtype=np.float64).reshape(len(level), -1)
    C = dy.shape[1]
    weight, scale = coef
    on = (texel >= 0) & (dy != 0).any(axis=1).reshape((-1,) + (1,) * (texel.ndim - 1))
    pix = np.broadcast_to(np.arange(len(level)).reshape((-1,) + (1,) * (texel.ndim - 1)), texel.shape)
    grads, Ss, cnts = [], [], []
    for l, shp in enumerate(shapes):
        m = on & (level == l)
        t, p = texel[m], pix[m]
        nt = int(np.prod(shp[:-1]))
        g, S, cnt = np.zeros((nt, C)), np.zeros((nt, C)), np.zeros(nt, dtype=np.int64)
        np.add.at(g, t, (weight[m] * scale[m])[:, None] * dy[p])
        np.add.at(S, t, np.abs(scale[m][:, None] * dy[p]))
        np.add.at(cnt, t, 1)
        grads.append(g.reshape(shp)); Ss.append(S.reshape(shp)); cnts.append(cnt.reshape(shp[:-1]))
    return grads, Ss, cnts


def cube_scatter(widths, C, dirs, dy, bias=None):
    """Transpose of `cube_sample` in float64: dy (n, C) -> (grads, S, cnt), lists with one entry per level: grads
    (6, w, w, C), S (6, w, w, C) = per texel and channel the sum over its contributions of |scale dy|, and cnt
    (6, w, w) = their number.  Built from the footprints and the level split `cube_sample` uses."""
    level, texel, weight, scale = cube_contributions(widths, dirs, bias)
    return _scatter([(6, w, w, C) for w in widths], level, texel, (weight, scale), dy)


def tex2d_footprint(u, v, W, H):
    """uv (float32 values) -> [(iy, ix, weight)] x 4, the index rules of the clamped bilinear lookup."""
    u, v = float(np.float32(u)), float(np.float32(v))
    u = min(max(u * W - 0.5, 0.0), W - 1.0)
    v = min(max(v * H - 0.5, 0.0), H - 1.0)
    iu0, iv0 = int(np.floor(u)), int(np.floor(v))
    iu1 = iu0 + (0 if u in (0.0, W - 1.0) else 1)
    iv1 = iv0 + (0 if v in (0.0, H - 1.0) else 1)
    fu, fv = u - iu0, v - iv0
    return [(iv0, iu0, (1 - fu) * (1 - fv)), (iv0, iu1, fu * (1 - fv)), (iv1, iu0, (1 - fu) * fv), (iv1, iu1, fu * fv)]


def tex2d_clamp_sample(tex, uv):
    tex = np.asarray(tex, dtype=np.float64)
    H, W, _ = tex.shape
    out = np.zeros((len(uv), tex.shape[-1]))
    for i, (u, v) in enumerate(uv):
        for iy, ix, w_ in tex2d_footprint(u, v, W, H):
            out[i] += w_ * tex[iy, ix]
    return out


def tex2d_contributions(H, W, uv):
    """-> texel (ix + W iy) and weight, each (n, 4)."""
    texel, weight = np.zeros((len(uv), 4), dtype=np.int64), np.zeros((len(uv), 4))
    for i, (u, v) in enumerate(uv):
        for k, (iy, ix, w_) in enumerate(tex2d_footprint(u, v, W, H)):
            texel[i, k], weight[i, k] = ix + W * iy, w_
    return texel, weight


def tex2d_clamp_scatter(H, W, C, uv, dy):
    """Transpose of `tex2d_clamp_sample` in float64: dy (n, C) -> (grad (H, W, C), S (H, W, C), cnt (H, W)), S and cnt as
    in `cube_scatter` (scale = 1)."""
    texel, weight = tex2d_contributions(H, W, uv)
    g, S, cnt = _scatter([(H, W, C)], np.zeros_like(texel), texel, (weight, np.ones_like(weight)), dy)
    return g[0], S[0], cnt[0]
