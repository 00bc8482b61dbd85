"""A plain numpy reference of the instance emission (csrc/binning.hip: emit_kernel, emit_heavy_kernel, recount_heavy_kernel;
csrc/common.h: gs2m_heavy, gs2m_reaches_quads) for tests/test_emit_gpu.py, tests/test_cull_cover_gpu.py and tests/test_emit_ref.py.
Written from the description of the stage, not from the kernels: every integer of the layout follows from the rectangles and from
the quadrant masks the kernel produced, and the masks themselves are bracketed between two sets computed here:

  must_hit  the quadrants that hold a pixel of the image the blend kernels would accept (alpha = opacity * exp(power) >= 1/255 with
            `power` as the blend kernels round it): a mask that misses one of them loses a contribution;
  may_hit   the quadrants whose pixel rectangle the region {A dx^2 + 2B dx dy + C dy^2 <= t2} can reach at all, in float64, with
            the margins the culling is documented to have: a mask bit outside it is wasted work (and a sign of a wrong test).

Pixel centres are integers; tile t holds pixels 16 t .. 16 t + 15; quadrant q of a tile is the 8 x 8 pixels from
(16 tx + 8 (q & 1), 16 ty + 8 (q >> 1))."""
import numpy as np

TILE = 16
HEAVY_TILES, HEAVY_TILES_CROWDED, CROWDED_WAVE, CROWDED_OFF = 40, 8, 320, 0xFFFFFFFF
UNIT, ROWS_BIG, GID_BITS = 64, 0x80000000, 28
ALPHA_MIN = 1.0 / 255.0
AMBIGUOUS = 1.0e-5      # relative band around 1/255: the exp argument (7e-7), v_exp_f32 (~1 ulp) and the product, times ten
REL_MARGIN = 1.0e-3     # the relative margin gs2m_reaches_quads is documented to compare with
OFF = 3.0e38            # t2 at and above: the culling of this Gaussian is switched off

# ---- (a) the heavy rule -------------------------------------------------------------------------------------------------


def heavy_rule(cnt, crowded):
    """-> (heavy[P] bool, units[P]): per wave of 64 consecutive Gaussians `light` = the sum of the counts below 40; heavy from 40
    instances, from 8 in a wave whose light sum exceeds `crowded`; a heavy Gaussian owns ceil(cnt / 64) units"""
    cnt = np.asarray(cnt, np.int64)
    P = len(cnt)
    w = np.concatenate([cnt, np.zeros((-P) % 64, np.int64)]).reshape(-1, 64)
    light = (w * (w < HEAVY_TILES)).sum(1)
    bar = np.where(light > int(crowded), HEAVY_TILES_CROWDED, HEAVY_TILES)
    heavy = (w >= bar[:, None]).reshape(-1)[:P]
    return heavy, np.where(heavy, (cnt + UNIT - 1) // UNIT, 0)


def block_counts(cnt, crowded):
    """-> (block_tt, block_hu): instances and heavy units per block of 256 Gaussians"""
    cnt = np.asarray(cnt, np.int64)
    _, units = heavy_rule(cnt, crowded)
    pad = (-len(cnt)) % 256
    s = lambda a: np.concatenate([a, np.zeros(pad, np.int64)]).reshape(-1, 256).sum(1).astype(np.uint32)
    return s(cnt), s(units)


def rect_counts(rect):
    rect = np.asarray(rect, np.uint32).reshape(-1, 2)
    return (rect[:, 1] & 0xFFFF).astype(np.int64) * (rect[:, 1] >> 16).astype(np.int64)


def instances(rect):
    """-> (gid, t, tx, ty) of every emission slot: Gaussians in index order, instance t of a rectangle row by row"""
    rect = np.asarray(rect, np.uint32).reshape(-1, 2)
    cnt = rect_counts(rect)
    off = np.cumsum(cnt) - cnt
    gid = np.repeat(np.arange(len(cnt)), cnt)
    t = np.arange(int(cnt.sum())) - off[gid]
    rw = np.maximum((rect[:, 1] & 0xFFFF).astype(np.int64), 1)[gid]
    tx = (rect[:, 0] & 0xFFFF).astype(np.int64)[gid] + t % rw
    ty = (rect[:, 0] >> 16).astype(np.int64)[gid] + t // rw
    return gid, t, tx, ty


def popcount4(m):
    m = np.asarray(m, np.int64)
    return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1)


# ---- (b) the layout, given the masks ------------------------------------------------------------------------------------


def expected_layout(rect, depth_key, masks, crowded, tiles_x, plan):
    """Every integer the stage writes, from the rectangles, the depth keys and the quadrant mask of every emission slot.
    plan: (npass, bits[4], shift[4]) of the tile sort.  -> dict of uint32 arrays (hrec: gid, off, pop as separate arrays)"""
    rect = np.asarray(rect, np.uint32).reshape(-1, 2)
    P = len(rect)
    cnt = rect_counts(rect)
    off = np.cumsum(cnt) - cnt
    R = int(cnt.sum())
    gid, t, tx, ty = instances(rect)
    masks = np.asarray(masks, np.int64)
    assert masks.shape == (R,)
    pc = popcount4(masks)
    heavy, units = heavy_rule(cnt, crowded)
    first_unit = np.cumsum(units) - units
    U = int(units.sum())
    nw = (P + 63) // 64
    hs = heavy[gid]
    pcl = np.where(hs, 0, pc)                                    # rows the waves number themselves
    wave_rows = np.bincount(gid // 64, weights=pcl, minlength=nw).astype(np.int64)
    wave_excl = np.cumsum(wave_rows) - wave_rows
    dense = (np.cumsum(pcl) - pcl) - wave_excl[gid // 64]        # first row of a light instance relative to its wave's first row
    unit = first_unit[gid] + t // UNIT
    row = np.where(hs, ROWS_BIG | (4 * (UNIT * unit + t % UNIT)), dense)
    e_rec = np.zeros((R, 4), np.uint32)
    e_rec[:, 0] = (gid | (masks << GID_BITS)).astype(np.uint32)
    e_rec[:, 1] = row.astype(np.uint32)
    e_rec[:, 2] = np.asarray(depth_key, np.uint32)[gid]
    gauss_rows = np.where(heavy, ROWS_BIG | first_unit, np.bincount(gid, weights=pcl, minlength=P).astype(np.int64)).astype(np.uint32)
    h_gid = np.repeat(np.arange(P), units)
    pop = np.zeros((U, UNIT), np.uint8)
    pop[unit[hs], (t % UNIT)[hs]] = pc[hs]
    keys = (ty * tiles_x + tx).astype(np.uint32)
    npass, bits, shift = plan
    hist = np.zeros((4, 256), np.uint32)
    for p in range(npass):
        hist[p] = np.bincount((keys >> np.uint32(shift[p])) & np.uint32((1 << bits[p]) - 1), minlength=256)
    rows = 4 * UNIT * U + int(wave_rows.sum())
    return dict(keys=keys, e_rec=e_rec, gauss_rows=gauss_rows, wave_rows=wave_rows.astype(np.uint32),
                wave_rowbase=(4 * UNIT * U + wave_excl).astype(np.uint32), h_gid=h_gid.astype(np.uint32), h_off=off[h_gid].astype(np.uint32),
                pop=pop, hist=hist, R=R, U=U, rows=rows, heavy=heavy, units=units, cnt=cnt)


# ---- (c) must_hit: what the blend kernels accept -------------------------------------------------------------------------


def pixel_alpha(gx, gy, A, B, C, op, px, py):
    """-> (power float32, alpha float64) of pixel (px, py) under a Gaussian: `power` in float32, every operation rounded on its own
    and in the written order -0.5 (A dx dx + C dy dy) - B dx dy with dx = x - px; alpha = opacity * exp(power) in float64"""
    f = lambda a: np.asarray(a, np.float32)
    dx, dy = f(gx) - f(px), f(gy) - f(py)
    t1 = (f(A) * dx) * dx
    t2 = (f(C) * dy) * dy
    t3 = (f(B) * dx) * dy
    power = (np.float32(-0.5) * (t1 + t2)) - t3
    with np.errstate(over="ignore"):
        alpha = np.asarray(op, np.float64) * np.exp(power.astype(np.float64))
    return power, alpha


def accepts(power, alpha):
    """-> (required, ambiguous): accepted for certain / within the band around 1/255 in which either answer is right"""
    neg = power <= 0
    return neg & (alpha >= ALPHA_MIN * (1 + AMBIGUOUS)), neg & (alpha >= ALPHA_MIN * (1 - AMBIGUOUS)) & (alpha < ALPHA_MIN * (1 + AMBIGUOUS))


def must_hit(geo, tx, ty, W, H):
    """geo: dict of per-instance gx, gy, A, B, C, op.  -> (must[n, 4] bool, required pixels, ambiguous pixels); a quadrant with an
    ambiguous pixel and no required one is not in must"""
    n = len(tx)
    must = np.zeros((n, 4), bool)
    n_req = n_amb = 0
    o = np.arange(8)
    g = {k: np.asarray(v)[:, None, None] for k, v in geo.items()}
    for q in range(4):
        px = (TILE * np.asarray(tx) + 8 * (q & 1))[:, None, None] + o[None, None, :]
        py = (TILE * np.asarray(ty) + 8 * (q >> 1))[:, None, None] + o[None, :, None]
        power, alpha = pixel_alpha(g["gx"], g["gy"], g["A"], g["B"], g["C"], g["op"], px, py)
        inside = (px < W) & (py < H)
        req, amb = accepts(power, alpha)
        req &= inside; amb &= inside
        must[:, q] = req.any(axis=(1, 2))
        n_req += int(req.sum()); n_amb += int(amb.sum())
    return must, n_req, n_amb


# ---- (d) may_hit: the exact minimum of the quadratic over a quadrant's pixel rectangle -------------------------------------------
# The float32 evaluation the bound `err` has to cover, per edge (dx = l fixed, the minimiser m in dy clamped to the edge; the
# other two edges with x and y exchanged), u = 2^-24, T1 = |A l^2|, T2 = |2 B l m|, T3 = |C m^2|:
#   l = (x0 + o) - x              1 rounding                                   T1: 2u, T2: 1u
#   m = ly or uy when clamped     1 rounding                                   T2: 1u, T3: 2u
#   (A l) l                       2 roundings                                  T1: 2u
#   2B l                          1 rounding (B + B is exact)                  T2: 1u
#   fma(C, m, 2B l)               1 rounding of C m + 2B l, then times m       T2: 1u, T3: 1u
#   fma(.., m, A l^2)             1 rounding of the result, |q| <= T1+T2+T3    T1: 1u, T2: 1u, T3: 1u
# which adds up to T1: 5u, T2: 5u, T3: 4u <= 5u (T1 + T2 + T3) to first order.  An unclamped minimiser is -2B l times a
# reciprocal of 1 ulp: at most 5 roundings, relative error d < 2^-21, and since the derivative vanishes there it moves the
# value by C m^2 d^2 = T3 2^-42 only.  ERR_ROUNDINGS = 6 takes the 5 and one more for every second-order product of them.
ERR_ROUNDINGS = 6
U24 = 2.0 ** -24


def _edge_min(a, b, c, l, lo, hi):
    """min over m in [lo, hi] of a l^2 + 2 b l m + c m^2 -> (value, sum of the absolute terms at the minimiser)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.clip(np.where(c > 0, -b * l / c, lo), lo, hi)
    t1, t2, t3 = a * l * l, 2 * b * l * m, c * m * m
    return t1 + t2 + t3, np.abs(t1) + np.abs(t2) + np.abs(t3) * (1 + 2.0 ** -18)


def quadrant_min(gx, gy, A, B, C, x0, y0):
    """-> (inside, [(value, abs terms)] of the four edges) for the pixel rectangle [x0, x0 + 7] x [y0, y0 + 7], in float64"""
    d = lambda a: np.asarray(a, np.float64)
    gx, gy, A, B, C = d(gx), d(gy), d(A), d(B), d(C)
    lx, ux, ly, uy = d(x0) - gx, d(x0) + 7 - gx, d(y0) - gy, d(y0) + 7 - gy
    inside = (lx <= 0) & (ux >= 0) & (ly <= 0) & (uy >= 0)
    edges = [_edge_min(A, B, C, lx, ly, uy), _edge_min(A, B, C, ux, ly, uy), _edge_min(C, B, A, ly, lx, ux), _edge_min(C, B, A, uy, lx, ux)]
    return inside, edges


def may_hit(geo, tx, ty, W, H):
    """geo: per-instance gx, gy, A, B, C, t2.  -> may[n, 4] bool.  The float32 test computes every edge's value with its own error and
    compares the smallest: it can fire only if some edge's exact minimum lies within t2 (1 + 1e-3) + that edge's err; the centre
    inside the rectangle always counts (the minimum is 0 there); t2 >= 3e38: every quadrant; no pixels in the image: never."""
    n = len(tx)
    may = np.zeros((n, 4), bool)
    t2 = np.asarray(geo["t2"], np.float64)
    for q in range(4):
        x0, y0 = TILE * np.asarray(tx) + 8 * (q & 1), TILE * np.asarray(ty) + 8 * (q >> 1)
        inside, edges = quadrant_min(geo["gx"], geo["gy"], geo["A"], geo["B"], geo["C"], x0, y0)
        with np.errstate(invalid="ignore", over="ignore"):
            reach = np.zeros(n, bool)
            for v, s in edges:
                reach |= v <= t2 * (1 + REL_MARGIN) + ERR_ROUNDINGS * U24 * s
        may[:, q] = (inside | reach | ~(t2 < OFF)) & (x0 < W) & (y0 < H)
    return may


def exact_min(gx, gy, A, B, C, x0, y0):
    """the float64 minimum itself (0 with the centre inside): for the cross-check against sampling"""
    inside, edges = quadrant_min(gx, gy, A, B, C, x0, y0)
    return np.where(inside, 0.0, np.minimum.reduce([v for v, _ in edges]))


# ---- (e) what the preprocess kernel derives from a conic and an opacity ----------------------------------------------------------


def cull_params(A, B, C, op):
    """-> (ex, ey, tau2f) float32: half extents of the bounding box of the alpha >= 1/255 ellipse and the bound on the quadratic,
    with the preprocess kernel's margins; -1 below 1/255; infinite for conics that are indefinite or have A C > 1e4 det"""
    A, B, C = (np.asarray(v, np.float32).astype(np.float64) for v in (A, B, C))
    op32 = np.asarray(op, np.float32)
    det = A * C - B * B
    with np.errstate(divide="ignore", invalid="ignore"):
        tau2 = 2.0 * np.maximum(0.0, np.log(255.0 * op32.astype(np.float64)) + 1.0e-3)
        ex = np.sqrt(tau2 * C / det) * 1.001 + 0.01
        ey = np.sqrt(tau2 * A / det) * 1.001 + 0.01
        t2 = tau2 * 1.002 + 1.0e-3
    off = ~(det > 0) | ~(A > 0) | ~(C > 0) | (A * C > 1.0e4 * det)
    ex, ey, t2 = (np.where(off, np.inf, v) for v in (ex, ey, t2))
    low = op32 < np.float32(1.0) / np.float32(255.0)
    ex, ey, t2 = (np.where(low, -1.0, v) for v in (ex, ey, t2))
    return ex.astype(np.float32), ey.astype(np.float32), t2.astype(np.float32)


def conic(major, minor, angle):
    """float32 (A, B, C) of the Gaussian with standard deviations `major` along `angle` (radians) and `minor` across"""
    c, s = np.cos(angle), np.sin(angle)
    ia, ib = 1.0 / np.square(np.asarray(major, np.float64)), 1.0 / np.square(np.asarray(minor, np.float64))
    return (c * c * ia + s * s * ib).astype(np.float32), (c * s * (ia - ib)).astype(np.float32), (s * s * ia + c * c * ib).astype(np.float32)


def tile_rect(gx, gy, ex, ey, tiles_x, tiles_y, max_tiles=None):
    """{xmin | ymin << 16, w | h << 16} of the tiles the box [x - ex, x + ex] x [y - ey, y + ey] reaches, clipped to the grid; (0, 0)
    when there is none (also for negative extents); max_tiles: at most that many tiles either way, around the centre's tile"""
    gx, gy, ex, ey = (np.asarray(v, np.float64) for v in (gx, gy, ex, ey))

    def span(c, e, n):
        big = ~np.isfinite(e)
        e = np.where(big, 0.0, e)
        lo = np.where(big, 0, np.clip(np.ceil((c - e - 15.0) / TILE), 0, n)).astype(np.int64)
        hi = np.where(big, n, np.clip(np.floor((c + e) / TILE) + 1, 0, n)).astype(np.int64)
        if max_tiles is not None:
            mid = np.clip(np.floor((c + 0.5) / TILE), 0, n - 1).astype(np.int64)
            lo, hi = np.maximum(lo, mid - max_tiles // 2), np.minimum(hi, mid - max_tiles // 2 + max_tiles)
        return lo, np.maximum(hi, lo)
    x0, x1 = span(gx, ex, tiles_x)
    y0, y1 = span(gy, ey, tiles_y)
    none = (ex < 0) | (x1 == x0) | (y1 == y0)
    r = np.stack([x0 | (y0 << 16), (x1 - x0) | ((y1 - y0) << 16)], axis=1)
    r[none] = 0
    return r.astype(np.uint32)


# ---- the cases of tests/test_emit_gpu.py (and of the caps tests/test_emit_ref.py checks on the reference alone) -----------------
OPACITIES = np.array([np.float32(1.0) / np.float32(255.0), np.nextafter(np.float32(1.0) / np.float32(255.0), np.float32(1.0)), 0.004, 0.5, 1.0], np.float32)
RATIOS = (2, 10, 50, 150, 190)
# at 1/255 and one float above, a centre on a pixel centre makes that pixel ambiguous (alpha = 1/255 to 6e-8 and 2e-7): few of them
OPACITY_SHARES = (0.05, 0.05, 0.2, 0.35, 0.35)
IMAGES = {8: (184, 120), 9: (185, 121)}   # W % 16 = H % 16 = 8: the last tile column / row has its left / upper quadrants only; 9: all four


def centres(rng, n, W, H):
    """a sixth each: pixel centres, the quadrant seam (x = 16 k + 7.5), tile corners (16 k - 0.5), anywhere inside, up to 500 pixels
    outside the image on one side, on both"""
    x, y = rng.uniform(0, W, n), rng.uniform(0, H, n)
    k = np.arange(n) % 6
    x, y = np.where(k == 0, np.round(x), x), np.where(k == 0, np.round(y), y)
    x = np.where(k == 1, 16 * np.floor(x / 16) + 7.5, x)
    y = np.where((k == 1) & (rng.random(n) < 0.5), 16 * np.floor(y / 16) + 7.5, y)
    x, y = np.where(k == 2, 16 * np.round(x / 16) - 0.5, x), np.where(k == 2, 16 * np.round(y / 16) - 0.5, y)
    out = rng.uniform(0, 500, (2, n)) * rng.choice([-1, 1], (2, n))
    ox, oy = np.where(out[0] < 0, out[0], W + out[0]), np.where(out[1] < 0, out[1], H + out[1])
    side = rng.random(n) < 0.5
    x = np.where((k == 4) & side, ox, np.where(k == 5, ox, x))
    y = np.where((k == 4) & ~side, oy, np.where(k == 5, oy, y))
    return x.astype(np.float32), y.astype(np.float32)


def make_records(gx, gy, A, B, C, op, t2=None):
    """(P, 32) float32 blend records with the words the stage reads: x, y, A, B | C, opacity | t2 (the rest: a pattern)"""
    P = len(gx)
    rec = np.full((P, 32), 12345.0, np.float32)
    ex, ey, tau = cull_params(A, B, C, op)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 5], rec[:, 6], rec[:, 7] = gx, gy, A, B, C, op, ex, ey
    rec[:, 11] = tau if t2 is None else t2
    return rec


def family_case(name, seed=0, n=600):
    """One conic family: n Gaussians, rectangles = the tiles the bounding box of their alpha >= 1/255 ellipse reaches (the whole
    grid with the culling off).  name: 'iso', 'ratio<r>', 'off', 'low'.  -> case dict"""
    which = 8 if seed % 2 == 0 else 9
    W, H = IMAGES[which]
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    gx, gy = centres(rng, n, W, H)
    op = OPACITIES[rng.choice(len(OPACITIES), n, p=OPACITY_SHARES)]
    fixed = np.deg2rad(np.array([0.0, 45.0, 90.0, 135.0]))
    angle = np.where(np.arange(n) % 2 == 0, fixed[(np.arange(n) // 2) % 4], rng.uniform(0, np.pi, 20)[rng.integers(0, 20, n)])
    max_tiles = None
    if name == "iso":
        major = minor = np.exp(rng.uniform(np.log(0.25), np.log(300.0), n))
    elif name.startswith("ratio"):
        r = float(name[5:])
        minor = np.exp(rng.uniform(np.log(0.3), np.log(min(20.0, 400.0 / r)), n))
        major = r * minor
    elif name == "off":   # 1 + (r - 1/r)^2 sin^2(2 angle) / 4 > 1e4: ratio 210 within 8 degrees of a diagonal, ratio 1000 beyond 6 degrees from an axis
        r = np.where(np.arange(n) % 2 == 0, 210.0, 1000.0)
        diag = np.deg2rad(np.where(rng.random(n) < 0.5, 45.0, 135.0))
        angle = np.where(r == 210.0, diag + np.deg2rad(rng.uniform(-8, 8, n)) * (np.arange(n) % 4 == 0), diag + np.deg2rad(rng.uniform(-35, 35, n)) * (np.arange(n) % 4 == 1))
        minor = np.exp(rng.uniform(np.log(0.3), np.log(2.0), n))
        major = r * minor
        max_tiles = 5    # (the radius rectangle of the reference bounds these in a frame)
    elif name == "low":   # below 1/255: never contributes; the test for the centre's own quadrant remains
        major = np.exp(rng.uniform(np.log(0.5), np.log(40.0), n))
        minor = major / rng.choice([1.0, 3.0, 20.0], n)
        op = np.where(np.arange(n) % 2 == 0, np.float32(0.0039), np.float32(0.002)).astype(np.float32)   # (0.55 % below 1/255: outside the ambiguous band)
        max_tiles = 3
    else:
        raise ValueError(name)
    A, B, C = conic(major, minor, angle)
    rec = make_records(gx, gy, A, B, C, op)
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    ex, ey = rec[:, 6].astype(np.float64), rec[:, 7].astype(np.float64)
    if name == "low":
        ex = ey = np.full(n, 20.0)   # (a frame emits nothing for these; the stage has to cope with what it is given)
    rect = tile_rect(gx, gy, ex, ey, tiles_x, tiles_y, max_tiles)
    depth = rng.uniform(0.2, 50.0, n).astype(np.float32).view(np.uint32)
    return dict(name=f"{name}-{seed}", rect=rect, rec=rec, depth_key=depth, W=W, H=H, tiles_x=tiles_x, tiles_y=tiles_y,
                tile_bits=int(tiles_x * tiles_y).bit_length(), crowded=CROWDED_WAVE)


FAMILIES = ["iso"] + [f"ratio{r}" for r in RATIOS] + ["off", "low"]
CULLED_FAMILIES = FAMILIES[:-2]     # the families whose culling is on: both inclusions have something to say


def geometry(case, gid):
    """the per-instance geometry dict that must_hit / may_hit take"""
    rec = case["rec"]
    return dict(gx=rec[gid, 0], gy=rec[gid, 1], A=rec[gid, 2], B=rec[gid, 3], C=rec[gid, 4], op=rec[gid, 5], t2=rec[gid, 11])


def brackets(case):
    """-> (must[R, 4], may[R, 4], required pixels, ambiguous pixels) of a case's emission slots"""
    gid, _, tx, ty = instances(case["rect"])
    geo = geometry(case, gid)
    must, n_req, n_amb = must_hit({k: geo[k] for k in ("gx", "gy", "A", "B", "C", "op")}, tx, ty, case["W"], case["H"])
    return must, may_hit(geo, tx, ty, case["W"], case["H"]), n_req, n_amb


def bits(mask):
    """(n,) 4-bit masks -> (n, 4) bool"""
    return ((np.asarray(mask, np.int64)[:, None] >> np.arange(4)[None, :]) & 1).astype(bool)


TALL = {8: (88, 696), 9: (89, 697)}       # 6 x 44 = 264 tiles (9 tile bits): room for rectangles of 65 = 5 x 13 and 129 = 3 x 43 tiles
SPECIAL = [(1, 1), (1, 7), (6, 1), (3, 13), (5, 8), (4, 16), (5, 13), (3, 43)]   # w x h: 1, 7, 6, 39, 40, 64, 65, 129 instances


def layout_case(P, kind, seed=0):
    """Rectangles chosen for their COUNTS (the heavy rule, the units, the partial waves and blocks) with conics of every family.
    kind: 'mixed' (SPECIAL among counts of 0 .. 9, on the tall image), 'all-heavy' (every Gaussian of the first wave heavy),
    'crowded' / 'crowded-off' (a wave of light sum 480 holding 7s and 8s, then one of exactly 320), 'light-320'"""
    rng = np.random.default_rng([P, seed, sum(map(ord, kind))])
    which = 8 if (P + seed) % 2 == 0 else 9
    W, H = (TALL if kind == "mixed" else IMAGES)[which]
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    w, h = rng.integers(0, 4, P), rng.integers(0, 4, P)    # counts 0 .. 9, zeros interleaved
    n0 = min(P, 64)
    if kind == "mixed":
        for k, i in enumerate(rng.permutation(P)[:2 * len(SPECIAL)]):
            w[i], h[i] = SPECIAL[k % len(SPECIAL)]
    elif kind == "all-heavy":
        w[:n0], h[:n0] = rng.integers(5, 13, n0), 8
    elif kind in ("crowded", "crowded-off"):
        w[:n0], h[:n0] = np.where(np.arange(n0) % 2 == 0, 7, 8), 1      # light sum 32 x 7 + 32 x 8 = 480 with the rule off
        w[64:128], h[64:128] = 5, 1                                    # 64 x 5 = 320: not crowded
    elif kind == "light-320":
        w[:n0], h[:n0] = 5, 1
    else:
        raise ValueError(kind)
    x0, y0 = rng.integers(0, 1 << 16, P) % (tiles_x - np.maximum(w, 1) + 1), rng.integers(0, 1 << 16, P) % (tiles_y - np.maximum(h, 1) + 1)
    rect = np.stack([x0 | (y0 << 16), w | (h << 16)], axis=1)
    rect[(w == 0) | (h == 0)] = 0
    rect = rect.astype(np.uint32)
    # a centre near the rectangle and a conic of any family: culling on, off and below 1/255
    cx, cy = 16.0 * (x0 + 0.5 * w) + rng.normal(0, 12, P), 16.0 * (y0 + 0.5 * h) + rng.normal(0, 12, P)
    minor = np.exp(rng.uniform(np.log(0.3), np.log(30.0), P))
    major = minor * rng.choice([1.0, 2.0, 10.0, 50.0, 190.0, 1000.0], P)
    A, B, C = conic(major, minor, rng.uniform(0, np.pi, P))
    op = np.where(rng.random(P) < 0.1, np.float32(0.002), OPACITIES[rng.choice(len(OPACITIES), P, p=OPACITY_SHARES)]).astype(np.float32)
    rec = make_records(cx.astype(np.float32), cy.astype(np.float32), A, B, C, op)
    depth = rng.uniform(0.2, 50.0, P).astype(np.float32).view(np.uint32)
    return dict(name=f"{kind}-{P}", rect=rect, rec=rec, depth_key=depth, W=W, H=H, tiles_x=tiles_x, tiles_y=tiles_y,
                tile_bits=int(tiles_x * tiles_y).bit_length(), crowded=CROWDED_OFF if kind == "crowded-off" else CROWDED_WAVE)


LAYOUT_CASES = [(P, "mixed") for P in (1, 63, 64, 65, 255, 256, 257, 1000)] + [(65, "all-heavy"), (257, "all-heavy"), (64, "crowded"), (300, "crowded"),
                                                                                (64, "crowded-off"), (300, "crowded-off"), (64, "light-320"), (255, "light-320")]
