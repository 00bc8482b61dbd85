"""Plain numpy statement of the two blend kernels (csrc/blend_fwd_q.hip, csrc/blend_bwd_q.hip) on caller-made quadrant
lists, and the cases tests/test_blend_ref.py (CPU) and tests/test_blend_gpu.py (GPU) run.  No GPU, no torch.

Layout (common.h: BinningState::qlist / qrow, ImageState; pinned by tests/test_tile_sort_gpu.py): ranges[tile] = (first,
last + 1) of the tile's span; quadrant q of the tile has its list at 4 * first + q * (span length), qcount[4 tile + q]
entries {Gaussian id | quadrant mask << 28, position in the tile's span}; qrow, parallel to the lists, holds the absolute
gradient row of every entry.  A quadrant without pixels has no entries (binning.hip clears its mask bit).  The blend
record is 32 floats per Gaussian (common.h:31-45): x, y, A, B | C, opacity, hx, hy | bin quad | 13 channels + 3 pad |
unused.  The row indices are a random permutation of a range larger than the number of entries: every other row of the
buffer is a guard row.

`forward` / `backward` restate renderCUDA (cuda_rasterizer/forward.cu:315-371, backward.cu:512-596) per pixel over the
quadrant's list, once in float64 and once in float32 in the reference's written order of operations (gs2m_power's order
for the exponent, (c * alpha) * T, T = T / (1 - alpha) entry by entry, one colour-behind recurrence per channel; the sum
over a quadrant's pixels -- the reference's atomicAdd in some order -- in pixel order).  Same code, other dtype.

WHAT A ROW HOLDS (read in blend_bwd_q.hip:358-378 and gaussian_bwd.hip): FINISHED partial gradients, not moments.  The
kernel accumulates moments of s = opacity G dL/dalpha about the Gaussian's own mean, but scales them itself before the
row leaves (-W/2 (A Sx + B Sy), -1/2 Sxx, M0 / opacity, ...), so a row is exactly the sum over the quadrant's pixels of
what backward.cu:582-595 and :551/:560 add with atomicAdd: 0 dL/dmean2D.x, 1 .y, 2 |.x|, 3 |.y|, 4 dL/dconic.x, 5 .y
(once, as backward.cu:591), 6 .w, 7 dL/dopacity, 8..10 dL/dcolour, 11.. dL/dfeature; gaussian_bwd.hip only adds a
Gaussian's rows.  No finishing step is applied here.

THRESHOLD-FREE cases: `settle` evaluates every (pixel, entry) pair in float64 and changes the opacity of an offending
Gaussian (a redraw when nudging does not help) until NO pair lies within the bands BANDS of a branch of the blend.  Two
correct implementations then take the same branches: integer outputs are equal, float outputs differ by rounding only."""
import functools

import numpy as np

TILE = 16
NUM_FEATURES = 10
REC_FLOATS = 32
ROW_FEAT = 11
GID_MASK = 0x0FFFFFFF
# relative bands around the thresholds of the blend inside which a pair counts as near-threshold (power: absolute)
BANDS = dict(alpha=1e-3, power=1e-5, test_T=1e-3, half=1e-3, clamp=1e-3)
# the reference's constants are fp32 literals: both precisions compare against the same numbers
C_099, C_255, C_1EM4 = (float(np.float32(0.99)), float(np.float32(1.0) / np.float32(255.0)), float(np.float32(0.0001)))
GARBAGE = 3.0e18  # magnitude of what unused record / gradient channels hold (finite, also when multiplied by a channel)


def exp32(p):
    """fp32 exp, correctly rounded (through float64): the same on every machine"""
    return np.exp(p.astype(np.float64)).astype(np.float32)


class Case:
    pass


def conic(sx, sy, rho):
    d = 1.0 - rho * rho
    return 1.0 / (sx * sx * d), -rho / (sx * sy * d), 1.0 / (sy * sy * d)


def draw_geo(rng, box, sig=(1.5, 4.0), op=(0.03, 0.3), rho=0.5):
    """one Gaussian {x, y, A, B, C, opacity} centred in the pixel box (x0, y0, x1, y1), off the pixel centres"""
    x0, y0, x1, y1 = box
    x = rng.integers(x0, max(x1, x0 + 1)) + 0.2 + 0.6 * rng.random()
    y = rng.integers(y0, max(y1, y0 + 1)) + 0.2 + 0.6 * rng.random()
    A, B, C = conic(rng.uniform(*sig), rng.uniform(*sig), rng.uniform(-rho, rho))
    return [x, y, A, B, C, rng.uniform(*op)]


def quad_box(tile, q, tiles_x, W, H):
    """pixel box of quadrant q of `tile` clipped to the image, or None when it has no pixels"""
    x0 = (tile % tiles_x) * TILE + (q & 1) * 8
    y0 = (tile // tiles_x) * TILE + (q >> 1) * 8
    return None if x0 >= W or y0 >= H else (x0, y0, min(x0 + 8, W), min(y0 + 8, H))


def assemble(name, W, H, fc, bg, geo, tile_lists, seed, opaque=()):
    """tile_lists: per tile a list of (Gaussian id, quadrant mask); mask bits of quadrants without pixels are cleared and
    entries left without a quadrant are dropped.  `opaque`: Gaussians `settle` must leave as they are."""
    rng = np.random.default_rng(seed + 9000)
    c = Case()
    c.name, c.W, c.H, c.fc, c.bg, c.seed = name, W, H, fc, np.asarray(bg, np.float32), seed
    c.tiles_x, c.tiles_y = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    c.tiles = c.tiles_x * c.tiles_y
    assert len(tile_lists) == c.tiles
    c.geo = np.asarray(geo, np.float64).astype(np.float32).reshape(-1, 6)
    c.P = len(c.geo)
    c.opaque = frozenset(opaque)
    # positive channels: the forward's sums do not cancel, so its bound stays at rounding level (the gradients are signed)
    c.chan = rng.uniform(0.05, 1.5, (c.P, 3 + NUM_FEATURES)).astype(np.float32)
    c.lists = []
    for t, tl in enumerate(tile_lists):
        live = sum(1 << q for q in range(4) if quad_box(t, q, c.tiles_x, W, H))
        c.lists.append([(g, m & live) for g, m in tl if m & live])
    R = sum(len(tl) for tl in c.lists)
    c.R = R
    c.ranges = np.zeros((c.tiles, 2), np.uint32)
    c.qcount = np.zeros(c.tiles * 4, np.uint32)
    c.qlist = np.zeros((max(4 * R, 1), 2), np.uint32)  # unused slots: Gaussian 0, a valid entry
    n_entries = sum(bin(m).count("1") for tl in c.lists for _, m in tl)
    c.n_rows = 2 * n_entries + 16
    perm = rng.permutation(c.n_rows).astype(np.uint32)
    c.guard_row = int(perm[n_entries])  # unused qrow slots point at a guard row: a stray write through them is seen and stays in bounds
    c.qrow = np.full(max(4 * R, 1), c.guard_row, np.uint32)
    c.quads = []  # (tile, q, box, base, [(gid, pos)], rows)
    first, k = 0, 0
    for t, tl in enumerate(c.lists):
        L = len(tl)
        c.ranges[t] = (first, first + L) if L else (0, 0)
        for q in range(4):
            box = quad_box(t, q, c.tiles_x, W, H)
            ent = [(g, pos) for pos, (g, m) in enumerate(tl) if (m >> q) & 1]
            base = 4 * first + q * L
            c.qcount[4 * t + q] = len(ent)
            for i, (g, pos) in enumerate(ent):
                c.qlist[base + i] = (g | (tl[pos][1] << 28), pos)
                c.qrow[base + i] = perm[k + i]
            if box is not None:
                c.quads.append((t, q, box, base, ent, perm[k:k + len(ent)].astype(np.int64)))
            k += len(ent)
        first += L
    assert k == n_entries
    c.used_rows = np.sort(perm[:n_entries].astype(np.int64))
    gr = np.random.default_rng(seed + 17)
    c.grad_color = gr.normal(0.0, 1.0, (3, H, W)).astype(np.float32)
    c.grad_buffer = gr.normal(0.0, 1.0, (NUM_FEATURES, H, W)).astype(np.float32)
    c.grad_buffer[fc:] = np.where(gr.random((NUM_FEATURES - fc, H, W)) < 0.5, -GARBAGE, GARBAGE)
    return c


def record(c):
    """the blend records: garbage in everything the kernels must not use (channels >= fc, pad floats, hx, hy, bin quad, q7)"""
    rng = np.random.default_rng(c.seed + 31)
    rec = np.where(rng.random((c.P, REC_FLOATS)) < 0.5, -GARBAGE, GARBAGE).astype(np.float32)
    rec[:, 0:6] = c.geo
    rec[:, 12:15 + c.fc] = c.chan[:, :3 + c.fc]
    return rec


def _quad_pixels(box):
    x0, y0, x1, y1 = box
    ys, xs = np.mgrid[y0:y1, x0:x1]
    return xs.ravel(), ys.ravel()


def _alpha(c, g, pxf, pyf, dt, exp):
    x, y, A, B, C, op = (dt(v) for v in c.geo[g])
    dx, dy = x - pxf, y - pyf
    power = (dt(-0.5) * ((A * dx) * dx + (C * dy) * dy)) - (B * dx) * dy  # gs2m_power's order
    G = exp(power)
    return dx, dy, power, G, op * G


def forward(c, dt=np.float64, exp=None, margins=False):
    """-> dict(color, buffer, final_T, n_contrib, observe, qlast, qvalid[, margin, offenders])"""
    exp = exp or (np.exp if dt is np.float64 else exp32)
    H, W, fc = c.H, c.W, c.fc
    out = dict(color=np.zeros((3, H, W), dt), buffer=np.zeros((NUM_FEATURES, H, W), dt), final_T=np.ones((H, W), dt),
               n_contrib=np.zeros((H, W), np.uint32), observe=np.zeros(c.P, np.int64), qlast=np.zeros(c.tiles * 4, np.uint32),
               qvalid=np.zeros(c.tiles * 4, bool))
    margin = dict(alpha=np.inf, power=np.inf, test_T=np.inf, half=np.inf, clamp=np.inf)
    offenders = set()
    c99, c255, c1em4 = dt(C_099), dt(C_255), dt(C_1EM4)
    for t, q, box, base, ent, rows in c.quads:
        px, py = _quad_pixels(box)
        pxf, pyf = px.astype(dt), py.astype(dt)
        n = len(px)
        T = np.ones(n, dt)
        acc = np.zeros((n, 3 + fc), dt)
        last = np.zeros(n, np.uint32)
        live = np.ones(n, bool)
        prev_g = np.full(n, -1)  # the Gaussian that left each pixel its T
        ilast = 0
        for i, (g, pos) in enumerate(ent):
            dx, dy, power, G, oG = _alpha(c, g, pxf, pyf, dt, exp)
            alpha = np.minimum(c99, oG)
            cand = live & (power <= 0) & (alpha >= c255)
            test_T = T * (dt(1) - alpha)
            fin = cand & (test_T < c1em4)
            contrib = cand & ~fin
            if margins:
                m = dict(alpha=np.abs(oG / c255 - 1).min(), power=np.abs(power).min(), clamp=np.abs(oG / c99 - 1).min(),
                         test_T=np.abs(test_T[cand] / c1em4 - 1).min(initial=np.inf),
                         half=np.abs(T[contrib] / 0.5 - 1).min(initial=np.inf))
                for k, v in m.items():
                    margin[k] = min(margin[k], float(v))
                    if v < BANDS[k] and k != "half":
                        offenders.add((g, k))
                # T > 0.5 does not depend on this entry: the one to change is the entry that left the pixel its T
                offenders.update((int(p), "half") for p in prev_g[contrib & (np.abs(T / 0.5 - 1) < BANDS["half"])])
            live &= ~fin
            if contrib.any():
                ilast = i + 1
                ch = c.chan[g, :3 + fc].astype(dt)
                w = np.where(contrib, T, dt(0))
                acc += (ch[None, :] * alpha[:, None]) * w[:, None]  # forward.cu:343: c * alpha * T
                out["observe"][g] += int(np.count_nonzero(contrib & (T > 0.5)))
                T = np.where(contrib, test_T, T)
                last = np.where(contrib, np.uint32(pos + 1), last)
                prev_g = np.where(contrib, g, prev_g)
            if not live.any() and not margins:
                break
        out["qlast"][4 * t + q], out["qvalid"][4 * t + q] = ilast, True
        out["final_T"][py, px] = T
        out["n_contrib"][py, px] = last
        bg = c.bg.astype(dt)
        for k in range(3):
            out["color"][k, py, px] = acc[:, k] + T * bg[k]
        for k in range(fc):
            out["buffer"][k, py, px] = acc[:, 3 + k]
    if margins:
        out["margin"], out["offenders"] = margin, offenders
    return out


def backward(c, fwd, dt=np.float64, exp=None, pair_sum=None, keep_terms=False):
    """fwd: final_T, n_contrib, qlast (any precision; converted).  -> rows (n_rows, 11 + fc) in `dt`; rows no entry owns stay NaN.
    pair_sum: dtype the sum over a quadrant's pixels is carried in (default dt, in pixel order).  keep_terms: also
    -> {row: (gid, terms (pixels, 11 + fc))}, the addends of backward.cu's atomicAdds."""
    exp = exp or (np.exp if dt is np.float64 else exp32)
    pair_sum = pair_sum or dt
    fc, NV = c.fc, ROW_FEAT + c.fc
    rows_out = np.full((c.n_rows, NV), np.nan, dt)
    terms_out = {}
    c99, c255 = dt(C_099), dt(C_255)
    halfW, halfH = dt(0.5 * c.W), dt(0.5 * c.H)
    one = dt(1)
    for t, q, box, base, ent, rows in c.quads:
        px, py = _quad_pixels(box)
        pxf, pyf = px.astype(dt), py.astype(dt)
        n = len(px)
        T_final = fwd["final_T"][py, px].astype(dt)
        T = T_final.copy()
        lastc = fwd["n_contrib"][py, px]
        g_pix = np.concatenate([c.grad_color[:, py, px], c.grad_buffer[:fc, py, px]]).T.astype(dt)  # (n, 3 + fc)
        bgdot = np.zeros(n, dt)
        for k in range(3):
            bgdot = bgdot + dt(c.bg[k]) * g_pix[:, k]
        accum = np.zeros((n, 3 + fc), dt)
        last_alpha = np.zeros(n, dt)
        last_col = np.zeros((n, 3 + fc), dt)
        np_ = int(fwd["qlast"][4 * t + q])
        for i in range(len(ent) - 1, -1, -1):
            g, pos = ent[i]
            if i >= np_:
                rows_out[rows[i]] = 0  # behind the quadrant's last contributor: never processed, the row is zeros
                continue
            dx, dy, power, G, oG = _alpha(c, g, pxf, pyf, dt, exp)
            alpha = np.minimum(c99, oG)
            act = (np.uint32(pos) < lastc) & (power <= 0) & (alpha >= c255)
            a = np.where(act, alpha, dt(0))
            T = np.where(act, T / (one - a), T)
            dcd = a * T
            col = c.chan[g, :3 + fc].astype(dt)
            accum = np.where(act[:, None], last_alpha[:, None] * last_col + (one - last_alpha)[:, None] * accum, accum)
            last_col = np.where(act[:, None], col[None, :], last_col)
            dLda = np.zeros(n, dt)
            for k in range(3 + fc):
                dLda = dLda + (col[k] - accum[:, k]) * g_pix[:, k]
            dLda = dLda * T
            last_alpha = np.where(act, alpha, last_alpha)
            dLda = dLda + (-T_final / (one - a)) * bgdot
            op, A, B, C = dt(c.geo[g, 5]), dt(c.geo[g, 2]), dt(c.geo[g, 3]), dt(c.geo[g, 4])
            dL_dG = op * dLda
            gdx, gdy = G * dx, G * dy
            dGx, dGy = -gdx * A - gdy * B, -gdy * C - gdx * B
            terms = np.zeros((n, NV), dt)
            terms[:, 0] = dL_dG * dGx * halfW
            terms[:, 1] = dL_dG * dGy * halfH
            terms[:, 2] = np.abs(terms[:, 0])
            terms[:, 3] = np.abs(terms[:, 1])
            terms[:, 4] = dt(-0.5) * gdx * dx * dL_dG
            terms[:, 5] = dt(-0.5) * gdx * dy * dL_dG
            terms[:, 6] = dt(-0.5) * gdy * dy * dL_dG
            terms[:, 7] = G * dLda
            terms[:, 8:] = dcd[:, None] * g_pix
            terms[~act] = 0
            rows_out[rows[i]] = np.cumsum(terms.astype(pair_sum), axis=0)[-1]
            if keep_terms:
                terms_out[int(rows[i])] = (g, terms)
    return (rows_out, terms_out) if keep_terms else rows_out


def settle(c, max_rounds=400):
    """change opacities until no (pixel, entry) pair is within BANDS of a threshold -> the smallest margins found"""
    rng = np.random.default_rng(c.seed + 77)
    tries = {}
    for _ in range(max_rounds):
        f = forward(c, margins=True)
        if not f["offenders"]:
            c.rec = record(c)
            c.margin = f["margin"]
            return c
        for g in sorted({g for g, _ in f["offenders"]}):
            k = tries[g] = tries.get(g, 0) + 1
            assert g not in c.opaque or k < 50, (c.name, g)
            o = float(c.geo[g, 5])
            if g in c.opaque:  # the structure of the case rests on this one: stay close
                o *= 1.0 + 0.004 * rng.uniform(-1, 1)
            else:
                o = o * (1.0 + 0.05 * rng.uniform(0.2, 1.0)) if k % 4 else rng.uniform(0.03, 0.6)
            c.geo[g, 5] = np.float32(min(o, 0.9995))
    raise AssertionError(f"{c.name}: near-threshold pairs left after {max_rounds} rounds: {sorted(f['offenders'])[:8]}")


# ---- the cases -------------------------------------------------------------------------------------------------------------
def _random_tile(rng, geo, t, lengths, tiles_x, W, H, **kw):
    """a tile list in which quadrant q holds lengths[q] entries (quadrants without pixels: none): every entry is a Gaussian
    of its own, centred in one of its quadrants"""
    boxes = [quad_box(t, q, tiles_x, W, H) for q in range(4)]
    lengths = [l if boxes[q] else 0 for q, l in enumerate(lengths)]
    L = max(lengths)
    masks = np.zeros(L, np.int64)
    for q, l in enumerate(lengths):
        sel = np.arange(L) if l == L else rng.choice(L, l, replace=False)
        masks[sel] |= 1 << q
    tl = []
    for m in masks:
        if m == 0:
            continue
        qs = [q for q in range(4) if (m >> q) & 1]
        geo.append(draw_geo(rng, boxes[qs[rng.integers(len(qs))]], **kw))
        tl.append((len(geo) - 1, int(m)))
    return tl


def _lengths_case(name, seed, lengths, W=16, H=16, fc=5, bg=(0, 0, 0)):
    rng = np.random.default_rng(seed)
    geo = []
    tiles_x, tiles = (W + 15) // 16, ((W + 15) // 16) * ((H + 15) // 16)
    # low opacities: nothing saturates, every list is walked to its end
    op = (0.02, 0.12) if max(max(l) for l in lengths) > 40 else (0.03, 0.3)
    lists = [_random_tile(rng, geo, t, lengths[t % len(lengths)], tiles_x, W, H, op=op) for t in range(tiles)]
    return assemble(name, W, H, fc, bg, geo, lists, seed)


def _big(box, op, sigma=100.0):
    """a splat that is flat over the quadrant `box`: G > 0.993 on every pixel"""
    A, B, C = conic(sigma, sigma, 0.0)
    return [0.5 * (box[0] + box[2]) + 0.37, 0.5 * (box[1] + box[3]) - 0.41, A, B, C, op]


def _stop_case(name, seed, s, partial=False):
    """every pixel of quadrant 0 is finished by entry s of a 40-entry list (n_contrib = s: entries s - 2 and s - 1 leave
    T ~ 1e-3 of what the fillers in front left, entry s is refused by the T test).  (1 - 0.99)^2 IS the threshold 1e-4, so
    two clamped entries alone cannot finish a pixel away from it: s = 2 is the earliest stop a threshold-free case has.
    partial: four small stoppers (alpha ~ 0.95 at best: entries s - 3 .. s) finish only the pixels around (3, 3) at entry s; the
    others walk the whole list."""
    rng = np.random.default_rng(seed)
    W = H = 16
    geo, tl, opaque = [], [], []
    box = quad_box(0, 0, 1, W, H)
    for i in range(40):
        if i in (s - 2, s - 1, s) or (partial and i == s - 3):
            o = 0.999 if i != s - 1 else 0.9
            if partial:
                A, B, C = conic(2.0, 2.0, 0.0)
                geo.append([3.3, 3.4, A, B, C, o])
            else:
                geo.append(_big(box, o))
            opaque.append(len(geo) - 1)
            tl.append((len(geo) - 1, 0x1))
        else:
            geo.append(draw_geo(rng, box, sig=(1.5, 3.0), op=(0.02, 0.08)))
            tl.append((len(geo) - 1, 0x1 | (int(rng.integers(0, 8)) << 1)))
    return assemble(name, W, H, 5, (0.3, 0.2, 0.9), geo, [tl], seed, opaque=opaque)


def _spread_case(name, seed):
    """quadrant 0: entries 0..29 cover its left columns only, 30..69 its right columns: n_contrib differs by groups between the pixels
    of a wave, so the carried T / b / n_contrib of the left pixels sit unused in LDS while the right ones are worked on"""
    rng = np.random.default_rng(seed)
    geo, tl = [], []
    for i in range(70):
        A, B, C = conic(rng.uniform(0.7, 1.0), rng.uniform(3.0, 6.0), 0.0)
        x = (rng.integers(0, 2) if i < 30 else rng.integers(6, 8)) + 0.2 + 0.6 * rng.random()
        geo.append([x, rng.integers(0, 8) + 0.2 + 0.6 * rng.random(), A, B, C, rng.uniform(0.05, 0.3)])
        tl.append((i, 0x1))
    return assemble(name, 16, 16, 5, (0.5, 0.25, 1.0), geo, [tl], seed)


def _clamp_case(name, seed):
    """opacity * G well above 0.99 at the pixels next to a splat's centre and well below further out, several splats per quadrant"""
    rng = np.random.default_rng(seed)
    geo, tl = [], []
    for i in range(24):
        q = i % 4
        box = quad_box(0, q, 1, 16, 16)
        if i % 3 == 0:
            geo.append(draw_geo(rng, box, sig=(7.0, 10.0), op=(0.9985, 0.9995), rho=0.3))
        else:
            geo.append(draw_geo(rng, box, sig=(1.5, 4.0), op=(0.05, 0.4)))
        tl.append((i, 1 << q | int(rng.integers(0, 16))))
    return assemble(name, 16, 16, 5, (0.1, 0.2, 0.3), geo, [tl], seed)


def _shared_case(name, seed):
    """30 wide splats around the centre of a 32 x 32 image, each in all four tiles and all sixteen quadrants, a row for each.
    Gaussian 0 is in front everywhere and takes every pixel's T from 1 to below 0.25 in one step: with 1024 pixels under every
    splat, a T that wanders past 0.5 somewhere could not be kept out of the band by changing opacities."""
    rng = np.random.default_rng(seed)
    geo = [_big((0, 0, 32, 32), 0.9, sigma=40.0)] + [draw_geo(rng, (10, 10, 22, 22), sig=(6.0, 12.0), op=(0.03, 0.2)) for _ in range(29)]
    lists = [[(0, 0xF)] + [(int(g) + 1, 0xF) for g in rng.permutation(29)] for _ in range(4)]
    return assemble(name, 32, 32, 9, (0, 0, 0), geo, lists, seed, opaque=(0,))


def _many_tiles_case(name, seed):
    """5 x 8 tiles (not a multiple of 8: the last block-id group of the XCD mapping is partial), spans of 0 .. 80 entries"""
    rng = np.random.default_rng(seed)
    W, H = 80, 128
    geo, lists = [], []
    for t in range(40):
        L = int(rng.integers(0, 81)) if t not in (3, 17) else 0
        lists.append(_random_tile(rng, geo, t, [int(rng.integers(0, L + 1)) for _ in range(3)] + [L], 5, W, H, op=(0.02, 0.2)))
    return assemble(name, W, H, 9, (0.2, 0.4, 0.6), geo, lists, seed)


def _long_case(name, seed, n=330):
    """one quadrant (an 8 x 8 image), n entries: a large low-opacity splat in front, small ones behind it"""
    rng = np.random.default_rng(seed)
    A, B, C = conic(27.0, 27.0, 0.0)
    geo = [[3.4, 4.3, A, B, C, 0.1]]
    for _ in range(n - 1):
        geo.append(draw_geo(rng, (0, 0, 8, 8), sig=(0.8, 1.6), op=(0.03, 0.3)))
    return assemble(name, 8, 8, 9, (0.3, 0.1, 0.2), geo, [[(i, 0x1) for i in range(n)]], seed)


LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 100)
STOPS = (2, 15, 16, 17, 31, 32)
EDGES = ((1, 1), (7, 5), (8, 8), (9, 17), (16, 16), (17, 33), (23, 16))
FCS = (0, 1, 2, 4, 5, 6, 8, 9, 10)
BG_BIG = (37.5, 120.25, 64.0)

BUILDERS = {}
for _k, _l in enumerate(((0, 1, 15, 16), (17, 31, 32, 33), (47, 48, 49, 64), (65, 100, 16, 33))):
    BUILDERS[f"len{_k}"] = functools.partial(_lengths_case, seed=100 + _k, lengths=[_l])
for _s in STOPS:
    BUILDERS[f"stop{_s}"] = functools.partial(_stop_case, seed=200 + _s, s=_s)
BUILDERS["stop_some"] = functools.partial(_stop_case, seed=250, s=16, partial=True)
BUILDERS["spread"] = functools.partial(_spread_case, seed=300)
for _w, _h in EDGES:
    BUILDERS[f"edge{_w}x{_h}"] = functools.partial(_lengths_case, seed=400 + _w, lengths=[(20, 9, 33, 17), (5, 40, 12, 26)], W=_w, H=_h)
for _f in FCS:
    BUILDERS[f"fc{_f}"] = functools.partial(_lengths_case, seed=500 + _f, lengths=[(20, 35, 10, 18), (3, 17, 30, 8)], W=23, H=16, fc=_f)
BUILDERS["bg0"] = functools.partial(_lengths_case, seed=600, lengths=[(30, 12, 21, 40)], bg=(0, 0, 0))
BUILDERS["bgbig"] = functools.partial(_lengths_case, seed=600, lengths=[(30, 12, 21, 40)], bg=BG_BIG)
BUILDERS["clamp"] = functools.partial(_clamp_case, seed=700)
BUILDERS["shared"] = functools.partial(_shared_case, seed=800)
BUILDERS["many_tiles"] = functools.partial(_many_tiles_case, seed=900)
BUILDERS["long"] = functools.partial(_long_case, seed=1000)
SHORT_CASES = tuple(k for k in BUILDERS if k != "long")  # every quadrant list has at most 100 entries; "long" has its own bound


@functools.lru_cache(maxsize=None)
def case(name):
    return settle(BUILDERS[name](name))


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (case, forward64, rows64, forward32, rows32): computed once per process, shared by every test, never modified"""
    c = case(name)
    f64 = forward(c)
    f32 = forward(c, np.float32)
    return c, f64, backward(c, f64), f32, backward(c, f32, np.float32)


def truncated(c, n):
    """the case `c` (one tile) with its span cut to the first n entries: still threshold-free, the pairs are a subset"""
    t = assemble(f"{c.name}[:{n}]", c.W, c.H, c.fc, c.bg, c.geo, [c.lists[0][:n]], c.seed)
    t.geo = c.geo.copy()
    t.chan = c.chan
    t.rec = record(t)
    return t


def rel_err(a, ref, scale):
    """largest element-wise |a - ref| / (|ref| + 1e-6 scale); scale: a number, or per row (broadcast)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - ref) / (np.abs(ref) + 1e-6 * scale + 1e-300)))


ROW_GROUPS = ((0, 4), (4, 7), (7, 8), (8, 11), (11, None))  # dL/dmean2D, dL/dconic, dL/dopacity, dL/dcolour, dL/dfeature


def rows_norm_err(rows, ref):
    """largest ||rows[:, k] - ref[:, k]|| / ||ref[:, k]|| over the columns k: unlike the element-wise figure it is not set by the
    one element of a case that cancels furthest"""
    a, b = np.asarray(rows, np.float64), np.asarray(ref, np.float64)
    n = np.linalg.norm(b, axis=0)
    return float(np.max(np.linalg.norm(a - b, axis=0)[n > 0] / n[n > 0], initial=0.0))


# Measured by tests/test_blend_ref.py (fp32 restatement against float64, the largest over the cases; asserted there within 2 x):
E_IMAGE = 8.1e-7     # colour and buffer, relative to |ref| + 1e-6 max|image|      (all cases)
E_FINAL_T = 4.5e-6    # final_T (all cases; the clamp case: 1 - alpha at alpha = 0.99 carries 100 x alpha's rounding)
E_ROWS = 3.4e-2      # rows, element-wise, relative to |ref| + 1e-6 max|row|        (SHORT_CASES; set by one cancelling element)
E_ROWS_NORM = 1.8e-6   # rows, column norm-wise                                       (SHORT_CASES)
FACTOR = 4.0         # what the kernels may take on top: v_exp_f32 of x log2(e), packed-FMA / MFMA summation order, one reciprocal of the scanned product


def restatement_errors(name):
    """fp32 restatement against float64 on one case -> (colour and buffer, final_T, rows)"""
    c, f64, r64, f32, r32 = reference(name)
    e_img = max(rel_err(f32["color"], f64["color"], np.abs(f64["color"]).max()),
                rel_err(f32["buffer"][:c.fc], f64["buffer"][:c.fc], np.abs(f64["buffer"]).max()) if c.fc else 0.0)
    e_T = rel_err(f32["final_T"], f64["final_T"], np.abs(f64["final_T"]).max())
    u = c.used_rows
    e_rows = rel_err(r32[u], r64[u], np.abs(r64[u]).max(axis=1, keepdims=True)) if len(u) else 0.0
    return e_img, e_T, e_rows, (rows_norm_err(r32[u], r64[u]) if len(u) else 0.0)
