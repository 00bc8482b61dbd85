"""Row layouts with EXACT sums for the per-Gaussian backward (csrc/gaussian_bwd.hip), for tests/test_gaussian_bwd_gpu.py and
tests/test_gaussian_bwd_ref.py; numpy only, no GPU code.

A layout is what the binning stage (csrc/binning.hip) leaves for the backward: gauss_rows (rows of each Gaussian inside its wave's
dense run, or ROWS_BIG | first unit of a heavy one), tiles_touched (instances: ceil(/ 64) units of a heavy one), wave_rowbase (first
row of the run of each wave of 64 Gaussians), hrec (80 bytes per heavy unit, the last 64 of them the `pop` bytes: rows
256 u + 4 k .. + pop[k] - 1 are written), counters, and the rows buffer: the heavy units' 256 rows each first, the waves' runs behind
them.  `arrange` may leave a gap between two waves' runs: wave_rowbase is an input of the kernel.

Everything the kernel must not read is NaN: the gaps, the unwritten rows of a unit, the padding lanes 11 + fc .. rowf - 1 of every
row and GUARD_ROWS rows on either side of the buffer.

Every written element is k * 2^-12 with an integer |k| <= 64 (never -0), and `arrange` asserts in int64 that the sum of |k| over the
rows of every Gaussian stays below 2^24 in every lane: every partial sum, in any order, is then an integer below 2^24 times 2^-12,
exact in float32, whichever path of the kernel added it.  The expected sum is the int64 sum converted once.  That is what allows bit
comparison between 2 and 3 windows in flight, between row widths and between a dense and a heavy arrangement of the same rows."""
import numpy as np

import emit_ref as E
import preprocess_ref as R

F32 = np.float32
WAVE, UNIT, ROWS_BIG = 64, 64, 0x80000000
CNT_ROWS, CNT_HUNITS = 2, 3
GUARD_ROWS = 64
NCH = 21                      # lanes of a row at fc = 10: means2D 4, conic 3, opacity, colour 3, features 10
KMAX, STEP = 64, 2.0 ** -12
FCS = (0, 2, 6, 10)           # row widths of 12, 16, 20, 24 floats: 3, 4, 5, 6 float4
GROUPS = {0: 21, 2: 16, 6: 12, 10: 10}   # fc -> G = 64 // (float4 per row): lane groups that walk Gaussians j, j + G, ...
RANDOM_COUNTS = (0, 0, 1, 2, 3, 4, 7, 12, 40)


def row_floats(fc):
    return (11 + fc + 3) // 4 * 4


def make_values(counts, seed):
    """-> per Gaussian an int64 array (rows, NCH) of k in -64 .. 64"""
    counts = np.asarray(counts, np.int64)
    big = np.random.default_rng(seed).integers(-KMAX, KMAX + 1, (int(counts.sum()), NCH))
    return np.split(big, np.cumsum(counts)[:-1])


class Layout:
    pass


def arrange(name, fc, values, heavy=None, gaps=None):
    """values: per Gaussian an int array (rows, >= 11 + fc); heavy: {Gaussian: pop bytes, one per instance, 0 .. 4, their sum the
    Gaussian's rows}; gaps: rows left out in front of each wave's run.  -> Layout (arrays as the kernel reads them, `rows` with its
    guard rows, `sums` int64 (P, 11 + fc), `expected` {output: float32 array})"""
    heavy = heavy or {}
    P, nch, rowf = len(values), 11 + fc, row_floats(fc)
    nw = (P + WAVE - 1) // WAVE
    gaps = np.zeros(nw, np.int64) if gaps is None else np.asarray(gaps, np.int64)
    assert len(gaps) == nw
    vals = [np.asarray(v, np.int64)[:, :nch] for v in values]
    for i, v in enumerate(vals):   # the exactness condition (a condition on the case, not a tolerance)
        assert np.abs(v).max(initial=0) <= KMAX and np.abs(v).sum(0).max(initial=0) < 2 ** 24, f"{name}: Gaussian {i}"
    first_unit, units = {}, 0
    for i in sorted(heavy):
        pop = np.asarray(heavy[i])
        assert len(pop) > 0 and pop.max() <= 4 and pop.min() >= 0 and int(pop.sum()) == len(vals[i]), f"{name}: heavy Gaussian {i}"
        first_unit[i] = units
        units += (len(pop) + UNIT - 1) // UNIT
    cnt = np.array([0 if i in heavy else len(v) for i, v in enumerate(vals)], np.int64)
    n_rows = units * 4 * UNIT + int(cnt.sum()) + int(gaps.sum())
    rows = np.full((GUARD_ROWS + n_rows + GUARD_ROWS, rowf), np.nan, F32)
    body = rows[GUARD_ROWS:GUARD_ROWS + n_rows]
    hrec = np.zeros((units, 80), np.uint8)
    tiles_touched = ((cnt + 3) // 4).astype(np.uint32)
    gauss_rows = cnt.astype(np.uint32)
    for i in sorted(heavy):
        pop = np.asarray(heavy[i], np.int64)
        u0, nu = first_unit[i], (len(pop) + UNIT - 1) // UNIT
        start = np.cumsum(pop) - pop
        r = u0 * 4 * UNIT + np.repeat(4 * np.arange(len(pop)), pop) + (np.arange(int(pop.sum())) - np.repeat(start, pop))
        body[r, :nch] = (vals[i] * STEP).astype(F32)
        padded = np.zeros(nu * UNIT, np.uint8)
        padded[:len(pop)] = pop
        hrec[u0:u0 + nu, 16:] = padded.reshape(nu, UNIT)
        hrec[u0:u0 + nu, :16].view(np.uint32)[:] = np.array([i, 0xA5A5A5A5, 0xA5A5A5A5, 0xA5A5A5A5], np.uint32)
        tiles_touched[i] = len(pop)
        gauss_rows[i] = ROWS_BIG | u0
    wave_rowbase = np.zeros(nw, np.uint32)
    at = units * 4 * UNIT
    for w in range(nw):
        at += int(gaps[w])
        wave_rowbase[w] = at
        for i in range(w * WAVE, min(P, (w + 1) * WAVE)):
            if cnt[i]:
                body[at:at + cnt[i], :nch] = (vals[i] * STEP).astype(F32)
                at += int(cnt[i])
    assert at == n_rows
    counters = np.zeros(64, np.uint32)
    counters[CNT_ROWS], counters[CNT_HUNITS] = n_rows, units
    sums = np.stack([v.sum(0) for v in vals]) if P else np.zeros((0, nch), np.int64)
    s = (sums * STEP).astype(F32)
    assert np.array_equal(s.astype(np.float64), sums * STEP)   # converted once, exactly
    zero = np.zeros(P, F32)
    feat = np.zeros((P, R.NUM_FEATURES), F32)
    feat[:, :fc] = s[:, 11:11 + fc]
    L = Layout()
    L.__dict__.update(name=name, P=P, fc=fc, rowf=rowf, units=units, n_rows=n_rows, gauss_rows=gauss_rows, tiles_touched=tiles_touched,
                      wave_rowbase=wave_rowbase, hrec=hrec, counters=counters, rows=rows, sums=sums, heavy=sorted(heavy), first_unit=first_unit,
                      expected=dict(means2D=s[:, 0:4].copy(), conics=np.stack([s[:, 4], s[:, 5], zero, s[:, 6]], 1), opacities=s[:, 7].copy(),
                                    colors=s[:, 8:11].copy(), features=feat))
    return L


def unit_sum_rows(L):
    """rows of the buffer (guard rows counted) that the heavy units' sums are written over: the first row of every unit"""
    return GUARD_ROWS + 4 * UNIT * np.arange(L.units)


# ---- what a wave's counts contain ------------------------------------------------------------------------------------------------------


def wave_total(counts):
    return int(np.sum(counts))


def n_windows(counts):
    return (wave_total(counts) + WAVE - 1) // WAVE


def covers(counts):
    """-> [(j, first row, rows, first covered window, covered windows)] of the Gaussians of one wave that cover whole 64-row windows"""
    c = np.asarray(counts, np.int64)
    ex = np.cumsum(c) - c
    out = []
    for j in range(len(c)):
        w0, w1 = -(-int(ex[j]) // WAVE), int(ex[j] + c[j]) // WAVE
        if c[j] > 0 and w1 > w0:
            out.append((j, int(ex[j]), int(c[j]), w0, w1 - w0))
    return out


# ---- the row patterns, one per wave ----------------------------------------------------------------------------------------------------
WAVE_TOTALS = (63, 0, 64, 1, 65, 127, 128, 129, 192, 193, 257)   # nwin 0 .. 5: every residue mod 2 and mod 3; the empty wave between two busy ones


def _spread(rng, total):
    return rng.multinomial(total, np.full(WAVE, 1.0 / WAVE)).astype(np.int64)


def _random_wave(rng):
    c = rng.choice(RANDOM_COUNTS, WAVE).astype(np.int64)
    c[0], c[63] = 7, 3
    return c


ALIGNED_AT = 30   # lane of the window-aligned Gaussian: 30 - G = 9, 14, 18, 20 and its neighbours 29, 31 hold no rows


def _aligned_wave(n, at_end):
    """one Gaussian of n rows (a multiple of 64) whose first row is row 64 of the wave's run; zero-row Gaussians in front of it,
    behind it and at j - G of every row width; at_end: nothing behind it, the run of covered windows ends on the wave's last window"""
    c = np.zeros(WAVE, np.int64)
    c[[0, 3, 8, 10, 15, 22, 27]] = (9, 1, 14, 20, 5, 12, 3)     # 64 rows in front
    assert c[:ALIGNED_AT].sum() == 64
    c[ALIGNED_AT] = n
    if not at_end:
        c[[33, 40, 63]] = (5, 70, 2)
    return c


def _mid_wave(places):
    """places: [(lane, whole windows, rows behind them)]: Gaussians that start mid-window, cover that many whole windows and end
    mid-window; small ones between them"""
    c = np.zeros(WAVE, np.int64)
    c[0] = 20
    for lane, whole, tail in places:
        pos = int(c[:lane].sum())
        assert pos % WAVE != 0
        c[lane] = (WAVE - pos % WAVE) + WAVE * whole + tail
        if lane + 1 < WAVE and tail:
            c[lane + 1] = 3
    return c


def pattern_waves(which):
    """-> [(name, counts[64])] of pattern set 'A' or 'B', 16 waves each"""
    rng = np.random.default_rng(11 if which == "A" else 12)
    if which == "A":
        w = [(f"total-{t}", _spread(rng, t)) for t in WAVE_TOTALS]
        w.append(("random", _random_wave(rng)))
        w += [("aligned-64", _aligned_wave(64, False)), ("aligned-128", _aligned_wave(128, False)), ("aligned-192", _aligned_wave(192, False)),
              ("aligned-320-end", _aligned_wave(320, True))]
    else:
        w = [("mid", _mid_wave([(5, 2, 30)])), ("mid-two-groups", _mid_wave([(5, 2, 30), (40, 3, 11)]))]
        for G in (21, 16, 12, 10):
            w.append((f"mid-same-group-{G}", _mid_wave([(3, 2, 17), (3 + G, 2, 40)])))
        b = np.zeros(WAVE, np.int64)   # back to back: the second begins on the window edge the first ends on
        b[0], b[7], b[8], b[9] = 20, 44 + 128, 128 + 10, 6
        w.append(("back-to-back", b))
        w.append(("zero", np.zeros(WAVE, np.int64)))
        w.append(("all-40", np.full(WAVE, 40, np.int64)))
        last = np.zeros(WAVE, np.int64); last[63] = 130
        w.append(("lane-63-only", last))
        first = np.zeros(WAVE, np.int64); first[0] = 256
        w.append(("lane-0-only", first))
        w += [(f"random-{k}", _random_wave(rng)) for k in range(5)]
    assert len(w) == 16
    return w


PATTERN_SIZES = {"A": (1025, 1023), "B": (1024, 1027)}   # P % 256 = 1 (a last wave of one Gaussian), 255, 0, 3
TAILS = {1023: (), 1024: (), 1025: (70,), 1027: (5, 0, 9)}


def pattern_counts(which, P):
    assert P in PATTERN_SIZES[which]
    c = np.concatenate([x for _, x in pattern_waves(which)] + [np.array(TAILS[P], np.int64)])
    return c[:P] if P < len(c) else c


def pattern_gaps(P):
    nw = (P + WAVE - 1) // WAVE
    return (np.arange(nw) * 7) % 5 * 3


def pattern_layout(which, P, fc):
    counts = pattern_counts(which, P)
    return arrange(f"rows-{which}-{P}-fc{fc}", fc, make_values(counts, 100 + P), gaps=pattern_gaps(P))


# ---- the heavy patterns ----------------------------------------------------------------------------------------------------------------
HEAVY_P = 1030
HEAVY_UNITS = (1, 2, 4, 5, 63, 64, 65, 130)
MIXED_WAVE, ALL_HEAVY_WAVE = 2, 5


def heavy_spec():
    """-> (counts[P] of the ordinary Gaussians, {Gaussian: pop bytes}): Gaussians of 1 .. 130 units; wave 2 holds three heavy ones
    (1, 5 and 2 units: both ways of adding the unit sums) on lanes 0, 63 and 30 beside ordinary ones; all 64 of wave 5 are heavy;
    instance counts that are no multiples of 64; pop from 0 .. 4, pop[0] = 0 in every unit of every other heavy Gaussian"""
    rng = np.random.default_rng(21)
    P = HEAVY_P
    counts = rng.choice(RANDOM_COUNTS, P).astype(np.int64)
    units = {MIXED_WAVE * 64 + 0: 1, MIXED_WAVE * 64 + 63: 5, MIXED_WAVE * 64 + 30: 2, 8 * 64 + 10: 63, 9 * 64 + 63: 64, 10 * 64: 65, 12 * 64 + 33: 130,
             3 * 64 + 5: 4, 1029: 2}
    for lane in range(64):
        units[ALL_HEAVY_WAVE * 64 + lane] = {7: 4, 40: 5, 41: 9}.get(lane, 1)
    heavy = {}
    for n, (i, nu) in enumerate(sorted(units.items())):
        inst = (nu - 1) * UNIT + int(rng.integers(1, UNIT))
        if n % 7 == 3:
            inst = nu * UNIT
        pop = rng.integers(0, 5, inst).astype(np.uint8)
        if n % 2 == 0:
            pop[::UNIT] = 0
        heavy[i] = pop
        counts[i] = int(pop.sum())
    return counts, heavy


def heavy_layouts(fc):
    """-> (the heavy arrangement, the dense arrangement of the same rows)"""
    counts, heavy = heavy_spec()
    values = make_values(counts, 300)
    gaps = pattern_gaps(HEAVY_P)
    return arrange(f"heavy-fc{fc}", fc, values, heavy=heavy, gaps=gaps), arrange(f"heavy-as-dense-fc{fc}", fc, values, gaps=gaps)


# ---- the scene side --------------------------------------------------------------------------------------------------------------------


def visible_scene(P, seed=91):
    """P splats of 3 .. 40 pixels radius centred inside the image (preprocess_ref.opacity_case's construction, opacity 0.8): every
    Gaussian has a radius, so that a row pattern stays what it is"""
    W, H = E.IMAGES[9]
    cam, rng = R.camera(W, H), np.random.default_rng([seed, P])
    z = rng.uniform(1.0, 8.0, P)
    mean = R._place(cam, rng.uniform(2, W - 2, P), rng.uniform(2, H - 2, P), z)
    g = R._plain(P, rng, mean, R._round_scale(cam, mean, rng.integers(3, 41, P).astype(np.float64)))
    g["rotations"] = rng.normal(0, 1, (P, 4))
    g["rotations"] /= np.linalg.norm(g["rotations"], axis=1, keepdims=True)
    return R.make_case(f"visible-{P}", W, H, g)


def clamp_case(P=257):
    """layout_cases(P)'s scene with SH whose DC term puts colour channel c below zero exactly where bit c of (index % 8) is set
    (0.28 * -3 + 0.5 < 0 < 0.28 * 1 + 0.5, the higher bands within 0.05): all 8 combinations of the clamp bits"""
    c = dict(R.layout_cases(P)["aligned"])
    rng = np.random.default_rng(33)
    sh = rng.uniform(-0.05, 0.05, (P, 16, 3))
    bits = (np.arange(P)[:, None] >> np.arange(3)[None, :]) & 1
    sh[:, 0, :] = np.where(bits == 1, -3.0, 1.0)
    c["shs"], c["name"] = np.ascontiguousarray(sh, F32), f"clamp-{P}"
    return c


def scene_counts(P, vis, seed):
    """rows for the Gaussians of a scene: random counts, a few of them window-covering, for those with a radius; 0 for the others.
    -> (counts, {Gaussian: pop}) with up to three heavy Gaussians (1, 2 and 5 units) among the visible ones"""
    rng = np.random.default_rng([seed, P])
    counts = rng.choice(RANDOM_COUNTS + (150,), P).astype(np.int64)
    counts[~np.asarray(vis, bool)] = 0
    heavy = {}
    v = np.nonzero(vis)[0]
    if len(v) >= 8:
        for i, nu in zip(v[[1, len(v) // 2, len(v) - 1]], (1, 2, 5)):
            pop = rng.integers(0, 5, nu * UNIT - 7).astype(np.uint8)
            heavy[int(i)] = pop
            counts[i] = int(pop.sum())
    return counts, heavy


def scene_layout(c, vis, fc, seed=500):
    counts, heavy = scene_counts(c["P"], vis, seed)
    return arrange(f"{c['name']}-fc{fc}", fc, make_values(counts, seed + 1), heavy=heavy)


def rejected_calls():
    """-> what to change in the arguments of a good call (colour from SH, scales and rotations, rows with one heavy unit) for the
    hook to refuse it"""
    return (["P=0", "P=-1", "P=2^28", "W=0", "H=0", "fc=-1", "fc=11", "windows=1", "windows=4", "heavy_units=-2", "D=4", "M=9", "both:colors_precomp", "both:cov3D_precomp"]
            + [f"null:{k}" for k in ("means3D", "viewmatrix", "projmatrix", "radii", "shs", "scales", "rotations", "campos", "clamped", "sh_dir", "rows", "gauss_rows",
                                     "tiles_touched", "wave_rowbase", "hrec", "counters", "dL_dmeans2D", "dL_dopacities", "dL_dmeans3D", "dL_dscales", "dL_drots",
                                     "dL_dfeatures")]
            + [f"misaligned:{k}" for k in ("rows", "rotations", "dL_dmeans2D", "dL_dconics", "dL_drots", "sh_dir", "hrec")]
            + ["precomp:no-dL_dcolors", "precomp:no-dL_dcov3D", "rest:M=9", "rest:misaligned", "rest:dL-misaligned", "rest:only-dL_dshs", "rest:only-dL_dshs_rest",
               "packed:dL_dshs_rest"])
