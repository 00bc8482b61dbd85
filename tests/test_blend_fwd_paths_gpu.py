"""csrc/blend_fwd_q.hip alone (gs2m_debug_blend_forward), at the edges of its data paths: an entry's record quads are parked in
LDS a chunk of 16 entries ahead, the chunk's ids stay in a register of the wave, and a pixel's last contributor is kept as (slot
in the chunk, list index) and turned into a tile-list position by one gather at the end.  The cases also hold the edges of a
walk in sub-chunks of 2 or 4 entries whose channel quads are prefetched a sub-chunk ahead (built and measured, not kept:
profiles/blend_fwd_scalar_ab.md), so that a later attempt at it meets them.

The cases are built on tests/blend_ref.py (list builders, `settle`: THRESHOLD-FREE, float64 reference) and compared under the
rules of tests/test_blend_gpu.py (`check_forward`: n_contrib, qlast and observe equal, colour / buffer / final_T element-wise
within FACTOR x the fp32 restatement's error, zero exceptions, guard words intact).  The first half of the file runs WITHOUT a
GPU and asserts on the reference's output that every case has the structure it is there for.

Early stops.  A pixel finishes at the entry whose test_T falls below 1e-4; alpha is clamped to 0.99, so after entry 0 T >= 0.01
and after entry 1 T >= (1 - 0.99)^2, which IS the threshold: a stop at entry 0 does not exist and a stop at entry 1 is not
threshold-free (blend_ref._stop_case).  The earliest stop, entry 2, is the first entry of the second sub-chunk; entries 3 / 4 are
the last of a sub-chunk / the first of the next (for sub-chunks of 2 and of 4), 15 / 16 / 17 the last of a chunk and the first two
of the next.  A one-entry list (the lengths cases) is what remains of "finishes at entry 0".  Behind every stop the list goes
on with entries that all name the LARGEST id of the scene: a prefetch that ignores the stop reads the last record of the buffer.

`observe`.  Every list's first contributor sees T = 1, so "a list in which no entry has a pixel with T > 0.5" exists only as a
list without contributors (quadrant 3 of the tracking case).  The path behind it -- the wave stops watching once no live pixel
has T > 0.5, and later contributors are not observed -- is in every stop case (entry s - 1) and asserted there."""
import functools

import numpy as np
import pytest

import blend_ref as R

LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 48)  # per quadrant: sub-chunk and chunk tails for sub-chunks of 2 and 4
# 40 x 24: 3 x 2 tiles, the right column has quadrants 0 and 2 only, the lower row 0 and 1 only, the corner tile quadrant 0
FRAME_LENGTHS = [(0, 1, 2, 3), (4, 5, 15, 16), (17, 0, 31, 0), (32, 33, 0, 0), (48, 3, 0, 0), (5, 0, 0, 0)]
FCS = (1, 3, 5, 7, 9, 10)  # the four template instances, and a runtime fc below the template's (3 on FC 5, 7 on FC 9)
STOPS = (2, 3, 4, 15, 16, 17)
FAINT = (0.001, 0.002)  # opacities whose alpha stays below 1/255 by a factor 2: never a contributor


def _stop_case(name, seed, s, fc=9, tail=12):
    """quadrant 0: every pixel is finished by entry s (blend_ref._stop_case: entries s - 2 and s - 1 leave T ~ 1e-3 of what the
    fillers in front left, entry s is refused); behind it `tail` entries that all name the scene's largest id"""
    rng = np.random.default_rng(seed)
    geo, tl, opaque = [], [], []
    box = R.quad_box(0, 0, 1, 16, 16)
    for i in range(s + 1):
        if i >= s - 2:
            geo.append(R._big(box, 0.9 if i == s - 1 else 0.999))
            opaque.append(len(geo) - 1)
            tl.append((len(geo) - 1, 0x1))
        else:
            geo.append(R.draw_geo(rng, box, sig=(1.5, 3.0), op=(0.02, 0.08)))
            tl.append((len(geo) - 1, 0x1 | (int(rng.integers(0, 8)) << 1)))
    geo.append(R.draw_geo(rng, (0, 0, 16, 16), op=(0.1, 0.3)))
    tl += [(len(geo) - 1, 0xF)] * tail
    return R.assemble(name, 16, 16, fc, (0.3, 0.2, 0.9), geo, [tl], seed, opaque=opaque)


TRACK = dict(q0=(10, 9), q1=(40, 36), q2=(34, 31), q3=(5, None))  # quadrant: (list length, index of every pixel's last contributor)


def _track_case(name, seed, fc=9):
    """one tile, a list per quadrant, interleaved in the tile's span (positions in the span are not list indices):
    q0: a small opaque splat in front (T < 0.5 around its centre only), fillers, a flat splat over the quadrant at the end
    q1: the flat splat at index 36 (chunk 2), three faint entries behind it       q2: at index 31, the LAST slot of chunk 1
    q3: faint entries only -- no contributor at all, nothing observed"""
    rng = np.random.default_rng(seed)
    geo, opaque, per_q = [], [], []
    for q, (n, last) in enumerate(TRACK.values()):
        box = R.quad_box(0, q, 1, 16, 16)
        ids = []
        for i in range(n):
            if last is None or i > last:
                geo.append(R.draw_geo(rng, box, op=FAINT))
                opaque.append(len(geo) - 1)
            elif i == last:
                geo.append(R._big(box, 0.2))
                opaque.append(len(geo) - 1)
            elif q == 0 and i == 0:
                A, B, C = R.conic(2.0, 2.0, 0.0)
                geo.append([box[0] + 3.3, box[1] + 3.4, A, B, C, 0.9])
                opaque.append(len(geo) - 1)
            else:
                geo.append(R.draw_geo(rng, box, sig=(1.5, 3.0), op=(0.02, 0.06)))
            ids.append(len(geo) - 1)
        per_q.append(ids)
    tl = [(per_q[q][i], 1 << q) for i in range(max(map(len, per_q))) for q in range(4) if i < len(per_q[q])]
    c = R.assemble(name, 16, 16, fc, (0.2, 0.4, 0.6), geo, [tl], seed, opaque=opaque)
    c.per_q = per_q
    return c


BUILDERS = {f"frame_fc{f}": functools.partial(R._lengths_case, seed=1100 + f, lengths=FRAME_LENGTHS, W=40, H=24, fc=f) for f in FCS}
BUILDERS["full_tile"] = functools.partial(R._lengths_case, seed=1200, lengths=[(17, 31, 33, 48)], W=16, H=16, fc=9)
for _s in STOPS:
    BUILDERS[f"stop{_s}"] = functools.partial(_stop_case, seed=1300 + _s, s=_s)
BUILDERS["track"] = functools.partial(_track_case, seed=1400)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (settled case, float64 forward): computed once per process, shared by the CPU and the GPU tests, never modified"""
    c = R.settle(BUILDERS[name](name))
    return c, R.forward(c)


def _quad(c, q, t=0):
    return next(x for x in c.quads if x[0] == t and x[1] == q)


# ---- without a GPU: every case is threshold-free and has its structure ------------------------------------------------------
@pytest.mark.parametrize("name", list(BUILDERS))
def test_case_is_threshold_free(name):
    c, f64 = reference(name)
    chk = R.forward(c, margins=True)
    assert not chk["offenders"], sorted(chk["offenders"])
    for k, band in R.BANDS.items():
        assert chk["margin"][k] >= band, (name, k, chk["margin"][k])
    f32 = R.forward(c, np.float32)
    for k in ("n_contrib", "qlast", "observe"):
        assert np.array_equal(f64[k], f32[k]), (name, k)


@pytest.mark.parametrize("fc", FCS)
def test_frame_holds_every_list_length_and_partial_tiles(fc):
    c, f64 = reference(f"frame_fc{fc}")
    assert (c.W, c.H, c.tiles_x, c.tiles_y, c.fc) == (40, 24, 3, 2, fc)
    assert set(int(x) for x in c.qcount) >= set(LENGTHS)
    assert int(f64["qvalid"].sum()) == len(c.quads) == 5 * 3 and not f64["qvalid"].all(), "partial tiles on both edges"
    assert np.all(c.qcount[~f64["qvalid"]] == 0)
    assert np.all(f64["qlast"] + 2 >= c.qcount), "low opacities: every list is walked to its end"
    # positions in the tile's span are not list indices: n_contrib needs the gather
    t, q, box, base, ent, rows = _quad(c, 1, t=1)
    assert any(pos != i for i, (g, pos) in enumerate(ent))


def test_full_tile_structure():
    c, f64 = reference("full_tile")
    assert (c.W, c.H, c.tiles) == (16, 16, 1) and list(c.qcount) == [17, 31, 33, 48] and f64["qvalid"].all()


@pytest.mark.parametrize("s", STOPS)
def test_every_pixel_stops_at_entry_s_and_the_rest_names_the_largest_id(s):
    c, f64 = reference(f"stop{s}")
    t, q, box, base, ent, rows = _quad(c, 0)
    assert f64["qlast"][0] == s and np.all(f64["n_contrib"][:8, :8] == s) and np.all(f64["final_T"][:8, :8] < 2e-3)
    assert len(ent) == s + 1 + 12 and all(g == c.P - 1 for g, pos in ent[s + 1:]) and all(g < c.P - 1 for g, pos in ent[:s + 1])
    assert c.rec.shape == (c.P, R.REC_FLOATS), "the largest id's record is the last of the buffer"
    # entry s - 2 takes every pixel's T below 0.5: it is observed, and the entries behind that point (quadrant 0 only) are not --
    # entry s - 1 contributes to every pixel at T ~ 0.01, entry s is refused: the wave has stopped watching by then
    assert f64["observe"][ent[s - 2][0]] > 0 and f64["observe"][ent[s - 1][0]] == 0 and f64["observe"][ent[s][0]] == 0
    assert c.lists[0][s - 1][1] == c.lists[0][s][1] == 0x1


def test_stops_cover_the_sub_chunk_and_chunk_edges():
    assert {s % 2 for s in STOPS} == {0, 1} and {s % 4 for s in STOPS} >= {3, 0} and {15, 16} <= set(STOPS) and min(STOPS) == 2


def test_contributor_tracking_and_observe_structure():
    c, f64 = reference("track")
    for q, (n, last) in enumerate(TRACK.values()):
        t, _, box, base, ent, rows = _quad(c, q)
        nc = f64["n_contrib"][box[1]:box[3], box[0]:box[2]]
        assert len(ent) == n == c.qcount[q]
        if last is None:
            assert np.all(nc == 0) and f64["qlast"][q] == 0, "no contributor at all"
            assert all(f64["observe"][g] == 0 for g, pos in ent), "a list in which no entry sees a pixel with T > 0.5"
        else:
            assert np.all(nc == ent[last][1] + 1) and ent[last][1] != last and f64["qlast"][q] == last + 1
    assert TRACK["q0"][1] < 16 <= 2 * 16 <= TRACK["q1"][1] and TRACK["q2"][1] % 16 == 15, "chunk 0, a later chunk, the last slot of a chunk"
    # q0: behind the small opaque splat only some pixels still have T > 0.5 when the flat splat at the end arrives
    assert 0 < f64["observe"][c.per_q[0][9]] < 64 and f64["observe"][c.per_q[0][0]] == 64
    assert any(0 < f64["observe"][g] < 64 for g in c.per_q[0][1:9])


# ---- on the GPU -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BUILDERS))
def test_forward(name):
    import test_blend_gpu as G
    c, f64 = reference(name)
    G.check_forward(c, f64, G.gpu_forward(c))
