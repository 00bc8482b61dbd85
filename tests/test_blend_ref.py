"""tests/blend_ref.py, without a GPU: the restatement of the blend is pinned to the project's CPU oracle, every case the GPU
test runs is threshold-free (zero near-threshold pairs) and has the structure it is there for, and the fp32 restatement's
error against float64 -- the yardstick of tests/test_blend_gpu.py -- is measured and compared with the recorded figures."""
import os

import numpy as np
import pytest

import blend_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", list(R.BUILDERS))
def test_case_is_threshold_free_and_both_precisions_take_the_same_branches(name):
    c, f64, r64, f32, r32 = R.reference(name)
    chk = R.forward(c, margins=True)  # every pair once more, on the settled case
    assert not chk["offenders"], sorted(chk["offenders"])
    for k, band in R.BANDS.items():
        assert chk["margin"][k] >= band, (name, k, chk["margin"][k])
    for k in ("n_contrib", "qlast", "observe"):
        assert np.array_equal(f64[k], f32[k]), (name, k)
    u = c.used_rows
    assert np.all(np.isfinite(r64[u])) and np.all(np.isfinite(r32[u]))
    guards = np.setdiff1d(np.arange(c.n_rows), u)
    assert len(guards) >= len(u) + 16 and np.all(np.isnan(r64[guards]))
    assert len(np.unique(u)) == len(u) == sum(len(q[4]) for q in c.quads)


def test_restatement_reproduces_the_oracle(oracle_lib):
    """The oracle (oracle/gs2m_oracle.c) is fp32 per (pixel, entry) pair, in the reference's written order -- it is the SUMS over
    pixels that it accumulates in double.  So it is the fp32 restatement that has to reproduce it: images, final_T and n_contrib
    bit for bit, the per-Gaussian blend sums (fp32 addends added in double, rounded once) to the last fp32 bit -- the
    double sum's order may move the rounding by one ulp."""
    import ctypes
    import ctypes.util
    import helpers as Hh
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.expf.restype, libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
    expf = np.frompyfunc(lambda v: libm.expf(float(v)), 1, 1)  # the oracle's own exp: the C library's, not always correctly rounded
    exp = lambda p: expf(p).astype(np.float32)
    sc = Hh.scene_from_golden(np.load(os.path.join(GOLD, "raster_small.npz")))
    f, gr = Hh.run_oracle(oracle_lib, sc)
    W, H, fc, P = sc["W"], sc["H"], sc["fc"], f.P
    geo = np.concatenate([f.means2D, f.conic_opacity], axis=1)
    lists = [[(int(g), 0xF) for g in f.vals_sorted[a:b]] for a, b in f.ranges]
    c = R.assemble("oracle", W, H, fc, sc["bg"].numpy(), geo, lists, 1)
    c.chan = np.concatenate([f.rgb, sc["g"]["features"].numpy()], axis=1).astype(np.float32)
    c.grad_color, c.grad_buffer = sc["Gc"].numpy(), sc["Gb"].numpy()
    assert sum(len(t) for t in c.lists) == f.num_rendered > 0
    o = R.forward(c, np.float32, exp=exp)
    assert np.array_equal(o["n_contrib"], f.n_contrib)
    assert np.array_equal(o["final_T"], f.final_T)
    assert np.array_equal(o["color"], f.color)
    assert np.array_equal(o["buffer"][:fc], f.buffer[:fc])
    # every quadrant holds its tile's whole list, so a pixel's walk is the tile's: observe too
    assert np.array_equal(o["observe"], f.observe)
    _, terms = R.backward(c, dict(final_T=f.final_T, n_contrib=f.n_contrib, qlast=o["qlast"]), np.float32, exp=exp, keep_terms=True)
    sums, mags = np.zeros((P, R.ROW_FEAT + fc)), np.zeros((P, R.ROW_FEAT + fc))
    for g, t in terms.values():
        sums[g] += t.astype(np.float64).sum(0)
        mags[g] += np.abs(t.astype(np.float64)).sum(0)
    want = np.concatenate([gr["means2D"], gr["conics"][:, [0, 1, 3]], gr["opacities"].reshape(P, 1), gr["colors"], gr["features"][:, :fc]], axis=1)
    assert np.abs(want).max() > 0
    err = np.abs(sums.astype(np.float32).astype(np.float64) - want)
    assert np.all(err <= 2.0 ** -23 * np.abs(want) + 1e-12 * mags), f"{np.count_nonzero(err > 2.0 ** -23 * np.abs(want) + 1e-12 * mags)} sums differ, worst {err.max():.3e}"
    # and the float64 restatement is the same statement in another precision: it agrees with the oracle at fp32 rounding level
    o64 = R.forward(c)
    assert R.rel_err(o64["color"], f.color, np.abs(f.color).max()) < 1e-3 and R.rel_err(o64["final_T"], f.final_T, 1.0) < 1e-3


def test_measured_restatement_errors_are_the_recorded_ones():
    """the three figures of the issue (and the column norm-wise one) over the GPU cases, against the constants test_blend_gpu.py uses"""
    e = np.array([R.restatement_errors(n) for n in R.BUILDERS])
    short = np.array([n != "long" for n in R.BUILDERS])
    got = dict(E_IMAGE=e[:, 0].max(), E_FINAL_T=e[:, 1].max(), E_ROWS=e[short, 2].max(), E_ROWS_NORM=e[short, 3].max())
    print({k: f"{v:.3e}" for k, v in got.items()}, "long list alone:", [f"{v:.3e}" for v in e[~short][0]])
    for k, v in got.items():
        rec = getattr(R, k)
        assert rec / 2 <= v <= rec * 2, f"{k}: measured {v:.3e}, recorded {rec:.3e}"
    assert R.E_IMAGE < 2e-6 and R.E_FINAL_T < 1e-5 and R.E_ROWS_NORM < 4e-6, "rounding level: a few hundred fp32 operations"


def _quad(c, t, q):
    return next(x for x in c.quads if x[0] == t and x[1] == q)


def test_every_list_length_class_occurs():
    seen, chunks, groups = set(), set(), set()
    for k in range(4):
        c, f64 = R.reference(f"len{k}")[:2]
        assert np.all(f64["qlast"] + 2 >= c.qcount), "low opacities: every list is walked to its end"
        seen |= set(int(x) for x in c.qcount)
        chunks |= set((int(x) + 15) // 16 for x in c.qcount)
        groups |= set((int(x) + 15) // 16 for x in f64["qlast"])
    assert seen >= set(R.LENGTHS)
    assert chunks >= {0, 1, 2, 3, 4, 5, 7} and groups >= {0, 1, 2, 3, 4, 5, 7}
    # quadrant masks: positions in the tile's span have gaps, and n_contrib reports them (+ 1), not list positions
    c, f64 = R.reference("len1")[:2]
    t, q, box, base, ent, rows = _quad(c, 0, 0)
    assert any(pos != i for i, (g, pos) in enumerate(ent)) and ent[-1][1] + 1 > len(ent)
    assert f64["n_contrib"][box[1]:box[3], box[0]:box[2]].max() == ent[-1][1] + 1


@pytest.mark.parametrize("s", R.STOPS)
def test_every_pixel_stops_at_the_entry_it_is_meant_to(s):
    c, f64 = R.reference(f"stop{s}")[:2]
    assert c.qcount[0] == 40 and f64["qlast"][0] == s
    assert np.all(f64["n_contrib"][:8, :8] == s) and np.all(f64["final_T"][:8, :8] < 2e-3)


def test_partial_stop_and_spread_and_clamp_structure():
    c, f64 = R.reference("stop_some")[:2]
    nc = f64["n_contrib"][:8, :8]
    assert f64["qlast"][0] == 40 and np.count_nonzero(nc == 16) >= 2 and np.count_nonzero(nc > 32) >= 16
    c, f64 = R.reference("spread")[:2]
    nc = f64["n_contrib"][:8, :8]
    assert f64["qlast"][0] > 64 and nc[:, :2].max() <= 30 and nc[:, 6:].min() > 48, "n_contrib of one wave spread over > 2 groups"
    c = R.case("clamp")
    ys, xs = np.mgrid[0:16, 0:16]
    both = 0
    for g in range(c.P):
        oG = R._alpha(c, g, xs.ravel().astype(np.float64), ys.ravel().astype(np.float64), np.float64, np.exp)[4]
        both += bool((oG > 0.99 * 1.002).any() and ((oG < 0.99 * 0.9) & (oG > 0.1)).any())
    assert both >= 4


def test_edges_shared_and_many_tiles_structure():
    for (w, h) in R.EDGES:
        c, f64 = R.reference(f"edge{w}x{h}")[:2]
        n_valid = int(f64["qvalid"].sum())
        assert n_valid == len(c.quads) == ((w + 7) // 8) * ((h + 7) // 8)
        assert np.all(c.qcount[~f64["qvalid"]] == 0), "a quadrant without pixels has no entries"
    assert not R.reference("edge9x17")[1]["qvalid"].all() and R.case("edge23x16").tiles == 2 and R.case("edge17x33").tiles == 6
    c = R.case("shared")
    owners = {}
    for t, q, box, base, ent, rows in c.quads:
        for (g, pos), r in zip(ent, rows):
            owners.setdefault(g, set()).add(int(r))
    assert all(len(v) == 16 for v in owners.values()) and len(owners) == 30
    c = R.case("many_tiles")
    assert c.tiles == 40 and (c.ranges[:, 1] == c.ranges[:, 0]).any() and int(c.qcount.max()) > 64
    # (40 IS a multiple of 8; tile counts that are not -- 1, 2, 4, 6 -- are the other cases)
    assert {R.case(n).tiles for n in R.BUILDERS} >= {1, 2, 4, 6, 40}
    c = R.case("long")
    assert list(c.qcount) == [330, 0, 0, 0] and R.reference("long")[1]["qlast"][0] == 330
