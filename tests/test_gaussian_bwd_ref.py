"""tests/gaussian_bwd_ref.py alone (no GPU): the layout builder against a plain re-reading of what it built, the exactness condition,
and every row and heavy pattern of tests/test_gaussian_bwd_gpu.py shown to contain what its name says."""
import numpy as np
import pytest

import gaussian_bwd_ref as B
import preprocess_ref as R

NAN_BITS = np.array([np.nan], np.float32).view(np.uint32)[0]


def _read_back(L):
    """the sums of a layout re-read from its arrays as the kernels address them (float64 of the stored floats), and the mask of the
    buffer's elements that were read"""
    body = L.rows[B.GUARD_ROWS:]
    nch = 11 + L.fc
    read = np.zeros(L.rows.shape, bool)
    out = np.zeros((L.P, nch))
    for i in range(L.P):
        gr = int(L.gauss_rows[i])
        if gr & B.ROWS_BIG:
            u0, nu = gr & ~B.ROWS_BIG, (int(L.tiles_touched[i]) + 63) // 64
            for u in range(u0, u0 + nu):
                pop = L.hrec[u, 16:].astype(np.int64)
                assert L.hrec[u, :4].view(np.uint32)[0] == i
                for k in range(64):
                    r = 256 * u + 4 * k
                    out[i] += body[r:r + pop[k], :nch].astype(np.float64).sum(0)
                    read[B.GUARD_ROWS + r:B.GUARD_ROWS + r + pop[k], :nch] = True
        else:
            w = i // 64
            r = int(L.wave_rowbase[w]) + int(sum(int(x) for x in L.gauss_rows[w * 64:i] if not x & B.ROWS_BIG))
            out[i] = body[r:r + gr, :nch].astype(np.float64).sum(0)
            read[B.GUARD_ROWS + r:B.GUARD_ROWS + r + gr, :nch] = True
    return out, read


def _check_layout(L):
    out, read = _read_back(L)
    assert np.array_equal(out, L.sums * B.STEP)
    bits = L.rows.view(np.uint32)
    assert np.all(bits[~read] == NAN_BITS), "something the kernel must not read is not NaN"
    assert np.all(np.isfinite(L.rows[read])) and not np.any(np.signbit(L.rows[read]) & (L.rows[read] == 0)), "a written element is NaN or -0"
    k = L.rows[read].astype(np.float64) / B.STEP
    assert np.array_equal(k, np.round(k)) and np.abs(k).max(initial=0) <= B.KMAX
    assert not read[:B.GUARD_ROWS].any() and not read[-B.GUARD_ROWS:].any() and not read[:, 11 + L.fc:].any()
    assert L.counters[B.CNT_HUNITS] == L.units and L.counters[B.CNT_ROWS] == L.n_rows == len(L.rows) - 2 * B.GUARD_ROWS
    e = L.expected
    assert np.array_equal(e["means2D"], (L.sums[:, :4] * B.STEP).astype(np.float32)) and not e["conics"][:, 2].view(np.uint32).any()
    assert not e["features"][:, L.fc:].view(np.uint32).any()
    return read


def test_row_floats():
    assert [B.row_floats(fc) for fc in range(11)] == [12, 12, 16, 16, 16, 16, 20, 20, 20, 20, 24]
    assert {fc: 64 // (B.row_floats(fc) // 4) for fc in B.FCS} == B.GROUPS


def test_exactness_condition_is_enforced():
    """20 000 rows of one Gaussian stay at 1.3 M; 2^24 / 64 rows of |k| = 64 do not"""
    B.arrange("ok", 0, [np.full((20000, 21), 64)])
    with pytest.raises(AssertionError):
        B.arrange("too many", 0, [np.full((2 ** 18, 21), 64)])
    with pytest.raises(AssertionError):
        B.arrange("too large", 0, [np.full((1, 21), 65)])


@pytest.mark.parametrize("which,P", [(w, P) for w in "AB" for P in B.PATTERN_SIZES[w]])
def test_pattern_layouts_read_back(which, P):
    for fc in (0, 10):
        L = B.pattern_layout(which, P, fc)
        assert L.P == P and L.units == 0
        read = _check_layout(L)
        gaps = B.pattern_gaps(P)
        assert gaps.max() > 0 and (~read[B.GUARD_ROWS:-B.GUARD_ROWS].any(1)).sum() == gaps.sum(), "the gaps between the waves' runs"
    assert sorted(P % 256 for w in "AB" for P in B.PATTERN_SIZES[w]) == [0, 1, 3, 255]


def test_pattern_set_A():
    w = dict(B.pattern_waves("A"))
    names = [n for n, _ in B.pattern_waves("A")]
    assert [B.wave_total(w[f"total-{t}"]) for t in B.WAVE_TOTALS] == list(B.WAVE_TOTALS)
    nwin = [B.n_windows(w[f"total-{t}"]) for t in B.WAVE_TOTALS]
    assert set(nwin) == {0, 1, 2, 3, 4, 5} and {n % 2 for n in nwin} == {0, 1} and {n % 3 for n in nwin} == {0, 1, 2}
    k = names.index("total-0")
    assert B.wave_total(w[names[k - 1]]) > 0 and B.wave_total(w[names[k + 1]]) > 0, "the empty wave stands between two busy ones"
    r = w["random"]
    assert r[0] > 0 and r[63] > 0 and set(r) <= set(B.RANDOM_COUNTS) and (r == 0).any() and (r == 40).any()
    for n, end in ((64, False), (128, False), (192, False), (320, True)):
        c = w[f"aligned-{n}" + ("-end" if end else "")]
        (j, ex, cn, w0, nw), = [x for x in B.covers(c) if x[0] == B.ALIGNED_AT]
        assert cn == n and ex % 64 == 0 and ex > 0 and nw == n // 64
        assert c[j - 1] == 0 and (end or c[j + 1] == 0) and all(c[j - G] == 0 for G in B.GROUPS.values())
        assert (c[j + 1:].sum() == 0 and w0 + nw == B.n_windows(c)) if end else c[j + 1:].sum() > 0
    assert B.pattern_counts("A", 1025)[1024] > 0, "a last wave of one Gaussian with rows"


def test_pattern_set_B():
    w = dict(B.pattern_waves("B"))

    def mids(c):   # start mid-window, cover at least two whole windows
        return [x for x in B.covers(c) if x[1] % 64 != 0 and x[4] >= 2]
    (m,) = mids(w["mid"])
    assert (m[1] + m[2]) % 64 != 0
    a, b = mids(w["mid-two-groups"])
    assert all((a[0] % G) != (b[0] % G) for G in B.GROUPS.values()) and (a[1] + a[2]) % 64 != 0 and (b[1] + b[2]) % 64 != 0
    for G in B.GROUPS.values():
        a, b = mids(w[f"mid-same-group-{G}"])
        assert b[0] == a[0] + G and a[0] < G
    a, b = B.covers(w["back-to-back"])
    assert b[0] == a[0] + 1 and a[1] % 64 != 0 and (a[1] + a[2]) % 64 == 0 and b[1] == a[1] + a[2] and a[4] >= 2 and b[4] >= 2
    assert B.wave_total(w["zero"]) == 0 and B.n_windows(w["all-40"]) == 40 and not B.covers(w["all-40"])
    assert B.covers(w["lane-63-only"]) == [(63, 0, 130, 0, 2)] and B.covers(w["lane-0-only"]) == [(0, 0, 256, 0, 4)]


def test_heavy_patterns():
    counts, heavy = B.heavy_spec()
    units = {i: (len(p) + 63) // 64 for i, p in heavy.items()}
    assert set(B.HEAVY_UNITS) <= set(units.values()), "Gaussians of 1, 2, 4, 5, 63, 64, 65 and 130 units"
    assert sum(len(p) % 64 != 0 for p in heavy.values()) > 10 and any(len(p) % 64 == 0 for p in heavy.values())
    assert any(p[len(p) // 64 * 64:].size and (len(p) % 64) for p in heavy.values())
    assert sum(not p[::64].any() for p in heavy.values()) > 5, "units whose first instance has no row"
    assert {int(v) for p in heavy.values() for v in np.unique(p)} == {0, 1, 2, 3, 4}
    mixed = [i for i in heavy if i // 64 == B.MIXED_WAVE]
    assert sorted(i % 64 for i in mixed) == [0, 30, 63] and min(units[i] for i in mixed) <= 4 < max(units[i] for i in mixed)
    assert (counts[B.MIXED_WAVE * 64:B.MIXED_WAVE * 64 + 64] > 0).sum() > 20
    allh = [i for i in heavy if i // 64 == B.ALL_HEAVY_WAVE]
    assert len(allh) == 64 and min(units[i] for i in allh) <= 4 < max(units[i] for i in allh)
    assert max(int(p.sum()) for p in heavy.values()) * B.KMAX < 2 ** 24
    for fc in (0, 10):
        H, Dn = B.heavy_layouts(fc)
        _check_layout(H)
        _check_layout(Dn)
        assert np.array_equal(H.sums, Dn.sums) and H.units == sum(units.values()) and Dn.units == 0
        assert all(np.array_equal(H.expected[k].view(np.uint32), Dn.expected[k].view(np.uint32)) for k in H.expected)
        first = H.rows[B.unit_sum_rows(H), 0].view(np.uint32)
        assert (first == NAN_BITS).sum() > 20, "unit sums that land on a row nobody wrote"


def test_scene_cases(oracle_lib):
    """the row patterns' scene: every Gaussian has a radius; the clamp case: all 8 combinations of the clamp bits among the Gaussians
    with a radius; the degenerate case holds centres beyond the 1.3 tan(fov) clamp with a radius; rows go to Gaussians with a radius"""
    for P in (1023, 1024, 1025, 1027, B.HEAVY_P):
        assert np.all(R.oracle_forward(oracle_lib, B.visible_scene(P)).radii > 0)
    c = B.clamp_case()
    f = R.oracle_forward(oracle_lib, c)
    assert set(R.clamp_bits(f.clamped)[f.radii > 0]) == set(range(8))
    c = R.degenerate_case()
    f = R.oracle_forward(oracle_lib, c)
    t = np.abs(c["means3D"][:, :2] / c["means3D"][:, 2:3]) / np.array([[c["cam"]["tanfovx"], c["cam"]["tanfovy"]]], np.float32)
    assert ((t > 1.3).any(1) & (f.radii > 0)).sum() > 20
    L = B.scene_layout(c, f.radii > 0, 10)
    _check_layout(L)
    assert not L.sums[f.radii <= 0].any() and len(L.heavy) == 3 and (L.gauss_rows[f.radii > 0] > 0).any()


def test_rejected_calls_are_distinct():
    r = B.rejected_calls()
    assert len(set(r)) == len(r)
