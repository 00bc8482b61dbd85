"""The two one-workgroup-per-1024 prefix scans of csrc/binning.hip on caller-made counts (gs2m_debug_block_scans): blockscan_kernel
(block instance counts and block heavy-unit counts, 8 x 1024 elements in front per round) and rowscan_kernel (wave row counts,
16 x 1024 per round) at the lengths where a workgroup starts a further round -- lengths a frame reaches only beyond 2 M
Gaussians -- against numpy's cumsum in uint64.  Integer work: every comparison is array_equal."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
PATTERN = np.uint32(0xA5C3F00D)
SATURATED = 0xFFFFFFFE


def _common_h(name):
    txt = open(os.path.join(ROOT, "gs-2m_amd", "csrc", "common.h")).read()
    return int(re.search(r"^#define\s+" + name + r"\s+(\d+)u?\s*$", txt, flags=re.M).group(1))


UNIT = _common_h("GS2M_UNIT")
CNT_ROWS, CNT_HUNITS, CNT_SPAN_MID, CNT_SPAN_LONG = (_common_h("GS2M_CNT_" + n) for n in ("ROWS", "HUNITS", "SPAN_MID", "SPAN_LONG"))
LAND_R, LAND_HUNITS, LAND_PREFILTERED, LAND_ROWS = (_common_h("GS2M_LAND_" + n) for n in ("R", "HUNITS", "PREFILTERED", "ROWS"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).reshape(-1).copy()).cuda()


class Guarded:
    """`words` pattern words with GUARD pattern words in front and behind"""

    def __init__(self, words):
        self.words, self.t = words, _dev(np.full(words + 2 * GUARD, PATTERN, np.uint32))
        self.ptr = self.t.data_ptr() + 4 * GUARD

    def inside(self):
        return self.t[GUARD:GUARD + self.words].cpu().numpy().view(np.uint32)

    def guards_intact(self):
        g = self.t.cpu().numpy().view(np.uint32)
        return bool(np.all(g[:GUARD] == PATTERN) and np.all(g[GUARD + self.words:] == PATTERN))


def _exclusive(counts):
    incl = np.cumsum(counts.astype(np.uint64), dtype=np.uint64)
    return incl - counts.astype(np.uint64), int(incl[-1])


def run_scans(block_tt, block_hu, wave_rows):
    """-> nothing; asserts every output word.  The arrays hold 32-bit words: a prefix is compared modulo 2^32 (it only differs from
    the exact one where the total does not fit, which the published, saturated total tells the host)."""
    import gs2m_native
    nb, nw = len(block_tt), len(wave_rows)
    t_tt, t_hu, t_wr = _dev(block_tt), _dev(block_hu), _dev(wave_rows)
    inputs0 = [t.clone() for t in (t_tt, t_hu, t_wr)]
    pref, hupref, rowbase, counters, landing = Guarded(nb), Guarded(nb), Guarded(nw), Guarded(64), Guarded(4)
    gs2m_native.launch("gs2m_debug_block_scans", torch.device("cuda", torch.cuda.current_device()), nb, t_tt.data_ptr(), t_hu.data_ptr(), pref.ptr,
                       hupref.ptr, nw, t_wr.data_ptr(), rowbase.ptr, counters.ptr, landing.ptr)
    torch.cuda.synchronize()
    for t, t0 in zip((t_tt, t_hu, t_wr), inputs0):
        assert torch.equal(t, t0), "an input was written"
    for name, g in (("block_pref", pref), ("block_hupref", hupref), ("wave_rowbase", rowbase), ("counters", counters), ("landing", landing)):
        assert g.guards_intact(), f"guard words of {name} were written"

    def same(name, got, want64):
        want = (want64 & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (f"{name}, {len(got)} words: {bad.size} differ, the first at {bad[0]} (workgroup {bad[0] // 1024}): "
                               f"{int(got[bad[0]])}, expected {int(want[bad[0]])}")

    e_tt, R = _exclusive(block_tt)
    e_hu, U = _exclusive(block_hu)
    e_wr, rows = _exclusive(wave_rows)
    same("block_pref", pref.inside(), e_tt)
    same("block_hupref", hupref.inside(), e_hu)
    R32, U32 = min(R, SATURATED), min(U, SATURATED)
    heavy_rows = (4 * UNIT * U32) & 0xFFFFFFFF   # the heavy units' rows come first, 4 x GS2M_UNIT each
    same("wave_rowbase", rowbase.inside(), e_wr + np.uint64(heavy_rows))
    rows32 = (heavy_rows + rows) & 0xFFFFFFFF
    want_c = np.full(64, PATTERN, np.uint32)
    want_c[1], want_c[CNT_HUNITS], want_c[CNT_ROWS], want_c[CNT_SPAN_MID], want_c[CNT_SPAN_LONG] = R32, U32, rows32, 0, 0
    got_c = counters.inside()
    assert np.array_equal(got_c, want_c), f"counters: words {np.nonzero(got_c != want_c)[0]} are {got_c[got_c != want_c]}, expected {want_c[got_c != want_c]}"
    want_l = np.full(4, PATTERN, np.uint32)
    want_l[LAND_R], want_l[LAND_HUNITS], want_l[LAND_ROWS] = R32, U32, (rows32 + 1) & 0xFFFFFFFF
    got_l = landing.inside()
    assert (LAND_R, LAND_HUNITS) == (0, 1), "{num_rendered, heavy units} are one 8-byte word"
    assert int(got_l[:2].view(np.uint64)[0]) == R32 | (U32 << 32), f"landing: the packed {{R, units}} is {int(got_l[:2].view(np.uint64)[0]):#x}, expected {R32 | (U32 << 32):#x}"
    assert np.array_equal(got_l, want_l), f"landing: {got_l}, expected {want_l}"


def _counts(rng, n, usual, large, n_large):
    """random counts below `usual`, a third of them zero, `n_large` of them `large`"""
    c = rng.integers(0, usual, n, dtype=np.uint64).astype(np.uint32)
    c[rng.random(n) < 1.0 / 3.0] = 0
    c[rng.integers(0, n, min(n_large, n))] = large
    return c


def _frame_like(rng, n_blocks, n_waves):
    # totals that fit: instances < 67 585 x 2000 + 8 x 2^26 < 2^30; units < 67 585 x 4 + 8 x 1000, their rows (x 256) < 2^27;
    # rows < 66 567 x 3000 + 8 x 2^24 < 2^29
    return _counts(rng, n_blocks, 2000, 1 << 26, 8), _counts(rng, n_blocks, 4, 1000, 8), _counts(rng, n_waves, 3000, 1 << 24, 8)


# a workgroup owns 1024 elements and reads what lies in front of them in rounds of 8 x 1024 (block counts) or 16 x 1024 (wave
# rows): one workgroup, one full, one element into the second; the last workgroup that needs one round, the first that needs two,
# three rounds; beyond 64 workgroups
N_BLOCKS = [1, 2, 1023, 1024, 1025, 8 * 1024 + 1024, 8 * 1024 + 1025, 16 * 1024 + 1025, 65536 + 1024 + 1]
N_WAVES = [1, 1024, 1025, 16 * 1024 + 1024, 16 * 1024 + 1025, 65536 + 1024 + 7]


@pytest.mark.parametrize("n_blocks", N_BLOCKS)
def test_block_prefixes_at_every_round_edge(n_blocks):
    rng = np.random.default_rng(n_blocks)
    run_scans(*_frame_like(rng, n_blocks, N_WAVES[N_BLOCKS.index(n_blocks) % len(N_WAVES)]))


@pytest.mark.parametrize("n_waves", N_WAVES)
def test_wave_row_bases_at_every_round_edge(n_waves):
    rng = np.random.default_rng(7 + n_waves)
    run_scans(*_frame_like(rng, N_BLOCKS[(N_WAVES.index(n_waves) + 4) % len(N_BLOCKS)], n_waves))


def test_all_zero_counts():
    z = np.zeros(8 * 1024 + 1025, np.uint32)
    run_scans(z, z, np.zeros(16 * 1024 + 1025, np.uint32))


@pytest.mark.parametrize("which", ["instances", "units", "both"])
def test_totals_beyond_32_bits_are_published_saturated(which):
    """a sum beyond 2^32 - 2 leaves as 0xFFFFFFFE, not wrapped, so that it cannot pass the caller's range check; the sum is reached
    in the second round of the last workgroups, i.e. in the 64-bit part of the scan"""
    rng = np.random.default_rng(99)
    n_blocks, n_waves = 8 * 1024 + 1025, 1025
    tt, hu, wr = _frame_like(rng, n_blocks, n_waves)
    big = rng.integers(1 << 19, 1 << 20, n_blocks, dtype=np.uint64).astype(np.uint32)   # 9217 x ~786 000 = 7.2e9 > 2^32
    if which in ("instances", "both"):
        tt = big
    if which in ("units", "both"):
        hu = big[::-1].copy()
    assert (int(tt.sum(dtype=np.uint64)) > 0xFFFFFFFF) == (which != "units") and (int(hu.sum(dtype=np.uint64)) > 0xFFFFFFFF) == (which != "instances")
    run_scans(tt, hu, wr)
