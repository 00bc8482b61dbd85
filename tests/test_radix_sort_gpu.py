"""csrc/radix_sort.hip on caller-made pairs (gs2m_debug_radix_sort): every pass width, the look-back's group and window edges,
ticket and blockIdx tile ids, every argument combination and the tile ranges, against numpy's stable argsort of the masked keys.
Integer work: every comparison is array_equal.  The test owns every buffer: 4096 guard words on either side of each must stay as
they were, the inputs must not change, and a scratch the sort zeroes itself starts out full of a nonzero pattern."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096                      # words on either side of every buffer the sort may write
PATTERN = np.uint32(0xA5C3F00D)   # guard words and a scratch that is not pre-zeroed
TILE = 4096                       # keys per workgroup (RS_TILE)
ERR_INVALID_ARG = -1


def _common_h(name):
    txt = open(os.path.join(ROOT, "gs-2m_amd", "csrc", "common.h")).read()
    return int(re.search(r"^#define\s+" + name + r"\s+(\d+)\s*$", txt, flags=re.M).group(1))


HIST_COPIES, HIST_COPY_WORDS = _common_h("GS2M_HIST_COPIES"), _common_h("GS2M_HIST_COPY_WORDS")


@pytest.fixture(autouse=True)
def tickets():
    """tile ids from blockIdx where the size rule allows it (the default) unless a test switches the tickets on; switched back
    whatever the test does"""
    import gs2m_native
    gs2m_native.set_sort_tickets(False)
    yield gs2m_native.set_sort_tickets
    gs2m_native.set_sort_tickets(False)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).reshape(-1).copy()).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


class Guarded:
    """`words` words with GUARD pattern words in front and behind; the inside starts as `fill` (an array or one value)"""

    def __init__(self, words, fill=PATTERN):
        a = np.full(words + 2 * GUARD, PATTERN, np.uint32)
        a[GUARD:GUARD + words] = fill
        self.words, self.t = words, _dev(a)
        self.before = self.t.clone()
        self.ptr = self.t.data_ptr() + 4 * GUARD

    def inside(self):
        return _host(self.t[GUARD:GUARD + self.words])

    def guards_intact(self):
        return bool(torch.equal(self.t[:GUARD], self.before[:GUARD]) and torch.equal(self.t[GUARD + self.words:], self.before[GUARD + self.words:]))

    def untouched(self):
        return bool(torch.equal(self.t, self.before))


def plan(total_bits):
    import gs2m_native
    npass, bits, shift = C.c_int(0), (C.c_int * 4)(), (C.c_int * 4)()
    gs2m_native.check(gs2m_native.lib().gs2m_debug_radix_plan(total_bits, C.byref(npass), bits, shift), "gs2m_debug_radix_plan")
    return npass.value, list(bits)[:npass.value], list(shift)[:npass.value]


def temp_bytes(n, total_bits):
    import gs2m_native
    b = C.c_ulonglong(0)
    gs2m_native.check(gs2m_native.lib().gs2m_debug_radix_temp_bytes(n, total_bits, C.byref(b)), "gs2m_debug_radix_temp_bytes")
    return b.value


def split_hist(keys, total_bits, rng):
    """the digit counts of every pass of the plan, each bin's count split at random over the copies emit_kernel spreads its atomics
    over: copy c at word c * HIST_COPY_WORDS, pass p of it at word 256 p"""
    npass, bits, shift = plan(total_bits)
    h = np.zeros((HIST_COPIES, HIST_COPY_WORDS), np.uint32)
    for p in range(npass):
        digit = (keys >> np.uint32(shift[p])) & np.uint32((1 << bits[p]) - 1)
        counts = np.bincount(digit, minlength=256)
        h[:, 256 * p:256 * p + 256] = rng.multinomial(counts, [1.0 / HIST_COPIES] * HIST_COPIES).T
    assert np.array_equal(h.sum(axis=0, dtype=np.uint64)[:256 * npass].reshape(npass, 256).sum(axis=1), np.full(npass, len(keys)))
    return h


def expected(keys, vals, total_bits):
    mask = np.uint32((1 << total_bits) - 1)
    order = np.argsort(keys & mask, kind="stable")
    return keys[order], (order.astype(np.uint32) if vals is None else vals[order])


def expected_ranges(sorted_keys, total_bits):
    table = np.zeros(2 << total_bits, np.uint32)
    present = np.unique(sorted_keys)
    table[2 * present] = ~np.searchsorted(sorted_keys, present, side="left").astype(np.uint32)
    table[2 * present + 1] = np.searchsorted(sorted_keys, present, side="right").astype(np.uint32)
    return table


def run_sort(keys, vals, total_bits, *, prezeroed=False, with_ranges=False, ext_hist=None, scratch_bytes=None, expect_rc=0):
    """one call of the hook with every check that holds for every case; -> (sorted keys, sorted values, range table or None)"""
    import gs2m_native
    n = len(keys)
    t_kin = _dev(keys)
    t_vin = None if vals is None else _dev(vals)
    kin0, vin0 = t_kin.clone(), (None if t_vin is None else t_vin.clone())
    kA, vA, kB, vB = (Guarded(n) for _ in range(4))
    rr = Guarded(2 << total_bits, 0) if with_ranges else None
    need = temp_bytes(n, total_bits)
    assert need % 4 == 0
    have = need if scratch_bytes is None else scratch_bytes
    temp = Guarded(max(have, 4) // 4, 0 if prezeroed else PATTERN)
    t_hist = None if ext_hist is None else _dev(ext_hist)
    hist0 = None if t_hist is None else t_hist.clone()
    rc = gs2m_native.lib().gs2m_debug_radix_sort(n, total_bits, t_kin.data_ptr() if n else None,
                                                 None if t_vin is None or n == 0 else t_vin.data_ptr(), kA.ptr, vA.ptr, kB.ptr, vB.ptr,
                                                 temp.ptr, have, int(prezeroed), None if rr is None else rr.ptr,
                                                 None if t_hist is None else t_hist.data_ptr(), gs2m_native.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect_rc, rc
    assert torch.equal(t_kin, kin0), "kin was written"
    assert t_vin is None or torch.equal(t_vin, vin0), "vin was written"
    assert t_hist is None or torch.equal(t_hist, hist0), "ext_hist was written"
    for name, g in (("kA", kA), ("vA", vA), ("kB", kB), ("vB", vB), ("range_raw", rr), ("temp", temp)):
        assert g is None or g.guards_intact(), f"guard words of {name} were written"
    if expect_rc != 0 or n == 0:
        for name, g in (("kA", kA), ("vA", vA), ("kB", kB), ("vB", vB), ("range_raw", rr), ("temp", temp)):
            assert g is None or g.untouched(), f"{name} was written by a call that must not launch anything"
        return None
    return kB.inside(), vB.inside(), (None if rr is None else rr.inside())


def check_sort(keys, vals, total_bits, **kw):
    ek, ev = expected(keys, vals, total_bits)
    k, v, r = run_sort(keys, vals, total_bits, **kw)
    bad = np.nonzero((k != ek) | (v != ev))[0]
    assert bad.size == 0, (f"n {len(keys)}, {total_bits} bits, plan {plan(total_bits)}: {bad.size} pairs differ, the first at position {bad[0]} "
                           f"(tile {bad[0] // TILE}, group {bad[0] // (32 * TILE)}): key {int(k[bad[0]]):#x} value {int(v[bad[0]])}, expected {int(ek[bad[0]]):#x} {int(ev[bad[0]])}")
    if r is not None:
        er = expected_ranges(ek, total_bits)
        badr = np.nonzero(r != er)[0]
        assert badr.size == 0, f"n {len(keys)}, {total_bits} bits: range word {badr[0]} (key {badr[0] // 2}) is {int(r[badr[0]]):#x}, expected {int(er[badr[0]]):#x}"
    return k, v, r


def random_keys(rng, n, total_bits, garbage=True):
    """uniform in the sorted bits; half of the keys carry random bits above them (bit 31 included), which the sort must ignore"""
    mask = np.uint32((1 << total_bits) - 1)
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    clean = ~(rng.random(n) < 0.5) if garbage else np.ones(n, bool)
    keys[clean] &= mask
    return keys


def random_vals(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def test_every_total_bits_runs_every_pass_width():
    """total_bits 1 .. 32 at three tiles, the last partial; the plans read back through the hook must between them hold every pass
    width 0 .. 8 (make_plan: two passes up to 16 bits, four beyond; total_bits 1 has the pass of 0 bits, whose keys here carry
    bit 31 and everything else above bit 0)"""
    rng = np.random.default_rng(100)
    n = 10000
    widths = set()
    for total_bits in range(1, 33):
        npass, bits, shift = plan(total_bits)
        assert npass == (2 if total_bits <= 16 else 4) and sum(bits) == total_bits, (total_bits, bits)
        assert shift == [sum(bits[:k]) for k in range(npass)] and all(0 <= b <= 8 for b in bits), (total_bits, bits, shift)
        widths.update(bits)
        keys = random_keys(rng, n, total_bits)
        if total_bits < 32:
            assert (keys >> np.uint32(31)).any() and (keys >> np.uint32(total_bits)).any()
        check_sort(keys, random_vals(rng, n), total_bits)
    assert widths == set(range(9)), sorted(widths)


SIZE_EDGES = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 32 * TILE - 1, 32 * TILE, 32 * TILE + 1, 64 * TILE + 5]


@pytest.mark.parametrize("forced_tickets", [False, True], ids=["by-size", "tickets"])
@pytest.mark.parametrize("total_bits", [13, 32])
@pytest.mark.parametrize("n", SIZE_EDGES)
def test_size_edges(n, total_bits, forced_tickets, tickets):
    """one key .. one tile .. the group of 32 tiles and one tile more .. three groups, with tile ids from blockIdx and from tickets"""
    tickets(forced_tickets)
    rng = np.random.default_rng(1000 + n + total_bits)
    check_sort(random_keys(rng, n, total_bits), random_vals(rng, n), total_bits)


@pytest.mark.parametrize("forced_tickets", [False, True], ids=["by-size", "tickets"])
@pytest.mark.parametrize("total_bits", [13, 32])
def test_no_keys_is_a_success_that_touches_nothing(total_bits, forced_tickets, tickets):
    tickets(forced_tickets)
    assert run_sort(np.zeros(0, np.uint32), np.zeros(0, np.uint32), total_bits) is None


@pytest.mark.parametrize("total_bits", [13, 32])
@pytest.mark.parametrize("n", [545 * TILE + 17, 1057 * TILE + 3], ids=["18-groups", "34-groups-tickets-by-size"])
def test_second_round_trip_of_the_group_look_back(n, total_bits):
    """18 groups of 32 tiles: the last groups read the group prefixes in two windows of 16; 1057 tiles: more than four workgroups
    per compute unit of a whole MI355X, so the size rule hands out tickets"""
    rng = np.random.default_rng(n + total_bits)
    check_sort(random_keys(rng, n, total_bits), random_vals(rng, n), total_bits)


def _distributions(rng, n, total_bits):
    """{name: keys below 2^total_bits}; the tie-heavy ones prove stability and make runs of one key span many workgroup tiles"""
    mask = (1 << total_bits) - 1
    npass, bits, shift = plan(total_bits)
    top = max(p for p in range(npass) if bits[p] > 0)
    u = lambda hi: rng.integers(0, hi, n, dtype=np.uint64).astype(np.uint32)
    a, b = 0x5A5A5A5A & mask, 0x2DB6DB6D & mask
    heavy = u(mask + 1)
    for lo, hi in ((0.0, 0.3), (0.35, 0.65), (0.7, 1.0)):  # 90 % of the keys, in three runs of 14 tiles and more at n = 200 000
        heavy[int(lo * n):int(hi * n)] = a
    srt = np.sort(u(mask + 1))
    return {
        "equal": np.full(n, a, np.uint32),
        "two-values": np.where(rng.random(n) < 0.5, np.uint32(a), np.uint32(b)),
        "sorted": srt,
        "reversed": srt[::-1].copy(),
        "uniform": u(mask + 1),
        "one-value-90-percent": heavy,
        "top-digit-only": (u(1 << bits[top]) << np.uint32(shift[top])) | np.uint32(a & ((1 << shift[top]) - 1)),
        "bottom-digit-only": u(1 << bits[0]) | np.uint32(a & (mask ^ ((1 << bits[0]) - 1))),
    }


DIST_NAMES = ["equal", "two-values", "sorted", "reversed", "uniform", "one-value-90-percent", "top-digit-only", "bottom-digit-only"]


@pytest.mark.parametrize("total_bits", [1, 6, 13, 16, 17, 32])
def test_key_distributions(total_bits):
    """n = 200 000 (49 tiles, two groups); half of the keys carry random bits above the sorted ones, so equal sorted bits are told
    apart in the keys as well as in the values"""
    n = 200000
    rng = np.random.default_rng(7000 + total_bits)
    dists = _distributions(rng, n, total_bits)
    assert sorted(dists) == sorted(DIST_NAMES)
    for name in DIST_NAMES:
        keys = dists[name]
        assert keys.max() <= (1 << total_bits) - 1, name
        if total_bits < 32:
            keys = keys | (random_vals(rng, n) & np.uint32(~((1 << total_bits) - 1) & 0xFFFFFFFF) & np.where(rng.random(n) < 0.5, np.uint32(0xFFFFFFFF), np.uint32(0)))
        try:
            check_sort(keys, random_vals(rng, n), total_bits)
        except AssertionError as e:
            raise AssertionError(f"distribution {name}: {e}") from None


@pytest.mark.parametrize("n", [1, 4097, 200000])
@pytest.mark.parametrize("total_bits", [1, 5, 13])
def test_tile_ranges(total_bits, n):
    """range_raw: {~first, last + 1} of every key's run in the output, {0, 0} for a key that does not occur; runs that cross
    workgroup tiles are combined by the atomicMax"""
    rng = np.random.default_rng(9000 + 31 * total_bits + n)
    dists = _distributions(rng, n, total_bits)
    for name in DIST_NAMES:
        try:
            check_sort(dists[name], random_vals(rng, n), total_bits, with_ranges=True)
        except AssertionError as e:
            raise AssertionError(f"distribution {name}: {e}") from None


@pytest.mark.parametrize("n,total_bits", [(1, 13), (4097, 1), (10000, 13), (10000, 17), (200000, 13), (200000, 32), (33 * TILE + 1, 16)])
def test_argument_combinations_agree(n, total_bits):
    """vin null or arange(n), the sort's own histogram kernel or the producer's counts in GS2M_HIST_COPIES copies, scratch zeroed
    by the caller or by the sort: one output"""
    rng = np.random.default_rng(11000 + n + total_bits)
    keys = random_keys(rng, n, total_bits)
    hist = split_hist(keys, total_bits, rng)
    ek, ev = expected(keys, None, total_bits)
    for vals in (None, np.arange(n, dtype=np.uint32)):
        for ext in (None, hist):
            for prezeroed in (False, True):
                k, v, _ = run_sort(keys, vals, total_bits, prezeroed=prezeroed, ext_hist=ext)
                what = f"vin {'null' if vals is None else 'arange'}, ext_hist {'no' if ext is None else 'yes'}, prezeroed {prezeroed}"
                assert np.array_equal(k, ek) and np.array_equal(v, ev), what


@pytest.mark.parametrize("n,total_bits", [(4097, 1), (10000, 5), (200000, 13), (40 * TILE + 9, 13)])
def test_external_histogram_with_tile_ranges(n, total_bits):
    """the frame's arrangement: counts from the producer of the keys, pre-zeroed scratch, tile ranges out of the last pass; the same
    output and ranges as with the sort's own histogram kernel"""
    rng = np.random.default_rng(12000 + n + total_bits)
    keys = _distributions(rng, n, total_bits)["one-value-90-percent"]
    vals = random_vals(rng, n)
    own = check_sort(keys, vals, total_bits, with_ranges=True)
    ext = check_sort(keys, vals, total_bits, with_ranges=True, prezeroed=True, ext_hist=split_hist(keys, total_bits, rng))
    for a, b in zip(own, ext):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n,total_bits", [(1, 13), (10000, 13), (10000, 32)])
def test_undersized_scratch_is_refused_and_nothing_written(n, total_bits):
    rng = np.random.default_rng(5)
    need = temp_bytes(n, total_bits)
    for have in (need - 4, need // 2, 0):
        assert run_sort(random_keys(rng, n, total_bits), random_vals(rng, n), total_bits, scratch_bytes=have, expect_rc=ERR_INVALID_ARG) is None
