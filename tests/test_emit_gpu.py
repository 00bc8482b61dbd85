"""The instance emission of csrc/binning.hip alone (gs2m_debug_emit: recount_heavy_kernel, blockscan_kernel, emit_kernel,
emit_heavy_kernel, rowscan_kernel through the launchers of a frame) on caller-made rectangles and records, against
tests/emit_ref.py:

  * every integer the stage writes -- tile keys, instance records, dense and reserved row numbers, rows per Gaussian and per wave,
    row bases, heavy units and their populations, digit counts, totals -- follows exactly from the rectangles and the quadrant
    masks the kernel produced (array_equal);
  * the masks themselves: must_hit <= mask <= may_hit, quadrant by quadrant.  The first inclusion is the soundness of the culling
    (a quadrant that holds a pixel the blend kernels would accept is never dropped) and has no exception budget;
  * guard words around every output come back untouched; inputs are not written.

The share of set bits outside must_hit -- what the margins of the culling cost -- is printed per family (DESIGN.md records it)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import emit_ref as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
PATTERN = np.uint32(0xA5C3F00D)
HIST_COPIES, HIST_COPY_WORDS, HRECW = 8, 1024, 20     # common.h: GS2M_HIST_*, sizeof(HeavyUnit) / 4


def _common_h(name):
    txt = open(os.path.join(ROOT, "gs-2m_amd", "csrc", "common.h")).read()
    return int(re.search(r"^#define\s+" + name + r"\s+(0x[0-9A-Fa-f]+|\d+)u?\b", txt, flags=re.M).group(1), 0)


def test_the_reference_uses_the_constants_of_common_h():
    for name, v in (("GS2M_HEAVY_TILES", E.HEAVY_TILES), ("GS2M_HEAVY_TILES_CROWDED", E.HEAVY_TILES_CROWDED), ("GS2M_CROWDED_WAVE", E.CROWDED_WAVE),
                    ("GS2M_CROWDED_OFF", E.CROWDED_OFF), ("GS2M_UNIT", E.UNIT), ("GS2M_ROWS_BIG", E.ROWS_BIG), ("GS2M_GID_BITS", E.GID_BITS),
                    ("GS2M_HIST_COPIES", HIST_COPIES), ("GS2M_HIST_COPY_WORDS", HIST_COPY_WORDS), ("GS2M_CNT_ROWS", 2), ("GS2M_CNT_HUNITS", 3),
                    ("GS2M_LAND_R", 0), ("GS2M_LAND_HUNITS", 1), ("GS2M_LAND_ROWS", 3), ("REC_GEO0", 0), ("REC_GEO1", 1), ("REC_BIN", 2)):
        assert _common_h(name) == v, name


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1).copy()).cuda()


class Guarded:
    """`words` words (the pattern, or `fill`) with GUARD pattern words in front and behind"""

    def __init__(self, words, fill=None):
        a = np.full(words + 2 * GUARD, PATTERN, np.uint32)
        if fill is not None:
            a[GUARD:GUARD + words] = fill
        self.words, self.t = words, _dev(a)
        self.ptr = self.t.data_ptr() + 4 * GUARD

    def inside(self):
        return self.t[GUARD:GUARD + self.words].cpu().numpy().view(np.uint32)

    def guards_intact(self):
        g = self.t.cpu().numpy().view(np.uint32)
        return bool(np.all(g[:GUARD] == PATTERN) and np.all(g[GUARD + self.words:] == PATTERN))


@functools.lru_cache(maxsize=None)
def _plan(tile_bits):
    import ctypes as C
    import gs2m_native
    npass, bits, shift = C.c_int(0), (C.c_int * 4)(), (C.c_int * 4)()
    gs2m_native.check(gs2m_native.lib().gs2m_debug_radix_plan(tile_bits, C.byref(npass), bits, shift), "gs2m_debug_radix_plan")
    return npass.value, list(bits), list(shift)


def run_case(case):
    """-> (mask bits[R, 4], must, may); asserts the layout, the guard words and the two inclusions"""
    import ctypes as C
    import gs2m_native
    rect, rec, depth, crowded = case["rect"], case["rec"], case["depth_key"], case["crowded"]
    P, name = len(rect), case["name"]
    cnt = E.rect_counts(rect)
    R = int(cnt.sum())
    nb, nw = (P + 255) // 256, (P + 63) // 64
    block_tt, block_hu_on = E.block_counts(cnt, E.CROWDED_WAVE)        # as the preprocess kernel leaves them: the rule on
    _, block_hu = E.block_counts(cnt, crowded)
    U = int(block_hu.sum())
    t_rect, t_rec, t_depth, t_tt = _dev(rect), _dev(rec), _dev(depth), _dev(block_tt)
    inputs0 = [t.clone() for t in (t_rect, t_rec, t_depth, t_tt)]
    out = dict(block_hu=Guarded(nb, block_hu_on), block_pref=Guarded(nb), block_hupref=Guarded(nb), keys=Guarded(R), e_rec=Guarded(4 * R),
               hrec=Guarded(HRECW * U), gauss_rows=Guarded(P), wave_rows=Guarded(nw), wave_rowbase=Guarded(nw), counters=Guarded(64),
               tile_hist=Guarded(HIST_COPIES * HIST_COPY_WORDS, 0), landing=Guarded(4))
    gs2m_native.launch("gs2m_debug_emit", torch.device("cuda", torch.cuda.current_device()), P, case["W"], case["H"], case["tiles_x"], case["tile_bits"],
                       C.c_int(crowded).value, U, t_rect.data_ptr(), t_rec.data_ptr(), t_depth.data_ptr(), t_tt.data_ptr(), out["block_hu"].ptr,
                       out["block_pref"].ptr, out["block_hupref"].ptr, out["keys"].ptr, out["e_rec"].ptr, out["hrec"].ptr, out["gauss_rows"].ptr,
                       out["wave_rows"].ptr, out["wave_rowbase"].ptr, out["counters"].ptr, out["tile_hist"].ptr, out["landing"].ptr)
    torch.cuda.synchronize()
    for t, t0 in zip((t_rect, t_rec, t_depth, t_tt), inputs0):
        assert torch.equal(t, t0), f"{name}: an input was written"
    for k, g in out.items():
        assert g.guards_intact(), f"{name}: guard words of {k} were written"
    got = {k: g.inside() for k, g in out.items()}
    e_rec = got["e_rec"].reshape(R, 4)
    masks = (e_rec[:, 0] >> np.uint32(E.GID_BITS)).astype(np.int64)
    want = E.expected_layout(rect, depth, masks, crowded, case["tiles_x"], _plan(case["tile_bits"]))
    assert (want["R"], want["U"]) == (R, U)

    def same(what, a, b):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape == b.shape and a.size == 0:
            return
        bad = np.nonzero((a != b).reshape(len(a), -1).any(1))[0] if a.shape == b.shape else [-1]
        assert len(bad) == 0, f"{name}: {what}: {len(bad)} entries differ, the first at {bad[0]}: {a[bad[0]] if a.shape == b.shape else a.shape}, expected {b[bad[0]] if a.shape == b.shape else b.shape}"

    same("block_hu", got["block_hu"], block_hu)
    same("block_pref", got["block_pref"], np.cumsum(block_tt.astype(np.int64)) - block_tt)
    same("block_hupref", got["block_hupref"], np.cumsum(block_hu.astype(np.int64)) - block_hu)
    same("keys_unsorted", got["keys"], want["keys"])
    same("e_rec", e_rec, want["e_rec"])
    same("gauss_rows", got["gauss_rows"], want["gauss_rows"])
    same("wave_rows", got["wave_rows"], want["wave_rows"])
    same("wave_rowbase", got["wave_rowbase"], want["wave_rowbase"])
    hrec = got["hrec"].reshape(U, HRECW)
    same("hrec.gid", hrec[:, 0], want["h_gid"])
    same("hrec.off", hrec[:, 1], want["h_off"])
    same("hrec.pop", np.ascontiguousarray(hrec[:, 4:]).view(np.uint8).reshape(U, E.UNIT), want["pop"])
    hist = got["tile_hist"].reshape(HIST_COPIES, 4, 256).astype(np.int64).sum(0)
    same("tile_hist", hist, want["hist"])
    want_c = np.full(64, PATTERN, np.uint32)
    want_c[:6] = (R, R, want["rows"], U, 0, 0)
    same("counters", got["counters"], want_c)
    want_l = np.array([R, U, PATTERN, want["rows"] + 1], np.uint32)
    same("landing", got["landing"], want_l)

    must, may, n_req, n_amb = E.brackets(case)
    m = E.bits(masks)
    lost = np.nonzero((must & ~m).any(1))[0]
    gid, _, tx, ty = E.instances(rect)
    assert len(lost) == 0, (f"{name}: {len(lost)} instances miss a quadrant that holds an accepted pixel; the first: Gaussian {gid[lost[0]]} "
                            f"{rec[gid[lost[0]], :6]} t2 {rec[gid[lost[0]], 11]} tile ({tx[lost[0]]}, {ty[lost[0]]}) mask {masks[lost[0]]:#x}, required {must[lost[0]]}")
    extra = np.nonzero((m & ~may).any(1))[0]
    assert len(extra) == 0, (f"{name}: {len(extra)} instances have a quadrant set that the region cannot reach; the first: Gaussian {gid[extra[0]]} "
                             f"{rec[gid[extra[0]], :6]} t2 {rec[gid[extra[0]], 11]} tile ({tx[extra[0]]}, {ty[extra[0]]}) mask {masks[extra[0]]:#x}, allowed {may[extra[0]]}")
    return m, must, may


@pytest.mark.parametrize("P,kind", E.LAYOUT_CASES, ids=[f"{k}-{P}" for P, k in E.LAYOUT_CASES])
def test_layout_at_every_count_class(P, kind):
    """partial last waves and blocks; counts of 0; 1 x 1, 1 x N, N x 1; 39 | 40; 64, 65, 129 (one, two, three units); a wave that is all
    heavy; a crowded wave of 7s and 8s with the rule on and off; a wave of light sum exactly 320; 7 and 9 tile bits"""
    case = E.layout_case(P, kind)
    cnt = E.rect_counts(case["rect"])
    heavy, units = E.heavy_rule(cnt, case["crowded"])
    if kind == "mixed" and P >= 63:
        assert {0, 1, 6, 7, 39, 40, 64, 65, 129} <= set(cnt.tolist()) and {1, 2, 3} <= set(units.tolist()) and case["tile_bits"] == 9
        assert not heavy[cnt == 39].any() and heavy[cnt == 40].all()
    if kind == "all-heavy":
        assert heavy[:64].all() and case["tile_bits"] == 7
    if kind == "crowded":
        assert np.array_equal(heavy[:64], cnt[:64] == 8) and not heavy[64:128].any()
    if kind in ("crowded-off", "light-320"):
        assert not heavy[:64].any() and cnt[:64].sum() in (480, 320)
    run_case(case)


@pytest.mark.parametrize("seed", [0, 1], ids=["w8", "w9"])
@pytest.mark.parametrize("family", E.FAMILIES)
def test_masks_between_must_and_may(family, seed):
    """isotropic 0.25 .. 300 pixels; axis ratios 2 .. 190 at 0, 45, 90, 135 degrees and twenty random angles; ratios 210 and 1000 with
    the culling off; below 1/255.  seed 0: the image's last tile column and row have pixels in their left / upper quadrants only
    (W % 16 = H % 16 = 8); seed 1: one pixel of the right / lower ones (9)"""
    case = E.family_case(family, seed)
    m, must, may = run_case(case)
    if family == "off":
        assert np.array_equal(m, may), "culling off: every quadrant that has pixels"
    if family == "low":
        assert m.sum() > 0 and np.all(m.sum(1) <= 1) and (m.sum(1) == 0).sum() > 1000, "below 1/255: the centre's quadrant at most; most instances carry no row"
    print(f"\n[emit] {case['name']}: {int(m.sum())} quadrant bits set, {int(must.sum())} required, "
          f"share of set bits outside must_hit {float((m & ~must).sum()) / max(int(m.sum()), 1):.4f}")
