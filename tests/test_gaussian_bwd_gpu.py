"""The per-Gaussian backward of csrc/gaussian_bwd.hip alone (gs2m_debug_gaussian_bwd: heavy_reduce_kernel and gaussian_bwd_kernel
through the launchers of a frame, in a frame's order) on the row layouts of tests/gaussian_bwd_ref.py, which
tests/test_gaussian_bwd_ref.py shows to hold their edge cases.  With no exception budget:

  * the plain sums (dL/dmeans2D, dL/dconics, dL/dopacities, dL/dcolors with precomputed colours, dL/dfeatures) are BIT-EQUAL to the
    exact sums of the layout (every row element is k 2^-12 and every partial sum exact in float32) at 3, 4, 5 and 6 float4 per
    row, with 2 and 3 windows in flight, with the heavy unit count known on the host and read on the device;
  * path equivalences, every output byte for byte: 2 against 3 windows; the dense against the heavy arrangement of the same rows;
    the packed aligned, the packed one-float-off and the split SH tensors; dL/dSH wanted or not (everything else);
  * the chain (dL/dmeans3D, dL/dSH, dL/dscales, dL/drots, dL/dcov3D with precomputed covariances) against the C oracle's evaluation
    of the same chain on the same exact sums (oracle.backward_pergaussian, which tests/test_reference_gpu.py pins to the reference
    build) at the bound of helpers.assert_two_stage: rel 1e-5, floor 1e-6 of the rms, no exceptions;
  * Gaussians without a radius, coefficients above the active degree, dL/dscales and dL/drots with precomputed covariances, every
    sum without rows: +0 bits;
  * the 64 guard words around every output keep their sentinel, and the rows buffer (NaN wherever the kernel must not read: gaps
    between the waves' runs, unwritten rows of a unit, padding lanes, guard rows) is unchanged but for the units' sums.

radii, clamped and sh_dir of a scene come from one gs2m_debug_preprocess call (tested alone in tests/test_preprocess_gpu.py); radii
and clamped bits are compared with the oracle's before use.

Elements of the chain not bit-equal to the oracle, as printed on an MI355X (of the elements of Gaussians with a radius):
dL/dmeans3D 0 of 90 618, dL/dSH 0 of 1 226 454, dL/dscales 0 of 90 618, dL/drots 0 of 120 824, dL/dcov3D 0 of 12 132 over all tests of
this file: none (the counts are printed per case, with the running totals, when the file is run with -s)."""
import numpy as np
import pytest
import torch

import gaussian_bwd_ref as B
import helpers as Hh
import preprocess_ref as R
import test_preprocess_gpu as TP
from test_preprocess_gpu import Out, _bits, _dev

pytestmark = pytest.mark.gpu

F32 = np.float32
ARGS = ("P", "D", "M", "means3D", "shs", "shs_rest", "colors_precomp", "scales", "scale_modifier", "rotations", "cov3D_precomp", "viewmatrix", "projmatrix",
        "campos", "W", "H", "tan_fovx", "tan_fovy", "radii", "fc", "rec", "gauss_rows", "tiles_touched", "wave_rowbase", "clamped", "sh_dir", "hrec", "counters",
        "rows", "have_rows", "heavy_units", "windows", "dL_dmeans2D", "dL_dconics", "dL_dopacities", "dL_dcolors", "dL_dmeans3D", "dL_dcov3D", "dL_dshs",
        "dL_dshs_rest", "dL_dscales", "dL_drots", "dL_dfeatures")
PLAIN = ("means2D", "conics", "opacities", "colors", "features")
CHAIN = ("means3D", "shs", "scales", "rotations", "cov3D")


def _arg(k):
    """the hook's parameter of output k"""
    return "dL_d" + {"rotations": "rots"}.get(k, k)


class ShiftedOut(Out):
    """an Out whose data start one float behind a 16-byte boundary; the float in front belongs to the guard"""

    def __init__(self, n):
        super().__init__(n + 1, F32)
        self.ptr += 4

    def get(self):
        return super().get()[1:]

    def guards_intact(self):
        return super().guards_intact() and _bits(super().get()[:1])[0] == TP.SENT


def _devu(a):
    """integer / byte arrays on the device as they are (allocations are 256-byte aligned) -> (tensor, address)"""
    raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    t = torch.from_numpy(np.concatenate([raw, np.zeros(16, np.uint8)])).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr()


_PRE = {}


def preprocess_of(oracle, c):
    """radii, clamped and sh_dir of a case from the preprocess hook, once per case; radii and clamped bits checked against the oracle"""
    if c["name"] not in _PRE:
        f = TP.oracle_of(oracle, c)
        got, _ = TP.run(c, 1)
        assert np.array_equal(got["radii"], f.radii), f"{c['name']}: radii differ from the oracle's"
        vis = f.radii > 0
        if c["colors_precomp"] is None:
            assert np.array_equal(got["clamped"][vis], R.clamp_bits(f.clamped)[vis]), f"{c['name']}: clamped bits differ from the oracle's"
        _PRE[c["name"]] = dict(radii=got["radii"].copy(), clamped=got["clamped"].copy(), sh_dir=got["sh_dir"].copy(), vis=vis)
    return _PRE[c["name"]]


def make_call(c, pre, L, windows=0, units_known=True, want_sh=True, have_rows=True):
    """-> (args dict in the hook's order, outputs {name: Out}, the rows tensor, the tensors kept alive)"""
    P, M, cam = c["P"], c["M"], c["cam"]
    assert L.P == P
    keep, a = [], {}

    def put(name, arr, shift=0, raw=False):
        if arr is None:
            a[name] = None
            return
        t, p = _devu(arr) if raw else _dev(arr, shift)
        keep.append(t); a[name] = p
    precov, precol = c["cov3D_precomp"] is not None, c["colors_precomp"] is not None
    split, offset = (not precol) and c["layout"] == "split", (not precol) and c["layout"] == "offset"
    a.update(P=P, D=c["D"], M=M, scale_modifier=float(c["scale_modifier"]), W=c["W"], H=c["H"], tan_fovx=cam["tanfovx"], tan_fovy=cam["tanfovy"], fc=L.fc,
             rec=None, have_rows=int(have_rows), heavy_units=L.units if units_known else -1, windows=windows)
    put("means3D", c["means3D"]); put("viewmatrix", cam["viewmatrix"]); put("projmatrix", cam["projmatrix"]); put("campos", cam["campos"])
    put("scales", None if precov else c["scales"]); put("rotations", None if precov else c["rotations"]); put("cov3D_precomp", c["cov3D_precomp"])
    put("colors_precomp", c["colors_precomp"])
    if precol:
        put("shs", None); put("shs_rest", None)
    elif split:
        assert M == 16
        put("shs", c["shs"][:, :1]); put("shs_rest", c["shs"][:, 1:])
    else:
        put("shs", c["shs"], shift=1 if offset else 0); put("shs_rest", None)
    put("radii", pre["radii"].astype(np.int32), raw=True); put("clamped", pre["clamped"], raw=True); put("sh_dir", pre["sh_dir"])
    for k in ("gauss_rows", "tiles_touched", "wave_rowbase", "hrec", "counters"):
        put(k, getattr(L, k) if have_rows else None, raw=True)
    if have_rows and L.units == 0:
        put("hrec", np.zeros(80, np.uint8), raw=True)
    rows_t = torch.from_numpy(L.rows).cuda() if have_rows else None
    a["rows"] = rows_t.data_ptr() + 4 * B.GUARD_ROWS * L.rowf if have_rows else None
    out = dict(means2D=Out(4 * P, F32), conics=Out(4 * P, F32), opacities=Out(P, F32), colors=Out(3 * P, F32), means3D=Out(3 * P, F32), cov3D=Out(6 * P, F32),
               scales=Out(3 * P, F32), rotations=Out(4 * P, F32), features=Out(R.NUM_FEATURES * P, F32))
    if split:
        out["shs"], out["shs_rest"] = Out(3 * P, F32), Out(45 * P, F32)
    else:
        n = 3 * M * P if not precol else 4
        out["shs"], out["shs_rest"] = ShiftedOut(n) if offset else Out(n, F32), Out(4, F32)
    for k, o in out.items():
        a[_arg(k)] = o.ptr
    if not precol:
        a["dL_dcolors"] = None
    if not precov:
        a["dL_dcov3D"] = None
    if not split:
        a["dL_dshs_rest"] = None
    if precol or not want_sh:
        a["dL_dshs"] = a["dL_dshs_rest"] = None
    assert set(a) == set(ARGS)
    return a, out, rows_t, keep


def call(a):
    import gs2m_native
    return gs2m_native.lib().gs2m_debug_gaussian_bwd(*[a[k] for k in ARGS], gs2m_native.stream_ptr())


def run(c, pre, L, **kw):
    """-> {name: array} of the outputs (shs as (P, M, 3) whatever the layout; None for what the call does not write).  The return
    code is checked before anything is read back, every guard word and the rows buffer after"""
    import gs2m_native
    a, out, rows_t, keep = make_call(c, pre, L, **kw)
    gs2m_native.check(call(a), "gs2m_debug_gaussian_bwd")
    torch.cuda.synchronize()
    name = f"{L.name} {kw}"
    for k, o in out.items():
        assert o.guards_intact(), f"{name}: guard words of {k} were written"
    if rows_t is not None:   # nothing but the units' sums is written
        after, before = rows_t.cpu().numpy().view(np.uint32), L.rows.view(np.uint32)
        same = (after == before).all(1)
        assert same[np.setdiff1d(np.arange(len(same)), B.unit_sum_rows(L))].all(), f"{name}: rows other than the units' first were written"
    P, M = c["P"], c["M"]
    res = {}
    for k, o in out.items():
        if a[_arg(k)] is None:
            assert o.untouched(), f"{name}: {k} was written without being asked for"
            res[k] = None
        else:
            res[k] = o.get()
            assert not np.any(_bits(res[k]) == TP.SENT), f"{name}: {int((_bits(res[k]) == TP.SENT).sum())} elements of {k} were not written"
    if res["shs_rest"] is not None:
        res["shs"] = np.concatenate([res["shs"].reshape(P, 1, 3), res.pop("shs_rest").reshape(P, 15, 3)], 1)
    else:
        res.pop("shs_rest")
        if res["shs"] is not None:
            res["shs"] = res["shs"].reshape(P, M, 3)
    for k, w in (("means2D", 4), ("conics", 4), ("colors", 3), ("means3D", 3), ("cov3D", 6), ("scales", 3), ("rotations", 4), ("features", R.NUM_FEATURES)):
        if res[k] is not None:
            res[k] = res[k].reshape(P, w)
    return res


def assert_plain(name, L, got):
    for k in PLAIN:
        if got[k] is None:
            assert k == "colors"
            continue
        g, w = _bits(got[k]).reshape(L.P, -1), _bits(L.expected[k]).reshape(L.P, -1)
        bad = np.nonzero((g != w).any(1))[0]
        assert len(bad) == 0, (f"{name}: dL/d{k}: {len(bad)} Gaussians not bit-equal to the exact sums, the first {bad[0]} (gauss_rows {L.gauss_rows[bad[0]]:#x}): "
                               f"{got[k][bad[0]]}, expected {L.expected[k][bad[0]]}")


def assert_same(name, a, b, skip=()):
    for k in a:
        if k in skip:
            continue
        assert (a[k] is None) == (b[k] is None), f"{name}: {k}"
        if a[k] is not None:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{name}: {k}: {int((_bits(a[k]) != _bits(b[k])).sum())} elements differ"


_COUNTS = {}


def assert_chain(oracle, c, pre, L, got, want_sh=True):
    """the chain outputs against the oracle's chain on the same exact sums; the structural zeros; -> counts not bit-equal"""
    name, P, D, M = L.name, c["P"], c["D"], c["M"]
    f = TP.oracle_of(oracle, c)
    e = L.expected
    chain = oracle.backward_pergaussian(f, e["means2D"], e["conics"], e["colors"])
    vis = pre["vis"]
    precov, precol = c["cov3D_precomp"] is not None, c["colors_precomp"] is not None
    line = []
    for k in CHAIN:
        if got[k] is None:
            assert (k == "cov3D" and not precov) or (k == "shs" and (precol or not want_sh)), f"{name}: {k}"
            continue
        ref = chain[k].reshape(got[k].shape)
        assert np.all(np.isfinite(ref)), f"{name}: the oracle's dL/d{k} is not finite"
        Hh.assert_grad_close(f"{name}: chain:{k}", got[k], ref, rel=1e-5, floor_frac=1e-6, max_exceptions=0.0)
        assert not _bits(got[k][~vis]).any(), f"{name}: dL/d{k} of a Gaussian without a radius is not +0"
        ne = int((_bits(got[k][vis]) != _bits(ref[vis])).sum())
        line.append(f"{k} {ne}/{got[k][vis].size}")
        _COUNTS.setdefault(k, [0, 0])
        _COUNTS[k][0] += ne; _COUNTS[k][1] += got[k][vis].size
    if got["shs"] is not None:
        assert not _bits(got["shs"][:, (D + 1) ** 2:]).any(), f"{name}: coefficients above degree {D} are not +0"
    if precov:
        assert not _bits(got["scales"]).any() and not _bits(got["rotations"]).any(), f"{name}: dL/dscales, dL/drots with precomputed covariances"
    for k in PLAIN:
        if got[k] is not None:
            assert not _bits(got[k][~vis]).any(), f"{name}: dL/d{k} of a Gaussian without a radius is not +0"
    print(f"\n[gaussian_bwd] {name}: {int(vis.sum())} of {P} with a radius; not bit-equal to the oracle: " + ", ".join(line)
          + "; so far " + ", ".join(f"{k} {v[0]}/{v[1]}" for k, v in _COUNTS.items()))


def run_scene(oracle, c, fc=10, **kw):
    """one scene case with random rows (a few window-covering, three heavy Gaussians) on the Gaussians with a radius: plain sums and chain"""
    pre = preprocess_of(oracle, c)
    L = B.scene_layout(c, pre["vis"], fc)
    got = run(c, pre, L, **kw)
    assert_plain(L.name, L, got)
    assert_chain(oracle, c, pre, L, got, want_sh=kw.get("want_sh", True))
    return pre, L, got


# ---- row patterns --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("which,P", [(w, P) for w in "AB" for P in B.PATTERN_SIZES[w]])
def test_row_patterns(oracle_lib, which, P):
    """wave totals of 0 .. 257 rows (0 .. 5 windows), an empty wave, random counts, window-aligned Gaussians of 64 .. 320 rows,
    Gaussians from mid-window over whole windows to mid-window (alone, two per wave in different and in the same lane group, back
    to back on a window edge), gaps between the waves' runs, P % 256 = 1, 255, 0, 3: exact sums at every row width with 2 and 3
    windows in flight, and 2 against 3 byte for byte; the chain once per layout"""
    c = B.visible_scene(P)
    pre = preprocess_of(oracle_lib, c)
    assert pre["vis"].all()
    for fc in B.FCS:
        L = B.pattern_layout(which, P, fc)
        res = {}
        for win in (2, 3):
            res[win] = run(c, pre, L, windows=win)
            assert_plain(f"{L.name} windows={win}", L, res[win])
        assert_same(f"{L.name}: 2 against 3 windows", res[2], res[3])
        if fc == 10:
            assert_same(f"{L.name}: the launcher's own rule", run(c, pre, L, windows=0), res[3])
            assert_chain(oracle_lib, c, pre, L, res[2])


@pytest.mark.parametrize("fc", B.FCS)
def test_heavy_patterns(oracle_lib, fc):
    """Gaussians of 1 .. 130 units, three heavy ones of both kinds in one wave, a wave of heavy ones only, instance counts that are
    no multiples of 64, units whose sum lands on a row nobody wrote: exact sums with the unit count known on the host and read on
    the device, with 2 and 3 windows; the dense arrangement of the same rows gives the same bytes"""
    c = B.visible_scene(B.HEAVY_P)
    pre = preprocess_of(oracle_lib, c)
    assert pre["vis"].all()
    H, Dn = B.heavy_layouts(fc)
    first = None
    for win in (2, 3):
        for known in (True, False):
            got = run(c, pre, H, windows=win, units_known=known)
            assert_plain(f"{H.name} windows={win} units known={known}", H, got)
            first = first or got
            assert_same(f"{H.name}: windows={win} units known={known} against the first run", got, first)
        dense = run(c, pre, Dn, windows=win)
        assert_plain(f"{Dn.name} windows={win}", Dn, dense)
        assert_same(f"{H.name}: the dense arrangement, windows={win}", dense, first)
    if fc == 10:
        assert_chain(oracle_lib, c, pre, H, first)


# ---- the scene side ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("P", R.SIZES)
def test_sizes(oracle_lib, P):
    """every P % 4, one block, a full block and a partial one, a last wave of one lane; 184 x 120 and 185 x 121; fc = 10 and 2"""
    run_scene(oracle_lib, R.sizes_case(P, 8), fc=10)
    run_scene(oracle_lib, R.sizes_case(P, 9), fc=2, windows=2)


@pytest.mark.parametrize("P", R.LAYOUT_SIZES)
def test_sh_layouts(oracle_lib, P):
    """dL/dSH packed through LDS, one float off alignment (straight stores), split DC / rest (45 P % 4 = 1 and 3: the scalar tail),
    M = 1, 4, 9 at their degree, M = 16 at degrees 0 .. 3; the three layouts of the same coefficients give the same bytes; without
    dL/dSH everything else is the same and dL/dSH keeps the sentinel (checked by run)"""
    assert sorted(45 * p % 4 for p in R.LAYOUT_SIZES) == [1, 3]
    res = {}
    for k, c in R.layout_cases(P).items():
        pre, L, res[k] = run_scene(oracle_lib, c)
        if k in ("aligned", "split", "M4"):
            without = run(c, pre, L, want_sh=False)
            assert without["shs"] is None
            assert_same(f"{L.name}: without dL/dSH", res[k], without, skip=("shs",))
    for other in ("offset", "split"):
        assert_same(f"sh layouts {P}: {other} against aligned", res["aligned"], res[other])


def test_clamp_bits(oracle_lib):
    """all 8 combinations of the clamped channels (tests/test_gaussian_bwd_ref.py) at fc = 0 and 6"""
    c = B.clamp_case()
    pre = preprocess_of(oracle_lib, c)
    assert set(pre["clamped"][pre["vis"]]) == set(range(8))
    run_scene(oracle_lib, c, fc=0)
    run_scene(oracle_lib, c, fc=6)


@pytest.mark.parametrize("kind", ["cov3D_precomp", "colors_precomp", "both_precomp", "modifier0.5", "modifier2.5", "no_features"])
def test_other_inputs(oracle_lib, kind):
    """precomputed covariances (dL/dcov3D; dL/dscales and dL/drots +0) and colours (dL/dcolors, no dL/dSH), scale modifiers 0.5 and 2.5"""
    c = R.other_case(kind, oracle_lib)
    _, _, got = run_scene(oracle_lib, c, fc=0 if kind == "no_features" else 10)
    assert (got["cov3D"] is not None) == ("cov3D" in kind or kind == "both_precomp") and (got["colors"] is not None) == ("colors" in kind or kind == "both_precomp")


def test_degenerate_and_near_plane(oracle_lib):
    """centres beyond the 1.3 tan(fov) clamp (x_grad_mul = 0), det == 0, splats that cover every tile; view depths around 0.2"""
    c = R.degenerate_case()
    pre, _, got = run_scene(oracle_lib, c)
    g = c["groups"]
    assert pre["vis"][g["clamp"]].sum() > 20 and not pre["vis"][g["zero"]].any() and pre["vis"][g["whole"]].all()
    assert np.abs(got["means3D"][g["clamp"]]).max() > 0
    c = R.near_plane_case()
    pre, _, _ = run_scene(oracle_lib, c)
    assert pre["vis"][c["groups"]["front"]].all() and not pre["vis"][c["groups"]["behind"]].any()


@pytest.mark.parametrize("P", [1, 257, 700])
def test_without_rows(oracle_lib, P):
    """have_rows = 0, rows null: every plain sum is +0, the chain is the oracle's on zero sums"""
    c = R.sizes_case(P, 9) if P != 700 else R.other_case("both_precomp", oracle_lib)
    pre = preprocess_of(oracle_lib, c)
    Z = B.arrange(f"{c['name']}-no-rows", 10, B.make_values(np.zeros(P, np.int64), 1))
    got = run(c, pre, Z, have_rows=False)
    for k in PLAIN:
        assert got[k] is None or not _bits(got[k]).any(), k
    assert_chain(oracle_lib, c, pre, Z, got)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------


def _good_call(split=False):
    c = dict(B.visible_scene(70), layout="split" if split else "aligned")
    pre = dict(radii=np.full(70, 3, np.int32), clamped=np.zeros(70, np.uint8), sh_dir=np.zeros(9 * 70, F32))
    counts = np.random.default_rng(5).choice(B.RANDOM_COUNTS, 70).astype(np.int64)
    pop = np.random.default_rng(6).integers(0, 5, 60).astype(np.uint8)
    counts[1] = int(pop.sum())
    L = B.arrange("good-call", 10, B.make_values(counts, 7), heavy={1: pop})
    return (c, L) + make_call(c, pre, L, windows=2)


@pytest.mark.parametrize("what", B.rejected_calls())
def test_rejected_arguments(what):
    """GS2M_ERR_INVALID_ARG and nothing launched: every output still holds the sentinel and no row has changed"""
    c, L, a, out, rows_t, keep = _good_call(split=what.startswith("rest:"))
    spare, spare_p = _dev(np.zeros(70 * 48, F32))
    kind, _, arg = what.partition(":")
    if kind == "null":
        assert a[arg] is not None
        a[arg] = None
    elif kind == "misaligned":
        a[arg] += 2 if arg == "hrec" else 4
    elif kind == "both":
        a[arg] = spare_p
    elif what == "precomp:no-dL_dcolors":
        a["shs"], a["colors_precomp"] = None, spare_p
    elif what == "precomp:no-dL_dcov3D":
        a["scales"], a["rotations"], a["cov3D_precomp"] = None, None, spare_p
    elif what == "rest:M=9":
        a["M"], a["D"] = 9, 2
    elif what == "rest:misaligned":
        a["shs_rest"] += 4
    elif what == "rest:dL-misaligned":
        a["dL_dshs_rest"] += 4
    elif what == "rest:only-dL_dshs":
        a["dL_dshs_rest"] = None
    elif what == "rest:only-dL_dshs_rest":
        a["dL_dshs"] = None
    elif what == "packed:dL_dshs_rest":
        a["dL_dshs_rest"] = spare_p
    else:
        k, _, v = what.partition("=")
        a[k] = (1 << 28) if v == "2^28" else int(v)
    assert call(a) == -1, what
    torch.cuda.synchronize()
    for k, o in out.items():
        assert o.untouched(), f"{what}: {k} was written"
    assert np.array_equal(rows_t.cpu().numpy().view(np.uint32), L.rows.view(np.uint32)), f"{what}: rows were written"


def test_the_good_call_of_the_rejection_test_is_accepted():
    for split in (False, True):
        c, L, a, out, rows_t, keep = _good_call(split)
        assert call(a) == 0
        torch.cuda.synchronize()
        assert not out["means2D"].untouched() and all(o.guards_intact() for o in out.values())
        assert np.array_equal(_bits(out["means2D"].get()), _bits(L.expected["means2D"]).reshape(-1))
