"""The per-Gaussian forward preprocess kernel of csrc/preprocess.hip alone (gs2m_debug_preprocess: the launcher of a frame on
caller-made inputs and caller-owned outputs) against tests/preprocess_ref.py, on the case families that file builds and
tests/test_preprocess_ref.py shows to hold their edge cases.  With no exception budget:

  * radii, the depth key, the record's centre, conic, opacity, colour, feature and padding lanes, the clamped bits: bit for bit the
    C oracle's (which tests/test_reference_gpu.py pins to the reference build);
  * ex, ey, tau2f: emit_ref.cull_params, equal where that is -1 or infinite, else within one float32 ulp (a double log and two
    double roots, each within an ulp or two of double, behind one rounding to float);
  * tiles_touched, rect and the record's REC_BIN words: preprocess_ref.shrunk_rect of the kernel's own (checked) ex and ey;
    block_tt, block_hu: emit_ref.block_counts of those counts;
  * sh_dir: |kernel - float64| <= (terms + 4) 2^-24 sum |terms| of preprocess_ref.sh_dir -- the forward error of a float32 sum of
    that many products with headroom for the products' own roundings and those of the normalised direction;
  * what is NOT stored: records and clamped bytes of Gaussians without a radius, sh_dir with precomputed colours, and the 64 guard
    words on either side of every output keep the sentinel the test put there."""
import numpy as np
import pytest
import torch

import emit_ref as E
import preprocess_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = np.uint32(0xA5A5A5A5)
_SENT_I32 = int(np.array([SENT]).view(np.int32)[0])
U24 = 2.0 ** -24
F32 = np.float32
ARGS = ("P", "D", "M", "means3D", "scales", "scale_modifier", "rotations", "opacities", "shs", "shs_rest", "cov3D_precomp", "colors_precomp", "features",
        "viewmatrix", "projmatrix", "cam_pos", "W", "H", "tan_fovx", "tan_fovy", "shrink", "radii", "observe_zero", "rec", "tiles_touched", "rect", "block_tt",
        "block_hu", "depth_key", "clamped", "sh_dir", "zero_words", "zero_count")
OUTPUTS = ("radii", "observe_zero", "rec", "tiles_touched", "rect", "block_tt", "block_hu", "depth_key", "clamped", "sh_dir")


class Out:
    """`n` elements of `dtype` filled with the sentinel, 64 sentinel words in front and behind (and up to the next whole word)"""

    def __init__(self, n, dtype=np.uint32):
        self.n, self.dtype = n, np.dtype(dtype)
        self.bytes = n * self.dtype.itemsize
        self.t = torch.full(((self.bytes + 3) // 4 + 2 * GUARD,), _SENT_I32, dtype=torch.int32, device="cuda")
        self.ptr = self.t.data_ptr() + 4 * GUARD

    def _raw(self):
        return self.t.cpu().numpy().view(np.uint8)

    def get(self):
        return self._raw()[4 * GUARD:4 * GUARD + self.bytes].copy().view(self.dtype)

    def guards_intact(self):
        b = self._raw()
        return bool(np.all(b[:4 * GUARD] == 0xA5) and np.all(b[4 * GUARD + self.bytes:] == 0xA5))

    def untouched(self):
        return bool(np.all(self._raw() == 0xA5))


def _dev(a, shift=0):
    """a float32 array on the device, `shift` floats off the allocation's (16-byte aligned) start -> (tensor, address)"""
    flat = np.ascontiguousarray(a, F32).reshape(-1)
    t = torch.zeros(len(flat) + shift + 4, dtype=torch.float32, device="cuda")
    t[shift:shift + len(flat)] = torch.from_numpy(flat)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * shift


def make_call(c, shrink, zero_words=0):
    """-> (args dict in the hook's order, outputs {name: Out}, the zero job's Out, the tensors kept alive)"""
    P, M, cam = c["P"], c["M"], c["cam"]
    keep, a = [], {}

    def put(name, arr, shift=0):
        if arr is None:
            a[name] = None
            return
        t, p = _dev(arr, shift)
        keep.append(t); a[name] = p
    a.update(P=P, D=c["D"], M=M, scale_modifier=float(c["scale_modifier"]), W=c["W"], H=c["H"], tan_fovx=cam["tanfovx"], tan_fovy=cam["tanfovy"],
             shrink=int(shrink))
    put("means3D", c["means3D"]); put("opacities", c["opacities"])
    precov, precol = c["cov3D_precomp"] is not None, c["colors_precomp"] is not None
    put("scales", None if precov else c["scales"]); put("rotations", None if precov else c["rotations"]); put("cov3D_precomp", c["cov3D_precomp"])
    put("colors_precomp", c["colors_precomp"])
    if precol:
        put("shs", None); put("shs_rest", None)
    elif c["layout"] == "split":
        assert M == 16
        put("shs", c["shs"][:, :1]); put("shs_rest", c["shs"][:, 1:])
    else:
        put("shs", c["shs"], shift=1 if c["layout"] == "offset" else 0); put("shs_rest", None)
    put("features", c["features"]); put("viewmatrix", cam["viewmatrix"]); put("projmatrix", cam["projmatrix"]); put("cam_pos", cam["campos"])
    nb = (P + 255) // 256
    out = dict(radii=Out(P, np.int32), observe_zero=Out(P, np.int32), rec=Out(32 * P, F32), tiles_touched=Out(P), rect=Out(2 * P), block_tt=Out(nb),
               block_hu=Out(nb), depth_key=Out(P), clamped=Out(P, np.uint8), sh_dir=Out(9 * P, F32))
    for k, o in out.items():
        a[k] = o.ptr
    if not c["observe"]:
        a["observe_zero"] = None
    zero = Out(zero_words)
    a["zero_words"], a["zero_count"] = zero.ptr, zero_words
    assert set(a) == set(ARGS)
    return a, out, zero, keep


def call(a):
    """the hook on an args dict -> its return code (nothing is read back here)"""
    import gs2m_native
    fn = gs2m_native.lib().gs2m_debug_preprocess
    return fn(*[a[k] for k in ARGS], gs2m_native.stream_ptr())


def run(c, shrink, zero_words=0):
    """-> ({name: array} of the outputs, the zero job's words); the return code is checked before anything is read back, and every
    guard word after"""
    import gs2m_native
    a, out, zero, keep = make_call(c, shrink, zero_words)
    gs2m_native.check(call(a), "gs2m_debug_preprocess")
    torch.cuda.synchronize()
    for k, o in out.items():
        assert o.guards_intact(), f"{c['name']}: guard words of {k} were written"
    assert zero.guards_intact(), f"{c['name']}: guard words of the zero job were written"
    if not c["observe"]:
        assert out["observe_zero"].untouched()
    return {k: o.get() for k, o in out.items()}, zero.get()


_ORACLE = {}


def oracle_of(oracle, c):
    """the oracle's forward of a case, computed once per case and shared"""
    if c["name"] not in _ORACLE:
        _ORACLE[c["name"]] = R.oracle_forward(oracle, c)
    return _ORACLE[c["name"]]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same(name, what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{name}: {what}: shape {got.shape}, expected {want.shape}"
    bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0] if got.size else []
    assert len(bad) == 0, f"{name}: {what}: {len(bad)} entries differ, the first at {bad[0]}: {got[bad[0]]}, expected {want[bad[0]]}"


def _within_one_ulp(name, what, got, want):
    """float32 arrays: bitwise equal where `want` is -1 or infinite, else both positive and finite and at most one float apart"""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    special = (want == F32(-1.0)) | np.isinf(want)
    _same(name, what + " (where the reference is -1 or infinite)", _bits(got)[special], _bits(want)[special])
    g, w = got[~special], want[~special]
    assert np.all(np.isfinite(g)) and np.all(g > 0) and np.all(w > 0), f"{name}: {what}"
    d = np.abs(g.view(np.int32).astype(np.int64) - w.view(np.int32).astype(np.int64))
    assert d.max(initial=0) <= 1, f"{name}: {what}: {int((d > 1).sum())} values are more than one float32 ulp away, the worst {int(d.max())}"
    return int((d != 0).sum()), len(d)


def check(c, f, shrink, got):
    """every output of one call against the reference; -> (values of ex, ey, tau2f not bit-equal, compared)"""
    name = f"{c['name']} shrink={shrink}"
    P, D = c["P"], c["D"]
    vis = f.radii > 0
    precol = c["colors_precomp"] is not None
    # always written
    _same(name, "radii", got["radii"], f.radii)
    _same(name, "depth_key", got["depth_key"], np.where(vis, _bits(f.depths), np.uint32(0xFFFFFFFF)))
    if c["observe"]:
        assert not got["observe_zero"].any(), f"{name}: observe is not zeroed"
    # the record: stored with a radius only
    rec = got["rec"].reshape(P, 32)
    recu = rec.view(np.uint32)
    assert np.all(recu[~vis] == SENT), f"{name}: the record of a Gaussian without a radius was stored"
    assert np.all(got["clamped"][~vis] == 0xA5), f"{name}: the clamped byte of a Gaussian without a radius was stored"
    v = np.nonzero(vis)[0]
    _same(name, "record: centre", recu[v, 0:2], _bits(f.means2D[v]))
    _same(name, "record: conic", np.stack([recu[v, 2], recu[v, 3], recu[v, 4]], 1), _bits(f.conic_opacity[v, :3]))
    _same(name, "record: opacity", recu[v, 5], _bits(f.conic_opacity[v, 3]))
    _same(name, "record: colour", recu[v, 12:15], _bits(c["colors_precomp"][v] if precol else f.rgb[v]))
    _same(name, "record: features", recu[v, 15:25], _bits(c["features"][v]) if c["features"] is not None else np.zeros((len(v), 10), np.uint32))
    _same(name, "record: padding", recu[v, 25:32], np.zeros((len(v), 7), np.uint32))
    rex, rey, rtau = E.cull_params(f.conic_opacity[v, 0], f.conic_opacity[v, 1], f.conic_opacity[v, 2], f.conic_opacity[v, 3])
    ne = nc = 0
    for what, k, want in (("ex", 6, rex), ("ey", 7, rey), ("tau2f", 11, rtau)):
        a, b = _within_one_ulp(name, what, rec[v, k], want)
        ne += a; nc += b
    # the rectangle, from the kernel's own (checked) extents: a last-bit difference of the double log cannot move a tile boundary
    ex, ey = np.where(vis, rec[:, 6], F32(0.0)).astype(F32), np.where(vis, rec[:, 7], F32(0.0)).astype(F32)
    tt, rect, bin_ = R.shrunk_rect(f.means2D[:, 0], f.means2D[:, 1], ex, ey, f.radii, f.tiles_x, f.tiles_y, shrink)
    _same(name, "tiles_touched", got["tiles_touched"], tt)
    _same(name, "rect", got["rect"].reshape(P, 2), rect)
    if not shrink:
        _same(name, "tiles_touched (the reference's)", got["tiles_touched"], f.tiles_touched)
    _same(name, "record: REC_BIN", recu[v, 8:11], np.concatenate([np.zeros((len(v), 1), np.uint32), bin_[v]], 1))
    bt, bh = E.block_counts(tt, E.CROWDED_WAVE)
    _same(name, "block_tt", got["block_tt"], bt)
    _same(name, "block_hu", got["block_hu"], bh)
    # colour side
    sd = got["sh_dir"].reshape(P, 9)
    if precol:
        assert np.all(_bits(sd) == SENT), f"{name}: sh_dir was written with precomputed colours"
        _same(name, "clamped", got["clamped"][v], np.zeros(len(v), np.uint8))
    else:
        _same(name, "clamped", got["clamped"][v], R.clamp_bits(f.clamped)[v])
        assert not np.any(_bits(sd) == SENT), f"{name}: {int((_bits(sd) == SENT).sum())} elements of sh_dir were not written"
        assert not _bits(sd[~vis]).any(), f"{name}: sh_dir of a Gaussian without a radius is not zero"
        if D == 0:
            assert not _bits(sd).any(), f"{name}: sh_dir at degree 0 is not zero"
        else:
            val, ab, n = R.sh_dir(D, c["shs"], R.unit_dirs(c["means3D"], c["cam"]["campos"]))
            err, bound = np.abs(sd.astype(np.float64) - val)[v], ((n + 4)[None, :] * U24 * ab)[v]
            bad = np.argwhere(err > bound)
            assert len(bad) == 0, (f"{name}: sh_dir: {len(bad)} elements outside (terms + 4) 2^-24 sum |terms|, the first: Gaussian {v[bad[0][0]]} element {bad[0][1]}: "
                                   f"{sd[v[bad[0][0]], bad[0][1]]!r}, expected {val[v[bad[0][0]], bad[0][1]]!r} +- {bound[bad[0][0], bad[0][1]]:.3e}")
            print(f"\n[preprocess] {name}: sh_dir worst error / bound {float((err / np.maximum(bound, 1e-300)).max(initial=0)):.3f}")
    return ne, nc


def run_and_check(oracle, c):
    f = oracle_of(oracle, c)
    res = {}
    for shrink in (0, 1):
        got, _ = run(c, shrink)
        ne, nc = check(c, f, shrink, got)
        res[shrink] = got
    print(f"\n[preprocess] {c['name']}: {int((f.radii > 0).sum())} of {c['P']} with a radius; ex, ey, tau2f not bit-equal to the reference: {ne} of {nc}")
    return f, res


@pytest.mark.parametrize("P", R.SIZES)
def test_sizes(oracle_lib, P):
    """every P % 4 (the 9 P % 4 tail of the sh_dir store, the end of the staged SH rows), one block, a full block and a partial
    one, a last wave of one lane; W x H = 184 x 120 and 185 x 121"""
    for which in (8, 9):
        run_and_check(oracle_lib, R.sizes_case(P, which))


@pytest.mark.parametrize("P", R.LAYOUT_SIZES)
def test_sh_layouts(oracle_lib, P):
    """one aligned (P, 16, 3) tensor, the same one float off alignment (no LDS staging), split DC / rest (P = 257: a full block and
    the not-full path; 45 P % 4 = 1 and 3: a tensor that ends inside a float4), M = 1, 4, 9 at their degree, M = 16 at degrees
    0 .. 3; the three layouts of the same coefficients give bit-identical records and sh_dir"""
    cases = R.layout_cases(P)
    res = {k: run_and_check(oracle_lib, c)[1] for k, c in cases.items()}
    for shrink in (0, 1):
        for other in ("offset", "split"):
            for k in OUTPUTS:
                assert np.array_equal(res["aligned"][shrink][k].view(np.uint8), res[other][shrink][k].view(np.uint8)), f"{k}: the {other} layout differs from the aligned one"


@pytest.mark.parametrize("kind", R.OTHER_KINDS)
def test_other_inputs(oracle_lib, kind):
    """precomputed covariances (the oracle's own of the scene) and colours, scale modifiers 0.5, 1, 2.5, no features (zero lanes), no
    observe array"""
    c = R.other_case(kind, oracle_lib)
    f, _ = run_and_check(oracle_lib, c)
    if kind == "cov3D_precomp":
        _same(kind, "radii against the scale / rotation run", f.radii, oracle_of(oracle_lib, R.other_case("modifier1")).radii)


def test_near_plane(oracle_lib):
    """view depth exactly 0.2f, one float below, one above, 0.2f + 1e-4, -1: visible beyond 0.2f only"""
    c = R.near_plane_case()
    f, res = run_and_check(oracle_lib, c)
    assert np.all(res[1]["radii"][c["groups"]["front"]] > 0) and not res[1]["radii"][c["groups"]["behind"]].any()
    assert np.all(res[1]["depth_key"][c["groups"]["behind"]] == 0xFFFFFFFF)


def test_degenerate_and_extreme_covariances(oracle_lib):
    """det == 0, the 0.1 floor, thin discs with the culling on and off, centres beyond the 1.3 tan(fov) clamp, large splats
    off-screen with and without a rectangle, splats that cover every tile"""
    c = R.degenerate_case()
    f, res = run_and_check(oracle_lib, c)
    g = c["groups"]
    assert not res[1]["radii"][g["zero"]].any() and np.all(res[1]["radii"][g["subpixel"]] == 2)
    assert np.all(res[0]["tiles_touched"][g["whole"]] == f.tiles_x * f.tiles_y)
    ex = res[1]["rec"].reshape(-1, 32)[g["discs"], 6]
    assert 0.05 <= float(np.isinf(ex).mean()) <= 0.5
    empty = (res[1]["radii"] > 0) & (res[1]["tiles_touched"] == 0)
    print(f"\n[preprocess] degenerate: {int(empty.sum())} with a radius and nothing emitted, {int(res[1]['tiles_touched'].sum())} of {int(res[0]['tiles_touched'].sum())} instances emitted")


def test_opacity_around_one_255th(oracle_lib):
    """below 1/255: radii > 0, tiles_touched == 0, rect == (0, 0), the record still stored, ex = ey = tau2f = -1"""
    c = R.opacity_case()
    f, res = run_and_check(oracle_lib, c)
    below, rest = c["groups"]["below"], np.setdiff1d(np.arange(c["P"]), c["groups"]["below"])
    d, rec = res[1], res[1]["rec"].reshape(-1, 32)
    assert np.all(d["radii"] > 0)
    assert not d["tiles_touched"][below].any() and not d["rect"].reshape(-1, 2)[below].any()
    assert np.all(rec[below][:, [6, 7, 11]] == -1.0) and np.array_equal(_bits(rec[below, 5]), _bits(c["opacities"][below]))
    assert np.all(rec[rest][:, [6, 7, 11]] > 0) and (d["tiles_touched"][rest] > 0).mean() > 0.9   # (a box of a few hundredths of a pixel can hold no pixel centre)
    assert np.all(res[0]["tiles_touched"] > 0), "the reference's rectangles do not look at the opacity"


def test_heavy_rule(oracle_lib):
    """crowded waves with and without Gaussians between the two bars, uncrowded waves with Gaussians of 40 tiles and more, a last
    partial wave with a heavy Gaussian: block_hu with shrink = 0 is a pure function of radius and centre"""
    c = R.heavy_case()
    f, res = run_and_check(oracle_lib, c)
    bt, bh = E.block_counts(f.tiles_touched, E.CROWDED_WAVE)
    _, bh_off = E.block_counts(f.tiles_touched, E.CROWDED_OFF)
    _same("heavy", "block_tt", res[0]["block_tt"], bt)
    _same("heavy", "block_hu", res[0]["block_hu"], bh)
    assert np.any(bh != bh_off)


@pytest.mark.parametrize("P", [1, 700])
def test_zero_job(oracle_lib, P):
    """0, 1, 255, 256, 257 and 5000 words: exactly those are zeroed, the guards around them stay, nothing else changes"""
    c = R.zero_case(P)
    base, _ = run(c, 1, 0)
    check(c, oracle_of(oracle_lib, c), 1, base)
    for words in R.ZERO_WORDS:
        got, zero = run(c, 1, words)
        assert len(zero) == words and not zero.any(), f"{words} words: not all zeroed"
        for k in OUTPUTS:
            assert np.array_equal(got[k].view(np.uint8), base[k].view(np.uint8)), f"{words} words: {k} differs from the call without a zero job"


@pytest.mark.parametrize("what", R.rejected_calls())
def test_rejected_arguments(what):
    """GS2M_ERR_INVALID_ARG and nothing launched: every output still holds the sentinel"""
    c = R.sizes_case(4, 8)
    if what.startswith("rest:"):
        c = dict(c, layout="split")
    a, out, zero, keep = make_call(c, 1, 16)
    kind, _, arg = what.partition(":")
    if kind == "null":
        assert a[arg] is not None
        a[arg] = None
    elif kind == "misaligned":
        a[arg] += 4
    elif what == "rest:M=9":
        a["M"], a["D"] = 9, 2
    elif what == "rest:misaligned":
        a["shs_rest"] += 4
    else:
        a["P"] = {"P=0": 0, "P=-1": -1, "P=2^28": 1 << 28}[what]
    assert call(a) == -1, what
    torch.cuda.synchronize()
    for k, o in list(out.items()) + [("zero job", zero)]:
        assert o.untouched(), f"{what}: {k} was written"


def test_the_good_call_of_the_rejection_test_is_accepted():
    for layout in ("aligned", "split"):
        a, out, zero, keep = make_call(dict(R.sizes_case(4, 8), layout=layout), 1, 16)
        assert call(a) == 0
        torch.cuda.synchronize()
        assert not zero.get().any() and not out["radii"].untouched()
