"""csrc/blend_fwd_q.hip and csrc/blend_bwd_q.hip alone, through their launchers, on caller-made quadrant lists
(gs2m_debug_blend_forward / gs2m_debug_blend_backward) against the float64 restatement of renderCUDA in tests/blend_ref.py.

Every case is THRESHOLD-FREE (no (pixel, entry) pair within 1e-3 of alpha = 1/255, test_T = 1e-4, T = 0.5, the 0.99 clamp, or
within 1e-5 of power = 0: tests/test_blend_ref.py checks it on the CPU), so both sides take the same branches: n_contrib,
qlast and observe are compared with array_equal, the floats element-wise with ZERO exceptions and no proofs.

Bounds: FACTOR = 4 times the error of the fp32 restatement (the reference's written order of operations) against float64,
measured over the cases by tests/test_blend_ref.py and recorded in blend_ref.py, each relative to |ref| + 1e-6 max:
    colour and buffer  E_IMAGE     = 8.1e-7  -> 3.2e-6
    final_T            E_FINAL_T   = 4.5e-6  -> 1.8e-5   (set by the clamp case: 1 - alpha at alpha = 0.99)
    rows, per element  E_ROWS      = 3.4e-2  -> 1.4e-1   (set by ONE element of the 40-tile case that cancels to 1e-5 of its row)
    rows, per column   E_ROWS_NORM = 1.8e-6  -> 7.2e-6   (||got - ref|| / ||ref|| of each of the 11 + fc columns of a case)
The element-wise row figure is the one the cases' worst-conditioned element dictates, so the column norm-wise figure is
asserted beside it: it is at rounding level and is what a kernel that is slightly wrong on a few pairs cannot meet.
The 330-entry list is held to north_star's bound, |a - b| <= 1e-3 |b| + 1e-5 rms, zero exceptions, and prints the error of the
FRONT entry's dL/dopacity and dL/dconic for the kernel and for the fp32 restatement side by side, at several truncations.

Guard words lie in front of and behind every output buffer, and every second row of the row buffer is a guard row."""
import numpy as np
import pytest
import torch

import blend_ref as R

pytestmark = pytest.mark.gpu

GUARD = 1024
PATTERN = np.uint32(0xA5C3F00D)


def _dev(a, dtype=np.uint32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).view(np.int32).reshape(-1).copy()).cuda()


class Guarded:
    """`words` words (the pattern, or zeros) with GUARD pattern words in front and behind"""

    def __init__(self, words, zero=False):
        a = np.full(words + 2 * GUARD, PATTERN, np.uint32)
        if zero:
            a[GUARD:GUARD + words] = 0
        self.words, self.t = words, _dev(a)
        self.ptr = self.t.data_ptr() + 4 * GUARD

    def inside(self, dtype=np.uint32):
        return self.t[GUARD:GUARD + self.words].cpu().numpy().view(dtype)

    def guards_intact(self):
        g = self.t.cpu().numpy().view(np.uint32)
        return bool(np.all(g[:GUARD] == PATTERN) and np.all(g[GUARD + self.words:] == PATTERN))


def _inputs(c):
    return dict(bg=_dev(c.bg, np.float32), ranges=_dev(c.ranges), qlist=_dev(c.qlist), qcount=_dev(c.qcount), qrow=_dev(c.qrow),
                rec=_dev(c.rec, np.float32))


def gpu_forward(c, inp=None):
    import gs2m_native
    inp = inp or _inputs(c)
    HW = c.W * c.H
    o = dict(color=Guarded(3 * HW), buffer=Guarded(R.NUM_FEATURES * HW), final_T=Guarded(HW), n_contrib=Guarded(HW),
             observe=Guarded(c.P, zero=True), qlast=Guarded(4 * c.tiles))
    gs2m_native.launch("gs2m_debug_blend_forward", torch.device("cuda", torch.cuda.current_device()), c.W, c.H, c.fc, inp["bg"].data_ptr(),
                       inp["ranges"].data_ptr(), inp["qlist"].data_ptr(), inp["qcount"].data_ptr(), inp["rec"].data_ptr(), o["color"].ptr,
                       o["buffer"].ptr, o["final_T"].ptr, o["n_contrib"].ptr, o["observe"].ptr, o["qlast"].ptr)
    torch.cuda.synchronize()
    for k, g in o.items():
        assert g.guards_intact(), f"{c.name}: guard words of {k} were written"
    return dict(color=o["color"].inside(np.float32).reshape(3, c.H, c.W), buffer=o["buffer"].inside(np.float32).reshape(-1, c.H, c.W),
                final_T=o["final_T"].inside(np.float32).reshape(c.H, c.W), n_contrib=o["n_contrib"].inside().reshape(c.H, c.W),
                observe=o["observe"].inside(np.int32), qlast=o["qlast"].inside())


def gpu_backward(c, f64, inp=None):
    """the kernel on the REFERENCE's forward state (final_T rounded to fp32, n_contrib, qlast): the backward alone -> (rows, raw words)"""
    import gs2m_native
    inp = inp or _inputs(c)
    rowf = gs2m_native.lib().gs2m_debug_row_floats(c.fc)
    assert rowf >= R.ROW_FEAT + c.fc and rowf % 4 == 0
    rows = Guarded(c.n_rows * rowf)
    st = [_dev(f64["qlast"]), _dev(f64["final_T"], np.float32), _dev(f64["n_contrib"]), _dev(c.grad_color, np.float32), _dev(c.grad_buffer, np.float32)]
    gs2m_native.launch("gs2m_debug_blend_backward", torch.device("cuda", torch.cuda.current_device()), c.W, c.H, c.fc, inp["bg"].data_ptr(),
                       inp["ranges"].data_ptr(), inp["qlist"].data_ptr(), inp["qcount"].data_ptr(), inp["qrow"].data_ptr(), st[0].data_ptr(),
                       inp["rec"].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr(), st[4].data_ptr(), rows.ptr)
    torch.cuda.synchronize()
    assert rows.guards_intact(), f"{c.name}: guard words of the rows were written"
    raw = rows.inside().reshape(c.n_rows, rowf)
    return raw.view(np.float32), raw


def _within(name, got, ref, scale, e):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.all(np.isfinite(got)), f"{name}: non-finite"
    err = R.rel_err(got, ref, scale)
    print(f"{name}: {err:.3e} (restatement figure {e:.2e}, bound {R.FACTOR * e:.2e})")
    assert err <= R.FACTOR * e, f"{name}: element-wise error {err:.3e} beyond {R.FACTOR} x {e:.2e}"


def check_forward(c, f64, got):
    name = c.name
    v = f64["qvalid"]
    assert np.array_equal(got["n_contrib"], f64["n_contrib"]), f"{name}: n_contrib"
    assert np.array_equal(got["qlast"][v], f64["qlast"][v]), f"{name}: qlast {got['qlast'][v]} != {f64['qlast'][v]}"
    assert np.all(got["qlast"][~v] == PATTERN), f"{name}: qlast of a quadrant without pixels was written"
    assert np.array_equal(got["observe"], f64["observe"]), f"{name}: observe"
    assert np.all(got["buffer"][c.fc:] == 0), f"{name}: an unused buffer channel is not 0"
    _within(f"{name} final_T", got["final_T"], f64["final_T"], np.abs(f64["final_T"]).max(), R.E_FINAL_T)
    _within(f"{name} colour", got["color"], f64["color"], np.abs(f64["color"]).max(), R.E_IMAGE)
    if c.fc:
        _within(f"{name} buffer", got["buffer"][:c.fc], f64["buffer"][:c.fc], np.abs(f64["buffer"]).max(), R.E_IMAGE)


def check_rows_layout(c, qlast, rows, raw):
    """every row a list entry owns is written, zeros behind qlast and in the padding; no other row is touched"""
    name, NV, u = c.name, R.ROW_FEAT + c.fc, c.used_rows
    guards = np.setdiff1d(np.arange(c.n_rows), u)
    assert np.all(raw[guards] == PATTERN), f"{name}: guard rows {guards[np.any(raw[guards] != PATTERN, axis=1)][:8]} were written"
    assert not np.any(raw[u] == PATTERN), f"{name}: rows {u[np.any(raw[u] == PATTERN, axis=1)][:8]} were not (completely) written"
    assert np.all(raw[u][:, NV:] == 0), f"{name}: row padding is not 0"
    # (an entry in front of qlast that reaches no pixel has a row of zeros too, of either sign: those are compared as numbers)
    behind = np.concatenate([r[int(qlast[4 * t + q]):] for t, q, box, base, ent, r in c.quads] + [np.zeros(0, np.int64)])
    assert np.all(raw[behind] == 0), f"{name}: rows behind a quadrant's last contributor are not exactly zero"
    assert np.all(np.isfinite(rows[u]))


@pytest.mark.parametrize("name", list(R.BUILDERS))
def test_forward(name):
    c, f64 = R.reference(name)[:2]
    check_forward(c, f64, gpu_forward(c))


@pytest.mark.parametrize("name", R.SHORT_CASES)
def test_backward(name):
    c, f64, r64 = R.reference(name)[:3]
    inp = _inputs(c)
    rows, raw = gpu_backward(c, f64, inp)
    check_rows_layout(c, f64["qlast"], rows, raw)
    assert np.array_equal(raw, gpu_backward(c, f64, inp)[1]), f"{name}: two runs differ"
    u, NV = c.used_rows, R.ROW_FEAT + c.fc
    if len(u) == 0:
        return
    got = rows[u][:, :NV]
    _within(f"{name} rows", got, r64[u], np.abs(r64[u]).max(axis=1, keepdims=True), R.E_ROWS)
    nerr = R.rows_norm_err(got, r64[u])
    print(f"{name} rows, column norm-wise: {nerr:.3e} (restatement figure {R.E_ROWS_NORM:.2e})")
    assert nerr <= R.FACTOR * R.E_ROWS_NORM, f"{name}: a column of the rows is {nerr:.3e} off in norm"


def test_backward_on_the_forward_kernels_own_state():
    """the pair as a frame runs it: the backward on what the forward kernel wrote (the 40-tile case)"""
    c, f64, r64 = R.reference("many_tiles")[:3]
    got = gpu_forward(c)
    state = dict(f64, final_T=got["final_T"], n_contrib=got["n_contrib"], qlast=np.where(f64["qvalid"], got["qlast"], 0))
    rows, raw = gpu_backward(c, state)
    check_rows_layout(c, f64["qlast"], rows, raw)
    assert R.rows_norm_err(rows[c.used_rows][:, :R.ROW_FEAT + c.fc], r64[c.used_rows]) <= R.FACTOR * R.E_ROWS_NORM


def _north_star(name, got, ref):
    worst = 0.0
    for a, b in R.ROW_GROUPS:
        g, r = got[:, a:b].astype(np.float64), ref[:, a:b]
        nz = r[r != 0]
        rms = float(np.sqrt(np.mean(nz * nz))) if nz.size else 0.0
        ratio = np.abs(g - r) / (1e-3 * np.abs(r) + 1e-5 * rms + 1e-300)
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1.0), f"{name}: columns {a}:{b}: {np.count_nonzero(ratio > 1)} elements outside 1e-3 |ref| + 1e-5 rms, worst {ratio.max():.2f} x the bound"
    return worst


def test_backward_one_long_list():
    c, f64, r64, f32, r32 = R.reference("long")
    rows, raw = gpu_backward(c, f64)
    check_rows_layout(c, f64["qlast"], rows, raw)
    assert np.array_equal(raw, gpu_backward(c, f64)[1]), "two runs differ"
    u, NV = c.used_rows, R.ROW_FEAT + c.fc
    worst = _north_star("long", rows[u][:, :NV], r64[u])
    print(f"long list, 330 entries: worst element at {worst:.3f} of north_star's bound; column norm-wise {R.rows_norm_err(rows[u][:, :NV], r64[u]):.3e} "
          f"(fp32 restatement {R.rows_norm_err(r32[u], r64[u]):.3e})")
    # the front entry (the large low-opacity splat): dL/dopacity and the conic terms, kernel and fp32 restatement side by side,
    # on the list cut to its first n entries
    print("front entry, relative error against float64:   n | kernel: dopacity, conic xx, xy, yy | fp32 restatement: the same")
    for n in (16, 17, 48, 100, 200, 330):
        t = c if n == 330 else R.truncated(c, n)
        t64 = R.forward(t)
        tr64 = R.backward(t, t64)
        tr32 = R.backward(t, R.forward(t, np.float32), np.float32)
        tg = gpu_backward(t, t64)[0]
        row = int(t.quads[0][5][0])
        rel = lambda a: np.abs(a[row, [7, 4, 5, 6]].astype(np.float64) - tr64[row, [7, 4, 5, 6]]) / np.abs(tr64[row, [7, 4, 5, 6]])
        print(f"    {n:4d} | " + " ".join(f"{x:.2e}" for x in rel(tg)) + " | " + " ".join(f"{x:.2e}" for x in rel(tr32)))


def test_hooks_validate_their_arguments():
    import gs2m_native
    L = gs2m_native.lib()
    d = torch.zeros(64, dtype=torch.int32, device="cuda").data_ptr()
    s = gs2m_native.stream_ptr()
    assert L.gs2m_debug_blend_forward(0, 8, 0, d, d, d, d, d, d, d, d, d, d, d, s) == -1
    assert L.gs2m_debug_blend_forward(8, 8, 11, d, d, d, d, d, d, d, d, d, d, d, s) == -1
    assert L.gs2m_debug_blend_forward(8, 8, 0, d, d, d, d, None, d, d, d, d, d, d, s) == -1
    assert L.gs2m_debug_blend_backward(8, 0, 0, d, d, d, d, d, d, d, d, d, d, d, d, s) == -1
    assert L.gs2m_debug_blend_backward(8, 8, -1, d, d, d, d, d, d, d, d, d, d, d, d, s) == -1
    assert L.gs2m_debug_blend_backward(8, 8, 0, d, d, d, d, d, d, d, d, d, d, d, None, s) == -1
    assert L.gs2m_debug_row_floats(11) == -1 and [L.gs2m_debug_row_floats(k) for k in (0, 1, 2, 5, 6, 9, 10)] == [12, 12, 16, 16, 20, 20, 24]
