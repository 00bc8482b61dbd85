"""The cube-map prefilter kernels (csrc/cubemap.hip) alone, on every dispatch route, against tests/cubemap_ref.py.

Every specular case first asserts, through gs2m_specular_cubemap_route, the kernel it means to run: specular_kernel with 1,
16 or 64 lanes per output, specular_tile_kernel with 8 or 4 waves per tile, and the fallback from the tile kernel when the
output is not 16-byte aligned.  The core are the probes: an input (or gradient) that is zero but for one texel per channel
makes the kernel write one column (row) of the weight matrix with no summation error, so every pair (output, texel) is
checked on its own: a pair surely outside the cone must be exactly 0.0, a pair surely inside within its own bound, a pair
within fp32 rounding of the cutoff (RIM) either, with no exception budget; forward column and backward row of a texel must
have the identical support, rim pairs included (the kernels' own contract: L . V is bit-identical whichever texel plays
the output).  The classes and bounds are derived in cubemap_ref's docstring; tests/test_cubemap_ref.py shows on the CPU
that rim pairs are a small share of every probe set and that the shapes contain the culling boxes they are meant to.
The dense tests then bound ordinary sums: sure - tol <= got <= sure + rim + tol with tol the per-pair bounds plus
n 2^-24 sum |w x| for any order of an n-term sum, for every row -- none is skipped.  Every test prints its worst err / bound."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cubemap_ref as R  # noqa: E402

U = R.U
INVALID = -1   # GS2M_ERR_INVALID_ARG
ALIGNED = [s for s in R.SHAPES if s[4]]
UNALIGNED = [s for s in R.SHAPES if not s[4]]


def _native():
    import gs2m_native
    return gs2m_native


def _table(N):
    import render_utils as RU
    return RU._texel_table(N, torch.device("cuda", torch.cuda.current_device()))


def _buffer(n, aligned):
    """n floats on the device whose address is 16-byte aligned, or 4 bytes past such an address"""
    buf = torch.zeros(n + 4, device="cuda")
    out = buf[4:4 + n] if aligned else buf[1:1 + n]
    assert (out.data_ptr() & 15 == 0) == bool(aligned)
    return out


def _specular(shape, inp, backward):
    """one raw C call; asserts the route first.  inp: (T, 3) forward, (T, 4) backward; -> (T, 4) or (T, 3)"""
    N, r, cutoff, route, aligned = shape
    nat = _native()
    cc = R.cos_cut_of(r, cutoff)
    T = 6 * N * N
    out = _buffer(T * (3 if backward else 4), aligned)
    assert nat.lib().gs2m_specular_cubemap_route(N, cc, int(out.data_ptr() & 15 == 0)) == route, "the thresholds moved: this case no longer runs the kernel it is about"
    assert inp.is_contiguous() and inp.shape == (T, 4 if backward else 3)
    nat.launch("gs2m_specular_cubemap_backward" if backward else "gs2m_specular_cubemap_forward", inp.device, N, float(r), cc, _table(N).data_ptr(),
               inp.data_ptr(), out.data_ptr())
    res = out.view(T, -1)
    assert bool(torch.isfinite(res).all())
    return res


def _sparse(col):
    nz = col.nonzero().view(-1)
    return nz.cpu().numpy(), col[nz].cpu().double().numpy()


@functools.lru_cache(maxsize=None)
def _probe_run(shape):
    """{texel: ((fwd support, values), (bwd support, values))} of every probe texel of the shape, three probes per launch,
    and the forward's weight-sum channel"""
    N = shape[0]
    T = 6 * N * N
    res, wsum = {}, None
    for trio in R.probe_texels(N):
        x = torch.zeros(T, 3, device="cuda")
        G = torch.zeros(T, 4, device="cuda")
        for c, t in enumerate(trio):
            x[t, c] = 1.0
            G[t, c] = 1.0
        raw, grad = _specular(shape, x, False), _specular(shape, G, True)
        if wsum is None:
            wsum = raw[:, 3].clone()
        assert torch.equal(raw[:, 3], wsum), "the weight sum does not depend on the input"
        for c, t in enumerate(trio):
            res[t] = (_sparse(raw[:, c]), _sparse(grad[:, c]))
    return res


def _check_probe(p, nz, val, what):
    """the three rules for one column / row; -> worst err / bound"""
    extra = np.setdiff1d(nz, p.idx)
    assert extra.size == 0, f"{what}: non-zero weight for pairs surely outside the cone: texels {extra[:8]}"
    got = np.zeros(len(p.idx))
    got[np.searchsorted(p.idx, nz)] = val
    must = (p.cls == R.IN) | (got != 0.0)
    ratio = np.abs(got - p.w)[must] / p.bound[must]
    k = int(np.argmax(ratio)) if ratio.size else 0
    assert (ratio <= 1.0).all(), (f"{what}: texel {p.idx[must][k]} d {p.d[must][k]:.9f} class {p.cls[must][k]} got {got[must][k]:.9e} want {p.w[must][k]:.9e} "
                                  f"bound {p.bound[must][k]:.3e}")
    return float(ratio.max()) if ratio.size else 0.0


def _shape_args(shape):
    N, r, cutoff = shape[:3]
    return N, R.f32(r), R.cos_cut_of(r, cutoff)


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_forward_probes_pair_by_pair(shape):
    N, r, cc = _shape_args(shape)
    worst = rims = 0
    for t, ((nz, val), _) in _probe_run(shape).items():
        p = R.column_pairs(N, r, cc, t)
        worst = max(worst, _check_probe(p, nz, val, f"forward column of texel {t}"))
        rims += p.n_rim
    print(f"{R.shape_id(shape)} route {shape[3]}: forward probes worst err / bound {worst:.3f}, {rims} rim pairs")


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_backward_probes_pair_by_pair(shape):
    N, r, cc = _shape_args(shape)
    worst = 0
    for o, (_, (nz, val)) in _probe_run(shape).items():
        worst = max(worst, _check_probe(R.row_pairs(N, r, cc, o), nz, val, f"backward row of texel {o}"))
    print(f"{R.shape_id(shape)} route {shape[3]}: backward probes worst err / bound {worst:.3f}")


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_forward_and_backward_accept_the_same_pairs(shape):
    """no tolerance: {o : W[o, a] != 0} from the forward equals {t : W[a, t] != 0} from the backward with G = e_a"""
    n = 0
    for a, ((fnz, _), (bnz, _)) in _probe_run(shape).items():
        assert np.array_equal(fnz, bnz), (a, np.setxor1d(fnz, bnz)[:8])
        n += len(fnz)
    print(f"{R.shape_id(shape)}: {n} accepted pairs, identical both ways")


@pytest.mark.parametrize("shape", UNALIGNED, ids=R.shape_id)
def test_unaligned_fallback_accepts_the_tile_kernels_pairs(shape):
    N, r, cc = _shape_args(shape)
    tile = next(s for s in ALIGNED if s[:3] == shape[:3])
    assert tile[3] in (R.TILE8, R.TILE4) and shape[3] in (R.TPO16, R.TPO64)
    a_run, b_run = _probe_run(tile), _probe_run(shape)
    worst = 0.0
    for t in a_run:
        for k, p in ((0, R.column_pairs(N, r, cc, t)), (1, R.row_pairs(N, r, cc, t))):
            (anz, av), (bnz, bv) = a_run[t][k], b_run[t][k]
            assert np.array_equal(anz, bnz), (t, k, np.setxor1d(anz, bnz)[:8])
            ratio = np.abs(av - bv) / (2.0 * p.bound[np.searchsorted(p.idx, anz)])
            assert (ratio <= 1.0).all()
            worst = max(worst, float(ratio.max()))
    print(f"{R.shape_id(shape)}: tile route vs fallback worst difference / (2 bound) {worst:.3f}")


# ------------------------------------------------------------------------------------------------ dense sums
def _rows(N, seed):
    T = 6 * N * N
    if N <= 65:
        return np.arange(T)
    special = [0, N - 1, N * N - 1, (N // 2) * N + N // 2, 3 * N * N + 5, 5 * N * N + (N - 1) * N, 2 * N * N + 7 * N + N - 1, T - 1]
    rnd = np.random.RandomState(seed).choice(T, 40, replace=False)
    rows = list(dict.fromkeys(special + [int(v) for v in rnd]))[:24]
    assert len(rows) == 24
    return np.array(sorted(rows))


def _dense_bounds(k, n_rows, cls, w, bound, v, signed):
    """per row: (lo, hi) of sum_pairs w v with the rim pairs either way; signed: v may be negative"""
    n = np.bincount(k, minlength=n_rows)
    wv = w * v
    sure = np.bincount(k, weights=wv * (cls == R.IN), minlength=n_rows)
    tol = np.bincount(k, weights=bound * np.abs(v), minlength=n_rows) + n * U * np.bincount(k, weights=np.abs(wv), minlength=n_rows)
    rim = np.bincount(k, weights=np.abs(wv) * (cls == R.RIM), minlength=n_rows)
    return (sure - rim - tol, sure + rim + tol) if signed else (sure - tol, sure + rim + tol)   # x >= 0: a rim pair can only add


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_dense_forward_and_backward_every_row(shape):
    """random x in [0, 1) and G ~ N(0, 1): forward sure - tol <= got <= sure + rim + tol per output and channel (the 4th
    is the weight sum), backward |got - sure| <= sum over rim |w G| + tol per texel and channel; every row of a level up
    to 65^2, 24 rows (special texels and random ones) of a larger one.  Both directions from one pass over the pairs."""
    N, r, cc = _shape_args(shape)
    T = 6 * N * N
    g = torch.Generator().manual_seed(7 * N + int(1000 * r))
    x = torch.rand(T, 3, generator=g)
    G = torch.randn(T, 4, generator=g)
    fwd = _specular(shape, x.cuda(), False).cpu().double().numpy()
    bwd = _specular(shape, G.cuda(), True).cpu().double().numpy()
    xv = np.concatenate([x.double().numpy(), np.ones((T, 1))], axis=1)
    Gv = G.double().numpy()
    rows = _rows(N, N)
    chunk = max(1, (1 << 22) // T)
    worst, checked, rim_rows = [0.0, 0.0], 0, 0
    for s in range(0, len(rows), chunk):
        rr = rows[s:s + chunk]
        k, idx, d, cls, w_row, b_row, w_col, b_col = R.pairs_flat(N, r, cc, rr, False, both=True)
        rim_rows += int((np.bincount(k, weights=(cls == R.RIM), minlength=len(rr)) > 0).sum())
        for which, got_all, w, bound, v, nc in ((0, fwd, w_row, b_row, xv, 4), (1, bwd, w_col, b_col, Gv, 3)):
            for c in range(nc):
                lo, hi = _dense_bounds(k, len(rr), cls, w, bound, v[idx, c], signed=bool(which))
                got = got_all[rr, c]
                bad = (got < lo) | (got > hi)
                j = int(np.argmax(bad))
                assert not bad.any(), (("forward", "backward")[which], int(rr[j]), c, got[j], lo[j], hi[j])
                worst[which] = max(worst[which], float((np.abs(got - 0.5 * (lo + hi)) / np.maximum(0.5 * (hi - lo), 1e-300)).max()))
        checked += len(rr)
    assert checked == len(rows)
    print(f"{R.shape_id(shape)} route {shape[3]}: {checked} rows ({rim_rows} with a rim pair), worst err / bound forward {worst[0]:.3f} backward {worst[1]:.3f}")


# ------------------------------------------------------------------------------------------------ the other kernels
E_C = 24.0 * U   # clamp(N . L): fp32 face coordinates (3u each, a turn of <= 4.3u per direction), sqrt and divide of the
                 # normalisation (4u per component, 8u for the product of two), the three-term dot product (3u)


@pytest.mark.parametrize("N", [1, 2, 3, 5, 16, 17])
def test_diffuse_forward_and_backward(N):
    """|got - W x| <= (6 N^2 / 64 + 8) 2^-24 sum |w x| (64 lanes stride over the inputs, then a 6-step butterfly) + sum
    |dw| |x|, dw = (E_C + c (area_rel + 3u)) area / pi: the clamp is 1-Lipschitz, so a pair at either of its edges (0 and
    0.999) needs no class of its own; the pairs it does clamp at 0.999 are counted."""
    nat = _native()
    T = 6 * N * N
    g = torch.Generator().manual_seed(N)
    x, G = torch.rand(T, 3, generator=g), torch.randn(T, 3, generator=g)
    W = R.diffuse_matrix(N)
    from oracle import cubemap_oracle as O
    d = O.texel_dirs(N)
    dots = d @ d.T
    clamped = int((dots >= 0.999 + E_C).sum())
    assert clamped >= T, "every self pair is clamped at 0.999"
    area = R.texel_areas(N)
    dW = 1.01 * (E_C + np.clip(dots, 0.0, 0.999) * (R.area_rel(N)[None, :] + 3 * U)) * area[None, :] / 3.141592
    worst = 0.0
    for name, inp, M, dM in (("forward", x, W, dW), ("backward", G, W.T, dW.T)):
        out = torch.empty(T, 3, device="cuda")
        nat.launch(f"gs2m_diffuse_cubemap_{name}", out.device, N, inp.cuda().data_ptr(), out.data_ptr())
        v = inp.double().numpy()
        want = M @ v
        bound = (T / 64 + 8) * U * (np.abs(M) @ np.abs(v)) + dM @ np.abs(v)
        ratio = np.abs(out.cpu().double().numpy() - want) / bound
        assert (ratio <= 1.0).all(), (name, np.unravel_index(np.argmax(ratio), ratio.shape), ratio.max())
        worst = max(worst, float(ratio.max()))
    print(f"diffuse N={N}: {clamped} of {T * T} pairs clamped at 0.999, worst err / bound {worst:.3f}")


@pytest.mark.parametrize("N", [1, 2, 3, 16, 63, 512])
def test_texel_table(N):
    """atanf((k + 1) / h) - atanf(k / h) against float64 atan: each atanf within ATANF_ULP ulp of its value plus the
    rounding of its argument, the difference rounded once (cubemap_ref.axis_table) -- the figure the weight bounds use"""
    tab = torch.full((N + 1,), -7.0, device="cuda")
    _native().launch("gs2m_cubemap_texel_table", tab.device, N, tab.data_ptr())
    got = tab.cpu().double().numpy()
    ax, err = R.axis_table(N)
    assert got[N] == -7.0
    if N == 1:
        assert got[0] == 1.0
        return
    ratio = np.abs(got[:N] - ax) / err
    print(f"texel table N={N}: worst err / bound {ratio.max():.3f}")
    assert (ratio <= 1.0).all()


@pytest.mark.parametrize("shape", [R.SHAPES[4], R.SHAPES[12], R.SHAPES[10]], ids=R.shape_id)
def test_normalized_pair_is_the_plain_pair_bitwise(shape):
    N, r, cc = _shape_args(shape)
    nat = _native()
    T = 6 * N * N
    if (N, shape[1]) == (24, 0.08):
        assert len(R.row_pairs(N, r, cc, 5 * N + 7).idx) == 1, "an output whose cone holds only the self pair"
    g = torch.Generator().manual_seed(N)
    x, g3 = torch.rand(T, 3, generator=g).cuda(), torch.randn(T, 3, generator=g).cuda()
    raw, out = _buffer(4 * T, True), torch.empty(T, 3, device="cuda")
    nat.launch("gs2m_specular_cubemap_normalized_forward", x.device, N, float(shape[1]), cc, _table(N).data_ptr(), x.data_ptr(), raw.data_ptr(), out.data_ptr())
    raw = raw.view(T, 4)
    assert torch.equal(raw, _specular(shape, x, False))
    assert bool((raw[:, 3] > 0).all()) and torch.equal(out, raw[:, :3] / raw[:, 3:])
    scratch, grad = _buffer(4 * T, True), _buffer(3 * T, True)
    nat.launch("gs2m_specular_cubemap_normalized_backward", x.device, N, float(shape[1]), cc, _table(N).data_ptr(), raw.data_ptr(), g3.data_ptr(),
               scratch.data_ptr(), grad.data_ptr())
    g4 = torch.cat([g3 / raw[:, 3:], torch.zeros(T, 1, device="cuda")], dim=1).contiguous()
    assert torch.equal(scratch.view(T, 4), g4)
    assert torch.equal(grad.view(T, 3), _specular(shape, g4, True))


@pytest.mark.parametrize("shape", [R.SHAPES[3], R.SHAPES[7], R.SHAPES[8], R.SHAPES[12], R.SHAPES[16]] + UNALIGNED, ids=R.shape_id)
def test_two_runs_are_bitwise_equal(shape):
    N = shape[0]
    T = 6 * N * N
    g = torch.Generator().manual_seed(N)
    x, G = torch.rand(T, 3, generator=g).cuda(), torch.randn(T, 4, generator=g).cuda()
    assert torch.equal(_specular(shape, x, False), _specular(shape, x, False))
    assert torch.equal(_specular(shape, G, True), _specular(shape, G, True))


def test_every_route_is_among_the_bitwise_cases():
    cases = [R.SHAPES[3], R.SHAPES[7], R.SHAPES[8], R.SHAPES[12], R.SHAPES[16]]
    assert sorted(s[3] for s in cases) == [0, 1, 2, 3, 4]


def test_argument_rejections_launch_nothing():
    L = _native().lib()
    N, T = 8, 6 * 64
    s = _native().stream_ptr()
    keep = torch.full((4 * T + 8,), -3.0, device="cuda")
    a, b = torch.zeros(4 * T + 8, device="cuda"), torch.zeros(4 * T + 8, device="cuda")
    tab = _table(N).data_ptr()
    o, pa, pb = keep.data_ptr(), a.data_ptr(), b.data_ptr()
    assert o % 16 == 0 and pa % 16 == 0 and pb % 16 == 0
    rcs = [L.gs2m_diffuse_cubemap_forward(0, pa, o, s), L.gs2m_diffuse_cubemap_forward(1025, pa, o, s), L.gs2m_diffuse_cubemap_backward(1025, pa, o, s),
           L.gs2m_diffuse_cubemap_forward(N, None, o, s), L.gs2m_diffuse_cubemap_backward(N, pa, None, s),
           L.gs2m_cubemap_texel_table(0, o, s), L.gs2m_cubemap_texel_table(4097, o, s), L.gs2m_cubemap_texel_table(N, None, s),
           L.gs2m_specular_cubemap_forward(0, 0.5, 0.9, tab, pa, o, s), L.gs2m_specular_cubemap_forward(4097, 0.5, 0.9, tab, pa, o, s),
           L.gs2m_specular_cubemap_forward(N, 0.5, 0.9, None, pa, o, s), L.gs2m_specular_cubemap_forward(N, 0.5, 0.9, tab, None, o, s),
           L.gs2m_specular_cubemap_forward(N, 0.5, 0.9, tab, pa, None, s),
           L.gs2m_specular_cubemap_backward(4097, 0.5, 0.9, tab, pa, o, s), L.gs2m_specular_cubemap_backward(N, 0.5, 0.9, tab, None, o, s),
           L.gs2m_specular_cubemap_normalized_forward(N, 0.5, 0.9, tab, pa, o + 4, pb, s),
           L.gs2m_specular_cubemap_normalized_forward(N, 0.5, 0.9, tab, pa, None, pb, s),
           L.gs2m_specular_cubemap_normalized_backward(N, 0.5, 0.9, tab, pa + 4, pb, o, o, s),
           L.gs2m_specular_cubemap_normalized_backward(N, 0.5, 0.9, tab, pa, pb, o + 8, o, s),
           L.gs2m_specular_cubemap_normalized_backward(N, 0.5, 0.9, tab, pa, pb, None, o, s),
           L.gs2m_specular_cubemap_normalized_backward(4097, 0.5, 0.9, tab, pa, pb, o, o, s)]
    assert rcs == [INVALID] * len(rcs), rcs
    torch.cuda.synchronize()
    assert bool((keep == -3.0).all()) and bool((b == 0).all()), "a refused call wrote to its output"
