"""grid_border_kernel<C, BWD, MODE> and det_finalize_kernel of csrc/mvs.hip alone: forward, d_grid and d_img per element against the
float64 restatement of tests/patch_ncc_ref.py (`grid_reference`: un-normalise, clip with the position gradient zeroed where the
clip binds, NaN as the clip at 0, bilinear lookup, exact dense scatter), in both scatter modes, for every channel count and for
images of one row, one column and one texel.  Bound: |got - f64| <= K e per element, K = 3 x the float32 yardstick's worst ratio
(patch_ncc_ref.RATIO); the exact-lattice, one-texel and workspace tests have no tolerance at all.
"""
import numpy as np
import pytest
import torch

import patch_ncc_ref as R

pytestmark = pytest.mark.gpu


def _run(img, grid, d_out, det=True, want_img=True, want_grid=True):
    """-> out, d_grid, d_img (numpy; None where not requested) through the raw entry points."""
    import gs2m_mvs as MV
    import gs2m_native as NV
    C, H, W = img.shape
    N = len(grid)
    dev = torch.device("cuda")
    ti, tg, td = (torch.tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda() for a in (img, grid, d_out))
    out = torch.full((N + 8, C), -5.5, device=dev)
    NV.launch("gs2m_grid_sample_border_forward", dev, N, C, H, W, ti.data_ptr(), tg.data_ptr(), out.data_ptr())
    d_img = torch.zeros_like(ti) if want_img else None
    d_grid = torch.full((N + 8, 2), -5.5, device=dev) if want_grid else None
    try:
        MV.set_deterministic(det)
        NV.launch("gs2m_grid_sample_border_backward", dev, N, C, H, W, ti.data_ptr(), tg.data_ptr(), td.data_ptr(), NV.ptr(d_img), NV.ptr(d_grid))
    finally:
        MV.set_deterministic(True)
    torch.cuda.synchronize()
    assert bool((out[N:] == -5.5).all()) and (d_grid is None or bool((d_grid[N:] == -5.5).all())), "wrote beyond N"
    return out[:N].cpu().numpy(), None if d_grid is None else d_grid[:N].cpu().numpy(), None if d_img is None else d_img.cpu().numpy()


def _check(img, grid, d_out, det, label):
    r = R.grid_reference(img, grid, d_out)
    out, dg, di = _run(img, grid, d_out, det)
    none = np.zeros(len(grid), dtype=bool)
    worst = {}
    for name, q in (("grid_out", R.ratios(out, r.out, r.e_out, none)), ("d_grid", R.ratios(dg, r.d_grid, r.e_dgrid, r.flip)),
                    ("d_img", R.ratios(di, r.d_img, r.e_img, np.zeros(di.shape, dtype=bool)))):
        worst[name] = float(np.nanmax(q)) / R.K[name][0] if not np.isnan(q).all() else 0.0
    print(label, {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), (label, worst)
    nan = np.isnan(grid)
    assert (dg[nan] == 0).all(), "NaN position: zero position gradient"
    assert (dg[r.binds & ~r.flip[:, None]] == 0).all(), "the clip zeroes the position gradient where it binds"
    return r, out, dg, di


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "float_atomics"])
@pytest.mark.parametrize("N", R.GRID_COUNTS)
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_every_element_every_channel_count(C, N, det):
    """37 x 53, N = 1, 255, 256, 257 (around one workgroup), 1000: positions inside, beyond both sides, exactly +-1, on cell lines,
    NaN and infinite; upstream gradients with exact zeros."""
    assert torch.cuda.is_available()
    img, grid, d_out = R.grid_case(C, 37, 53)
    _check(img, grid[:N], d_out[:N], det, f"C {C} N {N} {'det' if det else 'float'}")


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "float_atomics"])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("H,W", [(1, 9), (9, 1), (1, 1)])
def test_one_row_one_column_one_texel(H, W, C, det):
    """The second row / column does not exist: its weight is 0 and it is never read; an axis of one texel has no position gradient."""
    assert torch.cuda.is_available()
    img, grid, d_out = R.grid_case(C, H, W)
    r, out, dg, di = _check(img, grid, d_out, det, f"{H} x {W} C {C}")
    if W == 1:
        assert (dg[:, 0] == 0).all()
    if H == 1:
        assert (dg[:, 1] == 0).all()
    if H == 1 and W == 1:
        assert np.array_equal(out, np.broadcast_to(img.reshape(1, C), out.shape))


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "float_atomics"])
@pytest.mark.parametrize("C", [2, 3])
def test_either_gradient_may_be_null(C, det):
    """dL_dimage = NULL (then no workspace is touched) and dL_dgrid = NULL: the other gradient has the same bits as with both."""
    assert torch.cuda.is_available()
    img, grid, d_out = R.grid_case(C, 37, 53)
    _, dg, di = _run(img, grid, d_out, det)
    _, dg2, none = _run(img, grid, d_out, det, want_img=False)
    assert none is None and np.array_equal(dg.view(np.uint32), dg2.view(np.uint32))
    _, none, di2 = _run(img, grid, d_out, det, want_grid=False)
    assert none is None
    if det:
        assert np.array_equal(di.view(np.uint32), di2.view(np.uint32))
    else:
        r = R.grid_reference(img, grid, d_out)
        assert np.nanmax(R.ratios(di2, r.d_img, r.e_img, np.zeros(di2.shape, dtype=bool))) <= R.K["d_img"][0]


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "float_atomics"])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_exact_lattice_is_bit_equal_to_float64(C, det):
    """33 x 17, positions on multiples of 1/16 pixel, values and upstream gradients k 2^-10 (|k| <= 64; sum |k| per texel below
    2^24 in units of the products: asserted on the CPU, tests/test_patch_ncc_ref.py): every float32 operation is exact, so the
    forward, d_grid and d_img -- in both modes, in any order of the additions -- are the float64 results rounded once."""
    assert torch.cuda.is_available()
    img, grid, d_out = R.lattice_case(C)
    r = R.grid_reference(img, grid, d_out)
    out, dg, di = _run(img, grid, d_out, det)
    f = lambda a: a.astype(np.float32)
    assert np.array_equal(out, f(r.out)) and np.array_equal(di, f(r.d_img))
    assert np.array_equal(dg, f(r.d_grid))   # (exactly on a clip limit the contract is the kernel's: x <= 0 and x >= W - 1 bind)
    assert (dg[r.binds] == 0).all()


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "float_atomics"])
def test_every_sample_in_one_texel(det):
    """N = 2^17 + 3 samples clipped into texel (0, 0) with upstream 1.0: d_img[0, 0] == N exactly; then the opposite corner with
    alternating signs: the sum is 1.  In deterministic mode this catches a headroom that does not grow with N (a constant 3 bits
    overflows here: 2^58 N > 2^63).  It does NOT see det_headroom one bit short, and no input can: a sample adds at most |g| to one
    texel (its four weights go to four different texels and sum to 1), each scaled contribution is below 2^(62 - hb), and hb has
    2^(hb - 2) >= N, so a texel's sum stays below 2^60 of the 2^63 available -- the "four contributions per sample" and the 62
    leave three spare bits.  Float atomics add integers below 2^24 exactly."""
    assert torch.cuda.is_available()
    N = 2 ** 17 + 3
    img = np.zeros((2, 5, 7), np.float32)
    grid = np.full((N, 2), -1.5, np.float32)
    d_out = np.ones((N, 2), np.float32)
    d_out[:, 1] = 0.5
    _, dg, di = _run(img, grid, d_out, det)
    want = np.zeros((2, 5, 7), np.float32)
    want[0, 0, 0], want[1, 0, 0] = N, 0.5 * N
    assert np.array_equal(di, want) and (dg == 0).all()
    grid[:] = 1.25
    d_out[:, 0] = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    d_out[:, 1] = d_out[:, 0] * 3.0
    _, dg, di = _run(img, grid, d_out, det)
    want[:] = 0
    want[0, 4, 6], want[1, 4, 6] = 1.0, 3.0
    assert np.array_equal(di, want)


def test_workspace_regrows_and_is_left_clean():
    """On a stream of its own, whose integer workspace (kept per device and stream) starts empty: small image (45 sums) -> large
    (3 x 17 x 33 = 1683: regrown) -> small -> larger (4 x 17 x 33 = 2244: regrown again) -> large -> small, exact-lattice inputs.
    Every d_img is bit-equal to the float64 scatter rounded once -- the expectation never comes from an earlier kernel call -- so
    sums left over by a call, or a regrown workspace that was not cleared, show in the next."""
    assert torch.cuda.is_available()
    g = np.random.default_rng(5)

    def small():
        img = (g.integers(-64, 65, (1, 5, 9)) / 1024.0).astype(np.float32)
        grid = np.stack([g.integers(-8, 8 * 16 + 9, 300) / 64.0 - 1.0, g.integers(-8, 4 * 16 + 9, 300) / 32.0 - 1.0], 1).astype(np.float32)
        return img, grid, (g.integers(-64, 65, (300, 1)) / 1024.0).astype(np.float32)

    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for k, case in enumerate((small(), R.lattice_case(3), small(), R.lattice_case(4), R.lattice_case(3), small())):
            r = R.grid_reference(*case)
            _, _, di = _run(*case, True)
            assert np.array_equal(di, r.d_img.astype(np.float32)), f"call {k}"


def test_non_finite_upstream_gradients_differ_between_the_modes_as_documented():
    """include/gs2m_mvs.h: deterministic mode drops an infinite / NaN contribution (the texel gets the sum of its finite ones),
    the float-atomic mode poisons the texel; texels no such sample touches are the same as without those samples."""
    assert torch.cuda.is_available()
    img, grid, d_out = (a.copy() for a in R.lattice_case(2))
    grid[10], grid[11] = [-0.5, -0.5], [0.5, 0.5]     # x = 8, y = 4 and x = 24, y = 12: one texel each
    d_out[10], d_out[11] = [np.inf, 0.25], [0.125, np.nan]
    clean = d_out.copy()
    clean[10, 0], clean[11, 1] = 0.0, 0.0
    want = R.grid_reference(img, grid, clean).d_img.astype(np.float32)
    _, dg, det = _run(img, grid, d_out, True)
    assert np.array_equal(det, want), "deterministic: the non-finite contributions are dropped, everything else is exact"
    _, _, flt = _run(img, grid, d_out, False)
    assert np.isinf(flt[0, 4, 8]) and np.isnan(flt[1, 12, 24])
    hit = np.zeros(flt.shape, dtype=bool)   # (the other three texels of each footprint get inf x 0 = NaN)
    hit[0, 4:6, 8:10] = hit[1, 12:14, 24:26] = True
    assert np.array_equal(flt[~hit], want[~hit])
    ok = np.ones(len(grid), dtype=bool)
    ok[[10, 11]] = False
    assert np.isfinite(dg[ok]).all()
