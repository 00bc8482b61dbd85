"""tests/cubemap_ref.py (the float64 reference of tests/test_cubemap_kernels_gpu.py) against oracle/cubemap_oracle.py, and
the conditions the GPU file relies on, computed by the reference alone: the routes of its shapes, the share of pairs it
cannot decide, and the culling boxes its shapes are meant to contain.  No GPU."""
import numpy as np
import pytest

import cubemap_ref as R
from oracle import cubemap_oracle as O


@pytest.mark.parametrize("N,roughness,cos_cut", [(8, 0.5, 0.93), (8, 0.04, 0.999), (16, 0.27, 0.97), (16, 1.0, 0.3)])
def test_columns_and_rows_equal_the_oracle_matrix(N, roughness, cos_cut):
    # (relative to each weight: a cone that reaches d ~ 0 would measure the rounding of the oracle's own float64 dot
    # product, 1e-16 absolute, against d)
    W = O.specular_matrix(N, roughness, cos_cut)
    worst = 0.0
    for a in range(0, 6 * N * N, 7):
        for got, want in ((R.specular_column(N, roughness, cos_cut, a), W[:, a]), (R.specular_row(N, roughness, cos_cut, a), W[a, :])):
            assert np.array_equal(got != 0, want != 0)
            worst = max(worst, float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max()))
    print(f"worst relative difference {worst:.2e}")
    assert worst <= 1e-15


@pytest.mark.parametrize("N", [1, 2, 3, 8, 16])
def test_diffuse_and_areas_are_the_oracle_s(N):
    assert np.array_equal(R.diffuse_matrix(N), O.diffuse_matrix(N)) and np.array_equal(R.texel_areas(N), O.texel_areas(N))
    ax, err = R.axis_table(N)
    assert np.abs(np.outer(ax, ax).reshape(-1) - O.texel_areas(N)[:N * N]).max() <= 1e-15 and (err >= 0).all()
    assert R.diffuse_matrix(N).shape == (6 * N * N, 6 * N * N)


def test_the_transpose_is_the_backward():
    """L(x) = <G, W x> is linear in x: its central difference along e_t is its exact derivative, and that is the row
    product sum_o W[o, t] G[o] built from reference columns -- what the GPU file expects of the backward kernels."""
    N, r, cc = 8, 0.4, 0.9
    T = 6 * N * N
    rng = np.random.RandomState(0)
    x, G = rng.rand(T, 3), rng.randn(T, 3)
    rows = np.stack([R.specular_row(N, r, cc, o) for o in range(T)])
    L = lambda v: float((G * (rows @ v)).sum())  # noqa: E731
    for t in (0, 63, 200, T - 1):
        col = R.specular_column(N, r, cc, t)
        assert np.abs(col - rows[:, t]).max() <= 1e-15 * np.abs(col).max()
        for c in range(3):
            e = np.zeros_like(x)
            e[t, c] = 0.5
            fd = L(x + e) - L(x - e)
            want = float(col @ G[:, c])
            assert abs(fd - want) <= 1e-12 * max(1.0, abs(want))


def test_pair_classes_partition_and_bounds_are_finite():
    N, r, cc = 16, 0.27, R.f32(0.97)
    for a in (0, 100, 777):
        p = R.row_pairs(N, r, cc, a)
        Ed = R.err_d(p.d)
        assert (Ed <= 2e-6).all() and (p.d[p.cls == R.IN] - Ed[p.cls == R.IN] >= cc).all()
        rim = p.cls == R.RIM
        assert (np.abs(p.d[rim] - cc) <= Ed[rim]).all()
        assert np.isfinite(p.bound).all() and (p.bound[p.cls == R.IN] < 1e-3 * p.w[p.cls == R.IN] + 1e-12).all()
        assert a in p.idx and p.cls[list(p.idx).index(a)] == R.IN       # the self pair


def _lib():
    import gs2m_native
    return gs2m_native.lib()


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_shapes_take_the_route_the_gpu_file_means(shape):
    """through the export the launches themselves ask (the library loads without a GPU; the call launches nothing)"""
    N, r, cutoff, route, aligned = shape
    assert _lib().gs2m_specular_cubemap_route(N, R.cos_cut_of(r, cutoff), aligned) == route


def test_route_export_refuses_what_the_launches_refuse():
    L = _lib()
    assert L.gs2m_specular_cubemap_route(0, 0.5, 1) == -1 and L.gs2m_specular_cubemap_route(4097, 0.5, 1) == -1
    assert L.gs2m_specular_cubemap_route(4096, 0.5, 1) >= 0
    assert {s[3] for s in R.SHAPES} == {0, 1, 2, 3, 4}


def test_full_box_branch_and_its_switch_are_among_the_shapes():
    assert R.cos_cut_of(1.0, 0.99) <= 0.70710678 < R.cos_cut_of(0.3, 0.99)
    cc = R.cos_cut_of(1.0, 0.5)
    assert abs(cc - 0.70710678) < 2e-6, cc     # right at the switch between the full box and cone_range


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[4]], ids=R.shape_id)
def test_rim_share_cap_of_every_probe_set(shape):
    """Over all probes of a shape, rim pairs are at most 25 % of (in + rim) for the two sub-texel shapes and 5 % for the
    others; every probe whose cone reaches a texel other than itself has an IN pair besides the self pair."""
    N, r, cutoff = shape[:3]
    cc = R.cos_cut_of(r, cutoff)
    n_in = n_rim = 0
    for trio in R.probe_texels(N):
        for t in trio:
            p = R.column_pairs(N, R.f32(r), cc, t)
            n_in += p.n_in
            n_rim += p.n_rim
            assert p.cls[p.idx == t][0] == R.IN
            if len(p.idx) > 1:
                assert p.n_in >= 2, (t, p.n_in, p.n_rim)
    cap = 0.25 if (N, r) in R.SUB_TEXEL else 0.05
    print(f"{R.shape_id(shape)}: in {n_in} rim {n_rim} share {n_rim / (n_in + n_rim):.4f} cap {cap}")
    assert n_rim <= cap * (n_in + n_rim)


def test_wide_segment_shape_has_a_union_box_wider_than_64_columns():
    N, r = R.WIDE_SEGMENT
    cc = R.cos_cut_of(r, 0.99)
    tiles = 6 * (N // 8) ** 2
    widest = max(b[1] - b[0] + 1 for tile in range(0, tiles, 3) for f in range(6) for b in [R.union_box(N, cc, tile, f)] if b)
    print("widest union box", widest)
    assert widest > 64 + 2      # 2: the reference's box is float64, the kernel's fp32


def test_split8_shape_has_a_union_box_with_fewer_rows_than_waves():
    N, r = R.FEW_ROWS
    cc = R.cos_cut_of(r, 0.99)
    tiles = 6 * (N // 8) ** 2
    fewest = min(b[3] - b[2] + 1 for tile in range(tiles) for f in range(6) for b in [R.union_box(N, cc, tile, f)] if b)
    print("fewest rows of a union box", fewest)
    assert fewest < 8 - 2
