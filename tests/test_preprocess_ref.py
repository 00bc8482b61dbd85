"""tests/preprocess_ref.py alone (no GPU): its two additions against independent computations, and every case family of
tests/test_preprocess_gpu.py shown to hold the edge cases it is there for, on the C oracle's output for the family."""
import numpy as np
import pytest
import torch

import emit_ref as E
import preprocess_ref as R
import torch_ref


@pytest.mark.parametrize("D", [0, 1, 2, 3])
def test_sh_dir_against_central_differences(D):
    """torch_ref.eval_sh_color is a polynomial in the direction: central differences of it in float64 about 200 unit directions,
    taken after the normalisation (the polynomial extended off the sphere as it stands), step 1e-4: the truncation error is
    h^2 / 6 times a third derivative of at most ~50 = 1e-7, the rounding error 1e-16 / h = 1e-12"""
    rng = np.random.default_rng(D)
    d = rng.normal(0, 1, (200, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    sh = rng.uniform(-1, 1, (200, 16, 3))
    val, ab, n = R.sh_dir(D, sh, d)
    assert val.shape == (200, 9) and np.all(ab >= np.abs(val) - 1e-12)
    assert list(n) == {0: [0] * 9, 1: [1] * 9, 2: [5] * 3 + [5] * 3 + [4] * 3, 3: [15] * 3 + [15] * 3 + [12] * 3}[D]
    h = 1e-4
    f = lambda v: torch_ref.eval_sh_color(D, torch.from_numpy(sh), torch.from_numpy(v)).numpy()
    for a in range(3):
        e = np.zeros(3); e[a] = h
        fd = (f(d + e) - f(d - e)) / (2 * h)
        assert np.abs(fd - val[:, 3 * a:3 * a + 3]).max() <= 2e-7 * max(1.0, float(ab.max()))
    if D == 0:
        assert not val.any()


def test_shrunk_rect_against_tile_rect():
    """on inputs at least 1e-3 px away from every tile boundary the float32 rectangle is the float64 one of emit_ref.tile_rect
    intersected with the reference's radius rectangle (computed here in float64)"""
    rng = np.random.default_rng(5)
    n, tiles_x, tiles_y = 20000, 12, 8
    pix, piy = rng.uniform(-300, 500, n).astype(np.float32), rng.uniform(-300, 400, n).astype(np.float32)
    ex = np.exp(rng.uniform(np.log(0.05), np.log(400.0), n)).astype(np.float32)
    ey = np.exp(rng.uniform(np.log(0.05), np.log(400.0), n)).astype(np.float32)
    k = np.arange(n) % 10
    ex, ey = np.where(k == 0, np.float32(np.inf), ex), np.where(k == 0, np.float32(np.inf), ey)
    ex, ey = np.where(k == 1, np.float32(-1), ex), np.where(k == 1, np.float32(-1), ey)
    radius = rng.integers(0, 300, n)
    radius[k == 2] = 0
    far = lambda v: np.abs(v / 16.0 - np.round(v / 16.0)) * 16.0 >= 1e-3
    p64, q64, ex64, ey64 = pix.astype(np.float64), piy.astype(np.float64), np.where(np.isfinite(ex), ex, 0).astype(np.float64), np.where(np.isfinite(ey), ey, 0).astype(np.float64)
    ok = far(p64 - radius) & far(p64 + radius + 15) & far(q64 - radius) & far(q64 + radius + 15) & far(p64 - ex64 - 15) & far(p64 + ex64) & far(q64 - ey64 - 15) & far(q64 + ey64)
    assert ok.sum() > 15000
    tt, rect, bin_ = R.shrunk_rect(pix, piy, ex, ey, radius, tiles_x, tiles_y, 1)
    tt0, rect0, _ = R.shrunk_rect(pix, piy, ex, ey, radius, tiles_x, tiles_y, 0)
    # float64: the reference's rectangle ...
    cl = lambda v, m: np.clip(np.trunc(v).astype(np.int64), 0, m)
    rx0, rx1, ry0, ry1 = cl((p64 - radius) / 16, tiles_x), cl((p64 + radius + 15) / 16, tiles_x), cl((q64 - radius) / 16, tiles_y), cl((q64 + radius + 15) / 16, tiles_y)
    ref_n = np.where(radius > 0, (rx1 - rx0) * (ry1 - ry0), 0)
    assert np.array_equal(tt0[ok], ref_n[ok])
    want0 = np.stack([rx0 | (ry0 << 16), (rx1 - rx0) | ((ry1 - ry0) << 16)], 1)
    want0[ref_n == 0] = 0
    assert np.array_equal(rect0[ok], want0[ok].astype(np.uint32))
    # ... intersected with the box's tiles
    box = E.tile_rect(pix, piy, ex, ey, tiles_x, tiles_y).astype(np.int64)
    bx0, by0, bw, bh = box[:, 0] & 0xFFFF, box[:, 0] >> 16, box[:, 1] & 0xFFFF, box[:, 1] >> 16
    ix0, ix1, iy0, iy1 = np.maximum(rx0, bx0), np.minimum(rx1, bx0 + bw), np.maximum(ry0, by0), np.minimum(ry1, by0 + bh)
    w, h = np.maximum(ix1 - ix0, 0), np.maximum(iy1 - iy0, 0)
    n_want = np.where((ref_n > 0) & (bw * bh > 0), w * h, 0)
    assert np.array_equal(tt[ok], n_want[ok])
    full = ok & (n_want > 0)
    assert full.sum() > 2000 and (ok & (n_want == 0) & (ref_n > 0)).sum() > 500 and (ok & (n_want < ref_n) & (n_want > 0)).sum() > 500
    assert np.array_equal(rect[full], np.stack([ix0 | (iy0 << 16), w | (h << 16)], 1)[full].astype(np.uint32))
    assert not rect[ok & (n_want == 0)].any()
    assert np.array_equal(bin_[full], rect[full]) and np.array_equal(bin_[:, 1] & 0xFFFF, np.where(ref_n > 0, bin_[:, 1] & 0xFFFF, 0))
    assert not bin_[ref_n == 0].any(), "nothing is recorded without a reference rectangle"
    # an empty emitted rectangle: the record keeps a corner and a width or a height of 0
    e = ok & (ref_n > 0) & (tt == 0)
    assert np.all((bin_[e, 1] & 0xFFFF) * (bin_[e, 1] >> 16) == 0)


def _front(c):
    return c["means3D"][:, 2] > np.float32(0.2)


def test_sizes_family(oracle_lib):
    assert {P % 4 for P in R.SIZES} == {0, 1, 2, 3} and {1, 256, 257} <= set(R.SIZES) and any(P % 64 == 1 and P > 64 for P in R.SIZES)
    for which in (8, 9):
        c = R.sizes_case(1027, which)
        f = R.oracle_forward(oracle_lib, c)
        assert (f.radii > 0).sum() > 600 and (f.radii == 0).sum() >= 20 and (f.tiles_touched > 1).sum() > 200


def test_layout_family_clamps_every_pattern(oracle_lib):
    """Coefficients uniform in [-1, 1]: at degree 0 no colour can clamp (0.5 - 0.2821 > 0) and at P = 257 the pattern with all
    three channels clamped (about 1 % of the Gaussians at degree 3) cannot occur ten times: the ten occurrences of every pattern
    are asked of the family as a whole, and of its largest degree-3 case for all patterns but that one"""
    counts = np.zeros(8, np.int64)
    for P in R.LAYOUT_SIZES:
        for name, c in R.layout_cases(P).items():
            f = R.oracle_forward(oracle_lib, c)
            vis = f.radii > 0
            assert vis.sum() > 0.7 * P
            n = np.bincount(R.clamp_bits(f.clamped)[vis], minlength=8)
            counts += n
            if name == "aligned" and P == 1027:
                assert np.all(n[:7] >= 10), n
            if c["D"] == 0:
                assert n[1:].sum() == 0
    assert np.all(counts >= 10), counts


def test_near_plane_family(oracle_lib):
    c = R.near_plane_case()
    f = R.oracle_forward(oracle_lib, c)
    front, behind = c["groups"]["front"], c["groups"]["behind"]
    assert len(front) == 80 and len(behind) == 120
    assert np.all(f.radii[front] > 0) and not f.radii[behind].any(), "every centre is inside the image: visible exactly beyond 0.2f"
    z = c["means3D"][:, 2]
    for v in (np.float32(0.2), np.nextafter(np.float32(0.2), np.float32(0)), np.nextafter(np.float32(0.2), np.float32(1))):
        assert (z == v).sum() == 40


def test_degenerate_family(oracle_lib):
    c = R.degenerate_case()
    assert c["P"] <= 2100
    f = R.oracle_forward(oracle_lib, c)
    g, front = c["groups"], _front(c)
    tiles = f.tiles_x * f.tiles_y
    # centres inside the image, in front of the near plane: a non-zero determinant gives a radius >= 2 and with it a rectangle, so
    # radius 0 there means det == 0
    assert front[g["zero"]].all() and not f.radii[g["zero"]].any() and len(g["zero"]) >= 20
    assert np.all(f.radii[g["subpixel"]] == 2), "the 0.1 floor under the root sets the radius"
    # det != 0 (scales are not zero, the view depth is beyond the near plane) and an empty rectangle
    for name in ("offscreen", "clamp"):
        empty = front[g[name]] & (f.radii[g[name]] == 0)
        assert empty.sum() >= 20 and (f.radii[g[name]] > 0).sum() >= 20, (name, int(empty.sum()))
    cam = c["cam"]
    beyond = (np.abs(c["means3D"][:, 0] / c["means3D"][:, 2]) > 1.3 * cam["tanfovx"]) | (np.abs(c["means3D"][:, 1] / c["means3D"][:, 2]) > 1.3 * cam["tanfovy"])
    assert beyond[g["clamp"]].all() and (beyond & (f.radii > 0)).sum() >= 40, "centres beyond the clamp that reach the image"
    assert np.all(f.tiles_touched[g["whole"]] == tiles)
    # thin discs: the share whose culling is switched off
    d = g["discs"][f.radii[g["discs"]] > 0]
    ex, _, _ = E.cull_params(f.conic_opacity[d, 0], f.conic_opacity[d, 1], f.conic_opacity[d, 2], f.conic_opacity[d, 3])
    share = float(np.isinf(ex).mean())
    assert len(d) > 300 and 0.05 <= share <= 0.5, share
    assert np.all(np.abs(f.means2D[f.radii > 0]) < 1e6)


def test_opacity_family(oracle_lib):
    c = R.opacity_case()
    f = R.oracle_forward(oracle_lib, c)
    assert np.all(f.radii > 0) and np.all(f.tiles_touched > 0), "every reference rectangle is non-empty"
    below = c["groups"]["below"]
    assert len(below) == 200 and np.all(c["opacities"][below] < R.INV255)
    for v in R.AROUND_255:
        assert (c["opacities"] == v).sum() == 100
    assert (R.AROUND_255 < R.INV255).sum() == 2 and R.AROUND_255[1] == R.INV255


def test_heavy_family(oracle_lib):
    c = R.heavy_case()
    f = R.oracle_forward(oracle_lib, c)
    cnt, g = f.tiles_touched.astype(np.int64), c["groups"]
    tiles = f.tiles_x * f.tiles_y
    assert np.all(cnt[g["nine"]] == 9) and np.all(cnt[g["big"]] == 49) and np.all(cnt[g["whole"]] == tiles) and tiles == 96
    six = np.setdiff1d(g["six"], g["nine"])
    assert np.all(cnt[six] == 6) and np.all(np.delete(cnt, np.concatenate([g["six"], g["big"], g["whole"]])) == 1)
    heavy, units = E.heavy_rule(cnt, E.CROWDED_WAVE)
    heavy_off, _ = E.heavy_rule(cnt, E.CROWDED_OFF)
    P = c["P"]
    light = np.concatenate([cnt * (cnt < E.HEAVY_TILES), np.zeros((-P) % 64, np.int64)]).reshape(-1, 64).sum(1)
    crowded = light > E.CROWDED_WAVE
    assert list(crowded) == [True, True, False, False, True, False]
    wave_heavy = np.concatenate([heavy, np.zeros((-P) % 64, bool)]).reshape(-1, 64).any(1)
    assert (crowded & wave_heavy).sum() >= 1 and (~crowded & wave_heavy).sum() >= 1 and (crowded & ~wave_heavy).sum() >= 1
    assert heavy[g["nine"]].all() and not heavy_off[g["nine"]].any(), "heavy through the crowded-wave rule alone"
    assert P % 64 != 0 and heavy[P - P % 64:].any(), "a last partial wave that holds a heavy Gaussian"
    assert set(units[heavy].tolist()) == {1, 2}
    bt, bh = E.block_counts(cnt, E.CROWDED_WAVE)
    _, bh_off = E.block_counts(cnt, E.CROWDED_OFF)
    assert len(bt) == 2 and np.any(bh != bh_off)


def test_other_family(oracle_lib):
    base = R.oracle_forward(oracle_lib, R.other_case("modifier1"))
    for kind in R.OTHER_KINDS:
        c = R.other_case(kind, oracle_lib)
        f = R.oracle_forward(oracle_lib, c)
        assert (f.radii > 0).sum() > 400
        if kind == "cov3D_precomp":
            assert np.array_equal(f.radii, base.radii) and np.array_equal(f.conic_opacity, base.conic_opacity), "the oracle's own cov3D reproduces the scene"
        if kind.startswith("modifier") and kind != "modifier1":
            assert not np.array_equal(f.radii, base.radii)
