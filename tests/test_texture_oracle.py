"""oracle/texture_oracle.py's float64 transposes (`cube_scatter`, `tex2d_clamp_scatter`) against its own forward
restatement: the adjoint identity in every mode, and S / cnt against a brute-force recount.  No GPU."""
import numpy as np
import pytest

from oracle import texture_oracle as O


def _dirs(n, rng):
    d = rng.standard_normal((n, 3))
    k = n // 3                                                  # a third hugging edges / corners of the cube
    d[:k] = np.sign(d[:k]) * (1.0 - 0.02 * rng.random((k, 3)))
    d[k:2 * k, 0] = np.sign(d[k:2 * k, 0])
    d[-3:] = [[np.nan, 0.0, 1.0], [0.0, 0.0, 0.0], [np.inf, np.inf, 1.0]]
    return d.astype(np.float32)


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


@pytest.mark.parametrize("mode", ["cube", "cube_mip", "2d"])
def test_scatter_is_the_transpose_of_sample(mode):
    rng = np.random.default_rng(3)
    n, C = 400, 3
    dy = rng.standard_normal((n, C))
    dy[::9] = 0.0
    if mode == "2d":
        H, W = 7, 12
        tex = rng.standard_normal((H, W, C))
        uv = (rng.random((n, 2)) * 1.3 - 0.15).astype(np.float32)
        uv[:5] = [[0.0, 0.0], [1.0, 1.0], [0.5 / W, 0.5 / H], [1 - 0.5 / W, 0.3], [-1.0, 2.0]]
        lhs = (dy * O.tex2d_clamp_sample(tex, uv)).sum()
        g, S, cnt = O.tex2d_clamp_scatter(H, W, C, uv, dy)
        rhs = (g * tex).sum()
        assert g.shape == S.shape == (H, W, C) and cnt.shape == (H, W)
    else:
        widths = (8, 4, 2) if mode == "cube_mip" else (5,)
        levels = [rng.standard_normal((6, w, w, C)) for w in widths]
        d = _dirs(n, rng)
        bias = None
        if mode == "cube_mip":
            bias = (rng.random(n) * 3.4 - 0.7).astype(np.float32)
            bias[:5] = [0.0, 1.0, 2.0, 1.999, 5.0]
        lhs = (dy * O.cube_sample(levels, d, bias)).sum()
        g, S, cnt = O.cube_scatter(widths, C, d, dy, bias)
        rhs = sum((a * b).sum() for a, b in zip(g, levels))
        assert all(a.shape == s.shape == (6, w, w, C) and c.shape == (6, w, w) for a, s, c, w in zip(g, S, cnt, widths))
    assert _rel(lhs, rhs) < 1e-12, (lhs, rhs)


def test_cube_counts_and_sums_against_a_recount():
    """cnt and S, texel by texel, from `footprint_cube` and `level_split` directly: a dictionary keyed by the texel."""
    rng = np.random.default_rng(5)
    widths, C, n = (4, 2), 2, 60
    d = _dirs(n, rng)
    bias = (rng.random(n) * 2.0 - 0.5).astype(np.float32)
    bias[:3] = [0.0, 1.0, 0.5]
    dy = rng.standard_normal((n, C))
    dy[::7] = 0.0
    dy[1, 0] = 0.0                                              # zero in one channel only: still a contribution
    cnt, S, G = {}, {}, {}
    for i in range(n):
        if not dy[i].any():
            continue
        for lv, a in O.level_split(bias[i], len(widths)):
            fp = O.footprint_cube(d[i], widths[lv])
            if fp is None or a == 0.0:
                continue
            for t, w_ in fp:
                key = (lv,) + t
                cnt[key] = cnt.get(key, 0) + 1
                S[key] = S.get(key, 0.0) + np.abs(a * dy[i])
                G[key] = G.get(key, 0.0) + a * w_ * dy[i]
    g, Ss, cnts = O.cube_scatter(widths, C, d, dy, bias)
    assert sum(int(c.sum()) for c in cnts) == sum(cnt.values()) > 0
    for (lv, f, x, y), c in cnt.items():
        assert cnts[lv][f, y, x] == c
        assert np.allclose(Ss[lv][f, y, x], S[(lv, f, x, y)], rtol=1e-13, atol=0)
        assert np.allclose(g[lv][f, y, x], G[(lv, f, x, y)], rtol=1e-12, atol=1e-15)
    for lv in range(len(widths)):                               # and nothing anywhere else
        assert (g[lv][cnts[lv] == 0] == 0).all() and (Ss[lv][cnts[lv] == 0] == 0).all()


def test_tex2d_counts_and_sums_against_a_recount():
    rng = np.random.default_rng(6)
    H, W, C, n = 3, 5, 1, 40
    uv = (rng.random((n, 2)) * 1.4 - 0.2).astype(np.float32)
    dy = rng.standard_normal((n, C))
    dy[::5] = 0.0
    g, S, cnt = O.tex2d_clamp_scatter(H, W, C, uv, dy)
    c2, s2 = np.zeros((H, W), dtype=int), np.zeros((H, W, C))
    for i in range(n):
        if dy[i].any():
            for iy, ix, _ in O.tex2d_footprint(uv[i, 0], uv[i, 1], W, H):
                c2[iy, ix] += 1
                s2[iy, ix] += np.abs(dy[i])
    assert (cnt == c2).all() and np.allclose(S, s2, rtol=1e-13, atol=0) and cnt.sum() == 4 * (dy != 0).any(axis=1).sum()


def test_contributions_follow_the_lookup_order():
    """`cube_contributions` lists a pixel's texels in the order level part, then corner (u0 v0, u1 v0, u0 v1, u1 v1): what
    the run-length and table-load premises of the GPU tests are computed from."""
    w = 4
    d = np.array([[1.0, 0.1, 0.1], [1.0, -0.999, 0.999], [np.nan, 0.0, 0.0]], dtype=np.float32)
    level, texel, weight, scale = O.cube_contributions((w, 2), d, np.array([0.25, 0.0, 1.0], dtype=np.float32))
    assert texel.shape == (3, 2, 4)
    fp = O.footprint_slots(d[0], w)
    assert [int(t) for t in texel[0, 0]] == [x + w * (y + w * f) for (f, x, y), _ in fp]
    assert (level[0, 1] == 1).all() and np.allclose(scale[0], [[0.75] * 4, [0.25] * 4])
    assert (texel[1, 0] < 0).sum() == 1 and (texel[1, 1] < 0).all()        # a corner; bias 0 has no second part
    assert np.isclose(weight[1, 0][texel[1, 0] >= 0].sum(), 1.0)          # the missing corner's weight went to the others
    assert (texel[2] < 0).all()


def test_fold_is_memoised_and_still_a_search():
    O._FOLD.clear()
    a = O.fold(0, -1, 3, 128)
    assert (0, -1, 3, 128) in O._FOLD and a == O._fold_search(0, -1, 3, 128) and a[0] != 0
    assert O.fold(2, 128, 128, 128) is None
