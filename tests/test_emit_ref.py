"""tests/emit_ref.py checked on its own, without a GPU: the closed-form minimum of the quadratic over a pixel rectangle against
brute-force sampling, must_hit inside may_hit on every case family of tests/test_emit_gpu.py, and the two caps that keep that
test's inclusions from being vacuous (few ambiguous pixels; enough quadrants both required and unreachable)."""
import numpy as np
import pytest

import emit_ref as E


@pytest.fixture(scope="module")
def family_brackets():
    out = {}
    for name in E.FAMILIES:
        for seed in (0, 1):
            case = E.family_case(name, seed)
            out[name, seed] = (case,) + E.brackets(case)
    return out


def test_closed_form_minimum_against_sampling():
    """the minimum over the rectangle [x0, x0 + 7] x [y0, y0 + 7] on a 64 x 64 grid of samples is never below the closed form and
    exceeds it by no more than the quadratic can change over half a grid cell"""
    rng = np.random.default_rng(1)
    n = 4000
    major = np.exp(rng.uniform(np.log(0.3), np.log(300.0), n))
    minor = major / rng.choice([1.0, 2.0, 10.0, 50.0, 190.0], n)
    A, B, C = (v.astype(np.float64) for v in E.conic(major, minor, rng.uniform(0, np.pi, n)))
    gx, gy = rng.uniform(-40, 60, n), rng.uniform(-40, 60, n)
    gx[:200], gy[:200] = rng.uniform(8, 15, 200), rng.uniform(8, 15, 200)      # centres inside the rectangle
    x0 = y0 = np.full(n, 8.0)
    closed = E.exact_min(gx, gy, A, B, C, x0, y0)
    s = np.linspace(0.0, 7.0, 64)
    dx, dy = (8.0 + s)[None, None, :] - gx[:, None, None], (8.0 + s)[None, :, None] - gy[:, None, None]
    q = A[:, None, None] * dx * dx + 2 * B[:, None, None] * dx * dy + C[:, None, None] * dy * dy
    brute = q.min(axis=(1, 2))
    assert np.all(closed <= brute * (1 + 1e-12) + 1e-12), "the closed form is a lower bound of every sample"
    # from the closed-form minimiser the nearest sample is at most half a cell (7 / 126) away in x and y: with the gradient g
    # there and the curvature bounded by A + C, q rises by at most |g| d + (A + C) d^2, d = (7 / 126) sqrt 2
    d = 7.0 / 126.0 * np.sqrt(2.0)
    gmax = 2 * np.sqrt(np.maximum(closed, 0) * (A + C))          # |grad q| = 2 |M x| <= 2 sqrt(q lambda_max), lambda_max <= A + C
    assert np.all(brute <= closed + gmax * d + (A + C) * d * d + 1e-9)
    assert np.all(closed[:200] == 0.0) and (closed > 0).sum() > 3000


def test_must_hit_is_inside_may_hit(family_brackets):
    for (name, seed), (case, must, may, n_req, n_amb) in family_brackets.items():
        assert not np.any(must & ~may), f"{name}-{seed}: {int((must & ~may).sum())} quadrants are required but counted unreachable"


def test_caps(family_brackets):
    """ambiguous pixels are at most 0.1 % of the required ones in every case; every family whose culling is on has at least 200
    quadrants in must_hit and at least 200 outside may_hit (of those that have pixels)"""
    for (name, seed), (case, must, may, n_req, n_amb) in family_brackets.items():
        assert n_amb <= 1e-3 * n_req or (n_req == 0 and n_amb == 0), f"{name}-{seed}: {n_amb} ambiguous pixels beside {n_req} required"
        _, _, tx, ty = E.instances(case["rect"])
        has_pixels = np.stack([(16 * tx + 8 * (q & 1) < case["W"]) & (16 * ty + 8 * (q >> 1) < case["H"]) for q in range(4)], axis=1)
        if name in E.CULLED_FAMILIES:
            assert must.sum() >= 200 and (has_pixels & ~may).sum() >= 200, f"{name}-{seed}: {int(must.sum())} required, {int((has_pixels & ~may).sum())} unreachable"
        elif name == "off":
            t2 = case["rec"][:, 11]
            assert np.all(np.isinf(t2)) and must.sum() >= 200 and np.array_equal(may, has_pixels)
        else:   # below 1/255: nothing is required, only the centre's own quadrant is allowed
            assert np.all(case["rec"][:, 11] == -1.0) and must.sum() == 0 and np.all(may.sum(1) <= 1) and may.sum() >= 50


def test_layout_cases_also_respect_the_caps():
    for P, kind in E.LAYOUT_CASES:
        case = E.layout_case(P, kind)
        must, may, n_req, n_amb = E.brackets(case)
        assert not np.any(must & ~may), case["name"]
        assert n_amb <= 1e-3 * n_req, f"{case['name']}: {n_amb} ambiguous pixels beside {n_req} required"


def test_heavy_rule_and_layout_on_a_hand_made_example():
    """two waves: the first crowded (light sum 62 x 7 + 8 = 442 > 320: the 8 and the 70 are heavy), the second not (the 8 stays)"""
    cnt = np.array([7] * 62 + [8, 70] + [8, 3, 40, 0, 39], np.int64)
    heavy, units = E.heavy_rule(cnt, E.CROWDED_WAVE)
    assert list(np.nonzero(heavy)[0]) == [62, 63, 66] and list(units[[62, 63, 66]]) == [1, 2, 1]
    heavy, units = E.heavy_rule(cnt, E.CROWDED_OFF)
    assert list(np.nonzero(heavy)[0]) == [63, 66]
    tt, hu = E.block_counts(cnt, E.CROWDED_WAVE)
    assert list(tt) == [int(cnt.sum())] and list(hu) == [4]
    # one light Gaussian of 2 x 1 tiles with masks 0b0101, 0b1111 and one of 1 x 1 with mask 0: rows 0, 2 and 6; keys by row
    rect = np.array([[1 | (2 << 16), 2 | (1 << 16)], [0, 0], [3 | (0 << 16), 1 | (1 << 16)]], np.uint32)
    lay = E.expected_layout(rect, np.array([10, 11, 12], np.uint32), np.array([5, 15, 0]), E.CROWDED_WAVE, 12, (2, [2, 2, 0, 0], [0, 2, 0, 0]))
    assert list(lay["keys"]) == [25, 26, 3]
    assert lay["e_rec"].tolist() == [[0 | (5 << 28), 0, 10, 0], [0 | (15 << 28), 2, 10, 0], [2, 6, 12, 0]]
    assert list(lay["gauss_rows"]) == [6, 0, 0] and list(lay["wave_rows"]) == [6] and list(lay["wave_rowbase"]) == [0] and lay["rows"] == 6
    assert list(lay["hist"][0][:4]) == [0, 1, 1, 1] and list(lay["hist"][1][:4]) == [1, 0, 2, 0]


def test_cull_params_edges():
    inv = np.float32(1.0) / np.float32(255.0)
    A, B, C = E.conic(np.array([4.0, 4.0, 95.0, 105.0]), np.array([4.0, 4.0, 0.5, 0.5]), np.deg2rad(np.array([0.0, 0.0, 45.0, 45.0])))
    ex, ey, t2 = E.cull_params(A, B, C, np.array([np.nextafter(inv, np.float32(0)), inv, 1.0, 1.0], np.float32))
    assert (ex[0], ey[0], t2[0]) == (-1.0, -1.0, -1.0)
    assert 0.0 < t2[1] < 0.01 and 0.0 < ex[1] < 0.5, "at 1/255 exactly the region is the centre and the margins"
    assert np.isfinite(t2[2]) and abs(t2[2] - (2 * (np.log(255.0) + 1e-3) * 1.002 + 1e-3)) < 1e-5, "ratio 190 at 45 degrees is still culled"
    assert np.isinf(t2[3]) and np.isinf(ex[3]), "ratio 210 at 45 degrees is not"
