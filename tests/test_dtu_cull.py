"""The mask-culling restatement (tests/dtu_cull_ref.py) against definitions and library functions, and the host side of
gs2m_dtu_eval's culling: the view matrices and the PNG reader.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gs-2m_amd"))
import dtu_cull_ref as R  # noqa: E402
import gs2m_dtu_eval as E  # noqa: E402


@pytest.mark.parametrize("r", [0, 1, 2, 24])
def test_disk_is_the_formula(r):
    d = R.disk(r)
    assert d.shape == (2 * r + 1, 2 * r + 1)
    for j in range(2 * r + 1):
        for i in range(2 * r + 1):
            assert d[j, i] == ((i - r) ** 2 + (j - r) ** 2 <= r * r)


@pytest.mark.parametrize("r", [0, 1, 2, 3, 24])
def test_dilation_is_the_definition(r):
    rng = np.random.default_rng(r)
    m = (rng.random((11, 9)) < 0.06).astype(np.uint8) * rng.integers(1, 256, (11, 9)).astype(np.uint8)
    m[0, 0] = 7
    assert np.array_equal(R.dilate(m, r), R.dilate_brute(m, r))


def test_lookup_is_grid_sample():
    """the written-out lookup against torch's grid_sample: random positions, half-integer pixels (half to even), the frame's
    edge and positions outside it"""
    rng = np.random.default_rng(0)
    H, W = 7, 10
    dil = rng.random((H, W)) < 0.5
    px = np.concatenate([rng.uniform(-3, W + 2, 400), np.arange(-2, W + 2) + 0.5, np.arange(-2, W + 2) + 0.5, [0.0, W - 1.0, -0.5, W - 0.5]])
    py = np.concatenate([rng.uniform(-3, H + 2, 400), np.full(W + 4, 2.0), np.full(W + 4, 2.5), [0.0, H - 1.0, -0.5, H - 0.5]])
    nx = ((px / (W - 1) - 0.5) * 2).astype(np.float32)
    ny = ((py / (H - 1) - 0.5) * 2).astype(np.float32)
    # half-integer pixels survive the trip through the normalised coordinate only where the arithmetic is exact: state them
    # in normalised form as well, at a size whose steps are binary fractions
    H2, W2 = 5, 9
    dil2 = rng.random((H2, W2)) < 0.5
    hx = (np.arange(-3, 2 * W2 + 2) / 2.0).astype(np.float32)  # -1.5 .. W2 + 0.5 in steps of 0.5
    nx2 = (hx / np.float32(W2 - 1) - np.float32(0.5)) * np.float32(2)
    assert np.array_equal(((nx2 + 1) / 2) * (W2 - 1), hx)  # exact: the rounding under test is rint's
    for d, a, b in ((dil, nx, ny), (dil2, nx2, np.zeros_like(nx2)), (dil2, nx2, np.full_like(nx2, 0.25))):
        got, ref = R.sample_nearest_np(d, a, b), R.sample_nearest(d, a, b)
        assert np.array_equal(got.astype(np.float32), ref)
    # half to even, spelled out: 0.5 -> pixel 0, 1.5 -> pixel 2, 2.5 -> pixel 2
    row = np.zeros((1, W2), bool)
    row[0, 2] = True
    s = R.sample_nearest(row, nx2, np.zeros_like(nx2))
    assert [bool(s[np.argmin(np.abs(hx - q))]) for q in (0.5, 1.5, 2.5, 3.5)] == [False, True, True, False]


def _synthetic_P(rng, sign=1.0, scale=1.0):
    K = np.array([[800.0 + rng.uniform(-50, 50), rng.uniform(-2, 2), 400.0], [0.0, 790.0, 300.0], [0.0, 0.0, 1.0]])
    Rm = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    Rm *= np.linalg.det(Rm)
    Cc = rng.normal(size=3) * 3
    return K, Rm, Cc, (K @ np.hstack([Rm, (-Rm @ Cc)[:, None]])) * sign * scale


@pytest.mark.parametrize("sign,scale", [(1.0, 1.0), (-1.0, 1.0), (1.0, 300.0), (-1.0, 300.0)])
def test_view_matrix_is_the_normalised_projection(sign, scale):
    rng = np.random.default_rng(5)
    for _ in range(5):
        _, _, _, P = _synthetic_P(rng, sign, scale)
        Wm, Sm = np.eye(4), np.eye(4)
        Wm[:3] = P
        Sm[0, 0] = Sm[1, 1] = Sm[2, 2] = 1.5
        Sm[:3, 3] = [0.2, -0.1, 0.3]
        M = E.view_matrices([Wm], [Sm])
        assert M.shape == (1, 4, 4) and M.dtype == np.float32
        P32 = (Wm.astype(np.float32) @ Sm.astype(np.float32))[:3].astype(np.float64)
        exact = P32 / (np.sign(np.linalg.det(P32[:, :3])) * np.linalg.norm(P32[2, :3]))
        assert np.abs(M[0, :3] - exact).max() <= 1e-5 * np.abs(exact).max()
        assert np.array_equal(M[0, 3], [0, 0, 0, 1])


def test_decomposition_round_trip():
    rng = np.random.default_rng(6)
    for _ in range(5):
        K, Rm, Cc, P = _synthetic_P(rng)
        K2, R2, C2 = E.decompose_projection(P)
        assert K2[0, 0] > 0 and K2[1, 1] > 0 and abs(np.linalg.det(R2) - 1) < 1e-12 and abs(K2[1, 0]) + abs(K2[2, 0]) + abs(K2[2, 1]) < 1e-9
        assert np.abs(K2 / K2[2, 2] - K).max() <= 1e-5 * np.abs(K).max()
        assert np.abs(R2 - Rm).max() <= 1e-5 and np.abs(C2 - Cc).max() <= 1e-5
    assert E.view_matrices([], []).shape == (0, 4, 4)


def test_png_reader(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(1)
    g = (rng.random((6, 8)) < 0.5).astype(np.uint8) * 255
    Image.fromarray(g, "L").save(tmp_path / "grey.png")
    assert np.array_equal(E.read_mask_png(tmp_path / "grey.png"), g)
    rgb = rng.integers(0, 256, (6, 8, 3)).astype(np.uint8)
    Image.fromarray(rgb, "RGB").save(tmp_path / "rgb.png")
    assert np.array_equal(E.read_mask_png(tmp_path / "rgb.png"), rgb[:, :, 2])  # blue: channel 0 of a BGR read
    rgba = rng.integers(0, 256, (6, 8, 4)).astype(np.uint8)
    Image.fromarray(rgba, "RGBA").save(tmp_path / "rgba.png")
    assert np.array_equal(E.read_mask_png(tmp_path / "rgba.png"), rgba[:, :, 2])
    pal = Image.fromarray((g > 0).astype(np.uint8), "P")
    pal.putpalette([0, 0, 0, 10, 20, 250] + [0] * (254 * 3))
    pal.save(tmp_path / "pal.png")
    assert np.array_equal(E.read_mask_png(tmp_path / "pal.png"), np.where(g > 0, 250, 0))
    Image.fromarray((rng.random((6, 8)) * 65535).astype(np.uint16)).save(tmp_path / "deep.png")
    with pytest.raises(ValueError, match="16 bits"):
        E.read_mask_png(tmp_path / "deep.png")
    (tmp_path / "not.png").write_bytes(b"nothing of the kind, whatever the name says")
    with pytest.raises(ValueError, match="not a PNG"):
        E.read_mask_png(tmp_path / "not.png")


def test_load_cull_inputs(tmp_path):
    from PIL import Image
    world, scales = R.ring_cameras(2)
    ref = tmp_path / "scan1"
    os.makedirs(ref / "images")
    os.makedirs(ref / "mask")
    np.savez(ref / "cameras.npz", **{f"world_mat_{k}": world[k] for k in range(2)}, **{f"scale_mat_{k}": scales[k] for k in range(2)})
    for k in range(2):
        Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(ref / "images" / f"{k:03}.png")
    Image.fromarray(R.ellipse_mask(15, 20, 1)).save(ref / "mask" / "001.png")
    with pytest.raises(ValueError, match="1 masks for 2 images"):
        E.load_cull_inputs(str(ref))
    Image.fromarray(R.ellipse_mask(15, 20, 0)).save(ref / "mask" / "000.png")
    M, masks = E.load_cull_inputs(str(ref))
    assert np.array_equal(M, E.view_matrices(world, scales))
    assert [np.array_equal(masks[k], R.ellipse_mask(15, 20, k)) for k in range(2)] == [True, True]


def test_renumbering_keeps_unreferenced_vertices():
    v = np.arange(18, dtype=np.float64).reshape(6, 3)
    t = np.array([[0, 1, 2], [2, 3, 5], [5, 2, 0], [3, 3, 5], [0, 2, 5]], np.int32)
    keep = np.array([1, 0, 1, 1, 1, 1], bool)  # vertex 4 is kept and unreferenced
    cv, ct = R.cull_mesh(v, t, keep)
    assert np.array_equal(cv, v[[0, 2, 3, 4, 5]])
    assert np.array_equal(ct, [[1, 2, 4], [4, 1, 0], [2, 2, 4], [0, 1, 4]])  # the degenerate face stays: this is not post_process_mesh's rule


def test_e_follows_the_measured_error():
    """E_PX is four times the largest fp32 position error on the test inputs, rounded up to a power of two"""
    worst = max(R.position_error(c["vertices"], c["M"], c["image_size"]) for c in R.all_inputs())
    print(f"largest |fp32 - fp64| position: {worst:.3e} px; e = {R.e_for(worst)} px")
    assert R.E_PX == R.e_for(worst)


def test_undecided_cap_holds_for_every_gpu_input():
    """at most 0.2 % of an input's vertices are undecided, and a decided pair's fp32 verdict is the fp64 position's"""
    for c in R.all_inputs():
        n = len(c["vertices"])
        assert int(c["undecided"].sum()) <= R.UNDECIDED_CAP * n, (len(c["M"]), n, int(c["undecided"].sum()))
        keep64 = np.ones(n, bool)
        for k in range(len(c["M"])):
            qx, qy, _ = R.project(c["vertices"], c["M"][k], np.float64)
            keep64 &= R._verdict64(qx, qy, c["dilated"][k], *c["image_size"])
        d = ~c["undecided"]
        assert np.array_equal(keep64[d], c["keep"][d])
        if n >= 1000:  # the inputs exercise both verdicts, the shells every kind of point
            assert 0 < int(c["keep"].sum()) < n and ("triangles" in c or np.isnan(c["vertices"]).any())
            if "triangles" not in c:  # points behind a camera and points outside a frame are there
                behind, outside = R.point_kinds(c)
                assert behind >= 1 and outside >= 1, (behind, outside)
    c, v, t, cv, ct = R.decided_mesh(3, 2000, 3000, 7)
    assert int(c["undecided"].sum()) <= R.UNDECIDED_CAP * 2000 and 0 < len(ct) < len(t) and 0 < len(cv) < len(v)
