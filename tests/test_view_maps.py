"""The contract of include/gs2m_maps.h without a GPU: the numpy restatement tests/view_maps_ref.py against the
reference's own outputs recorded in tests/golden/ref_view_maps.npz (save_depth_map's decoded PNG, map_to_rgba,
convert_normal_for_save) and against np.percentile; gs2m_render's host planning against the same; the new exports."""
import ctypes
import os
import re

import numpy as np
import pytest

import view_maps_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ("37x53", "48x64")
DEPTHS = tuple(f"{kind}{tag}" for tag in TAGS for kind in ("", "half_", "const_")) + ("1x1",)


def _bits(x):
    return np.asarray(x, dtype=np.float32).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("name", DEPTHS)
def test_depth_restatement_is_the_reference_png(name):
    g = VR.golden()
    png = g[f"depth_{name}_png"]
    assert png.shape == g[f"depth_{name}"].shape + (4,) and (png[..., 3] == 255).all()
    assert np.array_equal(VR.depth_image(g[f"depth_{name}"]), png)


def test_constant_depth_takes_the_first_colour():
    g = VR.golden()
    assert (g["depth_const_37x53_png"] == np.append(g["magma_table"][0], 255)).all()


@pytest.mark.parametrize("tag", TAGS)
def test_map_to_rgba_restatement_is_byte_exact(tag):
    g = VR.golden()
    for name in ("map3", "map1"):
        assert np.array_equal(VR.pack_image(g[f"{name}_{tag}"], "chw", "trunc", alpha=g[f"alpha_{tag}"]), g[f"{name}_{tag}_rgba"]), name
    hwc = np.ascontiguousarray(g[f"map3_{tag}"].transpose(1, 2, 0))
    assert np.array_equal(VR.pack_image(hwc, "hwc", "trunc", alpha=g[f"alpha_{tag}"]), g[f"map3_{tag}_rgba"])


@pytest.mark.parametrize("tag", TAGS)
def test_normal_restatement_against_the_reference(tag):
    """sqrt and the 3x3 product are not pinned between numpy and torch: the values agree to a few ulps, the bytes by the
    boundary rule"""
    g = VR.golden()
    n = g[f"normal_{tag}"]
    for space, rot in (("view", g[f"wvt_{tag}"][:3, :3]), ("world", None)):
        ref = g[f"normal_{tag}_{space}"].transpose(1, 2, 0)
        got = VR.pack_values(n, "chw", normal=True, rot=rot)
        assert np.abs(got - ref).max() <= 4 * np.finfo(np.float32).eps
        VR.assert_bytes_close(VR.quant_round(got), VR.quant_round(ref), ref, "round", f"normal {space} {tag}")
    ref = g[f"normal_{tag}_view"].transpose(1, 2, 0)
    got = VR.pack_image(n, "chw", "trunc", alpha=g[f"alpha_{tag}"], normal=True, rot=g[f"wvt_{tag}"][:3, :3])
    VR.assert_bytes_close(got, g[f"normal_{tag}_view_rgba"], ref, "trunc", f"normal rgba {tag}")


SIZES = (1, 2, 3, 255, 256, 257, 4097, 37 * 53, 48 * 64, 64 * 96, 1200 * 1600)


@pytest.mark.parametrize("n", SIZES)
def test_percentiles_equal_numpy_bit_for_bit(n):
    import gs2m_render as GR
    rng = np.random.default_rng(n)
    x = (rng.random(n) * 7.0 + 0.5).astype(np.float32)
    for q in (1, 99, 0, 100, 50, 25):
        ref = np.percentile(x, q)
        assert ref.dtype == np.float32
        assert _bits(VR.percentile(x, q))[0] == _bits(ref)[0], (n, q)
        p, nx, t = VR.percentile_plan(n, q)
        p2, nx2, t2 = GR.percentile_plan(n, q)  # the product's host planning: numpy's own expressions
        assert (p, nx) == (p2, nx2) and _bits(t)[0] == _bits(t2)[0], (n, q)


def test_order_stats_restatement_against_numpy_sort():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(4097) * 10.0 ** rng.integers(-42, 30, 4097)).astype(np.float32)  # denormals included
    x[::97] = np.inf
    x[5::131] = -np.inf
    got, nonfinite = VR.order_stats(x, np.arange(x.size))
    assert np.array_equal(_bits(got), _bits(np.sort(x))) and nonfinite == np.count_nonzero(~np.isfinite(x))
    # signed zeros: numpy's sort calls them equal, so the values agree everywhere and the bits outside the run of zeros; inside it
    # the restatement has -0.0 first
    z = rng.choice(np.array([0.0, -0.0, 1.5, -1.5], np.float32), 257)
    got, _ = VR.order_stats(z, np.arange(z.size))
    ref = np.sort(z)
    assert np.array_equal(got, ref) and np.array_equal(_bits(got)[ref != 0], _bits(ref)[ref != 0])
    zeros = got[got == 0]
    assert (np.diff(np.signbit(zeros).astype(int)) <= 0).all() and np.signbit(zeros).any() and not np.signbit(zeros).all()
    nan = np.array([1.0, np.nan, -2.0, -np.nan], np.float32)
    got, nonfinite = VR.order_stats(nan, (0, 1, 2, 3))
    assert nonfinite == 2 and np.array_equal(got[:2], [-2.0, 1.0]) and np.isnan(got[2:]).all()


def test_magma_header_is_matplotlibs_table():
    src = open(os.path.join(ROOT, "gs-2m_amd", "csrc", "view_maps_magma.h")).read()
    words = np.array([int(w, 16) for w in re.findall(r"0x([0-9A-F]{8})u", src)], dtype=np.uint32)
    assert words.size == 256
    rgba = words.view(np.uint8).reshape(256, 4)
    assert np.array_equal(rgba[:, :3], VR.magma_table()) and (rgba[:, 3] == 255).all()


def test_library_exports_the_map_entry_points():
    import gs2m_native
    if not os.path.exists(gs2m_native.LIB_PATH):
        gs2m_native.build()
    lib = ctypes.CDLL(gs2m_native.LIB_PATH)
    for name in ("gs2m_order_stats_workspace_bytes", "gs2m_order_stats", "gs2m_depth_colorize", "gs2m_pack_image"):
        assert name in gs2m_native.SIGNATURES and hasattr(lib, name), name
    nbytes = ctypes.c_longlong(-1)
    q = lib.gs2m_order_stats_workspace_bytes
    q.restype, q.argtypes = gs2m_native.SIGNATURES["gs2m_order_stats_workspace_bytes"]
    assert q(1200 * 1600, 4, ctypes.byref(nbytes)) == 0 and nbytes.value > 0  # a host query: no device needed
    for n, k in ((0, 1), (2 ** 31, 1), (10, 0), (10, 9)):
        assert q(n, k, ctypes.byref(nbytes)) == -1, (n, k)


def test_wrappers_refuse_cpu_tensors():
    import torch
    import gs2m_render as GR
    with pytest.raises(RuntimeError, match="no CPU path"):
        GR.order_stats(torch.zeros(8), (0,))
    with pytest.raises(RuntimeError, match="no CPU path"):
        GR.depth_image(torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        GR.pack_image(torch.zeros(3, 4, 4))


def test_command_line_presets():
    import gs2m_render as GR
    a, bounds = GR.parse_args(["--ply", "out/point_cloud/iteration_7000/point_cloud.ply", "-s", "data", "-m", "out/Barn", "--tnt"])
    assert (a.iteration, a.label, a.max_depth, a.extract_mesh, a.skip_test, a.filter_depth, a.normal_world) == (7000, "ours", 3.0, True, True, True, False)
    assert bounds is None and a.voxel_size == 0.002 and a.sdf_trunc == 4.0 * 0.002
    a, _ = GR.parse_args(["--ply", "p.ply", "-s", "d", "-m", "m", "--iteration", "3", "--blender"])
    assert (a.skip_train, a.skip_test, a.normal_world, a.extract_mesh, a.max_depth, a.voxel_size) == (True, False, True, True, 8.0, 0.004)
    a, _ = GR.parse_args(["--ply", "p.ply", "-s", "d", "-m", "m", "--iteration", "3", "--dtu"])
    assert (a.skip_test, a.extract_mesh, a.max_depth, a.voxel_size, a.sdf_trunc) == (True, True, 5.0, 0.002, 0.008)
    with pytest.raises(SystemExit):
        GR.parse_args(["--ply", "p.ply", "-s", "d", "-m", "m"])  # no iteration to be found
