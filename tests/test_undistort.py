"""The undistortion contract without a GPU (include/gs2m_undistort.h, csrc/undistort_model.h): the numpy
restatement's own properties, the host entry point gs2m_undistort_camera against it bit for bit, and the conditions the GPU
comparison of tests/test_undistort_gpu.py rests on."""
import ctypes as C
import os

import numpy as np
import pytest

import undistort_ref as R

# (name, COLMAP model, distortion coefficients behind the intrinsics).  In this contract's sign convention a negative k1 pulls
# the distorted image inwards (barrel): its undistorted borders bulge outwards and blank_pixels = 1 grows the output.
COEFFS = [
    ("SIMPLE_PINHOLE", "SIMPLE_PINHOLE", []),
    ("PINHOLE", "PINHOLE", []),
    ("SIMPLE_RADIAL-barrel", "SIMPLE_RADIAL", [-0.08]),
    ("SIMPLE_RADIAL-pincushion", "SIMPLE_RADIAL", [0.1]),
    ("RADIAL-barrel", "RADIAL", [-0.1, 0.02]),
    ("RADIAL-pincushion", "RADIAL", [0.1, 0.02]),
    ("OPENCV-barrel", "OPENCV", [-0.25, 0.03, 0.003, -0.002]),
    ("OPENCV-pincushion", "OPENCV", [0.12, 0.01, -0.002, 0.003]),
    ("FULL_OPENCV-barrel", "FULL_OPENCV", [-0.1, 0.02, 0.003, -0.002, 0.01, 0.05, 0.01, 0.002]),
    ("FULL_OPENCV-pincushion", "FULL_OPENCV", [0.15, 0.02, -0.002, 0.003, 0.01, 0.02, 0.01, 0.002]),
]
SIZES = [(1, 1), (2, 2), (3, 5), (37, 23)]
SINGLE_FOCAL = ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL")


def params_for(model, coeffs, w, h):
    """intrinsics scaled to the image (a focal length near its longer side, the principal point off the centre) + the coefficients"""
    s = float(max(w, h))
    focal = [1.08 * s] if model in SINGLE_FOCAL else [1.08 * s, 1.13 * s]
    return np.array(focal + [0.49 * w + 0.1, 0.52 * h - 0.05] + list(coeffs), dtype=np.float64)


CASES = [(f"{name}-{w}x{h}", model, params_for(model, co, w, h), w, h) for name, model, co in COEFFS for w, h in SIZES]
BLANKS = (0.0, 0.5, 1.0)


def _lib():
    import gs2m_native
    if not os.path.exists(gs2m_native.LIB_PATH):
        gs2m_native.build()
    return gs2m_native.lib()


def host_camera(model_id, w, h, params, blank=0.0, min_scale=0.2, max_scale=2.0, sentinel=-7):
    """gs2m_undistort_camera through ctypes -> (rc, out_w, out_h, float64[4]); the outputs start as `sentinel`"""
    ow, oh = C.c_int(sentinel), C.c_int(sentinel)
    q = (C.c_double * 4)(*[float(sentinel)] * 4)
    p = None if params is None else (C.c_double * max(1, len(params)))(*[float(v) for v in params])
    rc = _lib().gs2m_undistort_camera(model_id, w, h, p, blank, min_scale, max_scale, C.byref(ow), C.byref(oh), q)
    return rc, ow.value, oh.value, np.array(list(q))


@pytest.mark.parametrize("name,model,coeffs", COEFFS, ids=[c[0] for c in COEFFS])
def test_distort_of_undistort_is_the_identity(name, model, coeffs):
    m = R.Model(R.MODEL_IDS[model], params_for(model, coeffs, 37, 23))
    worst = 0.0
    for y in np.linspace(0.0, 23.0, 9):
        for x in np.linspace(0.0, 37.0, 9):
            tu, tv = (x - m.cx) / m.fx, (y - m.cy) / m.fy
            u, v, ok = R.undistort(m, tu, tv)
            assert ok
            pu, pv = R.distort(m, u, v)
            worst = max(worst, abs(pu - tu), abs(pv - tv))
    assert worst <= 1e-12


@pytest.mark.parametrize("model", ["SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV"])
def test_zero_coefficients_are_the_identity(model):
    mid = R.MODEL_IDS[model]
    p = params_for(model, [0.0] * (R.N_PARAMS[mid] - (3 if model in SINGLE_FOCAL else 4)), 37, 23)
    m = R.Model(mid, p)
    for blank in BLANKS:
        ow, oh, q = R.camera(mid, 37, 23, p, blank)
        assert (ow, oh) == (37, 23) and q.tolist() == [m.fx, m.fy, m.cx, m.cy]
        rc, hw, hh, hq = host_camera(mid, 37, 23, p, blank)
        assert (rc, hw, hh) == (0, 37, 23) and hq.tobytes() == q.tobytes()
    src = np.random.default_rng(0).integers(0, 256, (2, 23, 37, 3), dtype=np.uint8)
    dst, valid = R.images(mid, p, src, q, 37, 23)
    assert np.array_equal(dst, src) and valid.min() == 255


@pytest.mark.parametrize("name,model,params,w,h", CASES, ids=[c[0] for c in CASES])
def test_host_camera_equals_the_restatement(name, model, params, w, h):
    """gs2m_undistort_camera (host only: the library is loaded, no GPU is touched) against undistort_ref.camera, bit for bit; and
    the condition of the GPU comparison: the restatement's Newton converges on every border sample"""
    mid = R.MODEL_IDS[model]
    for blank in BLANKS:
        stats = {}
        want = R.camera(mid, w, h, params, blank, stats=stats)
        assert want is not None and stats.get("failed", 0) == 0
        rc, ow, oh, q = host_camera(mid, w, h, params, blank)
        assert rc == 0 and (ow, oh) == want[:2], (blank, ow, oh, want)
        assert q.tobytes() == want[2].tobytes()


def test_host_camera_scale_clamps():
    mid, p = R.MODEL_IDS["OPENCV"], params_for("OPENCV", COEFFS[7][2], 3, 5)
    for lo, hi in ((0.2, 0.2), (2.0, 2.0), (1.5, 1.5)):
        want = R.camera(mid, 3, 5, p, 0.0, lo, hi)
        rc, ow, oh, q = host_camera(mid, 3, 5, p, 0.0, lo, hi)
        assert rc == 0 and (ow, oh) == want[:2] and q.tobytes() == want[2].tobytes()
    assert R.camera(mid, 3, 5, p, 0.0, 0.2, 0.2)[:2] == (1, 1)  # (int)(0.2 * 3) = 0 -> 1: the 1 x 1 output of the GPU test
    assert R.camera(mid, 3, 5, p, 0.0, 2.0, 2.0)[:2] == (6, 10)


def test_barrel_with_blank_pixels_grows_the_output_and_leaves_invalid_pixels():
    """the larger-than-the-source case of the GPU test exists: black pixels and valid = 0 occur"""
    mid, p = R.MODEL_IDS["OPENCV"], params_for("OPENCV", COEFFS[6][2], 37, 23)
    ow, oh, q = R.camera(mid, 37, 23, p, 1.0)
    assert ow > 37 and oh > 23
    _, valid = R.images(mid, p, np.full((1, 23, 37, 1), 200, np.uint8), q, ow, oh)
    assert valid.min() == 0 and valid.max() == 255


def test_refused_models_and_bad_arguments_leave_the_outputs_untouched():
    mid, p = R.MODEL_IDS["OPENCV"], params_for("OPENCV", COEFFS[6][2], 37, 23)
    nan_p, zero_f = p.copy(), p.copy()
    nan_p[4], zero_f[0] = np.nan, 0.0
    bad = [(m, 37, 23, [0.1] * 12, 0.0, 0.2, 2.0) for m in (5, 7, 8, 9, 10, -1, 11)]
    bad += [(mid, 0, 23, p, 0.0, 0.2, 2.0), (mid, 37, 0, p, 0.0, 0.2, 2.0), (mid, 37, 23, None, 0.0, 0.2, 2.0), (mid, 37, 23, p, -0.1, 0.2, 2.0),
            (mid, 37, 23, p, 1.5, 0.2, 2.0), (mid, 37, 23, p, 0.0, 0.0, 2.0), (mid, 37, 23, p, 0.0, 0.5, 0.4), (mid, 37, 23, p, 0.0, 0.2, float("inf")),
            (mid, 37, 23, p, 0.0, 0.2, 1e9), (mid, 37, 23, nan_p, 0.0, 0.2, 2.0), (mid, 37, 23, zero_f, 0.0, 0.2, 2.0)]
    for args in bad:
        rc, ow, oh, q = host_camera(*args)
        assert rc == -1 and (ow, oh) == (-7, -7) and q.tolist() == [-7.0] * 4, args
        if args[3] is not None:
            assert R.camera(*args) is None, args


def test_python_errors_name_the_model():
    import gs2m_colmap
    import gs2m_undistort as U
    for model, n in (("OPENCV_FISHEYE", 8), ("FOV", 5), ("SIMPLE_RADIAL_FISHEYE", 4), ("RADIAL_FISHEYE", 5), ("THIN_PRISM_FISHEYE", 12)):
        with pytest.raises(ValueError, match=model):
            U.undistort_camera(gs2m_colmap.Camera(1, model, 37, 23, np.full(n, 0.1)))
    with pytest.raises(ValueError, match="blank_pixels"):
        U.undistort_camera(gs2m_colmap.Camera(1, "OPENCV", 37, 23, params_for("OPENCV", COEFFS[6][2], 37, 23)), blank_pixels=2.0)


@pytest.mark.parametrize("name,model,coeffs", [c for c in COEFFS if c[2]], ids=[c[0] for c in COEFFS if c[2]])
def test_affine_field_comes_back_within_the_bilinear_bound(name, model, coeffs):
    """an affine intensity field on the undistorted plane, seen through `distort` as a source image, warps back to the field"""
    w, h = 37, 23
    mid, p = R.MODEL_IDS[model], params_for(model, coeffs, w, h)
    a, b, c = 120.0, 150.0, -90.0
    field, src = R.affine_field_source(mid, p, w, h, (a, b, c))
    ow, oh, q = R.camera(mid, w, h, p, 0.0)
    dst, valid = R.images(mid, p, src, q, ow, oh)
    x, y = np.meshgrid(np.arange(ow, dtype=np.float64), np.arange(oh, dtype=np.float64))
    want = a + b * ((x + 0.5 - q[2]) / q[0]) + c * ((y + 0.5 - q[3]) / q[1])
    err = np.abs(dst[0, :, :, 0].astype(np.float64) - want)[valid == 255]
    bound = R.bilinear_bound(field)
    assert err.size > 0.8 * ow * oh and bound < 1.5
    assert err.max() <= bound, (err.max(), bound)


def observations(model, w, h, n, seed=0):
    """n observations of a w x h image for the points tests; from n >= 63 on, two are placed to fail: one far beyond the fold of
    the barrel model (SIMPLE_RADIAL: the iteration runs out of steps) or at 1e200 (r^2 overflows: a non-finite determinant)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform([0.0, 0.0], [float(w), float(h)], (n, 2))
    if n >= 63:
        xy[7] = (-10.8 * w, -2.6 * h) if model == "SIMPLE_RADIAL" else (-1e200, 3.0)
        xy[n - 2] = (1e200, 3.0)
    return xy


POINT_COUNTS = (0, 1, 63, 64, 65, 1000)
POINT_CASES = [c for c in COEFFS if c[0] in ("PINHOLE", "SIMPLE_RADIAL-barrel", "RADIAL-pincushion", "OPENCV-barrel", "FULL_OPENCV-barrel")]


@pytest.mark.parametrize("name,model,coeffs", POINT_CASES, ids=[c[0] for c in POINT_CASES])
def test_observations_converge_except_the_placed_ones(name, model, coeffs):
    """the condition of the GPU comparison of the points kernel: exactly the two placed observations fail in the restatement"""
    mid, p = R.MODEL_IDS[model], params_for(model, coeffs, 37, 23)
    _, _, q = R.camera(mid, 37, 23, p)
    for n in POINT_COUNTS:
        out, failed = R.points(mid, p, q, observations(model, 37, 23, n))
        assert failed == (0 if n < 63 or model == "PINHOLE" else 2), (n, failed)
        assert out.shape == (n, 2)


def test_model_round_trip_through_write_model(tmp_path):
    """write_model -> read -> undistort_model -> write_model -> read: colmap_cameras refuses the distorted model and accepts the
    undistorted one, whose focal lengths are the distorted camera's"""
    import gs2m_colmap as K
    import gs2m_undistort as U
    cams = [K.Camera(1, "OPENCV", 37, 23, params_for("OPENCV", COEFFS[6][2], 37, 23)), K.Camera(2, "SIMPLE_RADIAL", 37, 23, params_for("SIMPLE_RADIAL", [-0.08], 37, 23)),
            K.Camera(3, "SIMPLE_PINHOLE", 37, 23, params_for("SIMPLE_PINHOLE", [], 37, 23))]
    images = [K.Image(k + 1, np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.1 * k, 0.0, 2.0]), 1 + k % 3, f"v{k}.png", None, None) for k in range(4)]
    K.write_model(str(tmp_path / "d"), cams, images, np.zeros((2, 3)), np.zeros((2, 3), np.uint8))
    intr, extr = K.read_intrinsics_binary(str(tmp_path / "d" / "cameras.bin")), K.read_extrinsics_binary(str(tmp_path / "d" / "images.bin"))
    with pytest.raises(ValueError, match="Unsupported COLMAP camera model"):
        K.colmap_cameras(extr, intr)
    out_cams, out_images = U.undistort_model(intr, extr, observations=False)
    K.write_model(str(tmp_path / "u"), out_cams.values(), out_images.values(), np.zeros((2, 3)), np.zeros((2, 3), np.uint8))
    intr2 = K.read_intrinsics_binary(str(tmp_path / "u" / "cameras.bin"))
    infos = K.colmap_cameras(K.read_extrinsics_binary(str(tmp_path / "u" / "images.bin")), intr2)
    assert len(infos) == 4
    for c in cams:
        ow, oh, q = R.camera(R.MODEL_IDS[c.model], c.width, c.height, c.params)
        o = intr2[c.id]
        assert o.model == "PINHOLE" and (o.width, o.height) == (ow, oh) and o.params.tobytes() == q.tobytes()
    for info in infos:
        m = R.Model(R.MODEL_IDS[cams[info.uid - 1].model], cams[info.uid - 1].params)
        assert (info.Fx, info.Fy) == (m.fx, m.fy)


def test_loader_flag_is_device_only():
    """--undistort beside add_ingest_arguments: it selects load_colmap_dataset's `undistort` route, and without --device-ingest
    it is a ValueError like the other device-only flags; every default is unchanged"""
    import argparse
    import gs2m_ingest
    ap = argparse.ArgumentParser()
    gs2m_ingest.add_ingest_arguments(ap)
    assert gs2m_ingest.ingest_keywords(ap.parse_args([])) == dict(ingest="host", masks="", mask_gt=False)
    assert gs2m_ingest.ingest_keywords(ap.parse_args(["--device-ingest"])) == dict(ingest="device", masks="", mask_gt=False)
    assert gs2m_ingest.ingest_keywords(ap.parse_args(["--device-ingest", "--undistort"]))["ingest"] == "undistort"
    with pytest.raises(ValueError, match="--undistort needs --device-ingest"):
        gs2m_ingest.ingest_keywords(ap.parse_args(["--undistort"]))
