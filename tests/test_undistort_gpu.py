"""The undistortion kernels on the GPU (csrc/undistort.hip) against the numpy restatement: bytes, the valid mask, the fp64
observations and the failure count are held to EQUALITY -- the arithmetic is IEEE + - * / in fp64 evaluated as written, so a
difference is a bug, not a tolerance.  Then the command line and the loader option on a four-view synthetic dataset."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest
import torch

import undistort_ref as R
from test_undistort import CASES, COEFFS, POINT_CASES, POINT_COUNTS, observations, params_for

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _cam(model, params, w, h, cid=1):
    import gs2m_colmap
    return gs2m_colmap.Camera(cid, model, w, h, np.asarray(params, dtype=np.float64))


def _source(n, h, w, ch, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, ch), dtype=np.uint8)


def _warp(model, params, src, out_cam, valid=True):
    import gs2m_undistort as U
    n, h, w, ch = src.shape
    out = U.undistort_images(torch.from_numpy(src).to(DEV), _cam(model, params, w, h), out_cam, valid=valid)
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) if valid else out.cpu().numpy()


@pytest.mark.parametrize("name,model,params,w,h", CASES, ids=[c[0] for c in CASES])
def test_images_equal_the_restatement(name, model, params, w, h):
    """every model at 1 x 1, 2 x 2, 3 x 5 and 37 x 23, one and three channels, batches of 1 and 3, blank_pixels 0 and 1"""
    import gs2m_undistort as U
    mid = R.MODEL_IDS[model]
    for blank in (0.0, 1.0):
        oc = U.undistort_camera(_cam(model, params, w, h), blank)
        for ch, n in ((1, 1), (3, 3), (1, 3), (3, 1)):
            src = _source(n, h, w, ch, seed=ch * 10 + n)
            want, want_valid = R.images(mid, params, src, oc.params, oc.width, oc.height)
            got, got_valid = _warp(model, params, src, oc)
            assert got.shape == want.shape and np.array_equal(got, want), (blank, ch, n)
            assert np.array_equal(got_valid, want_valid), (blank, ch, n)


def test_output_larger_than_the_source_has_black_invalid_pixels():
    import gs2m_undistort as U
    model, co = "OPENCV", COEFFS[6][2]
    p = params_for(model, co, 37, 23)
    oc = U.undistort_camera(_cam(model, p, 37, 23), blank_pixels=1.0)
    assert oc.width > 37 and oc.height > 23
    src = np.maximum(_source(3, 23, 37, 3, seed=5), 1)  # no zero byte in the source: every zero of the output is an outside pixel
    got, valid = _warp(model, p, src, oc)
    want, want_valid = R.images(R.MODEL_IDS[model], p, src, oc.params, oc.width, oc.height)
    assert np.array_equal(got, want) and np.array_equal(valid, want_valid)
    assert (valid == 0).any() and (valid == 255).any() and set(np.unique(valid)) == {0, 255}
    assert (got[:, valid == 0] == 0).all() and (got[:, valid == 255] > 0).all()


def test_one_by_one_output_from_the_min_scale_clamp():
    import gs2m_undistort as U
    model, p = "OPENCV", params_for("OPENCV", COEFFS[7][2], 3, 5)
    oc = U.undistort_camera(_cam(model, p, 3, 5), min_scale=0.2, max_scale=0.2)
    assert (oc.width, oc.height) == (1, 1)
    src = _source(3, 5, 3, 3, seed=6)
    got, valid = _warp(model, p, src, oc)
    want, want_valid = R.images(R.MODEL_IDS[model], p, src, oc.params, 1, 1)
    assert np.array_equal(got, want) and np.array_equal(valid, want_valid)


def test_position_exactly_on_the_last_column_and_row():
    """dyadic intrinsics and an output camera shifted by one pixel: output (x, y) reads source (x + 1, y + 1) EXACTLY, so column
    w - 2 sits on the w - 1 edge (valid, the source's last column, no tap outside) and column w - 1 is outside"""
    import gs2m_undistort as U
    w, h = 37, 23
    p = np.array([32.0, 64.0, 18.5, 11.5, 0.0, 0.0, 0.0, 0.0])
    oc = _cam("PINHOLE", [32.0, 64.0, 17.5, 10.5], w, h)
    sx, sy = R.source_positions(4, p, oc.params, w, h)
    assert sx[0, w - 2] == w - 1 and sy[h - 2, 0] == h - 1
    src = np.maximum(_source(2, h, w, 3, seed=7), 1)
    got, valid = _warp("OPENCV", p, src, oc)
    want, want_valid = R.images(4, p, src, oc.params, w, h)
    assert np.array_equal(got, want) and np.array_equal(valid, want_valid)
    assert np.array_equal(got[:, :h - 1, :w - 1], src[:, 1:, 1:]) and (valid[:h - 1, :w - 1] == 255).all()
    assert (valid[:, w - 1] == 0).all() and (valid[h - 1, :] == 0).all() and (got[:, :, w - 1] == 0).all()


def test_zero_coefficients_copy_the_image():
    import gs2m_undistort as U
    p = params_for("OPENCV", [0.0] * 4, 37, 23)
    cam = _cam("OPENCV", p, 37, 23)
    oc = U.undistort_camera(cam)
    assert (oc.width, oc.height) == (37, 23)
    src = _source(2, 23, 37, 3, seed=8)
    got, valid = _warp("OPENCV", p, src, oc)
    assert np.array_equal(got, src) and valid.min() == 255


def test_runs_and_batches_are_bitwise_identical():
    import gs2m_undistort as U
    model, p = "FULL_OPENCV", params_for("FULL_OPENCV", COEFFS[8][2], 37, 23)
    oc = U.undistort_camera(_cam(model, p, 37, 23), 0.5)
    src = _source(3, 23, 37, 3, seed=9)
    a, va = _warp(model, p, src, oc)
    b, vb = _warp(model, p, src, oc)
    assert np.array_equal(a, b) and np.array_equal(va, vb)
    for k in range(3):
        one, vk = _warp(model, p, src[k:k + 1], oc)
        assert np.array_equal(one[0], a[k]) and np.array_equal(vk, va)
    xy = observations(model, 37, 23, 1000)
    cam = _cam(model, p, 37, 23)
    o1, f1 = U.undistort_points(xy, cam, oc)
    o2, f2 = U.undistort_points(xy, cam, oc)
    assert o1.tobytes() == o2.tobytes() and f1 == f2


@pytest.mark.parametrize("name,model,coeffs", POINT_CASES, ids=[c[0] for c in POINT_CASES])
def test_points_equal_the_restatement(name, model, coeffs):
    import gs2m_undistort as U
    p = params_for(model, coeffs, 37, 23)
    cam = _cam(model, p, 37, 23)
    oc = U.undistort_camera(cam)
    for n in POINT_COUNTS:
        xy = observations(model, 37, 23, n)
        want, want_failed = R.points(R.MODEL_IDS[model], p, oc.params, xy)
        got, failed = U.undistort_points(xy, cam, oc)
        assert got.shape == (n, 2) and failed == want_failed, (n, failed, want_failed)
        assert got.tobytes() == want.tobytes(), n
    t = torch.from_numpy(observations(model, 37, 23, 65)).to(DEV)  # device tensors stay on the device
    got, failed = U.undistort_points(t, cam, oc)
    assert got.is_cuda and failed.is_cuda and got.cpu().numpy().tobytes() == R.points(R.MODEL_IDS[model], p, oc.params, t.cpu().numpy())[0].tobytes()


def test_every_error_leaves_the_outputs_untouched():
    import gs2m_native as N
    L = N.lib()
    p = (C.c_double * 12)(*([40.0, 42.0, 18.2, 11.9, -0.1, 0.02, 0.003, -0.002] + [0.0] * 4))
    q = (C.c_double * 4)(40.0, 42.0, 18.0, 11.0)
    src = torch.full((2, 23, 37, 3), 9, dtype=torch.uint8, device=DEV)
    dst = torch.full((2, 23, 37, 3), 77, dtype=torch.uint8, device=DEV)
    valid = torch.full((23, 37), 77, dtype=torch.uint8, device=DEV)
    s = N.stream_ptr()

    def images(model=4, params=p, w=37, h=23, ch=3, n=2, sp=src.data_ptr(), qq=q, ow=37, oh=23, dp=dst.data_ptr()):
        return L.gs2m_undistort_images_u8(model, params, w, h, ch, n, sp, qq, ow, oh, dp, valid.data_ptr(), s)

    for model in (5, 7, 8, 9, 10, -1, 11):
        assert images(model=model) == -1
    for kw in (dict(params=None), dict(w=0), dict(h=0), dict(ch=2), dict(ch=4), dict(n=0), dict(sp=None), dict(qq=None), dict(ow=0), dict(oh=0), dict(dp=None)):
        assert images(**kw) == -1, kw
    assert images(oh=262141) == -4
    xy = torch.full((8, 2), 5.0, dtype=torch.float64, device=DEV)
    out = torch.full((8, 2), 77.0, dtype=torch.float64, device=DEV)
    failed = torch.full((1,), 77, dtype=torch.int32, device=DEV)

    def points(n=8, xp=xy.data_ptr(), model=4, params=p, qq=q, op=out.data_ptr(), fp=failed.data_ptr()):
        return L.gs2m_undistort_points(n, xp, model, params, qq, op, fp, s)

    for kw in (dict(n=-1), dict(xp=None), dict(model=5), dict(model=10), dict(params=None), dict(qq=None), dict(op=None), dict(fp=None)):
        assert points(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (dst == 77).all() and (valid == 77).all() and (out == 77.0).all() and int(failed) == 77
    assert points(n=0, xp=None, op=None) == 0  # n = 0 is valid: the count is zeroed
    torch.cuda.synchronize()
    assert int(failed) == 0 and (out == 77.0).all()
    import gs2m_undistort as U
    with pytest.raises(RuntimeError, match="no CPU path"):
        U.undistort_images(torch.zeros((1, 23, 37, 3), dtype=torch.uint8), _cam("PINHOLE", [40.0, 42.0, 18.0, 11.0], 37, 23), _cam("PINHOLE", [40.0, 42.0, 18.0, 11.0], 37, 23))


# ---- the command line and the loader on a four-view synthetic dataset ---------------------------------------------------------
W, H = 61, 47


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """a raw reconstruction as the mapper leaves it: distorted/sparse/0 (one OPENCV and one SIMPLE_RADIAL camera, four views with
    observations) + input/*.png; undistorted once through the command line with the valid masks written"""
    from PIL import Image as PILImage
    import gs2m_colmap as K
    import gs2m_undistort as U
    root = tmp_path_factory.mktemp("undistort_scene")
    cams = [K.Camera(1, "OPENCV", W, H, params_for("OPENCV", COEFFS[6][2], W, H)), K.Camera(2, "SIMPLE_RADIAL", W, H, params_for("SIMPLE_RADIAL", [0.1], W, H))]
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H, 0:W]
    images, pixels = [], {}
    os.makedirs(root / "input")
    for k in range(4):
        a = 0.3 * k
        qv = np.array([np.cos(a / 2), 0.0, np.sin(a / 2), 0.0])
        xys = rng.uniform([0.0, 0.0], [W, H], (20 + k, 2))
        images.append(K.Image(k + 1, qv, np.array([0.1 * k, 0.0, 3.0]), 1 + k % 2, f"view_{k}.png", xys, np.arange(1, 21 + k)))
        img = np.stack([(xx * 4 + k * 20) % 256, (yy * 5 + xx) % 256, (xx * yy + k) % 256], axis=2).astype(np.uint8)
        img = np.maximum(img, 1)
        pixels[f"view_{k}.png"] = img
        PILImage.fromarray(img).save(root / "input" / f"view_{k}.png")
    K.write_model(str(root / "distorted" / "sparse" / "0"), cams, images, rng.uniform(-1, 1, (30, 3)), rng.integers(0, 256, (30, 3)))
    assert U.main(["-s", str(root), "--write-valid", "valid"]) == 0
    return dict(root=str(root), cams={c.id: c for c in cams}, images=images, pixels=pixels)


def _check_written(root, scene, images_dir="images", model_dir="sparse/0"):
    from PIL import Image as PILImage
    import gs2m_colmap as K
    intr = K.read_intrinsics_binary(os.path.join(root, model_dir, "cameras.bin"))
    extr = K.read_extrinsics_binary(os.path.join(root, model_dir, "images.bin"))
    for cid, c in scene["cams"].items():
        ow, oh, q = R.camera(R.MODEL_IDS[c.model], W, H, c.params)
        assert intr[cid].model == "PINHOLE" and (intr[cid].width, intr[cid].height) == (ow, oh) and intr[cid].params.tobytes() == q.tobytes()
    for im in scene["images"]:
        c, o = scene["cams"][im.camera_id], intr[im.camera_id]
        want, valid = R.images(R.MODEL_IDS[c.model], c.params, scene["pixels"][im.name][None], o.params, o.width, o.height)
        assert np.array_equal(np.asarray(PILImage.open(os.path.join(root, images_dir, im.name))), want[0]), im.name
        xy, failed = R.points(R.MODEL_IDS[c.model], c.params, o.params, im.xys)
        assert failed == 0 and extr[im.id].xys.tobytes() == xy.tobytes() and np.array_equal(extr[im.id].point3D_ids, im.point3D_ids)
        assert np.array_equal(extr[im.id].qvec, im.qvec) and np.array_equal(extr[im.id].tvec, im.tvec) and extr[im.id].name == im.name
        if os.path.isdir(os.path.join(root, "valid")):
            assert np.array_equal(np.asarray(PILImage.open(os.path.join(root, "valid", os.path.splitext(im.name)[0] + ".png"))), valid)
    with open(os.path.join(root, "distorted", "sparse", "0", "points3D.bin"), "rb") as f, open(os.path.join(root, model_dir, "points3D.bin"), "rb") as g:
        assert f.read() == g.read()


def test_command_line_writes_the_undistorted_dataset(scene):
    _check_written(scene["root"], scene)


def test_command_line_with_device_png(scene, tmp_path):
    import gs2m_undistort as U
    root = str(tmp_path / "copy")
    shutil.copytree(os.path.join(scene["root"], "distorted"), os.path.join(root, "distorted"))
    shutil.copytree(os.path.join(scene["root"], "input"), os.path.join(root, "input"))
    assert U.main(["-s", root, "--device-png"]) == 0
    _check_written(root, scene)


def test_loader_reads_the_written_dataset_and_undistort_gives_the_same_tensors(scene):
    import gs2m_train as T
    written = T.load_colmap_dataset(scene["root"], resolution=2, ingest="device", masks="valid", ncc_scale=1.0)
    memory = T.load_colmap_dataset(scene["root"], resolution=2, ingest="undistort", ncc_scale=1.0)
    assert len(written[0]) == len(memory[0]) == 4
    for ca, cb, ga, gb in zip(written[0], memory[0], written[1], memory[1]):
        assert (ca.image_width, ca.image_height, ca.Fx, ca.Fy) == (cb.image_width, cb.image_height, cb.Fx, cb.Fy)
        assert torch.equal(ga, gb) and torch.equal(ca.alpha_mask, cb.alpha_mask) and torch.equal(ca.gray_image, cb.gray_image)
        assert torch.equal(ca.world_view_transform, cb.world_view_transform)
    assert np.array_equal(written[2], memory[2]) and written[4] == memory[4]
    plain = T.load_colmap_dataset(scene["root"], resolution=1, ingest="device")  # the written dataset, as any loader call reads it
    assert plain[1][0].shape[0] == 3 and len(plain[0]) == 4


def test_default_loader_still_refuses_a_distorted_model(scene, tmp_path):
    import gs2m_train as T
    root = str(tmp_path / "raw")
    shutil.copytree(os.path.join(scene["root"], "distorted", "sparse"), os.path.join(root, "sparse"))
    shutil.copytree(os.path.join(scene["root"], "input"), os.path.join(root, "images"))
    for kw in (dict(), dict(ingest="device")):
        with pytest.raises(ValueError, match="Unsupported COLMAP camera model"):
            T.load_colmap_dataset(root, **kw)
    cams, gts, _, _, _ = T.load_colmap_dataset(root, ingest="undistort")  # sparse/0 + images, undistorted in memory
    assert len(cams) == 4 and gts[0].shape[1] < H + 1
