"""Dataset ingestion without a GPU: the numpy restatement tests/ingest_ref.py is held to Pillow's resize (called
here) and to what the reference's process_input_image and loadCam returned (tests/golden/ref_ingest.npz); the library's host-side
resize plan, gs2m_ingest.target_resolution and load_colmap_dataset's keywords are held to the restatement.  Equality throughout:
the arithmetic is integer or fp32 evaluated as written."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import ingest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_ingest.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _images(W, H, seed):
    """a random L image, a random RGB image and a 0 / 255 mask (its resize overshoots on both sides: both clamps run)"""
    rng = np.random.default_rng(seed)
    return {"L": rng.integers(0, 256, (H, W), dtype=np.uint8), "RGB": rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
            "mask": (rng.integers(0, 2, (H, W)) * 255).astype(np.uint8)}


@pytest.mark.parametrize("src,dst", R.SHAPES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in R.SHAPES])
def test_restatement_equals_pillow_resize(src, dst):
    from PIL import Image
    clamped = set()
    for kind, img in _images(src[0], src[1], seed=src[0] * 1000 + src[1]).items():
        want = np.asarray(Image.fromarray(img).resize(dst))
        got = R.resize(img, dst)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), f"{kind}: {int((got != want).sum())} of {want.size} bytes differ"
        if kind == "mask":
            clamped = {int(want.min()), int(want.max())}
    if src == (64, 48):  # the binary mask drives the accumulator past both ends
        assert clamped == {0, 255}


def test_pillow_default_filter_is_bicubic():
    """what `image.resize(resolution)` of the reference means"""
    from PIL import Image
    img = Image.fromarray(_images(37, 23, 1)["RGB"])
    assert np.array_equal(np.asarray(img.resize((18, 12))), np.asarray(img.resize((18, 12), Image.BICUBIC)))
    assert not np.array_equal(np.asarray(img.resize((18, 12))), np.asarray(img.resize((18, 12), Image.LANCZOS)))


CASES = [("rgb_mask", "rgb", "mask", False), ("rgb_mask_maskgt", "rgb", "mask", True), ("rgba", "rgba", None, False),
         ("rgba_maskgt", "rgba", None, True), ("rgba_mask", "rgba", "mask", False), ("rgba_mask_maskgt", "rgba", "mask", True),
         ("rgb_nomask", "rgb", None, True), ("l", "gray_in", None, False)]


def golden_input(golden, image, mask):
    img = np.dstack([golden["rgb"], golden["alpha"]]) if image == "rgba" else golden[image]
    return np.ascontiguousarray(img), (None if mask is None else golden[mask])


@pytest.mark.parametrize("name,image,mask,mask_gt", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_the_reference(golden, name, image, mask, mask_gt):
    img, m = golden_input(golden, image, mask)
    res = (40, 29) if name == "l" else (50, 38)
    rgb, alpha = R.process_input_image(img, res, mask_gt, m)
    want = golden[name + "_rgb"]
    assert rgb.dtype == np.float32 and rgb.shape == want.shape == ((1 if name == "l" else 3), res[1], res[0])
    assert np.array_equal(rgb.view(np.uint32), want.view(np.uint32))
    if name + "_alpha" in golden:
        assert alpha.dtype == np.float32 and alpha.shape == (1, res[1], res[0])
        assert np.array_equal(alpha.view(np.uint32), golden[name + "_alpha"].view(np.uint32))
    else:
        assert alpha is None
    if name != "l":
        g = R.gray_image(img, res, mask_gt, m)
        assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), golden[name + "_gray"].view(np.uint32))


def test_golden_covers_what_it_should(golden):
    assert golden["mask"].max() == 250 and 0 < np.count_nonzero((golden["mask"] > 0) & (golden["mask"] < 250))  # max(alpha) matters
    assert not np.array_equal(golden["rgb_mask_rgb"], golden["rgb_mask_maskgt_rgb"])
    assert np.array_equal(golden["rgb_mask_alpha"], golden["rgba_mask_alpha"])  # a given mask wins over the alpha channel
    assert not np.array_equal(golden["rgba_alpha"], golden["rgba_mask_alpha"])
    assert np.array_equal(golden["rgb_nomask_rgb"], golden["rgb_mask_rgb"])  # mask_gt without a mask does nothing
    assert golden["rgba_alpha"].max() == 1.0 and golden["rgb_mask_alpha"].max() == 1.0 and golden["rgb_mask_alpha"].min() == 0.0
    rs = {int(r) for r in golden["sizes"][:, 2]}
    assert {1, 2, 4, 8, -1} <= rs and any(r not in (1, 2, 4, 8, -1) for r in rs) and len(golden["sizes"]) >= 12
    wide = golden["sizes"][golden["sizes"][:, 2] == -1][:, 0]
    assert (wide > 1600).any() and (wide <= 1600).any()


def test_target_resolution_equals_loadcam(golden):
    import gs2m_ingest
    for w, h, r, ow, oh in golden["sizes"].tolist():
        assert gs2m_ingest.target_resolution(w, h, r) == (ow, oh), (w, h, r)
        assert R.target_resolution(w, h, r) == (ow, oh), (w, h, r)
    assert gs2m_ingest.target_resolution(1554, 1162, 2, resolution_scale=2.0) == (388, 290)


# ---- the library's host side: it loads and plans without a GPU (tests/test_cabi.py) ------------------------------------
@pytest.fixture(scope="module")
def lib():
    import gs2m_native
    if not os.path.exists(gs2m_native.LIB_PATH):
        gs2m_native.build()
    return gs2m_native.lib()


def _lib_plan(lib, n_in, n_out):
    nbytes, ksize = ctypes.c_longlong(), ctypes.c_int()
    assert lib.gs2m_resize_plan_bytes(n_in, n_out, ctypes.byref(nbytes), ctypes.byref(ksize)) == 0
    assert nbytes.value == 4 * (4 + 2 * n_out + n_out * ksize.value)
    plan = np.full(nbytes.value // 4 + 1, -77, np.int32)
    assert lib.gs2m_resize_plan(n_in, n_out, plan.ctypes.data) == 0
    assert plan[-1] == -77, "gs2m_resize_plan wrote past the size it reports"
    assert plan[:4].tolist() == [n_in, n_out, ksize.value, 0]
    return plan[4:4 + 2 * n_out].reshape(n_out, 2), plan[4 + 2 * n_out:-1].reshape(n_out, ksize.value), ksize.value


def _assert_plan(lib, n_in, n_out):
    bounds, coeffs, ksize = _lib_plan(lib, n_in, n_out)
    rb, rc, rk = R.plan(n_in, n_out)
    assert ksize == rk, (n_in, n_out)
    assert np.array_equal(bounds, rb), (n_in, n_out)
    assert np.array_equal(coeffs, rc), (n_in, n_out)
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 0).all() and (bounds.sum(axis=1) <= n_in).all() and (bounds[:, 1] <= ksize).all()


def test_resize_plan_equals_the_restatement_on_the_shape_list(lib):
    for (W, H), (w, h) in R.SHAPES + [((1554, 1162), (777, 581))]:
        _assert_plan(lib, W, w)
        _assert_plan(lib, H, h)


def test_resize_plan_equals_the_restatement_on_small_axes(lib):
    for n_in in range(1, 41):
        for n_out in range(1, 41):
            _assert_plan(lib, n_in, n_out)


def test_resize_plan_refuses_invalid_sizes(lib):
    nbytes, buf = ctypes.c_longlong(), np.zeros(64, np.int32)
    for n_in, n_out in ((0, 4), (4, 0), (-3, 4), (4, -1), (0, 0)):
        assert lib.gs2m_resize_plan_bytes(n_in, n_out, ctypes.byref(nbytes), None) == -1
        assert lib.gs2m_resize_plan(n_in, n_out, buf.ctypes.data) == -1
    assert lib.gs2m_resize_plan_bytes(4, 4, None, None) == -1 and lib.gs2m_resize_plan(4, 4, None) == -1
    assert not buf.any()
    ws = ctypes.c_longlong(-5)
    assert lib.gs2m_image_resize_workspace_bytes(8, 6, 3, 4, 3, ctypes.byref(ws)) == 0 and ws.value == 4 * 3 * 6
    assert lib.gs2m_image_resize_workspace_bytes(8, 6, 3, 8, 3, ctypes.byref(ws)) == 0 and ws.value == 0
    assert lib.gs2m_image_resize_workspace_bytes(8, 6, 3, 4, 6, ctypes.byref(ws)) == 0 and ws.value == 0
    for args in ((0, 6, 3, 4, 3), (8, 6, 2, 4, 3), (8, 6, 3, 0, 3), (8, 6, 3, 4, -1), (2 ** 30, 6, 3, 4, 3)):
        assert lib.gs2m_image_resize_workspace_bytes(*args, ctypes.byref(ws)) == -1, args


def test_host_plan_wrapper(lib):
    import gs2m_ingest
    plan, bounds, coeffs, ksize = gs2m_ingest.host_plan(101, 50)
    rb, rc, rk = R.plan(101, 50)
    assert ksize == rk and np.array_equal(bounds, rb) and np.array_equal(coeffs, rc) and plan.dtype == np.int32
    with pytest.raises(RuntimeError, match="invalid argument"):
        gs2m_ingest.host_plan(0, 5)


def test_new_exports_are_declared_and_exported(lib):
    import gs2m_native
    names = ("gs2m_resize_plan_bytes", "gs2m_resize_plan", "gs2m_image_max_u8", "gs2m_image_mask_u8", "gs2m_image_resize_workspace_bytes",
             "gs2m_image_resize_u8", "gs2m_image_unpack")
    header = open(os.path.join(ROOT, "include", "gs2m_ingest.h")).read()
    for n in names:
        assert n in gs2m_native.SIGNATURES and hasattr(lib, n) and n + "(" in header, n
    for n in names[2:]:
        if not n.endswith("_bytes"):
            assert gs2m_native.SIGNATURES[n][1][-1] is gs2m_native.STREAM, n


def test_ingest_refuses_cpu_tensors_and_unknown_modes():
    import gs2m_ingest
    from PIL import Image
    t = torch.zeros(8, 8, 3, dtype=torch.uint8)
    for call in (lambda: gs2m_ingest.resize(t, (4, 4)), lambda: gs2m_ingest.image_max(t), lambda: gs2m_ingest.unpack(t),
                 lambda: gs2m_ingest.mask_image(t, t[:, :, 0])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    for mode in ("I;16", "F", "P", "CMYK"):
        with pytest.raises(ValueError, match="mode " + mode):
            gs2m_ingest.process_input_image(Image.new(mode, (8, 8)), (4, 4), device="cpu")
    with pytest.raises(ValueError, match="zero everywhere"):
        gs2m_ingest.stage(np.full((8, 8, 3), 9, np.uint8), True, np.zeros((8, 8), np.uint8), device="cpu", name="view_7.png")
    with pytest.raises(ValueError, match="view_7.png"):
        gs2m_ingest.stage(np.full((8, 8, 3), 9, np.uint8), True, np.zeros((8, 8), np.uint8), device="cpu", name="view_7.png")


# ---- load_colmap_dataset: the default call is what it was ----------------------------------------------------------------
def _write_dataset(folder, n=3, W=64, H=48, seed=5):
    """a COLMAP-format dataset in export_colmap_dataset's format, from numpy arrays, without a GPU -> the images as uint8"""
    import gs2m_synth as S
    import gs2m_train as T
    from gs2m_scene import Camera
    rng = np.random.default_rng(seed)
    cams = [Camera(c, "cpu") for c in S.orbit_cameras(n, W, H, radius=6.0, centre=(0.0, -0.8, 6.0), fx=1.1 * W)]
    u8 = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(n)]
    gts = [torch.from_numpy(a.astype(np.float32) / 255.0).permute(2, 0, 1) for a in u8]
    pts = (rng.random((50, 3)) * 2.0 - 1.0 + np.array([0.0, -0.8, 6.0])).astype(np.float32)  # around the point the cameras look at
    T.export_colmap_dataset(str(folder), (cams, gts, pts, rng.random((50, 3)).astype(np.float32), 1.0))
    return u8


def test_load_colmap_dataset_default_is_unchanged(tmp_path):
    import gs2m_train as T
    from PIL import Image
    sig = inspect.signature(T.load_colmap_dataset)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [("images", "images"), ("device", "cuda"), ("resolution", 1), ("ingest", "host"),
                                                                        ("masks", ""), ("mask_gt", False), ("ncc_scale", None)]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("ingest", "masks", "mask_gt", "ncc_scale"))
    u8 = _write_dataset(tmp_path)
    cams, gts, xyz, rgb, radius = T.load_colmap_dataset(str(tmp_path), device="cpu")
    assert len(cams) == len(gts) == 3 and xyz.shape == (50, 3) and radius > 0
    for cam, gt, a in zip(cams, gts, u8):
        assert (cam.image_width, cam.image_height) == (64, 48) and not hasattr(cam, "alpha_mask") and cam.gray_image is None
        assert torch.equal(gt, torch.from_numpy(a.astype(np.float32) / 255.0).permute(2, 0, 1))
    cams2, gts2, _, _, _ = T.load_colmap_dataset(str(tmp_path), device="cpu", resolution=2, ingest="host")
    for cam, gt, a in zip(cams2, gts2, u8):  # the host route keeps its filter
        want = np.asarray(Image.fromarray(a).resize((32, 24), Image.LANCZOS), dtype=np.float32) / 255.0
        assert (cam.image_width, cam.image_height) == (32, 24) and torch.equal(gt, torch.from_numpy(want).permute(2, 0, 1))
        assert cam.Fx == pytest.approx(cams[0].Fx / 2)


def test_load_colmap_dataset_mask_flags_need_the_device_route(tmp_path):
    import gs2m_train as T
    _write_dataset(tmp_path, n=1)
    with pytest.raises(ValueError, match=r"`masks` needs ingest='device'"):
        T.load_colmap_dataset(str(tmp_path), device="cpu", masks="masks")
    with pytest.raises(ValueError, match=r"`mask_gt` needs ingest='device'"):
        T.load_colmap_dataset(str(tmp_path), device="cpu", mask_gt=True, ingest="host")
    with pytest.raises(ValueError, match=r"`ncc_scale` needs ingest='device'"):
        T.load_colmap_dataset(str(tmp_path), device="cpu", ncc_scale=0.5)
    with pytest.raises(ValueError, match="ingest must be"):
        T.load_colmap_dataset(str(tmp_path), device="cpu", ingest="gpu")


def test_multi_view_scene_takes_gray_images():
    import gs2m_mvs
    import gs2m_synth as S
    from gs2m_scene import Camera
    cams = [Camera(c, "cpu") for c in S.orbit_cameras(3, 16, 12, radius=6.0, centre=(0.0, -0.8, 6.0), fx=18.0)]
    gts = [torch.rand(3, 12, 16) for _ in cams]
    grays = [torch.rand(1, 24, 32) for _ in cams]
    gs2m_mvs.MultiViewScene(cams, gts, None, ncc_scale=0.5, gray_images=grays)
    assert all(torch.equal(c.gray_image, g) for c, g in zip(cams, grays))
    gs2m_mvs.MultiViewScene(cams, gts, None)  # None: formed from the training images, as before
    assert all(torch.equal(c.gray_image, (t[0:1] * 0.299 + t[1:2] * 0.587 + t[2:3] * 0.114)) for c, t in zip(cams, gts))
    with pytest.raises(ValueError, match="2 gray images for 3 cameras"):
        gs2m_mvs.MultiViewScene(cams, gts, None, gray_images=grays[:2])
