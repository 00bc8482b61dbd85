"""The ingestion kernels (csrc/ingest.hip) and gs2m_ingest on the GPU, held byte for byte and bit for bit to the numpy
restatement tests/ingest_ref.py and to what the reference returned (tests/golden/ref_ingest.npz).  No tolerance anywhere: the
arithmetic is integer or fp32 evaluated as written."""
import os

import numpy as np
import pytest
import torch

import ingest_ref as R
from test_ingest import CASES, GOLDEN, golden_input

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _rand(shape, seed, binary=False):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 2, shape) * 255).astype(np.uint8) if binary else rng.integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("src,dst", R.SHAPES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in R.SHAPES])
def test_resize_equals_the_restatement(src, dst):
    """1 and 3 channels, (H, W) and (H, W, 1) layouts; the list holds both passes, either one alone (50x40 -> 50x13,
    33x20 -> 11x20) and none (the copy); the binary image runs both clamps"""
    import gs2m_ingest
    (W, H), seed = src, src[0] * 1000 + src[1]
    for img in (_rand((H, W), seed), _rand((H, W, 3), seed + 1), _rand((H, W), seed + 2, binary=True), _rand((H, W, 1), seed + 3)):
        got = gs2m_ingest.resize(torch.from_numpy(img).to(DEV), dst)
        want = R.resize(img[:, :, 0], dst)[:, :, None] if img.ndim == 3 and img.shape[2] == 1 else R.resize(img, dst)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), f"{img.shape}: {int((got.cpu().numpy() != want).sum())} of {want.size} bytes differ"


def test_resize_at_the_dtu_size():
    """1554 x 1162 -> 777 x 581: more tiles than workgroups in both passes (the grid-stride loops go round), 13 column tiles and
    3 segments per row"""
    import gs2m_ingest
    img = _rand((1162, 1554, 3), 11)
    img[300:600, 400:900] = _rand((300, 500, 1), 12, binary=True)
    got = gs2m_ingest.resize(torch.from_numpy(img).to(DEV), (777, 581)).cpu().numpy()
    assert np.array_equal(got, R.resize(img, (777, 581)))


def test_resize_reads_taps_from_global_memory_when_they_outgrow_lds():
    """a reduction by more than 63: ksize > 128, the horizontal pass's other path"""
    import gs2m_ingest
    for shape, dst in (((5, 700, 3), (10, 3)), ((4, 333), (2, 4))):
        img = _rand(shape, 21)
        assert gs2m_ingest.host_plan(shape[1], dst[0])[3] > 128
        assert np.array_equal(gs2m_ingest.resize(torch.from_numpy(img).to(DEV), dst).cpu().numpy(), R.resize(img, dst))


def test_resize_refuses_what_it_cannot_do():
    import gs2m_ingest
    t = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="must be > 0"):
        gs2m_ingest.resize(t, (0, 4))
    with pytest.raises(RuntimeError, match="CH 1 or 3"):
        gs2m_ingest.resize(torch.zeros(8, 8, 2, dtype=torch.uint8, device=DEV), (4, 4))
    with pytest.raises(RuntimeError, match="must be uint8"):
        gs2m_ingest.resize(t.float(), (4, 4))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
def test_image_max(n):
    import gs2m_ingest
    base = (_rand((n + 3,), n) // 2).astype(np.uint8)  # below 128
    for where in (0, n - 1):
        for offset in (0, 3):  # an aligned and a misaligned first byte
            a = base.copy()
            a[offset + where] = 200 + (where % 50)
            t = torch.from_numpy(a).to(DEV)[offset:offset + n]
            got = gs2m_ingest.image_max(t)
            assert got.dtype == torch.int32 and got.item() == int(a[offset:offset + n].max()) == 200 + (where % 50)
    assert gs2m_ingest.image_max(torch.zeros(n, dtype=torch.uint8, device=DEV)).item() == 0
    assert gs2m_ingest.image_max(torch.zeros(0, dtype=torch.uint8, device=DEV)).item() == 0


def test_mask_kernel_equals_the_restatement(golden):
    import gs2m_ingest
    rgb, mask = golden["rgb"], golden["mask"]
    for m in (mask, golden["alpha"], np.full_like(mask, 7)):
        got = gs2m_ingest.mask_image(torch.from_numpy(rgb).to(DEV), torch.from_numpy(m).to(DEV)).cpu().numpy()
        assert np.array_equal(got, R.mask_image(rgb, m))
    # a mask that is zero everywhere: the reference divides by zero; here the output is defined -- zeros -- and nothing faults
    out = gs2m_ingest.mask_image(torch.from_numpy(rgb).to(DEV), torch.zeros(mask.shape, dtype=torch.uint8, device=DEV))
    assert out.shape == rgb.shape and not out.any().item()


def test_unpack_kernel_equals_the_restatement(golden):
    import gs2m_ingest
    rgb, mask = golden["rgb"], golden["mask"]
    t, a = torch.from_numpy(rgb).to(DEV), torch.from_numpy(mask).to(DEV)
    want = np.ascontiguousarray((rgb.astype(np.float32) / np.float32(255.)).transpose(2, 0, 1))
    want_alpha = (mask.astype(np.float32) / np.float32(mask.max()))[None]
    o_rgb, o_alpha, o_gray = gs2m_ingest.unpack(t, a, gray=True)
    assert np.array_equal(_bits(o_rgb), want.view(np.uint32))
    assert np.array_equal(_bits(o_alpha), want_alpha.view(np.uint32))
    assert np.array_equal(_bits(o_gray), R.gray(want).view(np.uint32))
    o_rgb, o_alpha, o_gray = gs2m_ingest.unpack(t)  # alpha absent
    assert o_alpha is None and o_gray is None and np.array_equal(_bits(o_rgb), want.view(np.uint32))
    o_rgb, o_alpha, o_gray = gs2m_ingest.unpack(t, rgb=False, gray=True)
    assert o_rgb is None and o_alpha is None and np.array_equal(_bits(o_gray), R.gray(want).view(np.uint32))
    one = gs2m_ingest.unpack(a)[0]  # one channel
    assert tuple(one.shape) == (1,) + mask.shape and np.array_equal(_bits(one), (mask.astype(np.float32) / np.float32(255.))[None].view(np.uint32))
    zeros = gs2m_ingest.unpack(t, torch.zeros_like(a))[1]  # all-zero alpha: defined, zeros
    assert tuple(zeros.shape) == (1,) + mask.shape and not zeros.any().item()
    with pytest.raises(ValueError, match="needs 3 channels"):
        gs2m_ingest.unpack(a, gray=True)


@pytest.mark.parametrize("name,image,mask,mask_gt", CASES, ids=[c[0] for c in CASES])
def test_process_input_image_equals_the_reference(golden, name, image, mask, mask_gt):
    import gs2m_ingest
    from PIL import Image
    img, m = golden_input(golden, image, mask)
    res = (40, 29) if name == "l" else (50, 38)
    for as_pil in (False, True):
        a = Image.fromarray(img) if as_pil else img
        b = (Image.fromarray(m) if as_pil else torch.from_numpy(m)) if m is not None else None
        out = gs2m_ingest.process_input_image(a, res, mask_gt, b, device=DEV, gray=name != "l")
        rgb, alpha = out[0], out[1]
        assert rgb.is_cuda and rgb.dtype == torch.float32 and tuple(rgb.shape) == golden[name + "_rgb"].shape
        assert np.array_equal(_bits(rgb), golden[name + "_rgb"].view(np.uint32))
        if name + "_alpha" in golden:
            assert tuple(alpha.shape) == (1, res[1], res[0]) and np.array_equal(_bits(alpha), golden[name + "_alpha"].view(np.uint32))
        else:
            assert alpha is None
        if name != "l":
            assert np.array_equal(_bits(out[2]), golden[name + "_gray"].view(np.uint32))
            g = gs2m_ingest.gray_image(a, res, mask_gt, b, device=DEV)
            assert tuple(g.shape) == (1, res[1], res[0]) and np.array_equal(_bits(g), golden[name + "_gray"].view(np.uint32))


def test_twice_on_a_side_stream_and_the_plan_cache(golden):
    import gs2m_ingest
    img, m = golden_input(golden, "rgb", "mask")
    gs2m_ingest.plan_cache_clear()
    side = torch.cuda.Stream()
    runs = []
    with torch.cuda.stream(side):
        for _ in range(2):
            runs.append(gs2m_ingest.process_input_image(img, (50, 38), True, m, device=DEV, gray=True))
            if len(runs) == 1:
                first = gs2m_ingest.plan_cache_info()
    side.synchronize()
    info = gs2m_ingest.plan_cache_info()
    assert first == {"hits": 2, "misses": 2, "size": 2}  # image and mask share the two plans of the first call
    assert info == {"hits": 6, "misses": 2, "size": 2}  # the second call builds none
    for x, y, key in zip(runs[0], runs[1], ("rgb", "alpha", "gray")):
        assert torch.equal(x, y)
        assert np.array_equal(_bits(x), golden["rgb_mask_maskgt_" + key].view(np.uint32))


def _write_masked_dataset(folder, n=6, W=64, H=48):
    from PIL import Image
    from test_ingest import _write_dataset
    u8 = _write_dataset(folder, n=n, W=W, H=H, seed=9)
    os.makedirs(os.path.join(folder, "masks"))
    y, x = np.mgrid[0:H, 0:W]
    masks = []
    for k in range(n):
        m = (np.clip((20.0 + k - np.hypot(x - 30.0 - k, y - 24.0)) / 3.0, 0.0, 1.0) * 255.0).astype(np.uint8)
        Image.fromarray(m).save(os.path.join(folder, "masks", f"view_{k:03d}.png"))
        masks.append(m)
    return u8, masks


def test_device_ingest_end_to_end(tmp_path):
    """a 6-view COLMAP-format dataset with masks at -r 2: gt, alpha_mask and gray_image equal the restatement; three iterations
    of train() with the alpha masks and the loader's gray images in the multi-view scene end in a finite loss"""
    import gs2m_mvs
    import gs2m_train as T
    folder = str(tmp_path)
    u8, masks = _write_masked_dataset(folder)
    scene = T.load_colmap_dataset(folder, resolution=2, ingest="device", masks="masks", mask_gt=True, ncc_scale=0.5)
    cams, gts = scene[0], scene[1]
    assert len(cams) == 6
    for cam, gt, a, m in zip(cams, gts, u8, masks):
        rgb, alpha = R.process_input_image(a, (32, 24), True, m)
        assert (cam.image_width, cam.image_height) == (32, 24) and cam.has_mask
        assert np.array_equal(_bits(gt), rgb.view(np.uint32))
        assert np.array_equal(_bits(cam.alpha_mask), alpha.view(np.uint32))
        assert tuple(cam.gray_image.shape) == (1, 48, 64)  # -r 2 with ncc_scale 1 / 2: the original size
        assert np.array_equal(_bits(cam.gray_image), R.gray_image(a, (64, 48), True, m).view(np.uint32))
    # absolute mask folder, no mask_gt, gray images at the training size; then no masks at all: ones
    plain = T.load_colmap_dataset(folder, resolution=2, ingest="device", masks=os.path.join(folder, "masks"), ncc_scale=1.0)
    for cam, gt, a, m in zip(plain[0], plain[1], u8, masks):
        rgb, alpha = R.process_input_image(a, (32, 24), False, m)
        assert np.array_equal(_bits(gt), rgb.view(np.uint32)) and np.array_equal(_bits(cam.alpha_mask), alpha.view(np.uint32))
        assert np.array_equal(_bits(cam.gray_image), R.gray(rgb).view(np.uint32))
    bare = T.load_colmap_dataset(folder, resolution=2, ingest="device")
    assert all(not c.has_mask and c.gray_image is None and torch.equal(c.alpha_mask, torch.ones(1, 24, 32, device=DEV)) for c in bare[0])
    with pytest.raises(ValueError, match="view_000.png"):  # a mask that is zero everywhere names its file
        from PIL import Image
        Image.fromarray(np.zeros((48, 64), np.uint8)).save(os.path.join(folder, "masks", "view_000.png"))
        T.load_colmap_dataset(folder, resolution=2, ingest="device", masks="masks")

    mv = gs2m_mvs.MultiViewParams()
    mv.multi_view_max_dist, mv.multi_view_max_angle, mv.nearby_cam_max_dist = 8.0, 65, 8.0  # the orbit: 6 units out, 60 degrees apart
    grays = [c.gray_image for c in cams]
    model, stats = T.train(iterations=3, scene=scene, geometry_from_iter=0, lambda_multi_view=T.OptimizationParams.lambda_multi_view, mv_opt=mv,
                           alpha_masks=[c.alpha_mask for c in cams], gray_images=grays, ncc_scale=0.5)
    assert np.isfinite(stats["loss_end"]) and len(stats["mv_loss"]) == 3 and all(np.isfinite(v) for v in stats["mv_loss"])
    assert torch.isfinite(model.get_xyz).all().item()
    assert all(c.gray_image.data_ptr() == g.data_ptr() for c, g in zip(cams, grays))  # the scene used the loader's images
