"""csrc/image_metrics.hip through gs2m_metrics.py against the float64 restatement tests/metrics_ref.py: the
squared error exactly, SSIM and PSNR at the bounds tests/test_ssim_gpu.py:54 holds the same operator to.  The shapes are the
smallest at which the tiling can go wrong: below, at and above the window's reach (5, 10, 11, 12) and each tile edge."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import metrics_ref as MR

pytestmark = pytest.mark.gpu

import gs2m_metrics as GM  # noqa: E402

T_W, T_H = GM.TILE_W, GM.TILE_H
HS = (1, 5, 10, 11, 12, T_H - 1, T_H, T_H + 1, 2 * T_H + 3)
WS = (1, 2, 3, 5, 10, 11, 12, T_W - 1, T_W, T_W + 1, 2 * T_W + 3)
# the product pruned: every H and every W at least once, both tile-edge straddles together, the extremes crossed
SHAPES = [(1, 1), (5, 2), (10, 3), (11, 5), (12, 10), (T_H - 1, 11), (T_H, 12), (T_H + 1, T_W - 1), (2 * T_H + 3, T_W),
          (1, T_W + 1), (5, 2 * T_W + 3), (T_H + 1, T_W + 1), (T_H - 1, T_W - 1), (T_H, T_W), (2 * T_H + 3, 2 * T_W + 3),
          (10, 10), (11, 11), (12, 12), (1, 2 * T_W + 3), (2 * T_H + 3, 1), (T_H + 1, 3), (5, 5)]
assert {s[0] for s in SHAPES} == set(HS) and {s[1] for s in SHAPES} == set(WS)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _score(a, b):
    """one pair (H, W, CH) uint8 numpy -> (sse int, psnr float, ssim float) from the device"""
    sse, _ = GM.image_sums(_dev(a)[None], _dev(b)[None])
    psnr, ssim = GM.image_metrics(_dev(a)[None], _dev(b)[None])
    return int(sse.item()), psnr.item(), ssim.item()


def _check(a, b):
    ref = MR.metrics(a, b)
    sse, psnr, ssim = _score(a, b)
    print(f"{a.shape}: sse {sse} / {ref['sse']}  psnr {psnr!r} / {ref['psnr']!r}  ssim {ssim!r} / {ref['ssim']!r}")
    assert sse == ref["sse"]
    assert np.isclose(ssim, ref["ssim"], rtol=1e-5, atol=1e-6), (ssim, ref["ssim"])
    if np.isinf(ref["psnr"]):
        assert psnr == ref["psnr"]
    else:
        assert np.isclose(psnr, ref["psnr"], rtol=1e-5, atol=0.0), (psnr, ref["psnr"])
    return sse, psnr, ssim


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matches_the_restatement(shape, ch):
    a, b = MR.gradient_noise_pair(shape[0], shape[1], ch, seed=1000 * shape[0] + shape[1] + ch)
    _check(a, b)


@pytest.mark.parametrize("ch", [1, 3])
def test_identical_images(ch):
    a, _ = MR.gradient_noise_pair(T_H + 5, T_W + 7, ch, seed=7)
    sse, psnr, ssim = _check(a, a.copy())
    assert sse == 0 and psnr == float("inf") and abs(ssim - 1.0) <= 1e-5 + 1e-6


@pytest.mark.parametrize("ch", [1, 3])
def test_black_against_white(ch):
    H, W = T_H + 5, T_W + 7
    sse, psnr, _ = _check(np.zeros((H, W, ch), np.uint8), np.full((H, W, ch), 255, np.uint8))
    assert sse == 65025 * H * W * ch and psnr == 0.0


@pytest.mark.parametrize("ch", [1, 3])
def test_two_different_constants(ch):
    """flat images: every variance is 0, and what an implementation returns for E[x^2] - mu^2 stands against C2 = 9e-4 at
    every pixel with one sign.  fp32 moments miss this bound (1.25e-5 apart on this pair, bound 4.1e-6; the reference's own
    fp32 `ssim` 2.2e-5); the kernel's fp64 moments meet it.  DESIGN.md section 12."""
    H, W = T_H + 5, T_W + 7
    _check(np.full((H, W, ch), 40, np.uint8), np.full((H, W, ch), 200, np.uint8))


CORNERS = {"top_left": (0, 0), "top_right": (0, -1), "bottom_left": (-1, 0), "bottom_right": (-1, -1),
           "tile_corner_last": (T_H - 1, T_W - 1), "tile_corner_first": (T_H, T_W)}


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("where", sorted(CORNERS))
def test_one_pixel_difference(where, ch):
    """one pixel differs: the halo and the padding decide what its 11x11 neighbourhood scores"""
    H, W = 2 * T_H + 3, 2 * T_W + 3
    a, _ = MR.gradient_noise_pair(H, W, ch, seed=11)
    b = a.copy()
    y, x = CORNERS[where]
    b[y, x] = a[y, x] ^ 0x80
    sse, _, ssim = _check(a, b)
    assert sse == 128 * 128 * ch and ssim < 1.0 - 1e-5


def test_batch_equals_single_calls_and_repeats_bitwise():
    H, W = T_H + 3, T_W + 9
    pairs = [MR.gradient_noise_pair(H, W, 3, seed=s) for s in (1, 2, 3)]
    a, b = _dev(np.stack([p[0] for p in pairs])), _dev(np.stack([p[1] for p in pairs]))
    sse, ssum = GM.image_sums(a, b)
    sse2, ssum2 = GM.image_sums(a, b)
    assert torch.equal(sse, sse2) and torch.equal(ssum, ssum2)
    for n in range(3):
        e, s = GM.image_sums(a[n:n + 1].clone(), b[n:n + 1].clone())
        assert torch.equal(e, sse[n:n + 1]) and torch.equal(s, ssum[n:n + 1])
        assert int(e.item()) == MR.squared_error(*pairs[n])
    assert len({float(v) for v in ssum.cpu()}) == 3  # three different images


def test_odd_byte_offset():
    """(N, 5, 5, 3): 75 bytes per image, so image 1 starts at an odd address and no row is dword-aligned"""
    rng = np.random.default_rng(5)
    a, b = _dev(rng.integers(0, 256, (3, 5, 5, 3), dtype=np.uint8)), _dev(rng.integers(0, 256, (3, 5, 5, 3), dtype=np.uint8))
    va, vb = a[1:], b[1:]
    assert va.is_contiguous() and va.data_ptr() % 2 == 1
    e, s = GM.image_sums(va, vb)
    e2, s2 = GM.image_sums(va.clone(), vb.clone())
    assert torch.equal(e, e2) and torch.equal(s, s2)
    for n in range(2):
        ref = MR.metrics(va[n].cpu().numpy(), vb[n].cpu().numpy())
        assert int(e[n].item()) == ref["sse"] and np.isclose(s[n].item() / 75, ref["ssim"], rtol=1e-5, atol=1e-6)


def test_full_size_against_torch_fp32():
    """one DTU-sized pair against the reference's formulation on the device: conv2d, groups = 3, padding 5, fp32"""
    import torch.nn.functional as F
    H, W = 1200, 1600
    an, bn = MR.gradient_noise_pair(H, W, 3, seed=49)
    a, b = _dev(an), _dev(bn)
    g = torch.from_numpy(MR.window_1d()).cuda()
    win = (g[:, None] * g[None, :]).float().expand(3, 1, 11, 11).contiguous()
    x, y = (t.permute(2, 0, 1)[None].float().div(255) for t in (a, b))
    mu1, mu2 = F.conv2d(x, win, padding=5, groups=3), F.conv2d(y, win, padding=5, groups=3)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(x * x, win, padding=5, groups=3) - mu1_sq
    s2 = F.conv2d(y * y, win, padding=5, groups=3) - mu2_sq
    s12 = F.conv2d(x * y, win, padding=5, groups=3) - mu1_mu2
    ref_map = ((2 * mu1_mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    ref_ssim = ref_map.double().mean().item()  # the mean in float64: an fp32 mean of 5.76 M values adds its own error
    ref_sse = int(((a.long() - b.long()) ** 2).sum().item())
    ref_psnr = (20 * torch.log10(1.0 / torch.sqrt(((x - y) ** 2).double().mean()))).item()
    sse, _ = GM.image_sums(a[None], b[None])
    psnr, ssim = GM.image_metrics(a[None], b[None])
    print(f"sse {int(sse.item())} / {ref_sse}  psnr {psnr.item()!r} / {ref_psnr!r}  ssim {ssim.item()!r} / {ref_ssim!r}")
    assert int(sse.item()) == ref_sse
    assert np.isclose(ssim.item(), ref_ssim, rtol=1e-5, atol=1e-6)
    assert np.isclose(psnr.item(), ref_psnr, rtol=1e-5, atol=0.0)


def _truth_and_views(n_true, n_views, W, H):
    import gs2m_synth as S
    from gaussian_renderer import render
    from gs2m_scene import Camera, GaussianParams, PipelineParams, inverse_sigmoid
    sc = S.make_surface_scene(n_true, seed=0)
    t = {k: v.cuda() for k, v in sc.items()}
    truth = GaussianParams(t["points"], t["shs"][:, :1].contiguous(), t["shs"][:, 1:].contiguous(), torch.log(t["scales"]),
                           t["rotations"], inverse_sigmoid(t["opacities"]),
                           *(inverse_sigmoid(torch.full((n_true, c), 0.5, device="cuda")) for c in (3, 1, 1)))
    views = [Camera(c, "cuda") for c in S.orbit_cameras(n_views, W, H, radius=6.0, centre=(0.0, -0.8, 6.0), fx=1.1 * W)]
    gen = torch.Generator().manual_seed(3)
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        for v in views:  # a "photograph": the truth's own rendering, tinted and with sensor noise
            out = render(v, truth, PipelineParams(), bg, material_stage=True)
            v.gt_image = (out["render"] * 0.9 + 0.04 + 0.03 * torch.randn(3, H, W, generator=gen).cuda()).clamp(0, 1)
            v.alpha_mask = (out["alpha_map"].reshape(1, H, W) > 0.5).float()
    return truth, views


def test_score_views_then_evaluate_the_written_files(tmp_path):
    from PIL import Image
    W, H = 100, 70
    truth, views = _truth_and_views(6000, 3, W, H)
    method_dir = tmp_path / "model" / "test" / "ours_7"
    got = GM.score_views(truth, views, torch.zeros(3, device="cuda"), out_dir=str(method_dir))
    assert got["names"] == ["00000", "00001", "00002"]
    assert sorted(os.listdir(method_dir)) == ["gt", "render"] and sorted(os.listdir(method_dir / "render")) == ["00000.png", "00001.png", "00002.png"]
    assert torch.isfinite(got["psnr"]).all() and ((got["ssim"] > 0.3) & (got["ssim"] < 1.0)).all()
    # the files are the device images: PNG is lossless, so scoring them gives the same bits
    psnr, ssim = GM.score_files(GM.collect_pairs(str(method_dir / "render"), str(method_dir / "gt")))
    assert torch.equal(psnr, got["psnr"]) and torch.equal(ssim, got["ssim"])
    ref = MR.metrics(np.asarray(Image.open(method_dir / "render" / "00001.png")), np.asarray(Image.open(method_dir / "gt" / "00001.png")))
    assert np.isclose(ssim[1].item(), ref["ssim"], rtol=1e-5, atol=1e-6) and np.isclose(psnr[1].item(), ref["psnr"], rtol=1e-5, atol=0.0)
    (tmp_path / "model" / "metrics.json").write_text(json.dumps({"ours_3": {"ssim": 0.5, "psnr": 20.0, "lpips": 0.3}}))
    out = GM.evaluate(str(tmp_path / "model"), "test", "ours_7")
    assert out == {"ssim": got["ssim"].mean().item(), "psnr": got["psnr"].mean().item(), "n_images": 3}
    written = json.loads((tmp_path / "model" / "metrics.json").read_text())
    assert written == {"ours_3": {"ssim": 0.5, "psnr": 20.0, "lpips": 0.3}, "ours_7": {"ssim": out["ssim"], "psnr": out["psnr"]}}
    # white_background: the ground truth is the background wherever the view's alpha mask is <= 0.5 (render.py:78-79)
    white = torch.tensor([1.0, 1.0, 1.0], device="cuda")
    GM.score_views(truth, views[:1], white, out_dir=str(tmp_path / "white"), white_background=True)
    gt = np.asarray(Image.open(tmp_path / "white" / "gt" / "00000.png"))
    outside = (views[0].alpha_mask[0] <= 0.5).cpu().numpy()
    assert outside.any() and (~outside).any() and (gt[outside] == 255).all()


def test_score_files_mixed_shapes_modes_and_batches(tmp_path):
    """RGBA keeps its first three channels, L stays one channel; shapes are grouped; a batch limit below one pair still scores"""
    from PIL import Image
    r, g = tmp_path / "render", tmp_path / "gt"
    r.mkdir(); g.mkdir()
    want = {}
    for k, (H, W, mode) in enumerate([(9, 14, "RGB"), (20, 7, "L"), (9, 14, "RGBA"), (20, 7, "L"), (9, 14, "RGB")]):
        ch = 1 if mode == "L" else 3
        a, b = MR.gradient_noise_pair(H, W, ch, seed=20 + k)
        for d, img in ((r, a), (g, b)):
            if mode == "L":
                img = img[:, :, 0]
            elif mode == "RGBA":
                img = np.concatenate([img, np.full((H, W, 1), 77 + k, np.uint8)], axis=2)
            Image.fromarray(img, mode).save(d / f"{k:02d}.png")
        want[f"{k:02d}.png"] = MR.metrics(a, b)
    pairs = GM.collect_pairs(str(r), str(g))
    psnr, ssim = GM.score_files(pairs)
    psnr1, ssim1 = GM.score_files(pairs, batch_bytes=1)
    assert torch.equal(psnr, psnr1) and torch.equal(ssim, ssim1)
    for k, (name, _, _) in enumerate(pairs):
        assert np.isclose(ssim[k].item(), want[name]["ssim"], rtol=1e-5, atol=1e-6)
        assert np.isclose(psnr[k].item(), want[name]["psnr"], rtol=1e-5, atol=0.0)


def test_invalid_arguments_write_nothing():
    import gs2m_native as N
    L = N.lib()
    INVALID = -1  # GS2M_ERR_INVALID_ARG
    a = torch.zeros(2 * 40 * 70 * 3, dtype=torch.uint8, device="cuda")
    sse = torch.full((2,), -12345, dtype=torch.int64, device="cuda")
    ssum = torch.full((2,), -7.5, dtype=torch.float64, device="cuda")
    nbytes = C.c_longlong(-1)
    assert L.gs2m_image_metrics_workspace_bytes(2, 40, 70, 3, C.byref(nbytes)) == 0 and nbytes.value > 0
    ws = torch.full((nbytes.value // 8,), -1, dtype=torch.int64, device="cuda")
    stream = N.stream_ptr(a.device)

    def call(n, h, w, ch, ws_bytes):
        return L.gs2m_image_metrics(n, h, w, ch, a.data_ptr(), a.data_ptr(), ws.data_ptr(), ws_bytes, sse.data_ptr(), ssum.data_ptr(), stream)

    bad = C.c_longlong(-1)
    for n, h, w, ch in ((2, 40, 70, 2), (2, 0, 70, 3), (0, 40, 70, 3), (2, 40, -1, 3), (2, 40, 70, 4), (1, 1 << 20, 1 << 20, 3),
                        (1, 1, (1 << 30) + 1, 1)):
        assert L.gs2m_image_metrics_workspace_bytes(n, h, w, ch, C.byref(bad)) == INVALID and bad.value == -1
        assert call(n, h, w, ch, nbytes.value) == INVALID
    assert call(2, 40, 70, 3, nbytes.value - 1) == INVALID  # a workspace one byte short
    assert L.gs2m_image_metrics(2, 40, 70, 3, None, a.data_ptr(), ws.data_ptr(), nbytes.value, sse.data_ptr(), ssum.data_ptr(), stream) == INVALID
    torch.cuda.synchronize()
    assert (sse == -12345).all() and (ssum == -7.5).all() and (ws == -1).all()
    assert call(2, 40, 70, 3, nbytes.value) == 0  # and the same buffers are fine for the call that is valid
    torch.cuda.synchronize()
    assert (sse == 0).all() and torch.allclose(ssum / (40 * 70 * 3), torch.ones(2, dtype=torch.float64, device="cuda"), rtol=1e-5, atol=1e-6)
