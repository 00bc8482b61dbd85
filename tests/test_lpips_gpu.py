"""csrc/lpips.hip through gs2m_lpips.py against the float64 restatement tests/lpips_ref.py: every kernel alone
-- the convolution at a rigorous forward-error bound, the pool bit for bit, the tap distance -- then the whole score on the
golden cases, where the yardstick is how far the REFERENCE's own fp32 result (tests/golden/ref_lpips.npz) lies from float64.
The weights are seeded (lpips_ref.make_weights); shapes are the smallest at which the tiling can go wrong."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as LR
import metrics_ref as MR

pytestmark = pytest.mark.gpu

import gs2m_lpips as GL  # noqa: E402
import gs2m_metrics as GM  # noqa: E402

TILE = 16  # GS2M_LPIPS_TILE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_lpips.npz")
CEILING = 1e-4  # the metric is reported to three or four decimals


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ---- the convolution alone ------------------------------------------------------------------------------------------------------
CONV_SIZES = ((1, 1, 1), (1, 2, 3), (2, 5, 7), (1, 33, 70), (1, TILE + 1, TILE + 1))  # (N, H, W)


@pytest.mark.parametrize("cin,cout", [(3, 64), (64, 64), (64, 128), (256, 512), (512, 512)])
def test_conv3x3_within_the_fp32_chain_bound(cin, cout):
    """|dev - ref64| <= (K + 2) 2^-24 (sum |a||w| + |bias|), K = 9 Cin: the forward error of a K-term fp32 fmaf chain in any
    order, the bias add and the final rounding.  A wrong tap, border or channel is an O(1) error."""
    rng = np.random.default_rng(100 * cin + cout)
    w, b = LR.make_conv(cin, cout, rng)
    packed = GL.pack_conv(_dev(w), _dev(b))
    K, worst = 9 * cin, 0.0
    for n, h, wd in CONV_SIZES:
        x = torch.from_numpy(rng.normal(0.0, 1.0, (n, cin, h, wd)).astype(np.float32))
        x = x * torch.from_numpy((rng.random((n, 1, h, wd)) > 0.1).astype(np.float32))  # some all-zero pixels
        ref, mag = LR.conv_relu(x, w, b), LR.conv_magnitude(x, w, b)
        got = GL.conv3x3(_nhwc(x).cuda(), packed, cout).cpu().permute(0, 3, 1, 2).double()
        assert got.shape == ref.shape
        ratio = ((got - ref).abs() / ((K + 2) * 2.0 ** -24 * mag)).max().item()
        worst = max(worst, ratio)
        print(f"conv {cin}->{cout} {n}x{h}x{wd}: max |err| / bound {ratio:.4f}, {(ref > 0).double().mean().item():.2f} of the outputs positive")
        assert ratio <= 1.0, (n, h, wd, ratio)
    print(f"conv {cin}->{cout}: largest ratio to the bound {worst:.4f}")
    # everything negative before the ReLU: positive inputs, negative weights and biases -> exactly 0
    x = torch.from_numpy(rng.random((1, cin, 5, 7)).astype(np.float32) + 0.1)
    neg = GL.pack_conv(_dev(-np.abs(w) - 1e-3), _dev(-np.abs(b) - 1e-3))
    got = GL.conv3x3(_nhwc(x).cuda(), neg, cout)
    assert got.shape == (1, 5, 7, cout) and (got == 0).all() and not torch.signbit(got).any()


def test_conv3x3_refuses_what_it_cannot_tile():
    import gs2m_native as N
    L = N.lib()
    x = torch.zeros(4096, device="cuda")
    s = N.stream_ptr(x.device)
    p = x.data_ptr()
    assert L.gs2m_lpips_conv3x3(1, 2, 2, 8, 64, p, p, p, s) == -4   # GS2M_ERR_UNSUPPORTED: Cin neither 3 nor a multiple of 16
    assert L.gs2m_lpips_conv3x3(1, 2, 2, 16, 32, p, p, p, s) == -4  # Cout no multiple of 64
    assert L.gs2m_lpips_conv3x3(1, 0, 2, 16, 64, p, p, p, s) == -1
    assert L.gs2m_lpips_conv3x3(1, 2, 2, 16, 64, None, p, p, s) == -1
    assert L.gs2m_lpips_conv3x3(1, 2, 2, 16, 64, p + 4, p, p, s) == -1  # float4 loads need 16-byte alignment
    torch.cuda.synchronize()
    assert (x == 0).all()


# ---- the pool alone -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2, 2, 4), (2, 5, 7, 64), (1, 35, 29, 128), (1, 3, 2, 512), (1, 16, 17, 64)], ids=str)
def test_maxpool_is_bit_equal_to_torch(shape):
    n, h, w, c = shape
    x = torch.from_numpy(np.random.default_rng(h * w + c).normal(0.0, 1.0, (n, c, h, w)).astype(np.float32))
    ref = F.max_pool2d(x, kernel_size=2, stride=2)
    got = GL.maxpool2x2(_nhwc(x).cuda()).cpu().permute(0, 3, 1, 2)
    assert got.shape == ref.shape == (n, c, h // 2, w // 2) and torch.equal(got, ref)


# ---- the tap distance alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [64, 128, 256, 512])
def test_tap_distance_alone(c):
    """the inputs are given, a pixel's value is an fp32 chain of at most 512 terms, pixels are added in fp64: 1e-5 relative.
    17 x 19 = 323 pixels: more than one workgroup of 256, the last one partly empty.  One pixel of fx is all zero (the 1e-10
    decides: 0 / 1e-10 = 0), one pixel is zero in both."""
    rng = np.random.default_rng(c)
    n, h, w = 2, 17, 19
    fx = np.maximum(rng.normal(0.0, 1.0, (n, c, h, w)), 0).astype(np.float32)
    fy = np.maximum(fx + rng.normal(0.0, 0.3, fx.shape), 0).astype(np.float32)
    fx[0, :, 3, 4] = 0.0
    fx[1, :, 16, 18] = 0.0
    fy[1, :, 16, 18] = 0.0
    lin = np.abs(rng.normal(0.0, 0.1, c)).astype(np.float32)
    ref = LR.tap_distance(torch.from_numpy(fx), torch.from_numpy(fy), lin).numpy()
    got = GL.tap_distance(_nhwc(torch.from_numpy(fx)).cuda(), _nhwc(torch.from_numpy(fy)).cuda(), _dev(lin))
    again = GL.tap_distance(_nhwc(torch.from_numpy(fx)).cuda(), _nhwc(torch.from_numpy(fy)).cuda(), _dev(lin))
    print(f"tap C={c}: {got.numpy()!r} / {ref!r}, relative {np.abs(got.numpy() / ref - 1).max():.2e}")
    assert torch.isfinite(got).all() and (ref > 0).all() and torch.equal(got, again)
    assert np.allclose(got.numpy(), ref, rtol=1e-5, atol=0.0)
    for k in range(n):  # an image's value does not depend on its neighbours in the batch
        one = GL.tap_distance(_nhwc(torch.from_numpy(fx[k:k + 1])).cuda(), _nhwc(torch.from_numpy(fy[k:k + 1])).cuda(), _dev(lin))
        assert torch.equal(one, got[k:k + 1])


# ---- the whole score ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    w = LR.make_weights(LR.GOLDEN_SEED)
    return GL.pack_weights([torch.from_numpy(x) for x in w["conv_w"]], [torch.from_numpy(x) for x in w["conv_b"]],
                           [torch.from_numpy(x) for x in w["lin"]])


@pytest.fixture(scope="module")
def golden():
    """{name: (a, b, golden total, golden layers, fp64 total, fp64 layers)}; the float64 restatement is computed once"""
    g = np.load(GOLDEN)
    w = LR.make_weights(LR.GOLDEN_SEED)
    out = {}
    for name in LR.cases():
        a, b = g[f"{name}/a"], g[f"{name}/b"]
        layers64, total64 = LR.lpips(a, b, w)
        out[name] = (a, b, float(g[f"{name}/lpips"]), g[f"{name}/layers"].astype(np.float64), total64, layers64)
    return out


def test_packed_weights_layout(weights):
    """[tap][cin][cout] then the bias, layer after layer, then the lin vectors"""
    w = LR.make_weights(LR.GOLDEN_SEED)
    p = weights.packed.cpu().numpy()
    assert p.shape == (GL.PACKED_FLOATS,)
    off = 0
    for l in (0, 1, 12):
        off = sum(9 * ci * co + co for ci, co in zip(LR.CONV_CIN[:l], LR.CONV_COUT[:l]))
        ci, co = LR.CONV_CIN[l], LR.CONV_COUT[l]
        want = w["conv_w"][l].transpose(2, 3, 1, 0).reshape(-1)  # OIHW -> (ky, kx, cin, cout)
        assert np.array_equal(p[off:off + 9 * ci * co], want) and np.array_equal(p[off + 9 * ci * co:off + 9 * ci * co + co], w["conv_b"][l])
    assert np.array_equal(p[-512:], w["lin"][4]) and np.array_equal(p[-1472:-1408], w["lin"][0])


def test_golden_cases_within_the_reference_own_fp32_error(weights, golden):
    """Device and reference are fp32 accumulations of the same products in different orders through 13 layers.  The yardstick
    is the largest deviation of the reference's recorded fp32 result from the float64 restatement over the cases; the device may
    deviate from float64 by at most 4x that (the factor covers the tail), and never by more than 1e-4."""
    yard_total = max(abs(gt - t64) for _, _, gt, _, t64, _ in golden.values())
    yard_layer = max(np.abs(gl - l64).max() for _, _, _, gl, _, l64 in golden.values())
    assert 0.0 < yard_total < CEILING / 4 and 0.0 < yard_layer < CEILING / 4
    worst_total = worst_layer = 0.0
    for name, (a, b, gt, gl, t64, l64) in golden.items():
        da, db = _dev(a)[None], _dev(b)[None]
        total, layers = GL.lpips(da, db, weights), GL.lpips_layers(da, db, weights)
        assert total.shape == (1,) and layers.shape == (1, 5) and total.dtype == layers.dtype == torch.float64
        dt, dl = abs(total.item() - t64), np.abs(layers[0].numpy() - l64).max()
        worst_total, worst_layer = max(worst_total, dt), max(worst_layer, dl)
        print(f"{name}: device {total.item()!r} golden {gt!r} fp64 {t64!r}; |device - fp64| {dt:.3e} (layers {dl:.3e}), "
              f"|golden - fp64| {abs(gt - t64):.3e} (layers {np.abs(gl - l64).max():.3e})")
        assert total.item() == sum(layers[0].tolist())  # the taps added in order
        assert dt <= 4 * yard_total and dl <= 4 * yard_layer and dt <= CEILING, name
        again = GL.lpips(da, db, weights)
        assert torch.equal(total, again), name  # bitwise run to run
        if name.startswith("identical"):
            assert total.item() == 0.0 and (layers == 0).all()
    print(f"yardstick: total {yard_total:.3e}, layer {yard_layer:.3e}; device worst: total {worst_total:.3e}, layer {worst_layer:.3e}")


def test_batch_equals_single_calls_bitwise(weights):
    pairs = [MR.gradient_noise_pair(35, 29, 3, seed=s) for s in (31, 32, 33)]
    a, b = _dev(np.stack([p[0] for p in pairs])), _dev(np.stack([p[1] for p in pairs]))
    total, layers = GL.lpips_device(a, b, weights)
    for n in range(3):
        t, l = GL.lpips_device(a[n:n + 1].clone(), b[n:n + 1].clone(), weights)
        assert torch.equal(t, total[n:n + 1]) and torch.equal(l, layers[n:n + 1])
    assert len({float(v) for v in total.cpu()}) == 3 and (total > 0).all()
    assert GL.lpips(a[:0], b[:0], weights).shape == (0,)


def test_invalid_arguments_write_nothing(weights):
    import gs2m_native as N
    L = N.lib()
    INVALID = -1
    a = torch.zeros(20 * 24 * 3, dtype=torch.uint8, device="cuda")
    total = torch.full((1,), -7.5, dtype=torch.float64, device="cuda")
    layers = torch.full((5,), -7.5, dtype=torch.float64, device="cuda")
    nbytes, bad = C.c_longlong(-1), C.c_longlong(-1)
    assert L.gs2m_lpips_workspace_bytes(1, 20, 24, C.byref(nbytes)) == 0 and nbytes.value >= 2 * 2 * 20 * 24 * 64 * 4
    ws = torch.full((nbytes.value // 4,), -1.0, dtype=torch.float32, device="cuda")
    stream = N.stream_ptr(a.device)

    def call(n, h, w, ws_bytes, pa=a.data_ptr()):
        return L.gs2m_lpips(n, h, w, pa, a.data_ptr(), weights.packed.data_ptr(), ws.data_ptr(), ws_bytes, total.data_ptr(),
                            layers.data_ptr(), stream)

    for n, h, w in ((1, 15, 24), (1, 20, 15), (0, 20, 24), (1, -1, 24), (1, 1 << 20, 1 << 20), (1, 32769, 16)):
        assert L.gs2m_lpips_workspace_bytes(n, h, w, C.byref(bad)) == INVALID and bad.value == -1
        assert call(n, h, w, nbytes.value) == INVALID
    assert call(1, 20, 24, nbytes.value - 1) == INVALID  # a workspace one byte short
    assert call(1, 20, 24, nbytes.value, pa=None) == INVALID
    torch.cuda.synchronize()
    assert (total == -7.5).all() and (layers == -7.5).all() and (ws == -1.0).all()
    assert call(1, 20, 24, nbytes.value) == 0  # and the same buffers are fine for the call that is valid
    torch.cuda.synchronize()
    assert total.item() == 0.0 and (layers == 0).all()


# ---- the metrics command ------------------------------------------------------------------------------------------------------------
def test_evaluate_writes_lpips_only_with_weights(tmp_path, weights, capsys):
    from PIL import Image
    method_dir = tmp_path / "model" / "test" / "ours_7"
    (method_dir / "render").mkdir(parents=True)
    (method_dir / "gt").mkdir()
    pairs = [MR.gradient_noise_pair(35, 29, 3, seed=s) for s in (41, 42, 43)]
    for k, (a, b) in enumerate(pairs):
        Image.fromarray(a, "RGB").save(method_dir / "render" / f"{k:05d}.png")
        Image.fromarray(b, "RGB").save(method_dir / "gt" / f"{k:05d}.png")
    metric_file = tmp_path / "model" / "metrics.json"
    other = {"ours_3": {"ssim": 0.5, "psnr": 20.0, "lpips": 0.3}}
    metric_file.write_text(json.dumps(other))
    plain = GM.evaluate(str(tmp_path / "model"), "test", "ours_7")
    assert sorted(plain) == ["n_images", "psnr", "ssim"] and "LPIPS" not in capsys.readouterr().out
    assert json.loads(metric_file.read_text()) == {**other, "ours_7": {"ssim": plain["ssim"], "psnr": plain["psnr"]}}
    per_image = GL.lpips(_dev(np.stack([p[0] for p in pairs])), _dev(np.stack([p[1] for p in pairs])), weights)
    out = GM.evaluate(str(tmp_path / "model"), "test", "ours_7", lpips_weights=weights)
    assert out == {**plain, "lpips": per_image.mean().item()} and out["lpips"] > 0
    assert "[-] LPIPS: {:>12.7f}".format(out["lpips"]) in capsys.readouterr().out
    assert json.loads(metric_file.read_text()) == {**other, "ours_7": {"ssim": out["ssim"], "psnr": out["psnr"], "lpips": out["lpips"]}}
    ref = np.mean([LR.lpips(a, b, LR.make_weights(LR.GOLDEN_SEED))[1] for a, b in pairs])
    assert abs(out["lpips"] - ref) <= CEILING
    # a grey pair cannot be scored with LPIPS: the error names the file
    Image.fromarray(pairs[0][0][:, :, 0], "L").save(method_dir / "render" / "00009.png")
    Image.fromarray(pairs[0][1][:, :, 0], "L").save(method_dir / "gt" / "00009.png")
    with pytest.raises(ValueError, match="00009.png is a grey image"):
        GM.evaluate(str(tmp_path / "model"), "test", "ours_7", lpips_weights=weights)
    assert GM.evaluate(str(tmp_path / "model"), "test", "ours_7")["n_images"] == 4  # without weights it is scored as before


def test_score_views_with_weights(weights):
    """the smallest synthetic scene of tests/test_metrics_gpu.py: "lpips" is `lpips` of the quantised render and ground truth"""
    import gs2m_synth as S
    from gaussian_renderer import render
    from gs2m_scene import Camera, GaussianParams, PipelineParams, inverse_sigmoid
    n_true, W, H = 6000, 100, 70
    sc = S.make_surface_scene(n_true, seed=0)
    t = {k: v.cuda() for k, v in sc.items()}
    truth = GaussianParams(t["points"], t["shs"][:, :1].contiguous(), t["shs"][:, 1:].contiguous(), torch.log(t["scales"]),
                           t["rotations"], inverse_sigmoid(t["opacities"]),
                           *(inverse_sigmoid(torch.full((n_true, c), 0.5, device="cuda")) for c in (3, 1, 1)))
    views = [Camera(c, "cuda") for c in S.orbit_cameras(2, W, H, radius=6.0, centre=(0.0, -0.8, 6.0), fx=1.1 * W)]
    gen = torch.Generator().manual_seed(3)
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        for v in views:
            out = render(v, truth, PipelineParams(), bg, material_stage=True)
            v.gt_image = (out["render"] * 0.9 + 0.04 + 0.03 * torch.randn(3, H, W, generator=gen).cuda()).clamp(0, 1)
        got = GM.score_views(truth, views, bg, lpips_weights=weights)
        plain = GM.score_views(truth, views, bg)
        assert sorted(plain) == ["names", "psnr", "ssim"] and sorted(got) == ["lpips", "names", "psnr", "ssim"]
        assert torch.equal(got["psnr"], plain["psnr"]) and torch.equal(got["ssim"], plain["ssim"])
        assert got["lpips"].shape == (2,) and got["lpips"].dtype == torch.float64 and (got["lpips"] > 0).all()
        for k, v in enumerate(views):
            img = GM.quantise(render(v, truth, PipelineParams(), bg, material_stage=True)["render"])
            gt = GM.quantise(v.gt_image[0:3].clamp(0.0, 1.0))
            assert torch.equal(GL.lpips(img[None], gt[None], weights), got["lpips"][k:k + 1])
