"""Float64 numpy restatement of the two image metrics of metrics.py on 8-bit input, written from the formulas
(utils/image_utils.py:22-24 `psnr`, utils/loss_utils.py:30-70 `ssim`); the checker of csrc/image_metrics.hip.

Images are uint8 (H, W, CH) as PIL decodes them.  The window is the reference's: the eleven fp32 weights
exp(-(x - 5)^2 / (2 1.5^2)) / sum and their fp32 outer product (`_1D_window.mm(_1D_window.t()).float()`), applied per channel with
zero "same" padding -- here as 121 shifted adds in float64 on value / 255."""
from math import exp

import numpy as np

C1, C2 = 0.01 ** 2, 0.03 ** 2


def window_1d():
    """torch.Tensor([exp(-(x - 5)^2 / (2 * 1.5^2)) ...]) / sum: the exponentials rounded to fp32, summed and divided in fp32"""
    g = np.array([exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=np.float32)
    s = np.float32(g.astype(np.float64).sum())  # the correctly rounded sum, 3.7592328: what torch's fp32 sum of these eleven gives
    return (g / s).astype(np.float32)          # (a sequential fp32 sum gives 3.7592325); tests/test_metrics.py pins the quotients to torch's


def window_2d():
    g = window_1d()
    return (g[:, None] * g[None, :]).astype(np.float32).astype(np.float64)  # the fp32 products, as the reference forms them


def _conv(x, w2):
    """per-channel 11x11 correlation of (H, W, CH) float64 with zero "same" padding"""
    H, W, _ = x.shape
    p = np.pad(x, ((5, 5), (5, 5), (0, 0)))
    out = np.zeros_like(x)
    for i in range(11):
        for j in range(11):
            out += w2[i, j] * p[i:i + H, j:j + W]
    return out


def ssim_map(a, b):
    """uint8 (H, W, CH) x 2 -> the SSIM map, float64 (H, W, CH)"""
    a = np.asarray(a, dtype=np.float64) / 255.0
    b = np.asarray(b, dtype=np.float64) / 255.0
    w2 = window_2d()
    mu1, mu2 = _conv(a, w2), _conv(b, w2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    sigma1_sq = _conv(a * a, w2) - mu1_sq
    sigma2_sq = _conv(b * b, w2) - mu2_sq
    sigma12 = _conv(a * b, w2) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


def squared_error(a, b):
    """the exact sum of (a - b)^2 over all elements, a Python int"""
    d = np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64)
    return int((d * d).sum())


def psnr_of(sse, count):
    """20 log10(1 / sqrt(mse)), mse = sse / (255^2 count); +inf when sse is 0 (1 / 0 in the reference's tensor arithmetic)"""
    if sse == 0:
        return float("inf")
    return float(20.0 * np.log10(1.0 / np.sqrt(sse / (255.0 * 255.0 * count))))


def metrics(a, b):
    """uint8 (H, W, CH) x 2 -> {"sse": exact int, "psnr": float, "ssim": float (the map's mean)}"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.ndim == 3
    sse = squared_error(a, b)
    return {"sse": sse, "psnr": psnr_of(sse, a.size), "ssim": float(ssim_map(a, b).mean())}


def gradient_noise_pair(H, W, CH, seed):
    """seeded test content: a smooth gradient plus noise (variances neither 0 nor saturated); b = a distorted"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = 60.0 + 120.0 * (x / max(W - 1, 1)) * (0.5 + 0.5 * y / max(H - 1, 1))
    base = base[:, :, None] + 25.0 * np.arange(CH)[None, None, :]
    a = np.clip(base + rng.normal(0.0, 18.0, (H, W, CH)), 0, 255).astype(np.uint8)
    b = np.clip(a.astype(np.float64) * 0.93 + 6.0 + rng.normal(0.0, 9.0, (H, W, CH)), 0, 255).astype(np.uint8)
    return a, b
