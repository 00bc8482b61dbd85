"""Scoring a DTU-sized test set, 49 pairs of 1600 x 1200 x 3 8-bit images that start in (pinned) host memory: gs2m_metrics
(csrc/image_metrics.hip) against the reference's formulation on the same device -- metrics.py's loop: per pair to_tensor's
float conversion, utils/loss_utils.py's conv2d `ssim` and utils/image_utils.py's `psnr` in fp32 torch.  Upload and conversion
are inside both timed windows; decoding PNGs is in neither.  Prints ms per pair for both routes, the new kernels alone on a
device-resident batch, and the traffic floor (2 x 5.76 MB per pair); DESIGN.md §12 "Measured" quotes the output.

    python tools/metrics_bench.py [--pairs 49] [--repeats 5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-2m_amd")):
    sys.path.insert(0, p)
import torch
import torch.nn.functional as F

import gs2m_metrics as GM

H, W, CH = 1200, 1600, 3


def make_set(n, seed=0):
    """(n, H, W, 3) uint8 x 2 in pinned host memory: smooth content plus noise, the second a distorted copy of the first"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.empty((n, H, W, CH), dtype=torch.uint8).pin_memory()
    b = torch.empty((n, H, W, CH), dtype=torch.uint8).pin_memory()
    y, x = torch.meshgrid(torch.linspace(0, 1, H, device="cuda"), torch.linspace(0, 1, W, device="cuda"), indexing="ij")
    for k in range(n):
        base = 60 + 120 * torch.stack([x * (0.5 + 0.5 * y), y * (1 - 0.3 * x), 0.5 * (x + y)], dim=2) + 3.0 * (k % 7)
        ia = (base + 18 * torch.randn(H, W, CH, device="cuda", generator=gen)).clamp(0, 255)
        ib = (ia * 0.93 + 6 + 9 * torch.randn(H, W, CH, device="cuda", generator=gen)).clamp(0, 255)
        a[k], b[k] = ia.to(torch.uint8).cpu(), ib.to(torch.uint8).cpu()
    return a, b


def route_hip(a, b):
    """as gs2m_metrics.score_files: batches of at most BATCH_BYTES, one upload and one launch each"""
    per = max(1, GM.BATCH_BYTES // (2 * H * W * CH))
    psnr, ssim = [], []
    for s in range(0, len(a), per):
        da, db = a[s:s + per].cuda(non_blocking=True), b[s:s + per].cuda(non_blocking=True)
        p, q = GM.image_metrics(da, db)
        psnr.append(p); ssim.append(q)
    return torch.cat(psnr), torch.cat(ssim)


def _window():
    from math import exp
    g = torch.Tensor([exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().unsqueeze(0).unsqueeze(0).expand(CH, 1, 11, 11).contiguous().cuda()


def route_torch(a, b, win):
    """metrics.py:26-56 per pair: upload, (1, 3, H, W) float / 255, ssim and psnr as the reference writes them"""
    psnr, ssim = [], []
    for k in range(len(a)):
        x = a[k].cuda(non_blocking=True).permute(2, 0, 1).contiguous().unsqueeze(0).float().div(255)
        y = b[k].cuda(non_blocking=True).permute(2, 0, 1).contiguous().unsqueeze(0).float().div(255)
        mu1, mu2 = F.conv2d(x, win, padding=5, groups=CH), F.conv2d(y, win, padding=5, groups=CH)
        mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        s1 = F.conv2d(x * x, win, padding=5, groups=CH) - mu1_sq
        s2 = F.conv2d(y * y, win, padding=5, groups=CH) - mu2_sq
        s12 = F.conv2d(x * y, win, padding=5, groups=CH) - mu1_mu2
        m = ((2 * mu1_mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
        ssim.append(m.mean())
        mse = ((x - y) ** 2).view(1, -1).mean(1, keepdim=True)
        psnr.append(20 * torch.log10(1.0 / torch.sqrt(mse)))
    return torch.stack([p.reshape(()) for p in psnr]).cpu().double(), torch.stack(ssim).cpu().double()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=49)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "metrics_bench needs a HIP device"
    n = args.pairs
    a, b = make_set(n)
    win = _window()
    routes = {"hip": lambda: route_hip(a, b), "torch": lambda: route_torch(a, b, win)}
    for fn in routes.values():  # warm-up: code objects, MIOpen's choice of convolution, the allocator's blocks
        fn(); fn()
    ms = {k: [] for k in routes}
    for _ in range(args.repeats):  # alternating, so that what else the host does falls on both
        for k, fn in routes.items():
            t, out = timed(fn)
            ms[k].append(t / n)
            if k == "hip":
                hip_out = out
            else:
                torch_out = out
    # the kernels alone, on a batch that already is on the device
    per = min(n, max(1, GM.BATCH_BYTES // (2 * H * W * CH)))
    da, db = a[:per].cuda(), b[:per].cuda()
    GM.image_sums(da, db)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        GM.image_sums(da, db)
    e1.record()
    torch.cuda.synchronize()
    kernel_ms = e0.elapsed_time(e1) / 10 / per
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    floor_bytes = 2 * H * W * CH
    print(json.dumps({
        "pairs": n, "shape": [H, W, CH], "repeats": args.repeats,
        "hip_ms_per_pair": round(med["hip"], 4), "hip_ms_per_pair_all": [round(v, 4) for v in ms["hip"]],
        "torch_ms_per_pair": round(med["torch"], 4), "torch_ms_per_pair_all": [round(v, 4) for v in ms["torch"]],
        "torch_over_hip": round(med["torch"] / med["hip"], 2),
        "hip_kernels_only_ms_per_pair": round(kernel_ms, 4),
        "hip_kernels_only_GBps": round(floor_bytes / kernel_ms / 1e6, 1),
        "traffic_floor_MB_per_pair": round(floor_bytes / 1e6, 2),
        "max_abs_ssim_difference": float((hip_out[1] - torch_out[1]).abs().max()),
        "max_abs_psnr_difference": float((hip_out[0] - torch_out[0]).abs().max()),
    }))


if __name__ == "__main__":
    main()
