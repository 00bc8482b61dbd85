"""LPIPS at the size the reference scores: one 1600x1200 pair and 49 pairs through gs2m_lpips (csrc/lpips.hip),
per-layer convolution times, and beside them the same computation as the reference formulates it -- torch.nn.functional.conv2d /
max_pool2d in fp32 on the same GPU.  Seeded random weights and images: the time does not depend on their values.

    python tools/lpips_bench.py [--out profiles/lpips_bench.json] [--pairs 49] [--height 1200 --width 1600] [--skip-torch]

Times are device events around work on one stream, after a warm-up of every shape; FLOP are counted from the shapes
(2 x 9 Cin Cout per output pixel, both images) and set against the 157.3 TFLOP/s fp32 matrix peak.  There is no threshold."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-2m_amd"))

import gs2m_lpips as GL  # noqa: E402

PEAK_TFLOPS = 157.3
POOL_AFTER = (1, 3, 6, 9)
TAP_AFTER = (1, 3, 6, 9, 12)


def seeded_weights(device, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    conv_w = [torch.randn((co, ci, 3, 3), generator=g) * (2.0 / (9 * ci)) ** 0.5 for ci, co in zip(GL.CONV_CIN, GL.CONV_COUT)]
    conv_b = [torch.randn(co, generator=g) * 0.05 for co in GL.CONV_COUT]
    lin = [(torch.randn(c, generator=g) * 0.5 / c ** 0.5).abs() for c in GL.TAP_CHANNELS]
    return [t.to(device) for t in conv_w], [t.to(device) for t in conv_b], [t.to(device) for t in lin]


def seeded_pairs(n, h, w, device, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    b = (a.float() * 0.93 + 6.0 + 9.0 * torch.randn(a.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    return a.to(device), b.to(device)


def layer_shapes(h, w):
    """[(cin, cout, h, w)] of the thirteen convolutions"""
    out = []
    for l, (ci, co) in enumerate(zip(GL.CONV_CIN, GL.CONV_COUT)):
        out.append((ci, co, h, w))
        if l in POOL_AFTER:
            h, w = h // 2, w // 2
    return out


def pair_flop(h, w):
    return sum(2 * 2 * 9 * ci * co * hh * ww for ci, co, hh, ww in layer_shapes(h, w))


def timed(fn, warmup, reps):
    """ms per call: device events around `reps` calls after `warmup`, the minimum and the median of the repetitions"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return {"min_ms": ms[0], "median_ms": ms[len(ms) // 2], "reps": reps}


def torch_lpips(a, b, conv_w, conv_b, lin):
    """the reference's formulation (lpipsPyTorch/modules) with framework convolutions, fp32, both images as a batch of two"""
    x = torch.cat([a, b]).permute(0, 3, 1, 2).float().div(255)
    mean = torch.tensor([-.030, -.088, -.188], device=x.device)[None, :, None, None]
    std = torch.tensor([.458, .448, .450], device=x.device)[None, :, None, None]
    x = (x - mean) / std
    total, k = 0.0, 0
    for l in range(13):
        x = F.relu(F.conv2d(x, conv_w[l], conv_b[l], padding=1))
        if l in TAP_AFTER:
            f = x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10)
            d = (f[0:1] - f[1:2]) ** 2
            total = total + F.conv2d(d, lin[k].reshape(1, -1, 1, 1)).mean()
            k += 1
        if l in POOL_AFTER:
            x = F.max_pool2d(x, 2, 2)
    return total


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_bench.json"))
    ap.add_argument("--pairs", type=int, default=49)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("lpips_bench: needs a HIP device; a CPU run says nothing about the GPU")
    dev = torch.device("cuda")
    h, w = args.height, args.width
    conv_w, conv_b, lin = seeded_weights(dev)
    weights = GL.pack_weights(conv_w, conv_b, lin, dev)
    a, b = seeded_pairs(1, h, w, dev)
    flop = pair_flop(h, w)
    res = {"device": torch.cuda.get_device_name(0), "height": h, "width": w, "flop_per_pair": flop, "peak_tflops_fp32_matrix": PEAK_TFLOPS,
           "weights": "seeded random (He-scaled)", "timing": "device events, one stream, warm-up of every shape first"}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    one = timed(lambda: GL.lpips_device(a, b, weights), warmup=2, reps=7)
    one["tflops"] = flop / (one["median_ms"] * 1e-3) / 1e12
    one["share_of_peak"] = one["tflops"] / PEAK_TFLOPS
    res["hip_one_pair"] = one
    print(f"HIP, one pair: {one['median_ms']:.2f} ms, {one['tflops']:.1f} TFLOP/s ({100 * one['share_of_peak']:.1f} % of {PEAK_TFLOPS})", flush=True)
    save()

    layers = []
    for l, (ci, co, hh, ww) in enumerate(layer_shapes(h, w)):
        x = torch.randn((2, hh, ww, ci), device=dev).relu_()
        packed = GL.pack_conv(conv_w[l], conv_b[l])
        t = timed(lambda: GL.conv3x3(x, packed, co), warmup=1, reps=5)
        fl = 2 * 2 * 9 * ci * co * hh * ww
        layers.append({"conv": l, "cin": ci, "cout": co, "h": hh, "w": ww, "median_ms": t["median_ms"], "min_ms": t["min_ms"],
                       "tflops": fl / (t["median_ms"] * 1e-3) / 1e12})
        print(f"  conv {l:2d} {ci:3d}->{co:3d} {hh}x{ww}: {t['median_ms']:.3f} ms, {layers[-1]['tflops']:.1f} TFLOP/s", flush=True)
        del x, packed
    res["hip_conv_layers"] = layers
    res["hip_conv_layers_sum_ms"] = sum(x["median_ms"] for x in layers)
    save()

    if args.pairs > 1:
        an, bn = a.expand(args.pairs, h, w, 3).contiguous(), b.expand(args.pairs, h, w, 3).contiguous()
        many = timed(lambda: GL.lpips_device(an, bn, weights), warmup=1, reps=2)
        res["hip_many_pairs"] = {"pairs": args.pairs, "ms_per_pair": many["median_ms"] / args.pairs, "total_ms": many["median_ms"],
                                 "tflops": flop * args.pairs / (many["median_ms"] * 1e-3) / 1e12}
        print(f"HIP, {args.pairs} pairs: {res['hip_many_pairs']['ms_per_pair']:.2f} ms per pair, {res['hip_many_pairs']['tflops']:.1f} TFLOP/s", flush=True)
        del an, bn
        save()

    if not args.skip_torch:
        with torch.no_grad():
            ref = torch_lpips(a, b, conv_w, conv_b, lin).item()
            t = timed(lambda: torch_lpips(a, b, conv_w, conv_b, lin), warmup=2, reps=5)
        t["tflops"] = flop / (t["median_ms"] * 1e-3) / 1e12
        t["value"] = ref
        res["torch_one_pair"] = t
        res["hip_value"] = GL.lpips(a, b, weights).item()
        print(f"torch conv2d fp32, one pair: {t['median_ms']:.2f} ms, {t['tflops']:.1f} TFLOP/s; value {ref!r} against HIP {res['hip_value']!r}", flush=True)
        save()
    print(json.dumps({k: v for k, v in res.items() if k != "hip_conv_layers"}))


if __name__ == "__main__":
    main()
