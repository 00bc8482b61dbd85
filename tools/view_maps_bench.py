"""Times the per-view map conversion of gs2m_render.py (csrc/view_maps.hip) against the reference's host
formulation of the same maps, per view at 1600 x 1200, and the PNG encoding on its own.

    python tools/view_maps_bench.py [--width 1600] [--height 1200] [--repeats 20] [--json OUT.json]

Three figures per set of maps, each the median over `--repeats` views after a warm-up, alternating the two formulations:
  device   gs2m_render: order_stats + depth_colorize + pack_image per map, until the 8-bit arrays are on the HOST (one
           copy per image); `device_kernels_ms` is the same work measured by device events without the copies
  host     what render.py does: the depth map copied to the host, np.percentile twice, np.clip, the normalisation,
           matplotlib's magma and the cast (utils/image_utils.py:79-86, without imsave); the other maps by the torch
           expressions of render.py and utils/image_utils.py on the device they live on, ending in the same host arrays
  png      PIL's encoder on the arrays (what both pipelines then pay), reported separately
The maps are synthetic (a smooth depth with a masked half, random normals and colours): the conversion does not depend on the
content except through ties in the depth.  The two formulations' arrays are compared before anything is timed."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-2m_amd"))

import gs2m_render as GR  # noqa: E402


def make_maps(h, w, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    depth = 3.0 + 1.5 * x / w + 0.8 * y / h + 0.05 * torch.randn(h, w, generator=g)
    alpha = ((x - w / 2) ** 2 / (0.45 * w) ** 2 + (y - h / 2) ** 2 / (0.45 * h) ** 2 < 1.0).float()[None]
    depth = depth * alpha[0]  # masked depth: the background is a run of zeros
    m = {"depth": depth, "alpha": alpha, "normal": torch.randn(3, h, w, generator=g), "gt": torch.rand(3, h, w, generator=g) * 1.1,
         "render": torch.rand(3, h, w, generator=g) * 1.1, "albedo": torch.rand(3, h, w, generator=g),
         "roughness": torch.rand(1, h, w, generator=g), "metallic": torch.rand(1, h, w, generator=g),
         "diffuse": torch.rand(h, w, 3, generator=g), "specular": torch.rand(h, w, 3, generator=g) * 0.3,
         "rot": torch.linalg.qr(torch.randn(3, 3, generator=g))[0].contiguous(), "bg": torch.ones(3)}
    return {k: v.to(device).contiguous() for k, v in m.items()}


def device_images(m, white):
    """gs2m_render's conversion of one view's maps (render.py:76-151, material branch included) -> {name: uint8 device array}"""
    q, a = ("trunc", m["alpha"]) if white else ("round", None)
    return {"gt": GR.pack_image(m["gt"], mask=m["alpha"] if white else None, background=m["bg"]),
            "normal": GR.pack_image(m["normal"], quant=q, alpha=a, normal=True, rot=m["rot"]),
            "depth": GR.depth_image(m["depth"]),
            "render": GR.pack_image(m["render"]),
            "albedo": GR.pack_image(m["albedo"], quant=q, alpha=a),
            "roughness": GR.pack_image(m["roughness"], quant=q, alpha=a),
            "metallic": GR.pack_image(m["metallic"], quant=q, alpha=a),
            "diffuse": GR.pack_image(m["diffuse"], "hwc", quant=q, alpha=a, srgb=True),
            "specular": GR.pack_image(m["specular"], "hwc", quant=q, alpha=a, srgb=True)}


def _save_image(t):  # torchvision.utils.save_image's array (make_grid: one channel becomes three)
    if t.shape[0] == 1:
        t = t.expand(3, -1, -1)
    return t.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()


def _map_to_rgba(t, alpha):
    tm, am = (t * 255).byte().cpu().numpy(), (alpha * 255).byte().cpu().numpy()
    return np.transpose(np.concatenate((tm, am) if tm.shape[0] == 3 else (tm, tm, tm, am), axis=0), (1, 2, 0))


def host_images(m, white):
    """the same images as the reference forms them -> {name: uint8 host array}"""
    import matplotlib.pyplot as plt
    from pbr import linear_to_srgb
    out = {}
    gt = torch.clamp(m["gt"], 0.0, 1.0)
    if white:
        gt = torch.where(m["alpha"] > 0.5, gt, m["bg"][:, None, None])
    out["gt"] = _save_image(gt)
    n = torch.nn.functional.normalize(m["normal"].permute(1, 2, 0).reshape(-1, 3).clone(), dim=1, p=2)
    n = (n @ m["rot"]) @ torch.tensor([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]], device=n.device).T
    n = (n * 0.5 + 0.5).reshape(m["normal"].shape[1], m["normal"].shape[2], 3).permute(2, 0, 1)
    put = (lambda t: _map_to_rgba(t, m["alpha"])) if white else _save_image
    out["normal"] = put(n)
    d = m["depth"].cpu().numpy()
    lo, hi = np.percentile(d, 1), np.percentile(d, 99)
    rgb = (plt.cm.magma((np.clip(d, lo, hi) - lo) / (hi - lo + 1e-8))[..., :3] * 255).astype(np.uint8)
    out["depth"] = np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=2)  # imsave adds the alpha
    out["render"] = _save_image(torch.clamp(m["render"], 0.0, 1.0))
    out["albedo"] = put(m["albedo"].clamp(0.0, 1.0))
    out["roughness"], out["metallic"] = put(m["roughness"]), put(m["metallic"])
    out["diffuse"] = put(linear_to_srgb(m["diffuse"]).clamp(0.0, 1.0).permute(2, 0, 1))
    out["specular"] = put(linear_to_srgb(m["specular"]).clamp(0.0, 1.0).permute(2, 0, 1))
    return out


def png_bytes(images):
    from PIL import Image
    total = 0
    for a in images.values():
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="PNG")
        total += buf.tell()
    return total


def _median(xs):
    return float(np.median(np.asarray(xs)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda")
    sets = [make_maps(a.height, a.width, dev, seed=s) for s in range(3)]
    result = {"width": a.width, "height": a.height, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "branches": {}}
    for white in (False, True):
        # the same images first: bytes equal where the arithmetic is pinned, within 1 elsewhere
        dimg = {k: v.cpu().numpy() for k, v in device_images(sets[0], white).items()}
        himg = host_images(sets[0], white)
        agree = {}
        for k in dimg:
            assert dimg[k].shape == himg[k].shape, (k, dimg[k].shape, himg[k].shape)
            diff = np.abs(dimg[k].astype(np.int16) - himg[k].astype(np.int16))
            assert diff.max() <= 1, (k, int(diff.max()))
            agree[k] = int(np.count_nonzero(diff))
        for s in sets:  # warm-up of every shape on both sides
            device_images(s, white), host_images(s, white)
        torch.cuda.synchronize()
        t_dev, t_host, t_kern, t_png = [], [], [], []
        for r in range(a.repeats):
            m = sets[r % len(sets)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            imgs = {k: v.cpu().numpy() for k, v in device_images(m, white).items()}
            t1 = time.perf_counter()
            host_images(m, white)
            t2 = time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            device_images(m, white)
            e1.record()
            e1.synchronize()
            t3 = time.perf_counter()
            png_bytes(imgs)
            t4 = time.perf_counter()
            t_dev.append((t1 - t0) * 1e3); t_host.append((t2 - t1) * 1e3); t_kern.append(e0.elapsed_time(e1)); t_png.append((t4 - t3) * 1e3)
        result["branches"]["white_background" if white else "black_background"] = {
            "images_per_view": len(dimg), "device_to_host_arrays_ms": _median(t_dev), "device_kernels_ms": _median(t_kern),
            "host_formulation_ms": _median(t_host), "png_encoding_ms": _median(t_png),
            "device_spread_ms": [float(min(t_dev)), float(max(t_dev))], "host_spread_ms": [float(min(t_host)), float(max(t_host))],
            "bytes_differing_from_host_formulation": agree}
    line = json.dumps(result)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
