"""What dataset ingestion costs on the host and on the device.

    python tools/ingest_bench.py [--views 49] [--width 1554] [--height 1162] [-r 2] [--out profiles/ingest_bench.json]

A DTU scan's worth of synthetic, already decoded images with masks, each turned into the training image, the alpha mask and
the NCC gray image (at the original size: ncc_scale = 1 / r) the way the reference does it:
  host    Pillow and numpy, as utils/image_utils.py process_input_image and scene/__init__.py _populate_gray_images: mask,
          resize, divide; once for the training image, once more for the gray image; the results uploaded
  device  gs2m_ingest: one upload of the bytes, everything else kernels (upload included in the time)
File decoding (PNG -> bytes) is common to both routes and stays on the host; it is timed separately on one image.  The two
routes' results are compared bit for bit before anything is timed."""
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

import gs2m_ingest  # noqa: E402


def host_route(image, mask, res, gray_res, device):
    """numpy / Pillow on the host, then the upload of the float results"""
    from PIL import Image

    def process(resolution):
        a = np.expand_dims(mask, axis=-1).astype(np.float32)
        masked = np.clip((image.astype(np.float32) / 255.) * (a / np.max(a)), 0., 1.)
        small = Image.fromarray((masked * 255.).astype(np.uint8)).resize(resolution)
        return torch.from_numpy(np.array(small)) / 255.

    rgb = process(res).permute(2, 0, 1)
    alpha = torch.from_numpy(np.array(Image.fromarray(mask).resize(res))).float()
    alpha = (alpha / torch.max(alpha)).unsqueeze(0)
    g = process(gray_res).permute(2, 0, 1)
    gray = g[0:1] * 0.299 + g[1:2] * 0.587 + g[2:3] * 0.114
    return rgb.to(device), alpha.to(device), gray.to(device)


def device_route(image, mask, res, gray_res, device):
    staged = gs2m_ingest.stage(image, True, mask, device)
    rgb, alpha = gs2m_ingest.process_input_image(staged, res)
    return rgb, alpha, gs2m_ingest.gray_image(staged, gray_res)


def timed(fn, views, repeats):
    """seconds of a pass over all views, ending in a device synchronisation: -> (best, median) of `repeats` passes"""
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = [fn(image, mask) for image, mask in views]  # (a loader keeps every view's tensors)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        del keep
    return min(times), float(np.median(times))


def main(argv=None):
    ap = argparse.ArgumentParser(description="host against device dataset ingestion")
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--width", type=int, default=1554)
    ap.add_argument("--height", type=int, default=1162)
    ap.add_argument("--resolution", "-r", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3, help="passes over all views on the host route; best and median are reported")
    ap.add_argument("--device-repeats", type=int, default=30, help="passes on the device route, whose pass is two orders of magnitude shorter")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    from PIL import Image
    dev = torch.device("cuda")
    W, H = a.width, a.height
    res = gs2m_ingest.target_resolution(W, H, a.resolution)
    ncc_scale = 1.0 / a.resolution if a.resolution in (1, 2, 4, 8) else 1.0
    gray_res = (int(res[0] / ncc_scale), int(res[1] / ncc_scale))
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:H, 0:W]
    views = []
    for k in range(a.views):
        image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        mask = (np.clip((0.4 * H - np.hypot(x - 0.5 * W - 3 * k, y - 0.5 * H)) / 4.0, 0.0, 1.0) * 255.0).astype(np.uint8)
        views.append((image, mask))

    for x_host, x_dev, name in zip(host_route(*views[0], res, gray_res, dev), device_route(*views[0], res, gray_res, dev), ("rgb", "alpha", "gray")):
        assert x_host.shape == x_dev.shape and torch.equal(x_host.view(torch.int32), x_dev.view(torch.int32)), f"{name}: the routes differ"

    buf = io.BytesIO()
    Image.fromarray(views[0][0]).save(buf, format="PNG")
    t0 = time.perf_counter()
    for _ in range(3):
        np.array(Image.open(io.BytesIO(buf.getvalue())))
    decode = (time.perf_counter() - t0) / 3

    device_route(*views[0], res, gray_res, dev)  # the plans are cached from here on, as after a loader's first view
    t_host, t_host_med = timed(lambda i, m: host_route(i, m, res, gray_res, dev), views, a.repeats)
    t_dev, t_dev_med = timed(lambda i, m: device_route(i, m, res, gray_res, dev), views, a.device_repeats)

    # the kernels alone, on bytes that are already on the device
    staged = [(torch.from_numpy(i).to(dev), torch.from_numpy(m).to(dev)) for i, m in views[:8]]
    t_kernels = timed(lambda i, m: device_route(i, m, res, gray_res, dev), staged, a.device_repeats)[1] / len(staged)

    result = {"views": a.views, "size": [W, H], "resolution": a.resolution, "target": list(res), "gray_target": list(gray_res),
              "device": torch.cuda.get_device_name(0), "bit_identical": True,
              "host_ms_per_view": 1e3 * t_host_med / a.views, "device_ms_per_view": 1e3 * t_dev_med / a.views,
              "host_ms_per_view_best": 1e3 * t_host / a.views, "device_ms_per_view_best": 1e3 * t_dev / a.views,
              "device_kernels_ms_per_view": 1e3 * t_kernels, "png_decode_ms_per_view_noise_image": 1e3 * decode,
              "host_s_total": t_host_med, "device_s_total": t_dev_med, "speedup": t_host_med / t_dev_med,
              "passes": {"host": a.repeats, "device": a.device_repeats}}
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=2)
            f.write("\n")
    return result


if __name__ == "__main__":
    main()
