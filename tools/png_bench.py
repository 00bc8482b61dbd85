"""Times the PNG encoding of one view's images, Pillow on the host against gs2m_png on the device (csrc/png.hip).

    python tools/png_bench.py [--width 1600] [--height 1200] [--repeats 20] [--json profiles/png_bench.json]

The input is the nine 8-bit arrays per view of tools/view_maps_bench.py's scene, black and white background; they sit in device
memory, as gs2m_render.py forms them.
  pillow   Image.fromarray(array).save (Pillow's defaults) into memory; the copy of the arrays to the host is not counted
  device   gs2m_png.encode of the RGB group and of the RGBA group: kernels, the read-back of the streams and the container
           (IHDR / IDAT / IEND, zlib.crc32), until the files are bytes on the host; the file write is not counted
  kernels  the same launches alone, by device events (workspace allocation included, no read-back)
The two routes alternate in one process; each figure is the median over `--repeats` views after a warm-up pass, with the spread.
Every device-made file is decoded by Pillow and compared with its array before anything is timed."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gs2m_png as P  # noqa: E402
import view_maps_bench as VB  # noqa: E402


def _groups(images):
    """the view's arrays grouped by shape, as gs2m_png.Writer.flush does: RGB and RGBA"""
    groups = {}
    for name, t in images.items():
        groups.setdefault(tuple(t.shape), []).append(t)
    return list(groups.values())


def device_route(images):
    return [f for g in _groups(images) for f in P.encode(g)]


def device_kernels(images):
    for g in _groups(images):
        P.encode_streams_device(g)


def pillow_route(arrays):
    from PIL import Image
    total = 0
    for a in arrays:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="PNG")
        total += buf.tell()
    return total


def _stats(xs):
    xs = np.asarray(xs)
    return {"median_ms": float(np.median(xs)), "min_ms": float(xs.min()), "max_ms": float(xs.max())}


def main(argv=None):
    from PIL import Image
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda")
    sets = [VB.make_maps(a.height, a.width, dev, seed=s) for s in range(3)]
    result = {"width": a.width, "height": a.height, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "branches": {}}
    for white in (False, True):
        views = [VB.device_images(m, white) for m in sets]
        hosts = [[t.cpu().numpy() for g in _groups(v) for t in g] for v in views]
        for v, h in zip(views, hosts):  # warm-up of both routes, and the files are right
            files = device_route(v)
            pillow_route(h)
            for f, arr in zip(files, h):
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), arr)
        torch.cuda.synchronize()
        t_pil, t_dev, t_kern, b_pil, b_dev = [], [], [], [], []
        for r in range(a.repeats):
            v, h = views[r % len(views)], hosts[r % len(views)]
            t0 = time.perf_counter()
            b_pil.append(pillow_route(h))
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            files = device_route(v)
            t3 = time.perf_counter()
            b_dev.append(sum(len(f) for f in files))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            device_kernels(v)
            e1.record()
            e1.synchronize()
            t_pil.append((t1 - t0) * 1e3); t_dev.append((t3 - t2) * 1e3); t_kern.append(e0.elapsed_time(e1))
        result["branches"]["white_background" if white else "black_background"] = {
            "images_per_view": len(hosts[0]), "raw_bytes_per_view": int(sum(x.size for x in hosts[0])),
            "pillow": dict(_stats(t_pil), bytes_per_view=float(np.mean(b_pil))),
            "device": dict(_stats(t_dev), bytes_per_view=float(np.mean(b_dev))),
            "device_kernels": _stats(t_kern),
            "bytes_ratio_device_over_pillow": float(np.sum(b_dev) / np.sum(b_pil)),
            "speedup_pillow_over_device": float(np.median(t_pil) / np.median(t_dev))}
    print(json.dumps(result))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
