"""What undistorting a dataset costs.

    python tools/undistort_bench.py [--views 49] [--width 1554] [--height 1162] [--points 500000] [--out profiles/undistort_bench.json]

A DTU scan's worth of synthetic images under an OPENCV camera with mild, DTU-like coefficients, and 500 k observations:
  warp        gs2m_undistort_images_u8 on the whole batch, bytes already on the device (device events around `--calls` calls)
  points      gs2m_undistort_points on the observations, likewise
  grid_sample the same warp through torch.nn.functional.grid_sample on the same GPU, same process: the sampling alone on a float
              batch with a prebuilt grid, and with the uint8 -> float conversion, the rounding back and the batch's grid included
              (what a caller who holds bytes has to run); the positions come from the same fp64 arithmetic
  host        the same warp on the CPU through OpenCV's remap where cv2 imports, through torch's CPU grid_sample otherwise
  dataset     the whole undistort_dataset on files (decode, upload, warp, encode, write), with Pillow's and with the device's PNG
Medians of `--repeats` after a warm-up.  The warp's bytes are compared with grid_sample's before anything is timed (fp32 against
fp64: a byte may differ by 1)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-2m_amd"))

import gs2m_colmap  # noqa: E402
import gs2m_undistort as U  # noqa: E402


def event_ms(fn, calls, repeats):
    """median over `repeats` windows of the device time of one call, each window `calls` calls between two events"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return float(np.median(out)), [float(v) for v in out]


def wall_s(fn, repeats, warm=True):
    if warm:
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out)), out


def source_grid(cam, oc, device):
    """the warp's source positions (the contract's fp64 arithmetic, in torch on the device) as grid_sample's normalised grid with
    align_corners=True, float32 (1, oh, ow, 2)"""
    p = [float(v) for v in cam.params]
    fx, fy, cx, cy, k1, k2, p1, p2 = p
    q = [float(v) for v in oc.params]
    x = torch.arange(oc.width, dtype=torch.float64, device=device)[None, :].expand(oc.height, oc.width)
    y = torch.arange(oc.height, dtype=torch.float64, device=device)[:, None].expand(oc.height, oc.width)
    u, v = ((x + 0.5) - q[2]) / q[0], ((y + 0.5) - q[3]) / q[1]
    u2, v2, uv = u * u, v * v, u * v
    r2 = u2 + v2
    rad = k1 * r2 + k2 * (r2 * r2)
    pu = u + ((u * rad + (2.0 * p1) * uv) + p2 * (r2 + 2.0 * u2))
    pv = v + ((v * rad + (2.0 * p2) * uv) + p1 * (r2 + 2.0 * v2))
    sx, sy = (fx * pu + cx) - 0.5, (fy * pv + cy) - 0.5
    return torch.stack([2.0 * sx / (cam.width - 1) - 1.0, 2.0 * sy / (cam.height - 1) - 1.0], dim=2)[None].float()


def main(argv=None):
    ap = argparse.ArgumentParser(description="undistortion: the HIP kernels against grid_sample and the host")
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--width", type=int, default=1554)
    ap.add_argument("--height", type=int, default=1162)
    ap.add_argument("--points", type=int, default=500_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="kernel calls per timed window")
    ap.add_argument("--skip-dataset", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the benchmark needs a HIP device"
    dev = torch.device("cuda")
    W, H, n = a.width, a.height, a.views
    f = 2.5 * W  # DTU: 1554 x 1162 at a focal length of ~2890 px, radial distortion of a few pixels at the corners
    cam = gs2m_colmap.Camera(1, "OPENCV", W, H, np.array([f, f * 1.002, 0.5 * W + 3.1, 0.5 * H - 2.3, -0.08, 0.05, 4e-4, -3e-4]))
    oc = U.undistort_camera(cam)
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(xx // 3 + yy // 5) % 256, (xx // 7 * 3 + yy // 2) % 256, (xx + yy) // 9 % 256], axis=2)
    views = [np.clip(base + rng.integers(-6, 7, (H, W, 3)) + 2 * k, 0, 255).astype(np.uint8) for k in range(n)]
    batch = torch.from_numpy(np.stack(views)).to(dev)
    xy = torch.from_numpy(rng.uniform([0.0, 0.0], [W, H], (a.points, 2))).to(dev)

    # ---- the yardstick computes the same warp ----
    grid1 = source_grid(cam, oc, dev)

    def grid_sample_u8(b):
        x = b.permute(0, 3, 1, 2).float()
        y = torch.nn.functional.grid_sample(x, grid1.expand(b.shape[0], -1, -1, -1), mode="bilinear", padding_mode="zeros", align_corners=True)
        return torch.floor(y + 0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    ours, valid = U.undistort_images(batch[:2], cam, oc, valid=True)
    theirs = grid_sample_u8(batch[:2])
    inner = (valid == 255)
    inner[0, :] = inner[-1, :] = False  # (grid_sample fades into its zero padding where a tap lies outside; the contract cuts)
    inner[:, 0] = inner[:, -1] = False
    diff = (ours.int() - theirs.int()).abs()[:, inner]
    assert int(diff.max()) <= 1, f"the warp and grid_sample differ by {int(diff.max())}"
    differing = float((diff != 0).float().mean())

    # ---- kernels ----
    warp_ms, warp_all = event_ms(lambda: U.undistort_images(batch, cam, oc), a.calls, a.repeats)
    points_ms, points_all = event_ms(lambda: U.undistort_points(xy, cam, oc), a.calls, a.repeats)
    xf = batch.permute(0, 3, 1, 2).float().contiguous()
    gridn = grid1.expand(n, -1, -1, -1).contiguous()
    gs_only_ms, gs_only_all = event_ms(lambda: torch.nn.functional.grid_sample(xf, gridn, mode="bilinear", padding_mode="zeros", align_corners=True),
                                       max(1, a.calls // 4), a.repeats)
    del xf, gridn
    gs_u8_ms, gs_u8_all = event_ms(lambda: grid_sample_u8(batch), max(1, a.calls // 4), a.repeats)

    # ---- the host ----
    try:
        import cv2
        mx = ((grid1[0, :, :, 0].double().cpu().numpy() + 1.0) * 0.5 * (W - 1)).astype(np.float32)
        my = ((grid1[0, :, :, 1].double().cpu().numpy() + 1.0) * 0.5 * (H - 1)).astype(np.float32)
        host_name = "cv2.remap (INTER_LINEAR), prebuilt maps"
        host_s, host_all = wall_s(lambda: [cv2.remap(v, mx, my, cv2.INTER_LINEAR) for v in views], a.repeats)
    except ImportError:
        gh = grid1.cpu()
        hb = [torch.from_numpy(v)[None] for v in views]
        host_name = f"torch CPU grid_sample, {torch.get_num_threads()} threads, uint8 -> float -> uint8, prebuilt grid (cv2 does not import here)"

        def host():
            for b in hb:
                y = torch.nn.functional.grid_sample(b.permute(0, 3, 1, 2).float(), gh, mode="bilinear", padding_mode="zeros", align_corners=True)
                torch.floor(y + 0.5).clamp_(0, 255).to(torch.uint8)

        host_s, host_all = wall_s(host, min(3, a.repeats))

    pix = oc.width * oc.height
    bytes_moved = n * pix * 3 * 2  # every output byte written once, about as many source bytes read once
    result = {"device": torch.cuda.get_device_name(0), "views": n, "size": [W, H], "out_size": [oc.width, oc.height], "camera": "OPENCV " + str([float(v) for v in cam.params]),
              "points": a.points, "repeats": a.repeats, "calls_per_window": a.calls,
              "warp_ms_per_batch": warp_ms, "warp_ms_per_batch_all": warp_all, "warp_ms_per_view": warp_ms / n,
              "warp_gbytes_per_s_read_plus_written": bytes_moved / (warp_ms * 1e-3) / 1e9,
              "points_ms": points_ms, "points_ms_all": points_all, "points_per_s": a.points / (points_ms * 1e-3),
              "grid_sample_only_ms_per_batch": gs_only_ms, "grid_sample_only_ms_per_batch_all": gs_only_all,
              "grid_sample_u8_ms_per_batch": gs_u8_ms, "grid_sample_u8_ms_per_batch_all": gs_u8_all,
              "warp_vs_grid_sample_only": gs_only_ms / warp_ms, "warp_vs_grid_sample_u8": gs_u8_ms / warp_ms,
              "bytes_differing_from_grid_sample_by_1": differing,
              "host": host_name, "host_s_per_batch": host_s, "host_s_per_batch_all": host_all, "warp_vs_host": host_s * 1e3 / warp_ms}

    # ---- the whole tool on files ----
    if not a.skip_dataset:
        from PIL import Image as PILImage
        root = tempfile.mkdtemp(prefix="undistort_bench_")
        try:
            os.makedirs(os.path.join(root, "input"))
            images = []
            per = a.points // n
            for k, v in enumerate(views):
                PILImage.fromarray(v).save(os.path.join(root, "input", f"view_{k:03d}.png"), compress_level=1)
                images.append(gs2m_colmap.Image(k + 1, np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.0, 0.0, 3.0]), 1, f"view_{k:03d}.png",
                                                rng.uniform([0.0, 0.0], [W, H], (per, 2)), np.arange(1, per + 1)))
            gs2m_colmap.write_model(os.path.join(root, "distorted", "sparse", "0"), [cam], images, np.zeros((16, 3)), np.zeros((16, 3), np.uint8))
            for key, device_png in (("dataset_s_host_png", False), ("dataset_s_device_png", True)):
                med, every = wall_s(lambda: U.undistort_dataset(root, device_png=device_png), a.repeats)
                result[key], result[key + "_all"] = med, every
        finally:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=2)
            fh.write("\n")
    return result


if __name__ == "__main__":
    main()
