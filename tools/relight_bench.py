"""Times the relighting stage (gs2m_envmap.py / gs2m_relight.py, csrc/envmap.hip) on one GPU.

    python tools/relight_bench.py [--width 4096] [--height 2048] [--res 512] [--repeats 20] [--json profiles/relight_bench.json]

The source is synthetic: a smooth sky of `--width` x `--height` with one very bright small disk (a sun about three pixels wide), written
once as a flat Radiance file by `write_hdr`.
  read_hdr            file -> (H, W, 3) on the device: the read, the header, the host scan, the upload and the decode kernel
  latlong_to_cubemap  the HIP conversion at `--res` with the default number of samples (device events)
  grid_sample         the same conversion written with torch.nn.functional.grid_sample over the S^2 sample grids, the directions and the
                      angles by torch operators (device events); `grid_sample_only`: the S^2 x 6 lookups alone, the grids prebuilt
  build_mips          CubemapLight.build_mips of the light (device events)
  relight_view        gs2m_relight.shade_view of one `--view-width` x `--view-height` view of a synthetic surface: render, shading, packing
The kernel and the baseline alternate in one process; each figure is the median over `--repeats` calls after a warm-up, with the spread.
Before anything is timed the baseline's cube map is compared with the kernel's."""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-2m_amd"))

import gs2m_envmap as E  # noqa: E402
import gs2m_relight as RL  # noqa: E402


def make_source(h, w, device):
    """(h, w, 3): a sky gradient and a sun -- 5e4 inside 1.5 pixels of its centre"""
    theta = ((torch.arange(h, device=device, dtype=torch.float32) + 0.5) / h * math.pi)[:, None]
    phi = (((torch.arange(w, device=device, dtype=torch.float32) + 0.5) * 2 / w - 1) * math.pi)[None, :]
    d = torch.stack(torch.broadcast_tensors(torch.sin(theta) * torch.sin(phi), torch.cos(theta), -torch.sin(theta) * torch.cos(phi)), dim=-1)
    sky = 0.2 + 0.6 * (d[..., 1:2] + 1) * torch.tensor([0.5, 0.7, 1.0], device=device) + 0.1 * torch.rand(h, w, 3, device=device,
                                                                                                         generator=torch.Generator(device).manual_seed(0))
    yy, xx = torch.meshgrid(torch.arange(h, device=device), torch.arange(w, device=device), indexing="ij")
    sun = ((yy - 0.3 * h) ** 2 + (xx - 0.62 * w) ** 2) <= 1.5 ** 2
    sky[sun] = torch.tensor([5e4, 4.6e4, 4e4], device=device)
    return sky.contiguous()


def cube_grids(hs, ws, res, s, angle, device):
    """the S^2 sample grids of every face for grid_sample on the source padded by one wrapped column on each side:
    -> (grids [(6, res, res, 2)] in (a, b) order, weights [(6, res, res)])"""
    from pbr.light import cube_to_dir
    k = torch.arange(res * s, device=device, dtype=torch.float32)
    coord = -1.0 + (2 * k + 1) / (res * s)
    y, x = torch.meshgrid(coord, coord, indexing="ij")
    inv = 1.0 / torch.sqrt(1.0 + x * x + y * y)
    w = inv * inv * inv
    ca, sa = math.cos(angle), math.sin(angle)
    gx, gy = [], []
    for f in range(6):
        d = cube_to_dir(f, x, y) * inv[..., None]
        rx, rz = ca * d[..., 0] - sa * d[..., 2], sa * d[..., 0] + ca * d[..., 2]
        theta = torch.acos(d[..., 1].clamp(-1.0, 1.0))
        phi = torch.atan2(rx, -rz)
        u = (phi / math.pi + 1.0) * 0.5 * ws - 0.5
        v = theta / math.pi * hs - 0.5
        gx.append(2.0 * (u + 1.5) / (ws + 2) - 1.0)  # pixel u of the source is pixel u + 1 of the padded one
        gy.append(2.0 * (v + 0.5) / hs - 1.0)
    grid = torch.stack((torch.stack(gx), torch.stack(gy)), dim=-1).view(6, res, s, res, s, 2)
    w6 = w.view(res, s, res, s)
    return ([grid[:, :, a, :, b].contiguous() for a in range(s) for b in range(s)],
            [w6[:, a, :, b].expand(6, res, res).contiguous() for a in range(s) for b in range(s)])


def grid_sample_lookups(src, grids, weights, scale):
    padded = torch.cat((src[:, -1:], src, src[:, :1]), dim=1).permute(2, 0, 1)[None].expand(6, -1, -1, -1)
    acc, wsum = 0.0, 0.0
    for g, w in zip(grids, weights):
        acc = acc + w[:, None] * F.grid_sample(padded, g, mode="bilinear", padding_mode="border", align_corners=False)
        wsum = wsum + w
    return (scale * acc / wsum[:, None]).permute(0, 2, 3, 1).contiguous()


def grid_sample_route(src, res, s, angle=0.0, scale=1.0):
    grids, weights = cube_grids(src.shape[0], src.shape[1], res, s, angle, src.device)
    return grid_sample_lookups(src, grids, weights, scale)


def _stats(xs):
    xs = np.asarray(xs)
    return {"median_ms": float(np.median(xs)), "min_ms": float(xs.min()), "max_ms": float(xs.max())}


def _events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def _view_scene(n_true, w, h):
    import gs2m_synth as S
    from gs2m_scene import Camera, GaussianParams, inverse_sigmoid
    sc = S.make_surface_scene(n_true, seed=0)
    t = {k: v.cuda() for k, v in sc.items()}
    gen = torch.Generator().manual_seed(1)
    material = [inverse_sigmoid(torch.rand(n_true, c, generator=gen).clamp(0.05, 0.95).cuda()) for c in (3, 1, 1)]
    model = GaussianParams(t["points"], t["shs"][:, :1].contiguous(), t["shs"][:, 1:].contiguous(), torch.log(t["scales"]), t["rotations"],
                           inverse_sigmoid(t["opacities"]), *material)
    views = [Camera(c, "cuda") for c in S.orbit_cameras(4, w, h, radius=6.0, centre=(0.0, -0.8, 6.0), fx=1.1 * w)]
    return model, views


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--view-width", type=int, default=1600)
    ap.add_argument("--view-height", type=int, default=1200)
    ap.add_argument("--gaussians", type=int, default=200_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("relight_bench: needs a HIP device; nothing is timed without one")
    dev = torch.device("cuda")
    src = make_source(a.height, a.width, dev)
    s = E.default_samples(a.res, a.width)
    result = {"source": [a.width, a.height], "res": a.res, "samples": s, "view": [a.view_width, a.view_height], "gaussians": a.gaussians,
              "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "sky.hdr")
        E.write_hdr(path, src)
        result["file_bytes"] = os.path.getsize(path)
        image = E.read_hdr(path, dev)  # warm-up
        t_read = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            image = E.read_hdr(path, dev)
            torch.cuda.synchronize()
            t_read.append((time.perf_counter() - t0) * 1e3)
        result["read_hdr"] = _stats(t_read)
    # the two conversions agree before they are timed
    cube = E.latlong_to_cubemap(image, a.res, s)
    base = grid_sample_route(image, a.res, s)
    result["baseline_relative_distance"] = float((cube - base).abs().max() / cube.abs().max())
    assert result["baseline_relative_distance"] < 1e-2, result["baseline_relative_distance"]
    grids, weights = cube_grids(a.height, a.width, a.res, s, 0.0, dev)
    t_kernel, t_base, t_lookup = [], [], []
    for r in range(a.repeats + 2):
        tk, _ = _events(lambda: E.latlong_to_cubemap(image, a.res, s))
        tb, _ = _events(lambda: grid_sample_route(image, a.res, s))
        tl, _ = _events(lambda: grid_sample_lookups(image, grids, weights, 1.0))
        if r >= 2:
            t_kernel.append(tk); t_base.append(tb); t_lookup.append(tl)
    result["latlong_to_cubemap"] = _stats(t_kernel)
    result["grid_sample"] = _stats(t_base)
    result["grid_sample_only"] = _stats(t_lookup)
    result["speedup_grid_sample_over_kernel"] = float(np.median(t_base) / np.median(t_kernel))
    del grids, weights, base
    light = E.EnvLight(cube)
    t_mips = []
    with torch.no_grad():
        for r in range(a.repeats + 2):
            t, _ = _events(light.cubemap.build_mips)
            if r >= 2:
                t_mips.append(t)
    result["build_mips"] = _stats(t_mips)
    model, views = _view_scene(a.gaussians, a.view_width, a.view_height)
    t_view = []
    for r in range(a.repeats + len(views)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        RL.shade_view(model, views[r % len(views)], light, gamma=True, background="env")
        torch.cuda.synchronize()
        if r >= len(views):
            t_view.append((time.perf_counter() - t0) * 1e3)
    result["relight_view"] = _stats(t_view)
    print(json.dumps(result))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
