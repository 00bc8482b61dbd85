"""Image quality of rendered views on the GPU: metrics.py's PSNR, SSIM (include/gs2m_metrics.h, csrc/image_metrics.hip;
DESIGN.md §12) and LPIPS (gs2m_lpips.py, include/gs2m_lpips.h, csrc/lpips.hip).

    python gs-2m_amd/gs2m_metrics.py -m MODEL [--split test] [--method ours_30000] [--lpips-vgg VGG16.pth --lpips-lin VGG.pth]

scores every MODEL/<split>/<method>/render/<name> against gt/<name> -- render.py's layout -- and merges the means into
MODEL/metrics.json under <method>, as metrics.py:38-78 does.  The images are scored as the 8-bit values they are stored as: one
kernel reads a pair once and returns the exact integer sum of squared differences and the fp64 sum of the SSIM map
(utils/loss_utils.py:30-70 on value / 255, its moments and the map in fp64); the host forms PSNR and the means in float64.

LPIPS (metrics.py:57) needs VGG weights this stack neither carries nor fetches: it is computed, and the `lpips` key written, when
the user passes the two files the reference downloads (torchvision's vgg16 state dict and the LPIPS v0.1 vgg.pth linear
layers); without them the key is not written.  `score_views` renders and scores views without leaving the device; of render.py's per-view outputs it can
write render/ and gt/ only.  gs2m_render.py writes the whole tree this command reads -- render, gt, normal, depth and the
material maps.

There is NO CPU fallback: `image_metrics` refuses CPU tensors.  `collect_pairs` and `merge_metrics` are host-only."""
import argparse
import ctypes as C
import json
import os

import torch

import gs2m_lpips
import gs2m_native as N

TILE_W, TILE_H = 64, 32  # GS2M_METRICS_TILE_W / _H of include/gs2m_metrics.h: the pixels one workgroup takes
BATCH_BYTES = 256 << 20  # `evaluate` uploads at most this much per batch (both images of every pair)


def _u8(t, name, who):
    """dtype and layout first, so that each refusal names what is wrong with the tensor wherever it lives"""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{who}: `{name}` must be a CUDA tensor on a HIP device; there is no CPU path")
    if t.dtype != torch.uint8:
        raise RuntimeError(f"{who}: `{name}` must be uint8, got {t.dtype}")
    if t.dim() != 4 or t.shape[3] not in (1, 3):
        raise RuntimeError(f"{who}: `{name}` must have shape (N, H, W, CH) with CH 1 or 3, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{who}: `{name}` must be contiguous (N, H, W, CH), got strides {t.stride()}")
    if not t.is_cuda:
        raise RuntimeError(f"{who}: `{name}` must be a CUDA tensor on a HIP device; there is no CPU path")
    return t


def image_sums(a, b):
    """uint8 device tensors (N, H, W, CH) -> (sse, ssim_sum): per image the exact int64 sum of (a - b)^2 and the float64 sum of
    the SSIM map over all CH H W elements, both on the device.  One launch pair for the whole batch."""
    who = "image_metrics"
    a, b = _u8(a, "a", who), _u8(b, "b", who)
    if a.shape != b.shape or a.device != b.device:
        raise RuntimeError(f"{who}: `a` {tuple(a.shape)} on {a.device} and `b` {tuple(b.shape)} on {b.device} must match")
    n, h, w, ch = a.shape
    dev = a.device
    sse = torch.empty(n, dtype=torch.int64, device=dev)
    ssim_sum = torch.empty(n, dtype=torch.float64, device=dev)
    if n == 0:
        return sse, ssim_sum
    nbytes = C.c_longlong()
    N.check(N.lib().gs2m_image_metrics_workspace_bytes(n, h, w, ch, C.byref(nbytes)), "gs2m_image_metrics_workspace_bytes")
    ws = torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device=dev)
    N.launch("gs2m_image_metrics", dev, n, h, w, ch, a.data_ptr(), b.data_ptr(), ws.data_ptr(), ws.numel() * 8, sse.data_ptr(),
             ssim_sum.data_ptr())
    return sse, ssim_sum


def psnr_from_sse(sse, count):
    """utils/image_utils.py:22-24 on 8-bit values, in float64: mse = sse / (255^2 count), 20 log10(1 / sqrt(mse)); +inf at 0."""
    mse = sse.to(torch.float64) / (255.0 * 255.0 * count)
    return 20.0 * torch.log10(1.0 / torch.sqrt(mse))


def image_metrics(a, b):
    """uint8 device tensors (N, H, W, CH), CH in {1, 3} -> (psnr, ssim): two float64 host tensors of length N."""
    sse, ssim_sum = image_sums(a, b)
    count = a.shape[1] * a.shape[2] * a.shape[3]
    return psnr_from_sse(sse.cpu(), count), ssim_sum.cpu() / count


def collect_pairs(render_dir, gt_dir):
    """[(name, render path, gt path)] for every file of `render_dir`, sorted by name; FileNotFoundError naming the first
    file that has no namesake in `gt_dir`."""
    pairs = []
    for name in sorted(os.listdir(render_dir)):
        gt = os.path.join(gt_dir, name)
        if not os.path.isfile(gt):
            raise FileNotFoundError(f"gs2m_metrics: {os.path.join(render_dir, name)} has no ground truth {gt}")
        pairs.append((name, os.path.join(render_dir, name), gt))
    return pairs


def merge_metrics(path, method, values):
    """metrics.py:63-76: the JSON object at `path` (empty when the file does not exist) with `method`'s entry replaced by
    `values`, written back with indent=4.  -> the whole object."""
    metrics = {}
    if os.path.exists(path):
        with open(path, "r") as f:
            metrics = json.load(f)
    metrics[method] = dict(values)
    with open(path, "w") as f:
        json.dump(metrics, f, indent=4)
    return metrics


def _channels(img, path):
    if img.mode in ("RGB", "RGBA"):  # metrics.py:33 keeps the first three channels
        return 3
    if img.mode == "L":
        return 1
    raise ValueError(f"gs2m_metrics: {path} has mode {img.mode}; 8-bit L, RGB and RGBA images are scored")


def _decode(path):
    import numpy as np
    from PIL import Image
    with Image.open(path) as img:
        arr = np.asarray(img)
    return arr[:, :, None] if arr.ndim == 2 else arr[:, :, :3]


def score_files(pairs, device="cuda", batch_bytes=BATCH_BYTES, lpips_weights=None):
    """(psnr, ssim) of every (name, render path, gt path) of `pairs` in their order: float64 host tensors.  Pairs of one
    (H, W, CH) go to the device together, at most `batch_bytes` per upload, one upload and one launch per batch.
    `lpips_weights` (gs2m_lpips.load_weights): -> (psnr, ssim, lpips), LPIPS from the same uploaded batch; a grey pair is a
    ValueError naming the file."""
    import numpy as np
    from PIL import Image
    groups = {}
    for k, (name, rp, gp) in enumerate(pairs):
        with Image.open(rp) as r, Image.open(gp) as g:  # the header only: nothing is decoded yet
            kr, kg = (r.size[1], r.size[0], _channels(r, rp)), (g.size[1], g.size[0], _channels(g, gp))
        if kr != kg:
            raise ValueError(f"gs2m_metrics: {rp} is (H, W, CH) = {kr} but its ground truth {gp} is {kg}")
        if lpips_weights is not None and kr[2] != 3:
            raise ValueError(f"gs2m_metrics: {rp} is a grey image; LPIPS scores 3-channel images (drop the LPIPS weights to score it)")
        groups.setdefault(kr, []).append(k)
    psnr = torch.empty(len(pairs), dtype=torch.float64)
    ssim = torch.empty(len(pairs), dtype=torch.float64)
    lp = torch.empty(len(pairs), dtype=torch.float64)
    for (h, w, ch), idx in groups.items():
        per = max(1, int(batch_bytes) // (2 * h * w * ch))
        for s in range(0, len(idx), per):
            part = idx[s:s + per]
            host = np.empty((2, len(part), h, w, ch), np.uint8)
            for j, k in enumerate(part):
                host[0, j], host[1, j] = _decode(pairs[k][1]), _decode(pairs[k][2])
            both = torch.from_numpy(host).to(device)
            p, q = image_metrics(both[0], both[1])
            psnr[part], ssim[part] = p, q
            if lpips_weights is not None:
                lp[part] = gs2m_lpips.lpips(both[0], both[1], lpips_weights)
    return (psnr, ssim) if lpips_weights is None else (psnr, ssim, lp)


def evaluate(model_path, split="test", method="ours_30000", device="cuda", lpips_weights=None):
    """metrics.py:38-78: -> {"ssim", "psnr", "n_images"}, the float64 means of the per-image values of
    <model_path>/<split>/<method>/{render, gt}; "ssim" and "psnr" are merged into <model_path>/metrics.json under `method`.
    With `lpips_weights` (gs2m_lpips.load_weights) "lpips" joins them, in the result and in the file."""
    split_dir = os.path.join(model_path, split)
    if not os.path.isdir(split_dir):
        raise FileNotFoundError(f"Split directory {split_dir} does not exist, did you forget to specify --split?.")
    method_dir = os.path.join(split_dir, method)
    pairs = collect_pairs(os.path.join(method_dir, "render"), os.path.join(method_dir, "gt"))
    print(f"[>] Evaluate metrics for: {method_dir}")
    psnr, ssim, *lp = score_files(pairs, device, lpips_weights=lpips_weights)
    out = {"ssim": ssim.mean().item(), "psnr": psnr.mean().item(), "n_images": len(pairs)}
    values = {"ssim": out["ssim"], "psnr": out["psnr"]}
    print("[-] SSIM : {:>12.7f}".format(out["ssim"]))
    print("[-] PSNR : {:>12.7f}".format(out["psnr"]))
    if lp:
        out["lpips"] = values["lpips"] = lp[0].mean().item()
        print("[-] LPIPS: {:>12.7f}".format(out["lpips"]))  # metrics.py:61
    metric_file = os.path.join(model_path, "metrics.json")
    merge_metrics(metric_file, method, values)
    print(f"[>] Metrics saved to: {metric_file}")
    return out


def quantise(image):
    """(3, H, W) float on the device -> (H, W, 3) uint8 on the device, as torchvision.utils.save_image rounds (and as
    gs2m_mesh.render_views saves its colours): clamp(0, 1) * 255 + 0.5, clamp, truncate."""
    return image.clamp(0.0, 1.0).mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).contiguous()


def score_views(gaussians, views, background, out_dir=None, white_background=False, png="host", lpips_weights=None):
    """Renders every view with this repository's render() and scores the 8-bit colour against the view's 8-bit ground truth
    (`view.gt_image`, (3+, H, W) float; render.py:77-79: clamped, `background` where `view.alpha_mask` <= 0.5 when
    `white_background`) on the device.  `out_dir`: also write out_dir/render/<stem>.png and out_dir/gt/<stem>.png, render.py's
    layout (`png`: "host" through Pillow, "device" through gs2m_png).  -> {"names", "psnr", "ssim"}: the stems and two float64 host tensors, one value per view;
    with `lpips_weights` (gs2m_lpips.load_weights) also "lpips", from the same two 8-bit images."""
    from gaussian_renderer import render
    from gs2m_scene import PipelineParams
    from gs2m_png import Writer
    writer = Writer(png)
    if out_dir is not None:
        for sub in ("render", "gt"):
            os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    names, sse, sums, counts, lp = [], [], [], [], []
    with torch.no_grad():
        for k, view in enumerate(views):
            if getattr(view, "image_name", None) is None:
                view.image_name = f"{k:05d}.png"
            stem = view.image_name.rsplit(".", 1)[0]
            if getattr(view, "gt_image", None) is None:
                raise ValueError(f"gs2m_metrics: view {stem} carries no gt_image")
            out = render(view, gaussians, PipelineParams(), background, material_stage=True)  # as gs2m_mesh.render_views
            img = quantise(out["render"])
            gt = torch.as_tensor(view.gt_image).to(img.device)[0:3].clamp(0.0, 1.0)
            if white_background:
                gt = torch.where(torch.as_tensor(view.alpha_mask).to(img.device) > 0.5, gt, background[:, None, None])
            gt = quantise(gt)
            e, s = image_sums(img[None], gt[None])
            names.append(stem); sse.append(e); sums.append(s); counts.append(img.numel())
            if lpips_weights is not None:
                lp.append(gs2m_lpips.lpips_device(img[None], gt[None], lpips_weights)[0])
            if out_dir is not None:
                writer.put(img, os.path.join(out_dir, "render", stem + ".png"))
                writer.put(gt, os.path.join(out_dir, "gt", stem + ".png"))
                writer.flush()
    if not names:
        out = {"names": [], "psnr": torch.empty(0, dtype=torch.float64), "ssim": torch.empty(0, dtype=torch.float64)}
    else:
        counts = torch.tensor(counts, dtype=torch.float64)
        out = {"names": names, "psnr": psnr_from_sse(torch.cat(sse).cpu(), counts), "ssim": torch.cat(sums).cpu() / counts}
    if lpips_weights is not None:
        out["lpips"] = torch.cat(lp).cpu() if lp else torch.empty(0, dtype=torch.float64)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="PSNR, SSIM and -- given the weight files -- LPIPS of rendered views (metrics.py)")
    ap.add_argument("--model_path", "-m", required=True, type=str)
    ap.add_argument("--split", type=str, default="test", help="Split to evaluate on (train/test)")
    ap.add_argument("--method", type=str, default="ours_30000")
    ap.add_argument("--lpips-vgg", type=str, default=None, help="torchvision's vgg16 state dict (.pth); with --lpips-lin: also score LPIPS")
    ap.add_argument("--lpips-lin", type=str, default=None, help="the LPIPS v0.1 vgg.pth linear layers; nothing is downloaded")
    args = ap.parse_args(argv)
    if (args.lpips_vgg is None) != (args.lpips_lin is None):
        ap.error("--lpips-vgg and --lpips-lin go together: LPIPS needs both files, or neither to leave it out")
    weights = None if args.lpips_vgg is None else gs2m_lpips.load_weights(args.lpips_vgg, args.lpips_lin)
    return evaluate(args.model_path, args.split, args.method, lpips_weights=weights)


if __name__ == "__main__":
    main()
