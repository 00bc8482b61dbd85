"""numpy restatement of the dataset ingestion arithmetic: Pillow's default 8-bit resize (BICUBIC, two
fixed-point passes), the reference's process_input_image (masking, floats, alpha), its gray image and loadCam's target size.
Imported by tests/test_ingest.py (which holds it to Pillow and to the golden file) and tests/test_ingest_gpu.py (which holds
the kernels to it).  Plain numpy, no GPU, no Pillow."""
import math

import numpy as np

PRECISION_BITS = 22

# (W, H) -> (w, h): the resize cases of both test files
SHAPES = [((37, 23), (18, 12)), ((64, 48), (32, 24)), ((101, 77), (50, 38)), ((31, 17), (40, 29)), ((388, 290), (194, 145)),
          ((50, 40), (50, 13)), ((9, 7), (3, 2)), ((200, 3), (67, 1)), ((5, 5), (1, 1)), ((33, 20), (11, 20)), ((300, 5), (150, 3)),
          ((24, 19), (24, 19))]


def bicubic(t, a=-0.5):
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def plan(n_in, n_out):
    """-> (bounds int32 (n_out, 2): first input sample and count, coeffs int32 (n_out, ksize), ksize) of one axis"""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    coeffs = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [bicubic((x + xmin - center + 0.5) / filterscale) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            coeffs[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
    return bounds, coeffs, ksize


def _pass(img, n_out, axis):
    """one pass along `axis` (0: rows, 1: columns) of a (H, W, C) uint8 array -> uint8"""
    n_in = img.shape[axis]
    if n_in == n_out:
        return img
    bounds, coeffs, _ = plan(n_in, n_out)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.int64)
    for xx in range(n_out):
        x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        k = coeffs[xx, :n].astype(np.int64).reshape((n,) + (1,) * (src.ndim - 1))
        out[xx] = ((1 << (PRECISION_BITS - 1)) + (src[x0:x0 + n] * k).sum(axis=0)) >> PRECISION_BITS
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resize(img, size):
    """Pillow's `Image.resize(size)` of an 8-bit L (H, W) or RGB (H, W, 3) array; size = (w, h)"""
    a = img[:, :, None] if img.ndim == 2 else img
    a = _pass(_pass(a, size[0], 1), size[1], 0)
    return np.ascontiguousarray(a[:, :, 0] if img.ndim == 2 else a)


def mask_image(rgb, alpha):
    """the mask_gt product at the original size: (H, W, 3) uint8 and (H, W) uint8 -> (H, W, 3) uint8"""
    image = rgb[..., :3].astype(np.float32)
    a = alpha[..., None].astype(np.float32)
    m = (image / np.float32(255.)) * (a / np.max(a))
    return (np.clip(m, np.float32(0.), np.float32(1.)) * np.float32(255.)).astype(np.uint8)


def process_input_image(image, resolution, mask_gt=False, mask=None):
    """image: (H, W) / (H, W, 3) / (H, W, 4) uint8; mask: (H, W) uint8 or None; resolution = (w, h)
    -> (rgb float32 (C, h, w), alpha float32 (1, h, w) or None)"""
    alpha = mask
    if image.ndim == 3 and image.shape[2] == 4:
        alpha = image[..., 3] if alpha is None else alpha
        image = image[..., :3]
    if mask_gt and alpha is not None:
        image = mask_image(image, alpha)
    out = resize(np.ascontiguousarray(image), resolution).astype(np.float32) / np.float32(255.)
    out = out[None] if out.ndim == 2 else np.ascontiguousarray(out.transpose(2, 0, 1))
    if alpha is not None:
        a = resize(np.ascontiguousarray(alpha), resolution).astype(np.float32)
        alpha = (a / np.max(a))[None]
    return out, alpha


def gray(rgb):
    """(3, h, w) float32 -> (1, h, w) float32, the products and sums rounded one by one in fp32"""
    return (rgb[0:1] * np.float32(0.299) + rgb[1:2] * np.float32(0.587)) + rgb[2:3] * np.float32(0.114)


def gray_image(image, resolution, mask_gt=False, mask=None):
    return gray(process_input_image(image, resolution, mask_gt, mask)[0][:3])


def target_resolution(orig_w, orig_h, resolution, resolution_scale=1.0):
    if resolution in (1, 2, 4, 8):
        scale = resolution_scale * resolution
        return round(orig_w / scale), round(orig_h / scale)
    if resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)
