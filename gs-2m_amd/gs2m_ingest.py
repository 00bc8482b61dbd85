"""Dataset ingestion on the GPU: the reference's process_input_image (utils/image_utils.py:48-77), loadCam's target size
(utils/camera_utils.py:19-42) and the NCC gray image (scene/__init__.py:193-204) on the decoded 8-bit pixels
(include/gs2m_ingest.h, csrc/ingest.hip).

    rgb, alpha = process_input_image(pil_image, target_resolution(W, H, 2), mask_gt=True, mask=pil_mask)

The decoded bytes go to the device once, as uint8; the `--mask_gt` product, Pillow's default resize (BICUBIC, two fixed-point
passes) and the conversion to planar floats are kernels on torch's current stream, with no host synchronisation between the
upload and the result.  Integer arithmetic and fp32 evaluated as written: the results equal the reference's bit for bit.
`stage` keeps an upload on the device so that several resizes (the training image and the gray image) share it.

There is NO CPU fallback: the kernels refuse CPU tensors.  `target_resolution` and `host_plan` are host-only."""
import ctypes as C

import numpy as np
import torch

import gs2m_native as N

PLAN_HEADER = 4  # GS2M_RESIZE_PLAN_HEADER of include/gs2m_ingest.h: {in, out, ksize, 0} in front of the bounds

_plans = {}  # (in, out, device index) -> the plan on that device
_plan_stats = {"hits": 0, "misses": 0}


def add_ingest_arguments(ap):
    """the loader flags gs2m_train.py, gs2m_render.py and gs2m_mesh.py share (arguments/__init__.py: --masks, --mask_gt)"""
    ap.add_argument("--device-ingest", action="store_true", help="COLMAP dataset: read the images through gs2m_ingest -- the reference's resize "
                    "(Pillow's default filter, loadCam's size), masks and alpha masks, on the GPU")
    ap.add_argument("--masks", default="", help="--device-ingest: folder of <stem>.png foreground masks (absolute, or relative to the dataset)")
    ap.add_argument("--mask_gt", action="store_true", help="--device-ingest: multiply the images by their masks before the resize")
    ap.add_argument("--undistort", action="store_true", help="--device-ingest: undistort a SIMPLE_RADIAL / RADIAL / OPENCV / FULL_OPENCV model in memory "
                    "(gs2m_undistort): PINHOLE cameras, the images warped on the GPU in front of the resize, the valid mask as the alpha mask; "
                    "--masks then holds masks of the undistorted images")


def ingest_keywords(a):
    """load_colmap_dataset's keywords for the flags of add_ingest_arguments"""
    if a.undistort and not a.device_ingest:
        raise ValueError("--undistort needs --device-ingest: the images are warped on the GPU, the host route reads undistorted datasets only")
    return dict(ingest="undistort" if a.undistort else ("device" if a.device_ingest else "host"), masks=a.masks, mask_gt=a.mask_gt)


def target_resolution(orig_w, orig_h, resolution, resolution_scale=1.0):
    """loadCam's (width, height) for `-r resolution` (utils/camera_utils.py:23-42): round() for 1, 2, 4 and 8; -1 caps the width at
    1600; any other value is the target width; the last two truncate."""
    if resolution in (1, 2, 4, 8):
        scale = resolution_scale * resolution
        return round(orig_w / scale), round(orig_h / scale)
    if resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


def host_plan(n_in, n_out):
    """The resize plan of an axis of n_in -> n_out samples, built on the host in double precision (no GPU is touched):
    -> (plan int32[4 + 2 n_out + n_out ksize] as the kernels take it, bounds (n_out, 2) = first input sample and tap count,
    coeffs (n_out, ksize) in 22-bit fixed point, ksize); bounds and coeffs are views of plan."""
    nbytes, ksize = C.c_longlong(), C.c_int()
    N.check(N.lib().gs2m_resize_plan_bytes(int(n_in), int(n_out), C.byref(nbytes), C.byref(ksize)), "gs2m_resize_plan_bytes")
    plan = np.empty(nbytes.value // 4, np.int32)
    N.check(N.lib().gs2m_resize_plan(int(n_in), int(n_out), plan.ctypes.data), "gs2m_resize_plan")
    k = ksize.value
    bounds = plan[PLAN_HEADER:PLAN_HEADER + 2 * n_out].reshape(n_out, 2)
    coeffs = plan[PLAN_HEADER + 2 * n_out:].reshape(n_out, k)
    return plan, bounds, coeffs, k


def _device_plan(n_in, n_out, device):
    key = (int(n_in), int(n_out), device.index if device.index is not None else torch.cuda.current_device())
    plan = _plans.get(key)
    if plan is None:
        _plan_stats["misses"] += 1
        plan = _plans[key] = torch.from_numpy(host_plan(n_in, n_out)[0]).to(device)
    else:
        _plan_stats["hits"] += 1
    return plan


def plan_cache_info():
    """{"hits", "misses", "size"} of the per-(in, out, device) plan cache"""
    return dict(_plan_stats, size=len(_plans))


def plan_cache_clear():
    _plans.clear()
    _plan_stats.update(hits=0, misses=0)


def _u8(t, name, who, dims):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: `{name}` must be a CUDA tensor on a HIP device; there is no CPU path")
    if t.dtype != torch.uint8:
        raise RuntimeError(f"{who}: `{name}` must be uint8, got {t.dtype}")
    if t.dim() not in dims or (t.dim() == 3 and t.shape[2] not in (1, 3)) or t.numel() == 0:
        raise RuntimeError(f"{who}: `{name}` must have shape (H, W, CH) with CH 1 or 3" + (" or (H, W)" if 2 in dims else "") + f", got {tuple(t.shape)}")
    return t.contiguous()


def image_max(t):
    """uint8 device tensor of any shape -> its maximum as an int32 tensor of one element on the device (0 when empty)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8:
        raise RuntimeError("image_max: `t` must be a uint8 CUDA tensor on a HIP device; there is no CPU path")
    t = t.contiguous()
    out = torch.empty(1, dtype=torch.int32, device=t.device)
    N.launch("gs2m_image_max_u8", t.device, t.numel(), N.ptr(t), out.data_ptr())
    return out


def mask_image(rgb, alpha, alpha_max=None):
    """The `--mask_gt` product at the original size: (H, W, 3) and (H, W) uint8 device tensors -> (H, W, 3) uint8;
    `alpha_max`: image_max(alpha) when the caller has it.  A mask whose maximum is 0 gives zeros."""
    who = "mask_image"
    rgb, alpha = _u8(rgb, "rgb", who, (3,)), _u8(alpha, "alpha", who, (2,))
    if rgb.shape[2] != 3 or alpha.shape != rgb.shape[:2] or alpha.device != rgb.device:
        raise RuntimeError(f"{who}: `rgb` {tuple(rgb.shape)} on {rgb.device} must be (H, W, 3) and `alpha` {tuple(alpha.shape)} on {alpha.device} its (H, W)")
    alpha_max = image_max(alpha) if alpha_max is None else alpha_max
    out = torch.empty_like(rgb)
    N.launch("gs2m_image_mask_u8", rgb.device, rgb.shape[1], rgb.shape[0], rgb.data_ptr(), alpha.data_ptr(), alpha_max.data_ptr(), out.data_ptr())
    return out


def resize(t, size):
    """Pillow's `Image.resize(size)` (BICUBIC) of an 8-bit image: (H, W) or (H, W, CH) uint8 device tensor, CH in {1, 3},
    size = (w, h) -> the same layout at (h, w), byte for byte what Pillow returns."""
    t = _u8(t, "t", "resize", (2, 3))
    h, w = t.shape[0], t.shape[1]
    ch = 1 if t.dim() == 2 else t.shape[2]
    ow, oh = int(size[0]), int(size[1])
    if ow < 1 or oh < 1:
        raise ValueError(f"resize: height and width must be > 0, got {(ow, oh)}")
    dev = t.device
    nbytes = C.c_longlong()
    N.check(N.lib().gs2m_image_resize_workspace_bytes(w, h, ch, ow, oh, C.byref(nbytes)), "gs2m_image_resize_workspace_bytes")
    plan_x = _device_plan(w, ow, dev) if w != ow else None
    plan_y = _device_plan(h, oh, dev) if h != oh else None
    tmp = torch.empty(nbytes.value, dtype=torch.uint8, device=dev) if nbytes.value else None
    out = torch.empty((oh, ow) if t.dim() == 2 else (oh, ow, ch), dtype=torch.uint8, device=dev)
    N.launch("gs2m_image_resize_u8", dev, w, h, ch, t.data_ptr(), ow, oh, N.ptr(plan_x), N.ptr(plan_y), N.ptr(tmp), out.data_ptr())
    return out


def unpack(t, alpha=None, alpha_max=None, rgb=True, gray=False):
    """One pass over a resized image, (H, W) or (H, W, CH) uint8 on the device: -> (rgb (CH, H, W) = u8 / 255 or None,
    alpha (1, H, W) = alpha / its maximum or None, gray (1, H, W) or None), float32.  `alpha`: (H, W) uint8; `alpha_max`:
    image_max(alpha) when the caller has it."""
    who = "unpack"
    t = _u8(t, "t", who, (2, 3))
    h, w = t.shape[0], t.shape[1]
    ch = 1 if t.dim() == 2 else t.shape[2]
    dev = t.device
    if gray and ch != 3:
        raise ValueError(f"{who}: the gray image needs 3 channels, got {ch}")
    if alpha is not None:
        alpha = _u8(alpha, "alpha", who, (2,))
        if alpha.shape != (h, w) or alpha.device != dev:
            raise RuntimeError(f"{who}: `alpha` {tuple(alpha.shape)} on {alpha.device} must be {(h, w)} on {dev}")
        alpha_max = image_max(alpha) if alpha_max is None else alpha_max
    o_rgb = torch.empty((ch, h, w), dtype=torch.float32, device=dev) if rgb else None
    o_alpha = torch.empty((1, h, w), dtype=torch.float32, device=dev) if alpha is not None else None
    o_gray = torch.empty((1, h, w), dtype=torch.float32, device=dev) if gray else None
    N.launch("gs2m_image_unpack", dev, w, h, ch, t.data_ptr(), N.ptr(alpha), N.ptr(alpha_max) if alpha is not None else None,
             N.ptr(o_rgb), N.ptr(o_alpha), N.ptr(o_gray))
    return o_rgb, o_alpha, o_gray


class Staged:
    """An image on the device as process_input_image sees it in front of the resize: `image` (H, W) or (H, W, 3) uint8 -- masked
    when `mask_gt` asked for it -- and `alpha` (H, W) uint8 or None."""

    def __init__(self, image, alpha):
        self.image, self.alpha = image, alpha

    @property
    def size(self):
        return self.image.shape[1], self.image.shape[0]


def _pixels(x, what, name):
    """PIL image / uint8 array / uint8 tensor -> uint8 tensor (H, W) or (H, W, C), on the host unless it was given on a device"""
    label = f" of {name}" if name else ""
    if isinstance(x, torch.Tensor):
        t = x
    else:
        mode = getattr(x, "mode", None)
        if mode is not None and mode not in ("L", "RGB", "RGBA"):
            raise ValueError(f"gs2m_ingest: the {what}{label} has mode {mode}; 8-bit L, RGB and RGBA images are read")
        t = torch.from_numpy(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else np.array(x))  # (a PIL image's array view is read-only)
    if t.dtype != torch.uint8 or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] not in (1, 3, 4)) or t.numel() == 0:
        raise ValueError(f"gs2m_ingest: the {what}{label} must be 8-bit (H, W), (H, W, 3) or (H, W, 4), got {t.dtype} {tuple(t.shape)}")
    return t[:, :, 0] if t.dim() == 3 and t.shape[2] == 1 else t


def stage(image, mask_gt=False, mask=None, device="cuda", name=None):
    """Uploads `image` (and `mask`) once and applies what process_input_image does in front of the resize: an RGBA image is
    split, its alpha is the mask unless one is given, and with `mask_gt` the image is multiplied by the mask.  -> Staged.
    `name`: the file, for the error messages.  A mask that is zero everywhere (the reference divides by zero) is refused
    with a ValueError when it comes from the host; one already on the device is not looked at: its outputs are zeros."""
    device = torch.device(device)
    img = _pixels(image, "image", name)
    alpha = None if mask is None else _pixels(mask, "mask", name)
    if alpha is not None and alpha.dim() != 2:
        raise ValueError(f"gs2m_ingest: the mask{' of ' + name if name else ''} must have one channel, got {tuple(alpha.shape)}")
    if alpha is not None and tuple(alpha.shape) != tuple(img.shape[:2]):
        raise ValueError(f"gs2m_ingest: the mask{' of ' + name if name else ''} is {tuple(alpha.shape)}, its image {tuple(img.shape[:2])}")
    host_alpha = alpha if alpha is not None else (img[:, :, 3] if img.dim() == 3 and img.shape[2] == 4 else None)
    if host_alpha is not None and not host_alpha.is_cuda and int(host_alpha.max()) == 0:
        raise ValueError(f"gs2m_ingest: the mask{' of ' + name if name else ''} is zero everywhere")
    img = img.to(device)
    alpha = None if alpha is None else alpha.to(device)
    if img.dim() == 3 and img.shape[2] == 4:  # RGBA: one upload, split on the device
        alpha = img[:, :, 3].contiguous() if alpha is None else alpha
        img = img[:, :, :3].contiguous()
    if mask_gt and alpha is not None:
        if img.dim() != 3:
            raise ValueError(f"gs2m_ingest: mask_gt needs an RGB image{', ' + name + ' has one channel' if name else ''}")
        img = mask_image(img, alpha)
    return Staged(img, alpha)


def process_input_image(image, resolution, mask_gt=False, mask=None, device="cuda", gray=False, name=None):
    """utils/image_utils.py:48-77 on the device.  `image`, `mask`: PIL images, uint8 arrays or uint8 tensors ((H, W), (H, W, 3),
    (H, W, 4); the mask (H, W)), or `image` a `Staged`; resolution = (w, h).
    -> (rgb (C, h, w), alpha (1, h, w) or None[, gray (1, h, w)]) float32 on the device: the reference's shapes and values."""
    st = image if isinstance(image, Staged) else stage(image, mask_gt, mask, device, name)
    small = resize(st.image, resolution)
    small_alpha = None if st.alpha is None else resize(st.alpha, resolution)
    out = unpack(small, small_alpha, gray=gray)
    return out if gray else out[:2]


def gray_image(image, resolution, mask_gt=False, mask=None, device="cuda", name=None):
    """scene/__init__.py:193-204 for one camera: the image masked and resized to `resolution` = (w, h), then its luma.
    -> (1, h, w) float32 on the device."""
    st = image if isinstance(image, Staged) else stage(image, mask_gt, mask, device, name)
    return unpack(resize(st.image, resolution), rgb=False, gray=True)[2]
