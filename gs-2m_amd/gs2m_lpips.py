"""LPIPS (VGG16, v0.1) of rendered views on the GPU: metrics.py:57's `lpips(render, gt, net_type='vgg')` (include/gs2m_lpips.h,
csrc/lpips.hip).

The WEIGHTS are the user's: `load_weights` reads the two files the reference downloads -- torchvision's `vgg16` state dict and the
LPIPS v0.1 `vgg.pth` linear layers -- from paths the user passes.  Nothing here fetches anything, and torchvision is not
imported.  The thirteen convolutions run on the fp32 matrix instructions in hand-written HIP; no framework convolution is called.

There is NO CPU fallback: `lpips` refuses CPU tensors.  `read_weights` (the file and key checks) is host-only."""
import ctypes as C
import os

import torch

import gs2m_native as N

CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)  # the Conv2d modules of vgg16().features[:30]
CONV_CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
CONV_COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
TAP_CHANNELS = (64, 128, 256, 512, 512)  # networks.py:93-94
MIN_SIZE = 16     # GS2M_LPIPS_MIN_SIZE: four floor-sized pools must leave a pixel
PACKED_FLOATS = sum(9 * ci * co + co for ci, co in zip(CONV_CIN, CONV_COUT)) + sum(TAP_CHANNELS)  # GS2M_LPIPS_PACKED_FLOATS


class Weights:
    """One weight set in the layout the kernels read: `packed`, a float32 device tensor of PACKED_FLOATS elements."""

    def __init__(self, packed):
        self.packed = packed
        self.device = packed.device


def _load(path, flag):
    if not os.path.isfile(path):
        raise FileNotFoundError(f"gs2m_lpips: {flag} {path} does not exist; pass the file the reference uses, nothing is downloaded")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"gs2m_lpips: {flag} {path} holds a {type(sd).__name__}, not a state dict")
    return sd


def _take(sd, keys, shape, path):
    """the tensor under the first of `keys` that `sd` has, checked: float32 of `shape`"""
    for key in keys:
        if key in sd:
            t = sd[key]
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise ValueError(f"gs2m_lpips: {path}: `{key}` must be a float32 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"gs2m_lpips: {path}: `{key}` must have shape {tuple(shape)}, got {tuple(t.shape)}")
            return t.detach().contiguous()
    raise KeyError(f"gs2m_lpips: {path} has no `{keys[0]}`" + (f" (nor `{'`, `'.join(keys[1:])}`)" if len(keys) > 1 else ""))


def read_weights(vgg_path, lin_path):
    """-> (conv_w, conv_b, lin): host float32 tensors, 13 OIHW weights, 13 biases, 5 lin vectors of shape (C,).
    `vgg_path`: torchvision's vgg16 state dict (`features.N.weight` / `.bias`; classifier keys are ignored) or a bare `features`
    state dict (`N.weight`).  `lin_path`: the LPIPS keys `lin{k}.model.1.weight` of shape (1, C, 1, 1), or as
    lpipsPyTorch/modules/utils.py:22-28 renames them (`{k}.1.weight`).  Every shape and dtype is checked; the error names the key."""
    vgg, lin_sd = _load(vgg_path, "--lpips-vgg"), _load(lin_path, "--lpips-lin")
    conv_w, conv_b = [], []
    for idx, ci, co in zip(CONV_INDEX, CONV_CIN, CONV_COUT):
        conv_w.append(_take(vgg, (f"features.{idx}.weight", f"{idx}.weight"), (co, ci, 3, 3), vgg_path))
        conv_b.append(_take(vgg, (f"features.{idx}.bias", f"{idx}.bias"), (co,), vgg_path))
    lin = [_take(lin_sd, (f"lin{k}.model.1.weight", f"{k}.1.weight"), (1, c, 1, 1), lin_path).reshape(c)
           for k, c in enumerate(TAP_CHANNELS)]
    return conv_w, conv_b, lin


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def pack_weights(conv_w, conv_b, lin, device="cuda"):
    """13 OIHW weights, 13 biases and 5 lin vectors (float32 tensors anywhere) -> Weights on `device`; once per weight set."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("gs2m_lpips: the weights are packed on a HIP device; there is no CPU path")
    up = [[t.to(device=device, dtype=torch.float32).contiguous() for t in ts] for ts in (conv_w, conv_b, lin)]
    for l, (ci, co) in enumerate(zip(CONV_CIN, CONV_COUT)):
        if tuple(up[0][l].shape) != (co, ci, 3, 3) or tuple(up[1][l].shape) != (co,):
            raise ValueError(f"gs2m_lpips: convolution {l} must be ({co}, {ci}, 3, 3) with bias ({co},)")
    for k, c in enumerate(TAP_CHANNELS):
        if up[2][k].numel() != c:
            raise ValueError(f"gs2m_lpips: lin vector {k} must have {c} elements")
    packed = torch.empty(PACKED_FLOATS, dtype=torch.float32, device=device)
    N.launch("gs2m_lpips_pack_weights", device, _ptr_array(up[0]), _ptr_array(up[1]), _ptr_array(up[2]), packed.data_ptr())
    torch.cuda.current_stream(device).synchronize()  # `up` may go once the kernels have read it
    return Weights(packed)


def load_weights(vgg_path, lin_path, device="cuda"):
    """The two files of the reference's LPIPS (see `read_weights`) -> Weights on `device`.  Nothing is downloaded: a missing
    file is a FileNotFoundError naming its flag."""
    return pack_weights(*read_weights(vgg_path, lin_path), device=device)


def _u8(t, name, who):
    """gs2m_metrics' refusals in its order, with CH = 3 and the smallest size the five taps allow"""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{who}: `{name}` must be a CUDA tensor on a HIP device; there is no CPU path")
    if t.dtype != torch.uint8:
        raise RuntimeError(f"{who}: `{name}` must be uint8, got {t.dtype}")
    if t.dim() != 4 or t.shape[3] != 3:
        raise RuntimeError(f"{who}: `{name}` must have shape (N, H, W, CH) with CH 3, got {tuple(t.shape)}")
    if t.shape[1] < MIN_SIZE or t.shape[2] < MIN_SIZE:
        raise RuntimeError(f"{who}: `{name}` must be at least {MIN_SIZE} x {MIN_SIZE} pixels (the last tap would be empty), got "
                           f"{t.shape[1]} x {t.shape[2]}")
    if not t.is_contiguous():
        raise RuntimeError(f"{who}: `{name}` must be contiguous (N, H, W, CH), got strides {t.stride()}")
    if not t.is_cuda:
        raise RuntimeError(f"{who}: `{name}` must be a CUDA tensor on a HIP device; there is no CPU path")
    return t


def lpips_device(a, b, weights):
    """uint8 device tensors (N, H, W, 3) -> (total, layers): float64 DEVICE tensors (N,) and (N, 5).  The pairs are taken one
    after the other with one pair's workspace (two buffers of 2 H W 64 floats)."""
    who = "lpips"
    a, b = _u8(a, "a", who), _u8(b, "b", who)
    if a.shape != b.shape or a.device != b.device:
        raise RuntimeError(f"{who}: `a` {tuple(a.shape)} on {a.device} and `b` {tuple(b.shape)} on {b.device} must match")
    if not isinstance(weights, Weights) or weights.device != a.device:
        raise RuntimeError(f"{who}: `weights` must come from load_weights on {a.device}")
    n, h, w, _ = a.shape
    dev = a.device
    total = torch.empty(n, dtype=torch.float64, device=dev)
    layers = torch.empty((n, 5), dtype=torch.float64, device=dev)
    if n == 0:
        return total, layers
    nbytes = C.c_longlong()
    N.check(N.lib().gs2m_lpips_workspace_bytes(n, h, w, C.byref(nbytes)), "gs2m_lpips_workspace_bytes")
    ws = torch.empty((nbytes.value + 15) // 16 * 4, dtype=torch.float32, device=dev)
    N.launch("gs2m_lpips", dev, n, h, w, a.data_ptr(), b.data_ptr(), weights.packed.data_ptr(), ws.data_ptr(), ws.numel() * 4,
             total.data_ptr(), layers.data_ptr())
    return total, layers


def lpips(a, b, weights):
    """uint8 device tensors (N, H, W, 3) -> float64 host tensor (N,): metrics.py:57's value of every pair."""
    return lpips_device(a, b, weights)[0].cpu()


def lpips_layers(a, b, weights):
    """-> float64 host tensor (N, 5): the five per-tap means whose sum `lpips` is."""
    return lpips_device(a, b, weights)[1].cpu()


# ---- the kernels one by one (what gs2m_lpips launches, on caller tensors) ------------------------------------------------------

def pack_conv(w_oihw, bias):
    """OIHW weight (Cout, Cin, 3, 3) and bias (Cout,) on the device -> the packed float32 tensor `conv3x3` reads."""
    who = "lpips.pack_conv"
    co, ci = w_oihw.shape[:2]
    w_oihw, bias = N.f32(w_oihw, "w_oihw", (co, ci, 3, 3), who=who), N.f32(bias, "bias", (co,), who=who)
    packed = torch.empty(9 * ci * co + co, dtype=torch.float32, device=w_oihw.device)
    N.launch("gs2m_lpips_pack_conv", w_oihw.device, ci, co, w_oihw.data_ptr(), bias.data_ptr(), packed.data_ptr())
    return packed


def conv3x3(x, packed, cout):
    """x (N, H, W, Cin) float32 on the device, `packed` from pack_conv -> relu(conv3x3(x) + bias), (N, H, W, cout)."""
    who = "lpips.conv3x3"
    x = N.f32(x, "x", who=who)
    n, h, w, ci = x.shape
    packed = N.f32(packed, "packed", (9 * ci * cout + cout,), who=who)
    out = torch.empty((n, h, w, cout), dtype=torch.float32, device=x.device)
    N.launch("gs2m_lpips_conv3x3", x.device, n, h, w, ci, cout, x.data_ptr(), packed.data_ptr(), out.data_ptr())
    return out


def maxpool2x2(x):
    """x (N, H, W, C) float32 on the device -> (N, H // 2, W // 2, C): 2x2 / stride 2 maximum, an odd last row or column dropped."""
    x = N.f32(x, "x", who="lpips.maxpool2x2")
    n, h, w, c = x.shape
    out = torch.empty((n, h // 2, w // 2, c), dtype=torch.float32, device=x.device)
    N.launch("gs2m_lpips_maxpool2x2", x.device, n, h, w, c, x.data_ptr(), out.data_ptr())
    return out


def tap_distance(fx, fy, lin):
    """fx, fy (N, H, W, C) float32 feature maps on the device, lin (C,) -> float64 host tensor (N,): steps 4-5 of one tap."""
    who = "lpips.tap_distance"
    fx = N.f32(fx, "fx", who=who)
    n, h, w, c = fx.shape
    fy, lin = N.f32(fy, "fy", (n, h, w, c), who=who), N.f32(lin, "lin", (c,), who=who)
    nbytes = C.c_longlong()
    N.check(N.lib().gs2m_lpips_tap_workspace_bytes(n, h, w, C.byref(nbytes)), "gs2m_lpips_tap_workspace_bytes")
    ws = torch.empty((nbytes.value + 7) // 8, dtype=torch.float64, device=fx.device)
    out = torch.empty(n, dtype=torch.float64, device=fx.device)
    N.launch("gs2m_lpips_tap_distance", fx.device, n, h, w, c, fx.data_ptr(), fy.data_ptr(), lin.data_ptr(), ws.data_ptr(),
             ws.numel() * 8, out.data_ptr())
    return out.cpu()
