"""Generates tests/golden/metrics.npz: the REFERENCE's own utils.loss_utils.ssim and utils.image_utils.psnr on a few small
8-bit image pairs, on the CPU in fp32 -- the values metrics.py:55-56 would score them with.  Run by hand where a checkout of the
reference exists:

    python tests/golden/make_metrics_golden.py <reference checkout>

What the image lacks is stood in for HERE, in the generator only: utils/loss_utils.py imports `cv2` and the reference's
`gaussian_renderer` at module level and uses neither in `ssim`; empty modules of those names are put in their place for the
import when the real ones cannot be imported.  torchvision's `to_tensor` (metrics.py:33) is restated as what it does to an
8-bit image: (H, W, CH) -> (CH, H, W), float32, .div(255).  The npz holds every pair and the two float32 values."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def cases():
    import metrics_ref as MR
    out = {}
    out["rgb_24x37"] = MR.gradient_noise_pair(24, 37, 3, seed=1)
    out["grey_13x9"] = MR.gradient_noise_pair(13, 9, 1, seed=2)
    out["rgb_5x70"] = MR.gradient_noise_pair(5, 70, 3, seed=3)       # shorter than the window
    a, _ = MR.gradient_noise_pair(16, 16, 3, seed=4)
    out["identical_16x16"] = (a, a.copy())                           # psnr = inf
    out["black_white_12x12"] = (np.zeros((12, 12, 3), np.uint8), np.full((12, 12, 3), 255, np.uint8))
    a, _ = MR.gradient_noise_pair(40, 33, 3, seed=5)
    b = a.copy()
    b[0, 0, 1] ^= 0x80                                               # one byte, at a corner
    out["one_byte_40x33"] = (a, b)
    return out


def reference_functions(ref_root):
    stood_in = []
    for name in ("cv2", "gaussian_renderer"):
        try:
            if name == "gaussian_renderer":
                raise ImportError  # the reference's own pulls in its CUDA extensions; `ssim` does not use it
            importlib.import_module(name)
        except ImportError:
            m = types.ModuleType(name)
            m.render = None
            sys.modules[name] = m
            stood_in.append(name)
    sys.path.insert(0, ref_root)
    try:
        for k in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
            del sys.modules[k]
        ssim = importlib.import_module("utils.loss_utils").ssim
        psnr = importlib.import_module("utils.image_utils").psnr
    finally:
        sys.path.remove(ref_root)
        for name in stood_in:
            del sys.modules[name]
    return ssim, psnr


def to_tensor(img):
    return torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).contiguous().float().div(255).unsqueeze(0)


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "utils", "loss_utils.py")):
        sys.exit("usage: make_metrics_golden.py <reference checkout>")
    ssim, psnr = reference_functions(os.path.abspath(sys.argv[1]))
    out = {}
    for name, (a, b) in cases().items():
        ta, tb = to_tensor(a), to_tensor(b)
        with torch.no_grad():
            s, p = ssim(ta, tb), psnr(ta, tb)
        assert s.dtype == torch.float32 and p.dtype == torch.float32 and p.numel() == 1
        out[f"{name}/a"], out[f"{name}/b"] = a, b
        out[f"{name}/ssim"], out[f"{name}/psnr"] = np.float32(s.item()), np.float32(p.item())
        print(f"{name}: {a.shape} ssim {s.item():.9f} psnr {p.item():.6f}")
    path = os.path.join(HERE, "metrics.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
