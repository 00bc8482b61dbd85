"""A restatement of the reference's LPIPS (VGG16, v0.1) in torch on the CPU, float64 by default, written from its description:

    metrics.py:33,57                        the input: the first three channels of the 8-bit image, value / 255, NOT mapped to [-1, 1]
    lpipsPyTorch/modules/networks.py:41-51  z_score: (x - mean) / std
    lpipsPyTorch/modules/networks.py:53-63  the features one module after the other, normalised taps after modules 4, 9, 16, 23, 30
    lpipsPyTorch/modules/networks.py:88-94  vgg16().features, the tap list and its channel counts
    lpipsPyTorch/modules/utils.py:6-8       normalize_activation: x / (sqrt(sum_c x^2) + 1e-10)
    lpipsPyTorch/modules/lpips.py:30-36     (fx - fy)^2, the 1x1 `lin` convolution, the spatial mean, the sum over the taps

`dtype=torch.float32` runs the same expressions in float32 (what the reference itself computes).  The pretrained weights cannot
be a fixture (59 MB): `make_weights(seed)` builds a seeded set for the tests and the golden generator alike."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
CONV_COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
POOL_AFTER_CONV = (1, 3, 6, 9)       # features 4, 9, 16, 23; the fifth pool (30) is never run
TAP_AFTER_CONV = (1, 3, 6, 9, 12)    # the ReLU outputs of features 3, 8, 15, 22, 29
TAP_CHANNELS = (64, 128, 256, 512, 512)
MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)


def make_conv(cin, cout, rng):
    """He-scaled normal weights (std = sqrt(2 / (9 cin))), small biases of both signs: float32 OIHW and (cout,)"""
    w = rng.normal(0.0, np.sqrt(2.0 / (9 * cin)), (cout, cin, 3, 3)).astype(np.float32)
    b = rng.normal(0.0, 0.05, cout).astype(np.float32)
    return w, b


@functools.lru_cache(maxsize=2)
def make_weights(seed=0):
    """{"conv_w": 13 x OIHW, "conv_b": 13 x (Cout,), "lin": 5 x (C,)} float32 numpy arrays from default_rng(seed); the lin
    vectors are non-negative, as the trained ones are.  Cached: callers must not write into the arrays."""
    rng = np.random.default_rng(seed)
    conv = [make_conv(ci, co, rng) for ci, co in zip(CONV_CIN, CONV_COUT)]
    lin = [np.abs(rng.normal(0.0, 0.5 / np.sqrt(c), c)).astype(np.float32) for c in TAP_CHANNELS]
    return {"conv_w": [w for w, _ in conv], "conv_b": [b for _, b in conv], "lin": lin}


def state_dicts(weights, full_model_keys=True, original_lin_keys=True):
    """the two state dicts the reference loads, from `make_weights`' arrays: (vgg, lin)"""
    pre = "features." if full_model_keys else ""
    vgg = {}
    for idx, w, b in zip(CONV_INDEX, weights["conv_w"], weights["conv_b"]):
        vgg[f"{pre}{idx}.weight"], vgg[f"{pre}{idx}.bias"] = torch.from_numpy(w), torch.from_numpy(b)
    lin = {(f"lin{k}.model.1.weight" if original_lin_keys else f"{k}.1.weight"): torch.from_numpy(v).reshape(1, -1, 1, 1)
           for k, v in enumerate(weights["lin"])}
    return vgg, lin


def to_input(img_u8, dtype=torch.float64):
    """(H, W, 3+) uint8 -> (1, 3, H, W): value / 255 formed in float32 as to_tensor does (metrics.py:33), then `dtype`"""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(img_u8)[:, :, :3])).permute(2, 0, 1).contiguous().float().div(255)
    return t.unsqueeze(0).to(dtype)


def conv_relu(x, w, b, dtype=torch.float64):
    """relu(conv3x3(x) + bias): x (N, Cin, H, W), stride 1, zero padding 1"""
    return F.relu(F.conv2d(x.to(dtype), torch.as_tensor(w).to(dtype), torch.as_tensor(b).to(dtype), stride=1, padding=1))


def conv_magnitude(x, w, b):
    """sum |a| |w| + |bias| per output element in float64: what the forward error of an fp32 product chain is relative to"""
    return F.conv2d(torch.as_tensor(x).double().abs(), torch.as_tensor(w).double().abs(), torch.as_tensor(b).double().abs(),
                    stride=1, padding=1)


def features(x, weights, dtype=torch.float64):
    """the five tap tensors (before normalisation) of x (N, 3, H, W) in [0, 1]"""
    mean = torch.tensor(MEAN, dtype=torch.float32).to(dtype)[None, :, None, None]  # torch.Tensor([...]) is float32
    std = torch.tensor(STD, dtype=torch.float32).to(dtype)[None, :, None, None]
    x = (x.to(dtype) - mean) / std
    taps = []
    for l in range(13):
        x = conv_relu(x, weights["conv_w"][l], weights["conv_b"][l], dtype)
        if l in TAP_AFTER_CONV:
            taps.append(x)
        if l in POOL_AFTER_CONV:
            x = F.max_pool2d(x, kernel_size=2, stride=2)  # floor sizing: ceil_mode=False
    return taps


def normalize(x, eps=1e-10):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


def tap_distance(fx, fy, lin, dtype=torch.float64):
    """steps 4-5 for one tap: fx, fy (N, C, H, W) features, lin (C,) -> (N,) spatial means"""
    fx, fy, lin = torch.as_tensor(fx).to(dtype), torch.as_tensor(fy).to(dtype), torch.as_tensor(lin).to(dtype)
    d = (normalize(fx) - normalize(fy)) ** 2
    return F.conv2d(d, lin.reshape(1, -1, 1, 1)).mean((2, 3)).reshape(-1)


def lpips(a_u8, b_u8, weights, dtype=torch.float64):
    """(H, W, 3) uint8 x 2 -> (layers, total): the five per-tap values (numpy, `dtype`) and their sum"""
    with torch.no_grad():
        fa, fb = features(to_input(a_u8, dtype), weights, dtype), features(to_input(b_u8, dtype), weights, dtype)
        layers = torch.stack([tap_distance(x, y, l, dtype)[0] for x, y, l in zip(fa, fb, weights["lin"])])
        return layers.numpy(), layers.sum().item()


def cases():
    """the golden cases: {name: (a, b)} uint8 (H, W, 3)"""
    import metrics_ref as MR
    out = {}
    out["rgb_16x16"] = MR.gradient_noise_pair(16, 16, 3, seed=11)      # one pixel at the last tap
    out["rgb_35x29"] = MR.gradient_noise_pair(35, 29, 3, seed=12)      # odd at every pool: 17x14, 8x7, 4x3, 2x1
    out["rgb_33x70"] = MR.gradient_noise_pair(33, 70, 3, seed=13)      # a tile remainder in both directions
    out["rgb_64x48"] = MR.gradient_noise_pair(64, 48, 3, seed=14)
    a, _ = MR.gradient_noise_pair(24, 20, 3, seed=15)
    out["identical_24x20"] = (a, a.copy())                             # exactly 0
    out["black_white_16x18"] = (np.zeros((16, 18, 3), np.uint8), np.full((16, 18, 3), 255, np.uint8))
    a, _ = MR.gradient_noise_pair(40, 33, 3, seed=16)
    b = a.copy()
    b[0, 0, 1] ^= 0x80                                                 # one byte, at a corner
    out["one_byte_40x33"] = (a, b)
    return out


GOLDEN_SEED = 2024  # the weight set the golden was recorded with
