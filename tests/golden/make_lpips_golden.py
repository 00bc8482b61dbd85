"""Generates tests/golden/ref_lpips.npz: the REFERENCE's own lpipsPyTorch code -- BaseNet.forward (z_score, the feature walk,
normalize_activation), LinLayers and LPIPS.forward -- in fp32 on the CPU, on a few small 8-bit pairs, with the SEEDED weight set
of tests/lpips_ref.make_weights (the pretrained 59 MB are no fixture).  Run by hand where a checkout of the reference exists:

    python tests/golden/make_lpips_golden.py <reference checkout>

Nothing here touches the network: LPIPS(...), VGG16(), get_state_dict and the package-level lpips() -- each of which downloads --
are NEVER called.  The network is a subclass of the reference's BaseNet whose `layers` is an nn.Sequential of the VGG16
configuration filled with the seeded weights; LPIPS.forward is bound to an object built without LPIPS.__init__.  torchvision,
which networks.py imports at module level for the constructors that are not called, is stood in for by an empty module when it
cannot be imported.  metrics.py:33's `to_tensor` is restated as in make_metrics_golden.py.  The npz holds every pair, the
recorded float32 total and the five float32 per-tap means."""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")


def reference_modules(ref_root):
    stood_in = []
    try:
        importlib.import_module("torchvision")
    except ImportError:
        m = types.ModuleType("torchvision")
        m.models = types.ModuleType("torchvision.models")
        sys.modules["torchvision"], sys.modules["torchvision.models"] = m, m.models
        stood_in += ["torchvision", "torchvision.models"]
    sys.path.insert(0, ref_root)
    try:
        networks = importlib.import_module("lpipsPyTorch.modules.networks")
        lpips_mod = importlib.import_module("lpipsPyTorch.modules.lpips")
    finally:
        sys.path.remove(ref_root)
        for name in stood_in:
            del sys.modules[name]
    return networks, lpips_mod


def build_criterion(networks, lpips_mod, weights):
    layers, cin, k = [], 3, 0
    for v in VGG16_CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            continue
        conv = nn.Conv2d(cin, v, kernel_size=3, padding=1)
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(weights["conv_w"][k]))
            conv.bias.copy_(torch.from_numpy(weights["conv_b"][k]))
        layers += [conv, nn.ReLU(inplace=True)]
        cin, k = v, k + 1

    class SeededVGG16(networks.BaseNet):
        def __init__(self):
            super().__init__()
            self.layers = nn.Sequential(*layers)
            self.target_layers = [4, 9, 16, 23, 30]
            self.n_channels_list = [64, 128, 256, 512, 512]
            self.set_requires_grad(False)

    crit = lpips_mod.LPIPS.__new__(lpips_mod.LPIPS)  # NOT LPIPS(...): its __init__ downloads
    nn.Module.__init__(crit)
    crit.net = SeededVGG16()
    crit.lin = networks.LinLayers(crit.net.n_channels_list)
    with torch.no_grad():
        for seq, v in zip(crit.lin, weights["lin"]):
            seq[1].weight.copy_(torch.from_numpy(v).reshape(1, -1, 1, 1))
    return crit.eval()


def to_tensor(img):
    return torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).contiguous().float().div(255).unsqueeze(0)


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "lpipsPyTorch", "modules", "lpips.py")):
        sys.exit("usage: make_lpips_golden.py <reference checkout>")
    import lpips_ref as LR
    networks, lpips_mod = reference_modules(os.path.abspath(sys.argv[1]))
    crit = build_criterion(networks, lpips_mod, LR.make_weights(LR.GOLDEN_SEED))
    out = {"seed": np.int64(LR.GOLDEN_SEED)}
    for name, (a, b) in LR.cases().items():
        ta, tb = to_tensor(a), to_tensor(b)
        with torch.no_grad():
            total = crit(ta, tb)  # LPIPS.forward
            fx, fy = crit.net(ta), crit.net(tb)  # BaseNet.forward: the normalised taps
            layers = torch.stack([lin((x - y) ** 2).mean() for x, y, lin in zip(fx, fy, crit.lin)])
        assert total.dtype == torch.float32 and total.numel() == 1 and layers.dtype == torch.float32
        out[f"{name}/a"], out[f"{name}/b"] = a, b
        out[f"{name}/lpips"], out[f"{name}/layers"] = np.float32(total.item()), layers.numpy()
        print(f"{name}: {a.shape} lpips {total.item():.9f} layers {layers.numpy()}")
    path = os.path.join(HERE, "ref_lpips.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
