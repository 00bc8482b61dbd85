"""Generates tests/golden/ref_view_maps.npz.  Run in the BUILD container only:

    python tests/golden/make_view_maps_golden.py

Small inputs and what the reference's own host helpers make of them -- utils/image_utils.py `save_depth_map` (the PNG it
writes, decoded), `convert_normal_for_save` and `map_to_rgba`, imported from /root/reference and run on the CPU (they cannot
travel to the GPU box, the vectors can) -- plus matplotlib's 8-bit magma table.  Data only: no reference text is copied.
tests/test_view_maps.py holds the numpy restatement tests/view_maps_ref.py to these bytes, tests/test_view_maps_gpu.py the
kernels of csrc/view_maps.hip.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = ((37, 53), (48, 64))


def depth_map(h, w, seed):
    """a tilted plane with a bump and sensor noise, 2 .. 6: every pixel distinct, the percentiles fall between samples"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    d = 3.0 + 1.5 * x / w + 0.8 * y / h + 0.7 * np.exp(-((x - 0.4 * w) ** 2 + (y - 0.6 * h) ** 2) / (0.02 * w * w + 8.0))
    return (d + 0.05 * rng.standard_normal((h, w))).astype(np.float32)


def view_rotation(seed):
    """world_view_transform of a camera: R^T in the upper 3x3 (row-vector convention), the translation in the last row"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = q.astype(np.float32)
    m[3, :3] = rng.standard_normal(3).astype(np.float32)
    return m


def main():
    sys.path.insert(0, "/root/reference")
    import matplotlib
    import matplotlib.pyplot as plt
    from PIL import Image
    from utils.image_utils import convert_normal_for_save, map_to_rgba, save_depth_map
    out = {"magma_table": (plt.cm.magma(np.arange(256))[:, :3] * 255).astype(np.uint8),
           "versions": np.array([np.__version__, matplotlib.__version__, torch.__version__])}
    tmp = tempfile.mkdtemp()

    def depth_case(name, d):
        path = os.path.join(tmp, name + ".png")
        save_depth_map(d.copy(), path)
        with Image.open(path) as img:
            assert img.mode == "RGBA", img.mode
            out[f"depth_{name}"], out[f"depth_{name}_png"] = d, np.asarray(img).copy()

    for k, (h, w) in enumerate(SIZES):
        tag = f"{h}x{w}"
        d = depth_map(h, w, 10 + k)
        depth_case(tag, d)
        half = d.copy()
        half[:, : w // 2] = 0.0  # masked depth: half the map is background
        depth_case(f"half_{tag}", half)
        depth_case(f"const_{tag}", np.full((h, w), 2.5, np.float32))

        rng = np.random.default_rng(20 + k)
        n = rng.standard_normal((3, h, w)).astype(np.float32) * rng.uniform(0.01, 3.0, (1, h, w)).astype(np.float32)
        n[:, 0, :5] = 0.0  # background pixels: the zero vector stays zero
        n[:, 1, 0] = (0.0, 0.0, -2.0)
        n[:, 1, 1] = (1e-20, 0.0, 0.0)  # below the 1e-12 floor of F.normalize
        wvt = view_rotation(30 + k)
        view = types.SimpleNamespace(world_view_transform=torch.from_numpy(wvt), image_height=h, image_width=w)
        out[f"normal_{tag}"], out[f"wvt_{tag}"] = n, wvt
        out[f"normal_{tag}_view"] = convert_normal_for_save(torch.from_numpy(n), view, False).contiguous().numpy()
        out[f"normal_{tag}_world"] = convert_normal_for_save(torch.from_numpy(n), view, True).contiguous().numpy()

        m3 = rng.random((3, h, w)).astype(np.float32)
        m3[:, 0, 0], m3[:, 0, 1], m3[:, 0, 2] = 0.0, 1.0, 0.5
        m3[0, 2, :] = (np.arange(w) % 256).astype(np.float32) / np.float32(255.0)  # k / 255: the truncation's boundaries
        m1 = rng.random((1, h, w)).astype(np.float32)
        alpha = (rng.random((1, h, w)) > 0.4).astype(np.float32) * rng.random((1, h, w)).astype(np.float32)
        alpha[0, 0, :3] = (0.0, 1.0, 0.5)
        out[f"map3_{tag}"], out[f"map1_{tag}"], out[f"alpha_{tag}"] = m3, m1, alpha
        out[f"map3_{tag}_rgba"] = np.asarray(map_to_rgba(torch.from_numpy(m3), torch.from_numpy(alpha))).copy()
        out[f"map1_{tag}_rgba"] = np.asarray(map_to_rgba(torch.from_numpy(m1), torch.from_numpy(alpha))).copy()
        # the normal image of a white-background run: map_to_rgba of convert_normal_for_save
        out[f"normal_{tag}_view_rgba"] = np.asarray(map_to_rgba(torch.from_numpy(out[f"normal_{tag}_view"]), torch.from_numpy(alpha))).copy()
    depth_case("1x1", np.full((1, 1), 1.25, np.float32))
    path = os.path.join(HERE, "ref_view_maps.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
