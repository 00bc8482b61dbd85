"""Generates tests/golden/ref_ingest.npz.  Run in the BUILD container only:

    python tests/golden/make_ingest_golden.py

Small seeded images and what the reference's own `process_input_image` (utils/image_utils.py) and `loadCam`
(utils/camera_utils.py) make of them, imported from /root/reference and run on the CPU (they cannot travel to the GPU box, the
vectors can).  Data only: no reference text is copied.  tests/test_ingest.py holds the numpy restatement tests/ingest_ref.py to
these bits, tests/test_ingest_gpu.py the kernels of csrc/ingest.hip.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
# (w, h, -r): 1 / 2 / 4 / 8 round, -1 caps the width at 1600, anything else is a width; odd sizes so that round and int differ
SIZES = ((1554, 1162, 2), (1554, 1162, 1), (1920, 1080, 4), (1959, 1091, 2), (1959, 1091, 8), (101, 77, 2), (1601, 1067, -1), (3001, 2003, -1),
         (1600, 1200, -1), (1555, 1163, -1), (1554, 1162, 777), (1959, 1091, 3), (1959, 1091, 500), (101, 77, 6))


def inputs():
    rng = np.random.default_rng(20240611)
    W, H = 101, 77
    y, x = np.mgrid[0:H, 0:W]
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rgb[10:30, 20:60] = (rgb[10:30, 20:60] // 8) * 8 + np.array([255, 0, 128], np.uint8) // 32  # a flatter patch
    # the mask: a soft-edged disc (values between 0 and 255 at the rim) that never reaches 255 -- max(alpha) = 250 is part of the
    # result -- plus binary specks, whose resize overshoots on both sides
    disc = np.clip(1.2 * (30.0 - np.hypot(x - 52.0, y - 36.0)) / 6.0, 0.0, 1.0)
    mask = (disc * 250.0).astype(np.uint8)
    specks = rng.random((H, W)) < 0.03
    mask[specks & (disc == 0.0)] = 250
    mask[specks & (disc == 1.0)] = 0
    alpha = ((rng.random((H, W)) < 0.6) * 255).astype(np.uint8)  # the RGBA image's own channel: binary
    gray = rng.integers(0, 256, (17, 31), dtype=np.uint8)
    return rgb, mask, alpha, gray


def main():
    sys.path.insert(0, "/root/reference")
    from PIL import Image
    import PIL
    from utils.image_utils import process_input_image

    # loadCam only: its module imports the scene package (the model, the rasterizer); a stand-in Camera returns what loadCam
    # hands it
    scene, cameras = types.ModuleType("scene"), types.ModuleType("scene.cameras")
    cameras.Camera = lambda **kw: kw
    scene.cameras = cameras
    sys.modules.setdefault("scene", scene)
    sys.modules.setdefault("scene.cameras", cameras)
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules["tqdm"] = types.SimpleNamespace(tqdm=None)
    from utils.camera_utils import loadCam

    rgb, mask, alpha, gray = inputs()
    out = {"rgb": rgb, "mask": mask, "alpha": alpha, "gray_in": gray,
           "versions": np.array([np.__version__, PIL.__version__, torch.__version__])}

    def run(name, image, resolution, mask_gt, pil_mask):
        img, a = process_input_image(image, resolution, mask_gt, pil_mask)
        out[name + "_rgb"] = img.numpy()
        assert img.dtype == torch.float32
        if a is not None:
            out[name + "_alpha"] = a.numpy()
        if img.shape[0] >= 3:  # scene/__init__.py:203 on the result
            c = img[:3]
            out[name + "_gray"] = (c[0:1, ...] * 0.299 + c[1:2, ...] * 0.587 + c[2:3, ...] * 0.114).numpy()

    for mask_gt in (False, True):
        tag = "_maskgt" if mask_gt else ""
        run("rgb_mask" + tag, Image.fromarray(rgb), (50, 38), mask_gt, Image.fromarray(mask))
        run("rgba" + tag, Image.fromarray(np.dstack([rgb, alpha]), "RGBA"), (50, 38), mask_gt, None)
        run("rgba_mask" + tag, Image.fromarray(np.dstack([rgb, alpha]), "RGBA"), (50, 38), mask_gt, Image.fromarray(mask))
    run("rgb_nomask", Image.fromarray(rgb), (50, 38), True, None)
    run("l", Image.fromarray(gray), (40, 29), False, None)

    sizes = []
    for w, h, r in SIZES:
        info = types.SimpleNamespace(Fx=1000.0, Fy=1000.0, width=w, height=h, image=types.SimpleNamespace(size=(w, h)), uid=0, R=None, T=None,
                                     image_name="x", mask=None, depth=None)
        args = types.SimpleNamespace(resolution=r, mask_gt=False, data_device="cpu")
        res = loadCam(args, info, 1.0)["resolution"]
        sizes.append((w, h, r, res[0], res[1]))
    out["sizes"] = np.array(sizes, np.int64)
    path = os.path.join(HERE, "ref_ingest.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")
    for row in sizes:
        print(row)


if __name__ == "__main__":
    main()
