"""Generates tests/golden/ref_mv_geo.npz: the geometric chain of multi_view_loss (utils/loss_utils.py:256-276) run from the
REFERENCE's own functions -- _get_points_from_depth, _sample_depth_normal, _reproject_points, _sample_normal_map, composed as
those lines compose them -- on one small scene with unequal views (reference 23 x 17, neighbour 19 x 13, different focal
lengths, off-centre principal point, a real relative pose).  Inputs and recorded outputs only; run on the CPU in the build
container, with the path of the reference checkout as the only argument:

    python tests/golden/make_mv_geo_golden.py <reference checkout>

The module is loaded as make_golden.py loads it (EMPTY placeholder modules for cv2 and the CUDA-only gaussian_renderer, neither
touched here).  _get_points_from_depth and _reproject_points move their camera constants with `.cuda()`: for the duration of
the call `Tensor.cuda` is the identity in this process, so the reference's float32 arithmetic runs unchanged on the CPU.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "gs-2m_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def _load_ref_loss_utils(reference_root):
    added = []
    for name in ("cv2", "gaussian_renderer"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.render = None
            sys.modules[name] = m
            added.append(name)
    spec = importlib.util.spec_from_file_location("ref_loss_utils", os.path.join(reference_root, "utils", "loss_utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    for name in added:
        del sys.modules[name]
    return ref


def main(reference_root):
    import mv_geo_ref as R
    ref = _load_ref_loss_utils(reference_root)
    g = torch.Generator().manual_seed(2468)
    rc = R.RefCam(23, 17, 21.0, 19.5, 11.5, 8.5, (0.0, 0.0, 0.0), (0.1, -0.1, 6.0))
    nc = R.RefCam(19, 13, 24.0, 26.5, 8.7, 7.1, (0.45, -0.25, 0.3), (0.0, 0.1, 6.0))
    depth, normal, depth_n, normal_n = R._maps(rc, nc, g, 5.5, 5.4)
    depth[0, 1:3, 1:4] = 0.0   # background.  (No zero-length normal: x / (|x| + 1e-8) has no float32 value there -- the reference's own
    # lookup at the pixel centres leaks ~1e-7 of the neighbouring normals into it, which the normalisation blows up to unit length.)
    occlusion = 0.05
    cam, near = rc.project_camera(), nc.project_camera()
    pixels = R.pixel_grid(rc.W, rc.H, torch.float32)
    saved = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        pts = ref._get_points_from_depth(cam, depth)                                                     # :256
        pts_near = pts @ near.world_view_transform[:3, :3] + near.world_view_transform[3, :3]            # :258
        map_z, map_n, valid = ref._sample_depth_normal(pts_near, near, {"depth_map": depth_n, "normal_map": normal_n})
        valid = valid & (pts_near[:, 2] - map_z <= occlusion)                                            # :263
        rep = ref._reproject_points(near, cam, pts_near, map_z)                                          # :266
        noise = torch.norm(rep - pixels.reshape(*rep.shape), dim=-1)                                     # :268
        normals = ref._sample_normal_map(pixels, normal)                                                 # :271
        normals = normals / (normals.norm(dim=1, keepdim=True) + 1e-8)
        angle = torch.acos(torch.sum(normals * map_n, dim=1).clamp(-1 + 1e-6, 1 - 1e-6))                 # :275-276
    finally:
        torch.Tensor.cuda = saved
    out = dict(depth=depth.numpy(), normal=normal.numpy(), depth_n=depth_n.numpy(), normal_n=normal_n.numpy(), ref_cam=rc.numbers(), near_cam=nc.numbers(),
               occlusion=np.float64(occlusion), noise=noise.numpy(), angle=angle.numpy(), valid=valid.numpy())
    np.savez_compressed(os.path.join(HERE, "ref_mv_geo.npz"), **out)
    print("wrote ref_mv_geo.npz: valid", int(valid.sum()), "of", valid.numel())


if __name__ == "__main__":
    main(sys.argv[1])
