"""Generates tests/golden/ref_patch_ncc.npz: the photometric chain of multi_view_loss (utils/loss_utils.py:308-342) run from the
REFERENCE's own functions -- _patch_offsets, _patch_warp, _loss_ncc and F.grid_sample, composed as those lines compose them --
and the roughness variant's chain (:200-205: _patch_gradient of both patches, _loss_ncc of the magnitudes, _loss_ncc with
std_mask), on one small scene (24 x 18 grey images, unequal cameras, 48 samples, 7 x 7 patches, a few of them reaching over the
image border).  Inputs and recorded outputs only; run on the CPU with the path of the reference checkout as the only argument:

    python tests/golden/make_patch_ncc_golden.py <reference checkout>

The module is loaded as make_mv_geo_golden.py loads it.  _patch_warp and _loss_ncc build their constants on `uv.device` /
`ref.device`, so they run on the CPU unchanged.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "gs-2m_amd"), os.path.join(ROOT, "tests"), HERE):
    sys.path.insert(0, p)


def main(reference_root):
    import patch_ncc_ref as R
    from make_mv_geo_golden import _load_ref_loss_utils
    ref = _load_ref_loss_utils(reference_root)
    g = np.random.default_rng(97531)
    rc = R.RefCam(24, 18, 26.0, 25.0, 11.7, 9.2, (0.0, 0.0, 0.0), (0.0, 0.0, 6.0))
    nc = R.RefCam(24, 18, 27.0, 26.5, 12.4, 8.6, (0.7, -0.25, 0.3), (0.0, 0.0, 6.0))
    ncc_scale, patch, N = 1.0, 3, 48
    gray_r, gray_n = R.plane_image(rc), R.plane_image(nc)
    pixels = np.stack([g.integers(3, 21, N), g.integers(3, 15, N)], 1).astype(np.float32)
    pixels[:6] = [[0, 0], [23, 17], [1, 9], [22, 4], [12, 0], [11, 17]]     # patches over every side and two corners
    gray_r[10:18, 0:8] = (0.5 + 3e-3 * g.random((8, 8))).astype(np.float32)  # a low-texture block: the switch is on for these four
    pixels[6:10] = [[3, 13], [4, 14], [3, 14], [4, 13]]
    n0, d0 = R.true_plane(rc)
    normals = n0[None] + 0.05 * g.standard_normal((N, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)
    dists = (d0 * (1.0 + 0.03 * g.standard_normal(N))).astype(np.float32)
    cam, near = R.project_camera(rc, gray_r), R.project_camera(nc, gray_n)
    pix, ln, ld = torch.tensor(pixels), torch.tensor(normals), torch.tensor(dists)

    offsets = ref._patch_offsets(patch, pix.device)                                               # :309
    ori = pix.reshape(-1, 1, 2) / ncc_scale + offsets.float()                                     # :310
    gt = cam.gray_image                                                                           # :312
    h, w = gt.squeeze().shape
    pp = ori.clone()
    pp[:, :, 0] = 2 * pp[:, :, 0] / (w - 1) - 1.0
    pp[:, :, 1] = 2 * pp[:, :, 1] / (h - 1) - 1.0
    ref_val = F.grid_sample(gt.unsqueeze(1), pp.view(1, -1, 1, 2), align_corners=True)            # :317
    tps = (patch * 2 + 1) ** 2
    ref_val = ref_val.reshape(-1, tps)
    rn_R = near.world_view_transform[:3, :3].transpose(-1, -2) @ cam.world_view_transform[:3, :3]  # :321
    rn_t = -rn_R @ cam.world_view_transform[3, :3] + near.world_view_transform[3, :3]
    H = rn_R[None] - torch.matmul(rn_t[None, :, None].expand(ld.shape[0], 3, 1),
                                  ln[:, :, None].expand(ld.shape[0], 3, 1).permute(0, 2, 1)) / ld[..., None, None]   # :329-331
    H = torch.matmul(near.get_K(ncc_scale)[None].expand(ld.shape[0], 3, 3), H)                    # :332
    H = H @ cam.get_inv_K(ncc_scale)                                                              # :333
    grid = ref._patch_warp(H.reshape(-1, 3, 3), ori)                                              # :335
    grid[:, :, 0] = 2 * grid[:, :, 0] / (w - 1) - 1.0
    grid[:, :, 1] = 2 * grid[:, :, 1] / (h - 1) - 1.0
    samp = F.grid_sample(near.gray_image[None], grid.reshape(1, -1, 1, 2), align_corners=True)    # :339
    samp = samp.reshape(-1, tps)
    ncc, mask = ref._loss_ncc(ref_val, samp)                                                      # :342
    ps = patch * 2 + 1                                                                            # roughness_loss :200-205
    ref_grad, nea_grad = ref._patch_gradient(ref_val, ps), ref._patch_gradient(samp, ps)
    ncc_grad, _ = ref._loss_ncc(ref_grad.view(-1, tps), nea_grad.view(-1, tps))
    ncc_gray, std_mask = ref._loss_ncc(ref_val, samp, std_mask=True)
    out = dict(ref_cam=rc.numbers(), near_cam=nc.numbers(), ncc_scale=np.float64(ncc_scale), patch=np.int64(patch), ref_gray=gray_r, near_gray=gray_n,
               pixels=pixels, normals=normals, dists=dists, ncc=ncc.numpy(), mask=mask.numpy(), ncc_gray=ncc_gray.numpy(), ncc_grad=ncc_grad.numpy(),
               std_mask=std_mask.numpy())
    np.savez_compressed(os.path.join(HERE, "ref_patch_ncc.npz"), **out)
    print("wrote ref_patch_ncc.npz: ncc", float(ncc.min()), "..", float(ncc.max()), "mask", int(mask.sum()), "of", N, "std_mask", int(std_mask.sum()))


if __name__ == "__main__":
    main(sys.argv[1])
