"""Dataset preparation on the GPU: what COLMAP's `image_undistorter` does between the mapper and the loaders
(scripts/colmap.py runs it after the mapper) -- `distorted/sparse/0` + `input/` become `images/` + `sparse/0` with PINHOLE
cameras (include/gs2m_undistort.h, csrc/undistort.hip, csrc/undistort_model.h).

    python gs-2m_amd/gs2m_undistort.py -s SCENE [--blank-pixels B] [--min-scale S] [--max-scale S] [--device-png] [--write-valid DIR]

    out_cam = undistort_camera(cam)                           # host only
    warped, valid = undistort_images(batch_u8, cam, out_cam, valid=True)
    xys, failed = undistort_points(xys, cam, out_cam)
    cameras, images = undistort_model(cameras, images)

The contract is this project's own, modelled on image_undistorter; no file of COLMAP's pins it -- tests/undistort_ref.py does.
SIMPLE_PINHOLE and PINHOLE are the identity; SIMPLE_RADIAL, RADIAL, OPENCV and FULL_OPENCV are undistorted; the fisheye family,
FOV and THIN_PRISM_FISHEYE are refused by name.  The written model carries the principal point of the crop (cx w'/w, cy h'/h);
the loaders, like the reference, read the focal lengths only.

There is NO CPU fallback: the kernels refuse CPU tensors.  `undistort_camera` is host-only."""
import ctypes as C
import os
import shutil

import numpy as np
import torch

import gs2m_colmap
import gs2m_native as N

SUPPORTED = ("SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV")
IDENTITY = ("SIMPLE_PINHOLE", "PINHOLE")
_IDS = {name: mid for mid, (name, _) in gs2m_colmap.CAMERA_MODELS.items()}
BATCH_BYTES = 1 << 30  # source + warped bytes of one batch of undistort_dataset, at most (and at most a quarter of the free memory)


def _model(cam, who):
    """-> (COLMAP's id, the parameters as a C double array); unsupported models are refused by name"""
    if cam.model not in SUPPORTED:
        raise ValueError(f"{who}: COLMAP camera model {cam.model} is not supported: SIMPLE_RADIAL, RADIAL, OPENCV and FULL_OPENCV are "
                         "undistorted, (SIMPLE_)PINHOLE pass through; the fisheye, FOV and thin-prism models need atan / tan")
    params = np.ascontiguousarray(cam.params, dtype=np.float64)
    if params.shape != (gs2m_colmap.CAMERA_MODELS[_IDS[cam.model]][1],):
        raise ValueError(f"{who}: {cam.model} takes {gs2m_colmap.CAMERA_MODELS[_IDS[cam.model]][1]} parameters, got {params.shape}")
    return _IDS[cam.model], (C.c_double * len(params))(*params)


def _pinhole(out_cam, who):
    if out_cam.model != "PINHOLE":
        raise ValueError(f"{who}: `out_cam` must be a PINHOLE camera (undistort_camera's), got {out_cam.model}")
    return (C.c_double * 4)(*np.asarray(out_cam.params, dtype=np.float64))


def undistort_camera(cam, blank_pixels=0.0, min_scale=0.2, max_scale=2.0):
    """The undistorted PINHOLE camera of `cam` (gs2m_colmap.Camera): a crop about the principal point sized from the undistorted
    image borders; blank_pixels 0 keeps no black pixel, 1 keeps every source pixel.  Host only."""
    who = "undistort_camera"
    mid, params = _model(cam, who)
    ow, oh, q = C.c_int(), C.c_int(), (C.c_double * 4)()
    rc = N.lib().gs2m_undistort_camera(mid, int(cam.width), int(cam.height), params, float(blank_pixels), float(min_scale), float(max_scale),
                                      C.byref(ow), C.byref(oh), q)
    if rc == -1:
        raise ValueError(f"{who}: invalid camera or options ({cam.model} {cam.width}x{cam.height} {list(cam.params)}, blank_pixels {blank_pixels}, "
                         f"scale [{min_scale}, {max_scale}]), or an image border that cannot be undistorted")
    N.check(rc, "gs2m_undistort_camera")
    return gs2m_colmap.Camera(cam.id, "PINHOLE", ow.value, oh.value, np.array(list(q), dtype=np.float64))


def undistort_images(batch_u8, cam, out_cam, valid=False):
    """batch_u8: uint8 device tensor (N, H, W, CH) or (H, W, CH), CH in {1, 3}, images of `cam` -> the same layout at out_cam's
    size; with `valid` also the (H', W') uint8 mask, 255 where the source position lay inside the image."""
    who = "undistort_images"
    if not isinstance(batch_u8, torch.Tensor) or not batch_u8.is_cuda:
        raise RuntimeError(f"{who}: `batch_u8` must be a CUDA tensor on a HIP device; there is no CPU path")
    if batch_u8.dtype != torch.uint8:
        raise RuntimeError(f"{who}: `batch_u8` must be uint8, got {batch_u8.dtype}")
    single = batch_u8.dim() == 3
    t = (batch_u8.unsqueeze(0) if single else batch_u8).contiguous()
    if t.dim() != 4 or t.shape[3] not in (1, 3) or t.numel() == 0:
        raise RuntimeError(f"{who}: `batch_u8` must have shape (N, H, W, CH) or (H, W, CH) with CH 1 or 3, got {tuple(batch_u8.shape)}")
    n, h, w, ch = t.shape
    if (w, h) != (cam.width, cam.height):
        raise ValueError(f"{who}: the images are {w}x{h}, their camera {cam.width}x{cam.height}")
    mid, params = _model(cam, who)
    q = _pinhole(out_cam, who)
    ow, oh = int(out_cam.width), int(out_cam.height)
    dev = t.device
    with N.device_guard(dev):
        out = torch.empty((n, oh, ow, ch), dtype=torch.uint8, device=dev)
        mask = torch.empty((oh, ow), dtype=torch.uint8, device=dev) if valid else None
    N.launch("gs2m_undistort_images_u8", dev, mid, params, w, h, ch, n, t.data_ptr(), q, ow, oh, out.data_ptr(), N.ptr(mask))
    out = out[0] if single else out
    return (out, mask) if valid else out


def undistort_points(xys, cam, out_cam, device="cuda"):
    """xys (n, 2) float64, observations in pixels of `cam` -> (xys in out_cam (n, 2), failed).  A device tensor gives a device
    tensor and the count as an int32 tensor of one element (no synchronisation); a numpy array goes to `device` and back and
    gives an int.  An observation whose Newton iteration fails keeps its last finite iterate and is counted."""
    who = "undistort_points"
    mid, params = _model(cam, who)
    q = _pinhole(out_cam, who)
    host = not isinstance(xys, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(xys, dtype=np.float64).reshape(-1, 2)).to(device) if host else xys
    if not t.is_cuda:
        raise RuntimeError(f"{who}: `xys` must be a numpy array or a CUDA tensor on a HIP device; there is no CPU path")
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 2:
        raise RuntimeError(f"{who}: `xys` must be float64 (n, 2), got {t.dtype} {tuple(t.shape)}")
    t = t.contiguous()
    with N.device_guard(t.device):
        out = torch.empty_like(t)
        failed = torch.empty(1, dtype=torch.int32, device=t.device)
    N.launch("gs2m_undistort_points", t.device, t.shape[0], N.ptr(t), mid, params, q, N.ptr(out), failed.data_ptr())
    if host:
        return out.cpu().numpy(), int(failed.item())
    return out, failed


def undistort_model(cameras, images, blank_pixels=0.0, min_scale=0.2, max_scale=2.0, observations=True, device="cuda", stats=None):
    """cameras {id: Camera}, images {id: Image} as gs2m_colmap reads them -> (cameras, images): every camera PINHOLE
    (undistort_camera), every image's observations transformed (one undistort_points call per distorted camera); poses, names and
    point ids are kept.  `observations=False`: the cameras only, no GPU is touched.  `stats`: a dict that receives the number of
    `observations` and of `failed` iterations."""
    out_cams = {cid: undistort_camera(c, blank_pixels, min_scale, max_scale) for cid, c in cameras.items()}
    out_images = dict(images)
    total = failed = 0
    if observations:
        for cid, cam in cameras.items():
            if cam.model in IDENTITY:
                continue
            ids = [iid for iid, im in images.items() if im.camera_id == cid and im.xys is not None and len(im.xys)]
            if not ids:
                continue
            xy, bad = undistort_points(np.concatenate([images[iid].xys for iid in ids]), cam, out_cams[cid], device)
            total, failed, pos = total + len(xy), failed + bad, 0
            for iid in ids:
                m = len(images[iid].xys)
                out_images[iid] = images[iid]._replace(xys=xy[pos:pos + m])
                pos += m
    if stats is not None:
        stats.update(observations=total, failed=failed)
    return out_cams, out_images


def _batch_size(n, in_bytes, out_bytes, device):
    """images per warp call: from memory, never from the CPU count"""
    free = torch.cuda.mem_get_info(device)[0]
    return int(max(1, min(n, min(BATCH_BYTES, free // 4) // max(1, in_bytes + out_bytes))))


def _decode(path, size):
    from PIL import Image as PILImage
    with PILImage.open(path) as f:
        img = f.convert("L") if f.mode in ("L", "1", "I;16", "I", "F") else f.convert("RGB")
    if img.size != size:
        raise ValueError(f"undistort_dataset: {path} is {img.size[0]}x{img.size[1]}, its camera {size[0]}x{size[1]}")
    a = np.asarray(img)
    return a[:, :, None] if a.ndim == 2 else a


def undistort_dataset(source, input_model="distorted/sparse/0", input_images="input", output_images="images", output_model="sparse/0",
                      blank_pixels=0.0, min_scale=0.2, max_scale=2.0, device_png=False, write_valid="", device="cuda"):
    """`SOURCE/distorted/sparse/0` + `SOURCE/input` -> `SOURCE/images/<name>` + `SOURCE/sparse/0/{cameras,images,points3D}.bin`:
    what scripts/colmap.py's image_undistorter step leaves.  The images of one camera, size and channel count are warped in
    batches sized from the device memory; a file's format follows its name's extension (PNG through gs2m_png.Writer, on the GPU
    with `device_png`); points3D.bin is copied byte for byte.  `write_valid`: a folder (absolute, or relative to `source`) that
    receives each image's valid mask as <stem>.png -- what the loaders' --masks reads.  -> dict(images, cameras, observations,
    failed, batches)."""
    import gs2m_png
    device = torch.device(device)
    src_model = os.path.join(source, input_model)
    cameras = gs2m_colmap.read_intrinsics_binary(os.path.join(src_model, "cameras.bin"))
    images = gs2m_colmap.read_extrinsics_binary(os.path.join(src_model, "images.bin"))
    stats = {}
    out_cams, out_images = undistort_model(cameras, images, blank_pixels, min_scale, max_scale, device=device, stats=stats)
    valid_dir = "" if write_valid == "" else (write_valid if os.path.isabs(write_valid) else os.path.join(source, write_valid))
    if valid_dir:
        os.makedirs(valid_dir, exist_ok=True)
    batches = 0
    with gs2m_png.Writer("device" if device_png else "host") as writer:
        for cid, cam in cameras.items():
            names = sorted(im.name for im in images.values() if im.camera_id == cid)
            pos = 0
            while pos < len(names):
                first = _decode(os.path.join(source, input_images, names[pos]), (cam.width, cam.height))
                ch = first.shape[2]
                oc = out_cams[cid]
                n = _batch_size(len(names) - pos, first.size, oc.width * oc.height * ch, device)
                batch, taken = [first], [names[pos]]
                for name in names[pos + 1:pos + n]:
                    a = _decode(os.path.join(source, input_images, name), (cam.width, cam.height))
                    if a.shape[2] != ch:  # a gray file among colour files: it starts the next batch
                        break
                    batch.append(a)
                    taken.append(name)
                pos += len(taken)
                warped, valid = undistort_images(torch.from_numpy(np.stack(batch)).to(device), cam, oc, valid=True)
                batches += 1
                for k, name in enumerate(taken):
                    path = os.path.join(source, output_images, name)
                    os.makedirs(os.path.dirname(path), exist_ok=True)
                    img = warped[k] if ch == 3 else warped[k, :, :, 0]
                    if name.lower().endswith(".png"):
                        writer.put(img, path)
                    else:
                        from PIL import Image as PILImage
                        PILImage.fromarray(img.cpu().numpy()).save(path)
                    if valid_dir:
                        writer.put(valid, os.path.join(valid_dir, os.path.splitext(os.path.basename(name))[0] + ".png"))
                writer.flush()  # a batch's tensors are released before the next is uploaded
    dst_model = os.path.join(source, output_model)
    gs2m_colmap.write_model(dst_model, out_cams.values(), out_images.values(), np.zeros((0, 3)), np.zeros((0, 3), dtype=np.uint8))
    shutil.copyfile(os.path.join(src_model, "points3D.bin"), os.path.join(dst_model, "points3D.bin"))
    return dict(images=len(images), cameras=len(cameras), batches=batches, **stats)


def main(argv=None):
    import argparse
    import gs2m_png
    ap = argparse.ArgumentParser(description="COLMAP's image_undistorter on the GPU: SCENE/distorted/sparse/0 + SCENE/input -> SCENE/images + "
                                 "SCENE/sparse/0 with PINHOLE cameras")
    ap.add_argument("-s", "--source_path", required=True)
    ap.add_argument("--input-model", default="distorted/sparse/0")
    ap.add_argument("--input-images", default="input")
    ap.add_argument("--blank-pixels", type=float, default=0.0, help="0: no black pixel in the output; 1: every source pixel kept")
    ap.add_argument("--min-scale", type=float, default=0.2)
    ap.add_argument("--max-scale", type=float, default=2.0)
    ap.add_argument("--write-valid", default="", help="folder for the per-image valid masks (<stem>.png), what the loaders' --masks reads")
    gs2m_png.add_png_argument(ap)
    a = ap.parse_args(argv)
    st = undistort_dataset(a.source_path, a.input_model, a.input_images, blank_pixels=a.blank_pixels, min_scale=a.min_scale,
                           max_scale=a.max_scale, device_png=a.device_png, write_valid=a.write_valid)
    print(f"undistorted {st['images']} images of {st['cameras']} cameras in {st['batches']} batches; {st['observations']} observations, "
          f"{st['failed']} failed iterations")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
