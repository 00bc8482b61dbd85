"""Per-view maps on the GPU: render.py's render, gt, normal, depth and BRDF images (include/gs2m_maps.h, csrc/view_maps.hip;
DESIGN.md §13).

    python gs-2m_amd/gs2m_render.py --ply point_cloud.ply -s SCENE -m MODEL [--label ours] [--iteration 30000]
                                    [--skip_train] [--skip_test] [--normal_world] [--normal_sobel] [--extract_mesh]
                                    [--dtu | --tnt | --blender]

writes MODEL/<split>/<label>_<iteration>/{render, gt, normal, depth}/<stem>.png -- the tree `gs2m_metrics.py -m MODEL` reads --
and, with --extract_mesh, .../mesh/{config.json, tsdf_mesh.ply, tsdf_post.ply} through gs2m_mesh.  Every image is formed on
the device as the 8-bit array that is stored: the depth image from exact order statistics (a radix select; np.percentile's
values bit for bit), numpy's fp32 interpolation and matplotlib's magma table; every other map by one packing kernel that
rounds as torchvision's save_image or truncates as map_to_rgba.  Only the PNG encoding is host work.

There is NO CPU fallback: `order_stats`, `depth_image` and `pack_image` refuse CPU tensors."""
import argparse
import ctypes as C
import json
import os
import re
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np
import torch

import gs2m_native as N

MAX_RANKS = 8  # GS2M_MAPS_MAX_RANKS
CHW, HWC = 0, 1  # GS2M_PACK_CHW / _HWC
TRUNC, SRGB, NORMAL = 1, 2, 4  # GS2M_PACK_*


def percentile_plan(n, q):
    """np.percentile(a, q) of a float32 array of `n` values, method 'linear', as numpy evaluates it (lib/_function_base_impl.py:
    `percentile`, `_quantile`, `_get_indexes`, `_get_gamma`): the quantile q / float32(100), the virtual index (n - 1) * quantile
    and the weight are FLOAT32.  -> (rank of `previous`, rank of `next`, weight as np.float32); the value is
    `lerp(previous, next, weight)` in numpy's two-sided form (gs2m_maps.h)."""
    quantile = np.asanyarray(np.true_divide(q, np.float32(100)))
    virtual = np.asanyarray((n - 1) * quantile)
    prev = np.asanyarray(np.floor(virtual))
    nxt = np.asanyarray(prev + 1)
    if virtual >= n - 1:
        prev, nxt = np.asanyarray(-1.0), np.asanyarray(-1.0)
    if virtual < 0:
        prev, nxt = np.asanyarray(0.0), np.asanyarray(0.0)
    prev, nxt = prev.astype(np.intp), nxt.astype(np.intp)
    gamma = np.asanyarray(np.asanyarray(virtual - prev), dtype=virtual.dtype)
    return int(prev) % n, int(nxt) % n, np.float32(gamma)


def order_stats(x, ranks):
    """x: float32 device tensor of any shape; ranks: up to 8 integers in [0, x.numel()), repeats allowed.  -> (values (k,)
    float32, nonfinite (1,) int64), both on the device: the values np.sort(x.ravel()) holds at `ranks`, bit for bit (-0.0
    directly below +0.0, NaN last), and the number of NaN / Inf in x.  Nothing is sorted and the host does not wait."""
    who = "order_stats"
    x = N.f32(x, "x", who=who)
    ranks = [int(r) for r in ranks]
    n, k = x.numel(), len(ranks)
    if n < 1 or not 1 <= k <= MAX_RANKS or any(r < 0 or r >= n for r in ranks):
        raise ValueError(f"{who}: {k} ranks {ranks} for {n} values; 1 to {MAX_RANKS} ranks in [0, n) of a non-empty tensor")
    dev = x.device
    nbytes = C.c_longlong()
    N.check(N.lib().gs2m_order_stats_workspace_bytes(n, k, C.byref(nbytes)), "gs2m_order_stats_workspace_bytes")
    with N.device_guard(dev):
        ws = torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device=dev)
        out = torch.empty(k, dtype=torch.float32, device=dev)
        nonfinite = torch.empty(1, dtype=torch.int64, device=dev)
    N.launch("gs2m_order_stats", dev, n, x.data_ptr(), k, (C.c_longlong * k)(*ranks), ws.data_ptr(), ws.numel() * 8, out.data_ptr(),
             nonfinite.data_ptr())
    return out, nonfinite


def depth_image(depth, lower=1, upper=99):
    """utils/image_utils.py:79-87 `save_depth_map` on the device: depth (H, W) float32 -> (H, W, 4) uint8, the RGBA array
    `plt.imsave` stores (magma of the map clipped to its `lower` / `upper` percentiles, alpha 255).  ValueError when the
    map holds a NaN or an Inf (numpy's percentile of such a map is NaN or the image meaningless)."""
    who = "depth_image"
    depth = N.f32(depth, "depth", who=who)
    if depth.dim() != 2 or depth.numel() == 0:
        raise RuntimeError(f"{who}: `depth` must have shape (H, W), got {tuple(depth.shape)}")
    h, w = depth.shape
    n = h * w
    lo0, lo1, t_lo = percentile_plan(n, lower)
    hi0, hi1, t_hi = percentile_plan(n, upper)
    stats, nonfinite = order_stats(depth, (lo0, lo1, hi0, hi1))
    with N.device_guard(depth.device):
        out = torch.empty((h, w, 4), dtype=torch.uint8, device=depth.device)
    N.launch("gs2m_depth_colorize", depth.device, h, w, depth.data_ptr(), stats.data_ptr(), float(t_lo), float(t_hi), out.data_ptr())
    bad = int(nonfinite.item())
    if bad:
        raise ValueError(f"{who}: the depth map holds {bad} non-finite values")
    return out


def pack_image(src, layout="chw", quant="round", alpha=None, mask=None, background=None, srgb=False, normal=False, rot=None,
               channels=None, out=None):
    """One map of render.py as the 8-bit image that is stored (gs2m_maps.h `gs2m_pack_image`).

    src         float32 device tensor, (C, H, W) [layout "chw"] or (H, W, C) ["hwc"], C in {1, 3}; C = 1 fills three channels
    quant       "round": torchvision.utils.save_image (= gs2m_metrics.quantise); "trunc": map_to_rgba's `(x * 255).byte()`
    alpha       (H, W) or (1, H, W) float32: a fourth byte trunc(alpha * 255) -- map_to_rgba
    mask, background   (H, W) / (1, H, W) float32 or bool, and (3,) float32: clamp(src, 0, 1) where mask > 0.5, else background
    srgb        pbr.linear_to_srgb first
    normal, rot convert_normal_for_save: normalise, with `rot` = world_view_transform[:3, :3] to view space with y and z
                flipped, then 0.5 x + 0.5
    channels    3 or 4 (default: 4 with alpha, else 3); `out`: a uint8 tensor or view of (H, W, channels) to write into
    -> (H, W, channels) uint8 on the device."""
    who = "pack_image"
    src = N.f32(src, "src", who=who)
    if layout not in ("chw", "hwc") or quant not in ("round", "trunc"):
        raise ValueError(f"{who}: layout {layout!r} / quant {quant!r}; 'chw' or 'hwc', 'round' or 'trunc'")
    if src.dim() != 3:
        raise RuntimeError(f"{who}: `src` must have three dimensions, got {tuple(src.shape)}")
    (c, h, w) = src.shape if layout == "chw" else (src.shape[2], src.shape[0], src.shape[1])
    if c not in (1, 3) or h < 1 or w < 1:
        raise RuntimeError(f"{who}: `src` {tuple(src.shape)} as {layout}: C must be 1 or 3, H and W at least 1")
    dev = src.device

    def plane(t, name):
        if t is None:
            return None
        if isinstance(t, torch.Tensor) and t.dtype in (torch.bool, torch.uint8):
            t = t.float()
        t = N.f32(t, name, who=who)
        if t.numel() != h * w:
            raise RuntimeError(f"{who}: `{name}` {tuple(t.shape)} does not match the image ({h}, {w})")
        return t

    alpha, mask = plane(alpha, "alpha"), plane(mask, "mask")
    if mask is not None:
        if background is None:
            raise ValueError(f"{who}: a mask needs a background colour")
        background = N.f32(background, "background", (3,), who=who)
    else:
        background = None
    if rot is not None:
        rot = N.f32(rot, "rot", (3, 3), who=who)
    if (normal and c != 3) or (rot is not None and not normal):
        raise ValueError(f"{who}: the normal transform takes a 3-channel source (and `rot` belongs to it)")
    channels = (4 if alpha is not None else 3) if channels is None else int(channels)
    if channels not in (3, 4) or (alpha is not None and channels != 4):
        raise ValueError(f"{who}: {channels} output channels" + (" with an alpha plane" if alpha is not None else ""))
    if out is None:
        with N.device_guard(dev):
            out = torch.empty((h, w, channels), dtype=torch.uint8, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (h, w, channels) or not out.is_contiguous()
          or out.device != dev):
        raise RuntimeError(f"{who}: `out` must be a contiguous uint8 tensor of shape {(h, w, channels)} on {dev}")
    flags = (TRUNC if quant == "trunc" else 0) | (SRGB if srgb else 0) | (NORMAL if normal else 0)
    N.launch("gs2m_pack_image", dev, h, w, c, CHW if layout == "chw" else HWC, src.data_ptr(), N.ptr(alpha), N.ptr(mask), N.ptr(background),
             N.ptr(rot), flags, channels, out.data_ptr())
    return out


# ---- render.py:35-151 -------------------------------------------------------------------------------------------------------

def update_points(point_file, key, count):
    """render.py:59-67: the JSON object at `point_file` with `key` set to the number of Gaussians."""
    points = {}
    if os.path.exists(point_file):
        with open(point_file, "r") as f:
            points = json.load(f)
    points[key] = int(count)
    with open(point_file, "w") as f:
        json.dump(points, f, indent=4)
    return points


def render_views_to_disk(gaussians, views, out_dir, background, white_background=False, normal_world=False, normal_sobel=False,
                         light=None, metallic=False, gamma=False, mask_gt=False, points_file=None, png="host"):
    """render.py:35-151 for one split: renders every view with this repository's render() and writes

        out_dir/{render, gt, normal, depth}/<stem>.png
        with `light` (anything with `.cubemap` and `.brdf_lut`: the material model's environment light), render/ holds the
        PBR image and out_dir/{albedo, roughness, metallic, diffuse, specular}/<stem>.png and out_dir/envmap.png are added

    with the reference's branches and rounding: gt and render through save_image's rounding (gt composed on `background`
    outside `view.alpha_mask` when `white_background`; the PBR image composed by the alpha mask when `mask_gt` or
    `white_background`, else by the normal mask, on black when `mask_gt`); the normal and BRDF maps as RGBA through
    map_to_rgba's truncation when `white_background`, else as RGB through save_image's rounding; depth through
    save_depth_map.  `normal_sobel`: the normal image shows the normals estimated from depth; `gamma`: diffuse and specular go
    through linear_to_srgb.  `points_file` (default: points.json two levels above out_dir, i.e. in the model directory) gets
    the number of Gaussians under out_dir's name.  `view.image_name` gives the stem (default: the view's index, five digits).
    `png`: "host" writes the files through Pillow; "device" encodes them with gs2m_png, a view's RGB images in one call and its
    RGBA images in another (the same pixels, not the same file bytes).
    -> (N, H, W) float32 depths on the device, what `gs2m_mesh.fuse_depths` takes."""
    import torch.nn.functional as F
    from gaussian_renderer import render
    from gs2m_scene import PipelineParams
    from gs2m_png import Writer
    writer = Writer(png)
    out_dir = str(out_dir)
    subs = ["render", "gt", "normal", "depth"] + (["albedo", "roughness", "metallic", "diffuse", "specular"] if light is not None else [])
    for sub in subs:
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    if points_file is None:
        points_file = os.path.join(os.path.dirname(os.path.dirname(os.path.normpath(out_dir))), "points.json")
    update_points(points_file, os.path.basename(os.path.normpath(out_dir)), gaussians.get_xyz.shape[0])
    quant = "trunc" if white_background else "round"
    depths = []
    with torch.no_grad():
        if light is not None:
            from pbr import pbr_render
            light.cubemap.build_mips()
            writer.put(pack_image(light.cubemap.export_envmap(return_img=True).contiguous(), "hwc"), os.path.join(out_dir, "envmap.png"))
            writer.flush()
        for k, view in enumerate(views):
            if getattr(view, "image_name", None) is None:
                view.image_name = f"{k:05d}.png"
            stem = view.image_name.rsplit(".", 1)[0]
            if getattr(view, "gt_image", None) is None:
                raise ValueError(f"gs2m_render: view {stem} carries no gt_image")
            dev = background.device
            alpha = getattr(view, "alpha_mask", None)
            if alpha is not None:
                alpha = torch.as_tensor(alpha).to(dev, torch.float32).contiguous()
            if alpha is None and (white_background or (light is not None and mask_gt)):
                raise ValueError(f"gs2m_render: view {stem} carries no alpha_mask")
            pkg = render(view, gaussians, PipelineParams(), background, material_stage=True, sobel_normal=normal_sobel,
                         blend_metallic=metallic)

            def put(sub, image):
                writer.put(image, os.path.join(out_dir, sub, stem + ".png"))

            def put_map(sub, src, layout="chw", **kw):  # render.py:140-151
                put(sub, pack_image(src, layout, quant, alpha=alpha if white_background else None, **kw))

            gt = torch.as_tensor(view.gt_image).to(dev, torch.float32)[0:3].contiguous()
            put("gt", pack_image(gt, mask=alpha if white_background else None, background=background))
            rot = None if normal_world else view.world_view_transform[:3, :3].contiguous()
            put_map("normal", (pkg["sobel_map"] if normal_sobel else pkg["normal_map"]).contiguous(), normal=True, rot=rot)
            depth = pkg["depth_map"].reshape(pkg["depth_map"].shape[-2:]).float().contiguous()
            put("depth", depth_image(depth))
            depths.append(depth.clone())
            if light is None:
                put("render", pack_image(pkg["render"].contiguous()))
                writer.flush()
                continue
            rays = getattr(view, "_render_rays", None)
            if rays is None:
                rays = F.normalize(view.get_rays().view(-1, 3), p=2, dim=-1)
                try:
                    view._render_rays = rays
                except AttributeError:
                    pass
            pbr = pbr_render(light, view, rays, pkg, metallic, gamma)
            pbr_mask = alpha if (mask_gt or white_background) else pkg["normal_mask"]
            h, w = depth.shape
            put("render", pack_image(pbr["render_rgb"].reshape(h, w, 3).contiguous(), "hwc", mask=pbr_mask,
                                     background=torch.zeros_like(background) if mask_gt else background))
            put_map("albedo", pkg["albedo_map"].contiguous())
            put_map("roughness", pbr["roughness_map"].reshape(1, h, w).contiguous())
            put_map("metallic", pbr["metallic_map"].reshape(1, h, w).contiguous())
            put_map("diffuse", pbr["diffuse_rgb"].reshape(h, w, 3).contiguous(), "hwc", srgb=gamma)
            put_map("specular", pbr["specular_rgb"].reshape(h, w, 3).contiguous(), "hwc", srgb=gamma)
            writer.flush()
    if not depths:
        return torch.empty((0, 0, 0), dtype=torch.float32, device=background.device)
    return torch.stack(depths)


# ---- command line -------------------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    """render.py's command line with its presets applied.  -> (namespace, bounds): bounds (3, 2) is --tnt's aabb_range, else None."""
    from gs2m_mesh import TNT_360_SCENES
    ap = argparse.ArgumentParser(
        description="Per-view images of a trained model (render.py): render, gt, normal and depth PNGs per split, and the TSDF mesh "
                    "with --extract_mesh.  The training loop saves the Gaussians only, not the environment light, so the command line "
                    "covers render.py's non-material branch (render/ holds the SH colour; no BRDF maps, no envmap.png); "
                    "gs2m_render.render_views_to_disk takes a light and writes them.")
    ap.add_argument("--ply", required=True, help="the model's point_cloud.ply")
    ap.add_argument("--source_path", "--source-path", "-s", required=True, help="COLMAP-format dataset (NeRF-synthetic with --blender)")
    ap.add_argument("--model_path", "-m", required=True, help="the images go to MODEL/<split>/<label>_<iteration>/")
    ap.add_argument("--label", default="ours", type=str)
    ap.add_argument("--iteration", default=-1, type=int, help="default: the N of an .../iteration_N/... in --ply")
    ap.add_argument("--resolution", "-r", type=int, default=1)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--white_background", action="store_true",
                    help="white background and RGBA normal maps; needs the views' alpha masks, which the --blender loader and --device-ingest provide")
    ap.add_argument("--skip_train", action="store_true")
    ap.add_argument("--skip_test", action="store_true")
    ap.add_argument("--extract_mesh", action="store_true")
    ap.add_argument("--max_depth", default=-1.0, type=float)
    ap.add_argument("--voxel_size", default=-1.0, type=float)
    ap.add_argument("--sdf_trunc", default=-1.0, type=float)
    ap.add_argument("--num_clusters", default=1, type=int)
    ap.add_argument("--filter_depth", action="store_true",
                    help="accepted and ignored: render.py's filter removes pixels where acos(|dot|) > 100 degrees, which no pixel meets "
                         "(DESIGN.md section 13)")
    ap.add_argument("--dtu", action="store_true", help="render.py's DTU preset: mesh at 5.0 / 0.002 / 0.008, train split only, view-space normals")
    ap.add_argument("--tnt", action="store_true", help="render.py's Tanks and Temples preset (as gs2m_mesh.py --tnt; the scene is MODEL's name)")
    ap.add_argument("--blender", action="store_true", help="render.py's Blender preset: test split only, world-space normals, mesh at 8.0 / 0.004")
    ap.add_argument("--normal_world", action="store_true", help="Save normals in world space, defaults to camera space")
    ap.add_argument("--normal_sobel", action="store_true", help="Use normal estimated from depths")
    from gs2m_ingest import add_ingest_arguments
    add_ingest_arguments(ap)  # COLMAP datasets: the views' alpha masks from --masks or the images' alpha channel
    from gs2m_png import add_png_argument
    add_png_argument(ap)
    a = ap.parse_args(argv)
    if a.dtu + a.tnt + a.blender > 1:
        ap.error("--dtu, --tnt and --blender are presets: choose one")
    if a.iteration < 0:
        m = re.search(r"iteration_(\d+)", a.ply)
        if m is None:
            ap.error("--iteration is needed: --ply names no iteration_N directory")
        a.iteration = int(m.group(1))
    bounds = None
    if a.dtu:
        a.max_depth, a.voxel_size, a.sdf_trunc, a.num_clusters = 5.0, 0.002, 4.0 * 0.002, 1
        a.filter_depth, a.extract_mesh, a.skip_test, a.normal_world = False, True, True, False
    if a.tnt:
        scene = os.path.basename(os.path.normpath(a.model_path)).lower()
        a.max_depth, a.num_clusters, a.voxel_size = (3.0 if scene in TNT_360_SCENES else 4.5), 1, 0.002
        a.filter_depth, a.extract_mesh, a.skip_test, a.normal_world = True, True, True, False
        tf = os.path.join(a.source_path, "transforms.json")
        if os.path.exists(tf):
            with open(tf) as f:
                aabb = json.load(f).get("aabb_range")
            if aabb is not None:
                bounds = np.asarray(aabb, dtype=np.float64).reshape(3, 2)
                a.voxel_size = float(np.max(bounds[:, 1] - bounds[:, 0])) / 2048
        a.sdf_trunc = 4.0 * a.voxel_size
    if a.blender:
        a.skip_train, a.skip_test, a.normal_world, a.extract_mesh = True, False, True, True
        a.max_depth, a.voxel_size, a.sdf_trunc, a.num_clusters = 8.0, 0.004, 4.0 * 0.004, 1
    return a, bounds


def render_split(a, split, model, cams, gts, extent, background, bounds=None):
    """One split of the command line: the images, then (--extract_mesh) render.py:153-183 through gs2m_mesh."""
    import gs2m_mesh as M
    if not cams:
        print(f"[!] No views to render in {split} set")
        return
    for k, (cam, gt) in enumerate(zip(cams, gts)):
        cam.gt_image = gt
        if getattr(cam, "image_name", None) is None:
            cam.image_name = f"{k:05d}.png"
    out_dir = os.path.join(a.model_path, split, f"{a.label}_{a.iteration}")
    depths = render_views_to_disk(model, cams, out_dir, background, a.white_background, a.normal_world, a.normal_sobel,
                                  points_file=os.path.join(a.model_path, "points.json"), png="device" if a.device_png else "host")
    print(f"[>] {len(cams)} views -> {out_dir}")
    if not a.extract_mesh:
        return
    mesh_dir = os.path.join(out_dir, "mesh")
    os.makedirs(mesh_dir, exist_ok=True)
    max_depth = a.max_depth if a.max_depth > 0 else 2.0 * extent
    voxel_size = a.voxel_size if a.voxel_size > 0 else max_depth / 1024.0
    sdf_trunc = a.sdf_trunc if a.sdf_trunc > 0 else 4.0 * voxel_size
    with open(os.path.join(mesh_dir, "config.json"), "w") as f:
        json.dump({"max_depth": max_depth, "voxel_size": voxel_size, "sdf_trunc": sdf_trunc}, f, indent=4)
    vol = M.fuse_depths(depths, cams, os.path.join(out_dir, "render"), max_depth, voxel_size, sdf_trunc, bounds, device=background.device)
    on_device = vol.extract_triangle_mesh(to_host=False)
    mesh, post = on_device.cpu(), M.post_process_mesh_gpu(on_device, a.num_clusters).cpu()
    M.write_mesh(os.path.join(mesh_dir, "tsdf_mesh.ply"), mesh)
    M.write_mesh(os.path.join(mesh_dir, "tsdf_post.ply"), post)
    print(f"[>] Num vertices mesh: {len(mesh.vertices)}\n[>] Num vertices post: {len(post.vertices)}\n[>] Meshes written to: {mesh_dir}")


def _blender_alpha(folder, transforms, device, extension=".png"):
    """The alpha planes of a NeRF-synthetic split's RGBA images, (1, H, W) float each: the views' alpha masks."""
    from PIL import Image
    with open(os.path.join(folder, transforms)) as f:
        frames = json.load(f)["frames"]
    return [torch.from_numpy(np.asarray(Image.open(os.path.join(folder, fr["file_path"] + extension)).convert("RGBA"), dtype=np.float32)[..., 3]
                             / 255.0)[None].to(device) for fr in frames]


def main(argv=None):
    a, bounds = parse_args(argv)
    import gs2m_train as T
    from gs2m_model import GaussianModel
    model = GaussianModel(a.sh_degree)
    model.load_ply(a.ply)
    background = torch.tensor([1.0, 1.0, 1.0] if a.white_background else [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    splits = {}
    if a.blender:
        for split in ("train", "test"):
            if not getattr(a, "skip_" + split):
                cams, gts, _, _, extent = T.load_blender_dataset(a.source_path, f"transforms_{split}.json", white_background=a.white_background)
                for cam, alpha in zip(cams, _blender_alpha(a.source_path, f"transforms_{split}.json", "cuda")):
                    cam.alpha_mask = alpha
                splits[split] = (cams, gts, extent)
    else:
        from gs2m_ingest import ingest_keywords
        cams, gts, _, _, extent = T.load_colmap_dataset(a.source_path, resolution=a.resolution, **ingest_keywords(a))
        if not a.skip_train:
            splits["train"] = (cams, gts, extent)
        if not a.skip_test:  # every 8th image, the reference's llffhold (as gs2m_mesh.py --split test)
            splits["test"] = (cams[::8], gts[::8], extent)
    for split, (cams, gts, extent) in splits.items():
        render_split(a, split, model, cams, gts, extent, background, bounds if split == "train" else None)


if __name__ == "__main__":
    main()
