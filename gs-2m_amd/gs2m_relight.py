"""Relighting: a trained material model under an environment it was not trained with.

    python gs-2m_amd/gs2m_relight.py --ply point_cloud.ply -s SCENE -m MODEL --envmap studio.hdr
           [--env-res 512] [--env-samples S] [--env-rotation DEG] [--exposure EV]
           [--metallic] [--gamma] [--background env|black|white] [--light-turntable N]
           [--blender] [-r N] [--skip_train] [--skip_test] [--device-png]

writes MODEL/<split>/<label>_<iteration>/relight/<envmap stem>/{render, diffuse, specular}/<stem>.png and envmap.png beside them;
with --light-turntable N also turntable/000.png ...: the split's first view under N rotations of the light, 360 / N degrees apart,
each a conversion of the source image at that angle (not a resampling of the cube map).

The light is an `gs2m_envmap.EnvLight` (the .hdr file decoded and converted to a cube map in HIP); rendering, shading, packing and
writing are the per-view stage's own: `render(..., material_stage=True)`, `pbr_render`, `gs2m_render.pack_image`, `gs2m_png.Writer`.
There is NO CPU fallback."""
import argparse
import math
import os
import re
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import torch

BACKGROUNDS = ("env", "black", "white")
MASKS = ("normal", "alpha")
MIN_RES = 64  # CubemapLight.build_mips spreads the roughness over its levels but the last: it needs three (64, 32, 16)


def _check(light, background, mask):
    if background not in BACKGROUNDS or mask not in MASKS:
        raise ValueError(f"gs2m_relight: background {background!r} / mask {mask!r}; one of {BACKGROUNDS} and of {MASKS}")
    res = int(light.cubemap.base.shape[1])
    if res < MIN_RES:
        raise ValueError(f"gs2m_relight: a {res}-texel light cannot be shaded with: build_mips and the shading need three specular levels, a resolution >= {MIN_RES}")


def environment_behind(light, view_dirs, gamma=False):
    """The environment seen along the view rays: the light's base cube map looked up at -view_dirs ((H, W, 3), surface -> eye, as
    pbr_render forms them), clamped to [0, 1] and through linear_to_srgb under `gamma`, like the shaded pixels."""
    import nvdiffrast.torch as dr
    from pbr import linear_to_srgb
    env = dr.texture(light.cubemap.base.detach()[None, ...], (-view_dirs)[None, ...].contiguous(), filter_mode="linear", boundary_mode="cube")[0]
    env = env.clamp(min=0.0, max=1.0)
    return linear_to_srgb(env) if gamma else env


def shade_view(gaussians, view, light, metallic=False, gamma=False, background="black", mask="normal"):
    """One view under `light`.  -> {"render", "diffuse", "specular"}: (H, W, 3) uint8 on the device, the arrays that are stored.
    render: the PBR image where the mask is set -- `mask` "normal": the render's normal mask, "alpha": `view.alpha_mask` -- and the
    `background` elsewhere ("env": `environment_behind`)."""
    import torch.nn.functional as F
    from gaussian_renderer import render
    from gs2m_render import pack_image
    from gs2m_scene import PipelineParams
    from pbr import pbr_render
    _check(light, background, mask)
    dev = light.cubemap.base.device
    with torch.no_grad():
        pkg = render(view, gaussians, PipelineParams(), torch.zeros(3, device=dev), material_stage=True, blend_metallic=metallic)
        rays = getattr(view, "_render_rays", None)
        if rays is None:
            rays = F.normalize(view.get_rays().view(-1, 3), p=2, dim=-1)
            try:
                view._render_rays = rays
            except AttributeError:
                pass
        pbr = pbr_render(light, view, rays, pkg, metallic, gamma)
        h, w = pkg["normal_map"].shape[-2:]
        if mask == "alpha":
            m = getattr(view, "alpha_mask", None)
            if m is None:
                raise ValueError("gs2m_relight: mask='alpha' needs the view's alpha_mask")
            m = torch.as_tensor(m).to(dev, torch.float32).reshape(h, w).contiguous()
        else:
            m = pkg["normal_mask"].to(torch.float32).reshape(h, w).contiguous()
        rgb = pbr["render_rgb"].reshape(h, w, 3).contiguous()
        if background == "env":
            view_dirs = view._pbr_view_dirs[1] if getattr(view, "_pbr_view_dirs", None) is not None else \
                F.normalize(-rays @ view.world_view_transform[:3, :3].T, p=2, dim=-1).reshape(h, w, 3)
            env = environment_behind(light, view_dirs, gamma)
            image = pack_image(torch.where(m[..., None] > 0.5, rgb.clamp(0.0, 1.0), env).contiguous(), "hwc")
        else:
            colour = torch.full((3,), 1.0 if background == "white" else 0.0, dtype=torch.float32, device=dev)
            image = pack_image(rgb, "hwc", mask=m, background=colour)
        return {"render": image,
                "diffuse": pack_image(pbr["diffuse_rgb"].reshape(h, w, 3).contiguous(), "hwc", srgb=gamma),
                "specular": pack_image(pbr["specular_rgb"].reshape(h, w, 3).contiguous(), "hwc", srgb=gamma)}


def relight_views_to_disk(gaussians, views, out_dir, light, metallic=False, gamma=False, background="black", mask="normal", png="host"):
    """out_dir/{render, diffuse, specular}/<stem>.png for every view and out_dir/envmap.png (the light's lat-long image, as
    render_views_to_disk writes it).  `view.image_name` gives the stem (default: the view's index, five digits).  `png`: "host" or
    "device", as render_views_to_disk.  -> the number of views written."""
    from gs2m_png import Writer
    from gs2m_render import pack_image
    _check(light, background, mask)
    writer = Writer(png)
    out_dir = str(out_dir)
    for sub in ("render", "diffuse", "specular"):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    with torch.no_grad():
        light.cubemap.build_mips()
        writer.put(pack_image(light.cubemap.export_envmap(return_img=True).contiguous(), "hwc"), os.path.join(out_dir, "envmap.png"))
        writer.flush()
    for k, view in enumerate(views):
        if getattr(view, "image_name", None) is None:
            view.image_name = f"{k:05d}.png"
        stem = view.image_name.rsplit(".", 1)[0]
        for sub, image in shade_view(gaussians, view, light, metallic, gamma, background, mask).items():
            writer.put(image, os.path.join(out_dir, sub, stem + ".png"))
        writer.flush()
    return len(views)


def light_turntable_to_disk(gaussians, view, out_dir, image, n, res=512, samples=None, angle=0.0, exposure=0.0, metallic=False, gamma=False,
                            background="black", mask="normal", png="host"):
    """out_dir/000.png ... : `view` under `n` rotations of the light, frame k at `angle` + 2 pi k / n radians; `image` is the (Hs, Ws, 3)
    source, converted anew for every frame."""
    from gs2m_envmap import EnvLight
    from gs2m_png import Writer
    n = int(n)
    if n < 1:
        raise ValueError(f"gs2m_relight: {n} turntable frames")
    writer = Writer(png)
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    for k in range(n):
        light = EnvLight.from_image(image, res, samples, angle + 2.0 * math.pi * k / n, exposure)
        writer.put(shade_view(gaussians, view, light, metallic, gamma, background, mask)["render"], os.path.join(out_dir, f"{k:03d}.png"))
        writer.flush()
    return n


# ---- command line -------------------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Relight a trained material model (its point_cloud.ply carries albedo, roughness and metallic) with "
                                             "a Radiance .hdr environment map: PBR renders and their diffuse and specular parts per view.")
    ap.add_argument("--ply", required=True, help="the model's point_cloud.ply")
    ap.add_argument("--source_path", "--source-path", "-s", required=True, help="COLMAP-format dataset (NeRF-synthetic with --blender)")
    ap.add_argument("--model_path", "-m", required=True, help="the images go to MODEL/<split>/<label>_<iteration>/relight/<envmap stem>/")
    ap.add_argument("--envmap", required=True, help="lat-long Radiance file (.hdr, 32-bit_rle_rgbe, -Y H +X W)")
    ap.add_argument("--env-res", type=int, default=512, help="cube-map resolution: a power of two >= 64")
    ap.add_argument("--env-samples", type=int, default=None, help="S x S taps per texel, 1 .. 16 (default: one per source pixel or finer)")
    ap.add_argument("--env-rotation", type=float, default=0.0, help="degrees about +y")
    ap.add_argument("--exposure", type=float, default=0.0, help="stops: the radiance is scaled by 2^EV")
    ap.add_argument("--metallic", action="store_true", help="shade with the model's metallic map (default: estimated from the roughness)")
    ap.add_argument("--gamma", action="store_true", help="linear_to_srgb on the shaded images")
    ap.add_argument("--background", choices=BACKGROUNDS, default="black", help="outside the mask: the environment along the view ray, black or white")
    ap.add_argument("--light-turntable", type=int, default=0, metavar="N", help="also render the split's first view under N rotations of the light")
    ap.add_argument("--label", default="ours", type=str)
    ap.add_argument("--iteration", default=-1, type=int, help="default: the N of an .../iteration_N/... in --ply")
    ap.add_argument("--resolution", "-r", type=int, default=1)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--skip_train", action="store_true")
    ap.add_argument("--skip_test", action="store_true")
    ap.add_argument("--blender", action="store_true", help="NeRF-synthetic dataset: test split only, composed by the images' alpha masks")
    from gs2m_ingest import add_ingest_arguments
    add_ingest_arguments(ap)
    from gs2m_png import add_png_argument
    add_png_argument(ap)
    a = ap.parse_args(argv)
    if a.iteration < 0:
        m = re.search(r"iteration_(\d+)", a.ply)
        if m is None:
            ap.error("--iteration is needed: --ply names no iteration_N directory")
        a.iteration = int(m.group(1))
    if a.env_res < MIN_RES or a.env_res & (a.env_res - 1):
        ap.error(f"--env-res must be a power of two >= {MIN_RES}")
    if a.light_turntable < 0:
        ap.error("--light-turntable takes a number of frames")
    if a.blender:
        a.skip_train, a.skip_test = True, False
    return a


def main(argv=None):
    a = parse_args(argv)
    import gs2m_render as GR
    import gs2m_train as T
    from gs2m_envmap import EnvLight, read_hdr
    from gs2m_model import GaussianModel
    model = GaussianModel(a.sh_degree)
    model.load_ply(a.ply)
    image = read_hdr(a.envmap, "cuda")
    angle = math.radians(a.env_rotation)
    light = EnvLight.from_image(image, a.env_res, a.env_samples, angle, a.exposure)
    splits = {}
    if a.blender:
        cams, _, _, _, _ = T.load_blender_dataset(a.source_path, "transforms_test.json")
        for cam, alpha in zip(cams, GR._blender_alpha(a.source_path, "transforms_test.json", "cuda")):
            cam.alpha_mask = alpha
        splits["test"] = cams
    else:
        from gs2m_ingest import ingest_keywords
        cams, _, _, _, _ = T.load_colmap_dataset(a.source_path, resolution=a.resolution, **ingest_keywords(a))
        if not a.skip_train:
            splits["train"] = cams
        if not a.skip_test:  # every 8th image, as gs2m_render.py
            splits["test"] = cams[::8]
    stem = os.path.splitext(os.path.basename(a.envmap))[0]
    shading = dict(metallic=a.metallic, gamma=a.gamma, background=a.background, mask="alpha" if a.blender else "normal",
                   png="device" if a.device_png else "host")
    for split, cams in splits.items():
        if not cams:
            print(f"[!] No views to relight in {split} set")
            continue
        for k, cam in enumerate(cams):
            if getattr(cam, "image_name", None) is None:
                cam.image_name = f"{k:05d}.png"
        out_dir = os.path.join(a.model_path, split, f"{a.label}_{a.iteration}", "relight", stem)
        relight_views_to_disk(model, cams, out_dir, light, **shading)
        print(f"[>] {len(cams)} views -> {out_dir}")
        if a.light_turntable:
            light_turntable_to_disk(model, cams[0], os.path.join(out_dir, "turntable"), image, a.light_turntable, a.env_res, a.env_samples, angle,
                                    a.exposure, **shading)
            print(f"[>] {a.light_turntable} light rotations -> {os.path.join(out_dir, 'turntable')}")


if __name__ == "__main__":
    main()
