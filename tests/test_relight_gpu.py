"""Relighting end to end (gs2m_relight.py): the tree it writes, its images against a pbr_render the test calls itself,
the light turntable, the command line on an exported COLMAP scene, and gs2m_render's output untouched by it."""
import filecmp
import os

import numpy as np
import pytest
import torch

import envmap_ref as ER
import gs2m_envmap as E
import gs2m_relight as RL
import gs2m_render as GR

pytestmark = pytest.mark.gpu

W, H, RES = 64, 48, 64  # 64: the smallest light CubemapLight.build_mips and the shading take (three specular levels: 64, 32, 16)


def _truth_and_views(n_true, n_views):
    import gs2m_synth as S
    from gaussian_renderer import render
    from gs2m_scene import Camera, GaussianParams, PipelineParams, inverse_sigmoid
    sc = S.make_surface_scene(n_true, seed=0)
    t = {k: v.cuda() for k, v in sc.items()}
    gen = torch.Generator().manual_seed(1)
    material = [inverse_sigmoid(torch.rand(n_true, c, generator=gen).clamp(0.05, 0.95).cuda()) for c in (3, 1, 1)]
    truth = GaussianParams(t["points"], t["shs"][:, :1].contiguous(), t["shs"][:, 1:].contiguous(), torch.log(t["scales"]),
                           t["rotations"], inverse_sigmoid(t["opacities"]), *material)
    views = [Camera(c, "cuda") for c in S.orbit_cameras(n_views, W, H, radius=6.0, centre=(0.0, -0.8, 6.0), fx=1.1 * W)]
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        for v in views:
            out = render(v, truth, PipelineParams(), bg, material_stage=True)
            v.gt_image = out["render"].clamp(0, 1)
            v.alpha_mask = (out["alpha_map"].reshape(1, H, W) > 0.5).float()
    return truth, views


@pytest.fixture(scope="module")
def scene():
    return _truth_and_views(4000, 2)


@pytest.fixture(scope="module")
def source():
    """a 32 x 16 environment: a gradient, a warm patch, one bright small light; as the RGBE pixels a file holds and their decoded values"""
    d = ER.latlong_dirs(16, 32)
    img = 0.3 + 0.4 * (d[..., 1:2] + 1) * np.array([0.6, 0.8, 1.0]) + 0.5 * np.maximum(d[..., 0:1], 0) * np.array([1.0, 0.7, 0.4])
    img[5, 20] = (40.0, 36.0, 30.0)
    rgbe = ER.float_to_rgbe(img.astype(np.float32))
    return rgbe, ER.rgbe_to_float(rgbe)


def _write_hdr(path, rgbe):
    h, w, _ = rgbe.shape
    path.write_bytes(ER.hdr_file(ER.write_pixels(rgbe, "mixed"), w, h))
    return str(path)


def _png(path):
    from PIL import Image
    with Image.open(path) as img:
        return np.asarray(img).copy()


def test_relight_views_to_disk_writes_the_tree_and_the_images_of_pbr_render(tmp_path, scene, source):
    import torch.nn.functional as F
    import nvdiffrast.torch as dr
    from gaussian_renderer import render
    from gs2m_scene import PipelineParams
    from pbr import linear_to_srgb, pbr_render
    truth, views = scene
    light = E.EnvLight(torch.from_numpy(ER.latlong_to_cubemap(source[1], RES, 2).astype(np.float32)).cuda())  # the restatement's cube map
    for background, mask, gamma, metallic in (("black", "normal", False, False), ("white", "normal", True, False), ("env", "normal", False, True),
                                             ("env", "alpha", True, False), ("white", "alpha", False, False)):
        out_dir = tmp_path / f"{background}_{mask}"
        assert RL.relight_views_to_disk(truth, views, str(out_dir), light, metallic=metallic, gamma=gamma, background=background, mask=mask) == 2
        assert sorted(os.listdir(out_dir)) == ["diffuse", "envmap.png", "render", "specular"]
        for sub in ("render", "diffuse", "specular"):
            assert sorted(os.listdir(out_dir / sub)) == ["00000.png", "00001.png"]
        assert _png(out_dir / "envmap.png").shape == (512, 1024, 3)
        for k, view in enumerate(views):
            with torch.no_grad():
                pkg = render(view, truth, PipelineParams(), torch.zeros(3, device="cuda"), material_stage=True, blend_metallic=metallic)
                rays = F.normalize(view.get_rays().view(-1, 3), p=2, dim=-1)
                pbr = pbr_render(light, view, rays, pkg, metallic, gamma)
                m = (view.alpha_mask if mask == "alpha" else pkg["normal_mask"]).float().reshape(H, W)
                rgb = pbr["render_rgb"].reshape(H, W, 3).contiguous()
                if background == "env":
                    dirs = -F.normalize(-rays @ view.world_view_transform[:3, :3].T, p=2, dim=-1).reshape(1, H, W, 3)
                    env = dr.texture(light.cubemap.base[None], dirs.contiguous(), filter_mode="linear", boundary_mode="cube")[0].clamp(0, 1)
                    env = linear_to_srgb(env) if gamma else env
                    want = GR.pack_image(torch.where(m[..., None] > 0.5, rgb.clamp(0, 1), env).contiguous(), "hwc")
                else:
                    want = GR.pack_image(rgb, "hwc", mask=m.contiguous(), background=torch.full((3,), float(background == "white"), device="cuda"))
                assert (m > 0.5).any() and not (m > 0.5).all()
                got = _png(out_dir / "render" / f"{k:05d}.png")
                assert np.array_equal(got, want.cpu().numpy()), (background, mask, k)
                outside = ~(m > 0.5).cpu().numpy()
                if background == "white":
                    assert (got[outside] == 255).all()
                elif background == "black":
                    assert (got[outside] == 0).all()
                else:
                    assert got[outside].min() > 0  # the environment is nowhere black
                for sub in ("diffuse", "specular"):
                    want = GR.pack_image(pbr[sub + "_rgb"].reshape(H, W, 3).contiguous(), "hwc", srgb=gamma)
                    assert np.array_equal(_png(out_dir / sub / f"{k:05d}.png"), want.cpu().numpy()), (sub, k)
    assert not np.array_equal(_png(tmp_path / "black_normal" / "render" / "00000.png"), _png(tmp_path / "env_normal" / "render" / "00000.png"))
    with pytest.raises(ValueError):
        RL.relight_views_to_disk(truth, views, str(tmp_path / "x"), light, background="sky")
    small = E.EnvLight(torch.from_numpy(ER.latlong_to_cubemap(source[1], 16, 1).astype(np.float32)).cuda())
    with pytest.raises(ValueError, match="three specular levels"):
        RL.relight_views_to_disk(truth, views, str(tmp_path / "y"), small)
    with pytest.raises(ValueError, match="three specular levels"):
        RL.relight_views_to_disk(truth, views, str(tmp_path / "y"), E.EnvLight(torch.ones(6, 32, 32, 3, device="cuda")))
    assert not (tmp_path / "x").exists() and not (tmp_path / "y").exists()


def test_the_light_from_the_file_is_the_restatements_light(tmp_path, scene, source):
    """EnvLight.from_hdr: the .hdr the test writes, decoded and converted on the device, against the restatement's cube map (the conversion's
    tolerance: tests/test_envmap_gpu.py); exposure in stops, the rotation in radians"""
    path = _write_hdr(tmp_path / "studio.hdr", source[0])
    assert np.array_equal(E.read_hdr(path).cpu().numpy(), source[1])
    light = E.EnvLight.from_hdr(path, RES, 2, angle=0.5, exposure=-1.0)
    want = ER.latlong_to_cubemap(source[1], RES, 2, 0.5, 0.5)
    assert ER.relative_distance(light.cubemap.base.cpu().numpy(), want) < 1e-4


def test_light_turntable(tmp_path, scene, source):
    truth, views = scene
    image = torch.from_numpy(source[1]).cuda()
    out = tmp_path / "turntable"
    assert RL.light_turntable_to_disk(truth, views[0], str(out), image, 4, res=RES, samples=2) == 4
    assert sorted(os.listdir(out)) == ["000.png", "001.png", "002.png", "003.png"]
    frames = [_png(out / f"{k:03d}.png") for k in range(4)]
    assert all(f.shape == (H, W, 3) for f in frames) and not np.array_equal(frames[0], frames[2])
    # frame 0 is the unrotated light's render
    RL.relight_views_to_disk(truth, views[:1], str(tmp_path / "still"), E.EnvLight.from_image(image, RES, 2))
    assert np.array_equal(frames[0], _png(tmp_path / "still" / "render" / "00000.png"))


def test_command_line_end_to_end(tmp_path, scene, source):
    import gs2m_train as T
    from gs2m_model import GaussianModel
    truth, _ = scene
    T.export_colmap_dataset(str(tmp_path / "scene"), T.synthetic_scene(4000, 3, W, H, seed=1))
    model = GaussianModel(3)
    model.parameterize((truth._xyz, truth._features_dc, truth._features_rest, truth._scaling, truth._rotation, truth._opacity,
                        truth._albedo, truth._roughness, truth._metallic))
    model.active_sh_degree = 3
    ply = tmp_path / "point_cloud" / "iteration_7" / "point_cloud.ply"
    ply.parent.mkdir(parents=True)
    model.save_ply(str(ply))
    hdr = _write_hdr(tmp_path / "studio.hdr", source[0])
    RL.main(["--ply", str(ply), "-s", str(tmp_path / "scene"), "-m", str(tmp_path / "model"), "--envmap", hdr, "--env-res", str(RES), "--env-samples", "2",
             "--env-rotation", "30", "--exposure", "0.5", "--gamma", "--background", "env", "--light-turntable", "4", "--skip_test"])
    out = tmp_path / "model" / "train" / "ours_7" / "relight" / "studio"
    assert sorted(os.listdir(out)) == ["diffuse", "envmap.png", "render", "specular", "turntable"]
    assert len(os.listdir(out / "render")) == 3 and len(os.listdir(out / "turntable")) == 4
    assert not (tmp_path / "model" / "test").exists()
    stem = sorted(os.listdir(out / "render"))[0]
    assert _png(out / "render" / stem).shape == (H, W, 3) and _png(out / "render" / stem).std() > 0
    assert not np.array_equal(_png(out / "turntable" / "000.png"), _png(out / "turntable" / "002.png"))
    # the same through the GPU's PNG encoder: other file bytes, the same pixels
    RL.main(["--ply", str(ply), "-s", str(tmp_path / "scene"), "-m", str(tmp_path / "model2"), "--envmap", hdr, "--env-res", str(RES), "--env-samples", "2",
             "--env-rotation", "30", "--exposure", "0.5", "--gamma", "--background", "env", "--skip_test", "--device-png"])
    out2 = tmp_path / "model2" / "train" / "ours_7" / "relight" / "studio"
    for sub in ("render", "diffuse", "specular"):
        assert np.array_equal(_png(out2 / sub / stem), _png(out / sub / stem))


def test_gs2m_render_writes_the_same_files_around_a_relight(tmp_path, scene, source):
    """render_views_to_disk before and after the views have been through the relighting: byte-identical trees"""
    truth, views = scene
    bg = torch.zeros(3, device="cuda")
    for v in views:  # as fresh views: nothing cached on them
        for name in ("_render_rays", "_pbr_view_dirs"):
            if hasattr(v, name):
                delattr(v, name)
    GR.render_views_to_disk(truth, views, str(tmp_path / "a" / "test" / "ours_1"), bg)
    light = E.EnvLight.from_image(torch.from_numpy(source[1]).cuda(), RES, 2)
    RL.relight_views_to_disk(truth, views, str(tmp_path / "a" / "test" / "ours_1" / "relight" / "studio"), light, gamma=True, background="env")
    GR.render_views_to_disk(truth, views, str(tmp_path / "b" / "test" / "ours_1"), bg)
    for sub in ("render", "gt", "normal", "depth"):
        names = sorted(os.listdir(tmp_path / "a" / "test" / "ours_1" / sub))
        assert names == ["00000.png", "00001.png"]
        match, mismatch, errors = filecmp.cmpfiles(tmp_path / "a" / "test" / "ours_1" / sub, tmp_path / "b" / "test" / "ours_1" / sub, names, shallow=False)
        assert match == names and not mismatch and not errors, sub
    # and with a light, as the material branch writes them
    GR.render_views_to_disk(truth, views[:1], str(tmp_path / "c" / "test" / "pbr_1"), bg, light=light, gamma=True)
    RL.relight_views_to_disk(truth, views[:1], str(tmp_path / "c" / "test" / "pbr_1" / "relight" / "studio"), light, gamma=True)
    for sub in ("diffuse", "specular", "render"):  # black background, normal mask: the relight images ARE the material branch's
        assert filecmp.cmp(tmp_path / "c" / "test" / "pbr_1" / sub / "00000.png", tmp_path / "c" / "test" / "pbr_1" / "relight" / "studio" / sub / "00000.png",
                           shallow=False), sub
