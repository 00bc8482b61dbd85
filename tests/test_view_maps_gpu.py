"""csrc/view_maps.hip through gs2m_render.py (include/gs2m_maps.h): the radix select bit for bit against a
sort, the depth image byte for byte against the reference's decoded PNG (tests/golden/ref_view_maps.npz) and the numpy
restatement tests/view_maps_ref.py, the packing kernel byte for byte where the arithmetic is pinned and by the boundary rule
where it is not (pow, sqrt, the 3x3 product), and render_views_to_disk end to end into the tree gs2m_metrics reads.

The sizes are the smallest at which the kernels can go wrong: below, at and above a workgroup (255, 256, 257), several
workgroups (4097), the golden 37 x 53 (1961 pixels: no multiple of four, so the RGB kernel's byte tail runs), and one
1200 x 1600 select (more than one round of the grid)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import view_maps_ref as VR

pytestmark = pytest.mark.gpu

import gs2m_native as N  # noqa: E402
import gs2m_render as GR  # noqa: E402


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(x):
    return np.asarray(x, dtype=np.float32).reshape(-1).view(np.uint32)


# ---- order statistics --------------------------------------------------------------------------------------------------------

def _values(kind, n, rng):
    if kind == "random":
        return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    if kind == "equal":
        return np.full(n, 2.5, np.float32)
    if kind == "two":  # two values: every rank lies inside a run of ties
        return rng.choice(np.array([1.25, 7.0], np.float32), n, p=[0.6, 0.4])
    if kind == "low_byte":  # the keys differ in the last digit only: the fourth pass decides
        return (np.uint32(0x40490F00) | rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    if kind == "high_byte":  # ... in the first digit only (both signs, every exponent finite: bit 23 is 0)
        return ((rng.integers(0, 256, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00345678)).view(np.float32)
    if kind == "signed_zeros":
        return rng.choice(np.array([0.0, -0.0, 1.5, -1.5, 1e-3, -1e-3], np.float32), n)
    if kind == "denormals":
        return ((rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)) | rng.integers(1, 1 << 23, n).astype(np.uint32)).view(np.float32)
    raise KeyError(kind)


def _ranks(n):
    lo0, lo1, _ = VR.percentile_plan(n, 1)
    hi0, hi1, _ = VR.percentile_plan(n, 99)
    return [0, n - 1, lo0, lo1, hi0, hi1, lo0]  # the ends, the percentile ranks, one rank twice


def _check_select(x, ranks):
    got, nonfinite = GR.order_stats(_dev(x), ranks)
    got = got.cpu().numpy()
    ref = np.sort(x.reshape(-1))[ranks]
    exact, bad = VR.order_stats(x, ranks)
    print(f"n {x.size} ranks {ranks}: {got.tolist()} / {ref.tolist()}")
    assert int(nonfinite.item()) == bad
    # np.sort, bit for bit.  numpy calls -0.0 and +0.0 equal and leaves their order inside a run of zeros to its algorithm (it
    # differs between sizes and between sort and partition), so at a rank that holds a zero the VALUE is compared with np.sort
    # and the bits with the sort of the integer keys, where -0.0 comes first
    assert np.array_equal(got, ref)
    assert np.array_equal(_bits(got)[ref != 0], _bits(ref)[ref != 0])
    assert np.array_equal(_bits(got), _bits(exact))


KINDS = ("random", "equal", "two", "low_byte", "high_byte", "signed_zeros", "denormals")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097, 37 * 53])
def test_order_stats_match_a_sort(n, kind):
    x = _values(kind, n, np.random.default_rng(1000 * n + len(kind)))
    if kind != "signed_zeros":
        assert not (x == 0).any()  # np.sort has one answer here: the comparison below is bit for bit against it
    _check_select(x, _ranks(n))


def test_order_stats_full_size_and_determinism():
    n = 1200 * 1600
    rng = np.random.default_rng(7)
    x = (3.0 + rng.random(n) * 2.0).astype(np.float32)
    x[rng.random(n) < 0.4] = 0.0  # a masked depth map: a long run of ties
    _check_select(x, _ranks(n) + [n // 2])
    d = _dev(x)
    a, b = GR.order_stats(d, _ranks(n)), GR.order_stats(d, _ranks(n))
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_non_finite_values_are_counted_and_refused():
    x = np.linspace(1.0, 2.0, 37 * 53).astype(np.float32)
    x[100] = np.nan
    got, nonfinite = GR.order_stats(_dev(x), [0, 5])
    assert int(nonfinite.item()) == 1 and np.array_equal(got.cpu().numpy(), np.sort(x)[[0, 5]])
    x[7], x[9] = np.inf, -np.inf
    got, nonfinite = GR.order_stats(_dev(x), [0, x.size - 1, x.size - 2])
    assert int(nonfinite.item()) == 3
    got = got.cpu().numpy()
    assert got[0] == -np.inf and np.isnan(got[1]) and got[2] == np.inf  # NaN last, as numpy sorts
    with pytest.raises(ValueError, match="non-finite"):
        GR.depth_image(_dev(x.reshape(37, 53)))


# ---- depth image -------------------------------------------------------------------------------------------------------------

GOLDEN_DEPTHS = tuple(f"{kind}{tag}" for tag in ("37x53", "48x64") for kind in ("", "half_", "const_")) + ("1x1",)


@pytest.mark.parametrize("name", GOLDEN_DEPTHS)
def test_depth_image_is_the_reference_png(name):
    g = VR.golden()
    got = GR.depth_image(_dev(g[f"depth_{name}"])).cpu().numpy()
    assert np.array_equal(got, g[f"depth_{name}_png"]) and np.array_equal(got, VR.depth_image(g[f"depth_{name}"]))


@pytest.mark.parametrize("kind", ["map", "half", "const"])
def test_depth_image_64x96(kind):
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:64, 0:96].astype(np.float32)
    d = (2.0 + 0.03 * x + 0.02 * y + 0.05 * rng.standard_normal((64, 96))).astype(np.float32)
    if kind == "half":
        d[rng.random((64, 96)) < 0.5] = 0.0
    if kind == "const":
        d[:] = 0.75
    dd = _dev(d)
    got = GR.depth_image(dd)
    assert np.array_equal(got.cpu().numpy(), VR.depth_image(d))
    assert torch.equal(got, GR.depth_image(dd))  # two calls, the same bytes
    if kind == "const":
        assert (got.cpu().numpy() == np.append(VR.magma_table()[0], 255)).all()


# ---- image packing -----------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (3, 5), (37, 53), (64, 96)]


def _source(c, h, w, rng, lo=-0.2, hi=1.2):
    s = (lo + (hi - lo) * rng.random((c, h, w))).astype(np.float32)
    k = (np.arange(s.size) % 256).astype(np.float32) / np.float32(255.0)  # k / 255: where the truncation steps
    flat = s.reshape(-1)
    flat[::3] = k[::3]
    return s


def _laid(s, layout):
    return s if layout == "chw" else np.ascontiguousarray(s.transpose(1, 2, 0))


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack_pinned_modes_are_byte_exact(shape, layout):
    h, w = shape
    rng = np.random.default_rng(100 * h + w)
    alpha = (rng.random((1, h, w)) * (rng.random((1, h, w)) > 0.3)).astype(np.float32)
    mask = (rng.random((1, h, w)) > 0.5).astype(np.float32)
    bg = np.array([1.0, 0.25, 0.0], np.float32)
    for c in (3, 1):
        wide, unit = _laid(_source(c, h, w, rng), layout), _laid(_source(c, h, w, rng, 0.0, 1.0), layout)
        cases = [("round", wide, dict()),  # save_image: the clamp is part of it
                 ("round4", wide, dict(channels=4)),
                 ("trunc", unit, dict(quant="trunc")),  # map_to_rgba is defined on [0, 1]
                 ("trunc+alpha", unit, dict(quant="trunc", alpha=alpha)),
                 ("round+alpha", wide, dict(alpha=alpha)),
                 ("compose", wide, dict(mask=mask, background=bg)),
                 ("saturate", wide, dict(quant="trunc"))]
        for name, src, kw in cases:
            dkw = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
            got = GR.pack_image(_dev(src), layout, **dkw)
            ref = VR.pack_image(src, layout, **kw)
            assert got.shape == ref.shape and np.array_equal(got.cpu().numpy(), ref), (name, c)
            assert torch.equal(got, GR.pack_image(_dev(src), layout, **dkw)), (name, c)
    # ROUND is gs2m_metrics.quantise
    import gs2m_metrics as GM
    src = _dev(_source(3, h, w, rng))
    assert torch.equal(GR.pack_image(src), GM.quantise(src))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack_tail_and_unaligned_output(shape):
    """the RGB kernel writes three words per four pixels: the last one to three pixels, and every pixel of an output that is
    not word aligned, go out as bytes; nothing beyond the image is written"""
    h, w = shape
    rng = np.random.default_rng(h + w)
    src = _source(3, h, w, rng)
    alpha = rng.random((1, h, w)).astype(np.float32)
    for ch, kw in ((3, {}), (4, {"alpha": alpha})):
        ref = VR.pack_image(src, **kw)
        for off in (4, 5, 6, 7):
            buf = torch.full((h * w * ch + 16,), 0xAB, dtype=torch.uint8, device="cuda")
            out = buf[off:off + h * w * ch].view(h, w, ch)
            assert out.data_ptr() % 4 == off % 4
            GR.pack_image(_dev(src), out=out, **{k: _dev(v) for k, v in kw.items()})
            host = buf.cpu().numpy()
            assert np.array_equal(host[off:off + h * w * ch].reshape(h, w, ch), ref), (ch, off)
            assert (host[:off] == 0xAB).all() and (host[off + h * w * ch:] == 0xAB).all(), (ch, off)


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack_srgb_and_normal_by_the_boundary_rule(shape, layout):
    h, w = shape
    rng = np.random.default_rng(7 * h + w)
    alpha = rng.random((1, h, w)).astype(np.float32)
    lin = _source(3, h, w, rng, 0.0, 1.3)
    lin.reshape(-1)[1::5] *= np.float32(0.004)  # both branches of the transfer
    nrm = (rng.standard_normal((3, h, w)) * rng.uniform(0.01, 3.0, (1, h, w))).astype(np.float32)
    nrm[:, 0, 0] = 0.0
    rot = np.linalg.qr(rng.standard_normal((3, 3)))[0].astype(np.float32)
    for name, src, kw in (("srgb", lin, dict(srgb=True)), ("normal world", nrm, dict(normal=True)),
                          ("normal view", nrm, dict(normal=True, rot=rot))):
        for quant, a in (("round", None), ("trunc", alpha)):
            s = _laid(src, layout)
            got = GR.pack_image(_dev(s), layout, quant, alpha=None if a is None else _dev(a),
                                **{k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
            values = VR.pack_values(s, layout, **kw)
            differ = VR.assert_bytes_close(got.cpu().numpy(), VR.pack_image(s, layout, quant, alpha=a, **kw), values, quant, f"{name} {quant}")
            print(f"{name} {quant} {h}x{w} {layout}: {differ} of {3 * h * w} bytes differ from the restatement")


@pytest.mark.parametrize("tag", ["37x53", "48x64"])
def test_pack_normal_against_the_reference(tag):
    g = VR.golden()
    n, alpha, rot = _dev(g[f"normal_{tag}"]), _dev(g[f"alpha_{tag}"]), _dev(g[f"wvt_{tag}"][:3, :3])
    for space, r in (("view", rot), ("world", None)):
        ref = g[f"normal_{tag}_{space}"].transpose(1, 2, 0)  # convert_normal_for_save's own values
        got = GR.pack_image(n, normal=True, rot=r).cpu().numpy()
        print(f"normal {space} {tag}:", VR.assert_bytes_close(got, VR.quant_round(ref), ref, "round", f"normal {space} {tag}"), "bytes differ")
    got = GR.pack_image(n, quant="trunc", alpha=alpha, normal=True, rot=rot).cpu().numpy()
    VR.assert_bytes_close(got, g[f"normal_{tag}_view_rgba"], g[f"normal_{tag}_view"].transpose(1, 2, 0), "trunc", f"normal rgba {tag}")
    # and map_to_rgba itself, byte for byte
    for name in ("map3", "map1"):
        got = GR.pack_image(_dev(g[f"{name}_{tag}"]), quant="trunc", alpha=alpha).cpu().numpy()
        assert np.array_equal(got, g[f"{name}_{tag}_rgba"]), name


# ---- invalid arguments -------------------------------------------------------------------------------------------------------

def test_invalid_arguments_launch_and_write_nothing():
    L, st = N.lib(), N.stream_ptr()
    n, h, w = 64, 4, 6
    x = torch.rand(n, device="cuda")
    nbytes = C.c_longlong()
    assert L.gs2m_order_stats_workspace_bytes(n, 2, C.byref(nbytes)) == 0
    ws = torch.full((nbytes.value // 8 + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    out = torch.full((8,), -7.0, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ranks = (C.c_longlong * 2)(0, n - 1)
    good = dict(n=n, x=x.data_ptr(), k=2, ranks=ranks, ws=ws.data_ptr(), ws_bytes=nbytes.value, out=out.data_ptr(), cnt=cnt.data_ptr())
    bad = [dict(n=0), dict(n=2 ** 31), dict(k=0), dict(k=9), dict(ranks=(C.c_longlong * 2)(0, n)), dict(ranks=(C.c_longlong * 2)(-1, 0)),
           dict(x=None), dict(ranks=None), dict(ws=None), dict(ws=ws.data_ptr() + 4), dict(ws_bytes=nbytes.value - 1), dict(out=None),
           dict(cnt=None)]
    for change in bad:
        a = {**good, **change}
        rc = L.gs2m_order_stats(a["n"], a["x"], a["k"], a["ranks"], a["ws"], a["ws_bytes"], a["out"], a["cnt"], st)
        assert rc == -1, change
    depth = torch.rand(h, w, device="cuda")
    stats = torch.tensor([0.1, 0.2, 0.8, 0.9], device="cuda")
    rgba = torch.full((h * w * 4 + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    good = dict(h=h, w=w, depth=depth.data_ptr(), stats=stats.data_ptr(), t_lo=0.25, t_hi=0.75, rgba=rgba.data_ptr())
    for change in [dict(h=0), dict(w=0), dict(h=65536, w=65536), dict(depth=None), dict(stats=None), dict(rgba=None),
                   dict(rgba=rgba.data_ptr() + 1), dict(t_lo=-0.5), dict(t_hi=1.5), dict(t_lo=float("nan"))]:
        a = {**good, **change}
        assert L.gs2m_depth_colorize(a["h"], a["w"], a["depth"], a["stats"], a["t_lo"], a["t_hi"], a["rgba"], st) == -1, change
    src = torch.rand(3, h, w, device="cuda")
    plane = torch.rand(h, w, device="cuda")
    bg = torch.zeros(3, device="cuda")
    rot = torch.eye(3, device="cuda")
    packed = torch.full((h * w * 4 + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    good = dict(h=h, w=w, c=3, layout=0, src=src.data_ptr(), alpha=None, mask=None, bg=None, rot=None, flags=0, ch=3, out=packed.data_ptr())
    for change in [dict(h=0), dict(w=-1), dict(h=65536, w=65536), dict(c=2), dict(c=4), dict(layout=2), dict(ch=2), dict(ch=5), dict(flags=8),
                   dict(flags=GR.NORMAL, c=1), dict(rot=rot.data_ptr()), dict(mask=plane.data_ptr()), dict(alpha=plane.data_ptr()),
                   dict(src=None), dict(out=None)]:
        a = {**good, **change}
        rc = L.gs2m_pack_image(a["h"], a["w"], a["c"], a["layout"], a["src"], a["alpha"], a["mask"], a["bg"], a["rot"], a["flags"], a["ch"], a["out"], st)
        assert rc == -1, change
    torch.cuda.synchronize()
    assert (ws == 0x5A5A5A5A5A5A5A5A).all() and (out == -7.0).all() and (cnt == -7).all()
    assert (rgba == 0xAB).all() and (packed == 0xAB).all()
    # the same buffers, valid: the calls do work (the sentinels above were not spared by a dead library)
    assert L.gs2m_order_stats(n, x.data_ptr(), 2, ranks, ws.data_ptr(), nbytes.value, out.data_ptr(), cnt.data_ptr(), st) == 0
    assert L.gs2m_pack_image(h, w, 3, 0, src.data_ptr(), None, plane.data_ptr(), bg.data_ptr(), None, 0, 3, packed.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert out[0] == x.min() and out[1] == x.max() and int(cnt) == 0 and (out[2:] == -7.0).all()
    assert (packed[h * w * 3:] == 0xAB).all()
    with pytest.raises(ValueError):
        GR.order_stats(x, [n])
    with pytest.raises(ValueError):
        GR.order_stats(x, list(range(9)))


# ---- end to end --------------------------------------------------------------------------------------------------------------

def _truth_and_views(n_true, n_views, W, H):
    """a synthetic surface and "photographs" of it: the truth's own rendering, tinted and with sensor noise"""
    import gs2m_synth as S
    from gaussian_renderer import render
    from gs2m_scene import Camera, GaussianParams, PipelineParams, inverse_sigmoid
    sc = S.make_surface_scene(n_true, seed=0)
    t = {k: v.cuda() for k, v in sc.items()}
    truth = GaussianParams(t["points"], t["shs"][:, :1].contiguous(), t["shs"][:, 1:].contiguous(), torch.log(t["scales"]),
                           t["rotations"], inverse_sigmoid(t["opacities"]),
                           *(inverse_sigmoid(torch.full((n_true, c), 0.5, device="cuda")) for c in (3, 1, 1)))
    views = [Camera(c, "cuda") for c in S.orbit_cameras(n_views, W, H, radius=6.0, centre=(0.0, -0.8, 6.0), fx=1.1 * W)]
    gen = torch.Generator().manual_seed(3)
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        for v in views:
            out = render(v, truth, PipelineParams(), bg, material_stage=True)
            v.gt_image = (out["render"] * 0.9 + 0.04 + 0.03 * torch.randn(3, H, W, generator=gen).cuda()).clamp(0, 1)
            v.alpha_mask = (out["alpha_map"].reshape(1, H, W) > 0.5).float()
    return truth, views


W, H = 64, 48


@pytest.fixture(scope="module")
def scene():
    return _truth_and_views(4000, 2, W, H)


def test_render_views_to_disk_writes_the_tree_metrics_reads(tmp_path, scene):
    from PIL import Image
    import gs2m_metrics as GM
    truth, views = scene
    bg = torch.zeros(3, device="cuda")
    model = tmp_path / "model"
    out_dir = model / "test" / "ours_7"
    (model).mkdir()
    (model / "points.json").write_text(json.dumps({"ours_3": 12}))
    depths = GR.render_views_to_disk(truth, views, str(out_dir), bg)
    assert tuple(depths.shape) == (2, H, W) and depths.is_cuda and depths.dtype == torch.float32
    assert sorted(os.listdir(out_dir)) == ["depth", "gt", "normal", "render"]
    for sub, mode in (("render", "RGB"), ("gt", "RGB"), ("normal", "RGB"), ("depth", "RGBA")):
        assert sorted(os.listdir(out_dir / sub)) == ["00000.png", "00001.png"], sub
        for f in ("00000.png", "00001.png"):
            with Image.open(out_dir / sub / f) as img:
                assert img.mode == mode and img.size == (W, H), (sub, f, img.mode, img.size)
    assert json.loads((model / "points.json").read_text()) == {"ours_3": 12, "ours_7": 4000}
    # the depth image is save_depth_map of the returned depth; its alpha is 255
    for k in range(2):
        png = np.asarray(Image.open(out_dir / "depth" / f"{k:05d}.png"))
        assert np.array_equal(png, VR.depth_image(depths[k].cpu().numpy()))
    # the tree scores as the views do
    want = GM.score_views(truth, views, bg)
    got = GM.evaluate(str(model), "test", "ours_7")
    assert got == {"ssim": want["ssim"].mean().item(), "psnr": want["psnr"].mean().item(), "n_images": 2}
    # white background: the normal image carries the alpha mask, the ground truth is white outside it
    white = torch.ones(3, device="cuda")
    GR.render_views_to_disk(truth, views[:1], str(model / "train" / "ours_7"), white, white_background=True, normal_world=True)
    with Image.open(model / "train" / "ours_7" / "normal" / "00000.png") as img:
        assert img.mode == "RGBA"
        a = np.asarray(img)[..., 3]
    inside = views[0].alpha_mask[0].cpu().numpy() > 0.5
    assert inside.any() and (~inside).any() and (a[inside] == 255).all() and (a[~inside] == 0).all()
    gt = np.asarray(Image.open(model / "train" / "ours_7" / "gt" / "00000.png"))
    assert gt.shape == (H, W, 3) and (gt[~inside] == 255).all()


def test_material_branch_writes_the_brdf_maps(tmp_path, scene):
    """with a light: the PBR image, the five BRDF maps and envmap.png; black background -> RGB through save_image's rounding"""
    from PIL import Image
    from gaussian_renderer import render
    from gs2m_scene import PipelineParams
    from gs2m_train import _Lighting
    truth, views = scene
    light = _Lighting(64, 0.01, "cuda")
    bg = torch.zeros(3, device="cuda")
    out_dir = tmp_path / "model" / "test" / "pbr_1"
    GR.render_views_to_disk(truth, views[:1], str(out_dir), bg, light=light, gamma=True)
    assert sorted(os.listdir(out_dir)) == ["albedo", "depth", "diffuse", "envmap.png", "gt", "metallic", "normal", "render", "roughness", "specular"]
    for sub in ("render", "albedo", "roughness", "metallic", "diffuse", "specular"):
        with Image.open(out_dir / sub / "00000.png") as img:
            assert img.mode == "RGB" and img.size == (W, H), (sub, img.mode, img.size)
    with Image.open(out_dir / "envmap.png") as img:
        assert img.mode == "RGB" and img.size == (1024, 512)
    rough = np.asarray(Image.open(out_dir / "roughness" / "00000.png"))
    assert (rough[..., 0] == rough[..., 1]).all() and (rough[..., 0] == rough[..., 2]).all() and rough.std() > 0
    with torch.no_grad():
        pkg = render(views[0], truth, PipelineParams(), bg, material_stage=True)
    assert np.array_equal(np.asarray(Image.open(out_dir / "albedo" / "00000.png")), VR.pack_image(pkg["albedo_map"].cpu().numpy()))
    # white background: RGBA through map_to_rgba's truncation, the view's alpha mask in the fourth byte
    GR.render_views_to_disk(truth, views[:1], str(tmp_path / "model" / "test" / "pbr_2"), torch.ones(3, device="cuda"), white_background=True, light=light)
    alpha = views[0].alpha_mask.cpu().numpy()
    got = np.asarray(Image.open(tmp_path / "model" / "test" / "pbr_2" / "albedo" / "00000.png"))
    assert np.array_equal(got, VR.pack_image(pkg["albedo_map"].cpu().numpy(), quant="trunc", alpha=alpha))
    assert json.loads((tmp_path / "model" / "points.json").read_text()) == {"pbr_1": 4000, "pbr_2": 4000}


def test_command_line_split_with_mesh(tmp_path, scene):
    """render.py --extract_mesh for one split, as the command line runs it: the images, then the mesh from the returned depths"""
    import gs2m_mesh as M
    truth, views = scene
    a, bounds = GR.parse_args(["--ply", "unused.ply", "-s", "unused", "-m", str(tmp_path / "model"), "--iteration", "9", "--label", "run", "--extract_mesh",
                               "--max_depth", "12", "--voxel_size", "0.04", "--filter_depth"])
    GR.render_split(a, "train", truth, views, [v.gt_image for v in views], 6.0, torch.zeros(3, device="cuda"), bounds)
    out_dir = tmp_path / "model" / "train" / "run_9"
    assert sorted(os.listdir(out_dir)) == ["depth", "gt", "mesh", "normal", "render"]
    assert sorted(os.listdir(out_dir / "mesh")) == ["config.json", "tsdf_mesh.ply", "tsdf_post.ply"]
    assert json.loads((out_dir / "mesh" / "config.json").read_text()) == {"max_depth": 12.0, "voxel_size": 0.04, "sdf_trunc": 0.16}
    mesh, post = M.read_mesh(out_dir / "mesh" / "tsdf_mesh.ply"), M.read_mesh(out_dir / "mesh" / "tsdf_post.ply")
    assert len(mesh.triangles) > 100 and 0 < len(post.triangles) <= len(mesh.triangles)
    assert json.loads((tmp_path / "model" / "points.json").read_text()) == {"run_9": 4000}
