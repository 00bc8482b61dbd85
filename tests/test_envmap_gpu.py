"""The device side of the environment-map stage (csrc/envmap.hip, gs2m_envmap.py) against the numpy restatement
(tests/envmap_ref.py): the RGBE codec bit for bit, the lat-long -> cube-map conversion against float64 with a tolerance taken from
what fp32 arithmetic costs the restatement itself, its orientation texel by texel, and its convention against export_envmap."""
import numpy as np
import pytest
import torch

import envmap_ref as ER
import gs2m_envmap as E

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- codec ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(1, 1), (7, 3), (8, 3), (9, 2), (130, 3), (300, 3), (4096, 2), (9001, 2)])
def test_decode_is_bit_identical(W, H):
    """RLE, flat and mixed files; e == 0, e == 255 and mantissa 255 among the pixels; 9001: a row that goes through LDS in three chunks,
    with codes that straddle them"""
    for kinds in ("rle", "flat", "mixed"):
        img = ER.sample_rgbe(W, H, seed=W + H)
        px = ER.write_pixels(img, kinds)
        want = ER.decode(px, W, H)
        got = E.decode_hdr(px, W, H).cpu().numpy()
        assert got.shape == (H, W, 3) and np.array_equal(_bits(got), _bits(want)), kinds
    assert W * H < 7 or ((img[..., 3] == 0).any() and (img[..., 3] == 255).any() and (img[..., :3] == 255).any())


def test_decode_covers_every_exponent_and_mantissa():
    m, e = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    img = np.stack([m, (m * 7 + 3) % 256, 255 - m, e], axis=-1).astype(np.uint8)  # (256, 256, 4): subnormals (e < 10) included
    img[(img[..., 0] == 1) & (img[..., 1] == 1) & (img[..., 2] == 1)] = 0
    for kinds in ("rle", "flat"):
        px = ER.write_pixels(img, kinds)
        got = E.decode_hdr(px, 256, 256).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(ER.rgbe_to_float(img)))


def _encode_input():
    rng = np.random.default_rng(5)
    pw = np.ldexp(1.0, np.arange(-110, 128)).astype(np.float32)
    rows = [np.zeros((4, 3), np.float32),
            np.array([[1e-33, 0, 0], [1e-33, 1e-33, 1e-33], [9.9e-33, 0, 0], [1e-32, 0, 0], [1.1e-32, 1e-33, 0]], np.float32),
            np.array([[-1, 2, 3], [np.nan, 1, 0.5], [np.inf, 1, 1], [-np.inf, np.nan, -0.0], [np.inf, np.inf, 3e38], [3.4e38, 1e38, 1]], np.float32),
            np.stack([pw, pw * np.float32(0.5), pw * np.float32(0.3)], axis=-1),
            np.stack([np.nextafter(pw, np.float32(0)), pw * np.float32(0.75), np.nextafter(pw, np.float32(0))], axis=-1),
            (rng.uniform(0.5, 1.0, (4000, 3)) * np.ldexp(1.0, rng.integers(-20, 20, (4000, 1)))).astype(np.float32)]
    x = np.concatenate(rows)
    pad = (-len(x)) % 61
    x = np.concatenate([x, rng.uniform(0, 1, (pad, 3)).astype(np.float32)])
    return x.reshape(-1, 61, 3)


def test_encode_is_byte_identical_and_round_trips(tmp_path):
    x = _encode_input()
    want = ER.float_to_rgbe(x)
    got = E.encode_hdr(torch.from_numpy(x).cuda()).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    path = tmp_path / "x.hdr"
    E.write_hdr(str(path), torch.from_numpy(x).cuda())
    back, info = E.read_hdr(str(path), "cuda", info=True)
    assert info["exposure"] == 1.0 and np.array_equal(_bits(back.cpu().numpy()), _bits(ER.rgbe_to_float(want)))


def test_read_hdr_reads_rle_files_and_names_what_it_refuses(tmp_path):
    img = ER.sample_rgbe(130, 5, seed=2)
    px = ER.write_pixels(img, "mixed")
    path = tmp_path / "a.hdr"
    path.write_bytes(ER.hdr_file(px, 130, 5, magic=b"#?RGBE", lines=(b"FORMAT=32-bit_rle_rgbe", b"EXPOSURE=0.5")))
    image, info = E.read_hdr(str(path), "cuda", info=True)
    assert info["exposure"] == 0.5 and np.array_equal(_bits(image.cpu().numpy()), _bits(ER.rgbe_to_float(img)))
    path.write_bytes(ER.hdr_file(px[:-3], 130, 5))
    with pytest.raises(ValueError, match="truncated") as err:
        E.read_hdr(str(path))
    assert err.value.code == ER.TRUNCATED


# ---- conversion ----------------------------------------------------------------------------------------------------------------

def _convert(src, R, S, angle=0.0, scale=1.0):
    return E.latlong_to_cubemap(torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32)).cuda(), R, S, angle, scale).cpu().numpy()


def test_conversion_against_float64():
    """72 cases: sources 16 x 8, 37 x 19 and 64 x 32 of random positive values times one 1e4 spike, R in {16, 32}, S in {1, 2, 4}, angle in
    {0, 1.0}, scale in {1, 0.25}.  The distance is max |a - b| / max |b| per case, its largest value over the cases the figure.  The
    yardstick is the restatement evaluated in numpy float32 against itself in float64; the device may be at most 4 times that (another
    order of the same sum, other atan2 / acos implementations: small factors).
    Measured: yardstick 4.33e-6, device 4.33e-6 (MI355X; both dominated by the fp32 rounding of u, v beside the spike)."""
    yardstick, device = 0.0, 0.0
    for src, R, S, angle, scale in ER.conversion_cases():
        ref = ER.latlong_to_cubemap(src, R, S, angle, scale)
        yardstick = max(yardstick, ER.relative_distance(ER.latlong_to_cubemap(src, R, S, angle, scale, np.float32), ref))
        got = _convert(src, R, S, angle, scale)
        assert got.shape == (6, R, R, 3) and np.isfinite(got).all()
        device = max(device, ER.relative_distance(got, ref))
    print(f"conversion: fp32 yardstick {yardstick:.3e}, device {device:.3e}")
    assert 0 < yardstick < 1e-4
    assert device <= 4 * yardstick, (device, yardstick)


@pytest.mark.parametrize("S", [1, 2, 3, 4, 16])
def test_constant_source_gives_a_constant_cubemap(S):
    """the weights are normalised: what is left is the rounding of the two sums, (S^2 + 4) 2^-23 relative"""
    for value, scale in ((3.7, 1.0), (0.011, 0.25)):
        got = _convert(np.full((19, 37, 3), value, np.float32), 16, S, 0.3, scale).astype(np.float64)
        want = float(np.float32(value)) * scale
        assert np.abs(got / want - 1).max() <= (S * S + 4) * 2.0 ** -23


ORIENTATION_PIXELS = {"+x": (8, 23), "-x": (8, 7), "+y": (0, 5), "-y": (15, 20), "+z": (8, 29), "-z": (8, 15), "seam left": (7, 0), "seam right": (8, 31)}
FACE = {"+x": 0, "-x": 1, "+y": 2, "-y": 3, "+z": 4, "-z": 5, "seam left": 4, "seam right": 4}


@pytest.mark.parametrize("name", list(ORIENTATION_PIXELS))
def test_orientation_is_exact(name):
    """a source that is zero but for one pixel, S = 1, R = 16: the non-zero texels are exactly the ones whose taps reach the pixel"""
    v, u = ORIENTATION_PIXELS[name]
    src = np.zeros((16, 32, 3), np.float32)
    src[v, u] = (1.0, 2.0, 3.0)
    ref = ER.latlong_to_cubemap(src, 16, 1)
    want = ref[..., 0] > 0
    assert ref[want][:, 0].min() > 1e-3, "a tap weight too small to call in fp32: choose another pixel"
    assert want.sum() >= 1 and want[FACE[name]].any()
    if name in ("+x", "-x", "-z", "+z"):
        assert not want[[f for f in range(6) if f != FACE[name]]].any()
    got = _convert(src, 16, 1)
    assert np.array_equal(got[..., 0] > 0, want)
    assert np.array_equal(got[..., 2] > 0, want)


def _export(cube, res):
    light = E.EnvLight(torch.from_numpy(np.ascontiguousarray(cube, dtype=np.float32)).cuda())
    with torch.no_grad():
        return light.cubemap.export_envmap(res=list(res), return_img=True).cpu().numpy()


def test_convention_against_export_envmap():
    """radiance -> 128 x 64 source -> R = 32 cube map -> export_envmap(res=[32, 64]), compared with the radiance at export_envmap's own
    sample directions.  The bound is the same distance (max |a - b| / max |b|) of the float64 restatement of both steps (the conversion
    and the cube lookup of oracle/texture_oracle.py), times 2.
    Measured: restatement 1.61e-3, device 1.61e-3 (MI355X)."""
    from oracle import texture_oracle as TO
    src = ER.radiance(ER.latlong_dirs(64, 128)).astype(np.float32)
    dirs = ER.export_dirs((32, 64))
    truth = ER.radiance(dirs)
    ref_cube = ER.latlong_to_cubemap(src, 32, 1)
    ref_err = ER.relative_distance(TO.cube_sample([ref_cube], dirs.reshape(-1, 3)).reshape(32, 64, 3), truth)
    assert 0 < ref_err < 5e-3  # the two interpolations of a smooth function; a wrong face or sign is O(1)
    got = _export(_convert(src, 32, E.default_samples(32, 128)), (32, 64))
    err = ER.relative_distance(got, truth)
    print(f"convention: float64 restatement {ref_err:.3e}, device {err:.3e}")
    assert err <= 2 * ref_err, (err, ref_err)


def test_rotation():
    """converting with angle = a is converting a source generated from the radiance turned by a: both are the turned radiance at the texel
    centres up to the conversion's interpolation error, which the float64 restatement measures for each; the two device results may differ
    by twice the sum of the two"""
    a = 0.9
    d = ER.latlong_dirs(64, 128)
    src = ER.radiance(d).astype(np.float32)
    src_turned = ER.radiance(ER.rotate_y(d, -a)).astype(np.float32)
    truth = ER.radiance(ER.rotate_y(ER.texel_dirs(32), -a))
    e1 = ER.relative_distance(ER.latlong_to_cubemap(src, 32, 1, angle=a), truth)
    e2 = ER.relative_distance(ER.latlong_to_cubemap(src_turned, 32, 1), truth)
    assert 0 < e1 < 5e-3 and 0 < e2 < 5e-3
    got1, got2 = _convert(src, 32, 1, angle=a), _convert(src_turned, 32, 1)
    assert ER.relative_distance(got1, got2) <= 2 * (e1 + e2)
    assert ER.relative_distance(got1, truth) <= 2 * e1 and ER.relative_distance(got2, truth) <= 2 * e2
    assert ER.relative_distance(_convert(src, 32, 1), got1) > 20 * (e1 + e2)  # and the angle does something


def test_refusals():
    img = torch.rand(8, 16, 3, device="cuda")
    for res in (24, 8, 0):
        with pytest.raises(ValueError, match="power of two"):
            E.latlong_to_cubemap(img, res)
    for s in (0, 17):
        with pytest.raises(ValueError, match="samples"):
            E.latlong_to_cubemap(img, 16, s)
    with pytest.raises(ValueError, match="2 x 2"):
        E.latlong_to_cubemap(torch.rand(1, 16, 3, device="cuda"), 16)
    with pytest.raises(RuntimeError, match="contiguous"):
        E.latlong_to_cubemap(torch.rand(8, 3, 16, device="cuda").permute(0, 2, 1), 16)
    with pytest.raises(RuntimeError, match="shape"):
        E.latlong_to_cubemap(torch.rand(8, 16, 4, device="cuda"), 16)
    # the library refuses the same by itself (the wrapper's checks are not the only ones): nothing is launched
    import gs2m_native as N
    out = torch.empty(6, 16, 16, 3, device="cuda")
    for hs, ws, R, S in ((8, 16, 24, 1), (8, 16, 8, 1), (8, 16, 16, 0), (8, 16, 16, 17), (1, 16, 16, 1)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            N.launch("gs2m_latlong_to_cubemap", img.device, hs, ws, img.data_ptr(), R, S, 0.0, 1.0, out.data_ptr())


def test_env_light_leaves_the_rng_alone_and_shades():
    torch.manual_seed(7)
    torch.cuda.manual_seed(7)
    a, b = torch.rand(3), torch.rand(3, device="cuda")
    torch.manual_seed(7)
    torch.cuda.manual_seed(7)
    base = torch.full((6, 16, 16, 3), 0.5, device="cuda")
    light = E.EnvLight(base)
    assert torch.equal(torch.rand(3), a) and torch.equal(torch.rand(3, device="cuda"), b)
    assert torch.equal(light.cubemap.base, base) and tuple(light.brdf_lut.shape) == (1, 256, 256, 2) and light.brdf_lut.is_cuda
    with torch.no_grad():
        light.cubemap.build_mips()
    assert len(light.cubemap.specular) == 1 and tuple(light.cubemap.diffuse.shape) == (6, 16, 16, 3)


def test_save_light_hdr_feeds_back_in(tmp_path):
    """a light written as .hdr and read back converts to (nearly) the light: export and conversion are inverse conventions"""
    cube = ER.latlong_to_cubemap(ER.radiance(ER.latlong_dirs(64, 128)), 32, 1)
    light = E.EnvLight(torch.from_numpy(cube.astype(np.float32)).cuda())
    path = E.save_light_hdr(light, str(tmp_path / "light.hdr"), res=(64, 128))
    back = E.EnvLight.from_hdr(path, res=32, samples=1)
    assert ER.relative_distance(back.cubemap.base.cpu().numpy(), cube) < 2e-2  # RGBE keeps 8 bits of mantissa; two more interpolations
