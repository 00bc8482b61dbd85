"""csrc/png.hip through gs2m_png.py: the row filter byte for byte against tests/png_ref.py; every file through
Pillow, pixel for pixel; every stream through the strict inflater with the planned segment lengths; determinism and batching;
size conditions against zlib measured here on the CPU; refused arguments; the wired writers end to end.  All data is synthetic."""
import ctypes
import functools
import io
import json
import math
import os
import types
import zlib

import numpy as np
import pytest
import torch

import png_ref as R
import gs2m_native as N
import gs2m_png as P  # (fails here on a tree without the feature)

pytestmark = pytest.mark.gpu


def _band():
    """zeros over rows 60 .. 75 of a 96 x 160 image: their filtered rows are zeros too (filter None), a run of 16 x 481 bytes
    that crosses the segment boundary behind row 67"""
    img = R.make_image("a", 96, 160, seed=4)
    img[60:76] = 0
    return img


IMAGES = {
    "a96": lambda: R.make_image("a", 96, 160), "b96": lambda: R.make_image("b", 96, 160), "c96": lambda: R.make_image("c", 96, 160),
    "d96": lambda: R.make_image("d", 96, 160),
    "1x1": lambda: R.make_image("a", 1, 1), "1x7": lambda: R.make_image("a", 1, 7), "7x1": lambda: R.make_image("a", 7, 1),
    "5x5": lambda: R.make_image("a", 5, 5),
    "3x8200x4": lambda: R.make_image("b", 3, 8200),
    "a600": lambda: R.make_image("a", 600, 800), "b600": lambda: R.make_image("b", 600, 800), "c600": lambda: R.make_image("c", 600, 800),
    "d600": lambda: R.make_image("d", 600, 800),
    "noise": lambda: R.make_image("noise", 96, 160),
    "band": _band,
}
CASES = sorted(IMAGES)


@functools.lru_cache(maxsize=None)
def _case(name):
    """the image, its reference filtered stream and plan, and what the device made of it -- computed once, read by every test"""
    img = IMAGES[name]()
    H, W, CH = img.shape
    t = torch.from_numpy(img).cuda()
    return types.SimpleNamespace(img=img, dev=t, filtered=R.filter_stream(img), seg=R.segments(H, W, CH),
                                 rows=P.filter_rows(t).cpu().numpy(), stream=P.encode_streams(t)[0], file=P.encode(t)[0])


def test_the_cases_cover_what_they_are_there_for():
    used = {k: set(R.filter_rows(IMAGES[k + "96"]())[:, 0].tolist()) for k in "abcd"}
    assert set().union(*used.values()) == {0, 1, 2, 3, 4}, used  # every filter is chosen somewhere
    assert [_case(k).seg["n_segments"] for k in ("a96", "b96", "c96", "d96")] == [2, 2, 1, 2]
    assert (_case("a600").seg["n_segments"], _case("b600").seg["n_segments"]) == (47, 60)
    s = _case("3x8200x4").seg
    assert (s["stride"], s["rows_per_segment"], s["n_segments"]) == (32801, 1, 3)
    f = np.frombuffer(_case("band").filtered, np.uint8)
    first = _case("band").seg["lengths"][0]
    assert not f[first - 300:first + 300].any()  # the run crosses the boundary, more than 258 bytes on either side


@pytest.mark.parametrize("name", CASES)
def test_filter_rows_equal_the_reference(name):
    c = _case(name)
    H, W, CH = c.img.shape
    assert c.rows.shape == (H, 1 + W * CH) and c.rows.dtype == np.uint8
    ref = np.frombuffer(c.filtered, np.uint8).reshape(H, 1 + W * CH)
    assert np.array_equal(c.rows[:, 0], ref[:, 0]), "filter choice"
    assert np.array_equal(c.rows, ref)


@pytest.mark.parametrize("name", CASES)
def test_files_open_in_pillow_with_the_pixels_of_the_input(name):
    from PIL import Image
    c = _case(name)
    H, W, CH = c.img.shape
    with Image.open(io.BytesIO(c.file)) as im:
        im.load()
        assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[CH] and im.size == (W, H)
        assert np.array_equal(np.asarray(im).reshape(H, W, CH), c.img)
    hdr = R.parse_png(c.file)
    assert hdr["chunks"] == ["IHDR", "IDAT", "IEND"] and hdr["zlib"] == c.stream
    assert (hdr["width"], hdr["height"], hdr["bit_depth"], hdr["color_type"], hdr["compression"], hdr["filter"], hdr["interlace"]) == \
        (W, H, 8, R.COLOR_TYPE[CH], 0, 0, 0)


@pytest.mark.parametrize("name", CASES)
def test_strict_inflate_accepts_the_stream(name):
    c = _case(name)
    assert c.stream[:2] == b"\x78\x01" and len(c.stream) <= c.seg["max_stream_bytes"]
    out, tokens = R.strict_inflate(c.stream, c.seg["lengths"])
    assert out == c.filtered
    assert out == c.rows.tobytes()
    assert zlib.decompress(c.stream) == c.filtered
    assert all(isinstance(t, int) or (t[1] == 1 and 3 <= t[0] <= 258) for t in tokens)
    if name in ("d96", "d600", "band", "b96"):
        assert any(not isinstance(t, int) and t[0] == 258 for t in tokens), "a long run is matches of 258"


def test_two_runs_and_a_batch_give_identical_bytes():
    a, b = _case("a96"), _case("d96")
    noise = torch.from_numpy(R.make_image("noise", 96, 160, seed=9)).cuda()
    assert P.encode(a.dev)[0] == a.file and P.encode_streams(a.dev)[0] == a.stream
    singles = [a.file, b.file, P.encode(noise)[0]]
    assert P.encode([a.dev, b.dev, noise]) == singles
    assert P.encode(torch.stack([a.dev, b.dev, noise])) == singles
    rows = P.filter_rows(torch.stack([a.dev, b.dev, noise])).cpu().numpy()
    assert np.array_equal(rows[0], a.rows) and np.array_equal(rows[1], b.rows)
    many = P.encode([a.dev] * 17 + [b.dev])  # more images than one filter launch carries pointers for
    assert many == [a.file] * 17 + [b.file]


def _zlib_rle(data):
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    return len(co.compress(data) + co.flush())


def test_a_constant_image_shrinks_by_more_than_a_hundred():
    """a 258-byte run costs at most 13 bits even with fixed codes: about 155 : 1 with the per-segment sync blocks"""
    c = _case("d600")
    print(f"constant 600 x 800 x 3: file {len(c.file)} bytes of {600 * c.seg['stride']} filtered")
    assert len(c.file) <= 600 * c.seg["stride"] / 100


def test_noise_costs_no_more_than_stored_blocks():
    c = _case("noise")
    bound = sum(n + 5 * math.ceil(n / 65535) for n in c.seg["lengths"]) + 5 * (c.seg["n_segments"] - 1) + 6
    print(f"noise: stream {len(c.stream)}, stored bound {bound}")
    assert len(c.stream) <= bound


@pytest.mark.parametrize("name", ["a96", "b96", "c96", "a600", "b600", "c600"])
def test_stream_is_within_three_percent_of_zlib_rle(name):
    """Z: zlib (level 6, Z_RLE) on the same filtered bytes, measured here.  96 bytes per segment: a dynamic-block header and the
    5-byte sync block; 3 %: the parse and the code-length heuristics."""
    c = _case(name)
    Z = _zlib_rle(c.filtered)
    bound = 1.03 * Z + 96 * c.seg["n_segments"]
    print(f"{name}: stream {len(c.stream)}, zlib Z_RLE {Z}, ratio {len(c.stream) / Z:.4f}, bound {bound:.0f}")
    assert len(c.stream) <= bound


def test_refusals_leave_the_output_untouched():
    L = N.lib()
    H, W, CH = 6, 5, 3
    img = torch.from_numpy(R.make_image("a", H, W)).cuda()
    p = P.plan(H, W, CH, 1)
    ws = torch.empty(p["workspace_bytes"] + 256, dtype=torch.uint8, device="cuda")
    out = torch.full((p["max_stream_bytes"] + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    sizes = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    filtered = torch.full((H * (1 + W * CH),), 0xA5, dtype=torch.uint8, device="cuda")
    ptrs = (ctypes.c_void_p * 1)(img.data_ptr())
    null = (ctypes.c_void_p * 1)(None)
    s = N.stream_ptr()

    def enc(n=1, h=H, w=W, ch=CH, images=ptrs, ws_ptr=ws.data_ptr(), ws_bytes=p["workspace_bytes"], out_ptr=out.data_ptr(),
            stride=p["max_stream_bytes"], sizes_ptr=sizes.data_ptr()):
        return L.gs2m_png_encode(n, h, w, ch, images, ws_ptr, ws_bytes, out_ptr, stride, sizes_ptr, s)

    assert enc(w=16384, ch=4) == -4                    # stride 65537
    assert enc(ch=2) == -1 and enc(n=0) == -1 and enc(h=0) == -1
    assert enc(images=None) == -1 and enc(images=null) == -1 and enc(ws_ptr=None) == -1 and enc(out_ptr=None) == -1 and enc(sizes_ptr=None) == -1
    assert enc(ws_bytes=p["workspace_bytes"] - 1) == -1      # short workspace
    assert enc(ws_ptr=ws.data_ptr() + 1) == -1               # misaligned workspace
    assert enc(stride=p["max_stream_bytes"] - 1) == -1       # short out_stride
    assert L.gs2m_png_filter(1, H, 16384, 4, ptrs, filtered.data_ptr(), s) == -4
    assert L.gs2m_png_filter(1, H, W, 2, ptrs, filtered.data_ptr(), s) == -1
    assert L.gs2m_png_filter(0, H, W, CH, ptrs, filtered.data_ptr(), s) == -1
    assert L.gs2m_png_filter(1, H, W, CH, null, filtered.data_ptr(), s) == -1
    assert L.gs2m_png_filter(1, H, W, CH, ptrs, None, s) == -1
    torch.cuda.synchronize()
    assert (out == 0xA5).all() and (filtered == 0xA5).all() and sizes.item() == -7
    assert enc() == 0                                       # and the same buffers are fine when the arguments are
    torch.cuda.synchronize()
    n = sizes.item()
    assert zlib.decompress(out[:n].cpu().numpy().tobytes()) == R.filter_stream(img.cpu().numpy()) and (out[n:] == 0xA5).all()
    with pytest.raises(RuntimeError, match="unsupported size"):
        P.encode(torch.zeros((1, 16384, 4), dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="CH in"):
        P.encode(torch.zeros((4, 4, 2), dtype=torch.uint8, device="cuda"))


# ---- the wired writers ---------------------------------------------------------------------------------------------------------

def _same_pixels(dir_host, dir_device):
    from PIL import Image
    n = 0
    for root, _, files in os.walk(dir_host):
        for f in files:
            if not f.endswith(".png"):
                continue
            other = os.path.join(dir_device, os.path.relpath(os.path.join(root, f), dir_host))
            with Image.open(os.path.join(root, f)) as a, Image.open(other) as b:
                assert a.mode == b.mode and a.size == b.size and np.array_equal(np.asarray(a), np.asarray(b)), other
            R.parse_png(open(other, "rb").read())
            n += 1
    assert n == sum(f.endswith(".png") for _, _, fs in os.walk(dir_device) for f in fs)
    return n


@pytest.fixture(scope="module")
def scene():
    from test_view_maps_gpu import _truth_and_views
    return _truth_and_views(4000, 2, 64, 48)


def test_render_views_to_disk_device_png(tmp_path, scene):
    import gs2m_render as GR
    from gs2m_train import _Lighting
    truth, views = scene
    bg = torch.zeros(3, device="cuda")
    light = _Lighting(64, 0.01, "cuda")  # (randomly initialised: one light for both runs)
    for png in ("host", "device"):
        GR.render_views_to_disk(truth, views, str(tmp_path / png / "test" / "ours_1"), bg, png=png)
        GR.render_views_to_disk(truth, views[:1], str(tmp_path / png / "test" / "white_1"), torch.ones(3, device="cuda"), white_background=True,
                                light=light, png=png)
    assert _same_pixels(tmp_path / "host", tmp_path / "device") == 8 + 9 + 1  # 4 per view; 9 and the envmap with a light
    with pytest.raises(ValueError):
        GR.render_views_to_disk(truth, views[:1], str(tmp_path / "x" / "test" / "ours_1"), bg, png="gpu")


def test_score_views_and_mesh_render_views_device_png(tmp_path, scene):
    import gs2m_mesh as M
    import gs2m_metrics as GM
    truth, views = scene
    bg = torch.zeros(3, device="cuda")
    scores = {png: GM.score_views(truth, views, bg, out_dir=str(tmp_path / png / "scored"), png=png) for png in ("host", "device")}
    assert torch.equal(scores["host"]["psnr"], scores["device"]["psnr"]) and torch.equal(scores["host"]["ssim"], scores["device"]["ssim"])
    depths = {png: M.render_views(truth, views, str(tmp_path / png / "renders"), png=png) for png in ("host", "device")}
    assert torch.equal(depths["host"], depths["device"])
    assert _same_pixels(tmp_path / "host", tmp_path / "device") == 4 + 2


def test_mesh_view_command_line_device_png(tmp_path):
    import gs2m_mesh as M
    import gs2m_mesh_view as G
    import mesh_view_ref as V
    v, t, records = V.cli_mesh()
    M.write_mesh(tmp_path / "m.ply", types.SimpleNamespace(vertices=v, triangles=t, vertex_colors=np.full((len(v), 3), 0.5)))
    (tmp_path / "cameras.json").write_text(json.dumps(records))
    common = ["--ply-path", str(tmp_path / "m.ply"), "--cameras", str(tmp_path / "cameras.json"), "--rendering", "--still", "--animation", "--ss", "1",
              "--frames", "3"]
    host = G.main(common + ["--out-dir", str(tmp_path / "host")])
    dev = G.main(common + ["--out-dir", str(tmp_path / "device"), "--device-png"])
    assert len(dev["views"]) == len(host["views"]) == 4 and len(dev["frames"]) == 3 and dev["still"] and os.path.exists(dev["gif"])
    assert _same_pixels(tmp_path / "host", tmp_path / "device") == 4 + 1 + 3
