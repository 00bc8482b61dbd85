"""The host side of the environment-map stage (include/gs2m_envmap.h): gs2m_hdr_scan through ctypes against the numpy
restatement (tests/envmap_ref.py), one code per kind of malformed file, the header parser, and the restatement's own round trip.
No GPU is touched."""
import numpy as np
import pytest
import torch

import envmap_ref as ER
import gs2m_envmap as E


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("W", [1, 7, 8, 9, 130, 300])
def test_scan_table_matches_the_restatement(W, H):
    for kinds in ("rle", "flat", "mixed"):
        img = ER.sample_rgbe(W, H, seed=10 * W + H)
        px = ER.write_pixels(img, kinds)
        want_code, want = ER.scan(px, W, H)
        code, table = E.hdr_scan(px, W, H)
        assert want_code == ER.OK and code == 0, (kinds, code)
        assert np.array_equal(table, want), kinds
        coded = 8 <= W and kinds != "flat"
        assert (table[0, 0] == ER.ROW_RLE) == coded
        if kinds == "mixed" and H > 1 and coded:
            assert table[1, 0] == ER.ROW_FLAT and table[2, 0] == ER.ROW_RLE
        assert np.array_equal(ER.expand(px, W, H), img)  # the writer and the table describe the same pixels


def test_long_runs_are_split_at_127():
    plane = [5] * 127 + [6] * 300 + [1, 2, 3] + [9] * 4
    assert ER.rle_plane(plane) == bytes([255, 5, 255, 6, 255, 6, 128 + 46, 6, 3, 1, 2, 3, 128 + 4, 9])
    assert ER.rle_plane(list(range(200))) == bytes([128]) + bytes(range(128)) + bytes([72]) + bytes(range(128, 200))


def _both(px, W, H):
    want, _ = ER.scan(px, W, H)
    code, _ = E.hdr_scan(px, W, H)
    assert code == want, (code, want)
    return code


def test_every_truncation_of_a_small_file_is_refused_as_truncated():
    for kinds in ("rle", "flat", "mixed"):
        px = ER.write_pixels(ER.sample_rgbe(9, 2, seed=4), kinds)
        assert _both(px, 9, 2) == 0
        for n in range(len(px)):
            assert _both(px[:n], 9, 2) == ER.TRUNCATED, (kinds, n)


def test_each_malformed_kind_has_its_own_code():
    W, H = 9, 2
    row = bytes([2, 2, 0, 9]) + b"".join(bytes([128 + 9, 40 + c]) for c in range(4))  # four runs of 9
    good = row + row
    assert _both(good, W, H) == 0
    assert _both(good[:6] + bytes([0]) + good[7:], W, H) == ER.ZERO_CODE                       # plane 1's code byte
    assert _both(good[:4] + bytes([128 + 10]) + good[5:], W, H) == ER.OVERRUN                 # a run of 10 in a row of 9
    literal = bytes([2, 2, 0, 9]) + bytes([5, 1, 2, 3, 4, 5, 5, 1, 2, 3, 4, 5]) + row[6:]      # literals 5 + 5 > 9
    assert _both(literal + row, W, H) == ER.OVERRUN
    assert _both(bytes([2, 2, 0, 10]) + good[4:], W, H) == ER.TRUNCATED                       # wrong width: the row is flat, and short
    assert _both(good + b"\x07", W, H) == ER.TRAILING
    flat = bytearray(ER.write_pixels(ER.sample_rgbe(W, H, seed=1), "flat"))
    assert _both(bytes(flat), W, H) == 0
    flat[4 * 11:4 * 11 + 4] = bytes([1, 1, 1, 3])
    assert _both(bytes(flat), W, H) == ER.OLD_RLE
    codes = {ER.TRUNCATED, ER.ZERO_CODE, ER.OVERRUN, ER.TRAILING, ER.OLD_RLE}
    assert len(codes) == 5 and set(E.HDR_ERRORS) == codes
    assert E.hdr_scan(good, 0, H)[0] == -1 and E.hdr_scan(good, W, 0)[0] == -1
    # a width new-style RLE cannot carry: the marker bytes are pixels
    assert _both(bytes([2, 2, 0, 7]) + bytes(24), 7, 1) == 0


def test_header_parsing():
    px = ER.write_pixels(ER.sample_rgbe(9, 2), "rle")
    w, h, start, info = E.parse_hdr_header(ER.hdr_file(px, 9, 2, magic=b"#?RGBE", lines=(b"# made by a test", b"FORMAT=32-bit_rle_rgbe", b"EXPOSURE=2.5")))
    data = ER.hdr_file(px, 9, 2, magic=b"#?RGBE", lines=(b"# made by a test", b"FORMAT=32-bit_rle_rgbe", b"EXPOSURE=2.5"))
    assert (w, h) == (9, 2) and data[start:] == px and info["exposure"] == 2.5 and info["format"] == "32-bit_rle_rgbe"
    assert E.parse_hdr_header(ER.hdr_file(px, 9, 2))[3]["exposure"] == 1.0
    with pytest.raises(ValueError, match=r"\+Y 2 \+X 9"):
        E.parse_hdr_header(ER.hdr_file(px, 9, 2, resolution=b"+Y 2 +X 9"))
    with pytest.raises(ValueError, match="-Y 2 -X 9"):
        E.parse_hdr_header(ER.hdr_file(px, 9, 2, resolution=b"-Y 2 -X 9"))
    with pytest.raises(ValueError, match="FORMAT"):
        E.parse_hdr_header(ER.hdr_file(px, 9, 2, lines=(b"EXPOSURE=1",)))
    with pytest.raises(ValueError, match="32-bit_rle_xyze"):
        E.parse_hdr_header(ER.hdr_file(px, 9, 2, lines=(b"FORMAT=32-bit_rle_xyze",)))
    with pytest.raises(ValueError, match="Radiance"):
        E.parse_hdr_header(ER.hdr_file(px, 9, 2, magic=b"P6"))


def test_restatement_round_trip():
    """encode(decode(b)) == b for every pixel whose largest mantissa is >= 128 (the normalised ones: what an encoder writes) -- down to
    the encoder's own floor: a pixel that decodes to less than 1e-32 (exponent bytes below 23) is written as 0 0 0 0, by the same rule"""
    rng = np.random.default_rng(0)
    b = rng.integers(0, 256, (64, 257, 4), dtype=np.uint8)
    b[0, :8] = [[128, 0, 0, 1], [255, 255, 255, 255], [200, 3, 0, 255], [128, 128, 128, 128], [0, 255, 7, 30], [129, 0, 255, 2], [255, 0, 0, 1], [1, 128, 1, 200]]
    norm = (b[..., :3].max(axis=-1) >= 128) & (b[..., 3] >= 1)
    assert (b[0, 0] == (128, 0, 0, 1)).all() and norm.sum() > 4000
    val = ER.rgbe_to_float(b)
    back = ER.float_to_rgbe(val)
    tiny = val.max(axis=-1) < np.float32(1e-32)
    assert (b[norm & tiny][:, 3] < 23).all() and (b[norm & ~tiny][:, 3] >= 22).all() and (norm & tiny).sum() > 100
    assert np.array_equal(back[norm & ~tiny], b[norm & ~tiny])
    assert (back[tiny] == 0).all()
    # and e == 0 decodes to zero whatever the mantissas
    assert (ER.rgbe_to_float(np.array([[9, 200, 1, 0]], dtype=np.uint8)) == 0).all()
    x = np.array([[0, 0, 0], [1e-33, 0, 0], [-1, np.nan, 2.0], [np.inf, 1, 1], [1.0, 0.5, 0.25], [0.99999994, 0, 0]], dtype=np.float32)
    want = [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 128, 130], [255, 0, 0, 255], [128, 64, 32, 129], [255, 0, 0, 128]]
    assert ER.float_to_rgbe(x).tolist() == want


def test_the_conversion_restatement_keeps_a_constant_and_follows_export_envmap():
    c = ER.latlong_to_cubemap(np.full((8, 16, 3), 3.7), 16, 2, angle=0.4, scale=0.5)
    assert np.allclose(c, 1.85, rtol=1e-14, atol=0)
    # a source that is the analytic radiance at its pixel centres -> texel values close to the radiance at the texel centres
    src = ER.radiance(ER.latlong_dirs(64, 128))
    cube = ER.latlong_to_cubemap(src, 32, 1)
    assert ER.relative_distance(cube, ER.radiance(ER.texel_dirs(32))) < 2e-3
    turned = ER.latlong_to_cubemap(src, 32, 1, angle=0.7)
    assert ER.relative_distance(turned, ER.radiance(ER.rotate_y(ER.texel_dirs(32), -0.7))) < 2e-3


def test_default_samples():
    assert [E.default_samples(512, w) for w in (1024, 2048, 2049, 4096, 8192, 10 ** 6)] == [1, 1, 2, 2, 4, 16]
    assert E.default_samples(16, 32) == 1 and E.default_samples(16, 65) == 2


def test_the_module_refuses_cpu_tensors(tmp_path):
    img = torch.ones(8, 16, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.latlong_to_cubemap(img, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.encode_hdr(img)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.write_hdr(str(tmp_path / "x.hdr"), img)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.EnvLight(torch.ones(6, 16, 16, 3))
    path = tmp_path / "a.hdr"
    path.write_bytes(ER.hdr_file(ER.write_pixels(ER.sample_rgbe(9, 2)), 9, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.read_hdr(str(path), "cpu")
    assert not (tmp_path / "x.hdr").exists()
