"""Environment light from an HDR image (include/gs2m_envmap.h, csrc/envmap.hip).

    image, info = read_hdr("studio.hdr", info=True)      # (H, W, 3) float32 on the device
    light = EnvLight.from_hdr("studio.hdr", res=512)     # .cubemap (a CubemapLight with that base) and .brdf_lut
    save_light_hdr(learned_light, "light.hdr")           # a learned light as a lat-long .hdr

A Radiance file's header is parsed on the host and its scanlines are walked there once (`gs2m_hdr_scan`: where a row starts is
known only after the row before it); the file's bytes and the row table go to the device, which expands the planes and converts
RGBE to float32 (exact).  `latlong_to_cubemap` is the solid-angle-weighted conversion in HIP, pinned to `CubemapLight.export_envmap`
and `cube_to_dir`.  There is NO CPU fallback: the device functions refuse CPU tensors.  `parse_hdr_header`, `hdr_scan` and
`default_samples` are host-only."""
import ctypes as C
import math
import os

import numpy as np
import torch

import gs2m_native as N

ROW_FLAT, ROW_RLE = 0, 1  # GS2M_HDR_ROW_*
TABLE_COLS = 5            # GS2M_HDR_TABLE_COLS
HDR_ERRORS = {-10: "truncated file", -11: "zero code in a run-length coded plane", -12: "a run or literal passes the row's width",
              -13: "trailing bytes behind the last row", -14: "old-style run-length repeat marker (not supported)"}
MAX_SAMPLES = 16          # GS2M_ENVMAP_MAX_SAMPLES


class HdrError(ValueError):
    """A malformed Radiance file; `.code` is gs2m_hdr_scan's GS2M_HDR_ERR_* (0 for a malformed header)."""

    def __init__(self, message, code=0):
        super().__init__(message)
        self.code = code


def parse_hdr_header(data):
    """The text in front of the pixels.  -> (W, H, offset of the first pixel byte, info); info = {"format", "exposure" (the product
    of the EXPOSURE= lines, 1.0 without one; returned, not applied), "lines"}.  ValueError naming what is not supported: a magic
    other than #?RADIANCE / #?RGBE, a FORMAT other than 32-bit_rle_rgbe (or none), an orientation other than -Y H +X W."""
    end = data.find(b"\n\n")
    if end < 0:
        raise HdrError("hdr: no blank line ends the header")
    lines = data[:end].split(b"\n")
    magic = lines[0].strip()
    if magic not in (b"#?RADIANCE", b"#?RGBE"):
        raise HdrError(f"hdr: not a Radiance file (first line {magic[:16]!r}; #?RADIANCE or #?RGBE)")
    fmt, exposure = None, 1.0
    for ln in lines[1:]:
        ln = ln.strip()
        if ln.startswith(b"FORMAT="):
            fmt = ln[7:].strip().decode("ascii", "replace")
        elif ln.startswith(b"EXPOSURE="):
            try:
                exposure *= float(ln[9:])
            except ValueError:
                raise HdrError(f"hdr: unreadable line {ln!r}") from None
    if fmt is None:
        raise HdrError("hdr: the header has no FORMAT= line (32-bit_rle_rgbe is required)")
    if fmt != "32-bit_rle_rgbe":
        raise HdrError(f"hdr: FORMAT={fmt} is not supported (32-bit_rle_rgbe only)")
    res_end = data.find(b"\n", end + 2)
    if res_end < 0:
        raise HdrError("hdr: no resolution line")
    res = data[end + 2:res_end].split()
    if len(res) != 4 or res[0] != b"-Y" or res[2] != b"+X":
        raise HdrError(f"hdr: orientation {data[end + 2:res_end].decode('ascii', 'replace')!r} is not supported (-Y H +X W only)")
    try:
        h, w = int(res[1]), int(res[3])
    except ValueError:
        raise HdrError(f"hdr: unreadable resolution line {data[end + 2:res_end]!r}") from None
    if h < 1 or w < 1:
        raise HdrError(f"hdr: resolution {w} x {h}")
    return w, h, res_end + 1, {"format": fmt, "exposure": exposure, "lines": [ln.decode("ascii", "replace") for ln in lines[1:]]}


def hdr_scan(pixels, W, H):
    """gs2m_hdr_scan over the pixel bytes of a W x H file.  -> (code, table): code 0 or a GS2M_HDR_ERR_* / GS2M_ERR_* value, table an
    int64 array (H, 5) of {kind, o0, o1, o2, o3} (rows behind a refused one are zero).  Host only."""
    pixels = bytes(pixels)
    table = np.zeros((max(int(H), 1), TABLE_COLS), dtype=np.int64)
    buf = (C.c_ubyte * max(len(pixels), 1)).from_buffer_copy(pixels or b"\0")
    rc = N.lib().gs2m_hdr_scan(C.cast(buf, C.c_void_p), len(pixels), int(W), int(H), table.ctypes.data)
    return int(rc), table


def _image(image, who):
    if not isinstance(image, torch.Tensor) or not image.is_cuda:
        raise RuntimeError(f"{who}: `image` must be a CUDA tensor on a HIP device; there is no CPU path")
    if image.dtype != torch.float32:
        raise RuntimeError(f"{who}: `image` must be float32, got {image.dtype}")
    if image.dim() != 3 or image.shape[2] != 3 or image.numel() == 0:
        raise RuntimeError(f"{who}: `image` must have shape (H, W, 3), got {tuple(image.shape)}")
    if not image.is_contiguous():
        raise RuntimeError(f"{who}: `image` must be contiguous")
    return image


def decode_hdr(pixels, W, H, device="cuda"):
    """The pixel bytes of a W x H file -> (H, W, 3) float32 on `device`: scan on the host, expand and convert on the device."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("decode_hdr: `device` must be a HIP device; there is no CPU path")
    rc, table = hdr_scan(pixels, W, H)
    if rc in HDR_ERRORS:
        raise HdrError(f"hdr: {HDR_ERRORS[rc]}", rc)
    N.check(rc, "gs2m_hdr_scan")
    with N.device_guard(device):
        d_bytes = torch.frombuffer(bytearray(pixels), dtype=torch.uint8).to(device)
        d_table = torch.from_numpy(table).to(device)
        out = torch.empty((H, W, 3), dtype=torch.float32, device=device)
    N.launch("gs2m_hdr_decode", device, d_bytes.data_ptr(), d_bytes.numel(), int(W), int(H), d_table.data_ptr(), out.data_ptr())
    return out


def read_hdr(path, device="cuda", info=False):
    """A Radiance .hdr file -> (H, W, 3) float32 on `device`; with `info`, (image, info dict of parse_hdr_header)."""
    with open(path, "rb") as f:
        data = f.read()
    w, h, start, meta = parse_hdr_header(data)
    image = decode_hdr(data[start:], w, h, device)
    return (image, meta) if info else image


def encode_hdr(image):
    """(H, W, 3) float32 on the device -> (H, W, 4) uint8 on the device: R G B E, flat scanlines."""
    image = _image(image, "encode_hdr")
    h, w, _ = image.shape
    with N.device_guard(image.device):
        out = torch.empty((h, w, 4), dtype=torch.uint8, device=image.device)
    N.launch("gs2m_hdr_encode", image.device, w, h, image.data_ptr(), out.data_ptr())
    return out


def write_hdr(path, image):
    """Encode on the device; the header and the flat scanlines are written on the host."""
    rgbe = encode_hdr(image)
    h, w, _ = rgbe.shape
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode("ascii"))
        f.write(rgbe.cpu().numpy().tobytes())


def default_samples(res, source_width):
    """The smallest power of two S with 4 res S >= source_width, at most 16: one sub-sample per source pixel or finer."""
    s = 1
    while 4 * int(res) * s < int(source_width) and s < MAX_SAMPLES:
        s *= 2
    return s


def latlong_to_cubemap(image, res=512, samples=None, angle=0.0, scale=1.0):
    """(Hs, Ws, 3) lat-long float32 on the device -> (6, res, res, 3): the solid-angle-weighted mean over samples x samples taps per
    texel of the light turned by `angle` (radians) about +y, times `scale`.  res: a power of two >= 16; samples: 1 .. 16
    (None: `default_samples`).  The inverse of CubemapLight.export_envmap."""
    who = "latlong_to_cubemap"
    image = _image(image, who)
    hs, ws, _ = image.shape
    res = int(res)
    s = default_samples(res, ws) if samples is None else int(samples)
    if res < 16 or res & (res - 1):
        raise ValueError(f"{who}: res must be a power of two >= 16, got {res}")
    if not 1 <= s <= MAX_SAMPLES:
        raise ValueError(f"{who}: samples must be in 1 .. {MAX_SAMPLES}, got {s}")
    if hs < 2 or ws < 2:
        raise ValueError(f"{who}: the source must be at least 2 x 2, got {ws} x {hs}")
    if not (math.isfinite(angle) and math.isfinite(scale)):
        raise ValueError(f"{who}: angle {angle} / scale {scale}")
    with N.device_guard(image.device):
        out = torch.empty((6, res, res, 3), dtype=torch.float32, device=image.device)
    N.launch("gs2m_latlong_to_cubemap", image.device, hs, ws, image.data_ptr(), res, s, float(angle), float(scale), out.data_ptr())
    return out


class EnvLight:
    """What pbr_render and render_views_to_disk take as a light: `.cubemap`, a CubemapLight whose base is `base` (6, R, R, 3), and
    `.brdf_lut`.  The CubemapLight is built without its random initialiser, so the caller's RNG streams are untouched."""

    def __init__(self, base):
        from pbr import CubemapLight, get_brdf_lut
        if not isinstance(base, torch.Tensor) or not base.is_cuda:
            raise RuntimeError("EnvLight: `base` must be a CUDA tensor on a HIP device; there is no CPU path")
        if base.dtype != torch.float32 or base.dim() != 4 or base.shape[0] != 6 or base.shape[1] != base.shape[2] or base.shape[3] != 3:
            raise RuntimeError(f"EnvLight: `base` must be float32 (6, R, R, 3), got {base.dtype} {tuple(base.shape)}")
        res = int(base.shape[1])
        if res < CubemapLight.LIGHT_MIN_RES or res & (res - 1):
            raise ValueError(f"EnvLight: the resolution must be a power of two >= {CubemapLight.LIGHT_MIN_RES}, got {res}")
        cubemap = CubemapLight.__new__(CubemapLight)
        torch.nn.Module.__init__(cubemap)
        cubemap.mtx = None
        cubemap.base = torch.nn.Parameter(base.detach().contiguous(), requires_grad=False)
        cubemap.register_parameter("env_base", cubemap.base)
        self.cubemap = cubemap
        self.brdf_lut = get_brdf_lut().to(base.device)

    @classmethod
    def from_image(cls, image, res=512, samples=None, angle=0.0, exposure=0.0):
        """`exposure` in stops: the radiance is scaled by 2^exposure."""
        return cls(latlong_to_cubemap(image, res, samples, angle, 2.0 ** float(exposure)))

    @classmethod
    def from_hdr(cls, path, res=512, samples=None, angle=0.0, exposure=0.0, device="cuda"):
        return cls.from_image(read_hdr(path, device), res, samples, angle, exposure)


def save_light_hdr(light, path, res=(512, 1024)):
    """The lat-long image of a light (an EnvLight, a training run's light, or a CubemapLight) as a Radiance file."""
    cubemap = getattr(light, "cubemap", light)
    with torch.no_grad():
        image = cubemap.export_envmap(res=list(res), return_img=True)
    write_hdr(path, image.contiguous())
    return os.fspath(path)
