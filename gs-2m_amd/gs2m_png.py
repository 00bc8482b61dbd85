"""PNG files from 8-bit images that sit in device memory (include/gs2m_png.h, csrc/png.hip).

    files = encode([rgb_u8, normal_u8])          # whole PNG files, as bytes
    save([rgb_u8, normal_u8], ["a.png", "b.png"])

The row filters, deflate and the Adler-32 are kernels on torch's current stream; the filtered bytes never leave the device.  The
compressed streams are read back in one copy and wrapped on the host -- signature, IHDR, one IDAT, IEND, chunk CRCs from
zlib.crc32: plumbing over bytes that have to reach the host anyway.  The bytes are a function of the image alone: two runs, and a
batch against single calls, give identical files.

Images are uint8 device tensors (H, W, CH) or (N, H, W, CH), or a list of (H, W, CH) tensors of one shape; CH in {1, 3, 4}
(gray, RGB, RGBA).  There is NO CPU fallback: the kernels refuse CPU tensors.  `plan` and `container` are host-only."""
import ctypes as C
import struct
import zlib

import torch

import gs2m_native as N

SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOR_TYPE = {1: 0, 3: 2, 4: 6}
MODES = ("host", "device")


def plan(H, W, CH, n=1):
    """-> dict(stride, rows_per_segment, n_segments, max_stream_bytes, workspace_bytes) of n images (H, W, CH).  No GPU is touched;
    the sizes the encoder refuses raise RuntimeError ("unsupported size" / "invalid argument")."""
    out = [C.c_longlong() for _ in range(4)]
    N.check(N.lib().gs2m_png_plan(int(H), int(W), int(CH), int(n), *[C.byref(o) for o in out]), "gs2m_png_plan")
    return dict(stride=1 + int(W) * int(CH), rows_per_segment=out[0].value, n_segments=out[1].value, max_stream_bytes=out[2].value,
                workspace_bytes=out[3].value)


def _images(images, who):
    """-> (list of contiguous (H, W, CH) uint8 device tensors of one shape on one device, whether a single image was given)"""
    single = isinstance(images, torch.Tensor) and images.dim() == 3
    if isinstance(images, torch.Tensor):
        if images.dim() not in (3, 4):
            raise RuntimeError(f"{who}: `images` must have shape (H, W, CH) or (N, H, W, CH), got {tuple(images.shape)}")
        images = [images] if single else list(images.unbind(0))
    images = list(images)
    if not images:
        raise RuntimeError(f"{who}: no image")
    for t in images:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{who}: `images` must be CUDA tensors on a HIP device; there is no CPU path")
        if t.dtype != torch.uint8:
            raise RuntimeError(f"{who}: `images` must be uint8, got {t.dtype}")
        if t.dim() != 3 or t.shape[2] not in COLOR_TYPE or t.numel() == 0 or t.shape != images[0].shape or t.device != images[0].device:
            raise RuntimeError(f"{who}: `images` must be (H, W, CH) tensors of one shape on one device, CH in (1, 3, 4), got {tuple(t.shape)} on {t.device}")
    return [t.contiguous() for t in images], single


def _pointers(images):
    return (C.c_void_p * len(images))(*[t.data_ptr() for t in images])


def filter_rows(images):
    """The filtered streams: per image H records [filter byte][W CH filtered bytes].  -> uint8 device tensor (N, H, 1 + W CH),
    (H, 1 + W CH) for a single (H, W, CH) image."""
    images, single = _images(images, "filter_rows")
    h, w, ch = images[0].shape
    dev = images[0].device
    plan(h, w, ch, len(images))  # refuses what the encoder refuses, by name
    with N.device_guard(dev):
        out = torch.empty((len(images), h, 1 + w * ch), dtype=torch.uint8, device=dev)
    N.launch("gs2m_png_filter", dev, len(images), h, w, ch, _pointers(images), out.data_ptr())
    return out[0] if single else out


def encode_streams_device(images):
    """The kernels alone, asynchronous: -> (out uint8 (N, max_stream_bytes), sizes int64 (N,)) on the device; image n's zlib stream
    is out[n, :sizes[n]]."""
    images, _ = _images(images, "encode")
    h, w, ch = images[0].shape
    dev = images[0].device
    p = plan(h, w, ch, len(images))
    with N.device_guard(dev):
        ws = torch.empty(p["workspace_bytes"], dtype=torch.uint8, device=dev)  # (torch's allocations are aligned to 512 bytes)
        out = torch.empty((len(images), p["max_stream_bytes"]), dtype=torch.uint8, device=dev)
        sizes = torch.empty(len(images), dtype=torch.int64, device=dev)
    N.launch("gs2m_png_encode", dev, len(images), h, w, ch, _pointers(images), ws.data_ptr(), ws.numel(), out.data_ptr(), out.stride(0),
             sizes.data_ptr())
    return out, sizes


def encode_streams(images):
    """-> list of the images' zlib streams (bytes): what a PNG's IDAT holds.  One synchronisation for the lengths, one copy."""
    out, sizes = encode_streams_device(images)
    sizes = sizes.tolist()
    flat = torch.cat([out[n, :s] for n, s in enumerate(sizes)]).cpu().numpy().tobytes()
    streams, pos = [], 0
    for s in sizes:
        streams.append(flat[pos:pos + s])
        pos += s
    return streams


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(body, zlib.crc32(kind)) & 0xFFFFFFFF)


def container(w, h, ch, stream):
    """A PNG file around a zlib stream: signature, IHDR (bit depth 8, no interlace), one IDAT, IEND.  Host only."""
    return (SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", int(w), int(h), 8, COLOR_TYPE[int(ch)], 0, 0, 0)) + _chunk(b"IDAT", stream)
            + _chunk(b"IEND", b""))


def encode(images):
    """-> list[bytes]: one whole PNG file per image."""
    imgs, _ = _images(images, "encode")
    h, w, ch = imgs[0].shape
    return [container(w, h, ch, s) for s in encode_streams(imgs)]


def save(images, paths):
    """Encodes `images` in one call and writes file n to paths[n]."""
    imgs, _ = _images(images, "save")
    paths = [paths] if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__") else list(paths)
    if len(paths) != len(imgs):
        raise ValueError(f"save: {len(imgs)} images, {len(paths)} paths")
    for path, data in zip(paths, encode(imgs)):
        with open(path, "wb") as f:
            f.write(data)


class Writer:
    """What the offline stages write their images through.  png="host": every `put` saves through Pillow at once, as the stages
    always did; png="device": `put` collects and `flush` encodes what was collected in as few calls as the shapes allow (a view's
    RGB images in one, its RGBA images in another) and writes the files."""

    def __init__(self, png="host"):
        if png not in MODES:
            raise ValueError(f"png must be one of {MODES}, got {png!r}")
        self.png = png
        self._pending = []  # (array, path)

    def put(self, array, path):
        """array: uint8 (H, W, CH) or (H, W), a device tensor (png="host" also takes a numpy array)"""
        if self.png == "host":
            from PIL import Image
            Image.fromarray(array.cpu().numpy() if isinstance(array, torch.Tensor) else array).save(path)
            return
        if isinstance(array, torch.Tensor) and array.dim() == 2:
            array = array.unsqueeze(2)
        self._pending.append((array, str(path)))

    def flush(self):
        groups = {}
        for array, path in self._pending:
            groups.setdefault((tuple(array.shape), str(getattr(array, "device", None))), []).append((array, path))
        self._pending = []
        for items in groups.values():
            save([a for a, _ in items], [p for _, p in items])

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.flush()
        return False


def add_png_argument(ap):
    """the flag gs2m_render.py and gs2m_mesh_view.py share"""
    ap.add_argument("--device-png", action="store_true", help="encode the PNG files on the GPU (gs2m_png: row filters, deflate and Adler-32 in HIP) "
                    "instead of through Pillow; the decoded pixels are the same, the files are not byte-identical")
