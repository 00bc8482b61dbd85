"""Drop-in for the two `render_utils` operators the reference's PBR stage imports (pbr/light.py:10:
`from render_utils import diffuse_cubemap, specular_cubemap`; submodules/render-utils/render_utils/ops.py:336-403) on
MI355X.  Same names and argument meaning; hand-written HIP behind include/gs2m_cubemap.h (csrc/cubemap.hip).  The
backward passes are deterministic gathers; no bounds table is built (the boxes are an acceleration structure in the
reference and do not change the result).  There is no CPU path."""
import numpy as np
import torch

import gs2m_native as _native


def _cubemap(t, name, ch):
    t = _native.f32(t, name, who="render_utils")
    if t.dim() != 4 or t.shape[0] != 6 or t.shape[1] != t.shape[2] or t.shape[3] != ch:
        raise RuntimeError(f"render_utils: `{name}` must be a float32 (6, res, res, {ch}) tensor, got {tuple(t.shape)}")
    return t


class _diffuse_cubemap_func(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cubemap):
        cubemap = _cubemap(cubemap, "cubemap", 3)
        out = torch.empty_like(cubemap)
        _native.launch("gs2m_diffuse_cubemap_forward", cubemap.device, cubemap.shape[1], cubemap.data_ptr(), out.data_ptr())
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = _cubemap(dout, "grad", 3)
        g = torch.empty_like(dout)
        _native.launch("gs2m_diffuse_cubemap_backward", dout.device, dout.shape[1], dout.data_ptr(), g.data_ptr())
        return g


def diffuse_cubemap(cubemap, use_python=False):
    assert not use_python
    return _diffuse_cubemap_func.apply(cubemap)


_tables = {}


def _texel_table(res, device):
    """(res,) separable texel-area factors of one cube-map level, cached per (device, res)."""
    key = (str(device), int(res))
    if key not in _tables:
        t = torch.empty((res,), dtype=torch.float32, device=device)
        _native.launch("gs2m_cubemap_texel_table", device, res, t.data_ptr())
        _tables[key] = t
    return _tables[key]


def _specular(fn, args, *tensors):
    """`fn(res, roughness, cutoff, texel table, *tensors)`; the last tensor is the result and fixes device and resolution."""
    out = tensors[-1]
    _native.launch(fn, out.device, out.shape[1], args[0], args[1], _texel_table(out.shape[1], out.device).data_ptr(),
                   *(t.data_ptr() for t in tensors))
    return out


def _like(t, ch):
    return torch.empty((*t.shape[:3], ch), dtype=torch.float32, device=t.device)


class _specular_cubemap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cubemap, roughness, costheta_cutoff):
        cubemap = _cubemap(cubemap, "cubemap", 3)
        ctx.args = (float(roughness), float(costheta_cutoff))
        return _specular("gs2m_specular_cubemap_forward", ctx.args, cubemap, _like(cubemap, 4))

    @staticmethod
    def backward(ctx, dout):
        dout = _cubemap(dout, "grad", 4)
        return _specular("gs2m_specular_cubemap_backward", ctx.args, dout, _like(dout, 3)), None, None


class _specular_cubemap_normalized(torch.autograd.Function):
    """specular_cubemap's `out[..., 0:3] / out[..., 3:]` folded into the operator (forward: gather + divide; backward: prescale +
    gather) -- two launches each way instead of ~16."""

    @staticmethod
    def forward(ctx, cubemap, roughness, costheta_cutoff):
        cubemap = _cubemap(cubemap, "cubemap", 3)
        raw = _like(cubemap, 4)
        ctx.args = (float(roughness), float(costheta_cutoff))
        out = _specular("gs2m_specular_cubemap_normalized_forward", ctx.args, cubemap, raw, torch.empty_like(cubemap))
        ctx.save_for_backward(raw)
        return out

    @staticmethod
    def backward(ctx, dout):
        (raw,) = ctx.saved_tensors
        dout = _cubemap(dout, "grad", 3)
        scratch, g = torch.empty_like(raw), torch.empty_like(dout)
        return _specular("gs2m_specular_cubemap_normalized_backward", ctx.args, raw, dout, scratch, g), None, None


_cutoff_cache = {}


def ndf_cutoff(roughness, cutoff):
    """cos of the angle inside which `cutoff` of the GGX NDF (alpha = roughness^2), summed over a million equally spaced
    angles in [0, pi/2], lies (render_utils/ops.py:373-388 without the bounds table)."""
    key = (float(roughness), float(cutoff))
    if key not in _cutoff_cache:
        costheta = np.cos(np.linspace(0, np.pi / 2.0, 1000000))
        a2 = roughness ** 4
        c = np.clip(costheta, 0.0, 1.0)
        d = (c * a2 - c) * c + 1.0
        D = np.cumsum(a2 / (d * d * np.pi))
        _cutoff_cache[key] = float(costheta[np.argmax(D >= D[-1] * cutoff)])
    return _cutoff_cache[key]


def specular_cubemap(cubemap, roughness, cutoff=0.99, use_python=False):
    assert not use_python
    assert cubemap.shape[0] == 6 and cubemap.shape[1] == cubemap.shape[2], "Bad shape for cubemap tensor: %s" % str(cubemap.shape)
    return _specular_cubemap_normalized.apply(cubemap, roughness, ndf_cutoff(roughness, cutoff))
