"""tests/ssim_ref.py checked without a GPU: the float64 restatement against float64 autograd of the map formulation, and both
a-priori bounds against a float32 evaluation of the same operator (torch_ssim_map's formulation in float32) on every input
family tests/test_ssim_kernels_gpu.py uses -- the bounds are satisfiable by a correct float32 implementation before a
kernel is held to them."""
import os
import re

import numpy as np
import pytest
import torch

import ssim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 3, 45, 64), (1, 1, 7, 9), (1, 1, 1, 1), (1, 2, 30, 70), (2, 4, 23, 33), (1, 1, 12, 129), (1, 2, 5, 6)]


def _flat(shape, va, vb):
    return torch.full(shape, va, dtype=torch.float32), torch.full(shape, vb, dtype=torch.float32)


def _step(shape):
    a = torch.zeros(shape)
    a[..., shape[-1] // 2:] = 1.0
    b = torch.zeros(shape)
    b[..., shape[-2] // 2:, :] = 1.0
    return a, b


def _families():
    """(label, img1, img2): the mixed planes of the GPU tests, and each ingredient on its own"""
    out = [(f"mixed{s}", *R.make_images(s, seed=sum(s))) for s in SHAPES]
    s = (1, 2, 24, 40)
    out += [("black", *_flat(s, 0.0, 0.0)), ("white", *_flat(s, 1.0, 1.0)), ("mid", *_flat(s, 0.5, 0.5)), ("white-black", *_flat(s, 1.0, 0.0)),
            ("mid-other", *_flat(s, 0.5, 0.37)), ("step", *_step(s))]
    gen = torch.Generator().manual_seed(5)
    a = torch.rand(s, generator=gen)
    out += [("noise", a, torch.rand(s, generator=gen)), ("identical", a, a.clone())]
    return out


FAMILIES = _families()
IDS = [f[0] for f in FAMILIES]


def test_window_is_the_kernels_window():
    """the 11 constants of csrc/window11.h, the one window csrc/ssim.hip walks, are these float32 weights, bit for bit; they
    sum to 1 within float32"""
    src = open(os.path.join(ROOT, "gs-2m_amd", "csrc", "window11.h")).read()
    assert '#include "window11.h"' in open(os.path.join(ROOT, "gs-2m_amd", "csrc", "ssim.hip")).read()
    body = re.search(r"WINDOW11_W\[11\]\s*=\s*\{(.*?)\}", src, flags=re.S).group(1)
    consts = np.array([np.float32(x.strip().rstrip("f")) for x in body.split(",")], dtype=np.float32)
    assert np.array_equal(consts, R.window32().numpy())
    assert abs(float(R.window().sum()) - 1.0) < 4 * R.U


@pytest.mark.parametrize("hw", [(1, 1), (7, 9), (13, 5), (30, 70)])
def test_conv_is_the_121_taps_with_zero_padding(hw):
    x = torch.rand(hw, generator=torch.Generator().manual_seed(hw[0]), dtype=torch.float64)
    assert np.abs(R.conv(x).numpy() - R.conv_direct(x.numpy())).max() < 1e-15


@pytest.mark.parametrize("label,a,b", FAMILIES, ids=IDS)
def test_closed_forms_reproduce_float64_autograd(label, a, b):
    a64, b64 = a.double(), b.double()
    # the three maps: derivatives of the map in (mu1, e1, e12), mu1 also through s1 = e1 - mu1^2 and s12 = e12 - mu1 mu2
    q = [t.requires_grad_(True) for t in R.window_sums(a64, b64)]
    m = R.ssim_map_from_sums(*q)
    g = torch.autograd.grad(m.sum(), [q[0], q[1], q[4]])
    closed = R.derivative_maps_from_sums(*[t.detach() for t in q])
    for name, x, y in zip(R.OUTPUTS[1:], closed, g):
        scale = y.abs().max().item() + 1.0
        assert (x - y).abs().max().item() < 1e-9 * scale, (label, name)   # flat white: terms of 2 / C2 = 2222 cancel
    # the epilogue as the kernel writes it is the same four functions
    out, _, _ = R._kernel_epilogue([t.detach() for t in q], R.C1, R.C2)
    f = R.forward(a64, b64)
    for name in R.OUTPUTS:
        assert (out[name] - f[name]).abs().max().item() < 1e-9 * (f[name].abs().max().item() + 1.0), (label, name)
    # backward: a non-uniform upstream gradient through the map formulation
    G = torch.rand(a.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64) - 0.3
    x = a64.clone().requires_grad_(True)
    (R.ssim_map(x, b64) * G).sum().backward()
    got = R.backward(a64, b64, G, f["dm_dmu1"], f["dm_dsigma1_sq"], f["dm_dsigma12"])
    assert (got - x.grad).abs().max().item() < 1e-10 * (x.grad.abs().max().item() + 1.0), label


@pytest.mark.parametrize("label,a,b", FAMILIES, ids=IDS)
def test_float32_evaluation_stays_inside_the_forward_bound(label, a, b):
    shape = a.shape
    a3, b3 = a.reshape(-1, *shape[-2:]), b.reshape(-1, *shape[-2:])
    got = R.forward32(a3, b3)
    ref = R.forward(a3.double(), b3.double())
    bound = R.bound_fwd(a3.double(), b3.double())
    for name in R.OUTPUTS:
        err = (got[name].double() - ref[name]).abs()
        ratio = R.worst_ratio(err, bound[name])
        print(f"{label} {name}: max err {err.max().item():.3e}, max err / bound {ratio:.4f}")
        assert ratio <= 1.0, (label, name, ratio)


@pytest.mark.parametrize("label,a,b", FAMILIES, ids=IDS)
def test_float32_evaluation_stays_inside_the_backward_bound(label, a, b):
    shape = a.shape
    dL, maps = R.make_backward_inputs(shape, seed=3)
    r3 = lambda t: t.reshape(-1, *shape[-2:])
    args32 = [r3(t) for t in (a, b, dL, *maps)]
    args64 = [t.double() for t in args32]
    got = R.backward32(*args32)
    err = (got.double() - R.backward(*args64)).abs()
    bound = R.bound_bwd(*args64)
    ratio = R.worst_ratio(err, bound)
    print(f"{label}: max err / bound {ratio:.4f}")
    assert ratio <= 1.0, (label, ratio)


def test_backward_inputs_have_zero_rows_and_columns_and_span_decades():
    dL, maps = R.make_backward_inputs((2, 3, 45, 64), seed=3)
    assert bool((dL[..., 2::5, :] == 0).all()) and bool((dL[..., :, 3::7] == 0).all())
    for m in maps:
        mag = m.abs()
        assert mag.min().item() < 1e-2 and mag.max().item() > 1e2 and bool((m < 0).any()) and bool((m > 0).any())


def test_images_hold_every_ingredient():
    a, b = R.make_images((2, 4, 45, 64), seed=9)
    assert a.min().item() >= 0 and a.max().item() <= 1 and b.min().item() >= 0 and b.max().item() <= 1
    for n in (0, 1, 2, 4, 5, 6, 7):   # plane 3 is white against black
        pa, pb = a.reshape(-1, 45, 64)[n], b.reshape(-1, 45, 64)[n]
        assert bool((pa == pb).any())
    assert bool((a.reshape(-1, 45, 64)[1] == 0).all()) and bool((b.reshape(-1, 45, 64)[2] == 1).all())


def test_strip_rows_entry_point_reports_the_class():
    """gs2m_ssim_strip_rows (host only, no device needed): the strip height the three SSIM calls use on a frame, the figures
    of csrc/ssim.hip's own comments among them, and a negative status for every frame they refuse or launch nothing for"""
    import gs2m_native
    rows = gs2m_native.lib().gs2m_ssim_strip_rows
    for shape, want in (((1, 3, 1080, 1920), 45), ((1, 3, 581, 777), 12), ((1, 3, 1200, 1600), 43), ((1, 1, 1, 1), 12), ((1, 3, 45, 64), 12),
                        ((120, 3, 37, 100), 13), ((315, 3, 50, 50), 23), ((43, 7, 100, 150), 44), ((100, 4, 91, 129), 45),
                        ((65535, 1, 1, 1), 31), ((1, 1, 65535 * 12, 1), 45)):
        assert rows(*shape) == want, shape
    for shape in ((65536, 1, 1, 1), (256, 256, 1, 1), (1, 1, 65536 * 12 - 11, 1), (0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0)):
        assert rows(*shape) == -4, shape
    for shape in ((-1, 3, 8, 8), (1, -3, 8, 8), (1, 3, -8, 8), (1, 3, 8, -8)):
        assert rows(*shape) == -1, shape
