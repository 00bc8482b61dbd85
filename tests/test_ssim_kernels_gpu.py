"""ssim_fwd_kernel and ssim_bwd_kernel of csrc/ssim.hip alone, through the C entry points, against the float64 restatement
of tests/ssim_ref.py (checked without a GPU by tests/test_ssim_ref.py), element by element and within that module's a-priori
bounds -- never a tensor-wide maximum, never a figure taken from the kernels.

Every strip height class `ssim_rows()` can choose is reached by a small frame with many planes, and each case reads its
class back through gs2m_ssim_strip_rows:

    12 (floor)  (1,3,45,64) (1,1,7,9) (1,1,1,1)   nrows 22; last strips of 9 and 7 rows
    13          (120,3,37,100)                    strips 13, 13, 11; nrows 23 = 2 * 11 + 1
    23          (315,3,50,50)                     strips 23, 23, 4; nrows 33
    44          (43,7,100,150)                    the class of a full DTU frame (43 at 1600 x 1200); nrows 54 = 5 * 11 - 1
    45 (cap)    (100,4,91,129)                    strips 45, 45, 1; the last has nrows 11

The float64 reference and the bounds are evaluated on the device over every plane (the same torch code as on the CPU), the
first, the last and three random planes are evaluated again on the CPU and the kernel's output is held to those too.  Every
output lives in one buffer with canary words before, between and after the arrays.

Largest err / bound measured on the MI355X (printed by every case; the bound is 1):

    rows  shape            map     dm_dmu1  dm_dsigma1_sq  dm_dsigma12  backward  composite
    12    (1,3,45,64)      0.0961  0.0754   0.0832         0.1120       0.1460    0.0406
    12    (1,1,7,9)        0.0485  0.0232   0.0319         0.0332       0.0706    0.0030
    12    (1,1,1,1)        0.0384  0.0312   0.0304         0.0524       0.0073    0.0142
    13    (120,3,37,100)   0.1441  0.1155   0.1182         0.1839       0.2585    0.0805
    23    (315,3,50,50)    0.1682  0.1222   0.1344         0.1805       0.2282    0.0860
    44    (43,7,100,150)   0.1468  0.1069   0.1075         0.1710       0.2639    0.0790
    45    (100,4,91,129)   0.1387  0.1161   0.1268         0.1709       0.2653    0.0685
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ssim_ref as R

pytestmark = pytest.mark.gpu

CANARY = -777.25
GUARD = 256
OK, INVALID, UNSUPPORTED = 0, -1, -4
CLASSES = [((1, 3, 45, 64), 12), ((1, 1, 7, 9), 12), ((1, 1, 1, 1), 12), ((120, 3, 37, 100), 13), ((315, 3, 50, 50), 23),
           ((43, 7, 100, 150), 44), ((100, 4, 91, 129), 45)]
CLASS_IDS = [f"rows{r}-{'x'.join(map(str, s))}" for s, r in CLASSES]
WIDTHS = [1, 5, 6, 59, 60, 64, 65, 68, 69, 70, 128, 129]
HEIGHTS = [1, 5, 6, 10, 11, 12, 13, 22, 23]


def _lib():
    import gs2m_native
    return gs2m_native.lib()


def _stream():
    import gs2m_native
    return gs2m_native.stream_ptr()


def _rows(shape):
    return _lib().gs2m_ssim_strip_rows(*shape)


class Arrays:
    """k float32 arrays of n elements in one canary-filled buffer: GUARD words before, between and after them"""

    def __init__(self, n, k):
        self.n, self.k = n, k
        self.buf = torch.full((GUARD + k * (n + GUARD),), CANARY, dtype=torch.float32, device="cuda")

    def _off(self, j):
        return GUARD + j * (self.n + GUARD)

    def view(self, j):
        return self.buf[self._off(j):self._off(j) + self.n]

    def ptr(self, j):
        return self.buf.data_ptr() + 4 * self._off(j)

    def intact(self, written):
        """every guard word, and every array not in `written`, still holds the canary"""
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        for j in written:
            keep[self._off(j):self._off(j) + self.n] = False
        return bool((self.buf[keep] == CANARY).all())


def _forward(shape, a, b, out, train=True, ptrs=None, c1=R.C1, c2=R.C2):
    """-> return code.  out: Arrays(n, 4); `ptrs` overrides the four output pointers"""
    p = [out.ptr(0)] + [out.ptr(j) if train else None for j in (1, 2, 3)] if ptrs is None else ptrs
    rc = _lib().gs2m_ssim_forward(*shape, c1, c2, a.data_ptr() if a is not None else None, b.data_ptr() if b is not None else None, *p, _stream())
    torch.cuda.synchronize()
    return rc


def _backward(shape, a, b, dL, maps, grad):
    rc = _lib().gs2m_ssim_backward(*shape, a.data_ptr(), b.data_ptr(), dL.data_ptr(), *[m.data_ptr() for m in maps], grad.ptr(0), _stream())
    torch.cuda.synchronize()
    return rc


def _backward_uniform(shape, a, b, g, mul, div, maps, grad):
    rc = _lib().gs2m_ssim_backward_uniform(*shape, a.data_ptr(), b.data_ptr(), g.data_ptr(), mul, div, *[m.data_ptr() for m in maps], grad.ptr(0), _stream())
    torch.cuda.synchronize()
    return rc


def _p3(t, shape):
    return t.reshape(-1, shape[2], shape[3])


def _build_case(shape, seed=None):
    """inputs on the device, the float64 forward reference and its bound over every plane, the caller-made backward inputs"""
    a, b = R.make_images(shape, seed=sum(shape) if seed is None else seed)
    dL, maps = R.make_backward_inputs(shape, seed=sum(shape))
    c = SimpleNamespace(shape=shape, n=a.numel(), a=a.cuda(), b=b.cuda(), dL=dL.cuda(), maps=[m.cuda() for m in maps])
    c.a64, c.b64 = _p3(c.a, shape).double(), _p3(c.b, shape).double()
    c.ref = R.forward(c.a64, c.b64)
    c.bound = R.bound_fwd(c.a64, c.b64)
    return c


@functools.lru_cache(maxsize=None)
def _case(shape):
    return _build_case(shape)


def _run_forward(c):
    """the forward kernel on case c, canaries checked -> {output: (planes, H, W) float32}"""
    out = Arrays(c.n, 4)
    assert _forward(c.shape, c.a, c.b, out) == OK
    assert out.intact(written=(0, 1, 2, 3)), "the forward wrote outside its four arrays"
    return {name: _p3(out.view(j), c.shape).clone() for j, name in enumerate(R.OUTPUTS)}


def _forward_ratios(c, got, label):
    ratios = {}
    for name in R.OUTPUTS:
        err = (got[name].double() - c.ref[name]).abs()
        ratios[name] = R.worst_ratio(err, c.bound[name])
    print(f"forward {label}: err / bound " + "  ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    return ratios


def _run_backward(c, dL, maps):
    grad = Arrays(c.n, 1)
    assert _backward(c.shape, c.a, c.b, dL, maps, grad) == OK
    assert grad.intact(written=(0,)), "the backward wrote outside dL_dimg1"
    return _p3(grad.view(0), c.shape).clone()


def _backward_ratio(c, got, dL, maps, label):
    args = [c.a64, c.b64, _p3(dL, c.shape).double()] + [_p3(m, c.shape).double() for m in maps]
    ratio = R.worst_ratio((got.double() - R.backward(*args)).abs(), R.bound_bwd(*args))
    print(f"backward {label}: err / bound {ratio:.4f}")
    return ratio


def _composite_ratio(c, got_fwd, label):
    """forward, then the backward on the kernel's own derivative maps, against float64 autograd of the map formulation;
    per element: the forward bound pushed through the (linear) backward, plus the backward's own bound on what it was given"""
    maps = [got_fwd[k].reshape(c.shape).contiguous() for k in R.OUTPUTS[1:]]
    got = _run_backward(c, c.dL, maps)
    G = _p3(c.dL, c.shape).double()
    x = c.a64.clone().requires_grad_(True)
    (R.ssim_map(x, c.b64) * G).sum().backward()
    Ga = G.abs()
    tol = (R.conv(Ga * c.bound["dm_dmu1"]) + 2 * c.a64 * R.conv(Ga * c.bound["dm_dsigma1_sq"]) + c.b64 * R.conv(Ga * c.bound["dm_dsigma12"])
           + R.bound_bwd(c.a64, c.b64, G, *[_p3(m, c.shape).double() for m in maps]))
    ratio = R.worst_ratio((got.double() - x.grad).abs(), tol)
    print(f"composite {label}: err / bound {ratio:.4f}")
    return ratio


# ---------------------------------------------------------------- the strip height classes
@pytest.mark.parametrize("shape,rows", CLASSES, ids=CLASS_IDS)
def test_forward_alone_every_strip_class(shape, rows):
    """the map and each derivative map, every element of every plane, within bound_fwd of float64; the float64 reference itself
    is the CPU's on five planes, and the kernel is held to the CPU's reference and bound there as well"""
    assert torch.cuda.is_available()
    assert _rows(shape) == rows
    c = _case(shape)
    got = _run_forward(c)
    ratios = _forward_ratios(c, got, f"rows {rows} {shape}")
    for name, r in ratios.items():
        assert r <= 1.0, (shape, name, "largest err / bound", r)
    P = c.a64.shape[0]
    planes = sorted({0, P - 1} | {int(p) for p in np.random.default_rng(P).integers(0, P, 3)})
    a, b = c.a64[planes].cpu(), c.b64[planes].cpu()
    ref, bound = R.forward(a, b), R.bound_fwd(a, b)
    for name in R.OUTPUTS:
        scale = ref[name].abs().max().item() + 1.0
        assert (c.ref[name][planes].cpu() - ref[name]).abs().max().item() < 1e-10 * scale, (name, "device float64 differs from the CPU's")
        assert R.worst_ratio((got[name][planes].cpu().double() - ref[name]).abs(), bound[name]) <= 1.0, (shape, name, planes)


@pytest.mark.parametrize("shape,rows", CLASSES, ids=CLASS_IDS)
def test_backward_alone_every_strip_class(shape, rows):
    """caller-made signed maps over six decades and a dL_dmap with zero rows and columns: every element within bound_bwd of
    ssim_ref.backward on the same float32 values -- a wrong ring slot, halo column or prefetched row is an error of a whole tap"""
    assert _rows(shape) == rows
    c = _case(shape)
    got = _run_backward(c, c.dL, c.maps)
    r = _backward_ratio(c, got, c.dL, c.maps, f"rows {rows} {shape}")
    assert r <= 1.0, (shape, "largest err / bound", r)
    P = c.a64.shape[0]
    for p in sorted({0, P - 1}):   # the CPU's float64 on the first and the last plane
        args = [t[p].cpu() for t in (c.a64, c.b64, _p3(c.dL, shape).double(), *[_p3(m, shape).double() for m in c.maps])]
        assert R.worst_ratio((got[p].cpu().double() - R.backward(*args)).abs(), R.bound_bwd(*args)) <= 1.0, (shape, p)


@pytest.mark.parametrize("shape,rows", CLASSES, ids=CLASS_IDS)
def test_forward_then_backward_every_strip_class(shape, rows):
    assert _rows(shape) == rows
    c = _case(shape)
    r = _composite_ratio(c, _run_forward(c), f"rows {rows} {shape}")
    assert r <= 1.0, (shape, "largest err / tolerance", r)


# ---------------------------------------------------------------- widths and heights at the predicates, rows = 12
@pytest.mark.parametrize("W", WIDTHS)
def test_widths_and_heights_at_the_predicates(W):
    """W around the halo predicate `lane < 10 && x0 + 59 + lane < W` and the strip edge, H around the 10 halo rows, the 11-way
    unrolled ring and the 12-row strip; 1 to 3 planes.  Forward, backward alone and the composite, as for the classes."""
    worst = {}
    for i, H in enumerate(HEIGHTS):
        shape = (1, 1 + (i + W) % 3, H, W)
        assert _rows(shape) == 12
        c = _build_case(shape, seed=1000 * W + H)
        got = _run_forward(c)
        ratios = _forward_ratios(c, got, str(shape))
        ratios["backward"] = _backward_ratio(c, _run_backward(c, c.dL, c.maps), c.dL, c.maps, str(shape))
        ratios["composite"] = _composite_ratio(c, got, str(shape))
        for k, r in ratios.items():
            assert r <= 1.0, (shape, k, "largest err / bound", r)
            worst[k] = max(worst.get(k, 0.0), r)
    print(f"W {W}, H in {HEIGHTS}: largest err / bound " + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))


# ---------------------------------------------------------------- the uniform path
@pytest.mark.parametrize("shape,rows", [CLASSES[0], CLASSES[3], CLASSES[6]], ids=[CLASS_IDS[0], CLASS_IDS[3], CLASS_IDS[6]])
def test_uniform_backward_is_the_map_backward_bit_for_bit(shape, rows):
    """gs2m_ssim_backward_uniform(g, mul, div) == gs2m_ssim_backward with dL_dmap filled with the float32 value (g * mul) / div"""
    assert _rows(shape) == rows
    c = _case(shape)
    numel = float(c.n)
    for g, mul, div in ((1.0, 1.0, numel), (1.7, -0.2, numel), (-3.5, 2.0, 7.0), (1e-3, -1.0, 1.0), (0.3, 0.2, 3.0)):
        gv = torch.tensor([g], dtype=torch.float32, device="cuda")
        value = (np.float32(g) * np.float32(mul)) / np.float32(div)
        assert value.dtype == np.float32
        grad = Arrays(c.n, 1)
        assert _backward_uniform(shape, c.a, c.b, gv, mul, div, c.maps, grad) == OK
        assert grad.intact(written=(0,))
        want = _run_backward(c, torch.full(shape, float(value), dtype=torch.float32, device="cuda"), c.maps)
        assert torch.equal(_p3(grad.view(0), shape), want), (g, mul, div)


# ---------------------------------------------------------------- stray writes, inference, empty frames
def test_inference_writes_only_the_map():
    """NULL derivative pointers: the map is the training call's map bit for bit, the three other arrays keep their canaries"""
    for shape in ((1, 3, 45, 64), (2, 2, 23, 129), (1, 1, 1, 1)):
        c = _build_case(shape)
        out = Arrays(c.n, 4)
        assert _forward(shape, c.a, c.b, out, train=False) == OK
        assert out.intact(written=(0,)), shape
        assert torch.equal(_p3(out.view(0), shape), _run_forward(c)["map"])


def test_empty_frames_return_ok_and_write_nothing():
    c = _build_case((1, 2, 12, 20))
    g = torch.ones(1, device="cuda")
    for shape in ((0, 2, 12, 20), (1, 0, 12, 20), (1, 2, 0, 20), (1, 2, 12, 0)):
        out, grad = Arrays(c.n, 4), Arrays(c.n, 1)
        assert _forward(shape, c.a, c.b, out) == OK and out.intact(written=())
        assert _backward(shape, c.a, c.b, c.dL, c.maps, grad) == OK and grad.intact(written=())
        assert _backward_uniform(shape, c.a, c.b, g, 1.0, 1.0, c.maps, grad) == OK and grad.intact(written=())


# ---------------------------------------------------------------- refusals
def test_refusals_write_nothing():
    g = torch.ones(1, device="cuda")

    def refused(shape, code, n):
        a = torch.rand(n, device="cuda")
        maps = [a, a, a]
        out, grad = Arrays(n, 4), Arrays(n, 1)
        assert _lib().gs2m_ssim_strip_rows(*shape) == code
        assert _forward(shape, a, a, out) == code and out.intact(written=())
        assert _backward(shape, a, a, a, maps, grad) == code and grad.intact(written=())
        assert _backward_uniform(shape, a, a, g, 1.0, 1.0, maps, grad) == code and grad.intact(written=())

    refused((65536, 1, 1, 1), UNSUPPORTED, 65536)       # B * CH beyond the grid's z extent
    refused((256, 256, 1, 1), UNSUPPORTED, 65536)
    H = 65536 * 12 - 11
    assert (H + 11) // 12 == 65536
    refused((1, 1, H, 1), UNSUPPORTED, H)                # more strips than the grid's y extent at the floor of 12 rows
    refused((1, 1, -1, 4), INVALID, 4)
    # one or two of the three derivative pointers
    c = _build_case((1, 2, 12, 20))
    for mask in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        out = Arrays(c.n, 4)
        ptrs = [out.ptr(0)] + [out.ptr(j + 1) if m else None for j, m in enumerate(mask)]
        assert _forward(c.shape, c.a, c.b, out, ptrs=ptrs) == INVALID and out.intact(written=()), mask
    out, grad = Arrays(c.n, 4), Arrays(c.n, 1)
    assert _forward(c.shape, c.a, c.b, out, ptrs=[None, out.ptr(1), out.ptr(2), out.ptr(3)]) == INVALID and out.intact(written=())
    assert _forward(c.shape, None, c.b, out) == INVALID and out.intact(written=())
    assert _backward_uniform(c.shape, c.a, c.b, g, 1.0, 0.0, c.maps, grad) == INVALID and grad.intact(written=())
    assert _backward_uniform(c.shape, c.a, c.b, g, 1.0, -0.0, c.maps, grad) == INVALID and grad.intact(written=())


def test_the_largest_plane_count_runs():
    """B * CH = 65535 with H = W = 1: the last plane index the grid can hold; one tap each way, within the bounds
    (65535 / 2048 puts it in the 31-row class: one strip of one row, nrows 11)"""
    shape = (65535, 1, 1, 1)
    assert _rows(shape) == 31
    gen = torch.Generator().manual_seed(65535)
    a, b = torch.rand(shape, generator=gen), torch.rand(shape, generator=gen)
    a[:100], b[:100] = 0.0, 0.0
    a[100:200], b[100:200] = 1.0, 1.0
    b[200:300] = a[200:300]
    dL, maps = R.make_backward_inputs(shape, seed=1)
    c = SimpleNamespace(shape=shape, n=a.numel(), a=a.cuda(), b=b.cuda(), dL=dL.cuda(), maps=[m.cuda() for m in maps])
    c.a64, c.b64 = _p3(c.a, shape).double(), _p3(c.b, shape).double()
    c.ref, c.bound = R.forward(c.a64, c.b64), R.bound_fwd(c.a64, c.b64)
    got = _run_forward(c)
    for name, r in _forward_ratios(c, got, str(shape)).items():
        assert r <= 1.0, (name, r)
    assert _backward_ratio(c, _run_backward(c, c.dL, c.maps), c.dL, c.maps, str(shape)) <= 1.0
    assert _composite_ratio(c, got, str(shape)) <= 1.0


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("shape,rows", [CLASSES[0], CLASSES[4], CLASSES[5]], ids=[CLASS_IDS[0], CLASS_IDS[4], CLASS_IDS[5]])
def test_two_runs_are_bit_identical(shape, rows):
    assert _rows(shape) == rows
    c = _case(shape)
    f1, f2 = _run_forward(c), _run_forward(c)
    for name in R.OUTPUTS:
        assert torch.equal(f1[name], f2[name]), name
    assert torch.equal(_run_backward(c, c.dL, c.maps), _run_backward(c, c.dL, c.maps))
    gv = torch.tensor([0.5], dtype=torch.float32, device="cuda")
    g1, g2 = Arrays(c.n, 1), Arrays(c.n, 1)
    assert _backward_uniform(shape, c.a, c.b, gv, -0.2, float(c.n), c.maps, g1) == OK
    assert _backward_uniform(shape, c.a, c.b, gv, -0.2, float(c.n), c.maps, g2) == OK
    assert torch.equal(g1.buf, g2.buf)
