"""Float64 restatement of the fused SSIM operator (csrc/ssim.hip, include/gs2m_ssim.h), its closed-form derivative maps, its
backward, and two a-priori float32 error bounds.  Written from the formulas only; plain torch, so the same code runs in
float64 on the CPU (tests/test_ssim_ref.py) and on the device over every plane (tests/test_ssim_kernels_gpu.py).

The operator, per (B, CH) plane with zero "same" padding and the 11-tap window w (sigma 1.5, normalised in float32):

    mu1 = conv(a)   e1 = conv(a a)   mu2 = conv(b)   e2 = conv(b b)   e12 = conv(a b)          conv = w (x) w, separable
    s1 = e1 - mu1^2   s2 = e2 - mu2^2   s12 = e12 - mu1 mu2
    C = 2 mu1 mu2 + C1   D = 2 s12 + C2   A = mu1^2 + mu2^2 + C1   B = s1 + s2 + C2        map = C D / (A B)

The derivative maps are those of the map as a function of (mu1, s1, s12) with e1 = s1 + mu1^2 and e12 = s12 + mu1 mu2, i.e.
dm_dmu1 is the derivative along mu1 at fixed e1, e12, and dm_dsigma1_sq, dm_dsigma12 are the partials in e1 and e12:

    dm_dmu1 = 2 mu2 (D - C) / (A B) + 2 mu1 C D (1 / (A B^2) - 1 / (A^2 B))
    dm_dsigma1_sq = -C D / (A B^2)          dm_dsigma12 = 2 C / (A B)

so that dL/da = conv(dL dm_dmu1) + 2 a conv(dL dm_dsigma1_sq) + b conv(dL dm_dsigma12) (the window is symmetric).

ERROR BOUNDS (u = 2^-24, the unit roundoff of float32; every bound is evaluated in float64, per element)

bound_bwd.  The backward is linear in its float32 inputs.  Per term of x_q = dL dm_q: one product, an 11-term fmaf chain along
the row, an 11-term fmaf chain down the column (22 roundings), and the combination R0 + 2 a R1 + b R2 (two products, two
additions; at most 3 on one term, 4 allowed):
    bound_bwd = (22 + 4) u (conv|x0| + 2 |a| conv|x1| + |b| conv|x2|).

bound_fwd.  Each of the five sums q is two 11-term chains of non-negative terms (inputs are in [0, 1]) plus the product that
forms the term and the one with the weight: |dq| <= (22 + 2) u q_abs, q_abs the window sum of absolute values.  These are
pushed to first order through each output f in (map, dm_dmu1, dm_dsigma1_sq, dm_dsigma12): sum_q |df/dq| |dq|, partials by
float64 autograd of the epilogue.  The epilogue's own roundings add  N_f u max_i |z_i df/dz_i|:  z_i runs over the rounded
float32 intermediates of the kernel's expressions (the library is built with -ffp-contract=off, so each written operation
rounds once; multiplications by 2 and negations are exact), |z_i df/dz_i| is the magnitude of that intermediate measured at
the output (a relative error u of z_i moves f by u |z_i df/dz_i|), and N_f counts them:

    shared by all four (14): mu1 mu1, s1, mu2 mu2, s2, mu1 mu2, s12, C, D, A (two additions), B (two additions), A B, 1 / (A B)
    map (+2 = 16):           C D, (C D) r
    dm_dmu1 (+12 = 26):      2 mu2 D, (..) r, 2 mu2 C, (..) r, 2 mu1 C, (..) D, (..) r, (..) / A, (..) / B, three additions
    dm_dsigma1_sq (+3 = 17): C D, (..) r, (..) / B
    dm_dsigma12 (13):        the shared ones but s12 and D, which it does not read, and (2 C) r

Second order.  On flat patches s1 + s2 cancels to rounding against C2, so the relative perturbation of B is not tiny: with
delta = dA / A + dB / B (dA, dB the first-order bounds of A and B themselves, sums and roundings included) delta reaches ~1e-2 on
a white patch.  The outputs are polynomials in the sums over A^i B^j with i, j <= 2, so a first derivative carries at most
three inverse powers of one denominator more than the numerator; over the perturbation box every partial is within
(1 - delta)^-3 of its value at the centre (mean-value form of the remainder).  The first-order bound is therefore divided by
(1 - delta)^3.  This is the only second-order term kept: the cross terms between two numerator factors are below 2^-18 of the
first-order bound and are dropped.  There is no other multiplier.
"""
from math import exp

import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = float(np.float32(0.01 ** 2)), float(np.float32(0.03 ** 2))   # the float32 values the kernel is handed, widened
U = 2.0 ** -24
SUM_ROUNDINGS = 22 + 2      # per window sum
BWD_ROUNDINGS = 22 + 4      # per backward term
N_OPS = {"map": 16, "dm_dmu1": 26, "dm_dsigma1_sq": 17, "dm_dsigma12": 13}
OUTPUTS = ("map", "dm_dmu1", "dm_dsigma1_sq", "dm_dsigma12")
SUMS = ("mu1", "e1", "mu2", "e2", "e12")


def window32():
    """the 11 float32 weights as utils/loss_utils.py builds them: exp(-(x - 5)^2 / (2 * 1.5^2)), normalised in float32"""
    g = torch.tensor([exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    return g / g.sum()


def window(device="cpu"):
    return window32().double().to(device)


def conv(x, w=None):
    """(..., H, W) -> (..., H, W): the separable 11 x 11 window with zero "same" padding, as 2 x 11 shifted sums in x's dtype"""
    w = window(x.device).to(x.dtype) if w is None else w
    H, W = x.shape[-2:]
    p = F.pad(x, (5, 5, 0, 0))
    h = sum(w[k] * p[..., :, k:k + W] for k in range(11))
    p = F.pad(h, (0, 0, 5, 5))
    return sum(w[k] * p[..., k:k + H, :] for k in range(11))


def conv_direct(x):
    """One numpy float64 (H, W) plane, the 121 taps written out: what `conv` is checked against."""
    w = window().numpy()
    H, W = x.shape
    p = np.pad(np.asarray(x, dtype=np.float64), 5)
    out = np.zeros((H, W))
    for i in range(11):
        for j in range(11):
            out += (w[i] * w[j]) * p[i:i + H, j:j + W]
    return out


def window_sums(a, b):
    """-> (mu1, e1, mu2, e2, e12) in the dtype of a"""
    return conv(a), conv(a * a), conv(b), conv(b * b), conv(a * b)


def ssim_map_from_sums(mu1, e1, mu2, e2, e12, c1=C1, c2=C2):
    s1, s2, s12 = e1 - mu1 * mu1, e2 - mu2 * mu2, e12 - mu1 * mu2
    return ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))


def ssim_map(a, b, c1=C1, c2=C2):
    return ssim_map_from_sums(*window_sums(a, b), c1, c2)


def derivative_maps_from_sums(mu1, e1, mu2, e2, e12, c1=C1, c2=C2):
    """-> (dm_dmu1, dm_dsigma1_sq, dm_dsigma12), closed form"""
    Cc = 2 * mu1 * mu2 + c1
    Dd = 2 * (e12 - mu1 * mu2) + c2
    Aa = mu1 * mu1 + mu2 * mu2 + c1
    Bb = (e1 - mu1 * mu1) + (e2 - mu2 * mu2) + c2
    dmu1 = 2 * mu2 * (Dd - Cc) / (Aa * Bb) + 2 * mu1 * Cc * Dd * (1 / (Aa * Bb * Bb) - 1 / (Aa * Aa * Bb))
    return dmu1, -Cc * Dd / (Aa * Bb * Bb), 2 * Cc / (Aa * Bb)


def forward(a, b, c1=C1, c2=C2):
    """float64 -> dict of the four outputs"""
    q = window_sums(a, b)
    d = derivative_maps_from_sums(*q, c1, c2)
    return {"map": ssim_map_from_sums(*q, c1, c2), "dm_dmu1": d[0], "dm_dsigma1_sq": d[1], "dm_dsigma12": d[2]}


def backward(img1, img2, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12):
    """dL/dimg1 = conv(dL dmu1) + 2 img1 conv(dL dsigma1_sq) + img2 conv(dL dsigma12); the maps are inputs"""
    return conv(dL_dmap * dm_dmu1) + 2 * img1 * conv(dL_dmap * dm_dsigma1_sq) + img2 * conv(dL_dmap * dm_dsigma12)


def bound_bwd(img1, img2, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12):
    """float64 in (the float32 values the kernel is given, widened) -> the per-element bound of the module docstring"""
    x = [(dL_dmap * m).abs() for m in (dm_dmu1, dm_dsigma1_sq, dm_dsigma12)]
    return BWD_ROUNDINGS * U * (conv(x[0]) + 2 * img1.abs() * conv(x[1]) + img2.abs() * conv(x[2]))


def _kernel_epilogue(q, c1, c2):
    """The kernel's epilogue, operation by operation, on float64 leaves q = (mu1, e1, mu2, e2, e12).
    -> ({output: tensor}, {output: [every rounded intermediate the output depends on]})"""
    mu1, e1, mu2, e2, e12 = q
    p11 = mu1 * mu1; s1 = e1 - p11
    p22 = mu2 * mu2; s2 = e2 - p22
    p12 = mu1 * mu2; s12 = e12 - p12
    Cc = 2 * p12 + c1
    Dd = 2 * s12 + c2
    A0 = p11 + p22; Aa = A0 + c1
    B0 = s1 + s2; Bb = B0 + c2
    AB = Aa * Bb; r = 1 / AB
    shared = [p11, s1, p22, s2, p12, s12, Cc, Dd, A0, Aa, B0, Bb, AB, r]
    CD = Cc * Dd; m = CD * r
    t1 = (mu2 * 2) * Dd; t1r = t1 * r
    t2 = (mu2 * 2) * Cc; t2r = t2 * r
    t3 = (mu1 * 2) * Cc; t3d = t3 * Dd; t3r = t3d * r; t3a = t3r / Aa; t3b = t3r / Bb
    d0 = t1r - t2r; d1 = d0 - t3a; dmu1 = d1 + t3b
    nCD = (-Cc) * Dd; n1 = nCD * r; ds1 = n1 / Bb
    ds12 = (2 * Cc) * r
    out = {"map": m, "dm_dmu1": dmu1, "dm_dsigma1_sq": ds1, "dm_dsigma12": ds12}
    ops = {"map": shared + [CD, m], "dm_dmu1": shared + [t1, t1r, t2, t2r, t3, t3d, t3r, t3a, t3b, d0, d1, dmu1],
           "dm_dsigma1_sq": shared + [nCD, n1, ds1], "dm_dsigma12": [z for z in shared if z is not s12 and z is not Dd] + [ds12]}
    for k in OUTPUTS:
        assert len(ops[k]) == N_OPS[k]
    return out, ops, (A0, Aa, B0, Bb, p11, p22, s1, s2)


def bound_fwd(a, b, c1=C1, c2=C2):
    """float64 images in [0, 1] -> {output: per-element bound} (module docstring)"""
    with torch.enable_grad():
        q = [t.detach().requires_grad_(True) for t in window_sums(a, b)]
        dq = [SUM_ROUNDINGS * U * t.detach().abs() for t in q]   # non-negative terms: the sum of absolute values is the sum
        out, ops, (A0, Aa, B0, Bb, p11, p22, s1, s2) = _kernel_epilogue(q, c1, c2)
        first = {}
        for k in OUTPUTS:
            nodes = ops[k]
            g = torch.autograd.grad(out[k].sum(), q + nodes, retain_graph=True, allow_unused=True)   # dm_dsigma12 has no e12
            gq, gz = g[:5], g[5:]
            sums = sum(x.abs() * d for x, d in zip(gq, dq) if x is not None)
            mag = torch.zeros_like(sums)
            for z, x in zip(nodes, gz):   # (out[k] is its own last intermediate, df/dz = 1)
                mag = torch.maximum(mag, (z.detach() * x).abs())
            first[k] = sums + N_OPS[k] * U * mag
        mu1, e1, mu2, e2, e12 = [t.detach() for t in q]
        # first-order bounds of A and B themselves (sums, their products, and every addition on the way)
        dA = 2 * mu1 * dq[0] + 2 * mu2 * dq[2] + U * (p11 + p22 + A0.abs() + Aa.abs()).detach()
        dB = dq[1] + dq[3] + 2 * mu1 * dq[0] + 2 * mu2 * dq[2] + U * (p11 + p22 + s1.abs() + s2.abs() + B0.abs() + Bb.abs()).detach()
        delta = dA / Aa.detach() + dB / Bb.detach()
    assert float(delta.max()) < 0.25, "the perturbation of a denominator is no longer small"
    return {k: v / (1 - delta) ** 3 for k, v in first.items()}


def worst_ratio(err, bound):
    """max over the elements of err / bound; an error where the bound is 0 (every term is exactly 0 there) counts as infinite"""
    nz = bound > 0
    if bool((err[~nz] != 0).any()) or not bool(torch.isfinite(err).all()):
        return float("inf")
    return (err[nz] / bound[nz]).max().item() if bool(nz.any()) else 0.0


# ---------------------------------------------------------------- float32 evaluation of the same operator (the yardstick)
def _window2d32(ch):
    g = window32().unsqueeze(1)
    return g.mm(g.t()).float().unsqueeze(0).unsqueeze(0).expand(ch, 1, 11, 11).contiguous()


def _conv32(x):
    """(N, H, W) float32 -> depthwise conv2d with the float32 11 x 11 window, as tests/test_ssim_gpu.py::torch_ssim_map does"""
    x = x.unsqueeze(0)
    return F.conv2d(x, _window2d32(x.size(1)).to(x.device), padding=5, groups=x.size(1)).squeeze(0)


def forward32(a, b, c1=C1, c2=C2):
    """torch_ssim_map in float32, with the derivative maps by the kernel's expressions: a correct float32 implementation
    that owes nothing to the kernel's strip walk.  (N, H, W) float32 -> dict of the four outputs, float32"""
    c1, c2 = np.float32(c1).item(), np.float32(c2).item()
    mu1, mu2 = _conv32(a), _conv32(b)
    s1 = _conv32(a * a) - mu1 * mu1
    s2 = _conv32(b * b) - mu2 * mu2
    s12 = _conv32(a * b) - mu1 * mu2
    Cc, Dd = 2 * (mu1 * mu2) + c1, 2 * s12 + c2
    Aa, Bb = mu1 * mu1 + mu2 * mu2 + c1, s1 + s2 + c2
    r = 1 / (Aa * Bb)
    dmu1 = (mu2 * 2 * Dd) * r - (mu2 * 2 * Cc) * r - (mu1 * 2 * Cc * Dd) * r / Aa + (mu1 * 2 * Cc * Dd) * r / Bb
    return {"map": (Cc * Dd) * r, "dm_dmu1": dmu1, "dm_dsigma1_sq": (-Cc * Dd) * r / Bb, "dm_dsigma12": (2 * Cc) * r}


def backward32(img1, img2, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12):
    return _conv32(dL_dmap * dm_dmu1) + 2 * img1 * _conv32(dL_dmap * dm_dsigma1_sq) + img2 * _conv32(dL_dmap * dm_dsigma12)


# ---------------------------------------------------------------- inputs
def make_images(shape, seed):
    """(B, CH, H, W) -> float32 img1, img2 in [0, 1] on the CPU.  Every plane mixes: uniform noise; a well-matched left half;
    a rectangle where img1 == img2; a rectangle with a step edge (the same step in both images on even planes, shifted by one
    column and inverted in contrast on odd ones); six flat patches of 13 x 13 (clipped to the plane) at 0, 1 and 0.5 in both
    images, and at 0, 1 in img1 only and 0.37 in img2 only.  With 8 planes or more, planes 1, 2, 3 are flat throughout:
    black / black, white / white, white / black."""
    B, CH, H, W = shape
    N = B * CH
    gen = torch.Generator().manual_seed(seed)
    a = torch.rand((N, H, W), generator=gen)
    b = torch.rand((N, H, W), generator=gen)
    b[..., : W // 2] = (a[..., : W // 2] + 0.05 * b[..., : W // 2]).clamp(0, 1)
    pos = torch.rand((N, 8, 2), generator=gen).numpy()
    rh, rw = max(1, H // 3), max(1, W // 3)
    ph, pw = min(13, H), min(13, W)
    for n in range(N):
        def at(k, h, w):
            return int(pos[n, k, 0] * (H - h + 1)), int(pos[n, k, 1] * (W - w + 1))
        y, x = at(0, rh, rw)
        b[n, y:y + rh, x:x + rw] = a[n, y:y + rh, x:x + rw]
        y, x = at(1, rh, rw)
        c = x + rw // 2
        a[n, y:y + rh, x:c], a[n, y:y + rh, c:x + rw] = 0.1, 0.9
        if n % 2 == 0:
            b[n, y:y + rh, x:x + rw] = a[n, y:y + rh, x:x + rw]
        else:
            b[n, y:y + rh, x:min(c + 1, x + rw)], b[n, y:y + rh, min(c + 1, x + rw):x + rw] = 0.8, 0.2
        for k, (va, vb) in enumerate(((0.0, 0.0), (1.0, 1.0), (0.5, 0.5), (0.0, None), (1.0, None), (None, 0.37))):
            y, x = at(2 + k, ph, pw)
            if va is not None:
                a[n, y:y + ph, x:x + pw] = va
            if vb is not None:
                b[n, y:y + ph, x:x + pw] = vb
    if N >= 8:
        a[1], b[1] = 0.0, 0.0
        a[2], b[2] = 1.0, 1.0
        a[3], b[3] = 1.0, 0.0
    return a.reshape(shape).contiguous(), b.reshape(shape).contiguous()


def make_backward_inputs(shape, seed):
    """Caller-made float32 inputs of the backward that come from no forward: three signed maps whose magnitudes span six
    decades (1e-3 .. 1e3), and a dL_dmap spanning 1e-6 .. 1 with every fifth row and every seventh column zero (and, on a plane of
    22 x 22 or more, the first plane's leading 11 x 11 corner)."""
    gen = torch.Generator().manual_seed(seed + 7919)

    def signed(lo, hi):
        mag = 10.0 ** (lo + (hi - lo) * torch.rand(shape, generator=gen))
        return (mag * torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)).float()
    maps = [signed(-3, 3) for _ in range(3)]
    dL = signed(-6, 0)
    dL[..., 2::5, :] = 0
    dL[..., :, 3::7] = 0
    if shape[2] >= 22 and shape[3] >= 22:
        dL[0, 0, :11, :11] = 0
    return dL.contiguous(), [m.contiguous() for m in maps]
