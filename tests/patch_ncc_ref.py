"""Float64 arbiters of the photometric half of csrc/mvs.hip -- patch_ncc_kernel<false / true>, patch_ncc_rough_kernel and
grid_border_kernel with det_finalize_kernel -- and the scenes those kernels are tested on.  CPU only, no device import.

Written from the kernel's contract (the header comment of csrc/mvs.hip, include/gs2m_mvs.h), NOT from gs2m_mvs.patch_ncc_torch,
which tests/test_patch_ncc_ref.py cross-checks against the same recorded outputs of the reference:

  `restate`        the patch-NCC chain in float64 torch: the warp h = M p - b (n . r) / d with the +1e-10, zero-padded bilinear
                   sampling of both grey images, the five sums, 1 - cross^2 / (var var + 1e-8) clamped to [0, 2], the NCC of
                   the 3x3 Sobel magnitudes and ref_var; differentiable by autograd with respect to normals and distances.
  `chain`          the same contract in numpy at a chosen precision, backward by hand (centred sums, row-major patch order,
                   serial summation): at float32 it is the YARDSTICK of what float32 can do on these inputs, at float64 it
                   supplies every per-tap term that the error scales and the margins are built from.
  `error_scales`   a first-order float32 error scale e_i per sample for every output and gradient component, from the sample's
                   own float64 terms: the rounding of the taps (position error x bilinear slope) and of the five sums is carried
                   through cross, the variances, D and the quotient, and in the backward through g_cross, g_var, the lookups'
                   derivatives and the chain to n and d.
  `classify`       flip band (a decision margin is below what float32 resolves: the sample is left out of the comparison the
                   margin belongs to), stiff class (D within a few orders of the 1e-8 guard, perfectly correlated patches, tiny
                   |hz|: compared against their own error scale, with their own K), the rest.
  `grid_restate`   the border grid-sample in float64: un-normalise, clip (position gradient zeroed where the clip binds, a NaN
                   position clips to 0), bilinear lookup; an exact dense scatter for d_img; `grid_yardstick` in numpy float32.

The bound of every GPU comparison is |got - f64| <= K e_i.  K is 3 x the largest ratio |float32 yardstick - f64| / e_i over all
scenes (`measure`), per output and class; the factor 3 covers the kernel's different summation order (eight partial sums and a
butterfly) and the hardware division.  K is never derived from a kernel's output.  The measured ratios are the constants below;
tests/test_patch_ncc_ref.py asserts that they still hold.
"""
import functools
import math
import types

import numpy as np
import torch

from mv_geo_ref import RefCam, dense_scatter  # noqa: F401  (RefCam: the cameras are plain numbers)

F64 = torch.float64
U = 2.0 ** -24          # unit roundoff of float32
STIFF_D = 1e3           # D = var_ref var_near + 1e-8 below STIFF_D x 1e-8: the guard decides the quotient
STIFF_CORR = 1e-3       # raw = 1 - cross^2 / D below this: perfectly correlated patches, the value is the rounding of 1 - (1 - tiny)
STIFF_HZ = 1e-2         # min |hz| over the patch below this share of hz's largest term: the projective division amplifies everything
SAFETY = 3.0            # K = SAFETY x the measured yardstick ratio
BAND = 4.0              # a threshold (raw at 0 and 2, ncc at 0.9, sqrt(ref_var) at 0.01) is within its band when BAND x the error scale
                        # of the compared quantity reaches it; K of those quantities must not exceed BAND (asserted on the CPU)

# Largest |float32 yardstick - float64| / e_i over every scene and patch size of `cases()`, outside the flip band, per output and
# class (regular, stiff), as `python tests/patch_ncc_ref.py` prints them (rounded up to two digits).
RATIO = {
    "ncc": (0.40, 0.0032), "d_normals": (0.022, 5.7e-6), "d_dists": (0.017, 4.4e-6),
    "ncc_grad": (0.13, 0.0045), "ref_var": (0.88, 0.079),
    "grid_out": (0.34, 0.34), "d_grid": (0.36, 0.36), "d_img": (0.24, 0.24),
}
# The largest ratios come from the scenes whose patches reach over the image border (taps of 0 next to taps of 0.5: large centred
# sums); on the production scene the yardstick stays below 0.02 e_i -- the scale is a bound, not an estimate.  The stiff class holds
# few samples, so its K is taken from the larger of the two measured ratios: e_i is already the sample's own scale, the classes are
# separated only so that the stiff samples' ratios cannot widen the others' bound.
K = {k: (SAFETY * a, SAFETY * max(a, b)) for k, (a, b) in RATIO.items()}


def kbound(name, stiff):
    """K of output `name` per sample: the stiff class has its own."""
    stiff = np.asarray(stiff)
    return np.where(stiff, K[name][1], K[name][0])


# ---------------------------------------------------------------- cameras, constants, images
def homography_constants(ref, near, ncc_scale):
    """M = K_near R_rn K_ref^-1, b = K_near t_rn, K_ref^-1 at the NCC scale (x_near = R_rn x_ref + t_rn), computed in float64 and
    rounded to float32 -- what the kernel is handed -- returned as float64 numpy arrays (9, 3, 9)."""
    Vr, Vn = ref.V.numpy(), near.V.numpy()
    R = Vn[:3, :3].T @ Vr[:3, :3]
    t = Vn[3, :3] - R @ Vr[3, :3]
    s = float(ncc_scale)
    Kn = np.array([[near.Fx / s, 0.0, near.Cx / s], [0.0, near.Fy / s, near.Cy / s], [0.0, 0.0, 1.0]])
    Ki = np.array([[s / ref.Fx, 0.0, -ref.Cx / ref.Fx], [0.0, s / ref.Fy, -ref.Cy / ref.Fy], [0.0, 0.0, 1.0]])
    f = lambda a: a.reshape(-1).astype(np.float32).astype(np.float64)
    return f(Kn @ R @ Ki), f(Kn @ t), f(Ki)


def project_camera(cam, gray, device="cpu"):
    """mv_geo_ref.RefCam.project_camera plus what gs2m_mvs.patch_ncc_torch reads: gray_image (1, h, w), get_K, get_inv_K."""
    c = cam.project_camera(device)
    c.gray_image = torch.as_tensor(gray, dtype=torch.float32).reshape(1, *gray.shape[-2:]).to(device)
    c.get_K = lambda s=1.0: torch.tensor([[c.Fx / s, 0.0, c.Cx / s], [0.0, c.Fy / s, c.Cy / s], [0.0, 0.0, 1.0]], device=device)
    c.get_inv_K = lambda s=1.0: torch.tensor([[s / c.Fx, 0.0, -c.Cx / c.Fx], [0.0, s / c.Fy, -c.Cy / c.Fy], [0.0, 0.0, 1.0]], device=device)
    return c


PLANE_N = np.array([0.15, -0.1, -1.0]) / np.linalg.norm([0.15, -0.1, -1.0])
PLANE_P = np.array([0.0, 0.0, 6.0])


def _texture(u, v):
    return (0.5 + 0.2 * np.sin(3.1 * u + 0.3) * np.cos(2.3 * v) + 0.15 * np.sin(5.7 * v + 1.0) + 0.1 * np.cos(4.1 * (u + v))
            + 0.06 * np.sin(23.0 * u + 0.7) * np.sin(19.0 * v))


def plane_image(cam, ncc_scale=1.0):
    """The grey image (h, w) = (H / scale, W / scale) a camera sees of the textured plane through PLANE_P: the texture at each
    pixel's ray / plane intersection (float64, then rounded to float32)."""
    s = float(ncc_scale)
    w, h = int(cam.W / s), int(cam.H / s)
    V = cam.V.numpy()
    centre = -V[3, :3] @ V[:3, :3].T
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    rays_c = np.stack([(s * u - cam.Cx) / cam.Fx, (s * v - cam.Cy) / cam.Fy, np.ones_like(u)], -1).reshape(-1, 3)
    rays_w = rays_c @ V[:3, :3].T
    t = ((PLANE_P - centre) @ PLANE_N) / (rays_w @ PLANE_N)
    X = centre + t[:, None] * rays_w - PLANE_P
    e1 = np.cross(PLANE_N, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(PLANE_N, e1)
    return _texture(X @ e1, X @ e2).reshape(h, w).astype(np.float32)


def true_plane(cam):
    """-> camera-space normal (3,) facing the camera and distance of the textured plane: n . X = -d."""
    V = cam.V.numpy()
    centre = -V[3, :3] @ V[:3, :3].T
    return PLANE_N @ V[:3, :3], abs((centre - PLANE_P) @ PLANE_N)


# ---------------------------------------------------------------- (a) the float64 restatement, torch autograd
def _sample_zero_t(img, x, y):
    """Zero-padded bilinear lookup of img (h, w) at pixel positions (x, y): 0 unless -1 < x < w and -1 < y < h (a NaN
    position: 0); texels outside the image count as 0.  Differentiable with respect to the position."""
    h, w = img.shape
    inside = (x > -1) & (x < w) & (y > -1) & (y < h)
    xs, ys = torch.where(inside, x, torch.zeros_like(x)), torch.where(inside, y, torch.zeros_like(y))
    xf, yf = xs.detach().floor(), ys.detach().floor()
    x0, y0 = xf.long(), yf.long()
    fx, fy = xs - xf, ys - yf

    def at(xx, yy):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return torch.where(ok, img[yy.clamp(0, h - 1), xx.clamp(0, w - 1)], torch.zeros_like(x))

    v = at(x0, y0) * (1 - fx) * (1 - fy) + at(x0 + 1, y0) * fx * (1 - fy) + at(x0, y0 + 1) * (1 - fx) * fy + at(x0 + 1, y0 + 1) * fx * fy
    return torch.where(inside, v, torch.zeros_like(v))


def _ncc_t(r, v):
    """(N, T) patches -> raw, and (Sr, Sn, Srr, Snn, Srn, cross, ref_var, nea_var, D)."""
    T = r.shape[1]
    Sr, Sn, Srr, Snn, Srn = r.sum(1), v.sum(1), (r * r).sum(1), (v * v).sum(1), (r * v).sum(1)
    ra, na = Sr / T, Sn / T
    cross, rvar, nvar = Srn - na * Sr, Srr - ra * Sr, Snn - na * Sn
    D = rvar * nvar + 1e-8
    return 1 - cross * cross / D, (Sr, Sn, Srr, Snn, Srn, cross, rvar, nvar, D)


def _sobel_t(P):
    """(N, ps, ps) patches indexed [a][b] (a: the x offset, b: the y offset, as the reference's _patch_offsets orders them)
    -> 3x3 Sobel magnitude sqrt(gx^2 + gy^2 + 1e-6) with zero padding at the patch border."""
    Z = torch.nn.functional.pad(P, (1, 1, 1, 1))
    s = lambda da, db: Z[:, 1 + da:1 + da + P.shape[1], 1 + db:1 + db + P.shape[2]]
    gx = (s(-1, 1) - s(-1, -1)) + 2 * (s(0, 1) - s(0, -1)) + (s(1, 1) - s(1, -1))
    gy = (s(1, -1) - s(-1, -1)) + 2 * (s(1, 0) - s(-1, 0)) + (s(1, 1) - s(-1, 1))
    return torch.sqrt(gx * gx + gy * gy + 1e-6)


def restate(pixels, normals, dists, ref_gray, near_gray, M, b, Kinv, ncc_scale, patch):
    """All float64 torch tensors (normals / dists leaves with requires_grad for gradients); grey images (h, w).
    -> namespace: ncc (clamped), raw, mask (ncc < 0.9), the five sums, cross, ref_var, nea_var, D, ncc_grad (Sobel magnitudes),
    switch (sqrt(ref_var) < 0.01), hz (N, T) and q (N, T, 2)."""
    assert all(t.dtype == F64 for t in (pixels, normals, dists, ref_gray, near_gray, M, b, Kinv))
    P = int(patch)
    ps = 2 * P + 1
    o = torch.arange(-P, P + 1, dtype=F64)
    c = pixels / ncc_scale
    px = (c[:, 0, None, None] + o[None, None, :]).expand(-1, ps, ps).reshape(-1, ps * ps)   # row major: oy outer, ox inner
    py = (c[:, 1, None, None] + o[None, :, None]).expand(-1, ps, ps).reshape(-1, ps * ps)
    rx, ry, rz = (Kinv[3 * i] * px + Kinv[3 * i + 1] * py + Kinv[3 * i + 2] for i in range(3))
    s = normals[:, 0:1] * rx + normals[:, 1:2] * ry + normals[:, 2:3] * rz
    k = s / dists[:, None]
    hx, hy, hz = (M[3 * i] * px + M[3 * i + 1] * py + M[3 * i + 2] - b[i] * k for i in range(3))
    hz = hz + 1e-10
    qx, qy = hx / hz, hy / hz
    r = _sample_zero_t(ref_gray, px, py)
    v = _sample_zero_t(near_gray, qx, qy)
    centre = P * ps + P
    raw, (Sr, Sn, Srr, Snn, Srn, cross, rvar, nvar, D) = _ncc_t(r - r[:, centre:centre + 1], v - v[:, centre:centre + 1])
    ncc = raw.clamp(0.0, 2.0)
    tr = lambda t: t.reshape(-1, ps, ps).transpose(1, 2)   # [a = x offset][b = y offset]
    gr, gv = _sobel_t(tr(r)).reshape(-1, ps * ps), _sobel_t(tr(v)).reshape(-1, ps * ps)
    raw_g, _ = _ncc_t(gr - gr[:, centre:centre + 1], gv - gv[:, centre:centre + 1])
    return types.SimpleNamespace(ncc=ncc, raw=raw, mask=ncc < 0.9, Sr=Sr, Sn=Sn, Srr=Srr, Snn=Snn, Srn=Srn, cross=cross, ref_var=rvar, nea_var=nvar,
                                 D=D, ncc_grad=raw_g.clamp(0.0, 2.0), switch=torch.sqrt(rvar) < 0.01, hz=hz, q=torch.stack([qx, qy], -1))


# ---------------------------------------------------------------- the contract in numpy at a chosen precision, backward by hand
def _ssum(x, dt):
    """Serial sum over axis 1 in precision dt, first to last."""
    return np.cumsum(x, axis=1, dtype=dt)[:, -1]


def _sample_zero_np(img, x, y, dt):
    """-> value, d/dx, d/dy, the mixed second difference v11 - v10 - v01 + v00 and the largest |texel| of the footprint."""
    h, w = img.shape
    inside = (x > -1) & (x < w) & (y > -1) & (y < h)
    xs, ys = np.where(inside, x, dt(0)), np.where(inside, y, dt(0))
    xf, yf = np.floor(xs), np.floor(ys)
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    fx, fy = xs - xf, ys - yf

    def at(xx, yy):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h) & inside
        return np.where(ok, img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], dt(0))

    one = dt(1)
    v00, v10, v01, v11 = at(x0, y0), at(x0 + 1, y0), at(x0, y0 + 1), at(x0 + 1, y0 + 1)
    v = v00 * (one - fx) * (one - fy) + v10 * fx * (one - fy) + v01 * (one - fx) * fy + v11 * fx * fy
    dx = (v10 - v00) * (one - fy) + (v11 - v01) * fy
    dy = (v01 - v00) * (one - fx) + (v11 - v10) * fx
    amax = np.maximum(np.maximum(np.abs(v00), np.abs(v10)), np.maximum(np.abs(v01), np.abs(v11)))
    return v, dx, dy, v11 - v10 - v01 + v00, amax


def _ncc_np(r, v, dt):
    T = dt(r.shape[1])
    Sr, Sn, Srr, Snn, Srn = _ssum(r, dt), _ssum(v, dt), _ssum(r * r, dt), _ssum(v * v, dt), _ssum(r * v, dt)
    ra, na = Sr / T, Sn / T
    cross, rvar, nvar = Srn - na * Sr, Srr - ra * Sr, Snn - na * Sn
    D = rvar * nvar + dt(1e-8)
    raw = dt(1) - cross * cross / D
    return types.SimpleNamespace(Sr=Sr, Sn=Sn, Srr=Srr, Snn=Snn, Srn=Srn, ra=ra, na=na, cross=cross, ref_var=rvar, nea_var=nvar, D=D, raw=raw,
                                 ncc=np.minimum(np.maximum(raw, dt(0)), dt(2)))


def _sobel_np(P, dt):
    Z = np.pad(P, ((0, 0), (1, 1), (1, 1)))
    n = P.shape[1]
    s = lambda da, db: Z[:, 1 + da:1 + da + n, 1 + db:1 + db + n]
    gx = (s(-1, 1) - s(-1, -1)) + dt(2) * (s(0, 1) - s(0, -1)) + (s(1, 1) - s(1, -1))
    gy = (s(1, -1) - s(-1, -1)) + dt(2) * (s(1, 0) - s(-1, 0)) + (s(1, 1) - s(-1, 1))
    return np.sqrt(gx * gx + gy * gy + dt(1e-6)), gx, gy


def chain(pixels, normals, dists, ref_gray, near_gray, M, b, Kinv, ncc_scale, patch, d_ncc=None, dtype=np.float64):
    """The kernel's contract evaluated in `dtype` with numpy: inputs are converted to it first (they are float32 values).  Centred
    sums, row-major patch order, serial summation, the backward as the header states it.  -> namespace of every term."""
    dt = dtype
    with np.errstate(all="ignore"):
        c = lambda a: np.asarray(a, dtype=np.float64).astype(dt)
        pixels, normals, dists, ref_gray, near_gray, M, b, Kinv = (c(a) for a in (pixels, normals, dists, ref_gray, near_gray, M, b, Kinv))
        P = int(patch)
        ps = 2 * P + 1
        T = ps * ps
        inv_scale = dt(1) / dt(ncc_scale)
        cx, cy = pixels[:, 0] * inv_scale, pixels[:, 1] * inv_scale
        o = np.arange(-P, P + 1).astype(dt)
        px = np.broadcast_to(cx[:, None, None] + o[None, None, :], (len(cx), ps, ps)).reshape(-1, T)
        py = np.broadcast_to(cy[:, None, None] + o[None, :, None], (len(cx), ps, ps)).reshape(-1, T)
        rx, ry, rz = (Kinv[3 * i] * px + Kinv[3 * i + 1] * py + Kinv[3 * i + 2] for i in range(3))
        s = normals[:, 0:1] * rx + normals[:, 1:2] * ry + normals[:, 2:3] * rz
        inv_d = (dt(1) / dists)[:, None]
        k = s * inv_d
        hx, hy, hz = (M[3 * i] * px + M[3 * i + 1] * py + M[3 * i + 2] - b[i] * k for i in range(3))
        hz = hz + dt(1e-10)
        qx, qy = hx / hz, hy / hz
        rv, rdx, rdy, _, ramax = _sample_zero_np(ref_gray, px, py, dt)
        bv, bdx, bdy, bxy, bamax = _sample_zero_np(near_gray, qx, qy, dt)
        ctr = P * ps + P
        r, v = rv - rv[:, ctr:ctr + 1], bv - bv[:, ctr:ctr + 1]
        n = _ncc_np(r, v, dt)
        out = types.SimpleNamespace(**vars(n), T=T, px=px, py=py, r3=(rx, ry, rz), s=s, inv_d=inv_d, h=(hx, hy, hz), qx=qx, qy=qy, r=r, v=v,
                                    rv=rv, bv=bv, rdx=rdx, rdy=rdy, ramax=ramax, bdx=bdx, bdy=bdy, bxy=bxy, bamax=bamax)
        tr = lambda t: t.reshape(-1, ps, ps).transpose(0, 2, 1)
        (gr, grx, gry), (gv, gvx, gvy) = _sobel_np(tr(rv), dt), _sobel_np(tr(bv), dt)
        gr, gv = gr.reshape(-1, T), gv.reshape(-1, T)
        out.sobel = _ncc_np(gr - gr[:, ctr:ctr + 1], gv - gv[:, ctr:ctr + 1], dt)
        out.gr, out.gv, out.sob_parts = gr, gv, (grx.reshape(-1, T), gry.reshape(-1, T), gvx.reshape(-1, T), gvy.reshape(-1, T))
        out.ncc_grad = out.sobel.ncc
        if d_ncc is not None:
            d_ncc = c(d_ncc).reshape(-1)
            g = np.where((n.raw >= 0) & (n.raw <= 2), -d_ncc, dt(0))
            g_cross = g * dt(2) * n.cross / n.D
            g_var = -g * n.cross * n.cross * n.ref_var / (n.D * n.D)
            gvk = g_cross[:, None] * (r - n.ra[:, None]) + g_var[:, None] * (dt(2) * v - dt(2) * n.na[:, None])
            gqx, gqy = gvk * bdx, gvk * bdy
            ghx, ghy, ghz = gqx / hz, gqy / hz, -(gqx * qx + gqy * qy) / hz
            gb = ghx * b[0] + ghy * b[1] + ghz * b[2]
            kk = -gb * inv_d
            live = (g != 0)
            dn = np.stack([np.where(live, _ssum(kk * ri, dt), dt(0)) for ri in (rx, ry, rz)], axis=1)
            dd = np.where(live, _ssum(gb * s * inv_d * inv_d, dt), dt(0))
            out.g, out.g_cross, out.g_var, out.gvk, out.gb, out.d_normals, out.d_dists = g, g_cross, g_var, gvk, gb, dn, dd
    return out


# ---------------------------------------------------------------- (c) first-order float32 error scales
def _ncc_escale(n, r, v, dr, dv):
    """The error of the five sums (tap errors dr, dv (N, T) plus sqrt(T) roundings of the accumulation) through cross, the
    variances, D and the quotient.  -> namespace of the d-terms."""
    T = r.shape[1]
    A = math.sqrt(T) + 1.0
    ab = np.abs
    dSr = dr.sum(1) + A * U * ab(r).sum(1)
    dSn = dv.sum(1) + A * U * ab(v).sum(1)
    dSrr = (2 * ab(r) * dr).sum(1) + (A + 1) * U * (r * r).sum(1)
    dSnn = (2 * ab(v) * dv).sum(1) + (A + 1) * U * (v * v).sum(1)
    dSrn = (ab(r) * dv + ab(v) * dr).sum(1) + (A + 1) * U * ab(r * v).sum(1)
    dra, dna = dSr / T + U * ab(n.ra), dSn / T + U * ab(n.na)
    dcross = dSrn + ab(n.na) * dSr + ab(n.Sr) * dna + U * (ab(n.Srn) + 2 * ab(n.na * n.Sr))
    drvar = dSrr + ab(n.ra) * dSr + ab(n.Sr) * dra + U * (ab(n.Srr) + 2 * ab(n.ra * n.Sr))
    dnvar = dSnn + ab(n.na) * dSn + ab(n.Sn) * dna + U * (ab(n.Snn) + 2 * ab(n.na * n.Sn))
    dD = ab(n.nea_var) * drvar + ab(n.ref_var) * dnvar + 2 * U * ab(n.D)
    cc = n.cross * n.cross / n.D
    draw = 2 * ab(n.cross) * dcross / n.D + cc * dD / n.D + 3 * U * cc + U * np.maximum(1.0, ab(n.raw))
    return types.SimpleNamespace(dra=dra, dna=dna, dcross=dcross, drvar=drvar, dnvar=dnvar, dD=dD, draw=draw)


def error_scales(f):
    """f: `chain(..., dtype=float64)` (with d_ncc for the gradient scales), b: the constants -> dict of per-sample scales:
    ncc, raw, ncc_grad, ref_var (N,), d_normals (N, 3), d_dists (N,), and eq (N, T, 2): the float32 position error of each tap."""
    ab = np.abs
    with np.errstate(all="ignore"):
        hx, hy, hz = f.h
        M, b = f.consts[0], f.consts[1]
        # the rounded chain of one homogeneous coordinate, operation by operation (each rounds by U x its own result):
        # r_j = (Kinv_j0 px + Kinv_j1 py) + Kinv_j2; s = (n0 rx + n1 ry) + n2 rz; k = s (1 / d); h_i = ((M_i0 px + M_i1 py) + M_i2) - b_i k
        Ki, nrm, k = f.consts[2], f.normals, f.s * f.inv_d
        dp = U * ab(f.px), U * ab(f.py)                                      # px = cx + ox (exact for integer pixels; bounded as rounded)
        dr = []
        for j, rj in enumerate(f.r3):
            t0, t1 = Ki[3 * j] * f.px, Ki[3 * j + 1] * f.py
            dr.append(U * (ab(t0) + ab(t1) + ab(t0 + t1) + ab(rj)) + ab(Ki[3 * j]) * dp[0] + ab(Ki[3 * j + 1]) * dp[1])
        t = [nrm[:, j:j + 1] * f.r3[j] for j in range(3)]
        ds_ = U * (ab(t[0]) + ab(t[1]) + ab(t[2]) + ab(t[0] + t[1]) + ab(f.s)) + sum(ab(nrm[:, j:j + 1]) * dr[j] for j in range(3))
        dk = ab(f.inv_d) * ds_ + 2 * U * ab(k)
        eh = []
        for i, h in enumerate((hx, hy, hz)):
            t0, t1 = M[3 * i] * f.px, M[3 * i + 1] * f.py
            eh.append(U * (ab(t0) + ab(t1) + ab(t0 + t1) + ab(t0 + t1 + M[3 * i + 2]) + ab(h) + ab(b[i] * k)) + ab(b[i]) * dk
                      + ab(M[3 * i]) * dp[0] + ab(M[3 * i + 1]) * dp[1] + (U * ab(h) if i == 2 else 0.0))
        eqx = (eh[0] + ab(f.qx) * eh[2]) / ab(hz) + U * ab(f.qx)
        eqy = (eh[1] + ab(f.qy) * eh[2]) / ab(hz) + U * ab(f.qy)
        eqx, eqy = np.nan_to_num(eqx, nan=np.inf), np.nan_to_num(eqy, nan=np.inf)
        z = lambda slope, e: np.where(slope == 0, 0.0, ab(slope) * np.where(np.isfinite(e), e, 1e30))   # 0 slope x unbounded error = 0
        dbv = z(f.bdx, eqx) + z(f.bdy, eqy) + 4 * U * f.bamax
        drv = (ab(f.rdx) * ab(f.px) + ab(f.rdy) * ab(f.py)) * U + 4 * U * f.ramax
        ctr = f.T // 2
        dr, dv = drv + drv[:, ctr:ctr + 1] + U * ab(f.r), dbv + dbv[:, ctr:ctr + 1] + U * ab(f.v)
        e = _ncc_escale(f, f.r, f.v, dr, dv)
        out = {"raw": e.draw, "ncc": np.minimum(e.draw, 2.0), "ref_var": e.drvar, "eq": np.stack([eqx, eqy], -1)}
        # the Sobel magnitudes: each is a combination of up to 8 taps with weights 1, 2, 1
        ps = int(round(math.sqrt(f.T)))
        tr = lambda t: t.reshape(-1, ps, ps).transpose(0, 2, 1)
        spread = lambda t: _sobel_abs(tr(t)).reshape(-1, f.T)
        grx, gry, gvx, gvy = f.sob_parts
        dgr = (ab(grx) + ab(gry)) * spread(drv) / f.gr + 6 * U * f.gr
        dgv = (ab(gvx) + ab(gvy)) * spread(dbv) / f.gv + 6 * U * f.gv
        gr, gv = f.gr - f.gr[:, ctr:ctr + 1], f.gv - f.gv[:, ctr:ctr + 1]
        es = _ncc_escale(f.sobel, gr, gv, dgr + dgr[:, ctr:ctr + 1] + U * ab(gr), dgv + dgv[:, ctr:ctr + 1] + U * ab(gv))
        out["ncc_grad"] = np.minimum(es.draw, 2.0)
        if hasattr(f, "g"):
            g, D = ab(f.g), f.D
            dgc = 2 * g * (e.dcross / D + ab(f.cross) * e.dD / (D * D)) + 3 * U * ab(f.g_cross)
            dgvar = g * (2 * ab(f.cross) * f.ref_var * e.dcross + f.cross ** 2 * e.drvar) / (D * D) + 2 * ab(f.g_var) * e.dD / D + 5 * U * ab(f.g_var)
            rc, vc = f.r - f.ra[:, None], f.v - f.na[:, None]
            dgv_k = (dgc[:, None] * ab(rc) + ab(f.g_cross)[:, None] * (dr + e.dra[:, None]) + 2 * dgvar[:, None] * ab(vc)
                     + 2 * ab(f.g_var)[:, None] * (dv + e.dna[:, None]) + 3 * U * (ab(f.g_cross[:, None] * rc) + 2 * ab(f.g_var[:, None] * vc)))
            dbdx, dbdy = z(f.bxy, eqy) + 4 * U * f.bamax, z(f.bxy, eqx) + 4 * U * f.bamax
            jx, jy = (b[0] - f.qx * b[2]) / hz, (b[1] - f.qy * b[2]) / hz
            djx = (ab(b[2]) * eqx + 3 * U * (ab(b[0]) + ab(f.qx * b[2]))) / ab(hz) + ab(jx) * eh[2] / ab(hz)
            djy = (ab(b[2]) * eqy + 3 * U * (ab(b[1]) + ab(f.qy * b[2]))) / ab(hz) + ab(jy) * eh[2] / ab(hz)
            tx, ty = ab(f.bdx * jx), ab(f.bdy * jy)
            dgb = (dgv_k * (tx + ty) + ab(f.gvk) * (z(jx, dbdx) + z(f.bdx, djx) + z(jy, dbdy) + z(f.bdy, djy)) + 6 * U * ab(f.gvk) * (tx + ty))
            dgb = np.where(f.g[:, None] == 0, 0.0, dgb)
            A = math.sqrt(f.T) + 1.0
            gbk = np.where(f.g[:, None] == 0, 0.0, ab(f.gb))
            idd = ab(f.inv_d)
            out["d_normals"] = np.stack([((dgb * ab(ri)).sum(1) + (A + 4) * U * (gbk * ab(ri)).sum(1)) * idd[:, 0] for ri in f.r3], axis=1)
            ds = 3 * U * sum(ab(f.normals[:, i:i + 1]) * ab(ri) for i, ri in enumerate(f.r3))
            out["d_dists"] = ((dgb * ab(f.s)).sum(1) + (gbk * ds).sum(1) + (A + 5) * U * (gbk * ab(f.s)).sum(1)) * idd[:, 0] ** 2
    return out


def _sobel_abs(E):
    """The Sobel weights' absolute values applied to per-tap errors E (N, ps, ps): a bound of the error of gx (and of gy)."""
    Z = np.pad(E, ((0, 0), (1, 1), (1, 1)))
    n = E.shape[1]
    s = lambda da, db: Z[:, 1 + da:1 + da + n, 1 + db:1 + db + n]
    return s(-1, 1) + s(-1, -1) + 2 * (s(0, 1) + s(0, -1)) + s(1, 1) + s(1, -1) + s(1, 0) + s(-1, 0)


# ---------------------------------------------------------------- (b) margins and classes
def classify(f, e):
    """f: chain at float64, e: error_scales(f).  -> dict of (N,) arrays: the float64 margins ("cell", "pad", "gate", "mask",
    "switch", "hz") and the bool classes flip_mask, flip_switch, flip_grad, stiff, nonfinite.
    Bands: a near-image tap is on a cell line (or on a padding limit, which are the cell lines -1 and w) when its float32 position
    error eq -- the rounded chain of h, operation by operation, carried through the division -- reaches the line; raw, ncc and sqrt(ref_var)
    are on their thresholds when BAND x their own error scale reaches them."""
    with np.errstate(all="ignore"):
        h, w = f.shape
        q = np.stack([f.qx, f.qy], -1)
        lim = np.array([w, h], dtype=np.float64)
        near_img = (q > -1.5).all(-1) & (q < lim + 0.5).all(-1)
        cell = np.abs(q - np.round(q))
        on_line = (near_img[..., None] & (cell < e["eq"])).any(-1) | ~np.isfinite(q).all(-1)
        pad = np.minimum(np.abs(q + 1), np.abs(q - lim)).min(-1)
        hz_scale = np.abs(f.consts[0][8]) + np.abs(f.consts[0][6] * f.px) + np.abs(f.consts[0][7] * f.py) + np.abs(f.consts[1][2] * f.s * f.inv_d)
        hz_rel = (np.abs(f.h[2]) / hz_scale).min(1)
        nonfinite = ~(np.isfinite(f.raw) & np.isfinite(q).all(-1).all(-1))
        stiff = (f.D < STIFF_D * 1e-8) | (f.raw < STIFF_CORR) | (hz_rel < STIFF_HZ) | nonfinite
        stiff |= (np.sign(f.h[2]).min(1) != np.sign(f.h[2]).max(1))   # hz changes sign inside the patch
        gate = np.minimum(np.abs(f.raw), np.abs(f.raw - 2.0))
        m_mask, m_switch = np.abs(f.ncc - 0.9), np.abs(np.sqrt(np.maximum(f.ref_var, 0.0)) - 0.01)
        sw_band = BAND * e["ref_var"] / (2 * np.sqrt(np.maximum(f.ref_var, 1e-300)))
        out = dict(cell=np.where(near_img[..., None], cell, np.inf).min(-1).min(-1), pad=pad.min(1), gate=gate, mask=m_mask, switch=m_switch,
                   hz=np.abs(f.h[2]).min(1), stiff=stiff, nonfinite=nonfinite,
                   flip_mask=m_mask <= BAND * e["ncc"], flip_switch=m_switch <= sw_band,
                   flip_grad=on_line.any(1) | (gate <= BAND * e["raw"]) | nonfinite)
    return out


# ---------------------------------------------------------------- evaluation of one case, shared by every test
def evaluate(s, patch):
    """One scene at one patch size: .f64 (chain at float64 with every term), .y32 (the float32 yardstick), .t (restate, torch
    autograd: ncc, ncc_grad, ref_var, mask, switch and .d_normals / .d_dists for the scene's upstream gradient), .e, .k."""
    args = (s.pixels, s.normals, s.dists, s.ref_gray, s.near_gray, s.M, s.b, s.Kinv, s.ncc_scale, patch)
    f = chain(*args, d_ncc=s.d_ncc, dtype=np.float64)
    f.consts, f.shape, f.normals = (s.M, s.b, s.Kinv), s.near_gray.shape, np.asarray(s.normals, np.float64)
    y = chain(*args, d_ncc=s.d_ncc, dtype=np.float32)
    tt = [torch.tensor(np.asarray(a, dtype=np.float64)) for a in args[:8]]
    tt[1].requires_grad_(True); tt[2].requires_grad_(True)
    with np.errstate(all="ignore"):
        t = restate(*tt, float(s.ncc_scale), patch)
        (t.ncc * torch.tensor(np.asarray(s.d_ncc, np.float64))).sum().backward()
    t.d_normals, t.d_dists = tt[1].grad.numpy(), tt[2].grad.numpy()
    e = error_scales(f)
    return types.SimpleNamespace(scene=s, patch=patch, f64=f, y32=y, t=t, e=e, k=classify(f, e))


@functools.lru_cache(maxsize=None)
def reference(name, patch):
    return evaluate(scene(name), patch)


def ratios(got, truth, e, exclude):
    """|got - truth| / e per element, 0 where both vanish, inf where the scale is 0 and the error is not, nan where excluded or
    the truth is not finite."""
    got, truth, e = (np.asarray(a, dtype=np.float64) for a in (got, truth, e))
    with np.errstate(all="ignore"):
        err = np.abs(got - truth)
        r = np.where(err == 0, 0.0, err / e)
        r = np.where(np.isnan(r), np.inf, r)
    ex = np.broadcast_to(np.asarray(exclude).reshape(exclude.shape + (1,) * (r.ndim - exclude.ndim)), r.shape)
    return np.where(ex | ~np.isfinite(truth), np.nan, r)


def outputs_of(x):
    """The comparable outputs of a chain / restate result as numpy float64: name -> array."""
    g = lambda a: a.detach().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    return {"ncc": g(x.ncc), "ncc_grad": g(x.ncc_grad), "ref_var": g(x.ref_var), "d_normals": g(x.d_normals), "d_dists": g(x.d_dists)}


EXCLUDE = {"ncc": None, "ncc_grad": None, "ref_var": None, "d_normals": "flip_grad", "d_dists": "flip_grad"}


def compare(r, got, n=None):
    """got: name -> array for some of the outputs.  -> {name: (worst ratio / K regular, worst ratio / K stiff)}; the caller asserts
    <= 1.  The truth is the torch autograd restatement; excluded: non-finite truths and, for gradients, the flip band."""
    truth = outputs_of(r.t)
    worst = {}
    n = len(r.k["stiff"]) if n is None else n   # the first n samples of the scene (samples are independent)
    for name, x in got.items():
        ex = r.k[EXCLUDE[name]][:n] if EXCLUDE[name] else np.zeros(n, dtype=bool)
        ex = ex | r.k["nonfinite"][:n]
        q = ratios(np.asarray(x).reshape(truth[name][:n].shape), truth[name][:n], r.e[name][:n], ex)
        st = np.broadcast_to(r.k["stiff"][:n].reshape((-1,) + (1,) * (q.ndim - 1)), q.shape)
        w = []
        for cls, kk in ((~st, K[name][0]), (st, K[name][1])):
            sel = cls & ~np.isnan(q)
            w.append(float((q[sel]).max() / kk) if sel.any() and kk > 0 else (0.0 if not sel.any() or float(q[sel].max()) == 0 else math.inf))
        worst[name] = tuple(w)
    return worst


# ---------------------------------------------------------------- (e) the scenes
REF_CAM = dict(W=32, H=24, Fx=35.0, Fy=34.0, Cx=15.7, Cy=12.2)   # small images keep |p|, and with it the float32 position error, small:
# the share of samples with one of up to 289 taps within that error of a cell line must stay below 2 %
PATCHES = (0, 1, 2, 3, 4, 8)
COUNTS = (1, 15, 16, 17, 1001)


def _cams(near_eye=(0.9, -0.3, 0.4), scale=1):
    ref = RefCam(eye=(0.0, 0.0, 0.0), target=(0.0, 0.0, 6.0), **REF_CAM)
    near = RefCam(eye=near_eye, target=(0.0, 0.0, 6.0), **dict(REF_CAM, Fx=36.0, Fy=35.5, Cx=16.3, Cy=11.55))
    if scale != 1:
        for c in (ref, near):
            c.W, c.H, c.Fx, c.Fy, c.Cx, c.Cy = c.W * scale, c.H * scale, c.Fx * scale, c.Fy * scale, c.Cx * scale, c.Cy * scale
    return ref, near


def _planes(ref, N, g, dn=0.05, dd=0.03):
    n0, d0 = true_plane(ref)
    n = n0[None] + dn * g.standard_normal((N, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = d0 * (1.0 + dd * g.standard_normal(N))
    return n.astype(np.float32), d.astype(np.float32)


def _upstream(N, g):
    """Upstream gradients of both signs with an exact zero on every 5th sample."""
    d = g.standard_normal(N).astype(np.float32)
    d[::5] = 0.0
    return d


def _pack(name, ref, near, scale, pixels, normals, dists, g, ref_gray=None, near_gray=None, patches=(3,), **extra):
    M, b, Kinv = homography_constants(ref, near, scale)
    rg = plane_image(ref, scale) if ref_gray is None else ref_gray
    ng = plane_image(near, scale) if near_gray is None else near_gray
    assert rg.shape == ng.shape and rg.shape[0] <= 48 and rg.shape[1] <= 64
    return types.SimpleNamespace(name=name, ref=ref, near=near, ncc_scale=float(scale), pixels=np.asarray(pixels, np.float32), normals=normals, dists=dists,
                                 ref_gray=rg, near_gray=ng, M=M, b=b, Kinv=Kinv, d_ncc=_upstream(len(dists), g), patches=tuple(patches), **extra)


SCENES = ("production", "half", "borders", "thrown", "flat", "identity", "degenerate")


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> namespace: pixels (N, 2), normals (N, 3), dists (N,), d_ncc (N,) float32; ref_gray, near_gray (h, w) float32; M, b, Kinv
    (float32 values as float64); ncc_scale; patches: the patch sizes the scene is evaluated at."""
    g = np.random.default_rng(SCENES.index(name) + 17)
    ref, near = _cams(scale=2 if name == "half" else 1)
    W, H = ref.W, ref.H
    if name == "production":   # integer pixel coordinates at ncc_scale 1, a few fractional ones; 1001 = 62 groups of 16 + 9
        N = 1001
        px = np.stack([g.integers(8, W - 8, N), g.integers(8, H - 8, N)], 1).astype(np.float64)
        px[-40:] += g.random((40, 2)) - 0.5
        n, d = _planes(ref, N, g)
        d[::3] *= (1.0 + 0.25 * g.standard_normal(len(d[::3]))).astype(np.float32)   # wrong planes: both sides of ncc < 0.9
        return _pack(name, ref, near, 1.0, px, n, d, g, patches=PATCHES)
    if name == "half":         # ncc_scale 2: half-resolution images, full-resolution coordinates, odd pixels included
        N = 300
        px = np.stack([g.integers(12, W - 12, N), g.integers(12, H - 12, N)], 1).astype(np.float64)
        px[:150] = px[:150] // 2 * 2 + 1
        n, d = _planes(ref, N, g)
        return _pack(name, ref, near, 2.0, px, n, d, g, patches=(3, 4))
    if name == "borders":      # reference patches that reach over every side and corner of the reference image
        edge = [(x, y) for x in (0, 1, 2, W - 3, W - 2, W - 1) for y in range(0, H, 5)] + [(x, y) for y in (0, 1, 2, H - 3, H - 2, H - 1) for x in range(0, W, 5)]
        edge += [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (0.4, 0.3), (W - 1.4, H - 1.2)]
        px = np.array(edge, dtype=np.float64)
        n, d = _planes(ref, len(px), g)
        return _pack(name, ref, near, 1.0, px, n, d, g, patches=(3, 8))
    if name == "thrown":       # planes that throw the warped patch partly (taps in (-1, 0) and (w-1, w)) or wholly outside the neighbour
        N = 400
        px = np.stack([g.integers(6, W - 6, N), g.integers(6, H - 6, N)], 1).astype(np.float64)
        n, d = _planes(ref, N, g, dn=0.02, dd=0.0)
        d = (d * np.exp(g.uniform(-1.2, 1.2, N))).astype(np.float32)      # a wrong distance slides the patch along the epipolar line
        d[:40] *= np.float32(0.05)                                        # far outside
        px[40:120, 1] = g.integers(3, 6, 80)                              # near the top, tilted planes: taps over the upper limit as well
        n[40:120] += (0.3 * g.standard_normal((80, 3))).astype(np.float32)
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        return _pack(name, ref, near, 1.0, px, n, d, g, patches=(3,))
    if name == "flat":         # a constant block and a block of contrast 1e-4 in the reference image
        rg = plane_image(ref, 1.0)
        rg[2:11, 2:14] = np.float32(0.4375)
        rg[13:22, 2:14] = (0.5 + 1e-4 * g.random((9, 12))).astype(np.float32)
        N = 240
        px = np.stack([g.integers(5, 11, N), g.integers(5, 8, N)], 1).astype(np.float64)
        px[80:160] = np.stack([g.integers(5, 11, 80), g.integers(16, 19, 80)], 1)
        px[160:] = np.stack([g.integers(18, W - 5, 80), g.integers(5, H - 5, 80)], 1)
        n, d = _planes(ref, N, g)
        kind = np.repeat([0, 1, 2], 80)   # constant, contrast 1e-4, ordinary
        return _pack(name, ref, near, 1.0, px, n, d, g, ref_gray=rg, patches=(3,), kind=kind)
    if name == "identity":     # the same camera and the same image: b = 0, h = p, perfectly correlated
        N = 200
        px = np.stack([g.integers(5, W - 5, N), g.integers(5, H - 5, N)], 1).astype(np.float64)
        px[100:] += g.random((100, 2)) - 0.5
        n, d = _planes(ref, N, g)
        img = plane_image(ref, 1.0)
        return _pack(name, ref, ref, 1.0, px, n, d, g, ref_gray=img, near_gray=img.copy(), patches=(3,))
    if name == "degenerate":   # benign samples with degenerate planes among them; `benign` holds replacements for those
        N = 64
        px = np.stack([g.integers(9, W - 9, N), g.integers(9, H - 9, N)], 1).astype(np.float64)
        n, d = _planes(ref, N, g)
        bn, bd = n.copy(), d.copy()
        M, b, Kinv = homography_constants(ref, near, 1.0)
        bad = np.array([3, 8, 13, 18, 27, 33, 42, 57])   # different lanes groups: 8 lanes per sample, 16 samples per workgroup
        d[3], d[8], d[13], d[18] = 1e-6, -0.7, 0.0, -0.0
        p = np.array([px[27, 0], px[27, 1], 1.0])
        r = Kinv.reshape(3, 3) @ p
        t = np.cross(r, [0.3, 1.0, 0.2])
        n[27] = (t / np.linalg.norm(t)).astype(np.float32)                       # n . r = 0 at the patch centre
        for i, off in ((33, 0.0), (42, 0.6), (57, -1.3)):                        # hz through 0 at / next to the centre
            p = np.array([px[i, 0] + off, px[i, 1], 1.0])
            sr = n[i].astype(np.float64) @ (Kinv.reshape(3, 3) @ p)
            d[i] = np.float32(b[2] * sr / (M[6:9] @ p))
        return _pack(name, ref, near, 1.0, px, n, d, g, patches=(3,), bad=bad, benign=(bn, bd))
    raise KeyError(name)


def cases():
    return [(name, p) for name in SCENES for p in scene(name).patches]


def measure(verbose=True):
    """The largest yardstick ratio per output and class over all cases: what RATIO records."""
    worst = {k: [0.0, 0.0] for k in EXCLUDE}
    for name, p in cases():
        r = reference(name, p)
        truth, y = outputs_of(r.t), outputs_of(r.y32)
        for out in EXCLUDE:
            ex = (r.k[EXCLUDE[out]] if EXCLUDE[out] else np.zeros(len(r.k["stiff"]), dtype=bool)) | r.k["nonfinite"]
            q = ratios(y[out], truth[out], r.e[out], ex)
            st = np.broadcast_to(r.k["stiff"].reshape((-1,) + (1,) * (q.ndim - 1)), q.shape)
            for j, cls in enumerate((~st, st)):
                sel = cls & ~np.isnan(q)
                if sel.any():
                    m = float(q[sel].max())
                    if verbose and m > worst[out][j]:
                        print(f"{name:11s} patch {p} {out:10s} {'stiff' if j else 'regular':8s} ratio {m:.4g} (n={int(sel.sum())})")
                    worst[out][j] = max(worst[out][j], m)
    return worst


# ---------------------------------------------------------------- (d) the border grid-sample
def grid_restate(img, grid):
    """torch.nn.functional.grid_sample(bilinear, border, align_corners=True) of a (C, H, W) image at N normalised positions,
    stated from include/gs2m_mvs.h in float64: x = (g + 1) / 2 (W - 1), clipped to [0, W - 1] with the position gradient zeroed
    where the clip binds; a NaN position behaves as the clip at 0.  -> out (N, C), differentiable to img and grid."""
    C, H, W = img.shape
    outs = []
    pos = []
    for k, n in ((0, W), (1, H)):
        x = (grid[:, k] + 1) * 0.5 * (n - 1)
        low, high = ~(x > 0), x >= n - 1     # ~(x > 0) takes NaN to the lower clip
        x = torch.where(low, torch.zeros_like(x), torch.where(high, torch.full_like(x, float(n - 1)), x))
        pos.append(x)
    x, y = pos
    x0, y0 = x.detach().floor().long(), y.detach().floor().long()
    fx, fy = x - x0, y - y0
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)   # (weight 0 where clamped: fx = 0 on the last column)
    for c in range(C):
        im = img[c]
        outs.append(im[y0, x0] * (1 - fx) * (1 - fy) + im[y0, x1] * fx * (1 - fy) + im[y1, x0] * (1 - fx) * fy + im[y1, x1] * fx * fy)
    return torch.stack(outs, 1)


def grid_positions(grid, W, H):
    """numpy float64: unclipped and clipped pixel positions, and whether the clip binds, per axis -> (N, 2) each."""
    g = np.asarray(grid, np.float64)
    size = np.array([W - 1, H - 1], dtype=np.float64)
    with np.errstate(all="ignore"):
        raw = (g + 1) * 0.5 * size
        low, high = ~(raw > 0), raw >= size
    return raw, np.where(low, 0.0, np.where(high, size, raw)), low | high


def grid_reference(img, grid, d_out):
    """float64 forward, d_grid (autograd) and the exact dense scatter for d_img, with error scales and margins.
    img (C, H, W), grid (N, 2), d_out (N, C): float32 values.  Non-finite upstream gradients are not handled here."""
    C, H, W = img.shape
    ti = torch.tensor(np.asarray(img, np.float64), requires_grad=True)
    tg = torch.tensor(np.asarray(grid, np.float64), requires_grad=True)
    G = torch.tensor(np.asarray(d_out, np.float64))
    out = grid_restate(ti, tg)
    (out * G).sum().backward()
    raw, pos, binds = grid_positions(grid, W, H)
    d_img = dense_scatter(G, torch.tensor(pos), W, H).numpy()
    assert np.abs(d_img - ti.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(d_img).max())
    # error scales: the position is three rounded operations of magnitude <= max(|x|, W - 1); it does not move where the clip binds
    size = np.array([W - 1, H - 1], dtype=np.float64)
    epos = np.where(binds, 0.0, 4 * U * np.maximum(np.abs(np.nan_to_num(raw)), size))
    x0 = np.minimum(np.floor(pos), np.maximum(size - 1, 0)).astype(np.int64)   # on the last column the cell to the left: same value
    f = pos - x0
    im = np.asarray(img, np.float64)
    x1, y1 = np.minimum(x0[:, 0] + 1, W - 1), np.minimum(x0[:, 1] + 1, H - 1)
    v00, v10, v01, v11 = im[:, x0[:, 1], x0[:, 0]].T, im[:, x0[:, 1], x1].T, im[:, y1, x0[:, 0]].T, im[:, y1, x1].T   # (N, C)
    fx, fy = f[:, 0:1], f[:, 1:2]
    sx = (v10 - v00) * (1 - fy) + (v11 - v01) * fy
    sy = (v01 - v00) * (1 - fx) + (v11 - v10) * fx
    mixed = v11 - v10 - v01 + v00
    amax = np.max(np.abs(np.stack([v00, v10, v01, v11])), axis=0)
    Gn = np.asarray(d_out, np.float64)
    e_out = np.abs(sx) * epos[:, 0:1] + np.abs(sy) * epos[:, 1:2] + 6 * U * amax
    m = np.where(binds, 0.0, 0.5 * size)
    e_dgrid = np.stack([(np.abs(Gn) * (np.abs(mixed) * epos[:, 1:2] + 6 * U * amax)).sum(1) * m[:, 0],
                        (np.abs(Gn) * (np.abs(mixed) * epos[:, 0:1] + 6 * U * amax)).sum(1) * m[:, 1]], 1) + 4 * U * np.abs(tg.grad.numpy())
    # d_img: each contribution g w moves by |g| (|dw/dx| ex + |dw/dy| ey) + 3 U |g w|; a texel adds cnt of them up
    econ = np.abs(Gn) * (epos[:, 0:1] + epos[:, 1:2]) + 3 * U * np.abs(Gn)
    tp = torch.tensor(pos)
    # ... on every texel of its footprint, and on the neighbour's where the position is within its error of a cell line
    e_img = np.zeros((C, H * W))
    fl = np.floor(pos).astype(np.int64)
    fr = pos - fl
    for dx in (-1, 0, 1, 2):
        okx = {-1: fr[:, 0] <= epos[:, 0], 0: True, 1: True, 2: 1 - fr[:, 0] <= epos[:, 0]}[dx] & (fl[:, 0] + dx >= 0) & (fl[:, 0] + dx <= W - 1)
        for dy in (-1, 0, 1, 2):
            oky = {-1: fr[:, 1] <= epos[:, 1], 0: True, 1: True, 2: 1 - fr[:, 1] <= epos[:, 1]}[dy] & (fl[:, 1] + dy >= 0) & (fl[:, 1] + dy <= H - 1)
            ok = okx & oky
            for c in range(C):
                np.add.at(e_img[c], ((fl[:, 1] + dy) * W + fl[:, 0] + dx)[ok], econ[ok, c])
    e_img = e_img.reshape(C, H, W)
    absum = dense_scatter(torch.tensor(np.abs(Gn)), tp, W, H).numpy()
    cnt = dense_scatter(torch.ones(len(pos), 1, dtype=F64), tp, W, H).numpy() * 4
    e_img = e_img + (np.sqrt(cnt) + 1) * U * absum
    # margins: d_grid jumps where the position crosses a cell line or a clip limit
    cell = np.abs(pos - np.round(pos))
    lim = np.minimum(np.abs(raw), np.abs(raw - size))
    with np.errstate(all="ignore"):
        band = 4 * U * np.maximum(np.abs(raw), size)
        live = np.array([W > 1, H > 1])[None]   # an axis of one texel has no position gradient at all
        flip = (((np.where(binds, np.inf, cell) <= band) | (lim <= band)) & live).any(1) & ~np.isnan(raw).any(1)
    return types.SimpleNamespace(out=out.detach().numpy(), d_grid=tg.grad.numpy(), d_img=d_img, e_out=e_out, e_dgrid=e_dgrid, e_img=e_img,
                                 flip=flip, pos=pos, raw=raw, binds=binds)


def grid_yardstick(img, grid, d_out):
    """The same contract in numpy float32, texels added up in sample order: the yardstick of the grid-sample bounds."""
    f = np.float32
    img, grid, d_out = np.asarray(img, f), np.asarray(grid, f), np.asarray(d_out, f)
    C, H, W = img.shape
    with np.errstate(all="ignore"):
        pos, m = [], []
        for k, n in ((0, W), (1, H)):
            x = (grid[:, k] + f(1)) * f(0.5) * f(n - 1)
            low, high = ~(x > 0), x >= f(n - 1)
            pos.append(np.where(low, f(0), np.where(high, f(n - 1), x)))
            m.append(np.where(low | high, f(0), f(0.5) * f(n - 1)))
    x, y = pos
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    fx, fy = (x - np.floor(x))[:, None], (y - np.floor(y))[:, None]
    bx, by = (x0 + 1 <= W - 1)[:, None], (y0 + 1 <= H - 1)[:, None]
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    v00, v10, v01, v11 = img[:, y0, x0].T, np.where(bx, img[:, y0, x1].T, f(0)), np.where(by, img[:, y1, x0].T, f(0)), np.where(bx & by, img[:, y1, x1].T, f(0))
    one = f(1)
    w00, w10, w01, w11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    out = v00 * w00 + v10 * w10 + v01 * w01 + v11 * w11
    gx = np.cumsum(d_out * ((v10 - v00) * (one - fy) + (v11 - v01) * fy), axis=1, dtype=f)[:, -1] * m[0]
    gy = np.cumsum(d_out * ((v01 - v00) * (one - fx) + (v11 - v10) * fx), axis=1, dtype=f)[:, -1] * m[1]
    d_img = np.zeros((C, H * W), f)
    for c in range(C):
        for wgt, xx, yy, ok in ((w00, x0, y0, np.ones_like(bx)), (w10, x1, y0, bx), (w01, x0, y1, by), (w11, x1, y1, bx & by)):
            ok = ok[:, 0]
            np.add.at(d_img[c], (yy * W + xx)[ok], (d_out[:, c] * wgt[:, 0])[ok])
    return out, np.stack([gx, gy], 1), d_img.reshape(C, H, W)


GRID_SIZES = ((37, 53), (1, 9), (9, 1), (1, 1))   # (H, W)
GRID_COUNTS = (1, 255, 256, 257, 1000)


@functools.lru_cache(maxsize=None)
def grid_case(C, H, W, N=1000):
    """-> img (C, H, W), grid (N, 2), d_out (N, C) float32: positions inside, beyond both sides, exactly +-1, on cell lines, NaN;
    upstream gradients with exact zeros."""
    g = np.random.default_rng(1000 * C + 10 * H + W)
    img = g.standard_normal((C, H, W)).astype(np.float32)
    grid = (g.random((N, 2)) * 2.6 - 1.3).astype(np.float32)
    special = np.array([[-1.0, -1.0], [1.0, 1.0], [0.0, 0.0], [1.0, -1.0], [-1.0, 0.3], [0.3, 1.0], [-1.3, 0.2], [0.2, 1.3], [np.nan, 0.1], [0.1, np.nan],
                        [np.nan, np.nan], [np.inf, 0.2], [-np.inf, -np.inf]], dtype=np.float32)
    lines = np.stack([2.0 * g.integers(0, max(W - 1, 1), 12) / max(W - 1, 1) - 1.0, g.random(12) * 2 - 1], 1).astype(np.float32)   # x on a cell line
    k = min(N, len(special))
    grid[:k] = special[:k]
    if N >= 40:
        grid[20:32] = lines
    d_out = g.standard_normal((N, C)).astype(np.float32)
    d_out[::7] = 0.0
    return img, grid, d_out


@functools.lru_cache(maxsize=None)
def lattice_case(C, N=1500):
    """33 x 17 image (W - 1 and H - 1 powers of two), positions on multiples of 1/16 pixel (some beyond every side, the corners
    exactly), image values and upstream gradients k 2^-10 with |k| <= 64: every float32 operation of the contract is exact."""
    g = np.random.default_rng(33 + C)
    img = (g.integers(-64, 65, (C, 17, 33)) / 1024.0).astype(np.float32)
    kx, ky = g.integers(-40, 16 * 32 + 41, N), g.integers(-40, 16 * 16 + 41, N)
    kx[:4], ky[:4] = [0, 512, 0, 512], [0, 0, 256, 256]
    grid = np.stack([kx / 256.0 - 1.0, ky / 128.0 - 1.0], 1).astype(np.float32)
    d_out = (g.integers(-64, 65, (N, C)) / 1024.0).astype(np.float32)
    return img, grid, d_out


def grid_measure():
    worst = {"grid_out": 0.0, "d_grid": 0.0, "d_img": 0.0}
    for C in (1, 2, 3, 4):
        for H, W in GRID_SIZES:
            img, grid, d_out = grid_case(C, H, W)
            r = grid_reference(img, grid, d_out)
            o, dg, di = grid_yardstick(img, grid, d_out)
            none = np.zeros(len(grid), dtype=bool)
            for name, q in (("grid_out", ratios(o, r.out, r.e_out, none)), ("d_grid", ratios(dg, r.d_grid, r.e_dgrid, r.flip)),
                            ("d_img", ratios(di, r.d_img, r.e_img, np.zeros(di.shape, dtype=bool)))):
                worst[name] = max(worst[name], float(np.nanmax(q)))
    return worst


if __name__ == "__main__":
    for k, v in measure().items():
        print(k, v)
    print(grid_measure())
