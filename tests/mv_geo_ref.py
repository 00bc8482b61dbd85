"""Float64 arbiter of the multi-view geometric term (utils/loss_utils.py:256-276) and the scenes the mv_geo kernels are tested on.

Plain torch on the CPU, no device import: `restate` is the reference's chain (back-project, move into the neighbour's camera,
project, border-clamped bilinear lookup of the neighbour's depth / normal, occlusion test, reprojection, |reprojection - pixel|,
acos of the clamped cosine of the two normalised normals) in float64 without a single float32 cast, differentiable by autograd
with respect to the four maps.  Next to the three outputs it returns, per pixel, the float64 MARGIN of every decision the chain
takes, from which `classify` derives

  * the flip band: pixels where a float32 evaluation may legitimately take the other side of a decision (`valid`, the border
    clip, the acos clamp, the bilinear cell), so a comparison must leave them out;
  * the stiff class: pixels where the chain is singular or ill conditioned (a zero-length normal under the `+1e-8`
    normalisation: gradient ~1e8; a point at or behind the neighbour's near limit; a reprojection error too small to have a
    direction; normals within a few degrees of parallel without reaching the clamp: acos' derivative amplifies the cosine's
    rounding by |c| / (1 - c^2)) -- they are compared too, but against their own error scale, so that they do not blunt the others' bound.

`dense_scatter` is the exact (float64) bilinear scatter of per-sample contributions, `scene` builds the four test scenes, and
`reference` evaluates one scene once (float64 with autograd, and gs2m_mvs.mv_geo_torch in float32 on the CPU as the
"op by op" yardstick) and keeps the result for every test that needs it.
"""
import functools
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
EPS32 = 2.0 ** -23
# The flip band.  A float32 evaluation reaches the projection q through a chain of about six rounded operations per component
# (ray, ray x depth, the 3x3 transform, the division, the focal scale, the principal point), each relative 2^-24 .. 2^-23 of the
# LARGEST term it adds, so |q32 - q64| <~ CHAIN x 2^-23 x max(|q|, Wn) plus the transform's cancellation error carried through
# the division; every other margin (Y.z, the occlusion difference, the cosine) gets the same CHAIN x 2^-23 x its magnitude plus
# what the error of q moves it by.  A pixel is in the band when any decision margin is smaller than its band.
CHAIN = 6.0
JUST_NOT_OCCLUDED = 0.02   # "just not occluded": 0 <= occlusion - (Y.z - zs) < this
STIFF_NORMAL = 0.05        # sampled normals shorter than this: 1 / length amplification of the normalisation's gradient
STIFF_NOISE = 1e-3         # reprojection errors below this (pixels) have no float32 direction
STIFF_ACOS = 50.0          # |c| / (1 - c^2), the relative condition number of acos' derivative -1 / sqrt(1 - c^2) with respect to the
                           # cosine c: above this a float32 cosine (error >= 2^-23) leaves the angle's gradient fewer than 17 bits
SCENES = ("general", "one_wave", "contention", "identity")


class RefCam:
    """A camera as plain numbers: V is the 4x4 world-to-view matrix as the project's Camera holds it (row vectors:
    x_cam = x_world @ V[:3, :3] + V[3, :3]), rounded to float32 and kept as float64, plus Fx, Fy, Cx, Cy, W, H."""

    def __init__(self, W, H, Fx, Fy, Cx, Cy, eye, target):
        self.W, self.H, self.Fx, self.Fy, self.Cx, self.Cy = int(W), int(H), float(Fx), float(Fy), float(Cx), float(Cy)
        eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
        fwd = (target - eye) / np.linalg.norm(target - eye)
        right = np.cross(np.array([0.0, 1.0, 0.0]), fwd)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        Rw2c = np.stack([right, down, fwd], axis=0)
        V = np.eye(4)
        V[:3, :3], V[3, :3] = Rw2c.T, -Rw2c @ eye
        self.V = torch.tensor(V.astype(np.float32).astype(np.float64))

    def numbers(self):
        return np.concatenate([self.V.numpy().reshape(-1), [self.Fx, self.Fy, self.Cx, self.Cy, self.W, self.H]])

    @classmethod
    def from_numbers(cls, a):
        c = cls.__new__(cls)
        c.V = torch.tensor(np.asarray(a[:16], np.float64).reshape(4, 4))
        c.Fx, c.Fy, c.Cx, c.Cy = (float(x) for x in a[16:20])
        c.W, c.H = int(a[20]), int(a[21])
        return c

    def project_camera(self, device="cpu"):
        """The attributes gs2m_mvs reads off a camera (gs2m_scene.Camera's names), float32 on `device`."""
        cam = types.SimpleNamespace(image_width=self.W, image_height=self.H, Fx=self.Fx, Fy=self.Fy, Cx=self.Cx, Cy=self.Cy,
                                    world_view_transform=self.V.float().to(device), device=device,
                                    R=self.V[:3, :3].numpy().astype(np.float32), T=self.V[3, :3].numpy().astype(np.float32))

        def get_rays(scale=1.0):  # scene/cameras.py:72-81
            h, w = int(cam.image_height / scale), int(cam.image_width / scale)
            u, v = torch.meshgrid(torch.arange(w, device=device, dtype=torch.float32), torch.arange(h, device=device, dtype=torch.float32), indexing="xy")
            return torch.stack(((scale * u - cam.Cx / scale) / cam.Fx, (scale * v - cam.Cy / scale) / cam.Fy, torch.ones_like(u)), dim=-1)

        cam.get_rays = get_rays
        return cam


def pixel_grid(W, H, dtype=F64):
    ix, iy = torch.meshgrid(torch.arange(W, dtype=dtype), torch.arange(H, dtype=dtype), indexing="xy")
    return torch.stack([ix, iy], dim=-1)  # (H, W, 2)


def _border_sample(img, x, y, W, H):
    grid = torch.stack([x / ((W - 1) / 2) - 1, y / ((H - 1) / 2) - 1], dim=-1).view(1, -1, 1, 2)
    return F.grid_sample(img[None], grid, mode="bilinear", padding_mode="border", align_corners=True)[0, :, :, 0]  # (C, N)


def restate(depth, normal, depth_n, normal_n, ref, near, occlusion):
    """utils/loss_utils.py:256-276 in float64.  depth (1,H,W), normal (3,H,W), depth_n (1,Hn,Wn), normal_n (3,Hn,Wn) as float64
    tensors (leaves with requires_grad for gradients) -> namespace: noise, angle (H W), valid (H W, bool), the intermediates a
    test needs (q, zs, nraw, c, Y -- zs and nraw keep their gradients) and `margins`, a dict of detached (H W) float64 tensors."""
    assert all(t.dtype == F64 for t in (depth, normal, depth_n, normal_n))
    H, W, Hn, Wn = ref.H, ref.W, near.H, near.W
    pix = pixel_grid(W, H).reshape(-1, 2)
    rays = torch.stack([(pix[:, 0] - ref.Cx) / ref.Fx, (pix[:, 1] - ref.Cy) / ref.Fy, torch.ones_like(pix[:, 0])], dim=-1)
    pts = rays * depth.reshape(-1, 1)
    Rr, Tr, Rn, Tn = ref.V[:3, :3], ref.V[3, :3], near.V[:3, :3], near.V[3, :3]
    world = (pts - Tr) @ Rr.transpose(-1, -2)                      # _get_points_from_depth
    Y = world @ Rn + Tn                                            # :258
    q = torch.stack([Y[:, 0] * near.Fx / Y[:, 2] + near.Cx, Y[:, 1] * near.Fy / Y[:, 2] + near.Cy], dim=-1)   # _sample_depth_normal
    valid = (q[:, 0] > 0) & (q[:, 0] < Wn) & (q[:, 1] > 0) & (q[:, 1] < Hn) & (Y[:, 2] > 0.1)
    zs = _border_sample(depth_n.reshape(1, Hn, Wn), q[:, 0], q[:, 1], Wn, Hn)[0]
    nraw = _border_sample(normal_n.reshape(3, Hn, Wn), q[:, 0], q[:, 1], Wn, Hn).permute(1, 0)
    ns = nraw / (nraw.norm(dim=1, keepdim=True) + 1e-8)
    valid = valid & (Y[:, 2] - zs <= occlusion)                    # :263
    Yp = Y / Y[:, 2:3] * zs[:, None]                               # _reproject_points
    Z = ((Yp - Tn) @ Rn.transpose(-1, -2)) @ Rr + Tr
    rep = torch.stack([Z[:, 0] * ref.Fx / Z[:, 2] + ref.Cx, Z[:, 1] * ref.Fy / Z[:, 2] + ref.Cy], dim=-1)
    noise = torch.norm(rep - pix, dim=-1)                          # :268
    nr = _border_sample(normal.reshape(3, H, W), pix[:, 0], pix[:, 1], W, H).permute(1, 0)     # _sample_normal_map
    m = nr / (nr.norm(dim=1, keepdim=True) + 1e-8)                 # :273
    c = torch.sum(m * ns, dim=1)
    angle = torch.acos(c.clamp(-1 + 1e-6, 1 - 1e-6))               # :276
    out = types.SimpleNamespace(noise=noise, angle=angle, valid=valid, q=q, zs=zs, nraw=nraw, c=c, Y=Y)
    # ---- decision margins and their float32 bands
    with torch.no_grad():
        M = Rr.transpose(-1, -2) @ Rn
        Ymag = pts.abs() @ M.abs() + (Tn - Tr @ M).abs()
    qd = q.detach()
    if q.requires_grad:
        gz = torch.autograd.grad(zs.sum(), q, retain_graph=True)[0].abs()
        gc = torch.autograd.grad(c.sum(), q, retain_graph=True)[0].abs()
        zs.retain_grad(); nraw.retain_grad()   # (after the two calls above: they would leave their own seeds in .grad)
    else:
        gz = gc = torch.zeros_like(qd)
    with torch.no_grad():
        Yd, k = Y.detach(), CHAIN * EPS32
        eY = k * Ymag
        size = torch.tensor([float(Wn), float(Hn)], dtype=F64)
        foc = torch.tensor([near.Fx, near.Fy], dtype=F64)
        eq = k * torch.maximum(qd.abs(), size) + foc * (eY[:, :2] + (Yd[:, :2] / Yd[:, 2:3]).abs() * eY[:, 2:3]) / Yd[:, 2:3].abs()
        ezs = k * zs.detach().abs() + (gz * eq).sum(1)
        inside = (qd > 0).all(1) & (qd < size - 1).all(1)
        kink = torch.where(inside[:, None], (qd - qd.round()).abs(), torch.full_like(qd, math.inf))
        margins = {"qx": qd[:, 0], "qy": qd[:, 1], "Wn-qx": Wn - qd[:, 0], "Hn-qy": Hn - qd[:, 1], "Y.z-0.1": Yd[:, 2] - 0.1,
                   "occlusion": occlusion - (Yd[:, 2] - zs.detach()), "clip x": (qd[:, 0] - (Wn - 1)).abs(), "clip y": (qd[:, 1] - (Hn - 1)).abs(),
                   "clamp": 1 - 1e-6 - c.detach().abs(), "noise": noise.detach(), "cell x": kink[:, 0], "cell y": kink[:, 1]}
        bands = {"qx": eq[:, 0], "qy": eq[:, 1], "Wn-qx": eq[:, 0], "Hn-qy": eq[:, 1], "Y.z-0.1": eY[:, 2], "occlusion": eY[:, 2] + ezs,
                 "clip x": eq[:, 0], "clip y": eq[:, 1], "clamp": k + (gc * eq).sum(1), "cell x": eq[:, 0], "cell y": eq[:, 1]}
    out.margins, out.bands = margins, bands
    return out


FORWARD_DECISIONS = ("qx", "qy", "Wn-qx", "Hn-qy", "Y.z-0.1", "occlusion", "clip x", "clip y", "clamp")


def classify(r, normal, near):
    """-> dict of (H W) bool masks from the float64 margins of `restate`'s result alone.
    flip: some decision of the forward chain (valid, clip, clamp) is within its float32 band; flip_bwd: that, or the projection is
    within its band of a bilinear cell boundary (the lookup's position gradient jumps there); stiff: see the module docstring;
    then the population classes of the edge cases."""
    m, b = r.margins, r.bands
    flip = torch.zeros_like(m["qx"], dtype=torch.bool)
    for k in FORWARD_DECISIONS:
        flip |= m[k].abs() < b[k]
    flip_bwd = flip | (m["cell x"] < b["cell x"]) | (m["cell y"] < b["cell y"])
    nrl = normal.detach().reshape(3, -1).norm(dim=0)
    nn = r.nraw.detach().norm(dim=1)
    Wn, Hn = near.W, near.H
    far = (m["qx"].abs() > 4 * Wn) | (m["qy"].abs() > 4 * Hn)
    cd = r.c.detach()
    stiff = (nrl == 0) | (nn < STIFF_NORMAL) | (m["Y.z-0.1"] <= 0) | far | (m["noise"] < STIFF_NOISE) | ~torch.isfinite(r.noise.detach())
    stiff |= (m["clamp"] > 0) & (cd.abs() > STIFF_ACOS * (1 - cd * cd))
    front = m["Y.z-0.1"] > 0
    in_x, in_y = (m["qx"] > 0) & (m["Wn-qx"] > 0), (m["qy"] > 0) & (m["Hn-qy"] > 0)
    cls = {
        "off left": front & (m["qx"] <= 0), "off right": front & (m["Wn-qx"] <= 0), "off top": front & (m["qy"] <= 0), "off bottom": front & (m["Hn-qy"] <= 0),
        "last column": r.valid & (m["qx"] >= Wn - 1), "last row": r.valid & (m["qy"] >= Hn - 1),
        "behind": m["Y.z-0.1"] <= 0,
        "occluded": front & in_x & in_y & (m["occlusion"] < 0),
        "just not occluded": r.valid & (m["occlusion"] < JUST_NOT_OCCLUDED),
        "clamp binds": m["clamp"] < 0,
        "zero reference normal": nrl == 0,
        "zero sampled normal": nn == 0,
    }
    cls = {k: v & ~flip for k, v in cls.items()}
    cls["ordinary"] = r.valid & ~flip_bwd & ~stiff & (m["qx"] < Wn - 1) & (m["qy"] < Hn - 1) & (m["clamp"] > 0)
    return dict(flip=flip, flip_bwd=flip_bwd, stiff=stiff, **cls)


def footprint(q, Wn, Hn):
    """The border-clamped bilinear footprint of positions q (N, 2), float64: x0, y0 (long), fx, fy, bx, by."""
    x, y = q[:, 0].clamp(0, Wn - 1), q[:, 1].clamp(0, Hn - 1)
    x0, y0 = x.floor(), y.floor()
    return x0.long(), y0.long(), x - x0, y - y0, x0 + 1 <= Wn - 1, y0 + 1 <= Hn - 1


def dense_scatter(values, q, Wn, Hn, flags=None):
    """The exact texel sums of a bilinear scatter: values (N, C) float64 contributions of the samples at q (N, 2) -> (C, Hn, Wn)
    float64.  With `flags` (N,) bool also -> (Hn, Wn) bool: the texels that a flagged sample's footprint touches."""
    x0, y0, fx, fy, bx, by = footprint(q, Wn, Hn)
    C = values.shape[1]
    out = torch.zeros(C, Hn * Wn, dtype=F64)
    hit = torch.zeros(Hn * Wn, dtype=torch.bool)
    for dx, dy, w, ok in ((0, 0, (1 - fx) * (1 - fy), torch.ones_like(bx)), (1, 0, fx * (1 - fy), bx), (0, 1, (1 - fx) * fy, by), (1, 1, fx * fy, bx & by)):
        o = ((y0 + dy) * Wn + x0 + dx)[ok]
        out.index_add_(1, o, (values[ok] * w[ok, None]).permute(1, 0).contiguous())
        if flags is not None:
            hit[o[flags[ok]]] = True
    out = out.reshape(C, Hn, Wn)
    return out if flags is None else (out, hit.reshape(Hn, Wn))


# ---------------------------------------------------------------- scenes
def _maps(ref, near, g, d0, dn0):
    H, W, Hn, Wn = ref.H, ref.W, near.H, near.W
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    yn, xn = torch.meshgrid(torch.linspace(-1, 1, Hn), torch.linspace(-1, 1, Wn), indexing="ij")
    depth = (d0 + 0.4 * torch.sin(2 * xx) * torch.cos(1.5 * yy))[None]
    depth_n = (dn0 + 0.4 * torch.cos(1.7 * xn + 0.3) * torch.cos(1.2 * yn))[None]
    normal = torch.stack([0.3 * xx, 0.3 * yy, -torch.ones_like(xx)], 0) * (0.6 + torch.rand(1, H, W, generator=g)) + 0.15 * torch.randn(3, H, W, generator=g)
    normal_n = torch.stack([0.3 * xn + 0.4, 0.3 * yn - 0.3, -torch.ones_like(xn)], 0) * 0.8 + 0.05 * torch.randn(3, Hn, Wn, generator=g)
    return depth, normal, depth_n, normal_n


def _upstream(n, g):
    """Random upstream gradients of both signs, NOT masked by valid; exact zeros on every 5th (noise) and every 7th (angle) pixel."""
    d_noise, d_angle = torch.randn(n, generator=g), torch.randn(n, generator=g)
    d_noise[::5] = 0.0
    d_angle[::7] = 0.0
    return d_noise, d_angle


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> namespace: depth, normal, depth_n, normal_n (float32, CPU), ref, near (RefCam), occlusion, d_noise, d_angle (float32, H W)."""
    if name == "general":  # every edge class, unequal views; 67 x 45 = 3015 pixels = 11 blocks + 199 lanes = 47 waves + 7 lanes
        g = torch.Generator().manual_seed(11)
        ref = RefCam(67, 45, 60.0, 58.0, 33.5, 22.5, (0.0, 0.0, 0.0), (0.0, 0.0, 6.0))
        near = RefCam(53, 41, 70.0, 75.0, 24.3, 22.1, (0.5, -0.2, 0.3), (0.0, 0.0, 6.0))
        depth, normal, depth_n, normal_n = _maps(ref, near, g, 5.5, 5.4)
        depth[0, 2:8, 2:8] = 0.0                                               # background
        depth[0, 2:8, 12:18] = 0.05 + 0.2 * torch.rand(6, 6, generator=g)      # in front of the neighbour's near limit
        normal[:, 36:42, 4:10] = 0.0
        normal_n[:, 15:22, 20:28] = 0.0
        occlusion = 0.05
        # the clamp: sixteen ordinary pixels get the direction of the normal the chain samples for them (which does not depend on
        # the reference normal), twelve along it and four against it
        d = [t.double() for t in (depth, normal, depth_n, normal_n)]
        r = restate(*d, ref, near, occlusion)
        k = classify(r, d[1], near)
        idx = torch.nonzero(k["ordinary"] & (r.nraw.norm(dim=1) > 0.3)).squeeze(1)
        idx = idx[torch.linspace(0, idx.numel() - 1, 16).long()]
        sign = torch.ones(16, dtype=F64)
        sign[12:] = -1.0
        length = 0.7 + 0.6 * torch.rand(16, generator=g).double()
        normal.reshape(3, -1)[:, idx] = (r.nraw[idx] / r.nraw[idx].norm(dim=1, keepdim=True) * (sign * length)[:, None]).permute(1, 0).float()
    elif name == "one_wave":  # a single partial wave in every kernel
        g = torch.Generator().manual_seed(5)
        ref = RefCam(5, 3, 5.0, 4.5, 2.5, 1.5, (0.0, 0.0, 0.0), (0.0, 0.0, 6.0))
        near = RefCam(4, 4, 5.5, 6.0, 2.2, 1.9, (0.3, -0.2, 0.2), (0.0, 0.0, 6.0))
        depth, normal, depth_n, normal_n = _maps(ref, near, g, 5.5, 5.6)
        occlusion = 0.05
    elif name == "contention":  # every contribution on the same four texels
        g = torch.Generator().manual_seed(7)
        ref = RefCam(67, 45, 60.0, 58.0, 33.5, 22.5, (0.0, 0.0, 0.0), (0.0, 0.0, 6.0))
        near = RefCam(2, 2, 1.0, 1.3, 0.9, 1.05, (0.5, -0.2, 0.3), (0.0, 0.0, 6.0))
        depth, normal, depth_n, normal_n = _maps(ref, near, g, 5.5, 5.75)
        occlusion = 0.05
    elif name == "identity":  # noise ~ 0
        # Same pose, size and focal lengths; the neighbour's principal point is a fraction of a pixel off so that no projection
        # sits ON a decision (q = the pixel itself would put every border pixel on `q > 0` and on the clip), and both depth maps
        # sample one affine function of the pixel, which the bilinear lookup reproduces exactly: depth_n(q) = depth(pixel).
        g = torch.Generator().manual_seed(9)
        ref = RefCam(33, 20, 30.0, 29.0, 16.5, 10.0, (0.2, 0.1, -0.3), (0.0, 0.0, 6.0))
        near = RefCam(33, 20, 30.0, 29.0, 16.87, 10.21, (0.2, 0.1, -0.3), (0.0, 0.0, 6.0))
        _, normal, _, normal_n = _maps(ref, near, g, 0.0, 0.0)
        p, pn = pixel_grid(33, 20), pixel_grid(33, 20)
        depth = (4.0 + 0.02 * p[..., 0] + 0.03 * p[..., 1])[None].float()
        depth_n = (4.0 + 0.02 * (pn[..., 0] - 0.37) + 0.03 * (pn[..., 1] - 0.21))[None].float()
        occlusion = 0.05
    else:
        raise KeyError(name)
    d_noise, d_angle = _upstream(ref.W * ref.H, g)
    return types.SimpleNamespace(name=name, depth=depth.contiguous(), normal=normal.contiguous(), depth_n=depth_n.contiguous(), normal_n=normal_n.contiguous(),
                                 ref=ref, near=near, occlusion=occlusion, d_noise=d_noise, d_angle=d_angle)


def evaluate(maps, ref, near, occlusion, d_noise, d_angle):
    """float64 forward + autograd backward -> namespace (restate's, plus grads = [d_depth, d_normal, d_depth_n, d_normal_n] and the
    per-sample contributions dzs (N,), dnraw (N, 3))."""
    leaves = [t.detach().double().requires_grad_(True) for t in maps]
    r = restate(*leaves, ref, near, occlusion)
    (r.noise * d_noise.double() + r.angle * d_angle.double()).sum().backward()
    r.grads = [t.grad for t in leaves]
    r.dzs, r.dnraw = r.zs.grad, r.nraw.grad
    r.leaves = leaves
    return r


def op_by_op(maps, ref, near, occlusion, d_noise, d_angle):
    """gs2m_mvs.mv_geo_torch in float32 on the CPU with autograd: the yardstick of what float32 can do on these inputs."""
    import gs2m_mvs as MV
    leaves = [t.detach().float().clone().requires_grad_(True) for t in maps]
    rc, nc = ref.project_camera(), near.project_camera()
    noise, angle, valid = MV.mv_geo_torch(*leaves, rc, nc, occlusion, pixel_grid(ref.W, ref.H, torch.float32))
    (noise * d_noise + angle * d_angle).sum().backward()
    return types.SimpleNamespace(noise=noise.detach(), angle=angle.detach(), valid=valid, grads=[t.grad for t in leaves])


@functools.lru_cache(maxsize=None)
def reference(name, scale=1.0):
    """One scene evaluated once: .f64 (evaluate), .op (op_by_op), .k (classify's masks), .texel_flip / .texel_stiff (Hn, Wn): the
    neighbour texels that a flip-band / stiff pixel's footprint touches, .scatter (4, Hn, Wn): dense_scatter of the float64
    per-sample contributions.  `scale` multiplies both upstream gradients."""
    s = scene(name)
    maps = (s.depth, s.normal, s.depth_n, s.normal_n)
    up = (s.d_noise * scale, s.d_angle * scale)
    f = evaluate(maps, s.ref, s.near, s.occlusion, *up)
    k = classify(f, f.leaves[1], s.near)
    contrib = torch.cat([f.dzs[:, None], f.dnraw], dim=1)
    qd = f.q.detach()
    scatter, texel_flip = dense_scatter(contrib, qd, s.near.W, s.near.H, k["flip_bwd"])
    _, texel_stiff = dense_scatter(contrib, qd, s.near.W, s.near.H, k["stiff"])
    return types.SimpleNamespace(scene=s, f64=f, op=op_by_op(maps, s.ref, s.near, s.occlusion, *up), k=k, texel_flip=texel_flip, texel_stiff=texel_stiff,
                                 scatter=scatter, upstream=up)


def grouped_errors(x, truth, exclude, stiff):
    """|x - truth| per element where truth is finite and `exclude` is false, split into the regular and the stiff group:
    -> {group: (max error, scale = max |truth|, count, flat index of the worst element)}."""
    x, truth = x.double().reshape(-1), truth.double().reshape(-1)
    ok = torch.isfinite(truth) & ~exclude.reshape(-1)
    out = {}
    for name, sel in (("regular", ok & ~stiff.reshape(-1)), ("stiff", ok & stiff.reshape(-1))):
        if bool(sel.any()):
            e = torch.nan_to_num((x[sel] - truth[sel]).abs(), nan=math.inf)
            out[name] = (float(e.max()), float(truth[sel].abs().max()), int(sel.sum()), int(torch.nonzero(sel).squeeze(1)[e.argmax()]))
        else:
            out[name] = (0.0, 0.0, 0, -1)
    return out
