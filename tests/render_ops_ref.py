"""The ten kernels of csrc/render_ops.hip (pack_features, gbuffer_post / gbuffer_maps, sobel_normal, pbr_inputs, activate,
each forward and backward) restated for the CPU in float64, from the formulas of the reference project -- get_normals and
build_rotation (scene/gaussian_model.py:146-160, utils/general_utils.py:75-98), the feature rows and the G-buffer
post-processing of render() (gaussian_renderer/__init__.py:83-96, 126-141), normal_from_depth_image with the alpha blend
(utils/normal_utils.py:3-72, GR:167-175), the preparation block of pbr_render (pbr/__init__.py:25-43) and the six model
getters (GM:113-144) -- not from the kernels.  Inputs are float32 values held as float64.

Two evaluations of every chain, written once (`_pack_chain`, `_gbuf_chain`, `_normalize4`, `_sigmoid`) and run in two
arithmetics (the sobel stencil: `sobel_f64` as the reference writes it, `SobelRef` on the cancelled form):

  torch float64   values, and the backward passes through autograd (`*_f64`);
  `E` arithmetic  the same lines on (value, error) pairs: every operation adds its own rounding C_* 2^-24 |result| to the
                  error its operands carry, propagated to first order -- |a| eb + |b| ea through a product, ea / |b| +
                  |a / b| eb / |b| through a quotient, ea / (2 sqrt a) through a root, hence e / |m| through m / |m|.  Summed
                  over one output element this is count x 2^-24 x the sum of |terms| that enter it; the counts are the
                  constants C_* below, one per kind of operation, never tuned against a kernel.  The backward passes are
                  written out by hand in this arithmetic (`.backward`); tests/test_render_ops_ref.py holds their values to
                  autograd and to central differences.

Decisions.  Those that compare float32 inputs (the argmin of the scales, the normal mask, the albedo clamp, `len > 0`, the
border) are evaluated on the float32 values and must match exactly.  Those on a computed quantity (the flip dot, s of |s|,
a norm against 1e-12) carry their float64 margin and the error of that quantity as the band: an element is in the flip
band when 0 < |margin| <= band.  A margin of exactly 0 is a planted case: its inputs are small dyadic numbers on which the
float32 evaluation is exact as well (asserted by test_render_ops_ref.py), so it is decided, not in the band."""
import numpy as np
import torch

F32, F64 = np.float32, np.float64
U = 2.0 ** -24                      # unit roundoff of float32
ETA = 2.0 ** -150                   # half the smallest subnormal: the absolute error of a product or quotient that underflows
EPS = F64(F32(1e-12))               # F.normalize's eps as the float32 the kernels compare with
DEN_EPS = F64(F32(1e-8))            # `denom + 1e-8`
SLACK = 1.0 + 2.0 ** -10            # second-order terms of the first-order propagation

# one rounding per correctly rounded float32 operation (the library is built with -ffp-contract=off; `/` and sqrtf are
# correctly rounded): a + b, a - b | a * b | a / b | sqrtf(a)
C_ADD, C_MUL, C_DIV, C_SQRT = 1, 1, 1, 1
# expf: 1 ulp = 2 u, as the device library documents
C_EXP = 2
# one entry of the camera-to-world rotation as the adjugate over the determinant, (a b - c d) * (1 / det): two products and
# their difference 3, the determinant (three cofactors of 3, three products, two adds) 8 relative to sum |terms| <= 3 at a
# rotation, the reciprocal 1, the product 1; entries and cofactors of a rotation are at most 1 -> an absolute 16 u
C_ADJ = 16


# ---------------------------------------------------------------- (value, error) arithmetic
class E:
    """float64 value `v` and a first-order bound `e` of the error a float32 evaluation of the same lines carries"""
    __array_priority__ = 1000
    __array_ufunc__ = None            # ndarray (op) E defers to E's reflected operator

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=F64)
        self.e = np.broadcast_to(np.asarray(e, dtype=F64), self.v.shape)

    @staticmethod
    def lift(x):
        return x if isinstance(x, E) else E(x)

    @staticmethod
    def _rounded(v, e, c, eta=0.0):
        return E(v, e + c * U * np.abs(v) + eta)

    def __add__(self, o):
        o = E.lift(o)
        return E._rounded(self.v + o.v, self.e + o.e, C_ADD)

    def __sub__(self, o):
        o = E.lift(o)
        return E._rounded(self.v - o.v, self.e + o.e, C_ADD)

    def __rsub__(self, o):
        return E.lift(o) - self

    __radd__ = __add__

    def __mul__(self, o):
        o = E.lift(o)
        return E._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e, C_MUL, ETA)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.lift(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = self.v / o.v
            e = self.e / np.abs(o.v) + np.where(o.e == 0, 0.0, np.abs(q) * o.e / np.abs(o.v))
        return E._rounded(q, e, C_DIV, ETA)

    def __rtruediv__(self, o):
        return E.lift(o) / self

    def __neg__(self):
        return E(-self.v, self.e)

    def __getitem__(self, k):
        return E(self.v[k], self.e[k])

    @property
    def shape(self):
        return self.v.shape

    def bound(self):
        return self.e * SLACK


class _Err:
    """the chains in (value, error) arithmetic"""
    @staticmethod
    def sqrt(x):
        r = np.sqrt(x.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(x.e == 0, 0.0, np.minimum(x.e / (2.0 * r), np.sqrt(x.e)))    # |sqrt(a + e) - sqrt(a)| <= sqrt(e) near 0
        return E._rounded(r, e, C_SQRT)

    @staticmethod
    def exp(x):
        r = np.exp(x.v)
        return E._rounded(r, r * x.e, C_EXP)

    @staticmethod
    def where(c, a, b):
        a, b = E.lift(a), E.lift(b)
        a, b = E(np.broadcast_to(a.v, c.shape), np.broadcast_to(a.e, c.shape)), E(np.broadcast_to(b.v, c.shape), np.broadcast_to(b.e, c.shape))
        return E(np.where(c, a.v, b.v), np.where(c, a.e, b.e))

    @staticmethod
    def pad(x):
        return E(np.pad(x.v, 1), np.pad(x.e, 1))


class _Torch:
    """the chains on torch float64 tensors (autograd)"""
    sqrt = staticmethod(torch.sqrt)
    exp = staticmethod(torch.exp)

    @staticmethod
    def where(c, a, b):
        c = torch.from_numpy(np.ascontiguousarray(c))
        a = a if torch.is_tensor(a) else torch.full(c.shape, float(a), dtype=torch.float64)
        b = b if torch.is_tensor(b) else torch.full(c.shape, float(b), dtype=torch.float64)
        return torch.where(c, a, b)

    @staticmethod
    def pad(x):
        return torch.nn.functional.pad(x, (1, 1, 1, 1))


def f64(x):
    return np.asarray(x, dtype=F64)


def t64(x, grad=False):
    return torch.tensor(np.asarray(x, dtype=F64), dtype=torch.float64, requires_grad=grad)


def _cols(a):
    """the columns of an (n, c) array as a list: exact inputs of either arithmetic"""
    return [a[:, j] for j in range(a.shape[1])]


def in_band(margin, band):
    """0 < |margin| <= band: a float32 evaluation may take the other side (a margin of exactly 0 is a planted, exact case)"""
    margin = np.abs(f64(margin))
    return (margin > 0) & (margin <= f64(band) * SLACK)


# ================================================================ pack_features
def first_minimum(scales):
    """torch.argmin: the FIRST index of the minimum -- on the float32 values, exact"""
    return np.argmin(np.asarray(scales, dtype=F32), axis=-1)


def _pack_chain(A, xyz, rot, view, campos, k, sgn, sabs, z_depth):
    """xyz, rot: lists of columns; view (4, 4) and campos (3) float64 constants; k, sgn, sabs: the decisions, given
    -> n[3], dist, dot (the flip's margin, before the flip), s, and the intermediates the backward needs"""
    view, campos = np.asarray(view, dtype=F64).tolist(), np.asarray(campos, dtype=F64).tolist()
    r, x, y, z = rot
    qn = A.sqrt(r * r + x * x + y * y + z * z)                 # build_rotation: norm
    r, x, y, z = r / qn, x / qn, y / qn, z / qn                # q = r / norm
    cols = [[1 - 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z - r * y)],      # R[:, 0]
            [2 * (x * y - r * z), 1 - 2 * (x * x + z * z), 2 * (y * z + r * x)],      # R[:, 1]
            [2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)]]      # R[:, 2]
    m = [A.where(k == 0, cols[0][a], A.where(k == 1, cols[1][a], cols[2][a])) for a in range(3)]   # bmm with the one-hot axis
    vd = [campos[a] - xyz[a] for a in range(3)]                # view_dirs
    dot = m[0] * vd[0] + m[1] * vd[1] + m[2] * vd[2]
    m = [m[a] * sgn for a in range(3)]                         # torch.where(flip_mask, -normals, normals)
    mlen = A.sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2])
    n = [m[a] / mlen for a in range(3)]                        # normals / normals.norm
    cn = [n[0] * view[0][j] + n[1] * view[1][j] + n[2] * view[2][j] for j in range(3)]
    cp = [xyz[0] * view[0][j] + xyz[1] * view[1][j] + xyz[2] * view[2][j] + view[3][j] for j in range(3)]
    s = cn[0] * cp[0] + cn[1] * cp[1] + cn[2] * cp[2]
    dist = cp[2] if z_depth else s * sabs                      # .abs() as the sign it takes
    return dict(n=n, dist=dist, dot=dot, s=s, q=(r, x, y, z), qn=qn, mlen=mlen, cn=cn, cp=cp)


class PackRef:
    """decisions with margins, forward values with error scales; .backward(dF) -> gradients with error scales"""

    def __init__(self, xyz, scales, rot, albedo, roughness, metallic, campos, view, z_depth, blend_metallic):
        self.args = [np.asarray(a, dtype=F32) for a in (xyz, scales, rot, albedo, roughness, metallic)]
        self.view, self.campos = f64(view).reshape(4, 4), f64(campos).reshape(3)
        self.z_depth, self.blend = bool(z_depth), bool(blend_metallic)
        xyz, scales, rot = (f64(a) for a in self.args[:3])
        self.P = xyz.shape[0]
        self.k = first_minimum(self.args[1]) if self.P else np.zeros(0, dtype=np.int64)
        one = np.ones(self.P)
        c0 = _pack_chain(_Err, [E(c) for c in _cols(xyz)], [E(c) for c in _cols(rot)], self.view, self.campos, self.k, one, one, z_depth)
        self.dot, self.dot_band = c0["dot"].v, c0["dot"].e
        self.flip = self.dot < 0.0                              # `< 0.0`: +0 and -0 are not flipped
        self.sgn = np.where(self.flip, -1.0, 1.0)
        self.s = c0["s"].v * self.sgn
        self.s_band = c0["s"].e
        self.sabs = np.sign(self.s)                             # abs backward: 0 at 0
        self.band = in_band(self.dot, self.dot_band) | (in_band(self.s, self.s_band) & (not self.z_depth))
        self.c = _pack_chain(_Err, [E(c) for c in _cols(xyz)], [E(c) for c in _cols(rot)], self.view, self.campos, self.k, self.sgn, self.sabs, z_depth)
        f = np.zeros((self.P, 10))
        e = np.zeros((self.P, 10))
        f[:, 0] = 1.0
        f[:, 1], e[:, 1] = self.c["dist"].v, self.c["dist"].e
        for a in range(3):
            f[:, 2 + a], e[:, 2 + a] = self.c["n"][a].v, self.c["n"][a].e
        f[:, 5:8], f[:, 8] = self.args[3], self.args[4].reshape(-1)
        if self.blend:
            f[:, 9] = self.args[5].reshape(-1)
        self.features, self.features_scale = f, e * SLACK       # channels 0, 5..9 are copies: scale 0

    def torch_forward(self, xyz_t, rot_t):
        c = _pack_chain(_Torch, [xyz_t[:, j] for j in range(3)], [rot_t[:, j] for j in range(4)], self.view, self.campos, self.k,
                        torch.from_numpy(self.sgn), torch.from_numpy(self.sabs), self.z_depth)
        return torch.stack([c["dist"]] + c["n"], dim=1)         # channels 1..4

    def backward_f64(self, dF):
        """float64 autograd -> d_xyz (P, 3), d_rot (P, 4)"""
        x, r = t64(self.args[0], True), t64(self.args[2], True)
        (self.torch_forward(x, r) * t64(dF)[:, 1:5]).sum().backward()
        return x.grad.numpy(), r.grad.numpy()

    def backward(self, dF):
        """the chain rule written out, in (value, error) arithmetic -> dict of (value, scale): d_xyz, d_rot; the copies
        d_albedo, d_roughness, d_metallic are exact"""
        dF = f64(dF)
        c, V = self.c, self.view.tolist()
        n, cn, cp = c["n"], c["cn"], c["cp"]
        dn = [E(dF[:, 2 + a]) for a in range(3)]
        ddist = dF[:, 1]
        if self.z_depth:
            dp = [E(ddist) * V[a][2] for a in range(3)]
        else:
            ds = ddist * self.sabs
            dn = [dn[a] + ((cp[0] * ds) * V[a][0] + (cp[1] * ds) * V[a][1] + (cp[2] * ds) * V[a][2]) for a in range(3)]
            dp = [(cn[0] * ds) * V[a][0] + (cn[1] * ds) * V[a][1] + (cn[2] * ds) * V[a][2] for a in range(3)]
        ndn = n[0] * dn[0] + n[1] * dn[1] + n[2] * dn[2]
        dc = [(dn[a] - n[a] * ndn) / c["mlen"] * self.sgn for a in range(3)]      # through m / |m| and the flip
        r, x, y, z = c["q"]
        jac = [  # d column k / d (r, x, y, z), row by row of the column
            [[0, 0, -4 * y, -4 * z], [2 * z, 2 * y, 2 * x, 2 * r], [-2 * y, 2 * z, -2 * r, 2 * x]],
            [[-2 * z, 2 * y, 2 * x, -2 * r], [0, -4 * x, 0, -4 * z], [2 * x, 2 * r, 2 * z, 2 * y]],
            [[2 * y, 2 * z, 2 * r, 2 * x], [-2 * x, -2 * r, 2 * z, 2 * y], [0, -4 * x, -4 * y, 0]]]
        dq = []
        for b in range(4):
            per_k = [E.lift(jac[kk][0][b]) * dc[0] + E.lift(jac[kk][1][b]) * dc[1] + E.lift(jac[kk][2][b]) * dc[2] for kk in range(3)]
            dq.append(_Err.where(self.k == 0, per_k[0], _Err.where(self.k == 1, per_k[1], per_k[2])))
        q = (r, x, y, z)
        qdq = q[0] * dq[0] + q[1] * dq[1] + q[2] * dq[2] + q[3] * dq[3]
        drot = [(dq[b] - q[b] * qdq) / c["qn"] for b in range(4)]                 # through rot / |rot|
        st = lambda L: (np.stack([t.v for t in L], 1), np.stack([t.e for t in L], 1) * SLACK)
        return dict(d_xyz=st(dp), d_rot=st(drot))


# ================================================================ gbuffer_post / gbuffer_maps
def _gbuf_chain(A, dist, nrm, rays, view, z_depth):
    view = np.asarray(view, dtype=F64).tolist()
    ln = [nrm[0] * view[0][j] + nrm[1] * view[1][j] + nrm[2] * view[2][j] for j in range(3)]   # normal_map^T @ V[:3, :3]
    if z_depth:
        return ln, dist, None
    denom = ln[0] * rays[0] + ln[1] * rays[1] + ln[2] * rays[2]
    e = denom + float(DEN_EPS)
    return ln, dist / -e, e


class GBufRef:
    """buffer (10, N) float32, rays (N, 3) or None"""

    def __init__(self, buffer, rays, view, z_depth):
        self.buf = np.asarray(buffer, dtype=F32).reshape(10, -1)
        self.rays = None if rays is None else f64(rays).reshape(-1, 3)
        self.view, self.z_depth = f64(view).reshape(4, 4), bool(z_depth)
        self.mask = (self.buf[2] != 0) & (self.buf[3] != 0) & (self.buf[4] != 0)     # (normal_map != 0).all(0): exact, -0 is 0
        b = f64(self.buf)
        self.rl = None if self.rays is None else [self.rays[:, j] for j in range(3)]
        ln, depth, e = _gbuf_chain(_Err, E(b[1]), [E(b[2]), E(b[3]), E(b[4])], self.rl, self.view, z_depth)
        self.e = e
        self.local_normal = (np.stack([t.v for t in ln]), np.stack([t.e for t in ln]) * SLACK)
        self.depth = (depth.v, depth.e * SLACK)

    def backward_f64(self, dl, dd):
        b = t64(self.buf, True)
        ln, depth, _ = _gbuf_chain(_Torch, b[1], [b[2], b[3], b[4]], None if self.rl is None else [t64(r) for r in self.rl], self.view, self.z_depth)
        ((torch.stack(ln) * t64(dl)).sum() + (depth * t64(dd)).sum()).backward()
        return b.grad.numpy()

    def backward(self, dl, dd, direct=None):
        """-> (d_buffer channels 1..4 (4, N), scale); direct: the ten upstream gradients of the plain slices or None"""
        b = f64(self.buf)
        N = b.shape[1]
        dl = np.zeros((3, N)) if dl is None else f64(dl).reshape(3, N)
        dd = np.zeros(N) if dd is None else f64(dd).reshape(N)
        dlj = [E(dl[j]) for j in range(3)]
        if self.z_depth:
            ddist = E(dd)
        else:
            ddist = -(E(dd) / self.e)                           # depth = -dist / e
            de = (E(dd) * b[1]) / (self.e * self.e)
            dlj = [dlj[j] + de * self.rl[j] for j in range(3)]
        V = self.view.tolist()
        out = [ddist] + [dlj[0] * V[a][0] + dlj[1] * V[a][1] + dlj[2] * V[a][2] for a in range(3)]
        if direct is not None:
            out = [out[c] if direct[1 + c] is None else out[c] + f64(direct[1 + c]).reshape(N) for c in range(4)]
        return np.stack([t.v for t in out]), np.stack([t.e for t in out]) * SLACK


# ================================================================ sobel_normal
def sobel_f64(depth_t, alpha_t, bg, view, fx, fy, cx, cy):
    """render_normal_from_depth_map as the reference writes it (normalised pixel grid, inverse intrinsics, inverse extrinsics,
    cross product of the point differences, F.normalize, zero border, alpha blend), on torch float64 -> (3, H, W)"""
    H, W = depth_t.shape
    K = t64([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    ext = t64(view).reshape(4, 4).t()
    vx = (torch.arange(W, dtype=torch.float64) / (W - 1)) if W > 1 else torch.zeros(1, dtype=torch.float64)
    vy = (torch.arange(H, dtype=torch.float64) / (H - 1)) if H > 1 else torch.zeros(1, dtype=torch.float64)
    vx, vy = torch.meshgrid(vx, vy, indexing="xy")
    cam = torch.stack([vx * (W - 1) * depth_t, vy * (H - 1) * depth_t, depth_t], dim=-1).reshape(-1, 3) @ torch.inverse(K.t())
    xyz = (torch.cat([cam, torch.ones_like(cam[:, :1])], dim=-1) @ torch.inverse(ext).t())[:, :3].reshape(H, W, 3)
    nrm = torch.zeros(H, W, 3, dtype=torch.float64)
    if H >= 3 and W >= 3:
        m = torch.cross(xyz[1:-1, 2:] - xyz[1:-1, :-2], xyz[:-2, 1:-1] - xyz[2:, 1:-1], dim=-1)
        nrm = torch.nn.functional.pad(torch.nn.functional.normalize(m, p=2, dim=-1, eps=float(EPS)).permute(2, 0, 1), (1, 1, 1, 1)).permute(1, 2, 0)
    out = nrm * alpha_t[..., None] + t64(bg)[None, None] * (1.0 - alpha_t[..., None])
    return out.permute(2, 0, 1)


class SobelRef:
    """the error scales on the form in which the camera centre has cancelled: X_right - X_left = d_r ray_r - d_l ray_l, ray =
    R_c2w K^-1 (u, v, 1).  Mathematically the reference's differences; a float32 evaluation that keeps the centre carries an
    error of |centre| u per point, far above this scale -- the kernels are asked for the accuracy the cancelled form has."""

    def __init__(self, depth, alpha, bg, view, fx, fy, cx, cy):
        self.depth, self.alpha = np.asarray(depth, dtype=F32), np.asarray(alpha, dtype=F32)
        self.bg, self.view = f64(np.asarray(bg, dtype=F32)), f64(view).reshape(4, 4)
        self.k = tuple(F64(F32(t)) for t in (fx, fy, cx, cy))
        H, W = self.depth.shape
        self.H, self.W = H, W
        self.interior = np.zeros((H, W), dtype=bool)
        self.interior[1:-1, 1:-1] = True
        Rc2w = np.linalg.inv(self.view[:3, :3].T)              # inverse of the world-to-camera rotation
        fx, fy, cx, cy = self.k
        u, v = np.meshgrid(np.arange(W, dtype=F64), np.arange(H, dtype=F64), indexing="xy")
        x, y = (E(u) - cx) / fx, (E(v) - cy) / fy
        Re = [[E(Rc2w[a, b], C_ADJ * U) for b in range(3)] for a in range(3)]
        self.ray = [Re[a][0] * x + Re[a][1] * y + Re[a][2] for a in range(3)]
        self.small = H < 3 or W < 3                             # everything is border
        if self.small:
            self.npad = [E(np.zeros((H, W))) for _ in range(3)]
            al = E(f64(self.alpha))
            out = [self.npad[c] * al + self.bg[c] * (1.0 - al) for c in range(3)]
            self.out = (np.stack([t.v for t in out]), np.stack([t.e for t in out]) * SLACK)
            self.band = np.zeros((H, W), dtype=bool)
            return
        D = E(f64(self.depth))
        r = self.ray
        self.a = [D[1:-1, 2:] * r[k][1:-1, 2:] - D[1:-1, :-2] * r[k][1:-1, :-2] for k in range(3)]
        self.b = [D[:-2, 1:-1] * r[k][:-2, 1:-1] - D[2:, 1:-1] * r[k][2:, 1:-1] for k in range(3)]
        a, b = self.a, self.b
        self.m = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        m = self.m
        mm = m[0] * m[0] + m[1] * m[1] + m[2] * m[2]
        self.len = _Err.sqrt(mm)
        self.side = self.len.v >= EPS                           # max(norm, eps): the norm's side, gradient included
        self.margin, self.margin_band = self.len.v - EPS, self.len.e
        dn = _Err.where(self.side, self.len, EPS)
        self.n = [m[k] / dn for k in range(3)]
        al = E(f64(self.alpha))
        npad = [_Err.pad(t) for t in self.n]
        out = [npad[c] * al + self.bg[c] * (1.0 - al) for c in range(3)]
        self.npad = npad
        self.out = (np.stack([t.v for t in out]), np.stack([t.e for t in out]) * SLACK)
        band = np.zeros((H, W), dtype=bool)
        band[1:-1, 1:-1] = in_band(self.margin, self.margin_band)
        self.band = band

    def border_exact(self):
        """the border as float32: 0 * alpha + bg * (1 - alpha), in this order"""
        al = self.alpha
        return np.stack([F32(0) * al + F32(self.bg[c]) * (F32(1) - al) for c in range(3)])

    def backward_f64(self, g):
        d, a = t64(self.depth, True), t64(self.alpha, True)
        (sobel_f64(d, a, self.bg, self.view, *self.k) * t64(g)).sum().backward()
        return (np.zeros((self.H, self.W)) if d.grad is None else d.grad.numpy()), a.grad.numpy()    # all border: the depth is not read

    def backward(self, g):
        """-> d_depth (value, scale), d_alpha (value, scale)"""
        g = f64(g).reshape(3, self.H, self.W)
        H, W = self.H, self.W
        d_alpha = g[0] * (self.npad[0] - self.bg[0]) + g[1] * (self.npad[1] - self.bg[1]) + g[2] * (self.npad[2] - self.bg[2])
        dv, de = np.zeros((H, W)), np.zeros((H, W))
        if not self.small:
            al = f64(self.alpha)[1:-1, 1:-1]
            dn = [E(g[k][1:-1, 1:-1]) * al for k in range(3)]
            n, a, b, r = self.n, self.a, self.b, self.ray
            ndn = n[0] * dn[0] + n[1] * dn[1] + n[2] * dn[2]
            with np.errstate(divide="ignore", invalid="ignore"):
                dm = [_Err.where(self.side, (dn[k] - n[k] * ndn) / self.len, dn[k] / EPS) for k in range(3)]
            da = [b[1] * dm[2] - b[2] * dm[1], b[2] * dm[0] - b[0] * dm[2], b[0] * dm[1] - b[1] * dm[0]]   # m = a x b
            db = [dm[1] * a[2] - dm[2] * a[1], dm[2] * a[0] - dm[0] * a[2], dm[0] * a[1] - dm[1] * a[0]]
            terms = [((slice(1, -1), slice(2, None)), da, 1.0), ((slice(1, -1), slice(None, -2)), da, -1.0),
                     ((slice(None, -2), slice(1, -1)), db, 1.0), ((slice(2, None), slice(1, -1)), db, -1.0)]
            mag = np.zeros((H, W))
            for sl, dv3, sign in terms:
                t = dv3[0] * r[0][sl] + dv3[1] * r[1][sl] + dv3[2] * r[2][sl]
                dv[sl] += sign * t.v
                de[sl] += t.e
                mag[sl] += np.abs(t.v)
            de += 3 * C_ADD * U * mag                           # the sum of the (up to) four stencil terms: three adds
        return (dv, de * SLACK), (d_alpha.v, d_alpha.e * SLACK)


# ================================================================ pbr_inputs
class PbrRef:
    """maps as (c, N) float32; metallic_map None: the estimate alpha * clamp(1 - roughness, 0, 1)"""

    def __init__(self, normal_map, albedo_map, roughness_map, alpha_map, metallic_map, rmin, rmax):
        nm = np.asarray(normal_map, dtype=F32).reshape(3, -1)
        am = np.asarray(albedo_map, dtype=F32).reshape(3, -1)
        ro = np.asarray(roughness_map, dtype=F32).reshape(-1)
        self.albedo_map = am
        with np.errstate(under="ignore"):
            len32 = np.sqrt(nm[0] * nm[0] + nm[1] * nm[1] + nm[2] * nm[2])       # torch.norm(dim=0) on the float32 map
        self.nonzero = len32 > 0                                # `> 0` on the float32 norm: exact (squares that underflow give 0)
        n = [E(f64(nm[c])) for c in range(3)]
        ln = _Err.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
        self.side = ln.v >= EPS
        self.margin, self.margin_band = ln.v - EPS, ln.e
        self.band = in_band(self.margin, self.margin_band) & self.nonzero
        dn = _Err.where(self.side, ln, EPS)
        with np.errstate(divide="ignore", invalid="ignore"):
            nn = [_Err.where(self.nonzero, n[c] / dn, n[c]) for c in range(3)]
        self.normals = (np.stack([t.v for t in nn], 1), np.stack([t.e for t in nn], 1) * SLACK)          # pixel-major (N, 3)
        self.albedo = np.where(am < 0, F32(0), np.where(am > 1, F32(1), am)).astype(F32).T.copy()        # clamp: exact, (N, 3)
        self.passes = (am >= 0) & (am <= 1)                    # clamp's backward: inclusive edges
        rough = E(f64(ro)) * (E(F64(F32(rmax))) - F64(F32(rmin))) + F64(F32(rmin))
        self.roughness = (rough.v, rough.e * SLACK)
        if metallic_map is not None:
            self.metallic_exact = np.asarray(metallic_map, dtype=F32).reshape(-1)
            self.metallic = None
        else:
            q = 1.0 - E(f64(ro))
            qc = E(np.clip(q.v, 0.0, 1.0), q.e)                # the clamp is 1-Lipschitz: it keeps the error
            met = E(f64(np.asarray(alpha_map, dtype=F32).reshape(-1))) * qc
            self.metallic_exact, self.metallic = None, (met.v, met.e * SLACK)

    def backward_exact(self, d_albedo):
        """d_albedo (N, 3) -> d_albedo_map (3, N): a selection, exact"""
        return np.where(self.passes, np.asarray(d_albedo, dtype=F32).T, F32(0)).astype(F32)


# ================================================================ activate
def _normalize4(A, q, side, zero):
    """F.normalize(q, dim=1): q / max(|q|, 1e-12) with the max's side given; zero: |q| == 0 (the norm's gradient is 0 there)"""
    qq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    nn = A.sqrt(A.where(zero, 1.0, qq))
    n = A.where(side, nn, float(EPS))
    return [q[b] / n for b in range(4)], nn, n


def _sigmoid(A, x):
    return 1.0 / (1.0 + A.exp(-x))


class ActivateRef:
    def __init__(self, scaling, rotation, opacity, albedo, roughness, metallic):
        self.raw = [None if a is None else np.asarray(a, dtype=F32) for a in (scaling, rotation, opacity, albedo, roughness, metallic)]
        self.out = [None] * 6
        if self.raw[0] is not None:
            y = _Err.exp(E(f64(self.raw[0])))
            self.out[0] = (y.v, y.e * SLACK)
        if self.raw[1] is not None:
            q = f64(self.raw[1])
            nn64 = np.sqrt((q * q).sum(1))
            self.zero = nn64 == 0
            self.side = nn64 >= EPS
            y, nn, _ = _normalize4(_Err, [E(c) for c in _cols(q)], self.side, self.zero)
            self.margin, self.margin_band = nn64 - EPS, np.where(self.zero, 0.0, nn.e)     # a norm of exact zeros is exactly 0
            self.band = in_band(self.margin, self.margin_band)
            self.out[1] = (np.stack([t.v for t in y], 1), np.stack([t.e for t in y], 1) * SLACK)
        for k in range(2, 6):
            if self.raw[k] is not None:
                y = _sigmoid(_Err, E(f64(self.raw[k])))
                self.out[k] = (y.v, y.e * SLACK)

    def forward_f64(self, k, x_t):
        if k == 0:
            return torch.exp(x_t)
        if k == 1:
            return torch.stack(_normalize4(_Torch, [x_t[:, b] for b in range(4)], self.side, self.zero)[0], dim=1)
        return torch.sigmoid(x_t)

    def backward_f64(self, k, g):
        x = t64(self.raw[k], True)
        (self.forward_f64(k, x) * t64(g)).sum().backward()
        return x.grad.numpy()

    def backward(self, k, g, y=None):
        """the backward as the entry point receives it: the upstream gradient g and, for exp and sigmoid, the SAVED float32
        activation y (an exact input) -> (value, scale)"""
        g = f64(g)
        if k == 0:
            d = E(g) * f64(y)                                   # d exp = g y
        elif k == 1:
            q = [E(c) for c in _cols(f64(self.raw[1]))]
            gq = _cols(g)
            _, nn, n = _normalize4(_Err, q, self.side, self.zero)
            dot = q[0] * gq[0] + q[1] * gq[1] + q[2] * gq[2] + q[3] * gq[3]
            with np.errstate(divide="ignore", invalid="ignore"):
                kk = _Err.where(self.side & ~self.zero, dot / (n * n * nn), 0.0)     # below the clamp the divisor is a constant
            dq = [E(gq[b]) / n - q[b] * kk for b in range(4)]
            return np.stack([t.v for t in dq], 1), np.stack([t.e for t in dq], 1) * SLACK
        else:
            yy = f64(y)
            d = (E(g) * (1.0 - E(yy))) * yy                     # d sigmoid = g (1 - y) y
        return d.v, d.e * SLACK


# ================================================================ scenes
def identity_camera(campos):
    """world_view_transform (row-vector convention) of an axis-aligned camera at `campos`: every product with it is exact"""
    view = np.eye(4, dtype=F32)
    view[3, :3] = -np.asarray(campos, dtype=F32)
    return view, np.asarray(campos, dtype=F32)


def general_camera(W=96, H=64, eye=(1.0, -0.7, 0.5), target=(0.2, 0.1, 6.0)):
    """the rotated, non-axis-aligned camera of tests/test_render_ops_gpu.py (gs2m_synth.look_at_camera) -> dict of float32 arrays"""
    import gs2m_synth as S
    cam = S.look_at_camera(W, H, eye, target)
    return dict(view=cam["viewmatrix"].numpy().astype(F32), campos=cam["campos"].numpy().astype(F32), fx=float(cam["fx"]), fy=float(cam["fy"]),
                cx=0.5 * W, cy=0.5 * H, W=W, H=H)


def rays_of(cam, W, H):
    """Camera.get_rays as float32: ((u - cx) / fx, (v - cy) / fy, 1), pixel-major (H W, 3)"""
    u, v = np.meshgrid(np.arange(W, dtype=F32), np.arange(H, dtype=F32), indexing="xy")
    rx, ry = (u - F32(0.5 * W)) / F32(cam["fx"]), (v - F32(0.5 * H)) / F32(cam["fy"])
    return np.stack([rx, ry, np.ones_like(rx)], axis=-1).reshape(-1, 3).astype(F32)


PACK_SEEDS = {1: 11, 255: 12, 256: 13, 257: 14, 513: 15}       # the general scenes: seeds for which the flip band stays under 1 %


def pack_scene(P, seed):
    """a general scene in front of general_camera(): positions in its frustum, anisotropic scales, quaternions of norm 0.5..2"""
    rng = np.random.default_rng(seed)
    xyz = (rng.standard_normal((P, 3)) * [1.5, 1.0, 1.5] + [0.2, 0.1, 6.0]).astype(F32)
    scales = np.exp(rng.uniform(-5.0, -2.0, (P, 3))).astype(F32)
    rot = rng.standard_normal((P, 4))
    rot = (rot / np.linalg.norm(rot, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (P, 1))).astype(F32)
    albedo, roughness, metallic = (rng.uniform(0.05, 0.95, s).astype(F32) for s in ((P, 3), (P, 1), (P, 1)))
    dF = rng.standard_normal((P, 10)).astype(F32)
    return dict(xyz=xyz, scales=scales, rot=rot, albedo=albedo, roughness=roughness, metallic=metallic, dF=dF)


PLANTED_CAMPOS = (0.5, -0.25, 1.0)
PLANTED_ROWS = ["tie01", "tie12", "tie02", "tie012", "dot+0", "dot-0", "front", "back", "qn1e-3", "qn1e3"]


def pack_planted():
    """the planted rows under identity_camera(PLANTED_CAMPOS); every number a small dyadic, so that the float32 evaluation of the
    flip dot and of s is exact.  -> scene dict (as pack_scene) with `rows`: name -> index, and `expect`: name -> (k, flip, dot)"""
    c = np.array(PLANTED_CAMPOS, dtype=F64)
    ident, half_x = [1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]    # R = I;  R = diag(1, -1, -1)
    g = np.array([0.6, -0.48, 0.64, 0.0])                         # a general unit quaternion for the norm rows
    rows = {
        # name: (xyz, scales, rot), expected (k, flip, dot)
        "tie01": ((1.0, 0.5, 3.0), (0.25, 0.25, 0.5), ident, (0, True, -0.5)),        # m = e0, dot = c0 - x0
        "tie12": ((1.0, 0.5, 3.0), (0.5, 0.25, 0.25), ident, (1, True, -0.75)),
        "tie02": ((1.0, 0.5, 3.0), (0.25, 0.5, 0.25), ident, (0, True, -0.5)),
        "tie012": ((0.25, 0.5, 3.0), (0.125, 0.125, 0.125), ident, (0, False, 0.25)),
        "dot+0": ((0.5, 0.75, 3.0), (0.125, 0.5, 0.5), ident, (0, False, 0.0)),        # on the plane through the centre: 1 * +0
        "dot-0": ((1.0, -0.25, 3.0), (0.5, 0.125, 0.5), half_x, (1, False, 0.0)),      # m = (0, -1, 0): 0 * -0.5 + -1 * +0 + 0 * -2 = -0
        "front": ((0.0, 0.5, 3.0), (0.125, 0.5, 0.5), ident, (0, False, 0.5)),         # the same |dot| on each side of the flip
        "back": ((1.0, 0.5, 3.0), (0.125, 0.5, 0.5), ident, (0, True, -0.5)),
        "qn1e-3": ((0.3, 0.2, 4.0), (0.02, 0.01, 0.03), list(g * 1e-3), None),
        "qn1e3": ((-0.4, 0.1, 5.0), (0.02, 0.03, 0.01), list(g * 1e3), None),
    }
    names = list(rows)
    assert names == PLANTED_ROWS
    rng = np.random.default_rng(7)
    P = len(names)
    sc = dict(xyz=np.array([rows[n][0] for n in names], dtype=F32), scales=np.array([rows[n][1] for n in names], dtype=F32),
              rot=np.array([rows[n][2] for n in names], dtype=F32), albedo=rng.uniform(0.05, 0.95, (P, 3)).astype(F32),
              roughness=rng.uniform(0.05, 0.95, (P, 1)).astype(F32), metallic=rng.uniform(0.05, 0.95, (P, 1)).astype(F32),
              dF=(rng.integers(-8, 9, (P, 10)) / 4.0).astype(F32))
    sc["rows"] = {n: i for i, n in enumerate(names)}
    sc["expect"] = {n: rows[n][3] for n in names}
    return sc


PIXEL_SIZES = [(1, 1), (2, 5), (3, 3), (16, 16), (17, 16), (16, 18), (33, 17), (35, 50)]       # (H, W)


def gbuffer_scene(H, W, seed, cam):
    """-> buffer (10, H, W), rays (H W, 3), the planted pixels (name -> flat index) where the frame has room for them"""
    rng = np.random.default_rng(seed)
    N = H * W
    buf = rng.standard_normal((10, N)).astype(F32)
    buf[1] = np.abs(buf[1]) + F32(0.5)
    rays = rays_of(cam, W, H)
    planted = {}
    if N >= 10:
        planted = {"one_zero": 1, "minus_zero": 2, "all_zero": 3, "small_denom": 4, "two_zero": 5}
        buf[3, 1] = 0.0                                         # exactly one zero channel: mask off, the rest unchanged
        buf[2, 2] = -0.0                                        # -0.0 != 0 is false: mask off
        buf[2:5, 3] = 0.0
        buf[2:4, 5] = 0.0
        # a normal nearly perpendicular to its pixel's ray: denom = 2^-10 |ray|^2 to a few ulp
        r = f64(rays[4])
        perp = np.cross(r, [0.3, 1.0, 0.2])
        ln = perp / np.linalg.norm(perp) + 2.0 ** -10 * r
        buf[2:5, 4] = (f64(cam["view"])[:3, :3] @ ln).astype(F32)     # world normal whose camera-space image is ln
    return buf.reshape(10, H, W), rays, planted


def sobel_scene(H, W, seed, kind="general"):
    rng = np.random.default_rng(seed)
    depth = (rng.random((H, W)) * 3.0 + 2.0).astype(F32)
    alpha = rng.random((H, W)).astype(F32)
    planted = {}
    if kind == "constant":
        depth[:] = F32(3.5)
    if kind == "general" and H * W >= 4:
        alpha.reshape(-1)[0], alpha.reshape(-1)[-1] = 0.0, 1.0    # alpha of exactly 0 and 1 on the border
    if kind == "general" and H >= 5 and W >= 5:
        alpha[2, 1], alpha[1, 2] = 0.0, 1.0                      # ... and inside
        depth[2, 1] = depth[2, 3] = 0.0                          # both horizontal neighbours of (2, 2) at the centre: a = 0 exactly
        planted["zero_cross"] = (2, 2)
    bg = np.array([0.3, 0.1, 0.7], dtype=F32)
    g = rng.standard_normal((3, H, W)).astype(F32)
    return dict(depth=depth, alpha=alpha, bg=bg, g=g, planted=planted)


def pbr_scene(H, W, seed):
    rng = np.random.default_rng(seed)
    N = H * W
    nm = rng.standard_normal((3, N)).astype(F32)
    am = rng.uniform(-0.2, 1.2, (3, N)).astype(F32)
    ro = rng.uniform(-0.3, 1.3, N).astype(F32)                  # 1 - roughness on both sides of [0, 1]
    al, mm = rng.random(N).astype(F32), rng.random(N).astype(F32)
    planted = {}
    if N >= 10:
        nxt = lambda v, to: np.nextafter(F32(v), F32(to))
        planted = {"zero_normal": 0, "underflow": 1, "below_eps": 2, "at_eps": 3, "albedo_edges": 4, "albedo_outside": 5}
        nm[:, 0] = 0.0
        nm[:, 1] = (1e-25, -2e-25, 5e-26)                       # squares underflow to 0: norm 0, the map passes unnormalised
        nm[:, 2] = (3e-13, 0.0, -4e-13)                         # norm 5e-13 < 1e-12: divided by the clamp
        nm[:, 3] = (F32(1e-12), 0.0, 0.0)                       # norm == float32(1e-12)
        am[:, 4] = (0.0, 1.0, -0.0)
        am[:, 5] = (nxt(0, -1), nxt(1, 2), -3.0)
        ro[4], ro[5], ro[6], ro[7] = -0.5, 1.5, 0.0, 1.0
    g = rng.standard_normal((N, 3)).astype(F32)
    return dict(normal=nm, albedo=am, roughness=ro, alpha=al, metallic=mm, g=g, planted=planted)


ACT_PLANTED = ["sig+20", "sig-20", "sig+90", "sig-90", "q_zero", "q_below", "q_at_eps", "q_large"]


def activate_scene(P, seed):
    """raw parameters (float32) and upstream gradients; the planted rows where P has room"""
    rng = np.random.default_rng(seed)
    shapes = [(P, 3), (P, 4), (P, 1), (P, 3), (P, 1), (P, 1)]
    raw = [(rng.standard_normal(s) * 2.0).astype(F32) for s in shapes]
    g = [rng.standard_normal(s).astype(F32) for s in shapes]
    planted = {}
    if P >= len(ACT_PLANTED):
        planted = {n: i for i, n in enumerate(ACT_PLANTED)}
        for name, v in (("sig+20", 20.0), ("sig-20", -20.0), ("sig+90", 90.0), ("sig-90", -90.0)):
            for k in (2, 3, 4, 5):
                raw[k][planted[name]] = v
        raw[1][planted["q_zero"]] = 0.0
        raw[1][planted["q_below"]] = (3e-13, 0.0, -4e-13, 0.0)
        raw[1][planted["q_at_eps"]] = (0.0, F32(1e-12), 0.0, 0.0)
        raw[1][planted["q_large"]] = (3e6, -4e6, 1e6, 2e6)
    return raw, g, planted
