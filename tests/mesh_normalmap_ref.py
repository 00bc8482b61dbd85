"""The tangent frame, the normal-map encode and decode, the texel conversion (include/gs2m_meshbake.h, the Tangent frame .. Normals
paragraphs) and the textured G-buffer (include/gs2m_meshview.h, the Textured paragraph) restated in float64 numpy,
operation for operation, with the synthetic scenes the tests of them share.  Visibility and barycentrics are mesh_view_ref's, the
atlas and its texels mesh_texture_ref's.  Not collected.  The arrays of the cached scenes are shared: leave them unchanged.

What two correct evaluations may settle differently is reported beside the values: `band`, a packed byte whose 255 (0.5 m + 0.5) +
0.5 lies within BAND of an integer -- counted only where m was computed: the constant (0, 0, 1) of an empty texel, an invalid
frame or an unusable normal is the same constant on both sides, and its 128 is exact --; and `margins`, the distance of every
decision (dot(N, Nf) > 0, m_z > 0, det == 0) from its threshold, relative to the size of its terms, 0 meaning exactly on it."""
import functools

import numpy as np

import mesh_texture_ref as T
import mesh_view_ref as MV
import tnt_cull_ref as R

BAND = 1e-9
# Encode then decode: each component of the unit m moves by at most 1/255 in the round trip -- the byte is the nearest of 256 levels
# 2/255 apart in [-1, 1], so at most half a step, 1/255, off -- which moves m by at most d = sqrt(3)/255 in length.  The decoded
# vector has length at least 1 - d, and a vector of length r >= 1 - d that ends within d of a unit vector makes with it an angle of
# at most asin(d / (1 - d)): 0.006839 rad.
QUANT_ANGLE = float(np.arcsin(np.sqrt(3.0) / 255.0 / (1.0 - np.sqrt(3.0) / 255.0)))


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def _unit(a):
    """-> (a / |a| where that exists, else 0; whether it exists)"""
    with np.errstate(all="ignore"):
        s = _dot(a, a)
        ok = (s > 0.0) & np.isfinite(a).all(-1)
        u = a / np.sqrt(s)[..., None]
        ok = ok & np.isfinite(u).all(-1)
    return np.where(ok[..., None], u, 0.0), ok


def frame(a, b, c, uv, N):
    """rows: corners (n, 3), uv (n, 3, 2) the fp32 UVs widened, N (n, 3) -> dict(T, B, N (n, 3), valid (n,), d_u, d_v (n, 3),
    margins: dict(nf, det) relative distances from the decisions' thresholds, inf where the decision is not taken)"""
    a, b, c, N = (np.asarray(x, np.float64).reshape(-1, 3) for x in (a, b, c, N))
    uv = np.asarray(uv, np.float64).reshape(-1, 3, 2)
    z = np.array([0.0, 0.0, 1.0])
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        du1, dv1, du2, dv2 = uv[:, 1, 0] - uv[:, 0, 0], uv[:, 1, 1] - uv[:, 0, 1], uv[:, 2, 0] - uv[:, 0, 0], uv[:, 2, 1] - uv[:, 0, 1]
        det = du1 * dv2 - du2 * dv1
        Nf = _cross(e1, e2)
        Uf, face = _unit(Nf)
        Un, own = _unit(N)
        d = _dot(Un, Nf)
        Nn = np.where(face[:, None], np.where((own & (d > 0.0))[:, None], Un, Uf), np.where(own[:, None], Un, z))
        det_ok = (det != 0.0) & np.isfinite(det)
        du = (e1 * dv2[:, None] - e2 * dv1[:, None]) / det[:, None]
        dv = (e2 * du1[:, None] - e1 * du2[:, None]) / det[:, None]
        t = du - Nn * _dot(Nn, du)[:, None]
        Tn, tok = _unit(t)
        valid = face & det_ok & tok
        Tn = np.where(valid[:, None], Tn, 0.0)
        B = np.where(valid[:, None], -_cross(Nn, Tn), 0.0)
        m_nf = np.where(face & own, np.abs(d) / np.sqrt(_dot(Nf, Nf)), np.inf)
        m_det = np.where(face, np.abs(det) / (np.abs(du1 * dv2) + np.abs(du2 * dv1)), np.inf)
        m_det = np.where(np.isnan(m_det), 0.0, m_det)
    return dict(T=Tn, B=B, N=Nn, valid=valid, d_u=du, d_v=dv, margins=dict(nf=m_nf, det=m_det))


def encode(F, n):
    """-> (m (n, 3), computed (n,): m came from arithmetic, not from the constant; margin (n,) of the m_z decision)"""
    u, ok = _unit(np.asarray(n, np.float64).reshape(-1, 3))
    with np.errstate(all="ignore"):
        q = np.stack([_dot(u, F["T"]), _dot(u, F["B"]), _dot(u, F["N"])], axis=-1)
        margin = np.where(ok & F["valid"], np.abs(q[:, 2]), np.inf)
        q[:, 2] = np.where(q[:, 2] > 0.0, q[:, 2], 0.0)
        m, mok = _unit(q)
    computed = ok & F["valid"] & mok
    return np.where(computed[:, None], m, np.array([0.0, 0.0, 1.0])), computed, margin


def pack(m):
    return np.floor(255.0 * (0.5 * np.asarray(m, np.float64) + 0.5) + 0.5).astype(np.uint8)


def band(m, computed):
    """(n, 3) bool: the byte may differ by one between two evaluations"""
    y = 255.0 * (0.5 * np.asarray(m, np.float64) + 0.5) + 0.5
    return (np.abs(y - np.rint(y)) < BAND) & np.asarray(computed, bool)[:, None]


def unpack(byte):
    return np.asarray(byte, np.float64) / 255.0 * 2.0 - 1.0


def decode(F, m):
    m = np.asarray(m, np.float64).reshape(-1, 3)
    s = (F["T"] * m[:, 0:1] + F["B"] * m[:, 1:2]) + F["N"] * m[:, 2:3]
    u, ok = _unit(s)
    return np.where((ok & F["valid"])[:, None], u, F["N"])


def texel_frames(owner, tnormals, tris, uvs, verts):
    """the frames of the texels (flattened) -> (F with every row filled, usable (n,): owner and corners in range)"""
    owner = np.asarray(owner, np.int64).reshape(-1)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    usable = (owner >= 0) & (owner < len(tris))
    t = tris[np.where(usable, owner, 0)] if len(tris) else np.zeros((len(owner), 3), np.int64)
    usable = usable & ((t >= 0) & (t < len(verts))).all(1)
    t = np.where(usable[:, None], t, 0)
    if len(verts) == 0:
        verts = np.zeros((1, 3))
    uv = np.asarray(uvs, np.float32).reshape(-1, 3, 2)[np.where(usable, owner, 0)] if len(tris) else np.zeros((len(owner), 3, 2))
    F = frame(verts[t[:, 0]], verts[t[:, 1]], verts[t[:, 2]], uv, np.asarray(tnormals, np.float64).reshape(-1, 3))
    F["valid"] = F["valid"] & usable
    return F, usable


def texture_normals(owner, tnormals, tris, uvs, verts, values, offset):
    """gs2m_texture_normals -> dict(tangent (n, 3), bytes (n, 3) uint8, band (n, 3), computed (n,), margins: dict(nf, det, mz))"""
    F, usable = texel_frames(owner, tnormals, tris, uvs, verts)
    v = np.asarray(values, np.float32).reshape(len(usable), -1)[:, offset:offset + 3].astype(np.float64)
    m, computed, mz = encode(F, v)
    inf = np.full(len(usable), np.inf)
    return dict(tangent=m, bytes=pack(m), band=band(m, computed), computed=computed,
                margins=dict(nf=np.where(usable, F["margins"]["nf"], inf), det=np.where(usable, F["margins"]["det"], inf), mz=mz))


# ---- the textured G-buffer -----------------------------------------------------------------------------------------------------

def srgb_decode(e):
    e = np.asarray(e, np.float64)
    return np.where(e <= 12.92 * 0.0031308, e / 12.92, np.power((np.maximum(e, 0.04) + 0.055) / 1.055, 2.4))


def lookup(image, u, v, decode_byte):
    """image (th, tw, 3) uint8; u, v (n,) -> (n, 3): the Textured paragraph's bilinear lookup, bytes decoded before the mix"""
    th, tw = image.shape[:2]
    x, y = u * float(tw) - 0.5, v * float(th) - 0.5
    fx0, fy0 = np.floor(x), np.floor(y)
    tx, ty = x - fx0, y - fy0
    x0 = np.clip(np.nan_to_num(fx0, nan=-1.0), -1, tw).astype(np.int64)
    y0 = np.clip(np.nan_to_num(fy0, nan=-1.0), -1, th).astype(np.int64)
    w = [(1.0 - tx) * (1.0 - ty), tx * (1.0 - ty), (1.0 - tx) * ty, tx * ty]
    tap = [decode_byte(image[np.clip(y0 + k // 2, 0, th - 1), np.clip(x0 + k % 2, 0, tw - 1)]) for k in range(4)]
    return ((tap[0] * w[0][:, None] + tap[1] * w[1][:, None]) + tap[2] * w[2][:, None]) + tap[3] * w[3][:, None]


def keys(vis):
    """mesh_view_ref.visibility's result as the device's int64 keys"""
    k = (vis["zbits"].astype(np.uint64) << np.uint64(32)) | (vis["tri"].astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    return np.where(vis["tri"] >= 0, k, np.uint64(0xFFFFFFFFFFFFFFFF)).view(np.int64)


def gbuffer_textured(verts, tris, uvs, w2c, fx, fy, cx, cy, H, W, ss, vis, normals, base, srgb=True, orm=None, normal_map=None):
    """-> dict(normal, view_dir, albedo (n, Hs, Ws, 3) float32, roughness, metallic (n, Hs, Ws) float32, coverage (n, Hs, Ws) bool, uv (n, Hs, Ws, 2) float64: the samples' texture coordinates).
    vis: mesh_view_ref.visibility of the same arguments; normals: (V, 3) vertex normals or None for flat."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    w2c = np.asarray(w2c, np.float64).reshape(-1, 4, 4)
    uvs = np.asarray(uvs, np.float32).astype(np.float64).reshape(-1, 3, 2)
    Hs, Ws = H * ss, W * ss
    r = R.pixel_rays(Hs, Ws, ss * fx, ss * fy, ss * cx, ss * cy)
    n = len(w2c)
    out = dict(normal=np.zeros((n, Hs * Ws, 3), np.float32), view_dir=np.zeros((n, Hs * Ws, 3), np.float32),
               albedo=np.zeros((n, Hs * Ws, 3), np.float32), roughness=np.zeros((n, Hs * Ws), np.float32),
               metallic=np.zeros((n, Hs * Ws), np.float32), coverage=np.zeros((n, Hs * Ws), bool), uv=np.zeros((n, Hs * Ws, 2)))
    world = lambda M, x: np.stack([(M[0, k] * x[:, 0] + M[1, k] * x[:, 1]) + M[2, k] * x[:, 2] for k in range(3)], axis=1)
    with np.errstate(all="ignore"):
        for v, M in enumerate(w2c):
            cam = R.to_camera(verts, M)
            p = np.nonzero(vis["tri"][v].ravel() >= 0)[0]
            ti = vis["tri"][v].ravel()[p]
            t = tris[ti]
            a, b, c, ray = cam[t[:, 0]], cam[t[:, 1]], cam[t[:, 2]], r[p]
            l0, l1, l2 = MV.barycentrics(a, b, c, ray)
            N = _cross(b - a, c - a)
            if normals is not None:
                vn = np.asarray(normals, np.float64)
                rot = np.stack([(M[d, 0] * vn[:, 0] + M[d, 1] * vn[:, 1]) + M[d, 2] * vn[:, 2] for d in range(3)], axis=1)
                S = (l0[:, None] * rot[t[:, 0]] + l1[:, None] * rot[t[:, 1]]) + l2[:, None] * rot[t[:, 2]]
                ok = (vn[t] != 0).any(axis=2).all(axis=1) & np.isfinite(S).all(axis=1) & (S != 0).any(axis=1)
                N = np.where(ok[:, None], S, N)
            uv = uvs[ti]
            u = (l0 * uv[:, 0, 0] + l1 * uv[:, 1, 0]) + l2 * uv[:, 2, 0]
            w = (l0 * uv[:, 0, 1] + l1 * uv[:, 1, 1]) + l2 * uv[:, 2, 1]
            out["uv"][v, p] = np.stack([u, w], axis=1)
            Vw = world(M, -ray)
            if normal_map is not None:
                F = frame(verts[t[:, 0]], verts[t[:, 1]], verts[t[:, 2]], uv, world(M, N))
                nw = decode(F, lookup(normal_map, u, w, unpack))
                nw = np.where((_dot(nw, world(M, ray)) > 0.0)[:, None], -nw, nw)
            else:
                N = np.where((_dot(N, ray) > 0.0)[:, None], -N, N)
                Nw = world(M, N)
                nw = Nw / np.sqrt(_dot(Nw, Nw))[:, None]
            out["normal"][v, p] = nw.astype(np.float32)
            out["view_dir"][v, p] = (Vw / np.sqrt(_dot(Vw, Vw))[:, None]).astype(np.float32)
            dec = (lambda x: srgb_decode(x / 255.0)) if srgb else (lambda x: x / 255.0)
            out["albedo"][v, p] = lookup(base, u, w, dec).astype(np.float32)
            out["roughness"][v, p], out["metallic"][v, p] = 1.0, 0.0
            if orm is not None:
                o = lookup(orm, u, w, lambda x: x / 255.0)
                out["roughness"][v, p], out["metallic"][v, p] = o[:, 1].astype(np.float32), o[:, 2].astype(np.float32)
            out["coverage"][v, p] = True
    return {k: x.reshape((n, Hs, Ws) + x.shape[2:]) for k, x in out.items()}


# ---- scenes --------------------------------------------------------------------------------------------------------------------

SCENES = ("one", "four", "six_classes", "zero_area", "opposed", "sphere")


def normal_field(p, g):
    """The analytic world-normal field the scenes bake: the unit of g (a texel's own normal) bent by a smooth vector of length up
    to 0.35 sqrt(3) < 0.61 -- it stays well inside the hemisphere of g, so no m_z decision is near its threshold.  (n, 3)"""
    u, _ = _unit(np.asarray(g, np.float64))
    return u + 0.35 * np.stack([np.sin(1.7 * p[:, 0] + 0.3), np.sin(2.3 * p[:, 1] + 1.1), np.sin(1.3 * p[:, 2] + 0.7)], axis=1)


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict(verts, tris, normals (V, 3) or None, density, atlas, tex, values (HW, 8) float32: five random material planes and
    the baked normal in the planes 5 .. 7, want: texture_normals of it)"""
    if name == "sphere":
        c = T.sphere_case()
        verts, tris, normals, density, atlas, tex = c["verts"], c["tris"], c["normals"], c["density"], c["atlas"], c["tex"]
    else:
        verts, tris, density = T.small_shape("two" if name == "opposed" else name)
        normals = None
        if name == "opposed":  # vertex normals that oppose the face normal (+z for the fan): the frame takes the face's
            normals = np.tile(np.array([0.1, -0.2, -1.0]), (len(verts), 1))
        atlas = T.build(verts, tris, density)
        tex = T.texels(verts, normals, tris, atlas)
    own = tex["owner"].reshape(-1) >= 0
    tn, pts = tex["normals"].reshape(-1, 3), tex["points"].reshape(-1, 3)
    g = -tn if name == "opposed" else tn
    rng = np.random.default_rng(SCENES.index(name))
    values = np.zeros((len(own), 8), np.float32)
    values[:, :5] = rng.random((len(own), 5))
    # a mean of unit normals is shorter than 1: scale the field as a bake would leave it
    values[:, 5:] = np.where(own[:, None], (0.6 + 0.4 * rng.random((len(own), 1))) * normal_field(pts, g), 0.0)
    idx = np.nonzero(own)[0]
    if len(idx) > 8:  # an unseen texel's zero, and values no encode can use
        values[idx[3], 5:] = 0.0
        values[idx[5], 6] = np.nan
        values[idx[7], 5] = np.inf
    want = texture_normals(tex["owner"], tn, tris, atlas["uvs"], verts, values, 5)
    return dict(verts=verts, tris=tris, normals=normals, density=density, atlas=atlas, tex=tex, values=values, want=want)


def random_textures(height, width, seed):
    """-> (base, orm) (height, width, 3) uint8"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (height, width, 3), dtype=np.uint8), rng.integers(0, 256, (height, width, 3), dtype=np.uint8)


VIEWS = 2  # of sphere_case's five


@functools.lru_cache(maxsize=None)
def sphere_visibility(ss):
    c = T.sphere_case()
    return MV.visibility(c["verts"], c["tris"], c["w2c"][:VIEWS], c["fx"], c["fy"], c["cx"], c["cy"], c["H"], c["W"], ss)


@functools.lru_cache(maxsize=None)
def sphere_gbuffer(ss, smooth=True, with_normal_map=True, srgb=True):
    """the restatement of the G-buffer test's input: the icosphere with random base and ORM textures and the scene's own normal
    map, from the first VIEWS views of sphere_case"""
    c, s = T.sphere_case(), scene("sphere")
    H, W = c["atlas"]["height"], c["atlas"]["width"]
    base, orm = random_textures(H, W, 21)
    nm = s["want"]["bytes"].reshape(H, W, 3) if with_normal_map else None
    return gbuffer_textured(c["verts"], c["tris"], c["atlas"]["uvs"], c["w2c"][:VIEWS], c["fx"], c["fy"], c["cx"], c["cy"], c["H"], c["W"], ss,
                            sphere_visibility(ss), c["normals"] if smooth else None, base, srgb, orm, nm)
