"""The mask culling of the DTU evaluation restated on the CPU (DESIGN.md §10 "Mask culling"), and the synthetic inputs the
tests of it share.  The dilation is scipy.ndimage.binary_dilation with the disk as its structure and the lookup is torch's
grid_sample on the CPU (nearest, zero padding, align_corners): the library functions the reference's script calls.

The vertex step is fp32 on the GPU and in the reference, so a pixel position that lies within rounding of a pixel's edge, or
of the frame, may fall either way.  `cull_flags` therefore also evaluates the position in fp64 and marks a (vertex, view)
pair undecided when the four positions (px +- e, py +- e) do not agree on the view's verdict, or when the vertex lies within
1e-4 of the camera plane (|c_2 + 1e-6| < 1e-4).  A vertex is undecided when any of its views is; every other vertex has to
match exactly.  E_PX is four times the largest fp32 error measured on these inputs, rounded up to a power of two
(`position_error`; tests/test_dtu_cull.py holds E_PX to that rule and DESIGN.md §10 records the figures)."""
import functools

import numpy as np
import torch
from scipy import ndimage

E_PX = 2.0 ** -10  # pixels; see position_error and test_dtu_cull.py::test_e_follows_the_measured_error
UNDECIDED_CAP = 0.002  # of the vertices of an input


def disk(r):
    a = np.arange(-r, r + 1)
    X, Y = np.meshgrid(a, a)
    return (X ** 2 + Y ** 2) <= r ** 2


def dilate(mask, r):
    """(H, W) any dtype, non-zero = foreground -> (H, W) bool"""
    return ndimage.binary_dilation(np.asarray(mask) != 0, structure=disk(r))


def dilate_brute(mask, r):
    """the definition, pixel by pixel (small masks only)"""
    m = np.asarray(mask) != 0
    H, W = m.shape
    out = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    if dx * dx + dy * dy <= r * r and 0 <= y + dy < H and 0 <= x + dx < W and m[y + dy, x + dx]:
                        out[y, x] = True
    return out


def pack_rows(dil):
    """(n, H, W) bool -> (n, H, ceil(W / 64)) uint64, bit x & 63 of word x >> 6, padding bits 0"""
    n, H, W = dil.shape
    pad = np.zeros((n, H, (W + 63) // 64 * 64), np.uint64)
    pad[:, :, :W] = dil
    return (pad.reshape(n, H, -1, 64) << np.arange(64, dtype=np.uint64)).sum(axis=3, dtype=np.uint64)


def sample_nearest(dil, nx, ny):
    """dil (H, W) bool, normalised coordinates nx, ny (n,) float32 -> (n,) float32 through torch's grid_sample on the CPU"""
    img = torch.from_numpy(np.ascontiguousarray(dil, dtype=np.float32))[None, None]
    grid = torch.from_numpy(np.stack([np.asarray(nx, np.float32), np.asarray(ny, np.float32)], axis=-1))[None, None]
    return torch.nn.functional.grid_sample(img, grid, mode="nearest", padding_mode="zeros", align_corners=True)[0, 0, 0].numpy()


def sample_nearest_np(dil, nx, ny):
    """the same lookup written out: ix = rint(((nx + 1) / 2) (W - 1)) (half to even) in the arrays' own precision, 0 outside"""
    H, W = dil.shape
    one = nx.dtype.type(1)
    with np.errstate(invalid="ignore"):
        fx, fy = np.rint(((nx + one) / 2) * (W - 1)), np.rint(((ny + one) / 2) * (H - 1))
        inside = (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
    ix, iy = np.where(inside, fx, 0).astype(np.int64), np.where(inside, fy, 0).astype(np.int64)
    return np.where(inside, dil[iy, ix], False)


def project(vertices, M, dtype):
    """The contract's pixel position of every vertex in one view, evaluated as written in `dtype` (the vertex is cast to
    float32 first, M is a float32 matrix).  -> px, py, c2 + 1e-6"""
    v = np.asarray(vertices).astype(np.float32).astype(dtype)
    m = np.asarray(M, np.float32).astype(dtype)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        c = [((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3)]
        d = c[2] + dtype(1e-6)
        return c[0] / d, c[1] / d, d


def normalise(px, py, Wn, Hn):
    t = px.dtype.type
    with np.errstate(all="ignore"):
        nx, ny = (px / t(Wn - 1) - t(0.5)) * t(2), (py / t(Hn - 1) - t(0.5)) * t(2)
        return nx, ny, (nx > -1) & (nx < 1) & (ny > -1) & (ny < 1)


def _verdict64(px, py, dil, Wn, Hn):
    nx, ny, valid = normalise(px, py, Wn, Hn)
    return sample_nearest_np(dil, nx, ny) | ~valid


def cull_flags(vertices, M, dilated, image_size, e=E_PX):
    """vertices (V, 3), M (n, 4, 4) float32, dilated (n, H, W) bool, image_size (Wn, Hn).
    -> keep (V,) bool as the reference's fp32 steps give it, undecided (V,) bool"""
    Wn, Hn = image_size
    V = len(vertices)
    keep, undecided = np.ones(V, bool), np.zeros(V, bool)
    for k in range(len(M)):
        px, py, _ = project(vertices, M[k], np.float32)
        nx, ny, valid = normalise(px, py, Wn, Hn)
        s = sample_nearest(dilated[k], nx, ny) if V else np.zeros(0, np.float32)
        keep &= (s + (1.0 - valid.astype(np.float32))) > 0
        qx, qy, d = project(vertices, M[k], np.float64)
        corners = [_verdict64(qx + sx * e, qy + sy * e, dilated[k], Wn, Hn) for sx in (-1, 1) for sy in (-1, 1)]
        with np.errstate(invalid="ignore"):
            undecided |= (corners[0] != corners[1]) | (corners[0] != corners[2]) | (corners[0] != corners[3]) | (np.abs(d) < 1e-4)
    return keep, undecided


def position_error(vertices, M, image_size):
    """The largest |fp32 position - fp64 position| in pixels over the (vertex, view) pairs that the contract's rounding can
    matter for: at least 1e-4 off the camera plane and, in fp64, inside the frame widened by one pixel.  (Further out a
    position is thousands of fp32 roundings away from anything that changes the verdict.)"""
    Wn, Hn = image_size
    worst = 0.0
    for k in range(len(M)):
        px, py, _ = project(vertices, M[k], np.float32)
        qx, qy, d = project(vertices, M[k], np.float64)
        with np.errstate(invalid="ignore"):
            sel = (np.abs(d) >= 1e-4) & (qx >= -1) & (qx <= Wn) & (qy >= -1) & (qy <= Hn)
        if sel.any():
            worst = max(worst, float(np.abs(px[sel] - qx[sel]).max()), float(np.abs(py[sel] - qy[sel]).max()))
    return worst


def e_for(measured):
    """four times the measured error, rounded up to a power of two"""
    return 2.0 ** int(np.ceil(np.log2(4.0 * measured)))


def cull_mesh(vertices, triangles, keep):
    """-> the kept vertices in order (referenced or not), the faces whose three vertices are kept, in order, renumbered"""
    keep = np.asarray(keep, bool)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    new_id = np.cumsum(keep) - 1
    return np.asarray(vertices)[keep], new_id[t[keep[t].all(axis=1)]].astype(np.int32)


# ---- synthetic inputs ------------------------------------------------------------------------------------------------------

IMAGE_SIZE = (200, 150)  # (Wn, Hn) of the ring cameras
FOCAL = 180.0
RING = 4.0               # the cameras' distance from the object's centre, in units of the scale
ELLIPSE = (50.0, 40.0)   # the silhouette's half axes in pixels of the (Wn, Hn) frame


def ring_cameras(n_views, scale=1.3, shift=(0.1, -0.05, 0.02), image_size=IMAGE_SIZE):
    """n cameras on a ring around `shift`, looking at it, with the field of view of FOCAL at IMAGE_SIZE whatever the frame.
    -> (world_mats, scale_mats), float32 (4, 4) each, as cameras.npz holds them: the mesh's coordinates x are world
    coordinates scale * x + shift"""
    Wn, Hn = image_size
    f = FOCAL * Wn / IMAGE_SIZE[0]
    K = np.array([[f, 0, (Wn - 1) / 2], [0, f, (Hn - 1) / 2], [0, 0, 1.0]])
    S = np.eye(4)
    S[0, 0] = S[1, 1] = S[2, 2] = scale
    S[:3, 3] = shift
    world, scales = [], []
    for k in range(n_views):
        a = 2 * np.pi * (k + 0.25) / max(n_views, 1)
        centre = np.asarray(shift) + RING * scale * np.array([np.sin(a), 0.0, -np.cos(a)])
        zc = (np.asarray(shift) - centre) / np.linalg.norm(np.asarray(shift) - centre)
        xc = np.cross([0.0, 1.0, 0.0], zc)
        xc /= np.linalg.norm(xc)
        R = np.stack([xc, np.cross(zc, xc), zc])
        Wm = np.eye(4)
        Wm[:3, :3], Wm[:3, 3] = K @ R, K @ (-R @ centre)
        world.append(Wm.astype(np.float32))
        scales.append(S.astype(np.float32))
    return world, scales


VARIANTS = (1.0, 0.9, 1.1)  # view k's silhouette is the ellipse scaled by VARIANTS[k % 3]: neighbouring views differ


@functools.lru_cache(maxsize=None)
def ellipse_mask(H, W, variant=0):
    """the silhouette, drawn for a mask of any size in the proportions of the (Wn, Hn) frame; values 255"""
    Wn, Hn = IMAGE_SIZE
    y, x = np.mgrid[0:H, 0:W]
    u, v = x * (Wn - 1) / max(W - 1, 1) - (Wn - 1) / 2, y * (Hn - 1) / max(H - 1, 1) - (Hn - 1) / 2
    f = VARIANTS[variant]
    return (((u / (f * ELLIPSE[0])) ** 2 + (v / (f * ELLIPSE[1])) ** 2) <= 1).astype(np.uint8) * 255


@functools.lru_cache(maxsize=None)
def _dilated_ellipse(H, W, variant, radius):
    return dilate(ellipse_mask(H, W, variant), radius)


def shell_points(n, M0, radius, mask_hw, seed):
    """n points in the mesh's coordinates around the origin, float32 values in an fp64 array: most of them deep inside every
    view's dilated silhouette, one in ten on a wider shell that crosses its rim, and a few each of: points beyond the ring
    (behind some cameras), points far off the ring's plane (outside the frame), points placed on the dilated silhouette's
    rim in view 0, and one NaN vertex"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    kind = rng.random(n)
    rad = np.where(kind < 0.8, rng.uniform(0.2, 0.5, n), rng.uniform(0.7, 1.3, n))
    p = u * rad[:, None]
    far = (kind >= 0.9) & (kind < 0.93)
    p[far] = u[far] * rng.uniform(5.0, 7.0, (int(far.sum()), 1))
    off = (kind >= 0.93) & (kind < 0.96)
    p[off] = u[off] * 0.5 + np.array([0.0, 1.0, 0.0]) * np.where(rng.random(int(off.sum())) < 0.5, -1.0, 1.0)[:, None] * rng.uniform(1.6, 2.3, (int(off.sum()), 1))
    rim = kind >= 0.96
    if rim.any():  # pixels near the ellipse grown by the radius, pushed back along view 0's rays to the object's depth
        m = int(rim.sum())
        th = rng.uniform(0, 2 * np.pi, m)
        Wn, Hn = IMAGE_SIZE
        grow = radius * (Wn - 1) / max(mask_hw[1] - 1, 1)
        px = (Wn - 1) / 2 + (ELLIPSE[0] + grow) * np.cos(th) + rng.uniform(-1.5, 1.5, m)
        py = (Hn - 1) / 2 + (ELLIPSE[1] + grow) * np.sin(th) + rng.uniform(-1.5, 1.5, m)
        # M0 x = depth (px, py, 1): solve for x at depths around the ring's
        depth = rng.uniform(0.9, 1.1, m) * RING
        A, b = M0[:3, :3].astype(np.float64), M0[:3, 3].astype(np.float64)
        rhs = np.stack([px * depth, py * depth, depth], axis=1) - b
        p[rim] = np.linalg.solve(A, rhs.T).T
    p = p.astype(np.float32).astype(np.float64)
    if n >= 3:
        p[n // 3, 0] = np.nan
    return p


VERTEX_CASES = [(views, n) for views in (1, 3, 49) for n in (0, 1, 63, 64, 65, 1000, 100000)]


@functools.lru_cache(maxsize=None)
def vertex_case(n_views, n_verts, mask_hw=(150, 200), radius=24):
    """One input of the vertex-flag tests with its restatement, computed once: dict(M, masks, dilated, vertices, keep,
    undecided, image_size, radius).  The arrays are shared: leave them unchanged."""
    import gs2m_dtu_eval as E
    world, scales = ring_cameras(n_views)
    M = E.view_matrices(world, scales)
    masks = np.stack([ellipse_mask(*mask_hw, k % 3) for k in range(n_views)]) if n_views else np.zeros((0,) + mask_hw, np.uint8)
    dilated = np.stack([_dilated_ellipse(*mask_hw, k % 3, radius) for k in range(n_views)]) if n_views else np.zeros((0,) + mask_hw, bool)
    verts = shell_points(n_verts, M[0], radius, mask_hw, seed=1000 * n_views + n_verts % 997)
    keep, undecided = cull_flags(verts, M, dilated, IMAGE_SIZE)
    return {"M": M, "masks": masks, "dilated": dilated, "vertices": verts, "keep": keep, "undecided": undecided,
            "image_size": IMAGE_SIZE, "radius": radius}


def small_mask_case():
    """a 75 x 100 mask under the (200, 150) normaliser, dilated by 12"""
    return vertex_case(3, 1000, (75, 100), 12)


def random_mesh(n_verts, n_tris, seed):
    """faces over n_verts vertices that share vertices, leave some unreferenced and hold one degenerate face"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, max(n_verts - n_verts // 10, 1), (n_tris, 3)).astype(np.int32)  # the last tenth stays unreferenced
    if n_tris > 2:
        t[n_tris // 2, 1] = t[n_tris // 2, 0]
    return t


def decided_mesh(n_views, n_verts, n_tris, seed):
    """vertices of vertex_case with the undecided ones taken out, random faces over them, and the restatement's culled mesh"""
    c = vertex_case(n_views, n_verts)
    v = c["vertices"][~c["undecided"]]
    keep = c["keep"][~c["undecided"]]
    t = random_mesh(len(v), n_tris, seed)
    k = np.nonzero(keep)[0]
    t[n_tris // 2] = [k[0], k[0], k[1]]  # the degenerate face names kept vertices: it has to survive
    cv, ct = cull_mesh(v, t, keep)
    return c, v, t, cv, ct


def sphere_mesh(radius, n_lat=40, n_lon=50):
    """a latitude-longitude sphere without its poles: float32 values in an fp64 array, int32 faces"""
    th = np.pi * (np.arange(n_lat) + 0.5) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    T, P = np.meshgrid(th, ph, indexing="ij")
    v = radius * np.stack([np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)], axis=-1).reshape(-1, 3)
    idx = np.arange(n_lat * n_lon).reshape(n_lat, n_lon)
    a, b, c, d = idx[:-1], np.roll(idx, -1, 1)[:-1], idx[1:], np.roll(idx, -1, 1)[1:]
    t = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)])
    return v.astype(np.float32).astype(np.float64), t.astype(np.int32)


CLI_IMAGE_SIZE = (1600, 1200)  # the normaliser the command line uses, as the reference hard-codes it
CLI_SCALE, CLI_SHIFT, CLI_VIEWS, CLI_SPHERE = 20.0, (10.0, -20.0, 300.0), 5, 1.45


@functools.lru_cache(maxsize=None)
def cli_case():
    """the command-line test's scan: five ring cameras of a 1600 x 1200 frame in millimetres, 150 x 200 masks, a sphere mesh"""
    import gs2m_dtu_eval as E
    world, scales = ring_cameras(CLI_VIEWS, CLI_SCALE, CLI_SHIFT, CLI_IMAGE_SIZE)
    M = E.view_matrices(world, scales)
    masks = np.stack([ellipse_mask(150, 200, k % 3) for k in range(CLI_VIEWS)])
    dilated = np.stack([_dilated_ellipse(150, 200, k % 3, 24) for k in range(CLI_VIEWS)])
    v, t = sphere_mesh(CLI_SPHERE)
    keep, undecided = cull_flags(v, M, dilated, CLI_IMAGE_SIZE)
    return {"world": world, "scales": scales, "M": M, "masks": masks, "dilated": dilated, "vertices": v, "triangles": t,
            "keep": keep, "undecided": undecided, "image_size": CLI_IMAGE_SIZE, "radius": 24}


def point_kinds(c):
    """-> (vertices behind some camera (c_2 + 1e-6 < 0), vertices outside some view's frame (not valid)), from the fp32 steps"""
    behind, outside = np.zeros(len(c["vertices"]), bool), np.zeros(len(c["vertices"]), bool)
    for k in range(len(c["M"])):
        px, py, d = project(c["vertices"], c["M"][k], np.float32)
        with np.errstate(invalid="ignore"):
            behind |= d < 0
        outside |= ~normalise(px, py, *c["image_size"])[2] & ~np.isnan(px)
    return int(behind.sum()), int(outside.sum())


def all_inputs():
    """every (vertices, M, dilated, image_size) the GPU tests hold to the restatement"""
    return [vertex_case(v, n) for v, n in VERTEX_CASES] + [small_mask_case(), cli_case()]
