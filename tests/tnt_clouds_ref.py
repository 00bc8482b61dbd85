"""The float64 arbiter of the Tanks and Temples clouds' normals (csrc/tnt_clouds.hip; include/gs2m_tnt.h states the rules) and
the test clouds.  Plain definitions in numpy: the neighbour set is the first k of lexsort((index, d2)) over the whole cloud,
the normal numpy.linalg.eigh's eigenvector of the smallest eigenvalue of the covariance about the mean, the colours
matplotlib's hot_r itself.  Open3D, which the reference calls, is not part of this stack."""
import functools

import numpy as np

import tnt_eval_ref as R

GAP_MIN = 1e-3        # normals are compared where (l1 - l0) / l2 is at least this
EXCLUDED_MAX = 0.01   # and at most this fraction of a cloud may lie under it
SURFACE_SEED = 0
SIZES = (1, 2, 3, 19, 20, 21, 64, 65, 257, 5000)


def knn_brute(p, k):
    """(n, k) int64: per point the min(k, n) points with the smallest (d2, index), d2 = (dx dx + dy dy) + dz dz in float64 as
    written; -1 beyond n.  Rows are cut at their k-th smallest d2 first, every tie included, then sorted with lexsort."""
    p = np.asarray(p, np.float64)
    n, m = len(p), min(k, len(p))
    out = np.full((n, k), -1, np.int64)
    for a in range(0, n, 1000):
        q = p[a:a + 1000]
        dx, dy, dz = (q[:, None, c] - p[None, :, c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        kth = np.partition(d2, m - 1, axis=1)[:, m - 1]
        for r in range(len(q)):
            cand = np.nonzero(d2[r] <= kth[r])[0]
            out[a + r, :m] = cand[np.lexsort((cand, d2[r, cand]))][:m]
    return out


def normals_ref(p, index):
    """-> (normals (n, 3) with n . z >= 0, eigenvalues (n, 3) ascending) of the neighbour sets `index` (n, k), all >= 0"""
    q = np.asarray(p, np.float64)[index]
    a = q - q.mean(axis=1, keepdims=True)
    w, v = np.linalg.eigh(np.einsum("nki,nkj->nij", a, a) / index.shape[1])
    nrm = v[:, :, 0]
    return nrm * np.where(nrm[:, 2:3] < 0, -1.0, 1.0), w


def gap(w):
    return (w[:, 1] - w[:, 0]) / w[:, 2]


def sine_cross(a, b):
    return np.linalg.norm(np.cross(a, b), axis=1)


def sign_rule_holds(n):
    """n . (0, 0, 1) >= 0, and where it is exactly 0 the first non-zero component is positive"""
    first = np.where(n[:, 0] != 0, n[:, 0], n[:, 1])
    return bool(np.all((n[:, 2] > 0) | ((n[:, 2] == 0) & (first > 0)) | (np.abs(n).sum(1) == 0)))


@functools.lru_cache(maxsize=None)
def surface(seed=SURFACE_SEED):
    """A jittered height field (120 x 120 samples of a bumpy sheet, each moved by up to 0.4 spacings in the sheet and 0.1
    across it), voxel-downsampled at 1.2 spacings by the restatement of the evaluator's own downsample: the workload's shape.
    -> (n, 3) float64, read-only, n > 5000."""
    raw, s = surface_raw(seed)
    p = R.voxel_downsample(raw, s)
    assert len(p) > SIZES[-1]
    p.setflags(write=False)
    return p


def surface_raw(seed=SURFACE_SEED):
    """the samples `surface` downsamples, and the voxel edge: for the GPU test, which runs the evaluator's own downsample"""
    rng = np.random.default_rng(seed)
    h = 1.0 / 120
    u, v = np.meshgrid(np.arange(120) * h, np.arange(120) * h, indexing="ij")
    u = u + rng.uniform(-0.4, 0.4, u.shape) * h
    v = v + rng.uniform(-0.4, 0.4, v.shape) * h
    z = 0.15 * np.sin(5 * u) * np.cos(4 * v) + 0.05 * np.sin(11 * u + 3 * v) + rng.uniform(-0.1, 0.1, u.shape) * h
    return np.stack([u, v, z], -1).reshape(-1, 3), 1.2 * h


@functools.lru_cache(maxsize=None)
def surface_knn(n, k=32):
    """the arbiter's neighbour sets of the first n surface points, computed once: k = 32 holds k = 1 and 20 as its prefixes"""
    idx = knn_brute(surface()[:n], k)
    idx.setflags(write=False)
    return idx


def lattice(nx=8, ny=8, nz=8):
    """integer coordinates, exact in float64: many equal distances, and d2 is exact whatever the compiler does"""
    return np.stack(np.meshgrid(np.arange(float(nx)), np.arange(float(ny)), np.arange(float(nz)), indexing="ij"), -1).reshape(-1, 3)


def hot_r_bytes(d, m):
    """round(hot_r(min(d, m) / m)[:3] * 255) as uint8: matplotlib's own lookup, Open3D's rounding"""
    import matplotlib
    c = matplotlib.colormaps["hot_r"](np.minimum(np.asarray(d, np.float64), m) / m)[:, :3]
    return np.rint(c * 255.0).astype(np.uint8)


def color_probe(m, seed=0):
    """0, the 255 interior bin edges of [0, m] with the doubles on either side, m, 2 m, +inf, and random distances"""
    e = np.arange(1, 256) / 256.0 * m
    rng = np.random.default_rng(seed)
    return np.concatenate([[0.0, m, 2 * m, np.inf], e, np.nextafter(e, 0), np.nextafter(e, np.inf), rng.uniform(0, 1.5 * m, 3000)])
