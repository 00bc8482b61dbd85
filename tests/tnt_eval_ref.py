"""Numpy restatement of the Tanks and Temples evaluation contract: the oracle of the kernels of
csrc/tnt_eval.hip and of gs2m_tnt_eval.py's driver.  It restates Open3D's behaviour as the contract reads it (Open3D itself
is not installed: unpinned); the score stage is pinned to the reference's own get_f1_score_histo2
(tests/golden/ref_tnt_eval.npz).  Nearest neighbours by brute force; scipy's cKDTree only on request, for random doubles
where ties cannot occur.  The voxel sums are np.add.at in input order; the ICP sums are numpy's (or math.fsum with
`exact=True`: the summation-order floor of §11).  Nothing here imports the product."""
import math

import numpy as np

from dtu_eval_ref import fixed_order_sum

AXES = {"X": (1, 2, 0), "Y": (0, 2, 1), "Z": (0, 1, 2)}
MAX_POINT_NUMBER = 4e6


def mesh_points(vertices, triangles):
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(triangles, np.int64).reshape(-1, 3)
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("a triangle names a vertex out of range")
    c = ((v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]) / 3.0
    return np.concatenate([v, c])


def transform(points, T):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(4, 4)
    if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError("the last row must be (0, 0, 0, 1)")
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def crop_flags(points, volume):
    """volume: dict(orthogonal_axis, axis_min, axis_max, bounding_polygon (m, 3))"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    u, v, w = AXES[str(volume["orthogonal_axis"]).upper()]
    P = np.asarray(volume["bounding_polygon"], np.float64).reshape(-1, 3)
    m = len(P)
    odd = np.zeros(len(p), bool)
    pu, pv = p[:, u], p[:, v]
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(m):
            j = (i + 1) % m
            cross = ((P[i, v] < pv) & (P[j, v] >= pv)) | ((P[j, v] < pv) & (P[i, v] >= pv))
            node = P[i, u] + ((pv - P[i, v]) / (P[j, v] - P[i, v])) * (P[j, u] - P[i, u])
            odd ^= cross & (node < pu)
    return odd & (p[:, w] >= volume["axis_min"]) & (p[:, w] <= volume["axis_max"])


def crop(points, volume):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    return p[crop_flags(p, volume)]


def voxel_downsample(points, s):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if len(p) == 0:
        return p.copy()
    lo = p.min(0) - s * 0.5
    idx = np.floor((p - lo) / s)
    if not (idx.max() < 2 ** 21):
        raise ValueError("a voxel index reaches 2^21")
    idx = idx.astype(np.int64)
    key = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    uniq, inv = np.unique(key, return_inverse=True)  # ascending (ix, iy, iz)
    sums = np.zeros((len(uniq), 3))
    np.add.at(sums, inv.reshape(-1), p)  # unbuffered: one addition per point, in input order
    cnt = np.bincount(inv.reshape(-1), minlength=len(uniq)).astype(np.float64)
    return sums / cnt[:, None]


def uniform_downsample(points, limit=MAX_POINT_NUMBER):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if len(p) > limit:
        return p[::int(round(len(p) / float(limit)))]
    return p


def nearest(queries, targets, max_dist, kdtree=False):
    """-> (index int64, dist): the lowest index among the targets at the smallest (dx dx + dy dy) + dz dz and its square root
    where that is < max_dist; else -1, +inf.  kdtree: candidates from scipy's cKDTree (random doubles only: no ties), the
    distance still evaluated as written."""
    q = np.asarray(queries, np.float64).reshape(-1, 3)
    t = np.asarray(targets, np.float64).reshape(-1, 3)
    idx = np.full(len(q), -1, np.int64)
    dist = np.full(len(q), np.inf)
    if len(t) == 0 or len(q) == 0:
        return idx, dist
    if kdtree:
        from scipy.spatial import cKDTree
        _, cand = cKDTree(t).query(q, k=min(4, len(t)))
        cand = cand.reshape(len(q), -1)
        d = q[:, None, :] - t[cand]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        best = d2.min(1)
        # the lowest index among the candidates at the minimum
        j = np.where(d2 == best[:, None], cand, np.iinfo(np.int64).max).min(1)
    else:
        best = np.empty(len(q))
        j = np.empty(len(q), np.int64)
        step = max(1, 4_000_000 // len(t))
        for a in range(0, len(q), step):
            d = q[a:a + step, None, :] - t[None]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            j[a:a + step] = d2.argmin(1)  # the first minimum: the lowest index
            best[a:a + step] = d2.min(1)
    dd = np.sqrt(best)
    ok = dd < max_dist
    idx[ok] = j[ok]
    dist[ok] = dd[ok]
    return idx, dist


def _sum(a, exact):
    a = np.asarray(a, np.float64)
    if exact:
        return np.array([math.fsum(a[:, k]) for k in range(a.shape[1])]) if a.ndim == 2 else math.fsum(a)
    return a.sum(0)


def icp_moments(source, targets, index, exact=False):
    """-> dict(c, sum_d2, mx, my, sigma (3, 3), sx2, terms): the moments over the pairs with index >= 0.  terms: the sum of the
    absolute values of each sum's terms, in the order [d2, mx (3), my (3), sigma (9), sx2] before any division (the scale
    of a summation-order allowance)."""
    x = np.asarray(source, np.float64).reshape(-1, 3)
    t = np.asarray(targets, np.float64).reshape(-1, 3)
    ok = np.asarray(index) >= 0
    c = int(ok.sum())
    if c == 0:
        return {"c": 0, "sum_d2": 0.0, "mx": np.zeros(3), "my": np.zeros(3), "sigma": np.zeros((3, 3)), "sx2": 0.0, "terms": np.zeros(17)}
    x, y = x[ok], t[np.asarray(index)[ok]]
    d = x - y
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    mx, my = _sum(x, exact) / c, _sum(y, exact) / c
    a, b = x - mx, y - my
    prod = b[:, :, None] * a[:, None, :]  # rows y, columns x
    sigma = _sum(prod.reshape(-1, 9), exact).reshape(3, 3) / c
    n2 = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    sx2 = float(_sum(n2, exact)) / c
    terms = np.concatenate([[d2.sum()], np.abs(x).sum(0), np.abs(y).sum(0), np.abs(prod).reshape(-1, 9).sum(0), [n2.sum()]])
    return {"c": c, "sum_d2": float(_sum(d2, exact)), "mx": mx, "my": my, "sigma": sigma, "sx2": sx2, "terms": terms}


def icp_moments_fixed_order(source, targets, index):
    """gs2m_tnt_icp_moments as the device and its host part compute it, to the bit.  -> (count, out (17,)): out = [sum_d2,
    mx (3), my (3), sigma (9, rows y, columns x), sx2].  Two passes of `fixed_order_sum` over the pairs with index >= 0: first
    d^2 = (dx dx + dy dy) + dz dz, x and y, whose sums the host divides by the count; then the products about those means,
    divided by the count as well.  Every output is 0 when no pair has index >= 0."""
    x = np.asarray(source, np.float64).reshape(-1, 3)
    t = np.asarray(targets, np.float64).reshape(-1, 3)
    index = np.asarray(index, np.int64).reshape(-1)
    ok = index >= 0
    c = int(ok.sum())
    out = np.zeros(17)
    if c == 0:
        return 0, out
    y = t[np.where(ok, index, 0)]
    keep = ok[:, None]
    d = x - y
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    s0 = fixed_order_sum(np.where(keep, np.concatenate([d2[:, None], x, y], 1), 0.0))
    cd = np.float64(c)
    out[0] = s0[0]
    out[1:7] = s0[1:7] / cd
    a, b = x - out[1:4], y - out[4:7]
    prod = (b[:, :, None] * a[:, None, :]).reshape(-1, 9)
    n2 = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    out[7:17] = fixed_order_sum(np.where(keep, np.concatenate([prod, n2[:, None]], 1), 0.0)) / cd
    return c, out


def umeyama_update(m):
    """Item 8: the similarity (4 x 4) from the moments: U D V^T = svd(Sigma), S = diag(1, 1, sign(det U det V)), R = U S V^T,
    scale = trace(D S) / sx2, t = my - scale R mx."""
    U, D, Vt = np.linalg.svd(m["sigma"])
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    scale = float((D * np.diag(S)).sum()) / m["sx2"]
    T = np.eye(4)
    T[:3, :3] = scale * R
    T[:3, 3] = m["my"] - scale * (R @ m["mx"])
    return T


def _evaluate(src, tgt, thr, kdtree, exact):
    idx, _ = nearest(src, tgt, thr, kdtree)
    m = icp_moments(src, tgt, idx, exact)
    c = m["c"]
    fitness = c / len(src) if len(src) and c else 0.0
    rmse = math.sqrt(m["sum_d2"] / c) if c else 0.0
    return m, fitness, rmse


def icp(source, target, thr, max_itr, kdtree=False, exact=False):
    """Item 9.  -> (T, fitness, rmse, iterations)"""
    src = np.asarray(source, np.float64).reshape(-1, 3).copy()
    tgt = np.asarray(target, np.float64).reshape(-1, 3)
    T = np.eye(4)
    m, fitness, rmse = _evaluate(src, tgt, thr, kdtree, exact)
    it = 0
    for _ in range(max_itr):
        if m["c"] < 3:
            break
        upd = umeyama_update(m)
        T = upd @ T
        src = transform(src, upd)
        prev = (fitness, rmse)
        m, fitness, rmse = _evaluate(src, tgt, thr, kdtree, exact)
        it += 1
        if abs(fitness - prev[0]) < 1e-6 and abs(rmse - prev[1]) < 1e-6:
            break
    return T, fitness, rmse, it


def register(source, gt, T0, volume, tau, kdtree=False, exact=False, limit=MAX_POINT_NUMBER):
    """Item 10.  -> (T, [dict(iterations, fitness, rmse, n_source, n_target) per stage])"""
    src0 = np.asarray(source, np.float64).reshape(-1, 3)
    gt_crop = crop(gt, volume)
    T = np.asarray(T0, np.float64).reshape(4, 4).copy()
    stages = []
    for kind, vox, thr in (("voxel", tau, 80 * tau), ("voxel", tau / 2.0, 20 * tau), ("uniform", None, 2 * tau)):
        s = crop(transform(src0, T), volume)
        if kind == "voxel":
            s, t = voxel_downsample(s, vox), voxel_downsample(gt_crop, vox)
        else:
            s, t = uniform_downsample(s, limit), uniform_downsample(gt_crop, limit)
        Ti, fit, rmse, it = icp(s, t, thr, 20, kdtree, exact)
        T = Ti @ T
        stages.append({"iterations": it, "fitness": fit, "rmse": rmse, "n_source": len(s), "n_target": len(t)})
    return T, stages


def fit_similarity(x, y):
    """Item 8 fitted to the pairs x[i] -> y[i]."""
    idx = np.arange(len(x))
    return umeyama_update(icp_moments(x, y, idx))


def align_trajectories(est, gt, gt_trans, dist=0.2, min_pairs=6, max_rounds=20):
    """Item 11: est, gt (n, 4, 4) poses; gt's centres moved by gt_trans; the deterministic trimmed fit."""
    x = np.asarray(est, np.float64)[:, :3, 3]
    y = transform(np.asarray(gt, np.float64)[:, :3, 3], gt_trans)
    if len(x) != len(y):
        raise ValueError("the trajectories differ in length")
    keep = np.ones(len(x), bool)
    T = None
    for _ in range(max_rounds):
        if keep.sum() < min_pairs:
            raise ValueError("fewer than 6 camera pairs agree")
        T = fit_similarity(x[keep], y[keep])
        new = np.linalg.norm(transform(x, T) - y, axis=1) < dist
        if np.array_equal(new, keep):
            break
        keep = new
    return T


def histogram(dist, edges):
    """numpy's rule for given edges: right-open bins, the last one closed"""
    return np.histogram(np.asarray(dist, np.float64), np.asarray(edges, np.float64))[0]


def score(distance1, distance2, tau, stretch=5):
    """Item 12 from the two distance arrays (+inf where >= stretch tau).  -> precision, recall, fscore, edges, cum_source,
    edges, cum_target as get_f1_score_histo2 returns them."""
    d1, d2 = np.asarray(distance1, np.float64), np.asarray(distance2, np.float64)
    if len(d1) == 0 or len(d2) == 0:
        z = np.array([0])
        return 0, 0, 0, z, z, z, z
    recall = float((d2 < tau).sum()) / float(len(d2))
    precision = float((d1 < tau).sum()) / float(len(d1))
    fscore = 2 * recall * precision / (recall + precision) if recall + precision != 0 else 0.0
    edges = np.arange(0, tau * stretch, tau / 100)
    cum1 = np.cumsum(histogram(d1, edges)).astype(float) / len(d1)
    cum2 = np.cumsum(histogram(d2, edges)).astype(float) / len(d2)
    return precision, recall, fscore, edges, cum1, edges, cum2


def evaluate(source, gt, T, volume, tau, kdtree=False):
    """Item 12.  -> dict(precision, recall, fscore, edges, cum_source, cum_target, distance1, distance2, n_source, n_target)"""
    s = voxel_downsample(crop(transform(source, T), volume), tau / 2.0)
    t = voxel_downsample(crop(gt, volume), tau / 2.0)
    _, d1 = nearest(s, t, 5 * tau, kdtree)
    _, d2 = nearest(t, s, 5 * tau, kdtree)
    p, r, f, e, c1, _, c2 = score(d1, d2, tau)
    return {"precision": p, "recall": r, "fscore": f, "edges": e, "cum_source": c1, "cum_target": c2, "distance1": d1,
            "distance2": d2, "n_source": len(s), "n_target": len(t)}
