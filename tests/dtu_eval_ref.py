"""numpy / scikit-learn restatement of the DTU evaluation contract, the oracle of tests/test_dtu_eval*.py.
tests/golden/ref_dtu_eval.npz pins it to the reference's own evaluator; the HIP kernels are held to it bit for bit."""
import numpy as np
import sklearn.neighbors as skln


def world_transform(vertices, scale_mat):
    S = np.asarray(scale_mat, np.float32).reshape(4, 4)
    return np.asarray(vertices, np.float64) * np.float64(S[0, 0]) + S[:3, 3].astype(np.float64)[None]


def _norm(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def sample_mesh(vertices, triangles, thresh):
    """-> the cloud: every vertex, then the kept candidates of every triangle (row major over (i, j)) in triangle order."""
    V = np.asarray(vertices, np.float64).reshape(-1, 3)
    F = np.asarray(triangles, np.int64).reshape(-1, 3)
    p0, p1, p2 = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    v1, v2 = p1 - p0, p2 - p0
    l1, l2 = _norm(v1), _norm(v2)
    c = np.stack([v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1], v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2],
                  v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]], axis=1)
    area2 = _norm(c)
    out = [V]
    for t in np.nonzero(area2 > 0)[0]:
        thr = thresh * np.sqrt((l1[t] * l2[t]) / area2[t])
        n1, n2 = np.floor(l1[t] / thr), np.floor(l2[t] / thr)
        i = np.arange(int(n1) + 1, dtype=np.float64)
        j = np.arange(int(n2) + 1, dtype=np.float64)
        k0 = np.repeat((i + 0.5) / max(n1, 1e-7), len(j))
        k1 = np.tile((j + 0.5) / max(n2, 1e-7), len(i))
        sel = k0 + k1 < 1
        k0, k1 = k0[sel], k1[sel]
        out.append((v1[t][None] * k0[:, None] + v2[t][None] * k1[:, None]) + p0[t][None])
    return np.concatenate(out, axis=0)


def thin(points, radius):
    """The keep mask of the greedy rule in index order (the points already shuffled), neighbours by scikit-learn's KD-tree."""
    p = np.asarray(points, np.float64)
    keep = np.ones(len(p), bool)
    if not len(p):
        return keep
    tree = skln.KDTree(p)
    nbrs = tree.query_radius(p, r=radius)
    removed = np.zeros(len(p), bool)
    for q in range(len(p)):
        if removed[q]:
            keep[q] = False
            continue
        removed[nbrs[q]] = True
    return keep


def thin_sequential(points, radius, order):
    """The same rule written out pairwise (no tree): (dx dx + dy dy) + dz dz <= radius^2, visiting `order`."""
    p = np.asarray(points, np.float64)
    keep = np.zeros(len(p), bool)
    removed = np.zeros(len(p), bool)
    r2 = radius * radius
    for q in order:
        if removed[q]:
            continue
        keep[q] = True
        d = p - p[q]
        removed |= (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r2
    return keep


def mask_flags(points, obs_mask, bb, res, patch):
    p = np.asarray(points, np.float64)
    BB = np.asarray(bb).astype(np.float32).reshape(2, 3)
    lo = (BB[:1] - np.float32(patch)).astype(np.float32)
    hi = (BB[1:] + np.float32(patch * 2)).astype(np.float32)
    inbound = np.all((p >= lo.astype(np.float64)) & (p < hi.astype(np.float64)), axis=1)
    g = np.rint((p - BB[:1].astype(np.float64)) / np.float64(res))
    shape = np.asarray(obs_mask.shape)
    ing = inbound & np.all((g >= 0) & (g < shape[None]), axis=1)
    obs = np.zeros(len(p), bool)
    gi = g[ing].astype(np.int64)
    obs[ing] = np.asarray(obs_mask)[gi[:, 0], gi[:, 1], gi[:, 2]] != 0
    return inbound, obs


def above_plane(points, plane):
    p = np.asarray(points, np.float64)
    P = np.asarray(plane, np.float64).reshape(-1)
    return ((P[0] * p[:, 0] + P[1] * p[:, 1]) + P[2] * p[:, 2]) + P[3] > 0


def nearest(queries, targets, max_dist):
    """distance to the nearest target where < max_dist, +inf elsewhere"""
    q = np.asarray(queries, np.float64).reshape(-1, 3)
    out = np.full(len(q), np.inf)
    if not len(q) or not len(targets):
        return out
    d, _ = skln.KDTree(np.asarray(targets, np.float64)).query(q, k=1)
    d = d[:, 0]
    out[d < max_dist] = d[d < max_dist]
    return out


def masked_mean(d, max_dist):
    d = np.asarray(d)
    s = d[d < max_dist]
    return float(s.mean()) if len(s) else float("nan")


def fixed_order_sum(terms):
    """The device's fixed-order fp64 sum of `terms` (n,) or (n, Q), column by column -> (Q,).
    256 workgroups of 256 threads: thread t of workgroup b adds the elements b * 256 + t + m * 65536 in m order, starting
    from +0.0; the 64 lanes of a wave fold by halves (lane l += lane l + o for o = 32, 16, 8, 4, 2, 1); the four waves add
    as (w0 + w1) + (w2 + w3); the 256 workgroup sums are added in workgroup order, starting from +0.0.  An element the
    device skips is a row of +0.0 here: no running sum is ever -0.0 (they start at +0.0), so adding +0.0 changes no bit."""
    t = np.asarray(terms, np.float64)
    t = t[:, None] if t.ndim == 1 else t
    n, Q = t.shape
    padded = np.zeros((max(-(-n // 65536), 1) * 65536, Q))
    padded[:n] = t
    acc = np.zeros((256, 256, Q))  # [workgroup, thread]
    for step in padded.reshape(-1, 256, 256, Q):
        acc = acc + step
    lanes = acc.reshape(256, 4, 64, Q)  # [workgroup, wave, lane]
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes[:, :, :o] + lanes[:, :, o:2 * o]
    w = lanes[:, :, 0]
    part = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    s = np.zeros(Q)
    for b in range(256):
        s = s + part[b]
    return s


def masked_sum_fixed_order(d, max_dist):
    """gs2m_eval_masked_mean's two outputs: the fixed-order sum of the entries < max_dist and their count."""
    d = np.asarray(d, np.float64).reshape(-1)
    ok = d < max_dist
    return float(fixed_order_sum(np.where(ok, d, 0.0))[0]), int(ok.sum())


def vis_colors(n, index, dist, max_dist, vis_dist):
    col = np.tile(np.array([[0.0, 0.0, 1.0]]), (n, 1))
    d = np.asarray(dist, np.float64).reshape(-1, 1)
    a = np.minimum(d, vis_dist) / vis_dist
    col[index] = np.array([[1.0, 0.0, 0.0]]) * a + np.array([[1.0, 1.0, 1.0]]) * (1 - a)
    col[index[d[:, 0] >= max_dist]] = np.array([0.0, 1.0, 0.0])
    return col


def evaluate(vertices, triangles, stl, obs_mask, bb, res, plane, thresh=0.2, patch=60.0, max_dist=20.0, seed=0, vis_dist=10.0):
    """The whole contract. -> dict of the means and every intermediate array."""
    cloud = sample_mesh(vertices, triangles, thresh)
    order = np.random.default_rng(seed).permutation(len(cloud))
    shuffled = cloud[order]
    keep = thin(shuffled, thresh)
    down = shuffled[keep]
    inbound, obs = mask_flags(down, obs_mask, bb, res, patch)
    data_in, data_in_obs = down[inbound], down[obs]
    stl = np.asarray(stl, np.float64)
    d2s = nearest(data_in_obs, stl, max_dist)
    above = above_plane(stl, plane)
    s2d = nearest(stl[above], data_in, max_dist)
    m1, m2 = masked_mean(d2s, max_dist), masked_mean(s2d, max_dist)
    return {"mean_d2s": m1, "mean_s2d": m2, "overall": (m1 + m2) / 2, "cloud": cloud, "order": order, "keep": keep, "down": down,
            "inbound": inbound, "obs": obs, "dist_d2s": d2s, "above": above, "dist_s2d": s2d,
            "d2s_colors": vis_colors(len(down), np.nonzero(obs)[0], d2s, max_dist, vis_dist),
            "s2d_colors": vis_colors(len(stl), np.nonzero(above)[0], s2d, max_dist, vis_dist)}
