"""The TSDF fusion + marching-cubes contract (include/gs2m_mesh.h) restated in plain numpy: the oracle of
gs-2m_amd/csrc/tsdf.hip.  Like the texture oracle it is UNPINNED -- Open3D, whose legacy ScalableTSDFVolume the contract
follows, is not available to compare against -- so it checks that the kernels do what the contract says, not that the
contract is Open3D's.  fp32 throughout, every expression in the kernels' order of operations (they are compiled with
-ffp-contract=off), so results can be compared bit for bit."""
import os
import re

import numpy as np

f32 = np.float32
BV = 4096
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_H = os.path.join(ROOT, "gs-2m_amd", "csrc", "tsdf_tables.h")

CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)])
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
# per edge: owner voxel offset from the cube origin (the lower end) and axis
EDGE_OWNER = np.array([np.minimum(CORNERS[a], CORNERS[b]).tolist() + [int(np.argmax(np.abs(CORNERS[a] - CORNERS[b])))] for a, b in EDGES])


def load_table():
    """tsdf_tables.h -> (256, 16) int array of edge ids, -1 padded (the same table the kernels read)."""
    txt = open(TABLE_H).read()
    body = txt[txt.index("GS2M_MC_TRI"):]
    rows = re.findall(r"\{([-\d,\s]+)\}", body)
    t = np.array([[int(x) for x in r.split(",")] for r in rows], dtype=np.int64)
    assert t.shape[0] == 256, t.shape
    return t


class Volume:
    def __init__(self, dom, voxel, trunc, depth_trunc):
        self.dom = [int(x) for x in dom]
        self.voxel, self.trunc, self.depth_trunc = f32(voxel), f32(trunc), f32(depth_trunc)
        self.L = f32(16) * self.voxel
        self.index = np.full(self.dom[3] * self.dom[4] * self.dom[5], -1, np.int64)
        self.coords = np.zeros((0, 3), np.int64)
        self.tsdf = np.zeros((0, BV), f32)
        self.weight = np.zeros((0, BV), f32)
        self.color = np.zeros((0, 3, BV), f32)
        self.ignored = 0

    @property
    def n(self):
        return len(self.coords)

    def linear(self, b):
        x0, y0, z0, nx, ny, nz = self.dom
        return ((b[..., 2] - z0) * ny + (b[..., 1] - y0)) * nx + (b[..., 0] - x0)

    def points(self, depth, fx, fy, cx, cy, c2w):
        H, W = depth.shape
        vv, uu = np.meshgrid(np.arange(0, H, 4), np.arange(0, W, 4), indexing="ij")
        d = depth[vv, uu].astype(f32)
        ok = (d > 0) & (d <= self.depth_trunc)
        uu, vv, d = uu[ok], vv[ok], d[ok]
        xc = ((uu.astype(f32) - f32(cx)) * d) / f32(fx)
        yc = ((vv.astype(f32) - f32(cy)) * d) / f32(fy)
        c = np.asarray(c2w, f32)
        return np.stack([((c[r, 0] * xc + c[r, 1] * yc) + c[r, 2] * d) + c[r, 3] for r in range(3)], axis=1)

    def touch(self, depth, fx, fy, cx, cy, c2w):
        """-> the view's touched slots (increasing linear block index); appends the new blocks."""
        p = self.points(depth, fx, fy, cx, cy, c2w)
        lo = np.floor((p - self.trunc) / self.L).astype(np.int64)
        hi = np.floor((p + self.trunc) / self.L).astype(np.int64)
        dmin, dn = np.array(self.dom[:3]), np.array(self.dom[3:])
        inside = np.all((lo >= dmin) & (hi < dmin + dn), axis=1)
        self.ignored += int((~inside).sum())
        lins = set()
        for a, b in zip(lo[inside], hi[inside]):
            for z in range(a[2], b[2] + 1):
                for y in range(a[1], b[1] + 1):
                    for x in range(a[0], b[0] + 1):
                        lins.add(int(self.linear(np.array([x, y, z]))))
        lins = np.array(sorted(lins), np.int64)
        new = lins[self.index[lins] < 0] if len(lins) else lins
        if len(new):
            nx, ny = self.dom[3], self.dom[4]
            bc = np.stack([new % nx + self.dom[0], (new // nx) % ny + self.dom[1], new // (nx * ny) + self.dom[2]], axis=1)
            self.index[new] = self.n + np.arange(len(new))
            self.coords = np.concatenate([self.coords, bc])
            self.tsdf = np.concatenate([self.tsdf, np.zeros((len(new), BV), f32)])
            self.weight = np.concatenate([self.weight, np.zeros((len(new), BV), f32)])
            self.color = np.concatenate([self.color, np.zeros((len(new), 3, BV), f32)])
        return self.index[lins] if len(lins) else lins

    def centres(self, slots):
        v = np.arange(BV)
        ijk = np.stack([v & 15, (v >> 4) & 15, v >> 8], axis=1).astype(f32)
        b = self.coords[slots].astype(f32)
        return [b[:, r:r + 1] * self.L + (ijk[None, :, r] + f32(0.5)) * self.voxel for r in range(3)]

    def integrate(self, depth, color255, fx, fy, cx, cy, w2c):
        """depth (H, W) fp32, color255 (H, W, 3) fp32 on 0..255, w2c (4, 4).  The c2w of the touch rule is c2w_of(w2c)."""
        w2c = np.asarray(w2c, f32)
        c2w = np.linalg.inv(w2c.astype(np.float64)).astype(f32)
        slots = self.touch(depth, fx, fy, cx, cy, c2w)
        if len(slots) == 0:
            return slots
        H, W = depth.shape
        fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
        x, y, z = self.centres(slots)
        m = w2c
        xc = ((m[0, 0] * x + m[0, 1] * y) + m[0, 2] * z) + m[0, 3]
        yc = ((m[1, 0] * x + m[1, 1] * y) + m[1, 2] * z) + m[1, 3]
        zc = ((m[2, 0] * x + m[2, 1] * y) + m[2, 2] * z) + m[2, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            uf = ((xc * fx) / zc + cx) + f32(0.5)
            vf = ((yc * fy) / zc + cy) + f32(0.5)
        ok = (zc > 0) & (uf >= f32(0.0001)) & (uf < f32(W)) & (vf >= f32(0.0001)) & (vf < f32(H))
        u = np.where(ok, uf, 0).astype(np.int64)
        v = np.where(ok, vf, 0).astype(np.int64)
        d = depth.astype(f32)[v, u]
        ok &= (d > 0) & (d <= self.depth_trunc)
        a = (u.astype(f32) - cx) / fx
        b = (v.astype(f32) - cy) / fy
        sdf = (d - zc) * np.sqrt((f32(1) + a * a) + b * b)
        ok &= sdf > -self.trunc
        t = np.minimum(f32(1), sdf / self.trunc)
        w = self.weight[slots]
        w1 = w + f32(1)
        ts = self.tsdf[slots]
        self.tsdf[slots] = np.where(ok, (ts * w + t) / w1, ts)
        col = color255.astype(f32)[v, u]  # (T, 4096, 3)
        for c in range(3):
            cc = self.color[slots, c]
            self.color[slots, c] = np.where(ok, (cc * w + col[..., c]) / w1, cc)
        self.weight[slots] = np.where(ok, w1, w)
        return slots


def voxel_ref(vol, slot, i, j, k):
    """Global voxel ids (slot * 4096 + v) of voxels (i, j, k) in [-1, 17) of the given slots' blocks, -1 where missing."""
    o = [np.where(q < 0, -1, np.where(q >= 16, 1, 0)) for q in (i, j, k)]
    b = vol.coords[slot] + np.stack(o, axis=-1)
    x0, y0, z0, nx, ny, nz = vol.dom
    rel = b - np.array([x0, y0, z0])
    ok = np.all((rel >= 0) & (rel < np.array([nx, ny, nz])), axis=-1)
    s = np.where(ok, vol.index[np.where(ok, vol.linear(b), 0)], -1)
    v = (i - 16 * o[0]) + 16 * (j - 16 * o[1]) + 256 * (k - 16 * o[2])
    return np.where(s >= 0, s * BV + v, -1)


def marching_cubes(vol, table=None):
    """-> (vertices (V, 3) fp32, colors (V, 3) fp32 in 0..1, triangles (F, 3) int32), in the kernels' order."""
    table = load_table() if table is None else table
    n = vol.n
    if n == 0:
        return np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros((0, 3), np.int32)
    slot = np.repeat(np.arange(n), BV)
    v = np.tile(np.arange(BV), n)
    i, j, k = v & 15, (v >> 4) & 15, v >> 8
    tsdf, weight = vol.tsdf.reshape(-1), vol.weight.reshape(-1)
    valid = np.ones(n * BV, bool)
    case = np.zeros(n * BV, np.int64)
    for q in range(8):
        g = voxel_ref(vol, slot, i + CORNERS[q, 0], j + CORNERS[q, 1], k + CORNERS[q, 2])
        gg = np.maximum(g, 0)
        valid &= (g >= 0) & (weight[gg] > 0)
        case |= np.where((g >= 0) & (tsdf[gg] < 0), 1 << q, 0)
    masks = np.zeros((n * BV, 3), bool)
    nbr = np.zeros((n * BV, 3), np.int64)
    for a in range(3):
        b1, b2 = (1 if a == 0 else 0), (1 if a == 2 else 2)
        anyv = np.zeros(n * BV, bool)
        for s in range(4):
            off = [0, 0, 0]
            off[b1], off[b2] = -(s & 1), -(s >> 1)
            g = voxel_ref(vol, slot, i + off[0], j + off[1], k + off[2])
            anyv |= (g >= 0) & valid[np.maximum(g, 0)]
        e = [int(a == 0), int(a == 1), int(a == 2)]
        g1 = voxel_ref(vol, slot, i + e[0], j + e[1], k + e[2])
        nbr[:, a] = g1
        masks[:, a] = anyv & ((tsdf < 0) != (tsdf[np.maximum(g1, 0)] < 0))
    flat = masks.reshape(-1)
    vid = np.cumsum(flat) - 1  # vertex id of (voxel, axis)
    base = np.concatenate([[0], np.cumsum(masks.sum(1))[:-1]])  # first vertex of each voxel
    L, vox = vol.L, vol.voxel
    bc = vol.coords[slot].astype(f32)
    p0 = np.stack([bc[:, 0] * L + (i.astype(f32) + f32(0.5)) * vox, bc[:, 1] * L + (j.astype(f32) + f32(0.5)) * vox,
                   bc[:, 2] * L + (k.astype(f32) + f32(0.5)) * vox], axis=1)
    g0, ax = np.nonzero(masks)  # row-major: (voxel, axis) order
    g1 = nbr[g0, ax]
    f0, f1 = tsdf[g0], tsdf[g1]
    af0 = np.abs(f0)
    t = af0 / (af0 + np.abs(f1))
    verts = p0[g0].copy()
    verts[np.arange(len(g0)), ax] = p0[g0, ax] + t * vox
    col = vol.color.transpose(0, 2, 1).reshape(-1, 3)  # (n * 4096, 3)
    c0, c1 = col[g0], col[g1]
    cols = (c0 + t[:, None] * (c1 - c0)) / f32(255)
    # triangles
    cubes = np.nonzero(valid)[0]
    rows = table[case[cubes]][:, :15]  # (C, 15)
    ent = rows >= 0
    ce = np.repeat(cubes, 15).reshape(-1, 15)
    e = np.maximum(rows, 0)
    ow = EDGE_OWNER[e]  # (C, 15, 4)
    go = voxel_ref(vol, slot[ce], i[ce] + ow[..., 0], j[ce] + ow[..., 1], k[ce] + ow[..., 2])
    go = np.maximum(go, 0)
    axis = ow[..., 3]
    below = np.where(axis >= 1, masks[go, 0], False).astype(np.int64) + np.where(axis >= 2, masks[go, 1], False).astype(np.int64)
    ids = base[go] + below
    tris = ids[ent].reshape(-1, 3).astype(np.int32)
    assert np.array_equal(vid[flat], np.arange(flat.sum()))
    return verts.astype(f32), cols.astype(f32), tris


def sphere_volume(centre, radius, voxel, trunc, margin_blocks=1):
    """A volume whose blocks cover the sphere's surface band, tsdf = clip((|x - c| - r) / trunc, -1, 1), weight 1."""
    L = 16 * voxel
    lo = np.floor((np.asarray(centre) - radius - trunc) / L).astype(int) - margin_blocks
    hi = np.floor((np.asarray(centre) + radius + trunc) / L).astype(int) + margin_blocks
    dom = list(lo) + list(hi - lo + 1)
    vol = Volume(dom, voxel, trunc, 100.0)
    bs = np.stack(np.meshgrid(*[np.arange(lo[r], hi[r] + 1) for r in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
    bs = bs[np.argsort(vol.linear(bs))]
    cen = (bs + 0.5) * L
    near = np.abs(np.linalg.norm(cen - np.asarray(centre), axis=1) - radius) < (np.sqrt(3) * L / 2 + trunc)
    bs = bs[near]
    vol.index[vol.linear(bs)] = np.arange(len(bs))
    vol.coords = bs.astype(np.int64)
    x, y, z = vol.centres(np.arange(len(bs)))
    dist = np.sqrt((x - f32(centre[0])) ** 2 + (y - f32(centre[1])) ** 2 + (z - f32(centre[2])) ** 2) - f32(radius)
    vol.tsdf = np.clip(dist / f32(trunc), -1, 1).astype(f32)
    vol.weight = np.ones_like(vol.tsdf)
    vol.color = np.full((len(bs), 3, BV), 128.0, f32)
    return vol


def mesh_stats(verts, tris):
    """-> (closed: every undirected edge in exactly two triangles, Euler characteristic, signed volume, components)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t = np.asarray(tris, np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    key = e[:, 0] * (len(verts) + 1) + e[:, 1]
    _, cnt = np.unique(key, return_counts=True)
    closed = bool(np.all(cnt == 2))
    used = np.unique(t)
    euler = len(used) - len(cnt) + len(t)
    v = np.asarray(verts, np.float64)
    vol = float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)
    g = coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(len(verts), len(verts)))
    ncomp, lab = connected_components(g, directed=False)
    comps = len(np.unique(lab[used]))
    return closed, euler, vol, comps
