"""An independent float64 reference of the TSDF fusion and of the marching-cubes output, written from DESIGN.md §9 and
include/gs2m_mesh.h (not from csrc/tsdf.hip or tests/mesh_ref.py, which restate each other in fp32).

Fusion (`fuse64`): per voxel centre and view, in float64: camera point, pixel floor(u + 0.5), SDF along the ray, truncation,
running weighted averages.  Beside the averages it returns how far every decision of every view was from its boundary;
a voxel is *decided* when all of them exceed the margin DELTA, and only decided voxels are compared with fp32 results.

Mesh (`MeshChecker`): invariants of (vertices, colours, triangles) against the volume they were extracted from, on a dense
global voxel grid.  No triangle table is read; the caller passes the 256 triangle counts, used in invariant 3 alone.
  1  one vertex per grid edge whose ends differ in (f < 0) and that lies in a valid cube (8 corners present, weight > 0),
     numbered by (slot, voxel, axis) as the header states; none missing, none extra, none unreferenced
  2  every vertex at the float64 zero crossing p0 + |f0| / (|f0| + |f1|) voxel of its edge, within POSITION_TOL_UNITS *
     eps32 * max(|coordinate|, voxel) per coordinate; its colour the same interpolation; everything finite, t in [0, 1]
  3  the triangles, taken in order, are the valid cubes' in (slot, voxel) order, each cube owning as many as its case has;
     every vertex of a triangle sits on one of its cube's 12 edges
  4  a mesh edge lying in a cube face: used twice, in opposite directions, when both cubes at the face are valid, once when
     one is; a mesh edge inside a cube: twice, in opposite directions
  5  orientation, without the table: for a directed triangle side A -> B lying in a face of its own cube, with N the face's
     outward normal, h = N x (B - A) points to the NON-negative ends of the two crossed grid edges and away from their
     negative ends.  The hand is fixed from case 1 (corner 0 negative): the triangle on the three edges leaving corner 0
     that faces away from it has the side (x edge) -> (y edge) in the face z = 0, and h . (corner 0 - midpoint) < 0 there.
     Each crossed grid edge has exactly one negative end, so the rule also holds on faces whose negative corners are
     diagonal, where "all the face's negative corners on one side" would not.

Tolerances (DESIGN.md §9 lists them; tests/test_tsdf_ref.py measures them again on the CPU and asserts they still hold):
  position   derived: voxel_centre rounds three times, t twice, the multiply and the add once each: 7 roundings of half an
             ulp = 3.5 eps32 max(|coordinate|, voxel) while no term exceeds the coordinate.  With a negative block the terms
             block * L and (i + 0.5) voxel cancel and each is up to L larger than the coordinate, so near the origin the
             error is larger in these units; measured on the marching-cubes inputs of tests/tsdf_inputs.py (fp32
             restatement against the float64 crossing): POSITION_MEASURED_UNITS.  POSITION_TOL_UNITS = max(3.5, 2 x measured).
  fusion     measured on the fusion input of tests/tsdf_inputs.py (fp32 restatement against `fuse64`, decided voxels):
             FUSION_TSDF_MEASURED, FUSION_COLOR_MEASURED; the tolerances are 4 x those.
Neither is measured against the HIP kernels: those must equal the fp32 restatement bit for bit."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
BV = 4096

DELTA = 1e-4                       # decision margin: pixels for u, v; metres for zc and sdf
FUSION_TSDF_MEASURED = 2.71e-6     # max |fp32 restatement - float64| over the decided voxels, tsdf on -1..1 (measured 2.703e-6)
FUSION_COLOR_MEASURED = 5.09e-6    # the same for the colour on 0..255 (measured 5.086e-6)
POSITION_DERIVED_UNITS = 3.5
POSITION_MEASURED_UNITS = 4.83     # measured 4.822 (every_case), 4.771 (sparse), 4.631 (checkerboard), 4.553 (big_pool)


# ---- fusion ----------------------------------------------------------------------------------------------------------

def centres64(coords, voxel):
    """(n, 3) block coordinates -> (n, 4096, 3) float64 voxel centres; voxel is the fp32 voxel size."""
    vx = float(np.float32(voxel))
    L = float(np.float32(16) * np.float32(voxel))
    v = np.arange(BV)
    ijk = np.stack([v % 16, (v // 16) % 16, v // 256], axis=1).astype(np.float64)
    return np.asarray(coords, np.float64)[:, None, :] * L + (ijk[None] + 0.5) * vx


def fuse64(coords, touched_per_view, views, voxel, trunc, depth_trunc):
    """coords (n, 3): the pool's blocks.  touched_per_view: per view the slots it integrates into.  views: tuples
    (depth (H, W) fp32, colour (H, W, 3) on 0..255, fx, fy, cx, cy, w2c (4, 4)); every number is taken as the fp32 value the
    kernels get, then used in float64.
    -> dict(tsdf, weight (n, 4096), color (n, 3, 4096), margin (n, 4096): the smallest distance of any decision of any view
    from its boundary, u_lo / u_hi (n_views,): voxels whose u fell in [0, 0.5) / [W - 0.5, W), straddle (n_views,): touched
    blocks with voxels on both sides of zc = 0)."""
    n = len(coords)
    tr, dt = float(np.float32(trunc)), float(np.float32(depth_trunc))
    cen = centres64(coords, voxel)
    tsdf, weight = np.zeros((n, BV)), np.zeros((n, BV))
    color = np.zeros((n, 3, BV))
    margin = np.full((n, BV), np.inf)
    u_lo, u_hi, straddle = [], [], []
    for slots, (depth, col, fx, fy, cx, cy, w2c) in zip(touched_per_view, views):
        slots = np.asarray(slots, np.int64)
        fx, fy, cx, cy = (float(np.float32(a)) for a in (fx, fy, cx, cy))
        m = np.asarray(w2c, np.float32).astype(np.float64)
        depth64 = np.asarray(depth, np.float32).astype(np.float64)
        col64 = np.asarray(col, np.float32).astype(np.float64)
        H, W = depth64.shape
        p = cen[slots]                                             # (T, 4096, 3)
        pc = p @ m[:3, :3].T + m[:3, 3]
        zc = pc[..., 2]
        mg = np.abs(zc)
        front = zc > 0
        straddle.append(int(np.sum(front.any(1) & (~front).any(1))))
        with np.errstate(divide="ignore", invalid="ignore"):
            uf = pc[..., 0] * fx / zc + cx + 0.5
            vf = pc[..., 1] * fy / zc + cy + 0.5
        live = front.copy()

        def image_axis(xf, size, live):
            d = np.minimum(np.abs(xf - 0.0001), np.abs(xf - size))
            inside = (xf >= 0.0001) & (xf < size)
            d = np.where(inside, np.minimum(d, np.abs(xf - np.rint(xf))), d)  # the pixel chosen: distance to the next integer
            return inside, np.where(live, d, np.inf)

        in_u, du = image_axis(uf, float(W), live)
        in_v, dv = image_axis(vf, float(H), live)
        mg = np.minimum(mg, np.minimum(du, dv))
        u_lo.append(int(np.sum(live & in_v & (uf >= 0.5) & (uf < 1.0))))
        u_hi.append(int(np.sum(live & in_v & (uf >= W) & (uf < W + 0.5))))
        live &= in_u & in_v
        u = np.where(live, np.floor(uf), 0).astype(np.int64)
        v = np.where(live, np.floor(vf), 0).astype(np.int64)
        d = depth64[v, u]
        with np.errstate(invalid="ignore"):
            live &= (d > 0) & (d <= dt)                             # NaN compares false; exact fp32 inputs: no margin
        d = np.where(live, d, 0.0)
        sdf = (d - zc) * np.sqrt(1.0 + ((u - cx) / fx) ** 2 + ((v - cy) / fy) ** 2)
        mg = np.minimum(mg, np.where(live, np.abs(sdf + tr), np.inf))
        live &= sdf > -tr
        t = np.minimum(1.0, sdf / tr)
        w = weight[slots]
        tsdf[slots] = np.where(live, (tsdf[slots] * w + t) / (w + 1.0), tsdf[slots])
        rgb = col64[v, u]                                          # (T, 4096, 3)
        for c in range(3):
            cc = color[slots, c]
            color[slots, c] = np.where(live, (cc * w + rgb[..., c]) / (w + 1.0), cc)
        weight[slots] = np.where(live, w + 1.0, w)
        margin[slots] = np.minimum(margin[slots], mg)
    return dict(tsdf=tsdf, weight=weight, color=color, margin=margin, u_lo=np.array(u_lo), u_hi=np.array(u_hi),
                straddle=np.array(straddle))


def fusion_compare(ref64, tsdf, weight, color):
    """A fp32 result against `fuse64`'s.  -> dict(undecided_fraction, weight_equal, tsdf_err, color_err) over the decided
    voxels; the fraction is of the voxels either side updated."""
    decided = ref64["margin"] > DELTA
    either = (ref64["weight"] > 0) | (np.asarray(weight) > 0)
    sel = decided & either
    return dict(undecided_fraction=float((~decided & either).sum()) / max(1, int(either.sum())),
                weight_equal=bool(np.array_equal(np.asarray(weight, np.float64)[decided], ref64["weight"][decided])),
                tsdf_err=float(np.abs(np.asarray(tsdf, np.float64) - ref64["tsdf"])[sel].max()) if sel.any() else 0.0,
                color_err=float(np.abs(np.asarray(color, np.float64) - ref64["color"])[np.broadcast_to(sel[:, None], color.shape)].max())
                if sel.any() else 0.0,
                n_decided=int(sel.sum()))


# ---- marching cubes --------------------------------------------------------------------------------------------------

CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)])  # standard numbering
# the 12 cube edges as (offset of the lower end from the cube origin, axis), standard numbering
CUBE_EDGES = np.array([(0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 1, 1), (0, 1, 1, 0), (0, 0, 1, 1),
                       (0, 0, 0, 2), (1, 0, 0, 2), (1, 1, 0, 2), (0, 1, 0, 2)])
UNIT = np.eye(3, dtype=np.int64)


def _case1_hand():
    """Invariant 5's hand: sign of h . (negative corner - midpoint) for the side (x edge) -> (y edge) of case 1's triangle."""
    px, py, pz = np.array([.5, 0, 0]), np.array([0, .5, 0]), np.array([0, 0, .5])
    assert np.cross(py - px, pz - px) @ np.ones(3) > 0          # (px, py, pz) faces away from corner 0
    h = np.cross(np.array([0, 0, -1.0]), py - px)               # the side lies in the face z = 0, outward normal -z
    return int(np.sign(h @ (np.zeros(3) - (px + py) / 2)))


NEG_HAND = _case1_hand()


class MeshInvariantError(AssertionError):
    def __init__(self, which, msg):
        super().__init__(f"mesh invariant {which}: {msg}")
        self.which = which


def _need(cond, which, msg):
    if not cond:
        raise MeshInvariantError(which, msg)


class MeshChecker:
    """vol: an object with dom (6 ints), coords (n, 3), tsdf, weight (n, 4096), color (n, 3, 4096), voxel (fp32).
    ntri: 256 triangle counts per cube case (bit q of the case = corner q negative)."""

    def __init__(self, vol, ntri):
        self.vol = vol
        self.ntri = np.asarray(ntri, np.int64)
        d0 = np.array(vol.dom[:3], np.int64)
        nb = np.array(vol.dom[3:], np.int64)
        X, Y, Z = (16 * nb).tolist()
        self.dims = np.array([X, Y, Z])
        self.F = np.zeros((X, Y, Z))
        Wt = np.zeros((X, Y, Z))
        self.C = np.zeros((3, X, Y, Z))
        self.slot_of = np.full(tuple(nb), -1, np.int64)
        coords = np.asarray(vol.coords, np.int64).reshape(-1, 3)
        for s, b in enumerate(coords):
            r = b - d0
            _need(np.all(r >= 0) and np.all(r < nb) and self.slot_of[tuple(r)] < 0, 0, f"block {b} outside the domain or twice")
            self.slot_of[tuple(r)] = s
            sl = tuple(slice(16 * int(q), 16 * int(q) + 16) for q in r)
            self.F[sl] = np.asarray(vol.tsdf[s], np.float64).reshape(16, 16, 16).transpose(2, 1, 0)
            Wt[sl] = np.asarray(vol.weight[s], np.float64).reshape(16, 16, 16).transpose(2, 1, 0)
            for c in range(3):
                self.C[c][sl] = np.asarray(vol.color[s][c], np.float64).reshape(16, 16, 16).transpose(2, 1, 0)
        ok = Wt > 0                                              # absent blocks have weight 0 here
        self.neg = self.F < 0                                    # -0.0 and +0.0: not negative
        vc = np.zeros((X, Y, Z), bool)                           # valid cube, by origin voxel
        inner = np.ones((X - 1, Y - 1, Z - 1), bool)
        for q in CORNERS:
            inner &= ok[q[0]:X - 1 + q[0], q[1]:Y - 1 + q[1], q[2]:Z - 1 + q[2]]
        vc[:X - 1, :Y - 1, :Z - 1] = inner
        self.vc = vc
        vcp = np.pad(vc, ((1, 0), (1, 0), (1, 0)))               # vcp[x + 1, y + 1, z + 1] = vc[x, y, z]; index 0: outside
        self.used = np.zeros((3, X, Y, Z), bool)                 # used[a, x, y, z]: the edge from the voxel to its +a neighbour
        for a in range(3):
            b1, b2 = [r for r in range(3) if r != a]
            cross = np.zeros((X, Y, Z), bool)
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[a], hi[a] = slice(0, self.dims[a] - 1), slice(1, self.dims[a])
            cross[tuple(lo)] = self.neg[tuple(lo)] != self.neg[tuple(hi)]
            held = np.zeros((X, Y, Z), bool)
            for s1 in (0, 1):
                for s2 in (0, 1):
                    sl = [slice(1, None)] * 3
                    sl[b1] = slice(1 - s1, self.dims[b1] + 1 - s1)
                    sl[b2] = slice(1 - s2, self.dims[b2] + 1 - s2)
                    held |= vcp[tuple(sl)]
            self.used[a] = cross & held
        # the vertices in the contract's order: (slot, voxel, axis)
        a, x, y, z = np.nonzero(self.used)
        slot = self.slot_of[x // 16, y // 16, z // 16]
        key = (slot * BV + (x % 16) + 16 * (y % 16) + 256 * (z % 16)) * 3 + a
        o = np.argsort(key, kind="stable")
        self.e_pos = np.stack([x[o], y[o], z[o]], axis=1)        # the lower voxel of vertex i's edge
        self.e_axis = a[o]
        self.e_slot = slot[o]
        self.vid = np.full((3, X, Y, Z), -1, np.int64)
        self.vid[self.e_axis, self.e_pos[:, 0], self.e_pos[:, 1], self.e_pos[:, 2]] = np.arange(len(o))
        # the valid cubes in (slot, voxel) order and their triangle counts
        x, y, z = np.nonzero(vc)
        slot = self.slot_of[x // 16, y // 16, z // 16]
        o = np.argsort(slot * BV + (x % 16) + 16 * (y % 16) + 256 * (z % 16), kind="stable")
        self.c_pos = np.stack([x[o], y[o], z[o]], axis=1)
        self.c_slot = slot[o]
        case = np.zeros(len(o), np.int64)
        for q, c in enumerate(CORNERS):
            case |= self.neg[self.c_pos[:, 0] + c[0], self.c_pos[:, 1] + c[1], self.c_pos[:, 2] + c[2]].astype(np.int64) << q
        self.c_case = case
        self.c_ntri = self.ntri[case]
        self.n_vertices, self.n_triangles = len(self.e_axis), int(self.c_ntri.sum())
        self.voxel64 = float(np.float32(vol.voxel))
        self.L64 = float(np.float32(16) * np.float32(vol.voxel))
        self.d0 = d0

    # -- what the reference says about the expected mesh ------------------------------------------------------------
    def crossing(self):
        """-> (positions (V, 3), colours (V, 3) in 0..1, t (V,)) in float64."""
        p, a = self.e_pos, self.e_axis
        q = p + UNIT[a]
        f0, f1 = self.F[p[:, 0], p[:, 1], p[:, 2]], self.F[q[:, 0], q[:, 1], q[:, 2]]
        t = np.abs(f0) / (np.abs(f0) + np.abs(f1))
        block = p // 16 + self.d0
        pos = block * self.L64 + (p % 16 + 0.5) * self.voxel64
        pos[np.arange(len(p)), a] += t * self.voxel64
        c0, c1 = self.C[:, p[:, 0], p[:, 1], p[:, 2]].T, self.C[:, q[:, 0], q[:, 1], q[:, 2]].T
        return pos, (c0 + t[:, None] * (c1 - c0)) / 255.0, t

    def position_units(self, verts):
        """|verts - crossing| per coordinate in units of eps32 max(|coordinate|, voxel) -> (V, 3)."""
        pos, _, _ = self.crossing()
        return np.abs(np.asarray(verts, np.float64) - pos) / (EPS32 * np.maximum(np.abs(pos), self.voxel64))

    # -- the invariants ---------------------------------------------------------------------------------------------
    def inv1(self, verts, cols, tris):
        V = self.n_vertices
        _need(len(verts) == V and len(cols) == V, 1, f"{len(verts)} vertices, {len(cols)} colours for {V} used crossed edges")
        t = np.asarray(tris, np.int64).reshape(-1, 3)
        _need(t.size == 0 or (t.min() >= 0 and t.max() < V), 1, "a vertex id outside [0, V)")
        seen = np.zeros(V, bool)
        seen[t.reshape(-1)] = True
        _need(bool(seen.all()), 1, f"{int((~seen).sum())} unreferenced vertices")

    def inv2(self, verts, cols, tris, tol_units=None):
        tol_units = POSITION_TOL_UNITS if tol_units is None else tol_units
        verts, cols = np.asarray(verts, np.float64), np.asarray(cols, np.float64)
        _need(len(verts) == self.n_vertices, 2, "vertex count")
        _need(bool(np.isfinite(verts).all() and np.isfinite(cols).all()), 2, "a vertex or colour is not finite")
        pos, col, t = self.crossing()
        _need(bool(np.isfinite(t).all() and (t >= 0).all() and (t <= 1).all()), 2, "t outside [0, 1]")
        units = np.abs(verts - pos) / (EPS32 * np.maximum(np.abs(pos), self.voxel64))
        _need(units.size == 0 or units.max() <= tol_units, 2, f"a vertex {units.max() if units.size else 0:.3g} units from its crossing (allowed {tol_units:.3g})")
        p, a = self.e_pos, self.e_axis
        q = p + UNIT[a]
        cmag = np.abs(self.C[:, p[:, 0], p[:, 1], p[:, 2]].T) + np.abs(self.C[:, q[:, 0], q[:, 1], q[:, 2]].T)
        # t: 2 roundings, c1 - c0, the product, the sum and the division one each: 6 half-ulps of terms no larger than |c0| + |c1|
        ctol = 3.0 * EPS32 * (cmag + 1.0) / 255.0
        _need(bool((np.abs(cols - col) <= ctol).all()), 2, "a vertex colour is off its interpolation")

    def _tri_cubes(self, tris):
        t = np.asarray(tris, np.int64).reshape(-1, 3)
        _need(len(t) == self.n_triangles, 3, f"{len(t)} triangles, the valid cubes' cases have {self.n_triangles}")
        return t, np.repeat(np.arange(len(self.c_ntri)), self.c_ntri)

    def inv3(self, verts, cols, tris):
        t, cube = self._tri_cubes(tris)
        if len(t) == 0:
            return
        _need(t.min() >= 0 and t.max() < self.n_vertices, 3, "a vertex id outside [0, V)")
        _need(bool(np.all((t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0]))), 3, "a triangle repeats a vertex")
        d = self.e_pos[t] - self.c_pos[cube][:, None, :]                    # (F, 3 corners, 3)
        ax = self.e_axis[t]
        on = np.all((d >= 0) & (d <= 1), axis=-1) & (np.take_along_axis(d, ax[..., None], axis=-1)[..., 0] == 0)
        _need(bool(on.all()), 3, f"{int((~on).any(1).sum())} triangles have a vertex off their cube's edges")

    def _sides(self, tris):
        """Per directed triangle side: ids (a, b), cube, local edge descriptors, the shared face (axis n or -1, side s)."""
        t, cube = self._tri_cubes(tris)
        a, b = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)
        cube = np.repeat(cube, 3)
        org = self.c_pos[cube]
        d1, d2 = self.e_pos[a] - org, self.e_pos[b] - org
        a1, a2 = self.e_axis[a], self.e_axis[b]
        n_face = np.full(len(a), -1, np.int64)
        count = np.zeros(len(a), np.int64)
        for n in range(3):
            share = (a1 != n) & (a2 != n) & (d1[:, n] == d2[:, n])
            n_face = np.where(share, n, n_face)
            count += share
        _need(bool((count <= 1).all()), 4, "a triangle side joins a grid edge to itself")
        s_face = np.where(n_face >= 0, np.take_along_axis(d1, np.maximum(n_face, 0)[:, None], axis=1)[:, 0], 0)
        return a, b, cube, org, d1, d2, a1, a2, n_face, s_face

    def inv4(self, verts, cols, tris):
        a, b, cube, org, d1, d2, a1, a2, n_face, s_face = self._sides(tris)
        if len(a) == 0:
            return
        X, Y, Z = self.dims.tolist()
        inface = n_face >= 0
        nn = np.maximum(n_face, 0)
        q = org + UNIT[nn] * s_face[:, None]                     # origin of the cube on the face's upper side
        below = q - UNIT[nn]
        vcp = np.pad(self.vc, ((1, 0), (1, 0), (1, 0)))
        n_valid = self.vc[q[:, 0], q[:, 1], q[:, 2]].astype(np.int64) + vcp[below[:, 0] + 1, below[:, 1] + 1, below[:, 2] + 1]
        place = np.where(inface, ((nn * X + q[:, 0]) * Y + q[:, 1]) * Z + q[:, 2], -1 - cube)
        rows = np.stack([place, np.minimum(a, b), np.maximum(a, b)], axis=1)
        o = np.lexsort(rows.T[::-1])
        rows, dirn, want = rows[o], np.where(a < b, 1, -1)[o], np.where(inface, n_valid, 2)[o]
        first = np.concatenate([[True], np.any(rows[1:] != rows[:-1], axis=1)])
        start = np.nonzero(first)[0]
        cnt = np.diff(np.concatenate([start, [len(rows)]]))
        dsum = np.add.reduceat(dirn, start)
        want = want[start]
        _need(bool((want >= 1).all()), 4, "a triangle side lies in a face without a valid cube")
        bad = cnt != want
        _need(not bad.any(), 4, f"{int(bad.sum())} mesh edges used {cnt[bad][:4]} times where {want[bad][:4]} valid cubes meet")
        twice = want == 2
        _need(bool((dsum[twice] == 0).all()), 4, f"{int((dsum[twice] != 0).sum())} mesh edges used twice in the same direction")

    def inv5(self, verts, cols, tris):
        a, b, cube, org, d1, d2, a1, a2, n_face, s_face = self._sides(tris)
        sel = n_face >= 0
        if not sel.any():
            return
        org, d1, d2, a1, a2, n_face, s_face = (q[sel] for q in (org, d1, d2, a1, a2, n_face, s_face))
        N = UNIT[n_face] * (2 * s_face - 1)[:, None]
        A, B = d1 + 0.5 * UNIT[a1], d2 + 0.5 * UNIT[a2]
        h = np.cross(N, B - A)
        M = (A + B) / 2
        for d, ax in ((d1, a1), (d2, a2)):
            for end in (d, d + UNIT[ax]):
                g = org + end
                neg = self.neg[g[:, 0], g[:, 1], g[:, 2]]
                side = np.sign(np.einsum("ij,ij->i", h, end - M)).astype(np.int64)
                want = np.where(neg, NEG_HAND, -NEG_HAND)
                _need(bool((side == want).all()), 5, f"{int((side != want).sum())} triangle sides wind the wrong way round their face")

    def check(self, verts, cols, tris, tol_units=None):
        self.inv1(verts, cols, tris)
        self.inv2(verts, cols, tris, tol_units)
        self.inv3(verts, cols, tris)
        self.inv4(verts, cols, tris)
        self.inv5(verts, cols, tris)

    # -- census helpers (tests/test_tsdf_ref.py) ------------------------------------------------------------------
    def per_slot_counts(self):
        """-> (vertices, triangles) owned per slot."""
        n = len(np.asarray(self.vol.coords).reshape(-1, 3))
        return np.bincount(self.e_slot, minlength=n), np.bincount(self.c_slot, weights=self.c_ntri, minlength=n).astype(np.int64)


POSITION_TOL_UNITS = max(POSITION_DERIVED_UNITS, 2.0 * POSITION_MEASURED_UNITS)
FUSION_TSDF_TOL = 4.0 * FUSION_TSDF_MEASURED
FUSION_COLOR_TOL = 4.0 * FUSION_COLOR_MEASURED
