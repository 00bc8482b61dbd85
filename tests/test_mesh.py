"""Mesh extraction, host side: the numpy restatement of the TSDF / marching-cubes contract (tests/mesh_ref.py) against
closed forms, the marching-cubes table the kernels read, and the host logic of gs2m_mesh (clusters, PLY, depth
quantisation).  No GPU needed."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as R  # noqa: E402
import gs2m_mesh as M  # noqa: E402


# ---- restatement: integration ----------------------------------------------------------------------------------------

def _plane_view(W=64, H=48, d0=1.0):
    fx = fy = 50.0
    cx, cy = W / 2.0, H / 2.0
    return np.full((H, W), d0, np.float32), fx, fy, cx, cy, np.eye(4, dtype=np.float32)


def test_restatement_plane_matches_closed_form():
    depth, fx, fy, cx, cy, w2c = _plane_view()
    voxel, trunc = 0.01, 0.04
    vol = R.Volume([-10, -10, 0, 20, 20, 20], voxel, trunc, 3.0)
    color = np.full(depth.shape + (3,), 200.0, np.float32)
    slots = vol.integrate(depth, color, fx, fy, cx, cy, w2c)
    # touched set: the AABB rule evaluated independently in fp64 over the stride-4 pixels
    L = 16 * voxel
    want = set()
    for v in range(0, depth.shape[0], 4):
        for u in range(0, depth.shape[1], 4):
            p = np.array([(u - cx) * 1.0 / fx, (v - cy) * 1.0 / fy, 1.0])
            lo, hi = np.floor((p - trunc) / L).astype(int), np.floor((p + trunc) / L).astype(int)
            want |= set(itertools.product(*[range(lo[r], hi[r] + 1) for r in range(3)]))
    got = {tuple(int(x) for x in b) for b in vol.coords[slots]}
    assert got == want
    assert list(slots) == sorted(slots, key=lambda s: vol.linear(vol.coords[s]))
    # every updated voxel: the closed form min(1, (d - z) mult / trunc) with the pixel it projects to
    x, y, z = [np.asarray(a, np.float64) for a in vol.centres(np.arange(vol.n))]
    upd = vol.weight > 0
    assert upd.sum() > 1000
    u = np.floor(x * fx / z + cx + 0.5)
    v = np.floor(y * fy / z + cy + 0.5)
    mult = np.sqrt(1 + ((u - cx) / fx) ** 2 + ((v - cy) / fy) ** 2)
    closed = np.minimum(1.0, (1.0 - z) * mult / trunc)
    assert np.abs(vol.tsdf[upd] - closed[upd]).max() < 1e-5
    assert np.all(closed[upd] > -1.0)
    assert np.all(vol.color[:, 0][upd] == 200.0)
    # a second identical view: TSDF unchanged, weights 2
    t1, w1 = vol.tsdf.copy(), vol.weight.copy()
    vol.integrate(depth, color, fx, fy, cx, cy, w2c)
    assert np.array_equal(vol.tsdf, t1)
    assert np.array_equal(vol.weight[upd], np.full(upd.sum(), 2.0, np.float32))
    assert np.array_equal(vol.weight[~upd], w1[~upd])


def test_restatement_depth_rules():
    """Holes, depths beyond depth_trunc and points outside the domain."""
    depth, fx, fy, cx, cy, w2c = _plane_view()
    depth[:, :20] = 0.0
    depth[:10] = 9.0  # beyond depth_trunc: empty
    vol = R.Volume([-10, -10, 0, 20, 20, 20], 0.01, 0.04, 3.0)
    vol.integrate(depth, np.zeros(depth.shape + (3,), np.float32), fx, fy, cx, cy, w2c)
    x, y, z = [np.asarray(a) for a in vol.centres(np.arange(vol.n))]
    u = np.floor(x * fx / z + cx + 0.5)
    assert np.all(u[vol.weight > 0] >= 20)
    small = R.Volume([0, 0, 0, 1, 1, 1], 0.01, 0.04, 3.0)
    small.touch(depth, fx, fy, cx, cy, np.eye(4, dtype=np.float32))
    assert small.ignored > 0


# ---- restatement: marching cubes -------------------------------------------------------------------------------------

def test_restatement_sphere_is_closed():
    c, r, voxel = (0.13, -0.07, 0.41), 0.3, 0.02
    vol = R.sphere_volume(c, r, voxel, 4 * voxel)
    verts, cols, tris = R.marching_cubes(vol)
    closed, euler, volume, comps = R.mesh_stats(verts, tris)
    assert closed and euler == 2 and comps == 1
    assert len(np.unique(tris)) == len(verts), "unreferenced vertices"
    assert volume > 0
    assert abs(volume - 4.0 / 3.0 * np.pi * r ** 3) < 0.03 * 4.0 / 3.0 * np.pi * r ** 3
    dist = np.abs(np.linalg.norm(verts.astype(np.float64) - np.array(c), axis=1) - r)
    assert dist.max() < 0.5 * voxel
    assert np.allclose(cols, 128.0 / 255.0)


# ---- the marching-cubes table ----------------------------------------------------------------------------------------

FACES = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (3, 7, 6, 2), (0, 4, 7, 3), (1, 2, 6, 5)]


def _edge(a, b):
    return next(e for e, (p, q) in enumerate(R.EDGES) if {p, q} == {a, b})


def test_table_is_the_generators_output():
    """One source: the header is what tools/make_mc_tables.py writes."""
    sys.path.insert(0, os.path.join(R.ROOT, "tools"))
    import make_mc_tables
    assert open(R.TABLE_H).read() == make_mc_tables.header_text()


def test_table_edges_and_faces():
    t = R.load_table()
    face_edges = [{_edge(f[i], f[(i + 1) % 4]) for i in range(4)} for f in FACES]
    seen = {}
    for case in range(256):
        row = [e for e in t[case] if e >= 0]
        assert len(row) % 3 == 0 and len(row) <= 15 and all(e < 0 for e in t[case][len(row):])
        inside = [(case >> k) & 1 for k in range(8)]
        crossed = {e for e, (a, b) in enumerate(R.EDGES) if inside[a] != inside[b]}
        assert set(row) <= crossed, f"case {case} uses an edge whose ends have the same sign"
        assert crossed <= set(row), f"case {case} leaves a crossed edge unused"
        tris = [row[3 * i:3 * i + 3] for i in range(len(row) // 3)]
        assert all(len(set(tr)) == 3 for tr in tris)
        for fi, f in enumerate(FACES):
            segs = frozenset(frozenset((tr[a], tr[(a + 1) % 3])) for tr in tris for a in range(3)
                             if tr[a] in face_edges[fi] and tr[(a + 1) % 3] in face_edges[fi])
            key = (fi, tuple(inside[k] for k in f))  # this face's own four corner signs
            assert seen.setdefault(key, segs) == segs, f"case {case}: face {f} drawn differently for the same corner signs"
    assert len(seen) == 6 * 16


def test_table_orientation_faces_outside():
    """Case 1 (corner 0 inside): the triangle's normal points away from corner 0."""
    t = R.load_table()
    mid = {e: (R.CORNERS[a] + R.CORNERS[b]) / 2.0 for e, (a, b) in enumerate(R.EDGES)}
    for case in range(1, 255):
        inside = np.array([(case >> k) & 1 for k in range(8)])
        grad = ((1 - 2 * inside)[:, None] * (R.CORNERS - 0.5)).sum(0)  # towards the outside corners
        row = [e for e in t[case] if e >= 0]
        if inside.sum() not in (1, 7):
            continue
        for i in range(0, len(row), 3):
            p = [mid[e] for e in row[i:i + 3]]
            n = np.cross(p[1] - p[0], p[2] - p[0])
            assert n @ grad > 0, case


# ---- host logic ------------------------------------------------------------------------------------------------------

def _strip(n, x0=0.0, vid0=0):
    """A connected strip of 2n triangles over 2(n + 1) vertices."""
    v = np.array([[x0 + i, y, 0.0] for i in range(n + 1) for y in (0.0, 1.0)], np.float32)
    t = []
    for i in range(n):
        a, b, c, d = 2 * i, 2 * i + 1, 2 * i + 2, 2 * i + 3
        t += [[a, c, b], [b, c, d]]
    return v, np.array(t, np.int32) + vid0


def _two_components(n1, n2):
    v1, t1 = _strip(n1)
    v2, t2 = _strip(n2, x0=1000.0, vid0=len(v1))
    v = np.concatenate([v1, v2])
    return M.TriangleMesh(v, np.concatenate([t1, t2]), np.tile(np.array([[0.2, 0.4, 0.6]], np.float32), (len(v), 1)))


def test_cluster_connected_triangles():
    m = _two_components(40, 30)
    lab, cnt = M.cluster_connected_triangles(m)
    assert sorted(cnt.tolist()) == [60, 80]
    assert len(set(lab[:80])) == 1 and len(set(lab[80:])) == 1 and lab[0] != lab[80]
    # sharing a vertex only is not a connection
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], np.float32)
    lab, cnt = M.cluster_connected_triangles(M.TriangleMesh(v, np.array([[0, 1, 2], [0, 3, 4]], np.int32)))
    assert len(cnt) == 2


def test_post_process_keeps_clusters():
    m = _two_components(40, 30)  # 80 and 60 triangles
    p1 = M.post_process_mesh(m, 1)
    assert len(p1.triangles) == 80 and len(p1.vertices) == 82
    assert np.array_equal(p1.vertices, m.vertices[:82]) and np.array_equal(p1.triangles, m.triangles[:80])
    p2 = M.post_process_mesh(m, 2)
    assert len(p2.triangles) == 140 and len(p2.vertices) == len(m.vertices)
    # the 50-triangle floor: a 60- and a 40-triangle component, keep 2 -> only the 60 stays
    m = _two_components(30, 20)
    p = M.post_process_mesh(m, 2)
    assert len(p.triangles) == 60 and len(p.vertices) == 62
    assert len(M.post_process_mesh(_two_components(10, 5), 1).triangles) == 0


def test_post_process_cleans_up():
    v, t = _strip(30)
    extra = np.array([[5.0, 5.0, 5.0]], np.float32)  # unreferenced
    v = np.concatenate([extra, v])
    t = t + 1
    t = np.concatenate([t, [[1, 1, 2]]]).astype(np.int32)  # degenerate, shares an edge with the strip
    m = M.TriangleMesh(v, t, np.zeros_like(v))
    p = M.post_process_mesh(m, 1)
    assert len(p.vertices) == 62 and np.array_equal(p.vertices, v[1:])
    assert len(p.triangles) == 60 and np.array_equal(p.triangles, t[:60] - 1)


def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    v = rng.normal(size=(100, 3)).astype(np.float32)
    c = rng.integers(0, 256, size=(100, 3)).astype(np.float32) / 255.0
    t = rng.integers(0, 100, size=(150, 3)).astype(np.int32)
    f = tmp_path / "m.ply"
    M.write_mesh(f, M.TriangleMesh(v, t, c))
    head = open(f, "rb").read(400)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n")
    r = M.read_mesh(f)
    assert np.array_equal(r.vertices, v) and np.array_equal(r.triangles, t)
    assert np.array_equal(np.rint(r.vertex_colors * 255), np.rint(c * 255))
    g = tmp_path / "m2.ply"
    M.write_mesh(g, r)
    assert open(f, "rb").read() == open(g, "rb").read()
    M.write_mesh(tmp_path / "e.ply", M.TriangleMesh())
    e = M.read_mesh(tmp_path / "e.ply")
    assert len(e.vertices) == 0 and len(e.triangles) == 0


def test_depth_quantisation():
    d = np.array([0.0, 0.0004, 0.0015, 1.23456, 2.9999, 65.535, 65.5359, 65.536, 70.0, -1.0], np.float32)
    q = M.quantize_depth_mm(torch.from_numpy(d)).numpy()
    ref = (d * 1000).astype(np.uint16).astype(np.float32) / np.float32(1000.0)  # the reference's uint16 step, read back
    keep = (d >= 0) & (d < 65.536)
    assert np.array_equal(q[keep], ref[keep])
    assert np.all(q[~keep] == 0)  # deliberate difference: dropped, not wrapped
    assert q[3] == np.float32(1234) / np.float32(1000)
