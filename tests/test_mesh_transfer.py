"""The closest-hit and detail-transfer contracts without a GPU (include/gs2m_meshao.h: Candidate, Facing, Answer;
include/gs2m_meshtransfer.h): the numpy restatement of tests/mesh_transfer_ref.py held to things known independently -- hand-worked
dyadic cases, the index rule at shared edges and vertices, the agreement with the any-hit restatement -- the balance of the cases
the GPU tests rely on, and the new entries of the binding table."""
import ctypes
import os

import numpy as np
import pytest

import mesh_ao_ref as A
import mesh_transfer_ref as R

TRI = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[0, 1, 2]], np.int32))
DOWN = [0.0, 0.0, -1.0]


def _one(mesh, o, d, **kw):
    tri, t, uv, _ = R.closest(*mesh, [o], [d], **kw)
    return int(tri[0]), float(t[0]), float(uv[0, 0]), float(uv[0, 1])


def test_dyadic_plane_by_hand():
    # T = o - a = (0.25, 0.5, 2); d = -z: P = d x e2 = (1, 0, 0), det = 1, u = 0.25; Q = T x e1 = (0, 2, -0.5), v = 0.5, t = 2
    assert _one(TRI, [0.25, 0.5, 2.0], DOWN) == (0, 2.0, 0.25, 0.5)
    assert _one(TRI, [0.25, 0.5, 2.0], [0.0, 0.0, -4.0]) == (0, 0.5, 0.25, 0.5)          # t scales with 1 / |d|, u and v do not
    assert _one(TRI, [0.25, 0.5, -8.0], [0.0, 0.0, 1.0]) == (0, 8.0, 0.25, 0.5)          # from below: det = -1
    assert _one(TRI, [1.0, 0.0, 1.0], DOWN) == (0, 1.0, 1.0, 0.0) and _one(TRI, [0.0, 1.0, 1.0], DOWN) == (0, 1.0, 0.0, 1.0)
    assert _one(TRI, [0.75, 0.5, 2.0], DOWN) == (-1, np.inf, 0.0, 0.0)                   # u + v > 1: the miss values
    assert _one(TRI, [0.25, 0.5, 2.0], [0.0, 0.0, 1.0]) == (-1, np.inf, 0.0, 0.0)        # behind the origin


def test_range_is_closed_at_both_ends():
    assert _one(TRI, [0.25, 0.5, 0.0], DOWN) == (0, 0.0, 0.25, 0.5)                      # on the surface: t == tmin == 0 is found
    assert _one(TRI, [0.25, 0.5, 2.0], DOWN, tmin=2.0)[0] == 0 and _one(TRI, [0.25, 0.5, 2.0], DOWN, tmax=2.0)[0] == 0
    assert _one(TRI, [0.25, 0.5, 2.0], DOWN, tmin=2.0, tmax=2.0) == (0, 2.0, 0.25, 0.5)
    assert _one(TRI, [0.25, 0.5, 2.0], DOWN, tmin=np.nextafter(2.0, 3.0))[0] == -1
    assert _one(TRI, [0.25, 0.5, 2.0], DOWN, tmax=np.nextafter(2.0, 0.0))[0] == -1
    # the any-hit predicate stays open at tmin
    assert not A.occluded(*TRI, [[0.25, 0.5, 0.0]], [DOWN])[0] and A.occluded(*TRI, [[0.25, 0.5, 2.0]], [DOWN], 0.0, 2.0)[0]


def test_facing_by_hand_and_as_a_partition():
    # cross(e1, e2) of TRI is +z; a ray coming down meets that side: det = -dot(d, +z) = 1 > 0
    assert _one(TRI, [0.25, 0.5, 2.0], DOWN, facing=1)[0] == 0 and _one(TRI, [0.25, 0.5, 2.0], DOWN, facing=-1)[0] == -1
    assert _one(TRI, [0.25, 0.5, -2.0], [0, 0, 1.0], facing=-1)[0] == 0 and _one(TRI, [0.25, 0.5, -2.0], [0, 0, 1.0], facing=1)[0] == -1
    with pytest.raises(ValueError):
        R.closest(*TRI, [[0, 0, 1.0]], [DOWN], facing=2)
    # the height field is wound consistently, cross(e1, e2) to +z
    v, f = A.height_field()
    p = v[f]
    assert (A.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])[:, 2] > 0).all()
    r = A.ray_family("random", v, f, 600)
    ok, t, u, w, det = R.triangle_table(v, f, r["origins"], r["dirs"])
    both, front, back = (R.select(ok, det, None, s) for s in (0, 1, -1))
    assert np.array_equal(front | back, both) and not (front & back).any() and front.any() and back.any()
    a0, a1, a2 = (R.answer(x, t, u, w) for x in (both, front, back))
    assert np.array_equal(a0[1], np.minimum(a1[1], a2[1])) and 0.1 < (a0[0] >= 0).mean() < 0.9
    first = np.where((a1[1] < a2[1]) | ((a1[1] == a2[1]) & ((a1[0] < a2[0]) | (a2[0] < 0))), a1[0], a2[0])
    assert np.array_equal(a0[0], first)
    # a front candidate is met against its normal cross(e1, e2), a back one along it
    along = r["dirs"] @ A.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).T
    assert (along[front] < 0).all() and (along[back] > 0).all()


def test_shared_edges_and_vertices_return_the_smaller_index():
    v, f = A.grid_mesh()
    floor = f[:128]                                               # the floor's triangles come first: indices 0 .. 127
    corner = lambda i, j: i * 9 + j
    # onto the lattice vertex (2, 2) / 8: six floor triangles meet there
    at = np.nonzero((floor == corner(2, 2)).any(1))[0]
    tri, t, uv, ties = R.closest(v, f, [[0.25, 0.25, 1.0]], [DOWN])
    assert len(at) == 6 and ties[0] == 6 and tri[0] == at.min() and t[0] == 0.5
    # onto the middle of the edge (2, 2) - (3, 2), of the edge (2, 2) - (2, 3) and of the diagonal (3, 2) - (2, 3)
    for (a, b), o in ((((2, 2), (3, 2)), [0.3125, 0.25, 1.0]), (((2, 2), (2, 3)), [0.25, 0.3125, 1.0]), (((3, 2), (2, 3)), [0.3125, 0.3125, 1.0])):
        share = np.nonzero((floor == corner(*a)).any(1) & (floor == corner(*b)).any(1))[0]
        tri, t, uv, ties = R.closest(v, f, [o], [DOWN])
        assert len(share) == 2 and ties[0] == 2 and tri[0] == share.min() and t[0] == 0.5
        assert R.closest(v, f, [o], [DOWN], skip=[share.min()])[0][0] == share.max()
    # two coplanar layers: the twin has the larger index
    lv, lf = R.layered_grid()
    r = R.tie_family(1000)
    tri, t, uv, ties = R.closest(lv, lf, r["origins"], r["dirs"])
    assert (ties[tri >= 0] >= 2).all() and (tri < len(f)).all() and 0.1 <= (tri >= 0).mean() <= 0.9
    assert np.array_equal(tri, R.closest(v, f, r["origins"], r["dirs"])[0])
    assert (R.closest(v, f, r["origins"], r["dirs"])[3] >= 2).sum() >= 100          # what the GPU tie test relies on


def test_identical_triangles_skip_nan_and_dead():
    v, f = A.identical_mesh()
    r = A.ray_family("random", v, f, 200)
    tri, t, uv, ties = R.closest(v, f, r["origins"], r["dirs"])
    hit = tri >= 0
    assert hit.any() and (~hit).any() and (tri[hit] == 0).all() and (ties[hit] == 257).all()
    again = R.closest(v, f, r["origins"], r["dirs"], skip=np.zeros(200, np.int32))
    assert np.array_equal(again[0] >= 0, hit) and (again[0][hit] == 1).all() and np.array_equal(again[1], t) and np.array_equal(again[2], uv)
    # a NaN anywhere in the ray: a miss with the miss values
    o, d = r["origins"].copy(), r["dirs"].copy()
    o[::2, 0], d[1::2, 2] = np.nan, np.nan
    tri, t, uv, _ = R.closest(v, f, o, d)
    assert (tri == -1).all() and np.isposinf(t).all() and (uv == 0).all()
    # dead triangles only, and none at all
    vd = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 1, 0]])
    fd = np.array([[0, 1, 2], [0, 1, 5], [-1, 0, 1], [0, 0, 1]], np.int32)
    for mesh in ((vd, fd), (vd, fd[:0]), A.random_mesh(0)):
        tri, t, uv, _ = R.closest(*mesh, r["origins"], r["dirs"])
        assert (tri == -1).all() and np.isposinf(t).all() and (uv == 0).all()
    # the dead among the live are never the answer
    v, f = A.dead_mesh()
    r = A.ray_family("random", v, f, 300)
    tri = R.closest(v, f, r["origins"], r["dirs"])[0]
    assert A.live_triangles(v, f)[tri[tri >= 0]].all() and (tri >= 0).any()


@pytest.mark.parametrize("mesh", ["n3", "n65", "dead100", "grid"])
def test_hit_mask_equals_the_any_hit_restatement(mesh):
    """Closest-hit and any-hit differ only at t == tmin: wherever no candidate sits there, `tri >= 0` is `occluded`; and the
    answer is the least (t, index) of the any-hit matrix's true entries"""
    v, f = A.MESHES[mesh]()
    families = [A.ray_family(k, v, f, 300) for k in A.FAMILIES] + ([A.grid_family(k, 300) for k in A.GRID_FAMILIES] if mesh == "grid" else [])
    for r in families:
        ok, t, u, w, det = R.triangle_table(v, f, r["origins"], r["dirs"], r["tmin"], r["tmax"])
        sel = R.select(ok, det, r["skip"], 0)
        tri = R.answer(sel, t, u, w)[0]
        clear = ~(sel & (t == r["tmin"])).any(1)
        want = A.occluded(v, f, r["origins"], r["dirs"], r["tmin"], r["tmax"], r["skip"])
        assert clear.sum() >= 250 and np.array_equal((tri >= 0)[clear], want[clear])
        m = A.hit_matrix(v, f, r["origins"], r["dirs"], r["tmin"], r["tmax"])
        assert np.array_equal(m[clear], ok[clear])


def test_balanced_cases_hold_their_bound():
    """Every entry of R.BALANCED -- the cases the GPU equality test runs -- has, under the restatement alone, a hit share of
    0.1 .. 0.9; every mesh has entries for each facing, without and (but n1, which has no second triangle) with a skip list"""
    for name in A.MESHES:
        if name == "n0":
            continue
        v, f = A.MESHES[name]()
        rays = {k: A.ray_family(k, v, f, 1000) for k in A.FAMILIES if not (name == "n1" and k == "skip")}
        if name == "grid":
            rays.update({k: A.grid_family(k, 1000) for k in A.GRID_FAMILIES})
        tables = {}
        for facing in (0, 1, -1):
            for with_skip in (False, True):
                families = R.BALANCED.get((name, facing, with_skip), ())
                assert families or (with_skip and name in ("n1", "n2", "n3")), (name, facing, with_skip)
                for k in families:
                    if k not in tables:
                        tables[k] = R.triangle_table(v, f, rays[k]["origins"], rays[k]["dirs"], rays[k]["tmin"], rays[k]["tmax"])
                    ok, t, u, w, det = tables[k]
                    skip = R.nearest_skip(rays[k], R.answer(ok, t, u, w)[0]) if with_skip else None
                    share = (R.answer(R.select(ok, det, skip, facing), t, u, w)[0] >= 0).mean()
                    assert 0.1 <= share <= 0.9, (name, k, facing, with_skip, share)
    assert {k for fam in R.BALANCED.values() for k in fam} == set(A.FAMILIES) | set(A.GRID_FAMILIES)


def _planes():
    """two unit squares wound to +z, the LOWER one (z = -0.25) first, and five attributes that are dyadic at the corners"""
    v = np.array([[0, 0, -0.25], [1, 0, -0.25], [1, 1, -0.25], [0, 1, -0.25], [0, 0, 0.25], [1, 0, 0.25], [1, 1, 0.25], [0, 1, 0.25]], np.float64)
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    att = (np.arange(40, dtype=np.float32).reshape(8, 5) + 0.5) / 64.0
    return v, f, att


def test_transfer_choice_and_values_by_hand():
    v, f, att = _planes()
    up = [0.0, 0.0, 1.0]
    pts = np.array([[0.75, 0.25, 0.0], [0.75, 0.25, 0.125], [0.75, 0.25, -0.125], [0.75, 0.25, 0.5], [0.75, 0.25, 0.25], [0.25, 0.5, 0.0]])
    fill = np.full((6, 9), 7.0, np.float32)
    out, hit, off, oc = R.transfer(v, f, pts, [up] * 6, None, 0.3, False, fill, att, None, True)
    # equal distances: the forward ray wins, though the lower plane has the smaller indices
    assert hit.tolist() == [2, 2, 0, 2, 2, 3] and off.tolist() == [0.25, 0.125, -0.125, -0.25, 0.0, 0.25] and oc.tolist() == [2, 2, 3, 3, 2, 2]
    # triangle 2 = (4, 5, 6) at (0.75, 0.25): u = 0.5 (towards corner 5), v = 0.25 (towards 6), w = 0.25
    want = (np.float64(0.25) * att[4].astype(np.float64) + 0.5 * att[5].astype(np.float64)) + 0.25 * att[6].astype(np.float64)
    assert np.array_equal(out[0, :5], want.astype(np.float32)) and np.array_equal(out[0, 5:8], np.array([0, 0, 1], np.float32))
    assert (out[:, 8] == 7).all()                                                    # beyond channels + 3: left alone
    # skipped and missing points keep their row
    own = np.array([0, -1, 3, 0, 0, 0], np.int32)
    nrm = np.array([up, up, up, [0, 0, 0], [np.nan, 0, 1], up])
    pts2 = pts.copy()
    pts2[5, 1] = np.inf
    out, hit, off, oc = R.transfer(v, f, pts2, nrm, own, 0.3, False, fill, att, None, True)
    assert oc.tolist() == [2, 0, 3, 0, 0, 0] and hit.tolist() == [2, -1, 0, -1, -1, -1] and (out[[1, 3, 4, 5]] == 7).all() and (off[[1, 3, 4, 5]] == 0).all()
    out, hit, off, oc = R.transfer(v, f, pts, [up] * 6, None, 0.0625, False, fill, att, None, True)
    assert oc.tolist() == [1, 1, 1, 1, 2, 1] and (out[[0, 1, 2, 3, 5]] == 7).all() and (off == 0).all()
    # one-sided: from above the upper plane, looking down the -n ray, its +z side counts; a flipped source counts for neither ray
    flipped = f[:, [0, 2, 1]]
    assert (R.transfer(v, flipped, pts, [up] * 6, None, 0.3, False, fill, att)[1] == -1).all()
    out2, hit2, off2, _ = R.transfer(v, flipped, pts, [up] * 6, None, 0.3, True, fill, att, None, True)
    assert hit2.tolist() == [2, 2, 0, 2, 2, 3] and np.array_equal(out2[0, 5:8], np.array([0, 0, -1], np.float32))
    # smooth normals are interpolated like the attributes and not normalised
    sn = np.arange(24, dtype=np.float64).reshape(8, 3) / 8.0
    out3 = R.transfer(v, f, pts, [up] * 6, None, 0.3, False, fill, None, sn, True)[0]
    assert np.array_equal(out3[0, :3], ((0.25 * sn[4] + 0.5 * sn[5]) + 0.25 * sn[6]).astype(np.float32)) and (out3[:, 3:] == 7).all()


def test_transfer_scene_has_every_outcome():
    """the scene of the GPU transfer test, sampled: at least a tenth forward, backward and missing, one-sided and with half of the
    source flipped"""
    v, f = A.height_field()
    pts, nrm = R.tilted_plane_samples(600)
    fill = np.zeros((600, 3), np.float32)
    oc = R.transfer(v, f, pts, nrm, None, R.TRANSFER_DISTANCE, False, fill, None, None, True)[3]
    assert (np.bincount(oc, minlength=4)[1:] >= 60).all()
    half = R.half_flipped(f)
    one = R.transfer(v, half, pts, nrm, None, R.TRANSFER_DISTANCE, False, fill, None, None, True)
    two = R.transfer(v, half, pts, nrm, None, R.TRANSFER_DISTANCE, True, fill, None, None, True)
    assert (np.bincount(one[3], minlength=4)[1:] >= 60).all() and np.array_equal(two[3], oc) and not np.array_equal(one[1], two[1])


def test_signatures_and_exports():
    import gs2m_native as N
    for name, n_args in (("gs2m_bvh_closest", 17), ("gs2m_mesh_transfer", 21)):
        restype, argtypes = N.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == n_args and argtypes[-1] is N.STREAM and name in N.EXPORTS
    if not os.path.exists(N.LIB_PATH):
        N.build()
    lib = ctypes.CDLL(N.LIB_PATH)
    assert hasattr(lib, "gs2m_bvh_closest") and hasattr(lib, "gs2m_mesh_transfer")
