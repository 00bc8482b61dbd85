"""The float64 TSDF reference (tests/tsdf_ref.py) and the inputs of the TSDF kernel tests (tests/tsdf_inputs.py), checked on the
CPU: the fusion reference against the fp32 restatement (undecided-voxel cap, measured tolerances), the mesh invariants
against the restatement's marching cubes (accepted) and against corrupted meshes (rejected, invariant by invariant), and the
censuses: that every input holds the cases its GPU test is there for.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as R  # noqa: E402
import tsdf_inputs as I  # noqa: E402
import tsdf_ref as T  # noqa: E402

NTRI = (R.load_table() >= 0).sum(1) // 3


@pytest.fixture(scope="module")
def checkers():
    return {name: T.MeshChecker(make(), NTRI) for name, make in I.MC_VOLUMES.items()}


# ---- fusion ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fusion():
    vol, touched = I.fusion_reference()
    dom, views = I.fusion_scene()
    return vol, touched, views, T.fuse64(vol.coords, touched, views, I.VOX, I.TRUNC, I.FUSION_DEPTH_TRUNC)


def test_fusion_restatement_against_float64(fusion):
    vol, touched, views, r64 = fusion
    c = T.fusion_compare(r64, vol.tsdf, vol.weight, vol.color)
    print(c)
    assert c["n_decided"] > 20000
    assert c["undecided_fraction"] <= 0.005, c
    assert c["weight_equal"], "the fp32 restatement and float64 disagree on a decided voxel: DELTA is too small, or one is wrong"
    # the recorded measurements still hold (the tolerances are 4 x these)
    assert c["tsdf_err"] <= T.FUSION_TSDF_MEASURED and c["tsdf_err"] >= 0.5 * T.FUSION_TSDF_MEASURED, c
    assert c["color_err"] <= T.FUSION_COLOR_MEASURED and c["color_err"] >= 0.5 * T.FUSION_COLOR_MEASURED, c
    assert T.FUSION_TSDF_TOL == 4 * T.FUSION_TSDF_MEASURED and T.FUSION_COLOR_TOL == 4 * T.FUSION_COLOR_MEASURED


def test_fusion_census(fusion):
    vol, touched, views, r64 = fusion
    assert 3 <= len(views) <= 5
    for d, col, fx, fy, cx, cy, w2c in views:
        H, W = d.shape
        assert W % 4 and H % 4 and fx != fy and abs(cx - W / 2) > 1 and abs(cy - H / 2) > 1
        assert np.abs(w2c[:3, :3]).max() < 0.999, "an axis-aligned pose"
        assert (d == 0).sum() > 20 and max(W, H) < 100
    assert set(np.unique(views[2][1])) == {0.0, 255.0}
    d3 = views[3][0]
    assert d3[d3 > 0].max() < 16 * I.VOX and r64["straddle"][3] > 0, "no touched block straddles the camera plane"
    assert r64["u_lo"].sum() > 0 and r64["u_hi"].sum() > 0
    w = r64["weight"]
    assert w.max() == len(views) and (w == len(views)).sum() > 50 and (w == 1).sum() > 1000
    assert vol.ignored == 0 and all(len(t) > 0 for t in touched)


# ---- mesh invariants -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(I.MC_VOLUMES))
def test_invariants_accept_the_restatement(checkers, name):
    v, c, t = I.mc_reference(name)
    ck = checkers[name]
    ck.check(v, c, t)
    u = ck.position_units(v)
    measured = float(u.max()) if u.size else 0.0
    print(name, "position error", measured, "units of eps32 max(|coordinate|, voxel)")
    assert measured <= T.POSITION_MEASURED_UNITS
    assert T.POSITION_TOL_UNITS == max(T.POSITION_DERIVED_UNITS, 2 * T.POSITION_MEASURED_UNITS)


def test_position_measurement_is_current(checkers):
    worst = max(float(checkers[n].position_units(I.mc_reference(n)[0]).max()) for n in ("every_case", "sparse", "checkerboard"))
    assert 0.9 * T.POSITION_MEASURED_UNITS <= worst <= T.POSITION_MEASURED_UNITS


def _rejected(ck, which, v, c, t):
    with pytest.raises(T.MeshInvariantError) as e:
        getattr(ck, f"inv{which}")(v, c, t)
    assert e.value.which == which


@pytest.mark.parametrize("name", ["every_case", "sparse"])
def test_invariants_reject_corrupted_meshes(checkers, name):
    v, c, t = I.mc_reference(name)
    ck = checkers[name]
    rng = np.random.default_rng(1)
    F, V = len(t), len(v)
    # two vertex ids swapped in the triangles: a triangle leaves its cube (3)
    a, b = 17, V - 5
    sw = t.copy()
    sw[t == a], sw[t == b] = b, a
    _rejected(ck, 3, v, c, sw)
    # two vertices swapped in the arrays: off their crossings (2)
    v2, c2 = v.copy(), c.copy()
    v2[[a, b]], c2[[a, b]] = v[[b, a]], c[[b, a]]
    _rejected(ck, 2, v2, c2, t)
    # one triangle flipped: the wrong way round its faces (5); where a side is shared with a neighbour (inside the volume:
    # every side of the first and last triangle lies in the domain's outer faces), the two now run the same way (4)
    for k in (0, F // 3, F // 2, int(rng.integers(F // 4, 3 * F // 4)), F - 1):
        fl = t.copy()
        fl[k] = fl[k, ::-1]
        _rejected(ck, 5, v, c, fl)
        if 0 < k < F - 1:
            _rejected(ck, 4, v, c, fl)
        ck.inv3(v, c, fl)
    # every triangle flipped: consistent, closed, and inside out -- only the orientation rule sees it
    ck.inv4(v, c, t[:, ::-1])
    _rejected(ck, 5, v, c, t[:, ::-1])
    # one triangle dropped (3), and replaced by a copy of its neighbour so that the count still fits (3 or 4)
    _rejected(ck, 3, v, c, np.delete(t, F // 2, axis=0))
    dup = t.copy()
    dup[F // 2] = dup[F // 2 - 1]
    with pytest.raises(T.MeshInvariantError):
        ck.check(v, c, dup)
    # one vertex moved by voxel / 4, along each axis (2); a NaN (2); one colour off by 1 / 255 (2)
    for r in range(3):
        mv = v.copy()
        mv[V // 3, r] += np.float32(I.VOX / 4)
        _rejected(ck, 2, mv, c, t)
    nanv = v.copy()
    nanv[5, 1] = np.nan
    _rejected(ck, 2, nanv, c, t)
    cc = c.copy()
    cc[V // 2, 2] += np.float32(1 / 255)
    _rejected(ck, 2, v, cc, t)
    # one vertex more, and one never referenced (1)
    _rejected(ck, 1, np.concatenate([v, v[:1]]), np.concatenate([c, c[:1]]), t)
    un = t.copy()
    un[t == a] = b
    _rejected(ck, 1, v, c, un)
    # a position error of one more unit than allowed is caught, one of half the allowance is not
    k = int(np.argmax(np.abs(v[:, 0])))
    step = T.EPS32 * max(abs(float(v[k, 0])), I.VOX)
    far = v.astype(np.float64)
    far[k, 0] += (T.POSITION_TOL_UNITS + T.POSITION_MEASURED_UNITS + 1) * step
    _rejected(ck, 2, far, c, t)


# ---- censuses: marching cubes ----------------------------------------------------------------------------------------

def _edge_number(d, axis):
    """local edge descriptors (offset (.., 3), axis) -> the cube edge's number 0..11"""
    key = ((d[..., 0] * 2 + d[..., 1]) * 2 + d[..., 2]) * 3 + axis
    table = np.full(24, -1)
    for e, (x, y, z, a) in enumerate(T.CUBE_EDGES):
        table[((x * 2 + y) * 2 + z) * 3 + a] = e
    return table[key]


def test_census_every_case(checkers):
    ck = checkers["every_case"]
    vol = I.every_case_volume()
    assert vol.n == 27 and np.all(vol.weight == 1) and np.all(np.abs(vol.tsdf) > 0) and np.all(np.abs(vol.tsdf) <= 1)
    assert np.array_equal(np.unique(ck.c_case), np.arange(256)), "not all 256 cases among the valid cubes"
    v, c, t = I.mc_reference("every_case")
    cube = np.repeat(np.arange(len(ck.c_ntri)), ck.c_ntri)
    org = ck.c_pos[cube]
    cls = ((org % 16 == 15) * np.array([1, 2, 4])).sum(1)                         # position class of the cube
    e = _edge_number(ck.e_pos[t] - org[:, None, :], ck.e_axis[t])                 # (F, 3)
    seen = np.zeros((8, 12), bool)
    seen[np.repeat(cls, 3), e.reshape(-1)] = True
    assert seen.all(), f"position class x edge never referenced: {np.argwhere(~seen).tolist()}"
    mask = (ck.used * np.array([1, 2, 4])[:, None, None, None]).sum(0)            # used-edge mask per owner voxel
    x, y, z = np.nonzero(mask)
    ocls = (x % 16 == 15) * 1 + (y % 16 == 15) * 2 + (z % 16 == 15) * 4
    got = np.zeros((8, 8), bool)
    got[ocls, mask[x, y, z]] = True
    assert got[:, 1:].all(), f"owner class x mask missing: {np.argwhere(~got[:, 1:]).tolist()}"
    # the forced checkerboards: 4-triangle cubes whose origin is the last voxel of its block on all three axes
    corner = np.all(ck.c_pos % 16 == 15, axis=1)
    assert (ck.c_ntri[corner] == 4).sum() >= 4


def test_census_sparse(checkers):
    vol = I.sparse_volume()
    ck = checkers["sparse"]
    d0, nb = np.array(vol.dom[:3]), np.array(vol.dom[3:])
    present = ck.slot_of >= 0
    assert 0.25 <= 1 - present.mean() <= 0.45
    assert vol.coords.min() < 0
    lin = vol.linear(vol.coords)
    assert not np.array_equal(lin, np.sort(lin)), "slots in linear order"
    rel = vol.coords - d0
    for r in range(3):
        assert (rel[:, r] == 0).any() and (rel[:, r] == nb[r] - 1).any(), "no block on a domain face"
    for dirn in I.NEIGHBOUR_DIRS:
        q = rel + np.array(dirn)
        inside = np.all((q >= 0) & (q < nb), axis=1)
        assert (~present[tuple(q[inside].T)]).any(), f"no present block lacks its neighbour {dirn} inside the domain"
    assert 0 < (vol.weight == 0).mean() < 0.03 and (vol.weight > 1).any()
    v = np.arange(4096)
    assert np.all(vol.weight[5][v % 16 == 0] == 0), "the face layer of slot 5"
    # boundary mesh edges exist (invariant 4 says where), and so do closed ones
    _, _, t = I.mc_reference("sparse")
    a, b, cube, org, d1, d2, a1, a2, n_face, s_face = ck._sides(t)
    nn = np.maximum(n_face, 0)
    q = org + T.UNIT[nn] * s_face[:, None]
    below = q - T.UNIT[nn]
    vcp = np.pad(ck.vc, ((1, 0), (1, 0), (1, 0)))
    n_valid = ck.vc[tuple(q.T)].astype(int) + vcp[tuple((below + 1).T)]
    assert ((n_face >= 0) & (n_valid == 1)).sum() > 1000 and ((n_face >= 0) & (n_valid == 2)).sum() > 1000


def test_census_value_edges(checkers):
    vol = I.value_edges_volume()
    ck = checkers["value_edges"]
    nv, nt = ck.per_slot_counts()
    assert nv[0] > 1000 and nt[0] > 1000 and nv[1] == nv[2] == nt[1] == nt[2] == 0
    assert np.all(vol.tsdf[1] > 0) and np.all(vol.tsdf[2] < 0)
    f = ck.F[:16]
    bits = np.asarray(f, np.float32).view(np.uint32)
    for s in np.array(I.SPECIALS, np.float32).view(np.uint32):
        x, y, z = np.nonzero(bits[:15] == s)
        nxt = f[x + 1, y, z]
        assert (nxt < 0).any() and (nxt > 0).any(), f"special {s:#x} lacks a neighbour of one sign"
    # crossings between two specials, denormal pairs among them, are vertices of the mesh
    p, a = ck.e_pos, ck.e_axis
    q = p + T.UNIT[a]
    tiny = float(np.finfo(np.float32).tiny)
    f0, f1 = np.abs(ck.F[tuple(p.T)]), np.abs(ck.F[tuple(q.T)])
    assert ((f0 < tiny) & (f0 > 0) & (f1 < tiny) & (f1 > 0)).any(), "no vertex between two denormals"
    assert ((f0 == 0) & (f1 < tiny) & (f1 > 0)).any() and ((f1 == 0) & (f0 < tiny) & (f0 > 0)).any(), "no vertex between a zero and a denormal"
    _, _, t = ck.crossing()
    assert (t == 0).any() and (t == 1).any() and np.isfinite(t).all()


def test_census_counts(checkers):
    assert checkers["no_crossing"].n_vertices == 0 and checkers["no_crossing"].n_triangles == 0
    assert I.no_crossing_volume().n == 2
    nv, nt = checkers["checkerboard"].per_slot_counts()
    s = I.CHECKER_CENTRE_SLOT
    assert nv[s] == 3 * 4096 == 12288 and nt[s] == 4 * 4096 == 16384
    assert nv.max() == 12288 and nt.max() == 16384 and nv[s] < 2 ** 16 and nt[s] < 2 ** 16
    vol = I.checkerboard_volume()
    assert np.array_equal(vol.coords[s], np.array(vol.dom[:3]) + 1)
    big = I.big_pool_volume()
    nv, nt = checkers["big_pool"].per_slot_counts()
    assert big.n == I.BIG_POOL_BLOCKS > 512
    live = np.zeros(big.n, bool)
    live[list(I.BIG_POOL_LIVE)] = True
    assert np.all(nv[live] > 1000) and np.all(nt[live] > 1000) and np.all(nv[~live] == 0) and np.all(nt[~live] == 0)
    assert np.all((big.weight > 0).any(1) == live)


# ---- censuses: touch and the AABB ------------------------------------------------------------------------------------

def test_census_touch_multichunk():
    N = I.MC_N
    assert N > 262144 and N % 1024 and (N + 1023) // 1024 > 256
    ref = I.touch_multichunk_reference()
    lins = [set(r["linear"].tolist()) for r in ref]
    assert 0 in lins[0] and N - 1 in lins[1]
    assert {262143, 262144} <= lins[2] and 262143 // 1024 == 255 and 262144 // 1024 == 256
    assert {49703, 49704} <= lins[3] and 49703 % 4 == 3 and 49703 // 1024 == 49704 // 1024
    last = (N - 1) // 1024
    for r in ref:
        ch = r["linear"] // 1024
        assert (ch < 256).sum() > 0 and (ch >= 256).sum() > 0, "a view without touched blocks on both loop trips of the scan"
        assert len(np.unique(ch)) > 20 and r["ignored"] > 0
    assert any((r["linear"] // 1024 == 0).any() for r in ref) and any((r["linear"] // 1024 == last).any() for r in ref)
    assert all(r["new"] > 0 for r in ref)
    assert 0 < ref[4]["new"] < len(ref[4]["slots"]), "the last view is neither part old nor part new"
    assert ref[-1]["n"] < 2000


def test_census_touch_rejection():
    cases = I.touch_rejection_cases()
    for axis in range(3):
        dt, view, _ = cases[f"box_axis{axis}"]
        vol, slots = I.touch_reference(I.REJ_DOM, dt, view)
        got = vol.coords[slots][:, axis]
        assert got.min() == 0 and got.max() == 2 and vol.ignored >= 3
        d = view[0][0, ::4]
        tr = np.float32(I.TRUNC)
        assert d[0] - tr == 0 and d[1] - tr < 0
    dt, view, _ = cases["depth_values"]
    vol, slots = I.touch_reference(I.REJ_DOM, dt, view)
    d = view[0][0, ::4]
    assert np.isnan(d).any() and np.isposinf(d).any() and (d < 0).any() and (d == 0).any()
    assert (d == np.float32(dt)).any() and (d == np.nextafter(np.float32(dt), np.float32(1))).any()
    assert vol.ignored == 0 and len(slots) == 3      # 0.3 (block 1), just below it, 0.1 (block 0): each with its neighbours' share
    for name in ("pose_1e30", "pose_inf", "pose_nan", "pose_nan_rotation"):
        dt, view, n_valid = cases[name]
        vol, slots = I.touch_reference(I.REJ_DOM, dt, view)
        assert n_valid > 10 and vol.ignored == n_valid and len(slots) == 0 and vol.n == 0
    dt, view, _ = cases["pose_good"]
    vol, slots = I.touch_reference(I.REJ_DOM, dt, view)
    assert len(slots) > 5


def test_census_aabb():
    cases = I.aabb_cases()
    assert [c[1][0][0].shape[::-1] for c in (cases["1x1"], cases["61x47"], cases["257x130"])] == [(1, 1), (61, 47), (257, 130)]
    assert I.aabb_expected(*cases["all_invalid"]) == (None, None)
    lo, hi = I.aabb_expected(*cases["signed_zeros"])
    assert lo[0] == 0 and np.signbit(lo[0]) and hi[0] == 0 and not np.signbit(hi[0]) and lo[1] < 0 and hi[2] < 0
    d = cases["last_pixel"][1][0][0]
    n = ((d.shape[1] + 3) // 4) * ((d.shape[0] + 3) // 4)
    assert n % 256 and (d[::4, ::4] > 0).sum() == 1 and d[::4, ::4].reshape(-1)[-1] > 0
    assert len(cases["two_views"][1]) >= 2
    lo1, hi1 = I.aabb_expected(*cases["61x47"])
    lo2, hi2 = I.aabb_expected(*cases["two_views"])
    assert np.any(lo2 < lo1) and np.any(hi2 > hi1)
    assert (cases["61x47"][1][0][0] > cases["61x47"][0]).any(), "no depth beyond depth_trunc"
