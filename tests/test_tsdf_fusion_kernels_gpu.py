"""The TSDF fusion kernels of csrc/tsdf.hip alone, through their C entry points (gs2m_tsdf_points_aabb, _touch, _integrate)
on buffers the test owns, every one between guard words.

  points_aabb   the decoded keys against the fp32 min / max of the restatement's points, bit for bit: 1 x 1, partial
                workgroups, no valid pixel, signed zeros, several views into one key array
  touch         a 70 x 70 x 61 domain (292 chunks of 1024 blocks, the last of 916: two loop trips of the chunk scan and a
                ragged end), five views on one pool: slot lists, block coordinates, the whole index table, the counts, the
                marks left zero -- all equal to tests/mesh_ref.py; truncation boxes ending on the domain's first and last
                block, poses of 1e30 / inf / NaN, every kind of invalid depth; the pool-full contract
  integrate     four views under general poses: bit-identical to the fp32 restatement on every voxel, and within the
                tolerances of tests/tsdf_ref.py of the independent float64 fusion on the decided ones
The inputs (tests/tsdf_inputs.py) are checked on the CPU by tests/test_tsdf_ref.py: what they contain, and that the
restatement itself meets the float64 reference."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gs2m_mesh as M  # noqa: E402
import gs2m_native as N  # noqa: E402
import tsdf_inputs as I  # noqa: E402
import tsdf_ref as T  # noqa: E402
from tsdf_gpu_buffers import DEV, SENTINEL, Guarded, Pool, bits  # noqa: E402

pytestmark = pytest.mark.gpu

KEY_INIT = np.array([2 ** 31 - 1] * 3 + [-2 ** 31] * 3, np.int32)


# ---- points_aabb -----------------------------------------------------------------------------------------------------

def _decode(k):
    """as gs2m_mesh._depth_aabb decodes the keys"""
    if k[0] > k[3]:
        return None, None
    b = np.where(k >= 0, k, k ^ np.int32(0x7FFFFFFF)).astype(np.int32)
    f = b.view(np.float32)
    return f[:3], f[3:]


@pytest.mark.parametrize("name", list(I.aabb_cases()))
def test_points_aabb(name):
    depth_trunc, views = I.aabb_cases()[name]
    key = Guarded(KEY_INIT)
    held = []
    for depth, fx, fy, cx, cy, c2w in views:
        d = Guarded(np.asarray(depth, np.float32))
        held.append(d)
        H, W = depth.shape
        N.launch("gs2m_tsdf_points_aabb", DEV, W, H, d.ptr, float(np.float32(depth_trunc)), *(float(np.float32(x)) for x in (fx, fy, cx, cy)),
                 M._host_mat(c2w), key.ptr)
    k = key.host()
    assert key.guards_intact() and all(d.unchanged() for d in held)
    lo, hi = _decode(k)
    want_lo, want_hi = I.aabb_expected(depth_trunc, views)
    if want_lo is None:
        assert lo is None and np.array_equal(k, KEY_INIT), "keys moved off the sentinels without a valid pixel"
        return
    assert lo is not None
    assert np.array_equal(bits(lo), bits(want_lo)) and np.array_equal(bits(hi), bits(want_hi)), (lo, want_lo, hi, want_hi)


def _as_view(depth, fx, fy, cx, cy, w2c):
    v = types.SimpleNamespace(Fx=fx, Fy=fy, Cx=cx, Cy=cy)
    v.world_view_transform = torch.from_numpy(np.asarray(w2c, np.float32)).T.contiguous()
    return torch.from_numpy(depth).to(DEV), v


def test_depth_aabb_host_decode():
    """gs2m_mesh._depth_aabb itself: (None, None) without a valid pixel, else the restatement's box."""
    w2c = I.look_at((0.3, -0.2, -0.4), (0.0, 0.1, 1.0), 0.4)
    rng = np.random.default_rng(2)
    depths = [I._general_depth(rng, 61, 47), I._general_depth(rng, 30, 21)]
    pairs = [_as_view(d, 70.0, 64.0, 28.3, 25.1, w2c) for d in depths]
    lo, hi = M._depth_aabb([p[0] for p in pairs], [p[1] for p in pairs], 2.5, DEV)
    want_lo, want_hi = I.aabb_expected(2.5, [(d, 70.0, 64.0, 28.3, 25.1, M.c2w_of(w2c)) for d in depths])
    assert np.array_equal(lo, want_lo.astype(np.float64)) and np.array_equal(hi, want_hi.astype(np.float64))
    none = [_as_view(np.zeros((47, 61), np.float32), 70.0, 64.0, 28.3, 25.1, w2c)]
    assert M._depth_aabb([none[0][0]], [none[0][1]], 2.5, DEV) == (None, None)


# ---- touch -----------------------------------------------------------------------------------------------------------

def _check_touch(pool, rc, info, want_slots, want_n, want_new, want_ignored, want_coords, want_index, what):
    assert rc == 0, what
    assert info.tolist() == [want_n, len(want_slots), want_new, want_ignored], what
    touched = pool.touched.host()
    assert np.array_equal(touched[:len(want_slots)], want_slots), f"{what}: touched-slot list or its order"
    assert np.all(touched[len(want_slots):] == SENTINEL), f"{what}: touched-slot list written past its end"
    coords = pool.coords.host()
    assert np.array_equal(coords[:want_n], want_coords), f"{what}: block coordinates / new-slot order"
    assert not coords[want_n:].any(), f"{what}: coordinates written past the blocks in use"
    assert np.array_equal(pool.index.host(), want_index), f"{what}: index table"
    assert pool.state.host().tolist() == [want_n, 0, 0, 0], what
    assert not pool.flags().any(), f"{what}: marks left set"
    assert pool.guards_intact(), f"{what}: guard words written"


def test_touch_multichunk():
    ref = I.touch_multichunk_reference()
    pool = Pool(I.MC_DOM, ref[-1]["n"], I.VOX, I.TRUNC, I.MC_DEPTH_TRUNC)
    ignored = 0
    for k, (view, r) in enumerate(zip(I.touch_multichunk_views(), ref)):
        pool.touched = Guarded(np.full(pool.capacity, SENTINEL, np.int32))
        rc, info = pool.touch(view)
        _check_touch(pool, rc, info, r["slots"], r["n"], r["new"], r["ignored"] - ignored, r["coords"], r["index"], f"view {k}")
        ignored = r["ignored"]


@pytest.mark.parametrize("name", list(I.touch_rejection_cases()))
def test_touch_rejection(name):
    depth_trunc, view, n_valid = I.touch_rejection_cases()[name]
    vol, slots = I.touch_reference(I.REJ_DOM, depth_trunc, view)
    pool = Pool(I.REJ_DOM, 27, I.VOX, I.TRUNC, depth_trunc)
    rc, info = pool.touch(view)
    _check_touch(pool, rc, info, slots, vol.n, vol.n, vol.ignored, vol.coords, vol.index, name)
    if n_valid is not None:  # a pose of 1e30, inf or NaN: every valid pixel is ignored, nothing is marked
        assert info.tolist() == [0, 0, 0, n_valid]
        assert np.all(pool.index.host() == -1)


def test_touch_pool_full_writes_nothing():
    ref = I.touch_multichunk_reference()
    views = I.touch_multichunk_views()
    need = ref[1]["n"]
    pool = Pool(I.MC_DOM, need - 1, I.VOX, I.TRUNC, I.MC_DEPTH_TRUNC)
    # capacity equal to the need of the first view alone would do for it
    exact = Pool(I.MC_DOM, ref[0]["n"], I.VOX, I.TRUNC, I.MC_DEPTH_TRUNC)
    rc, info = exact.touch(views[0])
    _check_touch(exact, rc, info, ref[0]["slots"], ref[0]["n"], ref[0]["new"], ref[0]["ignored"], ref[0]["coords"], ref[0]["index"], "capacity == need")
    rc, info = pool.touch(views[0])
    assert rc == 0
    snap = [g.host() for g in (pool.index, pool.coords, pool.touched, pool.state)]
    rc, info = pool.touch(views[1])  # one block short
    assert rc == M.POOL_FULL
    assert info[0] == need and info[3] == ref[1]["ignored"] - ref[0]["ignored"]
    for g, before, what in zip((pool.index, pool.coords, pool.touched, pool.state), snap, ("index", "block_coords", "touched_slots", "state")):
        assert np.array_equal(g.host(), before), f"pool full: {what} was written"
    assert not pool.flags().any(), "pool full: marks left set"
    assert pool.guards_intact()
    # one block too few by a single one on an empty pool as well
    tiny = Pool(I.MC_DOM, ref[0]["n"] - 1, I.VOX, I.TRUNC, I.MC_DEPTH_TRUNC)
    rc, info = tiny.touch(views[0])
    assert rc == M.POOL_FULL and info[0] == ref[0]["n"]
    assert np.all(tiny.index.host() == -1) and not tiny.coords.host().any() and tiny.state.host().tolist() == [0, 0, 0, 0]
    assert np.all(tiny.touched.host() == SENTINEL) and not tiny.flags().any() and tiny.guards_intact()
    # the repeat with enough room gives what a pool that was large enough from the start gives
    pool.grow(need)
    rc, info = pool.touch(views[1])
    r = ref[1]
    _check_touch(pool, rc, info, r["slots"], r["n"], r["new"], r["ignored"] - ref[0]["ignored"], r["coords"], r["index"], "repeat after growing")


# ---- integrate -------------------------------------------------------------------------------------------------------

def test_integrate_against_float64_and_restatement():
    dom, views = I.fusion_scene()
    vol, touched = I.fusion_reference()
    pool = Pool(dom, vol.n, I.VOX, I.TRUNC, I.FUSION_DEPTH_TRUNC, with_voxels=True)
    for k, (depth, col, fx, fy, cx, cy, w2c) in enumerate(views):
        view = (depth, fx, fy, cx, cy, M.c2w_of(w2c))
        pool.touched = Guarded(np.full(pool.capacity, SENTINEL, np.int32))
        rc, info = pool.touch(view)
        assert rc == 0 and info[1] == len(touched[k]) and info[3] == 0
        assert np.array_equal(pool.touched.host()[:info[1]], touched[k]), f"view {k}: touched slots"
        pool.integrate(view, col, w2c, int(info[1]))
        assert pool.image.unchanged()
    torch.cuda.synchronize()
    assert pool.guards_intact()
    tsdf, weight, color = pool.tsdf.host(), pool.weight.host(), pool.color.host()
    assert np.array_equal(pool.coords.host(), vol.coords)
    # every voxel, bit for bit, against the fp32 restatement
    assert np.array_equal(weight, vol.weight), f"{(weight != vol.weight).sum()} weights differ from the restatement"
    assert np.array_equal(bits(tsdf), bits(vol.tsdf)), f"tsdf differs from the restatement, max {np.abs(tsdf - vol.tsdf).max()}"
    assert np.array_equal(bits(color), bits(vol.color)), f"colour differs from the restatement, max {np.abs(color - vol.color).max()}"
    # decided voxels against the independent float64 fusion
    r64 = T.fuse64(vol.coords, touched, views, I.VOX, I.TRUNC, I.FUSION_DEPTH_TRUNC)
    c = T.fusion_compare(r64, tsdf, weight, color)
    print(c)
    assert c["undecided_fraction"] <= 0.005 and c["n_decided"] > 20000
    assert c["weight_equal"], "a decided voxel's weight is not the float64 reference's count"
    assert c["tsdf_err"] <= T.FUSION_TSDF_TOL, c
    assert c["color_err"] <= T.FUSION_COLOR_TOL, c


# ---- argument validation (the returns tests/test_cabi.py does not cover) ---------------------------------------------------

def test_argument_validation():
    L, INVALID = N.lib(), -1
    s = N.stream_ptr(DEV)
    buf = torch.zeros(4096, dtype=torch.int32, device=DEV)
    p = buf.data_ptr()
    good, bad = (C.c_int * 6)(0, 0, 0, 2, 2, 2), (C.c_int * 6)(0, 0, 0, 2, 0, 2)
    eye = M._host_mat(np.eye(4))
    info = (C.c_int * 4)()
    ll2 = (C.c_longlong * 2)(5, 5)
    tb = C.c_longlong()
    assert L.gs2m_tsdf_workspace_bytes(bad, 0, C.byref(tb), None) == INVALID
    assert L.gs2m_tsdf_workspace_bytes(None, 0, C.byref(tb), None) == INVALID
    assert L.gs2m_tsdf_workspace_bytes(good, -1, C.byref(tb), None) == INVALID
    assert L.gs2m_tsdf_workspace_bytes(good, 0, None, None) == 0
    aabb = lambda W=4, H=4, depth=p, c=eye, key=p: L.gs2m_tsdf_points_aabb(W, H, depth, 1.0, 1.0, 1.0, 0.0, 0.0, c, key, s)  # noqa: E731
    assert [aabb(W=0), aabb(H=-1), aabb(depth=None), aabb(c=None), aabb(key=None)] == [INVALID] * 5

    def touch(dom=good, voxel=0.01, trunc=0.04, W=4, H=4, depth=p, c=eye, cap=4, state=p, index=p, coords=p, touched=p, ws=p, inf=info):
        return L.gs2m_tsdf_touch(dom, voxel, trunc, W, H, depth, 1.0, 1.0, 1.0, 0.0, 0.0, c, cap, state, index, coords, touched, ws, inf, s)
    got = [touch(dom=bad), touch(dom=None), touch(voxel=0.0), touch(voxel=float("nan")), touch(trunc=0.0), touch(trunc=-1.0), touch(W=0),
           touch(H=0), touch(depth=None), touch(c=None), touch(cap=-1), touch(state=None), touch(index=None), touch(coords=None),
           touch(touched=None), touch(ws=None), touch(inf=None)]
    assert got == [INVALID] * len(got), got

    def integ(voxel=0.01, trunc=0.04, W=4, H=4, depth=p, color=p, w=eye, n=1, touched=p, coords=p, tsdf=p, weight=p, acc=p):
        return L.gs2m_tsdf_integrate(voxel, trunc, W, H, depth, color, 1.0, 1.0, 1.0, 0.0, 0.0, w, n, touched, coords, tsdf, weight, acc, s)
    got = [integ(voxel=0.0), integ(trunc=float("nan")), integ(W=0), integ(H=0), integ(depth=None), integ(color=None), integ(w=None),
           integ(n=-1), integ(touched=None), integ(coords=None), integ(tsdf=None), integ(weight=None), integ(acc=None)]
    assert got == [INVALID] * len(got), got
    assert integ(n=0) == 0  # nothing touched: nothing launched
    torch.cuda.synchronize()
    assert not buf.any()

    def count(dom=good, n=1, index=p, coords=p, tsdf=p, weight=p, ws=p, tot=ll2):
        return L.gs2m_tsdf_mesh_count(dom, n, index, coords, tsdf, weight, ws, tot, s)
    got = [count(dom=bad), count(n=-1), count(index=None), count(coords=None), count(tsdf=None), count(weight=None), count(ws=None),
           count(tot=None)]
    assert got == [INVALID] * len(got), got
    assert count(n=0) == 0 and list(ll2) == [0, 0]

    def emit(dom=good, voxel=0.01, n=1, index=p, coords=p, tsdf=p, acc=p, ws=p, V=1, F=1, verts=p, cols=p, tris=p):
        return L.gs2m_tsdf_mesh_emit(dom, voxel, n, index, coords, tsdf, acc, ws, V, F, verts, cols, tris, s)
    got = [emit(dom=bad), emit(voxel=0.0), emit(n=-1), emit(index=None), emit(coords=None), emit(tsdf=None), emit(acc=None), emit(ws=None),
           emit(V=-1), emit(F=-1), emit(verts=None), emit(cols=None), emit(tris=None)]
    assert got == [INVALID] * len(got), got
    assert emit(n=0) == 0 and emit(V=0, F=0, verts=None, cols=None, tris=None) == 0
    host = (C.c_int * 3)()
    assert L.gs2m_tsdf_block_coords(-1, p, host, s) == INVALID and L.gs2m_tsdf_block_coords(1, None, host, s) == INVALID
    assert L.gs2m_tsdf_block_coords(1, p, None, s) == INVALID and L.gs2m_tsdf_block_coords(0, None, None, s) == 0
    torch.cuda.synchronize()
    assert not buf.any()
