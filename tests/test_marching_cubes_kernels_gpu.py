"""The marching-cubes kernels of csrc/tsdf.hip alone: volumes are injected (index table, block coordinates, tsdf, weight,
colour written by the test, every array between guard words), gs2m_tsdf_mesh_count and _mesh_emit are called directly, and
every result is checked twice: with the table-free invariants of tests/tsdf_ref.py against the injected volume, and bit for
bit against tests/mesh_ref.py, which pins the ordering.

  every_case     3 x 3 x 3 blocks: all 256 cases, every cube edge referenced from every position class (cube origin on a
                 block's last voxel or not, per axis), every used-edge mask at every owner class
  sparse         a third of the blocks absent in every neighbour direction, blocks on all domain faces, negative block
                 coordinates, slots permuted, weight-0 voxels and a weight-0 face layer
  value_edges    +-0, +-1, smallest normal and denormal next to both signs; all-positive and all-negative blocks
  no_crossing    totals (0, 0), an emit of nothing
  checkerboard   the fullest block there is: 12288 vertices | 16384 triangles in the packed per-block count
  big_pool       515 blocks, crossings in slots 0, 255, 256, 511, 514 alone: three loop trips of the block scan
tests/test_tsdf_ref.py asserts on the CPU that the inputs hold all this (tests/tsdf_inputs.py builds them)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gs2m_native as N  # noqa: E402
import mesh_ref as R  # noqa: E402
import tsdf_inputs as I  # noqa: E402
import tsdf_ref as T  # noqa: E402
from tsdf_gpu_buffers import DEV, Guarded, bits, dom_array, workspace_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

NTRI = (R.load_table() >= 0).sum(1) // 3
CANARY = np.float32(-1234.5)


def extract(vol):
    """gs2m_tsdf_mesh_count + gs2m_tsdf_mesh_emit on the injected volume -> (totals, vertices, colours, triangles)."""
    n = vol.n
    dom = dom_array(vol.dom)
    inputs = [Guarded(vol.index.astype(np.int32)), Guarded(vol.coords.astype(np.int32)), Guarded(vol.tsdf), Guarded(vol.weight),
              Guarded(vol.color)]
    index, coords, tsdf, weight, color = inputs
    ws = Guarded(np.zeros(workspace_bytes(vol.dom, n)[1], np.uint8))
    tot = (C.c_longlong * 2)(-1, -1)
    N.launch("gs2m_tsdf_mesh_count", DEV, dom, n, index.ptr, coords.ptr, tsdf.ptr, weight.ptr, ws.ptr, tot)
    V, F = int(tot[0]), int(tot[1])
    verts = Guarded(np.full((max(V, 1), 3), CANARY, np.float32))
    cols = Guarded(np.full((max(V, 1), 3), CANARY, np.float32))
    tris = Guarded(np.full((max(F, 1), 3), -99, np.int32))
    N.launch("gs2m_tsdf_mesh_emit", DEV, dom, float(np.float32(vol.voxel)), n, index.ptr, coords.ptr, tsdf.ptr, color.ptr, ws.ptr, V, F,
             verts.ptr, cols.ptr, tris.ptr)
    torch.cuda.synchronize()
    assert all(g.unchanged() for g in inputs), "the volume was written"
    assert ws.guards_intact() and verts.guards_intact() and cols.guards_intact() and tris.guards_intact(), "guard words written"
    if V == 0:
        assert verts.unchanged() and cols.unchanged()
    if F == 0:
        assert tris.unchanged()
    return (V, F), verts.host()[:V], cols.host()[:V], tris.host()[:F]


@pytest.mark.parametrize("name", list(I.MC_VOLUMES))
def test_marching_cubes(name):
    vol = I.MC_VOLUMES[name]()
    (V, F), v, c, t = extract(vol)
    rv, rc, rt = I.mc_reference(name)
    ck = T.MeshChecker(vol, NTRI)
    assert (V, F) == (ck.n_vertices, ck.n_triangles) == (len(rv), len(rt))
    if name == "no_crossing":
        assert (V, F) == (0, 0)
        return
    assert V > 0 and F > 0
    # the invariants: independent of the table and of the restatement
    ck.check(v, c, t)
    # the restatement, bit for bit: vertex ids and triangle order (the block and voxel prefixes), positions, colours
    assert np.array_equal(t, rt), f"triangles differ from the restatement, first at {np.argwhere(t != rt)[:1].tolist()}"
    assert np.array_equal(bits(v), bits(rv)), f"vertices differ from the restatement, max {np.abs(v - rv).max()}"
    assert np.array_equal(bits(c), bits(rc)), f"vertex colours differ from the restatement, max {np.abs(c - rc).max()}"
    if name == "value_edges":
        assert np.isfinite(v).all() and np.isfinite(c).all()
    if name == "checkerboard":
        nv, nt = ck.per_slot_counts()
        s = I.CHECKER_CENTRE_SLOT
        assert (nv[s], nt[s]) == (12288, 16384)
        # the centre block's vertices and triangles are where the prefixes of the 13 blocks before it put them
        v0, t0 = int(nv[:s].sum()), int(nt[:s].sum())
        assert np.all(ck.e_slot[v0:v0 + 12288] == s)
        own = (t[t0:t0 + 16384] >= v0) & (t[t0:t0 + 16384] < v0 + 12288)
        assert own.sum() >= 3 * 16384 // 2, "the centre block's triangles do not mostly use its own vertices"
    if name == "big_pool":
        nv, nt = ck.per_slot_counts()
        assert set(np.nonzero(nv)[0].tolist()) == set(I.BIG_POOL_LIVE) == set(np.nonzero(nt)[0].tolist())
