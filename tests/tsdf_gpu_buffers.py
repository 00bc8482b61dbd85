"""Device buffers for the TSDF kernel tests: every array the C entry points read or write lives between guard words, and the
entry points are called with the raw addresses (gs2m_native.launch), not through TSDFVolume."""
import ctypes as C

import numpy as np
import torch

import gs2m_mesh as M
import gs2m_native as N

GUARD = 64                        # words on either side of every array
PATTERN = np.int32(0x5AC3F00D)
DEV = torch.device("cuda")


class Guarded:
    """`fill` (a numpy array of any type) on the device with GUARD pattern words in front and behind."""

    def __init__(self, fill):
        fill = np.ascontiguousarray(fill)
        self.dtype, self.shape, self.nbytes = fill.dtype, fill.shape, fill.nbytes
        a = np.full((self.nbytes + 3) // 4 + 2 * GUARD, PATTERN, np.int32)
        a.view(np.uint8)[4 * GUARD:4 * GUARD + self.nbytes] = fill.reshape(-1).view(np.uint8)
        self.before = a
        self.t = torch.from_numpy(a.copy()).to(DEV)
        self.ptr = self.t.data_ptr() + 4 * GUARD

    def _bytes(self):
        return self.t.cpu().numpy().view(np.uint8)

    def host(self):
        return self._bytes()[4 * GUARD:4 * GUARD + self.nbytes].copy().view(self.dtype).reshape(self.shape)

    def guards_intact(self):
        b, ref = self._bytes(), self.before.view(np.uint8)
        return bool(np.array_equal(b[:4 * GUARD], ref[:4 * GUARD]) and np.array_equal(b[4 * GUARD + self.nbytes:], ref[4 * GUARD + self.nbytes:]))

    def unchanged(self):
        return bool(np.array_equal(self._bytes(), self.before.view(np.uint8)))


def bits(a):
    """a float32 array as its bit patterns: equality of these tells -0.0 from +0.0 and compares NaNs"""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dom_array(dom):
    return (C.c_int * 6)(*[int(x) for x in dom])


def workspace_bytes(dom, n_blocks):
    tb, mb = C.c_longlong(), C.c_longlong()
    N.check(N.lib().gs2m_tsdf_workspace_bytes(dom_array(dom), int(n_blocks), C.byref(tb), C.byref(mb)), "gs2m_tsdf_workspace_bytes")
    return tb.value, mb.value


SENTINEL = -7                     # touched_slots entries the call did not write


class Pool:
    """The caller's side of gs2m_tsdf_touch / _integrate: index table, block pool of `capacity`, state, touch workspace."""

    def __init__(self, dom, capacity, voxel, trunc, depth_trunc, with_voxels=False):
        self.dom, self.capacity = [int(x) for x in dom], int(capacity)
        self.voxel, self.trunc, self.depth_trunc = (float(np.float32(x)) for x in (voxel, trunc, depth_trunc))
        self.N = self.dom[3] * self.dom[4] * self.dom[5]
        self.index = Guarded(np.full(self.N, -1, np.int32))
        self.state = Guarded(np.zeros(4, np.int32))
        self.ws = Guarded(np.zeros(workspace_bytes(dom, 0)[0], np.uint8))
        self._pool(np.zeros((self.capacity, 3), np.int32))
        if with_voxels:
            self.tsdf = Guarded(np.zeros((self.capacity, 4096), np.float32))
            self.weight = Guarded(np.zeros((self.capacity, 4096), np.float32))
            self.color = Guarded(np.zeros((self.capacity, 3, 4096), np.float32))

    def _pool(self, coords):
        self.coords = Guarded(coords)
        self.touched = Guarded(np.full(len(coords), SENTINEL, np.int32))

    def grow(self, capacity):
        """a larger pool holding the current blocks, as TSDFVolume._grow makes one"""
        coords = np.zeros((capacity, 3), np.int32)
        coords[:self.capacity] = self.coords.host()
        self.capacity = int(capacity)
        self._pool(coords)

    def touch(self, view):
        """view: (depth, fx, fy, cx, cy, c2w) -> (return code, info (4,))"""
        depth, fx, fy, cx, cy, c2w = view
        H, W = depth.shape
        self.depth = Guarded(np.asarray(depth, np.float32))
        info = (C.c_int * 4)(-1, -1, -1, -1)
        rc = N.launch("gs2m_tsdf_touch", DEV, dom_array(self.dom), self.voxel, self.trunc, W, H, self.depth.ptr, self.depth_trunc,
                      *(float(np.float32(x)) for x in (fx, fy, cx, cy)), M._host_mat(c2w), self.capacity, self.state.ptr, self.index.ptr,
                      self.coords.ptr, self.touched.ptr, self.ws.ptr, info)
        return rc, np.array(list(info))

    def integrate(self, view, color, w2c, n_touched):
        depth, fx, fy, cx, cy, _ = view
        H, W = depth.shape
        self.image = Guarded(np.asarray(color, np.float32))
        return N.launch("gs2m_tsdf_integrate", DEV, self.voxel, self.trunc, W, H, self.depth.ptr, self.image.ptr, self.depth_trunc,
                        *(float(np.float32(x)) for x in (fx, fy, cx, cy)), M._host_mat(w2c), int(n_touched), self.touched.ptr,
                        self.coords.ptr, self.tsdf.ptr, self.weight.ptr, self.color.ptr)

    def flags(self):
        return self.ws.host()[:self.N]

    def arrays(self):
        return [self.index, self.state, self.ws, self.coords, self.touched] + ([self.tsdf, self.weight, self.color] if hasattr(self, "tsdf") else [])

    def guards_intact(self):
        return all(g.guards_intact() for g in self.arrays()) and self.depth.unchanged()
