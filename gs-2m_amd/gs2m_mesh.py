"""Mesh extraction: TSDF depth fusion and marching cubes on the GPU (csrc/tsdf.hip, include/gs2m_mesh.h).

Drop-ins for the three functions the reference's render.py imports from utils/mesh_utils.py -- `fuse_depths`,
`post_process_mesh`, `write_mesh` -- and the volume behind them, `TSDFVolume`, which follows Open3D's legacy
ScalableTSDFVolume as DESIGN.md §9 writes it down (16^3-voxel blocks, allocation from the stride-4 back-projected depth,
per-voxel projective TSDF, marching cubes with shared vertices).  Fusion, extraction and the post-processing
(`post_process_mesh_gpu`: csrc/mesh_post.hip on a `DeviceMesh`; `post_process_mesh` is its host statement) run in HIP kernels;
the memory is torch tensors owned here (the library allocates nothing).  The blocks live in a dense block-index table over a
box fixed at creation: `fuse_depths` derives it from the depth maps (or `bounds`).

    python gs-2m_amd/gs2m_mesh.py --ply point_cloud.ply -s SCENE -o OUT [--dtu | --tnt [--scene NAME]]
writes OUT/tsdf_mesh.ply, OUT/tsdf_post.ply and OUT/config.json as render.py --extract_mesh does; with --simplify-cell X or
--simplify-triangles N also OUT/tsdf_simplified.ply (`simplify_mesh_gpu`: csrc/mesh_simplify.hip); with --texture-size N also
OUT/tsdf_textured.glb, that mesh (else tsdf_post.ply) with a baked texture atlas (gs2m_mesh_texture.py), and with --normal-map
beside it a tangent-space normal map in that file.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np
import torch

import gs2m_native as N
from gs2m_eval_util import workspace_for

BLOCK = 16
POOL_FULL = 1  # include/gs2m_mesh.h GS2M_TSDF_POOL_FULL


class TriangleMesh:
    """vertices (V, 3) float32, triangles (F, 3) int32, vertex_colors (V, 3) float32 in [0, 1]: numpy arrays, so
    `len(mesh.vertices)` and `np.asarray(mesh.triangles)` work as on Open3D's mesh."""

    def __init__(self, vertices=None, triangles=None, vertex_colors=None):
        self.vertices = np.zeros((0, 3), np.float32) if vertices is None else np.ascontiguousarray(vertices, dtype=np.float32)
        self.triangles = np.zeros((0, 3), np.int32) if triangles is None else np.ascontiguousarray(triangles, dtype=np.int32)
        self.vertex_colors = (np.zeros((len(self.vertices), 3), np.float32) if vertex_colors is None
                              else np.ascontiguousarray(vertex_colors, dtype=np.float32))


class DeviceMesh:
    """A TriangleMesh whose arrays are torch tensors on one device: vertices (V, 3) float32, triangles (F, 3) int32,
    vertex_colors (V, 3) float32.  What extraction hands to the post-processing without a host round trip."""

    def __init__(self, vertices, triangles, vertex_colors=None):
        self.vertices = torch.as_tensor(vertices).to(torch.float32).reshape(-1, 3).contiguous()
        dev = self.vertices.device
        self.triangles = torch.as_tensor(triangles).to(torch.int32).reshape(-1, 3).contiguous()
        self.vertex_colors = (torch.zeros_like(self.vertices) if vertex_colors is None
                              else torch.as_tensor(vertex_colors).to(torch.float32).reshape(-1, 3).contiguous())
        if self.triangles.device != dev or self.vertex_colors.device != dev:
            raise ValueError(f"gs2m_mesh: DeviceMesh arrays on {dev}, {self.triangles.device} and {self.vertex_colors.device}")
        if len(self.vertex_colors) != len(self.vertices):
            raise ValueError(f"gs2m_mesh: {len(self.vertex_colors)} colours for {len(self.vertices)} vertices")

    @property
    def device(self):
        return self.vertices.device

    @classmethod
    def from_mesh(cls, mesh, device="cuda"):
        dev = torch.device(device)
        return cls(torch.from_numpy(np.asarray(mesh.vertices, dtype=np.float32)).to(dev),
                   torch.from_numpy(np.asarray(mesh.triangles, dtype=np.int32)).to(dev),
                   torch.from_numpy(np.asarray(mesh.vertex_colors, dtype=np.float32)).to(dev))

    def cpu(self):
        return TriangleMesh(self.vertices.cpu().numpy(), self.triangles.cpu().numpy(), self.vertex_colors.cpu().numpy())


_ptr = N.ptr


def _host_mat(m):
    """(4, 4) -> HOST float[16] row major, fp32."""
    a = np.ascontiguousarray(np.asarray(m, dtype=np.float32).reshape(4, 4))
    return (C.c_float * 16)(*a.reshape(-1).tolist())


def c2w_of(w2c):
    """The camera-to-world matrix the touch rule uses: the fp64 inverse of the W2C matrix, rounded to fp32."""
    return np.linalg.inv(np.asarray(w2c, dtype=np.float64)).astype(np.float32)


class TSDFVolume:
    """A TSDF volume over the world box [domain_min, domain_max] (cut to whole blocks of 16 * voxel_length).

    integrate(depth (H, W), color (H, W, 3) uint8 or float in [0, 1], fx, fy, cx, cy, w2c (4, 4)) fuses one view;
    extract_triangle_mesh() runs marching cubes (to_host=False: the mesh stays on the device, a DeviceMesh).  Depths <= 0 or
    above `depth_trunc` are empty.  `ignored_points`: points of the integrated views whose trunc box left the domain (counted,
    not fused)."""

    def __init__(self, voxel_length, sdf_trunc, depth_trunc, domain_min, domain_max, device="cuda", capacity=256):
        self.voxel = float(np.float32(voxel_length))
        self.trunc = float(np.float32(sdf_trunc))
        self.depth_trunc = float(np.float32(depth_trunc))
        self.device = torch.device(device)
        L = BLOCK * self.voxel
        lo = [math.floor(float(a) / L) for a in domain_min]
        hi = [math.floor(float(b) / L) for b in domain_max]
        self.dom = [lo[0], lo[1], lo[2], hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1]
        self._dom = (C.c_int * 6)(*self.dom)
        if min(self.dom[3:]) <= 0:
            raise ValueError(f"gs2m_mesh: empty domain {domain_min} .. {domain_max}")
        self.index_bytes = 4 * self.dom[3] * self.dom[4] * self.dom[5]
        self.ignored_points = 0
        with N.device_guard(self.device):
            self.index = torch.full((self.dom[3] * self.dom[4] * self.dom[5],), -1, dtype=torch.int32, device=self.device)
            self.state = torch.zeros(4, dtype=torch.int32, device=self.device)
            self.touch_ws = workspace_for("gs2m_tsdf_workspace_bytes", self.device, self._dom, 0, only=0).zero_()
        self.n_blocks = 0
        self.capacity = 0
        self._grow(max(1, int(capacity)))

    def _grow(self, capacity):
        """A pool of `capacity` blocks holding the current ones (zero-filled beyond them)."""
        n, d = self.n_blocks, self.device
        with N.device_guard(d):
            coords = torch.zeros((capacity, 3), dtype=torch.int32, device=d)
            tsdf = torch.zeros((capacity, BLOCK ** 3), dtype=torch.float32, device=d)
            weight = torch.zeros_like(tsdf)
            color = torch.zeros((capacity, 3, BLOCK ** 3), dtype=torch.float32, device=d)
            if n:
                coords[:n] = self.block_coords[:n]
                tsdf[:n] = self.tsdf[:n]
                weight[:n] = self.weight[:n]
                color[:n] = self.color[:n]
            self.block_coords, self.tsdf, self.weight, self.color = coords, tsdf, weight, color
            self.touched = torch.zeros(capacity, dtype=torch.int32, device=d)
        self.capacity = capacity

    def _image(self, depth, color):
        d = torch.as_tensor(depth).to(self.device, torch.float32).contiguous()
        c = torch.as_tensor(color).to(self.device)
        if c.dim() == 3 and c.shape[0] == 3 and c.shape[-1] != 3:
            c = c.permute(1, 2, 0)
        c = c.float() if c.dtype == torch.uint8 else c.float() * 255.0
        H, W = d.shape
        if tuple(c.shape) != (H, W, 3):
            raise ValueError(f"gs2m_mesh: color {tuple(c.shape)} does not match depth {(H, W)}")
        return d, c.contiguous()

    def integrate(self, depth, color, fx, fy, cx, cy, w2c):
        d, c = self._image(depth, color)
        H, W = d.shape
        w2c = np.asarray(w2c.detach().cpu() if torch.is_tensor(w2c) else w2c, dtype=np.float32).reshape(4, 4)
        c2w = _host_mat(c2w_of(w2c))
        w2c_h = _host_mat(w2c)
        fx, fy, cx, cy = (float(np.float32(x)) for x in (fx, fy, cx, cy))
        info = (C.c_int * 4)()
        while True:
            rc = N.launch("gs2m_tsdf_touch", self.device, self._dom, self.voxel, self.trunc, W, H, _ptr(d), self.depth_trunc, fx, fy, cx, cy,
                          c2w, self.capacity, _ptr(self.state), _ptr(self.index), _ptr(self.block_coords), _ptr(self.touched),
                          _ptr(self.touch_ws), info)
            if rc != POOL_FULL:
                break
            self._grow(max(int(info[0]), 2 * self.capacity))  # nothing but the ignored count was written: repeat
        self.ignored_points += int(info[3])
        self.n_blocks = int(info[0])
        N.launch("gs2m_tsdf_integrate", self.device, self.voxel, self.trunc, W, H, _ptr(d), _ptr(c), self.depth_trunc, fx, fy, cx, cy, w2c_h,
                 int(info[1]), _ptr(self.touched), _ptr(self.block_coords), _ptr(self.tsdf), _ptr(self.weight), _ptr(self.color))
        return int(info[1])

    def extract_triangle_mesh(self, to_host=True):
        n = self.n_blocks
        if n == 0:
            return TriangleMesh() if to_host else DeviceMesh.from_mesh(TriangleMesh(), self.device)
        ws = workspace_for("gs2m_tsdf_workspace_bytes", self.device, self._dom, n, only=1)
        tot = (C.c_longlong * 2)()
        N.launch("gs2m_tsdf_mesh_count", self.device, self._dom, n, _ptr(self.index), _ptr(self.block_coords), _ptr(self.tsdf),
                 _ptr(self.weight), _ptr(ws), tot)
        V, F = int(tot[0]), int(tot[1])
        verts = torch.empty((max(V, 1), 3), dtype=torch.float32, device=self.device)
        cols = torch.empty_like(verts)
        tris = torch.empty((max(F, 1), 3), dtype=torch.int32, device=self.device)
        N.launch("gs2m_tsdf_mesh_emit", self.device, self._dom, self.voxel, n, _ptr(self.index), _ptr(self.block_coords), _ptr(self.tsdf),
                 _ptr(self.color), _ptr(ws), V, F, _ptr(verts), _ptr(cols), _ptr(tris))
        if not to_host:
            return DeviceMesh(verts[:V], tris[:F], cols[:V])
        return TriangleMesh(verts[:V].cpu().numpy(), tris[:F].cpu().numpy(), cols[:V].cpu().numpy())

    def state_arrays(self):
        """Tests: (block coords (n, 3) int32 -- read back through gs2m_tsdf_block_coords --, tsdf (n, 4096), weight (n, 4096),
        color (n, 3, 4096) on 0..255), slot order, numpy."""
        n = self.n_blocks
        coords = np.zeros((n, 3), np.int32)
        N.launch("gs2m_tsdf_block_coords", self.device, n, _ptr(self.block_coords), coords.ctypes.data_as(C.c_void_p))
        return coords, self.tsdf[:n].cpu().numpy(), self.weight[:n].cpu().numpy(), self.color[:n].cpu().numpy()


# ---- render.py's drop-ins ---------------------------------------------------------------------------------------------

def quantize_depth_mm(depth):
    """The reference's `(depth * 1000).astype(np.uint16)` read back with depth_scale 1000, as fp32 torch ops: whole
    millimetres, truncated.  Deliberate difference: depths >= 65.536 (and negative ones) become 0 instead of wrapping."""
    q = torch.trunc(depth * 1000.0)
    q = torch.where((q >= 0) & (q < 65536.0), q, torch.zeros_like(q))
    return q / 1000.0


def _view_w2c(view):
    return view.world_view_transform.transpose(0, 1).detach().cpu().double().numpy()


def _points_from_depth(view, depth):
    """loss_utils._get_points_from_depth at scale 1: camera rays times depth, to world space with the view's R, T."""
    rays = view.get_rays()
    pts = (rays * depth[..., None]).reshape(-1, 3)
    R = torch.as_tensor(np.asarray(view.R), dtype=torch.float32, device=depth.device)
    T = torch.as_tensor(np.asarray(view.T), dtype=torch.float32, device=depth.device)
    return (pts - T) @ R.transpose(-1, -2)


def _load_color(view, idx, render_dir, colors):
    if colors is not None:
        return colors[idx]
    from PIL import Image
    name = getattr(view, "image_name", None) or f"{idx:05d}.png"
    stem = name.rsplit(".", 1)[0]
    return torch.from_numpy(np.asarray(Image.open(os.path.join(str(render_dir), f"{stem}.png")).convert("RGB"), dtype=np.uint8).copy())


def fuse_depths(tsdf_depths, views, render_dir, max_depth, voxel_size, sdf_trunc, bounds=None, colors=None, quantize=True,
                device="cuda"):
    """utils/mesh_utils.py fuse_depths: every view's depth (tsdf_depths (N, H, W)) masked -- by the view's alpha_mask
    (< 0.5 -> 0) when `bounds` is None and the view has one, else to the points inside `bounds` (3, 2) --, quantised to whole
    millimetres (`quantize`), fused with the colour read from render_dir/<stem>.png (or colors[i]: (H, W, 3) uint8 / float in
    [0, 1], or (3, H, W) float) up to `max_depth`.  The volume's domain: `bounds`, or the box of all back-projected points
    (computed on the device), padded by sdf_trunc and one block (the block absorbs the fp32 rounding of the touch rule's
    floor((p -/+ trunc) / L) at the box's faces).  -> TSDFVolume."""
    dev = torch.device(device)
    depths = []
    for idx, view in enumerate(views):
        d = torch.as_tensor(tsdf_depths[idx]).to(dev, torch.float32).clone()
        h, w = d.shape
        if bounds is not None:
            b = torch.as_tensor(np.asarray(bounds, dtype=np.float32), device=dev)
            pts = _points_from_depth(view, d)
            out = ((pts[:, 0] < b[0, 0]) | (pts[:, 0] > b[0, 1]) | (pts[:, 1] < b[1, 0]) | (pts[:, 1] > b[1, 1]) |
                   (pts[:, 2] < b[2, 0]) | (pts[:, 2] > b[2, 1]))
            d[out.reshape(h, w)] = 0
        elif getattr(view, "alpha_mask", None) is not None:
            d[torch.as_tensor(view.alpha_mask).to(dev).squeeze() < 0.5] = 0
        depths.append((quantize_depth_mm(d) if quantize else d).contiguous())
    trunc, L = float(np.float32(sdf_trunc)), BLOCK * float(np.float32(voxel_size))
    if bounds is not None:
        b = np.asarray(bounds, dtype=np.float64)
        lo, hi = b[:, 0], b[:, 1]
    else:
        lo, hi = _depth_aabb(depths, views, float(np.float32(max_depth)), dev)
        if lo is None:
            lo = hi = np.zeros(3)
    lo, hi = lo - trunc - L, hi + trunc + L
    vol = TSDFVolume(voxel_size, sdf_trunc, max_depth, lo, hi, device=dev)
    for idx, view in enumerate(views):
        vol.integrate(depths[idx], _load_color(view, idx, render_dir, colors), view.Fx, view.Fy, view.Cx, view.Cy, _view_w2c(view))
    return vol


def _depth_aabb(depths, views, depth_trunc, dev):
    """The AABB of every view's stride-4 back-projected points (gs2m_tsdf_points_aabb), or (None, None) when there is none."""
    key = torch.tensor([2 ** 31 - 1] * 3 + [-2 ** 31] * 3, dtype=torch.int32, device=dev)
    for d, view in zip(depths, views):
        H, W = d.shape
        N.launch("gs2m_tsdf_points_aabb", dev, W, H, _ptr(d), depth_trunc, float(view.Fx), float(view.Fy), float(view.Cx), float(view.Cy),
                 _host_mat(c2w_of(_view_w2c(view))), _ptr(key))
    k = key.cpu().numpy().astype(np.int32)
    if k[0] > k[3]:
        return None, None
    bits = np.where(k >= 0, k, k ^ np.int32(0x7FFFFFFF)).astype(np.int32)
    f = bits.view(np.float32).astype(np.float64)
    return f[:3], f[3:]


def cluster_connected_triangles(mesh):
    """Open3D's TriangleMesh.cluster_connected_triangles: triangles sharing an edge are connected.
    -> (cluster index per triangle, triangles per cluster)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t = np.asarray(mesh.triangles, dtype=np.int64)
    F = len(t)
    if F == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    e = np.sort(np.stack([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], axis=1).reshape(-1, 2), axis=1)
    key = e[:, 0] * (int(t.max()) + 1) + e[:, 1]
    owner = np.repeat(np.arange(F), 3)
    order = np.argsort(key, kind="stable")
    ks, os_ = key[order], owner[order]
    same = ks[1:] == ks[:-1]
    g = coo_matrix((np.ones(int(same.sum())), (os_[:-1][same], os_[1:][same])), shape=(F, F))
    n, labels = connected_components(g, directed=False)
    return labels, np.bincount(labels, minlength=n)


def post_process_mesh(mesh, cluster_to_keep=1):
    """utils/mesh_utils.py post_process_mesh: keep the clusters of at least max(cluster_to_keep-th largest, 50) triangles,
    then drop unreferenced vertices and degenerate triangles (two equal vertex ids).  cluster_to_keep beyond the number of
    clusters keeps them all (the reference's numpy indexing would raise)."""
    t = np.asarray(mesh.triangles, dtype=np.int32)
    if len(t) == 0:
        return TriangleMesh(np.zeros((0, 3), np.float32), t, np.zeros((0, 3), np.float32))
    labels, counts = cluster_connected_triangles(mesh)
    nth = np.sort(counts)[-min(int(cluster_to_keep), len(counts))]
    keep = counts[labels] >= max(int(nth), 50)
    t = t[keep]
    used = np.zeros(len(mesh.vertices), bool)
    used[t.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    t = remap[t].astype(np.int32)
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])]
    return TriangleMesh(np.asarray(mesh.vertices)[used], t, np.asarray(mesh.vertex_colors)[used])


def _post_device(mesh, device, who):
    """The DeviceMesh the device post-processing works on (a TriangleMesh is copied to `device`).  No CPU path."""
    dm = mesh if isinstance(mesh, DeviceMesh) else None
    dev = dm.device if dm is not None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: the mesh must be on a HIP device, got `{dev}`; there is no CPU path (post_process_mesh and "
                           "cluster_connected_triangles are the host functions)")
    return dm if dm is not None else DeviceMesh.from_mesh(mesh, dev)


def post_workspace_bytes(n_vertices, n_triangles):
    """-> (cluster workspace, compaction workspace) in bytes, as the library sizes them."""
    a, b = C.c_longlong(), C.c_longlong()
    N.check(N.lib().gs2m_mesh_post_workspace_bytes(int(n_vertices), int(n_triangles), C.byref(a), C.byref(b)), "gs2m_mesh_post_workspace_bytes")
    return a.value, b.value


def _cluster_device(triangles, n_vertices):
    """triangles (F, 3) int32 on a HIP device -> (tri_cluster int32 (F,), cluster_size int32 (F,), C)."""
    dev, F = triangles.device, len(triangles)
    with N.device_guard(dev):
        lab = torch.empty(F, dtype=torch.int32, device=dev)
        size = torch.empty(F, dtype=torch.int32, device=dev)
    if F == 0:
        return lab, size, 0
    ws = workspace_for("gs2m_mesh_post_workspace_bytes", dev, int(n_vertices), F, only=0)
    n = C.c_longlong()
    N.launch("gs2m_mesh_cluster_triangles", dev, int(n_vertices), F, _ptr(triangles), _ptr(ws), _ptr(lab), _ptr(size), C.byref(n))
    return lab, size, int(n.value)


def cluster_connected_triangles_gpu(mesh_or_triangles, n_vertices=None, device="cuda"):
    """cluster_connected_triangles on the device (csrc/mesh_post.hip).  A TriangleMesh, a DeviceMesh or a (F, 3) array of
    triangles (`n_vertices`: the vertex count they index; default: the largest id + 1).  -> (cluster index per triangle,
    triangles per cluster) as int32 tensors; clusters are numbered by increasing smallest triangle index."""
    who = "cluster_connected_triangles_gpu"
    if isinstance(mesh_or_triangles, (TriangleMesh, DeviceMesh)):
        dm = _post_device(mesh_or_triangles, device, who)
        tris, nv = dm.triangles, len(dm.vertices) if n_vertices is None else int(n_vertices)
    else:
        t = mesh_or_triangles
        dev = t.device if torch.is_tensor(t) else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"{who}: the triangles must be on a HIP device, got `{dev}`; there is no CPU path")
        tris = torch.as_tensor(t).to(dev, torch.int32).reshape(-1, 3).contiguous()
        nv = int(n_vertices) if n_vertices is not None else (int(tris.max()) + 1 if len(tris) else 0)
    lab, size, n = _cluster_device(tris, nv)
    return lab, size[:n].clone()


def post_process_mesh_gpu(mesh, cluster_to_keep=1, device="cuda"):
    """post_process_mesh on the device: the same arrays, element for element.  A DeviceMesh is processed where it is and a
    DeviceMesh comes back; a TriangleMesh goes to `device` and comes back as a TriangleMesh.  One scalar (the size bound)
    and the three counts are read back; the mesh is not."""
    dm = _post_device(mesh, device, "post_process_mesh_gpu")
    dev, V, F = dm.device, len(dm.vertices), len(dm.triangles)
    if F == 0:
        out = DeviceMesh(dm.vertices[:0], dm.triangles[:0], dm.vertex_colors[:0])
    else:
        lab, size, n = _cluster_device(dm.triangles, V)
        nth = int(torch.sort(size[:n]).values[-min(int(cluster_to_keep), n)])  # numpy's indexing, as the host function's
        with N.device_guard(dev):
            keep = torch.empty(F, dtype=torch.uint8, device=dev)
            ov, oc, ot = torch.empty_like(dm.vertices), torch.empty_like(dm.vertex_colors), torch.empty_like(dm.triangles)
        N.launch("gs2m_mesh_keep_clusters", dev, F, _ptr(lab), _ptr(size), max(nth, 50), _ptr(keep))
        ws = workspace_for("gs2m_mesh_post_workspace_bytes", dev, V, F, only=1)
        tot = (C.c_longlong * 2)()
        N.launch("gs2m_mesh_compact", dev, V, F, _ptr(dm.vertices), _ptr(dm.vertex_colors), _ptr(dm.triangles), _ptr(keep), _ptr(ws),
                 _ptr(ov), _ptr(oc), _ptr(ot), tot)
        nv, nt = int(tot[0]), int(tot[1])
        out = DeviceMesh(ov[:nv].clone(), ot[:nt].clone(), oc[:nv].clone())  # clones: the input-sized buffers go
    return out if isinstance(mesh, DeviceMesh) else out.cpu()


# ---- simplification (csrc/mesh_simplify.hip, include/gs2m_simplify.h) ---------------------------------------------------

SIMPLIFY_STAGES = ("keys_sorts", "quadrics", "placement", "remap_dedupe", "compaction")
LADDER = 8  # rungs per octave of the target-count search


def simplify_count_gpu(vertices, triangles, cell):
    """(surviving vertices, emitted triangles) of the contract at `cell`, without placement: the probe of the search."""
    dev, V, F = vertices.device, len(vertices), len(triangles)
    if V == 0 or F == 0:
        return 0, 0
    ws = workspace_for("gs2m_simplify_workspace_bytes", dev, V, F, 0)
    tot = (C.c_longlong * 2)()
    N.launch("gs2m_simplify_count", dev, V, F, _ptr(vertices), _ptr(triangles), float(cell), _ptr(ws), tot)
    return int(tot[0]), int(tot[1])


def simplify_base_cell(vertices, triangles):
    """The first rung of the ladder: the shortest non-degenerate edge of the first 4096 triangles (fp64 lengths of the fp32
    corners), a pure function of the input; 1.0 when they have none."""
    t = triangles[:4096].long()
    if len(t) == 0:
        return 1.0
    p = vertices.double()[t]  # (n, 3 corners, 3)
    e = torch.cat([p[:, 1] - p[:, 0], p[:, 2] - p[:, 1], p[:, 0] - p[:, 2]]).norm(dim=1)
    e = e[(e > 0) & torch.isfinite(e)]
    return float(e.min()) if len(e) else 1.0


def simplify_target_cell(vertices, triangles, target_triangles, max_rungs=8 * 40):
    """The cell of the ladder cell_k = base * 2^(k / 8) (base: simplify_base_cell) that bisection with gs2m_simplify_count
    settles on: its result has at most `target_triangles` triangles and rung k - 1 has more.  -> (cell, k)."""
    base, n = simplify_base_cell(vertices, triangles), int(target_triangles)
    count = lambda k: simplify_count_gpu(vertices, triangles, base * 2.0 ** (k / LADDER))[1]
    lo, hi = -1, LADDER  # invariant: count(lo) > n (rung -1 stands for the input itself), count(hi) <= n
    while count(hi) > n:
        lo, hi = hi, hi * 2
        if hi > max_rungs:
            raise RuntimeError(f"simplify_mesh_gpu: no cell up to base * 2^{max_rungs // LADDER} reaches {n} triangles")
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if mid >= 0 and count(mid) <= n:
            hi = mid
        else:
            lo = mid
    return base * 2.0 ** (hi / LADDER), hi


def simplify_mesh_gpu(mesh, cell=None, target_triangles=None, attributes=None, weights=None, device="cuda", extras=False):
    """Vertex clustering with quadric placement on the device (include/gs2m_simplify.h has the contract).  A DeviceMesh is
    processed where it is and a DeviceMesh comes back; a TriangleMesh goes to `device` and comes back as a TriangleMesh.  The
    vertex colours are carried as three channels; `attributes` (V, k) are further fp32 channels, `weights` (V,) >= 0 weigh all
    of them within a cell (None: all ones).  With `extras` (or attributes) the result is (mesh, dict(attributes, weight,
    vertex_map, cell, input_triangles)): weight is a cell's weight sum (0: no weighted vertex, its values are the plain
    mean), vertex_map the new id of every input vertex or -1.

    Exactly one of `cell` and `target_triangles`.  target_triangles searches the ladder cell_k = base * 2^(k / 8), base the
    shortest non-degenerate edge of the first 4096 triangles, by bisection with the count-only entry point.  The count is NOT
    monotone in the cell (the lattice shifts against the surface), so only two facts are guaranteed: the result has at most
    target_triangles triangles, and the rung below the chosen one has more.  A target that is not below the input's count
    returns the mesh unchanged (cell = None in the extras)."""
    who = "simplify_mesh_gpu"
    if (cell is None) == (target_triangles is None):
        raise ValueError(f"{who}: give exactly one of `cell` and `target_triangles`")
    if cell is not None and not (math.isfinite(float(cell)) and float(cell) > 0):
        raise ValueError(f"{who}: `cell` must be finite and positive, got {cell}")
    if target_triangles is not None and int(target_triangles) < 0:
        raise ValueError(f"{who}: `target_triangles` must not be negative")
    dm = _post_device(mesh, device, who)
    dev, V, F = dm.device, len(dm.vertices), len(dm.triangles)
    with N.device_guard(dev):
        att = None if attributes is None else torch.as_tensor(attributes).to(dev, torch.float32).reshape(V, -1)
        w = None if weights is None else torch.as_tensor(weights).to(dev, torch.float32).reshape(-1).contiguous()
        if w is not None and len(w) != V:
            raise ValueError(f"{who}: {len(w)} weights for {V} vertices")
        k = 0 if att is None else att.shape[1]
        unchanged = target_triangles is not None and int(target_triangles) >= F
        if unchanged:
            out, oa = dm, att
            ow = torch.ones(V, device=dev) if w is None else w
            vmap = torch.arange(V, dtype=torch.int32, device=dev)
        else:
            if cell is None:
                cell, _ = simplify_target_cell(dm.vertices, dm.triangles, target_triangles)
            cell = float(cell)
            chan = dm.vertex_colors if att is None else torch.cat([dm.vertex_colors, att], dim=1).contiguous()
            nch = 3 + k
            ov, oc, ot = torch.empty_like(dm.vertices), torch.empty_like(chan), torch.empty_like(dm.triangles)
            ow = torch.empty(V, dtype=torch.float32, device=dev)
            vmap = torch.full((V,), -1, dtype=torch.int32, device=dev)
            tot = (C.c_longlong * 2)()
            if V and F:
                ws = workspace_for("gs2m_simplify_workspace_bytes", dev, V, F, nch)
                N.launch("gs2m_simplify", dev, V, F, _ptr(dm.vertices), _ptr(dm.triangles), nch, _ptr(chan), _ptr(w), cell, _ptr(ws),
                         _ptr(ov), _ptr(oc), _ptr(ow), _ptr(ot), _ptr(vmap), tot)
            nv, nt = int(tot[0]), int(tot[1])
            out = DeviceMesh(ov[:nv].clone(), ot[:nt].clone(), oc[:nv, :3].clone())  # clones: the input-sized buffers go
            oa, ow = (None if att is None else oc[:nv, 3:].clone()), ow[:nv].clone()
    res = out if isinstance(mesh, DeviceMesh) else out.cpu()
    if not (extras or attributes is not None):
        return res
    return res, {"attributes": oa, "weight": ow, "vertex_map": vmap, "cell": None if unchanged else cell, "input_triangles": F}


def simplify_stage_times(on=None):
    """on = True / False: switch the per-stage timing of gs2m_simplify (a stream synchronisation at every stage boundary);
    None: -> {stage: ms} of the last call."""
    if on is not None:
        N.check(N.lib().gs2m_simplify_set_timing(int(bool(on))), "gs2m_simplify_set_timing")
        return None
    ms = (C.c_float * 5)()
    N.check(N.lib().gs2m_simplify_stage_ms(ms), "gs2m_simplify_stage_ms")
    return {n: float(ms[k]) for k, n in enumerate(SIMPLIFY_STAGES)}


_PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_mesh(file, mesh):
    """Binary little-endian PLY: float x y z, uchar red green blue (colour * 255 rounded to nearest), int32 face lists.
    A DeviceMesh is read back once."""
    if isinstance(mesh, DeviceMesh):
        mesh = mesh.cpu()
    v = np.asarray(mesh.vertices, dtype=np.float32).reshape(-1, 3)
    c = np.asarray(mesh.vertex_colors, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(mesh.triangles, dtype=np.int32).reshape(-1, 3)
    va = np.zeros(len(v), _PLY_VERTEX)
    for k, n in enumerate("xyz"):
        va[n] = v[:, k]
    for k, n in enumerate(("red", "green", "blue")):
        va[n] = np.clip(np.rint(c[:, k] * 255.0), 0, 255).astype(np.uint8) if len(c) else 0
    fa = np.zeros(len(t), _PLY_FACE)
    fa["n"] = 3
    fa["v"] = t
    head = ("ply\nformat binary_little_endian 1.0\ncomment gs2m_mesh TSDF mesh\n"
            f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(str(file), "wb") as f:
        f.write(head.encode("ascii"))
        f.write(va.tobytes())
        f.write(fa.tobytes())


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2",
              "uint16": "<u2", "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4",
              "double": "<f8", "float64": "<f8"}


def _ply_elements(file):
    """The elements of a binary little-endian PLY, one after the other in file order -> (name, structured array, is_list): a
    list element (uchar|int counts, int|uint indices) has the fields n and v (3 indices), any other one field per scalar
    property.  ValueError for another format, and for a list element that is not all triangles when the walk reaches it."""
    with open(str(file), "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"{file}: not a binary little-endian PLY")
    elems = []
    for ln in lines:
        p = ln.split()
        if p and p[0] == "element":
            elems.append([p[1], int(p[2]), []])
        elif p and p[0] == "property":
            elems[-1][2].append(p[1:])
    off = end
    for name, n, props in elems:
        is_list = bool(props) and props[0][0] == "list"
        if is_list:
            dt = np.dtype([("n", _PLY_TYPES[props[0][1]]), ("v", _PLY_TYPES[props[0][2]], (3,))])
        else:
            dt = np.dtype([(q[1], _PLY_TYPES[q[0]]) for q in props])
        a = np.frombuffer(data, dt, n, off)
        if is_list and n and not np.all(a["n"] == 3):
            raise ValueError(f"{file}: only triangle faces are read")
        off += dt.itemsize * n
        yield name, a, is_list


def _ply_columns(a, names, scale=1.0):
    """the scalar properties `names` of a PLY element as one float32 array (n, len(names)), divided by `scale`"""
    return np.stack([a[k].astype(np.float32) / scale for k in names], axis=1) if len(a) else np.zeros((0, len(names)), np.float32)


def read_mesh(file):
    """Binary little-endian PLY with a vertex element (x y z, optional red green blue uchar, other scalar properties
    skipped) and a triangle face element (list uchar|int int|uint) -> TriangleMesh."""
    verts, tris, cols = None, None, None
    for name, a, is_list in _ply_elements(file):
        if is_list and name == "face":
            tris = a["v"].astype(np.int32)
        elif not is_list and name == "vertex":
            verts = _ply_columns(a, "xyz")
            if "red" in a.dtype.names:
                cols = _ply_columns(a, ("red", "green", "blue"), 255.0)
    return TriangleMesh(verts, tris if tris is not None else np.zeros((0, 3), np.int32), cols)


# ---- command line: render.py --extract_mesh for a saved model ---------------------------------------------------------

def render_views(gaussians, views, render_dir, device="cuda", png="host"):
    """Depth and the SH colour of every view with this repository's render(); the colours are saved as render_dir/<stem>.png
    as render.py saves them (torchvision.utils.save_image rounding; `png`: "host" through Pillow, "device" through gs2m_png).
    -> (N, H, W) depths on the device."""
    from gaussian_renderer import render
    from gs2m_scene import PipelineParams
    from gs2m_png import Writer
    writer = Writer(png)
    os.makedirs(render_dir, exist_ok=True)
    bg = torch.zeros(3, device=device)
    depths = []
    with torch.no_grad():
        for k, view in enumerate(views):
            if getattr(view, "image_name", None) is None:
                view.image_name = f"{k:05d}.png"
            out = render(view, gaussians, PipelineParams(), bg, material_stage=True)  # as render.py: the depth map needs the G-buffer
            depths.append(out["depth_map"].squeeze(0).float().clone())
            img = out["render"].clamp(0.0, 1.0).mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).contiguous()
            writer.put(img, os.path.join(render_dir, view.image_name.rsplit(".", 1)[0] + ".png"))
            writer.flush()
    return torch.stack(depths)


def extract_mesh(gaussians, views, cameras_extent, out_dir, max_depth=-1.0, voxel_size=-1.0, sdf_trunc=-1.0, num_clusters=1,
                 bounds=None, device="cuda", host_post=False, simplify_cell=None, simplify_triangles=None):
    """render.py's --extract_mesh path: render, fuse, extract, post-process; writes out_dir/{config.json, tsdf_mesh.ply,
    tsdf_post.ply}.  The mesh stays on the device from extraction through post_process_mesh_gpu; `host_post`: read it back
    and run the host post_process_mesh instead (the same two files, byte for byte).  -> (raw mesh, post-processed mesh),
    host TriangleMesh both.  `simplify_cell` / `simplify_triangles` (one of them): simplify_mesh_gpu runs on the post-processed mesh,
    out_dir/tsdf_simplified.ply is written too and config.json records the cell and both triangle counts."""
    if simplify_cell is not None and simplify_triangles is not None:
        raise ValueError("extract_mesh: give one of `simplify_cell` and `simplify_triangles`")
    os.makedirs(out_dir, exist_ok=True)
    max_depth = max_depth if max_depth > 0 else 2.0 * cameras_extent
    voxel_size = voxel_size if voxel_size > 0 else max_depth / 1024.0
    sdf_trunc = sdf_trunc if sdf_trunc > 0 else 4.0 * voxel_size
    with open(os.path.join(out_dir, "config.json"), "w") as f:
        json.dump({"max_depth": max_depth, "voxel_size": voxel_size, "sdf_trunc": sdf_trunc}, f, indent=4)
    render_dir = os.path.join(out_dir, "renders")
    depths = render_views(gaussians, views, render_dir, device)
    vol = fuse_depths(depths, views, render_dir, max_depth, voxel_size, sdf_trunc, bounds, device=device)
    if host_post:
        mesh = vol.extract_triangle_mesh()
        post = post_process_mesh(mesh, num_clusters)
        post_device = None
    else:
        on_device = vol.extract_triangle_mesh(to_host=False)
        post_device = post_process_mesh_gpu(on_device, num_clusters)
        mesh, post = on_device.cpu(), post_device.cpu()
    write_mesh(os.path.join(out_dir, "tsdf_mesh.ply"), mesh)
    write_mesh(os.path.join(out_dir, "tsdf_post.ply"), post)
    if simplify_cell is not None or simplify_triangles is not None:
        simple, info = simplify_mesh_gpu(post_device if post_device is not None else DeviceMesh.from_mesh(post, device),
                                         cell=simplify_cell, target_triangles=simplify_triangles, extras=True)
        write_mesh(os.path.join(out_dir, "tsdf_simplified.ply"), simple)
        with open(os.path.join(out_dir, "config.json"), "w") as f:
            json.dump({"max_depth": max_depth, "voxel_size": voxel_size, "sdf_trunc": sdf_trunc, "simplify_cell": info["cell"],
                       "simplify_input_triangles": len(post.triangles), "simplify_output_triangles": len(simple.triangles)}, f, indent=4)
        print(f"[>] simplified at cell {info['cell']}: {len(simple.vertices)} vertices / {len(simple.triangles)} triangles")
    print(f"[>] {len(mesh.vertices)} vertices / {len(mesh.triangles)} triangles raw, {len(post.vertices)} / {len(post.triangles)} "
          f"post-processed; {vol.n_blocks} blocks, {vol.ignored_points} points outside the domain -> {out_dir}")
    return mesh, post


TNT_360_SCENES = ("barn", "caterpillar", "ignatius", "truck")


def add_simplify_arguments(ap):
    """--simplify-cell X / --simplify-triangles N.  SUPPRESSed defaults: without the flags the namespace is what it was."""
    ap.add_argument("--simplify-cell", type=float, default=argparse.SUPPRESS, metavar="X",
                    help="also write tsdf_simplified.ply: the post-processed mesh clustered on a lattice of edge X (quadric placement)")
    ap.add_argument("--simplify-triangles", type=int, default=argparse.SUPPRESS, metavar="N",
                    help="the same with the lattice edge searched for at most N triangles")


def add_texture_arguments(ap):
    """--texture-size N [--normal-map] [--ao].  SUPPRESSed defaults: without the flags the namespace is what it was (and gs2m_mesh_texture
    is not imported)."""
    ap.add_argument("--texture-size", type=int, default=argparse.SUPPRESS, metavar="N",
                    help="also write tsdf_textured.glb: the simplified (else the post-processed) mesh with an atlas at most N texels wide")
    ap.add_argument("--normal-map", action="store_true", default=argparse.SUPPRESS,
                    help="with --texture-size: the views' normals as a tangent-space normal map in tsdf_textured.glb")
    ap.add_argument("--ao", action="store_true", default=argparse.SUPPRESS,
                    help="with --texture-size: ambient occlusion traced against the mesh in the ORM image's R channel (gs2m_mesh_ao.py)")


def simplify_keywords(a, ap=None):
    """-> extract_mesh's simplify keywords from a parsed namespace ({}: neither flag was given)."""
    kw = {k: getattr(a, k) for k in ("simplify_cell", "simplify_triangles") if hasattr(a, k)}
    if len(kw) == 2:
        if ap is None:
            raise ValueError("--simplify-cell and --simplify-triangles: choose one")
        ap.error("--simplify-cell and --simplify-triangles: choose one")
    return kw


def parse_args(argv=None):
    """The command line with render.py's presets applied.  -> (namespace, bounds): bounds (3, 2) is --tnt's aabb_range, else None."""
    ap = argparse.ArgumentParser(description="TSDF mesh of a trained model (render.py --extract_mesh)")
    ap.add_argument("--ply", required=True, help="the model's point_cloud.ply")
    ap.add_argument("--source-path", "-s", required=True, help="COLMAP-format dataset (or NeRF-synthetic with --blender)")
    ap.add_argument("--blender", action="store_true")
    ap.add_argument("--split", choices=("train", "test"), default="train",
                    help="test: transforms_test.json (--blender) or every 8th COLMAP image (the reference's llffhold)")
    ap.add_argument("--resolution", "-r", type=int, default=1)
    ap.add_argument("--output", "-o", required=True)
    ap.add_argument("--max_depth", type=float, default=-1.0)
    ap.add_argument("--voxel_size", type=float, default=-1.0)
    ap.add_argument("--sdf_trunc", type=float, default=-1.0)
    ap.add_argument("--num_clusters", type=int, default=1)
    ap.add_argument("--dtu", action="store_true", help="render.py's DTU preset: 5.0 / 0.002 / 0.008 / 1")
    ap.add_argument("--tnt", action="store_true",
                    help="render.py's Tanks and Temples preset: max_depth 3.0 (barn, caterpillar, ignatius, truck) or 4.5; voxel_size "
                         "max(aabb_range extent) / 2048 and bounds = aabb_range from the dataset's transforms.json, else 0.002; 1 cluster")
    ap.add_argument("--scene", default="", help="--tnt: the scene's name (default: the output directory's name)")
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--host-post", action="store_true", help="post-process on the host (numpy / scipy) instead of the device")
    from gs2m_ingest import add_ingest_arguments
    add_ingest_arguments(ap)  # COLMAP datasets: the alpha masks fuse_depths cuts the depths with
    add_simplify_arguments(ap)
    add_texture_arguments(ap)
    a = ap.parse_args(argv)
    if hasattr(a, "normal_map") and not hasattr(a, "texture_size"):
        ap.error("--normal-map needs --texture-size")
    if hasattr(a, "ao") and not hasattr(a, "texture_size"):
        ap.error("--ao needs --texture-size")
    simplify_keywords(a, ap)
    if a.dtu and a.tnt:
        ap.error("--dtu and --tnt are two presets: choose one")
    bounds = None
    if a.dtu:
        a.max_depth, a.voxel_size, a.sdf_trunc, a.num_clusters = 5.0, 0.002, 4.0 * 0.002, 1
    if a.tnt:
        scene = (a.scene or os.path.basename(os.path.normpath(a.output))).lower()
        a.max_depth, a.num_clusters, a.voxel_size = (3.0 if scene in TNT_360_SCENES else 4.5), 1, 0.002
        tf = os.path.join(a.source_path, "transforms.json")
        if os.path.exists(tf):
            with open(tf) as f:
                aabb = json.load(f).get("aabb_range")
            if aabb is not None:
                bounds = np.asarray(aabb, dtype=np.float64).reshape(3, 2)
                a.voxel_size = float(np.max(bounds[:, 1] - bounds[:, 0])) / 2048
        a.sdf_trunc = 4.0 * a.voxel_size
    return a, bounds


def main(argv=None):
    a, bounds = parse_args(argv)
    import gs2m_train as T
    from gs2m_model import GaussianModel
    if a.blender:
        cams, _, _, _, extent = T.load_blender_dataset(a.source_path, "transforms_test.json" if a.split == "test" else "transforms_train.json")
    else:
        from gs2m_ingest import ingest_keywords
        cams, _, _, _, extent = T.load_colmap_dataset(a.source_path, resolution=a.resolution, **ingest_keywords(a))
        if a.split == "test":
            cams = cams[::8]
    model = GaussianModel(a.sh_degree)
    model.load_ply(a.ply)
    extract_mesh(model, cams, extent, a.output, a.max_depth, a.voxel_size, a.sdf_trunc, a.num_clusters, bounds,
                 host_post=a.host_post, **simplify_keywords(a))
    if hasattr(a, "texture_size"):  # the textured asset, from the simplified mesh when this run wrote one
        from gs2m_mesh_texture import texture_mesh
        source = "tsdf_simplified.ply" if simplify_keywords(a) else "tsdf_post.ply"
        texture_mesh(model, cams, read_mesh(os.path.join(a.output, source)), os.path.join(a.output, "tsdf_textured.glb"),
                     texture_size=a.texture_size, **({"normal_map": True} if hasattr(a, "normal_map") else {}),
                     **({"ao": True} if hasattr(a, "ao") else {}))


if __name__ == "__main__":
    main()
