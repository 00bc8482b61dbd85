"""Visibility cull of a mesh against a camera trajectory on the GPU (csrc/mesh_depth.hip; include/gs2m_visibility.h).

The reference's scripts/eval_tnt/cull_mesh.py, as DESIGN.md §14 writes the contract down: the mesh's depth is rendered from
every camera (a z-buffer rasterizer in HIP instead of pyrender's OpenGL), every vertex is projected into every view and votes
where it lies inside the frame and not behind the rendered surface (z < depth + eps); vertices with at least `min_views` votes
are kept, then the faces whose three vertices are kept, then the vertices those faces still name.  Everything is fp64 on device
tensors owned here; there is no CPU path.

    python gs-2m_amd/gs2m_mesh_cull.py --traj-path T.log --ply-path M.ply [--out M_cull.ply]
writes M_cull.ply beside M.ply.  T holds camera-to-world matrices (.log or .npy) in the OpenCV convention; --opengl is for poses
in the GL convention (the y and z columns are flipped first, the reference's c2w[:3, 1:3] *= -1).
"""
import argparse
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np
import torch

import gs2m_native as N
from gs2m_eval_util import compact as _compact, device as _dev, ptr as _ptr, workspace_for

# scripts/eval_tnt/cull_mesh.py: the Tanks and Temples frame and the constants of extract_depth_from_mesh / point_masks
TNT_WIDTH, TNT_HEIGHT = 1920, 1080
TNT_FX, TNT_FY = 1163.8678928442187, 1172.793101201448
TNT_CX, TNT_CY = 962.3120628412543, 542.0667209577691
NEAR, FAR, EPS, MIN_VIEWS = 0.01, 20.0, 0.005, 20
VIEW_BATCH = 8  # views rendered per call: they share the triangle loads and one depth buffer


def _on_device(t, name, who, dtype, cols):
    """`t` as a contiguous (n, cols...) tensor of `dtype`, after checking that it is a tensor on a HIP device"""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{who}: `{name}` must be a tensor on a HIP device; there is no CPU path")
    return t.to(dtype).reshape((-1,) + cols).contiguous()


def _mesh_args(vertices, triangles, w2c, who):
    v = _on_device(vertices, "vertices", who, torch.float64, (3,))
    f = None if triangles is None else _on_device(triangles, "triangles", who, torch.int32, (3,))
    m = _on_device(w2c, "w2c", who, torch.float64, (4, 4))
    return v, f, m


def _mesh_on_device(mesh, device, who):
    """a mesh -- anything with .vertices and .triangles as numpy arrays or tensors -> its checked (vertices (V, 3) float64,
    triangles (F, 3) int32) on `device`"""
    v, f = mesh.vertices, mesh.triangles
    v = v.to(device) if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, np.float64)).to(device)
    f = f.to(device) if torch.is_tensor(f) else torch.as_tensor(np.asarray(f, np.int32)).to(device)
    return _on_device(v, "vertices", who, torch.float64, (3,)), _on_device(f, "triangles", who, torch.int32, (3,))


def render_mesh_depth(vertices, triangles, w2c, fx, fy, cx, cy, H, W, near=NEAR, far=FAR, out=None):
    """The mesh's depth from every view: (n_views, H, W) float32 on the device, the camera-space z of the nearest surface through
    each pixel centre (i + 0.5, j + 0.5), 0 where there is none.  vertices (V, 3), triangles (F, 3), w2c (n_views, 4, 4)
    world-to-camera, OpenCV convention: device tensors.  out: a float32 buffer of at least n_views H W elements to render into."""
    who = "render_mesh_depth"
    v, f, m = _mesh_args(vertices, triangles, w2c, who)
    dev, n = v.device, len(m)
    if out is None:
        depth = torch.empty((n, int(H), int(W)), dtype=torch.float32, device=dev)
    else:
        if not torch.is_tensor(out) or out.device != dev or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < n * int(H) * int(W):
            raise RuntimeError(f"{who}: `out` must be a contiguous float32 tensor of at least {n * int(H) * int(W)} elements on {dev}")
        depth = out.reshape(-1)[: n * int(H) * int(W)].view(n, int(H), int(W))
    ws = workspace_for("gs2m_meshdepth_workspace_bytes", dev, len(f), n)
    N.launch("gs2m_meshdepth_render", dev, len(v), _ptr(v), len(f), _ptr(f), n, _ptr(m), float(fx), float(fy), float(cx), float(cy),
             int(W), int(H), float(near), float(far), _ptr(ws), _ptr(depth))
    return depth


def visibility_votes(vertices, w2c, fx, fy, cx, cy, depth, eps=EPS, out=None):
    """The number of views that see each vertex: inside the frame and, where the bilinear sample d of the view's depth is > 0,
    z < d + eps.  depth: (n_views, H, W) float32 device tensor.  out: an int32 (V,) tensor the votes are ADDED to (views taken
    batch by batch); without it a new tensor.  -> int32 (V,)."""
    who = "visibility_votes"
    v, _, m = _mesh_args(vertices, None, w2c, who)
    d = _on_device(depth, "depth", who, torch.float32, ())
    if depth.dim() != 3 or depth.shape[0] != len(m):
        raise RuntimeError(f"{who}: `depth` must have shape (n_views, H, W) with n_views = {len(m)}, got {tuple(depth.shape)}")
    H, W = int(depth.shape[1]), int(depth.shape[2])
    if out is not None and (not torch.is_tensor(out) or out.device != v.device or out.dtype != torch.int32 or tuple(out.shape) != (len(v),)
                            or not out.is_contiguous()):
        raise RuntimeError(f"{who}: `out` must be a contiguous int32 tensor of shape ({len(v)},) on {v.device}")
    votes = torch.empty(len(v), dtype=torch.int32, device=v.device) if out is None else out
    N.launch("gs2m_visibility_votes", v.device, len(v), _ptr(v), len(m), _ptr(m), float(fx), float(fy), float(cx), float(cy), W, H,
             _ptr(d), float(eps), 0 if out is None else 1, _ptr(votes))
    return votes


def keep_flags(votes, min_views=MIN_VIEWS):
    """uint8 (V,): 1 where votes >= min_views"""
    t = _on_device(votes, "votes", "keep_flags", torch.int32, ())
    keep = torch.empty(len(t), dtype=torch.uint8, device=t.device)
    N.launch("gs2m_visibility_keep", t.device, len(t), _ptr(t), int(min_views), _ptr(keep))
    return keep


def cull_mesh_by_visibility(vertices, triangles, w2c, fx, fy, cx, cy, H, W, near=NEAR, far=FAR, eps=EPS, min_views=MIN_VIEWS,
                            view_batch=None, colors=None):
    """cull_mesh.py's Mesher.cull_mesh: the views are rendered and voted on `view_batch` at a time (default VIEW_BATCH) into one
    reused depth buffer; the vertices with at least `min_views` votes are kept, then the faces whose three vertices are kept, then
    the vertices those faces name, in their order.  colors: (V, 3) per-vertex values carried along.
    -> (vertices (V', 3) fp64, triangles (F', 3) int32, [colors (V', 3) fp64,] votes (V,) int32), device tensors."""
    import ctypes as C
    who = "cull_mesh_by_visibility"
    v, f, m = _mesh_args(vertices, triangles, w2c, who)
    col = None if colors is None else _on_device(colors, "colors", who, torch.float64, (3,))
    if col is not None and len(col) != len(v):
        raise RuntimeError(f"{who}: {len(col)} colours for {len(v)} vertices")
    dev = v.device
    batch = max(1, min(int(view_batch or VIEW_BATCH), max(len(m), 1)))
    votes = torch.zeros(len(v), dtype=torch.int32, device=dev)
    buf = torch.empty(batch * int(H) * int(W), dtype=torch.float32, device=dev)
    for k in range(0, len(m), batch):
        part = m[k:k + batch]
        depth = render_mesh_depth(v, f, part, fx, fy, cx, cy, H, W, near, far, out=buf)
        visibility_votes(v, part, fx, fy, cx, cy, depth, eps, out=votes)
    if len(m) == 0:  # no view: the indices are still checked
        render_mesh_depth(v, f, m, fx, fy, cx, cy, H, W, near, far, out=buf)
    keep = keep_flags(votes, min_views)
    flags = torch.empty_like(keep)
    N.launch("gs2m_visibility_referenced", dev, len(v), _ptr(keep), len(f), _ptr(f), _ptr(flags))
    out_f = torch.empty_like(f)
    ws = workspace_for("gs2m_eval_cull_workspace_bytes", dev, len(v), len(f))
    tot = (C.c_longlong * 2)()
    N.launch("gs2m_eval_cull_triangles", dev, len(v), _ptr(flags), len(f), _ptr(f), _ptr(ws), _ptr(out_f), tot)
    out = (_compact(v, flags, 0, dev).clone(), out_f[:tot[1]].clone())
    if col is not None:
        out += (_compact(col, flags, 0, dev).clone(),)
    return out + (votes,)


# ---- files -------------------------------------------------------------------------------------------------------------------

def world_to_camera(c2w, opengl=False):
    """(n, 4, 4) camera-to-world poses -> world-to-camera matrices in the OpenCV convention (numpy, fp64).  opengl: the poses
    look along -z with y up; their y and z columns are flipped first."""
    c = np.array(c2w, np.float64).reshape(-1, 4, 4)
    if opengl:
        c[:, :3, 1:3] *= -1
    return np.linalg.inv(c) if len(c) else c


def cull_file(ply_path, traj_path, out_path=None, opengl=False, width=TNT_WIDTH, height=TNT_HEIGHT, fx=TNT_FX, fy=TNT_FY, cx=TNT_CX,
              cy=TNT_CY, near=NEAR, far=FAR, eps=EPS, min_views=MIN_VIEWS, view_batch=None, device=None):
    """The command line's work: reads the mesh and the trajectory, culls, writes the mesh.  -> dict(out, n_views, the counts)."""
    import types
    import gs2m_mesh as M
    from gs2m_tnt_eval import read_trajectory
    dev = _dev(device)
    mesh = M.read_mesh(ply_path)
    w2c = world_to_camera(read_trajectory(traj_path), opengl)
    v, f = _mesh_on_device(mesh, dev, "cull_file")
    c = torch.zeros_like(v) if mesh.vertex_colors is None else torch.as_tensor(np.asarray(mesh.vertex_colors, np.float64).reshape(-1, 3)).to(dev)
    cv, cf, cc, votes = cull_mesh_by_visibility(v, f, torch.as_tensor(w2c).to(dev), fx, fy, cx, cy, height, width, near, far, eps,
                                                min_views, view_batch, colors=c)
    out_path = out_path or str(ply_path).replace(".ply", "_cull.ply")
    M.write_mesh(out_path, types.SimpleNamespace(vertices=cv.cpu().numpy(), triangles=cf.cpu().numpy(), vertex_colors=cc.cpu().numpy()))
    return {"out": out_path, "n_views": int(len(w2c)), "n_vertices": int(len(v)), "n_triangles": int(len(f)),
            "n_vertices_kept": int(len(cv)), "n_triangles_kept": int(len(cf))}


def parser():
    ap = argparse.ArgumentParser(description="Visibility cull of a mesh against a camera trajectory (scripts/eval_tnt/cull_mesh.py)")
    ap.add_argument("--traj-path", required=True, help="camera-to-world poses (.log or .npy)")
    ap.add_argument("--ply-path", required=True, help="the mesh to cull (binary PLY)")
    ap.add_argument("--out", default="", help="default: <ply-path without .ply>_cull.ply")
    ap.add_argument("--opengl", action="store_true", help="the poses are in the OpenGL convention (y up, looking along -z)")
    ap.add_argument("--width", type=int, default=TNT_WIDTH)
    ap.add_argument("--height", type=int, default=TNT_HEIGHT)
    ap.add_argument("--fx", type=float, default=TNT_FX)
    ap.add_argument("--fy", type=float, default=TNT_FY)
    ap.add_argument("--cx", type=float, default=TNT_CX)
    ap.add_argument("--cy", type=float, default=TNT_CY)
    ap.add_argument("--near", type=float, default=NEAR)
    ap.add_argument("--far", type=float, default=FAR)
    ap.add_argument("--eps", type=float, default=EPS, help="a vertex is in front when z < depth + eps")
    ap.add_argument("--min-views", type=int, default=MIN_VIEWS, help="views that must see a vertex for it to stay")
    ap.add_argument("--view-batch", type=int, default=VIEW_BATCH, help="views rendered per call")
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    r = cull_file(a.ply_path, a.traj_path, a.out.strip() or None, a.opengl, a.width, a.height, a.fx, a.fy, a.cx, a.cy, a.near, a.far,
                  a.eps, a.min_views, a.view_batch)
    print(f"[>] {r['n_views']} views: kept {r['n_vertices_kept']} of {r['n_vertices']} vertices, {r['n_triangles_kept']} of "
          f"{r['n_triangles']} triangles -> {r['out']}")
    return r


if __name__ == "__main__":
    main()
