"""What the mesh evaluators (gs2m_dtu_eval.py, gs2m_tnt_eval.py) and the mesh extraction (gs2m_mesh.py) share on the host
side: device and tensor plumbing for the fp64 point kernels of csrc/mesh_eval.hip, workspaces sized by the library, the
compaction, the target grid of the nearest-neighbour queries, the fixed-order masked mean and the point-cloud PLY files."""
import ctypes as C
import math

import numpy as np
import torch

import gs2m_native as N

ptr = N.ptr


def device(dev):
    return torch.device(dev if dev is not None else "cuda")


_device = device  # for the functions below whose own parameter is called `device`


def points(a, dev):
    """(n, 3) fp64 contiguous tensor on `dev` (numpy or torch input; a tensor that already is one comes back as it is)."""
    t = torch.as_tensor(a)
    return t.to(device=dev, dtype=torch.float64).reshape(-1, 3).contiguous()


def triangles_i32(triangles, dev):
    """(F, 3) int32 contiguous tensor on `dev` (numpy or torch input)."""
    f = torch.as_tensor(np.asarray(triangles, dtype=np.int64).reshape(-1, 3) if not torch.is_tensor(triangles) else triangles)
    return f.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()


def workspace(nbytes, dev):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def workspace_for(fn_name, dev, *sizes, only=None):
    """The workspace on `dev` whose size the library's `fn_name`(*sizes, &bytes) reports.  A function that reports two sizes
    gives the pair; `only` = 0 or 1 asks for that one alone (the other size is not asked for: its pointer is NULL)."""
    fn = getattr(N.lib(), fn_name)
    out = [C.c_longlong() if only in (None, k) else None for k in range(len(fn.argtypes) - len(sizes))]
    N.check(fn(*sizes, *[b if b is None else C.byref(b) for b in out]), fn_name)
    ws = [workspace(b.value, dev) for b in out if b is not None]
    return ws[0] if len(ws) == 1 else tuple(ws)


def compact(p, flags, bit, dev):
    """The points whose flag byte has `bit` set, in index order.  -> a view of the first rows of a buffer of len(p) rows:
    clone it to let the buffer go."""
    out = torch.empty_like(p)
    cnt = C.c_longlong()
    ws = workspace_for("gs2m_eval_scan_workspace_bytes", dev, len(p))
    N.launch("gs2m_eval_compact", dev, len(p), ptr(p), ptr(flags), int(bit), ptr(ws), ptr(out), C.byref(cnt))
    return out[:cnt.value]


def grid_cell(targets, max_dist):
    """The grid edge for nearest-neighbour queries against `targets` (a device tensor): about two point spacings of a surface
    sample (2 extent / sqrt(n)), never below a volume's spacing (extent / cbrt(n)), and within [max_dist / 128, max_dist] so
    that the walk's shells and the coarse bound stay few."""
    n = len(targets)
    if n == 0:
        return max_dist
    lo, hi = torch.aminmax(targets, dim=0)
    ext = float((hi - lo).max())
    h = max(2.0 * ext / math.sqrt(n), ext / n ** (1.0 / 3.0)) if ext > 0 else max_dist
    return min(max(h, max_dist / 128.0), max_dist)


class TargetGrid:
    """The hashed grid over a target cloud, built once and queried many times (an ICP stage: once per iteration)."""

    def __init__(self, targets, max_dist, cell=None, device=None):
        self.dev = _device(device)
        self.targets = points(targets, self.dev)
        self.cell = float(cell) if cell else grid_cell(self.targets, max_dist)
        self.grid, bws = workspace_for("gs2m_eval_grid_bytes", self.dev, len(self.targets))  # bws: gone when this returns
        N.launch("gs2m_eval_grid_build", self.dev, len(self.targets), ptr(self.targets), self.cell, ptr(self.grid), ptr(bws))

    def query(self, queries, max_dist):
        """-> (index int64 tensor, dist tensor): index -1 and dist +inf where nothing lies within max_dist"""
        q = points(queries, self.dev)
        index = torch.empty(len(q), dtype=torch.int64, device=self.dev)
        dist = torch.empty(len(q), dtype=torch.float64, device=self.dev)
        N.launch("gs2m_eval_nearest_index", self.dev, len(q), ptr(q), len(self.targets), self.cell, ptr(self.grid), float(max_dist),
                 ptr(index), ptr(dist))
        return index, dist

    def distances(self, queries, max_dist):
        """-> dist tensor alone (the same minimum over the same candidates, no index kept)"""
        q = points(queries, self.dev)
        dist = torch.empty(len(q), dtype=torch.float64, device=self.dev)
        N.launch("gs2m_eval_nearest", self.dev, len(q), ptr(q), len(self.targets), self.cell, ptr(self.grid), float(max_dist), ptr(dist))
        return dist


def masked_mean(dist, max_dist, device=None):
    """mean of the entries < max_dist (NaN when there is none), summed in a fixed order on the device.  -> (mean, count)."""
    dev = _device(device)
    d = torch.as_tensor(dist).to(dev, torch.float64).contiguous()
    tot, cnt = C.c_double(), C.c_longlong()
    ws = workspace_for("gs2m_eval_scan_workspace_bytes", dev, 0)  # the partials only: they sit in front for every n
    N.launch("gs2m_eval_masked_mean", dev, len(d), ptr(d), float(max_dist), ptr(ws), C.byref(tot), C.byref(cnt))
    return (tot.value / cnt.value if cnt.value else float("nan")), cnt.value


# ---- files -------------------------------------------------------------------------------------------------------------------

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2",
              "uint16": "<u2", "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4",
              "double": "<f8", "float64": "<f8"}


def read_ply(file):
    """Binary little-endian PLY -> (vertices (V, 3) fp64, triangles (F, 3) int32; empty without a face element).  Vertex
    coordinates are widened to fp64 exactly as stored (float or double); other scalar properties are skipped."""
    with open(str(file), "rb") as f:
        data = f.read()
    if not data.startswith(b"ply"):
        raise ValueError(f"{file}: not a PLY file")
    end = data.find(b"end_header\n")
    if end < 0:
        raise ValueError(f"{file}: PLY header without end_header")
    end += len(b"end_header\n")
    lines = data[:end].decode("ascii", "replace").split("\n")
    fmt = [ln for ln in lines if ln.startswith("format")]
    if not fmt or fmt[0].split()[1] != "binary_little_endian":
        raise ValueError(f"{file}: {fmt[0] if fmt else 'no format line'}: only binary little-endian PLY is read (convert ASCII PLY first)")
    elems = []
    for ln in lines:
        p = ln.split()
        if not p:
            continue
        if p[0] == "element":
            elems.append([p[1], int(p[2]), []])
        elif p[0] == "property":
            elems[-1][2].append(p[1:])
    off, verts, tris = end, np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int32)
    for name, n, props in elems:
        if props and props[0][0] == "list":
            if len(props) != 1:
                raise ValueError(f"{file}: element {name}: a list with other properties is not read")
            dt = np.dtype([("n", _PLY_TYPES[props[0][1]]), ("v", _PLY_TYPES[props[0][2]], (3,))])
            a = np.frombuffer(data, dt, n, off)
            if n and not np.all(a["n"] == 3):
                raise ValueError(f"{file}: only triangle faces are read")
            off += dt.itemsize * n
            if name == "face":
                tris = a["v"].astype(np.int32)
            continue
        dt = np.dtype([(q[1], _PLY_TYPES[q[0]]) for q in props])
        a = np.frombuffer(data, dt, n, off)
        off += dt.itemsize * n
        if name == "vertex":
            verts = np.stack([a[k].astype(np.float64) for k in "xyz"], axis=1) if n else np.zeros((0, 3), np.float64)
    return verts, tris


def write_point_cloud(file, points, colors=None, normals=None):
    """Binary little-endian PLY: double x y z, uchar red green blue (colour * 255 rounded to nearest).  With `normals` the file
    is what Open3D's write_point_cloud writes by default: its comment line, then double x y z, double nx ny nz, uchar red
    green blue."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    if normals is not None:
        fields += [("nx", "<f8"), ("ny", "<f8"), ("nz", "<f8")]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    a = np.zeros(len(p), np.dtype(fields))
    for k, n in enumerate("xyz"):
        a[n] = p[:, k]
    head = "ply\nformat binary_little_endian 1.0\n" + ("comment Created by Open3D\n" if normals is not None else "")
    head += f"element vertex {len(p)}\nproperty double x\nproperty double y\nproperty double z\n"
    if normals is not None:
        nrm = np.asarray(normals, np.float64).reshape(-1, 3)
        if len(nrm) != len(p):
            raise ValueError(f"write_point_cloud: {len(nrm)} normals for {len(p)} points")
        for k, n in enumerate(("nx", "ny", "nz")):
            a[n] = nrm[:, k]
        head += "property double nx\nproperty double ny\nproperty double nz\n"
    if colors is not None:
        c = np.clip(np.rint(np.asarray(colors, np.float64).reshape(-1, 3) * 255.0), 0, 255).astype(np.uint8)
        for k, n in enumerate(("red", "green", "blue")):
            a[n] = c[:, k]
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    with open(str(file), "wb") as f:
        f.write((head + "end_header\n").encode("ascii"))
        f.write(a.tobytes())
