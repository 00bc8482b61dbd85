"""Mesh simplification timed on tools/mesh_bake_bench.py's scene: tools/mesh_bench.py's sphere and ground disc fused from 49
views at 1600 x 1200 and extracted at `--voxel`, then clustered at cell = 2, 4 and 8 voxels.  Per cell: (a) gs2m_simplify as
simplify_mesh_gpu calls it, without attributes beyond the three colour channels, (b) its five stages -- keys + sorts,
quadrics, placement (with the cell means and attributes), triangle remap + dedupe, compaction -- with the library's stage
clock, which waits for the stream at every stage boundary, (c) the count-only probe, and (d) the same result formed with
torch operators on the same GPU: torch.unique over the cell keys, index_add_ for the sums, torch.linalg.eigh for the solve,
torch.unique over the sorted triples.  Each figure is the median of `--repeats` timed passes after one warm-up, bracketed by
synchronisations; writes profiles/mesh_simplify_bench.json (or `--out`) and prints it.  Nothing has measured this before: no
threshold.  All data is synthetic.

    python tools/mesh_simplify_bench.py [--views 49] [--voxel 0.004] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-2m_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gs2m_mesh as M  # noqa: E402

W, H = 1600, 1200


def timed(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out), min(out), max(out)


def torch_simplify(v, f, col, cell):
    """The contract with torch operators (index_add_ sums: their order is the atomics').  -> (vertices, triangles, colours)."""
    v64 = v.double()
    idx = torch.floor(v64 / cell).long()
    mn = idx.min(dim=0).values
    rel = idx - mn
    key = (rel[:, 0] << 42) | (rel[:, 1] << 21) | rel[:, 2]
    uk, vcell = torch.unique(key, return_inverse=True)
    C = len(uk)
    cidx = torch.stack([uk >> 42, (uk >> 21) & ((1 << 21) - 1), uk & ((1 << 21) - 1)], dim=1) + mn
    centre = (cidx.double() + 0.5) * cell
    cnt = torch.zeros(C, dtype=torch.float64, device=v.device).index_add_(0, vcell, torch.ones(len(v), dtype=torch.float64, device=v.device))
    m = torch.zeros((C, 3), dtype=torch.float64, device=v.device).index_add_(0, vcell, v64 - centre[vcell]) / cnt[:, None]
    csum = torch.zeros((C, 3), dtype=torch.float64, device=v.device).index_add_(0, vcell, col.double()) / cnt[:, None]
    fl = f.long()
    ct = vcell[fl]
    valid = (torch.ones(len(f), dtype=torch.bool, device=v.device), ct[:, 1] != ct[:, 0], (ct[:, 2] != ct[:, 0]) & (ct[:, 2] != ct[:, 1]))
    Q = torch.zeros((C, 12), dtype=torch.float64, device=v.device)
    for k in range(3):
        sel = valid[k]
        cells = ct[sel, k]
        p = v64[fl[sel]] - centre[cells][:, None]
        n = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1)
        ln = n.norm(dim=1)
        ok = ln > 0
        n, ln, cells, p0 = n[ok], ln[ok], cells[ok], p[ok, 0]
        d = -(n * p0).sum(dim=1)
        Q.index_add_(0, cells, torch.cat([(n[:, :, None] * n[:, None, :]).reshape(-1, 9), n * d[:, None]], dim=1) / ln[:, None])
    A, b = Q[:, :9].reshape(C, 3, 3), Q[:, 9:]
    l, U = torch.linalg.eigh(A)
    lmax = l.max(dim=1).values
    inv = torch.where(l > 1e-3 * lmax[:, None], 1.0 / l, torch.zeros_like(l))
    r = -b - torch.einsum("cij,cj->ci", A, m)
    z = m + torch.einsum("cik,ck->ci", U, torch.einsum("cik,ci->ck", U, r) * inv)
    good = (lmax > 0) & (z.abs() <= 0.5 * cell).all(dim=1)
    pos = centre + torch.where(good[:, None], z, m)
    distinct = valid[1] & valid[2] & (ct[:, 1] != ct[:, 2])
    cand = torch.nonzero(distinct)[:, 0]
    st = torch.sort(ct[cand], dim=1).values
    _, inverse = torch.unique(st, dim=0, return_inverse=True)
    first = torch.full((int(inverse.max()) + 1 if len(inverse) else 0,), len(f), dtype=torch.long, device=v.device)
    first.scatter_reduce_(0, inverse, cand, reduce="amin")
    kept = torch.sort(first).values
    used = torch.zeros(C, dtype=torch.bool, device=v.device)
    used[ct[kept].reshape(-1)] = True
    newid = torch.cumsum(used.long(), 0) - 1
    return pos[used].float(), newid[ct[kept]].int(), csum[used].float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--voxel", type=float, default=0.004)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_simplify_bench.json"))
    a = ap.parse_args()
    import mesh_bench as MBench
    cams, depths, colors = MBench.scene(200_000, a.views, W, H)
    lo, hi = M._depth_aabb(depths, cams, 10.0, torch.device("cuda"))
    L, tr = 16 * a.voxel, 4 * a.voxel
    _, mesh, _, _ = MBench.fuse(cams, depths, colors, a.voxel, 10.0, 4096, lo - tr - L, hi + tr + L)
    del depths, colors
    dev = torch.device("cuda")
    dm = M.DeviceMesh(torch.as_tensor(np.asarray(mesh.vertices, np.float32)).to(dev), torch.as_tensor(np.asarray(mesh.triangles, np.int32)).to(dev),
                      torch.as_tensor(np.asarray(mesh.vertex_colors, np.float32)).to(dev))
    ms = lambda t: {"median_ms": round(t[0], 3), "min_ms": round(t[1], 3), "max_ms": round(t[2], 3)}
    result = {"workload": f"{a.views} views {W}x{H}, voxel {a.voxel}, synthetic surface scene; 3 colour channels", "n_vertices": len(dm.vertices),
              "n_triangles": len(dm.triangles), "repeats": a.repeats, "cells": {}}
    for mult in (2, 4, 8):
        cell = mult * a.voxel
        t_all = timed(lambda: M.simplify_mesh_gpu(dm, cell=cell), a.repeats)
        t_count = timed(lambda: M.simplify_count_gpu(dm.vertices, dm.triangles, cell), a.repeats)
        M.simplify_stage_times(True)
        stages = []
        try:
            M.simplify_mesh_gpu(dm, cell=cell)
            for _ in range(a.repeats):
                M.simplify_mesh_gpu(dm, cell=cell)
                stages.append(M.simplify_stage_times())
        finally:
            M.simplify_stage_times(False)
        stage_ms = {k: round(statistics.median(s[k] for s in stages), 3) for k in M.SIMPLIFY_STAGES}
        t_torch = timed(lambda: torch_simplify(dm.vertices, dm.triangles, dm.vertex_colors, cell), a.repeats)
        out = M.simplify_mesh_gpu(dm, cell=cell)
        tv, tt, tc = torch_simplify(dm.vertices, dm.triangles, dm.vertex_colors, cell)
        same = tuple(tv.shape) == tuple(out.vertices.shape) and torch.equal(tt, out.triangles)
        result["cells"][f"{mult}_voxels"] = {
            "cell": cell, "out_vertices": len(out.vertices), "out_triangles": len(out.triangles),
            "simplify_mesh_gpu": ms(t_all), "count_only": ms(t_count), "stages_ms": stage_ms,
            "slowest_stage": max(stage_ms, key=stage_ms.get), "torch_route": ms(t_torch), "torch_over_device": round(t_torch[0] / t_all[0], 2),
            "same_triangles_as_torch": bool(same),
            "max_abs_position_difference_to_torch": float((tv - out.vertices).abs().max()) if same and len(tv) else None,
            "max_abs_colour_difference_to_torch": float((tc - out.vertex_colors).abs().max()) if same and len(tv) else None}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
