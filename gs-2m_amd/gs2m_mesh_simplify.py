"""Simplify a mesh: vertex clustering on a lattice with quadric placement, on the GPU (csrc/mesh_simplify.hip,
include/gs2m_simplify.h; gs2m_mesh.simplify_mesh_gpu).

    python gs-2m_amd/gs2m_mesh_simplify.py --ply-path IN.ply -o OUT.ply (--cell X | --triangles N)

IN is a plain mesh (gs2m_mesh.write_mesh: positions and colours) or a material mesh (gs2m_mesh_bake.py: albedo, roughness,
metallic, seen), told apart by its vertex properties.  A material mesh keeps its five channels, averaged within a cell over
the vertices that were `seen` (over all of them where none was: that vertex comes out unseen) -- an `occlusion` property
(gs2m_mesh_bake.py --ao) is a sixth channel, averaged like the roughness --, and is written as a material mesh again, so that gs2m_mesh_view.py --colour pbr loads the result as it loads the input.
"""
import argparse
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np
import torch


def parser():
    ap = argparse.ArgumentParser(description="Simplify a mesh by vertex clustering with quadric placement")
    ap.add_argument("--ply-path", "--ply_path", required=True, help="the mesh (binary PLY), plain or material")
    ap.add_argument("--output", "-o", required=True, help="the simplified mesh to write")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--cell", type=float, help="the lattice's edge length")
    g.add_argument("--triangles", type=int, help="at most this many triangles: the lattice edge is searched for")
    ap.add_argument("--device", default="cuda")
    return ap


def is_material_ply(file):
    """The header names roughness and metallic vertex properties."""
    with open(str(file), "rb") as f:
        head = f.read(4096).split(b"end_header")[0].decode("ascii", "replace")
    names = [ln.split()[-1] for ln in head.split("\n") if ln.startswith("property")]
    return "roughness" in names and "metallic" in names


def load(file):
    """-> (TriangleMesh, values (V, 5) or None -- (V, 6) with an occlusion property, the last column --, seen (V,) float32 or None)."""
    import gs2m_mesh as M
    if not is_material_ply(file):
        return M.read_mesh(file), None, None
    from gs2m_mesh_bake import read_material_mesh
    m = read_material_mesh(file)
    values = np.concatenate([m["albedo"], m["roughness"][:, None], m["metallic"][:, None]] +
                            ([m["occlusion"][:, None]] if "occlusion" in m else []), axis=1).astype(np.float32)
    return M.TriangleMesh(m["vertices"], m["triangles"], m["albedo"]), values, m["seen"].astype(np.float32)


def save(file, mesh, values=None, weight=None):
    """A material mesh when `values` are given (seen = weight > 0), else a plain one."""
    import gs2m_mesh as M
    if values is None:
        M.write_mesh(file, mesh)
        return
    from gs2m_mesh_bake import write_material_mesh
    host = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    values = host(values)
    write_material_mesh(file, host(mesh.vertices), host(mesh.triangles), values[:, :5], host(weight) > 0,
                        values[:, 5] if values.shape[1] == 6 else None)


def main(argv=None):
    a = parser().parse_args(argv)
    import gs2m_mesh as M
    mesh, values, seen = load(a.ply_path)
    if values is None:
        out, info = M.simplify_mesh_gpu(mesh, cell=a.cell, target_triangles=a.triangles, device=a.device, extras=True)
        save(a.output, out)
    else:
        out, info = M.simplify_mesh_gpu(mesh, cell=a.cell, target_triangles=a.triangles, attributes=values, weights=seen, device=a.device)
        save(a.output, out, info["attributes"], info["weight"])
    print(f"[>] {len(mesh.vertices)} vertices / {len(mesh.triangles)} triangles -> {len(out.vertices)} / {len(out.triangles)} at cell "
          f"{info['cell']} -> {a.output}")
    return {"out": a.output, "cell": info["cell"], "material": values is not None, "n_vertices": int(len(out.vertices)),
            "n_triangles": int(len(out.triangles)), "input_triangles": int(len(mesh.triangles))}


if __name__ == "__main__":
    main()
