"""Generates tests/golden/ref_dtu_eval.npz: the REFERENCE's own scripts/eval_dtu/eval.py (mesh mode) run as it is on small
synthetic cases.  Run in the BUILD container only:

    python tests/golden/make_dtu_eval_golden.py

What the image lacks is stood in for HERE, in the generator only (nothing of this travels, nothing of it is product or
oracle code): `open3d` is a module whose read_triangle_mesh / read_point_cloud return the case's arrays and whose
write_point_cloud captures the points and colours; multiprocessing.Pool is a serial map for the run; np.random.default_rng
is seeded.  ObsMask / Plane .mat files are written with scipy.io.savemat and read back by the script's own loadmat.  The
npz holds every case's inputs, the three means of results.json and both captured clouds with their colours (the d2s cloud
is the thinned cloud in shuffled order: it pins sampling, shuffle and thinning bit for bit).  sklearn's kneighbors refuses
an empty query set, so the "NaN" case has a non-empty data_in_obs whose every distance is >= max_dist."""
import json
import multiprocessing
import os
import runpy
import sys
import tempfile
import types

import numpy as np
from scipy.io import savemat

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF_EVAL = "/root/reference/scripts/eval_dtu/eval.py"


def _fibonacci(n):
    k = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * k / n)
    th = np.pi * (1 + 5 ** 0.5) * k
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)


def _mask(bb, res, hole):
    dims = (np.floor((bb[1] - bb[0]) / res).astype(int) + 1).tolist()
    i, j, k = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    m = ((i + 2 * j + 3 * k) % 7 != 0).astype(np.uint8)
    m[hole] = 0
    return m


def case_mc():
    """a marching-cubes mesh of a sphere (tests/mesh_ref.py's restatement of the extraction), STL on a slightly larger sphere
    plus a ground grid partly below the plane"""
    import mesh_ref as MR
    c, r = (1.3, -0.7, 2.1), 4.0
    vol = MR.sphere_volume(c, r, 0.5, 2.0)
    v, _, t = MR.marching_cubes(vol)
    rng = np.random.default_rng(1)
    sph = np.asarray(c) + (r + 0.05) * _fibonacci(1500) + rng.normal(0, 0.02, (1500, 3))
    gx, gz = np.meshgrid(np.linspace(-6, 8, 25), np.linspace(-4, 9, 25))
    ground = np.stack([gx.ravel(), np.full(gx.size, 4.3), gz.ravel()], axis=1)
    stl = np.concatenate([sph, ground])
    bb = np.array([[c[0] - 3.5, c[1] - 4.6, c[2] - 5.1], [c[0] + 4.7, c[1] + 3.3, c[2] + 3.9]])
    hole = (slice(0, 6), slice(None), slice(None))
    return dict(vertices=v.astype(np.float64), triangles=t, stl=stl, bb=bb, res=0.5, obs_mask=_mask(bb, 0.5, hole),
                plane=np.array([0.05, -1.0, 0.1, 3.9]), seed=11, thresh=0.4, patch=0.3, max_dist=2.0, vis=1.0)


def case_edges():
    """zero-area triangles (collinear, repeated vertex), slivers with n1 == 0, a few large triangles, unreferenced vertices,
    points exactly thresh apart"""
    V = [[0.0, 0.0, 0.0], [12.0, 0.0, 0.0], [0.0, 9.0, 0.0],          # 0-2 a large triangle
         [12.0, 9.0, 0.5], [3.0, 3.0, 6.0],                            # 3-4 two more large ones with 1, 2 / 0, 1
         [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [3.0, 3.0, 3.0],            # 5-7 collinear: zero area
         [0.05, 5.0, 1.0], [0.1, 5.0, 1.0], [0.05, 15.0, 1.0],         # 8-10 sliver: |v1| = 0.05 -> n1 == 0
         [0.0, -3.0, 0.0], [0.2, -3.0, 0.0], [0.4, -3.0, 0.0],          # 11-16 unreferenced, multiples of 0.2 apart
         [0.6000000000000001, -3.0, 0.0], [0.0, -3.2, 0.0], [0.0, -3.4, 0.0],
         [5.0, 5.0, -2.0], [5.3, 5.0, -2.0], [5.0, 5.25, -2.0]]       # 17-19 a small triangle
    F = [[0, 1, 2], [1, 3, 2], [0, 1, 4], [5, 6, 7], [5, 5, 6], [8, 9, 10], [10, 9, 8], [17, 18, 19], [2, 4, 3]]
    rng = np.random.default_rng(2)
    stl = np.concatenate([rng.uniform([-1, -4, -3], [13, 10, 7], (2500, 3)), np.asarray(V)[11:17] + 0.1])
    bb = np.array([[-1.1, -3.7, -2.9], [12.9, 9.3, 6.6]])
    hole = (slice(None), slice(None), slice(0, 2))
    return dict(vertices=np.asarray(V), triangles=np.asarray(F, np.int32), stl=stl, bb=bb, res=1.0, obs_mask=_mask(bb, 1.0, hole),
                plane=np.array([0.0, 0.2, 1.0, -0.5]), seed=5, thresh=0.2, patch=0.5, max_dist=1.5, vis=0.75)


def case_nan():
    """data_in_obs non-empty but every d2s distance >= max_dist (mean_d2s is NaN); s2d finite: part A of the mesh lies on the
    STL outside the mask, part B inside the mask far from it"""
    A = [[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]]
    B = [[0.0, 0.0, 9.0], [3.0, 0.0, 9.0], [0.0, 3.0, 9.0]]
    gx, gy = np.meshgrid(np.linspace(0, 3, 16), np.linspace(0, 3, 16))
    stl = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 0.1)], axis=1)
    stl = stl[stl[:, 0] + stl[:, 1] < 3.8]
    bb = np.array([[-1.0, -1.0, -1.0], [5.0, 5.0, 10.0]])
    m = np.zeros((7, 7, 12), np.uint8)
    m[:, :, 8:] = 1
    return dict(vertices=np.asarray(A + B), triangles=np.array([[0, 1, 2], [3, 4, 5]], np.int32), stl=stl, bb=bb, res=1.0,
                obs_mask=m, plane=np.array([0.0, 0.0, 1.0, 0.0]), seed=0, thresh=0.3, patch=60.0, max_dist=3.0, vis=2.0)


CASES = {"mc": case_mc, "edges": case_edges, "nan": case_nan}


class _SerialPool:
    def __init__(self, *a, **k):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def map(self, f, it, chunksize=None):
        return list(map(f, it))


def run_reference(cs, scan=7):
    captured = {}

    class PointCloud:
        points = None
        colors = None

    o3d = types.ModuleType("open3d")
    o3d.geometry = types.SimpleNamespace(PointCloud=PointCloud)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: np.array(a, dtype=np.float64))
    o3d.io = types.SimpleNamespace(
        read_triangle_mesh=lambda path: types.SimpleNamespace(vertices=np.array(cs["vertices"], np.float64),
                                                              triangles=np.array(cs["triangles"], np.int32)),
        read_point_cloud=lambda path: types.SimpleNamespace(points=np.array(cs["stl"], np.float64)),
        write_point_cloud=lambda f, pcd: captured.__setitem__(os.path.basename(f), (np.array(pcd.points), np.array(pcd.colors))))
    saved = sys.modules.get("open3d"), multiprocessing.Pool, np.random.default_rng, sys.argv
    orig_rng = np.random.default_rng
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "ObsMask"))
        savemat(os.path.join(d, "ObsMask", f"ObsMask{scan}_10.mat"),
                {"ObsMask": cs["obs_mask"], "BB": cs["bb"], "Res": np.array([[cs["res"]]])})
        savemat(os.path.join(d, "ObsMask", f"Plane{scan}.mat"), {"P": cs["plane"].reshape(1, 4)})
        try:
            sys.modules["open3d"] = o3d
            multiprocessing.Pool = _SerialPool
            np.random.default_rng = lambda *a, **k: orig_rng(cs["seed"])
            sys.argv = [REF_EVAL, "--data", "mesh.ply", "--scan", str(scan), "--mode", "mesh", "--dataset_dir", d, "--vis_out_dir", d,
                        "--downsample_density", repr(cs["thresh"]), "--patch_size", repr(cs["patch"]), "--max_dist", repr(cs["max_dist"]),
                        "--visualize_threshold", repr(cs["vis"])]
            runpy.run_path(REF_EVAL, run_name="__main__")
        finally:
            if saved[0] is None:
                sys.modules.pop("open3d", None)
            else:
                sys.modules["open3d"] = saved[0]
            multiprocessing.Pool, np.random.default_rng, sys.argv = saved[1], saved[2], saved[3]
        res = json.load(open(os.path.join(d, "results.json")))
    return res, captured[f"vis_{scan:03}_d2s.ply"], captured[f"vis_{scan:03}_s2d.ply"]


def main():
    out = {}
    for name, make in CASES.items():
        cs = make()
        res, (dp, dc), (sp, sc) = run_reference(cs)
        assert np.array_equal(sp, cs["stl"])
        for k in ("vertices", "triangles", "stl", "bb", "obs_mask", "plane"):
            out[f"{name}/{k}"] = np.asarray(cs[k])
        for k in ("res", "seed", "thresh", "patch", "max_dist", "vis"):
            out[f"{name}/{k}"] = np.asarray(cs[k])
        for k in ("mean_d2s", "mean_s2d", "overall"):
            out[f"{name}/{k}"] = np.float64(res[k])
        out[f"{name}/d2s_points"] = dp
        out[f"{name}/d2s_colors"] = dc
        out[f"{name}/s2d_colors"] = sc
        print(f"{name}: V {len(cs['vertices'])} F {len(cs['triangles'])} down {len(dp)} stl {len(sp)} -> "
              f"d2s {res['mean_d2s']} s2d {res['mean_s2d']} overall {res['overall']}")
    path = os.path.join(HERE, "ref_dtu_eval.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
