"""Mesh extraction on the GPU: tsdf.hip against the numpy restatement of its contract (tests/mesh_ref.py), determinism,
pool growth, an analytic sphere, the synthetic surface scene end to end, and the command line."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as R  # noqa: E402
import gs2m_mesh as M  # noqa: E402

pytestmark = pytest.mark.gpu


def _look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """W2C (4, 4) of a camera at `eye` looking at `target` (x right, y down, z forward)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64), z)
    if np.linalg.norm(x) < 1e-6:
        x = np.cross(np.array([1.0, 0.0, 0.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    Rm = np.stack([x, y, z])
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = Rm, -Rm @ eye
    return w2c


def _scene(seed, n_views=3, W=160, H=120):
    """A wavy surface seen from a few cameras; depth maps with holes, zeros, values beyond depth_trunc, near-border points."""
    rng = np.random.default_rng(seed)
    views = []
    for k in range(n_views):
        eye = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.1)])
        w2c = _look_at(eye, [rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 1.0])
        fx = fy = float(rng.uniform(0.8, 1.2) * W)
        cx, cy = W / 2.0 + rng.uniform(-3, 3), H / 2.0 + rng.uniform(-3, 3)
        u, v = np.meshgrid(np.arange(W), np.arange(H))
        d = (1.0 + 0.1 * np.sin(u / 9.0 + seed) * np.cos(v / 7.0) + 0.02 * rng.standard_normal((H, W))).astype(np.float32)
        # snap some depths so that points land on block borders (L = 16 voxel)
        snap = rng.random((H, W)) < 0.1
        d[snap] = (np.round(d[snap] / 0.16) * 0.16).astype(np.float32)
        d[rng.random((H, W)) < 0.1] = 0.0               # holes
        d[20:30, 40:70] = 0.0                              # a large hole
        d[rng.random((H, W)) < 0.03] = 5.0                # beyond depth_trunc
        col = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        views.append((d, col, fx, fy, cx, cy, w2c.astype(np.float32)))
    return views


VOX, TRUNC, DTRUNC = 0.01, 0.04, 3.0
DOM_MIN, DOM_MAX = (-0.5, -0.45, 0.5), (0.5, 0.45, 1.3)  # small enough that some points fall outside


def _fuse_gpu(views, capacity=4096):
    vol = M.TSDFVolume(VOX, TRUNC, DTRUNC, DOM_MIN, DOM_MAX, device="cuda", capacity=capacity)
    for d, c, fx, fy, cx, cy, w2c in views:
        vol.integrate(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), fx, fy, cx, cy, w2c)
    return vol


def _fuse_ref(views, dom):
    vol = R.Volume(dom, VOX, TRUNC, DTRUNC)
    for d, c, fx, fy, cx, cy, w2c in views:
        vol.integrate(d, c.astype(np.float32), fx, fy, cx, cy, w2c)
    return vol


def _ref_from_gpu(vol):
    coords, tsdf, weight, color = vol.state_arrays()
    r = R.Volume(vol.dom, VOX, TRUNC, DTRUNC)
    r.coords = coords.astype(np.int64)
    r.index[r.linear(r.coords)] = np.arange(len(coords))
    r.tsdf, r.weight, r.color = tsdf, weight, color
    return r


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_integration_matches_restatement(seed):
    views = _scene(seed)
    g = _fuse_gpu(views)
    r = _fuse_ref(views, g.dom)
    coords, tsdf, weight, color = g.state_arrays()
    assert g.n_blocks == r.n > 0
    assert np.array_equal(coords, r.coords), "block coordinates / slot order differ"
    assert g.ignored_points == r.ignored
    assert r.ignored > 0 or seed != 0  # seed 0 has points outside the domain
    assert np.array_equal(weight, r.weight), "weights differ"
    # fp32 with -ffp-contract=off and correctly rounded division / sqrt on both sides: bit-identical, not just close
    assert np.array_equal(tsdf, r.tsdf), f"tsdf differs, max {np.abs(tsdf - r.tsdf).max()}"
    assert np.array_equal(color, r.color), f"colour differs, max {np.abs(color - r.color).max()}"
    # extraction: marching cubes in numpy on the volume read back from the device
    mesh = g.extract_triangle_mesh()
    rv, rc, rt = R.marching_cubes(_ref_from_gpu(g))
    assert len(rt) > 100
    assert np.array_equal(mesh.triangles, rt)
    assert mesh.vertices.shape == rv.shape
    assert np.array_equal(mesh.vertices, rv), f"vertices differ, max {np.abs(mesh.vertices - rv).max()}"
    assert np.array_equal(mesh.vertex_colors, rc), f"vertex colours differ, max {np.abs(mesh.vertex_colors - rc).max()}"
    assert len(np.unique(mesh.triangles)) == len(mesh.vertices), "unreferenced vertices"


def test_determinism_and_pool_growth():
    views = _scene(7, n_views=4)
    a, b = _fuse_gpu(views), _fuse_gpu(views)
    small = _fuse_gpu(views, capacity=2)  # far too small: grown and the step repeated
    assert small.capacity >= small.n_blocks > 2
    sa = a.state_arrays()
    for other in (b, small):
        for x, y in zip(sa, other.state_arrays()):
            assert np.array_equal(x, y)
    ma, mb, ms = a.extract_triangle_mesh(), b.extract_triangle_mesh(), small.extract_triangle_mesh()
    for m in (mb, ms):
        assert np.array_equal(ma.vertices, m.vertices) and np.array_equal(ma.triangles, m.triangles)
        assert np.array_equal(ma.vertex_colors, m.vertex_colors)


def _fibonacci(n):
    k = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * k / n)
    th = np.pi * (1 + 5 ** 0.5) * k
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)


def test_analytic_sphere():
    c, r, dist, W = np.array([0.1, -0.2, 0.3]), 0.5, 2.0, 192
    fx = fy = float(W)
    vol = M.TSDFVolume(VOX, TRUNC, 10.0, c - r - 0.2, c + r + 0.2, device="cuda", capacity=64)
    for dirn in _fibonacci(24):
        eye = c + dist * dirn
        up = (0.0, -1.0, 0.0) if abs(dirn[1]) < 0.9 else (1.0, 0.0, 0.0)
        w2c = _look_at(eye, c, up)
        u, v = np.meshgrid(np.arange(W) + 0.0, np.arange(W) + 0.0)
        ray_c = np.stack([(u - W / 2) / fx, (v - W / 2) / fy, np.ones_like(u)], axis=-1)  # camera space, z = 1
        Rc = w2c[:3, :3]
        o = eye
        dw = ray_c @ Rc  # world directions (unnormalised, z-component in camera space = 1)
        oc = o - c
        a = (dw * dw).sum(-1)
        b = 2 * (dw @ oc)
        cc = oc @ oc - r * r
        disc = b * b - 4 * a * cc
        t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0.0)  # t = camera-space z
        depth = np.where(disc > 0, t, 0.0).astype(np.float32)
        vol.integrate(torch.from_numpy(depth).cuda(), torch.full((W, W, 3), 100, dtype=torch.uint8), fx, fy, W / 2, W / 2,
                      w2c.astype(np.float32))
    mesh = vol.extract_triangle_mesh()
    closed, euler, volume, comps = R.mesh_stats(mesh.vertices, mesh.triangles)
    assert closed and comps == 1 and euler == 2 and volume > 0
    err = np.abs(np.linalg.norm(mesh.vertices.astype(np.float64) - c, axis=1) - r)
    assert err.max() <= VOX


def _truth_and_cams(n_true, n_views, W, H):
    import gs2m_synth as S
    from gs2m_scene import Camera, GaussianParams, inverse_sigmoid
    sc = S.make_surface_scene(n_true, seed=0)
    t = {k: v.cuda() for k, v in sc.items()}
    truth = GaussianParams(t["points"], t["shs"][:, :1].contiguous(), t["shs"][:, 1:].contiguous(), torch.log(t["scales"]),
                           t["rotations"], inverse_sigmoid(t["opacities"]),
                           *(inverse_sigmoid(torch.full((n_true, c), 0.5, device="cuda")) for c in (3, 1, 1)))
    cams = [Camera(c, "cuda") for c in S.orbit_cameras(n_views, W, H, radius=6.0, centre=(0.0, -0.8, 6.0), fx=1.1 * W)]
    return truth, cams


def _surface_distance(p):
    c = np.array([0.0, 0.0, 6.0])
    ds = np.abs(np.linalg.norm(p - c, axis=1) - 1.5)
    rad = np.linalg.norm((p - c)[:, [0, 2]], axis=1)
    dd = np.where(rad <= 3.0, np.abs(p[:, 1] - 1.5), np.hypot(rad - 3.0, p[:, 1] - 1.5))
    return np.minimum(ds, dd)


def test_end_to_end_synthetic_surface(tmp_path):
    truth, cams = _truth_and_cams(40_000, 10, 320, 240)
    voxel = 0.01
    render_dir = tmp_path / "renders"
    depths = M.render_views(truth, cams, str(render_dir))
    vol = M.fuse_depths(depths, cams, render_dir, 12.0, voxel, 4 * voxel)
    post = M.post_process_mesh(vol.extract_triangle_mesh(), 1)
    M.write_mesh(tmp_path / "tsdf_post.ply", post)
    mesh = M.read_mesh(tmp_path / "tsdf_post.ply")
    assert len(mesh.triangles) > 1000
    d = _surface_distance(mesh.vertices.astype(np.float64))
    assert np.percentile(d, 95) <= 2 * voxel, np.percentile(d, [50, 90, 95, 99])
    # coverage of the camera-visible part of the sphere
    c = np.array([0.0, 0.0, 6.0])
    s = c + 1.5 * _fibonacci(4000)
    n = (s - c) / 1.5
    eyes = np.stack([cam.camera_center.cpu().numpy() for cam in cams])
    facing = ((eyes[None] - s[:, None]) * n[:, None]).sum(-1) / np.linalg.norm(eyes[None] - s[:, None], axis=-1)
    vis = (facing.max(1) > 0.3) & (s[:, 1] < 1.2)
    from scipy.spatial import cKDTree
    near, _ = cKDTree(mesh.vertices.astype(np.float64)).query(s[vis])
    assert vis.sum() > 500
    assert (near <= 2 * voxel).mean() >= 0.9, (near <= 2 * voxel).mean()
    # with `bounds` (the sphere's box; the disc is cut away): depth outside is dropped, nothing inside is ignored
    box = np.array([[-1.6, 1.6], [-1.6, 1.4], [4.4, 7.6]])
    vb = M.fuse_depths(depths, cams, render_dir, 12.0, voxel, 4 * voxel, bounds=box)
    assert vb.ignored_points == 0
    mb = vb.extract_triangle_mesh()
    assert len(mb.triangles) > 1000
    slack = 4 * voxel + voxel
    assert np.all(mb.vertices >= box[:, 0] - slack) and np.all(mb.vertices <= box[:, 1] + slack)


def test_cli_writes_the_three_files(tmp_path):
    import json
    import gs2m_train as T
    from gs2m_model import GaussianModel
    scene = T.synthetic_scene(8000, 4, 96, 64, seed=1)
    T.export_colmap_dataset(str(tmp_path / "scene"), scene)
    truth, _ = _truth_and_cams(8000, 1, 96, 64)
    model = GaussianModel(3)
    model.parameterize((truth._xyz, truth._features_dc, truth._features_rest, truth._scaling, truth._rotation, truth._opacity,
                        truth._albedo, truth._roughness, truth._metallic))
    model.active_sh_degree = 3
    model.save_ply(str(tmp_path / "model.ply"))
    out = tmp_path / "out"
    M.main(["--ply", str(tmp_path / "model.ply"), "-s", str(tmp_path / "scene"), "-o", str(out), "--voxel_size", "0.02"])
    cfg = json.load(open(out / "config.json"))
    assert cfg["voxel_size"] == 0.02 and cfg["sdf_trunc"] == 0.08 and cfg["max_depth"] > 0
    raw, post = M.read_mesh(out / "tsdf_mesh.ply"), M.read_mesh(out / "tsdf_post.ply")
    assert len(raw.triangles) > 0 and 0 < len(post.triangles) <= len(raw.triangles)
