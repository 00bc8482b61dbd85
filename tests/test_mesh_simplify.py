"""Mesh simplification without a GPU: the numpy restatement on its own (tests/mesh_simplify_ref.py), the conditions the GPU
comparison rests on (decision margins, the measured tolerance), the C ABI's host-side answers and the command lines."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gs2m_native as N
import mesh_simplify_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"gs2m_simplify_workspace_bytes": 4, "gs2m_simplify_count": 8, "gs2m_simplify": 16, "gs2m_simplify_set_timing": 1,
                "gs2m_simplify_stage_ms": 1}


# ---- the restatement ----

@pytest.mark.parametrize("cell", [0.23, 0.31])
def test_box_vertices_lie_on_the_surface_and_corners_are_kept(cell):
    v, t = R.box_mesh(24)  # coordinates in [-1.013, 0.987] etc.: the lattice is offset against the box
    assert len(v) == 3458
    r = R.simplify_ref(v, t, cell)
    lo, hi = R.box_planes(24)
    p = r["positions64"]
    dist = np.min(np.minimum(np.abs(p - lo), np.abs(p - hi)), axis=1)
    assert dist.max() <= 1e-12
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]).astype(np.float32)
    out = {tuple(q) for q in r["vertices"].tolist()}
    assert all(tuple(c) in out for c in corners.tolist())
    assert r["fallback"].sum() == 0


def test_planar_patch_returns_its_cell_means():
    v, t = R.plane_grid(40)
    r = R.simplify_ref(v, t, 0.1)
    assert r["totals"][0] > 10 and r["fallback"][r["survives"]].sum() == 0
    vcell, cidx = R.cells_of(v, 0.1)
    means = np.stack([v[vcell == c].astype(np.float64).mean(axis=0) for c in range(len(cidx))])[r["survives"]]
    # the cell's quadric has rank 1: the placement is the mean projected onto the plane the mean already lies on (up to the
    # fp32 rounding of the patch's vertices: 6e-8 at these magnitudes)
    assert np.abs(r["positions64"] - means).max() <= 2e-7


@pytest.mark.parametrize("cell", [0.11, 0.2, 0.37])
def test_sphere_cells_are_placed_by_their_rank_one_quadrics(cell):
    v, t = R.icosphere(5)
    r = R.simplify_ref(v, t, cell)
    assert r["fallback"].sum() <= 0.01 * len(r["fallback"])
    assert np.abs(np.linalg.norm(r["positions64"], axis=1) - 1.0).max() < 0.6 * cell  # and they stay near the sphere


def test_fixed_order_sum_is_the_documented_order():
    rng = np.random.default_rng(0)
    for n in (0, 1, 15, 16, 17, 256, 257, 1601):
        e = rng.standard_normal((n, 2))
        got = R.fixed_order_sum(e)
        width = 16 if n <= 256 else 256
        part = [np.zeros(2) for _ in range(width)]
        for k in range(n):
            part[k % width] = part[k % width] + e[k]
        if width == 16:
            o = 8
            while o:
                for l in range(o):
                    part[l] = part[l] + part[l + o]
                o //= 2
            want = part[0]
        else:
            ws = []
            for w in range(4):
                q = part[64 * w:64 * w + 64]
                o = 32
                while o:
                    for l in range(o):
                        q[l] = q[l] + q[l + o]
                    o //= 2
                ws.append(q[0])
            want = (ws[0] + ws[1]) + (ws[2] + ws[3])
        assert np.array_equal(got, want)


def test_triangle_rules():
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 1.5, 0.5], [0.6, 0.6, 0.5], [1.4, 0.4, 0.5], [2.6, 1.4, 0.5]], np.float32)
    t = np.array([[3, 5, 4], [0, 1, 2], [0, 3, 1]], np.int32)  # the first two share a cell triple, the third lies in two cells
    r = R.simplify_ref(v, t, 1.0)
    assert r["triangles"].tolist() == [[0, 2, 1]] and r["vertex_map"].tolist() == [0, 1, 2, 0, 1, 2]
    assert R.count_ref(v, t, 1.0) == (3, 1)
    with pytest.raises(OverflowError):
        R.cells_of(np.array([[0, 0, 0], [3e6, 0, 0]], np.float32), 1.0)


# ---- the conditions of the GPU comparison ----

@pytest.mark.parametrize("name", sorted(R.gpu_scenes()))
def test_no_gpu_scene_has_a_decision_within_the_margin(name):
    r = R.gpu_scene_ref(name)
    assert int((R.decision_distance(r) < R.MARGIN).sum()) == 0
    assert r["totals"][1] > 100


def test_measured_tolerance_between_the_two_placements():
    worst = 0.0
    for name in sorted(R.gpu_scenes()):
        a, j = R.gpu_scene_ref(name, R.place_eigh), R.gpu_scene_ref(name, R.place_jacobi)
        assert np.array_equal(a["triangles"], j["triangles"]) and np.array_equal(a["fallback"], j["fallback"])
        worst = max(worst, float(R.vertex_ulps(a["vertices"], j["vertices"]).max()))
    print(f"eigh against the written-out Jacobi: {worst} fp32 ulps")
    assert worst <= R.ULP_MEASURED
    assert R.ULP_BOUND == max(1.0, 4.0 * R.ULP_MEASURED)


def test_a_scene_has_a_cell_without_weight():
    r = R.gpu_scene_ref("box8")
    assert (r["weight"] == 0).any() and (r["weight"] > 1).any()


# ---- the ABI ----

def test_header_table_and_library_agree():
    src = open(os.path.join(ROOT, "include", "gs2m_simplify.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"int\s+(gs2m_simplify\w*)\s*\(([^)]*)\)", src)}
    assert declared == ENTRY_POINTS
    lib = N.lib()
    for name, arity in ENTRY_POINTS.items():
        assert len(N.SIGNATURES[name][1]) == arity and hasattr(lib, name)
    assert N.SIGNATURES["gs2m_simplify"][1][-1] is N.STREAM and N.SIGNATURES["gs2m_simplify_count"][1][-1] is N.STREAM


def test_workspace_bytes_answers_on_the_host():
    lib, b = N.lib(), C.c_longlong()
    assert lib.gs2m_simplify_workspace_bytes(1000, 2000, 5, C.byref(b)) == 0
    small = b.value
    assert lib.gs2m_simplify_workspace_bytes(2000, 4000, 5, C.byref(b)) == 0 and b.value > small > 158 * 1000
    assert lib.gs2m_simplify_workspace_bytes(0, 0, 0, C.byref(b)) == 0 and b.value > 0
    assert lib.gs2m_simplify_workspace_bytes(-1, 0, 0, C.byref(b)) == -1
    assert lib.gs2m_simplify_workspace_bytes(10, 10, 0, None) == -1
    assert lib.gs2m_simplify_workspace_bytes(1 << 31, 10, 0, C.byref(b)) == -4
    assert lib.gs2m_simplify_workspace_bytes(10, 1 << 30, 0, C.byref(b)) == -4


@pytest.mark.parametrize("cell", [0.0, -1.0, float("nan"), float("inf")])
def test_cell_limits_return_their_code_without_a_device(cell):
    """The 2^21-cells limit depends on the vertices, which live in device memory: it is answered on a device only
    (tests/test_mesh_simplify_gpu.py) and by the restatement (test_triangle_rules)."""
    lib, tot = N.lib(), (C.c_longlong * 2)(7, 7)
    assert lib.gs2m_simplify_count(3, 1, None, None, cell, None, tot, None) == -1
    assert lib.gs2m_simplify(3, 1, None, None, 0, None, None, cell, None, None, None, None, None, None, tot, None) == -1
    assert list(tot) == [7, 7]


def test_empty_inputs_need_no_device():
    lib, tot = N.lib(), (C.c_longlong * 2)(7, 7)
    assert lib.gs2m_simplify(0, 0, None, None, 0, None, None, 0.5, None, None, None, None, None, None, tot, None) == 0 and list(tot) == [0, 0]
    tot = (C.c_longlong * 2)(7, 7)
    assert lib.gs2m_simplify_count(5, 0, None, None, 0.5, None, tot, None) == 0 and list(tot) == [0, 0]


# ---- command lines ----

def test_mesh_command_line_has_the_flags_and_is_unchanged_without_them():
    import gs2m_mesh as M
    base = ["--ply", "m.ply", "-s", "scene", "-o", "out"]
    a, _ = M.parse_args(base)
    assert not any(k.startswith("simplify") for k in vars(a)) and M.simplify_keywords(a) == {}
    a, _ = M.parse_args(base + ["--simplify-cell", "0.02"])
    assert M.simplify_keywords(a) == {"simplify_cell": 0.02}
    a, _ = M.parse_args(base + ["--simplify-triangles", "5000"])
    assert M.simplify_keywords(a) == {"simplify_triangles": 5000}
    with pytest.raises(SystemExit):
        M.parse_args(base + ["--simplify-cell", "0.02", "--simplify-triangles", "5000"])


def test_simplify_command_line_takes_one_of_cell_and_triangles():
    import gs2m_mesh_simplify as S
    for extra in ([], ["--cell", "0.1", "--triangles", "10"]):
        with pytest.raises(SystemExit):
            S.parser().parse_args(["--ply-path", "a.ply", "-o", "b.ply"] + extra)
    assert S.parser().parse_args(["--ply-path", "a.ply", "-o", "b.ply", "--cell", "0.1"]).cell == 0.1
    assert S.parser().parse_args(["--ply-path", "a.ply", "-o", "b.ply", "--triangles", "10"]).triangles == 10


def test_simplify_mesh_gpu_argument_checks_and_no_cpu_path():
    import gs2m_mesh as M
    v, t = R.box_mesh(2)
    mesh = M.TriangleMesh(v, t)
    for kw in ({}, {"cell": 0.1, "target_triangles": 5}, {"cell": -1.0}, {"cell": float("nan")}):
        with pytest.raises(ValueError):
            M.simplify_mesh_gpu(mesh, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.simplify_mesh_gpu(mesh, cell=0.5, device="cpu")


def test_material_ply_round_trips_through_the_host_plumbing(tmp_path):
    import torch
    import gs2m_mesh as M
    import gs2m_mesh_bake as MB
    import gs2m_mesh_simplify as S
    v, t = R.box_mesh(3)
    rng = np.random.default_rng(3)
    values = (np.rint(rng.random((len(v), 5)) * 255) / 255).astype(np.float32)  # albedo bytes survive the file
    seen = rng.random(len(v)) < 0.7
    MB.write_material_mesh(tmp_path / "m.ply", v, t, values, seen)
    M.write_mesh(tmp_path / "p.ply", M.TriangleMesh(v, t, values[:, :3]))
    assert S.is_material_ply(tmp_path / "m.ply") and not S.is_material_ply(tmp_path / "p.ply")
    mesh, vals, w = S.load(tmp_path / "m.ply")
    assert np.array_equal(mesh.vertices, v) and np.array_equal(mesh.triangles, t) and np.array_equal(w, seen.astype(np.float32))
    assert np.array_equal(vals[:, 3:], values[:, 3:]) and np.abs(vals[:, :3] - values[:, :3]).max() < 1e-6
    S.save(tmp_path / "again.ply", mesh, torch.from_numpy(vals), torch.from_numpy(w))  # CPU tensors
    assert (tmp_path / "again.ply").read_bytes() == (tmp_path / "m.ply").read_bytes()
    plain, none, _ = S.load(tmp_path / "p.ply")
    assert none is None
    S.save(tmp_path / "p2.ply", plain)
    assert (tmp_path / "p2.ply").read_bytes() == (tmp_path / "p.ply").read_bytes()
