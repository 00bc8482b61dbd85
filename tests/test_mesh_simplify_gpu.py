"""Mesh simplification on the GPU (csrc/mesh_simplify.hip) against the fp64 restatement (tests/mesh_simplify_ref.py):
vertex_map, triangles and totals exactly, positions and attributes within R.ULP_BOUND fp32 ulps -- the bound measured on the
CPU between the restatement's two placements (tests/test_mesh_simplify.py), never from the kernels' output."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import gs2m_mesh as M
import gs2m_native as N
import mesh_simplify_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _run(v, t, cell, attributes=None, weights=None, fill=None):
    """gs2m_simplify through the raw ABI on a workspace of the caller's (filled with the byte `fill` first), and
    gs2m_simplify_count beside it: the two must agree.  -> dict of host arrays."""
    v = torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32)).reshape(-1, 3).to(DEV)
    t = torch.as_tensor(np.ascontiguousarray(t, dtype=np.int32)).reshape(-1, 3).to(DEV)
    V, F = len(v), len(t)
    a = None if attributes is None else torch.as_tensor(np.ascontiguousarray(attributes, dtype=np.float32)).reshape(V, -1).to(DEV)
    w = None if weights is None else torch.as_tensor(np.ascontiguousarray(weights, dtype=np.float32)).to(DEV)
    nch = 0 if a is None else a.shape[1]
    b = C.c_longlong()
    N.check(N.lib().gs2m_simplify_workspace_bytes(V, F, nch, C.byref(b)), "gs2m_simplify_workspace_bytes")
    ws = torch.empty(b.value, dtype=torch.uint8, device=DEV)
    if fill is not None:
        ws.fill_(fill)
    ov, ot = torch.full((V, 3), -7.0, device=DEV), torch.full((F, 3), -7, dtype=torch.int32, device=DEV)
    oa, ow = torch.full((V, max(nch, 1)), -7.0, device=DEV), torch.full((V,), -7.0, device=DEV)
    vm = torch.full((V,), -7, dtype=torch.int32, device=DEV)
    tot, cnt = (C.c_longlong * 2)(), (C.c_longlong * 2)()
    N.launch("gs2m_simplify", DEV, V, F, N.ptr(v), N.ptr(t), nch, N.ptr(a), N.ptr(w), float(cell), N.ptr(ws), N.ptr(ov), N.ptr(oa), N.ptr(ow),
             N.ptr(ot), N.ptr(vm), tot)
    N.launch("gs2m_simplify_count", DEV, V, F, N.ptr(v), N.ptr(t), float(cell), N.ptr(ws), cnt)
    assert list(cnt) == list(tot)
    nv, nt = int(tot[0]), int(tot[1])
    return dict(vertices=ov[:nv].cpu().numpy(), triangles=ot[:nt].cpu().numpy(), attributes=oa[:nv, :nch].cpu().numpy(),
                weight=ow[:nv].cpu().numpy(), vertex_map=vm.cpu().numpy(), totals=(nv, nt),
                rest=(ov[nv:].cpu().numpy(), ot[nt:].cpu().numpy()))


def _against(got, ref, attributes=True):
    assert got["totals"] == ref["totals"]
    assert np.array_equal(got["vertex_map"], ref["vertex_map"])
    assert np.array_equal(got["triangles"], ref["triangles"])
    u = R.vertex_ulps(got["vertices"], ref["vertices"])
    print(f"positions: {u.max() if u.size else 0.0} ulps (bound {R.ULP_BOUND})")
    assert u.size == 0 or u.max() <= R.ULP_BOUND
    assert (got["rest"][0] == -7.0).all() and (got["rest"][1] == -7).all()  # nothing beyond the rows the totals name
    if attributes and ref["attributes"] is not None:
        ua = R.ulp_diff(got["attributes"], ref["attributes"])
        print(f"attributes: {ua.max() if ua.size else 0.0} ulps")
        assert ua.size == 0 or ua.max() <= R.ULP_BOUND
        assert np.array_equal(got["weight"], ref["weight"])


# ---- the smallest shapes ----

def test_empty_inputs():
    v = np.array([[0.1, 0.2, 0.3], [1.1, 0.2, 0.3], [0.1, 1.2, 0.3]], np.float32)
    for vv, tt in ((v, np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))):
        out, info = M.simplify_mesh_gpu(M.DeviceMesh(torch.from_numpy(vv).to(DEV), torch.from_numpy(tt).to(DEV)), cell=0.5, extras=True)
        assert len(out.vertices) == 0 and len(out.triangles) == 0 and (info["vertex_map"] == -1).all() and len(info["vertex_map"]) == len(vv)
        assert M.simplify_count_gpu(torch.from_numpy(vv).to(DEV), torch.from_numpy(tt).to(DEV), 0.5) == (0, 0)


def test_one_triangle_in_three_cells_comes_back_unchanged():
    v = np.array([[0.5, 0.25, 0.75], [1.5, 0.5, 0.5], [2.25, 1.5, 0.625]], np.float32)
    t = np.array([[0, 1, 2]], np.int32)
    got = _run(v, t, 1.0)
    assert np.array_equal(got["vertices"], v) and np.array_equal(got["triangles"], t) and got["vertex_map"].tolist() == [0, 1, 2]
    _against(got, R.simplify_ref(v, t, 1.0))


def test_one_triangle_inside_one_cell_gives_an_empty_mesh():
    v = np.array([[0.5, 0.25, 0.75], [0.6, 0.5, 0.5], [0.25, 0.5, 0.625]], np.float32)
    got = _run(v, np.array([[0, 1, 2]], np.int32), 1.0)
    assert got["totals"] == (0, 0) and got["vertex_map"].tolist() == [-1, -1, -1]


def test_same_cell_triple_keeps_the_lower_index_with_its_corner_order():
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 1.5, 0.5], [0.6, 0.6, 0.5], [1.4, 0.4, 0.5], [2.6, 1.4, 0.5]], np.float32)
    t = np.array([[3, 5, 4], [0, 1, 2], [0, 3, 1]], np.int32)  # opposite orientations; the third lies in two cells only
    got = _run(v, t, 1.0)
    assert got["triangles"].tolist() == [[0, 2, 1]] and got["vertex_map"].tolist() == [0, 1, 2, 0, 1, 2]
    _against(got, R.simplify_ref(v, t, 1.0))


def test_vertices_on_lattice_planes_and_just_below_zero():
    cell = 0.25  # a power of two: k * cell is exact
    tiny = -1e-30
    v = np.array([[0.0, 0.0, 0.0], [3 * cell, 0.0, 0.0], [0.0, 2 * cell, 0.0],         # on planes: they belong to the upper cell
                  [tiny, tiny, tiny], [-cell, 5 * cell, 0.1], [-2 * cell, tiny, -cell],  # floor, not truncation
                  [np.nextafter(np.float32(0.75), np.float32(0)), 0.0, 0.0]], np.float32)
    t = np.array([[0, 1, 2], [3, 4, 5], [3, 6, 2], [0, 6, 1]], np.int32)
    ref = R.simplify_ref(v, t, cell)
    vcell, cidx = R.cells_of(v, cell)
    assert cidx[vcell[3]].tolist() == [-1, -1, -1] and cidx[vcell[1]].tolist() == [3, 0, 0] and cidx[vcell[6]].tolist() == [2, 0, 0]
    got = _run(v, t, cell)
    assert got["totals"] == ref["totals"] == (7, 4)
    assert np.array_equal(got["vertex_map"], ref["vertex_map"]) and np.array_equal(got["triangles"], ref["triangles"])
    # a vertex on a lattice plane sits exactly on the acceptance bound |x_k| = cell / 2: accepted or not, a cell of one vertex
    # is placed at that vertex, so the positions are held to the input here and not to the restatement's decision
    assert np.abs(got["vertices"][got["vertex_map"]].astype(np.float64) - v).max() <= 1e-7


def _long_segment_scene():
    """1600 coplanar vertices inside ONE cell (a segment longer than a workgroup, 3042 triangles of it) and a fan of three
    triangles that tie that cell to three others, so that it survives."""
    v, t = R.plane_grid(40, origin=(0.131, 0.147, 0.402))
    far = np.array([[1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [1.5, 1.5, 0.5]], np.float32)
    n = len(v)
    fan = np.array([[0, n, n + 2], [39, n + 2, n + 1], [n, n + 1, n + 2]], np.int32)
    return np.concatenate([v, far]), np.concatenate([t, fan])


def test_a_segment_longer_than_a_workgroup():
    v, t = _long_segment_scene()
    ref = R.simplify_ref(v, t, 1.0)
    assert ref["totals"] == (4, 3) and np.bincount(R.cells_of(v, 1.0)[0]).max() == 1600
    a, w = R.scene_attributes(len(v))
    _against(_run(v, t, 1.0, a, w), R.simplify_ref(v, t, 1.0, a, w))


def test_a_permuted_vertex_order_gives_the_same_mesh():
    v, t, cell = R.gpu_scenes()["box8"]
    perm = np.random.default_rng(5).permutation(len(v))  # new index k holds old vertex perm[k]
    inv = np.argsort(perm)
    a, b = _run(v, t, cell), _run(v[perm], inv[t].astype(np.int32), cell)
    assert a["totals"] == b["totals"] and np.array_equal(a["triangles"], b["triangles"])
    assert np.array_equal(a["vertex_map"], b["vertex_map"][inv])
    assert R.vertex_ulps(a["vertices"], b["vertices"]).max() <= R.ULP_BOUND  # the order of the sums changed, nothing else


def test_far_away_geometry_moves_no_cell():
    """The keys no longer fit 32 bits (14 + 14 + 14): the second sort runs."""
    v, t, cell = R.gpu_scenes()["box8"]
    far = np.array([[5000.0, 4000.0, 3000.0], [5001.0, 4000.0, 3000.0], [5000.0, 4001.0, 3001.0]], np.float32)
    v2 = np.concatenate([v, far])
    t2 = np.concatenate([t, np.array([[len(v), len(v) + 1, len(v) + 2]], np.int32)])
    a, b = _run(v, t, cell), _run(v2, t2, cell)
    n = a["totals"][0]
    assert b["totals"] == (n + 3, a["totals"][1] + 1)
    assert np.array_equal(b["vertices"][:n], a["vertices"]) and np.array_equal(b["triangles"][:-1], a["triangles"])
    _against(b, R.simplify_ref(v2, t2, cell))


# ---- the scenes ----

@pytest.mark.parametrize("name", sorted(R.gpu_scenes()))
def test_scene_against_the_restatement(name):
    v, t, cell = R.gpu_scenes()[name]
    a, w = R.scene_attributes(len(v))
    _against(_run(v, t, cell, a, w), R.gpu_scene_ref(name))


def test_attributes_and_weights():
    v, t, cell = R.gpu_scenes()["box8"]
    a, w = R.scene_attributes(len(v))
    ref = R.gpu_scene_ref("box8")
    got = _run(v, t, cell, a, w)
    zero = ref["weight"] == 0
    assert zero.any() and np.array_equal(got["weight"] == 0, zero)  # cells whose vertices all weigh 0: the plain mean
    vcell = ref["vertex_map"]
    c = int(np.nonzero(zero)[0][0])
    plain = a[vcell == c].astype(np.float64).mean(axis=0)
    assert np.abs(got["attributes"][c] - plain).max() <= 1e-6
    ones, null = _run(v, t, cell, a, np.ones(len(v), np.float32)), _run(v, t, cell, a, None)
    for k in ("vertices", "triangles", "attributes", "weight", "vertex_map"):
        assert np.array_equal(ones[k], null[k])
    assert np.array_equal(null["weight"], np.bincount(vcell[vcell >= 0]).astype(np.float32))


def test_two_runs_and_a_dirty_workspace_are_bitwise_identical():
    v, t, cell = R.gpu_scenes()["box24_a"]
    a, w = R.scene_attributes(len(v))
    first, again, dirty = _run(v, t, cell, a, w, fill=0), _run(v, t, cell, a, w, fill=0), _run(v, t, cell, a, w, fill=0xFF)
    for k in ("vertices", "triangles", "attributes", "weight", "vertex_map"):
        assert np.array_equal(first[k], again[k]) and np.array_equal(first[k], dirty[k])
    lv, lt = _long_segment_scene()
    la, lw = R.scene_attributes(len(lv))
    one, two = _run(lv, lt, 1.0, la, lw, fill=0), _run(lv, lt, 1.0, la, lw, fill=0xFF)
    for k in ("vertices", "triangles", "attributes", "weight", "vertex_map"):
        assert np.array_equal(one[k], two[k])


# ---- error codes ----

def _rc(v, t, cell):
    """-> (return code of gs2m_simplify, of gs2m_simplify_count, outputs untouched)."""
    v, t = torch.from_numpy(np.asarray(v, np.float32)).to(DEV), torch.from_numpy(np.asarray(t, np.int32)).to(DEV)
    V, F = len(v), len(t)
    b = C.c_longlong()
    N.check(N.lib().gs2m_simplify_workspace_bytes(V, F, 0, C.byref(b)), "gs2m_simplify_workspace_bytes")
    ws = torch.empty(b.value, dtype=torch.uint8, device=DEV)
    ov, ot = torch.full((V, 3), -7.0, device=DEV), torch.full((F, 3), -7, dtype=torch.int32, device=DEV)
    ow, vm = torch.full((V,), -7.0, device=DEV), torch.full((V,), -7, dtype=torch.int32, device=DEV)
    tot = (C.c_longlong * 2)()
    s = N.stream_ptr(DEV)
    rc = N.lib().gs2m_simplify(V, F, N.ptr(v), N.ptr(t), 0, None, None, float(cell), N.ptr(ws), N.ptr(ov), None, N.ptr(ow), N.ptr(ot), N.ptr(vm), tot, s)
    rc2 = N.lib().gs2m_simplify_count(V, F, N.ptr(v), N.ptr(t), float(cell), N.ptr(ws), tot, s)
    torch.cuda.synchronize()
    clean = bool((ov == -7).all() and (ot == -7).all() and (ow == -7).all() and (vm == -7).all())
    return rc, rc2, clean


def test_error_codes_leave_the_outputs_untouched():
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 1.5, 0.5]], np.float32)
    ok = np.array([[0, 1, 2]], np.int32)
    assert _rc(v, [[0, 1, 3]], 1.0) == (-1, -1, True)    # an id == V: tested, never used as an index
    assert _rc(v, [[0, -1, 2]], 1.0) == (-1, -1, True)
    bad = v.copy()
    bad[1, 2] = np.nan
    assert _rc(bad, ok, 1.0) == (-1, -1, True)
    bad[1, 2] = np.inf
    assert _rc(bad, ok, 1.0) == (-1, -1, True)
    wide = v.copy()
    wide[2, 0] = 3.0e6                                   # 3e6 cells of edge 1 along x: beyond 2^21
    assert _rc(wide, ok, 1.0) == (-4, -4, True)
    assert _rc(wide, ok, 1.5) == (0, 0, False)           # 2e6 cells: within the limit
    assert _rc(v, ok, 1e-30)[:2] == (-4, -4)             # indices beyond 2^52


# ---- the Python layer ----

def test_target_triangles_on_the_sphere():
    v, t, _ = R.gpu_scenes()["ico6"]
    mesh = M.DeviceMesh(torch.from_numpy(v).to(DEV), torch.from_numpy(t).to(DEV))
    n = 3000
    out, info = M.simplify_mesh_gpu(mesh, target_triangles=n, extras=True)
    assert isinstance(out, M.DeviceMesh) and 0 < len(out.triangles) <= n
    base = M.simplify_base_cell(mesh.vertices, mesh.triangles)
    k = round(M.LADDER * math.log2(info["cell"] / base))
    assert info["cell"] == base * 2.0 ** (k / M.LADDER)
    assert R.count_ref(v, t, info["cell"])[1] == len(out.triangles)
    below = R.count_ref(v, t, base * 2.0 ** ((k - 1) / M.LADDER))[1] if k > 0 else len(t)
    assert below > n
    # a target that is not below the input's count: the mesh as it is
    same = M.simplify_mesh_gpu(mesh, target_triangles=len(t))
    assert torch.equal(same.vertices, mesh.vertices) and torch.equal(same.triangles, mesh.triangles)
    # a host mesh goes and comes back; the colours ride along as channels
    host = M.simplify_mesh_gpu(M.TriangleMesh(v, t, np.abs(v)), cell=info["cell"])
    assert isinstance(host, M.TriangleMesh) and np.array_equal(host.triangles, out.triangles.cpu().numpy())
    assert np.abs(host.vertex_colors - np.abs(host.vertices)).max() < 0.2


def test_material_mesh_end_to_end(tmp_path):
    """Bake a tiny mesh as tests/test_mesh_bake_gpu.py's command-line test does (its modules, its golden model, its scene),
    simplify the material PLY from the command line, reload it and render one PBR view of the result."""
    import gs2m_envmap as E
    import gs2m_mesh_bake as MB
    import gs2m_mesh_simplify as S
    import gs2m_mesh_view as MVW
    import gs2m_train as T
    from gs2m_model import GaussianModel
    W, H = 48, 32
    scene = tmp_path / "scene"
    T.export_colmap_dataset(str(scene), T.synthetic_scene(2000, 3, W, H, seed=1))
    ply = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_small.ply")
    verts, tris = R.icosphere(3)
    verts = (0.8 * verts + np.array([0.0, -0.8, 6.0])).astype(np.float32)  # where the scene's cameras look
    cams, _, _, _, _ = T.load_colmap_dataset(str(scene), resolution=1)
    model = GaussianModel(3)
    model.load_ply(ply)
    values, seen, _ = MB.bake_materials(model, cams, M.TriangleMesh(verts, tris), metallic=True)
    MB.write_material_mesh(tmp_path / "material.ply", verts, tris, values, seen)
    out = tmp_path / "simple.ply"
    r = S.main(["--ply-path", str(tmp_path / "material.ply"), "-o", str(out), "--cell", "0.4"])
    back = MB.read_material_mesh(out)
    assert r["material"] and 0 < r["n_triangles"] == len(back["triangles"]) < len(tris) and len(back["vertices"]) == r["n_vertices"]
    src = MB.read_material_mesh(tmp_path / "material.ply")
    vals = np.concatenate([src["albedo"], src["roughness"][:, None], src["metallic"][:, None]], axis=1)
    ref = R.simplify_ref(src["vertices"], src["triangles"], 0.4, vals, src["seen"].astype(np.float32))
    assert np.array_equal(back["triangles"], ref["triangles"]) and np.array_equal(back["seen"], ref["weight"] > 0)
    assert R.vertex_ulps(back["vertices"], ref["vertices"]).max() <= R.ULP_BOUND
    assert np.abs(back["roughness"] - ref["attributes"][:, 3]).max() <= 1e-6
    light = E.EnvLight((0.2 + torch.rand((6, 64, 64, 3), generator=torch.Generator().manual_seed(2))).cuda())
    hdr = E.save_light_hdr(light, str(tmp_path / "tiny.hdr"), res=(16, 32))
    res = MVW.main(["--ply-path", str(out), "-s", str(scene), "--out-dir", str(tmp_path / "visual"), "--rendering", "--render_view_idx", "0",
                    "--colour", "pbr", "--envmap", hdr, "--env-res", "64"])
    assert len(res["views"]) == 1 and os.path.getsize(res["views"][0]) > 0
    # a plain mesh goes through the same command line
    M.write_mesh(tmp_path / "plain.ply", M.TriangleMesh(verts, tris, np.abs(np.sin(verts))))
    r2 = S.main(["--ply-path", str(tmp_path / "plain.ply"), "-o", str(tmp_path / "plain_simple.ply"), "--triangles", "200"])
    assert not r2["material"] and 0 < len(M.read_mesh(tmp_path / "plain_simple.ply").triangles) <= 200
