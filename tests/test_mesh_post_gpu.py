"""Mesh post-processing on the GPU (csrc/mesh_post.hip through gs2m_mesh.cluster_connected_triangles_gpu and
post_process_mesh_gpu) against the host functions gs2m_mesh.cluster_connected_triangles and post_process_mesh, which are
the oracle: the labels after renumbering the host's by first occurrence, the sizes, and the three arrays of the
post-processed mesh, element for element."""
import filecmp
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gs2m_mesh as M  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- inputs ----------------------------------------------------------------------------------------------------------

def _strip_tris(k, vid0=0):
    """The first k triangles of a connected strip, over the vertex ids vid0 .. vid0 + _strip_verts(k) - 1 (an odd k leaves
    the strip's last vertex unreferenced)."""
    t = []
    for i in range((k + 1) // 2):
        a, b, c, d = 2 * i, 2 * i + 1, 2 * i + 2, 2 * i + 3
        t += [[a, c, b], [b, c, d]]
    return np.asarray(t[:k], np.int64).reshape(-1, 3) + vid0


def _strip_verts(k):
    return 2 * ((k + 1) // 2 + 1) if k else 0


def _mesh(triangles, n_vertices, seed=0):
    """The triangles over n_vertices vertices with seeded positions and colours (every row different: a vertex or a colour
    that lands in the wrong place shows)."""
    rng = np.random.default_rng(1000 + seed)
    return M.TriangleMesh(rng.normal(size=(n_vertices, 3)).astype(np.float32), np.asarray(triangles, np.int32).reshape(-1, 3),
                          rng.random(size=(n_vertices, 3)).astype(np.float32))


def _strips(sizes, seed=None):
    """Disjoint strips of the given triangle counts, one after the other; `seed`: the triangle rows shuffled."""
    tris, v0 = [], 0
    for k in sizes:
        tris.append(_strip_tris(k, v0))
        v0 += _strip_verts(k)
    t = np.concatenate(tris) if tris else np.zeros((0, 3), np.int64)
    if seed is not None:
        t = t[np.random.default_rng(seed).permutation(len(t))]
    return _mesh(t, v0, seed or 0)


# ---- the comparison --------------------------------------------------------------------------------------------------

def _first_occurrence(labels):
    """Labels renumbered by first occurrence, i.e. by increasing smallest triangle index: the contract's numbering."""
    labels = np.asarray(labels)
    if len(labels) == 0:
        return labels.astype(np.int64)
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[inv.reshape(-1)]


def _host_clusters(mesh):
    want = _first_occurrence(M.cluster_connected_triangles(mesh)[0])
    return want, np.bincount(want) if len(want) else np.zeros(0, np.int64)


def _same_mesh(got, want):
    for name in ("vertices", "triangles", "vertex_colors"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape, f"{name}: {a.dtype} {a.shape} against {b.dtype} {b.shape}"
        assert np.array_equal(a, b), f"{name} differs in {int((a != b).sum())} places"


def _check(mesh, keeps=(1,), host=None):
    """Device clusters and post-processing of `mesh` against the host functions.  -> (labels, sizes) as numpy."""
    want, sizes = host if host is not None else _host_clusters(mesh)
    lab, size = M.cluster_connected_triangles_gpu(mesh)
    assert lab.dtype == torch.int32 and size.dtype == torch.int32 and lab.is_cuda and size.is_cuda
    lab, size = lab.cpu().numpy(), size.cpu().numpy()
    assert lab.shape == want.shape and np.array_equal(lab, want), f"labels differ in {int((lab != want).sum())} places"
    assert np.array_equal(size, sizes), (size[:10], sizes[:10])
    for k in keeps:
        post = M.post_process_mesh_gpu(mesh, k)
        assert isinstance(post, M.TriangleMesh)
        _same_mesh(post, M.post_process_mesh(mesh, k))
    return lab, size


def _bow_tie():
    """Two triangles sharing only vertex 0, then an edge with equal, then with opposite winding.  -> cluster counts."""
    out = []
    for t in ([[0, 1, 2], [0, 3, 4]], [[0, 1, 2], [0, 1, 3]], [[0, 1, 2], [1, 0, 3]]):
        _, size = _check(_mesh(t, 5))
        out.append(len(size))
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------

def test_bow_tie_and_shared_edge():
    assert _bow_tie() == [2, 1, 1]


@pytest.mark.parametrize("n", [3, 5, 60])
def test_non_manifold_edge(n):
    """n triangles on the edge (0, 1), alternating winding: one cluster (60: large enough to be kept)."""
    t = [[0, 1, 2 + i] if i % 2 == 0 else [1, 0, 2 + i] for i in range(n)]
    _, size = _check(_mesh(t, n + 2), keeps=(1, 2))
    assert size.tolist() == [n]


def test_duplicated_triangle():
    lab, size = _check(_mesh([[0, 1, 2], [0, 1, 2], [3, 4, 5]], 6))
    assert lab.tolist() == [0, 0, 1] and size.tolist() == [2, 1]
    t = np.concatenate([_strip_tris(60), _strip_tris(60)[10:20]])  # ten rows of a kept strip twice
    _, size = _check(_mesh(t, _strip_verts(60)), keeps=(1,))
    assert size.tolist() == [70]


def test_degenerates_and_unreferenced_vertices():
    # the host test's case: vertex 0 unreferenced, a degenerate (a, a, b) on an edge of the strip
    t = np.concatenate([_strip_tris(60, 1), [[1, 1, 2]]])
    m = _mesh(t, 1 + _strip_verts(60))
    _, size = _check(m)
    assert size.tolist() == [61]
    p = M.post_process_mesh_gpu(m, 1)
    assert len(p.vertices) == 62 and np.array_equal(p.vertices, m.vertices[1:]) and np.array_equal(p.triangles, t[:60] - 1)
    # vertex X is referenced only by the degenerate (1, 1, X), which hangs on the strip through the pair (1, 1) of
    # (1, 1, 2): X survives (unreferenced vertices go first), the triangle does not
    X = 1 + _strip_verts(60)
    t = np.concatenate([_strip_tris(60, 1), [[1, 1, 2], [1, 1, X]]])
    m = _mesh(t, X + 2)  # and an unreferenced vertex behind X
    _, size = _check(m)
    assert size.tolist() == [62]
    p = M.post_process_mesh_gpu(m, 1)
    assert len(p.vertices) == 63 and np.array_equal(p.vertices[-1], m.vertices[X]) and len(p.triangles) == 60
    assert np.array_equal(p.vertex_colors[-1], m.vertex_colors[X])


def test_long_chain_in_random_order():
    """A strip of 20,000 triangles, rows shuffled (vertex ids kept): one cluster, whatever the order of the unions."""
    base = _strip_tris(20_000)
    parts = []
    for seed in (11, 12):
        perm = np.random.default_rng(seed).permutation(len(base))
        lab, size = _check(_mesh(base[perm], _strip_verts(20_000)))
        assert size.tolist() == [20_000]
        orig = np.empty_like(lab)
        orig[perm] = lab  # the label of every triangle of the unshuffled strip
        parts.append(_first_occurrence(orig))
    assert np.array_equal(parts[0], parts[1])


@functools.lru_cache(maxsize=None)
def _threshold_mesh():
    rng = np.random.default_rng(5)
    sizes = rng.choice([2, 48, 49, 50, 51], size=299).tolist()
    sizes.insert(137, 200)  # one cluster of 200: the largest, alone
    m = _strips(sizes, seed=6)
    return m, sizes, _host_clusters(m)


@pytest.mark.parametrize("keep", [1, 2, 7])
def test_threshold_and_ties(keep):
    """300 disjoint strips in interleaved triangle order.  keep = 1: the cluster of 200 alone; 2 and 7: the bound is 51, a
    tie of many clusters, all kept."""
    m, sizes, host = _threshold_mesh()
    assert sizes.count(51) >= 7
    lab, size = _check(m, keeps=(keep,), host=host)
    assert sorted(size.tolist()) == sorted(sizes)
    post = M.post_process_mesh_gpu(m, keep)
    assert len(post.triangles) == (200 if keep == 1 else 200 + 51 * sizes.count(51))


@pytest.mark.parametrize("keep", [1, 2, 7])
def test_keep_beyond_the_cluster_count(keep):
    """Five clusters: 7 exceeds C and keeps every cluster of at least 50."""
    sizes = [2, 48, 50, 51, 200]
    m = _strips(sizes, seed=3)
    _check(m, keeps=(keep,))
    assert len(M.post_process_mesh_gpu(m, keep).triangles) == {1: 200, 2: 251, 7: 301}[keep]


def test_all_clusters_below_the_floor_and_empty_input():
    for m in (_strips([2, 48, 49, 30], seed=4), M.TriangleMesh(), _mesh(np.zeros((0, 3), np.int32), 7)):
        _check(m, keeps=(1, 3))
        p = M.post_process_mesh_gpu(m, 1)
        assert p.vertices.shape == (0, 3) and p.triangles.shape == (0, 3) and p.vertex_colors.shape == (0, 3)
        assert p.vertices.dtype == np.float32 and p.triangles.dtype == np.int32 and p.vertex_colors.dtype == np.float32
        d = M.post_process_mesh_gpu(M.DeviceMesh.from_mesh(m, "cuda"), 1)
        assert isinstance(d, M.DeviceMesh) and d.device.type == "cuda"
        assert tuple(d.vertices.shape) == (0, 3) and tuple(d.triangles.shape) == (0, 3) and d.triangles.dtype == torch.int32
    lab, size = M.cluster_connected_triangles_gpu(M.TriangleMesh())
    assert lab.shape == (0,) and size.shape == (0,) and lab.dtype == torch.int32


@functools.lru_cache(maxsize=None)
def _wide_mesh():
    """A 300 x 300 height-field grid (90,000 vertices: ids beyond 2^16) with three rows of quads removed -- four components
    of 40, 79, 129 and 48 rows --, 40 small floaters, the vertex ids permuted.  -> (mesh, host clusters)."""
    n = 300
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")  # quad (i, j): rows i, i + 1
    rows = ~np.isin(i, (40, 120, 250))
    a = (i * n + j)[rows]
    quads = np.stack([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)], 1).reshape(-1, 3)
    rng = np.random.default_rng(21)
    tris, v0 = [quads], n * n
    for k in rng.integers(1, 70, size=40).tolist():
        tris.append(_strip_tris(k, v0))
        v0 += _strip_verts(k)
    t = np.concatenate(tris)
    perm = rng.permutation(v0)  # old id -> new id
    m = _mesh(perm[t], v0, seed=21)
    return m, _host_clusters(m)


@pytest.mark.parametrize("keep", [1, 3])
def test_wide_ids(keep):
    m, host = _wide_mesh()
    assert len(m.vertices) > 90_000 and len(m.triangles) > 170_000
    lab, size = _check(m, keeps=(keep,), host=host)
    assert len(size) == 44 and sorted(size.tolist())[-4:] == [2 * 299 * r for r in (40, 48, 79, 129)]


@pytest.mark.parametrize("F", [0, 1, 255, 256, 257, 1023, 1025])
def test_sizes_around_the_block_edges(F):
    """F triangles of one strip and a floater of 60 far behind it in the arrays."""
    t = np.concatenate([_strip_tris(F), _strip_tris(60, _strip_verts(F) + 3)])
    lab, size = _check(_mesh(t, _strip_verts(F) + 3 + _strip_verts(60), seed=F), keeps=(1, 2))
    assert size.tolist() == ([F, 60] if F else [60])


def test_guard_refuses_ids_out_of_range():
    """The error path, not a fault: no kernel indexes with an id it has not tested; the context is sound afterwards."""
    V = _strip_verts(300)
    for bad in (V, -1):
        t = _strip_tris(300).copy()
        t[123, 1] = bad
        m = _mesh(t, V)
        with pytest.raises(RuntimeError, match="gs2m_mesh_cluster_triangles failed: invalid argument"):
            M.cluster_connected_triangles_gpu(m)
        with pytest.raises(RuntimeError, match="invalid argument"):
            M.post_process_mesh_gpu(m, 1)
        # the compaction's own guard, behind a clustering that did not see the id
        d = M.DeviceMesh.from_mesh(m, "cuda")
        out = [torch.empty_like(d.vertices), torch.empty_like(d.vertex_colors), torch.empty_like(d.triangles)]
        ws = M.workspace_for("gs2m_mesh_post_workspace_bytes", d.device, V, len(t), only=1)
        tot = (M.C.c_longlong * 2)()
        for keep in (torch.ones(len(t), dtype=torch.uint8, device="cuda"), torch.zeros(len(t), dtype=torch.uint8, device="cuda")):
            with pytest.raises(RuntimeError, match="gs2m_mesh_compact failed: invalid argument"):
                M.N.launch("gs2m_mesh_compact", d.device, V, len(t), d.vertices.data_ptr(), d.vertex_colors.data_ptr(), d.triangles.data_ptr(),
                           keep.data_ptr(), ws.data_ptr(), *[o.data_ptr() for o in out], tot)
    torch.cuda.synchronize()
    assert _bow_tie() == [2, 1, 1]


def test_determinism():
    m, _ = _wide_mesh()
    d = M.DeviceMesh.from_mesh(m, "cuda")
    runs = []
    for _ in range(2):
        lab, size = M.cluster_connected_triangles_gpu(d)
        p = M.post_process_mesh_gpu(d, 3)
        runs.append((lab, size, p.vertices, p.triangles, p.vertex_colors))
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and torch.equal(a, b)


# ---- end to end ------------------------------------------------------------------------------------------------------

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


def test_end_to_end_device_mesh(tmp_path):
    truth, cams = _truth_and_cams(40_000, 10, 320, 240)
    voxel = 0.01
    render_dir = tmp_path / "renders"
    depths = M.render_views(truth, cams, str(render_dir))
    vol = M.fuse_depths(depths, cams, render_dir, 12.0, voxel, 4 * voxel)
    host = vol.extract_triangle_mesh()
    dev = vol.extract_triangle_mesh(to_host=False)
    assert isinstance(host, M.TriangleMesh) and isinstance(dev, M.DeviceMesh) and dev.device.type == "cuda"
    assert len(host.triangles) > 1000
    _same_mesh(dev.cpu(), host)
    post = M.post_process_mesh_gpu(dev, 1)
    assert isinstance(post, M.DeviceMesh) and post.device == dev.device
    want = M.post_process_mesh(host, 1)
    assert 1000 < len(want.triangles) <= len(host.triangles)
    _same_mesh(post.cpu(), want)
    M.write_mesh(tmp_path / "a.ply", post)
    M.write_mesh(tmp_path / "b.ply", want)
    assert filecmp.cmp(tmp_path / "a.ply", tmp_path / "b.ply", shallow=False)
    # the whole path, both ways round: the same two files, and host meshes back
    outs = {}
    for name, host_post in (("device", False), ("host", True)):
        raw, pp = M.extract_mesh(truth, cams, 6.0, str(tmp_path / name), max_depth=12.0, voxel_size=voxel, host_post=host_post)
        assert isinstance(raw, M.TriangleMesh) and isinstance(pp, M.TriangleMesh)
        outs[name] = (raw, pp)
    for f in ("tsdf_mesh.ply", "tsdf_post.ply"):
        assert filecmp.cmp(tmp_path / "device" / f, tmp_path / "host" / f, shallow=False), f
    _same_mesh(outs["device"][0], outs["host"][0])
    _same_mesh(outs["device"][1], outs["host"][1])
    _same_mesh(outs["host"][1], want)
