"""Mesh post-processing on the device, the parts that need no GPU: the C ABI of csrc/mesh_post.hip as the header and the
signature table state it, the DeviceMesh type on CPU tensors, its PLY bytes, and the refusal to compute on the CPU."""
import os
import re

import numpy as np
import pytest
import torch

import gs2m_mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"gs2m_mesh_post_workspace_bytes": 4, "gs2m_mesh_cluster_triangles": 8, "gs2m_mesh_keep_clusters": 6,
                "gs2m_mesh_compact": 12}


def _mesh(seed=0, V=40, F=70):
    rng = np.random.default_rng(seed)
    return M.TriangleMesh(rng.normal(size=(V, 3)).astype(np.float32), rng.integers(0, V, size=(F, 3)).astype(np.int32),
                          rng.random(size=(V, 3)).astype(np.float32))


def test_header_and_signature_table_have_the_entry_points():
    import gs2m_native as N
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gs2m_mesh.h")).read(), flags=re.S)
    for name, n_params in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src)
        assert m, f"{name} is not declared in include/gs2m_mesh.h"
        assert len(m.group(1).split(",")) == n_params
        restype, argtypes = N.SIGNATURES[name]
        assert len(argtypes) == n_params
        assert (argtypes[-1] is N.STREAM) == (name != "gs2m_mesh_post_workspace_bytes")
    text = open(os.path.join(ROOT, "include", "gs2m_mesh.h")).read()
    assert "post-processing" in text and "smallest triangle index" in text  # the contract is stated with them


def test_library_sizes_the_workspaces():
    """No GPU call: the sizes alone.  Either output may be left out; the limits are refused."""
    import ctypes as C
    import gs2m_native as N
    if not os.path.exists(N.LIB_PATH):
        N.build()
    fn = N.lib().gs2m_mesh_post_workspace_bytes
    a, b = C.c_longlong(), C.c_longlong()
    assert fn(17_000_000, 33_000_000, C.byref(a), C.byref(b)) == 0
    assert 104 * 33_000_000 <= a.value <= 112 * 33_000_000, a.value  # the header's bytes per triangle
    assert 9 * 17_000_000 + 8 * 33_000_000 <= b.value <= 9 * 17_000_000 + 8 * 33_000_000 + (1 << 20)
    assert M.post_workspace_bytes(17_000_000, 33_000_000) == (a.value, b.value)
    only = C.c_longlong()
    assert fn(17_000_000, 33_000_000, None, C.byref(only)) == 0 and only.value == b.value
    assert fn(17_000_000, 33_000_000, C.byref(only), None) == 0 and only.value == a.value
    assert fn(0, 0, C.byref(a), C.byref(b)) == 0 and a.value > 0 and b.value > 0
    assert fn(10, 0xFFFFFFF0 // 3 + 1, C.byref(a), C.byref(b)) == -4  # 3 F beyond the sort's u32 slots
    assert fn(-1, 0, C.byref(a), C.byref(b)) == -1 and fn(1, 1, None, None) == -1


def test_device_mesh_round_trips_on_cpu_tensors():
    m = _mesh()
    d = M.DeviceMesh.from_mesh(m, "cpu")
    assert d.device.type == "cpu"
    assert d.vertices.dtype == torch.float32 and d.triangles.dtype == torch.int32 and d.vertex_colors.dtype == torch.float32
    assert tuple(d.vertices.shape) == (40, 3) and tuple(d.triangles.shape) == (70, 3) and tuple(d.vertex_colors.shape) == (40, 3)
    back = d.cpu()
    assert isinstance(back, M.TriangleMesh)
    for name in ("vertices", "triangles", "vertex_colors"):
        a, b = getattr(m, name), getattr(back, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    e = M.DeviceMesh.from_mesh(M.TriangleMesh(), "cpu").cpu()
    assert e.vertices.shape == (0, 3) and e.triangles.shape == (0, 3) and e.vertex_colors.shape == (0, 3)
    assert e.vertices.dtype == np.float32 and e.triangles.dtype == np.int32
    with pytest.raises(ValueError):
        M.DeviceMesh(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(5, 3))


def test_write_mesh_of_a_device_mesh_gives_the_same_bytes(tmp_path):
    m = _mesh(1)
    M.write_mesh(tmp_path / "host.ply", m)
    M.write_mesh(tmp_path / "device.ply", M.DeviceMesh.from_mesh(m, "cpu"))
    assert open(tmp_path / "host.ply", "rb").read() == open(tmp_path / "device.ply", "rb").read()
    M.write_mesh(tmp_path / "e_host.ply", M.TriangleMesh())
    M.write_mesh(tmp_path / "e_device.ply", M.DeviceMesh.from_mesh(M.TriangleMesh(), "cpu"))
    assert open(tmp_path / "e_host.ply", "rb").read() == open(tmp_path / "e_device.ply", "rb").read()


def test_device_post_processing_fails_loudly_without_a_device():
    m = _mesh(2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.post_process_mesh_gpu(m, 1, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.post_process_mesh_gpu(M.DeviceMesh.from_mesh(m, "cpu"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.cluster_connected_triangles_gpu(m, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.cluster_connected_triangles_gpu(torch.from_numpy(m.triangles), 40)
    if not torch.cuda.is_available():  # a HIP device asked for where there is none: torch's error, nothing computed
        with pytest.raises((RuntimeError, AssertionError)):
            M.post_process_mesh_gpu(m, 1)


def test_command_line_has_the_host_switch():
    a, _ = M.parse_args(["--ply", "p.ply", "-s", "scene", "-o", "out"])
    assert a.host_post is False
    a, _ = M.parse_args(["--ply", "p.ply", "-s", "scene", "-o", "out", "--host-post"])
    assert a.host_post is True
