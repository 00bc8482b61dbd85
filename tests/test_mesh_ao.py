"""The ray-casting contract without a GPU (include/gs2m_meshao.h): the numpy restatement of tests/mesh_ao_ref.py against
hand-worked cases, the host-side direction table, mix32 and the frame, the balance of the ray families the GPU tests rely on,
and the two file formats that gain an occlusion slot."""
import math

import numpy as np
import pytest

import mesh_ao_ref as A

TRI = (np.array([0.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
DOWN = np.array([0.0, 0.0, -1.0])


def _hit(o, d, tri=TRI, tmin=0.0, tmax=np.inf):
    return bool(A.triangle_hits(np.asarray(o, np.float64), np.asarray(d, np.float64), *tri, tmin, tmax))


def test_triangle_test_on_hand_worked_cases():
    assert _hit([0.25, 0.25, 1.0], DOWN)                                   # the interior
    assert not _hit([0.25, 0.25, 1.0], -DOWN)                              # behind the origin: t = -1
    assert _hit([0.25, 0.25, -1.0], -DOWN)                                 # two-sided
    # corners: u = v = 0; u = 1, v = 0; u = 0, v = 1 -- all inside the closed inequalities
    for c in TRI:
        assert _hit(c + np.array([0.0, 0.0, 1.0]), DOWN)
    assert not _hit([1.0 + 2.0 ** -52, 0.0, 1.0], DOWN) and not _hit([-2.0 ** -60, 0.0, 1.0], DOWN)
    # onto the edges from above: v = 0, u = 0 and u + v = 1 are hits, a step outside is not
    assert _hit([0.5, 0.0, 1.0], DOWN) and _hit([0.0, 0.5, 1.0], DOWN) and _hit([0.5, 0.5, 1.0], DOWN)
    assert not _hit([0.5, -2.0 ** -60, 1.0], DOWN) and not _hit([0.5, 0.5 + 2.0 ** -52, 1.0], DOWN)
    # along an edge, in the triangle's plane: det == 0
    assert not _hit([-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]) and not _hit([0.25, 0.25, 0.0], [1.0, 1.0, 0.0])
    # starting on the plane: t = 0 is not > tmin; with tmin < 0 it is
    assert not _hit([0.25, 0.25, 0.0], DOWN) and _hit([0.25, 0.25, 0.0], DOWN, tmin=-1.0)
    # exactly tmax is a hit, the next double below is not
    assert _hit([0.25, 0.25, 2.0], DOWN, tmax=2.0) and not _hit([0.25, 0.25, 2.0], DOWN, tmax=np.nextafter(2.0, 0.0))
    assert _hit([0.25, 0.25, 2.0], DOWN, tmax=np.inf)
    # parallel to the plane, above it
    assert not _hit([0.25, 0.25, 1.0], [1.0, 0.0, 0.0])
    # degenerate triangles: a point, a segment
    p = np.array([0.25, 0.25, 0.0])
    assert not _hit([0.25, 0.25, 1.0], DOWN, (p, p, p)) and not _hit([0.25, 0.25, 1.0], DOWN, (TRI[0], TRI[1], 0.5 * TRI[1]))
    # a NaN or infinite corner
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            tri = [c.copy() for c in TRI]
            tri[k][1] = bad
            assert not _hit([0.25, 0.25, 1.0], DOWN, tuple(tri))
    # a NaN ray
    assert not _hit([np.nan, 0.25, 1.0], DOWN) and not _hit([0.25, 0.25, 1.0], [0.0, np.nan, -1.0])


def test_occluded_skips_and_ignores_dead_triangles():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [np.nan, 0, 2]], np.float64)
    f = np.array([[0, 1, 2], [3, 4, 5], [0, 1, 9], [0, 1, -1], [6, 4, 5], [0, 0, 1]], np.int32)
    assert A.live_triangles(v, f).tolist() == [True, True, False, False, False, True]
    o, d = np.array([[0.25, 0.25, 3.0]] * 4), np.array([[0, 0, -1.0]] * 4)
    assert A.occluded(v, f, o, d, 0.0, np.inf, [-1, 1, 0, 5]).tolist() == [True, True, True, True]
    assert A.occluded(v, f, o, d, 0.0, 2.5, [-1, 1, 0, 5]).tolist() == [True, False, True, True]
    assert not A.occluded(v, f[2:], o, d).any() and not A.occluded(v, f[:0], o, d).any()


def test_mix32_against_the_written_steps():
    def mix(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        x ^= x >> 16
        return x
    xs = [0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 123456789]
    assert A.mix32(np.array(xs, np.uint64)).tolist() == [mix(x) for x in xs] and mix(0) == 0
    assert len(set(A.mix32(np.arange(4096)).tolist())) == 4096        # a bijection: no two of a run collide
    counts = np.bincount(A.mix32(np.arange(16000)) % 16, minlength=16)
    assert counts.min() > 800 and counts.max() < 1200


def test_duff_frame_is_orthonormal():
    rng = np.random.default_rng(0)
    n = np.concatenate([[[0, 0, 1.0], [0, 0, -1.0], [1.0, 0, 0.0], [0, 1.0, -0.0]], A.unit_rows(rng.standard_normal((100, 3)))])
    T, B = A.duff_frame(n)
    m = np.stack([T, B, n], 1)
    assert np.abs(m @ m.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-15
    assert np.abs(np.linalg.det(m) - 1.0).max() <= 1e-14             # right-handed for both signs of n_z


@pytest.mark.parametrize("K, R", [(1, 1), (64, 16), (100, 3), (7, 2)])
def test_direction_table(K, R):
    import gs2m_mesh_ao as AO
    t = AO.direction_table(K, R, seed=5)
    assert t.shape == (R, K, 3) and t.dtype == np.float64
    assert np.abs(np.sqrt((t * t).sum(2)) - 1.0).max() <= 1e-15
    assert (t[..., 2] > 0).all()
    # the mean and variance of l_z under a cosine-weighted hemisphere are 2/3 and 1/18: four standard errors of K random draws
    assert (np.abs(t[..., 2].mean(1) - 2.0 / 3.0) <= 4.0 * math.sqrt(1.0 / 18.0) / math.sqrt(K)).all()
    assert np.array_equal(t, AO.direction_table(K, R, seed=5)) and not np.array_equal(t, AO.direction_table(K, R, seed=6))
    # every table is the first one rotated about z
    assert np.abs(t[..., 2] - t[0, :, 2]).max() <= 1e-15
    for r in range(R):
        c = (t[r, :, 0] * t[0, :, 0] + t[r, :, 1] * t[0, :, 1]) / (1.0 - t[0, :, 2] ** 2)
        assert np.ptp(c) <= 1e-9
    if K == 64:  # stratified: every cell of the 8 x 8 grid over (u, v) holds one direction
        u, phi = 1.0 - t[0, :, 2] ** 2, np.arctan2(t[0, :, 1], t[0, :, 0]) % (2 * np.pi)
        cells = np.floor(u * 8).astype(int) * 8 + np.floor(phi / (2 * np.pi) * 8).astype(int)
        assert len(set(cells.tolist())) >= 60


def test_occlusion_bytes():
    orm = np.full((4, 3), 7, np.uint8)
    out = A.occlusion_bytes(orm, [0, -1, 3, 2], [64, 0, 0, 21], 64)
    assert out.tolist() == [[255, 7, 7], [7, 7, 7], [0, 7, 7], [84, 7, 7]]   # 255 * 21 / 64 = 83.67


@pytest.mark.parametrize("mesh", [m for m in A.MESHES if m != "n0"])
def test_every_ray_family_has_both_outcomes(mesh):
    """What the GPU equality tests rely on, checked where it is cheap: under the restatement alone at least a tenth of the rays of
    every family is occluded and a tenth is not, so a traversal that always answers the same cannot pass.  (n1 has no second
    triangle for the skip family to fall back on.)"""
    v, f = A.MESHES[mesh]()
    families = [(k, A.ray_family(k, v, f, 1000)) for k in A.FAMILIES if not (mesh == "n1" and k == "skip")]
    if mesh == "grid":
        families += [(k, A.grid_family(k, 1000)) for k in A.GRID_FAMILIES]
    for name, r in families:
        hit = A.occluded(v, f, r["origins"], r["dirs"], r["tmin"], r["tmax"], r["skip"])
        assert 0.1 <= hit.mean() <= 0.9, (mesh, name, hit.mean())
        if name == "skip":
            assert (r["skip"] >= 0).mean() >= 0.1 and hit.sum() <= A.occluded(v, f, r["origins"], r["dirs"]).sum()
        if name == "tmax":   # hits that end at tmax to the bit
            assert (hit & ~A.occluded(v, f, r["origins"], r["dirs"], 0.0, np.nextafter(r["tmax"], 0.0))).sum() >= 100
        if name == "faces":  # the rays lie in the floor's plane or next to it, and some run along its grid lines
            assert (r["dirs"][:, 2] == 0).all() and (np.abs(r["origins"][:, 2] - 0.5) <= 2.0 ** -40).all()
            assert ((r["dirs"][:, 1] == 0) & (r["origins"][:, 1] * 8 % 1 == 0)).sum() >= 20
        if name in ("axis1", "axis2"):
            assert ((r["dirs"] == 0).sum(1) == int(name[-1])).all()


def test_ambient_occlusion_restatement_on_fixed_cases():
    import gs2m_mesh_ao as AO
    table = AO.direction_table(16, 2, seed=1)
    plane = (np.array([[-5, -5, 0], [5, -5, 0], [5, 5, 0], [-5, 5, 0.0]]), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    pts = np.array([[0.1, 0.2, 0.0], [0.3, -0.4, 0.0]])
    up = np.array([[0, 0, 1.0]] * 2)
    assert A.ambient_occlusion(*plane, pts, up, None, table, 1e-4, np.inf).tolist() == [16, 16]
    v, f = A.closed_box()
    inside = np.array([[0.5, 0.5, 0.5], [0.2, 0.7, 0.4], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [np.nan, 0.5, 0.5]])
    nrm = np.array([[0, 0, 1.0], [0.6, 0, -0.8], [0, 0, 0], [np.nan, 0, 1], [0, 0, 1.0]])
    assert A.ambient_occlusion(v, f, inside, nrm, None, table, 1e-4, np.inf).tolist() == [0, 0, 16, 16, 16]
    assert A.ambient_occlusion(v, f, inside, nrm, [0, -1, 0, 0, 0], table, 1e-4, np.inf).tolist() == [0, 16, 16, 16, 16]
    assert A.ambient_occlusion(v, f, inside[:2], nrm[:2], None, table, 1e-4, 0.05).tolist() == [16, 16]   # nothing that close


def test_glb_occlusion_round_trip(tmp_path):
    import gs2m_mesh_texture as MT
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    nrm = np.array([[0, 0, 1]] * 3, np.float32)
    uv = np.array([[0, 0], [1, 0], [0, 1]], np.float32)
    idx = np.arange(3, dtype=np.uint32)
    png = [b"\x89PNG-base", b"\x89PNG-orm-image"]
    before = MT.write_glb(tmp_path / "a.glb", pos, nrm, uv, idx, png)
    assert MT.write_glb(tmp_path / "b.glb", pos, nrm, uv, idx, png, occlusion=False) == before
    assert (tmp_path / "a.glb").read_bytes() == (tmp_path / "b.glb").read_bytes()
    g = MT.read_glb(tmp_path / "a.glb")
    assert g["occlusion"] is False and "occlusionTexture" not in g["json"]["materials"][0]
    with_ao = MT.write_glb(tmp_path / "c.glb", pos, nrm, uv, idx, png, occlusion=True)
    g = MT.read_glb(tmp_path / "c.glb")
    material = g["json"]["materials"][0]
    assert g["occlusion"] is True and with_ao != before and g["images"] == png
    assert material["occlusionTexture"] == {"index": 1} == material["pbrMetallicRoughness"]["metallicRoughnessTexture"]
    tan = np.array([[1, 0, 0, -1]] * 3, np.float32)
    MT.write_glb(tmp_path / "d.glb", pos, nrm, uv, idx, png, tangents=tan, normal_image=b"\x89PNG-normal", occlusion=True)
    g = MT.read_glb(tmp_path / "d.glb")
    assert g["occlusion"] and g["normal_image"] == b"\x89PNG-normal" and g["images"] == png
    with pytest.raises(ValueError):
        MT.write_glb(tmp_path / "e.glb", pos, nrm, uv, idx, png[:1], occlusion=True)


def test_ply_occlusion_round_trip(tmp_path):
    import gs2m_mesh as M
    import gs2m_mesh_bake as MB
    import gs2m_mesh_simplify as MS
    rng = np.random.default_rng(2)
    v = rng.random((5, 3)).astype(np.float32)
    t = np.array([[0, 1, 2], [2, 3, 4]], np.int32)
    vals = rng.random((5, 5)).astype(np.float32)
    seen = np.array([1, 0, 1, 1, 0], bool)
    ao = rng.random(5).astype(np.float32)
    MB.write_material_mesh(tmp_path / "plain.ply", v, t, vals, seen)
    MB.write_material_mesh(tmp_path / "none.ply", v, t, vals, seen, None)
    MB.write_material_mesh(tmp_path / "ao.ply", v, t, vals, seen, ao)
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "none.ply").read_bytes()
    assert len((tmp_path / "ao.ply").read_bytes()) == len((tmp_path / "plain.ply").read_bytes()) + len("property float occlusion\n") + 4 * 5
    head = (tmp_path / "ao.ply").read_bytes().split(b"end_header")[0].decode().split("\n")
    assert head.index("property float occlusion") == head.index("property uchar seen") + 1
    m, p = MB.read_material_mesh(tmp_path / "ao.ply"), MB.read_material_mesh(tmp_path / "plain.ply")
    assert np.array_equal(m["occlusion"], ao) and "occlusion" not in p
    for k in ("vertices", "triangles", "albedo", "roughness", "metallic", "seen"):
        assert np.array_equal(m[k], p[k])
    mesh = M.read_mesh(tmp_path / "ao.ply")                          # still a mesh to every reader of plain meshes
    assert np.array_equal(np.asarray(mesh.vertices, np.float32), v) and np.array_equal(np.asarray(mesh.triangles), t)
    loaded, values, weight = MS.load(tmp_path / "ao.ply")
    assert values.shape == (5, 6) and np.array_equal(values[:, 5], ao) and MS.load(tmp_path / "plain.ply")[1].shape == (5, 5)
    MS.save(tmp_path / "again.ply", loaded, values, weight)
    again = MB.read_material_mesh(tmp_path / "again.ply")
    assert np.array_equal(again["occlusion"], ao) and np.array_equal(again["seen"], seen)
    with pytest.raises(ValueError):
        MB.write_material_mesh(tmp_path / "bad.ply", v, t, vals, seen, ao[:4])
