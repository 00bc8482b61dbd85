"""The tangent frame, the normal-map encode and decode and the glTF fields that carry them, without a GPU: the properties of the
contract (include/gs2m_meshbake.h, the Tangent frame paragraph) on its numpy restatement
(tests/mesh_normalmap_ref.py), the .glb round trip, and the conditions under which tests/test_mesh_normalmap_gpu.py may hold the
device to the restatement."""
import hashlib

import numpy as np
import pytest

import gs2m_mesh_texture as MT
import mesh_normalmap_ref as NM
import mesh_texture_ref as T


def _chart_triangles():
    """every half of every class: corners in the plane z = 0 scaled oddly, UVs of a 512 x 256 atlas -> (a, b, c, uv)"""
    rows = []
    rng = np.random.default_rng(0)
    for k in range(T.CLASSES):
        for half in (0, 1):
            p = rng.normal(size=(3, 3))
            uv = np.array([[(24 + x) / 512.0, (8 + y) / 256.0] for x, y in T.corners(8 << k, half)], np.float32)
            rows.append((p[0], p[1], p[2], uv))
    return [np.stack([r[i] for r in rows]) for i in range(4)]


def _random_triangles(n, seed):
    """random corners and random UVs of positive orientation (det > 0: the atlas makes no mirrored chart, and the frame's w = -1
    holds for those alone), and a normal within 60 degrees of the face normal"""
    rng = np.random.default_rng(seed)
    a, b, c = (rng.normal(size=(n, 3)) for _ in range(3))
    uv = rng.random((n, 3, 2)).astype(np.float32)
    d1, d2 = uv[:, 1].astype(np.float64) - uv[:, 0], uv[:, 2].astype(np.float64) - uv[:, 0]
    flip = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1] < 0
    uv[flip] = uv[flip][:, [0, 2, 1]]
    return a, b, c, uv


def _tilted(nf, rng, max_angle):
    """unit vectors within max_angle of the rows of nf"""
    u, _ = NM._unit(nf)
    x = np.cross(u, rng.normal(size=u.shape))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    ang = rng.random(len(u))[:, None] * max_angle
    return np.cos(ang) * u + np.sin(ang) * x


@pytest.mark.parametrize("which", ["charts", "random"])
def test_frame_is_orthonormal_and_left_handed_in_v(which):
    a, b, c, uv = _chart_triangles() if which == "charts" else _random_triangles(500, 1)
    rng = np.random.default_rng(2)
    nf = NM._cross(b - a, c - a)
    N = _tilted(nf, rng, np.radians(60.0)) * (0.5 + rng.random((len(a), 1)))  # not unit: the frame normalises
    F = NM.frame(a, b, c, uv, N)
    assert F["valid"].all()
    for x, y in (("T", "B"), ("T", "N"), ("B", "N")):
        assert np.abs(NM._dot(F[x], F[y])).max() <= 1e-14
    for x in ("T", "B", "N"):
        assert np.abs(NM._dot(F[x], F[x]) - 1.0).max() <= 1e-14
    assert (NM._dot(F["T"], F["d_u"]) > 0).all()
    assert (NM._dot(F["B"], F["d_v"]) < 0).all()       # the handedness: B towards decreasing v, w = -1
    assert np.abs(F["B"] + NM._cross(F["N"], F["T"])).max() <= 1e-15
    if which == "charts":  # d_u and d_v are the chart's legs: e1 and e2 for half 0, their negatives for half 1
        e1, e2 = b - a, c - a
        s = np.where(np.arange(len(a)) % 2 == 0, 1.0, -1.0)
        assert (NM._dot(F["d_u"], e1) * s > 0).all() and (NM._dot(F["d_v"], e2) * s > 0).all()
    # a normal on the far side of the face, a zero one and a NaN one give the face normal
    for bad in (-N, np.zeros_like(N), np.full_like(N, np.nan)):
        G = NM.frame(a, b, c, uv, bad)
        assert G["valid"].all() and np.abs(G["N"] - NM._unit(nf)[0]).max() <= 1e-15


def test_invalid_frames_are_flagged_and_encode_flat():
    a, b, c, uv = _random_triangles(6, 3)
    N = NM._cross(b - a, c - a)
    uv0 = uv.copy()
    uv0[0, 2] = uv0[0, 1]                       # det == 0: two UVs coincide
    b0 = b.copy()
    b0[1] = a[1] + 2.0 * (c[1] - a[1])          # a zero-area triangle
    a0 = a.copy()
    a0[2, 1] = np.nan
    uv1 = uv.copy()
    uv1[3, 0, 0] = np.inf
    F = NM.frame(a0, b0, c, np.where(np.isfinite(uv1), uv0, uv1), N)
    assert list(F["valid"]) == [False, False, False, False, True, True]
    assert (F["T"][:4] == 0).all() and (F["B"][:4] == 0).all() and np.isfinite(F["N"]).all()
    n = np.random.default_rng(4).normal(size=(6, 3))
    m, computed, _ = NM.encode(F, n)
    assert (m[:4] == [0.0, 0.0, 1.0]).all() and not computed[:4].any() and computed[4:].all()
    assert (NM.pack(m[:4]) == [128, 128, 255]).all()
    assert np.array_equal(NM.decode(F, np.random.default_rng(5).normal(size=(6, 3)))[:4], F["N"][:4])
    # a zero or non-finite normal encodes flat in a valid frame too
    G = NM.frame(a[4:], b[4:], c[4:], uv[4:], N[4:])
    for bad in (np.zeros((2, 3)), np.full((2, 3), np.inf)):
        assert (NM.encode(G, bad)[0] == [0.0, 0.0, 1.0]).all()
    # and so does one that clamps to zero: the opposite of N in an axis-aligned frame, where the dots are exact
    E = NM.frame([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], np.array([[[0.0, 0.0], [0.5, 0.0], [0.0, 0.5]]]), [0.0, 0.0, 2.0])
    assert E["valid"].all() and (E["T"] == [1.0, 0.0, 0.0]).all() and (E["B"] == [0.0, -1.0, 0.0]).all()
    assert (NM.encode(E, [[0.0, 0.0, -3.0]])[0] == [0.0, 0.0, 1.0]).all()


def test_encode_then_decode_is_within_the_quantisation_bound():
    a, b, c, uv = _random_triangles(2000, 6)
    rng = np.random.default_rng(7)
    F = NM.frame(a, b, c, uv, _tilted(NM._cross(b - a, c - a), rng, np.radians(50.0)))
    n = _tilted(F["N"], rng, np.radians(89.0))  # the upper hemisphere of the frame
    m, computed, _ = NM.encode(F, n * (0.2 + rng.random((len(n), 1))))
    assert computed.all() and np.abs(np.linalg.norm(m, axis=1) - 1.0).max() <= 1e-15
    back = NM.decode(F, NM.unpack(NM.pack(m)))
    angle = np.arccos(np.clip(NM._dot(back, n), -1.0, 1.0))
    assert 0.0067 < NM.QUANT_ANGLE < 0.0069
    assert angle.max() <= NM.QUANT_ANGLE
    assert np.abs(NM.unpack(NM.pack(m)) - m).max() <= 1.0 / 255.0 + 1e-15  # what the derivation rests on
    # below the horizon the encode clamps m_z: the decoded normal is the projection onto the tangent plane
    low = -0.5 * F["N"] + F["T"]
    m, _, _ = NM.encode(F, low)
    assert (m[:, 2] == 0).all() and np.abs(m[:, 0] - 1.0).max() <= 1e-14


# ---- glb -----------------------------------------------------------------------------------------------------------------------

def _glb_arrays():
    rng = np.random.default_rng(8)
    pos = rng.normal(size=(6, 3)).astype(np.float32)
    nrm = rng.normal(size=(6, 3)).astype(np.float32)
    uv = rng.random((6, 2)).astype(np.float32)
    idx = np.arange(6, dtype=np.uint32)
    images = [b"\x89PNG-base-colour-bytes", b"\x89PNG-orm"]  # write_glb embeds the files as they are
    return pos, nrm, uv, idx, images


# sha256 of the file the writer of the commit before this feature (git show HEAD~:gs-2m_amd/gs2m_mesh_texture.py) makes of _glb_arrays()
PARENT_GLB_SHA256 = "55b090b8c1d0873f9e519eeb5584d341830835d335933cdc1b7d25c47c924924"
PARENT_GLB_ONE_IMAGE_SHA256 = "0fa0aee99a4c8a416fe52b56c672c28eea2a9e1b8cb747301d2a4eb422744635"


def test_glb_without_the_new_arguments_is_the_parents_bytes(tmp_path):
    pos, nrm, uv, idx, images = _glb_arrays()
    data = MT.write_glb(tmp_path / "a.glb", pos, nrm, uv, idx, images)
    assert hashlib.sha256(data).hexdigest() == PARENT_GLB_SHA256
    one = MT.write_glb(tmp_path / "b.glb", pos, nrm, uv, idx, images[:1], tangents=None, normal_image=None)
    assert hashlib.sha256(one).hexdigest() == PARENT_GLB_ONE_IMAGE_SHA256
    g = MT.read_glb(tmp_path / "a.glb")
    assert g["tangents"] is None and g["normal_image"] is None and g["images"] == images


@pytest.mark.parametrize("n_images", [1, 2])
def test_glb_round_trips_tangents_and_the_normal_texture(tmp_path, n_images):
    pos, nrm, uv, idx, images = _glb_arrays()
    images = images[:n_images]
    tan = np.concatenate([np.random.default_rng(9).normal(size=(6, 3)), np.full((6, 1), -1.0)], 1).astype(np.float32)
    png = b"\x89PNG-normal-map!"
    data = MT.write_glb(tmp_path / "n.glb", pos, nrm, uv, idx, images, tangents=tan, normal_image=png)
    g = MT.read_glb(tmp_path / "n.glb")
    assert g["tangents"].tobytes() == tan.tobytes() and g["normal_image"] == png and g["images"] == images
    assert g["positions"].tobytes() == pos.tobytes() and g["uvs"].tobytes() == uv.tobytes()
    doc = g["json"]
    prim = doc["meshes"][0]["primitives"][0]
    acc = doc["accessors"][prim["attributes"]["TANGENT"]]
    assert acc["type"] == "VEC4" and acc["componentType"] == 5126 and acc["count"] == 6
    assert doc["bufferViews"][acc["bufferView"]]["byteOffset"] % 4 == 0
    tex = doc["textures"][doc["materials"][0]["normalTexture"]["index"]]
    assert doc["images"][tex["source"]]["mimeType"] == "image/png" and len(doc["images"]) == n_images + 1
    assert (tmp_path / "n.glb").read_bytes() == data and len(data) % 4 == 0
    # everything the old file holds is where it was: the new views come last
    old = MT.write_glb(tmp_path / "o.glb", pos, nrm, uv, idx, images)
    assert doc["bufferViews"][:4 + n_images] == MT.read_glb(tmp_path / "o.glb")["json"]["bufferViews"] and len(old) < len(data)
    for kw in (dict(tangents=tan), dict(normal_image=png), dict(tangents=tan[:5], normal_image=png)):
        with pytest.raises(ValueError):
            MT.write_glb(tmp_path / "bad.glb", pos, nrm, uv, idx, images, **kw)


# ---- the conditions of the GPU comparisons -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NM.SCENES)
def test_scenes_keep_their_decisions_and_bytes_away_from_the_edges(name):
    s = NM.scene(name)
    w = s["want"]
    assert w["band"].mean() <= 0.01
    for key, margin in w["margins"].items():
        near = (margin < 1e-9) & (margin != 0.0)
        assert not near.any(), key
    own = s["tex"]["owner"].reshape(-1) >= 0
    assert not w["computed"][~own].any() and (w["bytes"][~own] == [128, 128, 255]).all()
    if name not in ("zero_area",):
        assert w["computed"][own].mean() > 0.9
    if name == "zero_area":  # two of the three triangles have no area: their texels encode flat
        assert w["computed"].any() and (~w["computed"][own]).sum() > 30
    if name == "opposed":    # the frame took the face normal, +z, not the vertex normals
        F, _ = NM.texel_frames(s["tex"]["owner"], s["tex"]["normals"], s["tris"], s["atlas"]["uvs"], s["verts"])
        assert (F["N"][own] == [0.0, 0.0, 1.0]).all() and (w["margins"]["nf"][own] > 0.5).all()
    assert np.abs(np.linalg.norm(w["tangent"], axis=1) - 1.0).max() <= 1e-15


def test_the_atlas_charts_all_have_a_positive_determinant():
    """w = -1 for every triangle: test it, do not assume it -- on the UVs the atlas really writes, fp32 rounding included"""
    for name in NM.SCENES:
        s = NM.scene(name)
        uv = s["atlas"]["uvs"].astype(np.float64)
        d1, d2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
        assert (d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1] > 0).all(), name
        tris = np.asarray(s["tris"], np.int64)
        p = s["verts"][tris]
        nf = NM._cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        F = NM.frame(p[:, 0], p[:, 1], p[:, 2], uv, nf)
        ok = F["valid"]
        assert (NM._dot(F["B"], F["d_v"])[ok] < 0).all() and (NM._dot(F["T"], F["d_u"])[ok] > 0).all(), name


def test_sphere_gbuffer_restatement_decodes_its_own_bake():
    """the restatement closes its own loop: drawn through the normal map, the icosphere's normals are the baked field's within the
    quantisation and the bilinear mixing of neighbouring texels (the field turns by less than 0.05 rad over a texel here)"""
    c, s = T.sphere_case(), NM.scene("sphere")
    g = NM.sphere_gbuffer(1)
    cov = g["coverage"]
    assert cov.any() and np.abs(np.linalg.norm(g["normal"][cov].astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    flat = NM.sphere_gbuffer(1, with_normal_map=False)
    assert np.array_equal(flat["coverage"], cov) and np.array_equal(flat["albedo"], g["albedo"])
    moved = np.arccos(np.clip((g["normal"][cov].astype(np.float64) * flat["normal"][cov]).sum(1), -1, 1))
    assert 0.05 < np.median(moved) < 0.7  # the map does something, and nothing wild
