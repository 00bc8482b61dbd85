"""The triangle atlas, the texel bake's restatement and the glTF container without a GPU (tests/mesh_texture_ref.py,
gs2m_mesh_texture.write_glb / read_glb), and the conditions under which tests/test_mesh_texture_gpu.py may hold the device to the
restatement."""
import io
import json
import struct

import numpy as np
import pytest

import mesh_bake_ref as B
import mesh_texture_ref as T


def _cells_of(L):
    """every cell of a layout as (x, y, side, class, cell index)"""
    out = []
    for k in range(T.CLASSES):
        for m in range((L["hist"][k] + 1) // 2):
            ox, oy = T.cell_origin(L, k, m)
            out.append((ox, oy, 8 << k, k, m))
    return out


def _check_layout(L):
    cover = np.zeros((L["height"], L["width"]), np.int64)
    for ox, oy, s, _, _ in _cells_of(L):
        assert ox % s == 0 and oy % s == 0                       # aligned to its side
        assert ox + s <= L["width"] and oy + s <= L["height"]
        cover[oy:oy + s, ox:ox + s] += 1
    assert cover.max(initial=0) <= 1                              # cells do not overlap
    assert cover.sum() == 64 * L["total"]
    if L["total"]:
        j = int(np.log2(L["width"] // 8))
        assert 4 ** j >= L["total"] and (j == 0 or 4 ** (j - 1) < L["total"])
        assert L["height"] == (L["width"] // 2 if j >= 1 and 2 * L["total"] <= 4 ** j else L["width"])
    else:
        assert (L["width"], L["height"]) == (0, 0)
    for k in range(T.CLASSES):
        assert L["base"][k] % 4 ** k == 0
    # every texel has at most one owner, and every triangle's half owns exactly its texels
    n = sum(L["hist"])
    owner, side, half, li, lj = T.owners(L, np.arange(n))
    assert ((owner >= 0) <= (cover == 1)).all()
    ids, counts = np.unique(owner[owner >= 0], return_counts=True)
    assert np.array_equal(ids, np.arange(n))
    for k in range(T.CLASSES):
        s = 8 << k
        for r in range(L["hist"][k]):
            assert counts[L["start"][k] + r] == (s * (s + 1) // 2 if r % 2 == 0 else s * (s - 1) // 2)


def test_random_histograms():
    rng = np.random.default_rng(0)
    hists = [[0] * 6, [1, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0], [4, 0, 0, 0, 0, 0], [1] * 6, [0, 0, 0, 0, 0, 1], [64, 0, 0, 0, 0, 0],
             [65, 0, 0, 0, 0, 0]]
    hists += [list(rng.integers(0, 9, 6) * (rng.random(6) < 0.6)) for _ in range(12)]
    for h in hists:
        _check_layout(T.layout(h))
    assert (T.layout([64, 0, 0, 0, 0, 0])["width"], T.layout([64, 0, 0, 0, 0, 0])["height"]) == (64, 32)
    assert (T.layout([65, 0, 0, 0, 0, 0])["width"], T.layout([65, 0, 0, 0, 0, 0])["height"]) == (64, 64)
    assert T.layout([0, 0, 0, 0, 0, 8192])["width"] == 16384
    with pytest.raises(ValueError, match="unsupported"):
        T.layout([0, 0, 0, 0, 0, 8193])
    for m in list(range(70)) + [4 ** 11 - 1]:
        assert T.morton_encode(*T.morton_decode(m)) == m
    assert T.morton_decode(1) == (1, 0) and T.morton_decode(2) == (0, 1)  # x in the even bits


def test_gpu_scenes_layouts():
    for name in T.SMALL_SHAPES:
        v, f, d = T.small_shape(name)
        a = T.build(v, f, d)
        _check_layout(a)
        assert T.class_margin(v, f, d) > 1e-9  # no class decision sits on its threshold
        tex = T.texels(v, None, f, a)
        assert np.array_equal(np.unique(tex["owner"][tex["owner"] >= 0]), np.arange(len(f)))
    c = T.sphere_case()
    _check_layout(c["atlas"])
    assert T.class_margin(c["verts"], c["tris"], c["density"]) > 1e-9 and sum(h > 0 for h in c["atlas"]["hist"]) == 2
    assert T.build(*T.small_shape("clamped"))["hist"][5] == 1 and T.build(*T.small_shape("zero_area"))["hist"][0] == 2


@pytest.mark.parametrize("k", range(T.CLASSES))
def test_bilinear_taps_stay_in_the_chart(k):
    """Both halves of a cell of every class: all four taps of any point of the chart -- corners, legs and hypotenuse included, on
    a grid of 1/4 texel that hits every texel centre and boundary -- lie in the cell and are texels of that half, whatever their
    weight."""
    s = 8 << k
    Lc = s - 4
    L = T.layout([2 if c == k else 0 for c in range(T.CLASSES)])
    owner, *_ = T.owners(L, np.arange(2))
    g = np.arange(0, 4 * Lc + 1) / 4.0
    a, b = np.meshgrid(g, g)
    inside = a + b <= Lc
    a, b = a[inside], b[inside]
    for half in (0, 1):
        x, y = (1 + a, 1 + b) if half == 0 else (s - 1 - a, s - 1 - b)
        _, taps, w = T.sample_bilinear(np.zeros((s, s, 1)), np.stack([x / s, y / s], 1))
        assert w.shape == (len(a), 4) and (taps >= 0).all() and (taps < s).all()
        assert (owner[taps[..., 0], taps[..., 1]] == half).all()


def test_affine_field_comes_back_from_a_bilinear_lookup():
    """Before packing, in fp64: exact (1e-9) wherever the taps are interior texels -- an interior texel holds the field at its
    centre, and bilinear interpolation reproduces an affine function.  A skirt texel holds the field at a point ON the triangle
    (the clamp of include/gs2m_atlas.h), not its continuation, so a lookup that touches the skirt is off by at most the field's
    change over the clamp's displacement: under 1.5 texels along a leg and 2 across the hypotenuse, times the field's gradient
    per texel."""
    c = T.plane_case()
    verts, tris, a, tex = c["verts"], c["tris"], c["atlas"], c["tex"]
    values = np.where((tex["owner"] >= 0)[..., None], T.affine_field(tex["points"]), 0.0)
    rng = np.random.default_rng(2)
    t = rng.integers(0, len(tris), 2000)
    l = rng.dirichlet(np.ones(3), 2000)
    l[:60] = np.repeat(np.eye(3), 20, axis=0)               # corners
    l[60:120, 0] = 0.0                                      # the hypotenuse
    l[60:120, 1:] /= l[60:120, 1:].sum(1, keepdims=True)
    p = (l[:, :, None] * verts[tris[t]]).sum(1)
    uv = (l[:, :, None] * a["uvs"][t].astype(np.float64)).sum(1)
    got, taps, w = T.sample_bilinear(values, uv)
    assert (tex["owner"][taps[..., 0], taps[..., 1]] == t[:, None]).all()  # all four taps, whatever their weight
    err = np.abs(got - T.affine_field(p)).max(1)
    inner = (tex["interior"][taps[..., 0], taps[..., 1]] | (w == 0)).all(1)
    assert inner.sum() > 1000 and err[inner].max() <= 1e-9
    assert err.max() <= 2.0 * _field_change_per_texel(verts, tris, a)


def _field_change_per_texel(verts, tris, atlas):
    """The most any channel of the affine field changes over one texel step of a chart: a leg of L = side - 4 texels spans the
    edge a -> b (the step in i) or a -> c (the step in j), so the change per step is the field's change along the edge over L;
    the largest of each over all triangles and channels, the two directions added."""
    legs = (atlas["cells"][:, 2] - 4).astype(np.float64)[:, None]
    along_ab = np.abs((verts[tris[:, 1]] - verts[tris[:, 0]]) @ T.AFFINE[:, :3].T) / legs
    along_ac = np.abs((verts[tris[:, 2]] - verts[tris[:, 0]]) @ T.AFFINE[:, :3].T) / legs
    return along_ab.max() + along_ac.max()


def _png(a):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, format="PNG")
    return b.getvalue()


def test_glb_round_trip(tmp_path):
    import gs2m_mesh_texture as MT
    rng = np.random.default_rng(1)
    pos = rng.normal(size=(9, 3)).astype(np.float32)
    nrm = rng.normal(size=(9, 3)).astype(np.float32)
    uv = rng.random((9, 2)).astype(np.float32)
    idx = np.arange(9, dtype=np.uint32)
    base, orm = rng.integers(0, 256, (8, 16, 3), dtype=np.uint8), rng.integers(0, 256, (8, 16, 3), dtype=np.uint8)
    for images in ([_png(base), _png(orm)], [_png(base)[:-1] + b"\x82"]):  # (PNG lengths that are no multiple of 4, too)
        data = MT.write_glb(tmp_path / "a.glb", pos, nrm, uv, idx, images)
        assert (tmp_path / "a.glb").read_bytes() == data
        magic, version, total = struct.unpack_from("<III", data, 0)
        assert (magic, version, total) == (0x46546C67, 2, len(data)) and total % 4 == 0
        n, kind = struct.unpack_from("<II", data, 12)
        assert kind == 0x4E4F534A and n % 4 == 0
        doc = json.loads(data[20:20 + n])
        m, kind = struct.unpack_from("<II", data, 20 + n)
        assert kind == 0x004E4942 and m % 4 == 0 and 28 + n + m == total and doc["buffers"] == [{"byteLength": m}]
        end = 0
        for v in doc["bufferViews"]:
            assert v["byteOffset"] % 4 == 0 and v["byteOffset"] >= end and v["byteOffset"] + v["byteLength"] <= m
            end = v["byteOffset"] + v["byteLength"]
        acc = doc["accessors"]
        assert [x["count"] for x in acc] == [9, 9, 9, 9] and [x["type"] for x in acc] == ["VEC3", "VEC3", "VEC2", "SCALAR"]
        assert acc[0]["min"] == [float(x) for x in pos.min(0)] and acc[0]["max"] == [float(x) for x in pos.max(0)]
        assert all("min" not in x for x in acc[1:])
        prim = doc["meshes"][0]["primitives"][0]
        assert prim["attributes"] == {"POSITION": 0, "NORMAL": 1, "TEXCOORD_0": 2} and prim["indices"] == 3 and len(doc["meshes"]) == 1
        pbr = doc["materials"][0]["pbrMetallicRoughness"]
        assert pbr["baseColorTexture"] == {"index": 0} and ("metallicRoughnessTexture" in pbr) == (len(images) == 2)
        assert len(doc["images"]) == len(doc["textures"]) == len(images)
        g = MT.read_glb(tmp_path / "a.glb")
        assert g["uvs"].tobytes() == uv.tobytes() and g["indices"].tobytes() == idx.tobytes()
        assert g["positions"].tobytes() == pos.tobytes() and g["normals"].tobytes() == nrm.tobytes()
        assert g["images"] == images
    g = MT.read_glb(tmp_path / "a.glb")
    MT.write_glb(tmp_path / "b.glb", g["positions"], g["normals"], g["uvs"], g["indices"], g["images"])
    assert (tmp_path / "b.glb").read_bytes() == (tmp_path / "a.glb").read_bytes()
    data = MT.write_glb(tmp_path / "a.glb", pos, nrm, uv, idx, [_png(base), _png(orm)])
    px = [MT.decode_png(b) for b in MT.read_glb(tmp_path / "a.glb")["images"]]
    assert np.array_equal(px[0], base) and np.array_equal(px[1], orm)
    (tmp_path / "bad.glb").write_bytes(data[:-4])
    with pytest.raises(ValueError, match="not a glTF"):
        MT.read_glb(tmp_path / "bad.glb")
    with pytest.raises(ValueError):
        MT.write_glb(tmp_path / "c.glb", pos, nrm, uv, np.array([0, 1, 9], np.uint32), [_png(base)])


def test_conditions_of_the_gpu_comparison():
    """No per-view decision of the GPU scene lies within MARGIN of its threshold unless exactly on it, and at most 1 % of the
    packed sRGB bytes sit within 1e-6 of a rounding boundary."""
    c = T.sphere_case()
    for args in ((5, True, True), (3, False, True), (5, True, False)):
        s, w, use, margin = T.sphere_reference(*args)
        assert margin.min() >= B.MARGIN, args
        assert use.any(axis=0).all() and not use.all()
        seen = (w >= 0.3) & (w > 0)
        near = np.abs(w - 0.3)
        assert near[near > 0].min() >= B.MARGIN
        out, _ = T.resolve(c["tex"], c["tris"], s, w, 0.3, [0.2 + 0.1 * k for k in range(args[0])])
        assert (T.srgb_band(out) < 1e-6).mean() <= 0.01
    own = c["tex"]["owner"] >= 0
    assert own.any() and not own.all() and c["tex"]["interior"].any() and (own & ~c["tex"]["interior"]).any()
