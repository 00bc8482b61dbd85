"""The tangent-space normal-map bake and the textured G-buffer on the GPU (csrc/mesh_bake.hip, csrc/mesh_view.hip,
csrc/tangent_frame.h; gs2m_mesh_texture.py, gs2m_mesh_view.py) against the fp64 restatement of tests/mesh_normalmap_ref.py, and
the closed loop bake -> .glb -> draw.  All data is synthetic.

Tolerances: `tangent` to 1e-12 relative (the bound tests/test_mesh_texture_gpu.py uses for the same fp64 arithmetic); the bytes to
the restatement's packing of the device's own `tangent`, and to the restatement's bytes outside its 1e-9 band
(tests/test_mesh_normalmap.py asserts that the band holds at most 1 % of the bytes and that no decision is near its threshold);
G-buffer floats to 1 ulp of the restatement's fp32 rounding; a drawn normal to the derived quantisation bound
mesh_normalmap_ref.QUANT_ANGLE of the baked one."""
import os
import types

import numpy as np
import pytest
import torch

import gs2m_mesh_texture as MT
import gs2m_mesh_view as MVW
import gs2m_native as N
import mesh_bake_ref as B
import mesh_normalmap_ref as NM
import mesh_texture_ref as T
import mesh_view_ref as MV

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = "invalid argument", "unsupported size"
FLAT = [128, 128, 255]


def _cuda(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def _mesh(verts, tris):
    return types.SimpleNamespace(vertices=_cuda(verts, torch.float64), triangles=_cuda(tris, torch.int32))


def _close(got, want, rel):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= rel * np.abs(want)))


def _ulps(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(np.float32)).astype(np.float64)


def _scene_tensors(s):
    """the restatement's own texels and resolved values on the device"""
    tex, a = s["tex"], s["atlas"]
    return dict(owner=_cuda(tex["owner"], torch.int32).reshape(-1), tn=_cuda(tex["normals"]).reshape(-1, 3), tris=_cuda(s["tris"], torch.int32),
                uvs=_cuda(a["uvs"], torch.float32), verts=_cuda(s["verts"], torch.float64), values=_cuda(s["values"], torch.float32),
                width=a["width"], height=a["height"])


def _normals(d, lo=0, hi=None, tangent=True, C=8, offset=5, fill=7, **kw):
    """gs2m_texture_normals on the texels lo .. hi of the tensors d -> (bytes (n, 3), tangent (n, 3) or None), prefilled with `fill`"""
    hi = len(d["owner"]) if hi is None else hi
    n = hi - lo
    out = torch.full((n, 3), fill, dtype=torch.uint8, device="cuda")
    tan = torch.full((n, 3), float(fill), dtype=torch.float64, device="cuda") if tangent else None
    a = dict(n=n, owner=N.ptr(d["owner"][lo:hi]), tn=N.ptr(d["tn"][lo:hi]), nt=len(d["tris"]), tris=N.ptr(d["tris"]), uvs=N.ptr(d["uvs"]),
             nv=len(d["verts"]), verts=N.ptr(d["verts"]), C=C, offset=offset, values=N.ptr(d["values"][lo:hi]), out=N.ptr(out), tan=N.ptr(tan))
    a.update(kw)
    N.launch("gs2m_texture_normals", out.device, a["n"], a["owner"], a["tn"], a["nt"], a["tris"], a["uvs"], a["nv"], a["verts"], a["C"], a["offset"],
             a["values"], a["out"], a["tan"])
    torch.cuda.synchronize()
    return out, tan


# ---- gs2m_texture_normals ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NM.SCENES)
def test_texture_normals_against_the_restatement(name):
    s = NM.scene(name)
    d, want = _scene_tensors(s), s["want"]
    out, tan = _normals(d)
    got, m = out.cpu().numpy(), tan.cpu().numpy()
    assert _close(m, want["tangent"], 1e-12)
    assert np.array_equal(got, NM.pack(m))                          # the packing alone, on the device's own values
    assert np.array_equal(got[~want["band"]], want["bytes"][~want["band"]])
    assert np.abs(got.astype(int) - want["bytes"].astype(int)).max() <= 1
    empty = s["tex"]["owner"].reshape(-1) < 0
    assert (got[empty] == FLAT).all() and (m[empty] == [0.0, 0.0, 1.0]).all()
    assert (got[want["computed"]] != FLAT).any(axis=1).mean() > 0.9  # the field is tilted: the map is not flat where it was baked
    # tangent == NULL, and two calls over a split of the rows
    assert torch.equal(_normals(d, tangent=False)[0], out)
    k = (d["height"] // 2 + 1) * d["width"]
    (o1, t1), (o2, t2) = _normals(d, 0, k), _normals(d, k, None)
    assert torch.equal(torch.cat([o1, o2]), out) and torch.equal(torch.cat([t1, t2]), tan)
    if name == "one":
        assert (d["width"], d["height"]) == (8, 8) and empty.sum() == 28  # half 1 is empty
    if name == "six_classes":
        assert sorted(set(s["atlas"]["cells"][:, 2])) == [8, 16, 32, 64, 128, 256]


def test_empty_mesh_and_other_offsets():
    z = torch.zeros(0, device="cuda")
    N.launch("gs2m_texture_normals", z.device, 0, None, None, 0, None, None, 0, None, 3, 0, None, None, None)
    a = MT.build_atlas(_mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int32)), density=3.0)
    nm = MT.pack_normal_map(a, torch.zeros((0, 0, 8), device="cuda"))
    assert nm.shape == (0, 0, 3) and nm.dtype == torch.uint8
    # C = 3 with the normal alone, and C = 6 (an rgb bake) with it last: the same bytes as from the planes 5 .. 7 of 8
    s = NM.scene("four")
    d = _scene_tensors(s)
    want = _normals(d)[0]
    for C, offset, cols in ((3, 0, [5, 6, 7]), (6, 3, [0, 1, 2, 5, 6, 7]), (8, 2, [0, 1, 5, 6, 7, 2, 3, 4])):
        e = dict(d, values=d["values"][:, cols].contiguous())
        assert torch.equal(_normals(e, C=C, offset=offset)[0], want), (C, offset)


def test_untrusted_owners_and_corners_encode_flat():
    s = NM.scene("four")
    d = _scene_tensors(s)
    want = _normals(d)[0]
    own = d["owner"] >= 0
    bad = dict(d, owner=torch.where(d["owner"] == 2, torch.full_like(d["owner"], len(d["tris"])), d["owner"]))
    out, tan = _normals(bad)
    hit = (d["owner"] == 2)
    assert hit.any() and (out[hit].cpu().numpy() == FLAT).all() and (tan[hit].cpu().numpy() == [0.0, 0.0, 1.0]).all()
    assert torch.equal(out[~hit], want[~hit])
    tris = d["tris"].clone()
    tris[1, 2], tris[3, 0] = len(d["verts"]), -1
    out, _ = _normals(dict(d, tris=tris))
    hit = (d["owner"] == 1) | (d["owner"] == 3)
    assert (out[hit].cpu().numpy() == FLAT).all() and torch.equal(out[~hit], want[~hit]) and (own & ~hit).any()


def test_errors_leave_the_outputs_untouched():
    s = NM.scene("four")
    d = _scene_tensors(s)
    for kw in (dict(C=2, offset=0), dict(C=9), dict(offset=-1), dict(offset=6), dict(n=-1), dict(nt=-1), dict(nv=-1), dict(owner=None),
               dict(tn=None), dict(values=None), dict(tris=None), dict(uvs=None), dict(verts=None)):
        out = torch.full((len(d["owner"]), 3), 7, dtype=torch.uint8, device="cuda")
        tan = torch.full((len(d["owner"]), 3), 7.0, dtype=torch.float64, device="cuda")
        with pytest.raises(RuntimeError, match=INVALID):
            _normals(d, out=N.ptr(out), tan=N.ptr(tan), **kw)
        torch.cuda.synchronize()
        assert (out == 7).all() and (tan == 7).all(), kw
    out = torch.full((4, 3), 7, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match=INVALID):
        _normals(d, out=None)
    # the textured G-buffer
    g = _gbuffer_case(1)
    for kw in (dict(tw=0), dict(th=0), dict(ss=5), dict(ss=0), dict(W=0), dict(fx=0.0), dict(base=None), dict(uvs=None), dict(vis=None),
               dict(out_normal=None), dict(coverage=None)):
        with pytest.raises(RuntimeError, match=INVALID):
            _gbuffer(g, fill=7.0, **kw)
        assert all((x == 7).all() for x in g["last"]), kw
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        _gbuffer(g, fill=7.0, tw=16385)
    assert all((x == 7).all() for x in g["last"])


# ---- the bake with eight planes ------------------------------------------------------------------------------------------------

def test_eight_planes_leave_the_first_five_their_bits():
    c = T.sphere_case()
    a = MT.build_atlas(_mesh(c["verts"], c["tris"]), density=c["density"])
    rng = np.random.default_rng(31)
    n = rng.normal(size=(len(c["w2c"]), 3, c["H"], c["W"]))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    maps8 = np.concatenate([c["maps"], n.astype(np.float32)], axis=1)
    args = (_cuda(c["w2c"]), c["fx"], c["fy"], c["cx"], c["cy"])
    att = rng.random((len(c["verts"]), 5)).astype(np.float32)
    att8 = np.concatenate([att, np.zeros((len(att), 3), np.float32)], axis=1)
    five = MT.bake_texel_attributes(a, *args, _cuda(c["maps"]), _cuda(c["mask"]), view_batch=2, fallback=(1, 2, 3, 4, 5), attributes=_cuda(att))
    eight = MT.bake_texel_attributes(a, *args, _cuda(maps8), _cuda(c["mask"]), view_batch=3, fallback=(1, 2, 3, 4, 5, 0, 0, 0), attributes=_cuda(att8))
    assert eight[0].shape[2] == 8 and torch.equal(eight[0][..., :5], five[0]) and torch.equal(eight[1], five[1]) and torch.equal(eight[2], five[2])
    seen = eight[1]
    length = eight[0][..., 5:].norm(dim=2)
    assert seen.any() and (~seen).any() and (length[~seen] == 0).all()          # an unseen or empty texel carries a zero normal
    assert (length[seen] <= 1.0 + 1e-6).all() and (length[seen] > 0).any()     # a mean of unit vectors
    base5, orm5 = MT.pack_textures(five[0])
    base8, orm8 = MT.pack_textures(eight[0])                                    # the normal planes are not the materials'
    assert torch.equal(base5, base8) and torch.equal(orm5, orm8)
    nm = MT.pack_normal_map(a, eight[0])
    assert nm.shape == (a.height, a.width, 3) and (nm[~seen].cpu().numpy() == FLAT).all() and (nm[seen].cpu().numpy() != FLAT).any()


# ---- gs2m_meshview_gbuffer_textured --------------------------------------------------------------------------------------------

NAMES = ("normal", "view_dir", "albedo", "roughness", "metallic", "coverage")


def _gbuffer_case(ss, smooth=True, with_normal_map=True):
    c, s = T.sphere_case(), NM.scene("sphere")
    H, W = c["atlas"]["height"], c["atlas"]["width"]
    base, orm = NM.random_textures(H, W, 21)
    return dict(verts=_cuda(c["verts"], torch.float64), tris=_cuda(c["tris"], torch.int32), uvs=_cuda(c["atlas"]["uvs"], torch.float32),
                w2c=_cuda(c["w2c"][:NM.VIEWS]), fx=c["fx"], fy=c["fy"], cx=c["cx"], cy=c["cy"], W=c["W"], H=c["H"], ss=ss,
                vis=_cuda(NM.keys(NM.sphere_visibility(ss))), normals=_cuda(c["normals"]) if smooth else None, tw=W, th=H, base=_cuda(base),
                srgb=1, orm=_cuda(orm), nm=_cuda(s["want"]["bytes"].reshape(H, W, 3)) if with_normal_map else None)


def _gbuffer(g, fill=None, **kw):
    a = dict(g)
    a.update(kw)
    n, Hs, Ws = len(a["w2c"]), g["H"] * g["ss"], g["W"] * g["ss"]
    new = (lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="cuda")) if fill is None else \
        (lambda *shape, dtype=torch.float32: torch.full(shape, fill, dtype=dtype, device="cuda"))
    out = dict(normal=new(n, Hs, Ws, 3), view_dir=new(n, Hs, Ws, 3), albedo=new(n, Hs, Ws, 3), roughness=new(n, Hs, Ws), metallic=new(n, Hs, Ws),
               coverage=new(n, Hs, Ws, dtype=torch.uint8))
    g["last"] = list(out.values())
    p = {("out_" + k if k != "coverage" else k): N.ptr(x) for k, x in out.items()}
    for k in p:
        if k in kw:
            p[k] = kw[k]
    ptr = lambda k: None if a[k] is None else N.ptr(a[k])
    N.launch("gs2m_meshview_gbuffer_textured", g["verts"].device, len(a["verts"]), N.ptr(a["verts"]), len(a["tris"]), N.ptr(a["tris"]), ptr("uvs"), n,
             N.ptr(a["w2c"]), a["fx"], a["fy"], a["cx"], a["cy"], a["W"], a["H"], a["ss"], ptr("vis"), ptr("normals"), a["tw"], a["th"], ptr("base"),
             a["srgb"], ptr("orm"), ptr("nm"), p["out_normal"], p["out_view_dir"], p["out_albedo"], p["out_roughness"], p["out_metallic"], p["coverage"])
    torch.cuda.synchronize()
    return {k: x.cpu().numpy() for k, x in out.items()}


@pytest.mark.parametrize("ss,smooth,with_normal_map", [(1, True, True), (2, True, True), (2, False, False), (1, False, True)])
def test_textured_gbuffer_against_the_restatement(ss, smooth, with_normal_map):
    want = NM.sphere_gbuffer(ss, smooth, with_normal_map)
    got = _gbuffer(_gbuffer_case(ss, smooth, with_normal_map))
    cov = want["coverage"]
    assert np.array_equal(got["coverage"].astype(bool), cov) and 0.1 < cov.mean() < 0.9
    for k in NAMES[:5]:
        assert _ulps(got[k], want[k]).max() <= 1.0, k
        assert (got[k][~cov] == 0).all(), k
    assert np.abs(np.linalg.norm(got["normal"][cov].astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    assert ((got["normal"][cov].astype(np.float64) * got["view_dir"][cov]).sum(1) >= -1e-6).all()  # towards the eye


def test_without_textures_roughness_is_one_and_metallic_zero():
    g = _gbuffer_case(1)
    got, full = _gbuffer(g, orm=None), _gbuffer(g)
    cov = got["coverage"].astype(bool)
    assert (got["roughness"][cov] == 1).all() and (got["metallic"] == 0).all() and (got["roughness"][~cov] == 0).all()
    assert np.array_equal(got["albedo"], full["albedo"]) and np.array_equal(got["normal"], full["normal"])
    lin = _gbuffer(g, srgb=0)
    assert (lin["albedo"][cov] >= full["albedo"][cov]).all() and (lin["albedo"][cov] > full["albedo"][cov]).any()  # decode(x) <= x


@pytest.mark.parametrize("ss", [1, 2])
def test_null_normal_map_matches_the_vertex_gbuffer_on_an_affine_field(ss):
    """textures that hold the affine field (linear bytes; every texel the value at its point of the triangle) against
    gs2m_meshview_gbuffer with the field at the vertices: normal, view direction and coverage to the bit -- the same code --, the
    materials to the 8-bit quantisation, 1/255 per channel, on the samples whose taps are interior texels (a skirt texel holds
    the value of a point ON the triangle, not the field's continuation)."""
    c, k = T.plane_case(), T.FRAME
    verts, tris, a, tex = c["verts"], c["tris"], c["atlas"], c["tex"]
    H, W = a["height"], a["width"]
    field = T.affine_field(tex["points"].reshape(-1, 3)).astype(np.float32).reshape(H, W, 5)
    base, orm = T.pack(field, srgb=False)
    w2c = np.stack([T.R.look_at(e, [0.0, 0.0, 3.0]) for e in ([0.0, 0.0, 0.0], [0.8, 0.3, 0.2])])
    vis = MV.visibility(verts, tris, w2c, k["fx"], k["fy"], k["cx"], k["cy"], k["H"], k["W"], ss)
    keys = _cuda(NM.keys(vis))
    g = dict(verts=_cuda(verts, torch.float64), tris=_cuda(tris, torch.int32), uvs=_cuda(a["uvs"], torch.float32), w2c=_cuda(w2c), fx=k["fx"],
             fy=k["fy"], cx=k["cx"], cy=k["cy"], W=k["W"], H=k["H"], ss=ss, vis=keys, normals=None, tw=W, th=H, base=_cuda(base), srgb=0,
             orm=_cuda(orm), nm=None)
    got = _gbuffer(g)
    vf = T.affine_field(verts).astype(np.float32)
    ref = MVW.mesh_gbuffer(g["verts"], g["tris"], g["w2c"], k["fx"], k["fy"], k["cx"], k["cy"], k["H"], k["W"], keys.reshape(-1),
                           _cuda(vf[:, :3]), _cuda(vf[:, 3]), _cuda(vf[:, 4]), ss=ss)
    ref = {n: x.cpu().numpy() for n, x in ref.items()}
    assert np.array_equal(got["coverage"], ref["coverage"]) and np.array_equal(got["normal"], ref["normal"])
    assert np.array_equal(got["view_dir"], ref["view_dir"])
    want = NM.gbuffer_textured(verts, tris, a["uvs"], w2c, k["fx"], k["fy"], k["cx"], k["cy"], k["H"], k["W"], ss, vis, None, base, False, orm)
    cov = want["coverage"]
    _, taps, w = T.sample_bilinear(np.zeros((H, W, 1)), want["uv"][cov])
    inner = (tex["interior"][np.clip(taps[..., 0], 0, H - 1), np.clip(taps[..., 1], 0, W - 1)] | (w == 0)).all(1)
    assert cov.mean() > 0.2 and inner.mean() > 0.5
    tol = 1.0 / 255.0
    assert np.abs(got["albedo"][cov][inner] - ref["albedo"][cov][inner]).max() <= tol
    assert np.abs(got["roughness"][cov][inner] - ref["roughness"][..., 0][cov][inner]).max() <= tol
    assert np.abs(got["metallic"][cov][inner] - ref["metallic"][..., 0][cov][inner]).max() <= tol


def test_untrusted_keys_give_empty_samples():
    g = _gbuffer_case(1)
    good = _gbuffer(g)
    keys = g["vis"].clone()
    flat = keys.view(-1)
    covered = torch.nonzero(flat != -1).reshape(-1)
    i, j = int(covered[0]), int(covered[len(covered) // 2])
    flat[i] = (flat[i] & ~0xFFFFFFFF) | len(g["tris"])            # a triangle index that is not below n_tris
    flat[j] = (flat[j] & ~0xFFFFFFFF) | 0x7FFFFFFF
    tris = g["tris"].clone()
    t = int(flat[covered[-1]] & 0xFFFFFFFF)
    tris[t, 1] = len(g["verts"])                                    # a triangle that names a vertex out of range
    got = _gbuffer(g, vis=keys, tris=tris)
    dropped = np.zeros(good["coverage"].size, bool)
    dropped[[i, j]] = True
    dropped |= (NM.sphere_visibility(1)["tri"].reshape(-1) == t)
    dropped = dropped.reshape(good["coverage"].shape)
    assert dropped.sum() > 2
    for k in NAMES:
        assert (got[k][dropped] == 0).all() and np.array_equal(got[k][~dropped], good[k][~dropped]), k


# ---- the closed loop -----------------------------------------------------------------------------------------------------------

def _draw(tex, w2c, k, ss, smooth=True, keys=None):
    m = _cuda(w2c)
    vis = MVW.visibility_buffer(tex["vertices"], tex["triangles"], m, k["fx"], k["fy"], k["cx"], k["cy"], k["H"], k["W"], ss) if keys is None else keys
    g = MVW.mesh_gbuffer_textured(tex["vertices"], tex["triangles"], tex["uvs"], m, k["fx"], k["fy"], k["cx"], k["cy"], k["H"], k["W"], vis.reshape(-1),
                                  tex["base_color"], tex["orm"], tex["normal_map"], True, ss, tex["normals"] if smooth else None)
    return {n: x.cpu().numpy() for n, x in g.items()}


def test_closed_loop_on_a_flat_quad(tmp_path):
    """a constant world normal, 30 degrees off the face normal, baked from two views onto a two-triangle quad, written, read back
    and drawn: every covered sample's normal is within the quantisation bound of the baked one (the field is constant in tangent
    space, so the bilinear mixing adds nothing)"""
    k = T.FRAME
    verts, tris = MV.quad(z=2.0, half=0.5)
    tris = tris[:, [0, 2, 1]]                                       # wound towards the cameras below: the face normal is -z
    a = MT.build_atlas(_mesh(verts, tris), density=24.0)
    tilt = np.radians(30.0)
    n = np.array([np.sin(tilt) * 0.6, np.sin(tilt) * 0.8, -np.cos(tilt)])
    w2c = np.stack([T.R.look_at(e, [0.0, 0.0, 2.0]) for e in ([0.0, 0.0, 0.0], [0.4, -0.3, 0.2])])
    maps = np.zeros((2, 8, k["H"], k["W"]), np.float32)
    maps[:, :5] = np.float32([0.8, 0.5, 0.3, 0.6, 0.1])[:, None, None]
    maps[:, 5:] = n.astype(np.float32)[:, None, None]
    att = np.tile(maps[0, :, 0, 0], (len(verts), 1))               # (the quad's border fails the depth test: it reads the vertices)
    values, seen, _ = MT.bake_texel_attributes(a, _cuda(w2c), k["fx"], k["fy"], k["cx"], k["cy"], _cuda(maps), attributes=_cuda(att))
    owner = MT.atlas_texels(a)[0] >= 0
    assert seen[owner].float().mean() > 0.8
    base, orm = MT.pack_textures(values)
    nm = MT.pack_normal_map(a, values)
    own_id, px = MT.atlas_texels(a)[0].cpu().numpy(), nm.cpu().numpy().astype(int)
    for t in (0, 1):  # constant in the tangent space of each triangle, up to the last place of m
        assert np.ptp(px[own_id == t], axis=0).max() <= 1 and (px[own_id == t] != FLAT).any()
    MT.export_glb(tmp_path / "quad.glb", a, base, orm, normal_map=nm)
    tex = MVW.read_textured_mesh(tmp_path / "quad.glb", "cuda")
    assert torch.equal(tex["normal_map"], nm) and torch.equal(tex["base_color"], base) and torch.equal(tex["orm"], orm)
    for ss in (1, 2):
        for smooth in (True, False):
            g = _draw(tex, w2c, k, ss, smooth)
            cov = g["coverage"].astype(bool)
            assert cov.mean() > 0.1
            got = g["normal"][cov].astype(np.float64)
            angle = np.arccos(np.clip(got @ (n / np.linalg.norm(n)), -1.0, 1.0))
            assert angle.max() <= NM.QUANT_ANGLE + 1e-6, (ss, smooth)             # (+ the fp32 rounding of the output)
            assert np.abs(g["albedo"][cov] - [0.8, 0.5, 0.3]).max() <= 1.5 / 255.0  # sRGB bytes of a constant
    # the tangents: unit, perpendicular to the normals, w = -1, and along +u of the chart
    g = MT.read_glb(tmp_path / "quad.glb")
    tan = g["tangents"].astype(np.float64)
    assert (tan[:, 3] == -1).all() and np.abs(np.linalg.norm(tan[:, :3], axis=1) - 1.0).max() <= 1e-6
    assert np.abs((tan[:, :3] * g["normals"]).sum(1)).max() <= 1e-6
    p, uv = g["positions"].astype(np.float64).reshape(-1, 3, 3), g["uvs"].astype(np.float64).reshape(-1, 3, 2)
    F = NM.frame(p[:, 0], p[:, 1], p[:, 2], uv, g["normals"].astype(np.float64).reshape(-1, 3, 3)[:, 0])
    assert np.abs(tan[0::3, :3] - F["T"]).max() <= 1e-6


def test_closed_loop_on_the_icosphere(tmp_path):
    """the analytic field of mesh_normalmap_ref.scene("sphere") as the resolved values of a bake, packed on the device, written,
    read back and drawn from the restatement's keys: the device's bytes are the restatement's outside its band, and the drawn
    G-buffer is the restatement's decode of the file's arrays to 1 ulp, as in the G-buffer test"""
    c, s = T.sphere_case(), NM.scene("sphere")
    k = {n: c[n] for n in ("fx", "fy", "cx", "cy", "H", "W")}
    a = MT.build_atlas(_mesh(c["verts"], c["tris"]), density=c["density"])
    values = _cuda(s["values"]).reshape(a.height, a.width, 8)
    nm, tan = MT.pack_normal_map(a, values, return_tangent=True)
    want = s["want"]
    assert _close(tan.cpu().numpy().reshape(-1, 3), want["tangent"], 1e-12)
    got = nm.cpu().numpy().reshape(-1, 3)
    assert np.array_equal(got[~want["band"]], want["bytes"][~want["band"]])
    base, orm = MT.pack_textures(values)
    MT.export_glb(tmp_path / "sphere.glb", a, base, orm, normal_map=nm, device_png=True)
    tex = MVW.read_textured_mesh(tmp_path / "sphere.glb", "cuda")
    assert torch.equal(tex["normal_map"], nm)
    h = {n: (x.cpu().numpy() if x is not None else None) for n, x in tex.items()}
    w2c = c["w2c"][1:2]
    for ss in (1, 2):
        vis = MV.visibility(h["vertices"], h["triangles"], w2c, k["fx"], k["fy"], k["cx"], k["cy"], k["H"], k["W"], ss)
        ref = NM.gbuffer_textured(h["vertices"], h["triangles"], h["uvs"], w2c, k["fx"], k["fy"], k["cx"], k["cy"], k["H"], k["W"], ss, vis,
                                  h["normals"], h["base_color"], True, h["orm"], h["normal_map"])
        g = _draw(tex, w2c, k, ss, keys=_cuda(NM.keys(vis)))
        assert np.array_equal(g["coverage"].astype(bool), ref["coverage"]) and ref["coverage"].mean() > 0.1
        assert _ulps(g["normal"], ref["normal"]).max() <= 1.0 and _ulps(g["albedo"], ref["albedo"]).max() <= 1.0
        assert _ulps(g["roughness"][..., 0], ref["roughness"]).max() <= 1.0 and _ulps(g["metallic"][..., 0], ref["metallic"]).max() <= 1.0
        # and the device's own visibility draws the same picture but for samples the two rasterizers may settle differently
        own = _draw(tex, w2c, k, ss)
        same = ~vis["undecided"]
        assert np.array_equal(own["coverage"].astype(bool)[same], ref["coverage"][same])


# ---- the command lines ---------------------------------------------------------------------------------------------------------

def test_texture_and_view_command_lines(tmp_path):
    import gs2m_envmap as E
    import gs2m_mesh as M
    import gs2m_train as Tr
    from PIL import Image
    W, H = 48, 32
    scene = tmp_path / "scene"
    Tr.export_colmap_dataset(str(scene), Tr.synthetic_scene(2000, 3, W, H, seed=1))
    ply = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_small.ply")
    verts, tris = B.icosahedron()
    verts = 0.8 * verts + np.array([0.0, -0.8, 6.0])  # where the scene's cameras look
    M.write_mesh(tmp_path / "mesh.ply", types.SimpleNamespace(vertices=verts, triangles=tris, vertex_colors=np.full((12, 3), 0.25)))
    common = ["--ply", ply, "-s", str(scene), "--mesh", str(tmp_path / "mesh.ply"), "--texture-size", "128"]
    plain = MT.main(common + ["-o", str(tmp_path / "plain.glb"), "--metallic"])
    r = MT.main(common + ["-o", str(tmp_path / "nm.glb"), "--metallic", "--normal-map", "--textures-dir", str(tmp_path / "tex")])
    assert (r["width"], r["height"], r["n_seen"]) == (plain["width"], plain["height"], plain["n_seen"]) and r["n_seen"] > 0
    g0, g = MT.read_glb(tmp_path / "plain.glb"), MT.read_glb(tmp_path / "nm.glb")
    assert g0["tangents"] is None and g0["normal_image"] is None and "normalTexture" not in g0["json"]["materials"][0]
    assert g["tangents"].shape == (60, 4) and (g["tangents"][:, 3] == -1).all()
    assert g["json"]["materials"][0]["normalTexture"] == {"index": 2} and g["json"]["meshes"][0]["primitives"][0]["attributes"]["TANGENT"] == 4
    assert g["images"] == g0["images"] and g["positions"].tobytes() == g0["positions"].tobytes()  # the materials keep their bits
    px = MT.decode_png(g["normal_image"])
    assert px.shape == (r["height"], r["width"], 3) and (px[..., 2] >= 128).all() and (px != FLAT).any()
    assert sorted(os.listdir(tmp_path / "tex")) == ["base_color.png", "metallic_roughness.png", "normal.png"]
    assert (tmp_path / "tex" / "normal.png").read_bytes() == g["normal_image"]
    r3 = MT.main(common + ["-o", str(tmp_path / "rgb.glb"), "--rgb", "--normal-map"])
    g3 = MT.read_glb(tmp_path / "rgb.glb")
    assert len(g3["images"]) == 1 and g3["normal_image"] is not None and g3["json"]["materials"][0]["normalTexture"] == {"index": 1}
    assert r3["width"] == r["width"]
    # the viewer draws the file in both colour modes
    res = MVW.main(["--glb", str(tmp_path / "nm.glb"), "-s", str(scene), "--out-dir", str(tmp_path / "tex_views"), "--rendering", "--colour", "texture",
                    "--shading", "smooth"])
    assert len(res["views"]) == 3
    images = [np.asarray(Image.open(p)) for p in res["views"]]
    for im in images:
        assert im.shape == (H, W, 4) and (im[..., 3] == 255).any() and (im[..., 3] == 0).any() and im[im[..., 3] == 255][:, :3].max() > 0
    flat = MVW.main(["--glb", str(tmp_path / "plain.glb"), "-s", str(scene), "--out-dir", str(tmp_path / "plain_views"), "--rendering", "--colour", "texture",
                     "--shading", "smooth"])
    other = [np.asarray(Image.open(p)) for p in flat["views"]]
    assert all(np.array_equal(x[..., 3], y[..., 3]) for x, y in zip(images, other)) and any(not np.array_equal(x, y) for x, y in zip(images, other))
    light = E.EnvLight((0.2 + torch.rand((6, 64, 64, 3), generator=torch.Generator().manual_seed(2))).cuda())
    hdr = E.save_light_hdr(light, str(tmp_path / "tiny.hdr"), res=(16, 32))
    res = MVW.main(["--glb", str(tmp_path / "nm.glb"), "-s", str(scene), "--out-dir", str(tmp_path / "pbr_views"), "--rendering", "--colour", "pbr",
                    "--envmap", hdr, "--env-res", "64", "--env-samples", "2", "--gamma"])
    assert len(res["views"]) == 3
    for p in res["views"]:
        im = np.asarray(Image.open(p))
        assert im.shape == (H, W, 4) and (im[..., 3] == 255).any() and im[im[..., 3] == 255][:, :3].max() > 0
    with pytest.raises(RuntimeError, match="--glb"):
        MVW.main(["--ply-path", str(tmp_path / "mesh.ply"), "-s", str(scene), "--out-dir", str(tmp_path / "x"), "--rendering", "--colour", "texture"])
    with pytest.raises(RuntimeError, match="--colour texture or --colour pbr"):
        MVW.main(["--glb", str(tmp_path / "nm.glb"), "-s", str(scene), "--out-dir", str(tmp_path / "x"), "--rendering"])


def test_mesh_command_line_takes_normal_map(tmp_path):
    """gs2m_mesh.py --texture-size 256 with and without --normal-map: without it tsdf_textured.glb has neither tangents nor a normal
    texture; with it the file holds the same mesh and the same material images, and the two new things"""
    import gs2m_mesh as M
    import gs2m_train as Tr
    import test_mesh_gpu as TM
    from gs2m_model import GaussianModel
    Tr.export_colmap_dataset(str(tmp_path / "scene"), Tr.synthetic_scene(8000, 4, 96, 64, seed=1))
    truth, _ = TM._truth_and_cams(8000, 1, 96, 64)
    model = GaussianModel(3)
    model.parameterize((truth._xyz, truth._features_dc, truth._features_rest, truth._scaling, truth._rotation, truth._opacity,
                        truth._albedo, truth._roughness, truth._metallic))
    model.active_sh_degree = 3
    model.save_ply(str(tmp_path / "model.ply"))
    # (voxels of 0.24: some 1400 triangles, 700 cells of side 8 at the least, which an atlas 256 wide holds; 0.16 makes 3000)
    base = ["--ply", str(tmp_path / "model.ply"), "-s", str(tmp_path / "scene"), "--voxel_size", "0.24", "--texture-size", "256"]
    M.main(base + ["-o", str(tmp_path / "tex")])
    M.main(base + ["-o", str(tmp_path / "nm"), "--normal-map"])
    g0, g = MT.read_glb(tmp_path / "tex" / "tsdf_textured.glb"), MT.read_glb(tmp_path / "nm" / "tsdf_textured.glb")
    assert g0["tangents"] is None and g0["normal_image"] is None
    assert g["tangents"] is not None and len(g["tangents"]) == len(g["positions"]) and g["normal_image"] is not None
    assert (tmp_path / "tex" / "config.json").read_bytes() == (tmp_path / "nm" / "config.json").read_bytes()
    assert len(g["positions"]) == len(g0["positions"]) and MT.decode_png(g["normal_image"]).shape[1] <= 256
    with pytest.raises(SystemExit):
        M.main(["--ply", str(tmp_path / "model.ply"), "-s", str(tmp_path / "scene"), "-o", str(tmp_path / "x"), "--normal-map"])
