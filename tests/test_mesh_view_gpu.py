"""csrc/mesh_view.hip through gs2m_mesh_view.py against the float64 restatement tests/mesh_view_ref.py: the
visibility buffer against the depth rasterizer bit for bit and against the restatement sample by sample on every path (a lane, a
wave, a row of workgroups), index ties, launch-order independence, refused arguments; the shaded bytes pixel by pixel in every
mode; the vertex normal sums; batching; the command line end to end.  All data is synthetic."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mesh_view_ref as V  # noqa: E402
import tnt_cull_ref as R  # noqa: E402
import gs2m_mesh_cull as K  # noqa: E402
import gs2m_mesh_view as G  # noqa: E402  (fails here on a tree without the feature)
import gs2m_native as N  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(n, ss) for n, c in sorted(V.view_cases().items()) for ss in c["ss"]]


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


def _k(c):
    return c["fx"], c["fy"], c["cx"], c["cy"], c["H"], c["W"]


def _vis(c, ss=1, tris=None, views=None):
    """-> (high words (n, H ss, W ss) uint32, low words uint32)"""
    w2c = c["w2c"] if views is None else c["w2c"][views]
    b = G.visibility_buffer(_dev(c["verts"], torch.float64), _dev(c["tris"] if tris is None else tris, torch.int32), _dev(w2c, torch.float64),
                            *_k(c), ss=ss, near=c["near"], far=c["far"])
    assert b.dtype == torch.int64 and tuple(b.shape) == (len(w2c), c["H"] * ss, c["W"] * ss)
    u = b.cpu().numpy().view(np.uint64)
    return (u >> np.uint64(32)).astype(np.uint32), (u & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _shade(c, ss, shading="flat", colour="grey", srgb=True, **kw):
    return G.shade_views(_dev(c["verts"], torch.float64), _dev(c["tris"], torch.int32), _dev(c["w2c"], torch.float64), *_k(c), ss=ss,
                         shading=shading, colors=_dev(c["colors"], torch.float32) if colour == "vertex" else None, srgb=srgb,
                         near=c["near"], far=c["far"], **kw)


@pytest.mark.parametrize("name", sorted(R.depth_cases()))
def test_high_words_are_the_depth_image(name):
    """ss = 1: every pixel, no exception; an empty key is all ones"""
    c = R.depth_cases()[name]
    hi, lo = _vis(c)
    depth = K.render_mesh_depth(_dev(c["verts"], torch.float64), _dev(c["tris"], torch.int32), _dev(c["w2c"], torch.float64), *_k(c),
                                c["near"], c["far"]).cpu().numpy().view(np.uint32)
    empty = hi == 0xFFFFFFFF
    assert np.array_equal(np.where(empty, 0, hi), depth) and np.array_equal(empty, depth == 0)
    assert (lo[empty] == 0xFFFFFFFF).all() and (lo[~empty] < len(c["tris"])).all()


@pytest.mark.parametrize("name,ss", CASES)
def test_keys_match_the_restatement(name, ss):
    """decided samples: the z bits and the triangle index; everywhere: the index is a triangle that reaches that z there"""
    c = V.view_cases()[name]
    ref = V.reference_visibility(name, ss)
    hi, lo = _vis(c, ss)
    ok = ~ref["undecided"]
    print(name, ss, "samples", hi.size, "covered", int((ref["tri"] >= 0).sum()), "undecided", int(ref["undecided"].sum()))
    assert np.array_equal(hi[ok], ref["zbits"][ok])
    assert np.array_equal(np.where(hi == 0xFFFFFFFF, -1, lo.astype(np.int64))[ok], ref["tri"][ok])


def test_index_ties_go_to_the_lowest_index():
    c = V.duplicates_case()
    ref = V.visibility(c["verts"], c["tris"], c["w2c"], *_k(c), 1)
    hi, lo = _vis(c)
    tied = ref["tri"] == 1  # the duplicates 1 and 3 are the nearest surface there, at the same z exactly
    assert tied.sum() > 100 and (lo[tied] == 1).all() and np.array_equal(hi[tied], ref["zbits"][tied])
    assert not (lo == 3).any()
    # the list reversed: the duplicates are now 0 and 2, the lower wins again
    hi2, lo2 = _vis(c, tris=c["tris"][::-1])
    assert (lo2[tied] == 0).all() and np.array_equal(hi2, hi)
    for s in (2, 3):
        assert not (_vis(c, ss=s)[1] == 3).any()


@pytest.mark.parametrize("name,ss", [("soup_37x29", 3), ("soup_big", 1), ("mesh3", 2), ("mesh3", 4), ("fill_96x80", 2), ("crossing", 2)])
def test_keys_do_not_depend_on_the_launch_order(name, ss):
    c = V.view_cases()[name]
    hi, lo = _vis(c, ss)
    again = _vis(c, ss)
    assert np.array_equal(hi, again[0]) and np.array_equal(lo, again[1])
    perm = np.random.default_rng(1).permutation(len(c["tris"]))
    hp, lp = _vis(c, ss, tris=c["tris"][perm])  # triangle k of the permuted list is triangle perm[k]
    back = np.where(hp == 0xFFFFFFFF, 0xFFFFFFFF, perm[np.minimum(lp, len(perm) - 1)]).astype(np.uint32)
    und = V.reference_visibility(name, ss)["undecided"]  # (an exact z tie between two triangles may map back to the other one)
    assert np.array_equal(hp, hi) and np.array_equal(back[~und], lo[~und])
    for k in range(len(c["w2c"])):  # the views of a batch are the views alone
        one = _vis(c, ss, views=[k])
        assert np.array_equal(one[0][0], hi[k]) and np.array_equal(one[1][0], lo[k])


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("mode", [("flat", "grey", True), ("smooth", "vertex", True), ("smooth", "grey", False), ("flat", "vertex", False)])
@pytest.mark.parametrize("name,ss", CASES)
def test_shaded_views_match_the_restatement(name, ss, mode):
    """decided pixels: the four bytes (a loose byte within 1), the triangle index, the depth within 1 fp32 ulp"""
    c = V.view_cases()[name]
    ref = V.reference(name, ss, *mode)
    rgba, depth, tri = (x.cpu().numpy() for x in _shade(c, ss, *mode, return_aux=True))
    assert rgba.dtype == np.uint8 and rgba.shape == ref["rgba"].shape and depth.dtype == np.float32 and tri.dtype == np.int32
    ok = ~ref["undecided"]
    diff = np.abs(rgba.astype(np.int64) - ref["rgba"])[ok]
    loose = ref["loose"][ok]
    print(name, ss, mode, "pixels", ok.size, "undecided", int((~ok).sum()), "bytes off by one", int((diff == 1).sum()), "loose", int(loose.sum()),
          "largest difference", int(diff.max(initial=0)))
    assert (diff[~loose] == 0).all() and (diff[loose] <= 1).all()
    assert np.array_equal(tri[ok], ref["tri_id"][ok])
    assert np.array_equal((depth > 0)[ok], (ref["depth"] > 0)[ok]) and (_ulps(depth, ref["depth"])[ok] <= 1).all()


def test_vertex_normal_sums():
    for name in ("mesh3", "soup_big", "rejected_among_good"):
        c = V.view_cases()[name]
        want, deg, _ = V.vertex_normal_sums(c["verts"], c["tris"])
        v, f = _dev(c["verts"], torch.float64), _dev(c["tris"], torch.int32)
        normals, sums = G.vertex_normals(v, f)
        assert sums.dtype == torch.int64 and normals.dtype == torch.float64
        got = sums.cpu().numpy()
        print(name, "largest difference of a sum", int(np.abs(got - want).max()), "largest degree", int(deg.max()))
        assert (np.abs(got - want) <= deg[:, None]).all()
        assert torch.equal(G.vertex_normals(v, f)[1], sums) and torch.equal(G.vertex_normals(v, _dev(c["tris"][::-1], torch.int32))[1], sums)
        s = got.astype(np.float64)
        with np.errstate(all="ignore"):
            unit = np.where((got != 0).any(1)[:, None], s / np.sqrt(((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]))[:, None], 0.0)
        assert np.allclose(normals.cpu().numpy(), unit, rtol=0, atol=4e-16)
    v, t, axes = V.cube()
    got = G.vertex_normals(_dev(v, torch.float64), _dev(t, torch.int32))[1].cpu().numpy()
    assert np.array_equal(got, V.vertex_normal_sums(v, t)[0]), "axis-aligned faces: exact"


def test_bad_arguments_are_refused():
    c = V.view_cases()["mesh3"]
    v, m = _dev(c["verts"], torch.float64), _dev(c["w2c"], torch.float64)
    for bad in (len(c["verts"]), -1, 2 ** 31 - 1):
        t = c["tris"].copy()
        t[len(t) // 2, 1] = bad
        with pytest.raises(RuntimeError, match="invalid argument"):
            G.visibility_buffer(v, _dev(t, torch.int32), m, *_k(c))
        with pytest.raises(RuntimeError, match="invalid argument"):
            G.vertex_normals(v, _dev(t, torch.int32))
    torch.cuda.synchronize()  # nothing is left behind: the next call is served
    hi, _ = _vis(c)
    ref = V.reference_visibility("mesh3", 1)
    assert np.array_equal(hi[~ref["undecided"]], ref["zbits"][~ref["undecided"]])
    f = _dev(c["tris"], torch.int32)
    for ss in (0, 5):
        with pytest.raises(RuntimeError, match="invalid argument"):
            G.visibility_buffer(v, f, m, *_k(c), ss=ss)
        with pytest.raises(RuntimeError, match="invalid argument"):
            G.shade_views(v, f, m, *_k(c), ss=ss)
    with pytest.raises(RuntimeError, match="invalid argument"):  # W ss * H ss = 2^31 > 2^31 - 1
        G.visibility_buffer(v, f, m[:1], c["fx"], c["fy"], c["cx"], c["cy"], 2 ** 14, 2 ** 15, ss=2)
    # the library itself refuses them before it touches a buffer
    ws, one = torch.empty(4096, dtype=torch.uint8, device="cuda"), torch.empty(16, dtype=torch.int64, device="cuda")
    fn = N.lib().gs2m_meshview_visibility
    for W, H, ss in ((41, 33, 0), (41, 33, 5), (2 ** 15, 2 ** 14, 2), (46341, 46341, 1)):
        rc = fn(len(v), v.data_ptr(), len(f), f.data_ptr(), 1, m.data_ptr(), c["fx"], c["fy"], c["cx"], c["cy"], W, H, ss, 0.01, 20.0,
                ws.data_ptr(), one.data_ptr(), None)
        assert rc == -1, (W, H, ss, rc)
    assert fn(len(v), v.data_ptr(), 2 ** 32 - 1, f.data_ptr(), 1, m.data_ptr(), c["fx"], c["fy"], c["cx"], c["cy"], 4, 4, 1, 0.01, 20.0,
              ws.data_ptr(), one.data_ptr(), None) == -1
    with pytest.raises(RuntimeError, match="no CPU path"):
        G.shade_views(torch.zeros(3, 3, dtype=torch.float64), f, m, *_k(c))
    with pytest.raises(RuntimeError, match="no CPU path"):
        G.vertex_normals(v, torch.zeros(1, 3, dtype=torch.int32))


def test_view_batches_give_the_same_bytes():
    c = V.view_cases()["mesh3"]
    whole = _shade(c, 2, "smooth", "vertex", return_aux=True)
    for batch in (1, 2):
        part = _shade(c, 2, "smooth", "vertex", return_aux=True, view_batch=batch)
        assert all(torch.equal(a, b) for a, b in zip(whole, part)), batch
    assert not torch.equal(whole[0][0], whole[0][1])
    none = G.shade_views(_dev(c["verts"], torch.float64), _dev(c["tris"], torch.int32), torch.zeros((0, 4, 4), dtype=torch.float64, device="cuda"), *_k(c))
    assert tuple(none.shape) == (0, c["H"], c["W"], 4)


def test_command_line(tmp_path):
    import gs2m_mesh as M
    from PIL import Image
    v, t, records = V.cli_mesh()
    ints = np.random.default_rng(2).integers(0, 256, (len(v), 3))
    col, col32 = ints / 255.0, ints.astype(np.float32) / 255.0  # as written, and as read_mesh gives them back
    mesh_dir = tmp_path / "mesh"
    mesh_dir.mkdir()
    M.write_mesh(mesh_dir / "tsdf_post.ply", types.SimpleNamespace(vertices=v, triangles=t, vertex_colors=col))
    (tmp_path / "cameras.json").write_text(json.dumps(records))
    common = ["--ply-path", str(mesh_dir / "tsdf_post.ply"), "--cameras", str(tmp_path / "cameras.json")]
    r = G.main(common + ["--rendering", "--shading", "smooth", "--colour", "vertex"])
    assert r["out_dir"] == str(tmp_path / "visual") and [os.path.basename(p) for p in r["views"]] == [f"view_{k:02d}.png" for k in range(4)]
    views = G.read_cameras_json(tmp_path / "cameras.json")
    want = G.shade_views(_dev(v, torch.float64), _dev(t, torch.int32), _dev(np.stack([x["w2c"] for x in views]), torch.float64), 43.7, 44.1, 20.0, 15.0,
                         30, 40, ss=2, shading="smooth", colors=_dev(col32, torch.float32)).cpu().numpy()
    assert (want[..., 3] == 255).any() and (want[..., 3] == 0).any()
    for k, p in enumerate(r["views"]):
        im = Image.open(p)
        assert im.mode == "RGBA" and im.size == (40, 30) and np.array_equal(np.asarray(im), want[k]), p
    one = G.main(common + ["--rendering", "--render_view_idx", "2", "-r", "2", "--out-dir", str(tmp_path / "half")])
    assert [os.path.basename(p) for p in one["views"]] == ["view_02.png"] and Image.open(one["views"][0]).size == (20, 15)
    r = G.main(common + ["--animation", "--ss", "1", "--frames", "6", "--view-idx", "1", "--shift", "0.05", "0", "-0.02"])
    assert [os.path.basename(p) for p in r["frames"]] == [f"{k:03d}.png" for k in range(6)] and all(os.path.exists(p) for p in r["frames"])
    k = dict(fx=43.7 * 600 / 40, fy=44.1 * 600 / 30, cx=300.0, cy=300.0)
    frames = G.shade_views(_dev(v, torch.float64), _dev(t, torch.int32), _dev(G.turntable(views[1]["w2c"], 6, (0.05, 0.0, -0.02)), torch.float64),
                           k["fx"], k["fy"], k["cx"], k["cy"], 600, 600, ss=1).cpu().numpy()
    assert np.array_equal(np.asarray(Image.open(r["frames"][4])), frames[4]) and not np.array_equal(frames[4], frames[0])
    gif = Image.open(r["gif"])
    # (1000 // 24 ms in the format's hundredths of a second)
    assert gif.n_frames == 6 and gif.size == (600, 600) and gif.info["duration"] == 40 and gif.info.get("loop") == 0
    assert "transparency" in gif.info
    assert (r["webp"] is not None) == os.path.exists(tmp_path / "visual" / "anim.webp")
    r = G.main(common + ["--still"])
    still = Image.open(r["still"])
    assert os.path.basename(r["still"]) == "still.png" and still.mode == "RGBA" and still.size == (600, 600)
    assert (np.asarray(still)[..., 3] == 255).any()
