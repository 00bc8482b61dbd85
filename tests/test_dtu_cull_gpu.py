"""The mask culling of the DTU evaluation on the GPU (csrc/mesh_cull.hip) against the restatement (tests/dtu_cull_ref.py):
the dilation bit for bit against scipy, the vertex flags exactly on every decided vertex, the culled mesh element for element,
and --mask_cull through the command line."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gs-2m_amd"))
import dtu_cull_ref as R  # noqa: E402
import gs2m_dtu_eval as E  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 5), (49, 49), (60, 100), (130, 70), (64, 64), (65, 129)]


def _masks_for(H, W, seed):
    """the mask kinds of one size: empty, full, single pixels at the corners and the centre, sparse, dense, mixed values"""
    rng = np.random.default_rng(seed)
    ms = [np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)]
    for y, x in {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)}:
        m = np.zeros((H, W), np.uint8)
        m[y, x] = 1
        ms.append(m)
    ms.append((rng.random((H, W)) < 0.01).astype(np.uint8) * 255)
    ms.append((rng.random((H, W)) < 0.5).astype(np.uint8) * 255)
    ms.append((rng.random((H, W)) < 0.03).astype(np.uint8) * rng.choice(np.array([1, 128, 255], np.uint8), (H, W)))
    return ms


def _check_dilation(masks, r):
    d = E.dilate_masks(masks, r)
    ref = np.stack([R.dilate(m, r) for m in masks])
    assert np.array_equal(d.unpack(), ref)
    # the packed words themselves, padding bits included
    assert np.array_equal(d.packed.cpu().numpy().view(np.uint64), R.pack_rows(ref))


@pytest.mark.parametrize("r", [0, 1, 2, 24])
@pytest.mark.parametrize("H,W", SIZES)
def test_dilation_bit_for_bit(H, W, r):
    _check_dilation(_masks_for(H, W, 100 * H + W), r)  # one batched call: the views must not leak into each other either


def test_dilation_batch_of_three_and_other_radii():
    rng = np.random.default_rng(3)
    masks = [(rng.random((130, 70)) < p).astype(np.uint8) for p in (0.002, 0.02, 0.0005)]
    for r in (24, 7, 64):
        _check_dilation(masks, r)
        for k in range(3):  # each alone gives what it gives in the batch
            assert np.array_equal(E.dilate_masks(masks[k:k + 1], r).unpack()[0], R.dilate(masks[k], r))
    t = torch.as_tensor(np.stack(masks)).cuda()
    assert np.array_equal(E.dilate_masks(t, 24).unpack(), E.dilate_masks(masks, 24).unpack())
    assert len(E.dilate_masks(np.zeros((0, 5, 5), np.uint8))) == 0


def test_dilation_full_size():
    rng = np.random.default_rng(4)
    m = R.ellipse_mask(1200, 1600).copy()
    m[rng.integers(0, 1200, 300), rng.integers(0, 1600, 300)] = 1  # and speckles, some of them at the border
    m[0, 0] = m[1199, 1599] = 1
    _check_dilation([m], 24)


@pytest.mark.parametrize("r", [65, -1])
def test_dilation_refuses_a_radius_out_of_range(r):
    with pytest.raises(RuntimeError, match="invalid argument"):
        E.dilate_masks([np.ones((8, 8), np.uint8)], r)


def _check_flags(c):
    keep = E.cull_flags(c["vertices"], c["M"], E.dilate_masks(c["masks"], c["radius"]), c["image_size"]).cpu().numpy().astype(bool)
    d = ~c["undecided"]
    wrong = np.nonzero(keep[d] != c["keep"][d])[0]
    assert len(wrong) == 0, (len(wrong), wrong[:10])
    return keep


@pytest.mark.parametrize("n_views,n_verts", R.VERTEX_CASES)
def test_vertex_flags(n_views, n_verts):
    c = R.vertex_case(n_views, n_verts)
    assert int(c["undecided"].sum()) <= R.UNDECIDED_CAP * n_verts  # from the restatement alone
    keep = _check_flags(c)
    nan = np.isnan(c["vertices"]).any(axis=1)
    assert keep[nan].all()


def test_vertex_flags_mask_smaller_than_the_normaliser():
    c = R.small_mask_case()
    assert c["masks"].shape[1:] == (75, 100) and c["image_size"] == (200, 150)
    assert int(c["undecided"].sum()) <= R.UNDECIDED_CAP * len(c["vertices"])
    keep = _check_flags(c)
    assert 0 < int(keep.sum()) < len(keep)


def test_no_views_keep_everything():
    v = R.vertex_case(1, 1000)["vertices"]
    keep = E.cull_flags(v, np.zeros((0, 4, 4), np.float32), E.dilate_masks(np.zeros((0, 3, 3), np.uint8)))
    assert keep.cpu().numpy().all()
    cv, ct = E.cull_mesh(v, R.random_mesh(1000, 500, 0), np.zeros((0, 4, 4), np.float32), np.zeros((0, 3, 3), np.uint8))
    assert np.array_equal(cv.cpu().numpy(), v, equal_nan=True) and np.array_equal(ct.cpu().numpy(), R.random_mesh(1000, 500, 0))


def test_culled_mesh_is_exact():
    c, v, t, cv, ct = R.decided_mesh(3, 2000, 3000, 7)
    gv, gt = E.cull_mesh(v, t, c["M"], c["masks"], c["radius"], c["image_size"])
    assert gv.dtype == torch.float64 and gt.dtype == torch.int32 and gv.is_cuda and gt.is_cuda
    assert np.array_equal(gv.cpu().numpy(), cv, equal_nan=True)
    assert np.array_equal(gt.cpu().numpy(), ct)
    assert (t[:, 0] == t[:, 1]).sum() >= 1 and (ct[:, 0] == ct[:, 1]).sum() >= 1  # the degenerate face on kept vertices survives
    assert len(np.setdiff1d(np.arange(len(cv)), ct)) > 0  # kept vertices that no face names are still there
    # empty meshes
    ev, et = E.cull_mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int32), c["M"], c["masks"], c["radius"], c["image_size"])
    assert ev.shape == (0, 3) and et.shape == (0, 3)
    ev, et = E.cull_mesh(v, np.zeros((0, 3), np.int32), c["M"], c["masks"], c["radius"], c["image_size"])
    assert np.array_equal(ev.cpu().numpy(), cv, equal_nan=True) and et.shape == (0, 3)


@pytest.mark.parametrize("bad", [-1, 2000])
def test_triangle_id_out_of_range_is_refused(bad):
    keep = torch.ones(2000, dtype=torch.uint8, device="cuda")
    t = R.random_mesh(2000, 300, 1)
    t[17, 2] = bad
    with pytest.raises(RuntimeError, match="invalid argument"):
        E.cull_triangles(keep, t)


def test_two_runs_are_bitwise_equal():
    c, v, t, _, _ = R.decided_mesh(3, 2000, 3000, 7)
    a = E.cull_mesh(v, t, c["M"], c["masks"], c["radius"], c["image_size"])
    b = E.cull_mesh(v, t, c["M"], c["masks"], c["radius"], c["image_size"])
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1], b[1])
    big = R.vertex_case(49, 100000)
    d = E.dilate_masks(big["masks"], 24)
    k1, k2 = E.cull_flags(big["vertices"], big["M"], d, big["image_size"]), E.cull_flags(big["vertices"], big["M"], d, big["image_size"])
    assert torch.equal(k1, k2) and torch.equal(d.packed, E.dilate_masks(big["masks"], 24).packed)


# ---- the command line --------------------------------------------------------------------------------------------------------

def _scan_folder(tmp_path, c):
    """cameras.npz, images/, mask/ of the synthetic scan R.cli_case() and the DTU ground-truth files of its sphere"""
    from PIL import Image
    from scipy.io import savemat
    world, scales, n_views, scale, shift = c["world"], c["scales"], len(c["world"]), R.CLI_SCALE, R.CLI_SHIFT
    ref = tmp_path / "scan9"
    os.makedirs(ref / "images")
    os.makedirs(ref / "mask")
    np.savez(ref / "cameras.npz", **{f"world_mat_{k}": world[k] for k in range(n_views)},
             **{f"scale_mat_{k}": scales[k] for k in range(n_views)})
    for k in range(n_views):
        Image.fromarray(np.zeros((150, 200, 3), np.uint8)).save(ref / "images" / f"{k:04}.png")
        m = c["masks"][k]
        Image.fromarray(np.stack([m // 2, m // 3, m], axis=-1)).save(ref / "mask" / f"{k:03}.png")  # the blue channel is the mask
    dtu = tmp_path / "dtu"
    os.makedirs(dtu / "ObsMask")
    os.makedirs(dtu / "Points" / "stl")
    k = np.arange(60_000) + 0.5
    phi, th = np.arccos(1 - 2 * k / len(k)), np.pi * (1 + 5 ** 0.5) * k
    stl = R.CLI_SPHERE * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1) * scale + np.asarray(shift)
    E.write_point_cloud(dtu / "Points" / "stl" / "stl009_total.ply", stl)
    bb = np.stack([stl.min(0) - 5, stl.max(0) + 5])
    res = 2.0
    savemat(str(dtu / "ObsMask" / "ObsMask9_10.mat"), {"ObsMask": np.ones(np.floor((bb[1] - bb[0]) / res).astype(int) + 1, np.uint8), "BB": bb,
                                                       "Res": np.array([[res]])})
    savemat(str(dtu / "ObsMask" / "Plane9.mat"), {"P": np.array([[0.0, 1.0, 0.0, 1000.0]])})
    return ref, dtu


def test_mask_cull_through_the_cli(tmp_path):
    import gs2m_mesh as Mh
    c = R.cli_case()
    ref, dtu = _scan_folder(tmp_path, c)
    scales = c["scales"]
    # the decided input: the sphere without the vertices the restatement cannot decide (and the faces that name them);
    # the reference's normaliser is the hard-coded (1600, 1200), which the command line uses too
    assert E.CULL_IMAGE_SIZE == c["image_size"] and E.CULL_RADIUS == c["radius"]
    v, t, keep, undecided = c["vertices"], c["triangles"], c["keep"], c["undecided"]
    assert int(undecided.sum()) <= R.UNDECIDED_CAP * len(v)
    v, t = R.cull_mesh(v, t, ~undecided)
    keep = keep[~undecided]
    Mh.write_mesh(tmp_path / "mesh.ply", Mh.TriangleMesh(v, t, np.zeros((len(v), 3))))
    cv, ct = R.cull_mesh(v, t, keep)
    assert 0 < len(cv) < len(v)
    out = tmp_path / "eval"
    args = ["--input_ply", str(tmp_path / "mesh.ply"), "--ref_dir", str(ref), "--dtu_dir", str(dtu), "--out_dir", str(out), "--no_vis"]
    r = E.main(args + ["--mask_cull"])
    j = json.load(open(out / "results.json"))
    assert j["mask_cull"] is True and j["n_vertices_culled"] == len(v) - len(cv) and j["n_triangles_culled"] == len(t) - len(ct)
    assert 0 < j["n_vertices"] < len(v) and j["n_vertices"] == len(cv) and "cull" in j["ms"]
    gt = E.load_dtu_ground_truth(str(dtu), 9)
    want = E.evaluate_mesh(cv, ct, gt["stl"], gt["obs_mask"], gt["bb"], gt["res"], gt["plane"], scale_mat=scales[0])
    for k in ("mean_d2s", "mean_s2d", "overall"):
        assert np.isfinite(want[k]) and abs(r[k] - want[k]) <= 1e-12 * abs(want[k]), (k, r[k], want[k])
        assert j[k] == r[k]
    # culled_mesh.ply: the culled mesh in world coordinates, float32 as the mesh writer stores them
    pv, pt = E.read_ply(out / "culled_mesh.ply")
    world_v = E.world_transform(cv, scales[0]).cpu().numpy()
    assert np.array_equal(pt, ct) and np.array_equal(pv, world_v.astype(np.float32).astype(np.float64))
    # without the flag: the unculled mesh, and no trace of the culling
    out2 = tmp_path / "eval2"
    r2 = E.main(args[:7] + [str(out2)] + args[8:])
    plain = E.evaluate_mesh(v, t, gt["stl"], gt["obs_mask"], gt["bb"], gt["res"], gt["plane"], scale_mat=scales[0])
    for k in ("mean_d2s", "mean_s2d", "overall"):
        assert r2[k] == plain[k]
    assert set(r2) == set(plain) | {"scan"} and "cull" not in r2["ms"] and not os.path.exists(out2 / "culled_mesh.ply")
    assert r2["n_vertices"] == len(v) and r2["mean_d2s"] != r["mean_d2s"]
