"""The Tanks and Temples clouds without a GPU: the committed colour table against matplotlib's hot_r, the point-cloud PLY
with normals, the unchanged PLY without, and the arbiter's own share of the GPU normal test (tests/tnt_clouds_ref.py)."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import tnt_clouds_ref as CR  # noqa: E402
import gs2m_eval_util as U  # noqa: E402
import gs2m_tnt_eval as E  # noqa: E402


def _committed_table():
    txt = open(os.path.join(ROOT, "gs-2m_amd", "csrc", "tnt_hot_r.h")).read()
    rows = re.findall(r"\{([^{}]+)\}", txt[txt.index("#define GS2M_HOT_R_TABLE"):])
    return np.array([[float(x) for x in r.split(",")] for r in rows], np.float64)


def test_committed_colour_table_is_hot_r():
    import matplotlib
    t = _committed_table()
    assert t.shape == (256, 3)
    want = matplotlib.colormaps["hot_r"](np.arange(256))[:, :3]
    assert np.array_equal(t, want)
    # the float lookup the kernel restates: trunc(x * 256), 256 -> 255
    x = np.concatenate([np.linspace(0, 1, 10001), np.arange(257) / 256.0, np.nextafter(np.arange(1, 257) / 256.0, 0)])
    assert np.array_equal(matplotlib.colormaps["hot_r"](x)[:, :3], t[np.minimum((x * 256).astype(np.int64), 255)])
    # no channel sits on a half: round-half-even (the kernel) and round-half-away (Open3D's std::round) store the same byte
    assert not np.any(np.abs(t * 255.0 - np.floor(t * 255.0) - 0.5) < 1e-9)


def test_point_cloud_with_normals_round_trips(tmp_path):
    rng = np.random.default_rng(0)
    p, n = rng.normal(size=(1000, 3)) * 50, rng.normal(size=(1000, 3))
    c = rng.integers(0, 256, (1000, 3)).astype(np.uint8)
    f = tmp_path / "cloud.ply"
    U.write_point_cloud(f, p, c / 255.0, normals=n)
    data = open(f, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    assert data[:end].decode("ascii").split("\n")[:-1] == [
        "ply", "format binary_little_endian 1.0", "comment Created by Open3D", "element vertex 1000", "property double x", "property double y",
        "property double z", "property double nx", "property double ny", "property double nz", "property uchar red", "property uchar green",
        "property uchar blue", "end_header"]
    verts, tris = U.read_ply(f)
    assert np.array_equal(verts, p) and len(tris) == 0
    a = np.frombuffer(data, np.dtype([(k, "<f8") for k in ("x", "y", "z", "nx", "ny", "nz")] + [(k, "u1") for k in ("red", "green", "blue")]), 1000, end)
    assert len(data) == end + 1000 * 51
    assert np.array_equal(np.stack([a["nx"], a["ny"], a["nz"]], 1), n)
    assert np.array_equal(np.stack([a["red"], a["green"], a["blue"]], 1), c)


def _todays_writer(file, points, colors=None):
    """write_point_cloud as it stood before it took normals, statement for statement"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    a = np.zeros(len(p), np.dtype(fields))
    for k, n in enumerate("xyz"):
        a[n] = p[:, k]
    head = f"ply\nformat binary_little_endian 1.0\nelement vertex {len(p)}\nproperty double x\nproperty double y\nproperty double z\n"
    if colors is not None:
        c = np.clip(np.rint(np.asarray(colors, np.float64).reshape(-1, 3) * 255.0), 0, 255).astype(np.uint8)
        for k, n in enumerate(("red", "green", "blue")):
            a[n] = c[:, k]
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    with open(str(file), "wb") as f:
        f.write((head + "end_header\n").encode("ascii"))
        f.write(a.tobytes())


def test_point_cloud_without_normals_is_unchanged(tmp_path):
    rng = np.random.default_rng(1)
    p, c = rng.normal(size=(777, 3)), rng.uniform(-0.1, 1.1, (777, 3))
    for colors in (None, c):
        U.write_point_cloud(tmp_path / "new.ply", p, colors)
        _todays_writer(tmp_path / "old.ply", p, colors)
        assert open(tmp_path / "new.ply", "rb").read() == open(tmp_path / "old.ply", "rb").read()


def test_arbiter_excludes_at_most_one_per_cent():
    """the GPU normal test compares where the eigenvalue gap is at least GAP_MIN: on its clouds (the surface's first 5000 points,
    and the same moved by 1e4) the arbiter alone puts at most 1 % of the points under it"""
    p = CR.surface()[:5000]
    idx = CR.surface_knn(5000)[:, :20]
    assert np.array_equal(idx[:, 0], np.arange(5000)), "every point is its own first neighbour"
    for cloud, index in ((p, idx), (p + 1e4, CR.knn_brute(p + 1e4, 20))):
        nrm, w = CR.normals_ref(cloud, index)
        under = float((CR.gap(w) < CR.GAP_MIN).mean())
        print("under the gap:", under, "smallest gap:", CR.gap(w).min())
        assert under <= CR.EXCLUDED_MAX
        assert np.abs(np.linalg.norm(nrm, axis=1) - 1).max() <= 1e-14 and np.all(nrm[:, 2] >= 0)


def test_arbiter_neighbours_by_the_plain_definition():
    """knn_brute's cut at the k-th distance loses nothing: it equals lexsort((index, d2)) over whole rows, ties included"""
    p = CR.lattice(5, 5, 5)
    d = p[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    for k in (1, 20, 32):
        want = np.stack([np.lexsort((np.arange(len(p)), d2[i]))[:k] for i in range(len(p))])
        assert np.array_equal(CR.knn_brute(p, k), want)
    assert np.array_equal(CR.knn_brute(p[:3], 5), [[0, 1, 2, -1, -1], [1, 0, 2, -1, -1], [2, 1, 0, -1, -1]])


def test_cli_flags(tmp_path, monkeypatch):
    """--no-clouds and --plot reach evaluate_scene; without them the clouds are written and nothing is plotted"""
    seen = []
    monkeypatch.setattr(E, "evaluate_scene", lambda *a, **kw: seen.append(kw) or {"precision": 0.0, "recall": 0.0, "fscore": 0.0})
    monkeypatch.setattr(E, "read_ply", lambda f: (np.zeros((0, 3)), np.zeros((0, 3), np.int32)))
    monkeypatch.setattr(E, "read_crop_volume", lambda f: {})
    monkeypatch.setattr(E, "read_trajectory", lambda f: np.zeros((0, 4, 4)))
    monkeypatch.setattr(E, "read_trajectory_log", lambda f: np.zeros((0, 4, 4)))
    monkeypatch.setattr(np, "loadtxt", lambda f: np.eye(4))
    base = ["--dataset-dir", str(tmp_path / "Barn"), "--traj-path", "t.log", "--ply-path", str(tmp_path / "m.ply")]
    E.main(base)
    E.main(base + ["--no-clouds", "--plot"])
    assert (seen[0]["clouds"], seen[0]["plot"]) == (True, False) and (seen[1]["clouds"], seen[1]["plot"]) == (False, True)
