"""Host side of the image metrics (gs2m_metrics.py): the float64 restatement tests/metrics_ref.py against the
reference's own values (tests/golden/metrics.npz) and against hand-computed squared errors, the file pairing, the
metrics.json merge, and the refusals of `image_metrics`.  No GPU."""
import json
import os
import re

import numpy as np
import pytest
import torch

import metrics_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "metrics.npz")


def _golden_cases():
    if not os.path.exists(GOLDEN):
        return []
    return sorted({k.split("/")[0] for k in np.load(GOLDEN).files})


@pytest.mark.parametrize("name", _golden_cases())
def test_restatement_matches_the_reference_values(name):
    """the bounds tests/test_ssim_gpu.py:54 holds this operator to against fp32 torch"""
    z = np.load(GOLDEN)
    got = MR.metrics(z[f"{name}/a"], z[f"{name}/b"])
    ssim, psnr = float(z[f"{name}/ssim"]), float(z[f"{name}/psnr"])
    assert np.isclose(got["ssim"], ssim, rtol=1e-5, atol=1e-6), (got["ssim"], ssim)
    if np.isinf(psnr):
        assert got["psnr"] == psnr
    else:
        assert np.isclose(got["psnr"], psnr, rtol=1e-5, atol=0.0), (got["psnr"], psnr)


def test_squared_error_hand_computed():
    a = np.full((7, 5, 3), 93, np.uint8)
    assert MR.metrics(a, a.copy()) == {"sse": 0, "psnr": float("inf"), "ssim": pytest.approx(1.0, abs=1e-12)}
    z, o = np.zeros((4, 6, 3), np.uint8), np.full((4, 6, 3), 255, np.uint8)
    m = MR.metrics(z, o)
    assert m["sse"] == 4 * 6 * 3 * 255 * 255 and m["psnr"] == 0.0  # mse = 1
    b = a.copy()
    b[3, 2, 1] = 90
    m = MR.metrics(a, b)
    assert m["sse"] == 9
    assert m["psnr"] == pytest.approx(20 * np.log10(255.0 / np.sqrt(9 / 105.0)), rel=1e-14)
    big, other = np.zeros((1, 1, 1), np.uint8), np.full((1, 1, 1), 255, np.uint8)
    assert MR.squared_error(big, other) == 65025 and isinstance(MR.squared_error(big, other), int)


def test_window_is_the_kernels():
    """the eleven weights csrc/image_metrics.hip and csrc/ssim.hip take from csrc/window11.h, and nowhere else, are the
    restatement's (torch's fp32 arithmetic)"""
    from math import exp
    g = torch.Tensor([exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    assert np.array_equal((g / g.sum()).numpy(), MR.window_1d())
    csrc = os.path.join(ROOT, "gs-2m_amd", "csrc")
    for f in ("image_metrics.hip", "ssim.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "window11.h"' in src and "WINDOW11_W" not in src and "_W[11]" not in src, f
    body = re.search(r"_W\[11\] = \{([^}]*)\}", open(os.path.join(csrc, "window11.h")).read()).group(1)
    w = np.array([np.float32(t.strip().rstrip("f")) for t in body.split(",")], dtype=np.float32)
    assert np.array_equal(w, MR.window_1d())


def test_tile_constants_are_the_headers():
    import gs2m_metrics as GM
    src = open(os.path.join(ROOT, "include", "gs2m_metrics.h")).read()
    assert int(re.search(r"#define GS2M_METRICS_TILE_W (\d+)", src).group(1)) == GM.TILE_W
    assert int(re.search(r"#define GS2M_METRICS_TILE_H (\d+)", src).group(1)) == GM.TILE_H


def test_collect_pairs_sorted_and_missing_namesake(tmp_path):
    import gs2m_metrics as GM
    r, g = tmp_path / "render", tmp_path / "gt"
    r.mkdir(); g.mkdir()
    for n in ("00010.png", "00002.png", "00001.png"):
        (r / n).write_bytes(b"x"); (g / n).write_bytes(b"y")
    (g / "extra.png").write_bytes(b"y")  # a ground truth nobody rendered is not scored
    pairs = GM.collect_pairs(str(r), str(g))
    assert [p[0] for p in pairs] == ["00001.png", "00002.png", "00010.png"]
    assert pairs[1][1] == str(r / "00002.png") and pairs[1][2] == str(g / "00002.png")
    (r / "00005.png").write_bytes(b"x")
    with pytest.raises(FileNotFoundError, match="00005.png"):
        GM.collect_pairs(str(r), str(g))


def test_merge_metrics_keeps_other_methods_and_replaces_its_own(tmp_path):
    import gs2m_metrics as GM
    path = tmp_path / "metrics.json"
    GM.merge_metrics(str(path), "ours_7000", {"ssim": 0.8, "psnr": 25.0})
    GM.merge_metrics(str(path), "ours_30000", {"ssim": 0.9, "psnr": 30.0})
    GM.merge_metrics(str(path), "ours_30000", {"ssim": 0.95, "psnr": 31.5})
    text = path.read_text()
    assert json.loads(text) == {"ours_7000": {"ssim": 0.8, "psnr": 25.0}, "ours_30000": {"ssim": 0.95, "psnr": 31.5}}
    assert text == json.dumps(json.loads(text), indent=4)
    assert "lpips" not in text


def test_image_metrics_refuses_cpu_int32_and_permuted():
    import gs2m_metrics as GM
    a = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        GM.image_metrics(a, a)
    with pytest.raises(RuntimeError, match="must be uint8"):
        GM.image_metrics(a.int(), a.int())
    with pytest.raises(RuntimeError, match="must be contiguous"):
        GM.image_metrics(torch.zeros(1, 3, 8, 8, dtype=torch.uint8).permute(0, 2, 3, 1), a)
    with pytest.raises(RuntimeError, match="CH 1 or 3"):
        GM.image_metrics(torch.zeros(1, 8, 8, 2, dtype=torch.uint8), torch.zeros(1, 8, 8, 2, dtype=torch.uint8))


def test_score_files_names_the_file_on_a_size_or_mode_mismatch(tmp_path):
    """found while reading the headers, before anything is decoded or sent to a device"""
    from PIL import Image
    import gs2m_metrics as GM
    r, g = tmp_path / "render", tmp_path / "gt"
    r.mkdir(); g.mkdir()
    Image.fromarray(np.zeros((6, 9, 3), np.uint8)).save(r / "00000.png")
    Image.fromarray(np.zeros((6, 9, 3), np.uint8)).save(g / "00000.png")
    Image.fromarray(np.zeros((6, 9, 3), np.uint8)).save(r / "00001.png")
    Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(g / "00001.png")
    with pytest.raises(ValueError, match="00001.png"):
        GM.score_files(GM.collect_pairs(str(r), str(g)))
    Image.fromarray(np.zeros((6, 9), np.uint8)).save(g / "00001.png")  # same size, one channel against three
    with pytest.raises(ValueError, match="00001.png"):
        GM.score_files(GM.collect_pairs(str(r), str(g)))
    Image.fromarray(np.zeros((6, 9), np.uint16)).save(r / "00001.png")  # 16-bit: refused by name
    with pytest.raises(ValueError, match="00001.png has mode"):
        GM.score_files(GM.collect_pairs(str(r), str(g)))
