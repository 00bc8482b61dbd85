"""LPIPS without a GPU: the restatement tests/lpips_ref.py against what the reference's own code recorded
(tests/golden/ref_lpips.npz, make_lpips_golden.py), the weight files' key handling, the host-side refusals and the command line."""
import os

import numpy as np
import pytest
import torch

import lpips_ref as LR

import gs2m_lpips as GL  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_lpips.npz")


def test_restatement_fp32_matches_the_reference_recording():
    """the same expressions in float32 on the same CPU give the reference's bits or the next float (the conv2d may pick another
    algorithm for another build of torch: a few ulp of one tap's mean, not more); float64 stays within the fp32 error"""
    g = np.load(GOLDEN)
    assert int(g["seed"]) == LR.GOLDEN_SEED
    w = LR.make_weights(LR.GOLDEN_SEED)
    cases = LR.cases()
    assert sorted(k[:-2] for k in g.files if k.endswith("/a")) == sorted(cases)
    for name, (a, b) in cases.items():
        assert np.array_equal(g[f"{name}/a"], a) and np.array_equal(g[f"{name}/b"], b)
        layers32, total32 = LR.lpips(a, b, w, torch.float32)
        layers64, total64 = LR.lpips(a, b, w)
        gold, gold_layers = float(g[f"{name}/lpips"]), g[f"{name}/layers"].astype(np.float64)
        print(f"{name}: golden {gold!r} fp32 {total32!r} fp64 {total64!r}")
        assert np.allclose(layers32, gold_layers, rtol=1e-5, atol=1e-10) and np.isclose(total32, gold, rtol=1e-5, atol=1e-10)
        assert np.allclose(layers64, gold_layers, rtol=1e-4, atol=1e-9) and np.isclose(total64, gold, rtol=1e-4, atol=1e-9)
    assert float(g["identical_24x20/lpips"]) == 0.0 and LR.lpips(*cases["identical_24x20"], w)[1] == 0.0


def _thin(sd):
    """the same keys, shapes and dtypes on one-element storages: torch.save writes a few KB instead of 59 MB"""
    return {k: torch.zeros((), dtype=v.dtype).expand(v.shape) if v.numel() > 4096 else v for k, v in sd.items()}


@pytest.fixture(scope="module")
def dicts():
    w = LR.make_weights(LR.GOLDEN_SEED)
    return {(full, orig): tuple(_thin(sd) for sd in LR.state_dicts(w, full, orig)) for full in (True, False) for orig in (True, False)}


def _save(tmp_path, vgg, lin):
    v, l = str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg_lin.pth")
    torch.save(vgg, v)
    torch.save(lin, l)
    return v, l


@pytest.mark.parametrize("full", [True, False], ids=["full_model_keys", "bare_feature_keys"])
@pytest.mark.parametrize("orig", [True, False], ids=["lpips_lin_keys", "renamed_lin_keys"])
def test_read_weights_accepts_both_spellings(tmp_path, dicts, full, orig):
    vgg, lin = dicts[(full, orig)]
    vgg = dict(vgg)
    if full:  # torchvision's whole vgg16: the classifier is there and ignored
        vgg["classifier.0.weight"], vgg["classifier.0.bias"] = torch.zeros(()).expand(4096, 25088), torch.zeros(4096)
    conv_w, conv_b, lins = GL.read_weights(*_save(tmp_path, vgg, lin))
    assert [tuple(t.shape) for t in conv_w] == [(co, ci, 3, 3) for ci, co in zip(LR.CONV_CIN, LR.CONV_COUT)]
    assert [tuple(t.shape) for t in conv_b] == [(co,) for co in LR.CONV_COUT]
    assert [tuple(t.shape) for t in lins] == [(c,) for c in LR.TAP_CHANNELS]
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in conv_w + conv_b + lins)
    w = LR.make_weights(LR.GOLDEN_SEED)
    assert np.array_equal(conv_w[0].numpy(), w["conv_w"][0]) and np.array_equal(lins[4].numpy(), w["lin"][4])  # the small ones are kept whole
    assert sum(t.numel() for t in conv_w + conv_b + lins) == GL.PACKED_FLOATS == 14716160


def test_read_weights_names_the_offending_key(tmp_path, dicts):
    vgg, lin = dicts[(True, True)]
    bad = dict(vgg)
    bad["features.17.weight"] = torch.zeros(()).expand(512, 256, 3, 1)
    with pytest.raises(ValueError, match=r"`features\.17\.weight` must have shape \(512, 256, 3, 3\)"):
        GL.read_weights(*_save(tmp_path, bad, lin))
    bad = dict(vgg)
    bad["features.2.bias"] = vgg["features.2.bias"].double()
    with pytest.raises(ValueError, match=r"`features\.2\.bias` must be a float32 tensor"):
        GL.read_weights(*_save(tmp_path, bad, lin))
    bad = {k: v for k, v in vgg.items() if k != "features.28.bias"}
    with pytest.raises(KeyError, match=r"features\.28\.bias"):
        GL.read_weights(*_save(tmp_path, bad, lin))
    bad = dict(lin)
    bad["lin3.model.1.weight"] = torch.zeros(1, 256, 1, 1)
    with pytest.raises(ValueError, match=r"`lin3\.model\.1\.weight` must have shape \(1, 512, 1, 1\)"):
        GL.read_weights(*_save(tmp_path, vgg, bad))
    bad = {k: v for k, v in lin.items() if k != "lin0.model.1.weight"}
    with pytest.raises(KeyError, match=r"lin0\.model\.1\.weight"):
        GL.read_weights(*_save(tmp_path, vgg, bad))


def test_a_missing_file_names_its_flag(tmp_path, dicts):
    v, l = _save(tmp_path, *dicts[(True, True)])
    with pytest.raises(FileNotFoundError, match="--lpips-vgg"):
        GL.load_weights(str(tmp_path / "nowhere.pth"), l)
    with pytest.raises(FileNotFoundError, match="--lpips-lin"):
        GL.load_weights(v, str(tmp_path / "nowhere.pth"))


def test_host_side_refusals():
    w = GL.Weights(torch.zeros(1))
    ok = torch.zeros((1, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        GL.lpips(ok, ok, w)
    with pytest.raises(RuntimeError, match="no CPU path"):
        GL.lpips(ok.numpy(), ok, w)
    with pytest.raises(RuntimeError, match="must be uint8"):
        GL.lpips(ok.float(), ok, w)
    with pytest.raises(RuntimeError, match="must be uint8"):
        GL.lpips_layers(ok.to(torch.int8), ok, w)
    for shape in ((1, 16, 16, 1), (1, 16, 16, 4), (16, 16, 3)):
        with pytest.raises(RuntimeError, match="CH 3"):
            GL.lpips(torch.zeros(shape, dtype=torch.uint8), ok, w)
    for shape in ((1, 15, 16, 3), (1, 16, 15, 3), (1, 1, 1, 3)):
        with pytest.raises(RuntimeError, match="at least 16 x 16"):
            GL.lpips(torch.zeros(shape, dtype=torch.uint8), torch.zeros(shape, dtype=torch.uint8), w)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        GL.lpips(torch.zeros((1, 16, 32, 3), dtype=torch.uint8)[:, :, ::2], ok, w)
    with pytest.raises(RuntimeError, match="no CPU path"):
        GL.pack_weights([], [], [], device="cpu")


def test_cli_wants_both_weight_files_or_neither(tmp_path, capsys):
    import gs2m_metrics as GM
    for flag in ("--lpips-vgg", "--lpips-lin"):
        with pytest.raises(SystemExit) as e:
            GM.main(["-m", str(tmp_path), flag, str(tmp_path / "x.pth")])
        assert e.value.code == 2
        assert "--lpips-vgg and --lpips-lin go together" in capsys.readouterr().err
    with pytest.raises(FileNotFoundError, match="--lpips-vgg"):  # both given: the files are looked at, before any device
        GM.main(["-m", str(tmp_path), "--lpips-vgg", str(tmp_path / "v.pth"), "--lpips-lin", str(tmp_path / "l.pth")])
