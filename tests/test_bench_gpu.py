"""bench.py's one-line JSON contract (metric / value / unit / n_gpus / steps / warmup / ms_per_step / higher_is_better / scaling /
vs_baseline / dtype / data / config.workload; with --full also roofline + cpu_baseline and the rest), on short runs; and what a
plain run leaves out and writes with --dump-outputs."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_has_the_contract_fields():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "8", "--full"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "median_ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 8 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["unit"] == "views/s" and d["value"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-2 * d["value"]
    assert "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] in ("GB/s", "TFLOP/s") and rf["peak"] > 0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and "traffic" in rf
    assert rf["kernel"] == "blend_bwd" and rf["measured"] == "timed region", "the contract workload: live bracket of the backward blend"
    assert d["render_level_ms"] > d["ms_per_step"] * 0.9 and d["train_step_ms"] > d["ms_per_step"] * 0.9  # the callers
    assert d["material_step_ms"] > d["train_step_ms"], "the material stage adds the light's prefilter and the deferred shading"
    # the same workload on the reference's own (bit-identical) instance list, beside the default mode's subset of it
    rb = d["reference_binning"]
    assert d["reference_binning_ms_per_step"] == rb["ms_per_step"] > 0 and rb["num_rendered"] > d["config"]["num_rendered"]
    assert abs(sum(d["stages_ms"].values()) - d["ms_per_step"]) < 0.25 * d["ms_per_step"], "stage totals add up to about the step"
    # the same K steps timed right behind the first warm-up (inside the clock governor's ramp), beside the headline
    cr = d["clock_ramp"]
    assert cr["ms_per_step_at_start"] > 0 and abs(cr["value_at_start"] - 1e3 / cr["ms_per_step_at_start"]) < 1e-2 * cr["value_at_start"]
    cb = d["cpu_baseline"]
    assert cb["kind"] in ("reference", "port") and cb["cores"] >= 1 and cb["value"] > 0 and cb["unit"] == d["unit"] and cb["sample"]


def test_bench_two_ranks_share_one_gpu_over_gloo():
    """The N > 1 path of bench.py (launch contract, one collective per step over the gradient arena, blocking and
    pipelined timings, max over ranks) run functionally: two ranks on the one GPU of the box, gloo instead of RCCL."""
    # two processes share the one GPU here: the radix sort must not assume it has the device to itself
    env = dict(os.environ, GS2M_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", GS2M_BENCH_WATCHDOG_S="240")  # (bench.py switches the tile sort to tickets itself at N > 1)
    port = 29700 + os.getpid() % 200
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--gaussians", "30000", "--width", "320", "--height", "192", "--full"], capture_output=True, text=True, timeout=400, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, "rank 0 prints ONE line"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["steps"] == 3
    # north_star / BASELINE configs[4]: ONE view per rank and step on the camera ring, blocking sum of its gradients: that is `value`
    assert d["config"]["views_per_rank"] == 1 and d["views_per_step"] == 2
    assert abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) < 1e-2 * d["value"], "whole-job views/s"
    assert "one view per rank" in d["config"]["workload"] and "ring" in d["config"]["workload"] and "collective" in d["config"]["workload"]
    assert "cpu_baseline" not in d and d["median_ms_per_step"] > 0
    # beside it, labelled: pipelined, equal-work cameras, two accumulated views per rank, no collective at all
    for key, views in (("pipelined", 2), ("equal_work", 2), ("accumulate_v2", 4), ("compute_only", 2)):
        assert d[key + "_ms_per_step"] > 0 and abs(d[key + "_value"] - views * 1e3 / d[key + "_ms_per_step"]) < 1e-2 * d[key + "_value"], key
    assert 0 < d["scaling_efficiency_vs_compute_only"] <= 1.5
    rf = d["roofline"]  # small frame: either blend kernel may be the longer one; the line says which and how it was timed
    assert rf["kernel"] in ("blend_bwd", "blend_fwd") and rf["avg_launch_ms"] > 0
    assert rf["measured"] == ("timed region" if rf["kernel"] == "blend_bwd" else "stage pass (untimed, same step)")


def test_bench_gpus_2_as_typed_starts_its_own_ranks():
    """`python bench.py --gpus 2 --steps 3 --warmup 2 --full` as the driver would type it -- no launcher, WORLD_SIZE unset:
    bench.py starts `torch.distributed.run` as a child before it touches the GPU, relays rank 0's line and the child's
    exit code (BASELINE configs[4]; here both ranks share the box's one GPU over gloo)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(GS2M_DIST_BACKEND="gloo", GS2M_BENCH_WATCHDOG_S="500")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2", "--full"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, "rank 0 prints ONE line"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 2 and d["scaling"] == "weak"
    assert d["config"]["views_per_rank"] == 1 and d["views_per_step"] == 2
    for key in ("pipelined", "equal_work", "accumulate_v2", "compute_only"):
        assert d[key + "_ms_per_step"] > 0 and d[key + "_value"] > 0, key


FULL_ONLY = ("median_ms_per_step", "roofline", "stages_ms", "clock_ramp", "reference_binning", "reference_binning_ms_per_step",
             "cpu_baseline", "render_level_ms", "train_step_ms", "material_step_ms")
OUTPUTS = ("color", "radii", "observe", "buffer", "grad_means3D", "grad_means2D", "grad_shs", "grad_opacities", "grad_scales",
           "grad_rotations", "grad_features")


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run prints the headline only, takes exactly --steps timed steps and, with --dump-outputs, writes what the last
    timed step computed; two runs with the same arguments render the same inputs (small workload: the whole arrays)."""
    import numpy as np
    import helpers as Hh
    lines, dumps = [], []
    for run in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--gaussians", "20000",
               "--width", "320", "--height", "192", "--dump-outputs", str(tmp_path / run)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]))
        dumps.append({n: np.load(tmp_path / run / (n + ".npy")) for n in OUTPUTS})
    d = lines[0]
    assert d["steps"] == 4 and d["warmup"] == 2 and d["n_gpus"] == 1 and d["unit"] == "views/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-2 * d["value"]
    assert not [k for k in FULL_ONLY if k in d], "a plain run leaves these to --full"
    a, b = dumps
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in OUTPUTS)
    assert sum(x.nbytes for x in a.values()) <= 64e6 and all(x.dtype == np.float32 for x in a.values())
    assert a["color"].shape == (3, 192, 320) and a["radii"].shape == (20000,) and a["grad_shs"].shape == (20000, 16, 3)
    assert (a["radii"] > 0).sum() == d["config"]["visible"] and np.abs(a["grad_means3D"]).max() > 0
    assert np.array_equal(a["radii"], b["radii"]) and np.array_equal(a["observe"], b["observe"])
    Hh.assert_image_close("color", a["color"], b["color"])
    Hh.assert_image_close("buffer", a["buffer"], b["buffer"], scale=10.0)
    for n in OUTPUTS[4:]:
        Hh.assert_grad_close(n[5:], a[n], b[n])
