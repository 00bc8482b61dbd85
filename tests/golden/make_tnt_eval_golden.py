"""Generates tests/golden/ref_tnt_eval.npz and ref_tnt_scenes.json from the REFERENCE's own scripts/eval_tnt/ modules.
Run in the BUILD container only:

    python tests/golden/make_tnt_eval_golden.py

evaluation.py, trajectory_io.py and config.py are imported as they are; `open3d` (and matplotlib, where the image lacks it)
is an empty stand-in module registered HERE, in the generator only: the functions recorded below never touch it.  Recorded:
get_f1_score_histo2's seven outputs for several pairs of distance arrays (one pair empty, one with values at and beyond
5 tau, +inf among them), read_trajectory's matrices for a small .log written by write_trajectory (the file's text travels too),
and the scene / tau table.  Only arrays and settings are written."""
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/scripts/eval_tnt"


def distance_cases():
    rng = np.random.default_rng(7)
    tau = 0.01
    cases = {}
    cases["random"] = (tau, rng.gamma(2.0, 0.004, 5000), rng.gamma(1.5, 0.006, 7000))
    # values exactly on bin edges, at tau, at the last edge, at 5 tau, beyond, and +inf
    edges = np.arange(0, tau * 5, tau / 100)
    d1 = np.concatenate([edges[::7], [tau, edges[-1], 5 * tau, 5 * tau * (1 + 1e-15), 7 * tau, np.inf, np.inf, 0.0],
                         rng.uniform(0, 6 * tau, 900)])
    d2 = np.concatenate([edges[3::11], [np.nextafter(tau, 0), np.nextafter(edges[-1], 1), np.inf], rng.uniform(0, 5 * tau, 400)])
    cases["edges"] = (tau, d1, d2)
    cases["empty"] = (0.005, np.zeros(0), rng.uniform(0, 0.02, 50))
    cases["truck"] = (0.005, rng.gamma(2.0, 0.002, 3000), np.full(2000, np.inf))  # recall 0
    cases["ignatius"] = (0.003, np.abs(rng.normal(0, 0.002, 4000)), np.abs(rng.normal(0, 0.004, 2500)))
    return cases


def main():
    saved = {k: sys.modules.get(k) for k in ("open3d", "matplotlib", "matplotlib.pyplot")}
    sys.modules["open3d"] = types.ModuleType("open3d")
    try:
        importlib.import_module("matplotlib.pyplot")
    except Exception:
        sys.modules["matplotlib"] = types.ModuleType("matplotlib")
        sys.modules["matplotlib.pyplot"] = types.ModuleType("matplotlib.pyplot")
        sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.path.insert(0, REF)
    try:
        evaluation = importlib.import_module("evaluation")
        trajectory_io = importlib.import_module("trajectory_io")
        config = importlib.import_module("config")
    finally:
        sys.path.remove(REF)
        for k, m in saved.items():
            if m is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = m
    out = {}
    for name, (tau, d1, d2) in distance_cases().items():
        with contextlib.redirect_stdout(io.StringIO()):
            p, r, f, es, cs, et, ct = evaluation.get_f1_score_histo2(tau, "", 5, d1, d2)
        out[f"{name}/tau"], out[f"{name}/distance1"], out[f"{name}/distance2"] = np.float64(tau), d1, d2
        out[f"{name}/prf"] = np.array([p, r, f], np.float64)
        for k, a in (("edges_source", es), ("cum_source", cs), ("edges_target", et), ("cum_target", ct)):
            out[f"{name}/{k}"] = np.asarray(a)
        print(f"{name}: tau {tau} n1 {len(d1)} n2 {len(d2)} -> precision {p} recall {r} fscore {f}")
    rng = np.random.default_rng(3)
    traj = []
    for k in range(5):
        M = np.eye(4)
        M[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        M[:3, 3] = rng.normal(0, 3, 3)
        traj.append(trajectory_io.CameraPose([k, k, k + 1], M))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.log")
        trajectory_io.write_trajectory(traj, path)
        out["log/text"] = np.frombuffer(open(path, "rb").read(), np.uint8)
        out["log/poses"] = np.stack([t.pose for t in trajectory_io.read_trajectory(path)])
    np.savez_compressed(os.path.join(HERE, "ref_tnt_eval.npz"), **out)
    with open(os.path.join(HERE, "ref_tnt_scenes.json"), "w") as f:
        json.dump({"scenes_tau": config.scenes_tau_dict}, f, indent=1)
    print("written:", os.path.getsize(os.path.join(HERE, "ref_tnt_eval.npz")), "bytes")


if __name__ == "__main__":
    main()
