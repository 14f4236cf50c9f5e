"""bench.py --dump-outputs: the arrays of the last timed step, written so that two builds can be compared output for output, and --steps
as the number of timed steps behind ms_per_step."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_writes_float_arrays_by_name(tmp_path):
    outs = {"mll": np.array([-1.5]), "alpha": np.arange(5, dtype=np.float32), "mu": np.arange(3, dtype=np.int64)}
    assert bench.dump_outputs(str(tmp_path / "d"), outs) == 1
    got = {f: np.load(tmp_path / "d" / f) for f in sorted(os.listdir(tmp_path / "d"))}
    assert sorted(got) == ["alpha.npy", "mll.npy", "mu.npy"]
    assert got["alpha.npy"].dtype == np.float32 and np.array_equal(got["alpha.npy"], outs["alpha"])
    assert got["mu.npy"].dtype == np.float64 and np.array_equal(got["mu.npy"], [0.0, 1.0, 2.0])
    assert got["mll.npy"].tolist() == [-1.5]


def test_dump_thins_outputs_over_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 800)
    big = np.arange(250, dtype=np.float64)          # 2000 bytes + 8: every 3rd entry
    assert bench.dump_outputs(str(tmp_path), {"alpha": big, "mll": np.array([2.0])}) == 3
    assert np.array_equal(np.load(tmp_path / "alpha.npy"), big[::3])
    assert np.load(tmp_path / "mll.npy").tolist() == [2.0]


def test_steps_below_one_are_refused():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--steps" in out.stderr, out.stderr[-2000:]


@pytest.mark.gpu
def test_dumped_outputs_are_the_last_timed_step(tmp_path):
    """A small bench run: the line counts the timed steps asked for, and the dumped arrays are the fit + predict_f of the LAST timed
    step's hyper-parameters (bench.run_workload: step i adds 1e-3 * (i % 7 + 1) to every kernel parameter), against the fp64 oracle."""
    from oracle import gp_oracle as G

    n, d, p, steps, warmup = 4096, 8, 64, 3, 1
    dump = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--n", str(n), "--d", str(d), "--p", str(p), "--steps", str(steps),
                          "--warmup", str(warmup), "--no-secondary", "--no-cpu-baseline", "--dump-outputs", str(dump)],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [ln_ for ln_ in out.stdout.splitlines() if ln_.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, (out.returncode, out.stdout[-1500:], out.stderr[-3000:])
    j = json.loads(lines[0])
    assert j["steps"] == steps and j["ms_per_step"] > 0
    got = {k: np.load(dump / f"{k}.npy") for k in ("mll", "alpha", "mu", "sigma2")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["mll"].tolist() == [j["config"]["mll"]]
    assert got["alpha"].shape == (n,) and got["mu"].shape == (p,) and got["sigma2"].shape == (p,)
    x, y, xs = bench.synthetic_inputs(n, d, p)
    h = 1e-3 * ((warmup + steps - 1) % 7 + 1)
    spec = ("se_ard", [v + h for v in bench._ll(d)], h)
    ref = G.update_mll(spec, x, y, math.log(0.1))
    mu_o, s2_o = G.predict_f(spec, x, ref, xs)
    assert abs(got["mll"][0] - ref["mll"]) <= 1e-7 * abs(ref["mll"])
    np.testing.assert_allclose(got["alpha"], ref["alpha"], rtol=1e-6, atol=1e-7 * np.abs(ref["alpha"]).max())
    np.testing.assert_allclose(got["mu"], mu_o, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(got["sigma2"], s2_o, rtol=1e-5, atol=1e-8)
