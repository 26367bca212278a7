"""CPU: what a plain ``bench.py`` run does -- set-up, warm-up, exactly ``--steps`` timed steps, the outputs of the last timed
step under ``--dump-outputs DIR``, the line -- and that none of ``--full`` (sequential replay, per-kernel figures, secondary
region, CPU baseline) runs without it.  Dry run on the product's host path (``--device cpu --tiny``), one rank."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    res = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--device", "cpu", "--tiny", "--steps", "3", "--warmup", "1",
                          *extra], capture_output=True, text=True, env=env, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0])


def _load(path):
    return {f: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    d = _run("--dump-outputs", str(tmp_path / "a"))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "images/sec" and d["higher_is_better"] is True
    assert abs(d["value"] - 2 * d["steps"] / (d["ms_per_step"] * d["steps"] / 1e3)) <= 1e-6 * d["value"]
    assert d["replay_steps"] == 0 and d["kernels"] == {} and d["roofline"] is None and d["secondary"] is None
    assert "cpu_baseline" not in d and "roi_align_856MB" not in d["config"]
    a = _load(tmp_path / "a")
    assert "grad_sample.npy" in a and len(a) >= 3  # the gradient sample and the loss terms
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["grad_sample.npy"].size > 1000 and np.isfinite(a["grad_sample.npy"]).all()
    assert np.abs(a["grad_sample.npy"]).max() > 0
    # the same arguments give the same inputs, so a second run computes the same outputs
    _run("--dump-outputs", str(tmp_path / "b"))
    b = _load(tmp_path / "b")
    assert sorted(b) == sorted(a)
    for name in a:
        np.testing.assert_allclose(b[name], a[name], rtol=1e-5, atol=1e-8, err_msg=name)


def test_per_shape_csv_needs_full():
    res = subprocess.run([sys.executable, BENCH, "--device", "cpu", "--tiny", "--per-shape-csv", "x.csv"], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode != 0 and "--full" in res.stderr
