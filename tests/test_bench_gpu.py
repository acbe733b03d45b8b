"""bench.py's plain run on the GPU: it times exactly `--steps` steps, its line carries the headline fields and none of what `--full`
measures, and `--dump-outputs` writes the last step's results -- the same ones for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_times_the_given_steps_and_dumps_the_last_step(tmp_path):
    runs = []
    for d in ("a", "b"):
        out = _bench("--gpus", "1", "--steps", "6", "--warmup", "2", "--dump-outputs", str(tmp_path / d))
        assert out["steps"] == 6 and out["warmup"] == 2 and out["n_gpus"] == 1
        assert out["unit"] == "images/sec" and out["higher_is_better"] is True and out["dtype"] == "bf16" and out["metric"].startswith("images/sec")
        assert out["ms_per_step"] > 0 and abs(out["value"] - 256 * 6 / (out["ms_per_step"] * 6e-3)) < 1e-6 * out["value"]
        assert not {"roofline", "roofline_more", "secondary", "cpu_baseline"} & set(out)
        files = {f[:-4]: np.load(tmp_path / d / f) for f in os.listdir(tmp_path / d)}
        assert sorted(files) == ["acc1", "buffers", "loss", "params"]
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= 64_000_000
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in files.values())
        assert files["loss"].shape == (1,) and files["loss"][0] > 0
        runs.append(files)
    a, b = runs
    for k in a:                     # identical inputs: the same results, up to the run-to-run order of the fp64-atomic BatchNorm sums
        assert a[k].shape == b[k].shape
        assert float(np.abs(a[k] - b[k]).max()) <= 1e-5 * float(np.abs(a[k]).max()), k


def test_task_pass_plain_run_dumps_its_result(tmp_path):
    out = _bench("--workload", "herding_b50", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and "roofline" not in out
    picks = np.load(tmp_path / "exemplars.npy")
    assert picks.dtype == np.float64 and picks.shape == (3, 40)
    assert all(len(set(row.tolist())) == 40 and row.min() >= 0 and row.max() < 500 for row in picks)
