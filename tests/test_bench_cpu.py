"""bench.py's host side without a GPU: the files `--dump-outputs` writes (dtypes, the 64 MB cap, the fixed sample above it) and the
options of a plain run.  bench.py is imported in a child process: its import sets environment variables for the HIP runtime."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _py(code):
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def _files(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_keeps_dtypes_and_caps_the_total_with_a_fixed_sample(tmp_path):
    _py(f"""
import torch, bench
a = {{"big": torch.arange(12_000_000, dtype=torch.float32), "big64": torch.arange(4_000_000, dtype=torch.float64),
      "loss": torch.tensor([2.5], dtype=torch.float64), "acts": torch.ones(3, 4, dtype=torch.bfloat16)}}
for d in ("one", "two"):
    bench.dump_outputs({str(tmp_path)!r} + "/" + d, a)
""")
    one, two = _files(tmp_path / "one"), _files(tmp_path / "two")
    assert sorted(one) == ["acts", "big", "big64", "loss"]
    assert sum(os.path.getsize(tmp_path / "one" / f) for f in os.listdir(tmp_path / "one")) <= 64_000_000
    assert one["loss"].dtype == np.float64 and one["loss"].tolist() == [2.5]                   # small arrays whole
    assert one["acts"].dtype == np.float32 and one["acts"].shape == (3, 4) and (one["acts"] == 1).all()
    assert one["big"].dtype == np.float32 and one["big64"].dtype == np.float64
    for k, n in (("big", 12_000_000), ("big64", 4_000_000)):
        s = one[k]                                                                            # element i holds i: the sample's positions
        assert 0.7 * n < len(s) < n and (np.diff(s) > 0).all() and s[0] >= 0 and s[-1] < n
        np.testing.assert_array_equal(s, two[k])                                              # the same sample every run
    assert abs(len(one["big"]) / 12_000_000 - len(one["big64"]) / 4_000_000) < 1e-6            # one fraction for every large array


def test_dump_outputs_below_the_cap_writes_everything(tmp_path):
    _py(f"""
import torch, bench
bench.dump_outputs({str(tmp_path)!r}, {{"params": torch.arange(1_000_000, dtype=torch.float32), "loss": torch.tensor([1.0], dtype=torch.float64)}})
""")
    f = _files(tmp_path)
    np.testing.assert_array_equal(f["params"], np.arange(1_000_000, dtype=np.float32))
    assert f["loss"].dtype == np.float64


def test_plain_run_options():
    out = json.loads(_py("""
import json, sys
sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"]
import bench
a = bench.parse()
sys.argv = ["bench.py", "--steps", "7", "--full", "--dump-outputs", "d"]
b = bench.parse()
print(json.dumps([a.steps, a.warmup, a.full, a.dump_outputs, b.full, b.dump_outputs]))
"""))
    assert out == [7, 3, False, None, True, "d"]
