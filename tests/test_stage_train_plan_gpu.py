"""The plan's FORWARD wiring of the stage-level training launches (csrc/plan.hip over csrc/stage_train.hip) held to fp64 unit by unit on a real MI355X: a fresh child
per form (tests/stage_train_plan_worker.py) with CLHIP_STAGE_TRAIN=1, so that batches 5 and 72 take the launches as well, runs `cifar14` and `mod14` and judges z,
the recovered batch statistics, y and feat of every unit with plan_ref.judge in its forward-only mode -- which z / y pointer the plan hands to which table row, the
entry block inside its run's launch or in front of it, the pooling inside the last run's launch or behind it.  Forms: the default, STAGE_ENTRY=0, STAGE_POOL=0,
STAGE_XCH3=0; each asserts through clhip_plan_stage_info that the launches ran (as many backward as forward launches, `cifar14`: its three runs of 4 + 2 + 2 units)
and that the status word is 0.  Children run one at a time; after one that timed out or ended abnormally no other child is started.
The kernels themselves are held to fp64 in tests/test_stage_train_kernels_gpu.py; the BACKWARD of a run inside a plan is not judged here (its gradients never leave
LDS; DESIGN.md lists what a per-run judgement still needs) and keeps the comparison of tests/test_stage_train_gpu.py."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["cifar14-b5", "cifar14-b72", "mod14-b5", "mod14-b72"]
FORMS = [("default", {}), ("STAGE_ENTRY=0", dict(STAGE_ENTRY="0")), ("STAGE_POOL=0", dict(STAGE_POOL="0")), ("STAGE_XCH3=0", dict(STAGE_XCH3="0"))]
_STATE = {"abnormal": None}


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_plan_forward_in_stage_form_against_fp64(form):
    assert _STATE["abnormal"] is None, f"not started: the child of {_STATE['abnormal']} ended abnormally"
    name, sw = form
    env = dict(os.environ, CLHIP_STAGE_TRAIN="1")
    for k, v in sw.items():
        env["CLHIP_" + k] = v
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "stage_train_plan_worker.py"), ",".join(CASES)], env=env, capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired:
        _STATE["abnormal"] = name
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _STATE["abnormal"] = name
    assert r.returncode in (0, 1) and "RATIOS " in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    line = lambda tag: json.loads([ln for ln in r.stdout.splitlines() if ln.startswith(tag + " ")][-1][len(tag) + 1:])
    ratios, info = line("RATIOS"), line("INFO")
    for c in CASES:
        print(f"[ratio] stage_train_plan {name} {c} " + " ".join(f"{k}={v:.3g}" for k, v in sorted(ratios[c].items())) + f"  info {info[c]}")
        assert {"z", "mean", "var", "y", "feat"} <= set(ratios[c]), ratios[c].keys()
        units, fwd, bwd, status = info[c]
        assert status == 0, (c, status)
        assert units > 0 and fwd > 0 and fwd == bwd, (c, info[c])
        if c.startswith("cifar14"):
            assert (units, fwd, bwd) == (8, 3, 3), (c, info[c])
    print(f"[measure] stage_train_plan {name:16s} worst err/bound {max(v for d in ratios.values() for v in d.values()):.4f}   child {time.time() - t0:.1f} s")
    fails = [ln for ln in r.stdout.splitlines() if ln.startswith("FAIL ")]
    assert not fails, (name, fails[:20])
    assert all(v <= 1.0 for d in ratios.values() for v in d.values()), ratios
    assert r.returncode == 0


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_plan_backward_per_run_against_fp64(form):
    """dw, dgamma, dbeta of every unit of every run and the dy in front of the run, from dfeat / the stored dy at the run's output: a chain of
    stage_train_ref.judge_bwd blocks with the statistics recovered from the running statistics (the worker's docstring)"""
    assert _STATE["abnormal"] is None, f"not started: the child of {_STATE['abnormal']} ended abnormally"
    name, sw = form
    env = dict(os.environ, CLHIP_STAGE_TRAIN="1")
    for k, v in sw.items():
        env["CLHIP_" + k] = v
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "stage_train_plan_worker.py"), ",".join(CASES), "bwd"], env=env, capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired:
        _STATE["abnormal"] = name
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _STATE["abnormal"] = name
    assert r.returncode in (0, 1) and "RATIOS " in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    line = lambda tag: json.loads([ln for ln in r.stdout.splitlines() if ln.startswith(tag + " ")][-1][len(tag) + 1:])
    ratios, info = line("RATIOS"), line("INFO")
    for c in CASES:
        print(f"[ratio] stage_train_plan bwd {name} {c} " + " ".join(f"{k}={v:.3g}" for k, v in sorted(ratios[c].items())) + f"  info {info[c]}")
        assert {"dw", "dgamma", "dbeta", "dx"} <= set(ratios[c]), ratios[c].keys()
        assert info[c][3] == 0 and info[c][1] > 0 and info[c][1] == info[c][2], (c, info[c])
    print(f"[measure] stage_train_plan bwd {name:16s} worst err/bound {max(v for d in ratios.values() for v in d.values()):.4f}   child {time.time() - t0:.1f} s")
    fails = [ln for ln in r.stdout.splitlines() if ln.startswith("FAIL ")]
    assert not fails, (name, fails[:20])
    assert all(v <= 1.0 for d in ratios.values() for v in d.values()), ratios
    assert r.returncode == 0
