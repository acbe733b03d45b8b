"""The plan's side of the stage-level eval forward on a real MI355X: which units clhip_plan_forward_ex takes as one launch of csrc/stage.hip, what it hands that
launch, and what it does around it -- the path every CIFAR ResNet-32 method runs by default in eval mode, which tests/test_plan_units_gpu.py switches off so that
every activation is readable.  The child discipline is that file's: a fresh child per case (tests/stage_eval_worker.py, whose docstring lists the four checks) with
its own timeout, one at a time, no further child after one that timed out or ended abnormally; CLHIP_STAGE_TRAIN = 0, CLHIP_STAGE_EVAL left at its default.  The
kernel itself is held to fp64 in tests/test_stage_eval_kernels_gpu.py; here its output is the reference (bit-equal) and everything outside the runs is judged by
plan_ref.judge_eval.  The parent asserts CLHIP_FORM_FWD_EVAL_LAZY unit by unit: a unit keeps the consumer-side form it takes without runs exactly when neither it
nor the producer whose BatchNorm it applies lies in a run (a fused run reads and writes WRITTEN activations)."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

import stage_eval_worker as W              # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
F_EVAL_LAZY = 16                           # include/clhip.h: CLHIP_FORM_FWD_EVAL_LAZY
_STATE = {"abnormal": None}
MEASURE = {}


@pytest.fixture(scope="module", autouse=True)
def measure_table():
    yield
    for name, (ratios, secs) in MEASURE.items():
        print(f"\n[measure] {name:16s} " + " ".join(f"{k}={v:.3g}" for k, v in sorted(ratios.items())) + f"   child {secs:.1f} s", end="")
    print()


@pytest.mark.parametrize("case", list(W.CASES))
def test_plan_runs_selection_wiring_and_surroundings(case):
    assert _STATE["abnormal"] is None, f"not started: the child of {_STATE['abnormal']} ended abnormally"
    env = dict(os.environ, CLHIP_STAGE_TRAIN="0")
    env.pop("CLHIP_STAGE_EVAL", None)
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "stage_eval_worker.py"), case], env=env, capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired:
        _STATE["abnormal"] = case
        raise
    secs = time.time() - t0
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _STATE["abnormal"] = case
    assert r.returncode in (0, 1) and "SECONDS " in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    line = lambda tag: json.loads([ln for ln in r.stdout.splitlines() if ln.startswith(tag + " ")][-1][len(tag) + 1:])
    runs, refused, wiring, ratios, forms = line("RUNS"), line("REFUSED"), line("WIRING"), line("RATIOS"), line("FORMS")
    MEASURE[case] = (ratios, secs)
    print(f"[ratio] stage_eval_plan {case} runs {runs} " + " ".join(f"{k}={v:.3g}" for k, v in sorted(ratios.items())))
    print(f"[forms] stage_eval_plan {case} eval {forms['eval']} without runs {forms['eval_nostage']}")
    dt, want = W.CASES[case][3], W.CASES[case][4]
    # 1. run selection
    assert [ln for _, ln in runs] == want, runs
    assert refused["other"] == [] and refused["got"] == refused["expected"], refused
    assert len(refused["expected"]) == sum(ln - 1 for ln in want)
    # 2. wiring
    assert [w[:2] for w in wiring] == runs and all(w[2] == 0 for w in wiring), f"(first unit, length, elements that differ from clhip_stage_eval on the run's input): {wiring}"
    # 3. / 4. outside the runs
    fails = [ln for ln in r.stdout.splitlines() if ln.startswith("FAIL ")]
    assert not fails, fails[:20]
    n_units = len(forms["eval"])
    assert {"eval z", "eval y", "eval feat"} <= set(ratios) and ratios["units judged"] == n_units - sum(want)
    assert all(v <= 1.0 for k, v in ratios.items() if k != "units judged"), ratios
    assert r.returncode == 0
    # the consumer-side eval form, unit by unit
    in_run = {i + k for i, ln in runs for k in range(ln)}
    lazy = [bool(f & F_EVAL_LAZY) for f in forms["eval"]]
    lazy0 = [bool(f & F_EVAL_LAZY) for f in forms["eval_nostage"]]
    keep = [lazy0[i] and i not in in_run and (forms["src"][i] - 1) not in in_run for i in range(n_units)]
    assert lazy == keep, (lazy, keep)
    if dt == "f32":
        assert not any(lazy0)                                   # (the consumer-side eval forms are bf16 only)
    elif want:
        assert any(lazy0[i] for i in in_run)                    # the runs replace units that would have taken the form: the comparison above is not vacuous
