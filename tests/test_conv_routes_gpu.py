"""Every convolution kernel family against fp64 on a real MI355X: the cases of tests/conv_ref.py, each on the route clhip_conv_route names for it (asserted
before the launch), every element judged by the per-element bound of tests/conv_ref.py -- forward without statistics, with partial rows and with the fp64
accumulators (1 and 8 replicas), dgrad with accumulate 0 and 1, the weight gradient without and with scratch, += into earlier content and bitwise
repeatability with scratch, dgrad with the producer's BatchNorm-backward sums, and the write-through lazy-input forward.  Outputs start as NaN and a guard
row behind every buffer stays untouched.  conv9.hip (off by default) runs all its five forms at every legal geometry.  Families behind switches that are
cached at their first use run in one fresh child process per setting, one after another.  The module prints one `[measure]` line per family at its end
(pytest -s); profiles/conv_sweep.md holds the table of an MI355X run."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_ref as R                       # noqa: E402
import conv_run                            # noqa: E402
from libcontinual_amd import _lib          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURE = {}


@pytest.fixture(scope="module", autouse=True)
def measure_table():
    yield
    for fam in sorted(MEASURE):
        print(f"\n[measure] {fam:24s} err/bound {MEASURE[fam][0]:.4f}   {MEASURE[fam][1]}", end="")
    print()


def _judge(res):
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, bad


_STATE = {"abnormal": None}          # the first case or child whose GPU work ended in a HIP error or abnormally: nothing is launched after it


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_case_against_fp64_on_its_route(case):
    assert _STATE["abnormal"] is None, f"not started: {_STATE['abnormal']} left the GPU in an error state"
    try:
        res = conv_run.run_case(_lib.lib(), case, MEASURE)
    except (RuntimeError, _lib.ClhipError) as e:
        if "HIP error" in str(e) or "hip" in str(e).lower() and "failed" in str(e).lower():
            _STATE["abnormal"] = case["name"]
        raise
    assert res
    _judge(res)


def test_conv9_runs_all_five_forms():
    """the case list holds conv9.hip to every form it has (a case that loses one fails here, not silently)"""
    nine = [c for c in R.CASES if c["name"].startswith("conv9-") and "refused" not in c["name"]]
    assert len(nine) == 14
    for c in nine:
        assert {k for k, f in c["routes"]["bf16"].items() if f == R.CONV9} == {"fwd0", "fwd2", "dgrad", "bnr", "wt"}, c["name"]
        assert c["shape"][3] in (128, 256) and c["sw"]["CONV9"] == "1"


@pytest.mark.parametrize("gi", range(len(R.CACHED)), ids=["+".join(g["env"]) for g in R.CACHED])
def test_cached_switch_families_in_a_fresh_process(gi):
    """CONV_V1 (with and without WGRAD_NO_TR), WGRAD2_ATOMIC, NO_PARITY_DGRAD, CONV3G=2: one child at a time, none after an abnormal exit"""
    assert _STATE["abnormal"] is None, f"not started: the child of {_STATE['abnormal']} ended abnormally"
    group = R.CACHED[gi]
    env = dict(os.environ)
    for k, v in group["env"].items():
        env["CLHIP_" + k] = v
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "conv_route_worker.py"), str(gi), "run"], env=env, capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired:
        _STATE["abnormal"] = "+".join(group["env"])
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _STATE["abnormal"] = "+".join(group["env"])
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    routes = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROUTES ")][-1][7:])
    ratios = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RATIOS ")][-1][7:])
    for case in group["cases"]:
        want = {f"{dt}/{key}": fam for (dt, key), fam in R.expected_of(case).items()}
        assert routes[case["name"]] == want, case["name"]
        assert ratios[case["name"]], case["name"]
        for k, v in ratios[case["name"]].items():
            dt, key, what = k.split("/", 2)
            fam = R.FAMILY_NAMES[case["routes"][dt][key]] + " [" + "+".join(f"{a}={b}" for a, b in group["env"].items()) + "]"
            print(f"[ratio] {case['name']} {dt} {key} {fam} {what} {v:.4g}")
            if v > MEASURE.get(fam, (0.0, ""))[0] or fam not in MEASURE:
                MEASURE[fam] = (v, f"{case['name']} {dt} {key} {what}")
        _judge({(case["name"], k): v for k, v in ratios[case["name"]].items()})
