"""The ResNet plan executor (csrc/plan.hip) held to fp64 unit by unit on a real MI355X, in every form its switches select: tests/plan_ref.py judges every stored
tensor of a training step (z, the batch statistics, y, feat, dy of every activation, dw, dgamma, dbeta; a second pass onto the first one's gradients) and of an
eval forward against what fp64 makes of the plan's own stored inputs of that link.  The parent process never flips a switch (most are cached at their first
use and would leak across files): every form runs in a fresh child (tests/plan_unit_worker.py) with its switches as CLHIP_<NAME> in the environment, STAGE_TRAIN
= 0 in all of them (the stage-level launches keep their own file; dy does not exist inside them) and STAGE_EVAL = 0 (so every eval activation is readable; tests/test_stage_eval_plan_gpu.py holds the default, where runs of blocks are one launch).
Children run one at a time; after one that timed out or ended abnormally no other child is started.  Every form asserts through clhip_plan_unit_forms that the
units it is meant to exercise took that branch.  The module prints one `[measure]` line per form at its end (pytest -s); profiles/plan_units.md holds the table
of an MI355X run."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

import plan_ref as PR                      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURE = {}
_STATE = {"abnormal": None}

# include/clhip.h: CLHIP_FORM_FWD_* / CLHIP_FORM_BWD_*
F_LAZY, F_LAZY_RES, F_WT, F_PAIR, F_EVAL_LAZY = 1, 2, 4, 8, 16
B_BOTH, B_BN_GRAD, B_BN_GRAD_RES, B_LAZY_IN, B_EPI_SUMS, B_PAIR, B_PAIR_BN, B_WPAIR, B_SIDE, B_BRANCH, B_HOOK, B_POOL = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048

ALL = [PR.case_id(c) for c in PR.CASES]
EAGER = dict(BN_INPUT="0", BN_RES_INPUT="0", BN_INPUT_WT="0", BN_GRAD="0", BWD_FUSED="0", BN_FUSE="0", CONV6_PAIR="0", CONV7="0", POOL_BN_FUSE="0", PAIR_BN_FUSE="0",
             WGRAD_STREAM="0", BRANCH_STREAM="0", WGRAD_DEFER="0")
TWO = dict(WGRAD_NET_GFLOP="1")            # gives the small `wide` net at batch 16 a side stream (every 3x3 / s1 weight gradient there is >= 1 GFLOP)


def _form(name, env, dt="bf16", cases=ALL, cuts=False, expect=()):
    """expect: (case id, 'train' fwd word index 0 / bwd word index 1 / 'eval', bit, 'any' | 'none') -- over the units of that case"""
    return dict(name=name, env=env, dt=dt, cases=cases, cuts=cuts, expect=list(expect))


# what the default switches must exercise (bf16): a case that silently loses one of these branches fails here
NARROW = ["cifar14-b5", "cifar14-b36", "mod14-b5"]           # the 16 / 32 / 64-channel nets: lazy inputs, the one-launch backward forms, the stride-2 pairs
DEFAULT_EXPECT = ([(c, 0, b, "any") for c in NARROW for b in (F_LAZY, F_LAZY_RES, F_PAIR)] +
                  [(c, 1, b, "any") for c in NARROW for b in (B_BOTH, B_BN_GRAD, B_BN_GRAD_RES, B_LAZY_IN, B_EPI_SUMS, B_PAIR, B_PAIR_BN, B_WPAIR, B_POOL)] +
                  [(c, "eval", F_EVAL_LAZY, "any") for c in NARROW] + [("pre14-b6", 1, B_BOTH, "any")] +
                  [(c, 1, b, "any") for c in ("wide-b3", "wide-b16", "stem3-b3", "stem7-b3") for b in (B_EPI_SUMS, B_PAIR)] +
                  [(c, 1, B_SIDE | B_BRANCH | B_HOOK, "none") for c in ALL])          # (no layer of 4 GFLOP: one stream)

FORMS = [
    _form("eager", EAGER, expect=[(c, w, ~0, "none") for c in ALL for w in (0, 1)]),
    _form("eager-f32", EAGER, dt="f32", expect=[(c, w, ~0, "none") for c in ALL for w in (0, 1)]),
    _form("default", {}, expect=DEFAULT_EXPECT),
    _form("default-f32", {}, dt="f32", expect=[(c, 1, B_POOL, "any") for c in NARROW]),
    # (the max-pool stems train on the accumulator path only: the plan refuses them with BN_PARTIALS)
    _form("BN_PARTIALS=1", dict(BN_PARTIALS="1"), cases=[c for c in ALL if not c.startswith("stem")],
          expect=[(c, 0, F_LAZY | F_LAZY_RES | F_PAIR, "none") for c in ALL] + [(c, 1, B_EPI_SUMS | B_BN_GRAD | B_POOL, "none") for c in ALL]),
    _form("BN_FUSE=1", dict(BN_FUSE="1"), expect=[(c, 1, B_EPI_SUMS, "any") for c in ALL if c != "pre14-b6"]),
    _form("BN_FUSE=0", dict(BN_FUSE="0"), expect=[(c, 1, B_EPI_SUMS | B_PAIR_BN | B_POOL | B_BN_GRAD, "none") for c in ALL]),
    _form("BN_GRAD=0", dict(BN_GRAD="0"), expect=[(c, 1, B_BN_GRAD, "none") for c in ALL] + [(c, 1, b, "any") for c in NARROW for b in (B_BOTH, B_LAZY_IN)]),
    _form("BN_GRAD_RES=0", dict(BN_GRAD_RES="0"), expect=[(c, 1, B_BN_GRAD_RES, "none") for c in ALL] + [(c, 1, B_BN_GRAD, "any") for c in NARROW]),
    _form("BN_GRAD_MINC=32", dict(BN_GRAD_MINC="32"), expect=[(c, 1, B_BN_GRAD, "any") for c in NARROW]),
    _form("BWD_FUSED=0", dict(BWD_FUSED="0"), expect=[(c, 1, B_BOTH | B_BN_GRAD | B_LAZY_IN, "none") for c in ALL]),
    _form("BN_MASK_BITS=0", dict(BN_MASK_BITS="0"), expect=[(c, 1, B_BN_GRAD_RES, "none") for c in ALL] + [(c, 0, F_LAZY_RES, "none") for c in ALL]),
    _form("BN_MASK_FROM_Y=1", dict(BN_MASK_FROM_Y="1"), expect=[(c, 1, B_BN_GRAD, "none") for c in ALL] + [(c, 0, F_LAZY | F_LAZY_RES, "none") for c in ALL]),
    _form("FWD7=0,WGRAD7=0", dict(FWD7="0", WGRAD7="0"), expect=[(c, 0, F_PAIR, "none") for c in ALL] + [(c, 1, B_WPAIR, "none") for c in ALL] + [(c, 1, B_PAIR, "any") for c in NARROW]),
    _form("CONV6_PAIR=0", dict(CONV6_PAIR="0"), expect=[(c, 0, F_PAIR, "none") for c in ALL] + [(c, 1, B_PAIR | B_WPAIR | B_PAIR_BN, "none") for c in ALL]),
    _form("PREP_NARROW=1", dict(PREP_NARROW="1"), expect=DEFAULT_EXPECT),
    _form("WGRAD_DEFER=0", dict(WGRAD_DEFER="0"), expect=[(c, 1, B_WPAIR, "none") for c in ALL]),
    _form("cuts", {}, cuts=True, expect=[(c, 1, B_PAIR | B_WPAIR | B_PAIR_BN, "none") for c in ALL] + [(c, 1, B_BN_GRAD, "any") for c in NARROW]),
    # (one form more than the switch table of the issue: the only way to the write-through forward inside a plan)
    _form("BN_INPUT_WT=1", dict(BN_INPUT_WT="1", CONV8_MIN_TILES="1", CONV5_MIN_TILES="1"), cases=["wide-b3", "wide-b16"], expect=[("wide-b16", 0, F_WT, "any")]),
]
for extra in ([dict(DZ_BUFFERS=str(k)) for k in (2, 3, 4)] + [dict(BRANCH_STREAM=str(k)) for k in (0, 1, 2, 3)] +
              [dict(WGRAD_DEFER_SIDE="2"), dict(EVENT_RECORD="0"), dict(SIDE_PRIO="1")]):
    exp = [("wide-b16", 1, B_SIDE, "any")]
    if extra.get("BRANCH_STREAM") in ("1", "3"):
        exp.append(("wide-b16", 1, B_BRANCH, "any"))
    else:
        exp.append(("wide-b16", 1, B_BRANCH, "none"))
    exp.append(("wide-b16", 1, B_HOOK, "none" if "EVENT_RECORD" in extra else "any"))
    FORMS.append(_form("two-stream," + ",".join(f"{k}={v}" for k, v in extra.items()), dict(TWO, **extra), cases=["wide-b16"], expect=exp))


@pytest.fixture(scope="module", autouse=True)
def measure_table():
    yield
    for name in MEASURE:
        worst, where, secs, amb = MEASURE[name]
        print(f"\n[measure] {name:44s} err/bound {worst:.4f} ({where})   ambiguous share {amb:.2g}   child {secs:.1f} s", end="")
    print()


def _check_forms(form, forms):
    for case, word, bit, rule in form["expect"]:
        if case not in forms:
            continue
        words = [u[word] for u in forms[case]["train"]] if word in (0, 1) else forms[case]["eval"]
        hit = [i for i, w in enumerate(words) if w & bit]
        if rule == "any":
            assert hit, f"form {form['name']}: no unit of {case} took branch bit {bit} of word {word}: {words}"
        else:
            assert not hit, f"form {form['name']}: units {hit} of {case} took branch bit {bit} of word {word}, which this form switches off: {words}"


@pytest.mark.parametrize("form", FORMS, ids=[f["name"] for f in FORMS])
def test_form_unit_by_unit_against_fp64(form):
    assert _STATE["abnormal"] is None, f"not started: the child of {_STATE['abnormal']} ended abnormally"
    env = dict(os.environ, CLHIP_STAGE_TRAIN="0", CLHIP_STAGE_EVAL="0")
    for k, v in form["env"].items():
        env["CLHIP_" + k] = v
    args = [sys.executable, os.path.join(HERE, "plan_unit_worker.py"), form["dt"], ",".join(form["cases"])] + (["cuts"] if form["cuts"] else [])
    t0 = time.time()
    try:
        r = subprocess.run(args, env=env, capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired:
        _STATE["abnormal"] = form["name"]
        raise
    secs = time.time() - t0
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _STATE["abnormal"] = form["name"]
    line = lambda tag: json.loads([ln for ln in r.stdout.splitlines() if ln.startswith(tag + " ")][-1][len(tag) + 1:])
    assert r.returncode in (0, 1) and "RATIOS " in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    ratios, ambig, forms = line("RATIOS"), line("AMBIG"), line("FORMS")
    worst, where = max(((v, f"{c} {k}") for c, d in ratios.items() for k, v in d.items()), default=(0.0, ""))
    MEASURE[form["name"]] = (worst, where, secs, max(ambig.values()))
    for c in form["cases"]:
        print(f"[ratio] {form['name']} {c} " + " ".join(f"{k}={v:.3g}" for k, v in sorted(ratios[c].items())))
        print(f"[forms] {form['name']} {c} train {forms[c]['train']} eval {forms[c]['eval']}")
        assert {"z", "mean", "var", "y", "feat", "dy", "dw", "dgamma", "dbeta", "pass2 dw", "pass2 dy", "eval z", "eval y", "num_batches_tracked"} <= set(ratios[c]), ratios[c].keys()
    fails = [ln for ln in r.stdout.splitlines() if ln.startswith("FAIL ")]
    assert not fails, (form["name"], fails[:20])
    assert all(v <= 1.0 for d in ratios.values() for v in d.values()), ratios
    assert max(ambig.values()) <= 1e-4, ambig
    assert r.returncode == 0
    _check_forms(form, forms)
