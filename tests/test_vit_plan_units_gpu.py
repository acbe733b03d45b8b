"""The ViT executor (csrc/vit_plan.hip) held to fp64 launch by launch on a real MI355X, in every form its switches select: tests/vit_plan_ref.py judges every
stored tensor of a training step (the weight copies, patches, tokens, per layer the LN statistics, h1, qkv, lse, the attention output, x_mid, the GELU derivative,
the adapter's hidden rows, the block output; feat; the Gram matrices; every buffer of the backward chain through the gradient tap; every parameter gradient)
against what fp64 makes of the executor's own stored inputs of that launch.  The parent process never flips a switch (WGRAD_STREAM, ATTN_GENERIC and the GEMM
route switches are cached at their first use): every form runs in a fresh child (tests/vit_unit_worker.py) with its switches as CLHIP_<NAME> in the environment.
Children run one at a time, each under its own timeout; after one that timed out or ended abnormally no other child is started.  The module prints one
`[measure]` line per form at its end (pytest -s); profiles/vit_units.md holds the table of an MI355X run.

No leaf kernel sums with atomics (clhip_lora_grad, clhip_sdlora_grad, clhip_lora_grad_ab, clhip_adapter_wgrad and the prefix attention backward reduce slab
partials in order), so
the two-stream and the one-stream backward must agree bitwise on every tap and every parameter gradient, and so must the captured backward and the eager one."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

import gemm_ref as G                      # noqa: E402
import vit_plan_ref as VP                 # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURE, RESULTS = {}, {}
_STATE = {"abnormal": None}

ALL = [VP.case_id(c) for c in VP.CASES]
# the modes whose leaves may run on the side stream; the first CAPTURED of them also run under stream capture
LEAVES = ["t64-lora", "t64-sdlora", "t128-lora", "t128-sdlora", "t64-lora_ab", "t128-lora_ab", "d1-lora"]
CAPTURED = 6
SIDE_MODES = ("lora", "sdlora", "lora_ab")


def _form(name, env, dt, cases, capture=False, side="default", routes=None):
    """side: 'default' = the side stream exactly in the LoRA, SD-LoRA and LoRA-Sub cases, 'never'; routes: the GEMM family every bf16 GEMM of the cases must take"""
    return dict(name=name, env=env, dt=dt, cases=cases, capture=capture, side=side, routes=routes)


FORMS = [
    _form("default-bf16", {}, "bf16", ALL, routes=G.T64),
    _form("default-f32", {}, "f32", ALL, routes=G.F32_128),
    _form("WGRAD_STREAM=0-bf16", dict(WGRAD_STREAM="0"), "bf16", LEAVES, side="never"),
    _form("WGRAD_STREAM=0-f32", dict(WGRAD_STREAM="0"), "f32", LEAVES, side="never"),
    # (fp32 attention is the generic kernel in every form: the switch only moves the bf16 head-dim-64 calls)
    _form("ATTN_GENERIC=1-bf16", dict(ATTN_GENERIC="1"), "bf16", ["t128-lora", "t128-prefix", "t128-prefix_prompt"]),
    _form("capture-bf16", {}, "bf16", LEAVES[:CAPTURED], capture=True, side="never"),
    _form("capture-f32", {}, "f32", LEAVES[:CAPTURED], capture=True, side="never"),
    # the GEMM route switches that move these shapes (all of them take the 64 x 64 tiles by default; fp32 has one kernel): GEMM_MT forces the tile
    _form("GEMM_MT=4-bf16", dict(GEMM_MT="4"), "bf16", ["t64-lora", "t128-adapter"], routes=G.T128),
    _form("GEMM_MT=5-bf16", dict(GEMM_MT="5"), "bf16", ["t64-lora"], routes=G.T160),
    _form("GEMM_MT=8-bf16", dict(GEMM_MT="8"), "bf16", ["t64-lora"], routes=G.T256),
]


@pytest.fixture(scope="module", autouse=True)
def measure_table():
    yield
    for name in MEASURE:
        worst, where, secs = MEASURE[name]
        print(f"\n[measure] {name:24s} err/bound {worst:.4f} ({where})   child {secs:.1f} s", end="")
    print()


@pytest.mark.parametrize("form", FORMS, ids=[f["name"] for f in FORMS])
def test_form_launch_by_launch_against_fp64(form):
    assert _STATE["abnormal"] is None, f"not started: the child of {_STATE['abnormal']} ended abnormally"
    env = dict(os.environ)
    for k in ("WGRAD_STREAM", "ATTN_GENERIC", "GEMM_MT", "GEMM8", "GEMM_SPLITK", "GEMM_TAIL", "GEMM_NO_SPLIT", "ATTN_BWD", "ADAPTER_TM"):
        env.pop("CLHIP_" + k, None)
    for k, v in form["env"].items():
        env["CLHIP_" + k] = v
    args = [sys.executable, os.path.join(HERE, "vit_unit_worker.py"), form["dt"], ",".join(form["cases"])] + (["capture"] if form["capture"] else [])
    t0 = time.time()
    try:
        r = subprocess.run(args, env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _STATE["abnormal"] = form["name"]
        raise
    secs = time.time() - t0
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _STATE["abnormal"] = form["name"]
    line = lambda tag: json.loads([ln for ln in r.stdout.splitlines() if ln.startswith(tag + " ")][-1][len(tag) + 1:])
    assert r.returncode in (0, 1) and "RATIOS " in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    ratios, info, bits, routes = line("RATIOS"), line("INFO"), line("BITS"), line("ROUTES")
    RESULTS[form["name"]] = bits
    worst, where = max(((v, f"{c} {k}") for c, d in ratios.items() for k, v in d.items()), default=(0.0, ""))
    MEASURE[form["name"]] = (worst, where, secs)
    for c in form["cases"]:
        print(f"[ratio] {form['name']} {c} " + " ".join(f"{k}={v:.3g}" for k, v in sorted(ratios[c].items())))
        links = {k.split(" ", 1)[1] for k in ratios[c]}
        assert {"patches", "pe_out", "x0", "ln1 mean", "ln1 rstd", "qkv", "attn_o", "lse", "x_mid", "ln2 mean", "ln2 rstd", "hpre", "x_out", "feat", "gram", "g0", "dbig", "dfc1",
                "g_ln2", "dproj", "dq", "dk", "dv"} <= links, (c, sorted(links))
        mode = c.split("-", 1)[1]
        need = dict(lora={"h1", "d_lora_b k", "d_lora_b v"}, prompt={"dprompt", "dqin", "g_ln1"}, adapter={"ad_hd", "ad_dh", "ad_gx", "d_adapter dWd", "d_adapter dbu"},
                    adapter_drop={"ad_hd", "ad_dh", "ad_gx", "d_adapter dWu", "d_adapter dbd"}, sdlora={"h1", "d_sd dAq", "d_sd dBv", "d_sd dmag row", "d_mag"},
                    prefix={"dpk", "dpv"}, prefix_prompt={"dpk", "dpv", "dprompt"}, lora_ab={"h1", "d_ab dAk", "d_ab dBk", "d_ab dAv", "d_ab dBv"})[mode]
        assert need <= links, (c, sorted(need - links))
        for s, d in info[c].items():
            want_side = 1 if (form["side"] == "default" and mode in SIDE_MODES) else 0
            assert d["side"] == want_side, (c, s, d)
        if mode == "prefix" and not c.startswith("d1"):
            assert info[c]["s0"]["lowest"] == 1 and info[c]["s1"]["lowest"] == 1 and info[c]["s1"]["lowest_with_dprompt"] == 0, info[c]
        if form["routes"] is not None:
            assert all(fam == [form["routes"]] for fam in routes[c].values()), (c, routes[c])
    fails = [ln for ln in r.stdout.splitlines() if ln.startswith("FAIL ")]
    assert not fails, (form["name"], fails[:20])
    assert all(v <= 1.0 for d in ratios.values() for v in d.values()), ratios
    assert r.returncode == 0


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_two_streams_and_one_stream_agree_bitwise(dt):
    """every tap and every parameter gradient of the LoRA / SD-LoRA / LoRA-Sub cases: the side stream changes the order of launches, never a bit of a result"""
    two, one = RESULTS.get(f"default-{dt}"), RESULTS.get(f"WGRAD_STREAM=0-{dt}")
    assert two is not None and one is not None, "the forms this comparison needs did not run"
    for c in LEAVES:
        assert two[c] == one[c], (c, two[c], one[c])


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_captured_backward_equals_the_eager_one_stream_backward(dt):
    """the backward under stream capture (single stream, no fork / join) and one replay against the eager WGRAD_STREAM=0 run"""
    cap, one = RESULTS.get(f"capture-{dt}"), RESULTS.get(f"WGRAD_STREAM=0-{dt}")
    assert cap is not None and one is not None, "the forms this comparison needs did not run"
    for c in LEAVES[:CAPTURED]:
        assert cap[c] == one[c], (c, cap[c], one[c])
