"""Child process of tests/test_stage_eval_plan_gpu.py (a helper, not a test): the PLAN's side of the stage-level eval forward (csrc/plan.hip: the run selection,
the five pointer tables filled per run, the producers' lazy forms switched off for units that open a run), one case per process, CLHIP_STAGE_EVAL at its default.
usage: python stage_eval_worker.py CASE_ID
Build the net, apply plan_ref.trained_like, run ONE training forward on a different input (so every buffer holds stale values of the right shape), move the running
statistics away from (0, 1) as plan_unit_worker.py does, run the eval forward, then check:
  1. run selection: the activations debug_read refuses are exactly the inner activations of the runs expected from net._units by the rule stated in plan.hip
     (`expected_runs` below; nothing is read back from the plan);
  2. wiring, bit-equal: for every run its OUTPUT is read first, then its input (reading a lazily applied activation rebuilds it, so a run that consumed a stale,
     never-written input differs from the kernel's result on the rebuilt one); clhip_stage_eval on that input with the module's own parameters and running
     statistics (weight copies through clhip_conv_weight_prep) must return the plan's run output bit for bit;
  3. everything outside the runs (the stem, the down-sampling blocks, the shortcuts) against plan_ref.judge_eval;
  4. the features against the average pool of the last activation within bn_refs.bound_pool_fwd.
Last, a second eval forward with STAGE_EVAL = 0 reports which units take the consumer-side form without runs (the parent derives which must keep it with runs).
Prints `RUNS [[first unit, length], ...]`, `REFUSED {...}`, `WIRING [...]`, `RATIOS {...}`, `FORMS {"eval": [...], "eval_nostage": [...]}`, `SECONDS s`; exit status 1
when a check fails."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                              # noqa: E402

import bn_refs as B                       # noqa: E402
import plan_ref as PR                     # noqa: E402
import stage_ref as SR                    # noqa: E402

DEV = "cuda:0"
# case id -> (HipResNet arguments, image size, batch, dtype, the run lengths the issue expects, in unit order)
CASES = {
    "cifar20-b3": (dict(kind="cifar", depth=20), 32, 3, "bf16", [6, 4, 4]),
    "cifar32-b3": (dict(kind="cifar", depth=32), 32, 3, "bf16", [10, 8, 8]),                     # the product's net
    "cifar56-b2": (dict(kind="cifar", depth=56), 32, 2, "bf16", [16, 2, 16, 16]),                # stage 1 has 18 convolutions: the cap splits it into 16 + 2
    "mod14-b3": (dict(kind="modified", layers=[2, 2, 2]), 32, 3, "bf16", [4, 2]),                # no ReLU behind the last block: stage 3 has no run
    "pre14-b3": (dict(kind="preact", depth=14), 32, 3, "bf16", []),
    "wide-b3": (dict(kind="imagenet_style", layers=[1, 1, 1, 1]), 32, 3, "bf16", []),
    "cifar32-f32-b3": (dict(kind="cifar", depth=32), 32, 3, "f32", []),                          # the fused kernel is bf16 only
}


def expected_runs(units, dims, dt):
    """[(first unit, length)] by the rule of plan.hip: pairs (a, b) of 3x3 / stride-1 / pad-1 C -> C units with BatchNorm and ReLU on one map size, a on the block
    input without a residual, b on a's output with the block input as its residual, the next pair on b's output; at most 16 units per run; a geometry and type
    the kernel admits (stage_ref.GEOMS, bf16)"""
    runs, i, n = [], 0, len(units)
    while i + 1 < n:
        C, hw = units[i].cout, dims[units[i].src]
        s_in, ln = units[i].src, 0
        plain3 = lambda q: (q.k == 3 and q.stride == 1 and q.pad == 1 and q.cin == C and q.cout == C and C % 8 == 0 and dims[q.src] == hw and q.relu and
                            not q.flags & (PR.PRE_RES | PR.RAW_SRC | PR.NO_BN | PR.MAXPOOL))
        while i + ln + 1 < n and ln + 2 <= 16:
            a, b = units[i + ln], units[i + ln + 1]
            if not (plain3(a) and plain3(b) and a.res < 0 and a.src == s_in and b.src == i + ln + 1 and b.res == s_in):
                break
            ln += 2
            s_in = i + ln
        if ln >= 2 and dt == "bf16" and hw[0] == hw[1] and (C, hw[0]) in SR.GEOMS:
            runs.append((i, ln))
            i += ln
        else:
            i += 1
    return runs


def stage_call(xd, rows):
    """clhip_stage_eval on xd [N][H][W][C] bf16; rows: per convolution (weight [C, C, 3, 3], gamma, beta, running mean, running var) fp32 on the device"""
    from libcontinual_amd import _lib
    N, H, W, C = xd.shape
    st = torch.cuda.current_stream().cuda_stream
    keep = []
    for w, g, b, m, v in rows:
        master = w.detach().float().permute(0, 2, 3, 1).reshape(C, 9, C).contiguous()
        wf = torch.empty(C, 9, C, dtype=torch.bfloat16, device=DEV)
        _lib.call("clhip_conv_weight_prep", master.data_ptr(), wf.data_ptr(), None, C, 9, C, C, _lib.BF16, st)
        keep.append((wf,) + tuple(t.detach().float().contiguous() for t in (g, b, m, v)) + (master,))
    tabs = [(ctypes.c_void_p * len(rows))(*[k[j].data_ptr() for k in keep]) for j in range(5)]
    y = torch.full_like(xd, float("nan"))
    _lib.call("clhip_stage_eval", xd.data_ptr(), y.data_ptr(), N, H, W, C, len(rows), *tabs, B.EPS, _lib.BF16, st)
    torch.cuda.synchronize()
    return y


def main():
    from libcontinual_amd import _lib
    from libcontinual_amd._lib import ClhipError
    from libcontinual_amd.model.backbone.resnet import HipResNet
    name = sys.argv[1]
    kw, hw, N, dt, _ = CASES[name]
    t0 = time.time()
    ok = True
    net = HipResNet(dtype=dt, **kw)
    units = [PR.PU(u.cin, u.cout, u.k, u.stride, u.pad, u.src, u.res, bool(u.relu), int(u.flags)) for u in net._units]
    n = len(units)
    dims = net._act_dims(hw, hw)
    pw = net._pool_win
    lh, lw = dims[n]
    feat_dim = units[-1].cout * (lh // pw) * (lw // pw) if pw else units[-1].cout
    x, P, _ = PR.trained_like(units, 4321 + 17 * N + n, N, hw, feat_dim)
    named = dict(net.named_parameters())
    with torch.no_grad():
        for i, u in enumerate(net._units):
            named[u.conv + ".weight"].copy_(P["w"][i])
            if u.bn is not None:
                named[u.bn + ".weight"].copy_(P["gamma"][i])
                named[u.bn + ".bias"].copy_(P["beta"][i])
    net = net.to(DEV).train()
    net._ensure_flat(torch.device(DEV))
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        net(2.0 * torch.randn(x.shape, generator=g).to(DEV))                   # a training forward on ANOTHER input: stale values of the right shape everywhere
    net._stats.copy_((0.3 * torch.randn(net._nstat, generator=g)).to(DEV))
    for nm, shp, o in net._stat_layout:
        if nm.endswith("running_var"):
            net._stats[o:o + shp[0]].copy_((0.5 + torch.rand(shp[0], generator=g)).to(DEV))
    net.eval()
    xd = x.to(DEV)
    with torch.no_grad():
        out = net(xd)
    feat = (out if torch.is_tensor(out) else out["features"]).detach().double()
    torch.cuda.synchronize()
    forms = [f for f, _ in net.debug_unit_forms()]
    named, bufs = dict(net.named_parameters()), dict(net.named_buffers())
    runs = expected_runs(units, dims, dt)
    print("RUNS " + json.dumps(runs), flush=True)
    in_run = {i + k for i, ln in runs for k in range(ln)}
    inner = {i + 1 + k for i, ln in runs for k in range(ln - 1)}              # activation indices (unit + 1) that were never written
    # ---- 2. wiring, first: the output of every run, then its input
    Y, wiring = {}, []
    for i, ln in runs:
        Y[i + ln] = net.debug_read(i + ln, 0)
        a_in = units[i].src
        Y[a_in] = net.debug_read(a_in, 0)
        us = net._units[i:i + ln]
        rows = [(named[u.conv + ".weight"], named[u.bn + ".weight"], named[u.bn + ".bias"], bufs[u.bn + ".running_mean"], bufs[u.bn + ".running_var"]) for u in us]
        got = stage_call(Y[a_in].permute(0, 2, 3, 1).contiguous().to(torch.bfloat16), rows)
        want = Y[i + ln].permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
        assert bool((want.float() == Y[i + ln].permute(0, 2, 3, 1)).all())     # (a bf16 plan: the fp32 copy holds bf16 values)
        diff = 0 if B.same_bits(got, want) else int(((got.double() != want.double()) | ~torch.isfinite(got.double())).sum())
        wiring.append([i, ln, diff])
        ok = ok and diff == 0
    print("WIRING " + json.dumps(wiring), flush=True)
    # ---- 1. the refused set
    refused, other = set(), []
    for a in range(1, n + 1):
        try:
            t = net.debug_read(a, 0) if PR.has_bn(units[a - 1]) else None
            if t is not None:
                Y[a] = t
        except ClhipError as e:
            if "as one launch (stage.hip)" in str(e):
                refused.add(a)
            else:
                other.append([a, str(e)[:200]])
    torch.cuda.synchronize()
    print("REFUSED " + json.dumps(dict(got=sorted(refused), expected=sorted(inner), other=other)), flush=True)
    ok = ok and refused == inner and not other
    # ---- 3. everything outside the runs, 4. the features
    outside = [i for i in range(n) if i not in in_run]
    E = dict(x=net.debug_read(0)[:, :units[0].cin].double(), z=[None] * n, y=[None] * n)
    E["w"] = [named[u.conv + ".weight"].detach().double().contiguous() for u in net._units]
    for k, sfx in (("gamma", ".weight"), ("beta", ".bias")):
        E[k] = [None if u.bn is None else named[u.bn + sfx].detach().double().contiguous() for u in net._units]
    E["rm"] = [None if u.bn is None else bufs[u.bn + ".running_mean"].double() for u in net._units]
    E["rv"] = [None if u.bn is None else bufs[u.bn + ".running_var"].double() for u in net._units]
    for a, t in Y.items():
        if a >= 1:
            E["y"][a - 1] = t.double()
    for i in outside:
        E["z"][i] = net.debug_read(i + 1, 3 if units[i].flags & PR.MAXPOOL else 1).double()
    V = PR.judge_eval(units, E, dt, only=set(outside))
    ratios = V.worst_by_link()
    for k, v in V.failures().items():
        print(f"FAIL {name} {k}: {v:.4g}", flush=True)
    ylast = E["y"][n - 1]
    hwp = pw * pw if pw else ylast.shape[2] * ylast.shape[3]
    reff = PR.feat_of(ylast, pw)
    ratios["eval feat"] = SR.ratio(feat, reff, B.bound_pool_fwd(PR.feat_of(ylast.abs(), pw) * hwp, hwp, reff))
    ratios["units judged"] = float(len(outside))
    print("RATIOS " + json.dumps(ratios), flush=True)
    ok = ok and all(v <= 1.0 for k, v in ratios.items() if k != "units judged")
    # ---- the forms without runs (after every check: the checks saw the default)
    L = _lib.lib()
    assert L.clhip_config(b"STAGE_EVAL", b"0") == 0
    try:
        with torch.no_grad():
            net(xd)
        torch.cuda.synchronize()
        forms0 = [f for f, _ in net.debug_unit_forms()]
    finally:
        L.clhip_config(b"STAGE_EVAL", None)
    print("FORMS " + json.dumps(dict(eval=forms, eval_nostage=forms0, src=[u.src for u in units])), flush=True)
    print("SECONDS " + json.dumps(round(time.time() - t0, 2)), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
