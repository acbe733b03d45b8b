"""Child process of tests/test_plan_units_gpu.py (a helper, not a test): ONE form of the plan executor, its CLHIP_<NAME> switches set by the parent in this
process's environment (most are cached at their first use, so no in-process test can flip them).
usage: python plan_unit_worker.py DTYPE CASE_ID[,CASE_ID...] [CUTS]
For every case, in the order given: build the net, zero the running statistics, apply plan_ref.trained_like, run forward + backward twice (the second pass
without zeroing the gradients; with CUTS the backward goes through clhip_plan_backward_range at `_grad_segment_cuts`), read every stored tensor after
each pass and judge it with plan_ref.judge on the device; then an eval forward on running statistics moved away from (0, 1) against plan_ref.judge_eval.
Prints one line `RATIOS {case: {link: worst err / bound}}`, one `AMBIG {case: share}`, one `FORMS {case: {"train": [[fwd, bwd] per unit], "eval": [...]}}`
and one `SECONDS {case: s}`; exit status 1 when a link is outside its bound."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                              # noqa: E402

import plan_ref as PR                     # noqa: E402

DEV = "cuda:0"


def read_pass(net, units, xd, dfeat, feat, old):
    n = len(units)
    named, bufs = dict(net.named_parameters()), dict(net.named_buffers())
    D = dict(x=net.debug_read(0)[:, :units[0].cin].double(), z=[None] * n, y=[None] * n, dy=[None] * n, feat=feat.detach().double(), dfeat=dfeat.double())
    for i, u in enumerate(units):
        D["z"][i] = net.debug_read(i + 1, 3 if u.flags & PR.MAXPOOL else 1).double()
        if PR.has_bn(u):
            D["y"][i], D["dy"][i] = net.debug_read(i + 1, 0).double(), net.debug_read(i + 1, 2).double()
    us = net._units
    par = lambda nm: named[nm].detach().double().contiguous()
    grad = lambda nm: named[nm].grad.detach().double().contiguous().clone()
    D["w"], D["gw"] = [par(u.conv + ".weight") for u in us], [grad(u.conv + ".weight") for u in us]
    for k, sfx, src in (("gamma", ".weight", par), ("beta", ".bias", par), ("ggamma", ".weight", grad), ("gbeta", ".bias", grad)):
        D[k] = [None if u.bn is None else src(u.bn + sfx) for u in us]
    D["rm"] = [None if u.bn is None else bufs[u.bn + ".running_mean"].double().clone() for u in us]
    D["rv"] = [None if u.bn is None else bufs[u.bn + ".running_var"].double().clone() for u in us]
    for k in ("gw", "ggamma", "gbeta"):
        D[k + "0"] = [None if t is None else (torch.zeros_like(t) if old is None else old[k][i]) for i, t in enumerate(D[k])]
    nbt = [int(bufs[u.bn + ".num_batches_tracked"]) for u in us if u.bn is not None]
    return D, nbt


def run_case(name, N, dt, cuts):
    net = PR.build_net(name, dt)
    units = [PR.PU(u.cin, u.cout, u.k, u.stride, u.pad, u.src, u.res, bool(u.relu), int(u.flags)) for u in net._units]
    hw = PR.NETS[name][1]
    lh, lw = net._act_dims(hw, hw)[len(units)]
    pw = net._pool_win
    feat_dim = units[-1].cout * (lh // pw) * (lw // pw) if pw else units[-1].cout
    x, P, dfeat = PR.trained_like(units, 1234 + 17 * N + len(units), N, hw, feat_dim)
    named = dict(net.named_parameters())
    with torch.no_grad():
        for i, u in enumerate(net._units):
            named[u.conv + ".weight"].copy_(P["w"][i])
            if u.bn is not None:
                named[u.bn + ".weight"].copy_(P["gamma"][i])
                named[u.bn + ".bias"].copy_(P["beta"][i])
    net = net.to(DEV).train()
    net._ensure_flat(torch.device(DEV))
    xd, dfd = x.to(DEV), dfeat.to(DEV)
    if cuts:
        # cuts inside a block, and between a shortcut unit and its 3x3 partner (the pair then falls back to two launches)
        sc = [i for i, u in enumerate(units) if u.k == 1]
        net._grad_segment_cuts = sorted({c for c in [len(units) - 1] + sc + [s + 1 for s in sc] if 0 < c < len(units)}, reverse=True)
        net._grad_segment_hook = lambda *a: None
    ratios, ambig, old = {}, 0.0, None
    for p in range(2):
        net._stats.zero_()
        net._nbt.zero_()
        out = net(xd)
        feat = out if torch.is_tensor(out) else out["features"]
        feat.backward(dfd)
        torch.cuda.synchronize()
        D, nbt = read_pass(net, units, xd, dfd, feat, old)
        if p == 1:
            forms = net.debug_unit_forms()
        V = PR.judge(units, D, dt, pw, nbt=(1, nbt))
        for k, v in V.worst_by_link().items():
            key = k if p == 0 else "pass2 " + k
            ratios[key] = max(ratios.get(key, 0.0), v)
        for k, v in V.failures().items():
            print(f"FAIL {name}-b{N} pass {p + 1} {k}: {v:.4g}", flush=True)
        ambig = max(ambig, max(V.ambig.values()))
        old = D
    # ---- the eval forward, per unit, on running statistics away from (0, 1)
    g = torch.Generator().manual_seed(99)
    net._stats.copy_((0.3 * torch.randn(net._nstat, generator=g)).to(DEV))
    for nm, shp, o in net._stat_layout:
        if nm.endswith("running_var"):
            net._stats[o:o + shp[0]].copy_((0.5 + torch.rand(shp[0], generator=g)).to(DEV))
    net.eval()
    with torch.no_grad():
        net(xd)
    torch.cuda.synchronize()
    eforms = net.debug_unit_forms()
    bufs = dict(net.named_buffers())
    E = dict(x=D["x"], w=D["w"], gamma=D["gamma"], beta=D["beta"], z=[None] * len(units), y=[None] * len(units))
    E["rm"] = [None if u.bn is None else bufs[u.bn + ".running_mean"].double() for u in net._units]
    E["rv"] = [None if u.bn is None else bufs[u.bn + ".running_var"].double() for u in net._units]
    for i, u in enumerate(units):
        if PR.has_bn(u):                   # (y first: reading a consumer-side activation rebuilds it from z)
            E["y"][i] = net.debug_read(i + 1, 0).double()
        E["z"][i] = net.debug_read(i + 1, 3 if u.flags & PR.MAXPOOL else 1).double()
    VE = PR.judge_eval(units, E, dt)
    ratios.update(VE.worst_by_link())
    for k, v in VE.failures().items():
        print(f"FAIL {name}-b{N} {k}: {v:.4g}", flush=True)
    return ratios, ambig, dict(train=forms, eval=[f for f, _ in eforms])


def main():
    dt = sys.argv[1]
    cases = [c for c in PR.CASES if PR.case_id(c) in sys.argv[2].split(",")]
    cuts = len(sys.argv) > 3 and sys.argv[3] == "cuts"
    assert cases
    R, A, Fm, S = {}, {}, {}, {}
    for name, N in cases:
        t0 = time.time()
        R[f"{name}-b{N}"], A[f"{name}-b{N}"], Fm[f"{name}-b{N}"] = run_case(name, N, dt, cuts)
        S[f"{name}-b{N}"] = round(time.time() - t0, 2)
    print("RATIOS " + json.dumps(R))
    print("AMBIG " + json.dumps(A))
    print("FORMS " + json.dumps(Fm))
    print("SECONDS " + json.dumps(S))
    bad = any(not v <= 1.0 for r in R.values() for v in r.values()) or any(a > 1e-4 for a in A.values())
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
