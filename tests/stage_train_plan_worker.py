"""Child process of tests/test_stage_train_plan_gpu.py (a helper, not a test): the FORWARD of a plan whose training passes run as stage-level launches
(csrc/stage_train.hip; CLHIP_STAGE_TRAIN=1 and the form's switches set by the parent in this process's environment), judged unit by unit by plan_ref.judge in its
forward-only mode: z of every unit from its stored input, the batch statistics recovered from the running statistics, y (an activation inside a run is rebuilt by
the read from its z and coefficients), feat -- with the pooling inside the last run's launch or behind it.  The backward runs too, so that its launches are counted;
the gradients inside a run never leave LDS.
With `bwd` the BACKWARD is judged per run instead: from dfeat (the last run) or the stored dy at the run's output, a chain of stage_train_ref.judge_bwd blocks from
the run's last block to its first -- the unseen dx of a block, as (reference, bound), is the dy of the block in front -- with the batch statistics recovered from
the running statistics (plan_ref.recover and its error terms): dw, dgamma, dbeta of every unit of the run and the stored dy of the activation in front of it.
The runs are found from the unit list: pairs of 3x3 / stride-1 units that form BasicBlocks, and (unless CLHIP_STAGE_ENTRY=0) the down-sampling block in front.
usage: python stage_train_plan_worker.py CASE_ID[,CASE_ID...] [bwd]
Prints `RATIOS {case: {link: worst err / bound}}` and `INFO {case: [units inside runs, forward launches, backward launches, status word]}`; exit status 1 when a
link is outside its bound."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                              # noqa: E402

import bn_refs as B                       # noqa: E402
import plan_ref as PR                     # noqa: E402
import stage_train_ref as SR              # noqa: E402

DEV = "cuda:0"


def runs_of(units, entry_on):
    """the runs as lists of blocks, a block = its unit indices in table order.  Unit j writes activation j + 1; `src` / `res` are activation indices."""
    n = len(units)
    c3 = lambda u, s: u.k == 3 and u.stride == s and u.pad == 1 and u.relu          # (a block whose output has no ReLU -- the last one of `mod14` -- is no part of a run)
    def plain(i):
        return (i + 1 < n and c3(units[i], 1) and c3(units[i + 1], 1) and units[i].cin == units[i].cout == units[i + 1].cout and units[i].src == i and units[i].res < 0
                and units[i + 1].src == i + 1 and units[i + 1].res == i)
    def entry(i):
        return (i + 2 < n and c3(units[i], 2) and units[i + 1].k == 1 and units[i + 1].stride == 2 and not units[i + 1].relu and units[i + 1].src == units[i].src == i and c3(units[i + 2], 1)
                and units[i + 2].src == i + 1 and units[i + 2].res == i + 2)
    runs, i = [], 0
    while i < n:
        head = [[i, i + 1, i + 2]] if entry(i) else []
        j = i + 3 if head else i
        blocks = []
        while plain(j):
            blocks.append([j, j + 1])
            j += 2
        if blocks:
            runs.append((head if entry_on else []) + blocks)
        i = max(j, i + 1)
    return runs


def judge_runs(net, units, D, dfd, N):
    named = dict(net.named_parameters())
    grad = lambda nm: named[nm].grad.detach().double().contiguous()
    n = len(units)
    rec = []
    for i in range(n):
        zt = PR.mc(D["z"][i])
        M = zt.shape[0]
        noise = B.var_noise(zt.sum(0), (zt * zt).sum(0), M)
        mean, var, e_mean, e_var = PR.recover(D["rm"][i], D["rv"][i], M, noise)
        rec.append((mean, 1.0 / torch.sqrt(var + B.EPS), e_mean, 0.5 * (e_var + noise) / (var + B.EPS) + B.E_ISTD["rsqrt"] * B.U))
    V = SR.Verdict()
    for run in runs_of(units, os.environ.get("CLHIP_STAGE_ENTRY") != "0"):
        last = run[-1][-1]
        top = dict(dfeat=dfd.double()) if last == n - 1 else dict(dy=net.debug_read(last + 2 - 1, 2).double())
        bdy = None
        for b in range(len(run) - 1, -1, -1):
            blk = run[b]
            us = net._units
            rows = [dict(w=D["w"][i], gamma=D["gamma"][i], beta=D["beta"][i], dg0=torch.zeros_like(D["gamma"][i]), db0=torch.zeros_like(D["gamma"][i]),
                         k=units[i].k, s=units[i].stride, p=units[i].pad) for i in blk]
            src = units[blk[0]].src
            x = D["x"] if src == 0 else D["y"][src - 1]
            T = dict(z=[D["z"][i] for i in blk], y=[D["y"][i] for i in blk], mean=[rec[i][0] for i in blk], invstd=[rec[i][1] for i in blk])
            O = dict(dgamma=[grad(us[i].bn + ".weight") for i in blk], dbeta=[grad(us[i].bn + ".bias") for i in blk], slab=[grad(us[i].conv + ".weight")[None] for i in blk],
                     dx=net.debug_read(src, 2).double() if b == 0 else None, dz=None)
            SR.judge_bwd(x, rows, len(blk) == 3, T, O, ipg=N, ipg_entry=N, bdy=bdy, stat_err=[(rec[i][2], rec[i][3]) for i in blk], V=V, tag=f"u{blk[0]}:", **top)
            ref, bdy = V.dx
            top = dict(dy=ref)
    return V


def run_case(name, N, bwd=False):
    from libcontinual_amd import _lib
    net = PR.build_net(name, "bf16")
    units = [PR.PU(u.cin, u.cout, u.k, u.stride, u.pad, u.src, u.res, bool(u.relu), int(u.flags)) for u in net._units]
    hw = PR.NETS[name][1]
    x, P, dfeat = PR.trained_like(units, 4321 + 17 * N + len(units), N, hw, units[-1].cout)
    named = dict(net.named_parameters())
    with torch.no_grad():
        for i, u in enumerate(net._units):
            named[u.conv + ".weight"].copy_(P["w"][i])
            named[u.bn + ".weight"].copy_(P["gamma"][i])
            named[u.bn + ".bias"].copy_(P["beta"][i])
    net = net.to(DEV).train()
    net._ensure_flat(torch.device(DEV))
    xd, dfd = x.to(DEV), dfeat.to(DEV)
    net._stats.zero_()
    net._nbt.zero_()
    out = net(xd)
    feat = out if torch.is_tensor(out) else out["features"]
    feat.backward(dfd)
    torch.cuda.synchronize()
    n = len(units)
    named, bufs = dict(net.named_parameters()), dict(net.named_buffers())
    D = dict(x=net.debug_read(0)[:, :units[0].cin].double(), z=[None] * n, y=[None] * n, feat=feat.detach().double(), dfeat=dfd.double())
    for i in range(n):
        D["z"][i] = net.debug_read(i + 1, 1).double()
        D["y"][i] = net.debug_read(i + 1, 0).double()
    par = lambda nm: named[nm].detach().double().contiguous()
    D["w"] = [par(u.conv + ".weight") for u in net._units]
    D["gamma"], D["beta"] = [par(u.bn + ".weight") for u in net._units], [par(u.bn + ".bias") for u in net._units]
    D["rm"] = [bufs[u.bn + ".running_mean"].double().clone() for u in net._units]
    D["rv"] = [bufs[u.bn + ".running_var"].double().clone() for u in net._units]
    V = judge_runs(net, units, D, dfd, N) if bwd else PR.judge(units, D, "bf16", net._pool_win, forward_only=True)
    amb = max(V.ambig.values(), default=0.0)
    if amb > B.AMBIG_CAP:
        print(f"FAIL {name}-b{N} ambiguous share {amb:.3g}", flush=True)
    for k, v in V.failures().items():
        print(f"FAIL {name}-b{N} {k}: {v:.4g}", flush=True)
    L = _lib.lib()
    plans = [p for p, _ in net._handle.plans.values()]
    info = [sum(int(L.clhip_plan_stage_info(p, w)) for p in plans) for w in (0, 1, 2)] + [max(int(L.clhip_plan_stage_status(p)) for p in plans)]
    return V.worst_by_link(), info


def main():
    cases = [c for c in PR.CASES + [("cifar14", 72), ("mod14", 72)] if PR.case_id(c) in sys.argv[1].split(",")]
    assert cases
    R, I = {}, {}
    bwd = len(sys.argv) > 2 and sys.argv[2] == "bwd"
    for name, N in cases:
        R[f"{name}-b{N}"], I[f"{name}-b{N}"] = run_case(name, N, bwd)
    print("RATIOS " + json.dumps(R))
    print("INFO " + json.dumps(I))
    sys.exit(1 if any(not v <= 1.0 for r in R.values() for v in r.values()) else 0)


if __name__ == "__main__":
    main()
