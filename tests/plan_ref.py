"""Teacher-forced fp64 reference of the ResNet plan executor (csrc/plan.hip: clhip_plan_forward[_ex], clhip_plan_backward[_range]) -- a helper module, not a
conftest.  Plain torch fp64 on whatever device the tensors live on; the project is imported only for `HipResNet._units` (units_of).

The idea.  A plan keeps every link of the chain  x -> z_1 -> y_1 -> ... -> feat  and  dfeat -> dy_last -> ... -> dy_1, dw, dgamma, dbeta  in a readable
buffer.  `judge` takes ONE read of all of them (a dict, see `emulate` for its keys; everything in it is already in storage precision) and computes, per unit,
what each stored output must be FROM THE PLAN'S OWN STORED INPUTS of that link, with an allowed error per element.  A wiring fault (a wrong accumulate flag,
a mask from the wrong activation, sums taken too early, a stale operand) then breaks exactly one link by far more than a rounding bound, instead of hiding
in the 30 % end-to-end tolerance of a bf16 gradient.  Every bound is composed from the rules of tests/conv_ref.py and tests/bn_refs.py (the counts are
theirs); nothing is fitted to a kernel's output; a verdict is max over the elements of err / bound <= 1.

The saved batch statistics are not readable, but every BatchNorm of a test starts from running_mean = running_var = 0, so after ONE training forward
mean_b = running_mean / momentum and var_unbiased = running_var / momentum (`recover`, bounded by bn_refs.bound_running).  All BatchNorm references below
are functions of those recovered values, as bn_refs requires ("a function of the kernel's saved values").

Ambiguous elements.  Where |pre-ReLU value| lies inside the fp32 part of the forward bound either ReLU mask is right (likewise a max-pool window whose two
best candidates are that close).  bn_refs.err_ratio admits the error against EITHER reference there; here the unseen dz of a unit feeds further links, so
the same admission is carried as a per-element widening of the bound by |alt - ref| on exactly those elements (zero elsewhere), which then propagates
through the dgrad / wgrad magnitude products like any other term.  The share of such elements is returned and capped by bn_refs.AMBIG_CAP.

Summation chains.  The channel sums of the BatchNorm backward are reduced by different launches in different forms (reduce kernels, dgrad / pooling
epilogues, the fused pair): the bound takes d = M, "any summation order of M fp32 terms", the argument of conv_ref.acc_bound; a dgrad epilogue sums the
UNROUNDED dx where the reference sums the stored dy, which adds sum r |dy| (|xhat|) in the bf16 mode (r = 2^-8, the unit roundoff of bf16).  The fused down-sampling pair adds its two input
gradients in fp32 and rounds once; the reference counts one storage rounding per write, which contains it."""
import collections
import math

import torch
import torch.nn.functional as F

import bn_refs as B
import conv_ref as CR

PRE_RES, RAW_SRC, NO_BN, MAXPOOL = 2, 4, 8, 16          # include/clhip.h: CLHIP_UNIT_*
PU = collections.namedtuple("PU", "cin cout k stride pad src res relu flags")

# ------------------------------------------------------------------------------------------------ the case list
NETS = {
    "cifar14": (dict(kind="cifar", depth=14), 32),
    "mod14": (dict(kind="modified", layers=[2, 2, 2]), 32),
    "pre14": (dict(kind="preact", depth=14), 32),
    "wide": (dict(kind="imagenet_style", layers=[1, 1, 1, 1]), 32),
    "stem3": (dict(kind="imagenet_style", layers=[1, 1, 1, 1], stem="imagenet3"), 32),
    "stem7": (dict(kind="imagenet_style", layers=[1, 1, 1, 1], stem="imagenet7"), 64),
}
CASES = [("cifar14", 5), ("cifar14", 36), ("mod14", 5), ("pre14", 6), ("wide", 3), ("wide", 16), ("stem3", 3), ("stem7", 3)]
SMALLEST = [("cifar14", 5), ("mod14", 5), ("pre14", 6), ("wide", 3), ("stem3", 3), ("stem7", 3)]
FAULTS = ["drop_res", "dx_overwrite", "mask_other", "sums_early", "biased_var", "no_shortcut_dgrad", "wgrad_from_z", "wrong_gamma"]


def case_id(c):
    return f"{c[0]}-b{c[1]}"


def build_net(name, dtype=None):
    """the HipResNet of a case (the only place the project is imported)"""
    from libcontinual_amd.model.backbone.resnet import HipResNet
    return HipResNet(dtype=dtype, **NETS[name][0])


def units_of(name):
    net = build_net(name, "f32")
    return [PU(u.cin, u.cout, u.k, u.stride, u.pad, u.src, u.res, bool(u.relu), int(u.flags)) for u in net._units], net._pool_win


def trained_like(units, seed, N, hw, feat_dim):
    """seeded x, dfeat and parameters of a net that has trained for a while: conv N(0, sqrt(2 / (k k cout))), gamma = 1 + 0.3 randn with at least one
    negative gamma per unit, beta = 0.2 randn; the first residual unit has a channel with gamma = 0, beta < 0 and one with gamma = 0, beta > 0"""
    g = torch.Generator().manual_seed(seed)
    P = dict(w=[], gamma=[], beta=[])
    special = next(i for i, u in enumerate(units) if u.res >= 0 and not u.flags & NO_BN)
    for i, u in enumerate(units):
        P["w"].append(torch.randn(u.cout, u.cin, u.k, u.k, generator=g) * math.sqrt(2.0 / (u.k * u.k * u.cout)))
        ga, be = 1.0 + 0.3 * torch.randn(u.cout, generator=g), 0.2 * torch.randn(u.cout, generator=g)
        if not bool((ga < 0).any()):
            ga[3] = -ga[3]
        if i == special:
            ga[1], be[1], ga[2], be[2] = 0.0, -0.25, 0.0, 0.25
        P["gamma"].append(None if u.flags & NO_BN else ga)
        P["beta"].append(None if u.flags & NO_BN else be)
    x = torch.randn(N, units[0].cin, hw, hw, generator=g)
    dfeat = torch.randn(N, feat_dim, generator=g)
    return x, P, dfeat


# ------------------------------------------------------------------------------------------------ small helpers
def q(t, dt):
    """a value as its storage type holds it (None: no rounding)"""
    return t if dt is None else t.float().to(B.TDT[dt]).double()


def mc(t):
    """NCHW -> the [M, C] matrix bn_refs works on"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def nchw(m, like):
    N, C, H, W = like.shape
    return m.reshape(N, H, W, C).permute(0, 3, 1, 2)


def has_bn(u):
    return not u.flags & NO_BN


def raw_consumer(units, i):
    """the unit that consumes unit i's raw sum (PRE_RES / RAW_SRC), or None"""
    for c, u in enumerate(units):
        if (u.flags & PRE_RES and u.res == i + 1) or (u.flags & RAW_SRC and u.src == i + 1):
            return c
    return None


def unit_input(units, i, D):
    u = units[i]
    if u.flags & RAW_SRC:
        return D["z"][u.src - 1]
    return D["x"] if u.src == 0 else D["y"][u.src - 1]


def feat_of(y, pool_win):
    if pool_win:
        return B.avgpool_win_fwd(y.permute(0, 2, 3, 1), pool_win)
    return y.mean(dim=(2, 3))


def dy_of_feat(dfeat, like, pool_win):
    N, C, H, W = like.shape
    if pool_win:
        return B.avgpool_win_bwd(dfeat.cpu(), N, H, W, C, pool_win).to(dfeat.device).permute(0, 3, 1, 2)
    return (dfeat / (H * W))[:, :, None, None].expand(N, C, H, W)


def pool_bwd_exact(pre, dy):
    """gradient of max_pool2d(relu(pre), 3, 2, 1) at `pre` (torch's argmax: the first maximum of a window)"""
    h = pre.detach().clone().requires_grad_(True)
    F.max_pool2d(F.relu(h), 3, 2, 1).backward(dy)
    return h.grad


# ------------------------------------------------------------------------------------------------ an independent autograd network (the exact chain)
def autograd_chain(units, x, P, dfeat, pool_win):
    """the same dict from torch autograd in fp64, no rounding anywhere: what `judge` must reproduce to 1e-12"""
    x = x.double()
    w = [t.double().clone().requires_grad_(True) for t in P["w"]]
    ga = [None if t is None else t.double().clone().requires_grad_(True) for t in P["gamma"]]
    be = [None if t is None else t.double().clone().requires_grad_(True) for t in P["beta"]]
    z, y, rm, rv = [], [], [], []
    for i, u in enumerate(units):
        inp = z[u.src - 1] if u.flags & RAW_SRC else (x if u.src == 0 else y[u.src - 1])
        zi = F.conv2d(inp, w[i], stride=u.stride, padding=u.pad)
        if u.flags & PRE_RES:
            zi = zi + z[u.res - 1]
        z.append(zi)
        if not has_bn(u):
            y.append(None), rm.append(None), rv.append(None)
            continue
        yi = F.batch_norm(zi, None, None, ga[i], be[i], True, 0.0, B.EPS)
        rm.append(B.MOM * zi.detach().mean(dim=(0, 2, 3)))
        rv.append(B.MOM * zi.detach().var(dim=(0, 2, 3), unbiased=True))
        if u.res >= 0 and not u.flags & PRE_RES:
            yi = yi + y[u.res - 1]
        if u.relu:
            yi = F.relu(yi)
        if u.flags & MAXPOOL:
            yi = F.max_pool2d(yi, 3, 2, 1)
        yi.retain_grad()
        y.append(yi)
    feat = feat_of(y[-1], pool_win)
    feat.backward(dfeat.double())
    zero = lambda ts: [None if t is None else torch.zeros_like(t) for t in ts]
    return dict(x=x, z=[t.detach() for t in z], y=[None if t is None else t.detach() for t in y], dy=[None if t is None else t.grad for t in y], w=[t.detach() for t in w],
                gamma=[None if t is None else t.detach() for t in ga], beta=[None if t is None else t.detach() for t in be], gw=[t.grad for t in w],
                ggamma=[None if t is None else t.grad for t in ga], gbeta=[None if t is None else t.grad for t in be], gw0=zero(w), ggamma0=zero(ga), gbeta0=zero(be),
                rm=rm, rv=rv, feat=feat.detach(), dfeat=dfeat.double())


# ------------------------------------------------------------------------------------------------ the CPU emulator
def emulate(units, x, P, dfeat, dt, pool_win, fault=None, old=None, epilogue=False):
    """a generic executor of a unit list in fp64 that rounds every stored tensor to the storage type `dt` and sums a gradient in the plan's sweep order
    (units in reverse; within a unit the residual gradient, then the input gradient).  Returns the dict a plan read returns:
      x, z[i], y[i] (= activation i + 1), dy[i], w / gamma / beta[i] (fp32 masters), gw / ggamma / gbeta[i] (the gradient buffer after the pass) and
      gw0 / ggamma0 / gbeta0 (before it), rm / rv[i] (running statistics after ONE forward from 0), feat, dfeat.
    `fault` seeds ONE wiring fault (FAULTS); `old` = an earlier dict whose gradients this pass accumulates onto; `epilogue`: the BatchNorm-backward sums of a
    unit are taken from its dy BEFORE the last store rounded it, as the epilogue of the launch that completes dy (a dgrad, the pooling's backward) takes them."""
    n = len(units)
    x = q(x.double(), dt)
    D = dict(x=x, z=[None] * n, y=[None] * n, dy=[None] * n, w=[t.float().double() for t in P["w"]], gamma=[None if t is None else t.float().double() for t in P["gamma"]],
             beta=[None if t is None else t.float().double() for t in P["beta"]], rm=[None] * n, rv=[None] * n, dfeat=dfeat.float().double())
    for k in ("gw", "ggamma", "gbeta"):
        D[k + "0"] = [None if t is None else (torch.zeros_like(t) if old is None else old[k][i].clone()) for i, t in enumerate(D[{"gw": "w", "ggamma": "gamma", "gbeta": "beta"}[k]])]
        D[k] = [None] * n
    sv = [None] * n                                              # saved per unit: mean, invstd, pre-ReLU value, gamma used
    first_res = next(i for i, u in enumerate(units) if u.res >= 0 and has_bn(u) and not u.flags & PRE_RES) if any(u.res >= 0 and not u.flags & PRE_RES for u in units) else None
    for i, u in enumerate(units):
        inp = unit_input(units, i, D)
        zc = CR._fwd(inp, q(D["w"][i], dt), u.stride, u.pad)
        zi = q(zc, dt)
        if u.flags & PRE_RES:
            zi = q((zi + D["z"][u.res - 1]).float().double(), dt)
            zc = zi
        D["z"][i] = zi
        if not has_bn(u):
            continue
        M = zi.numel() // u.cout
        mean = zc.mean(dim=(0, 2, 3))                            # from the fp32 accumulators, before the store
        var = ((zc * zc).mean(dim=(0, 2, 3)) - mean * mean).clamp_min(0.0)
        unb = 1.0 if (fault == "biased_var" and i == 1) else B.unbias_factor(M)
        D["rm"][i] = (B.MOM * mean.float().double()).float().double()
        D["rv"][i] = (B.MOM * (var * unb).float().double()).float().double()
        mean32, istd32 = mean.float().double(), (1.0 / torch.sqrt(var + B.EPS)).float().double()
        gam = D["gamma"][i]
        if fault == "wrong_gamma" and i == 2:
            gam = D["gamma"][1]
        res = D["y"][u.res - 1] if (u.res >= 0 and not u.flags & PRE_RES) else None
        pre = nchw(B.bn_fwd(mc(zi), mean32, istd32, gam, D["beta"][i], None if res is None else mc(res)), zi)
        yi = F.relu(pre) if u.relu else pre
        if u.flags & MAXPOOL:
            yi = F.max_pool2d(yi, 3, 2, 1)
        D["y"][i] = q(yi.float().double(), dt)
        sv[i] = (mean32, istd32, pre)
    D["feat"] = feat_of(D["y"][-1], pool_win).float().double()
    # ---- backward
    D["dy"][n - 1] = q(dy_of_feat(D["dfeat"], D["y"][-1], pool_win).float().double(), dt)
    dy_raw = [None] * n                                          # an activation's gradient before its last store rounded it
    dy_raw[n - 1] = dy_of_feat(D["dfeat"], D["y"][-1], pool_win).float().double()
    written = [False] * n
    written[n - 1] = True
    dzr = [None] * n
    dy_first = [None] * n                                        # an activation's gradient after its FIRST write (fault sums_early)

    def write(a, val):                                           # activation a + 1
        if written[a] and not (fault == "dx_overwrite" and a == wfault):
            dy_raw[a] = (D["dy"][a] + val).float().double()
            D["dy"][a] = q(dy_raw[a], dt)
        else:
            dy_raw[a] = val.float().double()
            D["dy"][a] = q(dy_raw[a], dt)
            if not written[a]:
                dy_first[a] = D["dy"][a]
        written[a] = True

    # the first activation (in sweep order) that receives a second write through a dgrad: where dx_overwrite strikes
    wfault, seen = None, set()
    for i in range(n - 1, -1, -1):
        u = units[i]
        if u.res >= 0 and not u.flags & PRE_RES:
            seen.add(u.res - 1)
        if u.src != 0 and not u.flags & RAW_SRC:
            if u.src - 1 in seen and wfault is None:
                wfault = u.src - 1
            seen.add(u.src - 1)
    n_writes = collections.Counter()
    for i in range(n - 1, -1, -1):
        u = units[i]
        inp = unit_input(units, i, D)
        if not has_bn(u):
            dz = dzr[i]
        else:
            mean32, istd32, pre = sv[i]
            dyi = D["dy"][i]
            if u.flags & MAXPOOL:
                g = q(pool_bwd_exact(pre, dyi).float().double(), dt)
            else:
                mask_src = pre
                if fault == "mask_other" and i == first_res:
                    mask_src = sv[i - 1][2]
                g = dyi * (mask_src > 0) if u.relu else dyi
            zt, gt = mc(D["z"][i]), mc(g)
            xhat = (zt - mean32) * istd32
            gs = mc(dy_raw[i] * (pre > 0) if u.relu else dy_raw[i]) if (epilogue and not u.flags & MAXPOOL) else gt
            if fault == "sums_early" and i == sums_fault(units):
                gs = mc(dy_first[i] * (pre > 0) if u.relu else dy_first[i])
            s1, s2 = gs.sum(0), (gs * xhat).sum(0)
            D["gbeta"][i] = (D["gbeta0"][i] + s1.float().double()).float().double()
            D["ggamma"][i] = (D["ggamma0"][i] + s2.float().double()).float().double()
            M = zt.shape[0]
            dz = q(nchw(D["gamma"][i] * istd32 * (gt - s1 / M - xhat * (s2 / M)), D["z"][i]).float().double(), dt)
            if raw_consumer(units, i) is not None:
                dz = q((dz + dzr[i]).float().double(), dt)
            if u.flags & PRE_RES:
                dzr[u.res - 1] = dz
            if u.res >= 0 and not u.flags & PRE_RES and not (fault == "drop_res" and i == first_res):
                n_writes[u.res - 1] += 1
                write(u.res - 1, g)
        win = D["z"][u.src - 1] if (fault == "wgrad_from_z" and i == 2) else inp
        D["gw"][i] = (D["gw0"][i] + CR._wgrad(win, dz, u.k, u.stride, u.pad)).float().double()
        if u.src != 0 and not (fault == "no_shortcut_dgrad" and u.k == 1 and i == next(j for j, v in enumerate(units) if v.k == 1)):
            dx = CR._dgrad(dz, q(D["w"][i], dt), u.stride, u.pad, inp.shape[2], inp.shape[3])
            if u.flags & RAW_SRC:
                dzr[u.src - 1] = q(dx.float().double(), dt)
            else:
                n_writes[u.src - 1] += 1
                write(u.src - 1, dx)
    return D


def sums_fault(units):
    """the unit whose BatchNorm-backward sums the fault `sums_early` takes from the first of the two writes of its dy: the first unit (in unit order) whose
    activation has two readers"""
    for i in range(len(units)):
        readers = sum((u.src == i + 1 and not u.flags & RAW_SRC) + (u.res == i + 1 and not u.flags & PRE_RES) for u in units)
        if readers >= 2 and has_bn(units[i]):
            return i
    return -1


# ------------------------------------------------------------------------------------------------ the verdicts
class Verdict(dict):
    """(unit, tensor) -> err / bound; .rel: the same keys -> max |err| / max |ref| (the exact chain's figure); .ambig: unit -> ambiguous share"""

    def __init__(self):
        super().__init__()
        self.rel, self.ambig = {}, {}

    def add(self, unit, what, got, ref, bound):
        got, ref = got.double().reshape(ref.shape), ref.double()
        err = (got - ref).abs()
        bound = torch.as_tensor(bound, dtype=torch.float64, device=ref.device).expand_as(err)
        if not bool(torch.isfinite(got).all()):
            r = float("inf")
        else:
            qv = torch.where(err == 0, torch.zeros_like(err), err / bound)
            r = float("inf") if bool(torch.isnan(qv).any()) else float(qv.max())
        self[(unit, what)] = r
        self.rel[(unit, what)] = float(err.max() / ref.abs().max().clamp_min(1e-300))

    def worst_by_link(self):
        out = {}
        for (unit, what), r in self.items():
            out[what] = max(out.get(what, 0.0), r)
        return out

    def failures(self, limit=1.0):
        return {f"unit {u} {w}": r for (u, w), r in self.items() if not r <= limit}

    def check(self, tag=""):
        bad = self.failures()
        assert not bad, f"{tag}: links outside their bound (err / bound): {bad}"
        worst = max(self.ambig.values(), default=0.0)
        assert worst <= B.AMBIG_CAP, f"{tag}: ambiguous share {worst:.3g} of a tensor's elements exceeds the cap {B.AMBIG_CAP}"


def recover(rm, rv, M, noise):
    """(mean, biased var, abs error of mean, abs error of var) of a BatchNorm from its running statistics after ONE update from (0, 0): running = m * new in
    fp32 (bn_refs.bound_running with old = 0), divided by m in fp64 here"""
    mean, varu = rm / B.MOM, rv / B.MOM
    unb = B.unbias_factor(M)
    e_mean = B.bound_running(torch.zeros_like(mean), mean) / B.MOM
    e_var = B.bound_running(torch.zeros_like(varu), varu, noise * unb) / B.MOM / unb
    return mean, varu / unb, e_mean, e_var


def z_link(units, i, D, dt):
    """(ref, bound, accumulation part of the bound) of unit i's stored z from its stored input"""
    u = units[i]
    wq = q(D["w"][i], dt)
    ref, S = CR.conv_fwd_ref(unit_input(units, i, D), wq, u.stride, u.pad)
    R = u.k * u.k * u.cin
    bound, acc = CR.elem_bound(S, R, ref, dt), CR.acc_bound(S, R)
    if u.flags & PRE_RES:                                        # one more stored rounding of the fp32 sum (bn_refs.add_stored)
        zr = D["z"][u.res - 1]
        ref = ref + zr
        bound = bound + (CR.OUT_EPS[dt] + B.U) * (ref.abs() + bound)
        acc = bound
    return ref, bound, acc


def judge(units, D, dt, pool_win, nbt=None, forward_only=False):
    """every link of one training pass (see the module docstring) -> Verdict.  forward_only: the links of the forward alone (z, the statistics, y, feat) -- for a
    plan whose backward keeps the gradients of its activations in LDS (the stage-level training launches), where D holds no dy"""
    V = Verdict()
    n = len(units)
    kind = "rsqrt" if dt == "bf16" else "fp64"
    # relative distance of a stored value from the fp32 value it was rounded from.  bf16 keeps 8 significant bits, so round-to-nearest moves a value by up to
    # HALF AN ULP = 2^-8 of its magnitude: bn_refs.R is that unit roundoff itself, not an ulp, and nothing is halved.  (The first MI355X run showed it: the
    # pooling's backward sums dfeat / HW before the store, the stored dy is one rounded constant per image and channel, and at 3 to 5 images the few aligned
    # roundings reached 1.4 to 1.6 times a bound that counted r / 2; emulate(epilogue=True) reproduces it on the CPU.)
    half = B.R[dt] if dt == "bf16" else B.U
    fw = [None] * n                                              # per unit: mean, invstd, pre-ReLU value, ambiguous mask, e_mean, relative e_invstd, fp32 part
    for i, u in enumerate(units):
        z = D["z"][i]
        ref, bound, acc = z_link(units, i, D, dt)
        V.add(i, "z", z, ref, bound)
        if not has_bn(u):
            continue
        zt = mc(z)
        M = zt.shape[0]
        s1, s2 = zt.sum(0), (zt * zt).sum(0)
        noise = B.var_noise(s1, s2, M)
        mean, var, e_mean, e_var = recover(D["rm"][i], D["rv"][i], M, noise)
        # (a) the statistics link: the recovered values against those of the stored z; the sums came from fp32 accumulators before the store
        b1, b2 = CR.stat_bounds(z, acc)
        d1 = (half * (1 + half) * zt.abs().sum(0) + b1) / M
        d2 = (2 * half * (1 + half) * s2 + b2) / M
        mz = s1 / M
        V.add(i, "mean", mean, mz, d1 + e_mean)
        V.add(i, "var", var, (s2 / M - mz * mz).clamp_min(0.0), d2 + 2 * mz.abs() * d1 + d1 * d1 + e_var + noise)
        # (b) everything below is a function of the recovered statistics
        istd = 1.0 / torch.sqrt(var + B.EPS)
        e_istd = 0.5 * (e_var + noise) / (var + B.EPS)
        gam, bet = D["gamma"][i], D["beta"][i]
        res = D["y"][u.res - 1] if (u.res >= 0 and not u.flags & PRE_RES) else None
        rt = None if res is None else mc(res)
        pre = B.bn_fwd(zt, mean, istd, gam, bet, rt)
        refy = pre.clamp_min(0.0) if u.relu else pre
        bd, fp = B.bound_y(refy, zt, mean, istd, gam, bet, rt, dt, kind, e_istd)
        shift = (gam * istd).abs() * e_mean                          # the recovered mean's own error moves y by scale * e_mean
        bd, fp = bd + (1 + B.R[dt]) * shift, fp + shift
        amb = (pre.abs() <= fp) if u.relu else torch.zeros_like(pre, dtype=torch.bool)
        if u.flags & MAXPOOL:                                    # the pooled value is within the largest bound of its window
            V.add(i, "y", D["y"][i], F.max_pool2d(nchw(refy, z), 3, 2, 1), F.max_pool2d(nchw(bd, z), 3, 2, 1))
        else:
            V.add(i, "y", D["y"][i], nchw(refy, z), nchw(bd, z))
        fw[i] = (mean, istd, pre, amb, e_mean, e_istd + B.E_ISTD[kind] * B.U, fp)
        V.ambig[i] = float(amb.sum()) / amb.numel()
    ylast = D["y"][-1]
    hw = pool_win * pool_win if pool_win else ylast.shape[2] * ylast.shape[3]
    reff = feat_of(ylast, pool_win)
    V.add(n, "feat", D["feat"], reff, B.bound_pool_fwd(feat_of(ylast.abs(), pool_win) * hw, hw, reff))
    if nbt is not None:
        V[(n, "num_batches_tracked")] = 0.0 if all(int(v) == nbt[0] for v in nbt[1]) else float("inf")
    if forward_only:
        return V
    # ---- backward: unit by unit in reverse; DZ[i] = (reference, bound) of the unseen dz; contrib[a] = the writes of activation a + 1's gradient in sweep order
    DZ = [None] * n
    RAWG = [None] * n                                            # (reference, bound) of the raw-gradient buffer of unit i
    contrib = [[] for _ in range(n)]
    dyl = dy_of_feat(D["dfeat"], ylast, pool_win)
    contrib[n - 1].append(("w", dyl, B.bound_pool_bwd(dyl, dt)))
    for i in range(n - 1, -1, -1):
        u = units[i]
        inp = unit_input(units, i, D)
        if not has_bn(u):
            DZ[i] = RAWG[i]
        else:
            mean, istd, pre, amb, e_mean, e_i, fp = fw[i]
            z, dyi = D["z"][i], D["dy"][i]
            zt = mc(z)
            M = zt.shape[0]
            xhat = (zt - mean) * istd
            if u.flags & MAXPOOL:
                pre4, fp4 = nchw(pre, z), nchw(fp, z)
                gx = pool_bwd_exact(pre4, dyi)
                # windows with more than one candidate for the argmax (or one whose ReLU is ambiguous): either routing of that window's gradient is right
                hr = F.relu(pre4)
                maxlo = F.max_pool2d(hr - fp4, 3, 2, 1)
                neg = -1e300
                unf = lambda t, pad: F.unfold(F.pad(t, (1, 1, 1, 1), value=pad), 3, stride=2).reshape(t.shape[0], t.shape[1], 9, -1)
                cand = (unf(hr + fp4, neg) >= maxlo.reshape(maxlo.shape[0], maxlo.shape[1], 1, -1)) & (unf(pre4, neg) > -unf(fp4, 0.0))
                # candidates with bit-equal z are no ambiguity: equal z gives equal values in any arithmetic, and the tie rule (the first of them) decides
                zu = unf(z, 0.0)
                same_z = torch.where(cand, zu, torch.full_like(zu, neg)).amax(2, keepdim=True) == torch.where(cand, zu, torch.full_like(zu, -neg)).amin(2, keepdim=True)
                sure = same_z & ~(cand & (unf(pre4, neg) <= unf(fp4, 0.0))).any(2, keepdim=True)
                wide = (cand & ~sure).double() * dyi.abs().reshape(dyi.shape[0], dyi.shape[1], 1, -1)
                bg4 = F.fold(wide.reshape(wide.shape[0], -1, wide.shape[3]), (z.shape[2] + 2, z.shape[3] + 2), 3, stride=2)[:, :, 1:-1, 1:-1]
                V.ambig[i] = float((bg4 > 0).sum()) / bg4.numel()
                g = mc(gx)
                bg = mc(bg4) + (CR.OUT_EPS[dt] + 4 * B.U) * g.abs() + B.FLOOR[dt]      # the full-size gradient is a stored tensor: up to four fp32 adds, one rounding
                gmag = g.abs() + bg
            else:
                dyt = mc(dyi)
                g = dyt * B.relu_mask(pre) if u.relu else dyt
                bg = amb * dyt.abs()
                gmag = torch.where(amb, dyt.abs(), g.abs())
            s1, s2 = g.sum(0), (g * xhat).sum(0)
            dx = istd * e_mean + xhat.abs() * e_i                   # |error of the kernel's xhat against the recovered one|
            ds1 = B.bound_sum(M, B.T_SUM1, gmag.sum(0), bg.sum(0)) + (half * gmag.sum(0) if dt == "bf16" else 0.0)
            ds2 = B.bound_sum(M, B.T_SUM2, (gmag * xhat.abs()).sum(0), (bg * xhat.abs()).sum(0)) + (half * (gmag * xhat.abs()).sum(0) if dt == "bf16" else 0.0) + (gmag * dx).sum(0)
            V.add(i, "dbeta", D["gbeta"][i], D["gbeta0"][i] + s1, B.bound_grad_store(D["gbeta0"][i], s1, ds1))
            V.add(i, "dgamma", D["ggamma"][i], D["ggamma0"][i] + s2, B.bound_grad_store(D["ggamma0"][i], s2, ds2))
            gi = D["gamma"][i] * istd
            k0, k1 = s1 / M, s2 / M
            dz = gi * (g - k0 - xhat * k1)
            bdz = B.bound_dz(dz, gmag, xhat, gi, k0, k1, dt, ds1 / M, ds2 / M) + (1 + B.R[dt]) * (gi.abs() * bg + e_i * dz.abs() + gi.abs() * k1.abs() * dx)
            dz, bdz = nchw(dz, z), nchw(bdz, z)
            if raw_consumer(units, i) is not None:               # dz += the raw consumer's gradient: one fp32 add, one more stored rounding
                dz, bdz = dz + RAWG[i][0], bdz + RAWG[i][1]
                bdz = bdz + (CR.OUT_EPS[dt] + B.U) * (dz.abs() + bdz)
            DZ[i] = (dz, bdz)
            if u.flags & PRE_RES:                                # the gradient of the sum IS the gradient of the raw sum it added
                RAWG[u.res - 1] = DZ[i]
            if u.res >= 0 and not u.flags & PRE_RES:
                contrib[u.res - 1].append(("r", nchw(g, z), nchw(bg, z)))
        dz, bdz = DZ[i]
        dw, Sw = CR.conv_wgrad_ref(inp, dz, u.k, u.stride, u.pad)
        Rw = dz.shape[0] * dz.shape[2] * dz.shape[3]
        V.add(i, "dw", D["gw"][i], D["gw0"][i] + dw, CR.wgrad_bound(Sw, Rw, D["gw0"][i]) + CR._wgrad(inp.abs(), bdz, u.k, u.stride, u.pad))
        if u.src != 0:
            wq = q(D["w"][i], dt)
            dx, Sd = CR.conv_dgrad_ref(dz, wq, u.stride, u.pad, inp.shape[2], inp.shape[3])
            prop = CR._dgrad(bdz, wq.abs(), u.stride, u.pad, inp.shape[2], inp.shape[3])
            Rd = u.k * u.k * u.cout
            if u.flags & RAW_SRC:
                RAWG[u.src - 1] = (dx, CR.elem_bound(Sd, Rd, dx, dt) + prop)
            else:
                contrib[u.src - 1].append(("c", dx, Sd, Rd, prop))
    for a in range(n):
        if not contrib[a] or D["dy"][a] is None:
            continue
        part = bnd = None
        for c in contrib[a]:
            if c[0] == "w":
                part, bnd = c[1], c[2]
            elif c[0] == "r":                                    # a copy of g when it is the first write, else one fp32 add and one stored rounding
                if part is None:
                    part, bnd = c[1], c[2]
                else:
                    part = part + c[1]
                    bnd = bnd + c[2] + B.bound_dres_acc(part.abs() + bnd + c[2], dt)
            else:
                _, dx, Sd, Rd, prop = c
                if part is None:
                    part, bnd = dx, CR.elem_bound(Sd, Rd, dx, dt) + prop
                else:
                    bnd = bnd * (1 + CR.OUT_EPS[dt]) + CR.elem_bound(Sd, Rd, dx, dt, old=part) + prop
                    part = part + dx
        V.add(a, "dy", D["dy"][a], part, bnd)
    return V


def judge_eval(units, D, dt, only=None):
    """the eval forward per unit: z from its stored input, y = relu?(z scale + shift (+ res)) of the running statistics (bound_y kind "eval": the running
    mean is an exact fp32 input).  D: x, z, y, w, gamma, beta, rm, rv.  only: the units to judge (None: all) -- the units of a run that the eval forward took as
    one launch (stage.hip) have no stored z and y; tests/stage_eval_worker.py holds those to the kernel itself"""
    V = Verdict()
    for i, u in enumerate(units):
        if only is not None and i not in only:
            continue
        ref, bound, _ = z_link(units, i, D, dt)
        V.add(i, "eval z", D["z"][i], ref, bound)
        if not has_bn(u):
            continue
        zt = mc(D["z"][i])
        istd = 1.0 / torch.sqrt(D["rv"][i] + B.EPS)
        res = D["y"][u.res - 1] if (u.res >= 0 and not u.flags & PRE_RES) else None
        rt = None if res is None else mc(res)
        pre = B.bn_fwd(zt, D["rm"][i], istd, D["gamma"][i], D["beta"][i], rt)
        refy = pre.clamp_min(0.0) if u.relu else pre
        bd, _ = B.bound_y(refy, zt, D["rm"][i], istd, D["gamma"][i], D["beta"][i], rt, dt, "eval")
        if u.flags & MAXPOOL:
            V.add(i, "eval y", D["y"][i], F.max_pool2d(nchw(refy, D["z"][i]), 3, 2, 1), F.max_pool2d(nchw(bd, D["z"][i]), 3, 2, 1))
        else:
            V.add(i, "eval y", D["y"][i], nchw(refy, D["z"][i]), nchw(bd, D["z"][i]))
    return V
