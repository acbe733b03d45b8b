"""The two references of the stage-level eval forward (csrc/stage.hip: clhip_stage_eval, and the runs clhip_plan_forward_ex makes of it) -- a helper module, not a
conftest.  Plain torch fp64 on whatever device the tensors live on, built on tests/conv_ref.py (the convolution as an im2col product, its accumulation bound) and
tests/bn_refs.py (the eval BatchNorm formula, bound_y); every count and constant is theirs, nothing is fitted to the kernel's output.  The project is not imported.
Tensors are NCHW fp64 here; the layouts of the C ABI are the GPU files' business.  tests/test_stage_ref_cpu.py holds this module to an independent F.conv2d /
F.batch_norm chain and seeds faults into it; tests/test_stage_eval_kernels_gpu.py and tests/stage_eval_worker.py hold the kernel and the plan to it.

A run is `nconv` convolutions (3x3, C -> C, stride 1, zero padding 1), each followed by an eval-mode BatchNorm; an even one (the first of a BasicBlock) reads the
block input X, applies ReLU and writes Y; an odd one reads Y, adds the block input X, applies ReLU and overwrites X.  The kernel's control flow does not depend
on data values, which allows two complementary oracles:

(a) The exact routing chain (`exact_case`).  Parameters and inputs for which every intermediate value of a 16-convolution run is a small integer, so that any
summation order in fp32 and every bf16 store is exact and the kernel must reproduce the fp64 chain BIT FOR BIT: weights with exactly one nonzero entry (+1 / -1)
per output channel at a seeded (tap, input channel), drawn independently per convolution; gamma in {+1, -1}; var = the fp32 value with fp32(var + eps) == 1
(`unit_var`), so 1 / sqrtf(var + eps) is exactly 1; integer beta and mean with shift = beta - mean * scale in {0, -1, -2}, drawn per (convolution, channel), so
all four BatchNorm arrays of every convolution are in play; input integers in {-1, 0, 1}.  With non-positive shifts |y1| <= max |x| and |out| <= 2 max |x| per
block, hence magnitudes <= 256 after 8 blocks, which bf16 holds exactly.  `exact_case` asserts both facts (integers, <= 256) on the fp64 chain of every case
it hands out, and that the final output is not degenerate: at least EXACT_NONZERO of its elements are nonzero.  The draws favour +1 and a zero shift (a uniform
draw is extinct after three blocks: every block subtracts about one from values of one or two); the value SETS are the ones above.

(b) fp64 links with trained-like parameters (`link_case`, following plan_ref.trained_like: conv N(0, sqrt(2 / (9 C))), gamma = 1 + 0.3 randn with at least one
negative gamma per convolution, beta = 0.2 randn, one channel with gamma = 0, beta < 0 and one with gamma = 0, beta > 0; running mean 0.3 randn, running variance
in [0.5, 1.5) and one channel with variance 0, where invstd = 1 / sqrt(eps) -- that channel's gamma is +-1 / 256, so its scale stays near 1 and sixteen such
channels in a row do not blow the run up), on a general bf16 input whose border pixels are as large as its interior (randn everywhere).  The special channels move
with the convolution index.  Inner activations of a run cannot be read; they are made observable by PREFIX RUNS: the kernel is run with the same parameters at
nconv = 2, 4, ..., L, and the output of length 2k - 2 is the stored input of block k.  THE ASSUMPTION: the kernel is deterministic and its first 2k - 2
convolutions do not depend on nconv or on later parameters.  A filter-prefetch or table fault that breaks the assumption shows up as a failing link at some k.
For each block k three runs of length 2k are judged against what fp64 makes of that stored input (`link_ref`):
  first    conv 2k-2 real, conv 2k-1 the identity probe (`ident`: centre tap, unit channel matrix, gamma 1, beta 0, mean 0, var = unit_var).  z2 equals the stored
           y1 exactly (one nonzero product; storing a bf16 value changes nothing).  ref = relu(bn2(relu(bn1(conv(x_in)))) + x_in); bound = conv_ref.elem_bound
           for the unseen z1; bn_refs.bound_y(eval) for y1 plus (1 + R) |scale1| times the z1 bound; bound_y(res = x_in) for the output plus (1 + R) |scale2| times
           the y1 bound -- the idiom of plan_ref.judge for a value it cannot see.
  second   conv 2k-2 the identity probe, conv 2k-1 real: the path that reads Y, adds the block input from X and overwrites X in place.  The same composition with
           y1 = relu(bn1(x_in)) through the general formula; the probe being exact, the fp32 value of y1 is a bf16 value and its store adds nothing, so y1 carries
           the fp32 part of bound_y only.  Nothing but sharpness rests on that: a probe that were not exact fails the link, which is what the test is for.
  real     both convolutions real, the unseen y1's bound propagated through conv(|bound|, |w2|).  Rigorous but loose (a few tens of percent of a typical |z2|: it
           takes every inner rounding at its worst): the coarse net for "both register sets live at once"; the probes are the sharp one.
The verdict is max over ALL elements of err / bound <= 1; the output is continuous across the ReLU, so no element is left out and no ambiguous share is needed.

Faults (`FAULTS`, in the manner of plan_ref.FAULTS): `run(fault=(name, cv))` seeds one at convolution cv; the CPU test requires each to change the exact chain's
bits AND to push the matching link above 1, at every position."""
import torch
import torch.nn.functional as F

import bn_refs as B
import conv_ref as CR

GEOMS = [(16, 32), (32, 16), (64, 8)]          # (C, H = W): what clhip_stage_eval_supported admits
LMAX = 16
KINDS = ("first", "second", "real")
FAULTS = ["tap_shift", "chan_swap", "bn_prev", "mean_beta_swap", "res_drop", "res_from_y", "halo_wrap", "filter_plus2"]
RES_FAULTS = ("res_drop", "res_from_y")        # exist at the second convolution of a block only (the odd positions)
EPS32 = torch.tensor(B.EPS, dtype=torch.float32)
# smallest share of nonzero elements of the final output over the seeds and geometries of EXACT_SEEDS (measured on the CPU: tests/test_stage_ref_cpu.py prints
# it; 0.76 to 0.84 over N = 1, 3, 257, the smallest 0.764 at C = 64), required of every case with a margin for other seeds
EXACT_NONZERO = 0.5
EXACT_SEEDS = {16: 3, 32: 8, 64: 2}         # per C: the seed of the GPU file's routing cases (N = 1, 3, 257 draw N images from it)
LINK_SEEDS = {16: 21, 32: 22, 64: 23}
P_SIGN, P_SHIFT, P_X = [0.9, 0.1], [0.8, 0.15, 0.05], [0.6, 0.2, 0.2]          # the draws of the exact chain: +1 / -1; shift 0 / -1 / -2; x = 1 / 0 / -1


def bf(t):
    """a value as bf16 stores it, in fp64"""
    return t.float().to(torch.bfloat16).double()


def mc(t):
    """NCHW -> the [M, C] matrix bn_refs works on"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def nchw(m, like):
    N, C, H, W = like.shape
    return m.reshape(N, H, W, C).permute(0, 3, 1, 2)


def unit_var():
    """the fp32 value v with fp32(v + eps) == 1: the kernel's 1 / sqrtf(var + eps) is then exactly 1"""
    one, zero = torch.tensor(1.0), torch.tensor(0.0)
    v = one - EPS32
    for _ in range(16):
        s = float(v + EPS32)
        if s == 1.0:
            break
        v = torch.nextafter(v, one if s < 1.0 else zero)
    assert float(v + EPS32) == 1.0
    return float(v)


def affine(c, f32sum, dev):
    """(gamma, beta, mean, invstd) of a convolution's BatchNorm in fp64; f32sum: var + eps summed in fp32 as the kernel sums it (the exact chain, the emulation)"""
    g, b, m = (c[k].double().to(dev) for k in ("gamma", "beta", "mean"))
    s = (c["var"].float() + EPS32).double() if f32sum else c["var"].double() + B.EPS
    return g, b, m, (1.0 / torch.sqrt(s)).to(dev)


# ------------------------------------------------------------------------------------------------ the faults
def _prev_row(cv):
    return cv - 1 if cv > 0 else 1


def _other_filter(cv, L):
    return cv + 2 if cv + 2 < L else cv - 2


def _tap_shift(w):
    """the heaviest tap's weights act on the pixel of the next tap"""
    C = w.shape[0]
    w = w.reshape(C, C, 9).clone()
    t = int(w.abs().sum(dim=(0, 1)).argmax())
    w[:, :, (t + 1) % 9] += w[:, :, t]
    w[:, :, t] = 0
    return w.reshape(C, C, 3, 3)


def _chan_swap(w):
    """the heaviest input channel and its neighbour change places"""
    C = w.shape[0]
    w = w.clone()
    c0 = int(w.abs().sum(dim=(0, 2, 3)).argmax())
    c1 = (c0 + 1) % C
    w[:, [c0, c1]] = w[:, [c1, c0]]
    return w


def run(x, convs, lo, hi, fault=None, rounded=False, f32sum=False, keep=None):
    """convolutions lo .. hi - 1 (lo even) of a run on the block input x [N, C, H, H]; fp64 throughout.  rounded: every pre-BatchNorm value and every stored
    activation rounded to bf16 (the kernel's roundings: an emulation of it); f32sum: see affine; fault = (name, cv); keep: a list that receives X after every block"""
    assert lo % 2 == 0 and hi % 2 == 0
    X, Y, L, dev = x.double(), None, len(convs), x.device
    for cv in range(lo, hi):
        f = fault[0] if fault is not None and fault[1] == cv else None
        second = cv & 1
        S = Y if second else X
        c = convs[cv]
        w = bf(convs[_other_filter(cv, L)]["w"] if f == "filter_plus2" else c["w"]).to(dev)
        if f == "tap_shift":
            w = _tap_shift(w)
        elif f == "chan_swap":
            w = _chan_swap(w)
        z = F.conv2d(F.pad(S, (1, 1, 1, 1), mode="circular"), w) if f == "halo_wrap" else CR._fwd(S, w, 1, 1)
        if rounded:
            z = bf(z)
        g, b, m, istd = affine(convs[_prev_row(cv)] if f == "bn_prev" else c, f32sum, dev)
        if f == "mean_beta_swap":
            b, m = m, b
        res = None
        if second and f != "res_drop":
            res = Y if f == "res_from_y" else X
        v = nchw(B.bn_fwd(mc(z), m, istd, g, b, None if res is None else mc(res)), z).clamp_min(0.0)
        if rounded:
            v = bf(v)
        if second:
            X = v
            if keep is not None:
                keep.append(X)
        else:
            Y = v
    return X


# ------------------------------------------------------------------------------------------------ (a) the exact routing chain
def exact_case(C, H, N, seed, L=LMAX, dev="cpu"):
    """dict(x, convs, outs): outs[k - 1] = the fp64 chain after block k = what a run of nconv = 2k must return bit for bit (drawn on the CPU, evaluated on dev)"""
    g = torch.Generator().manual_seed(seed)
    uv = unit_var()
    ar = torch.arange(C)
    pick = lambda vals, probs: torch.tensor(vals)[torch.multinomial(torch.tensor(probs), C, replacement=True, generator=g)].float()
    convs = []
    for _ in range(L):
        w = torch.zeros(C, C, 9)
        w[ar, torch.randperm(C, generator=g), torch.randint(0, 9, (C,), generator=g)] = pick([1.0, -1.0], P_SIGN)
        gamma = pick([1.0, -1.0], P_SIGN)
        mean = torch.randint(-2, 3, (C,), generator=g).float()
        shift = pick([0.0, -1.0, -2.0], P_SHIFT)
        convs.append(dict(w=w.reshape(C, C, 3, 3), gamma=gamma, beta=shift + mean * gamma, mean=mean, var=torch.full((C,), uv)))
    x = torch.tensor([1.0, 0.0, -1.0], dtype=torch.float64)[torch.multinomial(torch.tensor(P_X), N * C * H * H, replacement=True, generator=g)].reshape(N, C, H, H).to(dev)
    parts = []
    for a in range(0, N, 64):                                    # (by 64 images: the im2col matrix of 257 images is 300 MB)
        parts.append([])
        run(x[a:a + 64], convs, 0, L, f32sum=True, keep=parts[-1])
    outs = [torch.cat(t) for t in zip(*parts)]
    for o in outs:
        assert bool((o == o.round()).all()) and float(o.abs().max()) <= 256.0
    share = float((outs[-1] != 0).double().mean())
    assert share >= EXACT_NONZERO, (C, H, N, seed, share)
    return dict(x=x, convs=convs, outs=outs, share=share)


# ------------------------------------------------------------------------------------------------ (b) the fp64 links
def link_case(C, H, N, seed, L=LMAX, dev="cpu"):
    """dict(x, convs): a bf16 input and trained-like parameters (see the module docstring)"""
    g = torch.Generator().manual_seed(seed)
    convs = []
    for i in range(L):
        w = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
        ga, be = 1.0 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
        rm, rv = 0.3 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
        c1, c2, c0 = (3 * i + 1) % C, (3 * i + 2) % C, (3 * i + 4) % C
        ga[c1], be[c1], ga[c2], be[c2] = 0.0, -0.25, 0.0, 0.25
        rv[c0] = 0.0
        ga[c0] = (1.0 if ga[c0] >= 0 else -1.0) / 256.0
        if not bool((ga < 0).any()):
            c3 = (3 * i + 3) % C
            ga[c3] = -ga[c3]
        convs.append(dict(w=w, gamma=ga, beta=be, mean=rm, var=rv))
    x = bf(torch.randn(N, C, H, H, generator=g)).to(dev)
    return dict(x=x, convs=convs)


def ident(C):
    """the identity probe: centre tap, unit channel matrix, gamma 1, beta 0, mean 0, scale exactly 1 in the kernel's fp32"""
    w = torch.zeros(C, C, 3, 3)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    return dict(w=w, gamma=torch.ones(C), beta=torch.zeros(C), mean=torch.zeros(C), var=torch.full((C,), unit_var()))


def probe_convs(convs, k, kind):
    """the parameter list of the run of length 2k that judges block k (1-based) in `kind`"""
    out = list(convs)
    if kind == "first":
        out[2 * k - 1] = ident(convs[0]["w"].shape[0])
    elif kind == "second":
        out[2 * k - 2] = ident(convs[0]["w"].shape[0])
    return out


def link_ref(kind, x_in, ca, cb):
    """(ref, bound) NCHW fp64 of the output of a block (ca, cb as the run had them) from its STORED input x_in"""
    x_in = x_in.double()
    dev, R9, r = x_in.device, 9 * x_in.shape[1], B.R["bf16"]
    xt = mc(x_in)
    g1, b1, m1, i1 = affine(ca, False, dev)
    g2, b2, m2, i2 = affine(cb, False, dev)
    w2 = bf(cb["w"]).to(dev)
    if kind == "second":
        y1 = B.bn_fwd(xt, m1, i1, g1, b1).clamp_min(0.0)
        _, by1 = B.bound_y(y1, xt, m1, i1, g1, b1, None, "bf16", "eval")
    else:
        z1, S1 = CR.conv_fwd_ref(x_in, bf(ca["w"]).to(dev), 1, 1)
        bz1, z1t = mc(CR.elem_bound(S1, R9, z1, "bf16")), mc(z1)
        y1 = B.bn_fwd(z1t, m1, i1, g1, b1).clamp_min(0.0)
        by1, _ = B.bound_y(y1, z1t, m1, i1, g1, b1, None, "bf16", "eval")
        by1 = by1 + (1 + r) * (g1 * i1).abs() * bz1
    if kind == "first":
        z2t, bz2 = y1, by1
    else:
        z2, S2 = CR.conv_fwd_ref(nchw(y1, x_in), w2, 1, 1)
        bz2, z2t = mc(CR.elem_bound(S2, R9, z2, "bf16") + CR._fwd(nchw(by1, x_in), w2.abs(), 1, 1)), mc(z2)
    out = B.bn_fwd(z2t, m2, i2, g2, b2, xt).clamp_min(0.0)
    bo, _ = B.bound_y(out, z2t, m2, i2, g2, b2, xt, "bf16", "eval")
    bo = bo + (1 + r) * (g2 * i2).abs() * bz2
    return nchw(out, x_in), nchw(bo, x_in)


def ratio(got, ref, bound):
    """max over ALL elements of |got - ref| / bound; a NaN or an infinity anywhere is an infinite ratio"""
    got = got.double().reshape(ref.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float("inf") if bool(torch.isnan(q).any()) else float(q.max())


def judge_link(kind, x_in, convs, k, got):
    """err / bound of the output `got` of a run of length 2k whose parameters were probe_convs(convs, k, kind), from the stored input x_in of block k"""
    pc = probe_convs(convs, k, kind)
    ref, bound = link_ref(kind, x_in, pc[2 * k - 2], pc[2 * k - 1])
    return ratio(got, ref, bound)
