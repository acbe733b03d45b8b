"""fp64 reference of ONE BLOCK of the stage-level training launches (csrc/stage_train.hip + csrc/xch.h through clhip_stage_train_fwd / clhip_stage_train_bwd) -- a
helper module, not a conftest.  Plain torch fp64 on whatever device the tensors live on, NCHW inside, built on tests/conv_ref.py (the convolutions as im2col
products and their accumulation bounds) and tests/bn_refs.py (the BatchNorm formulas and their counted bounds); plan_ref.Verdict collects the ratios.  The project
is not imported.  tests/test_stage_train_ref_cpu.py holds this module to an independent F.conv2d / F.batch_norm autograd chain and seeds faults into its emulator;
tests/test_stage_train_kernels_gpu.py holds the kernels to it.

A block is a BasicBlock  conv1 -> BN -> ReLU (= a1) -> conv2 -> BN -> + res -> ReLU (= y).  Plain block: both convolutions 3x3 / stride 1, C -> C, res = the block
input x; table rows [conv1, conv2].  ENTRY block (the stage's down-sampling block): conv1 3x3 / stride 2, C / 2 -> C, res = BN(shortcut 1x1 / stride 2), no ReLU
behind the shortcut's BatchNorm; table rows [conv1, shortcut, conv2] as the C ABI orders them.  BatchNorm is in training mode: batch statistics of every
convolution's output, momentum update of the running statistics with the unbiased variance.

Every link is TEACHER-FORCED: the reference of a stored tensor is computed from the STORED inputs of that link, so each bound covers one step of arithmetic.
  forward   z of a convolution from its stored input (the block input; the stored a1): conv_ref.elem_bound.  mean / invstd against the batch statistics of the fp64
            convolution: the kernel sums its fp32 ACCUMULATORS, not the stored z, so the sums carry conv_ref.stat_bounds of the accumulation term (as
            plan_ref.judge takes it), mean one fp32 rounding (bound_mean), the variance bn_refs.var_noise on top; invstd = 1 / sqrt(var + eps) is evaluated at
            var -+ that error (monotone, so the interval is exact; to first order it is bn_refs.bound_invstd) plus E_ISTD["rsqrt"] fp32 roundings.  scale / shift
            from the stored invstd / mean (one and two fp32 roundings).  Running statistics: bound_running with the M / (M - 1) factor (1 at M = 1).  a1, the
            shortcut's output and y from the stored z, mean, invstd through bn_refs.bound_y (res = the block input / the stored shortcut output).  feat from the
            stored y: bound_pool_fwd.  The launch accepts mask pointers and never writes them (the backward takes a block output's mask from y > 0); the GPU file
            asserts exactly that on a canary.
            a1 is not stored by a plan; the direct entry stores it when y[conv1] is given, and the identity probe (conv2 = centre-tap identity, whose z2 must
            then equal the stored a1 BIT FOR BIT) ties the stored copy to the one in LDS that conv2 reads.
  backward  the test supplies x, dy or dfeat, z, y, mean, invstd (the fp64 forward of this module rounded to storage: `forward`), gamma, beta and the dgrad weight
            copies, so the backward is judged whatever the forward kernel does.  Rounding points are the kernel header's: dy and dz pass through bf16, sums are
            fp32 per image and fp64 across images.
              g2 = dy (y > 0) is exact (products of stored values with 0 / 1); with dfeat, dy = bf16(fl(dfeat * 1 / HW)) is emulated exactly (1 / HW is a power of 2).
              dgamma / dbeta onto the old values: bound_sum with d = M (any order of M fp32 terms), then bound_grad_store.
              dz (unseen; stored as dzg by the group form and then judged directly): bound_dz with the sums' errors / M.
              the gradient of a1 = dgrad(dz2) (unseen): elem_bound + the |w| product of dz2's bound; g1 = bf16(that) * [scale1 z1 + shift1 > 0].  Elements with
              |scale1 z1 + shift1| inside the fp32 part of bound_y are admitted against either mask: |grad a1| joins the bound there (plan_ref's idiom); their share is
              returned and capped by bn_refs.AMBIG_CAP.
              dx = bf16(bf16(dgrad(dz1)) + g2 [+ old dx]): elem_bound + the |w| product of dz1's bound, then the residual term bound_dres_acc (one fp32 add, one
              storage rounding) and one more fp32 add when it accumulates.  Entry block: ONE accumulation over both strided dgrads (R = 9 C + C), one rounding.
              weight-gradient blocks as the kernel leaves them (per image; per group of 16 images in the group form) and their sum in block order: wgrad_bound with
              R = the block's pixels, plus the |x| product of dz's bound (and the a1 bound times |dz| for conv2, whose operand the kernel rebuilds from z1).
            Identity probes need no extra code here: with conv1 (conv2) = the centre-tap identity the |w| products collapse to the bound of the unseen tensor itself,
            so dx - g2 shows dz1 and dbeta1 / dgamma1 show the masked dz2 up to one storage rounding.  The all-real block is the coarse case.
No bound is fitted to kernel output.  The verdict is max over ALL elements of err / bound <= 1.

`emulate_*` = the same formulas with the kernel's roundings (fp64 sums standing in for its fp32 ones), with a FAULTS list in the manner of plan_ref.FAULTS."""
import math

import torch

import bn_refs as B
import conv_ref as CR
from plan_ref import Verdict, mc, nchw

GEOMS = [(16, 32), (32, 16), (64, 8)]          # (C, H = W) of a run; an entry block exists at C = 32 and 64
R16 = B.R["bf16"]
FAULTS = ["drop_image_fwd", "biased_var", "drop_image_bwd", "mask_other", "res_grad_drop", "res_before_mask", "dx_overwrite", "old_dgamma_ignored", "tap_mirror",
          "entry_parity", "group_last_twice"]
FWD_FAULTS = ("drop_image_fwd", "biased_var")
IPG = 16                                       # images per block of the group weight gradient (C = 64, N >= 128)
SEEDS = {16: 31, 32: 32, 64: 33}


def bf(t):
    return t.float().to(torch.bfloat16).double()


def f32(t):
    return t.float().double()


def rows_of(C, entry):
    """(cin, k, stride, pad) per table row of one block"""
    return [(C // 2, 3, 2, 1), (C // 2, 1, 2, 0), (C, 3, 1, 1)] if entry else [(C, 3, 1, 1), (C, 3, 1, 1)]


def ident_w(C):
    w = torch.zeros(C, C, 3, 3)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    return w


# ------------------------------------------------------------------------------------------------ cases
def link_case(C, H, N, seed, entry=False, block=0):
    """seeded inputs of one block in the manner of plan_ref.trained_like / stage_ref.link_case (drawn on the CPU): conv N(0, sqrt(2 / (k k cin))), gamma = 1 + 0.3
    randn with at least one negative gamma per convolution, beta = 0.2 randn; per convolution i one channel with gamma = 0, beta < 0 and one with gamma = 0,
    beta > 0, moving with i; x randn everywhere (border pixels as large as the interior), bf16, image N / 2 all zero (N >= 2).  conv2's output channel
    (5 i + 3) % C has zero weights (constant over the batch: variance 0, the clamp and invstd = 1 / sqrt(eps); gamma +-1 / 256 keeps its scale near 1), and its
    channel (5 i + 7) % C reads the constant a1 of conv1's (gamma = 0, beta > 0) channel through a centre tap of 120 on top of its random weights: mean about 30
    times its spread, in every image, so the variance is a cancellation and its bound must come from var_noise and the accumulation term.  Old running
    statistics, old dgamma / dbeta and the old dx are non-zero."""
    g = torch.Generator().manual_seed(seed * 1000 + block)
    rows = []
    for i, (cin, k, s, p) in enumerate(rows_of(C, entry)):
        idx = 3 * block + i
        w = torch.randn(C, cin, k, k, generator=g) * math.sqrt(2.0 / (k * k * cin))
        ga, be = 1.0 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
        c1, c2 = (3 * idx + 1) % C, (3 * idx + 2) % C
        ga[c1], be[c1], ga[c2], be[c2] = 0.0, -0.25, 0.0, 0.25
        if k == 3 and s == 1 and i > 0:                          # conv2
            c0, c4 = (5 * idx + 3) % C, (5 * idx + 7) % C
            while c0 in (c1, c2):
                c0 = (c0 + 1) % C
            while c4 in (c0, c1, c2):
                c4 = (c4 + 1) % C
            w[c0] = 0.0
            ga[c0] = (1.0 if ga[c0] >= 0 else -1.0) / 256.0
            w[c4, rows[0]["pos"], 1, 1] = 120.0
        if not bool((ga < 0).any()):
            c3 = (3 * idx + 3) % C
            ga[c3] = -(ga[c3].abs() + 0.5)
        rows.append(dict(w=w, gamma=ga, beta=be, rm0=0.3 * torch.randn(C, generator=g), rv0=0.5 + torch.rand(C, generator=g), dg0=torch.randn(C, generator=g),
                         db0=torch.randn(C, generator=g), k=k, s=s, p=p, pos=c2))
    cin, hin = rows_of(C, entry)[0][0], (2 * H if entry else H)
    x = bf(torch.randn(N, cin, hin, hin, generator=g))
    if N >= 2:
        x[N // 2] = 0.0
    dy = bf(torch.randn(N, C, H, H, generator=g))
    dfeat = f32(torch.randn(N, C, generator=g))
    dx0 = bf(torch.randn(N, cin, hin, hin, generator=g))
    return dict(x=x, rows=rows, dy=dy, dfeat=dfeat, dx0=dx0, C=C, H=H, N=N, entry=entry)


def with_identity(rows, which):
    """the rows with conv1 (which = 1; plain blocks only) or conv2 (which = 2) replaced by the centre-tap identity; BatchNorm parameters kept"""
    out = [dict(r) for r in rows]
    r = out[0 if which == 1 else -1]
    assert r["w"].shape[0] == r["w"].shape[1] and r["k"] == 3 and r["s"] == 1
    r["w"] = ident_w(r["w"].shape[0]).to(r["w"].device)
    return out


def to_dev(case, dev):
    out = dict(case)
    for k in ("x", "dy", "dfeat", "dx0"):
        out[k] = case[k].to(dev)
    out["rows"] = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in r.items()} for r in case["rows"]]
    return out


# ------------------------------------------------------------------------------------------------ shared formulas
def _par(r):
    return r["gamma"].double(), r["beta"].double()


def _stats(zc, drop=False):
    """(s1, s2, M, mean, biased var clamped at 0) per channel of an NCHW tensor; drop: the last image is left out of the sums (a fault)"""
    M = zc.numel() // zc.shape[1]
    zs = zc[:-1] if drop else zc
    s1, s2 = zs.sum(dim=(0, 2, 3)), (zs * zs).sum(dim=(0, 2, 3))
    mean = s1 / M
    return s1, s2, M, mean, (s2 / M - mean * mean).clamp_min(0.0)


def _dyl(dy, dfeat, like):
    """the gradient of the block output as the kernel holds it: dy, or bf16(fl(dfeat * (1 / HW))) at every pixel -- 1 / HW is a power of two, so the fp32 product of
    the fp64 emulation is the kernel's bit for bit"""
    if dfeat is None:
        return dy.double()
    N, C, H, W = like.shape
    return bf(f32(dfeat.double() / (H * W)))[:, :, None, None].expand(N, C, H, W)


def wgrad_blocks(x, dz, k, s, p, ipg):
    """[blocks, K, C, k, k]: the weight gradient of every group of ipg consecutive images (the last one may be short)"""
    N, K = dz.shape[0], dz.shape[1]
    cols = torch.nn.functional.unfold(x, k, padding=p, stride=s)
    per = torch.einsum("nkp,njp->nkj", dz.reshape(N, K, -1), cols)
    nb = (N + ipg - 1) // ipg
    if ipg > 1:
        pad = torch.zeros(nb * ipg - N, *per.shape[1:], dtype=per.dtype, device=per.device)
        per = torch.cat([per, pad]).reshape(nb, ipg, *per.shape[1:]).sum(1)
    return per.reshape(nb, K, x.shape[1], k, k)


# ------------------------------------------------------------------------------------------------ the forward: teacher and emulator
def forward(x, rows, entry, rounded=True, fault=None, pool=True):
    """fp64 forward of one block; rounded: every stored tensor as the kernel stores it (the TEACHER of the backward tests, and the emulator of the forward).
    Returns z, mean, invstd, scale, shift, rm, rv, y per table row (y: a1 / the shortcut's BatchNorm output / the block output) and feat.  fault = (name, row)."""
    q = bf if rounded else (lambda t: t)
    q32 = f32 if rounded else (lambda t: t)
    x = x.double()
    n = len(rows)
    F = dict(z=[None] * n, mean=[None] * n, invstd=[None] * n, scale=[None] * n, shift=[None] * n, rm=[None] * n, rv=[None] * n, y=[None] * n)
    iB = n - 1
    for i, r in enumerate(rows):
        f = fault[0] if fault is not None and fault[1] == i else None
        inp = F["y"][0] if i == iB else x
        zc = CR._fwd(inp, q(r["w"].double()), r["s"], r["p"])
        _, _, M, mean, var = _stats(zc, drop=(f == "drop_image_fwd"))
        z = q(zc)
        ga, be = _par(r)
        mean32 = q32(mean)
        istd = q32(1.0 / torch.sqrt(q32(var) + B.EPS))
        sc = q32(ga * istd)
        sh = q32(be - q32(mean32 * sc))
        unb = 1.0 if f == "biased_var" else B.unbias_factor(M)
        F["rm"][i] = q32((1.0 - B.MOM) * r["rm0"].double() + B.MOM * mean32)
        F["rv"][i] = q32((1.0 - B.MOM) * r["rv0"].double() + B.MOM * q32(var * unb))
        v = z * sc[None, :, None, None] + sh[None, :, None, None]
        if i == iB:
            v = q32(v) + (F["y"][1] if entry else x)
        if not (entry and i == 1):
            v = v.clamp_min(0.0)
        F["z"][i], F["mean"][i], F["invstd"][i], F["scale"][i], F["shift"][i], F["y"][i] = z, mean32, istd, sc, sh, q(q32(v))
    F["feat"] = q32(F["y"][iB].mean(dim=(2, 3))) if pool else None
    return F


def judge_fwd(x, rows, entry, G, V=None, tag=""):
    """every forward link of one block.  G: what the launch stored -- the keys of `forward` (y[0] and, entry, y[1] stored because the test passes their pointers)."""
    V = Verdict() if V is None else V
    x = x.double()
    n, iB = len(rows), len(rows) - 1
    for i, r in enumerate(rows):
        inp = G["y"][0].double() if i == iB else x
        wq = bf(r["w"].double())
        ref, S = CR.conv_fwd_ref(inp, wq, r["s"], r["p"])
        Rk = r["k"] * r["k"] * wq.shape[1]
        V.add(tag + f"row{i}", "z", G["z"][i], ref, CR.elem_bound(S, Rk, ref, "bf16"))
        # ---- batch statistics of the fp64 convolution; the kernel's sums are those of its fp32 accumulators
        s1, s2, M, mean, var = _stats(ref)
        b1, b2 = CR.stat_bounds(ref, CR.acc_bound(S, Rk))
        noise = B.var_noise(s1, s2, M)
        d1 = b1 / M
        dv = b2 / M + 2 * mean.abs() * d1 + d1 * d1 + noise
        V.add(tag + f"row{i}", "mean", G["mean"][i], mean, d1 + B.bound_mean(mean))
        istd = 1.0 / torch.sqrt(var + B.EPS)
        hi, lo = 1.0 / torch.sqrt((var - dv).clamp_min(0.0) + B.EPS), 1.0 / torch.sqrt(var + dv + B.EPS)
        V.add(tag + f"row{i}", "invstd", G["invstd"][i], istd, torch.maximum(hi - istd, istd - lo) + B.E_ISTD["rsqrt"] * B.U * hi)
        unb = B.unbias_factor(M)
        rm0, rv0 = r["rm0"].double(), r["rv0"].double()
        V.add(tag + f"row{i}", "running_mean", G["rm"][i], B.running_update(rm0, mean), B.bound_running(rm0, mean) + B.MOM * d1)
        V.add(tag + f"row{i}", "running_var", G["rv"][i], B.running_update(rv0, var * unb), B.bound_running(rv0, var * unb, dv * unb))
        # ---- everything below is a function of the STORED mean / invstd / z
        ga, be = _par(r)
        mst, ist = G["mean"][i].double(), G["invstd"][i].double()
        sc = ga * ist
        V.add(tag + f"row{i}", "scale", G["scale"][i], sc, B.U * sc.abs() + B.FLOOR["f32"])
        scs = G["scale"][i].double()
        V.add(tag + f"row{i}", "shift", G["shift"][i], be - mst * scs, 2 * B.U * (be.abs() + (mst * scs).abs()) + B.FLOOR["f32"])
        zt = mc(G["z"][i].double())
        res = None
        if i == iB:
            res = mc(G["y"][1].double() if entry else x)
        pre = B.bn_fwd(zt, mst, ist, ga, be, res)
        refy = pre if (entry and i == 1) else pre.clamp_min(0.0)
        bd, _ = B.bound_y(refy, zt, mst, ist, ga, be, res, "bf16", "rsqrt")
        V.add(tag + f"row{i}", "y", G["y"][i], nchw(refy, G["z"][i]), nchw(bd, G["z"][i]))
    if G.get("feat") is not None:
        y = G["y"][iB].double()
        hw = y.shape[2] * y.shape[3]
        reff = y.mean(dim=(2, 3))
        V.add(tag + "block", "feat", G["feat"], reff, B.bound_pool_fwd(y.abs().sum(dim=(2, 3)), hw, reff))
    return V


# ------------------------------------------------------------------------------------------------ the backward: emulator
def _bn_bwd(g, z, mean, istd, gamma, rounded, drop=False):
    """(s1, s2, dz) of one BatchNorm backward: g the masked gradient; drop: the last image is left out of the sums (a fault)"""
    q = bf if rounded else (lambda t: t)
    M = z.numel() // z.shape[1]
    bc = lambda v: v[None, :, None, None]
    xhat = (z - bc(mean)) * bc(istd)
    gs, xs = (g[:-1], xhat[:-1]) if drop else (g, xhat)
    s1, s2 = gs.sum(dim=(0, 2, 3)), (gs * xs).sum(dim=(0, 2, 3))
    dz = q(bc(gamma * istd) * (g - bc(s1 / M) - xhat * bc(s2 / M)))
    return s1, s2, dz


def emulate_bwd(x, rows, entry, T, dy=None, dfeat=None, dx0=None, ipg=1, rounded=True, fault=None):
    """the backward of one block from the teacher's stored tensors T (`forward`): dgamma / dbeta (onto dg0 / db0), slab [blocks, K, C, k, k] per row, dx
    (accumulated onto dx0 when given), dz per row (what the group form stores).  fault = (name, row)."""
    q = bf if rounded else (lambda t: t)
    q32 = f32 if rounded else (lambda t: t)
    x = x.double()
    n, iB = len(rows), len(rows) - 1
    fl = lambda name, i: fault is not None and fault == (name, i)
    O = dict(dgamma=[None] * n, dbeta=[None] * n, slab=[None] * n, dz=[None] * n)

    def sums_to(i, s1, s2):
        r = rows[i]
        dg0, db0 = (torch.zeros_like(s1), torch.zeros_like(s1)) if fl("old_dgamma_ignored", i) else (r["dg0"].double(), r["db0"].double())
        O["dbeta"][i], O["dgamma"][i] = q32(db0 + q32(s1)), q32(dg0 + q32(s2))

    def blocks(i, inp, dz, g_ipg):
        r = rows[i]
        sl = wgrad_blocks(inp, dz, r["k"], r["s"], r["p"], g_ipg)
        if fl("group_last_twice", i):                            # the last image of the last group is counted twice
            sl[-1] = sl[-1] + wgrad_blocks(inp[-1:], dz[-1:], r["k"], r["s"], r["p"], 1)[0]
        return q32(sl)

    def dgrad(i, dz, H, W):
        r = rows[i]
        w = q(r["w"].double())
        if fl("tap_mirror", i) and r["k"] == 3:                  # the taps mirrored along x only
            w = w.flip(3)
        d = CR._dgrad(dz, w, r["s"], r["p"], H, W)
        if fl("entry_parity", i) and r["s"] == 2:                # the stride-2 parity classes shifted by one pixel
            d = torch.roll(d, shifts=(1, 1), dims=(2, 3))
        return d

    yB, zB, zA = T["y"][iB].double(), T["z"][iB].double(), T["z"][0].double()
    dyl = _dyl(dy, dfeat, yB)
    maskB = yB > 0
    gaA, beA = _par(rows[0])
    scA = q32(gaA * T["invstd"][0])
    shA = q32(beA - q32(T["mean"][0] * scA))
    preA = zA * scA[None, :, None, None] + shA[None, :, None, None]
    maskA = preA > 0
    a1 = q(q32(preA.clamp_min(0.0)))
    g2 = dyl * (maskA if fl("mask_other", iB) else maskB)
    s1, s2, dzB = _bn_bwd(g2, zB, T["mean"][iB], T["invstd"][iB], _par(rows[iB])[0], rounded, fl("drop_image_bwd", iB))
    sums_to(iB, s1, s2)
    O["dz"][iB] = dzB
    O["slab"][iB] = blocks(iB, a1, dzB, ipg)
    da1 = q(q32(dgrad(iB, dzB, a1.shape[2], a1.shape[3])))
    g1 = da1 * (maskB if fl("mask_other", 0) else maskA)
    s1, s2, dzA = _bn_bwd(g1, zA, T["mean"][0], T["invstd"][0], gaA, rounded, fl("drop_image_bwd", 0))
    sums_to(0, s1, s2)
    O["dz"][0] = dzA
    resg = dyl if fault is not None and fault[0] == "res_before_mask" else g2
    if fault is not None and fault[0] == "res_grad_drop":
        resg = torch.zeros_like(g2)
    old = None if (dx0 is None or (fault is not None and fault[0] == "dx_overwrite")) else dx0.double()
    if entry:
        zD = T["z"][1].double()
        s1, s2, dzD = _bn_bwd(resg, zD, T["mean"][1], T["invstd"][1], _par(rows[1])[0], rounded, fl("drop_image_bwd", 1))
        sums_to(1, s1, s2)
        O["dz"][1] = dzD
        d = dgrad(0, dzA, x.shape[2], x.shape[3]) + dgrad(1, dzD, x.shape[2], x.shape[3])
        O["dx"] = q(q32(d if old is None else q32(d) + old))
        O["slab"][0] = blocks(0, x, dzA, 1)
        O["slab"][1] = blocks(1, x, dzD, 1)
    else:
        d = q32(q(q32(dgrad(0, dzA, x.shape[2], x.shape[3]))) + resg)
        O["dx"] = q(d if old is None else q32(d + old))
        O["slab"][0] = blocks(0, x, dzA, ipg)
    return O


# ------------------------------------------------------------------------------------------------ the backward: verdict
def _bn_bwd_link(V, key, r, g, bg, gmag, z, mean, istd, dgamma, dbeta, e_mean=0.0, e_i=0.0):
    """the sums and the dz of one BatchNorm backward from its (reference, bound, magnitude) of the masked gradient; returns (dz, its bound) NCHW.  e_mean, e_i:
    absolute error of `mean` and relative error of `istd` against the values the kernel worked with (statistics RECOVERED from running statistics, as in
    plan_ref.judge, whose terms these are: xhat moves by istd e_mean + |xhat| e_i); 0 where the test supplied the statistics itself"""
    zt, gt, bgt, gm = mc(z), mc(g), mc(bg), mc(gmag)
    M = zt.shape[0]
    ga = r["gamma"].double()
    xhat = (zt - mean) * istd
    s1, s2 = gt.sum(0), (gt * xhat).sum(0)
    ds1 = B.bound_sum(M, B.T_SUM1, gm.sum(0)) + bgt.sum(0)
    dxh = istd * e_mean + xhat.abs() * e_i
    ds2 = B.bound_sum(M, B.T_SUM2, (gm * xhat.abs()).sum(0)) + (bgt * xhat.abs()).sum(0) + (gm * dxh).sum(0)
    dg0, db0 = r["dg0"].double(), r["db0"].double()
    V.add(key, "dbeta", dbeta, db0 + s1, B.bound_grad_store(db0, s1, ds1))
    V.add(key, "dgamma", dgamma, dg0 + s2, B.bound_grad_store(dg0, s2, ds2))
    gi = ga * istd
    k0, k1 = s1 / M, s2 / M
    dz = gi * (gt - k0 - xhat * k1)
    bdz = B.bound_dz(dz, gm, xhat, gi, k0, k1, "bf16", ds1 / M, ds2 / M) + (1 + R16) * (gi.abs() * bgt + e_i * dz.abs() + gi.abs() * k1.abs() * dxh)
    return nchw(dz, z), nchw(bdz, z)


def _slab_link(V, key, r, inp, b_inp, dz, bdz, got, ipg):
    """the weight-gradient blocks as the kernel leaves them, and their sum in block order"""
    k, s, p = r["k"], r["s"], r["p"]
    ref = wgrad_blocks(inp, dz, k, s, p, ipg)
    S = wgrad_blocks(inp.abs(), dz.abs(), k, s, p, ipg)
    prop = wgrad_blocks(inp.abs() + b_inp, bdz, k, s, p, ipg) + wgrad_blocks(b_inp, dz.abs(), k, s, p, ipg)
    px = dz.shape[2] * dz.shape[3]
    V.add(key, "slab", got, ref, CR.wgrad_bound(S, min(ipg, dz.shape[0]) * px) + prop)
    V.add(key, "dw", got.double().sum(0), ref.sum(0), CR.wgrad_bound(S.sum(0), dz.shape[0] * px) + prop.sum(0))


def judge_bwd(x, rows, entry, T, O, dy=None, dfeat=None, dx0=None, ipg=1, V=None, tag="", ipg_entry=1, bdy=None, stat_err=None):
    """every backward link of one block.  T: the tensors the launch was GIVEN (z, y, mean, invstd per row); O: what it left (dgamma, dbeta, slab per row, dx,
    and dz per row where the group form stored it, else None).  ipg: images per weight-gradient block of the stride-1 rows; ipg_entry: of an entry block's two
    strided rows (the kernel: always 1).  For a CHAIN of blocks inside a run (the plan-level judgement): bdy = the bound of an unseen dy (the dx of the block
    behind, which V.dx returns as (reference, bound)); stat_err = per row (e_mean, e_i) of recovered statistics (see _bn_bwd_link); O["dx"] None: not stored.  Sets V.ambig[tag] to the share of a1's elements whose mask is ambiguous."""
    V = Verdict() if V is None else V
    x = x.double()
    n, iB = len(rows), len(rows) - 1
    dzs = O.get("dz") or [None] * n
    yB, zB, zA = T["y"][iB].double(), T["z"][iB].double(), T["z"][0].double()
    mA, iA, mB, iBs = (T[k][i].double() for k, i in (("mean", 0), ("invstd", 0), ("mean", iB), ("invstd", iB)))
    dyl = _dyl(dy, dfeat, yB)
    g2 = dyl * (yB > 0)
    bg2 = torch.zeros_like(g2) if bdy is None else bdy * (yB > 0)
    se = stat_err if stat_err is not None else [(0.0, 0.0)] * n
    dzB, bdzB = _bn_bwd_link(V, tag + f"row{iB}", rows[iB], g2, bg2, g2.abs() + bg2, zB, mB, iBs, O["dgamma"][iB], O["dbeta"][iB], *se[iB])
    if dzs[iB] is not None:
        V.add(tag + f"row{iB}", "dz", dzs[iB], dzB, bdzB)
    # ---- conv2's operand a1, rebuilt by the kernel from z1 and the given statistics, and its mask
    gaA, beA = _par(rows[0])
    ztA = mc(zA)
    preA = B.bn_fwd(ztA, mA, iA, gaA, beA)
    a1t = preA.clamp_min(0.0)
    ba1, fpA = B.bound_y(a1t, ztA, mA, iA, gaA, beA, None, "bf16", "rsqrt", se[0][1])
    shiftA = (gaA * iA).abs() * se[0][0]                         # (a recovered mean's own error moves the pre-ReLU value by scale * e_mean)
    ba1, fpA = ba1 + (1 + R16) * shiftA, fpA + shiftA
    a1, ba1 = nchw(a1t, zA), nchw(ba1, zA)
    amb = nchw((preA.abs() <= fpA).double(), zA)
    V.ambig[tag or "block"] = float(amb.sum()) / amb.numel()
    _slab_link(V, tag + f"row{iB}", rows[iB], a1, ba1, dzB, bdzB, O["slab"][iB], ipg)
    # ---- the gradient of a1 (unseen), masked
    wB = bf(rows[iB]["w"].double())
    da1, Sd = CR.conv_dgrad_ref(dzB, wB, 1, 1, a1.shape[2], a1.shape[3])
    bda1 = CR.elem_bound(Sd, 9 * wB.shape[0], da1, "bf16") + CR._dgrad(bdzB, wB.abs(), 1, 1, a1.shape[2], a1.shape[3])
    mask = (nchw(preA, zA) > 0).double()
    g1 = da1 * mask
    bg1 = torch.maximum(mask, amb) * bda1 + amb * da1.abs()
    dzA, bdzA = _bn_bwd_link(V, tag + "row0", rows[0], g1, bg1, g1.abs() + bg1, zA, mA, iA, O["dgamma"][0], O["dbeta"][0], *se[0])
    if dzs[0] is not None:
        V.add(tag + "row0", "dz", dzs[0], dzA, bdzA)
    r0 = rows[0]
    wA = bf(r0["w"].double())
    Hi, Wi = x.shape[2], x.shape[3]
    dA, SA = CR.conv_dgrad_ref(dzA, wA, r0["s"], r0["p"], Hi, Wi)
    propA = CR._dgrad(bdzA, wA.abs(), r0["s"], r0["p"], Hi, Wi)
    old = None if dx0 is None else dx0.double()
    if entry:
        r1 = rows[1]
        zD = T["z"][1].double()
        dzD, bdzD = _bn_bwd_link(V, tag + "row1", r1, g2, bg2, g2.abs() + bg2, zD, T["mean"][1].double(), T["invstd"][1].double(), O["dgamma"][1], O["dbeta"][1], *se[1])
        if dzs[1] is not None:
            V.add(tag + "row1", "dz", dzs[1], dzD, bdzD)
        wD = bf(r1["w"].double())
        dD, SD = CR.conv_dgrad_ref(dzD, wD, 2, 0, Hi, Wi)
        d, S = dA + dD, SA + SD
        prop = propA + CR._dgrad(bdzD, wD.abs(), 2, 0, Hi, Wi)
        V.dx = (d if old is None else d + old, CR.elem_bound(S, 9 * wA.shape[0] + wD.shape[0], d, "bf16", old=old) + prop * (1 + R16))
        _slab_link(V, tag + "row0", r0, x, torch.zeros_like(x), dzA, bdzA, O["slab"][0], ipg_entry)
        _slab_link(V, tag + "row1", r1, x, torch.zeros_like(x), dzD, bdzD, O["slab"][1], ipg_entry)
    else:
        bd = CR.elem_bound(SA, 9 * wA.shape[0], dA, "bf16") + propA + bg2    # of bf16(dgrad), and of the residual gradient where dy itself is unseen
        tot = dA + g2 if old is None else dA + g2 + old
        bnd = bd + B.bound_dres_acc(tot.abs() + bd, "bf16")                  # + the residual gradient: one fp32 add, one storage rounding
        if old is not None:
            bnd = bnd + B.U * (tot.abs() + bd)                               # ... and one more fp32 add
        V.dx = (tot, bnd)
        _slab_link(V, tag + "row0", r0, x, torch.zeros_like(x), dzA, bdzA, O["slab"][0], ipg)
    if O.get("dx") is not None:
        V.add(tag + "block", "dx", O["dx"], *V.dx)
    return V


def case_seed(C, N, entry):
    """the seed of the GPU file's case at (C, N, entry); the CPU file walks the same list for the ambiguity cap"""
    return SEEDS[C] + (100 if entry else 0) + 7 * N


def ambiguous_share(case):
    """the share judge_bwd would report for a case, from the reference alone (conv1 and its BatchNorm)"""
    r = case["rows"][0]
    x = case["x"].double()
    zc = CR._fwd(x, bf(r["w"].double()), r["s"], r["p"])
    _, _, M, mean, var = _stats(zc)
    mean32, istd = f32(mean), f32(1.0 / torch.sqrt(f32(var) + B.EPS))
    ga, be = _par(r)
    zt = mc(bf(zc))
    pre = B.bn_fwd(zt, mean32, istd, ga, be)
    _, fp = B.bound_y(pre.clamp_min(0.0), zt, mean32, istd, ga, be, None, "bf16", "rsqrt")
    return float((pre.abs() <= fp).sum()) / pre.numel()
