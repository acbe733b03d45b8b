"""Teacher-forced fp64 reference of the ViT executor (csrc/vit_plan.hip: clhip_vit_forward, clhip_vit_backward) -- a helper module, not a conftest; what
tests/plan_ref.py is for the ResNet plan.  Plain torch fp64 on the CPU; the project is not imported.

The idea.  The executor keeps every link of  images -> patches -> tokens -> depth x [LN1 -> qkv -> attention -> proj(+res) -> LN2 -> fc1(GELU) -> fc2(+res)
(+ adapter)] -> feat  in its workspace, and with a gradient tap set (clhip_vit_set_tap) every buffer of the backward chain as well.  `judge` takes ONE read of
all of them (a dict, see `emulate` for its keys; everything in it is already in storage precision) and computes, per launch, what its output must be FROM THE
EXECUTOR'S OWN STORED INPUTS of that launch, with an allowed error per element.  A wiring fault -- a stale h1 at the LoRA gradient, LN2's statistics at LN1's
backward, a lost += of a residual gradient, a g / g2 swap too many, a break one layer too high, a leaf that reads dqkv too late -- then breaks exactly one
link by far more than a rounding bound instead of hiding in an end-to-end tolerance.  References and bounds are those of the modules that already hold each
kernel alone (gemm_ref, vit_refs, adapter_ref, sdlora_ref, lorasub_ref, coda_ref); nothing is fitted to a kernel's output; a verdict is max over the elements of
err / bound <= 1.

Unseen tensors.  Two forward tensors are scratch and cannot be read: the LN2 output and the GELU output (and h1 where it aliases the LN2 scratch).  Their
links are chained: the reference of the unseen tensor feeds the next launch's reference, and its bound is carried through |W| into the next bound.

Two writers.  g is written by the pooled-LN backward (or the layer above) and accumulated into by each LN backward; x_in[l + 1] is written by the fc2 GEMM
and added to by the adapter.  The link's input is the stored value before the second writer (g: the tap of the writer before; x_in[l + 1]: the fc2
reference, whose own bound is carried), and the bound counts one storage rounding per write.

The reference statistics of a LayerNorm link are recomputed from the stored input; the stored statistics are tied to them by their own link (mean_floor,
rstd_floor: LSE_ABS, LN_MEAN_REL and LN_RSTD_REL are not measured, so the forward-bound floors decide alone)."""
import math

import torch

import adapter_ref as AR
import coda_ref as CR
import gemm_ref as G
import lorasub_ref as LR
import sdlora_ref as SR
import vit_refs as VR
from plan_ref import Verdict
from vit_refs import U, larger

# ------------------------------------------------------------------------------------------------ the case list
GEOS = {
    "t64": dict(img=32, patch=8, dim=64, heads=2, mlp=256, depth=3),       # head dim 32: generic attention in both types
    "t128": dict(img=32, patch=8, dim=128, heads=2, mlp=256, depth=3),     # head dim 64: the bf16 MFMA forward and the general MFMA backward
    "d1": dict(img=32, patch=8, dim=64, heads=2, mlp=256, depth=1),        # the per-layer Gram path; a backward that breaks in its first iteration
}
BATCHES = [(3, 0), (5, 4)]                                                 # (batch, prompt tokens): N = 17, M = 51 and N = 21, M = 105
MODES = ["lora", "prompt", "adapter", "adapter_drop", "sdlora", "prefix", "prefix_prompt", "lora_ab"]        # lora_ab: LoRA-Sub, A and B both train
CASES = [(g, m) for g in ("t64", "t128") for m in MODES] + [("d1", "lora"), ("d1", "prefix")]
LORA_RANK, ADAPTER_DIM, ADAPTER_SCALE, DROP_P, SD_RANKS, BLOCK_EPS = 4, 16, 0.1, 0.1, (4, 6), 1e-5
PREFIX_LP = {3: [0, 3, 8], 1: [3]}                                         # Lp[0] == 0 at depth 3: the prefix-only backward stops at layer 1
FAULTS = ["stale_h1", "ln1_st2", "lost_plus", "swap_twice", "break_high", "dqkv_late", "ad_wgrad_post_swap", "gram_from_ln2"]
FAULT_MODE = dict(stale_h1="lora", ln1_st2="lora", lost_plus="lora", swap_twice="adapter", break_high="prefix", dqkv_late="lora",
                  ad_wgrad_post_swap="adapter", gram_from_ln2="lora")
FAULT_LAYER = 1
# the tap's slots of one layer, in buffer order (include/clhip.h, clhip_vit_set_tap)
SLOTS = ["dbig", "ad_dh", "ad_gx", "dfc1", "g_ln2", "dproj", "dqkv", "dqin", "g_ln1"]


def _ws_totals():
    """clhip_vit_workspace_bytes of every (case, type, batch, prompt tokens, flags) the tests use, recorded from the build BEFORE the read access was added
    (key "<geo>-<mode>-<type>-b<B>-p<n_prompt>-f<flags>"): the read access and the tap are host bookkeeping and copies, they cost no workspace"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit_ws_totals.json")) as f:
        return json.load(f)


WS_TOTALS = _ws_totals()


def case_id(c):
    return f"{c[0]}-{c[1]}"


def mode_cfg(geo, mode):
    c = dict(GEOS[geo], lora_rank=LORA_RANK if mode in ("lora", "lora_ab") else 0, adapter_dim=ADAPTER_DIM if mode.startswith("adapter") else 0,
             p=DROP_P if mode == "adapter_drop" else 0.0, sd=mode == "sdlora", prefix=mode.startswith("prefix"), mode=mode)
    c["np"] = (c["img"] // c["patch"]) ** 2
    c["Kp"] = 3 * c["patch"] ** 2
    c["Lp"] = PREFIX_LP[c["depth"]] if c["prefix"] else [0] * c["depth"]
    return c


def batches_of(mode):
    """the (batch, prompt tokens) pairs a mode runs at: the prompt modes need prompt tokens"""
    return [(5, 4)] if mode in ("prompt", "prefix_prompt") else BATCHES


def wants(c, n_prompt):
    """which parameter gradients a step of this mode asks for"""
    m = c["mode"]
    return dict(dprompt=n_prompt > 0 and m != "prefix", lora=m == "lora", adapter=c["adapter_dim"] > 0, sd=c["sd"], prefix=c["prefix"], ab=m == "lora_ab")


def lowest_layer(c, n_prompt):
    w = wants(c, n_prompt)
    if w["prefix"] and not (w["dprompt"] or w["lora"] or w["adapter"] or w["sd"] or w["ab"]):
        return next(l for l, lp in enumerate(c["Lp"]) if lp > 0)
    return 0


def written_slots(c, n_prompt, lowest=None):
    """the (layer, slot) pairs a backward writes (layer -1: g after the pooled-LN backward): every layer from the top down to `lowest`; the qkv dgrad and the LN1
    backward of the lowest layer only when the prompt gradient needs them"""
    lowest = lowest_layer(c, n_prompt) if lowest is None else lowest
    dpr = wants(c, n_prompt)["dprompt"]
    out = {(-1, "g0")}
    for l in range(c["depth"] - 1, lowest - 1, -1):
        for s in SLOTS:
            if s in ("ad_dh", "ad_gx") and not c["adapter_dim"]:
                continue
            if s in ("dqin", "g_ln1") and l == lowest and not dpr:
                continue
            out.add((l, s))
    return out


def slot_floats(c, M, slot):
    D, R = c["dim"], c["adapter_dim"]
    return {"dbig": M * c["mlp"], "ad_dh": M * R, "ad_gx": M * D if R else 0, "dqkv": 3 * M * D}.get(slot, M * D)


def tap_map(c, M):
    """{(layer, slot): (offset, floats, columns)} of the tap buffer, and its size (the documented layout of clhip_vit_set_tap)"""
    D = c["dim"]
    out, off = {(-1, "g0"): (0, M * D, D)}, M * D
    for l in range(c["depth"]):
        for s in SLOTS:
            n = slot_floats(c, M, s)
            if n:
                out[(l, s)] = (off, n, n // M)
            off += n
    return out, off


# ------------------------------------------------------------------------------------------------ seeded inputs
def q(t, dt):
    """a value as its storage type holds it (None: no rounding)"""
    if dt is None:
        return t
    return t.float().to(torch.bfloat16).double() if dt == "bf16" else t.float().double()


def qf_of(dt):
    return AR.bf16 if dt == "bf16" else AR.ident


def trained_like(geo, mode, seed):
    """seeded fp32 parameters of a net that has trained for a while: LN gammas 1 + 0.3 randn with both signs and one zero, a non-zero lora_B, a non-zero
    adapter up-projection, two SD-LoRA terms of unequal rank"""
    c = mode_cfg(geo, mode)
    g = torch.Generator().manual_seed(seed)
    D, H, Kp = c["dim"], c["mlp"], c["Kp"]
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).float()

    def gamma():
        t = 1.0 + 0.3 * torch.randn(D, generator=g)
        t[3], t[5] = -t[3].abs() - 0.1, 0.0
        return t.float()
    P = dict(pe_w=rn(D, Kp, sc=1 / math.sqrt(Kp)), pe_b=rn(D, sc=0.1), cls=rn(D, sc=0.5), pos=rn(c["np"] + 1, D, sc=0.5), norm_w=gamma(), norm_b=rn(D, sc=0.1),
             prompt=rn(4, D, sc=0.5), layers=[])
    for l in range(c["depth"]):
        L = dict(qkv_w=rn(3 * D, D, sc=1.5 / math.sqrt(D)), qkv_b=rn(3 * D, sc=0.1), proj_w=rn(D, D, sc=1 / math.sqrt(D)), proj_b=rn(D, sc=0.1), ln1_w=gamma(),
                 ln1_b=rn(D, sc=0.1), fc1_w=rn(H, D, sc=1 / math.sqrt(D)), fc1_b=rn(H, sc=0.1), fc2_w=rn(D, H, sc=1 / math.sqrt(H)), fc2_b=rn(D, sc=0.1), ln2_w=gamma(),
                 ln2_b=rn(D, sc=0.1))
        if c["lora_rank"]:
            r = c["lora_rank"]
            L.update(lora_a_k=rn(r, D, sc=1 / math.sqrt(D)), lora_b_k=rn(D, r, sc=0.2), lora_a_v=rn(r, D, sc=1 / math.sqrt(D)), lora_b_v=rn(D, r, sc=0.2))
        if c["adapter_dim"]:
            L["adapter"] = [t.float() for t in AR.adapter_params(D, c["adapter_dim"], seed + 31 * l + 7)]
        if c["sd"]:
            L["sd"] = [[torch.empty(*((r, D) if w % 2 == 0 else (D, r))).uniform_(-0.3, 0.3, generator=g) for r in SD_RANKS] for w in range(4)]
            L["sd_inv"] = torch.stack([SR.inv_norms(L["sd"][0], L["sd"][1]), SR.inv_norms(L["sd"][2], L["sd"][3])]).float()
        P["layers"].append(L)
    if c["sd"]:
        P["sd_mag"] = torch.empty(len(SD_RANKS)).uniform_(0.5, 1.5, generator=g)
    return P


def step_inputs(c, B, n_prompt, seed, dt):
    """images, dfeat, the prefixes (already in the compute dtype's values) and, with dropout, the seeded keep masks of the CPU emulator"""
    g = torch.Generator().manual_seed(seed + 1000 * B)
    X = dict(img=torch.randn(B, 3, c["img"], c["img"], generator=g), dfeat=torch.randn(B, c["dim"], generator=g), B=B, n_prompt=n_prompt)
    X["pk"] = [None if not lp else q(torch.randn(B * lp, c["dim"], generator=g), dt).float() for lp in c["Lp"]]
    X["pv"] = [None if not lp else q(torch.randn(B * lp, c["dim"], generator=g), dt).float() for lp in c["Lp"]]
    M = B * (n_prompt + 1 + c["np"])
    X["mask"] = [(torch.rand(M, c["adapter_dim"], generator=g) >= c["p"]).to(torch.uint8) if c["p"] > 0 else None for _ in range(c["depth"])]
    return X


def eff_qkv(c, L, P):
    """the fp64 effective qkv weight of a layer, and (SD-LoRA) the |terms| mass of its bound"""
    W = L["qkv_w"].double()
    if c["lora_rank"]:
        return VR.weight_eff_ref(L["qkv_w"], L["lora_a_k"], L["lora_b_k"], L["lora_a_v"], L["lora_b_v"]), None
    if c["sd"]:
        d = [[t.double() for t in ts] for ts in L["sd"]]
        mag, inv = P["sd_mag"].double(), L["sd_inv"].double()
        eff = SR.effective_qkv(W, d[0], d[1], d[2], d[3], mag, inv[0], inv[1])
        ab = lambda w: sum((mag[i] * inv[w, i]).abs() * (d[2 * w + 1][i].abs() @ d[2 * w][i].abs()) for i in range(len(SD_RANKS)))
        Dm = c["dim"]
        mass = torch.cat([W[:Dm].abs() + ab(0), torch.zeros(Dm, Dm, dtype=torch.float64), W[2 * Dm:].abs() + ab(1)])
        return eff, mass
    return W, None


# ------------------------------------------------------------------------------------------------ small closed forms
def rows(t, B, H, hd):
    """[B, H, n, hd] -> [B * n, H * hd]"""
    return t.permute(0, 2, 1, 3).reshape(-1, H * hd)


def ln_dx(x, gamma, dy, mu, rstd):
    """the LayerNorm input gradient from GIVEN statistics (what the kernel computes from its saved pair)"""
    xh = (x - mu[:, None]) * rstd[:, None]
    dg = dy * gamma
    return rstd[:, None] * (dg - dg.mean(-1, keepdim=True) - xh * (dg * xh).mean(-1, keepdim=True))


def attention(c, qkv, pk, pv, dout, B, N, Lp):
    """(packed qkv, packed dout) of one layer: the prefix form written as plain attention over Lp + N tokens (coda_ref.pack_prefix)"""
    D = c["dim"]
    if dout is None:
        dout = torch.zeros(B * N, D, dtype=torch.float64)
    if not Lp:
        return qkv, dout
    return CR.pack_prefix(qkv.reshape(B, N, 3 * D), pk.double().reshape(B, Lp, D), pv.double().reshape(B, Lp, D), dout.reshape(B, N, D), B, N, Lp, D)


# ------------------------------------------------------------------------------------------------ the CPU emulator
def emulate(c, P, X, dt, fault=None, gram0=None, grads0=None):
    """the executor's step in fp64 with a rounding to the storage type `dt` wherever the executor stores (None: no rounding at all).  Returns the dict a read of
    a step returns:
      B, N, M, n_prompt, dt; img, dfeat; pe_wf, wf[l] / wb[l] = {qkv, proj, fc1, fc2}: the compute-dtype weight copies ([rows, cols] / transposed);
      patches, pe_out, x[l] (depth + 1 entries), h1[l] (None where it aliases scratch), st1[l] / st2[l] [2, M], qkv[l], lse[l] [B, H, N], attn_o[l], x_mid[l],
      hpre[l], ad_hd[l], feat; gram0 / gram [depth, D, D] (None: no Gram pass); tap {(layer, slot): tensor} of the slots the backward wrote;
      dprompt, d_lora_b[l] = (dBk, dBv) and d_lora_b0 (the value accumulated onto), d_adapter[l] = (dWd, dbd, dWu, dbu), d_sd[l] = (dAq, dBq, dAv, dBv),
      d_ab[l] = (dAk, dBk, dAv, dBv), d_mag_rows, d_mag, dpk[l], dpv[l]; mask[l]; lowest.
    `fault` seeds ONE wiring fault (FAULTS) at layer FAULT_LAYER."""
    B, n_prompt = X["B"], X["n_prompt"]
    D, Hh, H, depth, eps = c["dim"], c["heads"], c["mlp"], c["depth"], BLOCK_EPS
    hd, N = D // Hh, n_prompt + 1 + c["np"]
    M, Pp = B * N, max(n_prompt, 1)
    w, qq, qf = wants(c, n_prompt), (lambda t: q(t, dt)), (AR.ident if dt is None else qf_of(dt))
    f32 = (lambda t: t) if dt is None else (lambda t: t.float().double())
    fl = fault if fault else ""
    keep_h1 = bool(c["lora_rank"] or c["sd"])
    R = dict(B=B, N=N, M=M, n_prompt=n_prompt, dt=dt, img=X["img"].double(), dfeat=X["dfeat"].double(), mask=X["mask"], pk=X["pk"], pv=X["pv"])
    R["pe_wf"] = qq(P["pe_w"].double())
    R["wf"], R["wb"] = [], []
    for L in P["layers"]:
        wfl = dict(qkv=qq(f32(eff_qkv(c, L, P)[0])), proj=qq(L["proj_w"].double()), fc1=qq(L["fc1_w"].double()), fc2=qq(L["fc2_w"].double()))
        R["wf"].append(wfl)
        R["wb"].append({k: v.T.contiguous() for k, v in wfl.items()})
    R["patches"] = qq(VR.patchify_ref(X["img"].double(), c["patch"]))
    R["pe_out"] = qq(R["patches"] @ R["pe_wf"].T + P["pe_b"].double())
    x = [qq(VR.assemble_ref(R["pe_out"], P["cls"], P["pos"], P["prompt"] if n_prompt else None, B, c["np"], n_prompt, D))]
    for k in ("h1", "st1", "st2", "qkv", "lse", "attn_o", "x_mid", "hpre", "ad_hd"):
        R[k] = [None] * depth
    gsrc, h1_all = [None] * depth, []
    for l, L in enumerate(P["layers"]):
        wfl = R["wf"][l]
        y, mu, rstd, _ = VR.ln_ref(x[l], L["ln1_w"], L["ln1_b"], torch.zeros_like(x[l]), eps)
        R["st1"][l] = torch.stack([f32(mu), f32(rstd)])
        h1 = qq(y)
        R["qkv"][l] = qq(h1 @ wfl["qkv"].T + L["qkv_b"].double())
        Lp = c["Lp"][l]
        big, bd = attention(c, R["qkv"][l], X["pk"][l], X["pv"][l], None, B, N, Lp)
        o, lse, _, _, _ = VR.attn_ref(big, bd, B, N + Lp, Hh, hd)
        R["attn_o"][l], R["lse"][l] = qq(rows(o[:, :, Lp:], B, Hh, hd)), f32(lse[:, :, Lp:])
        R["x_mid"][l] = qq(R["attn_o"][l] @ wfl["proj"].T + L["proj_b"].double() + x[l])
        y2, mu2, rstd2, _ = VR.ln_ref(R["x_mid"][l], L["ln2_w"], L["ln2_b"], torch.zeros_like(x[l]), eps)
        R["st2"][l] = torch.stack([f32(mu2), f32(rstd2)])
        ln_out = qq(y2)
        act, hp = G.gelu_both(ln_out @ wfl["fc1"].T + L["fc1_b"].double())
        R["hpre"][l] = qq(hp)
        xo = qq(qq(act) @ wfl["fc2"].T + L["fc2_b"].double() + R["x_mid"][l])
        if c["adapter_dim"]:
            Wd, bd_, Wu, bu = [t.double() for t in L["adapter"]]
            delta, hdn = AR.fwd(R["x_mid"][l], Wd, bd_, Wu, bu, ADAPTER_SCALE, X["mask"][l], c["p"], qf)
            R["ad_hd"][l], xo = hdn, qq(xo + delta)
        x.append(xo)
        R["h1"][l] = h1 if (keep_h1 or gram0 is not None) else None
        gsrc[l] = ln_out if (fl == "gram_from_ln2" and l == FAULT_LAYER) else h1
        h1_all.append(h1)
    R["x"] = x
    R["gram0"] = gram0
    R["gram"] = None if gram0 is None else torch.stack([f32(gram0[l].double() + VR.gram_ref(gsrc[l])) for l in range(depth)])
    feat, g = VR.ln_pool_ref(x[depth], P["norm_w"], P["norm_b"], X["dfeat"], B, N, D, Pp, 1e-6)
    R["feat"] = f32(feat)
    # ---- backward
    lowest = lowest_layer(c, n_prompt)
    R["lowest"] = lowest
    stop = lowest + 1 if (fl == "break_high" and lowest + 1 < depth) else lowest
    tap = {(-1, "g0"): qq(g.reshape(M, D))}
    g = tap[(-1, "g0")]
    grads0 = grads0 or {}
    R["d_lora_b0"] = grads0.get("d_lora_b", [(torch.zeros(D, LORA_RANK, dtype=torch.float64),) * 2] * depth)
    for k in ("d_lora_b", "d_adapter", "d_sd", "d_ab", "dpk", "dpv"):
        R[k] = [None] * depth
    dq_of = [None] * depth
    for l in range(depth - 1, stop - 1, -1):
        L, wfl = P["layers"][l], R["wf"][l]
        tap[(l, "dbig")] = qq((g @ wfl["fc2"]) * R["hpre"][l])
        if c["adapter_dim"]:
            Wd, _, Wu, _ = [t.double() for t in L["adapter"]]
            dx, _, _, _, _, dh = AR.bwd(g, R["x_mid"][l], R["ad_hd"][l], Wd, Wu, ADAPTER_SCALE, c["p"], qf)
            gx = qq(g + dx)
            tap[(l, "ad_dh")], tap[(l, "ad_gx")] = dh, gx
            if w["adapter"]:
                gy = gx if (fl == "ad_wgrad_post_swap" and l == FAULT_LAYER) else g
                R["d_adapter"][l] = tuple(f32(t) for t in (dh.T @ R["x_mid"][l], dh.sum(0), ADAPTER_SCALE * gy.T @ R["ad_hd"][l], ADAPTER_SCALE * gy.sum(0)))
            if not (fl == "swap_twice" and l == FAULT_LAYER):
                g = gx
        tap[(l, "dfc1")] = qq(tap[(l, "dbig")] @ wfl["fc1"])
        dx2 = ln_dx(R["x_mid"][l], L["ln2_w"].double(), tap[(l, "dfc1")], R["st2"][l][0], R["st2"][l][1])
        g = qq(dx2 if (fl == "lost_plus" and l == FAULT_LAYER) else g + dx2)
        tap[(l, "g_ln2")] = g
        tap[(l, "dproj")] = qq(g @ wfl["proj"])
        Lp = c["Lp"][l]
        big, bd = attention(c, R["qkv"][l], X["pk"][l], X["pv"][l], tap[(l, "dproj")], B, N, Lp)
        _, _, dq, dk, dv = VR.attn_ref(big, bd, B, N + Lp, Hh, hd)
        tap[(l, "dqkv")] = qq(torch.cat([rows(t[:, :, Lp:], B, Hh, hd) for t in (dq, dk, dv)], 1))
        if Lp and w["prefix"]:
            R["dpk"][l], R["dpv"][l] = f32(rows(dk[:, :, :Lp], B, Hh, hd)), f32(rows(dv[:, :, :Lp], B, Hh, hd))
        dq_of[l] = tap[(l, "dqkv")]
        if l == stop and not w["dprompt"]:
            break
        tap[(l, "dqin")] = qq(tap[(l, "dqkv")] @ wfl["qkv"])
        st = R["st2"][l] if (fl == "ln1_st2" and l == FAULT_LAYER) else R["st1"][l]
        g = qq(g + ln_dx(x[l], L["ln1_w"].double(), tap[(l, "dqin")], st[0], st[1]))
        tap[(l, "g_ln1")] = g
    # the leaves: they read h1[l] and dqkv as layer l left it (dqkv_late: as the layer below left it)
    for l in range(depth - 1, stop - 1, -1):
        L = P["layers"][l]
        h1 = h1_all[(l + 1) % depth] if (fl == "stale_h1" and l == FAULT_LAYER) else h1_all[l]
        dqkv = dq_of[l - 1] if (fl == "dqkv_late" and l == FAULT_LAYER) else dq_of[l]
        if w["lora"]:
            rk, rv = VR.lora_db_ref(h1, dqkv, qq(L["lora_a_k"].double()), qq(L["lora_a_v"].double()), D)
            R["d_lora_b"][l] = (f32(R["d_lora_b0"][l][0] + rk), f32(R["d_lora_b0"][l][1] + rv))
        if w["sd"]:
            want, _ = SR.grads_bounded(h1, dqkv, L["sd"], P["sd_mag"], L["sd_inv"], qq, 0.0)
            R["d_sd"][l] = tuple(f32(t) for t in want[:4])
            R.setdefault("d_mag_rows", torch.zeros(depth, len(SD_RANKS), dtype=torch.float64))[l] = f32(want[4])
        if w["ab"]:
            R["d_ab"][l] = tuple(f32(t) for t in LR.grads_ab(h1, dqkv, *[qq(L[k].double()) for k in ("lora_a_k", "lora_b_k", "lora_a_v", "lora_b_v")]))
    if w["sd"]:
        R["d_mag"] = f32(R["d_mag_rows"].sum(0))
    R["dprompt"] = f32(VR.prompt_grad_ref(g, B, N, n_prompt, D)) if w["dprompt"] else None
    R["tap"] = tap
    return R


# ------------------------------------------------------------------------------------------------ the verdicts
def _gemm(V_, key, got, A, Bw, bias, Rs, Hs, epi, dt, bA=None):
    """one GEMM link: got (None: unseen) against gemm_ref of the stored operands; bA = the bound of an unseen A, carried through |B|.  Returns (reference C,
    its bound, reference H of epilogue 3, its bound)"""
    K = A.shape[1]
    pre, C, Hh = G.gemm_ref(A, Bw, bias, Rs, Hs, epi)
    bc, bh = G.gemm_bound(G.abs_prod(A, Bw), K, pre, C, Hh, Hs, epi, dt)
    if bA is not None:
        prop = (1 + G.OUT_EPS[dt]) * (bA.expand_as(A) @ Bw.double().abs().T)
        bc = bc + (G.GELU_D1_MAX if epi == 3 else 1.0) * prop
        if epi == 3:
            bh = bh + G.GELU_D2_MAX * prop
    if got is not None:
        V_.add(key[0], key[1], got, C, bc)
    return C, bc, Hh, bh


def _ln_fwd(V_, l, tag, xin, gamma, beta, st, eps, dt):
    """the statistics link of a LayerNorm and (reference y, its per-row bound)"""
    ry, rmean, rrstd, _ = VR.ln_ref(xin, gamma, beta, torch.zeros_like(xin), eps)
    V_.add(l, tag + " mean", st[0], rmean, larger(VR.measured(VR.LN_MEAN_REL) * rmean.abs(), VR.mean_floor(xin)))
    V_.add(l, tag + " rstd", st[1], rrstd, larger(VR.measured(VR.LN_RSTD_REL), VR.rstd_floor(xin.shape[1])) * rrstd)
    return ry, VR.LN[dt] * ry.abs().amax(1, keepdim=True) + VR.FLOOR * float(ry.abs().max())


def _ln_bwd(V_, key, got, g_before, dy, xin, gamma, beta, eps, dt):
    """g = (the stored g before this writer) + dLN/dx^T dy, the bound of tests/test_vit_ops_kernels_gpu.py's `g0 + dx`"""
    _, _, _, dx = VR.ln_ref(xin, gamma, beta, dy, eps)
    rg = g_before + dx
    V_.add(key[0], key[1], got, rg, (VR.LN[dt] * rg.abs().amax(1, keepdim=True) + VR.FLOOR * float(rg.abs().max())).expand_as(rg))


def judge(c, P, R, batched_gram=None):
    """every link of one step (see the module docstring) -> plan_ref.Verdict keyed (layer, tensor); layer -1 = the patch embedding, depth = the pooled LN.
    R: the dict of `emulate`.  batched_gram: whether the Gram pass took the one-launch form (default: depth > 1, the executor's rule for an evenly spaced h1)"""
    V_ = Verdict()
    dt = R["dt"] or "f32"
    B, N, M, n_prompt = R["B"], R["N"], R["M"], R["n_prompt"]
    D, Hh, depth, eps = c["dim"], c["heads"], c["depth"], BLOCK_EPS
    hd, Pp = D // Hh, max(n_prompt, 1)
    w, qf, v16 = wants(c, n_prompt), (AR.ident if R["dt"] is None else qf_of(dt)), (AR.V16 if dt == "bf16" else 0.0)
    s = ADAPTER_SCALE
    copyb = lambda ref: VR.COPY[dt] * float(ref.abs().max())
    # ---- the weight copies
    V_.add(-1, "w pe", R["pe_wf"], P["pe_w"].double(), copyb(P["pe_w"].double()))
    for l, L in enumerate(P["layers"]):
        eff, mass = eff_qkv(c, L, P)
        for n_, ref in (("qkv", eff), ("proj", L["proj_w"].double()), ("fc1", L["fc1_w"].double()), ("fc2", L["fc2_w"].double())):
            bound = torch.full_like(ref, copyb(ref))
            if n_ == "qkv" and mass is not None:              # clhip_sdlora_refresh's own rule on the q and v rows (tests/test_sdlora_kernels_gpu.py)
                sd_b = (sum(SD_RANKS) + 3 * len(SD_RANKS) + 2) * U * mass + 2 * v16 * ref.abs()
                sd_b[D:2 * D] = bound[D:2 * D]
                bound = sd_b
            V_.add(l, "wf " + n_, R["wf"][l][n_], ref, bound)
            V_.add(l, "wb " + n_, R["wb"][l][n_], ref.T, bound.T)
    # ---- the patch embedding and the token assembly
    ref = VR.patchify_ref(R["img"], c["patch"])
    V_.add(-1, "patches", R["patches"], ref, copyb(ref))
    _gemm(V_, (-1, "pe_out"), R["pe_out"], R["patches"], R["pe_wf"], P["pe_b"], None, None, 1, dt)
    ref = VR.assemble_ref(R["pe_out"], P["cls"], P["pos"], P["prompt"] if n_prompt else None, B, c["np"], n_prompt, D)
    V_.add(-1, "x0", R["x"][0], ref, copyb(ref))
    att = [None] * depth
    for l, L in enumerate(P["layers"]):
        wfl, x = R["wf"][l], R["x"]
        ry, ay = _ln_fwd(V_, l, "ln1", x[l], L["ln1_w"], L["ln1_b"], R["st1"][l], eps, dt)
        if R["h1"][l] is not None:
            V_.add(l, "h1", R["h1"][l], ry, ay.expand_as(ry))
            _gemm(V_, (l, "qkv"), R["qkv"][l], R["h1"][l], wfl["qkv"], L["qkv_b"], None, None, 1, dt)
        else:
            _gemm(V_, (l, "qkv"), R["qkv"][l], ry, wfl["qkv"], L["qkv_b"], None, None, 1, dt, bA=ay)
        Lp = c["Lp"][l]
        big, bd = attention(c, R["qkv"][l], R["pk"][l], R["pv"][l], R["tap"].get((l, "dproj")), B, N, Lp)
        bounds, cond, ref_lse = VR.attn_references(big, bd, B, N, Lp, Hh, hd, dt)
        att[l] = bounds
        ro, rel, extra = bounds["out"]
        V_.add(l, "attn_o", VR.heads(R["attn_o"][l], B, N, Hh, hd), ro, VR.blocked_allowed(ro, rel, extra))
        rl = ref_lse[:, :, Lp:]
        V_.add(l, "lse", R["lse"][l], rl, larger(torch.full_like(rl, VR.measured(VR.LSE_ABS)), VR.lse_floor(cond, N + Lp, rl)))
        _gemm(V_, (l, "x_mid"), R["x_mid"][l], R["attn_o"][l], wfl["proj"], L["proj_b"], x[l], None, 2, dt)
        ry2, ay2 = _ln_fwd(V_, l, "ln2", R["x_mid"][l], L["ln2_w"], L["ln2_b"], R["st2"][l], eps, dt)
        act, bact, href, bh = _gemm(V_, None, None, ry2, wfl["fc1"], L["fc1_b"], None, None, 3, dt, bA=ay2)        # (both scratch: the LN2 output, the GELU output)
        V_.add(l, "hpre", R["hpre"][l], href, bh)
        if not c["adapter_dim"]:
            _gemm(V_, (l, "x_out"), x[l + 1], act, wfl["fc2"], L["fc2_b"], R["x_mid"][l], None, 2, dt, bA=bact)
        else:
            y0, b0, _, _ = _gemm(V_, None, None, act, wfl["fc2"], L["fc2_b"], R["x_mid"][l], None, 2, dt, bA=bact)
            Wd, bd_, Wu, bu = [t.double() for t in L["adapter"]]
            delta, hd64 = AR.fwd(R["x_mid"][l], Wd, bd_, Wu, bu, s, R["mask"][l], c["p"], qf)
            e_hd, e_y = AR.fwd_bounds(R["x_mid"][l], y0, Wd, bd_, Wu, bu, s, hd64, delta, y0 + delta, c["p"], v16, qf)
            V_.add(l, "ad_hd", R["ad_hd"][l], hd64, e_hd)
            V_.add(l, "x_out", x[l + 1], y0 + delta, b0 * (1 + G.OUT_EPS[dt]) + e_y)        # two writers: fc2's stored rounding (in b0), then the adapter's
        if R["gram"] is not None:
            assert R["h1"][l] is not None
            ref = R["gram0"][l].double() + VR.gram_ref(R["h1"][l])
            one_launch = (depth > 1) if batched_gram is None else batched_gram
            V_.add(l, "gram", R["gram"][l], ref, (VR.GRAM_BATCHED if (one_launch and dt == "bf16") else VR.GRAM) * float(ref.abs().max()))
    rfeat, rg = VR.ln_pool_ref(R["x"][depth], P["norm_w"], P["norm_b"], R["dfeat"], B, N, D, Pp, 1e-6)
    V_.add(depth, "feat", R["feat"], rfeat, VR.LN_POOL_FEAT * rfeat.abs().amax(1, keepdim=True) + VR.FLOOR * float(rfeat.abs().max()))
    # ---- backward
    tap = R["tap"]
    expect = written_slots(c, n_prompt)
    for k in expect - set(tap):
        V_[(k[0], k[1] + " not written")] = float("inf")
    for k in set(tap) - expect:
        V_[(k[0], k[1] + " written")] = float("inf")
    if (-1, "g0") not in tap:
        return V_
    bg = (VR.LN[dt] * rg.abs().amax(2, keepdim=True) + VR.FLOOR * float(rg.abs().max())).expand_as(rg).clone()
    bg[:, Pp:] = 0.0                                                    # rows >= P are zeroed
    V_.add(depth, "g0", tap[(-1, "g0")].reshape(B, N, D), rg, bg)
    g = tap[(-1, "g0")]
    lowest = lowest_layer(c, n_prompt)
    for l in range(depth - 1, lowest - 1, -1):
        L, wbl = P["layers"][l], R["wb"][l]
        if (l, "dqkv") not in tap or any((l, k) not in tap for k in ("dbig", "dfc1", "g_ln2", "dproj")):
            break
        _gemm(V_, (l, "dbig"), tap[(l, "dbig")], g, wbl["fc2"], None, None, R["hpre"][l], 4, dt)
        if c["adapter_dim"]:
            Wd, _, Wu, _ = [t.double() for t in L["adapter"]]
            xm, hds, dhs = R["x_mid"][l], R["ad_hd"][l], tap[(l, "ad_dh")]
            dx64, _, _, _, _, dh64 = AR.bwd(g, xm, hds, Wd, Wu, s, c["p"], qf)
            e_dh, e_gx = AR.bwd_bounds(g, hds, Wd, Wu, s, dh64, dx64, g + dx64, c["p"], v16, qf)
            V_.add(l, "ad_dh", dhs, dh64, e_dh)
            V_.add(l, "ad_gx", tap[(l, "ad_gx")], g + dx64, e_gx)
            if w["adapter"]:                                             # on stored tensors only: fp32 accumulation over the M rows
                refs = (dhs.T @ xm, dhs.sum(0), s * g.T @ hds, s * g.sum(0))
                for nm, got, rf, bd_ in zip(("dWd", "dbd", "dWu", "dbu"), R["d_adapter"][l], refs, AR.wgrad_bounds(g, hds, xm, dhs, s)):
                    V_.add(l, "d_adapter " + nm, got, rf, bd_)
            g = tap[(l, "ad_gx")]
        _gemm(V_, (l, "dfc1"), tap[(l, "dfc1")], tap[(l, "dbig")], wbl["fc1"], None, None, None, 0, dt)
        _ln_bwd(V_, (l, "g_ln2"), tap[(l, "g_ln2")], g, tap[(l, "dfc1")], R["x_mid"][l], L["ln2_w"], L["ln2_b"], eps, dt)
        g = tap[(l, "g_ln2")]
        _gemm(V_, (l, "dproj"), tap[(l, "dproj")], g, wbl["proj"], None, None, None, 0, dt)
        Lp = c["Lp"][l]
        gq, gk, gv = VR.split_qkv(tap[(l, "dqkv")], B, N, Hh, hd)
        got = dict(dq=gq, dk=gk, dv=gv)
        if Lp and w["prefix"]:
            got.update(dpk=VR.heads(R["dpk"][l], B, Lp, Hh, hd), dpv=VR.heads(R["dpv"][l], B, Lp, Hh, hd))
        for nm, t in got.items():
            rf, rel, extra = att[l][nm]
            V_.add(l, nm, t, rf, VR.blocked_allowed(rf, rel, extra))
        if w["lora"]:
            rk, rv = VR.lora_db_ref(R["h1"][l], tap[(l, "dqkv")], L["lora_a_k"], L["lora_a_v"], D)
            rel = VR.LORA_GRAD_MFMA if (dt == "bf16" and D % 64 == 0) else VR.LORA_GRAD
            for i, r_ in enumerate((rk, rv)):
                tot = R["d_lora_b0"][l][i].double() + r_
                V_.add(l, "d_lora_b " + "kv"[i], R["d_lora_b"][l][i], tot, rel * float(r_.abs().max()) + U * tot.abs())
        if w["sd"]:
            want, bound = SR.grads_bounded(R["h1"][l], tap[(l, "dqkv")], L["sd"], P["sd_mag"], L["sd_inv"], (lambda t: q(t.double(), R["dt"])), v16)
            for nm, got_, rf, bd_ in zip(("dAq", "dBq", "dAv", "dBv", "dmag row"), list(R["d_sd"][l]) + [R["d_mag_rows"][l]], want, bound):
                V_.add(l, "d_sd " + nm, got_, rf, bd_)
        if w["ab"]:                                                      # clhip_lora_grad_ab's own reference and bound (tests/test_lorasub_kernels_gpu.py)
            host = [L[k] for k in ("lora_a_k", "lora_b_k", "lora_a_v", "lora_b_v")]
            want, bound = LR.grads_ab_bounded(R["h1"][l], tap[(l, "dqkv")], host, (lambda t: q(t.double(), R["dt"])), v16)
            for nm, got_, rf, bd_ in zip(("dAk", "dBk", "dAv", "dBv"), R["d_ab"][l], want, bound):
                V_.add(l, "d_ab " + nm, got_, rf, bd_)
        if l == lowest and not w["dprompt"]:
            break
        if (l, "dqin") not in tap or (l, "g_ln1") not in tap:             # (reported above as "not written")
            break
        _gemm(V_, (l, "dqin"), tap[(l, "dqin")], tap[(l, "dqkv")], wbl["qkv"], None, None, None, 0, dt)
        _ln_bwd(V_, (l, "g_ln1"), tap[(l, "g_ln1")], g, tap[(l, "dqin")], R["x"][l], L["ln1_w"], L["ln1_b"], eps, dt)
        g = tap[(l, "g_ln1")]
    if w["sd"] and (0, "dqkv") in tap:
        rf = R["d_mag_rows"].sum(0)
        V_.add(depth, "d_mag", R["d_mag"], rf, (depth + 1) * U * R["d_mag_rows"].abs().sum(0))
    if w["dprompt"] and (0, "g_ln1") in tap:
        rf = VR.prompt_grad_ref(g, B, N, n_prompt, D)
        V_.add(depth, "dprompt", R["dprompt"], rf, VR.PROMPT_GRAD * float(rf.abs().max()))
    return V_
