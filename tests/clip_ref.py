"""fp64 restatement of the CLIP path (csrc/clip.hip, epilogue 6 of clhip_gemm_nt, the executor's CLIP mode) and the per-element bounds of its tests.

QuickGELU (reference core/model/backbone/transformer.py:137-139): q(x) = x s, s = sigmoid(1.702 x);  q'(x) = s (1 + 1.702 x (1 - s));
q''(x) = 1.702 s (1 - s) (2 + 1.702 x (1 - 2 s)).  sup |q'| = 1.0998 (at 1.702 x = 2.3994), sup |q''| = 0.851 = q''(0): QGELU_D1_MAX / QGELU_D2_MAX
carry them rounded up, and tests/test_clip_cpu.py checks both on a fine fp64 grid.

Bound of one element of epilogue 6, from S = |A| . |B|^T (the terms of tests/gemm_ref.py, whose constants are imported, not repeated):
  accumulation   (K + 8) 2^-24 S reaches C through |q'| <= QGELU_D1_MAX and H through |q''| <= QGELU_D2_MAX
  output         2^-8 |ref| (bf16), 2^-23 |ref| (fp32)
  the sigmoid    C_Q max(1, |x|): the error of the hardware exp and reciprocal in s is not derivable; it is measured, as gemm_ref.C_G is:
                 C_Q = max(2^-20, 4 x the largest `[measure] c_q` of tests/test_gemm_quickgelu_gpu.py on an MI355X, rounded up to a power of two).
                 Both outputs are |x| times a quantity with a relative error of a few ulp, hence the max(1, |x|).
Epilogue 4 on the stored H is gemm_ref's own epilogue 4.

CLIP logits (clip.py:405-412), exact fp32 in the kernel: with u = feat . proj, n = u / |u|, logits = scale n . txt^T each fp32 sum of k terms is within
(k + 2) 2^-24 of its sum of absolute values (fixed order, fused multiply-adds; the 2 spare units carry the final roundings), so
  |u err|        <= EU = (D + 2) 2^-24 (|feat| . |proj|)
  |1/|u| err|    <= relative (E + 4) 2^-24 + |u| . EU / |u|^2           (sum of squares, sqrt, reciprocal: one rounding each)
  |n err|        <= EN = EU / |u| + |n| x that relative error
  |logits err|   <= scale (EN . |txt| + (E + 3) 2^-24 |n| . |txt|)
and for the backward, with g = scale dlogits . txt, du = (g - n (n . g)) / |u|, dfeat = proj . du, the same rule applied launch-internal step by step
(logits_bound / dfeat_bound below).  The bounds are first order with every constant rounded up; tests/test_clip_cpu.py holds an fp32 torch evaluation of the same
formulas to them and checks they are not vacuous (a 1e-3 relative perturbation of one input exceeds them).
"""
import math

import numpy as np
import torch

import gemm_ref as G

QGELU_D1_MAX = 1.10
QGELU_D2_MAX = 0.86
C_Q_FLOOR = 2.0 ** -20
C_Q_MEASURED = 0.0          # largest [measure] c_q of tests/test_gemm_quickgelu_gpu.py on an MI355X: never positive on any case (0 at x = 0 of the controlled f32 130x72x64 case; < 0 elsewhere: the error stays inside the other terms), so the floor decides
QGELU_EPI = 6               # include/clhip.h: 5 is not an epilogue (tests/test_gemm_kernels_gpu.py pins its refusal)


def c_q():
    if C_Q_MEASURED is None or C_Q_MEASURED <= 0:
        return C_Q_FLOOR
    return max(C_Q_FLOOR, 2.0 ** math.ceil(math.log2(4.0 * C_Q_MEASURED)))


def qgelu_both(x):
    """fp64 q(x) and q'(x); s and 1 - s from exp(-|t|), so neither tail cancels"""
    x = x.double()
    t = 1.702 * x
    e = torch.exp(-t.abs())
    r = 1.0 / (1.0 + e)
    s = torch.where(t >= 0, r, e * r)
    c = torch.where(t >= 0, e * r, r)
    return x * s, s * (1.0 + t * c)


def qgelu_d2(x):
    x = x.double()
    t = 1.702 * x
    s = torch.sigmoid(t)
    return 1.702 * s * (1 - s) * (2 + t * (1 - 2 * s))


def qgelu_ref(A, B, bias, prod=None):
    """(pre-activation, C, H) of epilogue 6 in fp64"""
    x = (A.double() @ B.double().T if prod is None else prod.clone()) + bias.double()
    c, h = qgelu_both(x)
    return x, c, h


def qgelu_other_terms(S, K, Cref, Href, dt):
    acc = (K + 8) * G.U24 * S
    eps = G.OUT_EPS[dt]
    return QGELU_D1_MAX * acc + eps * Cref.abs(), QGELU_D2_MAX * acc + eps * Href.abs()


def qgelu_bound(S, K, pre, Cref, Href, dt):
    bc, bh = qgelu_other_terms(S, K, Cref, Href, dt)
    g = c_q() * pre.abs().clamp(min=1.0)
    return bc + g, bh + g


# ------------------------------------------------------------------------------------------------ CLIP logits
U24 = 2.0 ** -24


def logits_ref(feat, proj, txt, scale):
    """fp64: (logits, u, 1 / |u|)"""
    u = feat.double() @ proj.double()
    inv = 1.0 / u.norm(dim=1)
    n = u * inv[:, None]
    return scale * (n @ txt.double().T), u, inv


def dfeat_ref(dlogits, proj, txt, scale, u, inv):
    """fp64 input gradient through the product with txt, the normalisation and proj"""
    g = scale * (dlogits.double() @ txt.double())
    n = u.double() * inv.double()[:, None]
    du = (g - n * (n * g).sum(1, keepdim=True)) * inv.double()[:, None]
    return du @ proj.double().T


def _n_err(feat, proj):
    """(|u|, |n|, EU, relative error of 1 / |u|, EN) in fp64"""
    D, E = proj.shape
    u = feat.double() @ proj.double()
    nu = u.norm(dim=1, keepdim=True)
    EU = (D + 2) * U24 * (feat.double().abs() @ proj.double().abs())
    rel = (E + 4) * U24 + (u.abs() * EU).sum(1, keepdim=True) / nu ** 2
    n = (u / nu).abs()
    EN = EU / nu + n * rel + 2 * U24 * n
    return nu, n, EU, rel, EN


def logits_bound(feat, proj, txt, scale):
    E = proj.shape[1]
    _, n, _, _, EN = _n_err(feat, proj)
    ta = txt.double().abs()
    return abs(scale) * (EN @ ta.T + (E + 3) * U24 * (n @ ta.T))


def saved_bound(feat, proj):
    """(bound of the saved u, bound of the saved 1 / |u|)"""
    nu, _, EU, rel, _ = _n_err(feat, proj)
    return EU, (rel / nu)[:, 0]


def dfeat_bound(dlogits, feat, proj, txt, scale):
    """bound of dfeat for the kernel pair: the backward reads the fp32 u and 1 / |u| the forward saved (their errors are EU and rel)"""
    D, E = proj.shape
    C = txt.shape[0]
    nu, n, EU, rel, EN = _n_err(feat, proj)
    g_abs = abs(scale) * (dlogits.double().abs() @ txt.double().abs())
    g = scale * (dlogits.double() @ txt.double())
    Eg = (C + 3) * U24 * g_abs
    ng_abs = (n * g.abs()).sum(1, keepdim=True)
    Eng = (EN * g.abs()).sum(1, keepdim=True) + (n * Eg).sum(1, keepdim=True) + (E + 3) * U24 * ng_abs
    inner = g.abs() + n * ng_abs                                     # magnitude of g - n (n . g) before the cancellation
    Einner = Eg + EN * ng_abs + n * Eng + 3 * U24 * inner
    du_abs = inner / nu
    Edu = Einner / nu + inner / nu * (rel + 2 * U24)
    pa = proj.double().abs()
    return Edu @ pa.T + (E + 3) * U24 * (du_abs @ pa.T)


# ------------------------------------------------------------------------------------------------ the CLIP path restated (fixture tests/golden/clip_tiny.npz)
# The visual tower in the executor's batch-first form, launch by launch; the text tower; InfLoRA_OPT's task loop on them (Gram -> SVD -> lora_A, Adam on the
# visual lora_B, merge, DualGPM).  tools/gen_clip_golden.py runs the REFERENCE's classes in fp64 and writes the fixture; run_fixture below is this project's
# own statement of the same arithmetic and is held to it at 1e-10 (tests/test_clip_cpu.py).
CFG = dict(img=32, patch=8, width=64, depth=3, embed=32, ctx=77, twidth=64, theads=1, tlayers=2)
RANK, INC, TASKS, STEPS, BATCH, NI = 4, 3, 2, 3, 9, 12
LR, BETAS, ADAM_EPS, LAME, LAMB = 0.0005, (0.9, 0.999), 1e-8, 1.0, 0.95
TEMPLATE = "a bad photo of a {}."
F32_TOL = 5e-3                  # the project's standing method-level criterion: max |got - want| <= 5e-3 max |want|
CUT_MARGIN = 1e-4               # condition (a): every DualGPM rank cut is this far (in spectrum fraction) from its threshold
# bf16 method-level deviations of the committed fixture (tests/golden/clip_tiny.npz, seed 211) from its fp64 values, measured on an MI355X by
# tests/test_clip_gpu.py (its `[measure]` line prints exactly these); a gate is 4 x its figure, never more.
#   lora_B      : the largest element deviation over max-abs.  Under Adam the first steps move every element by about lr * sign(g); an element whose gradient
#                 is below the bf16 noise takes the other sign, so this figure sits at its largest possible value, 2, and its gate excludes only non-finite
#                 values.  It is kept as the issue lists it; lora_B_rms is the check that can fail.
#   lora_B_rms  : |B - B_ref| / |B_ref| over all layers' k and v factors of one step as one vector.  An untrained B gives exactly 1, a B of the wrong sign 2,
#                 random signs about 1.41: the gate, 0.644, excludes all three.
#   logits, lora_A: condition (b) of the fixture (every top-two gap is wider than the bf16 logits gate) was searched against a logits gate of 0.0716 and no seed
#                 of 200 tried separates every pair by 4 x 0.0397 = 0.159, so BF16_GATE_CAP keeps these two gates below 4 x the figure ON PURPOSE: 1.8 x
#                 (logits) and 2 x (lora_A) the committed fixture's own deviation.  That is tighter than the rule asks, never wider.
BF16_MEASURED = dict(losses=0.00798, logits=0.0397, lora_B=2.0, lora_B_rms=0.161, lora_A=0.0164, bases=0.00797)
BF16_GATE_CAP = dict(logits=0.0716, lora_A=0.03308)


def bf16_gate(key):
    return min(4.0 * BF16_MEASURED[key], BF16_GATE_CAP.get(key, float("inf")))


def fixture_weights(fix, dtype=torch.float64):
    return {k[2:]: torch.from_numpy(fix[k]).view(torch.bfloat16).to(dtype) for k in fix.keys() if k.startswith("w/")}


def images(a, dtype=torch.float64):
    return torch.from_numpy(np.asarray(a)).to(dtype) / 255.0


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def qgelu(x):
    """torch-differentiable QuickGELU with the same two-sided sigmoid as qgelu_both"""
    return x * torch.sigmoid(1.702 * x)


def visual_forward(w, x, lora=None, keep=False, pre="visual."):
    """ln_post output at the class token [B, width] (and, with keep, what the executor saves per layer: x_in, h1, qkv, attn_o, x_mid, the QuickGELU derivative).
    lora: per layer (A_k, B_k, A_v, B_v) or None; the effective qkv weight is W + [0; B_k A_k; B_v A_v] (transformer.py:248-254)."""
    W = w[pre + "conv1.weight"]
    D, p = W.shape[0], W.shape[-1]
    B = x.shape[0]
    g = x.shape[-1] // p
    patches = x.reshape(B, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, 3 * p * p)      # the patch convolution as a product (no bias, :2107)
    tok = patches @ W.reshape(D, -1).T
    tok = torch.cat([w[pre + "class_embedding"].expand(B, 1, D), tok], dim=1) + w[pre + "positional_embedding"]
    h = _ln(tok, w[pre + "ln_pre.weight"], w[pre + "ln_pre.bias"])
    depth = len({k.split(".")[3] for k in w if k.startswith(pre + "transformer.blocks.")})
    heads = max(D // 64, 1)
    N, hd = h.shape[1], D // max(D // 64, 1)
    saved = []
    for l in range(depth):
        b = f"{pre}transformer.blocks.{l}."
        h1 = _ln(h, w[b + "ln_1.weight"], w[b + "ln_1.bias"])
        Wq = w[b + "attn.qkv.weight"]
        if lora is not None:
            Ak, Bk, Av, Bv = lora[l]
            Wq = torch.cat([Wq[:D], Wq[D:2 * D] + Bk @ Ak, Wq[2 * D:] + Bv @ Av], dim=0)
        qkv = h1 @ Wq.T + w[b + "attn.qkv.bias"]
        q, k, v = qkv.view(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
        att = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)
        ao = (att @ v).transpose(1, 2).reshape(B, N, D)
        xm = h + ao @ w[b + "attn.proj.weight"].T + w[b + "attn.proj.bias"]
        z = _ln(xm, w[b + "ln_2.weight"], w[b + "ln_2.bias"]) @ w[b + "mlp.fc1.weight"].T + w[b + "mlp.fc1.bias"]
        if keep:
            saved.append(dict(x_in=h, h1=h1, qkv=qkv, attn_o=ao, x_mid=xm, hpre=qgelu_both(z)[1].to(z.dtype), pre=z))
        h = xm + qgelu(z) @ w[b + "mlp.fc2.weight"].T + w[b + "mlp.fc2.bias"]
    feat = _ln(h[:, 0], w[pre + "ln_post.weight"], w[pre + "ln_post.bias"])
    return (feat, saved, h) if keep else feat


def text_features(w, emb, tokens):
    """normalised text features [C, embed]: embedding rows `emb` (the fixture keeps only the used ones), causal blocks, ln_final, the row of the largest token
    id through text_projection (clip.py:385-398, :409)"""
    x = emb[tokens] + w["positional_embedding"]
    B, L, W = x.shape
    heads = max(W // 64, 1)
    mask = torch.full((L, L), float("-inf"), dtype=x.dtype).triu_(1)
    depth = len({k.split(".")[2] for k in w if k.startswith("transformer.blocks.")})
    for l in range(depth):
        b = f"transformer.blocks.{l}."
        qkv = _ln(x, w[b + "ln_1.weight"], w[b + "ln_1.bias"]) @ w[b + "attn.qkv.weight"].T + w[b + "attn.qkv.bias"]
        q, k, v = qkv.view(B, L, 3, heads, W // heads).permute(2, 0, 3, 1, 4)
        att = ((q @ k.transpose(-2, -1)) * (W // heads) ** -0.5 + mask).softmax(dim=-1)
        x = x + (att @ v).transpose(1, 2).reshape(B, L, W) @ w[b + "attn.proj.weight"].T + w[b + "attn.proj.bias"]
        z = _ln(x, w[b + "ln_2.weight"], w[b + "ln_2.bias"]) @ w[b + "mlp.fc1.weight"].T + w[b + "mlp.fc1.bias"]
        x = x + qgelu(z) @ w[b + "mlp.fc2.weight"].T + w[b + "mlp.fc2.bias"]
    x = _ln(x, w["ln_final.weight"], w["ln_final.bias"])
    t = x[torch.arange(B), tokens.argmax(dim=-1)] @ w["text_projection"]
    return t / t.norm(dim=-1, keepdim=True)


def logits_torch(feat, proj, txt, scale):
    u = feat @ proj
    return scale * (u / u.norm(dim=-1, keepdim=True)) @ txt.T


def cross_entropy(logits, y):
    return (torch.logsumexp(logits, dim=1) - logits[torch.arange(len(y)), y]).mean()


def grams(w, xs):
    """mean over all tokens of all batches of X^T X, X = every layer's attention input (transformer.py:241-244)"""
    tot, n = None, 0
    for x in xs:
        _, saved, _ = visual_forward(w, x, keep=True)
        g = torch.stack([s["h1"].reshape(-1, s["h1"].shape[-1]).T @ s["h1"].reshape(-1, s["h1"].shape[-1]) for s in saved])
        tot, n = (g if tot is None else tot + g), n + x.shape[0] * saved[0]["h1"].shape[1]
    return tot / n


def _svd(a):
    U, S, Vt = np.linalg.svd(np.asarray(a, dtype=np.float64), full_matrices=False)
    return U, S, Vt


def dualgpm_update(act, feature, ptype, task, task_num=TASKS, margins=None):
    """one layer of InfLoRA_opt.py:290-369 (before the remove -> retain switch): the new basis; `margins` collects |cumulative ratio - threshold| at each cut"""
    thr = (LAME - LAMB) * task / task_num + LAMB
    act = np.asarray(act, dtype=np.float64)

    def note(vals):
        if margins is not None:
            margins.append(float(np.abs(np.asarray(vals) - thr).min()))
    if task == 0:
        U, S, _ = _svd(act)
        cum = np.cumsum(S ** 2 / (S ** 2).sum())
        note(cum)
        r = max(int(np.sum(cum < thr)), 1)
        assert r < act.shape[0] / 2
        return U[:, :r]
    _, S, _ = _svd(act)
    total = (S ** 2).sum()
    fm = feature @ feature.T
    if ptype == "remove":
        U, S, _ = _svd(act - fm @ act)
        acc = (total - (S ** 2).sum()) / total
        note([acc])
        if acc < thr:
            cum = np.cumsum(S ** 2 / total) + acc
            note(cum)
            r = int(np.sum(cum < thr)) + 1
            Ui = np.hstack((feature, U[:, :r]))
            return Ui[:, : min(Ui.shape)]
        return feature
    U, S, _ = _svd(fm @ act)
    acc = (S ** 2).sum() / total
    note([1 - acc])
    if acc >= 1 - thr:
        rest = acc - np.cumsum(S ** 2 / total)
        note(1 - rest)
        r = int(np.sum(rest >= 1 - thr)) + 1
        af = feature - U[:, :r] @ U[:, :r].T @ feature
        U2 = np.linalg.svd(af, full_matrices=True)[0]
        return U2[:, : feature.shape[1] - r]
    return feature


def run_fixture(fix, dtype=torch.float64):
    """the fixture's two tasks restated -> dict with the fixture's per-step / per-task keys, and "margins" (condition (a))"""
    w = fixture_weights(fix, dtype)
    emb = w.pop("token_embedding.weight")
    D, depth = CFG["width"], CFG["depth"]
    scale = float(w["logit_scale"].double().exp())
    x, y, xi = images(fix["x_u8"], dtype), torch.from_numpy(fix["y"]), images(fix["xi_u8"], dtype)
    out, feats, ptypes, margins = {}, [], [], []
    for t in range(TASKS):
        curr = text_features(w, emb, torch.from_numpy(fix[f"t{t}/curr_tokens"]))
        accm = text_features(w, emb, torch.from_numpy(fix[f"t{t}/accm_tokens"]))
        out[f"t{t}/curr_txt"], out[f"t{t}/accm_txt"] = curr, accm
        G = grams(w, [x[t, s] for s in range(STEPS)])
        A = []
        for l in range(depth):
            g = G[l].double().numpy()
            if t > 0:
                fm = feats[l] @ feats[l].T
                g = g - fm @ g if ptypes[l] == "remove" else fm @ g
            A.append(torch.from_numpy(_svd(g)[0][:, :RANK].T / math.sqrt(3)).to(dtype))
        out[f"t{t}/lora_A"] = torch.stack(A)
        Bs = [torch.zeros(D, RANK, dtype=dtype, requires_grad=True) for _ in range(2 * depth)]
        m = [torch.zeros_like(b) for b in Bs]
        v = [torch.zeros_like(b) for b in Bs]
        for s in range(STEPS):
            lora = [(A[l], Bs[2 * l], A[l], Bs[2 * l + 1]) for l in range(depth)]
            logits = logits_torch(visual_forward(w, x[t, s], lora), w["visual.proj"], curr, scale)
            loss = cross_entropy(logits, y[t, s] - INC * t)
            gr = torch.autograd.grad(loss, Bs)
            with torch.no_grad():
                for i, b in enumerate(Bs):                    # torch.optim.Adam, weight_decay 0
                    m[i] = BETAS[0] * m[i] + (1 - BETAS[0]) * gr[i]
                    v[i] = BETAS[1] * v[i] + (1 - BETAS[1]) * gr[i] ** 2
                    b -= LR / (1 - BETAS[0] ** (s + 1)) * m[i] / (v[i].sqrt() / math.sqrt(1 - BETAS[1] ** (s + 1)) + ADAM_EPS)
            out[f"t{t}/s{s}/loss"], out[f"t{t}/s{s}/logits"] = loss.detach(), logits.detach()
            out[f"t{t}/s{s}/lora_B"] = torch.stack([b.detach().clone() for b in Bs]).view(depth, 2, D, RANK)
        for l in range(depth):                                # merge_weight (transformer.py:228-234)
            k = f"visual.transformer.blocks.{l}.attn.qkv.weight"
            Wq = w[k]
            w[k] = torch.cat([Wq[:D], Wq[D:2 * D] + Bs[2 * l].detach() @ A[l], Wq[2 * D:] + Bs[2 * l + 1].detach() @ A[l]], dim=0)
        G = grams(w, [x[t, s] for s in range(STEPS)])
        for l in range(depth):
            f = dualgpm_update(G[l].double().numpy(), feats[l] if t else None, ptypes[l] if t else None, t, margins=margins)
            if t == 0:
                feats.append(f); ptypes.append("remove")
            else:
                feats[l] = f
        for l in range(depth):                                # InfLoRA_opt.py:358-369
            f = feats[l]
            if ptypes[l] == "remove" and f.shape[1] > f.shape[0] / 2:
                feats[l] = np.linalg.svd(f, full_matrices=True)[0][:, f.shape[1]:]
                ptypes[l] = "retain"
        for l in range(depth):
            out[f"t{t}/basis{l}"] = feats[l].copy()
        out[f"t{t}/ptype"] = np.array(ptypes)
        out[f"t{t}/infer_logits"] = logits_torch(visual_forward(w, xi), w["visual.proj"], accm, scale).detach()
        out[f"t{t}/infer_pred"] = out[f"t{t}/infer_logits"].argmax(1)
    out["margins"] = margins
    return out


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def align_rows(A, ref):
    """A with every row's sign chosen to match ref (singular vectors are defined up to sign); returns (aligned, signs [..., r])"""
    A, ref = np.asarray(A, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    sg = np.sign((A * ref).sum(-1, keepdims=True))
    sg[sg == 0] = 1.0
    return A * sg, sg[..., 0]


def projector_dev(f, ref):
    """bases are compared as projectors F F^T (sign and rotation free), relative to max-abs"""
    f, ref = np.asarray(f, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if f.shape != ref.shape:
        return float("inf")
    return rel(f @ f.T, ref @ ref.T)


def deviations(got, fix):
    """max relative-to-max-abs deviation per family; lora_B is compared after aligning the sign of each lora_A row (B A is what the network sees)"""
    d = dict(losses=0.0, logits=0.0, lora_B=0.0, lora_B_rms=0.0, lora_A=0.0, bases=0.0, txt=0.0, preds_equal=True)
    for t in range(TASKS):
        A, sg = align_rows(got[f"t{t}/lora_A"], fix[f"t{t}/lora_A"])
        d["lora_A"] = max(d["lora_A"], rel(A, fix[f"t{t}/lora_A"]))
        for k in ("curr_txt", "accm_txt"):
            d["txt"] = max(d["txt"], rel(got[f"t{t}/{k}"], fix[f"t{t}/{k}"]))
        for s in range(STEPS):
            d["losses"] = max(d["losses"], abs(float(got[f"t{t}/s{s}/loss"]) - float(fix[f"t{t}/s{s}/loss"])) / abs(float(fix[f"t{t}/s{s}/loss"])))
            d["logits"] = max(d["logits"], rel(got[f"t{t}/s{s}/logits"], fix[f"t{t}/s{s}/logits"]))
            Bg = np.asarray(got[f"t{t}/s{s}/lora_B"], dtype=np.float64) * sg[:, None, None, :]
            d["lora_B"] = max(d["lora_B"], rel(Bg, fix[f"t{t}/s{s}/lora_B"]))
            Bf = np.asarray(fix[f"t{t}/s{s}/lora_B"], dtype=np.float64)
            d["lora_B_rms"] = max(d["lora_B_rms"], float(np.linalg.norm(Bg - Bf) / np.linalg.norm(Bf)))      # all layers, k and v, of one step as one vector
        for l in range(CFG["depth"]):
            d["bases"] = max(d["bases"], projector_dev(got[f"t{t}/basis{l}"], fix[f"t{t}/basis{l}"]))
        d["logits"] = max(d["logits"], rel(got[f"t{t}/infer_logits"], fix[f"t{t}/infer_logits"]))
        d["preds_equal"] = d["preds_equal"] and bool(np.array_equal(np.asarray(got[f"t{t}/infer_pred"]), fix[f"t{t}/infer_pred"]))
        d["preds_equal"] = d["preds_equal"] and list(np.asarray(got[f"t{t}/ptype"])) == list(fix[f"t{t}/ptype"])
    return d


def top2_gap(logits):
    s = np.sort(np.asarray(logits, dtype=np.float64), axis=1)
    return (s[:, -1] - s[:, -2]) if s.shape[1] > 1 else np.full(s.shape[0], np.inf)


def condition_a(margins):
    return "" if min(margins) >= CUT_MARGIN else f"(a) a DualGPM cut is {min(margins):.3g} from its threshold"


def condition_b(fix, factor=1.0):
    """in every stored logits row the top two entries differ by more than `factor` x the bf16 gate of the GPU test (a fraction of the tensor's max-abs)"""
    worst = np.inf
    for t in range(TASKS):
        rows = [fix[f"t{t}/s{s}/logits"] for s in range(STEPS)] + [fix[f"t{t}/infer_logits"]]
        for r in rows:
            worst = min(worst, float((top2_gap(r) / (factor * bf16_gate("logits") * np.abs(r).max())).min()))
    return "" if worst > 1.0 else f"(b) a top-two gap is {worst:.3g} of {factor} x the bf16 logits gate"


def check_f32(got, fix):
    d = deviations(got, fix)
    bad = {k: v for k, v in d.items() if k != "preds_equal" and v >= F32_TOL}
    return "" if not bad and d["preds_equal"] else f"f32: {bad} preds_equal {d['preds_equal']}"
