"""Plain-torch restatement of the three LoRA-Sub-DRS kernels of csrc/lorasub.hip (core/model/lora_sub.py of the reference), in the precision of its inputs
(the tests call it in fp64), with the fp32 error bounds the GPU tests hold the kernels to; at the end the method on the toy ViT: its weight forms, one training
step, and the three tasks of tests/golden/lorasub_tiny.npz (fp64 runs of the reference's own classes, tools/gen_lorasub_golden.py), which
tests/test_lorasub_cpu.py holds this file to at 1e-10 and tests/test_lorasub_gpu.py holds the HIP path to.

Bounds, by the rule of tests/test_sdlora_kernels_gpu.py (u = 2^-24; v = 2^-8 in the bf16 mode): a sum of K products in fp32 is within K u sum|a b| of fp64
whatever the order; an operand that carries an error e adds e |b| summed; every further fp32 operation on a value c adds u |c|; a value stored as bf16 adds
2 v |c|.  Nothing here is measured on the kernels: each function states the operations it counts.
"""
import math

import torch

U = 2.0 ** -24
SEP = 1e-3                    # condition (b): the separation of every selection and of every hinge argument from 0


# ------------------------------------------------------------------------------------------------------------- augmented triplet loss
def _normalise(x):
    return x / x.norm(dim=1, keepdim=True)


def atl_select(f, y, protos):
    """the selections of AugmentedTripletLoss.forward (lora_sub.py:45-63) with the distances formed from the differences n_i - n_j.
    -> dict: d [B, B] and e [B, P] (clamped), jp [B], jn [B] (a batch row, B + p for prototype p, or -1), ap, an (None where jn = -1 is kept as ap + margin by the caller)"""
    B = f.shape[0]
    n = _normalise(f)
    a = ((n[:, None, :] - n[None, :, :]) ** 2).sum(-1)
    d = a.clamp(min=1e-12).sqrt()
    P = 0 if protos is None else protos.shape[0]
    e = eraw = None
    if P:
        c = _normalise(protos)
        eraw = (n[:, None, :] - c[None, :, :]).norm(dim=-1)
        e = eraw.clamp(min=1e-12)
    same = y[:, None] == y[None, :]
    jp, jn, dv = [], [], d.detach().tolist()
    for i in range(B):
        pos = torch.nonzero(same[i]).flatten().tolist()
        neg = torch.nonzero(~same[i]).flatten().tolist()
        bj = pos[0]
        for j in pos:                                          # ties to the lower index
            if dv[i][j] > dv[i][bj]:
                bj = j
        jp.append(bj)
        bn = -1
        for j in neg:
            if bn < 0 or dv[i][j] < dv[i][bn]:
                bn = j
        jn.append(bn)
    return dict(n=n, a=a, d=d, e=e, eraw=eraw, jp=jp, jn=jn, P=P)


def atl(f, y, protos, margin, weight=1.0):
    """-> (loss (unweighted mean hinge), df = weight * d loss / d f, info).  f may require grad or not; df comes from autograd through the restatement.
    info: per row jp, jn (after the prototype chain), ap, an, hinge argument h, and `gaps`: the smallest best / second-best separation of every max and min
    (exact ties of bitwise equal candidates excluded: every precision resolves them to the lower index) and the smallest |h|."""
    f = f.detach().clone().requires_grad_(True)
    s = atl_select(f, y, protos)
    B, P, d, e = f.shape[0], s["P"], s["d"], s["e"]
    same = (y[:, None] == y[None, :]).tolist()
    hs, jps, jns, aps, ans = [], [], [], [], []
    gap = math.inf
    dv, ev = d.detach().tolist(), e.detach().tolist() if P else None
    for i in range(B):
        jp, jn = s["jp"][i], s["jn"][i]
        ap = d[i, jp]
        an = d[i, jn] if jn >= 0 else ap + margin            # lora_sub.py:53-56
        # candidates of the minimum, in the order the reference visits them: batch negatives (or the one stand-in), then prototypes ascending
        negd = [dv[i][j] for j in range(B) if not same[i][j]] or [float(ap.detach() + margin)]
        for p in range(P):
            if ev[i][p] < float(an.detach()):                 # strict: ties stay with the earlier candidate (:60-63)
                an, jn = e[i, p], B + p
            negd.append(ev[i][p])
        posd = sorted((dv[i][j] for j in range(B) if same[i][j]), reverse=True)
        negd = sorted(negd)
        for vals in (posd, negd):
            if len(vals) > 1 and vals[0] != vals[1]:
                gap = min(gap, abs(vals[0] - vals[1]))
        h = (ap - an) + margin
        nothing = jn < 0                                       # no negative of any kind: contributes nothing (ap - (ap + m) + m)
        if not nothing:
            gap = min(gap, abs(float(h.detach())))
        hs.append(torch.zeros((), dtype=f.dtype) if nothing else torch.relu(h))
        jps.append(jp); jns.append(jn); aps.append(float(ap.detach())); ans.append(float(an.detach()))
    loss = torch.stack(hs).mean()
    (df,) = torch.autograd.grad(loss, f) if loss.requires_grad else (torch.zeros_like(f),)
    info = dict(jp=jps, jn=jns, ap=aps, an=ans, h=[float(x.detach()) for x in hs], gap=gap, n=s["n"].detach(), d=d.detach(), e=None if e is None else e.detach(),
                a=s["a"].detach(), eraw=None if e is None else s["eraw"].detach())
    return loss.detach(), weight * df, info


def atl_bounded(f32, y, protos32, margin, weight):
    """fp64 loss and df of fp32 inputs with the fp32 bounds of clhip_atl.  Operation counts (K = D):
    inverse norm: K products, a square root and a division: eps_inv = (K + 2) u;  n = f * inv: eps_n = eps_inv + u, relative.
    t = n_i - n_j carries eps_n (|n_i| + |n_j|) + u |t|;  a = sum t^2 (K terms): by Cauchy-Schwarz with |n| = 1,
        da <= 4 eps_n d + (K + 3) u d^2 + (2 eps_n + u d)^2;   d = sqrt(a): dd <= da / d + u d   (an unclamped d; a clamped one is exact)
    hinge h = (ap - an) + m: dh <= dd_ap + dd_an + u |ap - an| + u |h|;  loss: mean of B terms, (B + 1) u sum|h| / B.
    gradient term c (n_a - n_b) with c = 1 / d: relative dd / d + 3 u on |t| / d, plus eps_n (|n_a| + |n_b|) / d; a row gathers K_j terms: (K_j + 1) u sum|term|.
    dot = n . g (K products on operands with errors), y = g - n dot (2 operations), out = (weight / B) * (y * inv) (4 operations and eps_inv)."""
    f, pr = f32.double(), None if protos32 is None else protos32.double()
    m, wgt = float(torch.tensor(margin, dtype=torch.float32)), float(torch.tensor(weight, dtype=torch.float32))
    loss, df, info = atl(f, y, pr, m, wgt)
    B, K = f.shape
    eps_inv = (K + 2) * U
    eps_n = eps_inv + U
    n, d, e = info["n"], info["d"], info["e"]
    c = None if pr is None else _normalise(pr)

    def derr(dist):
        da = 4 * eps_n * dist + (K + 3) * U * dist ** 2 + (2 * eps_n + U * dist) ** 2
        return da / dist + U * dist

    e_loss, sum_h = 0.0, 0.0
    terms = [[] for _ in range(B)]                              # per row: (value [D], error [D]) of every gradient term it gathers
    for i in range(B):
        jp, jn, h = info["jp"][i], info["jn"][i], info["h"][i]
        if jn < 0 or h <= 0.0:
            continue
        ap, an = info["ap"][i], info["an"][i]
        clamped = (bool(info["a"][i, jp] < 1e-12), bool(info["a"][i, jn] < 1e-12) if jn < B else bool(info["eraw"][i, jn - B] < 1e-12))
        e_ap = 0.0 if clamped[0] else derr(ap)                # a clamped distance is the constant itself
        e_an = 0.0 if clamped[1] else derr(an)
        e_loss += e_ap + e_an + U * abs(ap - an) + U * abs(h)
        sum_h += abs(h)
        for sign, dist, ed, other, j in ((1.0, ap, e_ap, n[jp], jp), (-1.0, an, e_an, n[jn] if jn < B else c[jn - B], jn)):
            if clamped[0 if sign > 0 else 1]:
                continue                                        # a clamped pair (the self pair, a twin): no gradient
            t = n[i] - other
            val = sign * t / dist
            err = (t.abs() * (ed / dist + 3 * U) + eps_n * (n[i].abs() + other.abs())) / dist
            terms[i].append((val, err))
            if j < B:
                terms[j].append((-val, err))
    e_loss = e_loss / B + (B + 1) * U * sum_h / B
    e_df = torch.zeros_like(f)
    for j in range(B):
        if not terms[j]:
            continue
        g = sum(t[0] for t in terms[j])
        mass = sum(t[0].abs() for t in terms[j])
        eg = sum(t[1] for t in terms[j]) + (len(terms[j]) + 1) * U * mass
        nj = n[j]
        dot = (nj * g).sum()
        edot = (nj.abs() * eg).sum() + eps_n * (nj.abs() * g.abs()).sum() + (K + 1) * U * (nj * g).abs().sum()
        yv = g - nj * dot
        ey = eg + nj.abs() * edot + (eps_n + U) * (nj * dot).abs() + U * yv.abs()
        e_df[j] = abs(wgt) / B / f[j].norm() * (ey + yv.abs() * (eps_inv + 4 * U))
    return loss, df, float(e_loss), e_df, info


# ------------------------------------------------------------------------------------------------------- gradients of the four factors
def grads_ab(X, dqkv, Ak, Bk, Av, Bv):
    """d_a_k, d_b_k, d_a_v, d_b_v of one layer: the k / v rows of the qkv weight are W + B A (transformer.py:401-424)"""
    D = X.shape[1]
    out = []
    for A, B, dY in ((Ak, Bk, dqkv[:, D:2 * D]), (Av, Bv, dqkv[:, 2 * D:])):
        out += [(dY @ B).T @ X, dY.T @ (X @ A.T)]
    return tuple(out)


def grads_ab_bounded(X64, dY64, host, q, v):
    """clhip_lora_grad_ab's four results with their bounds: sdlora_ref.grads_bounded for one term of magnitude 1 on the k and v columns.  host = (A_k, B_k,
    A_v, B_v) fp32; q rounds a factor to the compute dtype where the MFMA products read it; v = 2^-8 in the bf16 mode (P = X A^T and U = dY B are stored in
    the compute dtype between the K = D and the K = M products), else 0."""
    M, D = X64.shape
    want, bound = [], []
    for w, dYw in ((0, dY64[:, D:2 * D]), (1, dY64[:, 2 * D:])):
        A16, B16 = q(host[2 * w]).double(), q(host[2 * w + 1]).double()
        P = X64 @ A16.T
        eP = D * U * (X64.abs() @ A16.abs().T) + 2 * v * P.abs()
        S = dYw.T @ P
        eS = dYw.abs().T @ eP + (M + 2) * U * (dYw.abs().T @ P.abs())
        Uw = dYw @ B16
        eU = D * U * (dYw.abs() @ B16.abs()) + 2 * v * Uw.abs()
        want += [Uw.T @ X64, S]
        bound += [eU.T @ X64.abs() + (M + 2) * U * (Uw.abs().T @ X64.abs()), eS]
    return want, bound


# ------------------------------------------------------------------------------------------------------------------- projected Adam
def proj_adam(p, g, m, v, T, lr, b1, b2, eps, wd, step, ref_form=False):
    """one step of lora_sub.py:120-157, :193-233 on one tensor: -> (p, m, v) new.  T [D, D] or None; p [D, r] is multiplied from the left, [r, D] from the right.
    The kernels take clhip_adam_step's form, m / (sqrt(v) / sqrt(bc2) + eps) * lr / bc1; `ref_form`: the reference's own (lora_sub.py:224-232),
    m / (sqrt(v) + eps) * lr sqrt(bc2) / bc1 -- the same but for eps, which there is not divided by sqrt(bc2) (1e-8 against sqrt(v))"""
    d = g + wd * p
    m = b1 * m + (1 - b1) * d
    v = b2 * v + (1 - b2) * d * d
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    qv = m / (v.sqrt() + eps) * math.sqrt(bc2) if ref_form else m / (v.sqrt() / math.sqrt(bc2) + eps)
    if T is not None:
        qv = T @ qv if T.shape[0] == qv.shape[0] else qv @ T
    return p - (lr / bc1) * qv, m, v


def proj_adam_bounded(p32, g32, m32, v32, T32, lr, b1, b2, eps, wd, step):
    """fp64 step of fp32 inputs (the scalars as their fp32 values) with the fp32 bound of the new parameter.  Counts: d = fma(wd, p, g): u |d|;  m' and v':
    two and three products and a sum on a freshly rounded 1 - beta: 4 u and 6 u on the mass of their terms, plus the error of d;  bc = 1 - powf(beta, t): powf within
    2 ulp of a value below 1 and one subtraction: relative 2 u / bc + u (bc2 enters through a square root: half, plus u);  denom: a square root, a division, a sum;
    q = m' / denom: one division;  T q: D products on operands with errors;  p - (lr / bc1) out: a division, a product and a sum."""
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    p, g, m, v = p32.double(), g32.double(), m32.double(), v32.double()
    T = None if T32 is None else T32.double()
    want, m1, v1 = proj_adam(p, g, m, v, T, lr, b1, b2, eps, wd, step)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    e_bc1, e_bc2s = 2 * U / bc1 + U, (2 * U / bc2 + U) / 2 + U
    d = g + wd * p
    ed = U * d.abs()
    em = 4 * U * ((b1 * m).abs() + ((1 - b1) * d).abs()) + (1 - b1) * ed
    ev = 6 * U * ((b2 * v).abs() + (1 - b2) * d * d) + (1 - b2) * 2 * d.abs() * ed
    root = v1.sqrt() / math.sqrt(bc2)
    denom = root + eps
    e_denom = ev / (2 * v1.sqrt().clamp_min(1e-300) * math.sqrt(bc2)) + root * (2 * U + e_bc2s) + U * denom
    qv = m1 / denom
    eq = em / denom + qv.abs() * (e_denom / denom + U)
    if T is None:
        out, eout = qv, eq
    else:
        D = T.shape[0]
        left = T.shape[0] == qv.shape[0]
        out = T @ qv if left else qv @ T
        eout = (T.abs() @ eq if left else eq @ T.abs()) + D * U * (T.abs() @ qv.abs() if left else qv.abs() @ T.abs())
    a = lr / bc1
    bound = a * (eout + out.abs() * (e_bc1 + 2 * U)) + U * want.abs()
    return want, m1, v1, bound


# --------------------------------------------------------------------------------------------------- the method on the tiny ViT
CFG = dict(img=32, patch=8, dim=64, depth=3, heads=2, mlp=256)
RANK, INC, LR, FC_LR, MARGIN, LAMBADA = 4, 3, 0.004, 0.002, 1.0, 0.05
FACTORS = ("lora_A_k", "lora_B_k", "lora_A_v", "lora_B_v")


def qkv_form(W, prev_k, prev_v, form, fac=None):
    """the three forms of the k / v rows (transformer.py:405-422): "sub" W - prev (the Gram pass), "plain" W + prev, "lora" (W + prev) + B A"""
    q, k, v = W.chunk(3, dim=0)
    if form == "sub":
        return torch.cat([q, k - prev_k, v - prev_v])
    k, v = k + prev_k, v + prev_v
    if form == "lora":
        Ak, Bk, Av, Bv = fac
        k, v = k + Bk @ Ak, v + Bv @ Av
    return torch.cat([q, k, v])


def features(P, x, form, fac=None, gram=None):
    """cls features of the toy under one weight form; P: the backbone's state dict (`feat.*`, with the prev buffers) in the dtype of the run; fac: per
    block (A_k, B_k, A_v, B_v) for "lora"; gram: a list that collects (X^T X, tokens) of every block's attention input"""
    from oracle import vit as ov
    Q = dict(P)
    for b in range(CFG["depth"]):
        pre = f"feat.transformer.blocks.{b}.attn."
        Q[pre + "qkv.weight"] = qkv_form(P[pre + "qkv.weight"], P[pre + "prev_k_weight"], P[pre + "prev_v_weight"], form, None if fac is None else fac[b])
    return ov.cls_features(Q, x, CFG, gram=gram)


def step_loss_and_grads(P, fac, head_w, head_b, x, y, protos, margin=MARGIN, lambada=LAMBADA, extra=None):
    """observe (lora_sub.py:293-311) on shifted labels y: -> (loss, ATL term, gradients of every factor [depth][4], of the head weight and bias)"""
    leaves = [t.detach().clone().requires_grad_(True) for blk in fac for t in blk] + [head_w.detach().clone().requires_grad_(True),
                                                                                       head_b.detach().clone().requires_grad_(True)]
    fl = [tuple(leaves[4 * b:4 * b + 4]) for b in range(CFG["depth"])]
    f = features(P, x, "lora", fl)
    logits = torch.nn.functional.linear(f, leaves[-2], leaves[-1])
    ce = torch.nn.functional.cross_entropy(logits, y)
    term, df, info = atl(f.detach(), y, protos, margin, lambada)
    if extra is not None:
        extra.update(pred=logits.detach().argmax(1), info=info)
    g = torch.autograd.grad(ce + (f * df).sum(), leaves)           # (f * df).sum(): the triplet term's gradient, chained through the features
    return float(ce.detach()) + lambada * float(term), float(term), [list(g[4 * b:4 * b + 4]) for b in range(CFG["depth"])], g[-2], g[-1]


def fixture_images(a):
    """the fixture stores its images at half resolution: every pixel doubled -> [..., 3, 32, 32] bytes"""
    return torch.as_tensor(a).repeat_interleave(2, -1).repeat_interleave(2, -2)


def fixture_weights(fix):
    """the backbone's state dict of the fixture (stored as bf16 words) -> fp32 tensors"""
    return {k[2:]: torch.from_numpy(v).view(torch.bfloat16).float() for k, v in fix.items() if k.startswith("w/")}


def run_fixture(fix, dtype=torch.float64, ref_form=True):
    """the three tasks of tests/golden/lorasub_tiny.npz (tools/gen_lorasub_golden.py) through this restatement, from the fixture's weights, inputs and random
    draws: -> the fixture's keys recomputed, plus `infos` (lorasub_ref.atl's info of every triplet evaluation, [task][step])"""
    P = {k: v.to(dtype) for k, v in fixture_weights(fix).items()}
    x = fixture_images(fix["x_u8"]).to(dtype) / 255.0
    xi = fixture_images(fix["xi_u8"]).to(dtype) / 255.0
    y = torch.from_numpy(fix["y"])
    depth, tasks, steps = CFG["depth"], x.shape[0], x.shape[1]
    pre = "backbone.feat.transformer.blocks.{}.attn.{}.weight"
    out, protos = {"infos": [], "losses": torch.zeros(tasks, steps, dtype=torch.float64), "atl": torch.zeros(tasks, steps, dtype=torch.float64), "preds": []}, None
    for t in range(tasks):
        train = {str(n): torch.from_numpy(fix[f"t{t}/init/{n}"]).to(dtype).clone() for n in fix[f"t{t}/trainable"]}
        T = None
        if t > 0:                                             # before_task: the Gram mean under W - prev over the task's batches, one SVD per block
            G, cnt = [torch.zeros(CFG["dim"], CFG["dim"], dtype=dtype) for _ in range(depth)], 0
            for s in range(steps):
                gram = []
                features(P, x[t, s], "sub", gram=gram)
                for b in range(depth):
                    G[b] = (G[b] * cnt + gram[b][0]) / (cnt + gram[b][1])         # transformer.py:409
                cnt += gram[0][1]
            S, ks, T = [], [], []
            for b in range(depth):
                _, Sb, Vh = torch.linalg.svd(G[b].double())
                ratio = Sb.cumsum(0) / Sb.sum()
                k = int((ratio >= 0.99).nonzero()[0][0]) + 1
                V = Vh[:k].T
                Tb = V @ V.T
                S.append(Sb); ks.append(k); T.append((Tb / Tb.norm()).to(dtype))
            out[f"t{t}/G"], out[f"t{t}/S"], out[f"t{t}/k"], out[f"t{t}/T"] = torch.stack(G), torch.stack(S), ks, torch.stack(T)
        state = {n: (torch.zeros_like(p), torch.zeros_like(p)) for n, p in train.items()}
        hw, hb = f"classifier_pool.{t}.weight", f"classifier_pool.{t}.bias"
        out["infos"].append([])
        for s in range(steps):
            fac = [tuple(train[pre.format(b, n)] for n in FACTORS) for b in range(depth)]
            extra = {}
            loss, term, gf, gw, gb = step_loss_and_grads(P, fac, train[hw], train[hb], x[t, s], y[t, s] - INC * t, protos, extra=extra)
            out["losses"][t, s], out["atl"][t, s] = loss, term
            out["preds"].append(extra["pred"])
            out["infos"][-1].append(extra["info"])
            grads = {hw: gw, hb: gb}
            for b in range(depth):
                for j, n in enumerate(FACTORS):
                    grads[pre.format(b, n)] = gf[b][j]
            for n in train:
                blk = int(n.split("blocks.")[1].split(".")[0]) if "blocks." in n else None
                m, v = state[n]
                train[n], m, v = proj_adam(train[n], grads[n], m, v, None if (T is None or blk is None) else T[blk], LR if blk is not None else FC_LR, 0.9, 0.999,
                                           1e-8, 0.0, s + 1, ref_form=ref_form)
                state[n] = (m, v)
                out[f"t{t}/s{s}/{n}"] = train[n].clone()
        for b in range(depth):                                # after_task: save_weight, then one prototype per new class under W + prev
            a = f"feat.transformer.blocks.{b}.attn."
            P[a + "prev_k_weight"] = P[a + "prev_k_weight"] + train[pre.format(b, "lora_B_k")] @ train[pre.format(b, "lora_A_k")]
            P[a + "prev_v_weight"] = P[a + "prev_v_weight"] + train[pre.format(b, "lora_B_v")] @ train[pre.format(b, "lora_A_v")]
        out["prev_k"] = torch.stack([P[f"feat.transformer.blocks.{b}.attn.prev_k_weight"] for b in range(depth)])
        out["prev_v"] = torch.stack([P[f"feat.transformer.blocks.{b}.attn.prev_v_weight"] for b in range(depth)])
        feats = torch.cat([features(P, x[t, s], "plain") for s in range(steps)])
        labels = torch.cat([y[t, s] for s in range(steps)])
        means = torch.stack([feats[labels == c].mean(0) for c in range(INC * t, INC * t + INC)])
        protos = means if protos is None else torch.cat([protos, means])
        out[f"t{t}/protos"] = protos.clone()
        f = features(P, xi, "plain")                          # inference: lora_sub.py:313-331
        f = f / (f.norm(dim=1, keepdim=True) + 1e-8)
        c = protos / protos.norm(dim=1, keepdim=True)
        out[f"t{t}/infer_pred"] = ((f[:, None, :] - c[None, :, :]) ** 2).sum(-1).argmin(1)
    out["preds"] = torch.stack(out["preds"]).view(tasks, steps, -1)
    return out


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def deviations(got, fix):
    """-> dict of the figures the fixture tests assert: first losses, all losses, the triplet terms, the worst trained tensor, T, G, prototypes, prev (G, T and
    prev are stored in fp32: a run in fp64 agrees with them to fp32 rounding, 6e-8, and the trained tensors of the later steps hold them to 1e-10 all the same)"""
    tasks = fix["losses"].shape[0]
    worst = max(((rel(v, fix[k]), k) for k, v in got.items() if "/s" in k and k in fix), default=(0.0, ""))
    return dict(first=max(rel(got["losses"][t, :1], fix["losses"][t, :1]) for t in range(tasks)), losses=rel(got["losses"], fix["losses"]),
                atl=rel(got["atl"], fix["atl"]), worst=worst,
                T=max(rel(got[f"t{t}/T"], fix[f"t{t}/T"]) for t in range(1, tasks)), protos=max(rel(got[f"t{t}/protos"], fix[f"t{t}/protos"]) for t in range(tasks)),
                G=max(rel(got[f"t{t}/G"], fix[f"t{t}/G"]) for t in range(1, tasks)), prev=max(rel(got["prev_k"], fix["prev_k"]), rel(got["prev_v"], fix["prev_v"])))


def condition_a(fix):
    """'' or why not: for every task >= 1 and layer 1 <= k < D and the cumulative ratio at least 1e-4 from 0.99 on both sides of the cut"""
    for t in range(1, fix["losses"].shape[0]):
        S, ks = fix[f"t{t}/S"], fix[f"t{t}/k"]
        for b in range(S.shape[0]):
            ratio = S[b].cumsum() / S[b].sum()
            k = int(ks[b])
            if not 1 <= k < S.shape[1] or k != int((ratio >= 0.99).nonzero()[0][0]) + 1:
                return f"(a) task {t} layer {b}: k = {k}"
            if ratio[k - 1] - 0.99 < 1e-4 or (k > 1 and 0.99 - ratio[k - 2] < 1e-4):
                return f"(a) task {t} layer {b}: the cut is {ratio[k - 1] - 0.99:.1e} above and {0.99 - ratio[k - 2]:.1e} below 0.99"
    return ""


def condition_b(got):
    """'' or why not, on run_fixture's fp64 result: every selection and hinge argument of every triplet evaluation SEP apart, a row active, and from task 1 on
    a row that takes a prototype as its negative"""
    for t, infos in enumerate(got["infos"]):
        for s, info in enumerate(infos):
            B = len(info["jp"])
            if info["gap"] < SEP:
                return f"(b) task {t} step {s}: a selection or a hinge argument is {info['gap']:.1e} apart"
            if not any(h > 0 for h in info["h"]):
                return f"(b) task {t} step {s}: no active row"
            if t > 0 and not any(j >= B for j in info["jn"]):
                return f"(b) task {t} step {s}: no row takes a prototype"
    return ""


F32_TOL = dict(first=2e-4, losses=5e-3, tensors=5e-3, T=5e-3, protos=5e-3)        # tests/test_sdlora_gpu.py's, the project's f32 tolerances


def check_f32(got, fix):
    """'' or why not: a run's deviations from the fixture against the f32 tolerances, k per layer and the predictions equal"""
    d = deviations(got, fix)
    if d["first"] >= F32_TOL["first"] or d["losses"] >= F32_TOL["losses"] or d["worst"][0] >= F32_TOL["tensors"] or d["T"] >= F32_TOL["T"] or \
            d["protos"] >= F32_TOL["protos"]:
        return f"deviations {d}"
    for t in range(fix["losses"].shape[0]):
        if t > 0 and list(got[f"t{t}/k"]) != fix[f"t{t}/k"].tolist():
            return f"k of task {t}: {list(got[f't{t}/k'])} against {fix[f't{t}/k'].tolist()}"
        if not bool((torch.as_tensor(got[f"t{t}/infer_pred"]) == torch.from_numpy(fix[f"t{t}/infer_pred"])).all()):
            return f"inference predictions of task {t}"
    return ""
