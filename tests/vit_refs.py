"""fp64 references of the ViT-path kernels between the GEMMs (csrc/attn.hip, csrc/vit_ops.hip), a helper module, not a conftest: plain torch
on the CPU, every gradient written out by hand (closed-form softmax / LayerNorm / normalize backward), never taken from the kernels and never
from autograd -- tests/test_vit_refs_cpu.py holds each of them to torch autograd in fp64, and tests/test_vit_ops_kernels_gpu.py holds the
kernels to them per block.  Also here: the seeded input generators (the shifted-logit attention inputs, the L2P tie constructions) and the error bounds, so the
CPU test can check the generators against the conditions the GPU tests rely on."""
import math

import torch

from head_refs import U, NEAR_TIE_CAP, err_ratio, f64, larger, sum_bound        # noqa: F401  (re-exported: one error measure for both sweeps)

NORM_EPS = 1e-12        # F.normalize


def randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def rand01(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g)


def rb(t):
    """fp32 values rounded to bf16 (still stored as fp32): what the bf16 mode is fed, and what its reference sees"""
    return t.to(torch.bfloat16).float()


def as_mode(t, dt):
    return rb(t) if dt == "bf16" else t


# ----------------------------------------------------------------------------------------------- bounds
# the numbers the suite already holds each op to (tests/test_vit_kernels_gpu.py), now applied per block
ATTN_OUT = {"bf16": 2e-2, "f32": 2e-5}
ATTN_GRAD = {"bf16": 4e-2, "f32": 5e-5}
LN = {"bf16": 2e-2, "f32": 2e-5}
LN_POOL_FEAT = 1e-5
COPY = {"bf16": 4e-3, "f32": 1e-6}          # patchify / assemble / weight prep
LORA_GRAD_MFMA, LORA_GRAD = 1e-2, 1e-4
GRAM, GRAM_BATCHED = 1e-4, 1e-5
L2P_SIM, L2P_DKEY = 1e-5, 1e-4
PROMPT_GRAD = 1e-5
FLOOR = 1e-7                                # absolute floor, times the largest max|ref| of the whole tensor


def block_bound(rel, ref_block, ref_all):
    """rel * max|ref| of the block + 1e-7 * max|ref| of the whole tensor (a block that is legitimately near zero does not divide by nothing)"""
    return rel * float(ref_block.abs().max()) + FLOOR * float(ref_all.abs().max())


# lse, LN mean and LN rstd have no project number.  Each is held to four times the largest error measured on the MI355X against the
# references below over all cases of tests/test_vit_ops_kernels_gpu.py (which prints the maxima as `[measure]`), and never to less than the
# order-independent forward bound of the sums involved (lse_floor / mean_floor / rstd_floor).  None = NOT MEASURED YET: the forward bound
# alone holds, which is the tighter of the two readings; the numbers go here once a run has printed them, never from a second run of the
# kernel against itself
LSE_ABS = None          # absolute, natural-log units
LN_MEAN_REL = None      # relative to |mean|
LN_RSTD_REL = None      # relative to rstd


def measured(x):
    """a measured bound, or 0 where none has been measured (the forward-bound floor then decides alone)"""
    return 0.0 if x is None else x


def lse_floor(logit_err, N, lse):
    """forward bound of the logit (logit_err = hd 2^-24 scale max_key sum_i |q_i k_i| of the row: an hd-term fp32 dot product), of the
    N-term sum of exponentials (relative N 2^-24 of the sum = absolute in its log), and one rounding of the stored value"""
    return logit_err + N * U + U * lse.abs()


def mean_floor(x):
    """|mean error| <= D 2^-24 sum|x| / D per row"""
    return U * x.abs().sum(-1)


def rstd_floor(D):
    """rstd = (var + eps)^-1/2: half the relative forward bound of the D-term sum of squares, plus the roundings of the mean, the
    division, the eps add and rsqrt"""
    return (0.5 * D + 4) * U


# -------------------------------------------------------------------------------------------- attention
def heads(t, B, N, H, hd):
    """[B*N, H*hd] -> [B, H, N, hd]"""
    return t.reshape(B, N, H, hd).permute(0, 2, 1, 3)


def split_qkv(t, B, N, H, hd):
    """packed [B*N, 3*H*hd] -> q, k, v each [B, H, N, hd]"""
    q, k, v = t.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    return q, k, v


def attn_ref(qkv, dout, B, N, H, hd):
    """softmax(q k^T / sqrt(hd)) v on the packed qkv [B*N, 3D] and its backward for the upstream gradient dout [B*N, D], in closed form:
    P = exp(S - lse), dV = P^T dO, dP = dO V^T, dS = P (dP - rowsum(dO O)), dQ = dS K scale, dK = dS^T Q scale.
    Returns out, lse (natural log, [B,H,N]), dq, dk, dv, the tensors as [B,H,N,hd]."""
    qkv, dout = f64(qkv), f64(dout)
    q, k, v = split_qkv(qkv, B, N, H, hd)
    scale = 1.0 / math.sqrt(hd)
    s = (q @ k.transpose(-2, -1)) * scale
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    o = p @ v
    do = heads(dout, B, N, H, hd)
    dv = p.transpose(-2, -1) @ do
    dp = do @ v.transpose(-2, -1)
    ds = p * (dp - (do * o).sum(-1, keepdim=True))
    dq = (ds @ k) * scale
    dk = (ds.transpose(-2, -1) @ q) * scale
    return o, lse, dq, dk, dv


def attn_logit_abs(qkv, B, N, H, hd):
    """scale * max_key sum_i |q_i k_i| per query row, [B,H,N]: hd 2^-24 times this is the forward bound of the fp32 logit, and a rounding
    error in the logit is a relative error in P"""
    q, k, _ = split_qkv(f64(qkv), B, N, H, hd)
    return (q.abs() @ k.abs().transpose(-2, -1)).amax(-1) / math.sqrt(hd)


def attn_cancel_bound(qkv, dout, B, N, H, hd, eps_o, eps_ds):
    """forward bounds of dq and dk where they are cancellations (one token: dS = P (dP - rowsum(dO O)) is exactly zero; identical keys:
    dq = scale sum_j dS_j k_j with sum_j dS_j = 0), elementwise, from the fp64 reference: the two hd-term fp32 sums dP and rowsum(dO O) carry
    hd 2^-24 sum|term| each, O as stored carries eps_o (2^-9 in the bf16 modes), dS as fed to the second product carries eps_ds (2^-9 where
    it is packed to bf16 for the MFMA, N 2^-24 for an fp32 sum over N terms).  Returns the bounds of dq and dk, [B,H,N,hd]."""
    qkv, dout = f64(qkv), f64(dout)
    q, k, v = split_qkv(qkv, B, N, H, hd)
    scale = 1.0 / math.sqrt(hd)
    o, lse, _, _, _ = attn_ref(qkv, dout, B, N, H, hd)
    p = torch.exp((q @ k.transpose(-2, -1)) * scale - lse.unsqueeze(-1))
    do = heads(dout, B, N, H, hd)
    ds = p * (do @ v.transpose(-2, -1) - (do * o).sum(-1, keepdim=True))
    ds_err = p * (hd * U * (do.abs() @ v.abs().transpose(-2, -1)) + (hd * U + eps_o) * (do.abs() * o.abs()).sum(-1, keepdim=True)) + eps_ds * ds.abs()
    return scale * (ds_err @ k.abs()), scale * (ds_err.transpose(-2, -1) @ q.abs())


def attn_references(big, bd, B, N, Lp, H, hd, dt):
    """fp64 reference of the packed form (coda_ref.pack_prefix; Lp = 0: plain attention) cut to the rows the kernels produce: {tensor: (ref, relative
    bound, elementwise extra)} for out, dq, dk, dv (token rows) and dpk, dpv (prefix rows), the conditioning of the token queries' exponent [B,H,N], and the
    whole lse reference [B,H,T].  The bounds of run_attention (tests/test_vit_ops_kernels_gpu.py) / run_prefix (tests/test_prefix_attn_kernels_gpu.py), which
    the executor's test shares: judged per (batch, head) block by `blocked_ratio`"""
    T = N + Lp
    ref_o, ref_lse, ref_dq, ref_dk, ref_dv = attn_ref(big, bd, B, T, H, hd)
    assert float(ref_dq[:, :, :Lp].abs().max()) == 0.0 if Lp else True       # zero dout: the prefix rows' queries get nothing, as the kernel assumes
    labs = attn_logit_abs(big, B, T, H, hd)[:, :, Lp:]                       # [B,H,N]: the token queries
    cond = hd * U * labs
    bf = dt == "bf16"
    mfma = bf and hd == 64
    cq, ck = attn_cancel_bound(big, bd, B, T, H, hd, 2.0 ** -9 if bf else U, 2.0 ** -9 if mfma else T * U)

    def amax(t):
        return t.abs().amax(dim=(-1, -2), keepdim=True)
    tok, pre = (lambda t: t[:, :, Lp:]), (lambda t: t[:, :, :Lp])
    cmax = cond.amax(-1)[..., None, None]
    store = 2.0 ** -9 if bf else 0.0                                          # the bf16 store step dpk / dpv do not have
    bounds = {"out": (tok(ref_o), ATTN_OUT[dt], cond[..., None] * amax(tok(ref_o)).expand_as(tok(ref_o))),
              "dq": (tok(ref_dq), ATTN_GRAD[dt], tok(cq) + cond[..., None] * amax(tok(ref_dq))),
              "dk": (tok(ref_dk), ATTN_GRAD[dt], tok(ck) + cmax * amax(tok(ref_dk))),
              "dv": (tok(ref_dv), ATTN_GRAD[dt], (cmax * amax(tok(ref_dv))).expand_as(tok(ref_dv)))}
    if Lp:
        bounds["dpk"] = (pre(ref_dk), ATTN_GRAD[dt] - store, pre(ck) + cmax * amax(pre(ref_dk)))
        bounds["dpv"] = (pre(ref_dv), ATTN_GRAD[dt] - store, (cmax * amax(pre(ref_dv))).expand_as(pre(ref_dv)))
    return bounds, cond, ref_lse


def blocked_allowed(ref, rel, extra=None):
    """the elementwise bound of a [B,H,...] tensor judged per (batch, head) block: rel * the block's max|ref| + 1e-7 max|ref| of the tensor, or `extra` where larger"""
    allowed = rel * ref.abs().amax(dim=(-1, -2), keepdim=True).expand_as(ref) + FLOOR * float(ref.abs().max())
    return allowed if extra is None else larger(allowed, extra)


def attn_inputs(B, N, H, hd, seed, dt):
    """the inputs of the existing attention test: qkv = 1.5 randn, dout = randn, rounded to the mode's dtype"""
    D = H * hd
    return as_mode(randn((B * N, 3 * D), seed, 1.5), dt), as_mode(randn((B * N, D), seed + 1), dt)


def shift_amplitude(hd):
    """a (a multiple of 1/4, bf16-exact) with a^2 sqrt(hd) ~ 128: q = -+a against keys a + noise puts every logit of the row near -+128"""
    return round(4 * math.sqrt(128.0 / math.sqrt(hd))) / 4


SHIFT_LOW, SHIFT_HIGH, SHIFT_ONEHOT = 0, 1, 2       # query rows of the constructions below (batch 0)
SHIFT_ONEHOT_KEY = 5
SHIFT_UNIFORM = (1, 2)                              # (batch, head) whose keys are all identical


def attn_shifted_inputs(B, N, H, hd, seed):
    """bf16-exact qkv / dout (both modes see the same numbers) with logits far from zero.  Needs B >= 2, H >= 3, N >= 8.
    batch 0, head 0: every key = a + unit noise in every element; query row 0 = -a (all logits near -128, lse < -100), query row 1 = +a
                     (all logits near +128, lse > +100); the other rows of the head see logits a sum(q) / sqrt(hd) + noise
    batch 0, head 1: query row 2 = 6 x key 5 (logit 6 |k|^2 / sqrt(hd) ~ 6 sqrt(hd) against N(0, 6^2) for the others: a one-hot softmax)
    batch 1, head 2: all keys identical (a uniform softmax in every row)"""
    assert B >= 2 and H >= 3 and N >= 8
    D = H * hd
    a = shift_amplitude(hd)
    x = randn((B, N, 3, H, hd), seed)
    x[0, :, 1, 0, :] = a + randn((N, hd), seed + 2)
    x[0, SHIFT_LOW, 0, 0, :] = -a
    x[0, SHIFT_HIGH, 0, 0, :] = a
    x[0, SHIFT_ONEHOT, 0, 1, :] = 6 * x[0, SHIFT_ONEHOT_KEY, 1, 1, :]
    x[1, :, 1, 2, :] = x[1, 0, 1, 2, :].clone()
    return rb(x.reshape(B * N, 3 * D)), rb(randn((B * N, D), seed + 1))


# -------------------------------------------------------------------------------------------- LayerNorm
def ln_ref(x, gamma, beta, dy, eps):
    """y, mean, rstd, dx of LayerNorm over the last dimension (gamma / beta frozen: input gradient only)"""
    x, gamma, beta, dy = f64(x), f64(gamma), f64(beta), f64(dy)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mu) * rstd
    dg = dy * gamma
    dx = rstd * (dg - dg.mean(-1, keepdim=True) - xh * (dg * xh).mean(-1, keepdim=True))
    return xh * gamma + beta, mu.squeeze(-1), rstd.squeeze(-1), dx


def ln_inputs(M, D, seed, dt, offset=False):
    """x (2 randn + 0.3, or 100 + 0.5 randn: |mean| >> std, where a one-pass variance goes wrong), gamma, beta, dy, g0 (the gradient
    accumulated into); x, dy, g0 rounded to the mode's dtype"""
    x = 100 + randn((M, D), seed, 0.5) if offset else randn((M, D), seed, 2.0) + 0.3
    return (as_mode(x, dt), randn((D,), seed + 1, 0.2) + 1, randn((D,), seed + 2, 0.1), as_mode(randn((M, D), seed + 3), dt),
            as_mode(randn((M, D), seed + 4), dt))


def ln_pool_ref(x, gamma, beta, dfeat, B, N, D, P, eps):
    """feat[b] = mean over the first P tokens of LN(x[b]); g = its input gradient for dfeat (rows >= P: zero).  Returns feat [B,D], g [B,N,D]"""
    x3 = f64(x).reshape(B, N, D)
    dy = (f64(dfeat) / P).unsqueeze(1).expand(B, P, D)
    y, _, _, dx = ln_ref(x3[:, :P], gamma, beta, dy, eps)
    g = torch.zeros(B, N, D, dtype=torch.float64)
    g[:, :P] = dx
    return y.mean(1), g


def ln_pool_inputs(B, N, D, seed, dt):
    return as_mode(randn((B * N, D), seed, 2.0), dt), randn((D,), seed + 1, 0.2) + 1, randn((D,), seed + 2, 0.1), randn((B, D), seed + 3)


# ----------------------------------------------------------------------------- weight preparation, LoRA
def weight_eff_ref(w, Ak=None, Bk=None, Av=None, Bv=None):
    """the effective qkv weight [3 Dl, C]: W, + B_k A_k on the k rows [Dl, 2 Dl), + B_v A_v on the v rows [2 Dl, 3 Dl)"""
    eff = f64(w).clone()
    if Ak is not None:
        Dl = eff.shape[0] // 3
        eff[Dl:2 * Dl] += f64(Bk) @ f64(Ak)
        eff[2 * Dl:] += f64(Bv) @ f64(Av)
    return eff


def lora_inputs(rows, cols, rank, seed):
    """w [rows, cols], A_k / A_v [rank, cols], B_k / B_v [rows / 3, rank] in fp32 (rank 0: no LoRA tensors)"""
    w = randn((rows, cols), seed)
    if rank == 0:
        return w, None, None, None, None
    Dl = rows // 3
    return w, randn((rank, cols), seed + 1), randn((Dl, rank), seed + 2), randn((rank, cols), seed + 3), randn((Dl, rank), seed + 4)


def lora_db_ref(x, dqkv, Ak, Av, D):
    """dB_k = dK^T (X A_k^T), dB_v = dV^T (X A_v^T): the B gradient through the rank-r shortcut (x [M,D], dqkv [M,3D])"""
    x, d = f64(x), f64(dqkv)
    return d[:, D:2 * D].T @ (x @ f64(Ak).T), d[:, 2 * D:].T @ (x @ f64(Av).T)


def gram_ref(x):
    x = f64(x)
    return x.T @ x


# ------------------------------------------------------------------------------------------------- L2P
def l2p_ref(q, key, top_k):
    """prompt.py's selection on q [B,D] and key [pool,D], in fp64.  Returns a dict:
    sim [B,pool] cosines (F.normalize, eps 1e-12); topk [B,top_k] per-sample picks (largest first, ties to the lower id); counts [pool];
    ids: the top_k prompt ids under "count descending, then id ascending"; reduce_sim = sum_b sum_{j in ids} sim[b,j] / B; dkey = its
    gradient w.r.t. key (a row whose norm sits under the clamp has the constant denominator 1e-12); gap [B]: k-th minus (k+1)-th
    cosine of every sample (inf where pool == top_k); noise [B]: the fp32 forward bounds D 2^-24 sum|q_i k_i| / (|q||k|) of those two
    cosines, added"""
    q, key = f64(q), f64(key)
    B, D = q.shape
    pool = key.shape[0]
    qn_ = (q * q).sum(1).sqrt().clamp_min(NORM_EPS)
    kn_ = (key * key).sum(1).sqrt().clamp_min(NORM_EPS)
    qn, kn = q / qn_[:, None], key / kn_[:, None]
    sim = qn @ kn.T
    order = torch.sort(-sim, dim=1, stable=True)[1]
    topk = order[:, :top_k]
    counts = torch.bincount(topk.reshape(-1), minlength=pool)
    ids = sorted(range(pool), key=lambda j: (-int(counts[j]), j))[:top_k]
    sel = torch.tensor(ids)
    reduce_sim = sim[:, sel].sum() / B
    sbar = qn.mean(0)
    dkey = torch.zeros_like(key)
    for j in ids:
        if float((key[j] * key[j]).sum().sqrt()) < NORM_EPS:
            dkey[j] = sbar / NORM_EPS
        else:
            dkey[j] = (sbar - kn[j] * (kn[j] @ sbar)) / kn_[j]
    cos_abs = (q.abs() @ key.abs().T) / (qn_[:, None] * kn_[None, :])
    noise_all = D * U * cos_abs
    if pool > top_k:
        ssort = sim.gather(1, order)
        gap = ssort[:, top_k - 1] - ssort[:, top_k]
        noise = noise_all.gather(1, order[:, top_k - 1:top_k + 1]).sum(1)
    else:
        gap = torch.full((B,), float("inf"), dtype=torch.float64)
        noise = torch.zeros(B, dtype=torch.float64)
    return dict(sim=sim, topk=topk, counts=counts, ids=ids, reduce_sim=reduce_sim, dkey=dkey, gap=gap, noise=noise)


L2P_CASES = [(1, 8, 1, 1, 1), (16, 128, 10, 5, 5), (40, 100, 64, 5, 2), (7, 64, 6, 6, 3)]      # B, D, pool, top_k, length
L2P_ZERO_KEY_CASE, L2P_ZERO_KEY_ROW = (7, 64, 6, 6, 3), 2                                     # top_k == pool: the zero key is selected


def l2p_seed(B, D, pool):
    return 4000 + 7 * B + D + pool


def l2p_inputs(B, D, pool, length, seed, zero_key_row=None):
    """q = randn, key and prompt uniform in (0, 1) (the existing test's inputs); optionally one all-zero key row"""
    q, key, prompt = randn((B, D), seed), rand01((pool, D), seed + 1), rand01((pool, length, D), seed + 2)
    if zero_key_row is not None:
        key[zero_key_row] = 0.0
    return q, key, prompt


L2P_TIE_SHAPE = (6, 16, 5, 2, 2)                                                              # B, D, pool, top_k, length
L2P_TIE_PICKS = [(1, 3), (3, 1), (1, 3), (0, 4), (4, 2), (3, 1)]                              # per-sample top-2, in order
L2P_TIE_IDS = [1, 3]


def l2p_tie_inputs(seed=77):
    """a batch-majority tie: the keys are near-orthogonal (e_j + 0.05 noise), sample b = key[first] + 0.6 key[second] + 0.02 noise, so its
    top-2 are exactly L2P_TIE_PICKS[b].  Prompt ids 1 and 3 are each picked by the same four samples and by no other; every other id is
    picked once or twice: the selected ids are [1, 3], the lower id first"""
    B, D, pool, top_k, length = L2P_TIE_SHAPE
    key = torch.eye(pool, D) + randn((pool, D), seed, 0.05)
    q = torch.stack([key[a] + 0.6 * key[b] for a, b in L2P_TIE_PICKS]) + randn((B, D), seed + 1, 0.02)
    return q, key, rand01((pool, length, D), seed + 2)


# ------------------------------------------------------------------------------------------------ tokens
def patchify_ref(img, p):
    """[B,3,S,S] -> [B * (S/p)^2, 3 p p], column order (c, i, j) = the Conv2d weight flattening, patches row-major"""
    B, C, S, _ = img.shape
    g = S // p
    x = img.reshape(B, C, g, p, g, p).permute(0, 2, 4, 1, 3, 5)
    return x.reshape(B * g * g, C * p * p)


def assemble_ref(pe, cls, pos, prompt, B, npch, n_prompt, D):
    """x[b] = [prompt tokens (no pos-embed); cls + pos[0]; patch_emb[b] + pos[1:]] -> [B * (n_prompt + 1 + npch), D]"""
    pe, cls, pos = f64(pe).reshape(B, npch, D), f64(cls), f64(pos)
    parts = [(cls + pos[0]).expand(B, 1, D), pe + pos[1:]]
    if n_prompt:
        parts.insert(0, f64(prompt)[:n_prompt].expand(B, n_prompt, D))
    return torch.cat(parts, 1).reshape(-1, D)


def prompt_grad_ref(g, B, N, P, D):
    return f64(g).reshape(B, N, D)[:, :P].sum(0)
