"""Plain-torch restatement of CODA-Prompt on the ViT path (a helper module, not a conftest), in the dtype of its inputs (fp64 in the tests):

  * prefix attention: MultiHeadAttention.forward with `prompt` (transformer.py:169-197) -- per sample Lp key / value rows without a query in front of the
    token keys -- and `pack_prefix`, which writes the same computation as PLAIN attention over Lp + N tokens (the first Lp rows carry the prefix keys and
    values, an arbitrary query and zero dout: their dS is exactly zero, they contribute nothing to dK / dV), so that the bounds and references of
    tests/vit_refs.py apply to the prefix form of csrc/attn.hip unchanged;
  * the prompt assembly, CodaPrompt.forward (prompt.py:158-220), on the literal formulas (F.normalize), gradients by autograd;
  * the prefixed ViT (VisionTransformer.forward with `prompt`, transformer.py:2272-2295, ViTZoo.forward, vit.py:120-138) on oracle.vit's blocks;
  * the method (core/model/codaprompt.py) with Adam.

tests/test_coda_cpu.py holds it to tests/golden/coda_tiny.npz (fp64 runs of the reference's own classes) at 1e-10; the GPU tests compare the kernels,
the executor and the method with it.  As in the reference, `task_count` never moves (nothing calls process_task_count): the window is [0, pool / n_tasks)
in every task, for training and inference alike.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vit as ov

CFG = dict(img=32, patch=8, dim=64, depth=6, heads=2, mlp=256)      # the fixture's toy ViT
W_TAG = "coda_tiny"                                                   # the frozen weights: oracle.vit.det_params(CFG, W_TAG)
LAYERS = (0, 1, 2, 3, 4)                                              # prompt.py:71
POOL, LENGTH, TASKS, STEPS, BATCH, INC = 6, 8, 2, 3, 6, 3
LR, BETAS = 0.004, (0.9, 0.999)                                       # tools/gen_coda_golden.py records why this lr


# ------------------------------------------------------------------------------------------------ prefix attention
def prefix_attention(qkv, pk, pv, heads):
    """qkv [B, N, 3D], pk / pv [B, Lp, D] -> [B, N, D] (before the projection)"""
    B, N, D3 = qkv.shape
    D = D3 // 3
    hd = D // heads
    q, k, v = qkv.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    k = torch.cat((pk.reshape(B, -1, heads, hd).permute(0, 2, 1, 3), k), dim=2)
    v = torch.cat((pv.reshape(B, -1, heads, hd).permute(0, 2, 1, 3), v), dim=2)
    a = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)
    return (a @ v).transpose(1, 2).reshape(B, N, D)


def pack_prefix(qkv, pk, pv, dout, B, N, Lp, D, qfill=None):
    """-> (packed qkv [B * (Lp + N), 3D], packed dout [B * (Lp + N), D]): sample b's rows are [prefix | tokens]; the prefix rows' queries are `qfill`
    ([B, Lp, D], default zero) and their dout is zero"""
    T = Lp + N
    big = torch.zeros(B, T, 3, D, dtype=qkv.dtype)
    big[:, Lp:] = qkv.reshape(B, N, 3, D)
    big[:, :Lp, 1] = pk.reshape(B, Lp, D)
    big[:, :Lp, 2] = pv.reshape(B, Lp, D)
    if qfill is not None:
        big[:, :Lp, 0] = qfill.reshape(B, Lp, D)
    bd = torch.zeros(B, T, D, dtype=dout.dtype)
    bd[:, Lp:] = dout.reshape(B, N, D)
    return big.reshape(B * T, 3 * D), bd.reshape(B * T, D)


# ------------------------------------------------------------------------------------------------------- assembly
def assemble(q, K, A, P, f):
    """prompt.py:190-201 over the components [0, f): -> ek, ev [B, L/2, D], c [B, f]"""
    K, A, P = K[:f], A[:f], P[:f]
    aq = torch.einsum("bd,kd->bkd", q, A)
    c = torch.einsum("bkd,kd->bk", F.normalize(aq, dim=2), F.normalize(K, dim=1))
    P_ = torch.einsum("bk,kld->bld", c, P)
    i = P.shape[1] // 2
    return P_[:, :i], P_[:, i:], c


def assemble_grads(q, K, A, P, s, f, dek, dev):
    """rows [s, f) of dK, dA, dP for the cotangents dek, dev (rows below s are detached, prompt.py:174-182), and the forward results"""
    Kt, At, Pt = (t[s:f].detach().clone().requires_grad_(True) for t in (K, A, P))
    cat = lambda past, cur: torch.cat((past[:s].detach(), cur), dim=0)
    ek, ev, c = assemble(q, cat(K, Kt), cat(A, At), cat(P, Pt), f)
    dK, dA, dP = torch.autograd.grad((ek * dek).sum() + (ev * dev).sum(), (Kt, At, Pt))
    return dK, dA, dP, ek.detach(), ev.detach(), c.detach()


# --------------------------------------------------------------------------------------------------- prefixed ViT
def block(W, i, x, heads, prefix=None, eps=1e-5):
    """oracle.vit.block with the attention of transformer.py:175-180 when `prefix` = (ek, ev) is given"""
    if prefix is None:
        return ov.block(W, i, x, heads, eps=eps)
    b = f"feat.transformer.blocks.{i}."
    D = x.shape[-1]
    h = F.layer_norm(x, (D,), W[b + "ln_1.weight"], W[b + "ln_1.bias"], eps)
    o = prefix_attention(F.linear(h, W[b + "attn.qkv.weight"], W[b + "attn.qkv.bias"]), prefix[0], prefix[1], heads)
    x = x + F.linear(o, W[b + "attn.proj.weight"], W[b + "attn.proj.bias"])
    h = F.layer_norm(x, (D,), W[b + "ln_2.weight"], W[b + "ln_2.bias"], eps)
    return x + F.linear(F.gelu(F.linear(h, W[b + "mlp.fc1.weight"], W[b + "mlp.fc1.bias"])), W[b + "mlp.fc2.weight"], W[b + "mlp.fc2.bias"])


def prefixed_features(W, img, cfg, prefixes):
    """prefixes: {layer: (ek, ev)}; -> the final-LN output at the cls token"""
    x = ov.tokens(W, img, cfg)
    for i in range(cfg["depth"]):
        x = block(W, i, x, cfg["heads"], prefixes.get(i))
    return F.layer_norm(x, (x.shape[-1],), W["feat.norm.weight"], W["feat.norm.bias"], 1e-6)[:, 0]


def coda_features(W, pool, img, cfg, f, layers=LAYERS):
    """ViTZoo.forward with a CODA pool (vit.py:120-127): query = cls feature of the prompt-free forward, without gradient.
    pool: {"e_k_{l}" / "e_a_{l}" / "e_p_{l}": tensor}"""
    with torch.no_grad():
        q = ov.cls_features(W, img, cfg)
    pre = {}
    for l in layers:
        ek, ev, _ = assemble(q, pool[f"e_k_{l}"], pool[f"e_a_{l}"], pool[f"e_p_{l}"], f)
        pre[l] = (ek, ev)
    return prefixed_features(W, img, cfg, pre)


# --------------------------------------------------------------------------------------------------------- method
def adam_step(params, grads, m, v, t, lr=LR, betas=BETAS, eps=1e-8):
    """torch.optim.Adam (weight_decay 0) on lists, in place"""
    with torch.no_grad():
        for p, g, mi, vi in zip(params, grads, m, v):
            mi.mul_(betas[0]).add_(g, alpha=1 - betas[0])
            vi.mul_(betas[1]).addcmul_(g, g, value=1 - betas[1])
            p.sub_(lr * (mi / (1 - betas[0] ** t)) / ((vi / (1 - betas[1] ** t)).sqrt() + eps))


class Method:
    """core/model/codaprompt.py on dicts of tensors.  W: the frozen `feat.*` weights; pool: the 15 pool tensors; the head grows per task (the new rows come
    from the caller: the fixture stores the reference's draws)"""

    def __init__(self, W, pool, cfg=CFG, n_tasks=TASKS, pool_size=POOL, dtype=torch.float64):
        self.W = {k: v.to(dtype) for k, v in W.items()}
        self.pool = {k: v.to(dtype).clone().requires_grad_(True) for k, v in pool.items()}
        self.cfg, self.dtype = cfg, dtype
        self.f = pool_size // n_tasks                         # task_count stays 0: the window of every task
        self.last_out, self.out_dim = 0, 0
        self.head_w = self.head_b = None

    def before_task(self, head_w, head_b):
        """the regrown head as the reference leaves it (old rows already copied in by the caller's values)"""
        self.head_w = torch.as_tensor(head_w).to(self.dtype).clone().requires_grad_(True)
        self.head_b = torch.as_tensor(head_b).to(self.dtype).clone().requires_grad_(True)
        self.out_dim = self.head_w.shape[0]
        self.names = sorted(self.pool) + ["classifier.weight", "classifier.bias"]
        self.params = [self.pool[n] for n in sorted(self.pool)] + [self.head_w, self.head_b]
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        self.t = 0

    def after_task(self):
        self.last_out = self.out_dim

    def logits(self, x):
        return F.linear(coda_features(self.W, self.pool, x, self.cfg, self.f), self.head_w, self.head_b)

    def step(self, x, y):
        logits = self.logits(x)
        loss = F.cross_entropy(logits[:, self.last_out:], y - self.last_out)          # -inf below last_out_dim == CE over the window
        grads = torch.autograd.grad(loss, self.params, allow_unused=True)
        grads = [torch.zeros_like(p) if g is None else g for p, g in zip(self.params, grads)]
        self.t += 1
        adam_step(self.params, grads, self.m, self.v, self.t)
        masked = logits.detach().clone()
        masked[:, :self.last_out] = -math.inf
        return loss.detach(), masked.argmax(1), grads

    def inference(self, x):
        with torch.no_grad():
            return self.logits(x).argmax(1)

    def state(self):
        return {n: p.detach().clone() for n, p in zip(self.names, self.params)}


# ------------------------------------------------------------------------------- the fixture, replayed by the restatement
def replay(fix, dtype):
    """tests/coda_ref.py on the fixture's inputs -> {key: tensor} in the fixture's layout"""
    W = ov.det_params(CFG, str(fix["w_tag"]))
    pool = {k[6:]: torch.as_tensor(v) for k, v in fix.items() if k.startswith("pool0/")}
    m = Method(W, pool, dtype=dtype)
    x = torch.as_tensor(fix["x_u8"]).to(dtype) / 255.0
    xi = torch.as_tensor(fix["infer_x_u8"]).to(dtype) / 255.0
    y = torch.as_tensor(fix["y"])
    got = {"losses": [], "preds": [], "infer_preds": []}
    for t in range(TASKS):
        m.before_task(fix[f"t{t}/init/classifier.weight"], fix[f"t{t}/init/classifier.bias"])
        for s in range(STEPS):
            loss, pred, _ = m.step(x[t, s], y[t, s])
            got["losses"].append(loss)
            got["preds"].append(pred)
            for n, v in m.state().items():
                got[f"t{t}/s{s}/{n}"] = v[:m.f] if n.startswith("e_") else v
        m.after_task()
        got["infer_preds"].append(m.inference(xi))
    got["losses"] = torch.stack(got["losses"]).view(TASKS, STEPS)
    got["preds"] = torch.stack(got["preds"]).view(TASKS, STEPS, BATCH)
    got["infer_preds"] = torch.stack(got["infer_preds"])
    return got


def deviations(got, fix):
    """(first losses, all losses, (worst trained tensor relative to its max-abs, its key)) against the fixture"""
    rel = lambda a, b: float((np.asarray(a, np.float64) - np.asarray(b, np.float64)).__abs__().max() / (np.abs(np.asarray(b, np.float64)).max() + 1e-300))
    first = max(rel(got["losses"][t, :1], fix["losses"][t, :1]) for t in range(TASKS))
    worst = max((rel(v, fix[k]), k) for k, v in got.items() if k.startswith("t"))
    return first, rel(got["losses"], fix["losses"]), worst
