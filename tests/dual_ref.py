"""Plain-torch restatement of DualPrompt on the ViT path (a helper module, not a conftest), in the dtype of its inputs (fp64 in the tests):

  * the pool's forward, DualPrompt.forward (prompt.py:269-337), train and eval, on the literal formulas (F.normalize, torch.topk), gradients by autograd;
  * the prefixed ViT (transformer.py:2272-2295, ViTZoo.forward, vit.py:120-138) on coda_ref.prefixed_features, with a prefix length per layer;
  * the method (core/model/dualprompt.py) with Adam.

tests/test_dual_cpu.py holds it to tests/golden/dual_tiny.npz (fp64 runs of the reference's own classes) at 1e-10; the GPU tests compare the kernels, the
executor and the method with it.  Training takes row `task_id` of every E-layer (`task_id_bootstrap` is hard-coded True, prompt.py:255; the other branch is
not restated); inference takes the top-1 key among all `POOL` keys.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import coda_ref as CR
from oracle import vit as ov

CFG = CR.CFG                                                          # the fixture's toy ViT: img 32, patch 8, D 64, depth 6, 2 heads
W_TAG = "dual_tiny"                                                   # the frozen weights: oracle.vit.det_params(CFG, W_TAG)
G_LAYERS, E_LAYERS = (0, 1), (2, 3, 4)                                # prompt.py:258-259
POOL, LG, LE, TASKS, STEPS, BATCH, INC, INFER = 10, 6, 8, 3, 3, 6, 3, 12
LR, BETAS = 0.004, (0.9, 0.999)                                       # tools/gen_dual_golden.py records why this lr
GAP = 1e-3                                                            # the fixture's least top-two cosine gap at inference
MARGIN_REL = 5e-3                                                     # logit margins below this fraction of the task's max |logit| are not compared


def names():
    """the pool's parameter names in the reference's creation order (prompt.py:241-251)"""
    return [f"g_p_{g}" for g in G_LAYERS] + [f"e_{w}_{e}" for e in E_LAYERS for w in ("p", "k")]


# --------------------------------------------------------------------------------------------------------- pool
def select(q, K, P, train, task_id):
    """one E-layer, prompt.py:272-306: -> pk, pv [B, Le/2, D], cos [B, pool], idx [B], the layer's key loss (0 in eval)"""
    B = q.shape[0]
    n_K = F.normalize(K, dim=1)
    qn = F.normalize(q, dim=1).detach()
    cos = torch.einsum("bj,kj->bk", qn, n_K)
    i = P.shape[1] // 2
    if train:
        loss = (1.0 - cos[:, task_id]).sum()
        P_ = P[task_id].expand(B, -1, -1)
        idx = torch.full((B,), int(task_id), dtype=torch.long)
    else:
        idx = torch.topk(cos, 1, dim=1).indices[:, 0]
        P_ = P[idx]
        loss = torch.zeros((), dtype=q.dtype)
    return P_[:, :i], P_[:, i:], cos, idx, loss


def shared(q, G):
    """one G-layer, prompt.py:310-316"""
    j = G.shape[0] // 2
    P_ = G.expand(q.shape[0], -1, -1)
    return P_[:, :j], P_[:, j:]


def prefixes(q, pool, train, task_id, g_layers=G_LAYERS, e_layers=E_LAYERS):
    """-> ({layer: (pk, pv)}, key loss (the E-layers in order), {layer: (cos, idx)})"""
    pre, sel = {}, {}
    loss = torch.zeros((), dtype=q.dtype)
    for l in g_layers:
        pre[l] = shared(q, pool[f"g_p_{l}"])
    for l in e_layers:
        pk, pv, cos, idx, ll = select(q, pool[f"e_k_{l}"], pool[f"e_p_{l}"], train, task_id)
        pre[l], sel[l] = (pk, pv), (cos.detach(), idx)
        loss = loss + ll
    return pre, loss, sel


def dual_features(W, pool, img, cfg, train, task_id):
    """ViTZoo.forward with a DualPrompt pool (vit.py:120-127): query = cls feature of the prompt-free forward, without gradient.
    -> features, key loss, {layer: (cos, idx)}"""
    with torch.no_grad():
        q = ov.cls_features(W, img, cfg)
    pre, loss, sel = prefixes(q, pool, train, task_id)
    return CR.prefixed_features(W, img, cfg, pre), loss, sel


# --------------------------------------------------------------------------------------------------------- method
class Method:
    """core/model/dualprompt.py on dicts of tensors.  W: the frozen `feat.*` weights; pool: the 8 pool tensors; the head grows per task (the new rows come
    from the caller: the fixture stores the reference's draws)"""

    def __init__(self, W, pool, cfg=CFG, dtype=torch.float64):
        self.W = {k: v.to(dtype) for k, v in W.items()}
        self.pool = {k: v.to(dtype).clone().requires_grad_(True) for k, v in pool.items()}
        self.cfg, self.dtype = cfg, dtype
        self.last_out, self.out_dim, self.task = 0, 0, 0
        self.head_w = self.head_b = None

    def before_task(self, task, head_w, head_b):
        self.task = task
        self.head_w = torch.as_tensor(head_w).to(self.dtype).clone().requires_grad_(True)
        self.head_b = torch.as_tensor(head_b).to(self.dtype).clone().requires_grad_(True)
        self.out_dim = self.head_w.shape[0]
        self.names = names() + ["classifier.weight", "classifier.bias"]
        self.params = [self.pool[n] for n in names()] + [self.head_w, self.head_b]
        self.m = [torch.zeros_like(p) for p in self.params]           # a fresh Adam per task
        self.v = [torch.zeros_like(p) for p in self.params]
        self.t = 0

    def after_task(self):
        self.last_out = self.out_dim

    def step(self, x, y):
        feat, key_loss, _ = dual_features(self.W, self.pool, x, self.cfg, True, self.task)
        logits = F.linear(feat, self.head_w, self.head_b)
        loss = key_loss + F.cross_entropy(logits[:, self.last_out:], y - self.last_out)      # -inf below last_out_dim == CE over the window
        grads = torch.autograd.grad(loss, self.params, allow_unused=True)
        grads = [torch.zeros_like(p) if g is None else g for p, g in zip(self.params, grads)]
        self.t += 1
        CR.adam_step(self.params, grads, self.m, self.v, self.t, lr=LR, betas=BETAS)
        masked = logits.detach().clone()
        masked[:, :self.last_out] = -math.inf
        return loss.detach(), key_loss.detach(), masked.argmax(1), grads

    def inference(self, x):
        """-> logits, cos [E-layers, B, pool], idx [E-layers, B]"""
        with torch.no_grad():
            feat, _, sel = dual_features(self.W, self.pool, x, self.cfg, False, self.task)
            logits = F.linear(feat, self.head_w, self.head_b)
        return logits, torch.stack([sel[l][0] for l in E_LAYERS]), torch.stack([sel[l][1] for l in E_LAYERS])

    def state(self):
        return {n: p.detach().clone() for n, p in zip(self.names, self.params)}


def is_pooled(name):
    return name.startswith("e_p_") or name.startswith("e_k_")


# ------------------------------------------------------------------------------- the fixture, replayed by the restatement
def replay(fix, dtype):
    """tests/dual_ref.py on the fixture's inputs -> {key: tensor} in the fixture's layout: `t{t}/s{s}/<name>` is the tensor after the step (of a pooled
    tensor row t, the only one that trains), `t{t}/s{s}/moved/<name>` [pool] marks the rows that differ from their value at the start of the task"""
    W = ov.det_params(CFG, str(fix["w_tag"]))
    pool = {k[6:]: torch.as_tensor(v) for k, v in fix.items() if k.startswith("pool0/")}
    m = Method(W, pool, dtype=dtype)
    x = torch.as_tensor(fix["x_u8"]).to(dtype) / 255.0
    xi = torch.as_tensor(fix["infer_x_u8"]).to(dtype) / 255.0
    y = torch.as_tensor(fix["y"])
    got = {"losses": [], "key_losses": [], "preds": [], "infer_preds": [], "infer_idx": [], "infer_cos": [], "infer_margin": []}
    for t in range(TASKS):
        m.before_task(t, fix[f"t{t}/init/classifier.weight"], fix[f"t{t}/init/classifier.bias"])
        start = m.state()
        for s in range(STEPS):
            loss, key_loss, pred, _ = m.step(x[t, s], y[t, s])
            got["losses"].append(loss)
            got["key_losses"].append(key_loss)
            got["preds"].append(pred)
            for n, v in m.state().items():
                got[f"t{t}/s{s}/{n}"] = v[t] if is_pooled(n) else v
                if is_pooled(n):
                    got[f"t{t}/s{s}/moved/{n}"] = (v != start[n]).reshape(POOL, -1).any(1)
        m.after_task()
        logits, cos, idx = m.inference(xi)
        top = logits.topk(2, dim=1).values
        got[f"infer_logits/t{t}"] = logits
        got["infer_preds"].append(logits.argmax(1))
        got["infer_idx"].append(idx)
        got["infer_cos"].append(cos)
        got["infer_margin"].append(top[:, 0] - top[:, 1])
    for k, shape in (("losses", (TASKS, STEPS)), ("key_losses", (TASKS, STEPS)), ("preds", (TASKS, STEPS, BATCH))):
        got[k] = torch.stack(got[k]).view(*shape)
    for k in ("infer_preds", "infer_idx", "infer_cos", "infer_margin"):
        got[k] = torch.stack(got[k])
    return got


def gaps(cos):
    """[..., pool] -> the top-two gap of every row"""
    top = torch.as_tensor(cos).topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


def comparable(fix, t):
    """the inference samples of task t whose fp64 logit margin exceeds MARGIN_REL of the task's largest |logit|: an f32 run, held to 5e-3 of max-abs on
    every trained tensor, cannot be asked to order two logits that are closer than that"""
    lg = np.asarray(fix[f"infer_logits/t{t}"], np.float64)
    return np.asarray(fix["infer_margin"][t], np.float64) > MARGIN_REL * np.abs(lg).max()


def deviations(got, fix):
    """(first losses, all losses, key losses, (worst trained tensor relative to its max-abs, its key)) against the fixture"""
    rel = lambda a, b: float((np.asarray(a, np.float64) - np.asarray(b, np.float64)).__abs__().max() / (np.abs(np.asarray(b, np.float64)).max() + 1e-300))
    first = max(rel(got["losses"][t, :1], fix["losses"][t, :1]) for t in range(TASKS))
    worst = max((rel(v, fix[k]), k) for k, v in got.items() if k.startswith("t") and "/moved/" not in k)
    return first, rel(got["losses"], fix["losses"]), rel(got["key_losses"], fix["key_losses"]), worst
