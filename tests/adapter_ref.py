"""fp64 restatement of the AdaptFormer branch (petl/vision_transformer_adapter.py:31-90, :165-183) and of a tiny adapter ViT, for the adapter tests.

    h = relu(x Wd^T + bd),  hd = h * mask / (1 - p),  x_out = x_mid + mlp(LN2(x_mid)) + s (hd Wu^T + bu)

The dropout mask is an INPUT (bytes of clhip_adapter_dropout_mask, or ones).  Forward and backward of the branch are written out by hand (`fwd`, `bwd`)
and checked against torch autograd of the same formula (`autograd`) on the CPU; `_Branch` plugs the hand-written pair into the tiny ViT, whose other
layers are oracle/vit.py's.  `q` rounds a tensor where csrc/adapter.hip stores or loads the compute dtype (identity for the fp32 mode).
"""
import math

import torch
import torch.nn.functional as F

from oracle import vit as OV

TINY = dict(img=32, patch=8, dim=64, depth=2, heads=2, mlp=256, block_eps=1e-6)      # 17 tokens; batch 3 -> M = 51
R_TINY, SCALE = 16, 0.1


def ident(t):
    return t


def bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def adapter_params(D, R, seed, zero_up=False, dtype=torch.float64):
    """down_proj as kaiming_uniform(a = sqrt 5) draws it (bound 1 / sqrt D); the rest random (a trained adapter) or, with zero_up, the initial zeros"""
    g = gen(seed)
    u = lambda *s, b: ((torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * b).to(dtype)
    Wd, bd = u(R, D, b=1 / math.sqrt(D)), u(R, b=0.2)
    Wu, bu = u(D, R, b=1 / math.sqrt(R)), u(D, b=0.2)
    if zero_up:
        bd, Wu, bu = torch.zeros_like(bd), torch.zeros_like(Wu), torch.zeros_like(bu)
    return Wd, bd, Wu, bu


def fwd(x, Wd, bd, Wu, bu, s, mask=None, p=0.0, q=ident):
    """-> (delta [M, D] = s (hd Wu^T + bu), hd [M, R]); with q = bf16: weights rounded on load, hd rounded where it is stored"""
    h = torch.relu(x @ q(Wd).T + bd)
    hd = h if mask is None or p == 0.0 else h * mask.to(h.dtype) / (1.0 - p)
    hd = q(hd)
    return s * (hd @ q(Wu).T + bu), hd


def bwd(gy, x, hd, Wd, Wu, s, p=0.0, q=ident):
    """gy = dL/dx_out -> (dx = dh Wd, dWd, dbd, dWu, dbu, dh).  hd > 0 <=> relu passed and the element was kept"""
    keep = 1.0 if p == 0.0 else 1.0 / (1.0 - p)
    dh = q(((s * gy) @ q(Wu)) * (hd > 0).to(gy.dtype) * keep)
    return dh @ q(Wd), dh.T @ x, dh.sum(0), s * gy.T @ hd, s * gy.sum(0), dh


# ---- the error bounds of csrc/adapter.hip (tests/test_adapter_kernels_gpu.py states the rule; tests/vit_plan_ref.py applies the same numbers inside the executor)
U, V16 = 2.0 ** -24, 2.0 ** -8


def fwd_bounds(x, y0, Wd, bd, Wu, bu, s, hd64, delta, y64, p, v, q):
    """(e_hd, e_y): x, y0 = the value y held before the += (fp64), hd64 / delta from `fwd`, y64 = q(y0 + delta); v = V16 in the bf16 mode, else 0"""
    keep = 1.0 / (1.0 - p) if p > 0 else 1.0
    D, R = x.shape[1], Wd.shape[0]
    pre_abs = x.abs() @ q(Wd).abs().T
    e_hd = keep * (D * U * pre_abs + 2 * U * (pre_abs + bd.abs())) + 2 * v * hd64.abs()
    e_y = s * (R * U * (hd64.abs() @ q(Wu).abs().T) + e_hd @ q(Wu).abs().T) + 4 * U * (y0.abs() + delta.abs() + s * bu.abs()) + 2 * v * y64.abs()
    return e_hd, e_y


def bwd_bounds(gy, hd64, Wd, Wu, s, dh64, dx64, gx64, p, v, q):
    """(e_dh, e_gx) of clhip_adapter_bwd"""
    keep = 1.0 / (1.0 - p) if p > 0 else 1.0
    D, R = gy.shape[1], Wd.shape[0]
    t_abs = gy.abs() @ q(Wu).abs()
    e_dh = (hd64 > 0) * s * keep * (D + 3) * U * t_abs + 2 * v * dh64.abs()
    e_gx = R * U * (dh64.abs() @ q(Wd).abs()) + e_dh @ q(Wd).abs() + 2 * U * (gy.abs() + dx64.abs()) + 2 * v * gx64.abs()
    return e_dh, e_gx


def wgrad_bounds(gy, hd64, x, dh64, s):
    """bounds of (dWd, dbd, dWu, dbu) of clhip_adapter_wgrad: fp32 accumulation over the M rows of stored tensors, nothing else"""
    MU = (gy.shape[0] + 2) * U
    return MU * (dh64.abs().T @ x.abs()), MU * dh64.abs().sum(0), s * MU * (gy.abs().T @ hd64.abs()), s * MU * gy.abs().sum(0)


def autograd(gy, x, Wd, bd, Wu, bu, s, mask=None, p=0.0):
    """the same gradients from torch autograd of the plain formula (no rounding)"""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, Wd, bd, Wu, bu)]
    xx, a, b, c, d = leaves
    h = torch.relu(xx @ a.T + b)
    if mask is not None and p > 0.0:
        h = h * mask.to(h.dtype) / (1.0 - p)
    out = s * (h @ c.T + d)
    out.backward(gy)
    return out.detach(), [t.grad for t in leaves]


class _Branch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Wd, bd, Wu, bu, s, mask, p):
        delta, hd = fwd(x, Wd, bd, Wu, bu, s, mask, p)
        ctx.save_for_backward(x, hd, Wd, Wu)
        ctx.s, ctx.p = s, p
        return delta

    @staticmethod
    def backward(ctx, gy):
        x, hd, Wd, Wu = ctx.saved_tensors
        dx, dWd, dbd, dWu, dbu, _ = bwd(gy, x, hd, Wd, Wu, ctx.s, ctx.p)
        return dx, dWd, dbd, dWu, dbu, None, None, None


def vit_features(P, A, img, cfg=TINY, s=SCALE, masks=None, p=0.0, prompt=None, hand=True):
    """cls (or prompt-mean) features of the adapter ViT.  P: oracle/vit.py parameter dict, A: [(Wd, bd, Wu, bu)] per layer or None, masks: [M, R] bytes
    per layer or None.  hand = False takes the branch through plain autograd instead of the hand-written backward."""
    x = OV.tokens(P, img, cfg)
    if prompt is not None:
        x = torch.cat((prompt.unsqueeze(0).expand(x.shape[0], -1, -1), x), dim=1)
    D = x.shape[-1]
    x = blocks(P, A, x, cfg, s, masks, p, hand)[-1]
    x = F.layer_norm(x, (D,), P["feat.norm.weight"], P["feat.norm.bias"], 1e-6)
    return x[:, 0] if prompt is None else x[:, :prompt.shape[0]].mean(1)


def blocks(P, A, x, cfg=TINY, s=SCALE, masks=None, p=0.0, hand=True):
    """the outputs of every block on tokens x [B, N, D] (vision_transformer_adapter.py:165-183, ffn_option "parallel")"""
    B, N, D = x.shape
    outs = []
    for i in range(cfg["depth"]):
        b = f"feat.transformer.blocks.{i}."
        eps = cfg.get("block_eps", 1e-5)
        x = x + OV.attention(P, b, F.layer_norm(x, (D,), P[b + "ln_1.weight"], P[b + "ln_1.bias"], eps), cfg["heads"])
        h = F.layer_norm(x, (D,), P[b + "ln_2.weight"], P[b + "ln_2.bias"], eps)
        h = F.linear(F.gelu(F.linear(h, P[b + "mlp.fc1.weight"], P[b + "mlp.fc1.bias"])), P[b + "mlp.fc2.weight"], P[b + "mlp.fc2.bias"])
        out = x + h
        if A is not None:
            m = None if masks is None else masks[i].reshape(B * N, -1)
            flat = x.reshape(B * N, D)
            if hand:
                delta = _Branch.apply(flat, *A[i], s, m, p)
            else:
                hh = torch.relu(flat @ A[i][0].T + A[i][1])
                if m is not None and p > 0.0:
                    hh = hh * m.to(hh.dtype) / (1.0 - p)
                delta = s * (hh @ A[i][2].T + A[i][3])
            out = out + delta.reshape(B, N, D)
        x = out
        outs.append(x)
    return outs


def cosine_logits(f, W, sigma):
    return sigma * (F.normalize(f, dim=1) @ F.normalize(W, dim=1).T)


class SGD:
    """torch.optim.SGD's update (weight decay into the gradient, momentum buffer seeded with the first gradient), on fp64 leaves"""

    def __init__(self, params, lr, momentum, weight_decay):
        self.params, self.lr, self.mu, self.wd = params, lr, momentum, weight_decay
        self.buf = [None] * len(params)

    def step(self):
        with torch.no_grad():
            for i, p in enumerate(self.params):
                if p.grad is None:
                    continue
                g = p.grad + self.wd * p
                self.buf[i] = g.clone() if self.buf[i] is None else self.mu * self.buf[i] + g
                p -= self.lr * self.buf[i]
                p.grad = None
