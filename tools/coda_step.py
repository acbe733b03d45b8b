"""Time the CODA-Prompt training step on ViT-B/16 (batch 128, bf16) and its parts, the prefix attention kernels against the plain ones they
extend, and the L2P step on the same box for scale.

    python tools/coda_step.py [--batch 128 --reps 7 --steps 5]

Random weights and images (the step time does not depend on them).  Every figure is the median of --reps event-timed repetitions of --steps steps
(or calls) after an untimed warm-up, all in one process.  Prints one line per part and a JSON summary line.
Parts: plain clhip_attn_fwd / _bwd at N = 197, H = 12; clhip_attn_prefix_fwd / _bwd at (197, 4); of the step: the query forward, the assembly
(clhip_coda_fwd, five layers), the prefixed forward, the backbone backward with the prefix gradients, clhip_coda_bwd and the Adam step.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import libcontinual_amd.model as M  # noqa: E402
from libcontinual_amd import _lib, optim  # noqa: E402
from libcontinual_amd._lib import call  # noqa: E402

DEV = "cuda"


def timed(fn, reps, inner):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return float(np.median(ms))


def attention_kernels(batch, reps, inner, N=197, Lp=4, H=12, D=768):
    st = torch.cuda.current_stream().cuda_stream
    bf = lambda *s: torch.randn(*s, device=DEV).bfloat16()
    qkv, dout, out, dqkv = bf(batch * N, 3 * D), bf(batch * N, D), bf(batch * N, D), bf(batch * N, 3 * D)
    pk, pv = bf(batch * Lp, D), bf(batch * Lp, D)
    lse, dsum = torch.empty(batch * H * N, device=DEV), torch.empty(batch * H * N, device=DEV)
    dpk, dpv = torch.empty(batch * Lp, D, device=DEV), torch.empty(batch * Lp, D, device=DEV)
    p = lambda t: t.data_ptr()
    res = {}
    res["attn_fwd_ms"] = timed(lambda: call("clhip_attn_fwd", p(qkv), p(out), p(lse), batch, N, H, D, _lib.BF16, st), reps, inner)
    res["attn_bwd_ms"] = timed(lambda: call("clhip_attn_bwd", p(qkv), p(out), p(lse), p(dout), p(dqkv), p(dsum), batch, N, H, D, _lib.BF16, st), reps, inner)
    res["prefix_fwd_ms"] = timed(lambda: call("clhip_attn_prefix_fwd", p(qkv), p(pk), p(pv), p(out), p(lse), batch, N, Lp, H, D, _lib.BF16, st), reps, inner)
    res["prefix_bwd_ms"] = timed(lambda: call("clhip_attn_prefix_bwd", p(qkv), p(pk), p(pv), p(out), p(lse), p(dout), p(dqkv), p(dpk), p(dpv), p(dsum), batch, N,
                                              Lp, H, D, _lib.BF16, st), reps, inner)
    return res


def step_fn(m, opt, batch, lo, hi):
    x = torch.rand(batch, 3, 224, 224, device=DEV)
    y = torch.randint(lo, hi, (batch,), device=DEV)
    m.train()

    def step():
        opt.zero_grad()
        _, _, loss = m.observe({"image": x, "label": y})
        if loss.requires_grad:                                   # (L2P runs its backward inside observe)
            loss.backward()
        opt.step()
    return step, x, y


def coda(batch, reps, inner):
    bb = M.vit_pt_imnet(pretrained=False, dtype="bf16").to(DEV)
    m = M.CodaPrompt(bb, DEV, num_class=100, task_num=10, init_cls_num=10, inc_cls_num=10, feat_dim=768, prompt_length=8, pool_size=100, mu=0.0).to(DEV)
    m.before_task(0, None, None, None)
    opt = optim.Adam(m.get_parameters(None), lr=1e-3, betas=(0.9, 0.999), weight_decay=0)
    step, x, y = step_fn(m, opt, batch, 0, 10)
    res = {"step_ms": timed(step, reps, inner)}
    vt, pool = bb.feat, bb.prompt
    s, st = vt._s, torch.cuda.current_stream().cuda_stream
    params = pool.layer_tensors()
    n, D, L, f = 5, 768, 8, pool.window()[1]
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    with torch.no_grad():
        res["query_forward_ms"] = timed(lambda: vt._run_forward(x, None, 0, None), reps, inner)
        q = vt._run_forward(x, None, 0, None)
        e = torch.empty(2, n, batch, L // 2, D, device=DEV, dtype=torch.bfloat16)
        c = torch.empty(n, batch, f, device=DEV)
        asm = lambda: call("clhip_coda_fwd", n, q.data_ptr(), arr(params[0::3]), arr(params[1::3]), arr(params[2::3]), arr(e[0].unbind(0)), arr(e[1].unbind(0)),
                           c.data_ptr(), batch, D, 100, L, f, _lib.BF16, st)
        res["assembly_ms"] = timed(asm, reps, inner)
        lp = [4] * 5 + [0] * 7
        pk, pv = [e[0, i] if i < 5 else None for i in range(12)], [e[1, i] if i < 5 else None for i in range(12)]
        res["prefixed_forward_ms"] = timed(lambda: vt._run_forward(x, None, 1, None, prefix=(lp, pk, pv)), reps, inner)
        dfeat = torch.randn(batch, D, device=DEV)
        res["backward_ms"] = timed(lambda: vt._run_backward(dfeat, prefix_lp=lp), reps, inner)
        g = vt._run_backward(dfeat, prefix_lp=lp)
        dpk, dpv = g["dpk"], g["dpv"]
        grads = [torch.zeros_like(t) for t in params]
        ws = torch.empty(_lib.lib().clhip_coda_ws_bytes(n, batch, 0, f) // 4, device=DEV)
        bwd = lambda: call("clhip_coda_bwd", n, q.data_ptr(), arr(params[0::3]), arr(params[1::3]), arr(params[2::3]), c.data_ptr(), arr(dpk[:5]), arr(dpv[:5]),
                           arr(grads[0::3]), arr(grads[1::3]), arr(grads[2::3]), ws.data_ptr(), batch, D, 100, L, 0, f, st)
        res["coda_bwd_ms"] = timed(bwd, reps, inner)
    step()                                                       # leave gradients behind for the optimizer alone
    res["adam_ms"] = timed(opt.step, reps, inner)
    return res


def l2p(batch, reps, inner):
    bb = M.vit_pt_imnet(pretrained=False, dtype="bf16").to(DEV)
    m = M.L2P(bb, DEV, init_cls_num=10, inc_cls_num=10, num_class=100, task_num=10, feat_dim=768, prompt_length=5, pool_size=10, top_k=5,
              pull_constraint_coeff=1.0)
    m.before_task(0, None, None, None)
    opt = optim.Adam(m.get_parameters(None), lr=1e-3, betas=(0.9, 0.999), weight_decay=0)
    return timed(step_fn(m, opt, batch, 0, 10)[0], reps, inner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    out = dict(batch=a.batch, dtype="bf16", device=torch.cuda.get_device_name(0), reps=a.reps, steps=a.steps)
    out["kernels"] = attention_kernels(a.batch, a.reps, 4 * a.steps)
    k = out["kernels"]
    print(f"attention b{a.batch} N=197 H=12: plain fwd {k['attn_fwd_ms']:.3f} ms bwd {k['attn_bwd_ms']:.3f} ms; prefix (197,4) fwd {k['prefix_fwd_ms']:.3f} ms "
          f"bwd {k['prefix_bwd_ms']:.3f} ms", flush=True)
    out["l2p_step_ms"] = l2p(a.batch, a.reps, a.steps)
    print(f"L2P step b{a.batch}: {out['l2p_step_ms']:.2f} ms", flush=True)
    torch.cuda.empty_cache()
    out["coda"] = coda(a.batch, a.reps, a.steps)
    print(f"CODA-Prompt step b{a.batch}: " + ", ".join(f"{k_[:-3]} {v:.3f} ms" for k_, v in out["coda"].items()), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
