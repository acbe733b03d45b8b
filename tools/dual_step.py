"""Time the DualPrompt training step on ViT-B/16 (batch 128, bf16) and its parts, with the CODA-Prompt step on the same box for scale.

    python tools/dual_step.py [--batch 128 --reps 7 --steps 5]

Random weights and images (the step time does not depend on them).  Every figure is the median of --reps event-timed repetitions of --steps steps
(or calls) after an untimed warm-up, all in one process.  Prints one line per method and a JSON summary line.
Parts of the step: the query forward, the selection (clhip_dual_fwd in train mode: two G-layers at Lg = 6, three E-layers at pool 10, Le = 20, and the
key loss -- one launch; the eval mode, with its arg-max, is timed next to it), the prefixed forward with Lp = [3, 3, 10, 10, 10, 0, ...], the backbone
backward with the prefix gradients, clhip_dual_bwd (one launch) and the Adam step.
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


def step_fn(m, opt, batch, lo, hi):
    x = torch.rand(batch, 3, 224, 224, device=DEV)
    y = torch.randint(lo, hi, (batch,), device=DEV)
    m.train()

    def step():
        opt.zero_grad()
        _, _, loss = m.observe({"image": x, "label": y})
        loss.backward()
        opt.step()
    return step, x, y


def dual(batch, reps, inner, task_id=3):
    bb = M.vit_pt_imnet(pretrained=False, dtype="bf16").to(DEV)
    m = M.DualPrompt(bb, DEV, num_class=100, task_num=10, init_cls_num=10, inc_cls_num=10, feat_dim=768, g_prompt_length=6, e_prompt_length=20).to(DEV)
    m.before_task(task_id, None, None, None)
    opt = optim.Adam(m.get_parameters(None), lr=1e-3, betas=(0.9, 0.999), weight_decay=0)
    step, x, y = step_fn(m, opt, batch, 10 * task_id, 10 * task_id + 10)
    res = {"step_ms": timed(step, reps, inner)}
    vt, pool = bb.feat, bb.prompt
    st = torch.cuda.current_stream().cuda_stream
    params = pool.layer_tensors()
    ng, ne, D, Lg, Le, size = 2, 3, 768, pool.g_p_length, pool.e_p_length, pool.e_pool_size
    g_p, e_k, e_p = params[:ng], params[ng::2], params[ng + 1::2]
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    with torch.no_grad():
        res["query_forward_ms"] = timed(lambda: vt._run_forward(x, None, 0, None), reps, inner)
        q = vt._run_forward(x, None, 0, None)
        pre = [torch.empty(2, batch, L // 2, D, device=DEV, dtype=torch.bfloat16) for L in [Lg] * ng + [Le] * ne]
        cos, idx = torch.empty(ne, batch, size, device=DEV), torch.empty(ne, batch, device=DEV, dtype=torch.int32)
        loss = torch.zeros(1, device=DEV)
        sel = lambda train: call("clhip_dual_fwd", ng, ne, q.data_ptr(), arr(g_p), arr(e_k), arr(e_p), arr([p[0] for p in pre]), arr([p[1] for p in pre]),
                                 cos.data_ptr(), idx.data_ptr(), loss.data_ptr(), batch, D, size, Lg, Le, train, task_id, _lib.BF16, st)
        res["select_eval_ms"] = timed(lambda: sel(0), reps, 4 * inner)
        res["select_train_ms"] = timed(lambda: sel(1), reps, 4 * inner)
        lp = [Lg // 2] * ng + [Le // 2] * ne + [0] * (12 - ng - ne)
        pk = [pre[i][0] if i < ng + ne else None for i in range(12)]
        pv = [pre[i][1] if i < ng + ne else None for i in range(12)]
        res["prefixed_forward_ms"] = timed(lambda: vt._run_forward(x, None, 1, None, prefix=(lp, pk, pv)), reps, inner)
        dfeat = torch.randn(batch, D, device=DEV)
        res["backward_ms"] = timed(lambda: vt._run_backward(dfeat, prefix_lp=lp), reps, inner)
        g = vt._run_backward(dfeat, prefix_lp=lp)
        dpk, dpv = g["dpk"], g["dpv"]
        grads = [torch.zeros_like(t) for t in params]
        one = torch.ones(1, device=DEV)
        bwd = lambda: call("clhip_dual_bwd", ng, ne, q.data_ptr(), arr(e_k), arr(dpk[:ng + ne]), arr(dpv[:ng + ne]), one.data_ptr(), arr(grads[:ng]),
                           arr(grads[ng::2]), arr(grads[ng + 1::2]), batch, D, size, Lg, Le, task_id, st)
        res["dual_bwd_ms"] = timed(bwd, reps, 4 * inner)
    step()                                                       # leave gradients behind for the optimizer alone
    res["adam_ms"] = timed(opt.step, reps, inner)
    return res


def coda(batch, reps, inner):
    bb = M.vit_pt_imnet(pretrained=False, dtype="bf16").to(DEV)
    m = M.CodaPrompt(bb, DEV, num_class=100, task_num=10, init_cls_num=10, inc_cls_num=10, feat_dim=768, prompt_length=8, pool_size=100, mu=0.0).to(DEV)
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
    out["coda_step_ms"] = coda(a.batch, a.reps, a.steps)
    print(f"CODA-Prompt step b{a.batch}: {out['coda_step_ms']:.2f} ms", flush=True)
    torch.cuda.empty_cache()
    out["dual"] = dual(a.batch, a.reps, a.steps)
    print(f"DualPrompt step b{a.batch}: " + ", ".join(f"{k_[:-3]} {v:.3f} ms" for k_, v in out["dual"].items()), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
