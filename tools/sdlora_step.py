"""Time the SD_LoRA training step on ViT-B/16 (batch 128, bf16) at task 0 (one term) and at task 9 (ten terms), the per-step refresh of the effective
qkv copies and the 12 per-layer gradient calls on their own, and the InfLoRA_OPT step on the same box as the yardstick.

    python tools/sdlora_step.py [--batch 128 --reps 7 --steps 5]

Random weights and images (the step time does not depend on them).  Every figure is the median of --reps event-timed repetitions of --steps steps
(or calls) after an untimed warm-up.  Prints one line per part and a JSON summary line.
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


def sd_model(tasks):
    bb = M.vit_pt_imnet(pretrained=False, attn_layer="MultiHeadAttention_SDLoRA", lora_rank=10, dtype="bf16").to(DEV)
    m = M.SD_LoRA(bb, DEV, init_cls_num=10, inc_cls_num=10, task_num=10, embd_dim=768, init_mag=1.0, rank_reduction=[False, 4, 8, 8, 6],
                  knowledge_dist=[False, 9e-4])
    for t in range(tasks):
        m.before_task(t, None, None, None)
        with torch.no_grad():                                    # finished tasks leave non-zero B behind
            for a in m.attention_modules:
                a.lora_B_q_list[t].weight.uniform_(-0.02, 0.02)
                a.lora_B_v_list[t].weight.uniform_(-0.02, 0.02)
        if t < tasks - 1:
            m.after_task(t, None, None, None)
    m._network.backbone.feat.sdlora_update_inv()
    return m


def step_fn(m, batch, lo, hi):
    opt = optim.SGD(m.get_parameters(None), lr=8e-3, momentum=0.9)
    x = torch.rand(batch, 3, 224, 224, device=DEV)
    y = torch.randint(lo, hi, (batch,), device=DEV)
    m.train()

    def step():
        _, _, loss = m.observe({"image": x, "label": y})
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


def parts(m, batch, reps, inner):
    """the refresh and the 12 gradient calls alone, on the executor state the last step left"""
    vt = m._network.backbone.feat
    s, st = vt._s, torch.cuda.current_stream().cuda_stream
    refresh = timed(lambda: call("clhip_vit_sdlora_refresh", s.handle, C.byref(s.cparams), s.shadow.data_ptr(), st), reps, inner)
    D, T1, Mrows = 768, vt.sd_terms(), batch * 197
    ranks = [h.weight.shape[0] for h in vt.attention_modules()[0].lora_A_q_list]
    x = torch.randn(Mrows, D, device=DEV).bfloat16()
    dy = (0.1 * torch.randn(Mrows, 3 * D, device=DEV)).bfloat16()
    r = ranks[-1]
    outs = [torch.empty(s_, device=DEV) for s_ in ((r, D), (D, r), (r, D), (D, r), (T1,))]
    ws = torch.empty(_lib.lib().clhip_sdlora_grad_ws_bytes(Mrows, D, sum(ranks)), dtype=torch.uint8, device=DEV)
    rk = (C.c_int * T1)(*ranks)

    def grads():
        for l in range(vt.depth):
            call("clhip_sdlora_grad", x.data_ptr(), dy.data_ptr(), s.sd_tab[4 * l].data_ptr(), rk, T1, s.sd_mag.data_ptr(), s.sd_inv[l].data_ptr(),
                 *[o.data_ptr() for o in outs], ws.data_ptr(), Mrows, D, _lib.BF16, st)
    return refresh, timed(grads, reps, max(1, inner // 2))


def inflora_step(batch):
    bb = M.vit_pt_imnet(pretrained=False, attn_layer="MultiHeadAttention_LoRA", lora_rank=10, dtype="bf16").to(DEV)
    m = M.InfLoRA_OPT(bb, DEV, init_cls_num=10, inc_cls_num=10, task_num=10, embd_dim=768, lame=1.0, lamb=0.95)
    m._network.update_fc(None)
    for a in m.attention_modules:
        a.init_param()
    for n, p in m._network.named_parameters():
        p.requires_grad_("classifier_pool.0." in n or "lora_B" in n)
    return step_fn(m, batch, 0, 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    out = dict(batch=a.batch, dtype="bf16", device=torch.cuda.get_device_name(0), reps=a.reps, steps=a.steps)
    out["inflora_opt_step_ms"] = timed(inflora_step(a.batch), a.reps, a.steps)
    print(f"InfLoRA_OPT step b{a.batch}: {out['inflora_opt_step_ms']:.2f} ms", flush=True)
    for tasks in (1, 10):
        m = sd_model(tasks)
        t = tasks - 1
        ms = timed(step_fn(m, a.batch, 10 * t, 10 * t + 10), a.reps, a.steps)
        refresh, grads = parts(m, a.batch, a.reps, a.steps)
        out[f"task{t}"] = dict(step_ms=ms, refresh_ms=refresh, grad_12_layers_ms=grads)
        print(f"SD_LoRA task {t} b{a.batch}: step {ms:.2f} ms, refresh {refresh:.3f} ms, 12 gradient calls {grads:.2f} ms", flush=True)
        del m
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
