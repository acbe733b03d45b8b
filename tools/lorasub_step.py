"""Time the LoRAsub_DRS training step on ViT-B/16 (batch 128, bf16) at task 0 (plain Adam, no prototypes) and at task 1 (projected Adam, 10 prototypes), its
three new launches on their own -- clhip_atl at P = 90 (the last CIFAR-100 task), clhip_proj_adam_multi over the 48 factors, the per-step refresh -- a
torch-on-device restatement of the reference lines the two kernels replace (lora_sub.py:34-68, :120-157), and the SD_LoRA and InfLoRA_OPT steps of the same
box (tools/sdlora_step.py) as yardsticks.

    python tools/lorasub_step.py [--batch 128 --reps 7 --steps 5]

Random weights and images (the step time does not depend on them).  Every figure is the median of --reps event-timed repetitions of --steps steps (200
back-to-back calls for a single launch) after an untimed warm-up.  Prints one line per part and a JSON summary line.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import libcontinual_amd.model as M  # noqa: E402
from libcontinual_amd import ops  # noqa: E402
from libcontinual_amd._lib import call  # noqa: E402
from sdlora_step import inflora_step, sd_model, step_fn, timed  # noqa: E402

DEV = "cuda"
D, RANK, DEPTH = 768, 10, 12


def lorasub_model(tasks, batch):
    """the method after `tasks` before_task calls; a finished task leaves prev != 0 and 10 prototypes, and its Gram pass sees one random batch"""
    bb = M.vit_pt_imnet(pretrained=False, attn_layer="MultiHeadAttention_LoRA_Sub", lora_rank=RANK, dtype="bf16").to(DEV)
    m = M.LoRAsub_DRS(bb, DEV, init_cls_num=10, inc_cls_num=10, task_num=10, embd_dim=D, fc_lrate=2e-3, margin_inter=1.0, lambada=0.05)
    for t in range(tasks):
        loader = [{"image": torch.rand(batch, 3, 224, 224, device=DEV), "label": torch.arange(batch, device=DEV) % 10 + 10 * t}]
        m.before_task(t, None, loader, None)
        with torch.no_grad():
            for a in m.attention_modules:
                a.lora_B_k.weight.uniform_(-0.02, 0.02)
                a.lora_B_v.weight.uniform_(-0.02, 0.02)
        if t < tasks - 1:
            m.after_task(t, None, loader, None)
    return m


def lorasub_step_fn(m, batch, lo, hi):
    opt = m.get_optimizer(5e-4, 0.0)
    x = torch.rand(batch, 3, 224, 224, device=DEV)
    y = torch.randint(lo, hi, (batch,), device=DEV)
    m.train()

    def step():
        _, _, loss = m.observe({"image": x, "label": y})
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


def torch_atl(f, y, protos, margin):
    """the reference's forward as it is written (a loop over the batch, a loop over batch x prototypes of small device calls) and its autograd backward"""
    f = f.clone().requires_grad_(True)
    x = f / f.norm(dim=-1, keepdim=True)
    n = x.size(0)
    sq = x.pow(2).sum(1, keepdim=True).expand(n, n)
    dist = (sq + sq.t() - 2 * x @ x.t()).clamp(min=1e-12).sqrt()
    mask = y.expand(n, n).eq(y.expand(n, n).t())
    ap, an = [], []
    for i in range(n):
        ap.append(dist[i][mask[i]].max().unsqueeze(0))
        neg = dist[i][mask[i] == 0]
        an.append((ap[-1] + margin) if neg.numel() == 0 else neg.min().unsqueeze(0))
    c = protos / protos.norm(dim=1, keepdim=True)
    for i in range(n):
        for j in range(c.size(0)):
            an[i] = torch.minimum(an[i], torch.norm(x[i] - c[j], 2).clamp(min=1e-12).unsqueeze(0))
    loss = torch.relu(torch.cat(ap) - torch.cat(an) + margin).mean()
    loss.backward()
    return loss.detach(), f.grad


def torch_proj_adam(rows, T, lr, step):
    """lora_sub.py:193-233 and :143-156 per tensor: the moments, the update, one torch.mm with the layer's transform, the add"""
    b1, b2, eps = 0.9, 0.999, 1e-8
    for t, (p, g, m, v) in enumerate(rows):
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = v.sqrt().add_(eps)
        upd = -(lr * (1 - b2 ** step) ** 0.5 / (1 - b1 ** step)) * m / denom
        Tl = T[t // 4]
        p.add_(torch.mm(Tl, upd) if Tl.shape[0] == upd.shape[0] else torch.mm(upd, Tl))


def kernels(m, batch, reps):
    out = {}
    g = torch.Generator(device=DEV).manual_seed(0)
    f = torch.randn(batch, D, device=DEV, generator=g)
    y = torch.arange(batch, device=DEV) % 10
    protos = torch.randn(90, D, device=DEV, generator=g)
    out["atl_p90_ms"] = timed(lambda: ops.atl(f, y, protos, 1.0, 0.05), reps, 200)
    out["atl_p90_torch_loop_ms"] = timed(lambda: torch_atl(f, y, protos, 1.0), 3, 1)
    rows = [[torch.randn(*((RANK, D) if t % 2 == 0 else (D, RANK)), device=DEV, generator=g) * s for s in (0.05, 0.01, 0.01, 0.0)] for t in range(4 * DEPTH)]
    for r in rows:
        r[3].add_(1e-4)
    T = torch.randn(DEPTH, D, D, device=DEV, generator=g) / D
    table = ops.proj_adam_table(rows)
    tt = torch.tensor([t.data_ptr() for t in T], dtype=torch.int64).to(DEV)
    ws = torch.empty(4 * DEPTH * D * RANK, device=DEV)
    out["proj_adam_ms"] = timed(lambda: ops.proj_adam_multi(table, tt, ws, D, RANK, 5e-4, 0.9, 0.999, 1e-8, 0.0, 3), reps, 200)
    out["plain_adam_ms"] = timed(lambda: ops.proj_adam_multi(table, None, None, D, RANK, 5e-4, 0.9, 0.999, 1e-8, 0.0, 3), reps, 200)
    out["proj_adam_torch_ms"] = timed(lambda: torch_proj_adam(rows, T, 5e-4, 3), reps, 20)
    # the bytes the projected step must move: every T once (28.3 MB), and p, g, m, v of the factors read, p, m, v written
    need = DEPTH * D * D * 4 + 4 * DEPTH * D * RANK * 4 * 7
    out["proj_adam_bytes_needed"] = need
    out["proj_adam_gb_per_s_of_needed"] = need / (out["proj_adam_ms"] * 1e-3) / 1e9
    vt = m._network.backbone.feat
    s, st = vt._s, torch.cuda.current_stream().cuda_stream
    out["refresh_ms"] = timed(lambda: call("clhip_vit_lora_refresh_ab", s.handle, C.byref(s.cparams), s.shadow.data_ptr(), st), reps, 200)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    out = dict(batch=a.batch, dtype="bf16", device=torch.cuda.get_device_name(0), reps=a.reps, steps=a.steps)
    out["inflora_opt_step_ms"] = timed(inflora_step(a.batch), a.reps, a.steps)
    print(f"InfLoRA_OPT step b{a.batch}: {out['inflora_opt_step_ms']:.2f} ms", flush=True)
    sd = sd_model(1)
    out["sd_lora_task0_step_ms"] = timed(step_fn(sd, a.batch, 0, 10), a.reps, a.steps)
    print(f"SD_LoRA task 0 step b{a.batch}: {out['sd_lora_task0_step_ms']:.2f} ms", flush=True)
    del sd
    torch.cuda.empty_cache()
    for tasks in (1, 2):
        m = lorasub_model(tasks, a.batch)
        t = tasks - 1
        out[f"lorasub_task{t}_step_ms"] = timed(lorasub_step_fn(m, a.batch, 10 * t, 10 * t + 10), a.reps, a.steps)
        print(f"LoRAsub_DRS task {t} step b{a.batch}: {out[f'lorasub_task{t}_step_ms']:.2f} ms (basis kept per layer: {m.reserved_basis})", flush=True)
        if tasks == 2:
            out.update(kernels(m, a.batch, a.reps))
        del m
        torch.cuda.empty_cache()
    for k in ("atl_p90_ms", "atl_p90_torch_loop_ms", "proj_adam_ms", "plain_adam_ms", "proj_adam_torch_ms", "proj_adam_gb_per_s_of_needed", "refresh_ms"):
        print(f"{k}: {out[k]:.4f}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
