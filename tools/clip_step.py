"""Time the CLIP path on one GPU and print the table that profiles/clip_step.md quotes:

  * one InfLoRA_OPT training step (observe + backward + Adam) on the `clip` backbone at ViT-B/16 geometry, batch 128, bf16, 20 classes in the task,
    next to the same step on the plain ViT backbone (`vit_pt_imnet`, MultiHeadAttention_LoRA) on the same box;
  * the logits pair (clhip_clip_logits_fwd + _bwd) at B 128, D 768, E 512, C 20 and C 100;
  * fc1 of ViT-B/16 at M = 128 x 197 under epilogue 6 (QuickGELU) and under epilogue 3 (erf GELU).

    python tools/clip_step.py [--steps 30] [--warmup 10] [--out FILE]

The table goes to stdout, and to FILE when --out names one.  profiles/clip_step.md holds it together with its reading and the bench.py A/B, which are
written by hand: the tool refuses to write over that file.

Random weights (no checkpoint is needed for a timing); device events around each repetition, the median is reported with the spread.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libcontinual_amd.model as M  # noqa: E402
from libcontinual_amd import _lib, optim  # noqa: E402

DEV = "cuda"


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def step_of(model, batch, classes):
    x = torch.rand(batch, 3, 224, 224, device=DEV)
    y = torch.randint(0, classes, (batch,), device=DEV)
    loader = [{"image": x, "label": y}]
    model.before_task(0, None, loader, None)
    opt = optim.Adam([p for p in model.get_parameters(None) if p.requires_grad], lr=5e-4, betas=(0.9, 0.999), weight_decay=0)
    model.train()

    def step():
        _, _, loss = model.observe({"image": x, "label": y})
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=None, help="also write the table to this file (not profiles/clip_step.md: its analysis is hand-written)")
    a = ap.parse_args()
    if a.out and os.path.realpath(a.out) == os.path.realpath(os.path.join(ROOT, "profiles", "clip_step.md")):
        ap.error("--out would replace profiles/clip_step.md and the analysis in it; name another file and paste the table")
    torch.manual_seed(0)
    rows = []
    common = dict(init_cls_num=20, inc_cls_num=20, task_num=5, lame=1.0, lamb=0.95, dataset="cifar100", use_ca=False, embd_dim=768)
    tokens = torch.zeros(100, 77, dtype=torch.int64)
    tokens[:, 0], tokens[:, 1:6], tokens[:, 6] = 49406, torch.randint(1000, 40000, (100, 5)), 49407
    clip = M.clip("ViT-B/16", DEV, pretrained=False, attn_layer="MultiHeadAttention_LoRA", lora_rank=10, act_layer="QuickGELU", norm_layer="LayerNorm", dtype="bf16")
    m = M.InfLoRA_OPT(clip, DEV, prompt_template="a bad photo of a {}.", visual_only=True, class_tokens=tokens, **common)
    rows.append(("InfLoRA_OPT step, `clip` ViT-B/16, batch %d, bf16" % a.batch,) + timed(step_of(m, a.batch, 20), a.steps, a.warmup))
    del m, clip
    torch.cuda.empty_cache()
    vit = M.vit_pt_imnet(pretrained=False, attn_layer="MultiHeadAttention_LoRA", lora_rank=10, dtype="bf16").to(DEV)
    m = M.InfLoRA_OPT(vit, DEV, **common)
    rows.append(("InfLoRA_OPT step, `vit_pt_imnet` ViT-B/16, batch %d, bf16" % a.batch,) + timed(step_of(m, a.batch, 20), a.steps, a.warmup))
    del m, vit
    torch.cuda.empty_cache()
    st = torch.cuda.current_stream().cuda_stream
    B, D, E = a.batch, 768, 512
    feat, proj = torch.randn(B, D, device=DEV), torch.randn(D, E, device=DEV) * D ** -0.5
    u, inv, df = torch.empty(B, E, device=DEV), torch.empty(B, device=DEV), torch.empty(B, D, device=DEV)
    for Cn in (20, 100):
        txt = torch.nn.functional.normalize(torch.randn(Cn, E, device=DEV), dim=1)
        out, dl = torch.empty(B, Cn, device=DEV), torch.randn(B, Cn, device=DEV)

        def pair():
            _lib.call("clhip_clip_logits_fwd", feat.data_ptr(), proj.data_ptr(), txt.data_ptr(), 14.3, out.data_ptr(), u.data_ptr(), inv.data_ptr(), B, D, E, Cn, st)
            _lib.call("clhip_clip_logits_bwd", dl.data_ptr(), proj.data_ptr(), txt.data_ptr(), 14.3, u.data_ptr(), inv.data_ptr(), df.data_ptr(), B, D, E, Cn, st)
        rows.append((f"logits pair (fwd + bwd), B {B}, D 768, E 512, C {Cn}",) + timed(pair, a.steps * 4, a.warmup))
    Mr, N, K = a.batch * 197, 3072, 768
    A = torch.randn(Mr, K, device=DEV).bfloat16()
    W = (torch.randn(N, K, device=DEV) * K ** -0.5).bfloat16()
    bias = torch.zeros(N, device=DEV)
    Cc, H = torch.empty(Mr, N, device=DEV, dtype=torch.bfloat16), torch.empty(Mr, N, device=DEV, dtype=torch.bfloat16)
    for epi, name in ((6, "QuickGELU, epilogue 6"), (3, "erf GELU, epilogue 3")):
        def fc1(epi=epi):
            _lib.call("clhip_gemm_nt", A.data_ptr(), W.data_ptr(), Cc.data_ptr(), bias.data_ptr(), None, H.data_ptr(), Mr, N, K, K, K, N, 0, N, epi, _lib.BF16, st)
        rows.append((f"fc1 [{Mr} x 3072 x 768] bf16, {name}, with H",) + timed(fc1, a.steps * 4, a.warmup))
    lines = ["| what | median ms | min | max |", "|---|---|---|---|"] + [f"| {n} | {med:.3f} | {lo:.3f} | {hi:.3f} |" for n, med, lo, hi in rows]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
