"""Write tests/golden/sdlora_tiny.npz from fp64 runs of the REFERENCE's own `MultiHeadAttention_SDLoRA` (core/model/backbone/transformer.py:276-357) and
`SD_LoRA` (core/model/sd_lora.py), imported through oracle.ref_shim with its stand-ins for timm.

    python tools/gen_sdlora_golden.py          (needs the reference tree; the fixture is committed)

Attention-module part (keys `a/...`): D 64, 2 heads, 4 terms of ranks 10, 10, 8, 6, every B non-zero except B^v of past term 1 (= 0: the reference skips
that term), distinct magnitudes.  Stored: the weights, the input [3, 17, 64], a random cotangent, the output and the gradients of every trainable tensor
(A and B of the last term for q and v, the four magnitudes).
Method part (keys `m/...`): a 2-block ViT (img 32, patch 8, D 64, 2 heads, mlp 256), lora_rank 4, 2 tasks of 3 classes x 3 SGD steps (lr 0.05, momentum 0.9,
a fresh optimizer per task as the reference's trainer builds it), batch 6.  Stored: the backbone weights (created in fp32 and kept as fp32; every fresh tensor is fp32-representable), what
`before_task` initialised at random (head, the new term's factors), images (as bytes, / 255) and labels, the losses and predictions, and after every step the head, the
current term's factors and the magnitudes; the names `before_task` left trainable.  tests/test_sdlora_cpu.py holds tests/sdlora_ref.py to it (1e-10).
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

D, HEADS, RANKS, B, N = 64, 2, (10, 10, 8, 6), 3, 17
CFG = dict(img=32, patch=8, dim=64, depth=2, heads=2, mlp=256)
TASKS, STEPS, BATCH, INC, RANK, LR, MOM, INIT_MAG = 2, 3, 6, 3, 4, 0.05, 0.9, 1.0
LISTS = ("lora_A_q_list", "lora_B_q_list", "lora_A_v_list", "lora_B_v_list")


def attention_part(tr, out):
    torch.manual_seed(4321)
    m = tr.MultiHeadAttention_SDLoRA(D, HEADS, lora_rank=RANKS[0])
    for i, r in enumerate(RANKS):
        m.lora_rank = r
        m.mag_lora = nn.ParameterList([nn.Parameter(torch.Tensor([1.0])) for _ in range(i + 1)])
        m.init_param()
    m.double()
    with torch.no_grad():
        for n in LISTS:
            for lin in getattr(m, n):
                lin.weight.uniform_(-0.3, 0.3)
        m.lora_B_v_list[1].weight.zero_()
        for i, p in enumerate(m.mag_lora):
            p.fill_(0.6 + 0.35 * i)
        m.qkv.bias.uniform_(-0.1, 0.1)
        m.proj.bias.uniform_(-0.1, 0.1)
    for p in m.parameters():
        p.requires_grad_(False)
    train = [getattr(m, n)[-1].weight for n in LISTS] + list(m.mag_lora)
    for p in train:
        p.requires_grad_(True)
    x = torch.randn(B, N, D, dtype=torch.float64)
    gy = torch.randn(B, N, D, dtype=torch.float64)
    y = m(x)
    (y * gy).sum().backward()
    out["a/x"], out["a/gy"], out["a/y"] = x, gy, y
    for k, v in m.state_dict().items():
        out["a/w/" + k] = v
    for n in LISTS:
        out[f"a/grad/{n}"] = getattr(m, n)[-1].weight.grad
    out["a/grad/mag"] = torch.cat([p.grad for p in m.mag_lora])


def method_part(tr, vit, sd, out):
    torch.manual_seed(99)
    zoo = vit.ViTZoo.__new__(vit.ViTZoo)
    nn.Module.__init__(zoo)
    zoo.task_id, zoo.feat_dim = None, CFG["dim"]
    zoo.feat = tr.VisionTransformer(img_size=CFG["img"], patch_size=CFG["patch"], embed_dim=CFG["dim"], depth=CFG["depth"], num_heads=CFG["heads"],
                                    ckpt_layer=0, drop_path_rate=0, attn_layer="MultiHeadAttention_SDLoRA", lora_rank=RANK)
    zoo.prompt, zoo.prompt_flag = None, ""
    with torch.no_grad():                                  # a trained-network-like scale, so that the branch matters
        for n, p in zoo.named_parameters():
            if n.endswith("bias"):
                p.uniform_(-0.05, 0.05)
            elif "ln_" in n or ".norm." in n:
                p.uniform_(0.8, 1.2)
            elif p.dim() >= 2 and "pos_embed" not in n and "cls_token" not in n:
                s = 1.7 / np.sqrt(p[0].numel())
                p.uniform_(-s, s)
    model = sd.SD_LoRA(zoo, "cpu", init_cls_num=INC, inc_cls_num=INC, task_num=TASKS, init_mag=INIT_MAG, rank_reduction=[False, 4, 8, 8, 6],
                       knowledge_dist=[False, 9e-4], embd_dim=CFG["dim"])
    for k, v in zoo.state_dict().items():
        out["m/w/" + k] = v.float()
    x8 = torch.randint(0, 256, (TASKS, STEPS, BATCH, 3, CFG["img"], CFG["img"]), dtype=torch.uint8)
    x = x8.double() / 255.0
    y = torch.stack([torch.randint(t * INC, (t + 1) * INC, (STEPS, BATCH)) for t in range(TASKS)])
    out["m/x_u8"], out["m/y"] = x8, y            # images = x_u8 / 255
    losses, preds = [], []
    for t in range(TASKS):
        model.before_task(t, None, None, None)
        with torch.no_grad():
            for a in model.attention_modules:              # a non-zero B of the new term, so that its A has a gradient from the first step on
                a.lora_B_q_list[t].weight.uniform_(-0.05, 0.05)
                a.lora_B_v_list[t].weight.uniform_(-0.05, 0.05)
        model._network.double()
        named = dict(model._network.named_parameters())
        train = sorted(n for n, p in named.items() if p.requires_grad)
        out[f"m/t{t}/trainable"] = np.array(train)
        for n in train:
            out[f"m/t{t}/init/{n}"] = named[n].detach().clone()
        opt = torch.optim.SGD([p for p in model.get_parameters(None) if p.requires_grad], lr=LR, momentum=MOM)
        model.train()
        for s in range(STEPS):
            pred, acc, loss = model.observe({"image": x[t, s], "label": y[t, s]})
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.detach())
            preds.append(pred)
            for n in train:
                out[f"m/t{t}/s{s}/{n}"] = named[n].detach().clone()
        model.after_task(t, None, None, None)
    out["m/losses"] = torch.stack(losses).view(TASKS, STEPS)
    out["m/preds"] = torch.stack(preds).view(TASKS, STEPS, BATCH)


def main():
    ref_shim.install_vit_standins()
    tr = ref_shim.load("core.model.backbone.transformer")
    vit = ref_shim.load("core.model.backbone.vit")
    sd = ref_shim.load("core.model.sd_lora")
    out = {}
    attention_part(tr, out)
    method_part(tr, vit, sd, out)
    path = os.path.join(ROOT, "tests", "golden", "sdlora_tiny.npz")
    np.savez_compressed(path, **{k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()})
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
