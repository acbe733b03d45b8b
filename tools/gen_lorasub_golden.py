"""Write tests/golden/lorasub_tiny.npz from fp64 runs of the REFERENCE's own `MultiHeadAttention_LoRA_Sub` (core/model/backbone/transformer.py:359-444),
`LoRAsub_DRS`, `AugmentedTripletLoss` and projected `Adam` (core/model/lora_sub.py), imported through oracle.ref_shim with its stand-ins for timm.

    python tools/gen_lorasub_golden.py          (needs the reference tree; the fixture is committed)

A 3-block ViT (img 32, patch 8, D 64, 2 heads, mlp 256), lora_rank 4, 3 tasks of 3 classes x 3 steps, batch 9 with labels [0, 1, 2] * 3 + 3 t (every class has
partners), lr 0.004, fc_lrate 0.002, margin 1, lambada 0.05, the optimizer from `get_optimizer` after `before_task` as the reference's trainer builds it.  A
task's loaders are the list of its three fixed batches; images are noise with a random gain per sample and channel; B of the new term is set to
uniform(-0.05, 0.05) after `before_task`, so that A has a gradient from the first step.  Stored: the backbone weights, per task the
names `before_task` left trainable and their initial values, images (bytes, / 255) and labels, per step the loss, the triplet term, the predictions and every
trained tensor, the draws of `init_param` under seed 4321 (`draw/`), per task the Gram mean G, its singular values S, k per layer, T, the prototypes and the inference predictions on a batch of 12, and
prev_{k,v} after the last task.  To stay under the size limit of a committed file the weights are bf16-representable and stored as 16-bit words, the images are
stored at half resolution (every pixel doubled), and G, T, prev are stored in fp32; losses, trained tensors, S and prototypes are fp64.

The file is written only when (a) for every task >= 1 and layer 1 <= k < D and the cumulative ratio is at least 1e-4 away from 0.99 on both sides of the
cut, (b) in every triplet evaluation every selection and hinge argument is 1e-3 apart (lorasub_ref.atl's `gap`), a row is active and, from task 1 on, a row
takes a prototype as its negative, (c) an fp32 CPU run of tests/lorasub_ref.py meets the f32 tolerances of tests/test_lorasub_gpu.py.  The seed counts up
from 99 until they hold and is stored; tests/test_lorasub_cpu.py asserts the conditions again and holds tests/lorasub_ref.py to the fixture at 1e-10.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim  # noqa: E402
import lorasub_ref as R  # noqa: E402

CFG = R.CFG
TASKS, STEPS, BATCH, NI = 3, 3, 9, 12
NAMES = ("lora_A_k", "lora_A_v", "lora_B_k", "lora_B_v")


def images(g, n):
    """noise at half the resolution (R.fixture_images doubles every pixel: the fixture has a size limit) with a random gain per sample and channel"""
    return (torch.rand(n, 3, CFG["img"] // 2, CFG["img"] // 2, generator=g) * torch.rand(n, 3, 1, 1, generator=g) * 255).to(torch.uint8)


def run(tr, vit, ls, seed):
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    zoo = vit.ViTZoo.__new__(vit.ViTZoo)
    nn.Module.__init__(zoo)
    zoo.task_id, zoo.feat_dim = None, CFG["dim"]
    zoo.feat = tr.VisionTransformer(img_size=CFG["img"], patch_size=CFG["patch"], embed_dim=CFG["dim"], depth=CFG["depth"], num_heads=CFG["heads"],
                                    ckpt_layer=0, drop_path_rate=0, attn_layer="MultiHeadAttention_LoRA_Sub", lora_rank=R.RANK)
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
        for v in zoo.state_dict().values():                # bf16-representable: the fixture stores 16 bits per weight
            v.copy_(v.bfloat16().float())
    model = ls.LoRAsub_DRS(zoo, "cpu", init_cls_num=R.INC, inc_cls_num=R.INC, task_num=TASKS, embd_dim=CFG["dim"], fc_lrate=R.FC_LR, margin_inter=R.MARGIN,
                           lambada=R.LAMBADA)
    out = {"seed": np.array(seed)}
    for k, v in zoo.state_dict().items():
        out["w/" + k] = v.bfloat16().view(torch.int16)
    x8 = torch.stack([images(g, STEPS * BATCH).view(STEPS, BATCH, 3, CFG["img"] // 2, CFG["img"] // 2) for _ in range(TASKS)])
    y = torch.stack([(torch.arange(BATCH) % R.INC + R.INC * t).expand(STEPS, BATCH) for t in range(TASKS)]).contiguous()
    xi8 = images(g, NI)
    out["x_u8"], out["y"], out["xi_u8"] = x8, y, xi8
    x, xi = R.fixture_images(x8).double() / 255.0, R.fixture_images(xi8).double() / 255.0
    rec = []                                               # every triplet evaluation: (normalised features, shifted labels, prototypes, value)
    model.criterion.register_forward_hook(lambda m, i, o: rec.append((i[0].detach().clone(), i[1].clone(), np.array(i[2]), o.detach().clone())))
    losses, atls, preds = [], [], []
    for t in range(TASKS):
        loader = [{"image": x[t, s], "label": y[t, s]} for s in range(STEPS)]
        model._network.double()                            # (before_task's Gram pass of task >= 1 runs in fp64 too)
        model.before_task(t, None, loader, None)
        with torch.no_grad():
            for a in model.attention_modules:              # a non-zero B of the new term, so that its A has a gradient from the first step on
                a.lora_B_k.weight.copy_(torch.empty(CFG["dim"], R.RANK).uniform_(-0.05, 0.05))
                a.lora_B_v.weight.copy_(torch.empty(CFG["dim"], R.RANK).uniform_(-0.05, 0.05))
        model._network.double()
        named = dict(model._network.named_parameters())
        train = sorted(n for n, p in named.items() if p.requires_grad)
        out[f"t{t}/trainable"] = np.array(train)
        for n in train:
            out[f"t{t}/init/{n}"] = named[n].detach().clone()
        opt = model.get_optimizer(R.LR, 0.0)
        if t > 0:
            mods = model.attention_modules
            out[f"t{t}/G"] = torch.stack([model.fea_in[a.lora_A_k.weight] for a in mods]).float()             # (fp32, like T and prev: the size limit)
            out[f"t{t}/S"] = torch.stack([opt.eigens[a.lora_A_k.weight]["eigen_value"] for a in mods])
            out[f"t{t}/T"] = torch.stack([opt.transforms[a.lora_A_k.weight] for a in mods]).float()
            for a in mods:                                 # the four factors of a block share one transform
                assert all(torch.equal(opt.transforms[getattr(a, n).weight], opt.transforms[a.lora_A_k.weight]) for n in NAMES)
            ratio = out[f"t{t}/S"].cumsum(1) / out[f"t{t}/S"].sum(1, keepdim=True)
            out[f"t{t}/k"] = np.array([int((r >= 0.99).nonzero()[0][0]) + 1 for r in ratio])
        model.train()
        for s in range(STEPS):
            pred, acc, loss = model.observe({"image": x[t, s], "label": y[t, s]})
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.detach())
            atls.append(rec[-1][3])
            preds.append(pred)
            for n in train:
                out[f"t{t}/s{s}/{n}"] = named[n].detach().clone()
        model.after_task(t, None, loader, None)
        if t == TASKS - 1:                                 # (the earlier ones are the sums of B A of the stored factors; the later tasks' losses depend on them)
            out["prev_k"] = torch.stack([a.prev_k_weight for a in model.attention_modules]).float()
            out["prev_v"] = torch.stack([a.prev_v_weight for a in model.attention_modules]).float()
        out[f"t{t}/protos"] = np.stack(model._protos)
        model.eval()
        ip, _ = model.inference({"image": xi, "label": torch.zeros(NI, dtype=torch.int64)})
        out[f"t{t}/infer_pred"] = np.asarray(ip).astype(np.int64)
    out["losses"] = torch.stack(losses).view(TASKS, STEPS)
    out["atl"] = torch.stack(atls).view(TASKS, STEPS)
    out["preds"] = torch.stack(preds).view(TASKS, STEPS, BATCH)
    return {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}, rec


def main():
    ref_shim.install_vit_standins()
    tr = ref_shim.load("core.model.backbone.transformer")
    vit = ref_shim.load("core.model.backbone.vit")
    ls = ref_shim.load("core.model.lora_sub")
    for seed in range(99, 1099):
        fix, rec = run(tr, vit, ls, seed)
        why = R.condition_a(fix)
        if not why:
            got = R.run_fixture(fix)
            d = R.deviations(got, fix)
            why = R.condition_b(got) or ("" if max(d["losses"], d["atl"], d["worst"][0], d["protos"]) < 1e-10 and max(d["T"], d["G"], d["prev"]) < 1e-6 else f"restatement: {d}")
        why = why or (lambda w: w and "(c) " + w)(R.check_f32(R.run_fixture(fix, torch.float32), fix))
        if not why:
            break
        print(f"seed {seed}: {why}", flush=True)
    else:
        raise SystemExit("no seed met the conditions")
    # what init_param draws under one seed (transformer.py:382-389), three modules in a row as before_task visits them (lora_sub.py:342-343)
    mods = [tr.MultiHeadAttention_LoRA_Sub(CFG["dim"], CFG["heads"], lora_rank=R.RANK) for _ in range(CFG["depth"])]
    torch.manual_seed(4321)
    for b, m in enumerate(mods):
        m.init_param()
        for n in NAMES:
            fix[f"draw/{b}/{n}"] = getattr(m, n).weight.detach().numpy().copy()
    path = os.path.join(ROOT, "tests", "golden", "lorasub_tiny.npz")
    np.savez_compressed(path, **fix)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(fix)} arrays, seed {seed}, k {[fix[f't{t}/k'].tolist() for t in (1, 2)]}")


if __name__ == "__main__":
    main()
