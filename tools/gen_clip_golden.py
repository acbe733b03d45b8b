"""Write tests/golden/clip_tiny.npz and tests/golden/clip_tokens.npz from fp64 runs of the REFERENCE's own `CLIP` (core/model/backbone/clip.py), `InfLoRA_OPT`
(core/model/InfLoRA_opt.py, CLIP branch, visual_only) and tokenizer, imported through oracle.ref_shim with its stand-ins for timm and ftfy.

    PYTHONHASHSEED=0 python tools/gen_clip_golden.py [--tokens-only]          (needs the reference tree; the fixtures are committed)

clip_tiny: image 32, patch 8 (17 tokens), visual width 64 / 1 head / 3 blocks, text width 64 / 1 head / 2 blocks / context 77, embed 32, lora_rank 4; 2 tasks
of 3 classes x 3 steps, batch 9 with labels [0, 1, 2] * 3 + 3 t, torch.optim.Adam at the reference config's values (lr 5e-4, betas 0.9 / 0.999, no decay) on
the parameters `before_task` left trainable.  The process runs with float64 as torch's default dtype, so the reference's `torch.Tensor(...)` casts and its
CPU Gram buffers are fp64 too; its LayerNorm subclass, which casts to fp32, runs nn.LayerNorm's forward instead.  Class names are the first six of CIFAR-100 under the template of the reference config; their tokens come from the
reference tokenizer and are REMAPPED to their rank among the used ids (order preserved, so argmax still finds the end token): the fixture stores only the
`token_embedding` rows that are used.  Stored: the weights (bf16-representable, as 16-bit words), tokens and normalised text features of both class sets per
task, images (bytes) and labels, per step the loss, the logits and every trained lora_B, per task the lora_A that before_task fixed, the DualGPM bases and
types after after_task, and inference logits / predictions on a batch of 12.

The file is written only when (a) every DualGPM rank cut is 1e-4 of the spectrum away from its threshold, (b) the top two entries of every stored logits
row differ by more than the bf16 gate of tests/test_clip_gpu.py allows them to move, (c) an fp32 CPU run of tests/clip_ref.py meets the f32 tolerances of
that test; and tests/clip_ref.py in fp64 reproduces it to 1e-10.  The seed counts up from 7 until they hold and is stored.

clip_tokens: the reference tokenizer's output for the 100 CIFAR-100 class names under the template, and for a few edge strings.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim  # noqa: E402
import clip_ref as R  # noqa: E402

CFG = R.CFG
CIFAR100 = """apple aquarium_fish baby bear beaver bed bee beetle bicycle bottle bowl boy bridge bus butterfly camel can castle caterpillar cattle chair chimpanzee
clock cloud cockroach couch crab crocodile cup dinosaur dolphin elephant flatfish forest fox girl hamster house kangaroo keyboard lamp lawn_mower leopard lion
lizard lobster man maple_tree motorcycle mountain mouse mushroom oak_tree orange orchid otter palm_tree pear pickup_truck pine_tree plain plate poppy porcupine
possum rabbit raccoon ray road rocket rose sea seal shark shrew skunk skyscraper snail snake spider squirrel streetcar sunflower sweet_pepper table tank telephone
television tiger tractor train trout tulip turtle wardrobe whale willow_tree wolf woman worm""".split()
EDGE = ["aquarium_fish", "lawn mower", "A Bad Photo of a MapleTree.", "  two   spaces\tand a tab ", "it's 42 o'clock &amp; more...", " ".join(["caterpillar"] * 80)]


class _Loader(list):
    """a task's loader: the list of its fixed batches, with the dataset interface the reference reads (get_class_names, trfms)"""

    def __init__(self, batches, names):
        super().__init__(batches)
        self.dataset = types.SimpleNamespace(get_class_names=lambda: list(names), trfms=None)


def pictures(g, n):
    return (torch.rand(n, 3, CFG["img"], CFG["img"], generator=g) * torch.rand(n, 3, 1, 1, generator=g) * 255).to(torch.uint8)


def run(clip, iopt, tokens_of, vocab, seed):
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    net = clip.CLIP(CFG["embed"], CFG["img"], CFG["depth"], CFG["width"], CFG["patch"], CFG["ctx"], vocab, CFG["twidth"], CFG["theads"], CFG["tlayers"],
                    attn_layer="MultiHeadAttention_LoRA", lora_rank=R.RANK, act_layer="QuickGELU", norm_layer="LayerNorm")
    with torch.no_grad():                                  # a trained-network-like scale
        for n, p in net.named_parameters():
            if n == "logit_scale":
                continue
            if n.endswith("bias"):
                p.uniform_(-0.05, 0.05)
            elif ".ln_" in n or "ln_p" in n or "ln_final" in n:
                p.uniform_(0.8, 1.2)
            elif p.dim() >= 2 and "embedding" not in n and n not in ("visual.proj", "text_projection"):
                s = 1.7 / np.sqrt(p[0].numel())
                p.uniform_(-s, s)
        for v in net.state_dict().values():                # bf16-representable: the fixture stores 16 bits per weight
            v.copy_(v.bfloat16().to(v.dtype))
    out = {"seed": np.array(seed)}
    for k, v in net.state_dict().items():
        out["w/" + k] = v.bfloat16().view(torch.int16)
    iopt.tokenize = lambda texts, context_length=77: torch.stack([tokens_of[t] for t in texts])
    names = CIFAR100[: R.INC * R.TASKS]
    model = iopt.InfLoRA_OPT(net, "cpu", init_cls_num=R.INC, inc_cls_num=R.INC, task_num=R.TASKS, lame=R.LAME, lamb=R.LAMB, dataset="cifar100", use_ca=False,
                             embd_dim=CFG["width"], prompt_template=R.TEMPLATE, visual_only=True)
    x8 = torch.stack([pictures(g, R.STEPS * R.BATCH).view(R.STEPS, R.BATCH, 3, CFG["img"], CFG["img"]) for _ in range(R.TASKS)])
    y = torch.stack([(torch.arange(R.BATCH) % R.INC + R.INC * t).expand(R.STEPS, R.BATCH) for t in range(R.TASKS)]).contiguous()
    xi8 = pictures(g, R.NI)
    out["x_u8"], out["y"], out["xi_u8"] = x8, y, xi8
    x, xi = x8.double() / 255.0, xi8.double() / 255.0
    for t in range(R.TASKS):
        loader = _Loader([{"image": x[t, s], "label": y[t, s]} for s in range(R.STEPS)], names[R.INC * t: R.INC * (t + 1)])
        model.before_task(t, None, loader, [loader])
        sn = model._network
        out[f"t{t}/curr_tokens"], out[f"t{t}/accm_tokens"] = sn.curr_text_tokens.clone(), sn.accm_text_tokens.clone()
        with torch.no_grad():
            for k, tok in (("curr", sn.curr_text_tokens), ("accm", sn.accm_text_tokens)):
                f = net.encode_text(tok)
                out[f"t{t}/{k}_txt"] = f / f.norm(dim=-1, keepdim=True)
        named = dict(model._network.named_parameters())
        train = sorted(n for n, p in named.items() if p.requires_grad)
        assert train == sorted(f"backbone.visual.transformer.blocks.{l}.attn.lora_B_{kv}.weight" for l in range(CFG["depth"]) for kv in "kv"), train
        out[f"t{t}/lora_A"] = torch.stack([a.lora_A_k.weight.detach().clone() for a in model.attention_modules])
        assert all(torch.equal(a.lora_A_k.weight, a.lora_A_v.weight) for a in model.attention_modules)
        opt = torch.optim.Adam([named[n] for n in train], lr=R.LR, betas=R.BETAS, weight_decay=0)
        model.train()
        for s in range(R.STEPS):
            _, _, loss = model.observe({"image": x[t, s], "label": y[t, s]})
            with torch.no_grad():
                out[f"t{t}/s{s}/logits"] = model._network(x[t, s]).clone()
            opt.zero_grad()
            loss.backward()
            opt.step()
            out[f"t{t}/s{s}/loss"] = loss.detach().clone()
            out[f"t{t}/s{s}/lora_B"] = torch.stack([torch.stack([a.lora_B_k.weight.detach().clone(), a.lora_B_v.weight.detach().clone()]) for a in model.attention_modules])
        model.after_task(t, None, loader, [loader])
        for l, f in enumerate(model.feature_list):
            out[f"t{t}/basis{l}"] = np.asarray(f, dtype=np.float64)
        out[f"t{t}/ptype"] = np.array(model.project_type)
        model.eval()
        with torch.no_grad():
            out[f"t{t}/infer_logits"] = model._network(xi, inference=True).clone()
            out[f"t{t}/infer_pred"] = model.inference({"image": xi, "label": torch.zeros(R.NI, dtype=torch.int64)})[0].clone()
    return {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def main():
    os.environ.setdefault("PYTHONHASHSEED", "0")
    torch.set_default_dtype(torch.float64)
    ref_shim.install_vit_standins()
    tr = ref_shim.load("core.model.backbone.transformer")
    # the reference's LayerNorm subclass "handles fp16" by casting its input to fp32 (transformer.py:129-135), which would make an fp64 run an fp32 one at
    # every norm: for this run it is nn.LayerNorm's own forward (the same arithmetic, in the dtype of the input)
    tr.LayerNorm.forward = torch.nn.LayerNorm.forward
    clip = ref_shim.load("core.model.backbone.clip")
    iopt = ref_shim.load("core.model.InfLoRA_opt")
    gold = os.path.join(ROOT, "tests", "golden")
    # ---- the tokenizer fixture
    texts = [R.TEMPLATE.format(c) for c in CIFAR100] + EDGE
    tok = clip.tokenize(texts)
    np.savez_compressed(os.path.join(gold, "clip_tokens.npz"), texts=np.array(texts), tokens=tok.numpy().astype(np.int32))
    if "--tokens-only" in sys.argv:
        return
    # ---- the tokens of the fixture's six classes, remapped to their rank among the used ids
    mine = [R.TEMPLATE.format(c) for c in CIFAR100[: R.INC * R.TASKS]]
    raw = clip.tokenize(mine)
    used = torch.unique(raw)                               # sorted; 0 (the padding) is among them
    remap = torch.searchsorted(used, raw)
    tokens_of = {t: remap[i] for i, t in enumerate(mine)}
    for seed in range(7, 1007):
        fix = run(clip, iopt, tokens_of, len(used), seed)
        why = R.condition_b(fix, 1.25)                      # (a quarter more than the test asks: the gate is re-measured on the fixture this writes)
        if why:
            print(f"seed {seed}: {why}", flush=True)
            continue
        got = R.run_fixture(fix)
        d = R.deviations(got, fix)
        why = R.condition_a(got["margins"])
        if not why and not (max(d["losses"], d["logits"], d["lora_B"], d["lora_A"], d["bases"], d["txt"]) < 1e-10 and d["preds_equal"]):
            why = f"restatement: {d}"
        why = why or (lambda w: w and "(c) " + w)(R.check_f32(R.run_fixture(fix, torch.float32), fix))
        if not why:
            break
        print(f"seed {seed}: {why}", flush=True)
    else:
        raise SystemExit("no seed met the conditions")
    path = os.path.join(gold, "clip_tiny.npz")
    np.savez_compressed(path, **fix)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(fix)} arrays, seed {seed}, ranks {[[fix[f't{t}/basis{l}'].shape[1] for l in range(CFG['depth'])] for t in range(R.TASKS)]}, "
          f"types {[fix[f't{t}/ptype'].tolist() for t in range(R.TASKS)]}, margins min {min(got['margins']):.3g}")


if __name__ == "__main__":
    main()
