"""Write tests/golden/coda_tiny.npz from fp64 runs of the REFERENCE's own classes: `CodaPrompt` of core/model/backbone/prompt.py:37-223, the prompted
`VisionTransformer.forward` / `ViTZoo.forward` (transformer.py:2263-2296, vit.py:120-138) and the method core/model/codaprompt.py, imported through
oracle.ref_shim with its stand-ins for timm.

    python tools/gen_coda_golden.py          (needs the reference tree; the fixture is committed)

Toy ViT: img 32, patch 8, D 64, depth 6, 2 heads, mlp 256; blocks 0-4 are prompted (prompt.py:71), block 5 is not.  Pool: CodaPrompt(64, n_tasks=2,
[6, 8, 0.0], key_dim=64) built right after torch.manual_seed(POOL_SEED) -- ViTZoo.create_prompt hard-codes 768, so the pool is assigned by hand.
2 tasks x 3 classes x 3 Adam steps at batch 6, a fresh optimizer per task (the reference's trainer builds one per task).

Two things the reference needs to run here, neither of which edits or copies it:
  * transformer.py:2272 builds the prompt loss as `torch.zeros((1,), requires_grad=True).to(device)`: on the CPU `.to` returns the leaf itself and the
    in-place `prompt_loss += loss` raises.  The loaded module's global `torch` is replaced by a proxy whose `zeros(..., requires_grad=True)` returns a
    non-leaf copy; every other attribute is torch's.
  * the run happens under torch.set_default_dtype(torch.float64): that zero would otherwise be fp32 and round the returned loss.
`process_task_count()` is called by nothing under core/, so `task_count` stays 0 and only components [0, 3) are used and trained in both tasks; the
fixture shows it (rows >= 3 of every pool tensor stay zero, which tests/test_coda_cpu.py asserts).

Stored (keys): `w_tag` the tag of the backbone weights (oracle.vit.det_params(CFG, tag): fp32 values generated from the parameter names, as the other ViT fixtures do), `pool0/...` the seeded initial pool (fp32, bit-exact), `x_u8`, `y`, per task `t{t}/init/classifier.*`
(the regrown head, rounded to fp32 before the run), `t{t}/s{s}/<name>` every trainable tensor after each step (of a pool tensor the rows [0, 3) of the window), `final_pool/...` the whole pool after the last
task, `losses`, `preds`, `infer_x_u8`,
`infer_preds` (inference after each task on a batch of 12).

Learning rate: Adam's first steps are lr sign(g), so an fp32 run can flip an element whose gradient is at rounding level.  Before writing, an fp32 CPU run
of tests/coda_ref.py itself is held to the f32 tolerances of the GPU method test (first loss 2e-4, losses 5e-3, every trained tensor 5e-3 of its max-abs,
first step's predictions equal).  It passes at lr 0.004 with seeds 77 / 2024 (the reference's config uses 0.001; 0.004 moves the parameters further
within three steps, so the comparison sees more of the gradient).
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim, vit as ov  # noqa: E402
import coda_ref as R  # noqa: E402

CFG = R.CFG
POOL_SEED, RUN_SEED = 2024, 77
F_WIN = R.POOL // R.TASKS


class _TorchProxy:
    """`torch` for the reference's transformer module: zeros(..., requires_grad=True) comes back as a non-leaf"""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def zeros(*a, **k):
        z = torch.zeros(*a, **k)
        return z.clone() if k.get("requires_grad") else z


def build(tr, vit, pr, cp):
    torch.manual_seed(RUN_SEED)
    zoo = vit.ViTZoo.__new__(vit.ViTZoo)
    nn.Module.__init__(zoo)
    zoo.task_id, zoo.feat_dim = None, CFG["dim"]
    zoo.feat = tr.VisionTransformer(img_size=CFG["img"], patch_size=CFG["patch"], embed_dim=CFG["dim"], depth=CFG["depth"], num_heads=CFG["heads"],
                                    ckpt_layer=0, drop_path_rate=0, attn_layer="MultiHeadAttention")
    zoo.prompt, zoo.prompt_flag = None, ""
    # the frozen weights are oracle.vit.det_params(CFG, W_TAG): generated from the parameter names, so the fixture need not carry them (they alone
    # would be 0.8 MB)
    zoo.load_state_dict({k: v for k, v in ov.det_params(CFG, R.W_TAG).items()}, strict=True)
    created = []
    zoo.create_prompt = lambda flag, **kw: created.append((flag, kw))          # (the method's constructor asks for the 768-wide pool: assigned below)
    model = cp.CodaPrompt(zoo, CFG["dim"], R.INC * R.TASKS, device="cpu", init_cls_num=R.INC, inc_cls_num=R.INC, task_num=R.TASKS, pool_size=R.POOL,
                          prompt_length=R.LENGTH, mu=0.0)
    assert created == [("coda", {"n_tasks": R.TASKS, "prompt_param": [R.POOL, R.LENGTH, 0.0]})]
    torch.manual_seed(POOL_SEED)
    zoo.prompt = pr.CodaPrompt(CFG["dim"], R.TASKS, [R.POOL, R.LENGTH, 0.0], key_dim=CFG["dim"])
    zoo.prompt_flag = "coda"
    return zoo, model


def run(zoo, model, out):
    out["w_tag"] = np.array(R.W_TAG)
    for k, v in zoo.prompt.state_dict().items():
        assert v.dtype == torch.float32
        out["pool0/" + k] = v.detach().clone()
    g = torch.Generator().manual_seed(RUN_SEED + 1)
    x8 = torch.randint(0, 256, (R.TASKS, R.STEPS, R.BATCH, 3, CFG["img"], CFG["img"]), dtype=torch.uint8, generator=g)
    y = torch.stack([torch.randint(t * R.INC, (t + 1) * R.INC, (R.STEPS, R.BATCH), generator=g) for t in range(R.TASKS)])
    xi8 = torch.randint(0, 256, (12, 3, CFG["img"], CFG["img"]), dtype=torch.uint8, generator=g)
    out["x_u8"], out["y"], out["infer_x_u8"] = x8, y, xi8
    torch.set_default_dtype(torch.float64)
    model.double()
    x, xi = x8.double() / 255.0, xi8.double() / 255.0
    losses, preds, ipreds = [], [], []
    for t in range(R.TASKS):
        model.before_task(t, None, None, None)
        with torch.no_grad():                              # the new head rows are drawn in fp64: kept fp32-representable
            for p in model.network.classifier.parameters():
                p.copy_(p.float().double())
        named = dict(model.network.named_parameters())
        train = sorted(n for n in named if n.startswith("backbone.prompt.") or n.startswith("classifier."))
        assert sorted(id(p) for p in model.get_parameters(None)) == sorted(id(named[n]) for n in train)
        out[f"t{t}/init/classifier.weight"] = named["classifier.weight"].detach().clone()
        out[f"t{t}/init/classifier.bias"] = named["classifier.bias"].detach().clone()
        opt = torch.optim.Adam(model.get_parameters(None), lr=R.LR, betas=R.BETAS, weight_decay=0)
        model.train()
        for s in range(R.STEPS):
            pred, acc, loss = model.observe({"image": x[t, s], "label": y[t, s]})
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.detach().reshape(()))
            preds.append(pred)
            for n in train:                                # (pool tensors: the rows of the window; `final_pool/` has them whole)
                v = named[n].detach()
                out[f"t{t}/s{s}/{n.replace('backbone.prompt.', '')}"] = (v[:F_WIN] if "prompt" in n else v).clone()
        assert zoo.prompt.task_count == 0
        model.after_task(t, None, None, None)
        model.eval()
        with torch.no_grad():
            ipreds.append(model.inference({"image": xi, "label": torch.zeros(12, dtype=torch.long)})[0])
    for k, v in zoo.prompt.state_dict().items():
        out["final_pool/" + k] = v.detach().clone()
    out["losses"] = torch.stack(losses).view(R.TASKS, R.STEPS)
    out["preds"] = torch.stack(preds).view(R.TASKS, R.STEPS, R.BATCH)
    out["infer_preds"] = torch.stack(ipreds)
    torch.set_default_dtype(torch.float32)


def main():
    ref_shim.install_vit_standins()
    tr = ref_shim.load("core.model.backbone.transformer")
    vit = ref_shim.load("core.model.backbone.vit")
    pr = ref_shim.load("core.model.backbone.prompt")
    cp = ref_shim.load("core.model.codaprompt")
    tr.torch = _TorchProxy()
    out = {}
    zoo, model = build(tr, vit, pr, cp)
    run(zoo, model, out)
    fix = {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    got = R.replay(fix, torch.float64)
    first, losses, worst = R.deviations({k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}, fix)
    print(f"coda_ref fp64 against the reference: first losses {first:.2e}, losses {losses:.2e}, worst tensor {worst[0]:.2e} ({worst[1]})")
    assert max(first, losses, worst[0]) < 1e-10
    got = R.replay(fix, torch.float32)
    first, losses, worst = R.deviations({k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}, fix)
    print(f"coda_ref fp32 against the reference: first losses {first:.2e}, losses {losses:.2e}, worst tensor {worst[0]:.2e} ({worst[1]})")
    assert first < 2e-4 and losses < 5e-3 and worst[0] < 5e-3, "an fp32 run of the restatement alone misses the f32 tolerances: lower lr or change the seed"
    assert all(np.array_equal(got["preds"][t, 0].numpy(), fix["preds"][t, 0]) for t in range(R.TASKS))
    path = os.path.join(ROOT, "tests", "golden", "coda_tiny.npz")
    np.savez_compressed(path, **fix)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(fix)} arrays")


if __name__ == "__main__":
    main()
