"""LoRAsub_DRS on the HIP ViT executor (model/lora_sub.py, backbone/vit.py, csrc/lorasub.hip inside csrc/vit_plan.hip) on a real MI355X: the three weight
forms of MultiHeadAttention_LoRA_Sub and one training step's gradients against the fp64 restatement of tests/lorasub_ref.py on the toy ViT (f32 mode, the
project's 5e-3 of max-abs), the fixture of fp64 runs of the reference's own classes (tests/golden/lorasub_tiny.npz) in f32 and bf16, and a three-task run
through the product Trainer."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lorasub_ref as R                              # noqa: E402
import libcontinual_amd.model as M                  # noqa: E402
from libcontinual_amd.model.lora_sub import ProjectedAdam   # noqa: E402

DEV = "cuda"
CFG = R.CFG


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def _model(dtype, seed=0):
    """the toy with a finished first task: non-zero prev buffers, fresh factors with B != 0, three prototypes"""
    torch.manual_seed(seed)
    bb = M.vit_pt_imnet(pretrained=False, attn_layer="MultiHeadAttention_LoRA_Sub", img_size=CFG["img"], patch_size=CFG["patch"], embed_dim=CFG["dim"],
                        depth=CFG["depth"], num_heads=CFG["heads"], dtype=dtype, lora_rank=R.RANK)
    model = M.LoRAsub_DRS(bb.to(DEV), DEV, init_cls_num=R.INC, inc_cls_num=R.INC, task_num=3, embd_dim=CFG["dim"], fc_lrate=R.FC_LR, margin_inter=R.MARGIN,
                          lambada=R.LAMBADA)
    g = torch.Generator().manual_seed(seed + 1)
    model.before_task(0, None, None, None)
    with torch.no_grad():
        for a in model.attention_modules:
            a.lora_B_k.weight.copy_(torch.empty(CFG["dim"], R.RANK).uniform_(-0.05, 0.05, generator=g))
            a.lora_B_v.weight.copy_(torch.empty(CFG["dim"], R.RANK).uniform_(-0.05, 0.05, generator=g))
    x0 = torch.rand(9, 3, CFG["img"], CFG["img"], generator=g) * torch.rand(9, 3, 1, 1, generator=g)
    y0 = torch.arange(9) % 3
    model.after_task(0, None, [{"image": x0, "label": y0}], None)                  # save_weight: prev += B A; three prototypes
    model.before_task(1, None, [{"image": x0, "label": y0}], None)                 # the Gram pass on W - prev, the SVDs, T
    with torch.no_grad():
        for a in model.attention_modules:
            a.lora_B_k.weight.copy_(torch.empty(CFG["dim"], R.RANK).uniform_(-0.05, 0.05, generator=g))
            a.lora_B_v.weight.copy_(torch.empty(CFG["dim"], R.RANK).uniform_(-0.05, 0.05, generator=g))
    x1 = torch.rand(9, 3, CFG["img"], CFG["img"], generator=g) * torch.rand(9, 3, 1, 1, generator=g)
    return model, x0, x1, torch.arange(9) % 3 + 3


def _state64(model):
    P = {k: v.detach().double().cpu() for k, v in model._network.backbone.state_dict().items()}
    fac = [tuple(getattr(a, n).weight.detach().double().cpu() for n in R.FACTORS) for a in model.attention_modules]
    return P, fac


def test_three_weight_forms_against_fp64():
    model, x0, x1, _ = _model("f32")
    P, fac = _state64(model)
    assert float(P["feat.transformer.blocks.0.attn.prev_k_weight"].abs().max()) > 0
    bb = model._network.backbone
    for form, lora, sub in (("lora", True, False), ("plain", False, False), ("sub", False, True)):
        for a in model.attention_modules:
            a.apply_lora, a.subtract = lora, sub
        with torch.no_grad():
            got = bb(x1.to(DEV)).cpu()
        want = R.features(P, x1.double(), form, fac)
        others = [R.features(P, x1.double(), o, fac) for o in ("lora", "plain", "sub") if o != form]
        d = rel(got, want)
        print(f"weight form {form}: features {d:.2e} of max-abs; the other forms differ by {min(rel(o, want) for o in others):.2e}")
        assert d < 5e-3 and min(rel(o, want) for o in others) > 10 * 5e-3            # ... and the tolerance tells the forms apart
    for a in model.attention_modules:
        a.apply_lora, a.subtract = True, False
    pre = {k: v.clone() for k, v in bb.state_dict().items() if k.endswith("qkv.weight")}
    with torch.no_grad():
        bb(x1.to(DEV))
    assert all(torch.equal(v, bb.state_dict()[k]) for k, v in pre.items())          # the pretrained weight is never modified


def test_step_gradients_of_all_factors_against_fp64():
    model, _, x1, y1 = _model("f32")
    P, fac = _state64(model)
    head = model._network.classifier_pool[1]
    protos = model._protos.double().cpu()
    loss, term, gf, gw, gb = R.step_loss_and_grads(P, fac, head.weight.detach().double().cpu(), head.bias.detach().double().cpu(), x1.double(), y1 - R.INC, protos)
    model.train()
    pred, acc, l = model.observe({"image": x1.to(DEV), "label": y1.to(DEV)})
    l.backward()
    print(f"step: loss {float(l.detach()):.6f} (fp64 {loss:.6f}), ATL {float(model.last_atl):.6f} (fp64 {term:.6f})")
    assert abs(float(l.detach()) - loss) < 2e-4 * abs(loss) and abs(float(model.last_atl) - term) < 2e-4 * abs(term) and term > 0
    worst = 0.0
    for b, a in enumerate(model.attention_modules):
        for j, n in enumerate(R.FACTORS):
            d = rel(getattr(a, n).weight.grad.cpu(), gf[b][j])
            worst = max(worst, d)
            assert d < 5e-3, (b, n, d)
            assert float(gf[b][j].abs().max()) > 0
    assert rel(head.weight.grad.cpu(), gw) < 5e-3 and rel(head.bias.grad.cpu(), gb) < 5e-3
    print(f"step: worst factor gradient {worst:.2e} of max-abs")


def test_optimizer_step_is_the_projected_adam():
    model, _, x1, y1 = _model("f32")
    opt = model.get_optimizer(R.LR, 0.0)
    assert isinstance(opt, ProjectedAdam) and [g["lr"] for g in opt.param_groups] == [R.LR, R.FC_LR] and opt.transforms is model.transforms
    model.train()
    _, _, l = model.observe({"image": x1.to(DEV), "label": y1.to(DEV)})
    opt.zero_grad()
    l.backward()
    a = model.attention_modules[1]
    before = {n: getattr(a, n).weight.detach().double().cpu() for n in R.FACTORS}
    grads = {n: getattr(a, n).weight.grad.detach().double().cpu() for n in R.FACTORS}
    opt.step()
    T = model.transforms[1].double().cpu()
    for n in R.FACTORS:
        want, _, _ = R.proj_adam(before[n], grads[n], torch.zeros_like(before[n]), torch.zeros_like(before[n]), T, R.LR, 0.9, 0.999, 1e-8, 0.0, 1, ref_form=True)
        d = rel(getattr(a, n).weight.detach().cpu() - before[n].float(), want - before[n])
        assert d < 5e-3, (n, d)


def test_forward_after_a_step_sees_the_moved_factors():
    """A and B both moved: the per-step refresh (clhip_vit_lora_refresh_ab) must bring the k / v rows of the executor's copies up to date -- the loss and the
    gradients of the step after an optimizer step against fp64 on the parameters as the step left them"""
    model, _, x1, y1 = _model("f32")
    opt = model.get_optimizer(0.05, 0.0)                       # (a rate at which two steps move the loss far beyond the tolerance below)
    model.train()
    batch = {"image": x1.to(DEV), "label": y1.to(DEV)}
    first = None
    for _ in range(2):
        _, _, l = model.observe(batch)
        first = float(l.detach()) if first is None else first
        opt.zero_grad()
        l.backward()
        opt.step()
    P, fac = _state64(model)
    head = model._network.classifier_pool[1]
    loss, term, gf, _, _ = R.step_loss_and_grads(P, fac, head.weight.detach().double().cpu(), head.bias.detach().double().cpu(), x1.double(), y1 - R.INC,
                                                 model._protos.double().cpu())
    _, _, l = model.observe(batch)
    opt.zero_grad()
    l.backward()
    stale = abs(float(l.detach()) - loss) / abs(loss)
    print(f"third step: loss {float(l.detach()):.6f} (fp64 {loss:.6f}; the first step's was {first:.6f})")
    assert stale < 2e-4 and abs(first - loss) > 100 * 2e-4 * abs(loss)
    for b, a in enumerate(model.attention_modules):
        for j, n in enumerate(R.FACTORS):
            assert rel(getattr(a, n).weight.grad.cpu(), gf[b][j]) < 5e-3, (b, n)


# ------------------------------------------------------------------------------- the fixture: fp64 runs of the reference's own classes
def run_fixture(fix, dtype):
    """tests/golden/lorasub_tiny.npz (tools/gen_lorasub_golden.py) through LoRAsub_DRS: three tasks of three steps with the optimizer of get_optimizer, as the
    reference's trainer builds it; what `before_task` draws at random is overwritten with the reference's draws"""
    bb = M.vit_pt_imnet(pretrained=False, attn_layer="MultiHeadAttention_LoRA_Sub", img_size=CFG["img"], patch_size=CFG["patch"], embed_dim=CFG["dim"],
                        depth=CFG["depth"], num_heads=CFG["heads"], dtype=dtype, lora_rank=R.RANK)
    bb.load_state_dict(R.fixture_weights(fix), strict=True)
    model = M.LoRAsub_DRS(bb.to(DEV), DEV, init_cls_num=R.INC, inc_cls_num=R.INC, task_num=3, embd_dim=CFG["dim"], fc_lrate=R.FC_LR, margin_inter=R.MARGIN,
                          lambada=R.LAMBADA)
    x = R.fixture_images(fix["x_u8"]).float() / 255.0
    xi = R.fixture_images(fix["xi_u8"]).float() / 255.0
    y = torch.from_numpy(fix["y"])
    out = {"losses": np.zeros((3, 3)), "atl": np.zeros((3, 3))}
    for t in range(3):
        loader = [{"image": x[t, s], "label": y[t, s]} for s in range(3)]
        model.before_task(t, None, loader, None)
        named = dict(model._network.named_parameters())
        names = sorted(n for n, p in named.items() if p.requires_grad)
        assert names == [str(n) for n in fix[f"t{t}/trainable"]]
        with torch.no_grad():
            for n in names:
                named[n].copy_(torch.from_numpy(fix[f"t{t}/init/{n}"]).float())
        opt = model.get_optimizer(R.LR, 0.0)
        if t:
            out[f"t{t}/k"], out[f"t{t}/T"] = list(model.reserved_basis), model.transforms.cpu()
        model.train()
        for s in range(3):
            pred, acc, loss = model.observe({"image": x[t, s].to(DEV), "label": y[t, s].to(DEV)})
            opt.zero_grad()
            loss.backward()
            opt.step()
            out["losses"][t, s], out["atl"][t, s] = float(loss.detach()), float(model.last_atl)
            for n in names:
                out[f"t{t}/s{s}/{n}"] = named[n].detach().cpu().clone()
        model.after_task(t, None, loader, None)
        out[f"t{t}/protos"] = model._protos.cpu().clone()
        model.eval()
        out[f"t{t}/infer_pred"] = model.inference({"image": xi, "label": torch.zeros(len(xi), dtype=torch.int64)})[0].cpu()
    out["prev_k"] = torch.stack([a.prev_k_weight for a in model.attention_modules]).cpu()
    out["prev_v"] = torch.stack([a.prev_v_weight for a in model.attention_modules]).cpu()
    for t in (1, 2):
        out[f"t{t}/G"] = torch.from_numpy(fix[f"t{t}/G"])                     # (the Gram is consumed inside before_task; T and k are its check)
    return out


def test_lorasub_golden_f32(golden):
    """f32 mode against the fp64 run of the reference's LoRAsub_DRS, at the project's tolerances (tests/test_sdlora_gpu.py): the first loss of a task 2e-4, all
    losses and every trained tensor after each of the 3 x 3 steps 5e-3 of max-abs, k per layer equal, T and the prototypes 5e-3, the inference predictions
    equal"""
    fix = golden("lorasub_tiny")
    got = run_fixture(fix, "f32")
    d = R.deviations(got, fix)
    print(f"LoRAsub_DRS fixture f32: first losses {d['first']:.2e}, all losses {d['losses']:.2e}, triplet terms {d['atl']:.2e}, worst trained tensor "
          f"{d['worst'][0]:.2e} ({d['worst'][1]}), T {d['T']:.2e}, prototypes {d['protos']:.2e}, prev {d['prev']:.2e}")
    assert d["first"] < 2e-4
    assert d["losses"] < 5e-3 and d["atl"] < 5e-3
    assert d["worst"][0] < 5e-3, d["worst"]
    for t in (1, 2):
        assert got[f"t{t}/k"] == fix[f"t{t}/k"].tolist(), (t, got[f"t{t}/k"])
    assert d["T"] < 5e-3 and d["protos"] < 5e-3 and d["prev"] < 5e-3
    for t in range(3):
        assert torch.equal(got[f"t{t}/infer_pred"], torch.from_numpy(fix[f"t{t}/infer_pred"])), t


def test_lorasub_golden_bf16(golden):
    """bf16 mode, by the project's bf16 convention: the first loss of a task 3e-2, all losses 0.1, everything finite, k per layer within 1 of the fixture's"""
    fix = golden("lorasub_tiny")
    got = run_fixture(fix, "bf16")
    d = R.deviations(got, fix)
    ks = {t: (got[f"t{t}/k"], fix[f"t{t}/k"].tolist()) for t in (1, 2)}
    print(f"LoRAsub_DRS fixture bf16: first losses {d['first']:.2e}, all losses {d['losses']:.2e}, worst trained tensor {d['worst'][0]:.2e} ({d['worst'][1]}), "
          f"T {d['T']:.2e}, prototypes {d['protos']:.2e}; k per layer (got, fixture) {ks}")
    assert d["first"] < 3e-2
    assert d["losses"] < 0.1
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for k, v in got.items() if k.startswith("t") or k.startswith("prev"))
    for t in (1, 2):
        assert all(abs(a - b) <= 1 for a, b in zip(*ks[t])), ks[t]


# ------------------------------------------------------------------------------------------------ through the product Trainer
def _cfg(dtype):
    from libcontinual_amd.config import Config
    cfg = Config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "lora_sub-vitb16-cifar100-b10x10.yaml")).get_config_dict()
    cfg["backbone"]["kwargs"].update({"pretrained": False, "img_size": 32, "patch_size": 8, "embed_dim": 64, "depth": 3, "num_heads": 2, "dtype": dtype,
                                      "lora_rank": 4})
    cfg["backbone"]["kwargs"].pop("model_name", None)
    cfg["classifier"]["kwargs"].update({"init_cls_num": 3, "inc_cls_num": 3, "task_num": 3, "embd_dim": 64})
    cfg["lr_scheduler"] = {"name": "CosineSchedule", "kwargs": {"K": 3}}
    cfg.update(dict(dataset="synthetic", image_size=32, total_cls_num=9, init_cls_num=3, inc_cls_num=3, task_num=3, epoch=3, init_epoch=3, batch_size=32,
                    val_per_epoch=1, testing_times=1, num_workers=0, save_path="", synthetic_per_class=64, synthetic_test_per_class=16, seed=5))
    cfg["optimizer"]["kwargs"]["lr"] = 0.004
    cfg.pop("train_trfms", None), cfg.pop("test_trfms", None)
    return cfg


def _train(dtype):
    from libcontinual_amd.trainer import Trainer
    os.environ.setdefault("PYTHONHASHSEED", "0")
    tr = Trainer(0, _cfg(dtype), log=lambda *a, **k: None)
    calls = []
    validate = tr._validate
    tr._validate = lambda t: (calls.append(t), validate(t))[1]
    out = tr.train_loop()
    torch.cuda.synchronize()
    return tr, out, calls


def test_three_tasks_through_the_trainer_reproducibly():
    tr, out, calls = _train("bf16")
    assert [h[:2] for h in tr.hook_trace if h[0] in ("before_task", "after_task")] == [(k, t) for t in range(3) for k in ("before_task", "after_task")]
    assert isinstance(tr.optimizer, ProjectedAdam) and tr.optimizer.transforms is tr.model.transforms and tr.model.transforms is not None
    assert calls == [0, 1, 2]                                                      # val_per_epoch = 1, and still only the per-task validation ran
    table = np.asarray(out["acc_table"])
    assert np.isfinite(table).all() and table[0, 0] > 100.0 / 3 + 10, table         # three classes: chance is 33 %
    assert tr.model._protos.shape == (9, 64) and len(tr.model.reserved_basis) == 3 and all(1 <= k <= 64 for k in tr.model.reserved_basis)
    a = tr.model.attention_modules[0]
    assert float(a.prev_k_weight.abs().max()) > 0 and not a.apply_lora
    tr2, out2, _ = _train("bf16")
    np.testing.assert_array_equal(table, np.asarray(out2["acc_table"]))
    s1, s2 = tr.model.state_dict(), tr2.model.state_dict()
    assert all(torch.equal(s1[k], s2[k]) for k in s1)                               # bitwise equal final parameters and prev buffers
    assert torch.equal(tr.model._protos, tr2.model._protos)
