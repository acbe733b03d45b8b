"""SD_LoRA on the HIP ViT executor (model/sd_lora.py, backbone/vit.py, csrc/sdlora.hip inside csrc/vit_plan.hip) on a real MI355X."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sdlora_ref as R                              # noqa: E402
import libcontinual_amd.model as M                  # noqa: E402
from libcontinual_amd import _lib, optim            # noqa: E402
from libcontinual_amd._lib import call              # noqa: E402

DEV = "cuda"
CFG = R.CFG


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def _backbone(dtype, attn="MultiHeadAttention_SDLoRA", rank=4):
    kw = {"lora_rank": rank} if rank else {}
    return M.vit_pt_imnet(pretrained=False, attn_layer=attn, img_size=CFG["img"], patch_size=CFG["patch"], embed_dim=CFG["dim"], depth=CFG["depth"],
                          num_heads=CFG["heads"], dtype=dtype, **kw)


def run_fixture(fix, dtype):
    """the method part of tests/golden/sdlora_tiny.npz through SD_LoRA: what `before_task` draws at random is overwritten with the reference's draws"""
    bb = _backbone(dtype)
    bb.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in fix.items() if k.startswith("m/w/")}, strict=True)
    model = M.SD_LoRA(bb.to(DEV), DEV, init_cls_num=R.INC, inc_cls_num=R.INC, task_num=2, init_mag=1.0, rank_reduction=[False, 4, 8, 8, 6],
                      knowledge_dist=[False, 9e-4], embd_dim=CFG["dim"])
    x = torch.from_numpy(fix["m/x_u8"]).float() / 255.0
    y = torch.from_numpy(fix["m/y"])
    out = {"losses": [], "preds": []}
    for t in range(2):
        model.before_task(t, None, None, None)
        named = dict(model._network.named_parameters())
        names = sorted(n for n, p in named.items() if p.requires_grad)
        assert names == [str(n) for n in fix[f"m/t{t}/trainable"]]
        with torch.no_grad():
            for n in names:
                named[n].copy_(torch.from_numpy(fix[f"m/t{t}/init/{n}"]).float())
        opt = optim.SGD(model.get_parameters(None), lr=R.LR, momentum=R.MOM)
        model.train()
        for s in range(3):
            pred, acc, loss = model.observe({"image": x[t, s].to(DEV), "label": y[t, s].to(DEV)})
            opt.zero_grad()
            loss.backward()
            opt.step()
            out["losses"].append(float(loss.detach()))
            out["preds"].append(pred.cpu().numpy())
            for n in names:
                out[f"t{t}/s{s}/{n}"] = named[n].detach().cpu().numpy().copy()
        model.after_task(t, None, None, None)
    out["losses"] = np.array(out["losses"]).reshape(2, 3)
    return out


def _deviations(got, fix):
    first = max(rel(got["losses"][t, :1], fix["m/losses"][t, :1]) for t in range(2))
    worst = (0.0, "")
    for k in got:
        if k.startswith("t"):
            worst = max(worst, (rel(got[k], fix["m/" + k]), k))
    return first, rel(got["losses"], fix["m/losses"]), worst


def test_sdlora_golden_f32(golden):
    """f32 mode against the fp64 run of the reference's SD_LoRA, at the tolerances tests/test_vit_parity_gpu.py::test_inflora_golden holds the same
    executor to: first losses 2e-4, all losses and every trained tensor (head, factors, magnitudes after each of the 2 x 3 steps) 5e-3."""
    fix = golden("sdlora_tiny")
    got = run_fixture(fix, "f32")
    first, losses, worst = _deviations(got, fix)
    print(f"SD_LoRA fixture f32: first losses {first:.2e}, all losses {losses:.2e}, worst trained tensor {worst[0]:.2e} ({worst[1]})")
    assert first < 2e-4
    assert losses < 5e-3
    np.testing.assert_array_equal(np.stack(got["preds"][:1]), fix["m/preds"][0, :1])
    assert worst[0] < 5e-3, worst


def test_sdlora_golden_bf16(golden):
    """bf16 mode, by the bf16 convention of tests/test_vit_parity_gpu.py (test_l2p_golden / test_inflora_golden): the first loss of a task 3e-2, all
    losses 0.1"""
    fix = golden("sdlora_tiny")
    got = run_fixture(fix, "bf16")
    first, losses, worst = _deviations(got, fix)
    print(f"SD_LoRA fixture bf16: first losses {first:.2e}, all losses {losses:.2e}, worst trained tensor {worst[0]:.2e} ({worst[1]})")
    assert first < 3e-2
    assert losses < 0.1
    assert all(np.isfinite(v).all() for k, v in got.items() if k.startswith("t"))


def test_first_step_gradients_against_restatement(golden):
    """one observe + backward in f32 mode: every gradient autograd receives from the executor against tests/sdlora_ref.py in fp64 on the same state
    (task 1 of the fixture: one past term, two magnitudes)"""
    fix = golden("sdlora_tiny")
    ref = R.Method({k[4:]: torch.from_numpy(v) for k, v in fix.items() if k.startswith("m/w/")})
    names0 = [str(n) for n in fix["m/t0/trainable"]]
    ref.start_task(0, {n: fix[f"m/t0/s2/{n}"] for n in names0})
    ref.end_task()
    names1 = [str(n) for n in fix["m/t1/trainable"]]
    ref.start_task(1, {n: fix[f"m/t1/init/{n}"] for n in names1})
    x = torch.from_numpy(fix["m/x_u8"]).double()[1, 0] / 255.0
    y = torch.from_numpy(fix["m/y"])[1, 0]
    loss = torch.nn.functional.cross_entropy(ref.logits(x)[:, R.INC:], y - R.INC)
    want = dict(zip(ref.train, torch.autograd.grad(loss, list(ref.train.values()))))
    bb = _backbone("f32")
    bb.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in fix.items() if k.startswith("m/w/")}, strict=True)
    model = M.SD_LoRA(bb.to(DEV), DEV, init_cls_num=R.INC, inc_cls_num=R.INC, task_num=2, init_mag=1.0, rank_reduction=[False, 4, 8, 8, 6],
                      knowledge_dist=[False, 9e-4], embd_dim=CFG["dim"])
    for t, src in ((0, "m/t0/s2/"), (1, "m/t1/init/")):
        model.before_task(t, None, None, None)
        named = dict(model._network.named_parameters())
        with torch.no_grad():
            for n in (names0 if t == 0 else names1):
                if t == 1 or "_list." in n:
                    named[n].copy_(torch.from_numpy(fix[src + n]).float())
        if t == 0:
            model.after_task(0, None, None, None)
    model._network.backbone.feat.sdlora_update_inv()                      # the past term was written after before_task computed its norms
    model.train()
    _, _, l = model.observe({"image": x.float().to(DEV), "label": y.to(DEV)})
    l.backward()
    assert abs(float(l) - float(loss)) < 2e-4 * abs(float(loss))
    for n in names1:
        d = rel(named[n].grad.cpu(), want[n])
        assert d < 5e-3, (n, d)
    assert float(named["backbone.feat.transformer.blocks.0.attn.mag_lora.0"].grad.abs()) > 0


# ------------------------------------------------------------------------------------------------ through the product Trainer
def _cfg(dtype):
    from libcontinual_amd.config import Config
    cfg = Config().get_config_dict()
    bb_kw = {"pretrained": False, "img_size": 32, "patch_size": 8, "embed_dim": 64, "depth": 2, "num_heads": 2, "dtype": dtype,
             "attn_layer": "MultiHeadAttention_SDLoRA", "lora_rank": 4}
    kw = {"dataset": "cifar100", "init_cls_num": 3, "inc_cls_num": 3, "task_num": 2, "embd_dim": 64, "init_mag": 1.0, "rank_reduction": [True, 1, 8, 3, 2],
          "knowledge_dist": [False, 9e-4]}
    cfg.update(dict(dataset="synthetic", image_size=32, init_cls_num=3, inc_cls_num=3, task_num=2, epoch=2, init_epoch=2, batch_size=32,
                    val_per_epoch=10, testing_times=1, num_workers=0, save_path="", synthetic_per_class=64, synthetic_test_per_class=16, seed=5,
                    backbone={"name": "vit_pt_imnet", "kwargs": bb_kw}, classifier={"name": "SD_LoRA", "kwargs": kw},
                    optimizer={"name": "SGD", "kwargs": {"lr": 0.05, "momentum": 0.9}}, lr_scheduler={"name": "Constant"}))
    return cfg


def _train(dtype):
    from libcontinual_amd.trainer import Trainer
    os.environ.setdefault("PYTHONHASHSEED", "0")
    tr = Trainer(0, _cfg(dtype), log=lambda *a, **k: None)
    out = tr.train_loop()
    torch.cuda.synchronize()
    return tr, out


def test_two_tasks_through_the_trainer_reproducibly():
    tr, out = _train("bf16")
    assert np.isfinite(out["acc_table"]).all()
    a = tr.model.attention_modules[0]
    assert [h.weight.shape[0] for h in a.lora_A_q_list] == [4, 3]                                    # rank reduction at task 1
    assert float(a.lora_B_q_list[1].weight.abs().max()) > 0 and float(a.lora_B_v_list[0].weight.abs().max()) > 0     # both terms were trained
    assert any(abs(float(p) - 1.0) > 1e-4 for p in a.mag_lora)                                       # and the magnitudes
    _, out2 = _train("bf16")
    np.testing.assert_array_equal(np.asarray(out["acc_table"]), np.asarray(out2["acc_table"]))


# ----------------------------------------------------------------------------------- the other attention layers are untouched
def _direct_features(bb, x, lora):
    """the features through the entry points the LoRA / plain backbones always used, on a handle of the test's own"""
    vt = bb.feat
    s = vt._ensure(torch.device(DEV, torch.cuda.current_device()))
    st = torch.cuda.current_stream().cuda_stream
    desc = _lib.VitDesc(vt.img_size, vt.patch_size, vt.embed_dim, vt.depth, vt.num_heads, vt.mlp_dim, vt.lora_rank, 0.0, 0, 0.0)
    h = _lib.lib().clhip_vit_create(C.byref(desc), _lib.BF16 if vt.compute_dtype == "bf16" else _lib.F32)
    assert h
    try:
        shadow = torch.empty(_lib.lib().clhip_vit_shadow_bytes(h), dtype=torch.uint8, device=DEV)
        ws = torch.empty(_lib.lib().clhip_vit_workspace_bytes(h, x.shape[0], 0, 0), dtype=torch.uint8, device=DEV)
        feat = torch.empty(x.shape[0], vt.embed_dim, device=DEV)
        call("clhip_vit_prep_weights", h, C.byref(s.cparams), shadow.data_ptr(), int(lora), 0, st)
        call("clhip_vit_forward", h, C.byref(s.cparams), shadow.data_ptr(), ws.data_ptr(), x.data_ptr(), x.shape[0], None, 0, 0, None, feat.data_ptr(), st)
        torch.cuda.synchronize()
    finally:
        _lib.lib().clhip_vit_destroy(h)
    return feat


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("attn", ["MultiHeadAttention", "MultiHeadAttention_LoRA"])
def test_other_attention_layers_bitwise_unchanged(attn, dtype):
    torch.manual_seed(3)
    lora = attn.endswith("LoRA")
    bb = _backbone(dtype, attn, 4 if lora else 0).to(DEV)
    if lora:
        for a in bb.feat.attention_modules():
            a.apply_lora = True
    x = torch.rand(5, 3, CFG["img"], CFG["img"], device=DEV)
    with torch.no_grad():
        got = bb(x)
    want = _direct_features(bb, x, lora)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert _lib.lib().clhip_vit_workspace_bytes(bb.feat._s.handle, 5, 0, 1) > 0
