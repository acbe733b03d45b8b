"""CODA-Prompt on the HIP ViT executor on a real MI355X: the executor's prefix mode (csrc/vit_plan.hip with the prefix form of csrc/attn.hip), the plugin
(model/codaprompt.py, backbone/vit.py with csrc/coda.hip) against tests/golden/coda_tiny.npz, and a run through the product Trainer.

Executor tolerances are the numbers the suite already holds this executor to (tests/test_vit_parity_gpu.py): block activations 1e-4 in f32 and 4e-2 in bf16
(test_vit_layer_activations_vs_oracle), first-step gradients 2e-3 in f32 (test_l2p_golden) and 0.1 in bf16 (its grad_cls_w0), each relative to the
tensor's max-abs.  Method tolerances are those tests/test_sdlora_gpu.py takes from test_inflora_golden."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import coda_ref as R                                 # noqa: E402
from oracle import vit as ov                         # noqa: E402
import libcontinual_amd.model as M                   # noqa: E402
from libcontinual_amd import optim                   # noqa: E402

DEV = "cuda"
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
LP = [4, 4, 4, 4, 4, 0]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def _backbone(cfg, dtype, tag):
    bb = M.vit_pt_imnet(pretrained=False, img_size=cfg["img"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
                        dtype=dtype)
    W = ov.det_params(cfg, tag)
    bb.load_state_dict(W, strict=True)
    return bb.to(DEV), W


# ------------------------------------------------------------------------------------------------------------- executor
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("dim", [64, 128])
def test_executor_prefix_mode_against_restatement(dim, dtype):
    """dim 64 / 2 heads: head dim 32, the generic kernels; dim 128 / 2 heads: head dim 64, the MFMA kernels in bf16.  Depth 6, Lp = 4 on layers 0-4"""
    cfg = dict(img=32, patch=8, dim=dim, depth=6, heads=2, mlp=4 * dim)
    bb, W = _backbone(cfg, dtype, f"coda_exec{dim}")
    vt, B = bb.feat, 5
    g = torch.Generator().manual_seed(dim)
    x = torch.rand(B, 3, 32, 32, generator=g)
    pk = [(0.5 * torch.randn(B, n, dim, generator=g)).to(TD[dtype]) if n else None for n in LP]
    pv = [(0.5 * torch.randn(B, n, dim, generator=g)).to(TD[dtype]) if n else None for n in LP]
    dfeat = torch.randn(B, dim, generator=g)
    W64 = {k: v.double() for k, v in W.items()}
    pre = {l: (pk[l].double().requires_grad_(True), pv[l].double().requires_grad_(True)) for l in range(6) if LP[l]}
    want = R.prefixed_features(W64, x.double(), cfg, pre)
    grads = torch.autograd.grad((want * dfeat.double()).sum(), [t for l in sorted(pre) for t in pre[l]])
    with torch.no_grad():
        plain0 = vt._run_forward(x.to(DEV), None, 0, None).clone()
        dk, dv = [None if t is None else t.to(DEV) for t in pk], [None if t is None else t.to(DEV) for t in pv]
        feat = vt._run_forward(x.to(DEV), None, 1, None, prefix=(LP, dk, dv)).clone()
        got = vt._run_backward(dfeat.to(DEV), prefix_lp=LP)
        dpk, dpv = got["dpk"], got["dpv"]
        plain1 = vt._run_forward(x.to(DEV), None, 0, None).clone()
        torch.cuda.synchronize()
    assert torch.equal(plain0, plain1) and not torch.equal(plain0, feat)               # the mode switched off again: bit for bit the plain forward
    f_tol, g_tol = (1e-4, 2e-3) if dtype == "f32" else (4e-2, 0.1)
    d = rel(feat.cpu(), want.detach())
    print(f"prefix executor dim {dim} {dtype}: features {d:.2e}")
    assert d < f_tol
    assert dpk[5] is None and dpv[5] is None
    for i, l in enumerate(sorted(pre)):
        a, b = rel(dpk[l].cpu(), grads[2 * i]), rel(dpv[l].cpu(), grads[2 * i + 1])
        print(f"  layer {l}: dpk {a:.2e} dpv {b:.2e}")
        assert a < g_tol and b < g_tol, (l, a, b)


def test_plain_backward_refuses_a_prefixed_forward_and_vice_versa():
    cfg = dict(img=32, patch=8, dim=64, depth=6, heads=2, mlp=256)
    bb, _ = _backbone(cfg, "f32", "coda_exec64")
    vt = bb.feat
    x = torch.rand(2, 3, 32, 32, device=DEV)
    pre = [torch.zeros(2, n, 64, device=DEV) if n else None for n in LP]
    from libcontinual_amd._lib import ClhipError
    with torch.no_grad():
        vt._run_forward(x, None, 1, None, prefix=(LP, pre, pre))
        with pytest.raises(ClhipError):
            vt._run_backward(torch.zeros(2, 64, device=DEV))
        vt._run_forward(x, None, 1, None)
        with pytest.raises(ClhipError):
            vt._run_backward(torch.zeros(2, 64, device=DEV), prefix_lp=LP)


# --------------------------------------------------------------------------------------------------------------- method
def run_fixture(fix, dtype):
    """tests/golden/coda_tiny.npz through M.CodaPrompt: the pool and the regrown head are overwritten with the reference's draws"""
    bb, _ = _backbone(R.CFG, dtype, str(fix["w_tag"]))
    model = M.CodaPrompt(bb, DEV, init_cls_num=R.INC, inc_cls_num=R.INC, task_num=R.TASKS, num_class=R.INC * R.TASKS, feat_dim=R.CFG["dim"],
                         pool_size=R.POOL, prompt_length=R.LENGTH, mu=0.0).to(DEV)
    pool = model.network.backbone.prompt
    with torch.no_grad():
        for k, v in pool.named_parameters():
            v.copy_(torch.from_numpy(fix["pool0/" + k]))
    x = torch.from_numpy(fix["x_u8"]).float() / 255.0
    xi = torch.from_numpy(fix["infer_x_u8"]).float() / 255.0
    y = torch.from_numpy(fix["y"])
    out = {"losses": [], "preds": [], "infer": []}
    for t in range(R.TASKS):
        model.before_task(t, None, None, None)
        head = model.network.classifier
        with torch.no_grad():
            head.weight.copy_(torch.from_numpy(fix[f"t{t}/init/classifier.weight"]).float())
            head.bias.copy_(torch.from_numpy(fix[f"t{t}/init/classifier.bias"]).float())
        opt = optim.Adam(model.get_parameters(None), lr=R.LR, betas=R.BETAS, weight_decay=0)
        model.train()
        for s in range(R.STEPS):
            pred, acc, loss = model.observe({"image": x[t, s].to(DEV), "label": y[t, s].to(DEV)})
            opt.zero_grad()
            loss.backward()
            opt.step()
            out["losses"].append(float(loss.detach()))
            out["preds"].append(pred.cpu().numpy())
            for k, v in pool.named_parameters():
                out[f"t{t}/s{s}/{k}"] = v.detach()[:R.POOL // R.TASKS].cpu().numpy().copy()
                assert bool((v.detach()[R.POOL // R.TASKS:] == 0).all())
            out[f"t{t}/s{s}/classifier.weight"] = head.weight.detach().cpu().numpy().copy()
            out[f"t{t}/s{s}/classifier.bias"] = head.bias.detach().cpu().numpy().copy()
        model.after_task(t, None, None, None)
        model.eval()
        out["infer"].append(model.inference({"image": xi.to(DEV), "label": torch.zeros(12, dtype=torch.long, device=DEV)})[0].cpu().numpy())
    out["losses"] = np.array(out["losses"]).reshape(R.TASKS, R.STEPS)
    assert pool.task_count == 0
    return out


def _deviations(got, fix):
    first = max(rel(got["losses"][t, :1], fix["losses"][t, :1]) for t in range(R.TASKS))
    worst = max((rel(v, fix[k]), k) for k, v in got.items() if k.startswith("t"))
    agree = float(np.mean(np.stack(got["infer"]) == fix["infer_preds"]))
    return first, rel(got["losses"], fix["losses"]), worst, agree


def test_codaprompt_golden_f32(golden):
    """f32 mode against the fp64 run of the reference's CodaPrompt: first losses 2e-4, all losses and every trained tensor (15 pool tensors and the
    head after each of the 2 x 3 Adam steps) 5e-3 of its max-abs, the first step's predictions equal"""
    fix = golden("coda_tiny")
    got = run_fixture(fix, "f32")
    first, losses, worst, agree = _deviations(got, fix)
    print(f"CodaPrompt fixture f32: first losses {first:.2e}, all losses {losses:.2e}, worst trained tensor {worst[0]:.2e} ({worst[1]}), "
          f"inference predictions agreeing {agree:.2f}")
    assert first < 2e-4
    assert losses < 5e-3
    np.testing.assert_array_equal(np.stack(got["preds"][:1]), fix["preds"][0, :1])
    assert worst[0] < 5e-3, worst


def test_codaprompt_golden_bf16(golden):
    """bf16 mode, by the bf16 convention of tests/test_sdlora_gpu.py: the first loss of a task 3e-2, all losses 0.1, everything finite"""
    fix = golden("coda_tiny")
    got = run_fixture(fix, "bf16")
    first, losses, worst, agree = _deviations(got, fix)
    print(f"CodaPrompt fixture bf16: first losses {first:.2e}, all losses {losses:.2e}, worst trained tensor {worst[0]:.2e} ({worst[1]}), "
          f"inference predictions agreeing {agree:.2f}")
    assert first < 3e-2
    assert losses < 0.1
    assert all(np.isfinite(v).all() for k, v in got.items() if k.startswith("t"))


# ------------------------------------------------------------------------------------------------ through the product Trainer
def _cfg(dtype):
    from libcontinual_amd.config import Config
    cfg = Config().get_config_dict()
    bb_kw = {"pretrained": False, "img_size": 32, "patch_size": 8, "embed_dim": 64, "depth": 6, "num_heads": 2, "dtype": dtype}
    kw = {"num_class": 6, "task_num": 2, "init_cls_num": 3, "inc_cls_num": 3, "feat_dim": 64, "prompt_length": 8, "pool_size": 6, "mu": 0.0}
    cfg.update(dict(dataset="synthetic", image_size=32, init_cls_num=3, inc_cls_num=3, task_num=2, epoch=2, init_epoch=2, batch_size=32,
                    val_per_epoch=10, testing_times=1, num_workers=0, save_path="", synthetic_per_class=64, synthetic_test_per_class=16, seed=5,
                    backbone={"name": "vit_pt_imnet", "kwargs": bb_kw}, classifier={"name": "CodaPrompt", "kwargs": kw},
                    optimizer={"name": "Adam", "kwargs": {"lr": 0.001, "betas": [0.9, 0.999], "weight_decay": 0}},
                    lr_scheduler={"name": "CosineSchedule", "kwargs": {"K": 2}}))
    return cfg


def _train(dtype):
    from libcontinual_amd.trainer import Trainer
    os.environ.setdefault("PYTHONHASHSEED", "0")
    tr = Trainer(0, _cfg(dtype), log=lambda *a, **k: None)
    out = tr.train_loop()
    torch.cuda.synchronize()
    return tr, out


def test_two_tasks_through_the_trainer_reproducibly():
    """the toy counterpart of config/codaprompt-vitb16-cifar100-b10x10.yaml (same method kwargs, optimizer and scheduler; a 6-block ViT of width 64)"""
    tr, out = _train("bf16")
    assert np.isfinite(out["acc_table"]).all()
    pool = tr.model.network.backbone.prompt
    assert pool.task_count == 0 and tr.model.network.classifier.out_features == 6
    k = pool.e_k_0.detach()
    assert bool((k[3:] == 0).all()) and abs(float(k[0].norm()) - 1.0) > 1e-4                      # the window trained, nothing beyond it moved
    _, out2 = _train("bf16")
    np.testing.assert_array_equal(np.asarray(out["acc_table"]), np.asarray(out2["acc_table"]))
