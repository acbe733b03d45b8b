"""DualPrompt on the HIP ViT executor on a real MI355X: the executor's prefix mode with prefix lengths that differ between layers, odd ones among them
(csrc/vit_plan.hip with the prefix form of csrc/attn.hip), the plugin (model/dualprompt.py, backbone/vit.py with csrc/dual.hip) against
tests/golden/dual_tiny.npz, and a run through the product Trainer.

No new numbers: the executor tolerances are those tests/test_codaprompt_gpu.py holds this executor to (features 1e-4 in f32 and 4e-2 in bf16, dpk / dpv 2e-3
and 0.1, each relative to the tensor's max-abs), the method tolerances those of its test_codaprompt_golden_f32 / _bf16."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import coda_ref as CR                                # noqa: E402
import dual_ref as R                                 # noqa: E402
from oracle import vit as ov                         # noqa: E402
import libcontinual_amd.model as M                   # noqa: E402
from libcontinual_amd import optim                   # noqa: E402

DEV = "cuda"
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
POOLED = [n for n in R.names() if R.is_pooled(n)]


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
@pytest.mark.parametrize("lp", [[3, 3, 10, 10, 10, 0], [1, 0, 5, 0, 2, 0]], ids=["dualprompt", "sparse"])
def test_executor_with_mixed_prefix_lengths(lp, dim, dtype):
    """the reference config's lengths (g 6, e 20: 3 rows on blocks 0-1, 10 on blocks 2-4) and a sparse set with Lp 1 and unprompted blocks in between.
    dim 64 / 2 heads: head dim 32, the generic kernels; dim 128 / 2 heads: head dim 64, the MFMA kernels in bf16"""
    cfg = dict(img=32, patch=8, dim=dim, depth=6, heads=2, mlp=4 * dim)
    bb, W = _backbone(cfg, dtype, f"dual_exec{dim}")
    vt, B = bb.feat, 5
    g = torch.Generator().manual_seed(dim + lp[0])
    x = torch.rand(B, 3, 32, 32, generator=g)
    pk = [(0.5 * torch.randn(B, n, dim, generator=g)).to(TD[dtype]) if n else None for n in lp]
    pv = [(0.5 * torch.randn(B, n, dim, generator=g)).to(TD[dtype]) if n else None for n in lp]
    dfeat = torch.randn(B, dim, generator=g)
    W64 = {k: v.double() for k, v in W.items()}
    pre = {l: (pk[l].double().requires_grad_(True), pv[l].double().requires_grad_(True)) for l in range(6) if lp[l]}
    want = CR.prefixed_features(W64, x.double(), cfg, pre)
    grads = torch.autograd.grad((want * dfeat.double()).sum(), [t for l in sorted(pre) for t in pre[l]])
    with torch.no_grad():
        plain0 = vt._run_forward(x.to(DEV), None, 0, None).clone()
        dk, dv = [None if t is None else t.to(DEV) for t in pk], [None if t is None else t.to(DEV) for t in pv]
        feat = vt._run_forward(x.to(DEV), None, 1, None, prefix=(lp, dk, dv)).clone()
        got = vt._run_backward(dfeat.to(DEV), prefix_lp=lp)
        dpk, dpv = got["dpk"], got["dpv"]
        plain1 = vt._run_forward(x.to(DEV), None, 0, None).clone()
        torch.cuda.synchronize()
    assert torch.equal(plain0, plain1) and not torch.equal(plain0, feat)               # the mode switched off again: bit for bit the plain forward
    f_tol, g_tol = (1e-4, 2e-3) if dtype == "f32" else (4e-2, 0.1)
    d = rel(feat.cpu(), want.detach())
    print(f"prefix executor Lp {lp} dim {dim} {dtype}: features {d:.2e}")
    assert d < f_tol
    for l in range(6):
        assert (dpk[l] is None) == (lp[l] == 0) and (dpv[l] is None) == (lp[l] == 0)
    for i, l in enumerate(sorted(pre)):
        assert tuple(dpk[l].shape) == (B, lp[l], dim)
        a, b = rel(dpk[l].cpu(), grads[2 * i]), rel(dpv[l].cpu(), grads[2 * i + 1])
        print(f"  layer {l}: dpk {a:.2e} dpv {b:.2e}")
        assert a < g_tol and b < g_tol, (l, a, b)


# --------------------------------------------------------------------------------------------------------------- method
def run_fixture(fix, dtype):
    """tests/golden/dual_tiny.npz through M.DualPrompt: the pool and the regrown head are overwritten with the reference's draws"""
    bb, _ = _backbone(R.CFG, dtype, str(fix["w_tag"]))
    model = M.DualPrompt(bb, DEV, init_cls_num=R.INC, inc_cls_num=R.INC, task_num=R.TASKS, num_class=R.INC * R.TASKS, feat_dim=R.CFG["dim"],
                         g_prompt_length=R.LG, e_prompt_length=R.LE).to(DEV)
    pool = model.network.backbone.prompt
    assert [k for k, _ in pool.named_parameters()] == R.names()
    with torch.no_grad():
        for k, v in pool.named_parameters():
            v.copy_(torch.from_numpy(fix["pool0/" + k]))
    x = torch.from_numpy(fix["x_u8"]).float() / 255.0
    xi = torch.from_numpy(fix["infer_x_u8"]).float() / 255.0
    y = torch.from_numpy(fix["y"])
    out = {"losses": [], "key_losses": [], "preds": [], "infer": [], "infer_idx": [], "infer_cos": [], "infer_logits": []}
    for t in range(R.TASKS):
        model.before_task(t, None, None, None)
        head = model.network.classifier
        with torch.no_grad():
            head.weight.copy_(torch.from_numpy(fix[f"t{t}/init/classifier.weight"]).float())
            head.bias.copy_(torch.from_numpy(fix[f"t{t}/init/classifier.bias"]).float())
        start = {k: v.detach().clone() for k, v in pool.named_parameters()}
        opt = optim.Adam(model.get_parameters(None), lr=R.LR, betas=R.BETAS, weight_decay=0)
        model.train()
        for s in range(R.STEPS):
            pred, acc, loss = model.observe({"image": x[t, s].to(DEV), "label": y[t, s].to(DEV)})
            opt.zero_grad()
            loss.backward()
            opt.step()
            out["losses"].append(float(loss.detach()))
            out["key_losses"].append(float(model._last_key_loss))
            out["preds"].append(pred.cpu().numpy())
            assert bool((pool.last_idx == t).all())
            for k, v in pool.named_parameters():
                v = v.detach()
                if R.is_pooled(k):
                    others = [r for r in range(R.POOL) if r != t]
                    assert torch.equal(v[others], start[k][others]), (t, s, k)              # rows other than task_id: bit-unchanged within a task
                    assert not torch.equal(v[t], start[k][t]), (t, s, k)
                    v = v[t]
                out[f"t{t}/s{s}/{k}"] = v.cpu().numpy().copy()
            out[f"t{t}/s{s}/classifier.weight"] = head.weight.detach().cpu().numpy().copy()
            out[f"t{t}/s{s}/classifier.bias"] = head.bias.detach().cpu().numpy().copy()
        model.after_task(t, None, None, None)
        model.eval()
        with torch.no_grad():
            logits = model.network(xi.to(DEV), train=False)
        out["infer_logits"].append(logits.cpu().numpy())
        out["infer_idx"].append(pool.last_idx.cpu().numpy().copy())
        out["infer_cos"].append(pool.last_cos.cpu().numpy().copy())
        out["infer"].append(model.inference({"image": xi.to(DEV), "label": torch.zeros(R.INFER, dtype=torch.long, device=DEV)})[0].cpu().numpy())
        np.testing.assert_array_equal(out["infer"][-1], out["infer_logits"][-1].argmax(1))
    out["losses"] = np.array(out["losses"]).reshape(R.TASKS, R.STEPS)
    out["key_losses"] = np.array(out["key_losses"]).reshape(R.TASKS, R.STEPS)
    return out


def _deviations(got, fix):
    first = max(rel(got["losses"][t, :1], fix["losses"][t, :1]) for t in range(R.TASKS))
    worst = max((rel(v, fix[k]), k) for k, v in got.items() if k.startswith("t"))
    sel = float(np.mean(np.stack(got["infer_idx"]) == fix["infer_idx"]))
    agree = float(np.mean(np.stack(got["infer"]) == fix["infer_preds"]))
    return first, rel(got["losses"], fix["losses"]), rel(got["key_losses"], fix["key_losses"]), worst, sel, agree


def test_dualprompt_golden_f32(golden):
    """f32 mode against the fp64 run of the reference's DualPrompt: first losses 2e-4, all losses, key losses and every trained tensor (8 pool tensors and
    the head after each of the 3 x 3 Adam steps) 5e-3 of its max-abs, the first step's predictions equal, rows other than task_id bit-unchanged (asserted
    in run_fixture).  Inference after every task selects the fixture's rows for ALL samples (the fixture's top-two cosine gap is >= 1e-3, the f32 query
    deviates by 1e-4 of max-abs); predictions are compared on the samples dual_ref.comparable keeps: those whose fp64 logit margin exceeds 5e-3 of the
    task's largest |logit|, the deviation this test allows the trained tensors (tests/test_dual_cpu.py: at most 2 of 12 are left out per task)."""
    fix = golden("dual_tiny")
    got = run_fixture(fix, "f32")
    first, losses, key_losses, worst, sel, agree = _deviations(got, fix)
    cosd = float(np.abs(np.stack(got["infer_cos"]) - fix["infer_cos"]).max())
    print(f"DualPrompt fixture f32: first losses {first:.2e}, all losses {losses:.2e}, key losses {key_losses:.2e}, worst trained tensor {worst[0]:.2e} "
          f"({worst[1]}), inference cosines off by {cosd:.2e}, selections agreeing {sel:.2f}, predictions agreeing {agree:.2f}")
    assert first < 2e-4
    assert losses < 5e-3 and key_losses < 5e-3
    for t in range(R.TASKS):
        np.testing.assert_array_equal(got["preds"][t * R.STEPS], fix["preds"][t, 0])
    assert worst[0] < 5e-3, worst
    np.testing.assert_array_equal(np.stack(got["infer_idx"]), fix["infer_idx"])
    for t in range(R.TASKS):
        ok = R.comparable(fix, t)
        assert int(ok.sum()) >= R.INFER - 2
        np.testing.assert_array_equal(got["infer"][t][ok], fix["infer_preds"][t][ok])


def test_dualprompt_golden_bf16(golden):
    """bf16 mode, by the bf16 convention of test_codaprompt_golden_bf16: the first loss of a task 3e-2, all losses 0.1, everything finite; the agreement
    of the selections is printed, not gated"""
    fix = golden("dual_tiny")
    got = run_fixture(fix, "bf16")
    first, losses, key_losses, worst, sel, agree = _deviations(got, fix)
    print(f"DualPrompt fixture bf16: first losses {first:.2e}, all losses {losses:.2e}, key losses {key_losses:.2e}, worst trained tensor {worst[0]:.2e} "
          f"({worst[1]}), selections agreeing {sel:.2f}, predictions agreeing {agree:.2f}")
    assert first < 3e-2
    assert losses < 0.1
    assert all(np.isfinite(v).all() for k, v in got.items() if k.startswith("t"))
    assert np.isfinite(np.stack(got["infer_cos"])).all()


# ------------------------------------------------------------------------------------------------ through the product Trainer
def _cfg(dtype):
    from libcontinual_amd.config import Config
    cfg = Config().get_config_dict()
    bb_kw = {"pretrained": False, "img_size": 32, "patch_size": 8, "embed_dim": 64, "depth": 6, "num_heads": 2, "dtype": dtype}
    kw = {"num_class": 9, "task_num": 3, "init_cls_num": 3, "inc_cls_num": 3, "feat_dim": 64, "g_prompt_length": 6, "e_prompt_length": 8}
    cfg.update(dict(dataset="synthetic", image_size=32, init_cls_num=3, inc_cls_num=3, task_num=3, epoch=2, init_epoch=2, batch_size=32,
                    val_per_epoch=10, testing_times=1, num_workers=0, save_path="", synthetic_per_class=32, synthetic_test_per_class=16, seed=5,
                    backbone={"name": "vit_pt_imnet", "kwargs": bb_kw}, classifier={"name": "DualPrompt", "kwargs": kw},
                    optimizer={"name": "Adam", "kwargs": {"lr": 0.001, "betas": [0.9, 0.999], "weight_decay": 0}},
                    lr_scheduler={"name": "MultiStepLR", "kwargs": {"gamma": 0.1, "milestones": [80, 120]}}))
    return cfg


def _train(dtype):
    from libcontinual_amd.trainer import Trainer
    os.environ.setdefault("PYTHONHASHSEED", "0")
    tr = Trainer(0, _cfg(dtype), log=lambda *a, **k: None)
    pool = tr.model.network.backbone.prompt
    init = {k: v.detach().clone() for k, v in pool.named_parameters()}
    out = tr.train_loop()
    torch.cuda.synchronize()
    return tr, out, init


def test_three_tasks_through_the_trainer_reproducibly():
    """the toy counterpart of config/dualprompt-vitb16-cifar100-b10x10.yaml (same optimizer and scheduler; a 6-block ViT of width 64)"""
    tr, out, init = _train("bf16")
    assert np.isfinite(out["acc_table"]).all()
    pool = tr.model.network.backbone.prompt
    assert tr.model.network.classifier.out_features == 9 and tr.model.network.backbone.task_id == 2
    assert not torch.equal(pool.g_p_0.detach(), init["g_p_0"])
    for n in POOLED:
        v = getattr(pool, n).detach()
        assert all(not torch.equal(v[r], init[n][r]) for r in range(3)), n                   # one row per task trained ...
        assert torch.equal(v[3:], init[n][3:]), n                                            # ... and nothing else: bit-equal to the initial draw
    _, out2, _ = _train("bf16")
    np.testing.assert_array_equal(np.asarray(out["acc_table"]), np.asarray(out2["acc_table"]))
