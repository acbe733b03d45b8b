"""RanPAC's first session on the MI355X: the adapter ViT inside the executor (forward, backward, dropout), `RanPAC.observe` on task 0, the Trainer.

Tiny ViT: img 32, patch 8, D 64, depth 2, 2 heads, R 16; batch 3 -> M = 51 token rows (a ragged 32-row tile).

Yardsticks.  fp32: the same computation in fp32 torch on the CPU, measured here against fp64; the device may be 4 x that far (the rule of
tests/test_ranpac_gpu.py: another, equally valid summation order).  bf16: the relative deviation, measured here, of the prompt-token gradient that
`features(x, tokens)` already returned before adapters existed, on this model in bf16 against fp64; the adapter gradients may deviate 2 x that
(the same backward chain with one more bf16-rounded product on each side).
"""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import adapter_ref as A
from oracle import vit as OV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
KW = dict(pretrained=False, img_size=32, patch_size=8, embed_dim=64, depth=2, num_heads=2)
KINDS = ("down_w", "down_b", "up_w", "up_b")


def _P():
    return OV.det_params(A.TINY, "first_session", dtype=torch.float64)


def _backbone(dtype, adapters, dropout=0.0, trained=True):
    """ViTZoo on the device holding _P(); adapters: None (plain, block eps 1e-6 like the adapter tree) or a seed for random non-zero ones"""
    import libcontinual_amd.model as M
    kw = dict(KW, dtype=dtype)
    if adapters is not None:
        kw.update(ffn_adapt=True, ffn_num=A.R_TINY, ffn_adapter_scalar=A.SCALE, adapter_dropout=dropout)
    bb = M.vit_pt_imnet_in21k_adapter(**kw)
    if adapters is None:
        bb.feat.block_ln_eps = 1e-6
    missing, unexpected = bb.load_state_dict({k: v.float() for k, v in _P().items()}, strict=False)
    assert not unexpected and all(".adaptmlp." in k for k in missing)
    ad = None
    if adapters is not None and trained:
        ad = [A.adapter_params(64, A.R_TINY, adapters + i) for i in range(2)]
        with torch.no_grad():
            for blk, layer in zip(bb.feat.transformer.blocks, ad):
                for t, v in zip(blk.adaptmlp.tensors(), layer):
                    t.copy_(v.float())
        ad = [[t.float().double() for t in layer] for layer in ad]
    return bb.to(DEV), ad


def _batch(seed=1):
    g = A.gen(seed)
    return torch.randn(3, 3, 32, 32, generator=g, dtype=torch.float64).float(), torch.randn(3, 64, generator=g, dtype=torch.float64).float()


def _masks(bb, M):
    from libcontinual_amd._lib import call
    seed = bb.feat.last_dropout_seed
    assert seed is not None and seed.is_cuda and seed.dtype == torch.int64
    out = []
    for layer in range(2):
        m = torch.empty(M, A.R_TINY, dtype=torch.uint8, device=DEV)
        call("clhip_adapter_dropout_mask", seed.data_ptr(), layer, M, A.R_TINY, bb.feat.adapter_dropout, m.data_ptr(), torch.cuda.current_stream().cuda_stream)
        out.append(m.cpu())
    return out


def _ref(ad, img, wt, masks, p, dtype):
    """features and adapter gradients of sum(features * wt) from the restatement in `dtype` on the CPU"""
    P = {k: v.to(dtype) for k, v in _P().items()}
    Ad = [[t.to(dtype).clone().requires_grad_(True) for t in layer] for layer in ad]
    f = A.vit_features(P, Ad, img.to(dtype), masks=masks, p=p)
    (f * wt.to(dtype)).sum().backward()
    return f.detach().double(), {k: torch.cat([layer[i].grad.double().reshape(-1) for layer in Ad]) for i, k in enumerate(KINDS)}


def _device(bb, img, wt):
    f = bb.feat.features(img.to(DEV))
    (f * wt.to(DEV)).sum().backward()
    grads = {k: torch.cat([blk.adaptmlp.tensors()[i].grad.double().cpu().reshape(-1) for blk in bb.feat.transformer.blocks]) for i, k in enumerate(KINDS)}
    for t in bb.feat.adapter_tensors():
        t.grad = None
    return f.detach().double().cpu(), grads


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_initial_adapters_are_the_identity(dtype):
    plain, _ = _backbone(dtype, None)
    fresh, _ = _backbone(dtype, 0, dropout=0.1, trained=False)
    img, _ = _batch()
    plain.eval()
    with torch.no_grad():
        want = plain.feat.features(img.to(DEV))
        for mode in (fresh.eval, fresh.train):
            mode()
            assert torch.equal(fresh.feat.features(img.to(DEV)), want)
    assert fresh.feat.last_dropout_seed is not None                    # the training-mode pass did run with dropout on
    # with grad: a saved forward gives the same bits, and a frozen adapter backbone saves nothing
    fresh.eval()
    assert torch.equal(fresh.feat.features(img.to(DEV)).detach(), want)
    for t in fresh.feat.adapter_tensors():
        t.requires_grad_(False)
    out = fresh.feat.features(img.to(DEV))
    assert not out.requires_grad and torch.equal(out, want)
    torch.cuda.synchronize()


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_forward_backward_f32(p):
    bb, ad = _backbone("f32", 20, dropout=p)
    img, wt = _batch()
    bb.train()
    f, g = _device(bb, img, wt)
    masks = _masks(bb, 51) if p > 0 else None
    assert p > 0 or bb.feat.last_dropout_seed is None
    f64, g64 = _ref(ad, img, wt, masks, p, torch.float64)
    f32, g32 = _ref(ad, img, wt, masks, p, torch.float32)
    rows = [("features", f, f64, f32)] + [(k, g[k], g64[k], g32[k]) for k in KINDS]
    rows.append(("all adapter gradients", torch.cat([g[k] for k in KINDS]), torch.cat([g64[k] for k in KINDS]), torch.cat([g32[k] for k in KINDS])))
    for name, dev, r64, r32 in rows:
        e_dev, e_cpu = float((dev - r64).norm()), float((r32 - r64).norm())
        print(f"f32 p={p} {name}: |device - fp64| {e_dev:.3e}, fp32 CPU {e_cpu:.3e}, ratio {e_dev / e_cpu:.3f} (|fp64| {float(r64.norm()):.3e})")
        assert e_dev <= 4 * e_cpu, name
    # eval mode: no dropout, no seed
    bb.eval()
    f_eval, _ = _device(bb, img, wt)
    assert bb.feat.last_dropout_seed is None
    if p > 0:
        assert not torch.equal(f_eval, f)
        bb.train()
        f2, _ = _device(bb, img, wt)
        assert not torch.equal(f2, f)                                   # a fresh seed per forward
    torch.cuda.synchronize()


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_forward_backward_bf16(p):
    img, wt = _batch()
    # the yardstick: the prompt-token gradient of the adapter-free model, bf16 against fp64
    plain, _ = _backbone("bf16", None)
    g = A.gen(9)
    tok = (torch.randn(2, 64, generator=g, dtype=torch.float64) * 0.2).float()
    tdev = tok.to(DEV).requires_grad_(True)
    (plain.feat.features(img.to(DEV), tdev) * wt.to(DEV)).sum().backward()
    t64 = tok.double().requires_grad_(True)
    (A.vit_features(_P(), None, img.double(), prompt=t64) * wt.double()).sum().backward()
    yard = float((tdev.grad.double().cpu() - t64.grad).norm() / t64.grad.norm())
    bb, ad = _backbone("bf16", 20, dropout=p)
    bb.train()
    f, gd = _device(bb, img, wt)
    masks = _masks(bb, 51) if p > 0 else None
    f64, g64 = _ref(ad, img, wt, masks, p, torch.float64)
    rel = {k: float((gd[k] - g64[k]).norm() / g64[k].norm()) for k in KINDS}
    cat = lambda d: torch.cat([d[k] for k in KINDS])
    rel["all"] = float((cat(gd) - cat(g64)).norm() / cat(g64).norm())
    print(f"bf16 p={p}: prompt-token gradient off fp64 by {yard:.3e} (relative); adapter gradients: "
          + ", ".join(f"{k} {v:.3e} ({v / yard:.2f} x)" for k, v in rel.items())
          + f"; features {float((f - f64).norm() / f64.norm()):.3e}")
    for k, v in rel.items():
        assert v <= 2 * yard, (k, v, yard)
    torch.cuda.synchronize()


def _restated_steps(ad, head_w, sigma, batches, dtype, lr, mu, wd):
    P = {k: v.to(dtype) for k, v in _P().items()}
    Ad = [[t.to(dtype).clone().requires_grad_(True) for t in layer] for layer in ad]
    W, sg = head_w.to(dtype).clone().requires_grad_(True), sigma.to(dtype).clone().requires_grad_(True)
    opt = A.SGD([t for layer in Ad for t in layer] + [W, sg], lr, mu, wd)
    losses = []
    for x, y in batches:
        loss = F.cross_entropy(A.cosine_logits(A.vit_features(P, Ad, x.to(dtype)), W, sg), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.array(losses), [t.detach().double() for layer in Ad for t in layer] + [W.detach().double(), sg.detach().double()]


def test_three_sgd_steps_of_observe():
    import libcontinual_amd.model as M
    from libcontinual_amd import optim
    from libcontinual_amd.trainer import _backward
    bb, ad = _backbone("f32", 30, dropout=0.0)
    model = M.RanPAC(bb, DEV, first_session_training=True, M=32, init_cls_num=4, inc_cls_num=3, task_num=2, total_cls_num=7)
    model.before_task(0, None, None, None)
    head = model._network.classifier
    hw, sg = head.weight.detach().double().cpu(), head.sigma.detach().double().cpu()
    g = A.gen(4)
    batches = [(torch.randn(3, 3, 32, 32, generator=g), torch.randint(0, 4, (3,), generator=g)) for _ in range(3)]
    lr, mu, wd = 0.05, 0.9, 5e-4
    frozen = {k: v.detach().clone() for k, v in model.named_parameters() if not v.requires_grad}
    assert len(frozen) > 0 and sum(v.requires_grad for v in model.parameters()) == 8 + 2
    opt = optim.SGD(model.get_parameters({}), lr=lr, momentum=mu, weight_decay=wd)
    model.train()
    losses = []
    for x, y in batches:
        pred, acc, loss = model.observe({"image": x, "label": y})
        assert tuple(pred.shape) == (3,) and 0.0 <= float(acc) <= 1.0
        opt.zero_grad()
        _backward(loss)
        opt.step()
        losses.append(float(loss.detach()))
    got = [t.detach().double().cpu() for t in bb.feat.adapter_tensors()] + [head.weight.detach().double().cpu(), head.sigma.detach().double().cpu()]
    l64, p64 = _restated_steps(ad, hw, sg, batches, torch.float64, lr, mu, wd)
    l32, p32 = _restated_steps(ad, hw, sg, batches, torch.float32, lr, mu, wd)
    e_dev, e_cpu = np.abs(np.array(losses) - l64).max(), np.abs(l32 - l64).max()
    print(f"losses {losses} (fp64 {l64.tolist()}): off by {e_dev:.3e}, fp32 CPU {e_cpu:.3e}")
    assert e_dev <= 4 * e_cpu
    cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
    for name, sl in (("adapters", slice(0, 8)), ("head", slice(8, 10))):
        d_dev, d_cpu = float((cat(got[sl]) - cat(p64[sl])).norm()), float((cat(p32[sl]) - cat(p64[sl])).norm())
        moved = float((cat(p64[sl]) - cat([t for layer in ad for t in layer] if name == "adapters" else [hw, sg])).norm())
        print(f"{name} after 3 steps: |device - fp64| {d_dev:.3e}, fp32 CPU {d_cpu:.3e}, ratio {d_dev / d_cpu:.3f}; moved by {moved:.3e}")
        assert moved > 100 * d_cpu and d_dev <= 4 * d_cpu
    assert all(torch.equal(v.detach(), frozen[k]) for k, v in model.named_parameters() if k in frozen)
    torch.cuda.synchronize()


def _cfg():
    from libcontinual_amd.config import Config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        cfg = Config(os.path.join(ROOT, "config", "ranpac-vitb16-cifar100-b10x10-fst.yaml")).get_config_dict()
    finally:
        os.chdir(cwd)
    cfg.pop("train_trfms"), cfg.pop("test_trfms")
    assert cfg["classifier"]["kwargs"]["first_session_training"] is True and cfg["backbone"]["kwargs"]["ffn_adapt"] is True
    cfg["backbone"]["kwargs"] = {"pretrained": False, "img_size": 32, "patch_size": 8, "embed_dim": 64, "depth": 2, "num_heads": 2, "dtype": "f32",
                                 "ffn_adapt": True, "ffn_num": 16, "ffn_adapter_scalar": 0.1, "adapter_dropout": 0.1}
    cfg["classifier"]["kwargs"].update(M=100, init_cls_num=4, inc_cls_num=3, task_num=2, total_cls_num=7)
    cfg.update(dataset="synthetic", image_size=32, init_cls_num=4, inc_cls_num=3, task_num=2, total_cls_num=7, init_epoch=3, epoch=1, batch_size=32,
               val_per_epoch=1, testing_times=1, num_workers=0, save_path="", synthetic_per_class=40, synthetic_test_per_class=10, seed=7)
    return cfg


def test_first_session_through_the_trainer():
    from libcontinual_amd import optim
    from libcontinual_amd.trainer import Trainer, _backward
    tr = Trainer(0, copy.deepcopy(_cfg()), log=lambda *a, **k: None)
    model = tr.model
    steps = []
    observe = model.observe

    def recording(data):
        out = observe(data)
        steps.append((model._skip_train, out[2].detach()))
        return out
    model.observe = recording
    out = tr.train_loop()
    model.observe = observe
    first = [float(l) for skip, l in steps if not skip]
    assert len(first) == 15 and all(skip for skip, _ in steps[15:]) and len(steps) > 15       # 160 images / 32 x 3 epochs, then the no-op task
    print(f"first-session losses: {[round(l, 4) for l in first]}")
    assert np.mean(first[-5:]) < np.mean(first[:5])
    feat = model._network.backbone.feat
    assert all(b.adaptmlp.up_proj.weight.detach().abs().max() > 0 for b in feat.transformer.blocks)
    assert not any(t.requires_grad for t in feat.adapter_tensors())
    # task 1's observe: backward and a step leave every parameter bit-unchanged
    opt = optim.SGD(model.get_parameters({}), lr=0.1, momentum=0.9, weight_decay=5e-4)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    model.train()
    o, acc, loss = model.observe(next(iter(tr.train_loader.get_loader(1))))
    assert o is None and acc == 0. and float(loss.detach()) == 0.0
    opt.zero_grad()
    _backward(loss)
    opt.step()
    assert all(torch.equal(v.detach(), before[k]) for k, v in model.named_parameters())
    acc = out["acc_table"]
    assert acc.shape == (2, 2) and np.isfinite(acc).all()
    assert acc[0, 0] > 40.0 and acc[1, :].min() > 25.0, acc
    assert tuple(model.Q.shape) == (100, 7) and model._network.classifier.use_RP is True
    torch.cuda.synchronize()
