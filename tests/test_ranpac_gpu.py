"""RanPAC on the MI355X: `RPClassifier` on the reference-generated fixture, the whole plugin on a tiny ViT, and the shipped YAML through the Trainer.

Yardstick: the reference's own arithmetic -- relu(F W), the two sums, torch.linalg.solve and the head product, all in fp32 on the CPU (ranpac.py:246-251,
:265, :55-59) -- is re-run here on the same features (`_Cpu32`) and its deviation from the fp64 restatement is measured at run time.  The device may be
4 x that far from fp64 (a different but equally valid elimination and summation order).  Near ties: a test row counts as a near tie when its two
largest fp64 logits are closer than 2 x 4 x the deviation of that fp32 CPU run's logits (both logits may move by the allowance); predictions are
compared outside those rows.
"""
import copy
import os

import numpy as np
import pytest
import torch

import ranpac_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


class _Cpu32:
    """the reference's fp32 CPU arithmetic with a given ridge"""

    def __init__(self, W):
        self.W = torch.as_tensor(W, dtype=torch.float32).cpu()
        m = self.W.shape[1]
        self.G, self.Q, self.Wo = torch.zeros(m, m), torch.zeros(m, 0), None

    def fit(self, feats, labels, C, ridge):
        f, l = torch.as_tensor(feats, dtype=torch.float32), torch.as_tensor(labels, dtype=torch.int64)
        m = self.W.shape[1]
        H = torch.relu(f @ self.W)
        self.Q = torch.cat((self.Q, torch.zeros(m, C - self.Q.shape[1])), dim=1) + H.T @ torch.nn.functional.one_hot(l, C).float()
        self.G = self.G + H.T @ H
        self.Wo = torch.linalg.solve(self.G + ridge * torch.eye(m), self.Q).T
        return self.Wo.double().numpy()

    def logits(self, feats):
        return (torch.relu(torch.as_tensor(feats, dtype=torch.float32) @ self.W) @ self.Wo.T).double().numpy()


def test_rp_classifier_on_the_reference_fixture(golden):
    from libcontinual_amd.model import RPClassifier
    g = golden("ranpac_tiny")
    W = torch.from_numpy(g["W_rand"])
    rp, ref = RPClassifier(R.D, R.M, DEV, w_rand=W), R.Ridge64(g["W_rand"])
    cpu32 = _Cpu32(g["W_rand"])
    for t in range(R.TASKS):
        C = (t + 1) * R.CLS
        f, l = torch.from_numpy(g[f"train_feats_{t}"]), torch.from_numpy(g[f"train_labels_{t}"])
        Wo = rp.update(f.to(DEV), l.to(DEV), C)
        ref.fit(g[f"train_feats_{t}"], g[f"train_labels_{t}"], C)
        assert tuple(Wo.shape) == (C, R.M) and tuple(rp.Q.shape) == (R.M, C) and rp.G.dtype == torch.float32 and rp.G.is_cuda
        assert torch.equal(rp.G, rp.G.T)
        assert round(np.log10(rp.ridge)) == int(g[f"ridge_exp_{t}"]) == ref.ridge_exp
        # the reference's arithmetic, here, on the CPU in fp32 (ranpac.py:246-251, :265): its error against fp64 is the yardstick of ours
        err_ref = np.linalg.norm(cpu32.fit(f, l, C, rp.ridge) - ref.Wo)
        err_dev = np.linalg.norm(Wo.double().cpu().numpy() - ref.Wo)
        print(f"task {t}: |Wo - fp64| device {err_dev:.3e}, reference's fp32 CPU solve {err_ref:.3e}, ratio {err_dev / err_ref:.3f}")
        assert err_dev <= 4 * err_ref
        X = np.concatenate([g[f"test_feats_{s}"] for s in range(t + 1)])
        l64 = ref.logits(X)
        logits = rp.logits(torch.from_numpy(X).to(DEV)).cpu().numpy()
        dev32 = np.abs(cpu32.logits(X) - l64).max()
        clear = R.top2_gap(l64) >= 2 * 4 * dev32
        print(f"task {t}: logits off fp64 by {np.abs(logits - l64).max():.2e} (the fp32 CPU run: {dev32:.2e}); rows outside near ties {clear.mean():.3f}")
        assert clear.mean() >= 0.98                       # the fixture keeps near ties under 2 % (tests/test_ranpac_cpu.py)
        assert np.array_equal(np.argmax(logits, 1)[clear], np.argmax(l64, 1)[clear])
        assert np.array_equal(np.argmax(logits, 1)[clear], np.argmax(g[f"logits_{t}"], 1)[clear])


def _cfg(M=144):
    from libcontinual_amd.config import Config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        cfg = Config(os.path.join(ROOT, "config", "ranpac-vitb16-cifar100-b10x10.yaml")).get_config_dict()
    finally:
        os.chdir(cwd)
    cfg.pop("train_trfms"), cfg.pop("test_trfms")
    cfg["backbone"]["kwargs"] = {"pretrained": False, "img_size": 32, "patch_size": 8, "embed_dim": 64, "depth": 2, "num_heads": 2, "dtype": "f32"}
    cfg["classifier"]["kwargs"].update(M=M, init_cls_num=4, inc_cls_num=3, task_num=3, total_cls_num=10)
    cfg.update(dataset="synthetic", image_size=32, init_cls_num=4, inc_cls_num=3, task_num=3, total_cls_num=10, init_epoch=1, epoch=1, batch_size=32,
               val_per_epoch=1, testing_times=1, num_workers=0, save_path="", synthetic_per_class=40, synthetic_test_per_class=10, seed=7)
    return cfg


def test_plugin_on_a_tiny_vit():
    from libcontinual_amd import optim
    from libcontinual_amd.trainer import Trainer, _backward
    tr = Trainer(0, _cfg(), log=lambda *a, **k: None)
    model = tr.model
    ref = cpu32 = None
    for t in range(3):
        train, tests = tr.train_loader.get_loader(t), tr.test_loader.get_loader(t)
        model.before_task(t, None, train, tests)
        head = model._network.classifier
        classes = 4 + 3 * t
        # the fresh cosine head is what inference uses until after_task (ranpac.py:105-106, :51-52)
        assert head.use_RP is False and tuple(head.weight.shape) == (classes, 64) and float(head.sigma.detach()) == 1.0
        batch = next(iter(tests[0]))
        model.eval()
        with torch.no_grad():
            feat = model._network.get_feature(batch["image"].to(DEV)).float()
            logits = model._network(batch["image"].to(DEV), True)
        cos = torch.nn.functional.normalize(feat.double().cpu(), dim=1) @ torch.nn.functional.normalize(head.weight.detach().double().cpu(), dim=1).T
        assert tuple(logits.shape) == (feat.shape[0], classes) and float((logits.double().cpu() - cos).abs().max()) < 1e-5
        # the skipped observe: backward and an optimizer step leave every parameter bit-unchanged (ranpac.py:184-186)
        opt = optim.SGD(model.get_parameters({}), lr=0.1, momentum=0.9, weight_decay=5e-4)
        before = {k: v.detach().clone() for k, v in model.named_parameters()}
        model.train()
        out, acc, loss = model.observe(next(iter(train)))
        assert out is None and acc == 0. and loss.is_cuda and loss.requires_grad and float(loss.detach()) == 0.0
        opt.zero_grad()
        _backward(loss)
        opt.step()
        assert all(torch.equal(v.detach(), before[k]) for k, v in model.named_parameters())
        test_trfms = tests[0].dataset.trfms
        model.after_task(t, None, train, tests)
        assert train.dataset.trfms is test_trfms and head.use_RP is True and tuple(head.weight.shape) == (classes, 144)
        assert model.G.is_cuda and model.Q.is_cuda and model.W_rand.is_cuda and tuple(model.Q.shape) == (144, classes)
        # the restatement on the features the plugin produced
        feats, labels = (a.cpu().numpy() for a in model.last_features)
        assert feats.shape == (len(train.dataset), 64) and sorted(set(labels.tolist())) == sorted(set(train.dataset.labels))
        if ref is None:
            ref, cpu32 = R.Ridge64(model.W_rand.cpu().numpy()), _Cpu32(model.W_rand.cpu().numpy())
        cpu32.fit(feats, labels, classes, model.rp.ridge)
        ref.fit(feats, labels, classes)
        srt = np.sort(ref.losses)
        print(f"task {t}: ridge 1e{ref.ridge_exp}, second-best / best hold-out loss {srt[1] / srt[0]:.3f}")
        if srt[1] >= 1.05 * srt[0]:
            assert round(np.log10(model.rp.ridge)) == ref.ridge_exp
        else:                                  # an fp64 near tie of two ridges: either is a correct pick
            assert model.rp.ridge in R.RIDGES[np.argsort(ref.losses)[:2]]
            ref.Wo = np.linalg.solve(ref.G + model.rp.ridge * np.eye(144), ref.Q).T
        model.eval()
        X, P = [], []
        for dl in tests:
            for b in dl:
                with torch.no_grad():
                    X.append(model._network.get_feature(b["image"].to(DEV)).float().cpu().numpy())
                P.append(model.inference(b)[0].cpu().numpy())
        X, P = np.concatenate(X), np.concatenate(P)
        l64 = ref.logits(X)
        dev32 = np.abs(cpu32.logits(X) - l64).max()
        clear = R.top2_gap(l64) >= 2 * 4 * dev32
        print(f"task {t}: rows outside near ties {clear.mean():.3f} (the fp32 CPU run's logits are off fp64 by {dev32:.2e})")
        assert clear.any()
        assert np.array_equal(P[clear], np.argmax(l64, 1)[clear])
    torch.cuda.synchronize()


def test_yaml_through_the_trainer():
    from libcontinual_amd.trainer import Trainer
    cfg = _cfg(M=100)
    cfg.update(task_num=2, total_cls_num=7)
    cfg["classifier"]["kwargs"].update(task_num=2, total_cls_num=7)
    tr = Trainer(0, copy.deepcopy(cfg), log=lambda *a, **k: None)
    out = tr.train_loop()
    acc = out["acc_table"]
    assert acc.shape == (2, 2) and np.isfinite(acc).all()
    assert acc[0, 0] > 40.0 and acc[1, :].min() > 25.0, acc            # 4 and 7 classes: chance = 25 % / 14 %
    assert [e[0] for e in tr.hook_trace if e[0] in ("before_task", "after_task")] == ["before_task", "after_task"] * 2
    assert tuple(tr.model.Q.shape) == (100, 7) and tr.model._network.classifier.use_RP is True
    torch.cuda.synchronize()
