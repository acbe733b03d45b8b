"""Classifier alignment on the GPU: `ClassAligner` on the inputs of tests/golden/ca_tiny.npz with ca_ref's normals and permutations injected, against
the fp64 restatement and the reference's own fp32 run; and `InfLoRA_OPT(use_ca=True)` through the product Trainer on the tiny random-init ViT of
tests/test_trainer_gpu.py (rebuilt here with equal class counts and `dataset: cifar100`, which the switch requires).

Measured on an MI355X (the tests print these): moments at 0.19 / 0.17 of their bounds; aligned heads 3.18e-08 off fp64 against dev_ref 3.68e-08
(bound 1.47e-07), the alignment having moved them by 7.4e-02; no held-out row left out by the top-2 gap rule, logits 3.3e-06 off the reference's.
"""
import os

import numpy as np
import pytest
import torch

import ca_ref as CA

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ca_tiny.npz"))


@pytest.fixture(scope="module")
def run64():
    return CA.run_fixture()


@pytest.fixture(scope="module")
def aligned():
    """the two-task run of the fixture on the device: (aligner, heads, flat W, flat b)"""
    from libcontinual_amd.model.class_align import ClassAligner
    from libcontinual_amd.model.heads import HipLinear
    al = ClassAligner(CA.D, DEV)
    heads = [HipLinear(CA.D, CA.CLS, bias=True).to(DEV) for _ in range(CA.TASKS)]
    with torch.no_grad():
        for h, (w, b) in zip(heads, CA.init_heads()):
            h.weight.copy_(torch.from_numpy(w))
            h.bias.copy_(torch.from_numpy(b))
    for t in range(CA.TASKS):
        f, l = CA.task_rows(t, "train")
        al.add_task(torch.from_numpy(f), torch.from_numpy(l), t * CA.CLS, CA.CLS)
    C = CA.TASKS * CA.CLS
    W, b = al.align(heads, CA.TASKS - 1, CA.CLS, normal_fn=lambda ep, shape: torch.from_numpy(CA.normals_epoch(ep, C)),
                    perm_fn=lambda ep, n: torch.from_numpy(CA.permutation(ep, n)))
    torch.cuda.synchronize()
    return al, heads, W, b


def test_aligner_moments_within_the_kernel_bounds(aligned, run64):
    al = aligned[0]
    assert tuple(al.means.shape) == (4, CA.D) and tuple(al.covs.shape) == tuple(al.chols.shape) == (4, CA.D, CA.D)
    worst_m = worst_c = 0.0
    for t in range(CA.TASKS):
        f, l = CA.task_rows(t, "train")
        for c in range(CA.CLS):
            k, x = t * CA.CLS + c, f[l == t * CA.CLS + c]
            worst_m = max(worst_m, float((np.abs(al.means[k].double().cpu().numpy() - run64["means"][k]) / CA.mean_bound(x)).max()))
            worst_c = max(worst_c, float((np.abs(al.covs[k].double().cpu().numpy() - run64["covs"][k]) / CA.cov_bound(x)).max()))
            assert torch.equal(al.covs[k], al.covs[k].T)
            assert bool((al.chols[k].triu(1) == 0).all())
    print(f"ClassAligner moments: largest error / bound, mean {worst_m:.4f}, covariance {worst_c:.4f}")
    assert worst_m <= 1.0 and worst_c <= 1.0


def test_aligned_heads_within_four_times_the_reference_deviation(aligned, run64, golden):
    """aligned heads within 4 x dev_ref of the fp64 restatement, dev_ref being the reference fp32 run's own distance from it (read from the golden)"""
    _, heads, W, b = aligned
    dev_ref = float(golden["dev_ref"])
    dev = max(np.abs(W.double().cpu().numpy() - run64["W"]).max(), np.abs(b.double().cpu().numpy() - run64["b"]).max())
    moved = np.abs(run64["W"] - run64["W0"]).max()
    print(f"aligned heads: off fp64 by {dev:.4e}; dev_ref {dev_ref:.4e}, bound 4 x dev_ref = {4 * dev_ref:.4e}; the alignment moved the heads by {moved:.4e}")
    assert torch.equal(torch.cat([h.weight for h in heads]), W) and torch.equal(torch.cat([h.bias for h in heads]), b)      # copied back
    assert dev <= 4 * dev_ref, (dev, dev_ref)


def test_held_out_argmax_matches_the_reference(aligned, golden):
    from libcontinual_amd import ops
    _, _, W, b = aligned
    held = np.concatenate([CA.task_rows(t, "held")[0] for t in range(CA.TASKS)])
    logits = ops.linear(torch.from_numpy(held).to(DEV), W, b).cpu().numpy()
    decided = CA.top2_gap(golden["held_logits"]) > 8 * float(golden["dev_ref"]) * np.abs(held.astype(np.float64)).sum(1)
    print(f"held-out rows: {len(held)}, left out by the top-2 gap rule {1 - decided.mean():.4f}; logits off the reference's by "
          f"{np.abs(logits - golden['held_logits']).max():.3e}")
    assert 1 - decided.mean() <= 0.02
    assert np.array_equal(np.argmax(logits, 1)[decided], np.argmax(golden["held_logits"], 1)[decided])


def test_default_draws_follow_the_seed(aligned):
    """without injected functions the normals come from torch.randn on the device and the shuffle from the CPU generator: a seed reproduces the run"""
    from libcontinual_amd.model.heads import HipLinear
    al = aligned[0]
    outs = []
    for _ in range(2):
        torch.manual_seed(11)
        heads = [HipLinear(CA.D, CA.CLS, bias=True).to(DEV) for _ in range(CA.TASKS)]
        outs.append(al.align(heads, CA.TASKS - 1, CA.CLS))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and bool(torch.isfinite(outs[0][0]).all())


# ------------------------------------------------------------------------------------------------ through the product Trainer
def _cfg(dtype, use_ca):
    """the tiny-ViT InfLoRA_OPT configuration of tests/test_trainer_gpu.py with equal class counts; use_ca: True / False / None (switch absent)"""
    from libcontinual_amd.config import Config
    cfg = Config().get_config_dict()
    bb_kw = {"pretrained": False, "img_size": 32, "patch_size": 8, "embed_dim": 128, "depth": 2, "num_heads": 2, "dtype": dtype,
             "attn_layer": "MultiHeadAttention_LoRA", "lora_rank": 4}
    kw = {"dataset": "cifar100", "init_cls_num": 3, "inc_cls_num": 3, "task_num": 3, "lame": 0.9, "lamb": 0.6, "embd_dim": 128}
    if use_ca is not None:
        kw["use_ca"] = use_ca
    cfg.update(dict(dataset="synthetic", image_size=32, init_cls_num=3, inc_cls_num=3, task_num=3, epoch=2, init_epoch=3, batch_size=32,
                    val_per_epoch=10, testing_times=1, num_workers=0, save_path="", synthetic_per_class=64, synthetic_test_per_class=16, seed=5,
                    backbone={"name": "vit_pt_imnet", "kwargs": bb_kw}, classifier={"name": "InfLoRA_OPT", "kwargs": kw},
                    optimizer={"name": "SGD", "kwargs": {"lr": 0.05, "momentum": 0.9}}, lr_scheduler={"name": "Constant"}))
    return cfg


def _run(dtype, use_ca, spy=None):
    from libcontinual_amd.trainer import Trainer
    os.environ.setdefault("PYTHONHASHSEED", "0")
    tr = Trainer(0, _cfg(dtype, use_ca), log=lambda *a, **k: None)
    if spy is not None:
        spy(tr.model)
    out = tr.train_loop()
    torch.cuda.synchronize()
    return tr, out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_use_ca_trains_end_to_end(dtype):
    snaps = {}

    def spy(model):
        inner = model._compact_classifier

        def wrapped(task_idx):
            head0 = model._network.classifier_pool[0]
            snaps[task_idx] = [head0.weight.detach().clone()]
            inner(task_idx)
            snaps[task_idx].append(head0.weight.detach().clone())
        model._compact_classifier = wrapped

    tr, out = _run(dtype, True, spy)
    assert np.isfinite(out["acc_table"]).all()
    m = tr.model
    assert tuple(m._class_means.shape) == (9, 128) and tuple(m._class_covs.shape) == (9, 128, 128)
    assert bool(torch.isfinite(m._class_means).all()) and bool(torch.isfinite(m._class_covs).all())
    assert sorted(snaps) == [1, 2]                                    # never at task 0 (InfLoRA_opt.py:287)
    before, after = snaps[1]
    assert not torch.equal(before, after) and bool(torch.isfinite(after).all())       # without CA the head of task 0 is frozen after task 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_use_ca_false_is_the_run_without_the_switch(dtype):
    (tr_a, out_a), (tr_b, out_b) = _run(dtype, False), _run(dtype, None)
    assert np.array_equal(out_a["acc_table"], out_b["acc_table"])
    sa, sb = tr_a.model.state_dict(), tr_b.model.state_dict()
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert tr_a.model._aligner is None and tr_a.model._class_means is None
