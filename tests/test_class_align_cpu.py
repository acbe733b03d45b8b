"""Classifier alignment without a GPU: the fp64 restatement (tests/ca_ref.py) against the reference's own run (tests/golden/ca_tiny.npz, written by
tools/gen_ca_golden.py), the two guards of `InfLoRA_OPT(use_ca=True)`, the constructor, and `use_ca=False` leaving the aligner alone."""
import os

import numpy as np
import pytest
import torch

import ca_ref as CA
import libcontinual_amd.model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ca_tiny.npz"))


@pytest.fixture(scope="module")
def run64():
    return CA.run_fixture()


def _rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def test_restatement_matches_the_reference_moments(golden, run64):
    """means and covariance summaries to 1e-5 relative: fp32 storage of an fp64 result"""
    covs = run64["covs"]
    figures = {"means": _rel(golden["means"], run64["means"]),
               "cov_diag": _rel(golden["cov_diag"], np.stack([np.diag(c) for c in covs])),
               "cov_corner": _rel(golden["cov_corner"], covs[:, :16, -16:]),
               "cov_sum": _rel(golden["cov_sum"], covs.sum((1, 2)))}
    print(figures)
    assert golden["means"].shape == (CA.TASKS * CA.CLS, CA.D)
    assert all(v <= 1e-5 for v in figures.values()), figures


def test_restatement_matches_the_reference_heads(golden, run64):
    """aligned heads within 1e-3 of the distance the alignment moved them"""
    assert np.array_equal(golden["W_before"], run64["W0"].astype(np.float32)) and np.array_equal(golden["b_before"], run64["b0"].astype(np.float32))
    moved = max(np.abs(golden["W_after"].astype(np.float64) - golden["W_before"]).max(), np.abs(golden["b_after"].astype(np.float64) - golden["b_before"]).max())
    dev = max(np.abs(golden["W_after"] - run64["W"]).max(), np.abs(golden["b_after"] - run64["b"]).max())
    print(f"moved {moved:.4e}, restatement off the reference by {dev:.4e} (recorded dev_ref {float(golden['dev_ref']):.4e})")
    assert moved > 1e-2                                               # the alignment did something
    assert dev <= 1e-3 * moved
    assert float(golden["dev_ref"]) <= 2.5e-4 * moved                 # the condition the generator asserts: the fixture resolves a wrong restatement
    assert np.array_equal(np.argmax(golden["held_logits"], 1), np.argmax(run64["logits"], 1))


def test_restatement_pieces():
    """sample() places draw perm[r] in row r with its class's label; the schedule is CosineAnnealingLR's"""
    means, scale = np.arange(6.0).reshape(3, 2), np.asarray([1.0, 2.0, 3.0])
    chols = np.stack([np.eye(2)] * 3)
    z, perm = np.zeros((6, 2)), np.asarray([5, 0, 3, 1, 4, 2])
    X, y = CA.sample(means, scale, chols, z, perm, class_lo=7)
    assert y.tolist() == [9, 7, 8, 7, 9, 8] and np.array_equal(X, (scale[:, None] * means)[y - 7])
    from libcontinual_amd.model.class_align import epoch_lrs
    assert np.allclose(epoch_lrs(), [CA.cosine_lr(e) for e in range(CA.EPOCHS)], rtol=1e-12)
    assert np.allclose(CA.mean_scale(4, 2, 1), [0.95, 0.95, 1.0, 1.0])


def _backbone():
    return M.vit_pt_imnet(pretrained=False, attn_layer="MultiHeadAttention_LoRA", lora_rank=4, img_size=32, patch_size=8, embed_dim=128, depth=1, num_heads=2)


def _kw(**over):
    kw = dict(init_cls_num=3, inc_cls_num=3, task_num=3, lame=0.9, lamb=0.6, embd_dim=128, dataset="cifar100", use_ca=True)
    kw.update(over)
    return kw


def test_use_ca_guards():
    with pytest.raises(NotImplementedError, match="445-447"):
        M.InfLoRA_OPT(_backbone(), "cpu", **_kw(dataset="imagenet-r"))
    with pytest.raises(NotImplementedError, match="445-447"):         # the dataset guard comes first
        M.InfLoRA_OPT(_backbone(), "cpu", **_kw(dataset="imagenet-r", init_cls_num=4))
    with pytest.raises(NotImplementedError, match="377-381"):
        M.InfLoRA_OPT(_backbone(), "cpu", **_kw(init_cls_num=4))


def test_use_ca_constructs():
    m = M.InfLoRA_OPT(_backbone(), "cpu", **_kw())
    assert m._use_class_alignment and m._aligner.feat_dim == 128
    assert m._class_means is None and m._class_covs is None           # InfLoRA_opt.py:159-160
    assert tuple(m._aligner.chols.shape) == (0, 128, 128)


def test_without_use_ca_after_task_never_touches_the_aligner(monkeypatch):
    for kw in (_kw(use_ca=False), {k: v for k, v in _kw(dataset="imagenet-r").items() if k != "use_ca"}):
        m = M.InfLoRA_OPT(_backbone(), "cpu", **kw)
        assert m._aligner is None and not m._use_class_alignment and m._class_means is None
        boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("classifier alignment ran"))
        monkeypatch.setattr(m, "_create_distribution", boom)
        monkeypatch.setattr(m, "_compact_classifier", boom)
        monkeypatch.setattr(m, "_update_feature", lambda *a, **k: None)
        monkeypatch.setattr(m, "attention_modules", [])
        m.after_task(1, None, None, None)


def test_aligner_refuses_cpu_tensors():
    from libcontinual_amd import _lib
    from libcontinual_amd.model.class_align import ClassAligner
    al = ClassAligner(8, "cpu")
    with pytest.raises(_lib.ClhipError):
        al.add_task(torch.zeros(6, 8), torch.tensor([0, 0, 0, 1, 1, 1]), 0, 2)


def test_c_abi_symbols_are_declared_and_bound():
    from libcontinual_amd import _lib
    declared = _lib.header_symbols()
    for n in ("clhip_class_moments", "clhip_ca_sample"):
        assert n in declared and n in _lib._PROTOS
    with open(os.path.join(ROOT, "include", "clhip.h")) as f:
        assert "InfLoRA_opt.py:371-456" in f.read()
    with open(os.path.join(ROOT, "libcontinual_amd", "csrc", "build.sh")) as f:
        assert " ca " in f.read()


def test_shipped_config_resolves():
    from libcontinual_amd.config import Config
    cfg = Config("config/inflora_opt-vitb16-cifar100-b10x10-ca.yaml").get_config_dict()
    kw = cfg["classifier"]["kwargs"]
    assert cfg["classifier"]["name"] == "InfLoRA_OPT" and kw["use_ca"] is True and kw["dataset"] == "cifar100"
    assert kw["init_cls_num"] == kw["inc_cls_num"] == 10 and kw["task_num"] == 10 and kw["embd_dim"] == 768
