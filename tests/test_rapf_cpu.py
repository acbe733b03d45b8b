"""RAPF's host side without a device: construction refusals, the two shipped configs, the host logic of model/rapf.py against the reference's fixture
(tests/golden/rapf_tiny.npz) and against tests/rapf_ref.py, the `is_rapf` transforms, and the bindings of the three entry points."""
import os

import numpy as np
import pytest
import torch

import rapf_ref as R
import libcontinual_amd.model as M
from libcontinual_amd import _lib
from libcontinual_amd.config import Config
from libcontinual_amd.data import transforms as T
from libcontinual_amd.model import rapf as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(init_cls_num=3, inc_cls_num=3, beta=2, shrinkage=False, threshold=0.5, train_batch_size=9, batch_size=9, num_workers=0, prompt_template="a good photo of a {}",
          fp16=False, mix_bias=0.6, seed=1)


def _tiny_clip():
    c = R.CFG
    return M.clip("ViT-B/16", None, pretrained=False, embed_dim=c["embed"], image_resolution=c["img"], vision_layers=1, vision_width=c["width"], vision_patch_size=c["patch"],
                  context_length=c["ctx"], vocab_size=40, transformer_width=c["twidth"], transformer_heads=1, transformer_layers=1, dtype="f32")


def test_construction_and_refusals():
    bb = _tiny_clip()
    m = M.RAPF(bb, "cpu", **KW)
    assert m.cuda_graph_safe is False and tuple(m.adapter.weight.shape) == (R.CFG["embed"],) * 2 and m.adapter.bias is None
    assert [n for n, p in m.named_parameters() if p.requires_grad] == ["adapter.weight"] and [id(p) for p in m.get_parameters(None)] == [id(m.adapter.weight)]
    with pytest.raises(NotImplementedError, match="fp16"):
        M.RAPF(bb, "cpu", **{**KW, "fp16": True})
    with pytest.raises(NotImplementedError, match="CLIP"):
        M.RAPF(torch.nn.Linear(2, 2), "cpu", **KW)
    with pytest.raises(NotImplementedError, match="n_gpu"):
        M.RAPF(bb, "cpu", **KW, n_gpu=2)
    with pytest.raises(ValueError, match="class_tokens"):
        M.RAPF(bb, "cpu", **KW, class_tokens=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="class names"):
        m.before_task(0, None, [], None)                                  # neither names nor tokens
    with pytest.raises(NotImplementedError, match="testing_per_task"):
        M.RAPF(bb, "cpu", **KW, testing_per_task=False).before_task(0, None, [], None)
    with pytest.raises(NotImplementedError):                              # the MoE block of the reference's RAPF configs keeps raising
        M.clip("ViT-B/16", None, pretrained=False, block_layer="ResidualAttentionBlock_MoE_MLP", experts_num=1)


def test_before_task_on_the_host_with_class_tokens():
    """text features once per task, hard pairs in the reference's order with label offsets, the old-class shuffle through the hook or the method's own generator"""
    tokens = torch.zeros(9, 77, dtype=torch.int64)
    for c in range(9):
        tokens[c, :4] = torch.tensor([38, 1 + c, 1 + (5 * c) % 37, 39])
    m = M.RAPF(_tiny_clip(), "cpu", **{**KW, "threshold": 2.5}, class_tokens=tokens)
    m.before_task(0, None, [], None)
    assert m.class_name_features.shape == (3, R.CFG["embed"]) and m.hard_pairs is None and m.old_adapter is None
    assert torch.allclose(m.class_name_features.norm(dim=1), torch.ones(3), atol=1e-6)
    m.prev_cls_num = 3
    m.before_task(1, None, [], None)
    assert m.hard_pairs.tolist() == [[o, n] for o in range(3) for n in range(3, 6)] and m._pos.tolist() == [o for o in range(3) for _ in range(3) for _ in range(40)]
    assert sorted(m.random_class_order_list) == [0, 1, 2] and m.old_adapter is not None and m.old_adapter is not m.adapter
    import random
    want = list(range(3))
    random.Random(KW["seed"]).shuffle(want)
    assert m.random_class_order_list == want                              # the method's own generator, seeded once
    m.class_order_fn = lambda t, classes: [2, 0, 1]
    m.accu_cls_num = 3                                                    # task 1 once more, with the hook
    m.before_task(1, None, [], None)
    assert m.random_class_order_list == [2, 0, 1]
    m.class_order_fn = lambda t, classes: [0, 0, 1]
    m.accu_cls_num = 3
    with pytest.raises(ValueError, match="permutation"):
        m.before_task(1, None, [], None)


@pytest.mark.parametrize("inc,k", [(3, 2), (10, 2), (5, 4)])
def test_replay_classes_walk_the_shuffled_list(inc, k):
    order = [4, 1, 3, 0, 2]
    for b in range(7):
        got = P.replay_classes(order, b, inc)
        assert got == [order[(b * k + i) % 5] for i in range(k)] == R.replay_classes(order, b, inc)


def test_host_logic_against_the_fixture(golden):
    fix = golden("rapf_tiny")
    for t in range(1, R.TASKS):
        txt = torch.from_numpy(fix[f"t{t}/txt"])
        hp = P.hard_pairs(txt, R.INC * t, float(fix["threshold"]))
        assert hp.dtype == torch.int64 and np.array_equal(hp.numpy(), fix[f"t{t}/hard_pairs"].reshape(-1, 2))
        # mix_matrix: from the adapter after the task's last step and the one the task began with to the stored mixed one
        w_new, w_old = torch.from_numpy(fix[f"t{t}/s{R.STEPS - 1}/adapter"]), torch.from_numpy(fix[f"t{t - 1}/adapter"])
        os.environ["CLHIP_SVD"] = "host"
        try:
            got = P.mix_matrix(w_new, w_old, R.MIX_BIAS)
        finally:
            del os.environ["CLHIP_SVD"]
        assert R.rel(got, fix[f"t{t}/adapter"]) < 1e-10
    assert len(fix["t1/hard_pairs"]) + len(fix["t2/hard_pairs"]) > 0


def test_hard_pair_order_is_old_major():
    txt = torch.eye(6)[:, :4].clone()
    txt[3], txt[4], txt[5] = txt[1], txt[0], txt[1]                        # new 3 ~ old 1, new 4 ~ old 0, new 5 ~ old 1
    assert P.hard_pairs(txt, 3, 0.1).tolist() == [[0, 4], [1, 3], [1, 5]]
    assert P.hard_pairs(txt, 3, 0.0).shape == (0, 2)


def test_shrink_cov_is_the_reference_formula():
    g = torch.Generator().manual_seed(2)
    a = torch.randn(6, 6, generator=g)
    cov = a @ a.T
    got = P.shrink_cov(cov)
    off = cov - torch.diag(torch.diagonal(cov))
    want = cov + torch.diagonal(cov).mean() * torch.eye(6) + off.sum() / 30 * (1 - torch.eye(6))
    assert torch.allclose(got, want, atol=1e-6) and torch.allclose(got, R.shrink_cov(cov))
    torch.linalg.cholesky(got)                                            # still positive definite


def test_is_rapf_transform_is_the_spelled_out_list():
    from libcontinual_amd.data.dataset import get_dataloader
    t = T.rapf_transform(24)
    spelled = T.Compose([T.Resize(24, interpolation="BICUBIC"), T.CenterCrop(24), T.ToTensor(),
                         T.Normalize((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))])
    img = (np.arange(40 * 30 * 3) % 251).astype(np.uint8).reshape(40, 30, 3)
    a, b = t(img), spelled(img)
    assert a.shape == (3, 24, 24) and torch.equal(a, b)
    grey = t(img[:, :, 0])
    assert grey.shape == (3, 24, 24)
    cfg = dict(dataset="synthetic", data_root="", is_rapf=True, image_size=16, init_cls_num=2, inc_cls_num=2, task_num=2, batch_size=4, num_workers=0, seed=1,
               train_trfms=[{"RandomHorizontalFlip": {}}])
    for mode in ("train", "test"):                                        # both modes, and ahead of any *_trfms
        ds = get_dataloader(cfg, mode).dataloaders[0].dataset
        assert [type(x) for x in ds.trfms.transforms] == [T.Resize, T.CenterCrop, T.ToTensor, T.Normalize] and ds.trfms.transforms[0].interp == 3


@pytest.mark.parametrize("name,inc,tasks", [("rapf-clip-vitb16-cifar100-b10x10.yaml", 10, 10), ("rapf-clip-vitb16-cifar100-b50-5x10.yaml", 5, 11)])
def test_shipped_configs_parse_and_resolve(name, inc, tasks, monkeypatch):
    monkeypatch.chdir(ROOT)
    cfg = Config(os.path.join(ROOT, "config", name)).get_config_dict()
    assert cfg["classifier"]["name"] == "RAPF" and hasattr(M, "RAPF") and cfg["backbone"]["name"] == "clip" and cfg["is_rapf"] is True
    kw = cfg["classifier"]["kwargs"]
    assert kw["inc_cls_num"] == cfg["inc_cls_num"] == inc and cfg["task_num"] == tasks and kw["beta"] == 2 and kw["mix_bias"] == 0.6 and kw["fp16"] is False
    assert cfg["optimizer"]["name"] == "Adam" and cfg["lr_scheduler"]["name"] == "MultiStepLR" and cfg["lr_scheduler"]["kwargs"]["milestones"] == [4, 10]
    assert "block_layer" not in cfg["backbone"]["kwargs"] and "experts_num" not in cfg["backbone"]["kwargs"] and cfg["testing_per_task"] is True
    assert cfg["train_batch_size"] == 100 and cfg["epoch"] == 15


def test_entry_points_are_declared_and_bound():
    names = ["clhip_rapf_draw", "clhip_rapf_step_fwd", "clhip_rapf_step_bwd"]
    assert all(n in _lib.header_symbols() and n in _lib._PROTOS for n in names)
    if os.path.exists(_lib.LIB_PATH):
        assert all(hasattr(_lib.lib(), n) for n in names)
    from libcontinual_amd import ops
    assert all(hasattr(ops, n) for n in ("rapf_draw", "rapf_step_fwd", "rapf_step_bwd", "rapf_loss"))
