"""AdaptFormer adapters without a GPU: the fp64 restatement against torch autograd, the adapter backbone's parameters, RanPAC's first-session switch."""
import math
import os

import torch

import adapter_ref as A
from oracle import vit as OV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY_KW = dict(pretrained=False, img_size=32, patch_size=8, embed_dim=64, depth=2, num_heads=2, dtype="f32")
RP_KW = dict(M=32, init_cls_num=4, inc_cls_num=3, task_num=2, total_cls_num=7)


def _close(a, b, tol):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def test_restatement_matches_autograd():
    for M, D, R, p in ((51, 64, 16, 0.0), (51, 64, 16, 0.1), (7, 128, 64, 0.3)):
        g = A.gen(M + R)
        x, gy = torch.randn(M, D, generator=g, dtype=torch.float64), torch.randn(M, D, generator=g, dtype=torch.float64)
        mask = (torch.rand(M, R, generator=g) >= p).to(torch.uint8)
        Wd, bd, Wu, bu = A.adapter_params(D, R, 3)
        delta, hd = A.fwd(x, Wd, bd, Wu, bu, A.SCALE, mask, p)
        dx, dWd, dbd, dWu, dbu, _ = A.bwd(gy, x, hd, Wd, Wu, A.SCALE, p)
        out, (ax, aWd, abd, aWu, abu) = A.autograd(gy, x, Wd, bd, Wu, bu, A.SCALE, mask, p)
        for got, want in ((delta, out), (dx, ax), (dWd, aWd), (dbd, abd), (dWu, aWu), (dbu, abu)):
            assert _close(got, want, 1e-12)
        assert 0.0 < float((hd > 0).double().mean()) < 1.0         # both sides of the ReLU are exercised


def test_tiny_vit_restatement_matches_autograd():
    P = {k: v.requires_grad_(False) for k, v in OV.det_params(A.TINY, "adapter_cpu", dtype=torch.float64).items()}
    g = A.gen(5)
    img = torch.randn(3, 3, 32, 32, generator=g, dtype=torch.float64)
    masks = [(torch.rand(51, A.R_TINY, generator=g) >= 0.1).to(torch.uint8) for _ in range(2)]
    grads = []
    for hand in (True, False):
        Ad = [[t.clone().requires_grad_(True) for t in A.adapter_params(64, A.R_TINY, 10 + i)] for i in range(2)]
        f = A.vit_features(P, Ad, img, masks=masks, p=0.1, hand=hand)
        f.square().sum().backward()
        grads.append((f.detach(), [t.grad for layer in Ad for t in layer]))
    assert _close(grads[0][0], grads[1][0], 1e-12)
    for a, b in zip(grads[0][1], grads[1][1]):
        assert float(b.abs().max()) > 0 and _close(a, b, 1e-12)
    # zero up_proj / biases: the adapter ViT is the plain ViT of oracle/vit.py
    Z = [A.adapter_params(64, A.R_TINY, 10 + i, zero_up=True) for i in range(2)]
    assert torch.equal(A.vit_features(P, Z, img), OV.cls_features(P, img, A.TINY))


def test_adapter_backbone_parameters():
    import libcontinual_amd.model as M
    torch.manual_seed(3)
    plain = M.vit_pt_imnet_in21k_adapter(**TINY_KW)
    torch.manual_seed(3)
    bb = M.vit_pt_imnet_in21k_adapter(ffn_adapt=True, ffn_num=16, ffn_adapter_scalar=0.1, adapter_dropout=0.1, **TINY_KW)
    assert type(bb) is type(plain) and not hasattr(plain.feat, "block_ln_eps") and plain.feat.adapter_dim == 0
    assert bb.feat.block_ln_eps == 1e-6 and bb.feat.adapter_dim == 16 and bb.feat.adapter_scale == 0.1 and bb.feat.adapter_dropout == 0.1
    sd, psd = bb.state_dict(), plain.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in psd.items())           # the adapters are drawn after everything else
    extra = sorted(set(sd) - set(psd))
    want = {"down_proj.weight": (16, 64), "down_proj.bias": (16,), "up_proj.weight": (64, 16), "up_proj.bias": (64,)}
    assert extra == sorted(f"feat.transformer.blocks.{i}.adaptmlp.{n}" for i in range(2) for n in want)
    for k in extra:
        # the reference's own key: `blocks.{i}.adaptmlp.*` under its timm tree (load_pretrained's `blocks.` -> `transformer.blocks.` rename)
        assert k.replace("feat.transformer.", "").startswith("blocks.") and ".adaptmlp." in k
        name = k.split(".adaptmlp.")[1]
        assert tuple(sd[k].shape) == want[name]
        if name == "down_proj.weight":
            bound = 1 / math.sqrt(64)                                   # kaiming_uniform_(a = sqrt 5): U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
            assert float(sd[k].abs().max()) <= bound and float(sd[k].abs().max()) > 0.8 * bound and abs(float(sd[k].mean())) < 0.1 * bound
        else:
            assert not sd[k].any()
    grad = {k for k, v in bb.named_parameters() if v.requires_grad}
    assert grad == set(extra)
    assert len(bb.feat.adapter_tensors()) == 8 and plain.feat.adapter_tensors() == []


def test_ranpac_first_session_switch():
    import pytest
    import libcontinual_amd.model as M
    bb = M.vit_pt_imnet_in21k_adapter(ffn_adapt=True, ffn_num=16, **TINY_KW)
    m = M.RanPAC(bb, "cpu", first_session_training=True, **RP_KW)
    assert m.first_session_training is True
    assert {k for k, v in m.named_parameters() if v.requires_grad} == {f"_network.backbone.{k}" for k in bb.state_dict() if ".adaptmlp." in k}
    m.before_task(0, None, None, None)
    assert m._skip_train is False and all(t.requires_grad for t in bb.feat.adapter_tensors())
    m.before_task(1, None, None, None)
    assert m._skip_train is True and not any(t.requires_grad for t in bb.feat.adapter_tensors())
    # the adapter backbone without the switch stays frozen; the switch on a backbone without adapters names the way out
    frozen = M.RanPAC(M.vit_pt_imnet_in21k_adapter(ffn_adapt=True, ffn_num=16, **TINY_KW), "cpu", first_session_training=False, **RP_KW)
    assert not any(p.requires_grad for p in frozen._network.backbone.parameters())
    with pytest.raises(NotImplementedError, match="first_session_training.*ffn_adapt"):
        M.RanPAC(M.vit_pt_imnet_in21k_adapter(**TINY_KW), "cpu", first_session_training=True, **RP_KW)
    with pytest.raises(NotImplementedError, match="ffn_num"):
        M.vit_pt_imnet_in21k_adapter(ffn_adapt=True, ffn_num=48, **TINY_KW)


def test_first_session_yaml_loads():
    from libcontinual_amd.config import Config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        cfg = Config(os.path.join(ROOT, "config", "ranpac-vitb16-cifar100-b10x10-fst.yaml")).get_config_dict()
        old = Config(os.path.join(ROOT, "config", "ranpac-vitb16-cifar100-b10x10.yaml")).get_config_dict()
    finally:
        os.chdir(cwd)
    assert cfg["classifier"]["name"] == "RanPAC" and cfg["classifier"]["kwargs"]["first_session_training"] is True
    kw = cfg["backbone"]["kwargs"]
    assert cfg["backbone"]["name"] == "vit_pt_imnet_in21k_adapter"
    assert (kw["ffn_adapt"], kw["ffn_num"], kw["ffn_adapter_scalar"], kw["adapter_dropout"]) == (True, 64, 0.1, 0.1)
    assert (cfg["init_epoch"], cfg["epoch"], cfg["batch_size"], cfg["seed"]) == (20, 1, 48, 2)
    assert cfg["optimizer"] == {"name": "SGD", "kwargs": {"momentum": 0.9, "lr": 0.01, "weight_decay": 0.0005}}
    assert cfg["lr_scheduler"] == {"name": "CosineAnnealingLR", "kwargs": {"T_max": 20, "eta_min": 0.0}}
    # everything but the two switches is the existing file
    kw.pop("ffn_adapt"), kw.pop("ffn_num"), kw.pop("ffn_adapter_scalar"), kw.pop("adapter_dropout")
    cfg["classifier"]["kwargs"]["first_session_training"] = False
    assert cfg == old


def test_restatement_matches_the_reference_blocks(golden):
    """tests/golden/adapter_tiny.npz comes from the reference's own Block / Adapter classes in fp64 (tools/gen_adapter_golden.py): branch placement,
    scale, LayerNorm eps and the gradients of the eight adapter tensors"""
    g = {k: torch.from_numpy(v) for k, v in golden("adapter_tiny").items()}
    P = {k: v for k, v in g.items() if k.startswith("feat.") and ".adaptmlp." not in k}
    names = ("down_proj.weight", "down_proj.bias", "up_proj.weight", "up_proj.bias")
    for hand in (True, False):
        Ad = [[g[f"feat.transformer.blocks.{i}.adaptmlp.{n}"].clone().requires_grad_(True) for n in names] for i in range(2)]
        outs = A.blocks(P, Ad, g["x"], hand=hand)
        (outs[-1] * g["gy"]).sum().backward()
        for i in range(2):
            assert _close(outs[i].detach(), g[f"block_out_{i}"], 1e-10)
            for t, n in zip(Ad[i], names):
                want = g[f"grad.blocks.{i}.adaptmlp.{n}"]
                assert float(want.abs().max()) > 0 and _close(t.grad, want, 1e-10), (i, n)
    # the fixture is sensitive to what it is there for: another scale or eps, or the branch fed from LN2's output, is far outside 1e-10
    Ad = [[g[f"feat.transformer.blocks.{i}.adaptmlp.{n}"] for n in names] for i in range(2)]
    assert not _close(A.blocks(P, Ad, g["x"], s=0.2)[-1], g["block_out_1"], 1e-6)
    assert not _close(A.blocks(P, Ad, g["x"], cfg=dict(A.TINY, block_eps=1e-5))[-1], g["block_out_1"], 1e-8)
