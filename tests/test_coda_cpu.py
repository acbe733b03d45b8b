"""CODA-Prompt without a device: tests/coda_ref.py against tests/golden/coda_tiny.npz (fp64 runs of the reference's own CodaPrompt pool, prompted ViT and
method; tools/gen_coda_golden.py), the seeded construction of the pool, and the plugin's host-side behaviour."""
import numpy as np
import pytest
import torch

import coda_ref as R
import libcontinual_amd.model as M
from libcontinual_amd.model.codaprompt import CodaPrompt
from libcontinual_amd.model.backbone.vit import CodaPromptPool

POOL_SEED = 2024                 # tools/gen_coda_golden.py


def _np(got):
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}


def test_restatement_matches_the_reference_run(golden):
    fix = golden("coda_tiny")
    got = _np(R.replay(fix, torch.float64))
    first, losses, worst = R.deviations(got, fix)
    assert first < 1e-10 and losses < 1e-10 and worst[0] < 1e-10, (first, losses, worst)
    np.testing.assert_array_equal(got["preds"], fix["preds"])
    np.testing.assert_array_equal(got["infer_preds"], fix["infer_preds"])
    assert sum(k.startswith("t") for k in got) == R.TASKS * R.STEPS * 17                  # 15 pool tensors and the head, after every step


def test_prefix_attention_is_plain_attention_over_the_packed_rows():
    """coda_ref.pack_prefix: the packed form the GPU kernel tests hand to vit_refs.attn_ref gives the prefix form's output and gradients"""
    import vit_refs as V
    B, N, Lp, H, hd = 2, 5, 3, 2, 8
    D = H * hd
    g = torch.Generator().manual_seed(5)
    qkv, dout = torch.randn(B * N, 3 * D, generator=g, dtype=torch.float64), torch.randn(B * N, D, generator=g, dtype=torch.float64)
    pk, pv = (torch.randn(B, Lp, D, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(2))
    x = qkv.clone().requires_grad_(True)
    out = R.prefix_attention(x.reshape(B, N, 3 * D), pk, pv, H)
    dx, dpk, dpv = torch.autograd.grad((out.reshape(B * N, D) * dout).sum(), (x, pk, pv))
    big, bd = R.pack_prefix(qkv, pk.detach(), pv.detach(), dout, B, N, Lp, D, qfill=torch.randn(B, Lp, D, generator=g, dtype=torch.float64))
    o, _, dq, dk, dv = V.attn_ref(big, bd, B, N + Lp, H, hd)
    tok = lambda t: t[:, :, Lp:].permute(0, 2, 1, 3).reshape(B * N, D)
    pre = lambda t: t[:, :, :Lp].permute(0, 2, 1, 3).reshape(B, Lp, D)
    assert float((tok(o) - out.detach().reshape(B * N, D)).abs().max()) < 1e-12
    assert float((torch.cat((tok(dq), tok(dk), tok(dv)), dim=1) - dx).abs().max()) < 1e-12
    assert float((pre(dk) - dpk).abs().max()) < 1e-12 and float((pre(dv) - dpv).abs().max()) < 1e-12
    assert float(pre(dq).abs().max()) == 0.0                                                # zero dout: the prefix rows' own queries get nothing


def test_seeded_pool_equals_the_reference_bit_for_bit(golden):
    fix = golden("coda_tiny")
    torch.manual_seed(POOL_SEED)
    pool = CodaPromptPool(R.CFG["dim"], R.TASKS, [R.POOL, R.LENGTH, 0.0], key_dim=R.CFG["dim"])
    sd = pool.state_dict()
    assert sorted(sd) == sorted(f"e_{w}_{l}" for w in "pka" for l in range(5))
    for k, v in sd.items():
        assert v.dtype == torch.float32 and v.is_contiguous()
        np.testing.assert_array_equal(v.numpy(), fix["pool0/" + k])


def _plugin(mu=0.0):
    bb = M.vit_pt_imnet(pretrained=False, img_size=32, patch_size=8, embed_dim=64, depth=6, num_heads=2, dtype="f32")
    return CodaPrompt(bb, "cpu", init_cls_num=3, inc_cls_num=3, task_num=2, num_class=6, feat_dim=64, pool_size=6, prompt_length=8, mu=mu)


def test_mu_above_zero_raises():
    with pytest.raises(NotImplementedError, match="mu"):
        _plugin(mu=0.1)


def test_task_count_stays_zero_and_rows_beyond_the_window_are_zero(golden):
    fix = golden("coda_tiny")
    model = _plugin()
    pool = model.network.backbone.prompt
    for t in range(2):
        model.before_task(t, None, None, None)
        assert pool.task_count == 0 and pool.window() == (0, 3)
        assert model.network.classifier.out_features == 3 * (t + 1)
        model.after_task(t, None, None, None)
    assert model.last_out_dim == 6
    for k, v in pool.state_dict().items():
        assert bool((v[3:] == 0).all()) and bool((v[:3] != 0).any())
        assert (fix["final_pool/" + k][3:] == 0).all() and (fix["pool0/" + k][3:] == 0).all()
    names = {n for n, _ in model.network.named_parameters()}
    got = {id(p) for p in model.get_parameters(None)}
    want = {id(p) for n, p in model.network.named_parameters() if n.startswith("backbone.prompt.") or n.startswith("classifier.")}
    assert got == want and "backbone.prompt.e_p_0" in names


def test_head_regrowth_keeps_the_old_rows_and_draws_like_a_fresh_linear():
    model = _plugin()
    model.before_task(0, None, None, None)
    w0 = model.network.classifier.weight.detach().clone()
    torch.manual_seed(11)
    model.before_task(1, None, None, None)
    torch.manual_seed(11)
    fresh = torch.nn.Linear(64, 6)
    w1 = model.network.classifier.weight.detach()
    assert torch.equal(w1[:3], w0) and torch.equal(w1[3:], fresh.weight.detach()[3:])


def test_process_task_count_moves_the_window():
    torch.manual_seed(3)
    pool = CodaPromptPool(64, 2, [6, 8, 0.0], key_dim=64)
    old = pool.e_k_0.detach().clone()
    pool.process_task_count()
    assert pool.task_count == 1 and pool.window() == (3, 6)
    assert torch.equal(pool.e_k_0[:3], old[:3]) and bool((pool.e_k_0[3:] != 0).any())
    gram = pool.e_k_0.detach() @ pool.e_k_0.detach().T
    assert float((gram - torch.eye(6)).abs().max()) < 1e-5


def test_shipped_config_carries_the_reference_settings():
    from libcontinual_amd.config import Config
    cfg = Config("config/codaprompt-vitb16-cifar100-b10x10.yaml").get_config_dict()
    assert cfg["classifier"]["name"] == "CodaPrompt" and cfg["backbone"]["name"] == "vit_pt_imnet"
    assert cfg["classifier"]["kwargs"] == {"num_class": 100, "task_num": 10, "init_cls_num": 10, "inc_cls_num": 10, "feat_dim": 768, "prompt_length": 8,
                                           "pool_size": 100, "mu": 0.0}
    assert cfg["optimizer"] == {"name": "Adam", "kwargs": {"lr": 0.001, "betas": [0.9, 0.999], "weight_decay": 0}}
    assert cfg["lr_scheduler"] == {"name": "CosineSchedule", "kwargs": {"K": 20}}
    assert (cfg["batch_size"], cfg["epoch"], cfg["val_per_epoch"], cfg["image_size"]) == (128, 20, 20, 224)
