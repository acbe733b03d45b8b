"""DualPrompt without a device: tests/dual_ref.py against tests/golden/dual_tiny.npz (fp64 runs of the reference's own DualPrompt pool, prompted ViT and
method; tools/gen_dual_golden.py), the conditions the generator wrote the fixture under, the seeded construction of the pool, and the plugin's host-side
behaviour."""
import numpy as np
import pytest
import torch

import dual_ref as R
import libcontinual_amd.model as M
from libcontinual_amd.model.dualprompt import DualPrompt
from libcontinual_amd.model.backbone.vit import DualPromptPool

POOLED = [n for n in R.names() if R.is_pooled(n)]


def _np(got):
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}


@pytest.fixture(scope="module")
def replayed(golden):
    fix = golden("dual_tiny")
    return fix, _np(R.replay(fix, torch.float64))


def test_restatement_matches_the_reference_run(replayed):
    fix, got = replayed
    first, losses, key_losses, worst = R.deviations(got, fix)
    assert first < 1e-10 and losses < 1e-10 and key_losses < 1e-10 and worst[0] < 1e-10, (first, losses, key_losses, worst)
    np.testing.assert_array_equal(got["preds"], fix["preds"])
    np.testing.assert_array_equal(got["infer_idx"], fix["infer_idx"])
    np.testing.assert_array_equal(got["infer_preds"], fix["infer_preds"])
    assert float(np.abs(got["infer_cos"] - fix["infer_cos"]).max()) < 1e-10
    trained = [k for k in got if k.startswith("t") and "/moved/" not in k]
    assert len(trained) == R.TASKS * R.STEPS * 10                                            # 8 pool tensors and the head, after every step
    assert bool((fix["key_losses"] > 0).all()) and bool((fix["key_losses"] < fix["losses"]).all())


def test_only_the_task_row_of_the_pooled_tensors_moves(replayed):
    """prompt.py:286-287 index row task_id alone: every other row of e_p_* / e_k_* gets a zero gradient, and a fresh Adam leaves it where it was"""
    fix, got = replayed
    for src in (fix, got):
        for t in range(R.TASKS):
            want = np.arange(R.POOL) == t
            for s in range(R.STEPS):
                for n in POOLED:
                    np.testing.assert_array_equal(src[f"t{t}/s{s}/moved/{n}"], want, err_msg=f"t{t}/s{s}/{n}")
    for n in POOLED:                                                                         # the whole pool at the end: rows >= TASKS never trained
        a, b = fix["final_pool/" + n], fix["pool0/" + n]
        assert np.array_equal(a[R.TASKS:], b[R.TASKS:]) and all((a[t] != b[t]).any() for t in range(R.TASKS))
        np.testing.assert_array_equal(a[R.TASKS - 1], fix[f"t{R.TASKS - 1}/s{R.STEPS - 1}/{n}"])
    for g in R.G_LAYERS:
        assert (fix[f"final_pool/g_p_{g}"] != fix[f"pool0/g_p_{g}"]).all()


def test_fixture_meets_the_conditions_it_was_generated_under(golden):
    fix = golden("dual_tiny")
    assert fix["infer_cos"].shape == (R.TASKS, len(R.E_LAYERS), R.INFER, R.POOL) and fix["infer_idx"].shape == (R.TASKS, len(R.E_LAYERS), R.INFER)
    assert float(R.gaps(fix["infer_cos"]).min()) >= R.GAP
    np.testing.assert_array_equal(fix["infer_cos"].argmax(-1), fix["infer_idx"])
    for l in range(len(R.E_LAYERS)):
        assert len(set(fix["infer_idx"][-1, l].tolist())) >= 2
    assert bool((fix["infer_idx"][0] >= 1).any())                     # after task 0 keys that no task has trained are already chosen
    for t in range(R.TASKS):
        ok = R.comparable(fix, t)
        assert int((~ok).sum()) <= 2, (t, fix["infer_margin"][t])
        np.testing.assert_array_equal(fix[f"infer_logits/t{t}"].argmax(1), fix["infer_preds"][t])
    assert float(fix["lr"]) == R.LR


def test_fp32_run_of_the_restatement_meets_the_f32_method_tolerances(golden):
    """the generator's last condition: what the GPU method test asks of the executor, an fp32 run of plain torch can deliver on this fixture"""
    fix = golden("dual_tiny")
    got = _np(R.replay(fix, torch.float32))
    first, losses, key_losses, worst = R.deviations(got, fix)
    assert first < 2e-4 and losses < 5e-3 and key_losses < 5e-3 and worst[0] < 5e-3, (first, losses, key_losses, worst)
    np.testing.assert_array_equal(got["infer_idx"], fix["infer_idx"])
    assert all(np.array_equal(got["preds"][t, 0], fix["preds"][t, 0]) for t in range(R.TASKS))


def test_seeded_pool_equals_the_reference_bit_for_bit(golden):
    fix = golden("dual_tiny")
    torch.manual_seed(int(fix["pool_seed"]))
    pool = DualPromptPool(R.CFG["dim"], R.TASKS, [R.POOL, R.LE, R.LG], key_dim=R.CFG["dim"])
    sd = pool.state_dict()
    assert list(sd) == R.names() == ["g_p_0", "g_p_1", "e_p_2", "e_k_2", "e_p_3", "e_k_3", "e_p_4", "e_k_4"]
    assert sorted("pool0/" + k for k in sd) == sorted(k for k in fix if k.startswith("pool0/"))
    for k, v in sd.items():
        assert v.dtype == torch.float32 and v.is_contiguous()
        np.testing.assert_array_equal(v.numpy(), fix["pool0/" + k])
    assert tuple(pool.g_p_0.shape) == (R.LG, 64) and tuple(pool.e_p_2.shape) == (R.POOL, R.LE, 64) and tuple(pool.e_k_2.shape) == (R.POOL, 64)


def _backbone():
    return M.vit_pt_imnet(pretrained=False, img_size=32, patch_size=8, embed_dim=64, depth=6, num_heads=2, dtype="f32")


def _plugin(task_num=3, g=6, e=8):
    return DualPrompt(_backbone(), "cpu", init_cls_num=3, inc_cls_num=3, task_num=task_num, num_class=3 * task_num, feat_dim=64, g_prompt_length=g,
                      e_prompt_length=e)


def test_what_the_reference_cannot_run_raises_at_construction():
    with pytest.raises(NotImplementedError, match="e_prompt_length"):
        _plugin(e=7)
    with pytest.raises(NotImplementedError, match="g_prompt_length"):
        _plugin(g=3)
    with pytest.raises(NotImplementedError, match="g_prompt_length"):
        _plugin(g=0)
    with pytest.raises(NotImplementedError, match="task_num 11"):
        _plugin(task_num=11)
    _plugin(task_num=10)
    with pytest.raises(NotImplementedError, match="key_dim"):
        _backbone().create_prompt("dual", n_tasks=3, prompt_param=[10, 8, 6], key_dim=32)
    with pytest.raises(NotImplementedError, match="key_dim"):
        DualPromptPool(64, 3, [10, 8, 6])                             # the reference's default, 768


def test_create_prompt_builds_the_pool_at_the_backbone_width():
    bb = _backbone()
    bb.create_prompt("dual", n_tasks=3, prompt_param=[10, 8, 6])
    assert isinstance(bb.prompt, DualPromptPool) and bb.prompt_flag == "dual" and bb.prompt.key_d == 64 and bb.prompt.e_pool_size == 10
    assert M.DualPrompt is DualPrompt and DualPrompt.cuda_graph_safe is False


def test_plugin_head_and_parameters():
    model = _plugin()
    pool = model.network.backbone.prompt
    assert (pool.e_pool_size, pool.e_p_length, pool.g_p_length, pool.g_layers, pool.e_layers) == (10, 8, 6, [0, 1], [2, 3, 4])
    for t in range(3):
        model.before_task(t, None, None, None)
        assert model.network.backbone.task_id == t and model.network.classifier.out_features == 3 * (t + 1)
        assert model.last_out_dim == 3 * t
        model.after_task(t, None, None, None)
    got = [id(p) for p in model.get_parameters(None)]
    want = {id(p) for n, p in model.network.named_parameters() if n.startswith("backbone.prompt.") or n.startswith("classifier.")}
    assert len(got) == len(set(got)) == 10 and set(got) == want


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


def test_shipped_config_carries_the_reference_settings():
    from libcontinual_amd.config import Config
    cfg = Config("config/dualprompt-vitb16-cifar100-b10x10.yaml").get_config_dict()
    assert cfg["classifier"]["name"] == "DualPrompt" and cfg["backbone"]["name"] == "vit_pt_imnet"
    assert cfg["classifier"]["kwargs"] == {"num_class": 100, "task_num": 10, "init_cls_num": 10, "inc_cls_num": 10, "feat_dim": 768, "g_prompt_length": 6,
                                           "e_prompt_length": 20}
    assert cfg["optimizer"] == {"name": "Adam", "kwargs": {"lr": 0.001, "betas": [0.9, 0.999], "weight_decay": 0}}
    assert cfg["lr_scheduler"] == {"name": "MultiStepLR", "kwargs": {"gamma": 0.1, "milestones": [80, 120]}}
    assert (cfg["batch_size"], cfg["epoch"], cfg["val_per_epoch"], cfg["image_size"]) == (128, 10, 5, 224)
    import torch.optim.lr_scheduler as S
    assert hasattr(S, cfg["lr_scheduler"]["name"])
