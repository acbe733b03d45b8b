"""SD-LoRA without a GPU: tests/sdlora_ref.py (the effective-weight form the HIP path computes) against tests/golden/sdlora_tiny.npz -- fp64 runs of the
reference's own MultiHeadAttention_SDLoRA and SD_LoRA (tools/gen_sdlora_golden.py) -- at 1e-10, and the host-side logic of model/sd_lora.py: the
parameter-name filter, the rank-reduction schedule, the magnitude re-initialisation and the knowledge_dist guard."""
import numpy as np
import pytest
import torch

import sdlora_ref as R
import libcontinual_amd.model as M

TOL = 1e-10


def _err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


@pytest.fixture(scope="module")
def fix(golden):
    return golden("sdlora_tiny")


def test_attention_module_matches_reference(fix):
    w = {k[4:]: torch.from_numpy(v) for k, v in fix.items() if k.startswith("a/w/")}
    T1 = 4
    fac = {n: [w[f"{n}.{i}.weight"].clone() for i in range(T1)] for n in R.LISTS}
    assert [a.shape[0] for a in fac["lora_A_q_list"]] == [10, 10, 8, 6]
    assert float(fac["lora_B_v_list"][1].abs().max()) == 0.0 and all(float(b.abs().max()) > 0 for b in fac["lora_B_q_list"])
    mag = [w[f"mag_lora.{i}"].clone().reshape(()).requires_grad_(True) for i in range(T1)]
    for n in R.LISTS:
        fac[n][-1].requires_grad_(True)
    Aq, Bq, Av, Bv = (fac[n] for n in R.LISTS)
    assert float(R.inv_norms(Av, Bv)[1]) == 0.0                                   # the skipped term
    P = {"attn.qkv.weight": w["qkv.weight"], "attn.qkv.bias": w["qkv.bias"], "attn.proj.weight": w["proj.weight"], "attn.proj.bias": w["proj.bias"]}
    x, gy = torch.from_numpy(fix["a/x"]), torch.from_numpy(fix["a/gy"])
    y = R.attention(x, P, "", 2, R.effective_qkv(w["qkv.weight"], Aq, Bq, Av, Bv, mag))
    assert _err(y.detach(), fix["a/y"]) < TOL
    (y * gy).sum().backward()
    for n in R.LISTS:
        assert _err(fac[n][-1].grad, fix[f"a/grad/{n}"]) < TOL, n
    assert _err(torch.stack([m.grad for m in mag]), fix["a/grad/mag"]) < TOL
    # the closed-form gradients the kernels implement, from the same dqkv
    D = 64
    X = x.reshape(-1, D)
    W_eff = R.effective_qkv(w["qkv.weight"], Aq, Bq, Av, Bv, mag).detach()
    qkv = (X @ W_eff.T + w["qkv.bias"]).requires_grad_(True)
    B_, N_ = x.shape[:2]
    q, k, v = qkv.reshape(B_, N_, 3, 2, D // 2).permute(2, 0, 3, 1, 4)
    o = ((q @ k.transpose(-2, -1)) * (D // 2) ** -0.5).softmax(-1) @ v
    yy = torch.nn.functional.linear(o.transpose(1, 2).reshape(B_, N_, D), w["proj.weight"], w["proj.bias"])
    (yy * gy).sum().backward()
    det = lambda ts: [t.detach() for t in ts]
    got = R.grads(X, qkv.grad, det(Aq), det(Bq), det(Av), det(Bv), det(mag), R.inv_norms(Aq, Bq), R.inv_norms(Av, Bv))
    for g, n in zip(got[:4], R.LISTS):
        assert _err(g, fix[f"a/grad/{n}"]) < TOL, n
    assert _err(got[4], fix["a/grad/mag"]) < TOL


def run_method_ref(fix, dtype=torch.float64):
    m = R.Method({k[4:]: torch.from_numpy(v) for k, v in fix.items() if k.startswith("m/w/")}, dtype)
    x = torch.from_numpy(fix["m/x_u8"]).to(dtype) / 255.0
    y = torch.from_numpy(fix["m/y"])
    losses, states = [], {}
    for t in range(x.shape[0]):
        names = [str(n) for n in fix[f"m/t{t}/trainable"]]
        m.start_task(t, {n: fix[f"m/t{t}/init/{n}"] for n in names})
        for s in range(x.shape[1]):
            loss, pred = m.step(x[t, s], y[t, s])
            losses.append(float(loss))
            states[(t, s)] = ({n: p.detach().clone() for n, p in m.train.items()}, pred)
        m.end_task()
    return np.array(losses).reshape(x.shape[0], x.shape[1]), states


def test_method_matches_reference(fix):
    losses, states = run_method_ref(fix)
    assert _err(losses, fix["m/losses"]) < TOL
    for (t, s), (params, pred) in states.items():
        np.testing.assert_array_equal(pred.numpy(), fix["m/preds"][t, s])
        for n, p in params.items():
            assert _err(p, fix[f"m/t{t}/s{s}/{n}"]) < TOL, (t, s, n)
    assert _err(states[(1, 2)][0]["backbone.feat.transformer.blocks.0.attn.mag_lora.0"], 1.0) > 1e-4          # the magnitudes did move


def _model(**kw):
    bb = M.vit_pt_imnet(pretrained=False, attn_layer="MultiHeadAttention_SDLoRA", lora_rank=4, img_size=32, patch_size=8, embed_dim=64, depth=2, num_heads=2,
                        dtype="f32")
    args = dict(init_cls_num=3, inc_cls_num=3, task_num=3, init_mag=1.0, rank_reduction=[False, 4, 8, 8, 6], knowledge_dist=[False, 9e-4], embd_dim=64)
    args.update(kw)
    return M.SD_LoRA(bb, "cpu", **args)


def test_name_filter_selects_the_reference_names(fix):
    m = _model()
    for t in range(3):
        m.before_task(t, None, None, None)
        got = sorted(n for n, p in m._network.named_parameters() if p.requires_grad)
        assert got == R.trainable_names(t)
        if t < 2:
            assert got == [str(n) for n in fix[f"m/t{t}/trainable"]]                # what the reference's own filter selected
        assert m._network.classifier.out_features == 3 * (t + 1)
        m.after_task(t, None, None, None)
        assert m._known_classes == 3 * (t + 1)


def test_head_growth_keeps_old_rows():
    m = _model()
    m.before_task(0, None, None, None)
    w0, b0 = m._network.classifier.weight.detach().clone(), m._network.classifier.bias.detach().clone() + 0.5
    with torch.no_grad():
        m._network.classifier.bias.add_(0.5)
    m.before_task(1, None, None, None)
    c = m._network.classifier
    assert torch.equal(c.weight[:3], w0) and torch.equal(c.bias[:3], b0) and float(c.bias[3:].detach().abs().max()) == 0.0
    bound = (3.0 / 64) ** 0.5                                                       # kaiming_uniform_, nonlinearity 'linear'
    assert 0.5 * bound < float(c.weight[3:].detach().abs().max()) <= bound


def test_rank_reduction_schedule():
    m = _model(rank_reduction=[True, 1, 2, 3, 2])
    for t in range(3):
        m.before_task(t, None, None, None)
    for a in m.attention_modules:
        assert [h.weight.shape[0] for h in a.lora_A_q_list] == [4, 3, 2] and [h.weight.shape[1] for h in a.lora_B_v_list] == [4, 3, 2]
        assert [tuple(h.weight.shape) for h in a.lora_A_v_list] == [(4, 64), (3, 64), (2, 64)]
        assert float(a.lora_B_q_list[-1].weight.detach().abs().max()) == 0.0 and float(a.lora_A_q_list[-1].weight.detach().abs().max()) > 0.0
    m = _model()                                                                    # flag off: the rank stays
    for t in range(3):
        m.before_task(t, None, None, None)
    assert [h.weight.shape[0] for h in m.attention_modules[0].lora_A_q_list] == [4, 4, 4]


def test_magnitudes_are_recreated_and_shared():
    m = _model(init_mag=0.7)
    m.before_task(0, None, None, None)
    first = m.attention_modules[0].mag_lora
    with torch.no_grad():
        first[0].fill_(3.0)
    m.before_task(1, None, None, None)
    mag = m.attention_modules[0].mag_lora
    assert mag is not first and len(mag) == 2 and all(abs(float(p.detach()) - 0.7) < 1e-7 and tuple(p.shape) == (1,) and p.requires_grad for p in mag)
    assert all(a.mag_lora is mag for a in m.attention_modules)
    assert all(len(a.assimilated_mag_lora_q) == 2 and len(a.assimilated_mag_lora_v) == 2 for a in m.attention_modules)
    inv = m._network.backbone.feat._s.sd_inv
    assert tuple(inv.shape) == (2, 2, 2) and float(inv[:, :, -1].min()) == 1.0 and float(inv[:, :, 0].abs().max()) == 0.0      # B of task 0 stayed zero


def test_knowledge_dist_is_refused():
    with pytest.raises(NotImplementedError, match="alphas.solution"):
        _model(knowledge_dist=[True, 9e-4])


def test_unknown_attention_layer_still_refused():
    with pytest.raises(NotImplementedError):
        M.vit_pt_imnet(pretrained=False, attn_layer="MultiHeadAttention_CL_LoRA", img_size=32, patch_size=8, embed_dim=64, depth=2, num_heads=2)
