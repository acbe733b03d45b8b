"""tests/lorasub_ref.py on the CPU: its triplet loss against a literal restatement of the reference's loop (lora_sub.py:34-68) and of its autograd, its Adam step
against torch.optim.Adam, its factor gradients against autograd, and its fp32 bounds against an fp32 evaluation of the same formulas (a bound the plain fp32
CPU arithmetic already breaks would be no yardstick for the kernels).  And the C ABI of csrc/lorasub.hip: declared, bound, built.
"""
import os

import torch

import lorasub_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loop_atl(f, y, protos, margin):
    """the loss as the reference writes it: the expanded squared distances, a loop over the batch, a loop over batch x prototypes"""
    x = f / f.norm(dim=1, keepdim=True)
    B = x.shape[0]
    sq = (x * x).sum(1, keepdim=True)
    dist = (sq + sq.T - 2.0 * x @ x.T).clamp(min=1e-12).sqrt()
    same = y[:, None] == y[None, :]
    ap, an = [], []
    for i in range(B):
        ap.append(dist[i][same[i]].max())
        an.append(dist[i][~same[i]].min() if bool((~same[i]).any()) else ap[-1] + margin)
    if protos is not None and len(protos):
        c = protos / protos.norm(dim=1, keepdim=True)
        for i in range(B):
            for p in range(len(c)):
                e = (x[i] - c[p]).norm().clamp(min=1e-12)
                if float(e.detach()) < float(an[i].detach()):
                    an[i] = e
    return torch.relu(torch.stack(ap) - torch.stack(an) + margin).mean()


def _random_case(B, D, P, classes, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(B, D, generator=g, dtype=torch.float64) + 2.0 * torch.randn(classes, D, generator=g, dtype=torch.float64)[torch.arange(B) % classes]
    y = torch.arange(B) % classes + 5
    pr = torch.randn(P, D, generator=g, dtype=torch.float64) + 1.0 if P else None
    return f, y, pr


def test_atl_matches_the_reference_loop_and_its_autograd():
    for B, D, P, classes, margin in ((9, 16, 0, 3, 1.0), (9, 16, 4, 3, 1.0), (12, 32, 5, 12, 1.0), (7, 16, 3, 1, 1.0), (7, 16, 0, 1, 1.0), (10, 16, 6, 2, 0.3)):
        f, y, pr = _random_case(B, D, P, classes, 100 + B + P)
        loss, df, info = R.atl(f, y, pr, margin, weight=0.05)
        fr = f.clone().requires_grad_(True)
        want = _loop_atl(fr, y, pr, margin)
        gw = torch.autograd.grad(want, fr)[0] if want.requires_grad else torch.zeros_like(f)
        if classes == 1 and P == 0:
            # ap - (ap + margin) + margin: the reference's two paths cancel to rounding; the restatement says 0
            assert float(loss) == 0.0 and float(want.detach()) < 1e-12 and float(gw.abs().max()) < 1e-12
            continue
        assert abs(float(loss) - float(want.detach())) < 1e-10, (B, P, classes)
        assert float((df - 0.05 * gw).abs().max()) < 1e-10, (B, P, classes)
        if P:
            assert info["gap"] > 0


def test_atl_bounds_hold_an_fp32_evaluation():
    for B, D, P, classes in ((9, 64, 4, 3), (33, 128, 7, 10)):
        for draw in range(50):                                                                       # drawn until the case is comparable; none is skipped
            f, y, pr = _random_case(B, D, P, classes, 7 + B + 1000 * draw)
            f32, p32 = f.float(), pr.float()
            loss, df, e_loss, e_df, info = R.atl_bounded(f32, y, p32, 1.0, 0.05)
            if info["gap"] >= R.SEP:
                break
        assert info["gap"] >= R.SEP, (B, D, info["gap"])
        l32, d32, _ = R.atl(f32, y, p32, 1.0, 0.05)
        assert abs(float(l32) - float(loss)) <= e_loss
        assert bool(((d32.double() - df).abs() <= e_df).all())
        assert float(e_df.max()) < 1e-3 * float(df.abs().max())                                      # ... and the bound says something


def test_proj_adam_is_adam_and_the_transform_multiplies_the_update():
    g = torch.Generator().manual_seed(1)
    D, r = 16, 3
    for shape in ((D, r), (r, D)):
        p0 = torch.randn(shape, generator=g, dtype=torch.float64)
        p = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adam([p], lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
        mine, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        T = torch.randn(D, D, generator=g, dtype=torch.float64)
        proj, pm, pv = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        for step in range(1, 4):
            grad = torch.randn(shape, generator=g, dtype=torch.float64)
            p.grad = grad.clone()
            before = p.detach().clone()
            opt.step()
            mine, m, v = R.proj_adam(mine, grad, m, v, None, 5e-4, 0.9, 0.999, 1e-8, 1e-2, step)
            assert float((mine - p.detach()).abs().max()) < 1e-14
            # the projected step from the same state: the plain update, multiplied (lora_sub.py:143-156)
            upd = p.detach() - before
            proj, pm, pv = R.proj_adam(before, grad, pm, pv, T, 5e-4, 0.9, 0.999, 1e-8, 1e-2, step)
            assert float((proj - (before + (T @ upd if shape[0] == D else upd @ T))).abs().max()) < 1e-14


def test_grads_ab_match_autograd():
    g = torch.Generator().manual_seed(2)
    M, D, r = 11, 16, 3
    X, dY = torch.randn(M, D, generator=g, dtype=torch.float64), torch.randn(M, 3 * D, generator=g, dtype=torch.float64)
    W = torch.randn(3 * D, D, generator=g, dtype=torch.float64)
    fac = [torch.randn(*s, generator=g, dtype=torch.float64, requires_grad=True) for s in ((r, D), (D, r), (r, D), (D, r))]
    Weff = torch.cat([W[:D], W[D:2 * D] + fac[1] @ fac[0], W[2 * D:] + fac[3] @ fac[2]])
    want = torch.autograd.grad(((X @ Weff.T) * dY).sum(), fac)
    got = R.grads_ab(X, dY, *[t.detach() for t in fac])
    assert all(float((a - b).abs().max()) < 1e-12 for a, b in zip(got, want))
    # the bounds hold an fp32 evaluation of the same products
    f32 = [t.detach().float() for t in fac]
    w64, bound = R.grads_ab_bounded(X.float().double(), dY.float().double(), f32, lambda t: t.double(), 0.0)
    got32 = R.grads_ab(X.float(), dY.float(), *f32)
    assert all(bool(((a.double() - b).abs() <= c).all()) for a, b, c in zip(got32, w64, bound))


# --------------------------------------------------------------------------------------------------------------- the host classes
def _toy(**kw):
    import libcontinual_amd.model as M
    bb = M.vit_pt_imnet(pretrained=False, attn_layer="MultiHeadAttention_LoRA_Sub", img_size=32, patch_size=8, embed_dim=64, depth=3, num_heads=2, dtype="f32",
                        lora_rank=4, **kw)
    return M, bb, M.LoRAsub_DRS(bb, "cpu", init_cls_num=3, inc_cls_num=3, task_num=3, embd_dim=64, fc_lrate=2e-3, margin_inter=1.0, lambada=0.05)


def test_init_param_draws_what_the_reference_draws(golden):
    """under seed 4321 three modules in a row draw, bit for bit, what the reference's MultiHeadAttention_LoRA_Sub.init_param drew (the fixture's `draw/`)"""
    fix = golden("lorasub_tiny")
    M, bb, model = _toy()
    torch.manual_seed(4321)
    for a in model.attention_modules:
        a.init_param()
    for b, a in enumerate(model.attention_modules):
        for n in R.FACTORS:
            assert torch.equal(getattr(a, n).weight.detach(), torch.from_numpy(fix[f"draw/{b}/{n}"])), (b, n)
        assert a.apply_lora and float(a.lora_A_k.weight.detach().abs().max()) > 0 and float(a.lora_B_k.weight.detach().abs().max()) == 0


_RUN = {}


def _run64(fix):
    if "got" not in _RUN:
        _RUN["got"] = R.run_fixture(fix)
    return _RUN["got"]


def test_ref_matches_fixture(golden):
    """tests/lorasub_ref.py in fp64 against the fp64 runs of the reference's own classes (tools/gen_lorasub_golden.py): 1e-10 of max-abs on what the fixture
    stores in fp64 (losses, triplet terms, every trained tensor after each of the 3 x 3 steps, prototypes), fp32 rounding on what it stores in fp32 (G, T,
    prev -- which the fp64 quantities of the later steps and tasks depend on), and k, the predictions and the inference predictions equal"""
    fix = golden("lorasub_tiny")
    got = _run64(fix)
    d = R.deviations(got, fix)
    print(d)
    assert d["losses"] < 1e-10 and d["atl"] < 1e-10 and d["worst"][0] < 1e-10 and d["protos"] < 1e-10, d
    assert d["T"] < 1e-6 and d["G"] < 1e-6 and d["prev"] < 1e-6, d
    assert len([k for k in got if "/s" in k]) == 3 * 3 * 14
    for t in range(3):
        if t:
            assert list(got[f"t{t}/k"]) == fix[f"t{t}/k"].tolist() and R.rel(got[f"t{t}/S"], fix[f"t{t}/S"]) < 1e-9
        assert torch.equal(got[f"t{t}/infer_pred"], torch.from_numpy(fix[f"t{t}/infer_pred"]))
    assert torch.equal(got["preds"], torch.from_numpy(fix["preds"]))


def test_fixture_conditions(golden):
    """the conditions the generator wrote the file under, asserted again: (a) the cut of every layer 1e-4 from 0.99, (b) every selection and hinge argument
    1e-3 apart, active rows, prototype negatives from task 1 on, (c) an fp32 CPU run of the restatement within the f32 tolerances of the GPU test"""
    fix = golden("lorasub_tiny")
    assert int(fix["seed"]) >= 99
    assert R.condition_a(fix) == ""
    assert R.condition_b(_run64(fix)) == ""
    assert R.check_f32(R.run_fixture(fix, torch.float32), fix) == ""
    assert fix["y"].tolist() == [[[0 + 3 * t, 1 + 3 * t, 2 + 3 * t] * 3] * 3 for t in range(3)]


def test_before_task_leaves_the_reference_names_trainable(golden):
    fix = golden("lorasub_tiny")
    M, bb, model = _toy()
    model.before_task(0, None, None, None)
    assert sorted(n for n, p in model._network.named_parameters() if p.requires_grad) == [str(n) for n in fix["t0/trainable"]]
    assert sorted(dict(model._network.named_parameters())) == sorted(set(str(n).replace("classifier_pool.1.", "classifier_pool.0.").replace(
        "classifier_pool.2.", "classifier_pool.0.") for t in range(3) for n in fix[f"t{t}/trainable"]) | {n for n, _ in model._network.named_parameters()
                                                                                                          if "lora" not in n and "classifier_pool.0." not in n})


def test_trainable_names_groups_and_weight_forms():
    M, bb, model = _toy()
    names = sorted(k for k in bb.state_dict() if "blocks.0.attn" in k)
    assert [n.split("attn.")[1] for n in names] == ["lora_A_k.weight", "lora_A_v.weight", "lora_B_k.weight", "lora_B_v.weight", "prev_k_weight", "prev_v_weight",
                                                    "proj.bias", "proj.weight", "qkv.bias", "qkv.weight"]
    model.before_task(0, None, None, None)
    want = ["classifier_pool.0.bias", "classifier_pool.0.weight"] + [f"backbone.feat.transformer.blocks.{b}.attn.{n}.weight" for b in range(3) for n in R.FACTORS]
    assert sorted(n for n, p in model._network.named_parameters() if p.requires_grad) == sorted(want)
    opt = model.get_optimizer(5e-4, 0.0)
    assert [g["lr"] for g in opt.param_groups] == [5e-4, 2e-3] and [len(g["params"]) for g in opt.param_groups] == [12, 2]
    assert opt.param_groups[0]["svd"] and opt.param_groups[0]["thres"] == 0.99 and opt.transforms is None
    from libcontinual_amd.scheduler import CosineSchedule
    sch = CosineSchedule(opt, K=20)
    sch.step(); sch.step(); sch.step()
    assert opt.param_groups[0]["lr"] < 5e-4 and abs(opt.param_groups[1]["lr"] / opt.param_groups[0]["lr"] - 4.0) < 1e-9
    # the three forms of the k / v rows, composed without touching the pretrained weight
    a = model.attention_modules[0]
    w0 = a.qkv.weight.detach().clone()
    with torch.no_grad():
        a.lora_B_k.weight.uniform_(-0.1, 0.1); a.lora_B_v.weight.uniform_(-0.1, 0.1)
    a.save_weight()
    assert not a.apply_lora and torch.equal(a.prev_k_weight, a.lora_B_k.weight @ a.lora_A_k.weight)
    plus = a.executor_weight()
    assert torch.equal(plus[:64], w0[:64]) and torch.equal(plus[64:128], w0[64:128] + a.prev_k_weight) and torch.equal(plus[128:], w0[128:] + a.prev_v_weight)
    a.subtract = True
    minus = a.executor_weight()
    assert torch.equal(minus[64:128], w0[64:128] - a.prev_k_weight) and torch.equal(a.qkv.weight, w0)
    assert "_w_plus" not in bb.state_dict() and not any("_w_" in k for k in bb.state_dict())


def test_refusals_of_the_host_classes():
    import pytest
    import libcontinual_amd.model as M
    with pytest.raises(NotImplementedError, match="lora_bias"):
        _toy(lora_bias=True)
    plain = M.vit_pt_imnet(pretrained=False, img_size=32, patch_size=8, embed_dim=64, depth=1, num_heads=2)
    with pytest.raises(ValueError, match="MultiHeadAttention_LoRA_Sub"):
        M.LoRAsub_DRS(plain, "cpu", init_cls_num=3, inc_cls_num=3, task_num=3, embd_dim=64, fc_lrate=2e-3, margin_inter=1.0, lambada=0.05)
    M_, bb, model = _toy()
    with pytest.raises(NotImplementedError):
        model.attention_modules[0].merge_weight()
    with pytest.raises(RuntimeError, match="prototypes"):
        model.inference({"image": torch.zeros(1, 3, 32, 32), "label": torch.zeros(1, dtype=torch.int64)})
    assert model.cuda_graph_safe is False


def test_c_abi_symbols_are_declared_and_bound():
    from libcontinual_amd import _lib
    declared = _lib.header_symbols()
    for n in ("clhip_atl", "clhip_atl_ws_bytes", "clhip_lora_grad_ab", "clhip_lora_grad_ab_ws_bytes", "clhip_proj_adam_multi", "clhip_vit_lora_refresh_ab",
              "clhip_vit_backward"):
        assert n in declared and n in _lib._PROTOS
        assert hasattr(_lib.lib(), n)
    with open(os.path.join(ROOT, "include", "clhip.h")) as f:
        text = f.read()
    assert "lora_sub.py:34-68" in text and "lora_sub.py:120-157" in text and "transformer.py:401-424" in text
    with open(os.path.join(ROOT, "libcontinual_amd", "csrc", "build.sh")) as f:
        assert " lorasub " in f.read()


def test_host_side_refusals_need_no_device():
    """every entry point checks its arguments before it touches the device: the refusals answer on a machine without one"""
    from libcontinual_amd import _lib
    L = _lib.lib()
    one = 1 << 12                                                 # any non-null address: never dereferenced
    assert L.clhip_atl(one, one, None, 0, 64, 0, 1.0, 1.0, one, one, one, None) != 0 and b"B = 0" in L.clhip_last_error()
    assert L.clhip_atl(one, one, None, 4, 96, 0, 1.0, 1.0, one, one, one, None) != 0 and b"D = 96" in L.clhip_last_error()
    assert L.clhip_atl(one, one, None, 4, 64, 2, 1.0, 1.0, one, one, one, None) != 0 and b"protos" in L.clhip_last_error()
    assert L.clhip_atl(one, one, one, 4, 64, 1025, 1.0, 1.0, one, one, one, None) != 0 and b"P = 1025" in L.clhip_last_error()
    assert L.clhip_lora_grad_ab(*[one] * 11, 8, 64, 17, _lib.F32, None) != 0 and b"rank 17" in L.clhip_last_error()
    assert L.clhip_lora_grad_ab(*[one] * 11, 0, 64, 4, _lib.F32, None) != 0 and b"M = 0" in L.clhip_last_error()
    assert L.clhip_proj_adam_multi(6, one, None, None, 64, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None) != 0 and b"count = 6" in L.clhip_last_error()
    assert L.clhip_proj_adam_multi(4, one, one, None, 64, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None) != 0 and b"workspace" in L.clhip_last_error()
    assert L.clhip_atl_ws_bytes(128, 90) > 0 and L.clhip_lora_grad_ab_ws_bytes(394, 768) > 0 and L.clhip_lora_grad_ab_ws_bytes(0, 768) == 0
