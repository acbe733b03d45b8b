"""The CLIP path without a device: tests/clip_ref.py against the fixture of the reference's own run, its bounds against fp32 evaluations of the same formulas,
the package's CLIP module tree, the C interface as text, the shipped config, every refusal, the tokenizer and the datasets' class names."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import clip_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _fix():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "clip_tiny.npz"), allow_pickle=False))


@functools.lru_cache(maxsize=None)
def _run(dtype):
    return R.run_fixture(_fix(), dtype)


# ------------------------------------------------------------------------------------------------ the restatement and the fixture's conditions
def test_restatement_reproduces_the_reference_run():
    d = R.deviations(_run(torch.float64), _fix())
    assert max(d[k] for k in ("losses", "logits", "lora_B", "lora_A", "bases", "txt")) < 1e-10 and d["preds_equal"], d


def test_condition_a_rank_cuts_are_clear_of_their_thresholds():
    m = _run(torch.float64)["margins"]
    assert len(m) >= R.CFG["depth"] * R.TASKS and R.condition_a(m) == "", min(m)


def test_condition_b_no_prediction_is_excused():
    assert R.condition_b(_fix()) == ""
    assert all(R.bf16_gate(k) <= 4.0 * v for k, v in R.BF16_MEASURED.items()) and R.bf16_gate("logits") == 0.0716     # 4 x the measurement, or tighter
    assert R.bf16_gate("lora_B_rms") < 1.0                                 # an untrained lora_B deviates by exactly 1 in this measure


def test_condition_c_an_fp32_run_meets_the_f32_tolerances():
    assert R.check_f32(_run(torch.float32), _fix()) == ""


def test_fixture_is_no_larger_than_the_largest_before_it():
    gold = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(gold, "clip_tiny.npz")) <= os.path.getsize(os.path.join(gold, "lorasub_tiny.npz"))
    assert os.path.getsize(os.path.join(gold, "clip_tokens.npz")) < 64 * 1024


# ------------------------------------------------------------------------------------------------ QuickGELU
def test_quickgelu_derivative_against_autograd_and_its_suprema():
    x = torch.linspace(-30, 30, 200001, dtype=torch.float64, requires_grad=True)
    y, h = R.qgelu_both(x)
    (g,) = torch.autograd.grad((x * torch.sigmoid(1.702 * x)).sum(), x, create_graph=True)
    assert float((h - g).detach().abs().max()) < 1e-14 and float((y - x * torch.sigmoid(1.702 * x)).detach().abs().max()) < 1e-14
    (g2,) = torch.autograd.grad(g.sum(), x)
    assert float((R.qgelu_d2(x).detach() - g2).abs().max()) < 1e-13
    assert 1.09 < float(h.detach().abs().max()) <= R.QGELU_D1_MAX and 0.85 < float(g2.abs().max()) <= R.QGELU_D2_MAX
    big = torch.tensor([1e3, -1e3, 1e4, -1e4], dtype=torch.float64)          # exp(-1702) underflows in fp64: s is exactly 1 or 0, nothing is inf or NaN
    yb, hb = R.qgelu_both(big)
    assert torch.equal(yb, torch.tensor([1e3, -0.0, 1e4, -0.0], dtype=torch.float64)) and torch.equal(hb, torch.tensor([1.0, 0.0, 1.0, 0.0], dtype=torch.float64))


def _kernel_form_f32(x):
    """the epilogue's arithmetic in fp32 torch: one exp of -|t|, one reciprocal"""
    x = x.float()
    t = x * 1.702
    e = torch.exp(-t.abs())
    r = 1.0 / (1.0 + e)
    s, c = torch.where(t >= 0, r, e * r), torch.where(t >= 0, e * r, r)
    return x * s, t * s * c + s


def test_quickgelu_bound_holds_for_an_fp32_evaluation_and_is_not_vacuous():
    x = torch.cat([torch.linspace(-110, 110, 100001), torch.linspace(-6, 6, 100001), torch.tensor([0.0, -0.0, 2.0 ** -20, 1 / 1.702, 20.0, 61.0, 100.0])])
    y, h = _kernel_form_f32(x)
    cref, href = R.qgelu_both(x)
    zero = torch.zeros_like(cref)[None]
    bc, bh = R.qgelu_bound(zero, 64, x.double()[None], cref[None], href[None], "f32")
    assert bool(((y.double() - cref).abs() <= bc[0]).all()) and bool(((h.double() - href).abs() <= bh[0]).all())
    assert bool(y.isfinite().all()) and bool(h.isfinite().all())
    # not vacuous: the erf GELU, or a sigmoid slope of 1.7 instead of 1.702, is far outside
    gel = 0.5 * x.double() * (1 + torch.erf(x.double() / math.sqrt(2)))
    assert float(((gel - cref).abs() / bc[0]).max()) > 1e3
    assert float((((x.double() * torch.sigmoid(1.7 * x.double())) - cref).abs() / bc[0]).max()) > 1e2
    assert R.c_q() >= R.C_Q_FLOOR and R.C_Q_MEASURED is not None


# ------------------------------------------------------------------------------------------------ the logits bounds
@pytest.mark.parametrize("B,D,E,Cn", [(1, 64, 32, 1), (5, 64, 32, 3), (9, 128, 64, 20), (33, 768, 512, 100)])
def test_logits_bounds_hold_for_an_fp32_evaluation_and_are_not_vacuous(B, D, E, Cn):
    g = torch.Generator().manual_seed(B)
    feat, proj = torch.randn(B, D, generator=g), torch.randn(D, E, generator=g) * D ** -0.5
    txt = torch.nn.functional.normalize(torch.randn(Cn, E, generator=g).double(), dim=1).float()
    dl = torch.randn(B, Cn, generator=g) / B
    for scale in (1 / 0.07, 100.0):
        lref, uref, iref = R.logits_ref(feat, proj, txt, scale)
        u = feat @ proj
        inv = 1 / u.norm(dim=1)
        n = u * inv[:, None]
        bl, (bu, bi), bd = R.logits_bound(feat, proj, txt, scale), R.saved_bound(feat, proj), R.dfeat_bound(dl, feat, proj, txt, scale)
        gg = scale * (dl @ txt)
        df = ((gg - n * (n * gg).sum(1, keepdim=True)) * inv[:, None]) @ proj.T
        dref = R.dfeat_ref(dl, proj, txt, scale, uref, iref)
        for got, ref, b in ((scale * (n @ txt.T), lref, bl), (u, uref, bu), (inv, iref, bi), (df, dref, bd)):
            assert bool(((got.double() - ref).abs() <= b).all())
        # not vacuous: a product that loses its last term, or logits 1 % off, are outside
        lost = scale * ((feat[:, :-1] @ proj[:-1]) / (feat[:, :-1] @ proj[:-1]).norm(dim=1, keepdim=True)).double() @ txt.double().T
        assert float(((lost - lref).abs() / bl).max()) > 1.0
        assert float(((lref * 1.01 - lref).abs() / bl).max()) > 1.0
        assert float(((dref / iref[:, None] - dref).abs() / bd).max()) > 1.0 or Cn == 1       # a backward that forgets one factor 1 / |u| (C = 1: dfeat is 0 in any form)


# ------------------------------------------------------------------------------------------------ the package's module tree
def _tiny_clip(**kw):
    import libcontinual_amd.model as M
    c = R.CFG
    args = dict(embed_dim=c["embed"], image_resolution=c["img"], vision_layers=c["depth"], vision_width=c["width"], vision_patch_size=c["patch"], context_length=c["ctx"],
                transformer_width=c["twidth"], transformer_heads=c["theads"], transformer_layers=c["tlayers"],
                attn_layer="MultiHeadAttention_LoRA", lora_rank=R.RANK, act_layer="QuickGELU", norm_layer="LayerNorm", dtype="f32")
    args.update(kw)
    if "vocab_size" not in args:
        args["vocab_size"] = _fix()["w/token_embedding.weight"].shape[0]
    return M.clip(args.pop("model_name", "ViT-B/16"), None, **args)


def test_state_dict_names_and_shapes_are_the_references():
    own = {k: tuple(v.shape) for k, v in _tiny_clip().state_dict().items()}
    want = {k[2:]: tuple(v.shape) for k, v in _fix().items() if k.startswith("w/")}
    assert own == want
    import libcontinual_amd.model as M
    assert M.clip is not None and "clip" in dir(M)


def test_text_tower_matches_the_fixture_and_the_restatement():
    fix = _fix()
    bb = _tiny_clip()
    bb.load_state_dict(R.fixture_weights(fix, torch.float32), strict=True)
    for t in range(R.TASKS):
        got = bb.text_features(torch.from_numpy(fix[f"t{t}/accm_tokens"]))
        assert R.rel(got.numpy(), fix[f"t{t}/accm_txt"]) < 1e-5


def test_entry_points_are_declared_defined_once_and_bound():
    from libcontinual_amd import _lib
    names = ["clhip_vit_set_clip", "clhip_clip_logits_fwd", "clhip_clip_logits_bwd"]
    with open(os.path.join(ROOT, "include", "clhip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    csrc = os.path.join(ROOT, "libcontinual_amd", "csrc")
    for n in names:
        assert len(re.findall(r"\bint " + n + r"\(", header)) == 1, n
        where = [f for f in sorted(os.listdir(csrc)) if f.endswith(".hip") and re.search(r'^extern "C" int ' + n + r"\(", open(os.path.join(csrc, f)).read(), re.M)]
        assert where == [{"clhip_vit_set_clip": "vit_plan.hip"}.get(n, "clip.hip")], (n, where)
        assert n in _lib._PROTOS and n in _lib.header_symbols()
    with open(os.path.join(csrc, "build.sh")) as f:
        assert " clip " in f.read()


def test_shipped_config_parses():
    from libcontinual_amd.config import Config
    cfg = Config(os.path.join(ROOT, "config", "inflora_opt-clip-vitb16-cifar100-b20x5.yaml")).get_config_dict()
    assert cfg["backbone"]["name"] == "clip" and cfg["backbone"]["kwargs"]["lora_rank"] == 10 and "experts_num" not in cfg["backbone"]["kwargs"]
    assert cfg["classifier"]["name"] == "InfLoRA_OPT" and cfg["classifier"]["kwargs"]["visual_only"] is True
    assert cfg["classifier"]["kwargs"]["prompt_template"] == R.TEMPLATE
    assert (cfg["init_cls_num"], cfg["inc_cls_num"], cfg["task_num"]) == (20, 20, 5)


# ------------------------------------------------------------------------------------------------ every refusal
@pytest.mark.parametrize("kw,exc,needle", [(dict(model_name="RN50"), NotImplementedError, "ModifiedResNet"), (dict(model_name="RN50x4"), NotImplementedError, "ModifiedResNet"),
                                           (dict(block_layer="ResidualAttentionBlock_MoE_MLP"), NotImplementedError, "block_layer"),
                                           (dict(experts_num=2), NotImplementedError, "experts_num 2"), (dict(act_layer="GELU"), NotImplementedError, "act_layer 'GELU'"),
                                           (dict(attn_layer="MultiHeadAttention_SDLoRA"), NotImplementedError, "attn_layer 'MultiHeadAttention_SDLoRA'"),
                                           (dict(attn_layer="MultiHeadAttention_LoRA", lora_rank=0), NotImplementedError, "lora_rank >= 1"),
                                           (dict(vision_layers=(3, 4, 6, 3)), NotImplementedError, "ModifiedResNet"),
                                           (dict(pretrained=True, checkpoint="/nonexistent/ViT-B-16.pt"), FileNotFoundError, "no local checkpoint at '/nonexistent/ViT-B-16.pt'.*CLHIP_CLIP_CHECKPOINT")])
def test_backbone_refusals(kw, exc, needle):
    with pytest.raises(exc, match=needle):                 # (no fixture is read on the way: the message is the refusal's own)
        _tiny_clip(vocab_size=40, **kw)


def test_backbone_accepts_the_absent_and_zero_experts_and_the_plain_attention():
    assert _tiny_clip(experts_num=0) is not None and _tiny_clip(block_layer="ResidualAttentionBlock") is not None
    plain = _tiny_clip(attn_layer="MultiHeadAttention", lora_rank=0)
    assert not any("lora" in k for k in plain.state_dict())


_OPENAI = (("attn.qkv.", "attn.in_proj_"), ("attn.proj.", "attn.out_proj."), ("mlp.fc1.", "mlp.c_fc."), ("mlp.fc2.", "mlp.c_proj."), (".blocks.", ".resblocks."))


def _openai_state(model):
    """the model's tensors under OpenAI's key names in fp16, without the LoRA factors, plus the three scalars their archives carry"""
    out = {}
    for k, v in model.state_dict().items():
        if ".lora_" in k:
            continue
        for own, theirs in _OPENAI:
            k = k.replace(own, theirs)
        out[k] = v.detach().half()
    out.update(input_resolution=torch.tensor(R.CFG["img"]), context_length=torch.tensor(R.CFG["ctx"]), vocab_size=torch.tensor(40))
    return out


def _as_module(state):
    """a module tree whose state_dict() has exactly these dotted names (what a TorchScript archive of the model holds)"""
    class Node(torch.nn.Module):
        def forward(self):
            return 0
    root = Node()
    for k, v in state.items():
        node, parts = root, k.split(".")
        for p in parts[:-1]:
            if p not in node._modules:
                node.add_module(p, Node())
            node = node._modules[p]
        node.register_buffer(parts[-1], v.clone())
    return root


@pytest.mark.parametrize("form", ["state_dict", "wrapped", "jit"])
def test_pretrained_loads_a_local_openai_checkpoint(form, tmp_path, monkeypatch):
    torch.manual_seed(7)
    src = _tiny_clip(vocab_size=40)
    with torch.no_grad():
        for n, p in src.named_parameters():
            if "ln_" in n or n.endswith(".bias"):                # (ones and zeros as initialised: make every tensor tell)
                p.add_(torch.randn_like(p) * 0.1)
    state = _openai_state(src)
    assert any(".resblocks.0.attn.in_proj_weight" in k for k in state) and any("mlp.c_fc.bias" in k for k in state)
    path = str(tmp_path / "ViT-tiny.pt")
    if form == "jit":
        torch.jit.script(_as_module(state)).save(path)
    else:
        torch.save({"state_dict": state} if form == "wrapped" else state, path)
    if form == "state_dict":                                    # the path from the environment; the geometry kwargs are the checkpoint's, not the caller's
        monkeypatch.setenv("CLHIP_CLIP_CHECKPOINT", path)
        got = _tiny_clip(pretrained=True, vision_width=128, vocab_size=7)
    else:
        monkeypatch.delenv("CLHIP_CLIP_CHECKPOINT", raising=False)
        got = _tiny_clip(pretrained=True, checkpoint=path, vocab_size=40)
    own, want = got.state_dict(), src.state_dict()
    assert sorted(own) == sorted(want) and not got.training
    for k, v in own.items():
        assert v.dtype == torch.float32 and v.shape == want[k].shape, k
        if ".lora_" not in k:
            assert torch.equal(v, want[k].half().float()), k      # the fp16 value, upcast


def test_pretrained_refuses_a_checkpoint_that_does_not_fill_the_model(tmp_path):
    src = _tiny_clip(vocab_size=40)
    path = str(tmp_path / "bad.pt")
    state = _openai_state(src)
    del state["visual.ln_pre.weight"]
    torch.save(state, path)
    with pytest.raises(ValueError, match=r"missing tensors \['visual.ln_pre.weight'\]"):
        _tiny_clip(pretrained=True, checkpoint=path)
    state = _openai_state(src)
    state["visual.proj"] = state["visual.proj"][:, :-1].contiguous()        # the model is sized by text_projection: this one no longer fits
    state["visual.attnpool.positional_embedding"] = torch.zeros(3)
    torch.save(state, path)
    with pytest.raises(ValueError, match=r"\['visual.attnpool.positional_embedding', 'visual.proj'\]"):
        _tiny_clip(pretrained=True, checkpoint=path)


def _plugin(bb=None, **kw):
    import libcontinual_amd.model as M
    args = dict(init_cls_num=R.INC, inc_cls_num=R.INC, task_num=R.TASKS, lame=R.LAME, lamb=R.LAMB, dataset="cifar100", use_ca=False, embd_dim=R.CFG["width"],
                prompt_template=R.TEMPLATE, visual_only=True, class_tokens=torch.zeros(R.INC * R.TASKS, 77, dtype=torch.int64))
    args.update(kw)
    return M.InfLoRA_OPT(bb if bb is not None else _tiny_clip(), "cpu", **args)


@pytest.mark.parametrize("kw,needle", [(dict(visual_only=False), "170-171"), (dict(use_ca=True), "88-105"), (dict(n_gpu=2), "n_gpu")])
def test_plugin_refusals(kw, needle):
    with pytest.raises(NotImplementedError, match=needle):
        _plugin(**kw)


def test_plugin_refuses_a_backbone_without_lora_rank_and_bad_tokens():
    with pytest.raises(NotImplementedError, match="lora_rank"):
        _plugin(_tiny_clip(attn_layer="MultiHeadAttention", lora_rank=0))
    with pytest.raises(ValueError, match="class_tokens"):
        _plugin(class_tokens=torch.zeros(2, 77, dtype=torch.int64))
    m = _plugin()
    with pytest.raises(NotImplementedError, match="assert 0"):
        m._network.get_feature(None)
    with pytest.raises(NotImplementedError, match="assert 0"):
        m._network.fc_only(None)
    assert len(m.attention_modules) == R.CFG["depth"] and not hasattr(m._network, "classifier_pool")


def test_update_fc_tokenizes_the_datasets_class_names_and_accumulates_them(tmp_path, monkeypatch):
    """the shipped config's default path (no class_tokens): get_class_names of a folder dataset -> prompt_template -> tokenize, for the running task's classes
    and for all classes so far (InfLoRA_opt.py:76-85), over two tasks; the tokenizer is a stand-in that needs no merges file"""
    from PIL import Image
    from libcontinual_amd.data import dataset as DS
    from libcontinual_amd.model import inflora_opt as I
    names = ["apple", "bus", "maple_tree", "zebra"]
    for n in names:
        os.makedirs(tmp_path / "train" / n)
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "train" / n / "0.png")
    cfg = dict(data_root=str(tmp_path), class_order=[2, 3, 1, 0], init_cls_num=2, inc_cls_num=2, task_num=2, num_workers=0)
    loaders = DS.preloaded_datasets(cfg, "train", lambda a: a, 2, None, None)
    calls = []

    def rows(texts, context_length):
        out = torch.zeros(len(texts), context_length, dtype=torch.int64)
        for i, t in enumerate(texts):
            row = [38] + [1 + ord(c) % 37 for c in t] + [39]             # 39, the end token, is the largest id: encode_text pools there
            out[i, :len(row)] = torch.tensor(row)
        return out

    def fake(texts, context_length, bpe_path):
        calls.append((list(texts), context_length, bpe_path))
        return rows(texts, context_length)
    monkeypatch.setattr(I, "tokenize", fake)
    m = _plugin(_tiny_clip(vocab_size=40), class_tokens=None, bpe_path="/some/merges", init_cls_num=2, inc_cls_num=2, task_num=2)
    sn, bb = m._network, m._network.backbone
    order = [["maple_tree", "zebra"], ["bus", "apple"]]
    seen = []
    for t in range(2):
        sn.update_fc(loaders.get_loader(t))
        seen += order[t]
        assert sn._cur_task_id == t and sn.curr_class_names == order[t] and sn.accm_class_names == seen
        assert calls[2 * t] == ([R.TEMPLATE.format(n) for n in order[t]], R.CFG["ctx"], "/some/merges")
        assert calls[2 * t + 1] == ([R.TEMPLATE.format(n) for n in seen], R.CFG["ctx"], "/some/merges")
        assert torch.equal(sn.curr_text_tokens, rows([R.TEMPLATE.format(n) for n in order[t]], 77)) and sn.accm_text_tokens.shape == (len(seen), 77)
        assert torch.equal(sn.curr_text_features, bb.text_features(sn.curr_text_tokens))
        assert torch.equal(sn.accm_text_features[-2:], sn.curr_text_features) and sn.accm_text_features.shape == (len(seen), R.CFG["embed"])
        assert torch.allclose(sn.accm_text_features.norm(dim=1), torch.ones(len(seen)), atol=1e-6)
        if t == 0:
            first = sn.accm_text_features.clone()
    assert torch.equal(sn.accm_text_features[:2], first) and len(calls) == 4
    assert sn._scale == pytest.approx(1 / 0.07)


def test_missing_merges_file_says_so(monkeypatch):
    from libcontinual_amd.model.backbone import clip_tokenizer as T
    monkeypatch.delenv("CLHIP_CLIP_BPE", raising=False)
    with pytest.raises(FileNotFoundError, match="not part of this repository"):
        T.tokenize(["a cat"])
    with pytest.raises(FileNotFoundError, match="user's to supply"):
        T.tokenize(["a cat"], bpe_path="/nonexistent/bpe.txt.gz")


# ------------------------------------------------------------------------------------------------ the tokenizer
def test_cleaning_and_the_ascii_refusal_need_no_merges_file():
    from libcontinual_amd.model.backbone import clip_tokenizer as T
    assert T.clean("  A  Bad\tPhoto of a\n Maple_Tree. ") == "a bad photo of a maple_tree."
    assert T.clean("salt &amp;amp; pepper") == "salt & pepper"
    for bad in ("café", "na\u00efve bear", "&eacute;clair"):
        with pytest.raises(ValueError, match="not ASCII"):
            T.clean(bad)
    tok = T.ClipTokenizer.__new__(T.ClipTokenizer)          # encode refuses before it touches a merge table
    with pytest.raises(ValueError, match="not ASCII"):
        tok.encode("café")


def _merges_file():
    p = os.environ.get("CLHIP_CLIP_BPE")
    if p and os.path.isfile(p):
        return p
    from oracle import ref_shim
    if ref_shim.available():
        p = os.path.join(ref_shim.REF_ROOT, "core", "model", "backbone", "tokenizer", "bpe_simple_vocab_16e6.txt.gz")
        return p if os.path.isfile(p) else None
    return None


def test_tokenizer_against_the_reference_tokens():
    path = _merges_file()
    if path is None:
        pytest.skip("no CLIP merges file reachable ($CLHIP_CLIP_BPE): bpe_simple_vocab_16e6.txt.gz is the user's to supply, it is not part of this repository")
    from libcontinual_amd.model.backbone.clip_tokenizer import ClipTokenizer
    fix = np.load(os.path.join(ROOT, "tests", "golden", "clip_tokens.npz"), allow_pickle=False)
    tok = ClipTokenizer(path)
    got = tok([str(t) for t in fix["texts"]]).numpy()
    assert got.shape == fix["tokens"].shape == (len(fix["texts"]), 77)
    np.testing.assert_array_equal(got, fix["tokens"].astype(np.int64))
    assert tok.vocab_size == 49408 and got[-1, -1] != tok.eot and (got[-1] != 0).all()            # the long row is truncated: its end token is cut off
    with pytest.raises(ValueError, match="not ASCII"):
        tok.encode("café")


# ------------------------------------------------------------------------------------------------ class names of the task datasets
def test_task_datasets_give_their_class_names_in_label_order(tmp_path):
    from PIL import Image
    from libcontinual_amd.data import dataset as DS
    names = ["zebra", "apple", "maple_tree", "bus"]
    for mode in ("train",):
        for n in names:
            os.makedirs(tmp_path / mode / n)
            Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / mode / n / "0.png")
    cls_map = {0: "maple_tree", 1: "zebra", 2: "bus", 3: "apple"}
    ds = DS.SingleDataset(str(tmp_path), "train", cls_map, lambda im: im, 1, 3)
    assert ds.get_class_names() == ["zebra", "bus"]
    cfg = dict(data_root=str(tmp_path), class_order=[2, 3, 1, 0], init_cls_num=2, inc_cls_num=2, task_num=2, num_workers=0)
    pre = DS.preloaded_datasets(cfg, "train", lambda a: a, 2, None, None)
    assert pre.get_loader(1).dataset.get_class_names() == [sorted(names)[1], sorted(names)[0]]
    import copy
    assert copy.deepcopy(pre.get_loader(0).dataset).get_class_names() == [sorted(names)[2], sorted(names)[3]]
    syn = DS.synthetic_datasets(dict(init_cls_num=2, inc_cls_num=2, task_num=2, image_size=8, seed=1, synthetic_per_class=2), "train", lambda a: a, 2)
    assert syn.get_loader(1).dataset.get_class_names() == ["class 2", "class 3"]
    with pytest.raises(ValueError):
        DS.ArrayDataset(np.zeros((1, 8, 8, 3), np.uint8), [0], [0], None).get_class_names()
