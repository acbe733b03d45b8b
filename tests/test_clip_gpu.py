"""InfLoRA_OPT on the `clip` backbone (model/inflora_opt.py, backbone/clip.py; the executor's CLIP mode and csrc/clip.hip) on a real MI355X against
tests/golden/clip_tiny.npz, the fp64 run of the reference's own CLIP + InfLoRA_OPT (tools/gen_clip_golden.py).  f32: the project's 5e-3 of max-abs for losses,
logits, every lora_B after each step, lora_A per task and the DualGPM bases (as projectors; lora_A / lora_B up to the sign of each singular vector), all
predictions equal.  bf16: the `[measure]` lines print the same deviations; clip_ref.BF16_MEASURED records them and the gates are 4 x those, or tighter (clip_ref.bf16_gate).
lora_B has a second measure, the deviation of a step's factors as one vector over their norm, because under Adam the element-wise one saturates in bf16."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_ref as R                                # noqa: E402
import libcontinual_amd.model as M                  # noqa: E402
from libcontinual_amd import optim                  # noqa: E402

DEV = "cuda"
CFG = R.CFG


def _backbone(fix, dtype):
    vocab = fix["w/token_embedding.weight"].shape[0]
    bb = M.clip("ViT-B/16", None, pretrained=False, embed_dim=CFG["embed"], image_resolution=CFG["img"], vision_layers=CFG["depth"], vision_width=CFG["width"],
                vision_patch_size=CFG["patch"], context_length=CFG["ctx"], vocab_size=vocab, transformer_width=CFG["twidth"], transformer_heads=CFG["theads"],
                transformer_layers=CFG["tlayers"], attn_layer="MultiHeadAttention_LoRA", lora_rank=R.RANK, act_layer="QuickGELU", norm_layer="LayerNorm", dtype=dtype)
    bb.load_state_dict(R.fixture_weights(fix, torch.float32), strict=True)
    return bb.to(DEV)


def _model(fix, dtype):
    tokens = torch.from_numpy(fix[f"t{R.TASKS - 1}/accm_tokens"])          # the accumulated set of the last task = all classes in label order
    return M.InfLoRA_OPT(_backbone(fix, dtype), DEV, init_cls_num=R.INC, inc_cls_num=R.INC, task_num=R.TASKS, lame=R.LAME, lamb=R.LAMB, dataset="cifar100",
                         use_ca=False, embd_dim=CFG["width"], prompt_template=R.TEMPLATE, visual_only=True, class_tokens=tokens)


def run_fixture(fix, dtype):
    model = _model(fix, dtype)
    x = (torch.from_numpy(fix["x_u8"]).float() / 255.0).to(DEV)
    y = torch.from_numpy(fix["y"]).to(DEV)
    xi = (torch.from_numpy(fix["xi_u8"]).float() / 255.0).to(DEV)
    out = {}
    for t in range(R.TASKS):
        loader = [{"image": x[t, s], "label": y[t, s]} for s in range(R.STEPS)]
        model.before_task(t, None, loader, None)
        sn = model._network
        assert torch.equal(sn.curr_text_tokens.cpu(), torch.from_numpy(fix[f"t{t}/curr_tokens"])) and torch.equal(sn.accm_text_tokens.cpu(), torch.from_numpy(fix[f"t{t}/accm_tokens"]))
        out[f"t{t}/curr_txt"], out[f"t{t}/accm_txt"] = sn.curr_text_features.cpu().numpy(), sn.accm_text_features.cpu().numpy()
        named = dict(model._network.named_parameters())
        train = sorted(n for n, p in named.items() if p.requires_grad)
        assert train == sorted(f"backbone.visual.transformer.blocks.{l}.attn.lora_B_{kv}.weight" for l in range(CFG["depth"]) for kv in "kv"), train
        assert not hasattr(model._network, "classifier_pool")
        out[f"t{t}/lora_A"] = np.stack([a.lora_A_k.weight.detach().cpu().numpy() for a in model.attention_modules])
        opt = optim.Adam([p for p in model.get_parameters(None) if p.requires_grad], lr=R.LR, betas=R.BETAS, weight_decay=0)
        model.train()
        for s in range(R.STEPS):
            with torch.no_grad():
                out[f"t{t}/s{s}/logits"] = model._network(x[t, s]).cpu().numpy()
            _, _, loss = model.observe({"image": x[t, s], "label": y[t, s]})
            opt.zero_grad()
            loss.backward()
            opt.step()
            out[f"t{t}/s{s}/loss"] = float(loss.detach())
            out[f"t{t}/s{s}/lora_B"] = np.stack([np.stack([a.lora_B_k.weight.detach().cpu().numpy(), a.lora_B_v.weight.detach().cpu().numpy()]) for a in model.attention_modules])
            if s == 1:                                     # the cached text features are what encode_text gives at any later step, bit for bit
                again = model._network.backbone.text_features(sn.curr_text_tokens)
                assert torch.equal(again, sn.curr_text_features)
        model.after_task(t, None, loader, [None])
        for l, f in enumerate(model.feature_list):
            out[f"t{t}/basis{l}"] = np.asarray(f, dtype=np.float64)
        out[f"t{t}/ptype"] = np.array(model.project_type)
        model.eval()
        with torch.no_grad():
            out[f"t{t}/infer_logits"] = model._network(xi, inference=True).cpu().numpy()
        pred, _ = model.inference({"image": xi, "label": torch.zeros(R.NI, dtype=torch.int64, device=DEV)})
        out[f"t{t}/infer_pred"] = pred.cpu().numpy()
    return out


def _step_preds_equal(got, fix):
    return all(np.array_equal(np.argmax(got[f"t{t}/s{s}/logits"], 1), np.argmax(fix[f"t{t}/s{s}/logits"], 1)) for t in range(R.TASKS) for s in range(R.STEPS))


def test_clip_inflora_golden_f32(golden):
    fix = golden("clip_tiny")
    d = R.deviations(run_fixture(fix, "f32"), fix)
    print("[measure] CLIP InfLoRA_OPT fixture f32: " + " ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in d.items()))
    for k in ("losses", "logits", "lora_B", "lora_B_rms", "lora_A", "bases", "txt"):
        assert d[k] < R.F32_TOL, (k, d)
    assert d["preds_equal"]


def test_clip_inflora_golden_bf16(golden):
    fix = golden("clip_tiny")
    got = run_fixture(fix, "bf16")
    d = R.deviations(got, fix)
    print("[measure] CLIP InfLoRA_OPT fixture bf16: " + " ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in d.items()))
    for k in ("losses", "logits", "lora_B", "lora_B_rms", "lora_A", "bases"):
        assert d[k] < R.bf16_gate(k), (k, d)
    assert d["txt"] < R.F32_TOL                            # the text tower is fp32 in both modes
    assert d["preds_equal"] and _step_preds_equal(got, fix)


NAMES = ["apple", "aquarium_fish", "maple_tree", "pickup_truck", "sweet_pepper", "zebra"]


def _stand_in_tokenize(texts, context_length=77, bpe_path=None):
    """a tokenizer that needs no merges file: start 38, one id in 1..37 per character, end 39 (the largest id, where encode_text pools)"""
    out = torch.zeros(len(texts), context_length, dtype=torch.int64)
    for i, t in enumerate(texts):
        row = [38] + [1 + ord(c) % 37 for c in t][:context_length - 2] + [39]
        out[i, :len(row)] = torch.tensor(row)
    return out


def _folder_tree(root):
    """the synthetic classes as a class-folder tree of PNGs (data_root/{train,test}/<class name>/<k>.png), the on-disk format of the datasets"""
    from PIL import Image
    from libcontinual_amd.data.dataset import synthetic_store
    for mode, per, split in (("train", 32, 0), ("test", 8, 1)):
        imgs, labels = synthetic_store(len(NAMES), per, 32, 5, split)
        for k, (im, l) in enumerate(zip(imgs, labels)):
            d = root / mode / NAMES[int(l)]
            d.mkdir(parents=True, exist_ok=True)
            Image.fromarray(im).save(d / f"{k}.png")


def _cfg(dtype, root):
    from libcontinual_amd.config import Config
    cfg = Config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "inflora_opt-clip-vitb16-cifar100-b20x5.yaml")).get_config_dict()
    bb = dict(cfg["backbone"]["kwargs"])
    bb.update(pretrained=False, embed_dim=32, image_resolution=32, vision_layers=2, vision_width=64, vision_patch_size=8, vocab_size=40, transformer_width=64,
              transformer_heads=1, transformer_layers=1, lora_rank=4, dtype=dtype)
    kw = dict(cfg["classifier"]["kwargs"])
    assert "class_tokens" not in kw and cfg["dataset"] == "cifar100"             # the shipped path: class names from the dataset, tokenized
    kw.update(init_cls_num=3, inc_cls_num=3, task_num=2, embd_dim=64)
    cfg.update(dict(data_root=str(root), class_order=[2, 5, 0, 4, 1, 3], image_size=32, init_cls_num=3, inc_cls_num=3, total_cls_num=6, task_num=2, epoch=2, init_epoch=2,
                    batch_size=32, val_per_epoch=10, testing_times=1, num_workers=0, save_path="", seed=5,
                    backbone={"name": "clip", "kwargs": bb}, classifier={"name": "InfLoRA_OPT", "kwargs": kw}))
    cfg.pop("train_trfms", None), cfg.pop("test_trfms", None)
    return cfg


def test_one_trainer_run_through_the_shipped_config(tmp_path, monkeypatch):
    """the shipped config's code path (backbone `clip`, InfLoRA_OPT, Adam, CosineSchedule; class names from a folder dataset -> prompt_template -> tokenize) at
    the tiny geometry on a synthetic class-folder tree; only the tokenizer is a stand-in, since the merges file is not part of the repository"""
    from libcontinual_amd.model import inflora_opt as I
    from libcontinual_amd.trainer import Trainer
    _folder_tree(tmp_path)
    asked = []
    monkeypatch.setattr(I, "tokenize", lambda texts, n=77, path=None: (asked.append(list(texts)), _stand_in_tokenize(texts, n, path))[1])
    os.environ.setdefault("PYTHONHASHSEED", "0")
    tr = Trainer(0, _cfg("bf16", tmp_path), log=lambda *a, **k: None)
    out = tr.train_loop()
    torch.cuda.synchronize()
    assert np.isfinite(out["acc_table"]).all()
    order = [NAMES[i] for i in (2, 5, 0, 4, 1, 3)]
    want = [[R.TEMPLATE.format(n) for n in ns] for ns in (order[:3], order[:3], order[3:], order)]
    assert asked == want and tr.model._network.accm_class_names == order
    assert tr.model._network.accm_text_features.shape == (6, 32) and tr.model._network.curr_text_features.shape == (3, 32)
    a = tr.model.attention_modules[0]
    assert len(tr.model.attention_modules) == 2 and not a.apply_lora                  # merged after the last task
    assert len(tr.model.feature_list) == 2
