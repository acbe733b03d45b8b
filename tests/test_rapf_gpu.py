"""RAPF (model/rapf.py on csrc/rapf.hip, csrc/ca.hip and the executor's CLIP mode) on a real MI355X against tests/golden/rapf_tiny.npz, the fp64 run of the
reference's own RAPF (tools/gen_rapf_golden.py).  The fixture's normals and class orders are injected through `normal_fn` / `class_order_fn`.
f32: every stored quantity within the project's 5e-3 of max-abs, all predictions and hard pairs equal.  bf16: the `[measure]` line prints the same deviations;
rapf_ref.BF16_MEASURED records them and the gates are 4 x those, or tighter (rapf_ref.bf16_gate).  The adapter stage is fp32 in both modes; the means and
covariances go through the tower and carry its bf16 deviation.  Below that, one short Trainer run on synthetic data."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rapf_ref as R                                # noqa: E402
import libcontinual_amd.model as M                  # noqa: E402
from libcontinual_amd import optim                  # noqa: E402

DEV = "cuda"
CFG = R.CFG


def _model(fix, dtype):
    vocab = fix["w/token_embedding.weight"].shape[0]
    bb = M.clip("ViT-B/16", None, pretrained=False, embed_dim=CFG["embed"], image_resolution=CFG["img"], vision_layers=CFG["depth"], vision_width=CFG["width"],
                vision_patch_size=CFG["patch"], context_length=CFG["ctx"], vocab_size=vocab, transformer_width=CFG["twidth"], transformer_heads=CFG["theads"],
                transformer_layers=CFG["tlayers"], act_layer="QuickGELU", norm_layer="LayerNorm", dtype=dtype)
    bb.load_state_dict(R.CR.fixture_weights(fix, torch.float32), strict=True)
    model = M.RAPF(bb.to(DEV), DEV, init_cls_num=R.INC, inc_cls_num=R.INC, beta=R.BETA, shrinkage=False, threshold=float(fix["threshold"]), train_batch_size=R.BATCH,
                   batch_size=R.BATCH, num_workers=0, prompt_template=R.TEMPLATE, fp16=False, mix_bias=R.MIX_BIAS, seed=int(fix["seed"]),
                   class_tokens=torch.from_numpy(fix["tokens"])).to(DEV)
    with torch.no_grad():
        model.adapter.weight.copy_(torch.from_numpy(fix["adapter0"]).float())
    return model


def run_fixture(fix, dtype):
    model = _model(fix, dtype)
    x, xs, xi = (R.images(fix[k], torch.float32).to(DEV) for k in ("x_u8", "xs_u8", "xi_u8"))
    y, ys = torch.from_numpy(fix["y"]).to(DEV), torch.from_numpy(fix["ys"]).to(DEV)
    model.class_order_fn = lambda t, classes: [int(c) for c in fix[f"t{t}/order"]]
    out = {}
    for t in range(R.TASKS):
        loader = [{"image": xs[t, b], "label": ys[t, b]} for b in range(xs.shape[1])]
        model.before_task(t, None, loader, None)
        out[f"t{t}/txt"] = model.class_name_features.cpu().numpy()
        if t > 0:
            out[f"t{t}/hard_pairs"] = model.hard_pairs.numpy()
        opt = optim.Adam(list(model.get_parameters(None)), lr=R.LR, weight_decay=0)
        model.train()
        for s in range(R.STEPS):
            if t > 0:
                model.normal_fn = lambda shape, z=fix[f"t{t}/s{s}/z"]: torch.from_numpy(z).reshape(shape)
            pred, acc, loss = model.observe({"image": x[t, s], "label": y[t, s], "batch_id": s})
            opt.zero_grad()
            loss.backward()
            opt.step()
            st = model.last_step
            assert torch.equal(pred, st.logits[:R.BATCH].argmax(1)) and float(acc) == float((pred == y[t, s]).sum()) / R.BATCH
            out[f"t{t}/s{s}/loss"], out[f"t{t}/s{s}/logits"] = float(loss.detach()), st.logits.cpu().numpy()
            out[f"t{t}/s{s}/adapter"] = model.adapter.weight.detach().cpu().numpy()
        model.after_task(t, None, loader, None)
        lo, hi = R.INC * t, R.INC * (t + 1)
        out[f"t{t}/means"], out[f"t{t}/covs"] = model.class_means[lo:hi].cpu().numpy(), model.class_covs[lo:hi].cpu().numpy()
        out[f"t{t}/adapter"] = model.adapter.weight.detach().cpu().numpy()
        model.eval()
        prob, acc = model.inference({"image": xi, "label": torch.arange(R.NI, device=DEV) % R.INC})
        assert abs(acc - float((prob.argmax(1).cpu() == torch.arange(R.NI) % R.INC).sum()) / R.NI) < 1e-12
        out[f"t{t}/infer_prob"] = prob.cpu().numpy()
    assert model.class_chols.shape == (R.INC * R.TASKS, CFG["embed"], CFG["embed"])      # one factor per stored class, made once
    return out


def _line(tag, d):
    print(f"[measure] RAPF fixture {tag}: " + " ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in d.items()))


def test_rapf_golden_f32(golden):
    fix = golden("rapf_tiny")
    d = R.deviations(run_fixture(fix, "f32"), fix)
    _line("f32", d)
    for k in R.FAMILIES + ("txt",):
        assert d[k] < R.F32_TOL, (k, d)
    assert d["preds_equal"] and d["pairs_equal"]


def test_rapf_golden_bf16(golden):
    fix = golden("rapf_tiny")
    d = R.deviations(run_fixture(fix, "bf16"), fix)
    _line("bf16", d)
    for k in R.FAMILIES:
        assert R.BF16_MEASURED[k] is not None and d[k] < R.bf16_gate(k), (k, d)
    assert d["txt"] < R.F32_TOL                            # the text tower is fp32 in both modes
    assert d["preds_equal"] and d["pairs_equal"]


def _cfg(root, inc):
    from libcontinual_amd.config import Config
    name = "rapf-clip-vitb16-cifar100-b50-5x10.yaml" if inc == 5 else "rapf-clip-vitb16-cifar100-b10x10.yaml"
    cfg = Config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", name)).get_config_dict()
    bb = dict(cfg["backbone"]["kwargs"])
    bb.update(pretrained=False, embed_dim=32, image_resolution=32, vision_layers=2, vision_width=64, vision_patch_size=8, vocab_size=40, transformer_width=64,
              transformer_heads=1, transformer_layers=1, dtype="bf16")
    n = 2 * inc
    tokens = torch.zeros(n, 77, dtype=torch.int64)
    for c in range(n):                                     # start 38, two class-dependent ids, end 39 (the largest id, where encode_text pools)
        tokens[c, :4] = torch.tensor([38, 1 + c, 1 + (7 * c) % 37, 39])
    kw = dict(cfg["classifier"]["kwargs"])
    kw.update(init_cls_num=inc, inc_cls_num=inc, class_tokens=tokens, threshold=2.5)       # every old x new pair is hard: unit rows are at most 2 apart
    cfg.update(dict(dataset="synthetic", data_root=str(root), image_size=32, init_cls_num=inc, inc_cls_num=inc, total_cls_num=n, task_num=2, epoch=1, init_epoch=1,
                    batch_size=32, train_batch_size=32, val_per_epoch=10, testing_times=1, num_workers=0, save_path="", seed=5,
                    backbone={"name": "clip", "kwargs": bb}, classifier={"name": "RAPF", "kwargs": kw}))
    return cfg


def test_one_trainer_run_on_synthetic_data(tmp_path, monkeypatch):
    """two tasks, one epoch: batch_id reaches observe, set_class_names is called with the loader's cls_map, the is_rapf transforms are the loaders', MultiStepLR is
    the scheduler, and CLHIP_CUDA_GRAPH=1 does not capture this method"""
    from libcontinual_amd.data import transforms as T
    from libcontinual_amd.trainer import Trainer
    monkeypatch.setenv("CLHIP_CUDA_GRAPH", "1")
    seen, names = [], []
    observe = M.RAPF.observe
    monkeypatch.setattr(M.RAPF, "observe", lambda self, data: (seen.append((self.task_id, data["batch_id"], torch.cuda.is_current_stream_capturing())), observe(self, data))[1])
    monkeypatch.setattr(M.RAPF, "set_class_names", lambda self, m: names.append(m))
    tr = Trainer(0, _cfg(tmp_path, 3), log=lambda *a, **k: None)
    trf = tr.train_loader.get_loader(0).dataset.trfms.transforms
    assert [type(t) for t in trf] == [T.Resize, T.CenterCrop, T.ToTensor, T.Normalize] and trf[0].interp == 3
    out = tr.train_loop()
    torch.cuda.synchronize()
    assert np.isfinite(out["acc_table"]).all()
    assert len(names) == 1 and isinstance(tr.scheduler, torch.optim.lr_scheduler.MultiStepLR)
    assert [b for t, b, _ in seen if t == 1] == list(range(len([1 for t, _, _ in seen if t == 1]))) and not any(c for _, _, c in seen)
    m = tr.model
    assert m.hard_pairs.shape == (9, 2) and m.class_means.shape == (6, 32) and m.old_adapter is not None
    assert m.last_step.G.shape[0] == m.last_step.pred.shape[0] + 2 * 20 + 9 * 40          # image rows | two replay groups | nine edge groups
    assert m.adapter.weight.grad is not None and bool(torch.isfinite(m.adapter.weight).all())
