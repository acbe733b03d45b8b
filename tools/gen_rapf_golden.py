"""Write tests/golden/rapf_tiny.npz from an fp64 run of the REFERENCE's own `RAPF` (core/model/rapf.py) on its own `CLIP` (default block), imported through
oracle.ref_shim with its stand-ins for timm and ftfy.

    PYTHONHASHSEED=0 python tools/gen_rapf_golden.py          (needs the reference tree; the fixture is committed)

Geometry: tests/clip_ref.CFG (image 32, patch 8, visual width 64 / 3 blocks, text width 64 / 2 blocks, embed E = 32).  Three tasks of three classes, three
steps of nine images each under torch.optim.Adam(lr 1e-3) on the adapter alone (a new optimizer per task, as the trainer builds one), beta 2, shrinkage off,
mix_bias 0.6, 64 = 2 E rows per class in the after_task loader.  The reference config's block (ResidualAttentionBlock_MoE_MLP) cannot construct in the
reference (its arguments reach ResidualAttentionBlock by position); its intended arithmetic with one zero-initialised, never-trained expert is the default
block's, which is what runs here.

Supplied by this tool, not by oracle/: empty stand-ins for `core.data` / `core.data.dataloader` (rapf.py imports the names only); nn.LayerNorm's forward in place
of the reference subclass's fp32 cast; `model.model.dtype = torch.float64` and an adapter of width E (the reference hard-codes fp32 and 512); a proxy for the
`torch` and `random` names of the rapf module that records every `torch.randn` and `random.shuffle` it makes, so that the fixture stores the normals and the class
orders a GPU run injects; a wrapper of the inner model's forward that keeps the logits.

Stored: the weights (bf16-representable, as 16-bit words) and the initial adapter, the nine classes' tokens (remapped to their rank among the used ids), images
as 8 x 8 bytes (rapf_ref.images shows them four times as large), labels; per step the loss, the logits of all CE rows, the adapter after Adam and the normals;
per task the normalised text features (fp64, and the fp32 copy the reference keeps for the hard pairs and the hinge), the shuffled old-class list, the hard pairs, the new classes' means and covariances, the adapter after mix_matrix, and
the inference probabilities of a held-out batch of 12.  `threshold` is placed between the text-feature distances so that one of the two later tasks has hard
pairs (at most three) and the other has none.

The file is written only when (a) a task >= 1 has edge rows and one has none, and not every old x new pair is hard; (b) the top two logits of every stored image
row differ by more than the bf16 gate lets them move; (c) every stored edge row's pre-relu value is farther from 0 than that gate; (d) an fp32 CPU run of
tests/rapf_ref.py meets the f32 tolerance; and tests/rapf_ref.py in fp64 reproduces it to 1e-10.  The seed counts up from 3 until they hold and is stored.
"""
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim  # noqa: E402
import rapf_ref as R  # noqa: E402

CFG = R.CFG
NAMES = "apple aquarium_fish baby bear beaver bed bee beetle bicycle".split()


class _Recorder:
    """stands where the rapf module keeps a module name: every attribute is the real module's, except the recorded call"""

    def __init__(self, real, name, log):
        self.__dict__.update(_real=real, _name=name, _log=log)

    def __getattr__(self, k):
        v = getattr(self._real, k)
        if k != self._name:
            return v

        def recorded(*a, **kw):
            out = v(*a, **kw)
            self._log.append(out.clone() if torch.is_tensor(out) else list(a[0]))      # randn returns the draw; shuffle works in place on its argument
            return out
        return recorded


def pictures(g, base, labels):
    """one 8 x 8 picture per label: a pattern common to all classes (bytes 60 .. 195) plus the class's own of +- 30, under pixel noise of +- 15.  The class
    Gaussians are distinct, and the rows of a step rank the classes alike unless the text side is close -- a random tiny tower has no other reason to prefer a
    class, and with independent pictures no seed separates the top two logits of every stored row (condition (b))"""
    noise = (torch.rand(*labels.shape, 3, 8, 8, generator=g) * 2 - 1) * 15
    return (base[labels] + noise).round().clamp(0, 255).to(torch.uint8)


def pick_threshold(txt):
    """between the old x new text distances, so that one later task has 1-3 hard pairs and the other none; None if the gap around it is narrow"""
    d = [torch.cdist(txt[:R.INC * t], txt[R.INC * t:R.INC * (t + 1)]).flatten().sort().values for t in range(1, R.TASKS)]
    lo, hi = (d[0], d[1]) if d[0][0] < d[1][0] else (d[1], d[0])
    below = lo[lo < hi[0]]
    k = min(len(below), 3)
    upper = below[k] if k < len(below) else hi[0]
    if float(upper - below[k - 1]) < 1e-2:
        return None
    return float((below[k - 1] + upper) / 2)


def run(clip, rapf, tokens, vocab, seed):
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    net = clip.CLIP(CFG["embed"], CFG["img"], CFG["depth"], CFG["width"], CFG["patch"], CFG["ctx"], vocab, CFG["twidth"], CFG["theads"], CFG["tlayers"],
                    act_layer="QuickGELU", norm_layer="LayerNorm")
    with torch.no_grad():                                  # a trained-network-like scale (tools/gen_clip_golden.py)
        for n, p in net.named_parameters():
            if n == "logit_scale":
                continue
            if n.endswith("bias"):
                p.uniform_(-0.05, 0.05)
            elif ".ln_" in n or "ln_p" in n or "ln_final" in n:
                p.uniform_(0.8, 1.2)
            elif p.dim() >= 2 and "embedding" not in n and n not in ("visual.proj", "text_projection"):
                s = 1.7 / np.sqrt(p[0].numel())
                p.uniform_(-s, s)
        for v in net.state_dict().values():                # bf16-representable: the fixture stores 16 bits per weight
            v.copy_(v.bfloat16().to(v.dtype))
        t = net.encode_text(tokens)
        thr = pick_threshold(t / t.norm(dim=-1, keepdim=True))
    if thr is None:
        return None
    out = {"seed": np.array(seed), "threshold": np.array(thr), "tokens": tokens.clone()}
    for k, v in net.state_dict().items():
        out["w/" + k] = v.bfloat16().view(torch.int16)
    E = CFG["embed"]
    rapf.tokenize = lambda texts: torch.stack([tokens[NAMES.index(t[len(R.TEMPLATE) - 2:])] for t in texts])
    normals, orders = [], []
    rapf.torch, rapf.random = _Recorder(torch, "randn", normals), _Recorder(random, "shuffle", orders)
    model = rapf.RAPF(net, seed=seed, device="cpu", init_cls_num=R.INC, inc_cls_num=R.INC, beta=R.BETA, shrinkage=False, threshold=thr, train_batch_size=R.BATCH,
                      batch_size=R.BATCH, num_workers=0, prompt_template=R.TEMPLATE, fp16=False, mix_bias=R.MIX_BIAS)
    inner = model.model
    inner.dtype = torch.float64
    inner.adapter = torch.nn.Linear(E, E, bias=False)
    with torch.no_grad():
        inner.adapter.weight.copy_(inner.adapter.weight.bfloat16().to(torch.float64))
    out["adapter0"] = inner.adapter.weight.detach().clone()
    inner.classes_names = list(NAMES)
    kept = []
    forward = inner.forward
    inner.forward = lambda *a, **kw: (lambda r: (kept.append(r[0].detach().clone()), r)[1])(forward(*a, **kw))
    nb = R.INC * R.NSTAT // R.STAT_BATCH
    y = torch.stack([(torch.arange(R.BATCH) % R.INC + R.INC * t).expand(R.STEPS, R.BATCH) for t in range(R.TASKS)]).contiguous()
    ys = torch.stack([(torch.arange(nb * R.STAT_BATCH) % R.INC + R.INC * t).view(nb, R.STAT_BATCH) for t in range(R.TASKS)]).contiguous()
    base = 60 + 135 * torch.rand(3, 8, 8, generator=g) + 30 * (2 * torch.rand(len(NAMES), 3, 8, 8, generator=g) - 1)
    x8, xs8, xi8 = pictures(g, base, y), pictures(g, base, ys), pictures(g, base, torch.arange(R.NI) % R.INC)      # (the held-out batch: classes of task 0)
    out.update(x_u8=x8, xi_u8=xi8, xs_u8=xs8, y=y, ys=ys)
    x, xi, xs = R.images(x8.numpy()), R.images(xi8.numpy()), R.images(xs8.numpy())
    for t in range(R.TASKS):
        loader = [{"image": xs[t, b], "label": ys[t, b]} for b in range(nb)]
        del orders[:]
        model.before_task(t, None, loader, [loader])
        with torch.no_grad():                              # (inner.class_name_features is this through an fp32 cast, rapf.py:124)
            f = inner.encode_text(inner.text_tokens)
            out[f"t{t}/txt"] = f / f.norm(dim=-1, keepdim=True)
        out[f"t{t}/txt32"] = inner.class_name_features.detach().clone()      # the fp32 copy the hard pairs and the hinge read
        if t > 0:
            assert len(orders) == 1
            out[f"t{t}/order"] = np.array(orders[0])
            out[f"t{t}/hard_pairs"] = inner.hard_pairs.clone()
        opt = torch.optim.Adam(model.get_parameters(None), lr=R.LR, weight_decay=0.0)
        model.train()
        for s in range(R.STEPS):
            del normals[:], kept[:]
            _, _, loss = model.observe({"image": x[t, s], "label": y[t, s], "batch_id": s})
            opt.zero_grad()
            loss.backward()
            opt.step()
            out[f"t{t}/s{s}/loss"], out[f"t{t}/s{s}/logits"] = loss.detach().clone(), kept[0]
            out[f"t{t}/s{s}/adapter"] = inner.adapter.weight.detach().clone()
            if t > 0:
                out[f"t{t}/s{s}/z"] = torch.cat(normals)
        model.after_task(t, None, loader, [loader])
        lo, hi = R.INC * t, R.INC * (t + 1)
        out[f"t{t}/means"], out[f"t{t}/covs"] = torch.stack(inner.class_mean_list[lo:hi]), torch.stack(inner.class_cov_list[lo:hi])
        out[f"t{t}/adapter"] = inner.adapter.weight.detach().clone()
        model.eval()
        out[f"t{t}/infer_prob"] = model.inference({"image": xi, "label": torch.zeros(R.NI, dtype=torch.int64)})[0].clone()
    return {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def main():
    os.environ.setdefault("PYTHONHASHSEED", "0")
    os.environ.setdefault("TQDM_DISABLE", "1")             # (rapf.py's after_task wraps its loader in tqdm)
    torch.set_default_dtype(torch.float64)
    ref_shim.install_vit_standins()
    for name in ("core.data", "core.data.dataloader"):     # rapf.py imports the names and never uses them
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["core.data"].dataloader = sys.modules["core.data.dataloader"]
    tr = ref_shim.load("core.model.backbone.transformer")
    tr.LayerNorm.forward = torch.nn.LayerNorm.forward      # the reference subclass casts to fp32 (transformer.py:129-135): an fp64 run keeps its dtype
    clip = ref_shim.load("core.model.backbone.clip")
    rapf = ref_shim.load("core.model.rapf")
    raw = clip.tokenize([R.TEMPLATE.format(c) for c in NAMES])
    used = torch.unique(raw)                               # sorted; 0 (the padding) is among them, and argmax still finds the end token
    tokens = torch.searchsorted(used, raw)
    for seed in range(3, 403):
        fix = run(clip, rapf, tokens, len(used), seed)
        if fix is None:
            print(f"seed {seed}: no threshold with a clear gap", flush=True)
            continue
        why = R.condition_a(fix) or R.condition_b(fix, 1.25)
        if not why:
            got = R.run_fixture(fix)
            d = R.deviations(got, fix)
            if not (max(d[k] for k in R.FAMILIES + ("txt",)) < 1e-10 and d["preds_equal"] and d["pairs_equal"]):
                why = f"restatement: {d}"
            why = why or R.condition_c(fix, got, 1.25)
            why = why or (lambda w: w and "(d) " + w)(R.check_f32(R.run_fixture(fix, torch.float32), fix))
        if not why:
            break
        print(f"seed {seed}: {why}", flush=True)
    else:
        raise SystemExit("no seed met the conditions")
    path = os.path.join(ROOT, "tests", "golden", "rapf_tiny.npz")
    np.savez_compressed(path, **fix)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(fix)} arrays, seed {seed}, threshold {float(fix['threshold']):.4f}, "
          f"hard pairs {[fix[f't{t}/hard_pairs'].tolist() for t in range(1, R.TASKS)]}")


if __name__ == "__main__":
    main()
