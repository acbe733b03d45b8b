"""Time RAPF's step on one GPU and print the table that profiles/rapf_step.md quotes.

Workload: ViT-B/16 `clip` backbone, bf16 tower, batch 100, a task >= 1 with 90 stored classes (synthetic Gaussians: a random SPD covariance per class, factored
once), beta 2, with 0 and with 8 hard pairs.  Rows, per step (device events around each repetition; median, min, max):

  * the whole step (observe + backward + Adam);
  * the frozen tower's forward (executor + visual.proj);
  * the adapter stage alone on this project's launches (clhip_rapf_draw + clhip_rapf_step_fwd + clhip_rapf_step_bwd), given the same features;
  * the same stage as a torch-on-device restatement of rapf.py:304-353, twice: as the reference writes it, with `torch.linalg.cholesky` of every sampled
    class's covariance in every step, and with the factors hoisted.

    python tools/rapf_step.py [--steps 30] [--warmup 10] [--out FILE] [--only-kernels]

--only-kernels runs the adapter stage alone a few times and nothing else: the form to put behind `rocprofv3 --kernel-trace --stats --` for the per-launch
times (a run of its own).  Random weights; no checkpoint is needed for a timing.  profiles/rapf_step.md is written by hand: the tool refuses to write over it.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libcontinual_amd.model as M  # noqa: E402
from libcontinual_amd import ops, optim  # noqa: E402

DEV = "cuda"
E, STORED, NEW, BETA = 512, 90, 10, 2


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def gaussians():
    mean = torch.randn(STORED, E, device=DEV)
    a = torch.randn(STORED, E, 2 * E, device=DEV) / (2 * E) ** 0.5
    cov = a @ a.transpose(1, 2) + 1e-4 * torch.eye(E, device=DEV)
    return mean, cov, torch.linalg.cholesky(cov).contiguous()      # (the solver may hand back a column-major batch)


def torch_stage(feats, y, W, txt, scale, mean, cov, chol, cls, pairs, hoisted):
    """rapf.py:304-353 on the device with autograd; `hoisted`: the factors are read, not recomputed"""
    def sample(c, n):
        L = chol[c] if hoisted else torch.linalg.cholesky(cov[c])
        return torch.randn(n, E, device=DEV) @ L.t() + mean[c]
    rows, labels = [feats] + [sample(c, 10 * BETA) for c in cls], [y] + [torch.full((10 * BETA,), c, device=DEV) for c in cls]
    x, lab = torch.cat(rows), torch.cat(labels)
    if len(pairs):
        edge = torch.cat([sample(p, 20 * BETA) for p, _ in pairs])
        pt = torch.cat([torch.full((20 * BETA,), p, device=DEV) for p, _ in pairs])
        nt = torch.cat([torch.full((20 * BETA,), n, device=DEV) for _, n in pairs])
        x = torch.cat([x, edge])
    f = torch.nn.functional.linear(x, W)
    f = f / f.norm(dim=1, keepdim=True)
    loss = torch.nn.functional.cross_entropy(scale * f[:len(lab)] @ txt.t(), lab)
    if len(pairs):
        e = f[len(lab):]
        e = e / e.norm(dim=-1, keepdim=True)
        tp, tn = txt[pt] / txt[pt].norm(dim=-1, keepdim=True), txt[nt] / txt[nt].norm(dim=-1, keepdim=True)
        loss = loss + torch.relu(-(e * tp).sum(-1) + (e * tn).sum(-1) + 0.1).mean()
    W.grad = None
    loss.backward()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-kernels", action="store_true")
    a = ap.parse_args()
    if a.out and os.path.realpath(a.out) == os.path.realpath(os.path.join(ROOT, "profiles", "rapf_step.md")):
        ap.error("--out would replace profiles/rapf_step.md and the analysis in it; name another file and paste the table")
    torch.manual_seed(0)
    B = a.batch
    mean, cov, chol = gaussians()
    txt = torch.nn.functional.normalize(torch.randn(STORED + NEW, E, device=DEV), dim=1)
    W = torch.nn.Parameter(torch.eye(E, device=DEV) + 0.02 * torch.randn(E, E, device=DEV))
    feats, y = torch.randn(B, E, device=DEV), torch.randint(STORED, STORED + NEW, (B,), device=DEV)
    rows = []
    for npairs in (0, 8):
        pairs = [(7 * i % STORED, STORED + i % NEW) for i in range(npairs)]
        cls = [3, 41]
        groups, counts = cls + [p for p, _ in pairs], [10 * BETA] * 2 + [20 * BETA] * npairs
        labels = torch.cat([y, torch.tensor(cls, device=DEV).repeat_interleave(10 * BETA)])
        pos = torch.tensor([p for p, _ in pairs], device=DEV).repeat_interleave(20 * BETA) if npairs else None
        neg = torch.tensor([n for _, n in pairs], device=DEV).repeat_interleave(20 * BETA) if npairs else None
        nd = sum(counts)

        def stage():
            X = torch.empty(B + nd, E, device=DEV)
            X[:B] = feats
            ops.rapf_draw(mean, chol, torch.randn(nd, E, device=DEV), X, B, groups, counts)
            st = ops.rapf_step_fwd(X, W.detach(), txt, 100.0, labels, pos, neg, B)
            return ops.rapf_step_bwd(st.G, X)
        if a.only_kernels:
            for _ in range(5):
                stage()
            torch.cuda.synchronize()
            continue
        rows.append((f"adapter stage, this project's launches (draw + step_fwd + step_bwd), {npairs} hard pairs, R = {B + nd}",) + timed(stage, a.steps * 4, a.warmup))
        for hoisted in (False, True):
            name = "hoisted factors" if hoisted else "torch.linalg.cholesky per sampled class per step (as rapf.py:41)"
            rows.append((f"adapter stage, torch restatement of rapf.py:304-353, {name}, {npairs} hard pairs",) +
                        timed(lambda: torch_stage(feats, y, W, txt, 100.0, mean, cov, chol, cls, pairs, hoisted), a.steps * 4 if hoisted else a.steps, a.warmup))
    if not a.only_kernels:
        tokens = torch.zeros(STORED + NEW, 77, dtype=torch.int64)
        tokens[:, 0], tokens[:, 1:6], tokens[:, 6] = 49406, torch.randint(1000, 40000, (STORED + NEW, 5)), 49407
        clip = M.clip("ViT-B/16", DEV, pretrained=False, act_layer="QuickGELU", norm_layer="LayerNorm", dtype="bf16")
        for npairs in (0, 8):
            m = M.RAPF(clip, DEV, init_cls_num=STORED, inc_cls_num=NEW, beta=BETA, shrinkage=False, threshold=0.0, train_batch_size=B, batch_size=128, num_workers=0,
                       prompt_template="a good photo of a {}", fp16=False, mix_bias=0.6, seed=0, class_tokens=tokens).to(DEV)
            m.before_task(0, None, [], None)
            m.class_means, m.class_covs, m.class_chols, m.prev_cls_num = mean, cov, chol, STORED
            m.before_task(1, None, [], None)
            hp = torch.tensor([(7 * i % STORED, STORED + i % NEW) for i in range(npairs)], dtype=torch.int64).reshape(-1, 2)
            m.hard_pairs = hp
            m._pos = hp[:, 0].repeat_interleave(20 * BETA).to(DEV) if npairs else None
            m._neg = hp[:, 1].repeat_interleave(20 * BETA).to(DEV) if npairs else None
            x = torch.rand(B, 3, 224, 224, device=DEV)
            opt = optim.Adam(list(m.get_parameters(None)), lr=1e-3, weight_decay=0)
            m.train()

            def step():
                _, _, loss = m.observe({"image": x, "label": y, "batch_id": 3})
                opt.zero_grad()
                loss.backward()
                opt.step()
            rows.append((f"RAPF step (observe + backward + Adam), ViT-B/16, batch {B}, bf16 tower, {npairs} hard pairs",) + timed(step, a.steps, a.warmup))
            if npairs == 0:
                rows.append((f"frozen tower forward + visual.proj, batch {B}, bf16",) + timed(lambda: m.image_features(x), a.steps, a.warmup))
    lines = ["| what | median ms | min | max |", "|---|---|---|---|"] + [f"| {n} | {med:.3f} | {lo:.3f} | {hi:.3f} |" for n, med, lo, hi in rows]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
