"""Time the classifier alignment of one InfLoRA_OPT `after_task` (model/class_align.py, csrc/ca.hip) at the last CIFAR-100 task, part by part, on
synthetic features: 5 000 rows of width 768 in 10 new classes, then 100 Gaussians and 5 epochs of 100 steps on 256 rows.

    python tools/inflora_ca_task.py [--n 5000 --d 768 --new 10 --classes 100 --reps 3]

Beside every part the torch-on-device restatement of the same reference lines is timed on the same box: `torch.cov` per class (InfLoRA_opt.py:396-397),
`MultivariateNormal(mean, cov).sample((256,))` per class and epoch (:418-431; it re-factors every covariance in every epoch, as the reference does),
`nn.Linear` heads + `torch.optim.SGD` steps (:439-454).  Every figure is the median of --reps event-timed repetitions after one untimed warm-up;
a part's inputs are made before its start event.  Prints one line per part and a JSON summary line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libcontinual_amd import ops  # noqa: E402
from libcontinual_amd.model import class_align as ca  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--new", type=int, default=10)
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    N, D, K, C, S = a.n, a.d, a.new, a.classes, ca.NUM_SAMPLE
    out = dict(N=N, D=D, new_classes=K, classes=C, samples=S, epochs=ca.EPOCHS, device=torch.cuda.get_device_name(0))
    labels = torch.arange(N, device=dev) % K
    feats = (torch.randn(K, D, device=dev)[labels] + 0.5 * torch.randn(N, D, device=dev)).contiguous()

    # ---- the Gaussians of the task's classes
    def sort_rows():
        order = torch.argsort(labels, stable=True)
        counts = torch.bincount(labels, minlength=K)
        offsets = torch.zeros(K + 1, dtype=torch.int32, device=dev)
        offsets[1:] = torch.cumsum(counts, 0)
        return feats[order], offsets
    out["sort_ms"] = timed(sort_rows, a.reps)
    fs, offsets = sort_rows()
    out["moments_hip_ms"] = timed(lambda: ops.class_moments(fs, offsets, ca.COV_EPS), a.reps)
    eye = torch.eye(D, device=dev)
    out["moments_torch_ms"] = timed(lambda: [(feats[labels == c].mean(0), torch.cov(feats[labels == c].double().T).float() + eye * 1e-4) for c in range(K)],
                                    a.reps)
    mean_new, cov_new = ops.class_moments(fs, offsets, ca.COV_EPS)
    out["cholesky_new_classes_ms"] = timed(lambda: torch.linalg.cholesky(cov_new), a.reps)

    # ---- the draws: all C Gaussians (the task's own, repeated, stand in for the stored ones)
    rep = (C + K - 1) // K
    means, covs = mean_new.repeat(rep, 1)[:C].contiguous(), cov_new.repeat(rep, 1, 1)[:C].contiguous()
    chols = torch.linalg.cholesky(covs)
    scale = torch.linspace(0.91, 1.0, C, device=dev)
    z = torch.randn(C * S, D, device=dev)
    dest = torch.randperm(C * S).to(dev)
    out["randn_epoch_ms"] = timed(lambda: torch.randn(C * S, D, device=dev), a.reps)
    out["sample_hip_epoch_ms"] = timed(lambda: ops.ca_sample(means, scale, chols, z, dest, 0), a.reps)

    def torch_draws():
        rows = [torch.distributions.multivariate_normal.MultivariateNormal(means[c] * scale[c], covs[c]).sample(sample_shape=(S,)) for c in range(C)]
        return torch.cat(rows)[dest]
    out["sample_torch_epoch_ms"] = timed(torch_draws, a.reps)

    # ---- the steps of one epoch
    X, y = ops.ca_sample(means, scale, chols, z, dest, 0)
    W, b = (torch.randn(C, D, device=dev) * 0.03).contiguous(), torch.zeros(C, device=dev)
    mw, mb = torch.zeros_like(W), torch.zeros_like(b)

    def hip_steps():
        ws = None
        for it in range(C):
            ws = ops.head_sgd_step(X[it * S:(it + 1) * S], y[it * S:(it + 1) * S], W, b, mw, mb, ca.LR, ca.MOMENTUM, ca.WEIGHT_DECAY, ws)
    out["steps_hip_epoch_ms"] = timed(hip_steps, a.reps)
    heads = nn.ModuleList([nn.Linear(D, K) for _ in range(C // K)]).to(dev)
    opt = torch.optim.SGD(heads.parameters(), lr=ca.LR, momentum=ca.MOMENTUM, weight_decay=ca.WEIGHT_DECAY)

    def torch_steps():
        for it in range(C):
            logits = torch.cat([h(X[it * S:(it + 1) * S]) for h in heads], dim=1)
            loss = F.cross_entropy(logits, y[it * S:(it + 1) * S])
            opt.zero_grad()
            loss.backward()
            opt.step()
    out["steps_torch_epoch_ms"] = timed(torch_steps, a.reps)

    E = ca.EPOCHS
    out["after_task_hip_ms"] = (out["sort_ms"] + out["moments_hip_ms"] + out["cholesky_new_classes_ms"]
                                + E * (out["randn_epoch_ms"] + out["sample_hip_epoch_ms"] + out["steps_hip_epoch_ms"]))
    out["after_task_torch_ms"] = out["moments_torch_ms"] + E * (out["sample_torch_epoch_ms"] + out["steps_torch_epoch_ms"])
    for k, v in out.items():
        print(f"{k:>26}: {v:.3f}" if isinstance(v, float) else f"{k:>26}: {v}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
