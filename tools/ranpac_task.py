"""Time one RanPAC `after_task` (model/ranpac.py, csrc/rp.hip) at the workload's shape on synthetic features, phase by phase.

    python tools/ranpac_task.py [--n 5000 --d 768 --m 10000 --c 100 --batch 48 --reps 3 --vit]

Phases: projection (relu(F W), fitting and hold-out rows), the two Grams (G_val over int(0.8 N) rows, G_rest over the remainder) with
torch.matmul(H.T, H) in fp32 beside them, the two label sums, the 18 solves (17 ridge candidates + the final one, torch.linalg.solve on the device),
the classify call at the inference batch, and with --vit the frozen ViT-B/16 eval forward over N images (bf16, random weights) on its own.
Every figure is the median of --reps event-timed repetitions after one untimed warm-up; events bracket device work only, and a phase's inputs are
made before its start event.  Prints one line per phase and a JSON summary line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libcontinual_amd import ops  # noqa: E402
from libcontinual_amd.model.ranpac import RIDGES, RPClassifier  # noqa: E402


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
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--c", type=int, default=100)
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--vit", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    N, D, M, C = a.n, a.d, a.m, a.c
    feats = torch.randn(N, D).to(dev)
    labels = torch.randint(0, C, (N,)).to(dev)
    rp = RPClassifier(D, M, dev)
    nv = int(N * 0.8)
    out = dict(N=N, D=D, M=M, C=C, batch=a.batch, device=torch.cuda.get_device_name(0))

    out["project_ms"] = timed(lambda: (ops.rp_project(feats[:nv], rp.W_rand), ops.rp_project(feats[nv:], rp.W_rand)), a.reps)
    Hv, Hr = ops.rp_project(feats[:nv], rp.W_rand), ops.rp_project(feats[nv:], rp.W_rand)
    Gv, Gr = torch.zeros(M, M, device=dev), torch.zeros(M, M, device=dev)
    out["gram_val_ms"] = timed(lambda: ops.rp_gram_accum(Hv, Gv), a.reps)
    out["gram_rest_ms"] = timed(lambda: ops.rp_gram_accum(Hr, Gr), a.reps)
    out["torch_matmul_val_ms"] = timed(lambda: torch.matmul(Hv.T, Hv), a.reps)
    out["torch_matmul_rest_ms"] = timed(lambda: torch.matmul(Hr.T, Hr), a.reps)
    out["gram_val_tflops"] = M * (M + 128) * nv / out["gram_val_ms"] / 1e9           # the multiply-adds it really does (upper tiles), as 2 flop each
    Qv, Qr = torch.zeros(M, C, device=dev), torch.zeros(M, C, device=dev)
    out["label_sum_ms"] = timed(lambda: (ops.rp_label_sum(Hv, labels[:nv], Qv), ops.rp_label_sum(Hr, labels[nv:], Qr)), a.reps)
    # fresh sums for the solves (the timed repetitions above accumulated several times)
    Gv.zero_(), Qv.zero_()
    ops.rp_gram_accum(Hv, Gv)
    ops.rp_label_sum(Hv, labels[:nv], Qv)

    def solves():
        for ridge in list(RIDGES) + [RIDGES[8]]:
            A = Gv.clone()
            A.diagonal().add_(float(ridge))
            torch.linalg.solve(A, Qv)
    out["solves_18_ms"] = timed(solves, max(1, a.reps - 1))
    Wo = torch.randn(C, M, device=dev) * 0.01
    x = feats[:a.batch].contiguous()
    out["classify_ms"] = timed(lambda: ops.rp_classify(x, rp.W_rand, Wo), a.reps)
    out["holdout_predict_ms"] = timed(lambda: ops.rp_classify(feats[nv:].contiguous(), rp.W_rand, Wo), a.reps)
    total = out["project_ms"] + out["gram_val_ms"] + out["gram_rest_ms"] + out["label_sum_ms"] + out["solves_18_ms"] + 17 * out["holdout_predict_ms"]
    out["after_task_total_ms"] = total
    out["solves_share"] = out["solves_18_ms"] / total
    if a.vit:
        import libcontinual_amd.model as Mo
        bb = Mo.vit_pt_imnet_in21k_adapter(pretrained=False, dtype="bf16").to(dev).eval()
        img = torch.randn(a.batch, 3, 224, 224, device=dev)
        with torch.no_grad():
            ms = timed(lambda: bb(img), a.reps)
        out["vit_forward_batch_ms"] = ms
        out["vit_forward_task_ms"] = ms * ((N + a.batch - 1) // a.batch)
    for k, v in out.items():
        print(f"{k:>24}: {v:.3f}" if isinstance(v, float) else f"{k:>24}: {v}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
