"""Time one RanPAC first-session step (observe -> zero_grad -> backward -> SGD step) at the shipped shape: ViT-B/16 with AdaptFormer adapters
(R 64, scale 0.1, dropout 0.1), batch 48, bf16, random weights -- and the fused adapter forward beside the same math from existing kernels.

    python tools/ranpac_first_session.py [--batch 48 --reps 10 --dtype bf16 --steps-only]

Step: event-timed, median of --reps after two untimed warm-up steps.  Under `rocprofv3 --kernel-trace --stats -- python tools/ranpac_first_session.py
--steps-only` the kernel statistics give the adapter launches' share (kernel names adapter_fwd_kernel / adapter_bwd_kernel / adapter_wgrad_kernel /
adapter_wgrad_reduce_kernel).
Fused forward against its baseline at M = batch x 197, D 768, R 64: clhip_adapter_fwd (one launch, hidden tile on chip; 32- and 64-row workgroups)
beside two clhip_gemm_nt calls (bias + ReLU through torch, hidden matrix through HBM) plus the torch elementwise ops for the mask, the scale and the
residual add -- once with compute-dtype weights and the mask tensor ready-made, once making them inside the timed region as a training step must.
Prints one line per figure and a JSON summary line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libcontinual_amd import _lib, optim  # noqa: E402
from libcontinual_amd._lib import call  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
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
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--steps-only", action="store_true")
    a = ap.parse_args()
    import libcontinual_amd.model as M
    from libcontinual_amd.trainer import _backward
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    st = lambda: torch.cuda.current_stream().cuda_stream
    out = dict(batch=a.batch, dtype=a.dtype, device=torch.cuda.get_device_name(0))

    def model_for(ffn_adapt, fst):
        kw = dict(ffn_adapt=True, ffn_num=64, ffn_adapter_scalar=0.1, adapter_dropout=0.1) if ffn_adapt else {}
        bb = M.vit_pt_imnet_in21k_adapter(pretrained=False, dtype=a.dtype, **kw)
        m = M.RanPAC(bb, dev, first_session_training=fst, M=10000, init_cls_num=10, inc_cls_num=10, task_num=10, total_cls_num=100)
        m.before_task(0, None, None, None)
        return m

    model = model_for(True, True)
    with torch.no_grad():                                  # a trained adapter: non-zero up-projection
        for t in model.backbone.feat.adapter_tensors():
            if not t.any():
                t.uniform_(-0.05, 0.05)
    opt = optim.SGD(model.get_parameters({}), lr=0.01, momentum=0.9, weight_decay=5e-4)
    batch = {"image": torch.randn(a.batch, 3, 224, 224, device=dev), "label": torch.randint(0, 10, (a.batch,), device=dev)}
    model.train()

    def step():
        _, _, loss = model.observe(batch)
        opt.zero_grad()
        _backward(loss)
        opt.step()
    out["first_session_step_ms"] = timed(step, a.reps)
    with torch.no_grad():
        model.eval()
        out["adapter_eval_forward_ms"] = timed(lambda: model._network.get_feature(batch["image"]), a.reps)
        plain = model_for(False, False).eval()
        out["plain_eval_forward_ms"] = timed(lambda: plain._network.get_feature(batch["image"]), a.reps)
    if not a.steps_only:
        dt, tdt = (_lib.BF16, torch.bfloat16) if a.dtype == "bf16" else (_lib.F32, torch.float32)
        Mr, D, R, s, p = a.batch * 197, 768, 64, 0.1, 0.1
        x, y = torch.randn(Mr, D, device=dev).to(tdt), torch.randn(Mr, D, device=dev).to(tdt)
        Wd, bd, Wu, bu = (torch.randn(R, D, device=dev) * 0.03, torch.randn(R, device=dev) * 0.1, torch.randn(D, R, device=dev) * 0.1,
                          torch.randn(D, device=dev) * 0.1)
        seed = torch.tensor([12345], dtype=torch.int64, device=dev)
        hd = torch.empty(Mr, R, device=dev, dtype=tdt)
        fused = lambda: call("clhip_adapter_fwd", x.data_ptr(), Wd.data_ptr(), bd.data_ptr(), Wu.data_ptr(), bu.data_ptr(), y.data_ptr(), hd.data_ptr(),
                             seed.data_ptr(), 0, p, s, Mr, D, R, dt, st())
        for tm in (b"32", b"64"):                          # both workgroup heights of the fused kernel
            _lib.lib().clhip_config(b"ADAPTER_TM", tm)
            out[f"adapter_fwd_fused_tm{tm.decode()}_ms"] = timed(fused, a.reps)
        _lib.lib().clhip_config(b"ADAPTER_TM", None)
        out["adapter_fwd_fused_ms"] = timed(fused, a.reps)       # the default
        # the baseline: compute-dtype weight copies made once, outside the timing; mask bytes given
        Wd_c, Wu_c = Wd.to(tdt).contiguous(), Wu.to(tdt).contiguous()
        mask = torch.empty(Mr, R, dtype=torch.uint8, device=dev)
        call("clhip_adapter_dropout_mask", seed.data_ptr(), 0, Mr, R, p, mask.data_ptr(), st())
        keep = mask.to(tdt) / (1 - p)
        h, o = torch.empty(Mr, R, device=dev, dtype=tdt), torch.empty(Mr, D, device=dev, dtype=tdt)

        def baseline():
            call("clhip_gemm_nt", x.data_ptr(), Wd_c.data_ptr(), h.data_ptr(), bd.data_ptr(), None, None, Mr, R, D, D, D, R, 0, 0, 1, dt, st())
            hh = torch.relu_(h).mul_(keep)
            call("clhip_gemm_nt", hh.data_ptr(), Wu_c.data_ptr(), o.data_ptr(), bu.data_ptr(), None, None, Mr, D, R, R, R, D, 0, 0, 1, dt, st())
            y.add_(o, alpha=s)
        out["adapter_fwd_baseline_ms"] = timed(baseline, a.reps)

        def baseline_per_step():                             # what a training step pays: the weights moved, the mask is new
            nonlocal Wd_c, Wu_c, keep
            Wd_c, Wu_c = Wd.to(tdt), Wu.to(tdt)
            call("clhip_adapter_dropout_mask", seed.data_ptr(), 0, Mr, R, p, mask.data_ptr(), st())
            keep = mask.to(tdt).mul_(1 / (1 - p))
            baseline()
        out["adapter_fwd_baseline_per_step_ms"] = timed(baseline_per_step, a.reps)
        byts = (3 * Mr * D + Mr * R) * (2 if a.dtype == "bf16" else 4)                 # x read, y read + written, hd written
        out["adapter_fwd_fused_GBps"] = byts / out["adapter_fwd_fused_ms"] / 1e6
    for k, v in out.items():
        print(f"{k:>28}: {v:.3f}" if isinstance(v, float) else f"{k:>28}: {v}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
