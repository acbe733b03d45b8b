"""ms per WA training step (task 0: forward, cross-entropy, backward, fused SGD) of ResNet-18 with the ImageNet stem (7x7 / s2 conv + max-pool,
the imagenet-r configs) on 224 x 224 images:  python tools/imagenet_step.py [batch ...] [--steps S] [--dtype bf16|f32]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import libcontinual_amd.model as M
from libcontinual_amd import optim, trainer, utils

ap = argparse.ArgumentParser()
ap.add_argument("batch", type=int, nargs="*", default=[10, 64])
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--dtype", default="bf16")
a = ap.parse_args()
dev = torch.device("cuda")
torch.manual_seed(0)
for B in a.batch:
    bb = M.resnet18(args={"dataset": "imagenet-r", "init_cls_num": 20, "inc_cls_num": 20}, dtype=a.dtype)
    m = M.WA(bb, 512, 200, device=dev, init_cls_num=20, inc_cls_num=20).to(dev)
    m.before_task(0, None, None, None)
    opt = optim.SGD(m.get_parameters({}), lr=0.1, momentum=0.9, weight_decay=2e-4)
    m.train()
    batches = [{"image": torch.randn(B, 3, a.size, a.size, device=dev), "label": torch.randint(0, 20, (B,), device=dev)} for _ in range(4)]
    utils.quiesce_gc()
    trainer.train_steps(m, opt, [batches[i % 4] for i in range(5)], device=dev)
    torch.cuda.synchronize()
    t0 = time.time()
    trainer.train_steps(m, opt, [batches[i % 4] for i in range(a.steps)], device=dev)
    torch.cuda.synchronize()
    dt = (time.time() - t0) / a.steps
    print(f"WA ResNet-18 (ImageNet stem) {a.dtype}, batch {B}, {a.size}x{a.size}: {dt * 1e3:.3f} ms/step, {B / dt:.0f} img/s", flush=True)
