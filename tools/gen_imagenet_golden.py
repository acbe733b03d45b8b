"""Writes tests/golden/backbone_resnet18_imagenet{7,3}.npz from the REFERENCE's own resnet18 (core/model/backbone/resnet.py, imported in place
through oracle.ref_shim; fp64, CPU) on the deterministic weights / images of tests/imagenet_stem_common.py: one train-mode batch (features, every
parameter gradient and the running statistics as oracle.fixtures.summarize rows, the stem's gradient in full), then eval features.  Needs the
reference tree: run where it is present, never on the GPU machine.   python tools/gen_imagenet_golden.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import imagenet_stem_common as C
from oracle import detrand, fixtures as fx, ref_shim

CASES = {"imagenet7": ("imagenet-r", 224), "imagenet3": ("tiny-imagenet", 64)}
B = 4


def scenario(stem):
    resnet = ref_shim.load("core.model.backbone.resnet")
    net = resnet.resnet18(args=C.ARGS[stem]).double()
    P, Bf = C.det_state("resnet18", stem, "golden")
    sd = net.state_dict()
    for k, v in {**P, **Bf}.items():
        assert k in sd and tuple(sd[k].shape) == tuple(v.shape), k
        sd[k] = v.double() if v.is_floating_point() else v
    net.load_state_dict(sd)
    x = C.det_images(f"golden/{stem}/x", B, CASES[stem][1]).double()
    cw = torch.from_numpy(detrand.uniform(f"golden/{stem}/cw", (B, 512), -1.0, 1.0)).double()
    net.train()
    out = net(x)
    assert [t.shape[2] for t in out["fmaps"]] == ([56, 28, 14, 7] if stem == "imagenet7" else [32, 16, 8, 4])
    (out["features"] * cw).sum().backward()
    grads = {n: p.grad.detach() for n, _ in C.shapes("resnet18", stem) for p in [dict(net.named_parameters())[n]]}
    bufs = {k: v.detach() for k, v in net.state_dict().items() if "running" in k}
    net.eval()
    with torch.no_grad():
        fe = net(x)["features"]
    names, rows = fx.summarize(grads)
    bnames, brows = fx.summarize(bufs)
    return dict(features_train=out["features"].detach().numpy(), features_eval=fe.numpy(), grad_names=np.asarray(names), grad_rows=rows,
                grad_stem=grads["conv1.0.weight"].numpy().astype(np.float32), buf_names=np.asarray(bnames), buf_rows=brows)


if __name__ == "__main__":
    for stem in CASES:
        path = os.path.join(ROOT, "tests", "golden", f"backbone_resnet18_{stem}.npz")
        np.savez_compressed(path, **scenario(stem))
        print(path, os.path.getsize(path), "bytes")
