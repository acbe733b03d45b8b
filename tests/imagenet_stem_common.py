"""Shared fixtures of the ImageNet-stem tests (a helper module, not a conftest): the reference args that select each stem, deterministic
weights / images from oracle.detrand tags, and an fp64 torch.nn.functional restatement of the reference ResNet-18/34 (core/model/backbone/
resnet.py:110-223) keyed by state-dict names."""
import math

import torch
import torch.nn.functional as F

from oracle import detrand

LAYERS = {"resnet18": [2, 2, 2, 2], "resnet34": [3, 4, 6, 3]}
# resnet.py:133-149: 'imagenet' in the dataset name -> max-pool stem, 7x7 / s2 when the first task has as many classes as the others
ARGS = {
    "imagenet7": {"dataset": "imagenet-r", "init_cls_num": 20, "inc_cls_num": 20},
    "imagenet3": {"dataset": "tiny-imagenet", "init_cls_num": 100, "inc_cls_num": 10},
}


def shapes(arch, stem):
    """(parameter name, shape) and buffer names of the reference state dict, in module order"""
    k = 7 if stem == "imagenet7" else 3
    P = [("conv1.0.weight", (64, 3, k, k)), ("conv1.1.weight", (64,)), ("conv1.1.bias", (64,))]
    cin = 64
    for li, (planes, n) in enumerate(zip((64, 128, 256, 512), LAYERS[arch])):
        for b in range(n):
            s = 2 if (li > 0 and b == 0) else 1
            pre = f"layer{li + 1}.{b}"
            P += [(f"{pre}.conv1.weight", (planes, cin, 3, 3)), (f"{pre}.bn1.weight", (planes,)), (f"{pre}.bn1.bias", (planes,)),
                  (f"{pre}.conv2.weight", (planes, planes, 3, 3)), (f"{pre}.bn2.weight", (planes,)), (f"{pre}.bn2.bias", (planes,))]
            if s != 1 or cin != planes:
                P += [(f"{pre}.downsample.0.weight", (planes, cin, 1, 1)), (f"{pre}.downsample.1.weight", (planes,)), (f"{pre}.downsample.1.bias", (planes,))]
            cin = planes
    return P


def det_state(arch, stem, tag):
    """(P, B): weights with the reference's init scale (kaiming fan_out for convs), BN affine near (1, 0); running stats (0, 1)"""
    P, B = {}, {}
    for n, shp in shapes(arch, stem):
        t = f"{tag}/{arch}/{stem}/{n}"
        if len(shp) == 4:
            a = math.sqrt(3.0) * math.sqrt(2.0 / (shp[2] * shp[3] * shp[0]))
            P[n] = torch.from_numpy(detrand.uniform(t, shp, -a, a))
        elif n.endswith(".weight"):
            P[n] = torch.from_numpy(detrand.uniform(t, shp, 0.8, 1.2))
        else:
            P[n] = torch.from_numpy(detrand.uniform(t, shp, -0.1, 0.1))
    for n, shp in shapes(arch, stem):
        if n.endswith(".weight") and len(shp) == 1:
            bn = n[: -len(".weight")]
            B[bn + ".running_mean"] = torch.zeros(shp)
            B[bn + ".running_var"] = torch.ones(shp)
            B[bn + ".num_batches_tracked"] = torch.zeros((), dtype=torch.long)
    return P, B


def det_images(tag, n, size):
    return torch.from_numpy(detrand.uniform(tag, (n, 3, size, size), -2.0, 2.0))


class _RoundBf16(torch.autograd.Function):
    """identity whose value AND gradient are rounded to bf16: a tensor the bf16 mode stores, in both directions"""
    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def forward(arch, stem, P, B, x, training=True, round_stem=False):
    """fp64 (or whatever P / x hold) ResNet forward of the reference: {'features', 'fmaps'}; updates B's running statistics when training.
    round_stem: the stem's stored tensors -- its conv output z and the pooled activation, and their gradients -- rounded to bf16 (the stem's
    storage sites in the bf16 mode)"""
    rs = _RoundBf16.apply if round_stem else (lambda t: t)

    def bn(h, name):
        return F.batch_norm(h, B[name + ".running_mean"], B[name + ".running_var"], P[name + ".weight"], P[name + ".bias"], training, 0.1, 1e-5)

    if stem == "imagenet7":
        h = F.conv2d(x, P["conv1.0.weight"], stride=2, padding=3)
    else:
        h = F.conv2d(x, P["conv1.0.weight"], stride=1, padding=1)
    h = rs(F.max_pool2d(F.relu(bn(rs(h), "conv1.1")), 3, 2, 1))
    fmaps = []
    cin = 64
    for li, (planes, n) in enumerate(zip((64, 128, 256, 512), LAYERS[arch])):
        for b in range(n):
            s = 2 if (li > 0 and b == 0) else 1
            pre = f"layer{li + 1}.{b}"
            o = F.relu(bn(F.conv2d(h, P[f"{pre}.conv1.weight"], stride=s, padding=1), f"{pre}.bn1"))
            o = bn(F.conv2d(o, P[f"{pre}.conv2.weight"], padding=1), f"{pre}.bn2")
            idn = h
            if s != 1 or cin != planes:
                idn = bn(F.conv2d(h, P[f"{pre}.downsample.0.weight"], stride=s), f"{pre}.downsample.1")
            h = F.relu(o + idn)
            cin = planes
        fmaps.append(h)
    return {"features": torch.flatten(F.adaptive_avg_pool2d(h, 1), 1), "fmaps": fmaps}
