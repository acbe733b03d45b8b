"""Write tests/golden/adapter_tiny.npz from the REFERENCE's own `Block` / `Adapter` classes (core/model/backbone/petl/vision_transformer_adapter.py),
imported through oracle.ref_shim with its stand-ins for timm; the tuning config is a SimpleNamespace (the reference uses an EasyDict).

    python tools/gen_adapter_golden.py          (needs the reference tree; the fixture is committed)

Two blocks, D 64, 2 heads, mlp 256, R 16, LayerNorm eps 1e-6, scale 0.1, in fp64 with `adaptmlp.dropout = 0.0` and a non-zero up-projection.  Stored: the
weights under this project's key names (q / k / v projections concatenated into `attn.qkv`), the input tokens [3, 17, 64], the cotangent of the last
block's output, both block outputs and the gradients of the eight adapter tensors.  tests/test_adapter_cpu.py holds tests/adapter_ref.py to it (1e-10).
"""
import os
import sys
from functools import partial
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

D, HEADS, R, DEPTH, B, N = 64, 2, 16, 2, 3, 17


def main():
    ref_shim.install_vit_standins()
    vta = ref_shim.load("core.model.backbone.petl.vision_transformer_adapter")
    cfg = SimpleNamespace(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                          ffn_adapter_scalar="0.1", ffn_num=R, d_model=D)
    torch.manual_seed(1234)
    blocks = [vta.Block(D, HEADS, mlp_ratio=4.0, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), config=cfg, layer_id=i) for i in range(DEPTH)]
    out = {}
    for i, blk in enumerate(blocks):
        blk.adaptmlp.dropout = 0.0
        with torch.no_grad():
            for t in (blk.adaptmlp.up_proj.weight, blk.adaptmlp.up_proj.bias, blk.adaptmlp.down_proj.bias, blk.norm1.bias, blk.norm2.bias):
                t.uniform_(-0.2, 0.2)
            for t in (blk.norm1.weight, blk.norm2.weight):
                t.uniform_(0.8, 1.2)
        blk.double().train()
        b = f"feat.transformer.blocks.{i}."
        a = blk.attn
        out[b + "attn.qkv.weight"] = torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight])
        out[b + "attn.qkv.bias"] = torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias])
        for ours, theirs in (("attn.proj", a.proj), ("ln_1", blk.norm1), ("ln_2", blk.norm2), ("mlp.fc1", blk.fc1), ("mlp.fc2", blk.fc2),
                             ("adaptmlp.down_proj", blk.adaptmlp.down_proj), ("adaptmlp.up_proj", blk.adaptmlp.up_proj)):
            out[b + ours + ".weight"], out[b + ours + ".bias"] = theirs.weight, theirs.bias
    x = torch.randn(B, N, D, dtype=torch.float64)
    gy = torch.randn(B, N, D, dtype=torch.float64)
    h = x
    for i, blk in enumerate(blocks):
        h = blk(h)
        out[f"block_out_{i}"] = h
    (h * gy).sum().backward()
    for i, blk in enumerate(blocks):
        for n in ("down_proj", "up_proj"):
            for k in ("weight", "bias"):
                out[f"grad.blocks.{i}.adaptmlp.{n}.{k}"] = getattr(getattr(blk.adaptmlp, n), k).grad
    out["x"], out["gy"] = x, gy
    path = os.path.join(ROOT, "tests", "golden", "adapter_tiny.npz")
    np.savez_compressed(path, **{k: v.detach().numpy() for k, v in out.items()})
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
