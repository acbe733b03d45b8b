"""CLIP backbone (reference core/model/backbone/clip.py:267-416, its visual tower core/model/backbone/transformer.py:2086-2138) with the visual tower on
the HIP ViT executor in CLIP mode (clhip_vit_set_clip: bias-free patch convolution, ln_pre, QuickGELU, ln_post at eps 1e-5) and the image-side logits on
csrc/clip.hip.

Parameter names and shapes are those of the reference's `CLIP` after its own key mapping (clip.py:455-461), so state dicts interchange:

    visual.conv1.weight  visual.class_embedding  visual.positional_embedding  visual.ln_pre.*  visual.transformer.blocks.N.{ln_1, attn.{qkv, proj[, lora_*]},
    ln_2, mlp.{fc1, fc2}}  visual.ln_post.*  visual.proj  transformer.blocks.N.*  token_embedding.weight  positional_embedding  ln_final.*
    text_projection  logit_scale

`VisualTransformer` IS the `VisionTransformer` of backbone/vit.py with another stem and head: the executor handle, the weight copies, the autograd
functions, the Gram buffers and `debug_read` are inherited, not copied.  The text tower is plain torch in fp32 under no_grad and eval (causal mask, pooled
at the end token, clip.py:385-398): it is frozen in every method that runs here (`visual_only: true`), so it is plumbing, evaluated once per task.
Training it needs a causal attention forward / backward in the executor and is not built.
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ..._lib import call
from .vit import _P, MultiHeadAttention, MultiHeadAttention_LoRA, Transformer, VisionTransformer

_CLIP_ATTN = {"MultiHeadAttention": MultiHeadAttention, "MultiHeadAttention_LoRA": MultiHeadAttention_LoRA}
# embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size, context_length, vocab_size, transformer_width, transformer_heads, transformer_layers
_GEOMETRY = {"ViT-B/16": (512, 224, 12, 768, 16, 77, 49408, 512, 8, 12), "ViT-B/32": (512, 224, 12, 768, 32, 77, 49408, 512, 8, 12)}
_RESNET_NAMES = ("RN50", "RN101", "RN50x4", "RN50x16", "RN50x64")
_GEOMETRY_KEYS = ("embed_dim", "image_resolution", "vision_layers", "vision_width", "vision_patch_size", "context_length", "vocab_size", "transformer_width",
                  "transformer_heads", "transformer_layers")


def _check_tower_kwargs(kw):
    """the choices of the reference's Transformer (transformer.py:1949-2004) that exist here; everything else raises at construction"""
    kw = dict(kw)
    block = kw.pop("block_layer", "ResidualAttentionBlock")
    if block not in ("ResidualAttentionBlock", None):
        raise NotImplementedError(f"block_layer {block!r}: only the default ResidualAttentionBlock runs on the executor (the MoE / adapter blocks of "
                                  "transformer.py:1338-1947 are not built)")
    experts = kw.pop("experts_num", 0)
    if experts not in (0, None):
        raise NotImplementedError(f"experts_num {experts}: the mixture-of-experts block is not built")
    act = kw.pop("act_layer", "QuickGELU")
    if act != "QuickGELU":
        raise NotImplementedError(f"act_layer {act!r}: CLIP's towers run QuickGELU (epilogue 6 of clhip_gemm_nt); the checkpoint was trained with it")
    norm = kw.pop("norm_layer", "LayerNorm")
    if norm != "LayerNorm":
        raise NotImplementedError(f"norm_layer {norm!r}: only LayerNorm")
    attn = kw.pop("attn_layer", "MultiHeadAttention")
    if attn not in _CLIP_ATTN:
        raise NotImplementedError(f"attn_layer {attn!r}: the CLIP towers take MultiHeadAttention or MultiHeadAttention_LoRA")
    rank = int(kw.pop("lora_rank", 0) or 0)
    if attn == "MultiHeadAttention_LoRA" and rank <= 0:
        raise NotImplementedError("attn_layer MultiHeadAttention_LoRA needs lora_rank >= 1: the reference's block default of 0 (transformer.py:1293) builds a rank-0 "
                                  "LoRA whose lora_A has no rows for InfLoRA's SVD to fill (InfLoRA_opt.py:256-257)")
    return attn, rank, kw


class VisualTransformer(VisionTransformer):
    """transformer.py:2086-2138 on the executor.  `features()` is the ln_post output at the class token [B, width]; `forward` applies `proj`."""

    def __init__(self, img_size, patch_size, in_chans=3, width=768, depth=12, heads=8, output_dim=512, text_or_image="image", dtype="bf16", **kwargs):
        attn, rank, rest = _check_tower_kwargs(kwargs)
        if rest:
            raise TypeError(f"VisualTransformer: unexpected arguments {sorted(rest)}")
        super().__init__(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=width, depth=depth, num_heads=heads, attn_layer=attn,
                         dtype=dtype, lora_rank=rank)
        self.width, self.heads, self.output_dim = width, heads, output_dim
        self.proj = nn.Parameter((width ** -0.5) * torch.randn(width, output_dim))

    # ---- the stem and head under CLIP's names (transformer.py:2107-2117); the base class builds the blocks between them
    def _make_stem(self, img_size, patch_size, in_chans, embed_dim):
        self.conv1 = _P((embed_dim, in_chans, patch_size, patch_size), bias=False)
        self.class_embedding = nn.Parameter(torch.zeros(embed_dim))
        self.positional_embedding = nn.Parameter(torch.zeros(self.num_patches + 1, embed_dim))
        self.ln_pre = _P((embed_dim,))

    def _make_final_norm(self, embed_dim):
        self.ln_post = _P((embed_dim,))

    def _reset_stem(self):
        scale = self.embed_dim ** -0.5
        nn.init.kaiming_uniform_(self.conv1.weight, a=math.sqrt(5))
        nn.init.normal_(self.class_embedding, std=scale)
        nn.init.normal_(self.positional_embedding, std=scale)
        nn.init.ones_(self.ln_pre.weight); nn.init.zeros_(self.ln_pre.bias)

    def _reset_final_norm(self):
        nn.init.ones_(self.ln_post.weight); nn.init.zeros_(self.ln_post.bias)

    def _stem_tensors(self):
        return self.class_embedding, self.positional_embedding, self.conv1.weight, None, self.ln_post.weight, self.ln_post.bias

    def _ensure(self, dev):
        s = super()._ensure(dev)
        key = (s.handle, self.ln_pre.weight.data_ptr(), self.ln_pre.bias.data_ptr())
        if getattr(s, "clip_key", None) != key:              # a fresh handle, or ln_pre moved: the mode holds the pointers
            call("clhip_vit_set_clip", s.handle, key[1], key[2], 1e-5, 1)
            s.clip_key = key
        return s

    def forward(self, x, get_input_matrix=False, **kwargs):
        if kwargs:
            raise NotImplementedError(f"VisualTransformer.forward: {sorted(kwargs)} (prompts and experts do not combine with the CLIP mode)")
        return ops.linear(self.features(x, None, get_input_matrix), self.proj.t().contiguous())


class CLIP(nn.Module):
    def __init__(self, embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size, context_length, vocab_size, transformer_width,
                 transformer_heads, transformer_layers, baseline=False, dtype="bf16", **kwargs):
        super().__init__()
        if isinstance(vision_layers, (tuple, list)):
            raise NotImplementedError("the ModifiedResNet visual towers (RN50 family, clip.py:206-265) are not built: only the ViT towers run on the executor")
        attn, rank, rest = _check_tower_kwargs(kwargs)
        if rest:
            raise TypeError(f"CLIP: unexpected arguments {sorted(rest)}")
        self.baseline, self.context_length, self.vocab_size, self.lora_rank = baseline, context_length, vocab_size, rank
        self.visual = VisualTransformer(img_size=image_resolution, patch_size=vision_patch_size, width=vision_width, depth=vision_layers,
                                        heads=vision_width // 64, output_dim=embed_dim, dtype=dtype, attn_layer=attn, lora_rank=rank)
        tkw = {"lora_rank": rank} if attn == "MultiHeadAttention_LoRA" else {}
        self.transformer = Transformer(transformer_width, transformer_layers, transformer_heads, 4.0, _CLIP_ATTN[attn], **tkw)
        self.transformer.width, self.transformer.layers = transformer_width, transformer_layers
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, transformer_width))
        self.ln_final = _P((transformer_width,))
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self.initialize_parameters()

    def initialize_parameters(self):
        """clip.py:332-368 (the text tower's scales; the visual tower keeps its own)"""
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        w, n = self.transformer.width, self.transformer.layers
        for blk in self.transformer.blocks:
            nn.init.normal_(blk.attn.qkv.weight, std=w ** -0.5)
            nn.init.normal_(blk.attn.proj.weight, std=(w ** -0.5) * ((2 * n) ** -0.5))
            nn.init.normal_(blk.mlp.fc1.weight, std=(2 * w) ** -0.5)
            nn.init.normal_(blk.mlp.fc2.weight, std=(w ** -0.5) * ((2 * n) ** -0.5))
            for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
                nn.init.zeros_(lin.bias)
            for ln in (blk.ln_1, blk.ln_2):
                nn.init.ones_(ln.weight); nn.init.zeros_(ln.bias)
            if hasattr(blk.attn, "lora_rank"):
                for nme in ("lora_A_k", "lora_B_k", "lora_A_v", "lora_B_v"):
                    nn.init.kaiming_uniform_(getattr(blk.attn, nme).weight, a=math.sqrt(5))
        nn.init.ones_(self.ln_final.weight); nn.init.zeros_(self.ln_final.bias)
        nn.init.normal_(self.text_projection, std=w ** -0.5)

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    def encode_image(self, image, get_input_matrix=False, **kwargs):
        return self.visual(image, get_input_matrix=get_input_matrix, **kwargs)

    @torch.no_grad()
    def encode_text(self, text, **kwargs):
        """clip.py:385-398 in fp32 torch: embedding + positions, the causal blocks, ln_final, the row of the largest token id (the end token) through
        text_projection.  Frozen tower: no gradient, and a LoRA term on a text block is refused (training the text tower is not built)."""
        W = self.positional_embedding.shape[1]
        x = self.token_embedding.weight.float()[text] + self.positional_embedding.float()
        B, L, _ = x.shape
        mask = torch.full((L, L), float("-inf"), device=x.device).triu_(1)
        for blk in self.transformer.blocks:
            a = blk.attn
            if getattr(a, "apply_lora", False):
                raise NotImplementedError("a LoRA term on the text tower (visual_only: false, InfLoRA_opt.py:170-171): training the text tower is not built")
            H = a.num_heads
            h = F.layer_norm(x, (W,), blk.ln_1.weight, blk.ln_1.bias, 1e-5)
            q, k, v = F.linear(h, a.qkv.weight, a.qkv.bias).view(B, L, 3, H, W // H).permute(2, 0, 3, 1, 4)
            att = ((q @ k.transpose(-2, -1)) * a.scale + mask).softmax(dim=-1)
            x = x + F.linear((att @ v).transpose(1, 2).reshape(B, L, W), a.proj.weight, a.proj.bias)
            h = F.linear(F.layer_norm(x, (W,), blk.ln_2.weight, blk.ln_2.bias, 1e-5), blk.mlp.fc1.weight, blk.mlp.fc1.bias)
            x = x + F.linear(h * torch.sigmoid(1.702 * h), blk.mlp.fc2.weight, blk.mlp.fc2.bias)
        x = F.layer_norm(x, (W,), self.ln_final.weight, self.ln_final.bias, 1e-5)
        return x[torch.arange(B, device=x.device), text.argmax(dim=-1)] @ self.text_projection.float()

    def text_features(self, text):
        """the normalised rows CLIP.forward multiplies with (clip.py:409)"""
        t = self.encode_text(text)
        return (t / t.norm(dim=-1, keepdim=True)).contiguous()

    def image_logits(self, image, text_features, scale=None, get_input_matrix=False):
        """the hot path of a step: one executor forward and the logits kernel against already normalised text features -> (logits, u, 1 / |u|)"""
        feat = self.visual.features(image, None, get_input_matrix)
        scale = float(self.logit_scale.exp()) if scale is None else scale
        return ops.clip_logits(feat, self.visual.proj, text_features, scale, with_saved=True)

    def forward(self, image, text, get_input_matrix=False, **kwargs):
        """clip.py:400-416: (normalised image features, normalised text features, logits per image, logits per text)"""
        if image is None:
            return self.encode_text(text, **kwargs)
        if text is None:
            return self.encode_image(image, get_input_matrix=get_input_matrix, **kwargs)
        txt = self.text_features(text)
        logits, u, inv = self.image_logits(image, txt, get_input_matrix=get_input_matrix)
        return u * inv[:, None], txt, logits, logits.T


def _checkpoint_state(path):
    """an OpenAI checkpoint: a TorchScript archive or a pickled state dict -> {name: fp32 tensor} under this module's names (the mapping of clip.py:455-461)"""
    try:
        sd = torch.jit.load(path, map_location="cpu").state_dict()
    except RuntimeError:
        sd = torch.load(path, map_location="cpu")
        sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd.state_dict()
    out = {}
    for k, v in sd.items():
        if k in ("input_resolution", "context_length", "vocab_size"):
            continue
        k = k[7:] if k.startswith("module.") else k
        for old, new in (("attn.in_proj_", "attn.qkv."), ("attn.out_proj.", "attn.proj."), ("mlp.c_fc.", "mlp.fc1."), ("mlp.c_proj.", "mlp.fc2."), (".resblocks.", ".blocks.")):
            k = k.replace(old, new)
        out[k] = v.float()
    return out


def clip(model_name="ViT-B/16", device=None, jit=False, pretrained=False, checkpoint=None, **kwargs):
    """the registry entry `backbone.name: clip` (clip.py:667-668).  pretrained: a LOCAL OpenAI checkpoint (`checkpoint` kwarg or $CLHIP_CLIP_CHECKPOINT; there
    is no network here) sizes and fills the model; otherwise `model_name`'s geometry, each figure of which a kwarg of its name overrides (tests)."""
    if model_name in _RESNET_NAMES:
        raise NotImplementedError(f"{model_name}: the ModifiedResNet towers are not built; the ViT towers {sorted(_GEOMETRY)} run on the executor")
    kwargs.pop("num_classes", None)
    geo = {k: kwargs.pop(k) for k in _GEOMETRY_KEYS if k in kwargs}
    if pretrained:
        path = checkpoint or os.environ.get("CLHIP_CLIP_CHECKPOINT")
        if not path or not os.path.isfile(path):
            raise FileNotFoundError(f"pretrained CLIP weights for {model_name}: no local checkpoint at {path!r} (backbone.kwargs.checkpoint or $CLHIP_CLIP_CHECKPOINT); "
                                    "nothing is downloaded here -- supply OpenAI's ViT-B-16.pt or set pretrained: false")
        sd = _checkpoint_state(path)
        if "visual.proj" not in sd:
            raise NotImplementedError(f"{path}: a ModifiedResNet checkpoint; only the ViT towers are built")
        p = sd["visual.conv1.weight"].shape[-1]
        g = round((sd["visual.positional_embedding"].shape[0] - 1) ** 0.5)
        tw = sd["ln_final.weight"].shape[0]
        geo = dict(embed_dim=sd["text_projection"].shape[1], image_resolution=p * g,
                   vision_layers=len([k for k in sd if k.startswith("visual.") and k.endswith(".attn.qkv.weight")]), vision_width=sd["visual.conv1.weight"].shape[0],
                   vision_patch_size=p, context_length=sd["positional_embedding"].shape[0], vocab_size=sd["token_embedding.weight"].shape[0],
                   transformer_width=tw, transformer_heads=tw // 64,
                   transformer_layers=len({k.split(".")[2] for k in sd if k.startswith("transformer.blocks.")}))
        model = CLIP(**geo, **kwargs)
        own = model.state_dict()
        bad = sorted(k for k, v in sd.items() if k not in own or tuple(v.shape) != tuple(own[k].shape))
        bad += sorted(k for k in own if k not in sd and ".lora_" not in k)       # (the LoRA factors are this project's: no checkpoint has them)
        if bad:
            raise ValueError(f"{path}: the checkpoint does not fill the model it sized -- unknown, mis-shaped or missing tensors {bad[:8]}"
                             f"{' ...' if len(bad) > 8 else ''}; nothing is left at its random initial value silently")
        model.load_state_dict(sd, strict=False)
    else:
        if model_name not in _GEOMETRY:
            raise NotImplementedError(f"CLIP model {model_name!r}: known geometries are {sorted(_GEOMETRY)}")
        model = CLIP(**{**dict(zip(_GEOMETRY_KEYS, _GEOMETRY[model_name])), **geo}, **kwargs)
    model.eval()
    return model.to(device) if device is not None else model
