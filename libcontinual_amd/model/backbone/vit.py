"""ViT backbone of the L2P / InfLoRA_OPT path on the HIP executor (clhip_vit_*).

Mirror of the reference's object graph and parameter names so that checkpoints, YAML
kwargs and plugin code written against it keep working:

    ViTZoo                     core/model/backbone/vit.py:43-139     (.feat, .prompt, .prompt_flag, create_prompt, forward)
      feat: VisionTransformer  core/model/backbone/transformer.py:2147-2294
        patch_embed.proj, cls_token, pos_embed, transformer.blocks[i].{ln_1, attn.{qkv, proj[, lora_*]}, ln_2, mlp.{fc1, fc2}}, norm
        [ffn_adapt: transformer.blocks[i].adaptmlp.{down_proj, up_proj}   core/model/backbone/petl/vision_transformer_adapter.py:31-90]
    MultiHeadAttention_LoRA    transformer.py:199-274   (apply_lora, init_param, merge_weight, reset_input_matrix, cur_matrix)
    MultiHeadAttention_SDLoRA  transformer.py:276-357   (lora_{A,B}_{q,v}_list, mag_lora, assimilated_mag_lora_{q,v}, init_param)
    MultiHeadAttention_LoRA_Sub transformer.py:359-444  (lora_{A,B}_{k,v}, prev_{k,v}_weight, init_param, save_weight, reset_input_matrix, cur_matrix)
    L2PPrompt                  core/model/backbone/prompt.py:345-406 (prompt, prompt_key)
    CodaPromptPool             core/model/backbone/prompt.py:37-223  (e_p_{l}, e_k_{l}, e_a_{l}, task_count, process_task_count, gram_schmidt)
    DualPromptPool             core/model/backbone/prompt.py:231-337 (g_p_{l}, e_p_{l}, e_k_{l}, task_count, process_task_count)

The modules below only OWN parameters (fp32 masters on the device); they have no forward of their own.  All
compute happens in `VisionTransformer.features()`: ONE C call for the whole forward and ONE for the whole backward
(csrc/vit_plan.hip), wrapped in a single autograd.Function per use (plain / LoRA, L2P-prompted).  What differs from
the reference by design: tokens stay batch-first [B*N, D] in bf16 (or fp32 parity mode) with no permutes; the frozen
weights are kept as compute-dtype copies in both orientations so the backward is GEMMs only; LoRA's B gradient uses
the rank-r shortcut instead of a dense [3D, D] dW; the prompt vote, gather, pull loss and key gradient are one kernel.
"""
import ctypes as C
import math
import os

import torch
import torch.nn as nn

from ... import _lib
from ..._lib import call, require_gpu

_DT = {"bf16": (_lib.BF16, torch.bfloat16), "f32": (_lib.F32, torch.float32)}


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptrs(ts):
    """a C array of the tensors' device pointers (None -> NULL)"""
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _layer_views(flat, shapes):
    """flat [depth, sum of the shapes' sizes] -> one view of every shape per layer, in layer order"""
    sizes = [math.prod(shape) for shape in shapes]
    return [t.view(shape) for row in flat.unbind(0) for t, shape in zip(row.split(sizes), shapes)]


def _prefix_tables(depth, layers, pk, pv):
    """`prefix` of _run_forward from the prefixed layers and their [B, Lp, D] key / value tensors: (Lp, pk, pv), each [depth], 0 / None on a plain layer"""
    lp, k_, v_ = [0] * depth, [None] * depth, [None] * depth
    for l, k, v in zip(layers, pk, pv):
        lp[l], k_[l], v_[l] = k.shape[1], k, v
    return lp, k_, v_


def _check_token(vit, token):
    if vit._fwd_token != token:
        raise RuntimeError("the ViT workspace was overwritten by a later forward before this backward ran")


class _P(nn.Module):
    """parameter holder with nn.Linear-style attribute names"""

    def __init__(self, w_shape, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(*w_shape))
        self.bias = nn.Parameter(torch.zeros(w_shape[0])) if bias else None

    def forward(self, *a, **k):
        raise RuntimeError("parameter holder: the HIP executor (VisionTransformer.features) runs the layer")


class LazyGram:
    """running mean of X^T X over the tokens seen so far (transformer.py:241-244) whose per-batch sums stay ON THE DEVICE: the executor adds
    every batch's X^T X into `dev` (a [D, D] fp32 view of the backbone's resident [depth, D, D] buffer) and `n_dev` counts the tokens in it;
    the host tensor the reference keeps (`cur_matrix`, the SVD's input) is brought up to date when somebody READS it --
    (host * n_host + dev) / (n_host + n_dev), the reference's per-batch update with all pending batches as one -- i.e. one transfer per
    task boundary instead of one per batch and layer."""

    def __init__(self, dim):
        self.host, self.n_host = torch.zeros(dim, dim), 0
        self.dev, self.n_dev = None, 0

    def fold(self):
        if self.n_dev:
            self.host = (self.host * self.n_host + self.dev.cpu()) / (self.n_host + self.n_dev)
            self.n_host += self.n_dev
            self.drop_pending()

    def drop_pending(self):
        if self.n_dev:
            self.dev.zero_()
        self.n_dev = 0

    def __deepcopy__(self, memo):          # a copied module starts from the folded host state (device views are never shared)
        self.fold()
        c = LazyGram(self.host.shape[0])
        c.host, c.n_host = self.host.clone(), self.n_host
        return c


def lazy_gram_attrs(matrix_name, count_name, slot):
    """(matrix, count) properties over a LazyGram kept in `self.__dict__[slot]`: reads fold the pending device sums, `x = zeros` /
    `n = 0` drop them -- the plugin code written against the reference's plain attributes runs unchanged"""

    def get_m(self):
        g = self.__dict__[slot]
        g.fold()
        return g.host

    def set_m(self, v):
        g = self.__dict__[slot]
        g.drop_pending()
        g.host = v

    def get_n(self):
        g = self.__dict__[slot]
        return g.n_host + g.n_dev

    def set_n(self, v):
        g = self.__dict__[slot]
        if v == 0:
            g.drop_pending()
        else:
            g.fold()
        g.n_host = v

    return property(get_m, set_m), property(get_n, set_n)


class MultiHeadAttention(nn.Module):
    def __init__(self, dim, num_heads, **kw):
        super().__init__()
        self.dim, self.num_heads = dim, num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = _P((3 * dim, dim))
        self.proj = _P((dim, dim))


class MultiHeadAttention_LoRA(MultiHeadAttention):
    """transformer.py:199-274: LoRA on k and v; `cur_matrix` is the running mean of the attention input's Gram"""

    def __init__(self, dim, num_heads, lora_rank=10, lora_bias=False, **kw):
        super().__init__(dim, num_heads)
        assert not lora_bias
        self.lora_rank = lora_rank
        self.lora_A_k, self.lora_B_k = _P((lora_rank, dim), False), _P((dim, lora_rank), False)
        self.lora_A_v, self.lora_B_v = _P((lora_rank, dim), False), _P((dim, lora_rank), False)
        self.apply_lora = False
        self.__dict__["_gram"] = LazyGram(dim)           # `cur_matrix` (CPU, the SVD input, like the reference) / `n_cur_matrix` live in it

    cur_matrix, n_cur_matrix = lazy_gram_attrs("cur_matrix", "n_cur_matrix", "_gram")

    def init_param(self):
        nn.init.kaiming_uniform_(self.lora_A_k.weight, a=math.sqrt(5))
        nn.init.kaiming_uniform_(self.lora_A_v.weight, a=math.sqrt(5))
        nn.init.zeros_(self.lora_B_k.weight)
        nn.init.zeros_(self.lora_B_v.weight)
        self.apply_lora = True

    @torch.no_grad()
    def merge_weight(self):
        w = self.qkv.weight
        require_gpu(w)
        call("clhip_lora_merge", w.data_ptr(), self.lora_A_k.weight.data_ptr(), self.lora_B_k.weight.data_ptr(),
             self.lora_A_v.weight.data_ptr(), self.lora_B_v.weight.data_ptr(), self.dim, self.lora_rank, _st())
        w.add_(0)                                        # bump the version counter: the executor refreshes its copies
        self.apply_lora = False

    def reset_input_matrix(self):
        self.n_cur_matrix = 0                            # (drops the pending device sums first: nothing is transferred for a reset)
        self.cur_matrix.zero_()


class MultiHeadAttention_LoRA_Sub(MultiHeadAttention_LoRA):
    """transformer.py:359-444: LoRA on k and v whose finished terms are kept in the buffers `prev_k_weight` / `prev_v_weight` [D, D] instead of being merged
    into the pretrained weight, which is never modified.  The k / v rows of the qkv weight take three forms: W - prev for the Gram pass of `before_task`
    (the "subtraction"), (W + prev) + B A while `apply_lora` (training: A and B both train), W + prev otherwise.  The executor reads one of two composed
    fp32 masters (`executor_weight`), rebuilt on the device whenever W or prev changed -- once per task, plain torch."""

    def __init__(self, dim, num_heads, lora_rank=10, lora_bias=False, **kw):
        if lora_bias:
            raise NotImplementedError("lora_bias: true -- the effective-weight form W + B A has no place for the factors' biases")
        super().__init__(dim, num_heads, lora_rank=lora_rank)
        self.register_buffer("prev_k_weight", torch.zeros(dim, dim))
        self.register_buffer("prev_v_weight", torch.zeros(dim, dim))
        self.register_buffer("_w_plus", torch.zeros(3 * dim, dim), persistent=False)
        self.register_buffer("_w_minus", torch.zeros(3 * dim, dim), persistent=False)
        self.subtract = False            # True during the Gram pass: the executor reads W - prev
        self._composed = None

    @torch.no_grad()
    def executor_weight(self):
        """the composed master the executor's qkv_w points at: W - prev while `subtract`, else W + prev"""
        w = self.qkv.weight
        sig = (w.data_ptr(), w._version, self.prev_k_weight.data_ptr(), self.prev_k_weight._version, self.prev_v_weight.data_ptr(),
               self.prev_v_weight._version, self._w_plus.data_ptr())
        if self._composed != sig:
            D = self.dim
            for dst, sign in ((self._w_plus, 1.0), (self._w_minus, -1.0)):
                dst.copy_(w)
                dst[D:2 * D].add_(self.prev_k_weight, alpha=sign)
                dst[2 * D:].add_(self.prev_v_weight, alpha=sign)
            self._composed = sig
        return self._w_minus if self.subtract else self._w_plus

    @torch.no_grad()
    def save_weight(self):
        self.prev_k_weight += self.lora_B_k.weight @ self.lora_A_k.weight
        self.prev_v_weight += self.lora_B_v.weight @ self.lora_A_v.weight
        self.apply_lora = False

    def merge_weight(self):
        raise NotImplementedError("LoRA-Sub keeps its finished terms in prev_k_weight / prev_v_weight (save_weight); the pretrained weight is never modified")


class MultiHeadAttention_SDLoRA(MultiHeadAttention):
    """transformer.py:276-357: on q and v a sum over the tasks so far of low-rank terms, the past ones normalised to unit Frobenius norm, each scaled
    by a trainable scalar of `mag_lora` (a ParameterList the method assigns, the same object in every block).  The lists hold parameter holders, so
    the names are `...lora_A_q_list.{i}.weight` as in the reference (sd_lora.py:130-136 filters on them).  `lora_rank` is mutable: init_param appends
    a term of the rank it has then (rank reduction, sd_lora.py:112-119)."""

    def __init__(self, dim, num_heads, lora_rank=10, lora_bias=False, **kw):
        super().__init__(dim, num_heads)
        assert not lora_bias
        self.lora_rank, self.lora_bias = lora_rank, lora_bias
        self.lora_A_q_list, self.lora_B_q_list = nn.ModuleList([]), nn.ModuleList([])
        self.lora_A_v_list, self.lora_B_v_list = nn.ModuleList([]), nn.ModuleList([])
        self.assimilated_mag_lora_q, self.assimilated_mag_lora_v = [], []      # 0 unless knowledge distillation merges a term: never enter the kernels

    def factor_lists(self):
        return (self.lora_A_q_list, self.lora_B_q_list, self.lora_A_v_list, self.lora_B_v_list)

    def init_param(self):
        dev, r = self.qkv.weight.device, int(self.lora_rank)
        for lst, shape in zip(self.factor_lists(), ((r, self.dim), (self.dim, r), (r, self.dim), (self.dim, r))):
            lst.append(_P(shape, False))
        nn.init.kaiming_uniform_(self.lora_A_q_list[-1].weight, a=math.sqrt(5))
        nn.init.kaiming_uniform_(self.lora_A_v_list[-1].weight, a=math.sqrt(5))
        nn.init.zeros_(self.lora_B_q_list[-1].weight)
        nn.init.zeros_(self.lora_B_v_list[-1].weight)
        for lst in self.factor_lists():
            lst[-1].to(dev)
        self.assimilated_mag_lora_q.append(torch.zeros(1, device=dev))
        self.assimilated_mag_lora_v.append(torch.zeros(1, device=dev))
        assert len(self.lora_A_q_list) == len(self.mag_lora)
        assert len(self.mag_lora) == len(self.assimilated_mag_lora_q)


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1, self.fc2 = _P((hidden, dim)), _P((dim, hidden))


class Adapter(nn.Module):
    """petl/vision_transformer_adapter.py:31-90 with ffn_adapter_layernorm_option "none": down_proj [R, D] -> ReLU -> dropout -> up_proj [D, R], times
    `scale`, added to the block output in parallel to the MLP.  init_option "lora": kaiming_uniform(a = sqrt 5) on down_proj, zeros elsewhere, so a
    fresh adapter is the identity."""

    def __init__(self, dim, bottleneck, scale=0.1, dropout=0.1):
        super().__init__()
        self.n_embd, self.down_size, self.scale, self.dropout = dim, bottleneck, float(scale), float(dropout)
        self.down_proj, self.up_proj = _P((bottleneck, dim)), _P((dim, bottleneck))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.down_proj.weight, a=math.sqrt(5))
        nn.init.zeros_(self.up_proj.weight)
        nn.init.zeros_(self.down_proj.bias)
        nn.init.zeros_(self.up_proj.bias)

    def tensors(self):
        return [self.down_proj.weight, self.down_proj.bias, self.up_proj.weight, self.up_proj.bias]


class ResidualAttentionBlock(nn.Module):
    def __init__(self, dim, heads, mlp_ratio, attn_layer, **kw):
        super().__init__()
        self.attn = attn_layer(dim, heads, **kw)
        self.ln_1 = _P((dim,))
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        self.ln_2 = _P((dim,))


class Transformer(nn.Module):
    def __init__(self, dim, depth, heads, mlp_ratio, attn_layer, **kw):
        super().__init__()
        self.blocks = nn.ModuleList([ResidualAttentionBlock(dim, heads, mlp_ratio, attn_layer, **kw) for _ in range(depth)])


class _PatchEmbed(nn.Module):
    def __init__(self, img_size, patch_size, in_chans, embed_dim):
        super().__init__()
        self.num_patches = (img_size // patch_size) ** 2
        self.proj = _P((embed_dim, in_chans, patch_size, patch_size))


_ATTN = {"MultiHeadAttention": MultiHeadAttention, "MultiHeadAttention_LoRA": MultiHeadAttention_LoRA,
         "MultiHeadAttention_SDLoRA": MultiHeadAttention_SDLoRA, "MultiHeadAttention_LoRA_Sub": MultiHeadAttention_LoRA_Sub}


class _Scratch:
    """non-module state (C handle, device buffers): never copied / moved with the module, rebuilt on demand"""

    def __init__(self):
        self.handle = None
        self.shadow = None
        self.ws = None
        self.ws_key = None
        self.sig = None
        self.cparams = None
        self.keep = None
        self.gram = None
        self.sd_key = None        # SD-LoRA: identity of the term set the executor was told about, and its device tables
        self.sd_tab = self.sd_ranks = self.sd_mag = self.sd_inv = None
        self.prefix_on = False    # the executor's prefix mode (clhip_vit_set_prefix) as this module last left it
        self.layers = None        # the per-layer parameter table `cparams` points to
        self.ab_grads = self.ab_ws = None     # LoRA-Sub: the factor gradients [depth, 4 r D] and the scratch of clhip_lora_grad_ab, reused from step to step

    def __deepcopy__(self, memo):
        return _Scratch()


class _VitFn(torch.autograd.Function):
    """features = ViT(images [, prompt tokens]); backward -> the gradients `want` names (VisionTransformer._run_backward), d prompt tokens first, then those of
    `params` in its order: "lora_b" the lora_B weights (k, v per layer) and / or "adapter" the adapter tensors (down w, down b, up w, up b per layer); "sd" A_q,
    B_q, A_v, B_v of the current SD-LoRA term per layer, then the magnitudes (transformer.py:317-332 under autograd in the reference); "ab" A_k, B_k, A_v, B_v
    per layer (LoRA-Sub, transformer.py:415-418)"""

    @staticmethod
    def forward(ctx, vit, images, prompt_tokens, gram, need, want, *params):
        feat = vit._run_forward(images, prompt_tokens, need, gram)
        ctx.vit, ctx.token, ctx.want = vit, vit._fwd_token, want
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        _check_token(ctx.vit, ctx.token)
        g = ctx.vit._run_backward(dfeat, ctx.want)
        return (None, None, g.get("prompt"), None, None, None) + tuple(t for k in ("lora_b", "adapter", "sd", "ab") for t in g.get(k, ()))


class _CodaFn(torch.autograd.Function):
    """query pass (no prefix) -> prompt assembly (clhip_coda_fwd) -> prefixed forward; backward = clhip_vit_backward (dpk, dpv) -> clhip_coda_bwd.
    `params` = K, A, P of every prompted layer, in layer order"""

    @staticmethod
    def forward(ctx, vit, layers, images, need, s_, f_, pool, length, *params):
        q = vit._run_forward(images, None, 0, None)                      # norm(x)[:, 0] of the prompt-free forward (vit.py:121-123)
        B, D, n, Lp = q.shape[0], vit.embed_dim, len(layers), length // 2
        dev, (code, tdt) = q.device, _DT[vit.compute_dtype]
        for t in params:
            require_gpu(t)
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.ClhipError("the CODA-Prompt pool must be contiguous fp32")
        e = torch.empty(2, n, B, Lp, D, device=dev, dtype=tdt)
        c = torch.empty(n, B, f_, device=dev)
        K, A, P = params[0::3], params[1::3], params[2::3]
        ek, ev = e[0].unbind(0), e[1].unbind(0)
        call("clhip_coda_fwd", n, q.data_ptr(), _ptrs(K), _ptrs(A), _ptrs(P), _ptrs(ek), _ptrs(ev), c.data_ptr(), B, D, pool, length, f_, code, _st())
        lp, pk, pv = _prefix_tables(vit.depth, layers, ek, ev)
        feat = vit._run_forward(images, None, need, None, prefix=(lp, pk, pv))
        ctx.vit, ctx.token, ctx.lp, ctx.layers, ctx.dims = vit, vit._fwd_token, lp, layers, (pool, length, s_, f_)
        ctx.keep = (q, c, e)                                             # e: the executor reads the prefixes again in the backward
        ctx.params = params
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        vit = ctx.vit
        _check_token(vit, ctx.token)
        q, c, _ = ctx.keep
        pool, length, s_, f_ = ctx.dims
        n, B, D = len(ctx.layers), q.shape[0], vit.embed_dim
        g = vit._run_backward(dfeat, prefix_lp=ctx.lp)
        params = ctx.params
        grads = [torch.zeros_like(t) for t in params]                    # rows outside [s, f) get no gradient
        ws = torch.empty(_lib.lib().clhip_coda_ws_bytes(n, B, s_, f_) // 4, device=q.device)
        call("clhip_coda_bwd", n, q.data_ptr(), _ptrs(params[0::3]), _ptrs(params[1::3]), _ptrs(params[2::3]), c.data_ptr(),
             _ptrs([g["dpk"][l] for l in ctx.layers]), _ptrs([g["dpv"][l] for l in ctx.layers]), _ptrs(grads[0::3]), _ptrs(grads[1::3]), _ptrs(grads[2::3]),
             ws.data_ptr(), B, D, pool, length, s_, f_, _st())
        return (None,) * 8 + tuple(grads)


class _DualFn(torch.autograd.Function):
    """query pass (no prefix) -> prompt selection (clhip_dual_fwd) -> prefixed forward; backward = clhip_vit_backward (dpk, dpv) -> clhip_dual_bwd.
    -> (features, key loss [1]).  `params` = g_p of every G-layer, then e_k, e_p of every E-layer, in layer order"""

    @staticmethod
    def forward(ctx, vit, pool, images, need, train, task_id, *params):
        q = vit._run_forward(images, None, 0, None)                      # norm(x)[:, 0] of the prompt-free forward (vit.py:121-123)
        gl, el, Lg, Le, size = pool.g_layers, pool.e_layers, pool.g_p_length, pool.e_p_length, pool.e_pool_size
        B, D, ng, ne = q.shape[0], vit.embed_dim, len(gl), len(el)
        dev, (code, tdt) = q.device, _DT[vit.compute_dtype]
        for t in params:
            require_gpu(t)
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.ClhipError("the DualPrompt pool must be contiguous fp32")
        g_p, e_k, e_p = params[:ng], params[ng::2], params[ng + 1::2]
        pre = [torch.empty(2, B, L // 2, D, device=dev, dtype=tdt) for L in [Lg] * ng + [Le] * ne]
        cos = torch.empty(ne, B, size, device=dev)
        idx = torch.empty(ne, B, device=dev, dtype=torch.int32)
        loss = torch.zeros(1, device=dev)                                # (eval mode leaves it alone)
        ek, ev = [p[0] for p in pre], [p[1] for p in pre]
        call("clhip_dual_fwd", ng, ne, q.data_ptr(), _ptrs(g_p), _ptrs(e_k), _ptrs(e_p), _ptrs(ek), _ptrs(ev), cos.data_ptr(), idx.data_ptr(), loss.data_ptr(), B, D,
             size, Lg, Le, int(train), int(task_id) if train else 0, code, _st())
        lp, pk, pv = _prefix_tables(vit.depth, list(gl) + list(el), ek, ev)
        feat = vit._run_forward(images, None, need, None, prefix=(lp, pk, pv))
        pool.last_cos, pool.last_idx = cos, idx
        ctx.vit, ctx.token, ctx.lp, ctx.pool, ctx.task_id, ctx.train = vit, vit._fwd_token, lp, pool, task_id, train
        ctx.keep = (q, pre)                                              # pre: the executor reads the prefixes again in the backward
        ctx.params = params
        return feat, loss

    @staticmethod
    def backward(ctx, dfeat, dloss):
        vit, pool = ctx.vit, ctx.pool
        _check_token(vit, ctx.token)
        if not ctx.train:
            raise RuntimeError("DualPrompt: the inference selection (arg-max over the keys) has no backward")
        q, _ = ctx.keep
        gl, el = pool.g_layers, pool.e_layers
        B, D, ng, ne = q.shape[0], vit.embed_dim, len(gl), len(el)
        if dfeat is None:
            dfeat = torch.zeros(B, D, device=q.device)
        dloss = torch.zeros(1, device=q.device) if dloss is None else dloss.float().reshape(1).contiguous()
        g = vit._run_backward(dfeat, prefix_lp=ctx.lp)
        params = ctx.params
        grads = [torch.zeros_like(t) for t in params]                    # rows other than task_id get no gradient
        order = list(gl) + list(el)
        call("clhip_dual_bwd", ng, ne, q.data_ptr(), _ptrs(params[ng::2]), _ptrs([g["dpk"][l] for l in order]), _ptrs([g["dpv"][l] for l in order]),
             dloss.data_ptr(), _ptrs(grads[:ng]), _ptrs(grads[ng::2]), _ptrs(grads[ng + 1::2]), B, D, pool.e_pool_size, pool.g_p_length, pool.e_p_length,
             int(ctx.task_id), _st())
        return (None,) * 6 + tuple(grads)


class VisionTransformer(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, attn_layer="MultiHeadAttention",
                 mlp_ratio=4.0, dtype="bf16", lora_rank=0, ffn_adapt=False, ffn_num=64, ffn_adapter_scalar=0.1, adapter_dropout=0.1, **kwargs):
        super().__init__()
        assert in_chans == 3
        if isinstance(attn_layer, str):
            if attn_layer not in _ATTN:
                raise NotImplementedError(f"attn_layer {attn_layer} is outside the hot-path scope (SURVEY.md section 8)")
            attn_layer = _ATTN[attn_layer]
        self.img_size, self.patch_size, self.embed_dim, self.depth, self.num_heads = img_size, patch_size, embed_dim, depth, num_heads
        self.num_features = embed_dim
        self.mlp_dim = int(embed_dim * mlp_ratio)
        self.lora_sub = attn_layer is MultiHeadAttention_LoRA_Sub
        self.lora_rank = lora_rank if attn_layer is MultiHeadAttention_LoRA or self.lora_sub else 0
        self.compute_dtype = dtype
        self.num_patches = (img_size // patch_size) ** 2
        self._make_stem(img_size, patch_size, in_chans, embed_dim)
        self.sd_lora = attn_layer is MultiHeadAttention_SDLoRA
        kw = {"lora_rank": lora_rank} if self.lora_rank or self.sd_lora else {}
        if self.lora_sub:
            kw["lora_bias"] = kwargs.get("lora_bias", False)
        self.transformer = Transformer(embed_dim, depth, num_heads, mlp_ratio, attn_layer, **kw)
        self._make_final_norm(embed_dim)
        self._s = _Scratch()
        self._fwd_token = 0
        self.reset_parameters()
        # AdaptFormer adapters (the reference's tuning config of vit_pt_imnet_in21k_adapter: ffn_adapt, ffn_num 64, scalar 0.1, dropout 0.1): created
        # after every other parameter, so a model without them draws exactly the initial values it always drew.  The adapter tree is timm's:
        # every LayerNorm has eps 1e-6, and only the adapters train (vision_transformer_adapter.py:461-466).
        self.adapter_dim = int(ffn_num) if ffn_adapt else 0
        self.adapter_scale, self.adapter_dropout = float(ffn_adapter_scalar), float(adapter_dropout)
        self.last_dropout_seed = None
        if self.adapter_dim:
            if self.adapter_dim not in (16, 32, 64):
                raise NotImplementedError(f"ffn_num {ffn_num}: the adapter kernels take a bottleneck of 16, 32 or 64")
            if not 0.0 <= self.adapter_dropout < 1.0:
                raise ValueError(f"adapter_dropout {adapter_dropout} is outside [0, 1)")
            self.block_ln_eps = 1e-6
            for p in self.parameters():
                p.requires_grad_(False)
            for blk in self.transformer.blocks:
                blk.adaptmlp = Adapter(embed_dim, self.adapter_dim, self.adapter_scale, self.adapter_dropout)

    # ------------------------------------------------------------------ the parts a sibling tower names differently (backbone/clip.py: VisualTransformer)
    def _make_stem(self, img_size, patch_size, in_chans, embed_dim):
        self.patch_embed = _PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.num_patches + 1, embed_dim))

    def _make_final_norm(self, embed_dim):
        self.norm = _P((embed_dim,))

    def _reset_stem(self):
        nn.init.trunc_normal_(self.pos_embed, std=.02)
        nn.init.trunc_normal_(self.cls_token, std=.02)
        w = self.patch_embed.proj.weight
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        bound = 1 / math.sqrt(w[0].numel())
        nn.init.uniform_(self.patch_embed.proj.bias, -bound, bound)

    def _reset_final_norm(self):
        nn.init.ones_(self.norm.weight); nn.init.zeros_(self.norm.bias)

    def _stem_tensors(self):
        """(cls token, positional embedding, patch weight, patch bias or None, final norm weight, final norm bias): the executor's clhip_vit_params"""
        return self.cls_token, self.pos_embed, self.patch_embed.proj.weight, self.patch_embed.proj.bias, self.norm.weight, self.norm.bias

    # ------------------------------------------------------------------ init (transformer.py:2201-2213, timm PatchEmbed)
    def reset_parameters(self):
        self._reset_stem()
        for blk in self.transformer.blocks:
            for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
                nn.init.trunc_normal_(lin.weight, std=.02)
                nn.init.zeros_(lin.bias)
            for ln in (blk.ln_1, blk.ln_2):
                nn.init.ones_(ln.weight); nn.init.zeros_(ln.bias)
            if self.lora_rank:
                for n in ("lora_A_k", "lora_B_k", "lora_A_v", "lora_B_v"):
                    nn.init.trunc_normal_(getattr(blk.attn, n).weight, std=.02)
        self._reset_final_norm()

    # ------------------------------------------------------------------------------------ executor state
    def attention_modules(self):
        return [b.attn for b in self.transformer.blocks]

    def adapter_tensors(self):
        """down w, down b, up w, up b of every layer, in layer order (empty without adapters)"""
        return [t for b in self.transformer.blocks for t in b.adaptmlp.tensors()] if self.adapter_dim else []

    def _qkv_master(self, b):
        """the fp32 qkv weight the executor reads for block b: the parameter itself, or LoRA-Sub's composed W +- prev"""
        return b.attn.executor_weight() if self.lora_sub else b.attn.qkv.weight

    def _frozen_tensors(self):
        out = [self._stem_tensors()[2]]
        for b in self.transformer.blocks:
            out += [self._qkv_master(b), b.attn.proj.weight, b.mlp.fc1.weight, b.mlp.fc2.weight]
        return out

    def _all_tensors(self):
        return [p for p in self.parameters()]

    def _ensure(self, dev):
        s = self._s
        if s.handle is None:
            desc = _lib.VitDesc(self.img_size, self.patch_size, self.embed_dim, self.depth, self.num_heads, self.mlp_dim, self.lora_rank,
                                float(getattr(self, "block_ln_eps", 0.0)), self.adapter_dim, self.adapter_scale)
            h = _lib.lib().clhip_vit_create(C.byref(desc), _DT[self.compute_dtype][0])
            if not h:
                raise _lib.ClhipError(_lib.lib().clhip_last_error().decode())
            s.handle = h
        if s.shadow is None or s.shadow.device != dev:
            s.shadow = torch.empty(_lib.lib().clhip_vit_shadow_bytes(s.handle), dtype=torch.uint8, device=dev)
            s.sig = None
        # parameter pointer table + staleness signature of the compute-dtype weight copies
        ptrs = tuple(p.data_ptr() for p in self._all_tensors())
        if self.lora_sub:
            ptrs += tuple(self._qkv_master(b).data_ptr() for b in self.transformer.blocks)
        if s.cparams is None or s.keep != ptrs:
            for p in self._all_tensors():
                require_gpu(p)
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise _lib.ClhipError("ViT master parameters must be contiguous fp32")
            layers = (_lib.VitLayerParams * self.depth)()
            for i, b in enumerate(self.transformer.blocks):
                L = layers[i]
                L.qkv_w, L.qkv_b = self._qkv_master(b).data_ptr(), b.attn.qkv.bias.data_ptr()
                L.proj_w, L.proj_b = b.attn.proj.weight.data_ptr(), b.attn.proj.bias.data_ptr()
                L.ln1_w, L.ln1_b = b.ln_1.weight.data_ptr(), b.ln_1.bias.data_ptr()
                L.fc1_w, L.fc1_b = b.mlp.fc1.weight.data_ptr(), b.mlp.fc1.bias.data_ptr()
                L.fc2_w, L.fc2_b = b.mlp.fc2.weight.data_ptr(), b.mlp.fc2.bias.data_ptr()
                L.ln2_w, L.ln2_b = b.ln_2.weight.data_ptr(), b.ln_2.bias.data_ptr()
                if self.lora_rank:
                    L.lora_a_k, L.lora_b_k = b.attn.lora_A_k.weight.data_ptr(), b.attn.lora_B_k.weight.data_ptr()
                    L.lora_a_v, L.lora_b_v = b.attn.lora_A_v.weight.data_ptr(), b.attn.lora_B_v.weight.data_ptr()
                if self.adapter_dim:
                    L.ad_down_w, L.ad_down_b, L.ad_up_w, L.ad_up_b = [t.data_ptr() for t in b.adaptmlp.tensors()]
            cp = _lib.VitParams(*[None if t is None else t.data_ptr() for t in self._stem_tensors()], layers)
            s.cparams, s.keep, s.layers = cp, ptrs, layers
            s.sig = None
        lora_on = bool(self.lora_rank) and any(a.apply_lora for a in self.attention_modules())
        if lora_on and not all(a.apply_lora for a in self.attention_modules()):
            raise _lib.ClhipError("apply_lora must be set on all attention layers or none")
        frozen = self._frozen_tensors()
        if self.lora_sub and lora_on and any(a.subtract for a in self.attention_modules()):
            raise _lib.ClhipError("the Gram pass on W - prev runs without the LoRA term (transformer.py:407-413): clear apply_lora or subtract")
        if self.lora_rank and not self.lora_sub:   # lora_A is fixed within a task: a change (init_param / SVD in before_task) forces the full preparation
            for a in self.attention_modules():
                frozen = frozen + [a.lora_A_k.weight, a.lora_A_v.weight]
        if self.sd_lora:
            return self._ensure_sd(s, dev, frozen)
        sig = (tuple((t.data_ptr(), t._version) for t in frozen), lora_on)
        if s.sig != sig:
            call("clhip_vit_prep_weights", s.handle, C.byref(s.cparams), s.shadow.data_ptr(), int(lora_on), 0, _st())
            s.sig = sig
        elif lora_on and self.lora_sub:
            # A and B both move every optimizer step: the k / v rows of the qkv copies, nothing else is re-rounded
            call("clhip_vit_lora_refresh_ab", s.handle, C.byref(s.cparams), s.shadow.data_ptr(), _st())
        elif lora_on:
            # lora_B moves every optimizer step: refresh only the effective qkv copies (transformer.py:249-255)
            call("clhip_vit_prep_weights", s.handle, C.byref(s.cparams), s.shadow.data_ptr(), 1, 1, _st())
        return s

    # ------------------------------------------------------------------------------------ SD-LoRA state
    def sd_terms(self):
        return len(self.attention_modules()[0].lora_A_q_list) if self.sd_lora else 0

    def sd_trainable(self):
        """the autograd inputs of the SD-LoRA mode: A_q, B_q, A_v, B_v of the last term per layer, then the magnitudes"""
        out = []
        for a in self.attention_modules():
            out += [lst[-1].weight for lst in a.factor_lists()]
        return out + list(self.attention_modules()[0].mag_lora)

    @torch.no_grad()
    def sdlora_update_inv(self):
        """inv [depth, 2, T + 1] on the device, no host synchronisation: 1 / (|B_i|_F |A_i|_F) of the past terms (0 where a norm is 0: the reference
        skips such a term, transformer.py:325, :331) and 1 for the current one.  Constant within a task: sd_lora.SD_LoRA.before_task calls this."""
        mods, T1 = self.attention_modules(), self.sd_terms()
        norms = torch.stack([torch.stack([torch.linalg.vector_norm(h.weight) for h in lst]) for a in mods for lst in a.factor_lists()])
        norms = norms.view(len(mods), 2, 2, T1).double()
        prod = norms[:, :, 0] * norms[:, :, 1]
        inv = torch.where(prod != 0, 1.0 / prod, torch.zeros_like(prod)).float()
        inv[:, :, -1] = 1.0
        self._s.sd_inv = inv.contiguous()
        self._s.sd_key = None                                # the executor is handed the new vector at the next forward

    def _ensure_sd(self, s, dev, frozen):
        """SD-LoRA: the past terms and `inv` are fixed within a task (a change forces the full preparation); the current term and the magnitudes
        move every optimizer step (the fused optimizers write through raw pointers, so no version counter tells), hence the q / v rows of the
        effective qkv copies are refreshed before every forward, as the LoRA path does."""
        mods, T1 = self.attention_modules(), self.sd_terms()
        if T1 == 0:                                          # no term yet: the plain backbone
            if s.sd_key is not None:
                call("clhip_vit_set_sdlora", s.handle, 0, None, None, None, None)
                s.sd_key, s.sig = None, None
            sig = (tuple((t.data_ptr(), t._version) for t in frozen), "sd0")
            if s.sig != sig:
                call("clhip_vit_prep_weights", s.handle, C.byref(s.cparams), s.shadow.data_ptr(), 0, 0, _st())
                s.sig = sig
            return s
        if any(len(lst) != T1 for a in mods for lst in a.factor_lists()) or any(a.mag_lora is not mods[0].mag_lora for a in mods) \
                or len(mods[0].mag_lora) != T1:
            raise _lib.ClhipError("SD-LoRA: every attention layer needs the same number of terms and the one shared mag_lora list with a scalar per term")
        ranks = [h.weight.shape[0] for h in mods[0].lora_A_q_list]
        fact = [[h.weight for h in lst] for a in mods for lst in a.factor_lists()]           # [depth * 4][T1]
        for a in mods:
            for la, lb in ((a.lora_A_q_list, a.lora_B_q_list), (a.lora_A_v_list, a.lora_B_v_list)):
                if [h.weight.shape[0] for h in la] != ranks or [h.weight.shape[1] for h in lb] != ranks:
                    raise _lib.ClhipError("SD-LoRA: the rank of a term must be the same in every layer and for q and v")
        past = [t for row in fact for t in row[:-1]]
        key = (tuple(t.data_ptr() for row in fact for t in row), tuple(ranks), tuple((t.data_ptr(), t._version) for t in past), dev)
        if s.sd_inv is None or tuple(s.sd_inv.shape) != (self.depth, 2, T1) or s.sd_inv.device != dev:
            self.sdlora_update_inv()
        if s.sd_key != key:
            if s.sd_key is not None and s.sd_key[2] != key[2]:
                self.sdlora_update_inv()                     # a past term was changed by hand: its norm moved
            s.sd_tab = torch.tensor([[t.data_ptr() for t in row] for row in fact], dtype=torch.int64).to(dev)
            s.sd_ranks = (C.c_int * T1)(*ranks)
            s.sd_mag = torch.empty(T1, device=dev)
            call("clhip_vit_set_sdlora", s.handle, T1, s.sd_ranks, s.sd_tab.data_ptr(), s.sd_mag.data_ptr(), s.sd_inv.data_ptr())
            s.sd_key, s.sig = key, None
        sig = (tuple((t.data_ptr(), t._version) for t in frozen), key[2], "sd")
        if s.sig != sig:
            call("clhip_vit_prep_weights", s.handle, C.byref(s.cparams), s.shadow.data_ptr(), 0, 0, _st())
            s.sig = sig
        torch.cat([m.detach().reshape(1) for m in mods[0].mag_lora], out=s.sd_mag)
        call("clhip_vit_sdlora_refresh", s.handle, C.byref(s.cparams), s.shadow.data_ptr(), _st())
        return s

    def _workspace(self, s, B, n_prompt, save, dev):
        """`save`: bit 0 = keep what the backward needs, bit 1 = keep every layer's attention input for the Gram launch"""
        key = (B, n_prompt, int(save))
        need = _lib.lib().clhip_vit_workspace_bytes(s.handle, B, n_prompt, int(save))
        if need == 0:
            raise _lib.ClhipError(f"invalid ViT launch: batch {B}, {n_prompt} prompt tokens (max 256 tokens)")
        if s.ws is None or s.ws.device != dev or s.ws.numel() < need:
            s.ws = None
            s.ws = torch.empty(need, dtype=torch.uint8, device=dev)
        s.ws_key = key
        return s.ws

    def _run_forward(self, images, prompt_tokens, save, gram, prefix=None):
        """prefix: None, or (Lp [depth] ints, pk [depth], pv [depth] tensors or None) -- the layers with Lp > 0 attend over [prefix | tokens]"""
        require_gpu(images)
        images = images.float().contiguous()
        B = images.shape[0]
        if tuple(images.shape[1:]) != (3, self.img_size, self.img_size):
            raise _lib.ClhipError(f"expected images [B,3,{self.img_size},{self.img_size}], got {tuple(images.shape)}")
        dev = images.device
        s = self._ensure(dev)
        n_prompt = 0
        if prompt_tokens is not None:
            prompt_tokens = prompt_tokens.detach().float().contiguous()
            n_prompt = prompt_tokens.shape[0]
        ws = self._workspace(s, B, n_prompt, int(bool(save)) | (2 if gram is not None else 0), dev)
        feat = torch.empty(B, self.embed_dim, device=dev, dtype=torch.float32)
        if prefix is not None:
            lp, pk, pv = prefix
            call("clhip_vit_set_prefix", s.handle, (C.c_int * self.depth)(*lp), _ptrs(pk), _ptrs(pv))
            s.prefix_on = True
        elif s.prefix_on:                                    # the mode persists in the executor: every other forward runs without it
            call("clhip_vit_set_prefix", s.handle, None, None, None)
            s.prefix_on = False
        self.last_dropout_seed = None
        if self.adapter_dim and self.training and self.adapter_dropout > 0.0:
            # one 64-bit word from the device generator (the one init_seed seeds): no synchronisation, and the CPU generator is left alone
            self.last_dropout_seed = torch.empty(1, dtype=torch.int64, device=dev).random_()
            call("clhip_vit_set_adapter_dropout", s.handle, self.last_dropout_seed.data_ptr(), self.adapter_dropout)
        call("clhip_vit_forward", s.handle, C.byref(s.cparams), s.shadow.data_ptr(), ws.data_ptr(), images.data_ptr(), B,
             prompt_tokens.data_ptr() if n_prompt else None, n_prompt, int(save), gram.data_ptr() if gram is not None else None,
             feat.data_ptr(), _st())
        self._fwd_token += 1
        self._last = (B, n_prompt)
        return feat

    def _run_backward(self, dfeat, want=(), prefix_lp=None):
        """the backward of the last saving forward, one clhip_vit_backward -> {name: gradient(s)}.  want: names among "prompt" [n_prompt, D]; "lora_b" [D, r] k, v per
        layer; "adapter" d down w, down b, up w, up b per layer; "sd" d A_q, B_q, A_v, B_v of the current term per layer, then one [1] slice per magnitude; "ab" d A_k,
        B_k, A_v, B_v per layer (views of one buffer that is reused from step to step).  prefix_lp: Lp [depth] of a prefixed forward, which adds "dpk" / "dpv": per
        layer a fp32 [B, Lp, D] tensor, None where Lp = 0"""
        s = self._s
        B, n_prompt = self._last
        dfeat = dfeat.float().contiguous()
        dev, D, depth = dfeat.device, self.embed_dim, self.depth
        out, G = {}, _lib.VitGrads()
        if "prompt" in want:
            out["prompt"] = torch.empty(n_prompt, D, device=dev)
            G.dprompt_tokens = out["prompt"].data_ptr()
        if "lora_b" in want:
            out["lora_b"] = list(torch.zeros(2 * depth, D, self.lora_rank, device=dev).unbind(0))            # one fill, 2*depth views
            G.d_lora_b = _ptrs(out["lora_b"])
        if "adapter" in want:                                # (the kernels write every element of the adapter, SD-LoRA, LoRA-Sub and prefix gradients)
            R = self.adapter_dim
            out["adapter"] = _layer_views(torch.empty(depth, 2 * R * D + R + D, device=dev), [(R, D), (R,), (D, R), (D,)])
            G.d_adapter = _ptrs(out["adapter"])
        if "sd" in want:
            T1, r = self.sd_terms(), self.attention_modules()[0].lora_A_q_list[-1].weight.shape[0]
            fac = _layer_views(torch.empty(depth, 4 * r * D, device=dev), [(r, D), (D, r)] * 2)
            rows, dmag = torch.empty(depth, T1, device=dev), torch.empty(T1, device=dev)
            G.d_sd, G.d_mag_rows, G.d_mag = _ptrs(fac), rows.data_ptr(), dmag.data_ptr()
            out["sd"] = fac + [dmag[i:i + 1] for i in range(T1)]
        if "ab" in want:
            r, need = self.lora_rank, _lib.lib().clhip_lora_grad_ab_ws_bytes(B * (n_prompt + 1 + self.num_patches), D)
            if s.ab_grads is None or s.ab_grads.device != dev:
                s.ab_grads = torch.empty(depth, 4 * r * D, device=dev)
            if s.ab_ws is None or s.ab_ws.device != dev or s.ab_ws.numel() < need:
                s.ab_ws = torch.empty(need, dtype=torch.uint8, device=dev)
            out["ab"] = _layer_views(s.ab_grads, [(r, D), (D, r)] * 2)
            G.d_ab, G.ab_ws = _ptrs(out["ab"]), s.ab_ws.data_ptr()
        if prefix_lp is not None:
            for k in ("dpk", "dpv"):
                out[k] = [torch.empty(B, n, D, device=dev) if n else None for n in prefix_lp]
                setattr(G, k, _ptrs(out[k]))
        call("clhip_vit_backward", s.handle, C.byref(s.cparams), s.shadow.data_ptr(), s.ws.data_ptr(), dfeat.data_ptr(), C.byref(G), _st())
        return out

    def coda_features(self, images, pool, train=False):
        """ViTZoo.forward with a CODA-Prompt pool (vit.py:120-127): [B, D] fp32, the final-LN output at the cls token of the forward whose blocks
        `pool.e_layers` attend over the assembled prefixes.  Differentiable w.r.t. the pool's tensors (rows of the running task's window)."""
        if self.lora_rank or self.sd_lora or self.adapter_dim:
            raise NotImplementedError("CODA-Prompt runs on the plain frozen backbone")
        if train and pool.ortho_mu > 0:
            raise NotImplementedError("mu > 0: the orthogonality penalty is not built (the reference's ortho_penalty calls .cuda(), prompt.py:222-223)")
        params = pool.layer_tensors()
        need = torch.is_grad_enabled() and any(t.requires_grad for t in params)
        s_, f_ = pool.window()
        return _CodaFn.apply(self, tuple(pool.e_layers), images, need, s_, f_, pool.e_pool_size, pool.e_p_length, *params)

    def dual_features(self, images, pool, train=False, task_id=None):
        """ViTZoo.forward with a DualPrompt pool (vit.py:120-127) -> (features [B, D] fp32, key loss [1]): the final-LN output at the cls token of the
        forward whose blocks `pool.g_layers` attend over the shared G-prompts and whose blocks `pool.e_layers` attend over one E-prompt per sample -- row
        `task_id` when `train` (with the key loss of prompt.py:286), else the row whose key is closest to the query (key loss 0).  Differentiable in
        train mode w.r.t. the G-prompts and row `task_id` of the E-prompts and keys.  `pool.last_cos` [E-layers, B, pool] and `pool.last_idx` keep the
        cosines and the selection of the last call."""
        if self.lora_rank or self.sd_lora or self.adapter_dim:
            raise NotImplementedError("DualPrompt runs on the plain frozen backbone")
        if train and (task_id is None or not 0 <= int(task_id) < pool.e_pool_size):
            raise ValueError(f"DualPrompt: training indexes the pool by task_id, got {task_id} for a pool of {pool.e_pool_size} (prompt.py:287)")
        params = pool.layer_tensors()
        need = bool(train) and torch.is_grad_enabled() and any(t.requires_grad for t in params)
        return _DualFn.apply(self, pool, images, need, bool(train), task_id, *params)

    # --------------------------------------------------------------------------------------- public forward
    def _gram_buffer(self, dev):
        """the resident [depth, D, D] fp32 sums of X^T X; layer i's LazyGram (if its attention module has one) owns row i"""
        s = self._s
        if s.gram is not None:                           # (holders re-created or detached since: a deep copy, a new attention module)
            g0 = self.attention_modules()[0].__dict__.get("_gram")
            if g0 is not None and (g0.dev is None or g0.dev.data_ptr() != s.gram[0].data_ptr()):
                s.gram = None
        if s.gram is None or s.gram.device != dev:
            for a in self.attention_modules():
                g = a.__dict__.get("_gram")
                if g is not None:
                    g.fold()
            s.gram = torch.zeros(self.depth, self.embed_dim, self.embed_dim, device=dev)
            for i, a in enumerate(self.attention_modules()):
                g = a.__dict__.get("_gram")
                if g is not None:
                    g.dev, g.n_dev = s.gram[i], 0
        return s.gram

    def features(self, images, prompt_tokens=None, get_input_matrix=False, gram_out=None):
        """[B, D] fp32: final-LN output at the cls token, or (with L2P prompt tokens [P, D]) the mean over the P prompt
        token outputs (transformer.py:2254-2261).  Differentiable w.r.t. prompt_tokens, the lora_B weights and the adapter tensors; the adapters'
        dropout is on while the module is in training mode (its seed of the last forward: `last_dropout_seed`).
        get_input_matrix: every layer's X^T X (X = the attention input) is ADDED to a device-resident [depth, D, D] fp32 buffer by one
        MFMA launch at the end of the forward -- the modules' own (`cur_matrix`, read lazily) or the caller's `gram_out`."""
        gram = None
        if get_input_matrix:
            gram = gram_out if gram_out is not None else self._gram_buffer(images.device)
        if self.sd_lora and self.sd_terms() > 0:
            if prompt_tokens is not None or get_input_matrix:
                raise NotImplementedError("SD-LoRA runs without prompt tokens and without the input Gram")
            params = self.sd_trainable()
            need = torch.is_grad_enabled() and any(t.requires_grad for t in params)
            return _VitFn.apply(self, images, None, None, need, ("sd",), *params)
        if self.lora_sub and any(a.apply_lora for a in self.attention_modules()):
            if prompt_tokens is not None or get_input_matrix:
                raise NotImplementedError("LoRA-Sub trains without prompt tokens, and its Gram pass runs on W - prev without the LoRA term")
            params = [w for a in self.attention_modules() for w in (a.lora_A_k.weight, a.lora_B_k.weight, a.lora_A_v.weight, a.lora_B_v.weight)]
            need = torch.is_grad_enabled() and any(t.requires_grad for t in params)
            return _VitFn.apply(self, images, None, None, need, ("ab",), *params)
        lora_b = []
        if self.lora_rank and any(a.apply_lora for a in self.attention_modules()):
            for a in self.attention_modules():
                lora_b += [a.lora_B_k.weight, a.lora_B_v.weight]
        adapters = self.adapter_tensors()
        if not (torch.is_grad_enabled() and any(t.requires_grad for t in adapters)):
            adapters = []                                    # frozen adapters still run in the forward; they just are no autograd inputs
        need = torch.is_grad_enabled() and ((prompt_tokens is not None and prompt_tokens.requires_grad) or any(b.requires_grad for b in lora_b)
                                            or bool(adapters))
        want = tuple(k for k, on in (("prompt", prompt_tokens is not None), ("lora_b", lora_b), ("adapter", adapters)) if on)
        feat = _VitFn.apply(self, images, prompt_tokens, gram, need, want, *lora_b, *adapters)
        if get_input_matrix and gram_out is None:
            # the running mean over tokens (transformer.py:241-244) is taken when `cur_matrix` is read; here only the token count moves
            cnt = images.shape[0] * (self.num_patches + 1 + (0 if prompt_tokens is None else prompt_tokens.shape[0]))
            for a in self.attention_modules():
                g = a.__dict__.get("_gram")
                if g is not None:
                    g.n_dev += cnt
        return feat

    def forward(self, x, prompt=None, prompt_flag="", cls_features=None, get_input_matrix=False, **kwargs):
        """the two branches of transformer.py:2222-2294 that the in-scope methods use"""
        if prompt_flag == "l2p":
            if prompt is None:
                return self.features(x)
            tokens, reduce_sim = prompt(None, cls_features=cls_features)
            return self.features(x, tokens), reduce_sim
        if prompt is not None:
            raise NotImplementedError("prefix prompting goes through coda_features / dual_features (ViTZoo.forward)")
        return self.features(x, None, get_input_matrix), None

    def debug_read(self, layer, which):
        s = self._s
        B, n_prompt = self._last
        N = n_prompt + 1 + self.num_patches
        M = B * N
        D = self.embed_dim
        # include/clhip.h, clhip_vit_read_act: 5 the LN1 output, 6 lse [B, H, N], 7 / 8 the LN1 / LN2 statistics [2, M], 9 the adapter's hidden rows
        shape = {0: (M, D), 1: (M, 3 * D), 2: (M, D), 3: (M, D), 4: (M, self.mlp_dim), 5: (M, D), 6: (B, self.num_heads, N), 7: (2, M), 8: (2, M),
                 9: (M, self.adapter_dim)}[which]
        out = torch.empty(*shape, device=s.ws.device)
        call("clhip_vit_read_act", s.handle, s.ws.data_ptr(), layer, which, out.data_ptr(), _st())
        return out

    def __del__(self):
        s = getattr(self, "_s", None)
        if s is not None and s.handle is not None:
            try:
                _lib.lib().clhip_vit_destroy(s.handle)
            except Exception:
                pass
            s.handle = None


class _L2PSelectFn(torch.autograd.Function):
    """prompt.L2P.forward (prompt.py:369-406) as one kernel: -> (prompt tokens [top_k*length, D], reduce_sim)"""

    @staticmethod
    def forward(ctx, prompt, key, cls_features, top_k):
        require_gpu(prompt)
        _, pool, length, D = prompt.shape
        q = cls_features.detach().float().contiguous()
        B = q.shape[0]
        dev = prompt.device
        ids = torch.empty(top_k, dtype=torch.int32, device=dev)
        tokens = torch.empty(top_k * length, D, device=dev)
        rs = torch.empty(1, device=dev)
        dkey = torch.empty(pool, D, device=dev)
        scratch = torch.empty(B + pool + D + B * pool, device=dev)
        call("clhip_l2p_select", q.data_ptr(), key.detach().contiguous().data_ptr(), prompt.detach().contiguous().data_ptr(), B, D, pool, top_k, length,
             ids.data_ptr(), tokens.data_ptr(), rs.data_ptr(), dkey.data_ptr(), scratch.data_ptr(), _st())
        ctx.save_for_backward(ids, dkey)
        ctx.dims = (pool, top_k, length, D)
        ctx.mark_non_differentiable(ids)
        return tokens, rs.view(()), ids

    @staticmethod
    def backward(ctx, dtokens, drs, _):
        ids, dkey = ctx.saved_tensors
        pool, top_k, length, D = ctx.dims
        dpool = None
        if dtokens is not None:
            dpool = torch.empty(1, pool, length, D, device=ids.device)
            call("clhip_l2p_scatter", dtokens.float().contiguous().data_ptr(), ids.data_ptr(), dpool.data_ptr(), pool, top_k, length, D, _st())
        gk = None
        if drs is not None:
            gk = torch.empty_like(dkey)
            call("clhip_scale_dev", dkey.data_ptr(), gk.data_ptr(), dkey.numel(), 1.0, drs.reshape(1).float().contiguous().data_ptr(), _st())
        return dpool, gk, None, None


class L2PPrompt(nn.Module):
    """prompt.L2P (prompt.py:345-406): prompt pool [num_layers=1, pool, length, D] and keys [pool, D]"""

    def __init__(self, length, prompt_init=nn.init.uniform_, prompt_key=False, pool_size=None, top_k=None, num_layers=1, embed_dim=768):
        super().__init__()
        assert num_layers == 1
        self.length, self.pool_size, self.top_k, self.num_layers, self.embed_dim = length, pool_size, top_k, num_layers, embed_dim
        self.prompt = nn.Parameter(torch.empty(num_layers, pool_size, length, embed_dim))
        self.prompt_key = nn.Parameter(torch.empty(pool_size, embed_dim))
        prompt_init(self.prompt)
        prompt_init(self.prompt_key)
        self.last_ids = None

    def forward(self, x_embed, cls_features=None):
        tokens, reduce_sim, ids = _L2PSelectFn.apply(self.prompt, self.prompt_key, cls_features, self.top_k)
        self.last_ids = ids
        return tokens, reduce_sim


class CodaPromptPool(nn.Module):
    """prompt.CodaPrompt (prompt.py:37-223): per prompted layer l in `e_layers` the components e_p_{l} [pool, length, D], their keys e_k_{l} and attention
    vectors e_a_{l} [pool, key_dim].  Construction makes the reference's draws from torch's CPU generator in its order (prompt.py:47-64: uniform_ for p, k, a,
    then gram_schmidt on p, k, a with one randn_like per column), so a seeded run starts from the reference's tensors bit for bit.  The module only owns the
    parameters: VisionTransformer.coda_features assembles the prefixes (csrc/coda.hip) and runs the blocks."""

    def __init__(self, emb_d, n_tasks, prompt_param, key_dim=768):
        super().__init__()
        self.task_count, self.emb_d, self.key_d, self.n_tasks = 0, emb_d, key_dim, n_tasks
        self.e_pool_size, self.e_p_length, self.ortho_mu = int(prompt_param[0]), int(prompt_param[1]), prompt_param[2]
        self.e_layers = [0, 1, 2, 3, 4]
        if key_dim != emb_d:
            raise NotImplementedError("the query is the backbone's cls feature: key_dim must equal the embedding width")
        if self.e_p_length % 2 or self.e_p_length < 2:
            raise NotImplementedError("prompt_length must be even: one half is the key prefix, the other the value prefix")
        for e in self.e_layers:
            p = nn.init.uniform_(torch.empty(self.e_pool_size, self.e_p_length, emb_d, dtype=torch.float32))
            k = nn.init.uniform_(torch.empty(self.e_pool_size, self.key_d, dtype=torch.float32))
            a = nn.init.uniform_(torch.empty(self.e_pool_size, self.key_d, dtype=torch.float32))
            setattr(self, f"e_p_{e}", self.gram_schmidt(p))
            setattr(self, f"e_k_{e}", self.gram_schmidt(k))
            setattr(self, f"e_a_{e}", self.gram_schmidt(a))

    def window(self):
        """(s, f): the components [0, f) are used, [s, f) train (prompt.py:169-186)"""
        pt = int(self.e_pool_size / self.n_tasks)
        return int(self.task_count * pt), int((self.task_count + 1) * pt)

    def layer_tensors(self):
        """K, A, P of every prompted layer, in layer order"""
        return [getattr(self, f"e_{w}_{e}") for e in self.e_layers for w in ("k", "a", "p")]

    @torch.no_grad()
    def process_task_count(self):
        """prompt.py:76-96: move the window on and re-draw its components.  Nothing in the reference calls it (see model/codaprompt.py)"""
        self.task_count += 1
        for e in self.e_layers:
            for w in ("k", "a", "p"):                                  # (the reference's order: k, a, p)
                old = getattr(self, f"e_{w}_{e}")
                setattr(self, f"e_{w}_{e}", nn.Parameter(self.gram_schmidt(old.detach().cpu()).to(old.device)))

    @torch.no_grad()
    def gram_schmidt(self, vv):
        """prompt.py:100-156: columns [s, f) of the (flattened, transposed) tensor become fresh Gaussian draws, each orthogonalised against ALL columns
        before it -- the columns beyond the window among them, which are still zero -- and normalised; columns below s are kept, columns at or beyond f are
        zero.  Same operations in the same order as the reference, so fp32 results agree bit for bit."""
        shape = vv.shape
        vv = vv.reshape(shape[0], -1).T
        uu = torch.zeros_like(vv)
        s, f = self.window()
        if s > 0:
            uu[:, :s] = vv[:, :s].clone()
        for k in range(s, f):
            redo = True
            while redo:
                redo = False
                vk = torch.randn_like(vv[:, k])
                uk = 0
                for j in range(k):
                    if redo:
                        continue
                    uj = uu[:, j].clone()
                    den = (uj * uj).sum()
                    if den < 1e-8:
                        redo = True                                      # a degenerate earlier column: draw again
                    else:
                        uk = uk + (vk * uj).sum() / den * uj
                if not redo:
                    uu[:, k] = vk - uk
        for k in range(s, f):
            uk = uu[:, k].clone()
            uu[:, k] = uk / uk.norm()
        return nn.Parameter(uu.T.reshape(shape).contiguous())


class DualPromptPool(nn.Module):
    """prompt.DualPrompt (prompt.py:231-337): the shared G-prompts g_p_{l} [Lg, D] of the blocks `g_layers` and, per block l in `e_layers`, a pool of E-prompts
    e_p_{l} [pool, Le, D] with their keys e_k_{l} [pool, key_dim].  prompt_param = [pool, Le, Lg] (prompt.py:262-264).  Construction makes the reference's
    draws from torch's CPU generator in its order (prompt.py:241-251: uniform_ for g_p_0, g_p_1, then per E-layer p, k), so a seeded run starts from the
    reference's tensors bit for bit.  Training indexes the pool by task id (`task_id_bootstrap`, prompt.py:255, is hard-coded True and the branch for False
    is not built).  The module only owns the parameters: VisionTransformer.dual_features selects the prefixes (csrc/dual.hip) and runs the blocks."""

    def __init__(self, emb_d, n_tasks, prompt_param, key_dim=768):
        super().__init__()
        self.task_count, self.emb_d, self.key_d, self.n_tasks = 0, emb_d, key_dim, n_tasks
        self.top_k, self.task_id_bootstrap = 1, True
        self.g_layers, self.e_layers = [0, 1], [2, 3, 4]
        self.e_pool_size, self.e_p_length, self.g_p_length = int(prompt_param[0]), int(prompt_param[1]), int(prompt_param[2])
        if key_dim != emb_d:
            raise NotImplementedError("the query is the backbone's cls feature: key_dim must equal the embedding width (prompt.py:281 contracts them)")
        for name, n in (("e_prompt_length", self.e_p_length), ("g_prompt_length", self.g_p_length)):
            if n % 2 or n < 2:
                raise NotImplementedError(f"{name} must be even: rows [:n/2] are the key prefix and rows [n/2:] the value prefix (prompt.py:300-302, "
                                          ":312-316), which the attention concatenates to keys and values of one length (transformer.py:175-180)")
        if n_tasks > self.e_pool_size:
            raise NotImplementedError(f"task_num {n_tasks} > pool size {self.e_pool_size}: training takes row task_id of the pool (prompt.py:287)")
        for g in self.g_layers:
            setattr(self, f"g_p_{g}", nn.Parameter(nn.init.uniform_(torch.empty(self.g_p_length, emb_d, dtype=torch.float32))))
        for e in self.e_layers:
            setattr(self, f"e_p_{e}", nn.Parameter(nn.init.uniform_(torch.empty(self.e_pool_size, self.e_p_length, emb_d, dtype=torch.float32))))
            setattr(self, f"e_k_{e}", nn.Parameter(nn.init.uniform_(torch.empty(self.e_pool_size, self.key_d, dtype=torch.float32))))
        self.last_cos = self.last_idx = None

    def process_task_count(self):
        self.task_count += 1

    def layer_tensors(self):
        """g_p of every G-layer, then e_k, e_p of every E-layer, in layer order"""
        return [getattr(self, f"g_p_{g}") for g in self.g_layers] + [getattr(self, f"e_{w}_{e}") for e in self.e_layers for w in ("k", "p")]


class ViTZoo(nn.Module):
    """core/model/backbone/vit.py:43-139.  Extra kwargs (img_size, patch_size, embed_dim, depth, num_heads, dtype) size
    the model for tests; the defaults are the reference's hard-coded ViT-B/16."""

    def __init__(self, pretrained=False, model_name="vit_base_patch16_224", attn_layer="MultiHeadAttention", checkpoint=None, img_size=224,
                 patch_size=16, embed_dim=768, depth=12, num_heads=12, dtype="bf16", **kwargs):
        super().__init__()
        kwargs.pop("num_classes", None)
        kwargs.pop("device", None)
        self.task_id = None
        self.feat_dim = embed_dim
        self.feat = VisionTransformer(img_size=img_size, patch_size=patch_size, embed_dim=embed_dim, depth=depth, num_heads=num_heads,
                                      attn_layer=attn_layer, dtype=dtype, **kwargs)
        if pretrained:
            self.load_pretrained(model_name, checkpoint)
        self.prompt = None
        self.prompt_flag = ""

    def load_pretrained(self, model_name, checkpoint=None):
        """timm state dict -> reference key names (vit.py:69-84).  There is no network here: the checkpoint must be a
        local file (`checkpoint` kwarg, $CLHIP_VIT_CHECKPOINT, or torch hub's cache directory)."""
        cands = [checkpoint, os.environ.get("CLHIP_VIT_CHECKPOINT"),
                 os.path.expanduser(f"~/.cache/torch/hub/checkpoints/{model_name}.pt"),
                 os.path.expanduser(f"~/.cache/torch/hub/checkpoints/{model_name}.pth")]
        path = next((c for c in cands if c and os.path.exists(c)), None)
        if path is None:
            raise FileNotFoundError(f"pretrained ViT weights for {model_name} not found (looked in {[c for c in cands if c]}); "
                                    "pass backbone.kwargs.checkpoint or set pretrained: false")
        sd = torch.load(path, map_location="cpu")
        sd = sd.get("state_dict", sd.get("model", sd)) if isinstance(sd, dict) else sd
        out = {}
        for k, v in sd.items():
            for old, new in ((".norm1.", ".ln_1."), (".norm2.", ".ln_2."), ("blocks.", "transformer.blocks.")):
                if old in k:
                    k = k.replace(old, new)
            out[k] = v
        own = self.feat.state_dict()
        self.feat.load_state_dict({k: v for k, v in out.items() if k in own and tuple(v.shape) == tuple(own[k].shape)}, strict=False)

    def create_prompt(self, prompt_flag, **kwargs):
        if prompt_flag == "l2p":
            self.prompt = L2PPrompt(**kwargs)
        elif prompt_flag == "coda":
            kwargs.setdefault("key_dim", self.feat_dim)                    # (vit.py:97 hard-codes 768 for both; here the backbone's width)
            self.prompt = CodaPromptPool(self.feat_dim, **kwargs)
        elif prompt_flag == "dual":
            kwargs.setdefault("key_dim", self.feat_dim)                    # (vit.py:95 likewise)
            self.prompt = DualPromptPool(self.feat_dim, **kwargs)
        else:
            raise NotImplementedError("only the L2P, DualPrompt and CODA-Prompt pools are on the hot path (SURVEY.md section 8)")
        self.prompt_flag = prompt_flag

    def forward(self, image, text=None, pen=False, train=False, **kwargs):
        if self.prompt_flag == "l2p":
            with torch.no_grad():
                cls_features = self.feat(image, prompt_flag="l2p")
            return self.feat(image, prompt=self.prompt, cls_features=cls_features, prompt_flag="l2p")
        if self.prompt_flag == "coda":
            # vit.py:120-138: query pass without gradient, prompted pass, the cls feature; the prompt loss is the orthogonality penalty, 0 at mu = 0
            out = self.feat.coda_features(image, self.prompt, train=train)
            return (out, torch.zeros(1, device=out.device)) if train else out
        if self.prompt_flag == "dual":
            # the same lines with a DualPrompt pool: the prompt loss is the key loss of the three E-layers, shape (1,) (transformer.py:2272-2279)
            out, prompt_loss = self.feat.dual_features(image, self.prompt, train=train, task_id=self.task_id)
            return (out, prompt_loss) if train else out
        if self.prompt is not None:
            raise NotImplementedError
        out, _ = self.feat(image, **kwargs)
        return out.view(out.size(0), -1)


def vit_pt_imnet(pretrained=False, **kwargs):
    return ViTZoo(pretrained, **kwargs)


def vit_pt_imnet_in21k_adapter(pretrained=False, **kwargs):
    """the backbone name of the reference's RanPAC config (config/ranpac.yaml:48-52; core/model/backbone/vit.py ViT_in21k_adapter).  Its AdaptFormer
    adapters start as the identity (`up_proj` is zero-initialised, petl/adapter.py:45-50) and only first-session training moves them, so without
    the kwarg `ffn_adapt: true` this is the plain frozen ViT-B/16 with the ImageNet-21k weights.  With it (and `ffn_num`, `ffn_adapter_scalar`,
    `adapter_dropout`, the names of the reference's tuning config, core/model/backbone/vit.py:152-167) every block gets
    `adaptmlp.{down_proj, up_proj}`, the block LayerNorms use eps 1e-6 and only the adapters require grad: what RanPAC's
    `first_session_training: true` trains (csrc/adapter.hip inside the executor)."""
    kwargs.setdefault("model_name", "vit_base_patch16_224_in21k")
    return ViTZoo(pretrained, **kwargs)
