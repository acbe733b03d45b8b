"""csrc/clip.hip (clhip_clip_logits_fwd / _bwd) against fp64 with the per-element bounds of tests/clip_ref.py; below that the executor's CLIP mode
(clhip_vit_set_clip) launch by launch from its own stored tensors, its lora_B gradients end to end, the mode switched off again, and its refusals.
Outputs are written, not accumulated (NaN pre-fill), and a second call gives the same bits.  Every check prints `[ratio] name: max |err| / bound`."""
import ctypes as C

import pytest
import torch

import clip_ref as R

pytestmark = pytest.mark.gpu

from libcontinual_amd import _lib, ops           # noqa: E402

DEV = "cuda"
SHAPES = [(1, 64, 32, 1), (5, 64, 32, 3), (9, 128, 64, 20), (33, 768, 512, 100)]
SCALES = [1 / 0.07, 100.0]


def st():
    return torch.cuda.current_stream().cuda_stream


def rnd(shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV) * scale


def nanfill(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def judge(name, got, ref, allowed):
    err = (got.double() - ref).abs()
    ratio = float(torch.nan_to_num(err / allowed.clamp(min=1e-300), nan=float("inf")).max())
    print(f"[ratio] {name}: {ratio:.3g}")
    assert bool((err <= allowed).all()), f"{name}: max |err| / bound = {ratio:.3g}"


def inputs(B, D, E, Cn):
    feat = rnd((B, D), 1)
    proj = rnd((D, E), 2, D ** -0.5)
    txt = torch.nn.functional.normalize(rnd((Cn, E), 3).double(), dim=1).float()
    return feat, proj, txt


def fwd(feat, proj, txt, scale):
    (B, D), E, Cn = feat.shape, proj.shape[1], txt.shape[0]
    out, u, inv = nanfill(B, Cn), nanfill(B, E), nanfill(B)
    _lib.call("clhip_clip_logits_fwd", feat.data_ptr(), proj.data_ptr(), txt.data_ptr(), scale, out.data_ptr(), u.data_ptr(), inv.data_ptr(), B, D, E, Cn, st())
    return out, u, inv


def bwd(dl, proj, txt, scale, u, inv):
    (D, E), (B, Cn) = proj.shape, dl.shape
    df = nanfill(B, D)
    _lib.call("clhip_clip_logits_bwd", dl.data_ptr(), proj.data_ptr(), txt.data_ptr(), scale, u.data_ptr(), inv.data_ptr(), df.data_ptr(), B, D, E, Cn, st())
    return df


@pytest.mark.parametrize("scale", SCALES, ids=["s14.3", "s100"])
@pytest.mark.parametrize("B,D,E,Cn", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_logits_pair_against_fp64(B, D, E, Cn, scale):
    feat, proj, txt = inputs(B, D, E, Cn)
    out, u, inv = fwd(feat, proj, txt, scale)
    lref, uref, iref = R.logits_ref(feat, proj, txt, scale)
    bu, bi = R.saved_bound(feat, proj)
    name = f"{B}x{D}x{E}x{Cn} scale {scale:.3g}"
    judge(name + " logits", out, lref, R.logits_bound(feat, proj, txt, scale))
    judge(name + " u", u, uref, bu)
    judge(name + " 1/|u|", inv, iref, bi)
    dl = rnd((B, Cn), 4, 1.0 / B)
    df = bwd(dl, proj, txt, scale, u, inv)
    judge(name + " dfeat", df, R.dfeat_ref(dl, proj, txt, scale, uref, iref), R.dfeat_bound(dl, feat, proj, txt, scale))
    out2, u2, inv2 = fwd(feat, proj, txt, scale)
    df2 = bwd(dl, proj, txt, scale, u2, inv2)
    torch.cuda.synchronize()
    for a, b in ((out, out2), (u, u2), (inv, inv2), (df, df2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name + ": a second call gave other bits"


def test_one_class_gives_a_zero_gradient_downstream():
    """C = 1: softmax of one logit is 1, the CE gradient is exactly 0 and so is everything behind it"""
    feat, proj, txt = inputs(5, 64, 32, 1)
    feat.requires_grad_(True)
    logits = ops.clip_logits(feat, proj, txt, 1 / 0.07)
    loss = ops.classify_loss(logits, torch.zeros(5, dtype=torch.int64, device=DEV))
    loss.backward()
    assert float(loss) == 0.0
    assert bool((feat.grad == 0).all())


def test_an_exact_tie_goes_to_the_lower_index():
    """two identical text rows give identical logits bit for bit; ops.predict takes the lower index"""
    feat, proj, txt = inputs(9, 128, 64, 20)
    txt[7] = txt[3]
    txt = txt.contiguous()
    out, _, _ = fwd(feat, proj, txt, 100.0)
    assert torch.equal(out[:, 3].view(torch.int32), out[:, 7].view(torch.int32))
    out[:, 3] = out[:, 7] = out.max() + 1.0
    pred, _ = ops.predict(out, torch.zeros(9, dtype=torch.int64, device=DEV))
    assert bool((pred == 3).all())


def test_autograd_wrapper_matches_the_kernels():
    feat, proj, txt = inputs(9, 128, 64, 20)
    f = feat.clone().requires_grad_(True)
    logits = ops.clip_logits(f, proj, txt, 100.0)
    dl = rnd((9, 20), 4)
    logits.backward(dl)
    out, u, inv = fwd(feat, proj, txt, 100.0)
    assert torch.equal(logits.detach(), out) and torch.equal(f.grad, bwd(dl, proj, txt, 100.0, u, inv))


@pytest.mark.parametrize("what,kw", [("B = 0", dict(B=0)), ("D + E > 4096", dict(D=4096, E=64)), ("E + C > 4096", dict(E=64, Cn=4096)), ("NULL txt", dict(txt=None))])
def test_rejected_arguments_launch_nothing(what, kw):
    a = dict(B=2, D=64, E=32, Cn=3, txt=1)
    a.update(kw)
    big = torch.zeros(1 << 16, device=DEV)
    out, u, inv = nanfill(8, 8), nanfill(8, 64), nanfill(8)
    L = _lib.lib()
    rc = L.clhip_clip_logits_fwd(big.data_ptr(), big.data_ptr(), big.data_ptr() if a["txt"] else None, 1.0, out.data_ptr(), u.data_ptr(), inv.data_ptr(), a["B"], a["D"],
                                 a["E"], a["Cn"], st())
    rc2 = L.clhip_clip_logits_bwd(big.data_ptr(), big.data_ptr(), big.data_ptr() if a["txt"] else None, 1.0, u.data_ptr(), inv.data_ptr(), out.data_ptr(), a["B"], a["D"],
                                  a["E"], a["Cn"], st())
    torch.cuda.synchronize()
    assert rc == -1 and rc2 == -1, what
    assert bool(out.isnan().all()) and bool(u.isnan().all()) and bool(inv.isnan().all())


# ------------------------------------------------------------------------------------------------ the executor in CLIP mode, launch by launch
# What the mode adds is judged from the EXECUTOR'S OWN stored inputs of each launch (clhip_vit_read_act, the gradient tap), at the numbers the suite
# already holds each op to (vit_refs.LN, vit_refs.LN_POOL_FEAT, gemm_ref's bound, clip_ref.qgelu_bound): ln_pre behind the bias-free patch product,
# fc1 under epilogue 6 (its derivative, and its value through fc2), the pooled ln_post and its backward at the mode's eps.  The launches the mode does
# not touch are held by tests/test_vit_plan_units_gpu.py; the whole chain is held end to end by the lora_B gradients against fp64 autograd.
import math                                         # noqa: E402

import gemm_ref as G                                # noqa: E402
import vit_refs as VR                               # noqa: E402
import libcontinual_amd.model as M                  # noqa: E402
from libcontinual_amd.model.backbone.vit import VisionTransformer           # noqa: E402

GEOS = {"fixture": dict(width=64, depth=3), "w128": dict(width=128, depth=3)}


def _seeded_weights(bb, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in bb.named_parameters():
            if n == "logit_scale":
                continue
            if n.endswith("bias"):
                p.copy_(torch.empty_like(p).uniform_(-0.05, 0.05, generator=g))
            elif ".ln_" in n or "ln_p" in n or "ln_final" in n:
                p.copy_(torch.empty_like(p).uniform_(0.8, 1.2, generator=g))
            elif p.dim() >= 2 and "embedding" not in n and n not in ("visual.proj", "text_projection"):
                s = 1.7 / math.sqrt(p[0].numel())
                p.copy_(torch.empty_like(p).uniform_(-s, s, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
            p.copy_(p.bfloat16().float())


def _visual(geo, dt, golden):
    if geo == "fixture":
        fix = golden("clip_tiny")
        vocab = fix["w/token_embedding.weight"].shape[0]
    else:
        fix, vocab = None, 16
    c = R.CFG
    bb = M.clip("ViT-B/16", None, embed_dim=c["embed"], image_resolution=c["img"], vision_layers=GEOS[geo]["depth"], vision_width=GEOS[geo]["width"],
                vision_patch_size=c["patch"], context_length=c["ctx"], vocab_size=vocab, transformer_width=64, transformer_heads=1, transformer_layers=1 if fix is None else c["tlayers"],
                attn_layer="MultiHeadAttention_LoRA", lora_rank=R.RANK, dtype=dt)
    if fix is not None:
        bb.load_state_dict(R.fixture_weights(fix, torch.float32), strict=True)
    else:
        _seeded_weights(bb, 11)
    vt = bb.visual.to(DEV)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for a in vt.attention_modules():                 # a live LoRA term: A and B both non-zero
            a.init_param()
            for n in ("lora_A_k", "lora_A_v", "lora_B_k", "lora_B_v"):
                getattr(a, n).weight.copy_((torch.randn(getattr(a, n).weight.shape, generator=g) * 0.1).to(DEV))
    for p in vt.parameters():
        p.requires_grad_(False)
    for a in vt.attention_modules():
        a.lora_B_k.weight.requires_grad_(True); a.lora_B_v.weight.requires_grad_(True)
    return vt


def _w64(vt, dt):
    """the visual tower's weights as the executor holds them: the compute-dtype copies of the GEMM operands (bf16-rounded effective weights), fp32 masters else"""
    w = {"visual." + k: v.detach().cpu().double() for k, v in vt.state_dict().items()}
    return w


def _rb(t, dt):
    return t.to(torch.bfloat16).double() if dt == "bf16" else t.float().double()


def _judge(name, got, ref, allowed):
    err = (got.double().cpu() - ref).abs()
    ratio = float(torch.nan_to_num(err / allowed.clamp(min=1e-300), nan=float("inf")).max())
    print(f"[ratio] {name}: {ratio:.3g}")
    assert bool((err <= allowed).all()), f"{name}: max |err| / bound = {ratio:.3g}"


@pytest.mark.parametrize("B", [1, 3, 9])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("geo", list(GEOS))
def test_executor_clip_mode_launch_by_launch(geo, dt, B, golden):
    vt = _visual(geo, dt, golden)
    D, depth, N = vt.embed_dim, vt.depth, vt.num_patches + 1
    x = rnd((B, 3, 32, 32), 21).abs().clamp(max=1.0)
    feat = vt.features(x)
    s = vt._s
    L = _lib.lib()
    tap = nanfill(L.clhip_vit_tap_floats(s.handle))
    _lib.call("clhip_vit_set_tap", s.handle, tap.data_ptr(), tap.numel())
    dfeat = rnd((B, D), 22)
    try:
        feat.backward(dfeat)
    finally:
        _lib.call("clhip_vit_set_tap", s.handle, None, 0)
    torch.cuda.synchronize()
    w = _w64(vt, dt)
    name = f"{geo} {dt} B{B}"
    rel_ln = VR.LN[dt]
    eps_out = G.OUT_EPS[dt]
    # ---- ln_pre: x_in[0] from the images (patchify -> bias-free product -> assembly, both in the compute dtype, -> LayerNorm at 1e-5)
    p = vt.patch_size
    gsz = 32 // p
    patches = _rb(x.cpu().reshape(B, 3, gsz, p, gsz, p).permute(0, 2, 4, 1, 3, 5).reshape(B * gsz * gsz, 3 * p * p), dt)
    Wp = _rb(w["visual.conv1.weight"].reshape(D, -1), dt)
    pe = patches @ Wp.T
    e_pe = (Wp.shape[1] + 8) * G.U24 * (patches.abs() @ Wp.abs().T) + eps_out * pe.abs()
    tok = torch.cat([w["visual.class_embedding"].expand(B, 1, D), pe.view(B, N - 1, D)], 1) + w["visual.positional_embedding"]
    e_tok = torch.cat([torch.zeros(B, 1, D, dtype=torch.float64), e_pe.view(B, N - 1, D)], 1) + 2 * eps_out * tok.abs()
    ref0, _, rstd0, _ = VR.ln_ref(tok, w["visual.ln_pre.weight"], w["visual.ln_pre.bias"], torch.zeros_like(tok), 1e-5)
    carried = float(w["visual.ln_pre.weight"].abs().max()) * rstd0.unsqueeze(-1) * math.sqrt(D) * e_tok.amax(-1, keepdim=True)
    _judge(name + " ln_pre -> x_in[0]", vt.debug_read(0, 0).view(B, N, D), ref0, rel_ln * ref0.abs().max() + carried)
    for l, blk in enumerate(vt.transformer.blocks):
        pre = f"visual.transformer.blocks.{l}."
        xm = vt.debug_read(l, 3).double().cpu()                                   # the stored x_mid: the input of LN2 -> fc1 (epilogue 6) -> fc2
        h2, _, _, _ = VR.ln_ref(xm, w[pre + "ln_2.weight"], w[pre + "ln_2.bias"], torch.zeros_like(xm), 1e-5)
        e_h2 = rel_ln * h2.abs().max()                                           # the LN2 output is scratch: its bound is carried
        h2s = _rb(h2, dt)
        W1, W2 = _rb(w[pre + "mlp.fc1.weight"], dt), _rb(w[pre + "mlp.fc2.weight"], dt)
        pre1, cref, href = R.qgelu_ref(h2s, W1, w[pre + "mlp.fc1.bias"])
        S1 = h2s.abs() @ W1.abs().T
        bc, bh = R.qgelu_bound(S1, D, pre1, cref, href, dt)
        carry1 = float(e_h2) * W1.abs().sum(1)[None, :]
        _judge(f"{name} layer {l} fc1 epilogue 6 H", vt.debug_read(l, 4), href, bh + R.QGELU_D2_MAX * carry1)
        act = _rb(cref, dt)
        out = xm + act @ W2.T + w[pre + "mlp.fc2.bias"]
        e_act = bc + R.QGELU_D1_MAX * carry1
        b2 = (W2.shape[1] + 8) * G.U24 * (act.abs() @ W2.abs().T + xm.abs()) + eps_out * out.abs() + e_act @ W2.abs().T
        _judge(f"{name} layer {l} fc2 on QuickGELU -> x_in[{l + 1}]", vt.debug_read(l + 1, 0), out, b2)
    # ---- the pooled ln_post and its backward at eps 1e-5, from the stored last-block output
    xl = vt.debug_read(depth, 0).double().cpu()
    fref, gref = VR.ln_pool_ref(xl, w["visual.ln_post.weight"], w["visual.ln_post.bias"], dfeat.cpu(), B, N, D, 1, 1e-5)
    _judge(name + " ln_post feat", feat.detach(), fref, VR.LN_POOL_FEAT * fref.abs().max() + torch.zeros_like(fref))
    g0 = tap[: B * N * D].view(B, N, D)
    _judge(name + " ln_post backward g", g0, gref, rel_ln * gref.abs().max() + torch.zeros_like(gref))


@pytest.mark.parametrize("geo", list(GEOS))
def test_lora_b_gradients_end_to_end_f32(geo, golden):
    """the whole CLIP-mode chain (QuickGELU derivative in the backward, ln_post at 1e-5, no ln_pre backward needed): every lora_B gradient against fp64
    autograd through tests/clip_ref.py, at the project's 5e-3 of max-abs"""
    vt = _visual(geo, "f32", golden)
    B = 5
    x = rnd((B, 3, 32, 32), 31).abs().clamp(max=1.0)
    dfeat = rnd((B, vt.embed_dim), 32)
    vt.features(x).backward(dfeat)
    w = _w64(vt, "f32")
    lora = []
    for a in vt.attention_modules():
        lora.append(tuple(getattr(a, n).weight.detach().cpu().double().requires_grad_(n.startswith("lora_B")) for n in ("lora_A_k", "lora_B_k", "lora_A_v", "lora_B_v")))
    (R.visual_forward(w, x.cpu().double(), lora) * dfeat.cpu().double()).sum().backward()
    for l, a in enumerate(vt.attention_modules()):
        for got, want in ((a.lora_B_k.weight.grad, lora[l][1].grad), (a.lora_B_v.weight.grad, lora[l][3].grad)):
            d = float((got.cpu().double() - want).abs().max() / want.abs().max())
            print(f"[ratio] {geo} layer {l} d lora_B: {d / 5e-3:.3g}")
            assert d < 5e-3 and float(want.abs().max()) > 0


def _raw_forward(vt, x, n_prompt=0, prompt=None):
    """clhip_vit_forward on the module's own handle and tables -> (rc, feat pre-filled with NaN)"""
    s = vt._ensure(x.device)
    ws = torch.empty(_lib.lib().clhip_vit_workspace_bytes(s.handle, x.shape[0], n_prompt, 0), dtype=torch.uint8, device=DEV)
    feat = nanfill(x.shape[0], vt.embed_dim)
    rc = _lib.lib().clhip_vit_forward(s.handle, C.byref(s.cparams), s.shadow.data_ptr(), ws.data_ptr(), x.data_ptr(), x.shape[0], prompt.data_ptr() if prompt is not None else None,
                                      n_prompt, 0, None, feat.data_ptr(), st())
    torch.cuda.synchronize()
    return rc, feat


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_final_eps_is_the_callers_and_off_restores_the_plain_executor(dt):
    """a plain ViT executor (patch bias, GELU, 1e-6): its features; the same handle in CLIP mode with ln_pre weights of the test's own and final_eps 1e-2 follows
    the fp64 ln_post at 1e-2 from the stored last-block output; switched off again it gives the first bits back"""
    torch.manual_seed(3)
    vt = VisionTransformer(img_size=32, patch_size=8, embed_dim=64, depth=2, num_heads=1, dtype=dt).to(DEV)
    x = rnd((3, 3, 32, 32), 41).abs().clamp(max=1.0)
    rc, f0 = _raw_forward(vt, x)
    assert rc == 0 and bool(f0.isfinite().all())
    lw, lb = torch.full((64,), 1.1, device=DEV), torch.full((64,), 0.05, device=DEV)
    h = vt._s.handle
    _lib.call("clhip_vit_set_clip", h, lw.data_ptr(), lb.data_ptr(), 1e-2, 1)
    with torch.no_grad():
        f1 = vt.features(x.clone().requires_grad_(False))
    s = vt._s
    ws = torch.empty(_lib.lib().clhip_vit_workspace_bytes(h, 3, 0, 1), dtype=torch.uint8, device=DEV)
    feat = nanfill(3, 64)
    _lib.call("clhip_vit_forward", h, C.byref(s.cparams), s.shadow.data_ptr(), ws.data_ptr(), x.data_ptr(), 3, None, 0, 1, None, feat.data_ptr(), st())
    xl = nanfill(3 * 17, 64)
    _lib.call("clhip_vit_read_act", h, ws.data_ptr(), 2, 0, xl.data_ptr(), st())
    torch.cuda.synchronize()
    assert torch.equal(feat, f1) and not torch.equal(f1, f0)
    fref, _ = VR.ln_pool_ref(xl.cpu(), vt.norm.weight.detach().cpu(), vt.norm.bias.detach().cpu(), torch.zeros(3, 64), 3, 17, 64, 1, 1e-2)
    fwrong, _ = VR.ln_pool_ref(xl.cpu(), vt.norm.weight.detach().cpu(), vt.norm.bias.detach().cpu(), torch.zeros(3, 64), 3, 17, 64, 1, 1e-5)
    tol = VR.LN_POOL_FEAT * float(fref.abs().max())
    assert float((feat.cpu().double() - fref).abs().max()) <= tol < float((fwrong - fref).abs().max()) / 10
    _lib.call("clhip_vit_set_clip", h, None, None, 0.0, 0)
    rc, f2 = _raw_forward(vt, x)
    assert rc == 0 and torch.equal(f2.view(torch.int32), f0.view(torch.int32))


def test_refused_combinations_launch_nothing(golden):
    L = _lib.lib()
    vt = _visual("fixture", "f32", golden)
    x = rnd((2, 3, 32, 32), 51).abs().clamp(max=1.0)
    rc, feat = _raw_forward(vt, x)
    assert rc == 0 and bool(feat.isfinite().all())
    # prompt tokens
    rc, feat = _raw_forward(vt, x, 2, rnd((2, vt.embed_dim), 52))
    assert rc == -1 and bool(feat.isnan().all()), L.clhip_last_error()
    # prefix mode set after the CLIP mode: the forward refuses
    h = vt._s.handle
    pk = rnd((2, 3, vt.embed_dim), 53)
    lp = (C.c_int * vt.depth)(*([3] + [0] * (vt.depth - 1)))
    ptr = (C.c_void_p * vt.depth)(*([pk.data_ptr()] + [None] * (vt.depth - 1)))
    assert L.clhip_vit_set_prefix(h, lp, ptr, ptr) == 0
    rc, feat = _raw_forward(vt, x)
    assert rc == -1 and bool(feat.isnan().all())
    assert L.clhip_vit_set_prefix(h, None, None, None) == 0
    # ... and set_clip refuses an executor that is in prefix mode, has adapters, or runs SD-LoRA
    lw = torch.ones(64, device=DEV)
    plain = VisionTransformer(img_size=32, patch_size=8, embed_dim=64, depth=2, num_heads=1, dtype="f32").to(DEV)
    hp = plain._ensure(torch.device(DEV, torch.cuda.current_device())).handle
    lp2, ptr2 = (C.c_int * 2)(3, 0), (C.c_void_p * 2)(pk.data_ptr(), None)
    assert L.clhip_vit_set_prefix(hp, lp2, ptr2, ptr2) == 0
    assert L.clhip_vit_set_clip(hp, lw.data_ptr(), lw.data_ptr(), 1e-5, 1) == -1
    assert L.clhip_vit_set_prefix(hp, None, None, None) == 0
    assert L.clhip_vit_set_clip(hp, lw.data_ptr(), None, 1e-5, 1) == -1                      # ln_pre weight without bias
    assert L.clhip_vit_set_clip(hp, lw.data_ptr(), lw.data_ptr(), 0.0, 1) == -1              # no eps
    ad = VisionTransformer(img_size=32, patch_size=8, embed_dim=64, depth=2, num_heads=1, dtype="f32", ffn_adapt=True, ffn_num=16).to(DEV)
    ha = ad._ensure(torch.device(DEV, torch.cuda.current_device())).handle
    assert L.clhip_vit_set_clip(ha, lw.data_ptr(), lw.data_ptr(), 1e-5, 1) == -1
    # SD-LoRA (the pointers are only stored; the executor has no descriptor LoRA, as clhip_vit_set_sdlora asks): set_clip refuses it ...
    assert plain.lora_rank == 0
    dummy, ranks = torch.zeros(64, device=DEV), (C.c_int * 2)(4, 4)
    assert L.clhip_vit_set_sdlora(hp, 2, ranks, dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr()) == 0
    assert L.clhip_vit_set_clip(hp, lw.data_ptr(), lw.data_ptr(), 1e-5, 1) == -1
    assert L.clhip_vit_set_sdlora(hp, 0, None, None, None, None) == 0
    # ... and set after the CLIP mode, the forward refuses and writes nothing; with it off again the CLIP-mode forward runs
    assert L.clhip_vit_set_clip(hp, lw.data_ptr(), lw.data_ptr(), 1e-5, 1) == 0
    assert L.clhip_vit_set_sdlora(hp, 2, ranks, dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr()) == 0
    rc, feat = _raw_forward(plain, x)
    assert rc == -1 and bool(feat.isnan().all()), L.clhip_last_error()
    assert L.clhip_vit_set_sdlora(hp, 0, None, None, None, None) == 0
    rc, feat = _raw_forward(plain, x)
    assert rc == 0 and bool(feat.isfinite().all())
    assert L.clhip_vit_set_clip(hp, None, None, 0.0, 0) == 0
    # a NULL patch bias outside the mode is refused too
    s = plain._s
    saved = s.cparams.pe_b
    s.cparams.pe_b = None
    try:
        rc, feat = _raw_forward(plain, x)
    finally:
        s.cparams.pe_b = saved
    assert rc == -1 and bool(feat.isnan().all())
