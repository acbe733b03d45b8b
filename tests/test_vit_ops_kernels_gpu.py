"""Every entry point of csrc/attn.hip and csrc/vit_ops.hip through the C ABI against the fp64 references of tests/vit_refs.py, at every
dispatch path and edge.  Inputs are fp32 (or bf16-rounded values in the bf16 mode), the references see exactly those values, outputs are
pre-filled with NaN and carry a guard row that must come back bit-unchanged, every check prints `[ratio] name: max error / bound`, and
attention is judged per (batch, head) block, LayerNorm per row.

Bounds: the numbers tests/test_vit_kernels_gpu.py already holds each op to (vit_refs: ATTN_OUT, ATTN_GRAD, LN, ...), relative to the
block's max|ref|, plus 1e-7 of the tensor's max|ref|.  Widened only where the arithmetic says so:
  * attention, every case: where larger, the conditioning of the exponent -- a rounding error of the fp32 logit, hd 2^-24 scale
    sum_i|q_i k_i| of the row (from the fp64 reference), is a relative error of P and so of out, dq, dk, dv.  It only matters in the
    shifted-logit cases (up to 2e-3 there).
  * attention dq / dk, every case: where larger, vit_refs.attn_cancel_bound.  With one token dS = P (dP - rowsum(dO O)) is exactly zero in
    the reference and a difference of two hd-term fp32 sums in the kernel; with identical keys dq = scale sum_j dS_j k_j with
    sum_j dS_j = 0.  A relative bound on a reference that is zero admits nothing, so these take the forward bound of the cancelling
    terms (hd 2^-24 sum|term| each, O and dS as stored: 2^-9 where they are bf16).
  * LayerNorm, the offset case (x = 100 + 0.5 randn) only: y and dx admit, in addition, what the bound of the mean itself lets through:
    (x - mean) rstd moves by rstd times the mean's error.
  * sums longer than four times the old case (gram M = 2500 is the old case; none here is longer) would use head_refs.sum_bound.
lse, LN mean and LN rstd have no project number: vit_refs.LSE_ABS / LN_MEAN_REL / LN_RSTD_REL are four times the largest error
measured on the MI355X over all cases of this file, never below the order-independent forward bound (lse_floor / mean_floor /
rstd_floor).  Measured maxima (printed by every run as `[measure]`): see vit_refs."""
import ctypes as C
import math

import pytest
import torch

import vit_refs as V
from vit_refs import U, err_ratio, larger

pytestmark = pytest.mark.gpu

from libcontinual_amd import _lib           # noqa: E402
from libcontinual_amd._lib import call      # noqa: E402

DEV = "cuda"
TD = {"bf16": torch.bfloat16, "f32": torch.float32}
CODE = {"bf16": _lib.BF16, "f32": _lib.F32}
GUARD = 7.0


def st():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return t.data_ptr() if t is not None else None


def dev(t, dt="f32"):
    return t.to(DEV).to(TD[dt]).contiguous()


def nan_out(rows, cols, dt, guard=1):
    """rows NaN-filled output rows and `guard` rows of 7.0 behind them"""
    t = torch.full((rows + guard, cols), float("nan"), device=DEV, dtype=TD[dt])
    t[rows:] = GUARD
    return t


def guard_ok(t, rows):
    return bool((t[rows:].float() == GUARD).all())


def check(name, got, ref, allowed):
    r = err_ratio(got, ref, allowed)
    print(f"[ratio] {name}: {r:.3g}")
    assert r <= 1.0, (name, r)
    return r


def measure(name, got, ref, scale=None):
    e = (V.f64(got).reshape(ref.shape) - ref).abs()
    if scale is not None:
        e = e / scale
    print(f"[measure] {name}: {float(e.max()):.4g}")


def blocked(name, got, ref, rel, extra=None):
    """got / ref [B,H,...]: every (batch, head) block to rel * its own max|ref| + 1e-7 max|ref| of the tensor (+ extra, elementwise)"""
    worst = 0.0
    top = float(ref.abs().max())
    for b in range(ref.shape[0]):
        for h in range(ref.shape[1]):
            allowed = torch.full_like(ref[b, h], rel * float(ref[b, h].abs().max()) + V.FLOOR * top)
            if extra is not None:
                allowed = larger(allowed, extra[b, h])
            worst = max(worst, err_ratio(got[b, h], ref[b, h], allowed))
    print(f"[ratio] {name}: {worst:.3g}")
    assert worst <= 1.0, (name, worst)


# -------------------------------------------------------------------------------------------------------- attention
def run_attention(qkv, dout, B, N, H, hd, dt, tag):
    """forward (with and without lse), backward, zero-dout backward; every output against the fp64 reference per (batch, head)"""
    D = H * hd
    ref_o, ref_lse, ref_dq, ref_dk, ref_dv = V.attn_ref(qkv, dout, B, N, H, hd)
    dq_, do_ = dev(qkv, dt), dev(dout, dt)
    out, out2 = nan_out(B * N, D, dt), nan_out(B * N, D, dt)
    lse = torch.full((B * H * N + 8,), float("nan"), device=DEV)
    lse[B * H * N:] = GUARD
    dqkv = nan_out(B * N, 3 * D, dt)
    dsum = torch.empty(B * H * N, device=DEV)
    call("clhip_attn_fwd", p(dq_), p(out), p(lse), B, N, H, D, CODE[dt], st())
    call("clhip_attn_fwd", p(dq_), p(out2), None, B, N, H, D, CODE[dt], st())
    call("clhip_attn_bwd", p(dq_), p(out), p(lse), p(do_), p(dqkv), p(dsum), B, N, H, D, CODE[dt], st())
    torch.cuda.synchronize()
    assert guard_ok(out, B * N) and guard_ok(out2, B * N) and guard_ok(dqkv, B * N) and bool((lse[B * H * N:] == GUARD).all())
    assert torch.equal(out[:B * N].view(torch.int16 if dt == "bf16" else torch.int32), out2[:B * N].view(torch.int16 if dt == "bf16" else torch.int32))
    for t in (out[:B * N], lse[:B * H * N], dqkv[:B * N]):
        assert bool(torch.isfinite(t.float()).all()), tag
    labs = V.attn_logit_abs(qkv, B, N, H, hd)                          # [B,H,N]
    cond = hd * U * labs                                                # relative error of P of the row
    g_o = V.heads(V.f64(out[:B * N]), B, N, H, hd)
    gq, gk, gv = V.split_qkv(V.f64(dqkv[:B * N]), B, N, H, hd)
    bf = dt == "bf16"
    mfma = bf and hd == 64
    cq, ck = V.attn_cancel_bound(qkv, dout, B, N, H, hd, 2.0 ** -9 if bf else U, 2.0 ** -9 if mfma else N * U)

    def amax(t):
        return t.abs().amax(dim=(-1, -2), keepdim=True)
    cmax = cond.amax(-1)[..., None, None]
    blocked(f"{tag} out", g_o, ref_o, V.ATTN_OUT[dt], cond[..., None] * amax(ref_o).expand_as(ref_o))
    blocked(f"{tag} dq", gq, ref_dq, V.ATTN_GRAD[dt], cq + cond[..., None] * amax(ref_dq))
    blocked(f"{tag} dk", gk, ref_dk, V.ATTN_GRAD[dt], ck + cmax * amax(ref_dk))
    blocked(f"{tag} dv", gv, ref_dv, V.ATTN_GRAD[dt], (cmax * amax(ref_dv)).expand_as(ref_dv))
    g_lse = V.f64(lse[:B * H * N]).reshape(B, H, N)
    measure(f"{tag} lse abs", g_lse, ref_lse)
    check(f"{tag} lse", g_lse, ref_lse, larger(torch.full_like(ref_lse, V.measured(V.LSE_ABS)), V.lse_floor(cond, N, ref_lse)))
    zero = torch.zeros_like(do_)
    dz = nan_out(B * N, 3 * D, dt)
    call("clhip_attn_bwd", p(dq_), p(out), p(lse), p(zero), p(dz), p(dsum), B, N, H, D, CODE[dt], st())
    torch.cuda.synchronize()
    assert bool((dz[:B * N].float() == 0).all()) and guard_ok(dz, B * N), tag


MFMA_N = [1, 15, 16, 17, 32, 33, 192, 193, 197, 208, 209, 222, 224, 225, 240, 241, 255, 256]


@pytest.mark.parametrize("N", MFMA_N)
def test_attention_mfma_every_token_count(N):
    """bf16, head dim 64: forward <13> / <14> / <0>, backward mfma3 (193..224) / mfma (<= 240) / generic (241..256), first and last N of each"""
    qkv, dout = V.attn_inputs(2, N, 3, 64, 100 + N, "bf16")
    run_attention(qkv, dout, 2, N, 3, 64, "bf16", f"attn bf16 hd64 N={N}")


@pytest.mark.parametrize("dt,hd", [("f32", 64), ("bf16", 32)])
@pytest.mark.parametrize("N", [1, 17, 64, 197, 256])
def test_attention_generic(dt, hd, N):
    qkv, dout = V.attn_inputs(2, N, 3, hd, 300 + N, dt)
    run_attention(qkv, dout, 2, N, 3, hd, dt, f"attn {dt} hd{hd} N={N}")


def test_attention_more_workgroups_than_cus():
    """B * H = 264 workgroups at N = 17"""
    qkv, dout = V.attn_inputs(22, 17, 12, 64, 417, "bf16")
    run_attention(qkv, dout, 22, 17, 12, 64, "bf16", "attn bf16 hd64 BH=264")


@pytest.mark.parametrize("dt,hd,N", [("bf16", 64, 197), ("bf16", 64, 208), ("bf16", 64, 224), ("bf16", 64, 240), ("f32", 64, 197), ("bf16", 32, 197)])
def test_attention_shifted_logits(dt, hd, N):
    """a query row with every logit near -128 (lse < -100), one near +128, a one-hot row, a head of identical keys; bf16-exact values.
    At N = 197 and 208 the row with lse < -88.7 meets padded keys in attn_bwd_mfma3_kernel: P = exp2(0 - lse log2 e) overflows there"""
    qkv, dout = V.attn_shifted_inputs(2, N, 3, hd, 500 + N)
    run_attention(qkv, dout, 2, N, 3, hd, dt, f"attn shifted {dt} hd{hd} N={N}")


def test_attention_rejects_bad_arguments():
    """N = 257, head dim 128 and D % 8 != 0: the error code, and the NaN-filled outputs untouched"""
    for B, N, H, D in [(1, 257, 1, 64), (1, 16, 1, 128), (1, 16, 1, 60)]:
        qkv = torch.zeros(B * N, 3 * D, device=DEV, dtype=torch.bfloat16)
        out, dqkv = nan_out(B * N, D, "bf16"), nan_out(B * N, 3 * D, "bf16")
        lse = torch.full((B * H * N,), float("nan"), device=DEV)
        dsum = torch.empty(B * H * N, device=DEV)
        dout = torch.zeros(B * N, D, device=DEV, dtype=torch.bfloat16)
        with pytest.raises(_lib.ClhipError):
            call("clhip_attn_fwd", p(qkv), p(out), p(lse), B, N, H, D, CODE["bf16"], st())
        with pytest.raises(_lib.ClhipError):
            call("clhip_attn_bwd", p(qkv), p(out), p(lse), p(dout), p(dqkv), p(dsum), B, N, H, D, CODE["bf16"], st())
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[:B * N].float()).all()) and bool(torch.isnan(dqkv[:B * N].float()).all()) and bool(torch.isnan(lse).all())
    x = torch.zeros(4, 60, device=DEV)
    y = nan_out(4, 60, "f32")
    with pytest.raises(_lib.ClhipError):
        call("clhip_ln_fwd", p(x), p(x), p(x), p(y), None, None, 4, 60, 1e-5, CODE["f32"], st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[:4]).all())


# -------------------------------------------------------------------------------------------------------- LayerNorm
def run_ln(M, D, dt, eps, offset, tag):
    x, gamma, beta, dy, g0 = V.ln_inputs(M, D, 600 + M + D, dt, offset)
    ry, rmean, rrstd, rdx = V.ln_ref(x, gamma, beta, dy, eps)
    xd, gd, bd, dyd = dev(x, dt), dev(gamma), dev(beta), dev(dy, dt)
    y, y2 = nan_out(M, D, dt), nan_out(M, D, dt)
    mr = torch.full((2, M + 4), float("nan"), device=DEV)
    mr[:, M:] = GUARD
    call("clhip_ln_fwd", p(xd), p(gd), p(bd), p(y), p(mr[0]), p(mr[1]), M, D, eps, CODE[dt], st())
    call("clhip_ln_fwd", p(xd), p(gd), p(bd), p(y2), None, None, M, D, eps, CODE[dt], st())
    g = nan_out(M, D, dt)
    g[:M] = dev(g0, dt)
    call("clhip_ln_bwd", p(dyd), p(xd), p(gd), p(mr[0]), p(mr[1]), p(g), M, D, CODE[dt], st())
    torch.cuda.synchronize()
    assert guard_ok(y, M) and guard_ok(y2, M) and guard_ok(g, M) and bool((mr[:, M:] == GUARD).all())
    assert torch.equal(y[:M].view(torch.int16 if dt == "bf16" else torch.int32), y2[:M].view(torch.int16 if dt == "bf16" else torch.int32))
    mean_allowed = larger(V.measured(V.LN_MEAN_REL) * rmean.abs(), V.mean_floor(V.f64(x)))
    rstd_allowed = larger(V.measured(V.LN_RSTD_REL), V.rstd_floor(D)) * rrstd
    measure(f"{tag} mean rel", mr[0, :M], rmean, rmean.abs())
    measure(f"{tag} rstd rel", mr[1, :M], rrstd, rrstd)
    check(f"{tag} mean", mr[0, :M], rmean, mean_allowed)
    check(f"{tag} rstd", mr[1, :M], rrstd, rstd_allowed)
    rg = V.f64(g0) + rdx
    ay = V.LN[dt] * ry.abs().amax(1, keepdim=True) + V.FLOOR * float(ry.abs().max())
    ag = V.LN[dt] * rg.abs().amax(1, keepdim=True) + V.FLOOR * float(rg.abs().max())
    ay, ag = ay.expand_as(ry), ag.expand_as(rg)
    if offset:      # what the mean's own bound lets through: (x - mean) rstd moves by rstd * mean error
        xh_err = (rrstd * mean_allowed)[:, None]
        gam = V.f64(gamma).abs()[None, :]
        dg = V.f64(dy) * V.f64(gamma)
        xh = (V.f64(x) - rmean[:, None]) * rrstd[:, None]
        s2 = (dg * xh).mean(1, keepdim=True)
        ay = ay + xh_err * gam
        ag = ag + rrstd[:, None] * xh_err * (s2.abs() + xh.abs() * dg.abs().mean(1, keepdim=True))
    check(f"{tag} y", y[:M], ry, ay)
    check(f"{tag} g0+dx", g[:M], rg, ag)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("D", [8, 64, 520, 768, 1024, 1032, 2048])
def test_layernorm_every_path(dt, D):
    """NC = 2 up to D = 1024, NC = 4 above; one chunk in lane 0 (8), a second chunk held by one lane (520); M = 1 and M % 4 = 1, 2, 3"""
    for M in (1, 5, 6, 7, 64):
        for eps in (1e-5, 1e-6):
            run_ln(M, D, dt, eps, False, f"ln {dt} M={M} D={D} eps={eps:g}")


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("D", [768, 1032])
def test_layernorm_large_common_offset(dt, D):
    run_ln(5, D, dt, 1e-5, True, f"ln offset {dt} D={D}")


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("B,N,D,P", [(1, 1, 8, 1), (3, 5, 100, 5), (2, 7, 2040, 3), (2, 4, 2048, 1), (4, 197, 768, 1), (3, 30, 768, 25)])
def test_ln_pool(dt, B, N, D, P):
    x, gamma, beta, dfeat = V.ln_pool_inputs(B, N, D, 700 + D + N, dt)
    rfeat, rg = V.ln_pool_ref(x, gamma, beta, dfeat, B, N, D, P, 1e-6)
    xd, gd, bd, dfd = dev(x, dt), dev(gamma), dev(beta), dev(dfeat)
    feat, g = nan_out(B, D, "f32"), nan_out(B * N, D, dt)
    call("clhip_ln_pool_fwd", p(xd), p(gd), p(bd), p(feat), B, N, D, P, 1e-6, CODE[dt], st())
    call("clhip_ln_pool_bwd", p(dfd), p(xd), p(gd), p(g), B, N, D, P, 1e-6, CODE[dt], st())
    torch.cuda.synchronize()
    assert guard_ok(feat, B) and guard_ok(g, B * N)
    tag = f"ln_pool {dt} {(B, N, D, P)}"
    check(f"{tag} feat", feat[:B], rfeat, V.LN_POOL_FEAT * rfeat.abs().amax(1, keepdim=True) + V.FLOOR * float(rfeat.abs().max()))
    g3 = V.f64(g[:B * N]).reshape(B, N, D)
    check(f"{tag} g", g3[:, :P], rg[:, :P], V.LN[dt] * rg[:, :P].abs().amax(2, keepdim=True) + V.FLOOR * float(rg.abs().max()))
    assert bool((g3[:, P:] == 0).all())


# ------------------------------------------------------------------------------------------ weight preparation, LoRA
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("rows,cols,ranks", [(96, 32, (0, 1, 10, 16)), (120, 40, (0, 1, 10, 16)), (216, 72, (0, 1, 10, 16)), (50, 70, (0,))])
def test_weight_prep2(dt, rows, cols, ranks):
    """rows / columns no multiple of the 32-tile; wt alone, wt_t alone, both; the pointer not given is not written, the given one has a guard"""
    for rank in ranks:
        w, Ak, Bk, Av, Bv = V.lora_inputs(rows, cols, rank, 800 + rows + rank)
        eff = V.weight_eff_ref(w, Ak, Bk, Av, Bv)
        lo = [dev(t) if t is not None else None for t in (Ak, Bk, Av, Bv)]
        wd = dev(w)
        for use_wt, use_t in ((True, False), (False, True), (True, True)):
            wt, wtt = nan_out(rows, cols, dt), nan_out(cols, rows, dt)
            call("clhip_weight_prep2", p(wd), p(wt) if use_wt else None, p(wtt) if use_t else None, rows, cols, *[p(t) for t in lo], rank, CODE[dt], st())
            torch.cuda.synchronize()
            tag = f"weight_prep2 {dt} {(rows, cols)} r={rank} wt={use_wt} wt_t={use_t}"
            assert guard_ok(wt, rows) and guard_ok(wtt, cols)
            bound = V.COPY[dt] * float(eff.abs().max())
            if use_wt:
                check(f"{tag} wt", wt[:rows], eff, bound)
            else:
                assert bool(torch.isnan(wt[:rows].float()).all())
            if use_t:
                check(f"{tag} wt_t", wtt[:cols], eff.T, bound)
            else:
                assert bool(torch.isnan(wtt[:cols].float()).all())


def ptr_array(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("D,rank", [(32, 1), (32, 16), (96, 1), (96, 16)])
@pytest.mark.parametrize("layers", [1, 3, 33])
def test_lora_qkv_refresh(dt, D, rank, layers):
    """every layer its own weights (33 crosses the 32-entry descriptor table): k and v rows of wt / wt_t = the fp64 effective weight with
    the NEW B, q rows bit-unchanged from the weight_prep2 fill with the OLD B; equal bits to weight_prep2 on the same layer"""
    bits = torch.int16 if dt == "bf16" else torch.int32
    keep, ws, As, Bs, Cs, Ds, wts, wtts = [], [], [], [], [], [], [], []
    for l in range(layers):
        w, Ak, Bk_old, Av, Bv_old = V.lora_inputs(3 * D, D, rank, 900 + 10 * l)
        Bk, Bv = V.randn((D, rank), 901 + 10 * l + 5), V.randn((D, rank), 902 + 10 * l + 5)
        d = [dev(t) for t in (w, Ak, Bk_old, Av, Bv_old, Bk, Bv)]
        wt, wtt = nan_out(3 * D, D, dt), nan_out(D, 3 * D, dt)
        call("clhip_weight_prep2", p(d[0]), p(wt), p(wtt), 3 * D, D, p(d[1]), p(d[2]), p(d[3]), p(d[4]), rank, CODE[dt], st())
        want_wt, want_wtt = nan_out(3 * D, D, dt), nan_out(D, 3 * D, dt)
        call("clhip_weight_prep2", p(d[0]), p(want_wt), p(want_wtt), 3 * D, D, p(d[1]), p(d[5]), p(d[3]), p(d[6]), rank, CODE[dt], st())
        keep.append((d, wt.clone(), want_wt, want_wtt, V.weight_eff_ref(w, Ak, Bk, Av, Bv)))
        ws.append(d[0]); As.append(d[1]); Bs.append(d[5]); Cs.append(d[3]); Ds.append(d[6]); wts.append(wt); wtts.append(wtt)
    torch.cuda.synchronize()
    call("clhip_lora_qkv_refresh", layers, ptr_array(ws), ptr_array(As), ptr_array(Bs), ptr_array(Cs), ptr_array(Ds), ptr_array(wts), ptr_array(wtts),
         D, rank, CODE[dt], st())
    torch.cuda.synchronize()
    worst = 0.0
    for l in range(layers):
        _, before, want_wt, want_wtt, eff = keep[l]
        wt, wtt = wts[l], wtts[l]
        assert guard_ok(wt, 3 * D) and guard_ok(wtt, D), l
        assert torch.equal(wt[:D].view(bits), before[:D].view(bits)), l                          # q rows untouched
        assert torch.equal(wtt[:D, :D].view(bits), before[:D].T.contiguous().view(bits)), l
        if dt == "bf16":
            assert torch.equal(wt[:3 * D].view(bits), want_wt[:3 * D].view(bits)) and torch.equal(wtt[:D].view(bits), want_wtt[:D].view(bits)), l
        bound = V.COPY[dt] * float(eff.abs().max())
        worst = max(worst, err_ratio(wt[D:3 * D], eff[D:], bound), err_ratio(wtt[:D, D:], eff[D:].T, bound))
    print(f"[ratio] lora_qkv_refresh {dt} D={D} r={rank} layers={layers}: {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("D,rank", [(32, 1), (32, 16), (96, 1), (96, 16)])
def test_lora_merge(D, rank):
    w, Ak, Bk, Av, Bv = V.lora_inputs(3 * D, D, rank, 1000 + D + rank)
    wm = nan_out(3 * D, D, "f32")
    wm[:3 * D] = dev(w)
    lo = [dev(t) for t in (Ak, Bk, Av, Bv)]
    call("clhip_lora_merge", p(wm), *[p(t) for t in lo], D, rank, st())
    torch.cuda.synchronize()
    eff = V.weight_eff_ref(w, Ak, Bk, Av, Bv)
    assert guard_ok(wm, 3 * D) and torch.equal(wm[:D].cpu(), w[:D])
    check(f"lora_merge D={D} r={rank}", wm[:3 * D], eff, V.COPY["f32"] * float(eff.abs().max()))


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("rank", [1, 10, 16])
def test_lora_acat(dt, rank):
    """the layout lora_acat_kernel writes: [32, D], rows 0..r-1 = A_k, rows r..2r-1 = A_v, the rest zero"""
    D = 72
    Ak, Av = V.as_mode(V.randn((rank, D), 1100 + rank), dt), V.as_mode(V.randn((rank, D), 1101 + rank), dt)
    acat = nan_out(32, D, dt)
    Akd, Avd = dev(Ak), dev(Av)
    call("clhip_lora_acat", p(Akd), p(Avd), p(acat), D, rank, CODE[dt], st())
    torch.cuda.synchronize()
    want = torch.zeros(32, D)
    want[:rank], want[rank:2 * rank] = Ak, Av
    assert guard_ok(acat, 32) and torch.equal(acat[:32].float().cpu(), want)


LORA_GRAD_CASES = [(M, 128, 10) for M in (1, 511, 512, 513, 1024, 1025, 2700)] + \
                  [(M, D, r) for M in (513, 1025) for D, r in ((64, 1), (64, 16), (96, 1), (96, 10), (96, 16), (128, 1), (128, 16))] + [(513, 64, 10)]


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("M,D,rank", LORA_GRAD_CASES)
def test_lora_grad(dt, M, D, rank):
    """below one slab, on and one past the 512- / 1024-row slab boundaries; the slab kernels and (bf16, D % 64 == 0, a_cat given) the MFMA
    path; D = 96 with a_cat given takes the slab path and its bound; two runs agree bitwise.  The two column windows of the shared slab product
    (csrc/tn_slab.hip): rank 16 fills all 32 columns of P16, rank 1 keeps one column of each half, and at rank 10 in fp32 with M = 513 the v window
    of the last row ends the [M, 2r] P exactly.  dBk and dBv start non-zero (the += contract); only the 1e-4 bound of the slab path is tight enough
    to tell a lost preload, the MFMA path's 1e-2 of max|ref| is not -- both paths end in the same reduce kernel"""
    x, dqkv = V.as_mode(V.randn((M, D), 1200 + M), dt), V.as_mode(V.randn((M, 3 * D), 1201 + M), dt)
    Ak, Av = V.randn((rank, D), 1202 + rank), V.randn((rank, D), 1203 + rank)
    rk, rv = V.lora_db_ref(x, dqkv, Ak, Av, D)
    xd, dd, Akd, Avd = dev(x, dt), dev(dqkv, dt), dev(Ak), dev(Av)
    acat = torch.empty(32, D, device=DEV, dtype=TD[dt])
    call("clhip_lora_acat", p(Akd), p(Avd), p(acat), D, rank, CODE[dt], st())
    for fast in (False, True):
        runs = []
        for _ in range(2):
            dBk, dBv = nan_out(D, rank, "f32"), nan_out(D, rank, "f32")
            dBk[:D], dBv[:D] = 1.0, -2.0
            ws = torch.empty(_lib.lib().clhip_lora_grad_ws_bytes(M, D, rank), dtype=torch.uint8, device=DEV)
            call("clhip_lora_grad", p(xd), p(dd), p(Akd), p(Avd), p(acat) if fast else None, p(dBk), p(dBv), p(ws), M, D, rank, CODE[dt], st())
            torch.cuda.synchronize()
            assert guard_ok(dBk, D) and guard_ok(dBv, D)
            runs.append((dBk.clone(), dBv.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        rel = V.LORA_GRAD_MFMA if (fast and dt == "bf16" and D % 64 == 0) else V.LORA_GRAD
        tag = f"lora_grad {dt} M={M} D={D} r={rank} a_cat={fast}"
        check(f"{tag} dBk", runs[0][0][:D], 1 + rk, rel * float((1 + rk).abs().max()))
        check(f"{tag} dBv", runs[0][1][:D], rv - 2, rel * float(rv.abs().max()))


# -------------------------------------------------------------------------------------------------------------- Gram
@pytest.mark.parametrize("dt,M,D", [("f32", 1, 8), ("f32", 1023, 100), ("f32", 1025, 64), ("f32", 2500, 128), ("bf16", 130, 100)])
def test_gram_accum(dt, M, D):
    """fp32: ragged 64-tile (D = 100), ragged 1024-row slab; bf16 with D % 8 != 0 takes the generic kernel"""
    x = V.as_mode(V.randn((M, D), 1300 + M), dt)
    G = nan_out(D, D, "f32")
    G[:D] = 1.0
    xd = dev(x, dt)
    call("clhip_gram_accum", p(xd), p(G), M, D, CODE[dt], st())
    torch.cuda.synchronize()
    ref = 1 + V.gram_ref(x)
    assert guard_ok(G, D)
    check(f"gram {dt} M={M} D={D}", G[:D], ref, V.GRAM * float(ref.abs().max()))


@pytest.mark.parametrize("M,D,L", [(1, 8, 1), (130, 72, 2)])
def test_gram_accum_batched(M, D, L):
    stride = M * D + 64
    xs = [V.rb(V.randn((M, D), 1400 + l)) for l in range(L)]
    buf = torch.zeros(L * stride, device=DEV, dtype=torch.bfloat16)
    for l in range(L):
        buf[l * stride:l * stride + M * D] = dev(xs[l], "bf16").reshape(-1)
    G = nan_out(L * D, D, "f32")
    G[:L * D] = 0.5
    call("clhip_gram_accum_batched", p(buf), stride, L, p(G), M, D, CODE["bf16"], st())
    torch.cuda.synchronize()
    assert guard_ok(G, L * D)
    for l in range(L):
        ref = 0.5 + V.gram_ref(xs[l])
        check(f"gram_batched {(M, D, L)} layer {l}", G[l * D:(l + 1) * D], ref, V.GRAM_BATCHED * float(ref.abs().max()))


# --------------------------------------------------------------------------------------------------------------- L2P
def run_l2p(shape, q, key, prompt, tag, zero_row=None):
    B, D, pool, top_k, length = shape
    r = V.l2p_ref(q, key, top_k)
    qd, kd, pd = dev(q), dev(key), dev(prompt)
    ids = torch.full((top_k + 2,), -7, dtype=torch.int32, device=DEV)
    tokens = nan_out(top_k * length, D, "f32")
    rs = torch.full((2,), float("nan"), device=DEV)
    rs[1] = GUARD
    dkey = nan_out(pool, D, "f32")
    scratch = torch.empty(B + pool + D + B * pool, device=DEV)
    call("clhip_l2p_select", p(qd), p(kd), p(pd), B, D, pool, top_k, length, p(ids), p(tokens), p(rs), p(dkey), p(scratch), st())
    torch.cuda.synchronize()
    assert ids[top_k:].tolist() == [-7, -7] and guard_ok(tokens, top_k * length) and float(rs[1]) == GUARD and guard_ok(dkey, pool)
    near = int((r["gap"] <= r["noise"]).sum())
    assert near <= V.NEAR_TIE_CAP * B, (tag, near)
    if near == 0:
        assert ids[:top_k].tolist() == r["ids"], tag
    got_ids = ids[:top_k].tolist()
    if got_ids == r["ids"]:
        check(f"{tag} reduce_sim", rs[:1], r["reduce_sim"].reshape(1), V.L2P_SIM * abs(float(r["reduce_sim"])))
        bound = V.L2P_DKEY * r["dkey"].abs().amax(1, keepdim=True).clamp_min(V.FLOOR * float(r["dkey"].abs().max()))
        check(f"{tag} dkey", dkey[:pool], r["dkey"], bound.expand_as(r["dkey"]))
        assert torch.equal(tokens[:top_k * length].cpu(), prompt[torch.tensor(r["ids"])].reshape(-1, D))
    dtok = V.randn((top_k * length, D), 1500 + B)
    dpool = nan_out(pool * length, D, "f32")
    dtd = dev(dtok)
    call("clhip_l2p_scatter", p(dtd), p(ids), p(dpool), pool, top_k, length, D, st())
    torch.cuda.synchronize()
    want = torch.zeros(pool, length, D)
    want[torch.tensor(got_ids)] = dtok.reshape(top_k, length, D)
    assert guard_ok(dpool, pool * length) and torch.equal(dpool[:pool * length].cpu(), want.reshape(-1, D))


@pytest.mark.parametrize("shape", V.L2P_CASES)
def test_l2p_select(shape):
    """pool = 1, pool = 64 (all lanes), top_k = pool, B = 1, B = 40 (more samples than waves), D = 100, length = 1.  dkey is judged per key
    row (a key that is not selected has an exactly zero gradient: the floor is 1e-7 of the tensor's max)"""
    B, D, pool, top_k, length = shape
    q, key, prompt = V.l2p_inputs(B, D, pool, length, V.l2p_seed(B, D, pool))
    run_l2p(shape, q, key, prompt, f"l2p {shape}")


def test_l2p_all_zero_key():
    """F.normalize's clamp at 1e-12: the zero key's cosine is 0 and its gradient is sbar / 1e-12"""
    shape = V.L2P_ZERO_KEY_CASE
    B, D, pool, top_k, length = shape
    q, key, prompt = V.l2p_inputs(B, D, pool, length, V.l2p_seed(B, D, pool), V.L2P_ZERO_KEY_ROW)
    run_l2p(shape, q, key, prompt, f"l2p zero key {shape}", V.L2P_ZERO_KEY_ROW)


def test_l2p_batch_majority_tie():
    """prompt ids 1 and 3 are picked equally often: the lower id comes first"""
    q, key, prompt = V.l2p_tie_inputs()
    run_l2p(V.L2P_TIE_SHAPE, q, key, prompt, "l2p tie")


# ------------------------------------------------------------------------------------------------------------ tokens
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("B,S,pz", [(1, 8, 8), (3, 32, 8), (2, 48, 16)])
def test_patchify(dt, B, S, pz):
    img = V.randn((B, 3, S, S), 1600 + S)
    ref = V.patchify_ref(img, pz)
    rows = ref.shape[0]
    out = nan_out(rows, ref.shape[1], dt)
    imgd = dev(img)
    call("clhip_patchify", p(imgd), p(out), B, S, pz, CODE[dt], st())
    torch.cuda.synchronize()
    assert guard_ok(out, rows)
    if dt == "f32":
        assert torch.equal(out[:rows].cpu(), ref)
    check(f"patchify {dt} {(B, S, pz)}", out[:rows], ref.double(), V.COPY[dt] * float(ref.abs().max()))


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D", [8, 128])
@pytest.mark.parametrize("n_prompt", [0, 1, 6])
def test_assemble_and_prompt_grad(dt, B, D, n_prompt):
    """npch = 5 (no square, no relation to D); prompt_grad at n_prompt (and at N - 1 - npch = n_prompt: every token ahead of cls)"""
    npch = 5
    N = n_prompt + 1 + npch
    pe = V.as_mode(V.randn((B * npch, D), 1700 + D), dt)
    cls, pos, prompt = V.randn((D,), 1701), V.randn((npch + 1, D), 1702), V.randn((6, D), 1703)
    ref = V.assemble_ref(pe, cls, pos, prompt, B, npch, n_prompt, D)
    x = nan_out(B * N, D, dt)
    ped, clsd, posd, prd = dev(pe, dt), dev(cls), dev(pos), dev(prompt)
    call("clhip_vit_assemble", p(ped), p(clsd), p(posd), p(prd) if n_prompt else None, p(x), B, npch, n_prompt, D, CODE[dt], st())
    torch.cuda.synchronize()
    assert guard_ok(x, B * N)
    check(f"assemble {dt} B={B} D={D} P={n_prompt}", x[:B * N], ref, V.COPY[dt] * float(ref.abs().max()))
    if n_prompt:
        g = V.as_mode(V.randn((B * N, D), 1704 + B), dt)
        rg = V.prompt_grad_ref(g, B, N, n_prompt, D)
        dprompt = nan_out(n_prompt, D, "f32")
        gd = dev(g, dt)
        call("clhip_vit_prompt_grad", p(gd), p(dprompt), B, N, n_prompt, D, CODE[dt], st())
        torch.cuda.synchronize()
        assert guard_ok(dprompt, n_prompt)
        check(f"prompt_grad {dt} B={B} D={D} P={n_prompt}", dprompt[:n_prompt], rg, V.PROMPT_GRAD * float(rg.abs().max()))
