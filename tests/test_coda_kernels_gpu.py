"""csrc/coda.hip alone on the MI355X against the fp64 restatement of tests/coda_ref.py (the literal F.normalize formulas, gradients by autograd).

Bounds, by the rule in the header of tests/test_sdlora_kernels_gpu.py (u = 2^-24, v = 2^-8): a product over K terms in fp32 is within K u sum|a b| of fp64
whatever the summation order, each product with its own K; an operand that already carries an error e adds e |b| summed; every further fp32 operation on a
value c adds u |c|; a value STORED as bf16 adds one bf16 step, 2 v |c|.  Written out for the kernels (aq = q * A_k, m = max(norm, 1e-12)):
  num = <aq, K>             e_num = (D + 1) u sum|aq K|                       (the product aq itself is one operation)
  |aq|, |K|                 relative (D / 2 + 2) u                            (a D-term sum of squares, then the root)
  c = num / (ma mk)         e_c = e_num / (ma mk) + (D + 7) u |c|
  P_ = sum_k c_k P_k        sum_k e_c |P_k| + f u sum_k |c_k P_k|             (+ 2 v |P_| for ek / ev in bf16 mode)
  dc = <dP_, P_k>           e_dc = L D u sum|dP_ P_k|
  dP_k = sum_b c dP_        sum_b e_c |dP_| + B u sum_b |c dP_|
  dA_k = sum_b q coef (K - tt aq),  coef = dc / (ma mk),  tt = [na >= eps] num / (ma na):
                            e_coef = e_dc / (ma mk) + (D + 7) u |coef|,  e_tt = e_num / (ma na) + (D + 7) u |tt|, propagated through the two terms,
                            + B u sum_b (|q coef K| + |q coef tt aq|)
  dK_k = (sum_b w aq) / mk - [nk >= eps] S K / (mk^2 nk),  w = dc / ma,  S = sum_b w num:  the same propagation (e_w = e_dc / ma + (D / 2 + 3) u |w|).
A zero K row or A row has norm 0 < eps: m = eps, the indicator is off, and the same bounds hold relative to gradients that are 10^12 times larger."""
import ctypes as C

import pytest
import torch

import coda_ref as R
from libcontinual_amd import _lib
from libcontinual_amd._lib import call

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U, V = 2.0 ** -24, 2.0 ** -8
EPS = 1e-12
DT = {"f32": (_lib.F32, torch.float32), "bf16": (_lib.BF16, torch.bfloat16)}
SENTINEL = 7.0
WINDOWS = [(1, 0, 1), (6, 0, 3), (6, 3, 6), (100, 0, 10), (100, 90, 100)]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _arr(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def make_inputs(layers, B, D, pool, L, seed, zero_rows=None):
    """fp32 host tensors: q [B, D]; per layer K, A [pool, D], P [pool, L, D], cotangents dek, dev [B, L/2, D]"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, D, generator=g)
    lay = []
    for _ in range(layers):
        K, A = torch.randn(pool, D, generator=g), torch.rand(pool, D, generator=g) + 0.1 * torch.randn(pool, D, generator=g)
        P = torch.randn(pool, L, D, generator=g) * 0.2
        if zero_rows is not None:
            K[zero_rows[0]] = 0
            A[zero_rows[1]] = 0
        lay.append((K, A, P, torch.randn(B, L // 2, D, generator=g), torch.randn(B, L // 2, D, generator=g)))
    return q, lay


def reference(q, K, A, P, dek, dev, s, f):
    """fp64 results and the bounds of the header for one layer -> dict name -> (ref, bound)"""
    q, K, A, P, dek, dev = (t.double() for t in (q, K, A, P, dek, dev))
    B, D = q.shape
    L = P.shape[1]
    dK, dA, dP, ek, ev, c = R.assemble_grads(q, K, A, P, s, f, dek, dev)
    Kf, Af, Pf = K[:f], A[:f], P[:f]
    aq = q[:, None, :] * Af[None]                                   # [B, f, D]
    num, na, nk = (aq * Kf[None]).sum(-1), aq.norm(dim=-1), Kf.norm(dim=-1)
    ma, mk = na.clamp_min(EPS), nk.clamp_min(EPS)[None]
    e_num = (D + 1) * U * (aq * Kf[None]).abs().sum(-1)
    e_c = e_num / (ma * mk) + (D + 7) * U * c.abs()
    P_ = torch.cat((ek, ev), dim=1)
    b_P = torch.einsum("bk,kld->bld", e_c, Pf.abs()) + f * U * torch.einsum("bk,kld->bld", c.abs(), Pf.abs())
    g = torch.cat((dek, dev), dim=1)                                # [B, L, D]
    w_ = slice(s, f)
    dc = torch.einsum("bld,kld->bk", g, Pf)[:, w_]
    e_dc = L * D * U * torch.einsum("bld,kld->bk", g.abs(), Pf.abs())[:, w_]
    b_dP = torch.einsum("bk,bld->kld", e_c[:, w_], g.abs()) + B * U * torch.einsum("bk,bld->kld", c[:, w_].abs(), g.abs())
    aq, num, na, ma, e_num, Kw = aq[:, w_], num[:, w_], na[:, w_], ma[:, w_], e_num[:, w_], Kf[w_]
    mkw, nkw = mk[:, w_], nk[w_]
    coef = dc / (ma * mkw)
    e_coef = e_dc / (ma * mkw) + (D + 7) * U * coef.abs()
    on_a = na >= EPS
    tt = torch.where(on_a, num / (ma * na.clamp_min(1e-300)), torch.zeros_like(num))
    e_tt = torch.where(on_a, e_num / (ma * na.clamp_min(1e-300)), torch.zeros_like(num)) + (D + 7) * U * tt.abs()
    qa = q.abs()[:, None, :]
    inner = Kw[None] - tt[..., None] * aq
    b_dA = (qa * (e_coef[..., None] * inner.abs() + coef.abs()[..., None] * (e_tt[..., None] * aq.abs() + 3 * U * (Kw.abs()[None] + (tt[..., None] * aq).abs())))).sum(0)
    b_dA = b_dA + B * U * (qa * coef.abs()[..., None] * (Kw.abs()[None] + (tt[..., None] * aq).abs())).sum(0)
    w = dc / ma
    e_w = e_dc / ma + (D / 2 + 3) * U * w.abs()
    dKa = (w[..., None] * aq).sum(0)
    e_dKa = (e_w[..., None] * aq.abs()).sum(0) + (B + 1) * U * (w[..., None] * aq).abs().sum(0)
    S = (w * num).sum(0)
    e_S = (e_w * num.abs() + w.abs() * e_num).sum(0) + B * U * (w * num).abs().sum(0)
    mk1 = mkw[0]
    den = mk1 * mk1 * nkw.clamp_min(1e-300)
    second = torch.where(nkw >= EPS, e_S / den + (1.5 * D + 10) * U * S.abs() / den, torch.zeros_like(S))      # (off for a zero K row: den underflows there)
    b_dK = e_dKa / mk1[:, None] + (D / 2 + 3) * U * (dKa / mk1[:, None]).abs() + second[:, None] * Kw.abs()
    return {"c": (c, e_c), "P_": (P_, b_P), "dK": (dK, b_dK), "dA": (dA, b_dA), "dP": (dP, b_dP)}


def launch(q, lay, pool, L, s, f, dtype):
    code, tdt = DT[dtype]
    n, (B, D) = len(lay), q.shape
    qd = q.to(DEV)
    Kd, Ad, Pd, gk, gv = ([t[i].to(DEV).contiguous() for t in lay] for i in range(5))
    ek = [torch.full((B + 1, L // 2, D), float("nan"), device=DEV, dtype=tdt) for _ in range(n)]
    ev = [torch.full((B + 1, L // 2, D), float("nan"), device=DEV, dtype=tdt) for _ in range(n)]
    for t in ek + ev:
        t[B:] = SENTINEL
    c = torch.full((n * B * f + 8,), float("nan"), device=DEV)
    c[n * B * f:] = SENTINEL
    call("clhip_coda_fwd", n, qd.data_ptr(), _arr(Kd), _arr(Ad), _arr(Pd), _arr(ek), _arr(ev), c.data_ptr(), B, D, pool, L, f, code, _st())
    dK = [torch.full((pool, D), SENTINEL, device=DEV) for _ in range(n)]
    dA = [torch.full((pool, D), SENTINEL, device=DEV) for _ in range(n)]
    dP = [torch.full((pool, L, D), SENTINEL, device=DEV) for _ in range(n)]
    nws = _lib.lib().clhip_coda_ws_bytes(n, B, s, f)
    assert nws > 0 and nws % 4 == 0
    ws = torch.empty(nws // 4 + 8, device=DEV)
    ws[nws // 4:] = SENTINEL
    call("clhip_coda_bwd", n, qd.data_ptr(), _arr(Kd), _arr(Ad), _arr(Pd), c.data_ptr(), _arr(gk), _arr(gv), _arr(dK), _arr(dA), _arr(dP), ws.data_ptr(),
         B, D, pool, L, s, f, _st())
    torch.cuda.synchronize()
    assert bool((c[n * B * f:] == SENTINEL).all()) and bool((ws[nws // 4:] == SENTINEL).all())
    for t in ek + ev:
        assert bool((t[B:].float() == SENTINEL).all())
    return ek, ev, c[:n * B * f].view(n, B, f), dK, dA, dP


def ratio(name, got, ref, bound):
    err = (got.double().cpu().reshape(ref.shape) - ref).abs()
    assert bool(torch.isfinite(err).all()), name
    pos = bound > 0
    assert not bool((err[~pos] > 0).any()), name                     # a bound of zero admits nothing
    r = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    print(f"[ratio] {name}: {r:.3g}")
    assert r <= 1.0, (name, r)


def run_case(layers, B, D, pool, s, f, L, dtype, seed, zero_rows=None):
    q, lay = make_inputs(layers, B, D, pool, L, seed, zero_rows)
    ek, ev, c, dK, dA, dP = launch(q, lay, pool, L, s, f, dtype)
    tag = f"coda {dtype} layers={layers} B={B} D={D} pool={pool} [{s},{f}) L={L}"
    store = 2 * V if dtype == "bf16" else 0.0
    for l, (K, A, P, dek, dev) in enumerate(lay):
        ref = reference(q, K, A, P, dek, dev, s, f)
        ratio(f"{tag} l{l} c", c[l], *ref["c"])
        P_, bP = ref["P_"]
        got = torch.cat((ek[l][:B], ev[l][:B]), dim=1)
        ratio(f"{tag} l{l} ek|ev", got, P_, bP + store * P_.abs())
        for name, buf in (("dK", dK[l]), ("dA", dA[l]), ("dP", dP[l])):
            ratio(f"{tag} l{l} {name}", buf[s:f], *ref[name])
            assert bool((buf[:s] == SENTINEL).all()) and bool((buf[f:] == SENTINEL).all()), (tag, name)
    return c, dK, dA, lay


@pytest.mark.parametrize("L", [2, 8])
@pytest.mark.parametrize("pool,s,f", WINDOWS)
@pytest.mark.parametrize("B", [1, 5, 128])
@pytest.mark.parametrize("D", [64, 768])
@pytest.mark.parametrize("layers", [1, 5])
def test_assembly_forward_and_backward(layers, D, B, pool, s, f, L):
    """fp32 mode (ek / ev fp32); the bf16 mode differs by the store of ek / ev alone: test_assembly_bf16_store"""
    run_case(layers, B, D, pool, s, f, L, "f32", 1000 + 7 * B + D + pool + s + L)


@pytest.mark.parametrize("B,D,pool,s,f,L", [(5, 64, 6, 0, 3, 8), (128, 768, 100, 0, 10, 8), (1, 768, 100, 90, 100, 2)])
def test_assembly_bf16_store(B, D, pool, s, f, L):
    run_case(5, B, D, pool, s, f, L, "bf16", 77 + B)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_zero_key_row_and_zero_attention_row(dtype):
    """K row 1 and A row 2 are zero: their coefficients are exactly zero, everything is finite, and the gradients follow the clamp form
    x / max(|x|, eps) that torch differentiates (their rows are 10^12 times the others)"""
    c, dK, dA, lay = run_case(2, 5, 64, 6, 0, 3, 8, dtype, 5, zero_rows=(1, 2))
    assert bool((c[:, :, 1] == 0).all()) and bool((c[:, :, 2] == 0).all()) and bool((c[:, :, 0] != 0).all())
    assert float(dK[0][1].abs().max()) > 1e6 and float(dA[0][2].abs().max()) > 1e6


def test_assembly_is_bit_reproducible():
    q, lay = make_inputs(5, 128, 768, 100, 8, 9)
    a = launch(q, lay, 100, 8, 0, 10, "bf16")
    b = launch(q, lay, 100, 8, 0, 10, "bf16")
    for x, y in zip(a, b):
        for u, v in zip(x, y) if isinstance(x, list) else [(x, y)]:
            assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))


def test_assembly_rejects_bad_arguments():
    """D % 64 != 0, odd L, f > pool, f = 0; the backward also s = f"""
    for D, L, s, f in [(60, 8, 0, 3), (64, 7, 0, 3), (64, 8, 0, 7), (64, 8, 0, 0)]:
        with pytest.raises(_lib.ClhipError):
            t = torch.zeros(4096, device=DEV)
            call("clhip_coda_fwd", 1, t.data_ptr(), _arr([t]), _arr([t]), _arr([t]), _arr([t]), _arr([t]), t.data_ptr(), 2, D, 6, L, f, _lib.F32, _st())
    for D, L, s, f in [(60, 8, 0, 3), (64, 7, 0, 3), (64, 8, 0, 7), (64, 8, 3, 3), (64, 8, 0, 0)]:
        with pytest.raises(_lib.ClhipError):
            t = torch.zeros(4096, device=DEV)
            call("clhip_coda_bwd", 1, t.data_ptr(), _arr([t]), _arr([t]), _arr([t]), t.data_ptr(), _arr([t]), _arr([t]), _arr([t]), _arr([t]), _arr([t]),
                 t.data_ptr(), 2, D, 6, L, s, f, _st())
