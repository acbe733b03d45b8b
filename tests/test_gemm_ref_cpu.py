"""tests/gemm_ref.py checks itself on the CPU: its GELU' against autograd in fp64, its accumulation bound against a plain fp32 emulation of the
product in three summation orders, and -- through clhip_gemm_nt_route, host code that needs no device -- that the cases of
tests/test_gemm_kernels_gpu.py take the routes named for them and together reach every kernel family, both split forms and 2, 3 and 4 K slices."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_ref as G
from libcontinual_amd import _lib


def test_gelu_and_its_derivative_against_autograd_fp64():
    x = torch.cat([torch.linspace(-12, 12, 48001, dtype=torch.float64), torch.tensor([0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 2 ** 0.5, -2 ** 0.5], dtype=torch.float64)])
    xr = x.clone().requires_grad_(True)
    y = F.gelu(xr)
    (d,) = torch.autograd.grad(y.sum(), xr)
    c, h = G.gelu_both(x)
    # autograd's Phi = (1 + erf) / 2 carries an absolute error of a few 2^-53 (it cancels in the negative tail); the rest is relative
    assert bool(((c - y.detach()).abs() <= 1e-15 * x.abs().clamp(min=1) + 1e-13 * c.abs()).all())
    assert bool(((h - d).abs() <= 1e-15 * x.abs().clamp(min=1) + 1e-13 * h.abs()).all())
    assert float(h.max()) <= G.GELU_D1_MAX and float(h.min()) >= -0.13
    # the negative tail keeps its relative accuracy: Phi(-x) / phi(x) is the Mills ratio, 1/x (1 - 1/x^2 + 3/x^4 - 15/x^6 ..)
    t = torch.tensor([10.0, 11.0, 12.0], dtype=torch.float64)
    c_t, _ = G.gelu_both(-t)
    mills = (1 / t) * (1 - 1 / t ** 2 + 3 / t ** 4 - 15 / t ** 6 + 105 / t ** 8)
    want = -t * mills * torch.exp(-0.5 * t * t) / (2 * np.pi) ** 0.5
    assert bool(((c_t - want).abs() <= 2e-6 * want.abs()).all())          # the series' own truncation: 945 / x^10 <= 1e-7 at x = 10


def _emulate(A, B, order):
    """fp32 products summed in fp32, one k at a time"""
    M, K = A.shape
    ks = {"forward": [range(K)], "reversed": [range(K - 1, -1, -1)], "four slices": [range(i * K // 4, (i + 1) * K // 4) for i in range(4)]}[order]
    parts = []
    for sl in ks:
        acc = np.zeros((M, B.shape[0]), np.float32)
        for k in sl:
            acc = acc + A[:, k:k + 1] * B[:, k][None, :]
        parts.append(acc)
    out = parts[0]
    for q in parts[1:]:
        out = out + q
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("K", [64, 4096])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_accumulation_bound_holds_for_an_fp32_emulation(K, dt):
    g = torch.Generator().manual_seed(K)
    A = torch.randn(24, K, generator=g)
    B = torch.randn(40, K, generator=g) / K ** 0.5
    if dt == "bf16":
        A, B = A.bfloat16().float(), B.bfloat16().float()
    _, ref, _ = G.gemm_ref(A, B, None, None, None, 0)
    allowed = (K + 8) * G.U24 * G.abs_prod(A, B)
    for order in ("forward", "reversed", "four slices"):
        got = torch.from_numpy(_emulate(A.numpy(), B.numpy(), order)).double()
        over = (got - ref).abs() > allowed
        assert int(over.sum()) == 0, (order, int(over.sum()))
        assert float((got - ref).abs().max()) > 0.0          # the emulation does round (a worst-case bound sits a factor ~sqrt(K) above a random walk)


def test_epilogues_of_the_reference():
    g = torch.Generator().manual_seed(1)
    A, B, bias, R, H = torch.randn(5, 64, generator=g), torch.randn(8, 64, generator=g), torch.randn(8, generator=g), torch.randn(5, 8, generator=g), torch.randn(5, 8, generator=g)
    P = A.double() @ B.double().T
    assert torch.equal(G.gemm_ref(A, B, None, None, None, 0)[1], P)
    assert torch.equal(G.gemm_ref(A, B, bias, None, None, 1)[1], P + bias.double())
    assert torch.equal(G.gemm_ref(A, B, bias, R, None, 2)[1], P + bias.double() + R.double())
    x, c, h = G.gemm_ref(A, B, bias, None, None, 3)
    assert torch.equal(x, P + bias.double()) and torch.allclose(c, F.gelu(x), rtol=1e-13, atol=1e-15) and h is not None
    x, c, h = G.gemm_ref(A, B, None, None, H, 4, prod=P)
    assert torch.equal(x, P) and torch.equal(c, P * H.double()) and h is None
    # epilogue 4's bound is epilogue 0's times |H|
    S = G.abs_prod(A, B)
    b0, _ = G.gemm_bound(S, 64, P, P, None, None, 0, "bf16")
    b4, _ = G.gemm_bound(S, 64, P, c, None, H, 4, "bf16")
    assert torch.allclose(b4, b0 * H.double().abs(), rtol=1e-14, atol=0)
    assert G.c_g() >= G.C_G_FLOOR


# ------------------------------------------------------------------------------------------------ the route query (host code: no device)
def route(case):
    L = _lib.lib()
    ld = G.pitches(case["N"], case["K"])
    buf = (C.c_int * 16)()
    L.clhip_gemm8_config(case["mode"])
    try:
        n = L.clhip_gemm_nt_route(case["M"], case["N"], case["K"], ld["lda"], ld["ldb"], ld["ldc"], ld["ldr"], ld["ldh"], {"bf16": _lib.BF16, "f32": _lib.F32}[case["dt"]], buf, 4)
    finally:
        L.clhip_gemm8_config(-1)
    assert 0 < n <= 3, (case["name"], n)
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(n)]


ALL_CASES = G.CASES + G.SPLITK_CASES + [G.SDLORA_CASE]


@pytest.mark.parametrize("case", ALL_CASES, ids=[c["name"] for c in ALL_CASES])
def test_each_case_takes_the_route_named_for_it(case):
    got = route(case)
    assert got == case["route"], (case["name"], got)
    assert got[0][1] == 0 and sum(l[2] for l in got) == case["M"] and all(a[1] + a[2] == b[1] for a, b in zip(got, got[1:]))      # the launches tile the rows


def test_the_cases_reach_every_kernel_family_and_split_form():
    routes = {c["name"]: route(c) for c in ALL_CASES}
    launches = [l for r in routes.values() for l in r]
    assert {l[0] for l in launches} == {G.GEMM8, G.T256, G.T160, G.T128, G.T64, G.F32_128}
    assert {l[3] for l in launches} == {1, 2, 3, 4}
    assert all(l[0] == G.T128 for l in launches if l[3] > 1)
    heads = {n: r for n, r in routes.items() if len(r) == 2 and r[0][0] == G.T256}
    # one round of 256 x 256 tiles (256 / (N / 256) row panels) + tail, and whole rounds (>= 2 here) + tail
    assert any(r[0][2] == (256 // (c["N"] // 256)) * 256 and c["K"] >= 2304 for c in ALL_CASES for n, r in heads.items() if n == c["name"])
    assert any(r[0][2] > (256 // (c["N"] // 256)) * 256 and c["K"] < 2304 for c in ALL_CASES for n, r in heads.items() if n == c["name"])
    assert any(len(r) == 2 and r[0][0] == G.GEMM8 for r in routes.values())          # gemm8 rows + a register-staged tail
    assert any(len(r) == 1 and r[0][0] == G.GEMM8 for r in routes.values())
    # both exits of the bf16 register-staged kernel: through LDS (N % 8 == 0) and direct (N % 8 == 4), on every tile that has both
    for fam in (G.T64, G.T128, G.T160):
        ns = {c["N"] % 8 for c in ALL_CASES if c["dt"] == "bf16" and any(l[0] == fam and l[3] == 1 for l in routes[c["name"]])}
        assert ns == {0, 4}, (fam, ns)


def test_route_query_rejects_what_the_call_rejects():
    L = _lib.lib()
    buf = (C.c_int * 16)()
    for M, N, K, lda in ((0, 64, 64, 64), (8, 6, 64, 64), (8, 64, 96, 96), (8, 64, 64, 68)):
        assert L.clhip_gemm_nt_route(M, N, K, lda, K, N, N, N, _lib.BF16, buf, 4) == -1
        assert b"invalid argument" in L.clhip_last_error()
    assert L.clhip_gemm_nt_route(8, 64, 64, 64, 64, 64, 64, 64, 7, buf, 4) == -1


def test_pitch_rule_of_the_call_is_the_querys_rule():
    """bf16 with N % 8 == 0 moves 16-byte chunks of C / R / H rows: pitches that are not multiples of 8 are refused by the check clhip_gemm_nt and the query share
    (asked through the query: no pointer, no device); fp32 and bf16 with N % 8 == 4 keep % 4"""
    L = _lib.lib()
    buf = (C.c_int * 16)()
    for ldc, ldr, ldh in ((68, 64, 64), (64, 68, 64), (64, 64, 68)):
        assert L.clhip_gemm_nt_route(8, 64, 64, 64, 64, ldc, ldr, ldh, _lib.BF16, buf, 4) == -1
        assert b"% 8 == 0" in L.clhip_last_error(), (ldc, ldr, ldh)
        assert L.clhip_gemm_nt_route(8, 64, 64, 64, 64, ldc, ldr, ldh, _lib.F32, buf, 4) == 1
        assert L.clhip_gemm_nt_route(8, 12, 64, 64, 64, ldc - 48, ldr - 48, ldh - 48, _lib.BF16, buf, 4) == 1          # N = 12, pitches 16 / 20
    for ldc, ldr, ldh in ((66, 64, 64), (64, 66, 64), (64, 64, 66)):
        assert L.clhip_gemm_nt_route(8, 64, 64, 64, 64, ldc, ldr, ldh, _lib.F32, buf, 4) == -1
        assert b"% 4" in L.clhip_last_error()
