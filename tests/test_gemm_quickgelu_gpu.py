"""Epilogue 6 of clhip_gemm_nt (CLIP's QuickGELU: C <- x s, H <- s (1 + 1.702 x (1 - s)), s = sigmoid(1.702 x)) and epilogue 4 on the H it stored, against
the fp64 reference and the per-element bound of tests/clip_ref.py, on every route of tests/gemm_ref.py's case list (split-K included) and in the windows of
tests/test_gemm_kernels_gpu.py: pitched buffers with guard rows, NaN pre-fills, every byte outside a window unchanged, a second call with the same bits, and
H = NULL giving C the bits of the call with H.  Every element is judged within its own bound.

`[measure] c_q` = the largest (|err| - other terms) / max(1, |x|): clip_ref.C_Q_MEASURED is entered from it.

The issue that asked for this epilogue numbered it 5; tests/test_gemm_kernels_gpu.py pins `epilogue 5` as a refused argument, so it is 6 and 5 stays refused
(checked below)."""
import ctypes

import pytest
import torch

import clip_ref as R
import gemm_ref as G

pytestmark = pytest.mark.gpu

from libcontinual_amd import _lib           # noqa: E402
from test_gemm_kernels_gpu import CODE, DEV, TD, Operands, Win, judge, st          # noqa: E402  (helpers only: no test of that file is collected here)

EPI = R.QGELU_EPI


def _call(op, epi, wC, wH, stream=None):
    l = op.ld
    return _lib.lib().clhip_gemm_nt(op.wA.ptr, op.wB.ptr, wC.ptr, op.wbias.ptr if epi == EPI else None, None, wH.ptr if wH is not None else None, op.M, op.N, op.K,
                                    l["lda"], l["ldb"], l["ldc"], l["ldr"], l["ldh"], epi, CODE[op.dt], st() if stream is None else stream)


def run_pair(name, op, fails, stream=None):
    """epilogue 6 into fresh C / H windows (twice, and once with H = NULL), then epilogue 4 with the H window it wrote; returns the bits of C, H and C of epilogue 4"""
    dt, M, N, K, l = op.dt, op.M, op.N, op.K, op.ld
    pre, cref, href = R.qgelu_ref(op.A, op.B, op.bias, prod=op.P)
    bc, bh = R.qgelu_bound(op.S, K, pre, cref, href, dt)
    outs = []
    for _ in range(2):
        wC, wH = Win(M, N, l["ldc"], l["offc"], dt), Win(M, N, l["ldh"], l["offh"], dt)
        rc = _call(op, EPI, wC, wH, stream)
        torch.cuda.synchronize()
        assert rc == 0, (name, rc, _lib.lib().clhip_last_error())
        outs.append((wC, wH))
    wC, wH = outs[0]
    judge(f"{name} epi {EPI} C", wC.win, cref, bc, fails)
    judge(f"{name} epi {EPI} H", wH.win, href, bh, fails)
    oc, oh = R.qgelu_other_terms(op.S, K, cref, href, dt)
    scale = pre.abs().clamp(min=1.0)
    m = max(float((((wC.win.double() - cref).abs() - oc) / scale).max()), float((((wH.win.double() - href).abs() - oh) / scale).max()))
    print(f"[measure] c_q {name} {dt} {M}x{N}x{K}: {m:.4g}")
    for w, what in ((wC, "C"), (wH, "H"), (outs[1][0], "C of the second call"), (outs[1][1], "H of the second call")):
        if not w.outside_untouched():
            fails.append(f"{name}: bytes outside the {what} window changed")
    if not (torch.equal(wC.bits(), outs[1][0].bits()) and torch.equal(wH.bits(), outs[1][1].bits())):
        fails.append(f"{name}: a second call gave other bits")
    wC0 = Win(M, N, l["ldc"], l["offc"], dt)
    rc = _call(op, EPI, wC0, None, stream)
    torch.cuda.synchronize()
    assert rc == 0, (name, rc)
    if not (torch.equal(wC0.bits(), wC.bits()) and wC0.outside_untouched()):
        fails.append(f"{name}: H = NULL gave other bits in C (or wrote outside it)")
    # the backward: epilogue 4 multiplies by the H that epilogue 6 stored (the window itself, at its pitch)
    hbits = wH.bits()
    Hs = wH.win.clone()
    _, c4ref, _ = G.gemm_ref(op.A, op.B, None, None, Hs, 4, prod=op.P)
    b4, _ = G.gemm_bound(op.S, K, op.P, c4ref, None, Hs, 4, dt)
    wC4 = Win(M, N, l["ldc"], l["offc"], dt)
    rc = _call(op, 4, wC4, wH, stream)
    torch.cuda.synchronize()
    assert rc == 0, (name, rc, _lib.lib().clhip_last_error())
    judge(f"{name} epi 4 on H C", wC4.win, c4ref, b4, fails)
    if not (wC4.outside_untouched() and torch.equal(wH.bits(), hbits) and wH.outside_untouched()):
        fails.append(f"{name}: epilogue 4 wrote outside C or into H")
    for w, what in ((op.wA, "A"), (op.wB, "B"), (op.wbias, "bias")):
        if not w.unchanged():
            fails.append(f"{name}: the {what} buffer changed")
    return wC.bits(), hbits, wC4.bits()


def run_case(case, **operands):
    L = _lib.lib()
    L.clhip_gemm8_config(case["mode"])
    try:
        ld = G.pitches(case["N"], case["K"])
        got = (ctypes.c_int * 12)()
        n = L.clhip_gemm_nt_route(case["M"], case["N"], case["K"], ld["lda"], ld["ldb"], ld["ldc"], ld["ldr"], ld["ldh"], CODE[case["dt"]], got, 3)
        if "route" in case:
            assert [tuple(got[4 * i:4 * i + 4]) for i in range(n)] == case["route"], case["name"]
        op = Operands(case["dt"], case["M"], case["N"], case["K"], **operands)
        fails = []
        run_pair(case["name"], op, fails)
        assert not fails, "\n".join(fails)
    finally:
        L.clhip_gemm8_config(-1)


@pytest.mark.parametrize("case", G.CASES, ids=[c["name"] for c in G.CASES])
def test_quickgelu_on_every_route(case):
    """gemm8, the register-staged 256 / 160 / 128 / 64 tiles through both exits (LDS-staged: N % 8 == 0; direct: N % 8 == 4), the head + tail splits and the fp32
    parity kernel; the route of every case is asserted before it runs"""
    run_case(case)


def test_quickgelu_split_k_scratch_grows_and_is_reused():
    """the reduce / epilogue pass of 2, 3 and 4 K slices, in the order that makes the scratch grow and be reused; the first shape's bits must come back"""
    stream = torch.cuda.Stream()
    by_name = {c["name"]: c for c in G.SPLITK_CASES}
    order = ["splitk4-130x256", "splitk4-1x4", "splitk2-3552x1024", "splitk3-3552x768", "splitk4-130x256"]
    fails, first = [], None
    with torch.cuda.stream(stream):
        for i, nm in enumerate(order):
            case = by_name[nm]
            op = Operands(case["dt"], case["M"], case["N"], case["K"])
            bits = run_pair(f"{nm} call {i}", op, fails, stream.cuda_stream)
            if i == 0:
                first = bits
            if i == len(order) - 1 and not all(torch.equal(a, b) for a, b in zip(first, bits)):
                fails.append(f"{nm}: other bits after the scratch was outgrown and reused")
    torch.cuda.synchronize()
    assert not fails, "\n".join(fails)


def grid_values(n, dt):
    """n values in the case's dtype: +-0, +-2^-20, the neighbours of 1 / 1.702 (1.702 x = 1), of the extremum of q' (1.702 x = 2.3994), of |x| = 20 (1 - s = e^-34: far below one
    ulp of s), of |x| = 61 (1.702 x = 103.8: exp(-|t|) leaves the normal fp32 range) and of |x| = 100 (1.702 x = 170: exp underflows, s is exactly 0 or 1), the ends +-110, and an even grid between them"""
    td = TD[dt]
    special = [0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 110.0, -110.0]
    for c in (1 / 1.702, 2.3994 / 1.702, 20.0, 61.0, 100.0):
        b = float(torch.tensor(c).to(td))
        step = b * 2.0 ** -7
        special += [s * (b + k * step) for k in (-1, 0, 1) for s in (1.0, -1.0)]
    sp = torch.tensor(special, dtype=torch.float32)
    assert n > 2 * sp.numel()
    half = (n - sp.numel()) // 2
    return torch.cat([sp, torch.linspace(-110, 110, half), torch.linspace(-6, 6, n - sp.numel() - half)]).to(td).float()


CONTROLLED = [("bf16", 130, 72, 64, -1), ("bf16", 130, 36, 64, -1), ("f32", 130, 72, 64, -1), ("f32", 130, 36, 64, -1), ("bf16", 300, 256, 256, 2)]


@pytest.mark.parametrize("dt,M,N,K,mode", CONTROLLED, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" + ("-gemm8" if c[4] == 2 else "") for c in CONTROLLED])
def test_quickgelu_on_controlled_preactivations(dt, M, N, K, mode):
    """A has one 1 per row and bias = 0: the pre-activation of row m is exactly column m % K of B, which holds the grid above.  The product is exact, so both
    outputs are judged at their output rounding + the sigmoid term alone.  Large |x| must give finite values: C = x or -0, H = 1 or 0."""
    A = torch.zeros(M, K)
    A[torch.arange(M), torch.arange(M) % K] = 1.0
    B = grid_values(N * K, dt).reshape(N, K)
    case = dict(name=f"controlled {dt} {M}x{N}x{K}", dt=dt, M=M, N=N, K=K, mode=mode)
    run_case(case, A=A, B=B, bias=torch.zeros(N))


def test_large_preactivations_are_exact_and_finite():
    """|x| = 100 and 110 through the fp32 kernel: exp(-170) underflows, so s is exactly 1 (C = x, H = 1) or exactly 0 (C = -0, H = 0): no inf, no NaN"""
    M, N, K = 4, 4, 64
    A = torch.zeros(M, K, device=DEV)
    A[:, 0] = 1.0
    B = torch.zeros(N, K, device=DEV)
    B[:, 0] = torch.tensor([100.0, -100.0, 110.0, -110.0])
    bias = torch.zeros(N, device=DEV)
    Cc = torch.full((M, N), float("nan"), device=DEV)
    H = torch.full((M, N), float("nan"), device=DEV)
    rc = _lib.lib().clhip_gemm_nt(A.data_ptr(), B.data_ptr(), Cc.data_ptr(), bias.data_ptr(), None, H.data_ptr(), M, N, K, K, K, N, 0, N, EPI, _lib.F32, st())
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().clhip_last_error()
    assert torch.equal(Cc[0].cpu(), torch.tensor([100.0, 0.0, 110.0, 0.0])) and torch.equal(H[0].cpu(), torch.tensor([1.0, 0.0, 1.0, 0.0]))


@pytest.mark.parametrize("what,epi,bias,msg", [("NULL bias", EPI, False, "bias != nullptr"), ("epilogue 5", 5, True, "unknown epilogue 5"),
                                               ("epilogue 7", 7, True, "unknown epilogue 7")])
def test_rejected_arguments(what, epi, bias, msg):
    L = _lib.lib()
    A = torch.ones(8 * 64, device=DEV, dtype=torch.bfloat16)
    B = torch.ones(64 * 64, device=DEV, dtype=torch.bfloat16)
    b = torch.zeros(64, device=DEV)
    Cc = torch.empty(8 * 64, device=DEV, dtype=torch.bfloat16)
    Cc.view(torch.int16).fill_(0x7FC1)
    H = torch.ones(8 * 64, device=DEV, dtype=torch.bfloat16)
    rc = L.clhip_gemm_nt(A.data_ptr(), B.data_ptr(), Cc.data_ptr(), b.data_ptr() if bias else None, None, H.data_ptr(), 8, 64, 64, 64, 64, 64, 64, 64, epi, _lib.BF16, st())
    torch.cuda.synchronize()
    assert rc == -1 and msg.encode() in L.clhip_last_error(), (what, rc, L.clhip_last_error())
    assert bool((Cc.view(torch.int16) == 0x7FC1).all()) and bool((H == 1).all())
