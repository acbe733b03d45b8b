"""clhip_gemm_nt (csrc/gemm.hip, csrc/gemm8.hip) against the fp64 reference and the per-element bound of tests/gemm_ref.py, on every route
clhip_gemm_nt_route names (tests/test_gemm_ref_cpu.py proves the case list reaches all of them) and always "in windows":

  * A, B, bias, C, R and H live inside larger buffers: lda = K + 8, ldb = K + 16, ldc = N + 16, ldr = N + 24, ldh = N + 32 (gemm_ref.pitches), the A / C / R / H
    windows start 8 / 8 / 16 / 24 elements into a row, one guard row lies in front of and one behind every window.  The three output-side pitches differ from
    each other and from N: a swapped pitch, or N used as one, lands elsewhere.
  * C and H windows are pre-filled with one NaN bit pattern, everything around them (and around the inputs) with a second one.
  * after the call: every element of the window within its own bound (nothing is judged by a norm, nothing is left out), every byte outside the window
    bit-identical to the pre-fill, a second call gives the same bits, epilogue 3 with H = NULL gives C the bits of the call with H.

Every check prints `[ratio] name: max |err| / bound` (per block of 2048 rows for the large shapes); epilogue 3 prints `[measure] c_g ...`, the largest
(|err| - other terms) / max(1, |x|), from which gemm_ref.C_G_MEASURED is entered."""
import math

import pytest
import torch

import gemm_ref as G

pytestmark = pytest.mark.gpu

from libcontinual_amd import _lib           # noqa: E402

DEV = "cuda"
TD = {"bf16": torch.bfloat16, "f32": torch.float32}
TI = {"bf16": torch.int16, "f32": torch.int32}
CODE = {"bf16": _lib.BF16, "f32": _lib.F32}
NAN_WIN = {"bf16": 0x7FC1, "f32": 0x7FC00001}           # unwritten output
NAN_OUT = {"bf16": 0x7FA5, "f32": 0x7FA00005}           # everything outside a window
BLOCK = 2048


def st():
    return torch.cuda.current_stream().cuda_stream


class Win:
    """a [rows, cols] window at column `off` of a [rows + 2, ld] buffer (row 0 and row rows + 1 are guards)"""

    def __init__(self, rows, cols, ld, off, dt, values=None):
        assert off + cols <= ld
        self.rows, self.cols, self.ld, self.off, self.dt = rows, cols, ld, off, dt
        self.buf = torch.empty((rows + 2) * ld, device=DEV, dtype=TD[dt])
        self.buf.view(TI[dt]).fill_(NAN_OUT[dt])
        self.win = self.buf.view(rows + 2, ld)[1:1 + rows, off:off + cols]
        if values is None:
            self.win.view(TI[dt]).fill_(NAN_WIN[dt])
        else:
            self.win.copy_(values)
        self.ptr = self.buf.data_ptr() + (ld + off) * self.buf.element_size()
        self.before = self.buf.view(TI[dt]).clone()

    def bits(self):
        return self.win.view(TI[self.dt]).clone()

    def outside_untouched(self):
        now = self.buf.view(TI[self.dt]).clone().view(self.rows + 2, self.ld)
        was = self.before.clone().view(self.rows + 2, self.ld)
        now[1:1 + self.rows, self.off:self.off + self.cols] = 0
        was[1:1 + self.rows, self.off:self.off + self.cols] = 0
        return torch.equal(now, was)

    def unchanged(self):
        return torch.equal(self.buf.view(TI[self.dt]), self.before)


def rnd(shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV) * scale


class Operands:
    """the inputs of one case (shared by its epilogues) with the fp64 product and S = |A| |B|^T on the device"""

    def __init__(self, dt, M, N, K, A=None, B=None, bias=None, R=None, H=None, ld=None):
        self.dt, self.M, self.N, self.K = dt, M, N, K
        td = TD[dt]
        self.ld = ld or G.pitches(N, K)
        self.A = (rnd((M, K), 1) if A is None else A.to(DEV)).to(td)
        self.B = (rnd((N, K), 2, 1 / math.sqrt(K)) if B is None else B.to(DEV)).to(td)
        self.bias = (rnd((N,), 3) if bias is None else bias.to(DEV)).float()
        self.R = (rnd((M, N), 4) if R is None else R.to(DEV)).to(td)
        self.H = (rnd((M, N), 5) if H is None else H.to(DEV)).to(td)
        self.P = self.A.double() @ self.B.double().T
        self.S = G.abs_prod(self.A, self.B)
        l = self.ld
        self.wA = Win(M, K, l["lda"], l["offa"], dt, self.A)
        self.wB = Win(N, K, l["ldb"], 0, dt, self.B)
        self.wbias = Win(1, N, N + 16, 8, "f32", self.bias[None, :])
        self.wR = Win(M, N, l["ldr"], l["offr"], dt, self.R)
        self.wH = Win(M, N, l["ldh"], l["offh"], dt, self.H)


def gemm(op, epi, wC, wH, stream=None):
    """one clhip_gemm_nt call of the case into the windows wC (and wH: output of epilogue 3, input of 4, else unused); returns the error code"""
    l = op.ld
    return _lib.lib().clhip_gemm_nt(op.wA.ptr, op.wB.ptr, wC.ptr, op.wbias.ptr if epi in (1, 2, 3) else None, op.wR.ptr if epi == 2 else None,
                                    wH.ptr if wH is not None else None, op.M, op.N, op.K, l["lda"], l["ldb"], l["ldc"], l["ldr"], l["ldh"], epi, CODE[op.dt],
                                    st() if stream is None else stream)


def judge(name, got, ref, allowed, fails):
    """every element against its own bound; the worst ratio per block of 2048 rows is printed"""
    err = (got.double() - ref).abs()
    bad = ~(err <= allowed)                                  # NaN (an unwritten element) is bad
    ratio = torch.nan_to_num(err / allowed.clamp(min=1e-300), nan=float("inf"))
    rows = ratio.amax(dim=1)
    worst = [float(rows[lo:lo + BLOCK].max()) for lo in range(0, rows.numel(), BLOCK)]
    print(f"[ratio] {name}: " + " ".join(f"{w:.3g}" for w in worst))
    if int(bad.sum()) != 0:
        i = int(torch.nan_to_num(ratio, posinf=3e38).argmax())
        fails.append(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside their bound, worst at row {i // got.shape[1]} col {i % got.shape[1]}: "
                     f"got {float(got.reshape(-1)[i])} ref {float(ref.reshape(-1)[i])} allowed {float(allowed.reshape(-1)[i]):.3g}")


def run_epilogue(name, op, epi, fails, stream=None):
    """the driver: one epilogue of one case in windows; returns the bits of C (and H of epilogue 3)"""
    dt, M, N, K, l = op.dt, op.M, op.N, op.K, op.ld
    name = f"{name} epi {epi}"
    pre, cref, href = G.gemm_ref(op.A, op.B, op.bias, op.R, op.H, epi, prod=op.P)
    bc, bh = G.gemm_bound(op.S, K, pre, cref, href, op.H, epi, dt)
    outs = []
    for _ in range(2):
        wC = Win(M, N, l["ldc"], l["offc"], dt)
        wH = Win(M, N, l["ldh"], l["offh"], dt) if epi == 3 else (op.wH if epi == 4 else None)
        rc = gemm(op, epi, wC, wH, stream)
        torch.cuda.synchronize()
        assert rc == 0, (name, rc, _lib.lib().clhip_last_error())
        outs.append((wC, wH))
    wC, wH = outs[0]
    judge(name + " C", wC.win, cref, bc, fails)
    if epi == 3:
        judge(name + " H", wH.win, href, bh, fails)
        oc, oh = G.other_terms(op.S, K, pre, cref, href, op.H, epi, dt)
        scale = pre.abs().clamp(min=1.0)
        m = max(float((((wC.win.double() - cref).abs() - oc) / scale).max()), float((((wH.win.double() - href).abs() - oh) / scale).max()))
        print(f"[measure] c_g {name}: {m:.4g}")
    for w, what in ((wC, "C"), (outs[1][0], "C of the second call")) + (((wH, "H"), (outs[1][1], "H of the second call")) if epi == 3 else ()):
        if not w.outside_untouched():
            fails.append(f"{name}: bytes outside the {what} window changed")
    for w, what in ((op.wA, "A"), (op.wB, "B"), (op.wbias, "bias"), (op.wR, "R"), (op.wH, "H input")):
        if not w.unchanged():
            fails.append(f"{name}: the {what} buffer changed")
    if not torch.equal(wC.bits(), outs[1][0].bits()):
        fails.append(f"{name}: a second call gave other bits in C")
    if epi == 3:
        if not torch.equal(wH.bits(), outs[1][1].bits()):
            fails.append(f"{name}: a second call gave other bits in H")
        wC0 = Win(M, N, l["ldc"], l["offc"], dt)
        rc = gemm(op, epi, wC0, None, stream)
        torch.cuda.synchronize()
        assert rc == 0, (name, rc)
        if not (torch.equal(wC0.bits(), wC.bits()) and wC0.outside_untouched()):
            fails.append(f"{name}: H = NULL gave other bits in C (or wrote outside it)")
    return wC.bits(), (wH.bits() if epi == 3 else None)


def run_case(case, **operands):
    L = _lib.lib()
    L.clhip_gemm8_config(case["mode"])
    try:
        op = Operands(case["dt"], case["M"], case["N"], case["K"], **operands)
        fails = []
        for epi in case["epis"]:
            run_epilogue(case["name"], op, epi, fails)
        assert not fails, "\n".join(fails)
    finally:
        L.clhip_gemm8_config(-1)


@pytest.mark.parametrize("case", G.CASES, ids=[c["name"] for c in G.CASES])
def test_gemm_in_windows(case):
    """every kernel family, both exits of the bf16 register-staged kernel (through LDS: N % 8 == 0; direct: N % 8 == 4), both head + tail splits, gemm8 alone and with
    a register-staged tail; M = 1, M < 64, N below one tile, KT = 2, a split-K request that falls back (49 K steps)"""
    run_case(case)


def test_gemm_two_half_windows_of_one_buffer():
    """the U product of csrc/sdlora.hip: two calls with lda = 3 D, K = D = 64, N = 16, ldc = 32 fill the two halves of one [M, 32] buffer from two column windows
    of one [M, 3 D] buffer and the two row halves of one [32, D] B.  The first half's bits survive the second call."""
    case = G.SDLORA_CASE
    M, N, K, dt = case["M"], case["N"], case["K"], case["dt"]
    X = rnd((M, 3 * K), 1).to(TD[dt])
    Bc = rnd((2 * N, K), 2, 1 / math.sqrt(K)).to(TD[dt])
    wX = Win(M, 3 * K, 3 * K, 0, dt, X)
    wB = Win(2 * N, K, K, 0, dt, Bc)
    wU = Win(M, 2 * N, 2 * N, 0, dt)
    es = 2
    fails = []
    first = None
    for half in range(2):
        rc = _lib.lib().clhip_gemm_nt(wX.ptr + half * 2 * K * es, wB.ptr + half * N * K * es, wU.ptr + half * N * es, None, None, None, M, N, K, 3 * K, K, 2 * N, 0, 0, 0,
                                      CODE[dt], st())
        torch.cuda.synchronize()
        assert rc == 0, (rc, _lib.lib().clhip_last_error())
        A, B = X[:, half * 2 * K:half * 2 * K + K], Bc[half * N:(half + 1) * N]
        _, cref, _ = G.gemm_ref(A, B, None, None, None, 0)
        bc, _ = G.gemm_bound(G.abs_prod(A, B), K, cref, cref, None, None, 0, dt)
        judge(f"{case['name']} half {half}", wU.win[:, half * N:(half + 1) * N], cref, bc, fails)
        if half == 0:
            first = wU.bits()[:, :N]
            assert bool((wU.bits()[:, N:] == NAN_WIN[dt]).all()), "the first call wrote into the second half"
        else:
            assert torch.equal(wU.bits()[:, :N], first), "the second call changed the first half"
    assert wU.outside_untouched() and wX.unchanged() and wB.unchanged()
    assert not fails, "\n".join(fails)


def test_gemm_split_k_in_windows_scratch_grows_and_is_reused():
    """2, 3 and 4 K slices with ldc != N (the partials are pitched by N, their epilogue by ldc), on a stream of the test's own so that this test sees the scratch
    being created (small), reused (smaller), outgrown (large), reused and reused again by the first shape, whose bits must not have changed"""
    stream = torch.cuda.Stream()
    by_name = {c["name"]: c for c in G.SPLITK_CASES}
    order = ["splitk4-130x256", "splitk4-1x4", "splitk2-3552x1024", "splitk3-3552x768", "splitk4-130x256"]
    fails, first = [], None
    with torch.cuda.stream(stream):
        for i, nm in enumerate(order):
            case = by_name[nm]
            op = Operands(case["dt"], case["M"], case["N"], case["K"])
            bits = [run_epilogue(f"{nm} call {i}", op, epi, fails, stream.cuda_stream) for epi in case["epis"]]
            if i == 0:
                first = bits
            if i == len(order) - 1:
                for epi, (a, b) in zip(case["epis"], zip(first, bits)):
                    if not (torch.equal(a[0], b[0]) and (a[1] is None or torch.equal(a[1], b[1]))):
                        fails.append(f"{nm} epi {epi}: other bits after the scratch was outgrown and reused")
    torch.cuda.synchronize()
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ controlled pre-activations
def grid_values(n):
    """n bf16 values over [-12, 12]: +-0, +-2^-20, the bf16 neighbours of the extrema of gelu' at +-sqrt 2 and of |x| = 5 (where the old tests' data ended), the ends,
    and an even grid in between"""
    special = [0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 12.0, -12.0]
    for c in (2 ** 0.5, 5.0, 0.7517916, 3.0):          # gelu' extrema; |x| = 5; gelu's own minimum at -0.7518; gelu'' changes sign again near 3
        b = float(torch.tensor(c).bfloat16())
        special += [s * (b + k * 2.0 ** -7 * (4 if c >= 4 else 2 if c >= 2 else 1 if c >= 1 else 0.5)) for k in (-1, 0, 1) for s in (1.0, -1.0)]
    sp = torch.tensor(special, dtype=torch.float32)
    assert n > sp.numel()
    return torch.cat([sp, torch.linspace(-12, 12, n - sp.numel())]).bfloat16().float()


CONTROLLED = [("bf16", 130, 72, 64, -1), ("bf16", 130, 36, 64, -1), ("f32", 130, 72, 64, -1), ("f32", 130, 36, 64, -1), ("bf16", 300, 256, 256, 2)]


@pytest.mark.parametrize("dt,M,N,K,mode", CONTROLLED, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" + ("-gemm8" if c[4] == 2 else "") for c in CONTROLLED])
def test_gelu_epilogues_on_controlled_preactivations(dt, M, N, K, mode):
    """A has one 1 per row and bias = 0: the pre-activation of row m is exactly column m % K of B, and B holds a bf16 grid over [-12, 12].  The product is exact, so
    epilogues 3 and 4 are judged at their output rounding + the erf term alone: GELU and GELU' beyond |x| = 5, at +-0, at +-2^-20 and around their extrema."""
    A = torch.zeros(M, K)
    A[torch.arange(M), torch.arange(M) % K] = 1.0
    B = grid_values(N * K).reshape(N, K)
    x = A.double() @ B.double().T
    _, h = G.gelu_both(x)
    case = dict(name=f"controlled {dt} {M}x{N}x{K}", dt=dt, M=M, N=N, K=K, mode=mode, epis=(3, 4))
    run_case(case, A=A, B=B, bias=torch.zeros(N), H=h.to(TD[dt]))


# ------------------------------------------------------------------------------------------------ argument checks
def _reject_base():
    return dict(M=8, N=64, K=64, lda=64, ldb=64, ldc=64, ldr=64, ldh=64, epi=0, dt="bf16", bias=True, R=True, H=True)


REJECTED = [
    ("K = 96", dict(K=96, lda=96, ldb=96), "K % 64"),
    ("N = 6", dict(N=6), "N % 4"),
    ("lda = K + 4", dict(lda=68), "lda % 8"),
    ("ldc = N + 2", dict(ldc=66), "ldc % 4"),
    ("NULL bias, epilogue 1", dict(epi=1, bias=False), "bias != nullptr"),
    ("NULL bias, epilogue 2", dict(epi=2, bias=False), "bias != nullptr"),
    ("NULL bias, epilogue 3", dict(epi=3, bias=False), "bias != nullptr"),
    ("NULL R, epilogue 2", dict(epi=2, R=False), "R != nullptr"),
    ("NULL H, epilogue 4", dict(epi=4, H=False), "H != nullptr"),
    ("ldh = N + 2 with H", dict(epi=3, ldh=66), "ldh % 4"),
    ("epilogue 5", dict(epi=5), "unknown epilogue 5"),
    ("dtype 7", dict(dt=7), "dtype =="),
    ("M = 0", dict(M=0), "M > 0"),
    ("bf16, N = 64, ldc = 68", dict(ldc=68), "% 8 == 0"),
    ("bf16, N = 64, ldr = 68 with R", dict(epi=2, ldr=68), "% 8 == 0"),
    ("bf16, N = 64, ldh = 68 with H", dict(epi=4, ldh=68), "% 8 == 0"),
]


@pytest.mark.parametrize("what,change,msg", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_arguments_leave_c_alone(what, change, msg):
    a = {**_reject_base(), **change}
    L = _lib.lib()
    big = 16 * 128
    A = torch.ones(big, device=DEV, dtype=torch.bfloat16)
    B = torch.ones(big, device=DEV, dtype=torch.bfloat16)
    bias = torch.zeros(128, device=DEV)
    R = torch.ones(big, device=DEV, dtype=torch.bfloat16)
    H = torch.ones(big, device=DEV, dtype=torch.bfloat16)
    Cc = torch.empty(big, device=DEV, dtype=torch.bfloat16)
    Cc.view(torch.int16).fill_(NAN_WIN["bf16"])
    L.clhip_gemm_nt(A.data_ptr(), B.data_ptr(), Cc.data_ptr(), None, None, None, 8, 64, 32, 32, 32, 64, 64, 64, 0, _lib.BF16, st())      # K = 32: sets another message
    assert b"K % 64" in L.clhip_last_error()
    if "K % 64" in msg:
        L.clhip_gemm_nt(A.data_ptr(), B.data_ptr(), Cc.data_ptr(), None, None, None, 8, 6, 64, 64, 64, 64, 64, 64, 0, _lib.BF16, st())
        assert b"N % 4" in L.clhip_last_error()
    rc = L.clhip_gemm_nt(A.data_ptr(), B.data_ptr(), Cc.data_ptr(), bias.data_ptr() if a["bias"] else None, R.data_ptr() if a["R"] else None, H.data_ptr() if a["H"] else None,
                         a["M"], a["N"], a["K"], a["lda"], a["ldb"], a["ldc"], a["ldr"], a["ldh"], a["epi"], CODE.get(a["dt"], a["dt"]), st())
    torch.cuda.synchronize()
    assert rc == -1, (what, rc)
    assert msg.encode() in L.clhip_last_error(), (what, L.clhip_last_error())
    assert bool((Cc.view(torch.int16) == NAN_WIN["bf16"]).all()), what
    assert bool((H == 1).all()) and bool((R == 1).all())


@pytest.mark.parametrize("dt,N", [("f32", 64), ("bf16", 12), ("bf16", 36)])
def test_pitches_of_4_mod_8_that_stay_legal_are_correct(dt, N):
    """the counterparts of the refused bf16 / N % 8 == 0 pitch: fp32 rows of ld % 4 == 0 are 16-byte aligned, bf16 with N % 8 == 4 stores 8 bytes at a time"""
    M, K = 70, 64
    c, r, h = (4, 12, 20) if N % 8 == 0 else (8, 16, 24)
    ld = dict(lda=K + 8, ldb=K + 16, ldc=N + c, ldr=N + r, ldh=N + h, offa=8, offc=4, offr=8, offh=12)
    assert all(ld[k] % 8 == 4 for k in ("ldc", "ldr", "ldh"))
    run_case(dict(name=f"pitch 4 mod 8 {dt} N {N}", dt=dt, M=M, N=N, K=K, mode=-1, epis=(0, 1, 2, 3, 4)), ld=ld)
