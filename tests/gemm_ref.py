"""fp64 reference and per-element error bound of clhip_gemm_nt (csrc/gemm.hip, csrc/gemm8.hip): C = epi(A . B^T).

The reference works on the operands as the kernel sees them (already rounded to bf16 in the bf16 mode) and returns the fp64
pre-activation x = A . B^T (+ bias) (+ R), the fp64 C and, for epilogue 3, the fp64 H = gelu'(x) = Phi(x) + x phi(x).  Phi comes from
erfc (Phi(x) = erfc(-x / sqrt 2) / 2), so the negative tail keeps its relative accuracy where 0.5 (1 + erf) cancels to nothing.

The bound of one element, in fp64, from S = |A| . |B|^T:
  accumulation   (K + 8) 2^-24 S     any summation order of K fp32 products (MFMA blocks, split-K slices summed afterwards) is within
                                     (K - 1) u S to first order, u = 2^-24; the 8 spare units carry the second-order terms and the bias / residual adds
  output         2^-8 |ref| (bf16: the figure the project's test headers use), 2^-23 |ref| (fp32)
  epilogue 4     C = x H with the stored H: both terms times |H|
  epilogue 3     the accumulation term reaches C through |gelu'| <= 1.13 and H through |gelu''| <= 1 (sup |gelu''| = gelu''(0) = 2 phi(0) = 0.798), plus the
                 absolute term C_G max(1, |x|) for the erf approximation of the kernel (Abramowitz-Stegun 7.1.26: 0.75e-7 on Phi; the shares of
                 the hardware exp and reciprocal are not derivable and are measured).
Every element of every case is judged; nothing is left out.

C_G: four times the largest (|err| - other terms) / max(1, |x|) that tests/test_gemm_kernels_gpu.py printed as `[measure]` on an MI355X
against this reference, rounded up to a power of two, never below the floor 2^-20 (about 6 x the 1.5e-7 of the erf formula)."""
import math

import torch

U24 = 2.0 ** -24
OUT_EPS = {"bf16": 2.0 ** -8, "f32": 2.0 ** -23}
GELU_D1_MAX = 1.13          # sup |gelu'| = 1.1289 at x = +1.4142...
GELU_D2_MAX = 1.0           # sup |gelu''| = 0.7979 at x = 0
C_G_FLOOR = 2.0 ** -20
C_G_MEASURED = 3.586e-08    # largest [measure] value of the GPU file on an MI355X (controlled f32 130x72x64, epilogue 3); 4 x = 1.4e-7 -> 2^-22, below the floor: the floor decides


def c_g():
    if C_G_MEASURED is None or C_G_MEASURED <= 0:
        return C_G_FLOOR
    return max(C_G_FLOOR, 2.0 ** math.ceil(math.log2(4.0 * C_G_MEASURED)))


def gelu_both(x):
    """fp64 gelu(x) = x Phi(x) and gelu'(x) = Phi(x) + x phi(x)"""
    x = x.double()
    Phi = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
    phi = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return x * Phi, Phi + x * phi


def gemm_ref(A, B, bias, R, H, epi, prod=None):
    """(pre-activation, C, H of epilogue 3 or None), all fp64 on the operands' device.  `prod` = a precomputed fp64 A . B^T."""
    x = A.double() @ B.double().T if prod is None else prod.clone()
    if epi in (1, 2, 3):
        x = x + bias.double()
    if epi == 2:
        x = x + R.double()
    if epi == 3:
        c, h = gelu_both(x)
        return x, c, h
    if epi == 4:
        return x, x * H.double(), None
    return x, x, None


def abs_prod(A, B):
    """S = |A| . |B|^T in fp64"""
    return A.double().abs() @ B.double().abs().T


def other_terms(S, K, pre, Cref, Href, H, epi, dt):
    """the bound without the C_G term: (for C, for H of epilogue 3 or None)"""
    acc = (K + 8) * U24 * S
    eps = OUT_EPS[dt]
    if epi == 3:
        return GELU_D1_MAX * acc + eps * Cref.abs(), GELU_D2_MAX * acc + eps * Href.abs()
    if epi == 4:
        return (acc + eps * pre.abs()) * H.double().abs(), None
    return acc + eps * Cref.abs(), None


def gemm_bound(S, K, pre, Cref, Href, H, epi, dt):
    """allowed |got - ref| per element: (for C, for H of epilogue 3 or None)"""
    bc, bh = other_terms(S, K, pre, Cref, Href, H, epi, dt)
    if epi == 3:
        g = c_g() * pre.abs().clamp(min=1.0)
        return bc + g, bh + g
    return bc, None


# ------------------------------------------------------------------------------------------------ the cases of the GPU file and their routes
GEMM8, T256, T160, T128, T64, F32_128 = 1, 2, 3, 4, 5, 6          # kernel families of clhip_gemm_nt_route (include/clhip.h)


def pitches(N, K):
    """the windows of tests/test_gemm_kernels_gpu.py: row pitches (all different from K / N and from each other) and the element offsets of the A / C / R / H
    windows inside their rows.  ldc < ldh, so a store to H with C's pitch stays inside the H buffer."""
    return dict(lda=K + 8, ldb=K + 16, ldc=N + 16, ldr=N + 24, ldh=N + 32, offa=8, offc=8, offr=16, offh=24)


def _c(name, dt, M, N, K, route, mode=-1, epis=(0, 1, 2, 3, 4)):
    return dict(name=name, dt=dt, M=M, N=N, K=K, route=route, mode=mode, epis=epis)


# route = the launches clhip_gemm_nt_route reports: (family, first row, rows, K slices); mode = clhip_gemm8_config around the call (-1: the default)
CASES = [
    _c("f32-1x4", "f32", 1, 4, 64, [(F32_128, 0, 1, 1)]),
    _c("f32-ragged", "f32", 129, 132, 128, [(F32_128, 0, 129, 1)]),
    _c("f32-300x192", "f32", 300, 192, 64, [(F32_128, 0, 300, 1)]),
    _c("64-direct-1x4", "bf16", 1, 4, 64, [(T64, 0, 1, 1)]),
    _c("64-direct-63x12", "bf16", 63, 12, 128, [(T64, 0, 63, 1)]),
    _c("64-direct-130x36", "bf16", 130, 36, 64, [(T64, 0, 130, 1)]),
    _c("64-direct-splitk-refused", "bf16", 5, 12, 3136, [(T64, 0, 5, 1)]),          # 49 K steps: no slice count divides them
    _c("64-staged-1x8", "bf16", 1, 8, 64, [(T64, 0, 1, 1)]),
    _c("64-staged-65x72", "bf16", 65, 72, 128, [(T64, 0, 65, 1)]),
    _c("64-staged-77x64", "bf16", 77, 64, 192, [(T64, 0, 77, 1)]),
    _c("64-staged-591x32", "bf16", 591, 32, 64, [(T64, 0, 591, 1)]),
    _c("128-staged", "bf16", 2041, 2040, 64, [(T128, 0, 2041, 1)]),
    _c("128-direct", "bf16", 2041, 2044, 64, [(T128, 0, 2041, 1)]),
    _c("160-staged", "bf16", 5000, 2040, 64, [(T160, 0, 5000, 1)]),
    _c("160-direct", "bf16", 5000, 2044, 64, [(T160, 0, 5000, 1)]),
    _c("256-three-rounds", "bf16", 12288, 4096, 64, [(T256, 0, 12288, 1)], mode=0, epis=(0, 2, 3, 4)),
    _c("256-whole-rounds-tail", "bf16", 14000, 4096, 64, [(T256, 0, 12288, 1), (T128, 12288, 1712, 1)], mode=0, epis=(0, 2, 3, 4)),
    _c("256-one-round-tail", "bf16", 16400, 1024, 2304, [(T256, 0, 16384, 1), (T64, 16384, 16, 1)], mode=0, epis=(0, 2, 3, 4)),
    _c("gemm8-300x256", "bf16", 300, 256, 256, [(GEMM8, 0, 300, 1)], mode=2),
    _c("gemm8-1000x512", "bf16", 1000, 512, 384, [(GEMM8, 0, 1000, 1)], mode=2),
    _c("gemm8-513x768", "bf16", 513, 768, 768, [(GEMM8, 0, 513, 1)], mode=2),
    # mode 1 hands gemm8 whole rounds only from 24 (rounds x K tiles) on: K = 256 of test_gemm8_whole_rounds_and_a_register_staged_tail is all small tiles today
    _c("gemm8-rounds-tail", "bf16", 256 * 86 + 100, 768, 1536, [(GEMM8, 0, 256 * 85, 1), (T64, 256 * 85, 356, 1)], mode=1),
]
# split-K (2-4 slices of 128 x 128 tiles + the reduce / epilogue pass), run in this order on one stream of the test's own: the scratch grows, then is reused
SPLITK_CASES = [
    _c("splitk4-130x256", "bf16", 130, 256, 4096, [(T128, 0, 130, 4)]),
    _c("splitk4-1x4", "bf16", 1, 4, 3072, [(T128, 0, 1, 4)]),
    _c("splitk3-3552x768", "bf16", 3552, 768, 3072, [(T128, 0, 3552, 3)]),
    _c("splitk2-3552x1024", "bf16", 3552, 1024, 3072, [(T128, 0, 3552, 2)]),
]
# the two half-windows of one [591, 32] buffer, A = two column windows of one [591, 192] buffer (csrc/sdlora.hip, the U product)
SDLORA_CASE = _c("64-staged-sdlora-halves", "bf16", 591, 16, 64, [(T64, 0, 591, 1)])
