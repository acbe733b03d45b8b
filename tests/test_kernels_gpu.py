"""Kernel-level parity on a real MI355X: every libclhip entry point against the CPU oracle (plain torch
fp32/fp64 CPU ops = the same arithmetic the reference runs) on seeded inputs.

bf16 mode: operands are rounded to bf16 first and the oracle is evaluated in fp64 on the ROUNDED operands,
so the only admissible differences are fp32 accumulation order and the final bf16 rounding of the output
(relative 2^-8 of the output magnitude).  f32 mode: rtol 2e-4 (fp32 accumulation order only)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from libcontinual_amd import _lib          # noqa: E402
from libcontinual_amd._lib import call     # noqa: E402

DEV = "cuda"
DT = {"bf16": (_lib.BF16, torch.bfloat16), "f32": (_lib.F32, torch.float32)}


def st():
    return torch.cuda.current_stream().cuda_stream


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def to_nhwc(x, tdt, cpad=None):
    """CPU NCHW fp32 -> device NHWC in `tdt`, channels zero-padded"""
    n, c, h, w = x.shape
    cpad = cpad or c
    y = torch.zeros(n, h, w, cpad)
    y[..., :c] = x.permute(0, 2, 3, 1)
    return y.to(tdt).to(DEV).contiguous()


def from_nhwc(y):
    return y.float().cpu().permute(0, 3, 1, 2).contiguous()


def quant(x, tdt):
    return x.to(tdt).float()


def tol(mode, ref):
    scale = float(ref.abs().max()) + 1e-30
    return (2 ** -7) * scale if mode == "bf16" else 2e-4 * scale


CONV_CASES = [
    # N, H, W, C, K, k, stride, pad
    (2, 8, 8, 16, 16, 3, 1, 1),
    (2, 8, 8, 16, 32, 3, 2, 1),
    (2, 8, 8, 16, 32, 1, 2, 0),
    (5, 32, 32, 16, 32, 3, 2, 1),      # CifarResNet-32 stage 2 entry: parity-class dgrad with a K-step spanning two taps
    (3, 5, 7, 32, 48, 3, 1, 1),        # ragged spatial size, K not a power of two
    (2, 6, 6, 64, 128, 3, 1, 1),
    (1, 4, 4, 256, 512, 3, 2, 1),
    (4, 16, 16, 3, 16, 3, 1, 1),       # stem: 3 channels padded to 8
    (9, 32, 32, 3, 64, 3, 1, 1),       # ... large enough for stem.hip's deterministic weight gradient (>= 2048 pixels)
    (11, 17, 13, 3, 32, 3, 1, 1),      # ... odd image, ragged last 32-pixel step
    (2, 9, 9, 128, 256, 1, 2, 0),
    (64, 32, 32, 16, 16, 3, 1, 1),     # M = 65536 -> the 128-row tile path
    (1, 1, 1, 16, 16, 3, 1, 1),        # single pixel
    (6, 16, 16, 32, 32, 3, 1, 1),      # CifarResNet-32 stage 2 (32 -> 32 channels, 16-wide images)
    # shapes served by the halo kernel (conv3.hip: 3x3 s1, channels multiple of 64), incl. ragged tiles,
    # tiles spanning several images and every workgroup shape it picks
    (8, 32, 32, 64, 64, 3, 1, 1),
    (3, 16, 16, 128, 128, 3, 1, 1),
    (5, 8, 8, 256, 256, 3, 1, 1),
    (7, 4, 4, 512, 512, 3, 1, 1),
    (2, 7, 5, 64, 64, 3, 1, 1),
    (130, 32, 32, 64, 64, 3, 1, 1),    # 512-pixel tiles (8 waves), ragged last tile
    (70, 16, 16, 128, 256, 3, 1, 1),   # 256x128 tiles
    (70, 8, 8, 256, 256, 3, 1, 1),     # enough pixels for the two-group 128-pixel tiles (fewer take the four-group 64-pixel ones)
    (130, 4, 4, 512, 512, 3, 1, 1),
    # step geometries of the LDS-DMA weight-gradient kernel (wgrad4.hip): 16 rows of an 8-wide image, four 4x8 images, two 8x4 images
    # per 128-pixel step, each with a ragged last step
    (3, 16, 8, 64, 64, 3, 1, 1),
    (5, 4, 8, 64, 128, 3, 1, 1),
    (7, 8, 4, 128, 64, 3, 1, 1),
    # ... its stride-2 and 1x1 / stride-2 forms (the layer-entry convolutions and shortcuts of ResNet-18), large enough to be picked
    # (>= 64 steps), with ragged last steps; 16-, 8- and 4-pixel-wide outputs
    (20, 32, 32, 64, 128, 3, 2, 1),
    (70, 16, 16, 128, 64, 3, 2, 1),
    (260, 8, 8, 64, 64, 3, 2, 1),
    (33, 32, 32, 64, 128, 1, 2, 0),
    (141, 16, 16, 128, 64, 1, 2, 0),      # (>= 8192 output pixels with a ragged last tile: shortcut.hip's input gradient when accumulating)
    (520, 8, 8, 64, 64, 1, 2, 0),
    # the register-resident-weight kernels for 16 -> 16 and 32 -> 32 channels (conv3.hip conv16 / conv32): tiles spanning several
    # images, ragged last tile, non-square and non-power-of-two images (division path of the tap masks), one-row images
    (5, 16, 16, 32, 32, 3, 1, 1),
    (33, 16, 16, 32, 32, 3, 1, 1),
    (140, 16, 16, 32, 32, 3, 1, 1),    # wgrad32 (conv3.hip): two images per workgroup, 70 groups; (33: two per group, ragged last group; 5 / 6: one)
    (3, 8, 16, 32, 32, 3, 1, 1),       # ... an 8-row image of width 16
    (3, 7, 5, 32, 32, 3, 1, 1),
    (2, 1, 9, 32, 32, 3, 1, 1),
    (9, 32, 32, 16, 16, 3, 1, 1),
    (3, 7, 5, 16, 16, 3, 1, 1),
    (2, 1, 9, 16, 16, 3, 1, 1),
    # stride-2 3x3: dgrad runs as 4 parity classes visiting only the contributing taps (conv2.hip)
    (4, 16, 16, 64, 128, 3, 2, 1),
    (33, 32, 32, 64, 128, 3, 2, 1),
    (3, 9, 9, 64, 128, 3, 2, 1),       # odd image size -> generic path
]


def conv_setup(case, mode, seed=0):
    N, H, W, C, K, k, s, p = case
    code, tdt = DT[mode]
    cpad = max(8, C)
    x = quant(rnd((N, C, H, W), seed), tdt)
    w = quant(rnd((K, C, k, k), seed + 1, 1.0 / (C * k * k) ** 0.5), tdt)
    xd = to_nhwc(x, tdt, cpad)
    wk = torch.zeros(K, k, k, cpad)
    wk[..., :C] = w.permute(0, 2, 3, 1)
    wfd = wk.to(tdt).to(DEV).contiguous()
    return x, w, xd, wfd, code, tdt, cpad


@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_fwd_and_stats(case, mode):
    N, H, W, C, K, k, s, p = case
    x, w, xd, wfd, code, tdt, cpad = conv_setup(case, mode)
    ref = F.conv2d(x.double(), w.double(), None, s, p)
    Ho, Wo = ref.shape[2:]
    z = torch.empty(N, Ho, Wo, K, dtype=tdt, device=DEV)
    tiles = _lib.lib().clhip_conv_fwd_tiles(N, H, W, cpad, K, k, s, p)
    part = torch.full((tiles, 2, K), float("nan"), device=DEV)
    call("clhip_conv_fwd", xd.data_ptr(), wfd.data_ptr(), z.data_ptr(), part.data_ptr(), N, H, W, cpad, K, k, s, p, code, st())
    got = from_nhwc(z)
    assert (got.double() - ref).abs().max() <= tol(mode, ref)
    # BatchNorm statistics from the fp32 accumulators: per-channel sum / sum of squares
    s1, s2 = part[:, 0].double().sum(0).cpu(), part[:, 1].double().sum(0).cpu()
    r1, r2 = ref.sum(dim=(0, 2, 3)), (ref * ref).sum(dim=(0, 2, 3))
    assert (s1 - r1).abs().max() <= 1e-4 * (ref.abs().sum(dim=(0, 2, 3)).max() + 1e-30)
    assert (s2 - r2).abs().max() <= 1e-4 * (r2.max() + 1e-30)
    # eval mode: no statistics requested
    z2 = torch.empty_like(z)
    call("clhip_conv_fwd", xd.data_ptr(), wfd.data_ptr(), z2.data_ptr(), None, N, H, W, cpad, K, k, s, p, code, st())
    special = cpad == 8 and k == 3 and s == 1
    # 64 -> 64 channels on >= 512 tiles of 256 pixels: the statistics-free (and the accumulator) call goes to the weight-stationary kernel
    # (conv5.hip), the partial-row call above to conv4.hip
    special = special or bool(_lib.lib().clhip_conv_fwd_tiles(N, H, W, cpad, K, k, s, p) and C == 64 and K == 64 and k == 3 and s == 1 and N * H * W >= 512 * 256)
    # ... and 64 -> 64 channels on small maps (<= 32 768 pixels, width <= 16) to the register-resident kernel of conv3.hip (conv64)
    special = special or (C == 64 and K == 64 and k == 3 and s == 1 and W <= 16 and N * H * W <= 32768)
    if mode == "bf16" and special:      # the stems: partial-row statistics come from the generic kernel, this call from stem.hip
        assert (z2.float() - z.float()).abs().max() <= 2 ** -7 * z.float().abs().max()      # one bf16 rounding of a different summation order
        assert (from_nhwc(z2).double() - ref).abs().max() <= tol(mode, ref)
    else:
        assert torch.equal(z2, z)


@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("case", [c for c in CONV_CASES if c[3] >= 16 and (c[4] & (c[4] - 1)) == 0])
def test_conv_dgrad(case, mode):
    N, H, W, C, K, k, s, p = case
    code, tdt = DT[mode]
    w = quant(rnd((K, C, k, k), 5, 1.0 / (K * k * k) ** 0.5), tdt)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dz = quant(rnd((N, K, Ho, Wo), 6), tdt)
    xr = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w.double(), None, s, p).backward(dz.double())
    ref = xr.grad
    wdg = w.permute(1, 2, 3, 0).contiguous().to(tdt).to(DEV)        # [C][R][S][K]
    dzd = to_nhwc(dz, tdt)
    dx = torch.full((N, H, W, C), float("nan"), dtype=tdt, device=DEV)
    call("clhip_conv_dgrad", dzd.data_ptr(), wdg.data_ptr(), dx.data_ptr(), 0, N, H, W, C, K, k, s, p, code, st())
    got = from_nhwc(dx)
    assert (got.double() - ref).abs().max() <= tol(mode, ref)
    # accumulate flag: dx += result
    base = quant(rnd((N, C, H, W), 7), tdt)
    dx2 = to_nhwc(base, tdt)
    call("clhip_conv_dgrad", dzd.data_ptr(), wdg.data_ptr(), dx2.data_ptr(), 1, N, H, W, C, K, k, s, p, code, st())
    ref2 = ref + base.double()
    assert (from_nhwc(dx2).double() - ref2).abs().max() <= tol(mode, ref2) * 1.5


CONV5_CASES = [(8, 32, 32), (3, 5, 7), (130, 32, 32), (33, 16, 16), (20, 8, 8), (70, 4, 4), (9, 1, 9), (2, 13, 2), (260, 32, 32)]


@pytest.mark.parametrize("shape", CONV5_CASES)
def test_weight_stationary_conv5(shape):
    """conv5.hip (64 -> 64 channels, 3x3 / s1, weights resident in registers) forced onto small problems (CONV5_MIN_TILES = 1) against
    the fp64 convolution and against conv4.hip on the same operands: forward + the fp64 BatchNorm accumulators, dgrad, dgrad with
    accumulation; ragged last tiles, tiles spanning images, non-power-of-two images (division path of the tap masks), one-row and
    two-column images, and the benchmark size (260 images: more tiles than workgroups, four per workgroup)."""
    N, H, W = shape
    case = (N, H, W, 64, 64, 3, 1, 1)
    L = _lib.lib()
    code, tdt = DT["bf16"]
    x, w, xd, wfd, _, _, cpad = conv_setup(case, "bf16", seed=21)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    rep = 4
    outs = {}
    try:
        for which in ("conv5", "conv4"):
            assert L.clhip_config(b"CONV5", b"1" if which == "conv5" else b"0") == 0
            assert L.clhip_config(b"CONV5_MIN_TILES", b"1") == 0
            z = torch.full((N, H, W, 64), float("nan"), dtype=tdt, device=DEV)
            acc = torch.zeros(rep, 2, 64, dtype=torch.float64, device=DEV)
            call("clhip_conv_fwd_acc", xd.data_ptr(), wfd.data_ptr(), z.data_ptr(), acc.data_ptr(), rep, N, H, W, 64, 64, 3, 1, 1, code, st())
            # dgrad: gradient dz [N,K,H,W], weight copy [C][R][S][K]
            wq = quant(rnd((64, 64, 3, 3), 5, 1.0 / 24.0), tdt)
            dz = quant(rnd((N, 64, H, W), 6), tdt)
            wdg = wq.permute(1, 2, 3, 0).contiguous().to(tdt).to(DEV)
            dzd = to_nhwc(dz, tdt)
            dx = torch.full((N, H, W, 64), float("nan"), dtype=tdt, device=DEV)
            call("clhip_conv_dgrad", dzd.data_ptr(), wdg.data_ptr(), dx.data_ptr(), 0, N, H, W, 64, 64, 3, 1, 1, code, st())
            base = quant(rnd((N, 64, H, W), 7), tdt)
            dx2 = to_nhwc(base, tdt)
            call("clhip_conv_dgrad", dzd.data_ptr(), wdg.data_ptr(), dx2.data_ptr(), 1, N, H, W, 64, 64, 3, 1, 1, code, st())
            torch.cuda.synchronize()
            outs[which] = (z.clone(), acc.sum(0).cpu(), dx.clone(), dx2.clone())
    finally:
        L.clhip_config(b"CONV5", None)
        L.clhip_config(b"CONV5_MIN_TILES", None)
    z5, s5, dx5, dxa5 = outs["conv5"]
    z4, s4, dx4, dxa4 = outs["conv4"]
    assert (from_nhwc(z5).double() - ref).abs().max() <= tol("bf16", ref)
    r1, r2 = ref.sum(dim=(0, 2, 3)), (ref * ref).sum(dim=(0, 2, 3))
    assert (s5[0] - r1).abs().max() <= 1e-4 * (ref.abs().sum(dim=(0, 2, 3)).max() + 1e-30)
    assert (s5[1] - r2).abs().max() <= 1e-4 * (r2.max() + 1e-30)
    xr = torch.zeros(N, 64, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, wq.double(), None, 1, 1).backward(dz.double())
    assert (from_nhwc(dx5).double() - xr.grad).abs().max() <= tol("bf16", xr.grad)
    ref2 = xr.grad + base.double()
    assert (from_nhwc(dxa5).double() - ref2).abs().max() <= tol("bf16", ref2) * 1.5
    # the two kernels sum the same 576 products per output in fp32 in different orders: they agree to the final bf16 rounding
    for a, b, r in ((z5, z4, ref), (dx5, dx4, xr.grad), (dxa5, dxa4, ref2)):
        assert (a.float() - b.float()).abs().max() <= 2 ** -7 * float(r.abs().max())


CONV8_CASES = [(8, 32, 32), (3, 16, 16), (5, 32, 64), (260, 32, 32), (1, 32, 32)]


@pytest.mark.parametrize("shape", CONV8_CASES)
def test_two_workgroups_per_cu_conv8(shape):
    """conv8.hip (64 -> 64 channels, 3x3 / s1: two four-wave workgroups per CU, the filters of 32 output channels resident per wave, zero-padded
    XOR-swizzled patch of whole image rows) forced onto small problems (CONV8_MIN_TILES = 1) against the fp64 convolution and against conv4.hip
    on the same operands: forward + the fp64 BatchNorm accumulators, dgrad, dgrad with accumulation; tiles at the top / bottom of an image and in
    its middle, 16-wide images (8 rows per tile), more tiles than workgroups (260 images: 2080 tiles, four or five per workgroup), a single tile
    range per XCD shorter than the grid."""
    N, H, W = shape
    case = (N, H, W, 64, 64, 3, 1, 1)
    L = _lib.lib()
    code, tdt = DT["bf16"]
    x, w, xd, wfd, _, _, cpad = conv_setup(case, "bf16", seed=21)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    rep = 4
    outs = {}
    try:
        for which in ("conv8", "conv4"):
            assert L.clhip_config(b"CONV8", b"1" if which == "conv8" else b"0") == 0
            assert L.clhip_config(b"CONV8_MIN_TILES", b"1") == 0
            assert L.clhip_config(b"CONV5", b"0") == 0
            z = torch.full((N, H, W, 64), float("nan"), dtype=tdt, device=DEV)
            acc = torch.zeros(rep, 2, 64, dtype=torch.float64, device=DEV)
            call("clhip_conv_fwd_acc", xd.data_ptr(), wfd.data_ptr(), z.data_ptr(), acc.data_ptr(), rep, N, H, W, 64, 64, 3, 1, 1, code, st())
            wq = quant(rnd((64, 64, 3, 3), 5, 1.0 / 24.0), tdt)
            dz = quant(rnd((N, 64, H, W), 6), tdt)
            wdg = wq.permute(1, 2, 3, 0).contiguous().to(tdt).to(DEV)
            dzd = to_nhwc(dz, tdt)
            dx = torch.full((N, H, W, 64), float("nan"), dtype=tdt, device=DEV)
            call("clhip_conv_dgrad", dzd.data_ptr(), wdg.data_ptr(), dx.data_ptr(), 0, N, H, W, 64, 64, 3, 1, 1, code, st())
            base = quant(rnd((N, 64, H, W), 7), tdt)
            dx2 = to_nhwc(base, tdt)
            call("clhip_conv_dgrad", dzd.data_ptr(), wdg.data_ptr(), dx2.data_ptr(), 1, N, H, W, 64, 64, 3, 1, 1, code, st())
            torch.cuda.synchronize()
            outs[which] = (z.clone(), acc.sum(0).cpu(), dx.clone(), dx2.clone())
    finally:
        L.clhip_config(b"CONV8", None)
        L.clhip_config(b"CONV8_MIN_TILES", None)
        L.clhip_config(b"CONV5", None)
    z8, s8, dx8, dxa8 = outs["conv8"]
    z4, s4, dx4, dxa4 = outs["conv4"]
    assert (from_nhwc(z8).double() - ref).abs().max() <= tol("bf16", ref)
    r1, r2 = ref.sum(dim=(0, 2, 3)), (ref * ref).sum(dim=(0, 2, 3))
    assert (s8[0] - r1).abs().max() <= 1e-4 * (ref.abs().sum(dim=(0, 2, 3)).max() + 1e-30)
    assert (s8[1] - r2).abs().max() <= 1e-4 * (r2.max() + 1e-30)
    xr = torch.zeros(N, 64, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, wq.double(), None, 1, 1).backward(dz.double())
    assert (from_nhwc(dx8).double() - xr.grad).abs().max() <= tol("bf16", xr.grad)
    ref2 = xr.grad + base.double()
    assert (from_nhwc(dxa8).double() - ref2).abs().max() <= tol("bf16", ref2) * 1.5
    for a, b, r in ((z8, z4, ref), (dx8, dx4, xr.grad), (dxa8, dxa4, ref2)):      # different summation orders: equal to the final bf16 rounding
        assert (a.float() - b.float()).abs().max() <= 2 ** -7 * float(r.abs().max())


@pytest.mark.parametrize("mask_from", ["bits", "z", "y", "none"])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", [(6, 32, 32), (3, 16, 16), (70, 32, 32)])
def test_conv8_dgrad_with_batchnorm_backward_sums(shape, accumulate, mask_from):
    """conv8.hip's dgrad epilogue: sum g and sum g * xhat of the PRODUCING layer's BatchNorm backward from the fp32 results, z' staged through LDS by
    the wave that needs it, the producer's ReLU mask from its packed bits / from z' (scale z' + shift > 0) / from its activation / absent
    (clhip_conv_dgrad_bn_reduce_ex) -- against the unfused clhip_conv_dgrad on the same kernel (dx bit-identical) and fp64 sums."""
    N, H, W = shape
    C = 64
    L = _lib.lib()
    code, tdt = DT["bf16"]
    dzn = quant(rnd((N, C, H, W), 31, 0.5), tdt)
    wd = quant(rnd((C, 9, C), 32, 0.05), tdt)
    zp = quant(rnd((N, C, H, W), 33, 1.5) + 0.2, tdt)
    gamma, beta = rnd((C,), 38) * 0.5 + 1.0, rnd((C,), 39) * 0.2
    mean, invstd = rnd((C,), 36) * 0.3, rnd((C,), 37).abs() + 0.5
    sc = gamma * invstd
    sh = beta - mean * sc
    if mask_from == "z":
        yact = torch.relu(zp.float() * sc.view(1, C, 1, 1) + sh.view(1, C, 1, 1))          # ReLU straight behind the BatchNorm
    else:
        yact = torch.relu(rnd((N, C, H, W), 34))
    yp = quant(yact, tdt)
    on = (yp.float() > 0) if mask_from != "none" else torch.ones_like(yp, dtype=torch.bool)
    old = quant(rnd((N, C, H, W), 35, 0.3), tdt)
    dzd, wdd, zpd, ypd = to_nhwc(dzn, tdt), wd.to(tdt).to(DEV).contiguous(), to_nhwc(zp, tdt), to_nhwc(yp, tdt)
    bits = on.permute(0, 2, 3, 1).reshape(-1, C // 8, 8).to(torch.uint8)
    packed = (bits << torch.arange(8, dtype=torch.uint8)).sum(-1).to(torch.uint8).to(DEV).contiguous()
    d = lambda t: t.to(DEV)
    md, isd, gd, bd = d(mean), d(invstd), d(gamma), d(beta)
    rep = 4
    res = {}
    try:
        assert L.clhip_config(b"CONV8_MIN_TILES", b"1") == 0
        assert L.clhip_config(b"CONV8_BNR", b"1") == 0
        # maps up to 16 wide and 32 768 pixels stay on conv3.hip's conv64 (by design: the launch is at its latency floor there): the same properties hold on it,
        # the mask always from the activation
        on_conv8 = W > 16
        assert L.clhip_conv_dgrad_bn_reduce_overlapped(N, H, W, C, C, 3, 1, 1, code) == (1 if on_conv8 else 0)
        assert L.clhip_conv_route(3, 0, N, H, W, C, C, C, 3, 1, 1, code) == (_lib.CONV_CONV8 if on_conv8 else _lib.CONV_CONV64)
        for fused in (1, 0):
            dx = to_nhwc(old, tdt).clone() if accumulate else torch.full((N, H, W, C), float("nan"), dtype=tdt, device=DEV)
            acc = torch.zeros(rep, 2, C, dtype=torch.float64, device=DEV)
            if fused:
                call("clhip_conv_dgrad_bn_reduce_ex", dzd.data_ptr(), wdd.data_ptr(), dx.data_ptr(), accumulate, zpd.data_ptr(),
                     ypd.data_ptr() if mask_from != "none" else None, packed.data_ptr() if mask_from == "bits" else None,
                     gd.data_ptr() if mask_from == "z" else None, bd.data_ptr() if mask_from == "z" else None,
                     md.data_ptr(), isd.data_ptr(), acc.data_ptr(), rep, N, H, W, C, C, 3, 1, 1, code, st())
            else:
                call("clhip_conv_dgrad", dzd.data_ptr(), wdd.data_ptr(), dx.data_ptr(), accumulate, N, H, W, C, C, 3, 1, 1, code, st())
            torch.cuda.synchronize()
            res[fused] = (dx.clone(), acc.sum(0).cpu())
    finally:
        L.clhip_config(b"CONV8_MIN_TILES", None)
        L.clhip_config(b"CONV8_BNR", None)
    assert torch.equal(res[1][0], res[0][0])
    w4 = wd.double().reshape(C, 3, 3, C).permute(3, 0, 1, 2).contiguous()
    dx_ref = F.conv_transpose2d(dzn.double(), w4, padding=1)
    if accumulate:
        dx_ref = dx_ref + old.double()
    assert (from_nhwc(res[1][0]).double() - dx_ref).abs().max() <= tol("bf16", dx_ref) * 1.5
    g = dx_ref * on.double()
    xhat = (zp.double() - mean.double().view(1, C, 1, 1)) * invstd.double().view(1, C, 1, 1)
    s_ref = torch.stack([g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))])
    scale = torch.stack([g.abs().sum((0, 2, 3)), (g * xhat).abs().sum((0, 2, 3))]) + 1e-9
    assert ((res[1][1] - s_ref).abs() / scale).max() < 4e-3


@pytest.mark.parametrize("shape", [(9, 32, 32, 16), (140, 32, 32, 16), (33, 16, 16, 32), (140, 16, 16, 32), (3, 8, 16, 32), (9, 8, 8, 64), (140, 8, 8, 64),
                                   (3, 16, 8, 64), (256, 8, 8, 64), (33, 4, 8, 64)])
@pytest.mark.parametrize("with_bn,accumulate", [(0, 0), (1, 1), (1, 0)])
def test_dgrad_and_wgrad_in_one_launch(shape, with_bn, accumulate):
    """clhip_conv_dgrad_wgrad (the input gradient and the weight gradient of a 16 -> 16 / 32 -> 32-channel layer as ONE launch: the two device
    bodies of the stand-alone kernels behind one grid) against the two-launch path on the same operands: dx, the BatchNorm-backward sums
    of its epilogue and dw are BIT-IDENTICAL (same code, same partial-block order), with and without accumulation into dx."""
    N, H, W, C = shape
    L = _lib.lib()
    code, tdt = DT["bf16"]
    assert L.clhip_conv_dgrad_wgrad_supported(N, H, W, C, C, C, 3, 1, 1, code) == 1
    x = to_nhwc(quant(rnd((N, C, H, W), 61), tdt), tdt)
    dz = to_nhwc(quant(rnd((N, C, H, W), 62, 0.5), tdt), tdt)
    wd = quant(rnd((C, 9, C), 63, 0.1), tdt).to(tdt).to(DEV).contiguous()
    zp, yp = to_nhwc(quant(rnd((N, C, H, W), 64, 1.5), tdt), tdt), to_nhwc(quant(torch.relu(rnd((N, C, H, W), 65)), tdt), tdt)
    mean, invstd = (rnd((C,), 66) * 0.3).to(DEV), (rnd((C,), 67).abs() + 0.5).to(DEV)
    old = to_nhwc(quant(rnd((N, C, H, W), 68, 0.3), tdt), tdt)
    wsb = L.clhip_conv_wgrad_ws_bytes(N, H, W, C, C, C, 3, 1, 1, code)
    assert wsb > 0
    rep = 4

    def run(fused):
        dx = old.clone() if accumulate else torch.full((N, H, W, C), float("nan"), dtype=tdt, device=DEV)
        dw = torch.full((C, 9, C), 0.25, device=DEV)
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        acc = torch.zeros(rep, 2, C, dtype=torch.float64, device=DEV)
        bn = (zp.data_ptr(), yp.data_ptr(), mean.data_ptr(), invstd.data_ptr(), acc.data_ptr(), rep) if with_bn else (None, None, None, None, None, 1)
        if fused:
            call("clhip_conv_dgrad_wgrad", x.data_ptr(), dz.data_ptr(), wd.data_ptr(), dx.data_ptr(), accumulate, dw.data_ptr(), ws.data_ptr(), *bn,
                 N, H, W, C, C, C, 3, 1, 1, code, st())
        else:
            if with_bn:
                call("clhip_conv_dgrad_bn_reduce", dz.data_ptr(), wd.data_ptr(), dx.data_ptr(), accumulate, zp.data_ptr(), yp.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                     acc.data_ptr(), rep, N, H, W, C, C, 3, 1, 1, code, st())
            else:
                call("clhip_conv_dgrad", dz.data_ptr(), wd.data_ptr(), dx.data_ptr(), accumulate, N, H, W, C, C, 3, 1, 1, code, st())
            call("clhip_conv_wgrad", x.data_ptr(), dz.data_ptr(), dw.data_ptr(), ws.data_ptr(), N, H, W, C, C, C, 3, 1, 1, code, st())
        torch.cuda.synchronize()
        return dx, dw, acc.sum(0)

    dx_f, dw_f, s_f = run(True)
    dx_u, dw_u, s_u = run(False)
    assert torch.equal(dx_f, dx_u) and torch.equal(dw_f, dw_u)
    if with_bn:          # fp64 atomics into 4 replicas: the same addends, summed in arrival order
        assert ((s_f - s_u).abs() <= 1e-12 * s_u.abs().clamp(min=1.0)).all()
    # and against fp64 math for the weight gradient (the dgrad / sums are covered by their own tests)
    xr = from_nhwc(x).double()
    wr = torch.zeros(C, C, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, wr, None, 1, 1).backward(from_nhwc(dz).double())
    got = dw_f.cpu().double().reshape(C, 3, 3, C).permute(0, 3, 1, 2) - 0.25
    assert (got - wr.grad).abs().max() <= 2e-4 * float(wr.grad.abs().max()) + 1e-6


@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_wgrad(case, mode):
    N, H, W, C, K, k, s, p = case
    x, w, xd, wfd, code, tdt, cpad = conv_setup(case, mode, seed=11)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dz = quant(rnd((N, K, Ho, Wo), 12), tdt)
    wr = w.double().clone().requires_grad_(True)
    F.conv2d(x.double(), wr, None, s, p).backward(dz.double())
    ref = wr.grad                                           # [K,C,k,k]
    dzd = to_nhwc(dz, tdt)
    dw = torch.zeros(K, k, k, C, device=DEV)                # K,R,S,Creal fp32
    wsb = _lib.lib().clhip_conv_wgrad_ws_bytes(N, H, W, cpad, C, K, k, s, p, code)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
    call("clhip_conv_wgrad", xd.data_ptr(), dzd.data_ptr(), dw.data_ptr(), None, N, H, W, cpad, C, K, k, s, p, code, st())   # atomics path
    got = dw.cpu().permute(0, 3, 1, 2).double()
    t = 2e-4 * float(ref.abs().max()) + 1e-6               # fp32 accumulation of exactly representable products
    assert (got - ref).abs().max() <= t
    # accumulation into existing content (+=), through the deterministic partial-block path when there is one
    call("clhip_conv_wgrad", xd.data_ptr(), dzd.data_ptr(), dw.data_ptr(), ws.data_ptr() if wsb else None, N, H, W, cpad, C, K, k, s, p, code, st())
    assert (dw.cpu().permute(0, 3, 1, 2).double() - 2 * ref).abs().max() <= 2 * t
    if wsb:   # bitwise reproducible
        d1, d2 = torch.zeros_like(dw), torch.zeros_like(dw)
        for d in (d1, d2):
            call("clhip_conv_wgrad", xd.data_ptr(), dzd.data_ptr(), d.data_ptr(), ws.data_ptr(), N, H, W, cpad, C, K, k, s, p, code, st())
        assert torch.equal(d1, d2)


def test_weight_prep_and_layout_converts():
    K, C, k = 32, 3, 3
    w = rnd((K, C, k, k), 3)
    wm = w.permute(0, 2, 3, 1).contiguous().to(DEV)          # master layout K,R,S,C
    for mode, (code, tdt) in DT.items():
        wf = torch.empty(K, k * k, 8, dtype=tdt, device=DEV)
        wd = torch.empty(8, k * k, K, dtype=tdt, device=DEV)
        call("clhip_conv_weight_prep", wm.data_ptr(), wf.data_ptr(), wd.data_ptr(), K, k * k, C, 8, code, st())
        ref = torch.zeros(K, k * k, 8)
        ref[..., :C] = w.permute(0, 2, 3, 1).reshape(K, k * k, C)
        assert torch.equal(wf.float().cpu(), ref.to(tdt).float())
        assert torch.equal(wd.float().cpu(), ref.permute(2, 1, 0).to(tdt).float())
        x = rnd((3, 3, 5, 6), 4)
        y = torch.empty(3, 5, 6, 8, dtype=tdt, device=DEV)
        call("clhip_nchw_to_nhwc", x.to(DEV).data_ptr(), y.data_ptr(), 3, 3, 5, 6, 8, code, st())
        assert torch.equal(y.float().cpu()[..., :3], x.permute(0, 2, 3, 1).to(tdt).float())
        assert float(y.float().abs().cpu()[..., 3:].max()) == 0.0
        back = torch.empty(3, 8, 5, 6, device=DEV)
        call("clhip_nhwc_to_nchw", y.data_ptr(), back.data_ptr(), 3, 8, 5, 6, code, st())
        assert torch.equal(back.cpu()[:, :3], x.to(tdt).float())


@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("shape", [(4, 8, 8, 16), (3, 5, 5, 64), (2, 4, 4, 512), (64, 16, 16, 32)])
@pytest.mark.parametrize("relu,res", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_batchnorm_fwd_bwd(shape, mode, relu, res):
    N, H, W, C = shape
    code, tdt = DT[mode]
    M = N * H * W
    z = quant(rnd((N, C, H, W), 20, 2.0) + 0.3, tdt)
    r = quant(rnd((N, C, H, W), 21), tdt) if res else None
    gamma, beta = rnd((C,), 22) * 0.5 + 1.0, rnd((C,), 23) * 0.2
    rm0, rv0 = rnd((C,), 24) * 0.1, rnd((C,), 25).abs() + 0.5
    dy = quant(rnd((N, C, H, W), 26), tdt)
    # device: statistics partials as the conv epilogue would produce them (exact sums of z)
    zd = to_nhwc(z, tdt)
    z2 = z.double().permute(0, 2, 3, 1).reshape(M, C)
    tiles = 3
    part = torch.zeros(tiles, 2, C, dtype=torch.float64)
    for t, ch in enumerate(torch.chunk(z2, tiles, 0)):
        part[t, 0], part[t, 1] = ch.sum(0), (ch * ch).sum(0)
    part = part.float().to(DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    rmd, rvd = rm0.clone().to(DEV), rv0.clone().to(DEV)
    mean, invstd, scale, shift = (torch.empty(C, device=DEV) for _ in range(4))
    call("clhip_bn_stats_finalize", part.data_ptr(), tiles, M, C, gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(),
         0.1, 1e-5, mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), st())
    rd = to_nhwc(r, tdt) if res else None
    yd = torch.empty(N, H, W, C, dtype=tdt, device=DEV)
    call("clhip_bn_apply", zd.data_ptr(), scale.data_ptr(), shift.data_ptr(), rd.data_ptr() if res else None, yd.data_ptr(), M, C,
         relu, code, st())
    # oracle (fp64): nn.BatchNorm2d train semantics.  The ReLU mask is taken from the device's stored y so
    # that elements within rounding distance of 0 cannot flip the comparison.
    zr = z.double().clone().requires_grad_(True)
    g64, b64 = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    rm, rv = rm0.double().clone(), rv0.double().clone()
    y = F.batch_norm(zr, rm, rv, g64, b64, True, 0.1, 1e-5)
    if res:
        rr = r.double().clone().requires_grad_(True)
        y = y + rr
    ypre = y.detach().clone()
    if relu:
        y = y * (from_nhwc(yd) > 0).double()
    y.backward(dy.double())
    assert torch.allclose(rmd.cpu().double(), rm, rtol=1e-5, atol=1e-6)
    assert torch.allclose(rvd.cpu().double(), rv, rtol=1e-4, atol=1e-6)
    yref = F.relu(ypre) if relu else ypre
    assert (from_nhwc(yd).double() - yref).abs().max() <= tol(mode, yref)
    # backward
    dyd = to_nhwc(dy, tdt)
    ws = torch.empty(_lib.lib().clhip_bn_bwd_ws_floats(M, C), device=DEV)
    dgamma, dbeta = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dz = torch.empty(N, H, W, C, dtype=tdt, device=DEV)
    dres = torch.empty(N, H, W, C, dtype=tdt, device=DEV) if res else None
    call("clhip_bn_bwd", dyd.data_ptr(), yd.data_ptr(), zd.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gd.data_ptr(),
         dgamma.data_ptr(), dbeta.data_ptr(), dz.data_ptr(), dres.data_ptr() if res else None, 0, M, C, relu, ws.data_ptr(), code, st())
    gz = zr.grad
    assert (from_nhwc(dz).double() - gz).abs().max() <= tol(mode, gz) * 2
    assert (dgamma.cpu().double() - g64.grad).abs().max() <= 2e-3 * (g64.grad.abs().max() + 1e-9) + 1e-4
    assert (dbeta.cpu().double() - b64.grad).abs().max() <= 2e-3 * (b64.grad.abs().max() + 1e-9) + 1e-4
    if res:
        assert (from_nhwc(dres).double() - rr.grad).abs().max() <= tol(mode, rr.grad)
        # accumulate variant
        call("clhip_bn_bwd", dyd.data_ptr(), yd.data_ptr(), zd.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gd.data_ptr(),
             dgamma.data_ptr(), dbeta.data_ptr(), dz.data_ptr(), dres.data_ptr(), 1, M, C, relu, ws.data_ptr(), code, st())
        assert (from_nhwc(dres).double() - 2 * rr.grad).abs().max() <= tol(mode, rr.grad) * 3
    # accumulator variants (what the plan runs): fp64 sums instead of per-tile partial rows, no finalize launches;
    # must reproduce the partial-buffer path on the same inputs
    REP = 4                                                                        # accumulator replicas: the sums split over 4 copies
    full = torch.stack([z2.sum(0), (z2 * z2).sum(0)])                              # [2, C] fp64, as the conv epilogue accumulates it
    acc = torch.stack([full * f for f in (0.4, 0.3, 0.2, 0.1)]).to(DEV)            # [REP, 2, C]
    rm2, rv2 = rm0.clone().to(DEV), rv0.clone().to(DEV)
    mean2, invstd2 = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    y2 = torch.empty(N, H, W, C, dtype=tdt, device=DEV)
    call("clhip_bn_apply_train", zd.data_ptr(), acc.data_ptr(), REP, M, C, gd.data_ptr(), bd.data_ptr(), rm2.data_ptr(), rv2.data_ptr(), 0.1, 1e-5,
         mean2.data_ptr(), invstd2.data_ptr(), rd.data_ptr() if res else None, y2.data_ptr(), relu, code, st())
    assert torch.allclose(mean2, mean, rtol=1e-5, atol=1e-6) and torch.allclose(invstd2, invstd, rtol=1e-5)
    assert torch.allclose(rm2.cpu().double(), rm, rtol=1e-5, atol=1e-6) and torch.allclose(rv2.cpu().double(), rv, rtol=1e-4, atol=1e-6)
    assert (from_nhwc(y2).double() - yref).abs().max() <= tol(mode, yref)
    bacc = torch.zeros(REP, 2, C, dtype=torch.float64, device=DEV)
    dg2, db2 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dz2 = torch.empty(N, H, W, C, dtype=tdt, device=DEV)
    dres2 = torch.empty(N, H, W, C, dtype=tdt, device=DEV) if res else None
    call("clhip_bn_bwd_acc", dyd.data_ptr(), yd.data_ptr(), zd.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gd.data_ptr(), dg2.data_ptr(),
         db2.data_ptr(), dz2.data_ptr(), dres2.data_ptr() if res else None, 0, M, C, relu, bacc.data_ptr(), REP, code, st())
    assert (from_nhwc(dz2).double() - gz).abs().max() <= tol(mode, gz) * 2
    assert (dg2.cpu().double() - g64.grad).abs().max() <= 2e-3 * (g64.grad.abs().max() + 1e-9) + 1e-4
    assert (db2.cpu().double() - b64.grad).abs().max() <= 2e-3 * (b64.grad.abs().max() + 1e-9) + 1e-4
    if res:
        assert (from_nhwc(dres2).double() - rr.grad).abs().max() <= tol(mode, rr.grad)
    if relu:
        # the packed ReLU mask (one bit per element, written by the forward apply) gives the backward the same mask as reading y
        rm3, rv3 = rm0.clone().to(DEV), rv0.clone().to(DEV)
        y3 = torch.empty(N, H, W, C, dtype=tdt, device=DEV)
        bits = torch.zeros(M * C // 8, dtype=torch.uint8, device=DEV)
        call("clhip_bn_apply_train_mask", zd.data_ptr(), acc.data_ptr(), REP, M, C, gd.data_ptr(), bd.data_ptr(), rm3.data_ptr(), rv3.data_ptr(), 0.1, 1e-5,
             mean2.data_ptr(), invstd2.data_ptr(), rd.data_ptr() if res else None, y3.data_ptr(), bits.data_ptr(), code, st())
        assert torch.equal(y3, y2)
        want = (y2.reshape(-1, 8).float() > 0).to(torch.int32)
        want = (want * (2 ** torch.arange(8, device=DEV, dtype=torch.int32))).sum(1).to(torch.uint8)
        assert torch.equal(bits, want)
        outs = []
        for code_relu, yptr in ((1, y2), (3, bits)):
            bacc.zero_()
            dgm, dbm = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            dzm = torch.empty(N, H, W, C, dtype=tdt, device=DEV)
            drm = torch.empty(N, H, W, C, dtype=tdt, device=DEV) if res else None
            call("clhip_bn_bwd_acc", dyd.data_ptr(), yptr.data_ptr(), zd.data_ptr(), mean2.data_ptr(), invstd2.data_ptr(), gd.data_ptr(), dgm.data_ptr(),
                 dbm.data_ptr(), dzm.data_ptr(), drm.data_ptr() if res else None, 0, M, C, code_relu, bacc.data_ptr(), REP, code, st())
            torch.cuda.synchronize()
            outs.append((dzm.clone(), drm.clone() if res else None, dgm.cpu().clone(), dbm.cpu().clone()))
        assert torch.equal(outs[0][0], outs[1][0])
        if res:
            assert torch.equal(outs[0][1], outs[1][1])
        assert torch.allclose(outs[0][2], outs[1][2], rtol=1e-5, atol=1e-5) and torch.allclose(outs[0][3], outs[1][3], rtol=1e-5, atol=1e-5)
    if relu and not res:
        # ReLU right after the BatchNorm: the mask recomputed from z (forward's own scale / shift expressions) is the mask read from y
        outs = []
        for variant in ("from_y", "from_z"):
            bacc.zero_(); dg2.zero_(); db2.zero_()
            dz3 = torch.empty(N, H, W, C, dtype=tdt, device=DEV)
            if variant == "from_y":
                call("clhip_bn_bwd_acc", dyd.data_ptr(), y2.data_ptr(), zd.data_ptr(), mean2.data_ptr(), invstd2.data_ptr(), gd.data_ptr(), dg2.data_ptr(),
                     db2.data_ptr(), dz3.data_ptr(), None, 0, M, C, 1, bacc.data_ptr(), REP, code, st())
            else:
                call("clhip_bn_bwd_acc_zmask", dyd.data_ptr(), zd.data_ptr(), mean2.data_ptr(), invstd2.data_ptr(), gd.data_ptr(), bd.data_ptr(), dg2.data_ptr(),
                     db2.data_ptr(), dz3.data_ptr(), M, C, bacc.data_ptr(), REP, code, st())
            outs.append((from_nhwc(dz3).clone(), dg2.cpu().clone(), db2.cpu().clone()))
        assert torch.equal(outs[0][0], outs[1][0])
        assert torch.allclose(outs[0][1], outs[1][1], rtol=1e-5, atol=1e-5) and torch.allclose(outs[0][2], outs[1][2], rtol=1e-5, atol=1e-5)
    # eval-mode affine
    call("clhip_bn_eval_affine", gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(), 1e-5, C, scale.data_ptr(),
         shift.data_ptr(), st())
    ye = F.batch_norm(z.double(), rmd.cpu().double(), rvd.cpu().double(), gamma.double(), beta.double(), False, 0.1, 1e-5)
    call("clhip_bn_apply", zd.data_ptr(), scale.data_ptr(), shift.data_ptr(), None, yd.data_ptr(), M, C, 0, code, st())
    assert (from_nhwc(yd).double() - ye).abs().max() <= tol(mode, ye)


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_avgpool(mode):
    code, tdt = DT[mode]
    a = quant(rnd((5, 64, 8, 8), 30), tdt)
    ad = to_nhwc(a, tdt)
    feat = torch.empty(5, 64, device=DEV)
    call("clhip_avgpool_fwd", ad.data_ptr(), feat.data_ptr(), 5, 64, 64, code, st())
    assert torch.allclose(feat.cpu(), a.mean(dim=(2, 3)), rtol=1e-5, atol=1e-6)
    df = rnd((5, 64), 31)
    da = torch.empty(5, 8, 8, 64, dtype=tdt, device=DEV)
    call("clhip_avgpool_bwd", df.to(DEV).data_ptr(), da.data_ptr(), 5, 64, 64, code, st())
    ref = (df / 64)[:, :, None, None].expand(5, 64, 8, 8)
    assert (from_nhwc(da) - ref).abs().max() <= tol(mode, ref)


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_windowed_avgpool(mode):
    """nn.AvgPool2d(8) + flatten of ResNet_BIC.forward (resnet.py:675-676) on a 16 x 16 map"""
    code, tdt = DT[mode]
    a = quant(rnd((3, 64, 16, 16), 32), tdt)
    ad = to_nhwc(a, tdt)
    feat = torch.empty(3, 256, device=DEV)
    call("clhip_avgpool_win_fwd", ad.data_ptr(), feat.data_ptr(), 3, 16, 16, 64, 8, code, st())
    ref = torch.nn.functional.avg_pool2d(a, 8).reshape(3, -1)
    assert torch.allclose(feat.cpu(), ref, rtol=1e-5, atol=1e-6)
    df = rnd((3, 256), 33)
    da = torch.empty(3, 16, 16, 64, dtype=tdt, device=DEV)
    call("clhip_avgpool_win_bwd", df.to(DEV).data_ptr(), da.data_ptr(), 3, 16, 16, 64, 8, code, st())
    a2 = a.clone().requires_grad_(True)
    (torch.nn.functional.avg_pool2d(a2, 8).reshape(3, -1) * df).sum().backward()
    assert (from_nhwc(da) - a2.grad).abs().max() <= tol(mode, a2.grad)


@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("shape", [(4, 16, 32, 32), (3, 32, 16, 16), (5, 64, 8, 8), (2, 128, 4, 4)])
def test_add_stats_and_add_inplace(mode, shape):
    """`out += residual` of BasicBlock2 (resnet.py:615) + the statistics the next BatchNorm needs, and the gradient join"""
    code, tdt = DT[mode]
    N, Cc, H, W = shape
    M = N * H * W
    z, r = quant(rnd(shape, 50), tdt), quant(rnd(shape, 51) * 0.7 + 0.3, tdt)
    zd, rd = to_nhwc(z, tdt), to_nhwc(r, tdt)
    rep = 4
    acc = torch.zeros(rep, 2, Cc, dtype=torch.float64, device=DEV)
    call("clhip_add_stats", zd.data_ptr(), rd.data_ptr(), acc.data_ptr(), rep, M, Cc, code, st())
    want = quant(z + r, tdt)
    assert (from_nhwc(zd) - want).abs().max() <= tol(mode, want)
    got = from_nhwc(zd).double()                      # the statistics are those of the STORED (rounded) sums
    sums = acc.sum(0).cpu()
    assert torch.allclose(sums[0], got.sum(dim=(0, 2, 3)), rtol=1e-5, atol=1e-3)
    assert torch.allclose(sums[1], (got * got).sum(dim=(0, 2, 3)), rtol=1e-5, atol=1e-3)
    z2 = to_nhwc(z, tdt)
    call("clhip_add_stats", z2.data_ptr(), rd.data_ptr(), None, 1, M, Cc, code, st())        # eval mode: the sum only
    assert torch.equal(from_nhwc(z2), from_nhwc(zd))
    a = to_nhwc(z, tdt)
    call("clhip_add_inplace", a.data_ptr(), rd.data_ptr(), M * Cc, code, st())
    assert torch.equal(from_nhwc(a), from_nhwc(zd))


# ------------------------------------------------------------------------------------ heads / losses
def test_linear_and_losses():
    from libcontinual_amd import ops
    B, D, O = 37, 512, 55
    x = rnd((B, D), 40).to(DEV).requires_grad_(True)
    w = (rnd((O, D), 41) * 0.05).to(DEV).requires_grad_(True)
    b = (rnd((O,), 42) * 0.1).to(DEV).requires_grad_(True)
    y = torch.from_numpy(np.random.RandomState(0).randint(50, 55, B)).to(DEV)
    soft = (rnd((B, 50), 43) * 3).to(DEV)
    logits = ops.linear(x, w, b)
    aux = ops.LossAux()
    loss = ops.classify_loss(logits, y, lo=50, hi=55, w_ce=1.0, teacher=soft, k=50, T=2.0, w_kd=3.0, aux=aux)
    (loss * 1.7).backward()
    xc, wc, bc = (t.detach().cpu().double().requires_grad_(True) for t in (x, w, b))
    lg = F.linear(xc, wc, bc)
    ce = F.cross_entropy(lg[:, 50:], y.cpu() - 50)
    lp = torch.log_softmax(lg[:, :50] / 2, dim=1)
    q = torch.softmax(soft.cpu().double() / 2, dim=1)
    kd = -(q * lp).sum() / B
    ref = ce + 3 * kd
    (ref * 1.7).backward()
    assert torch.allclose(logits.detach().cpu().double(), lg.detach(), rtol=1e-4, atol=1e-5)
    assert abs(loss.item() - ref.item()) < 1e-4 * abs(ref.item())
    for got, want in ((x.grad, xc.grad), (w.grad, wc.grad), (b.grad, bc.grad)):
        assert (got.cpu().double() - want).abs().max() <= 1e-4 * want.abs().max() + 1e-7
    assert torch.equal(aux.pred.cpu(), lg.argmax(1))
    assert aux.correct.item() == int((lg.argmax(1) == y.cpu()).sum())
    # plain CE over all columns, and predict()
    loss2 = ops.classify_loss(logits.detach(), y)
    assert abs(loss2.item() - F.cross_entropy(lg.detach(), y.cpu()).item()) < 1e-4
    pred, correct = ops.predict(logits.detach(), y, pred_hi=52)
    assert torch.equal(pred.cpu(), lg.detach()[:, :52].argmax(1))


@pytest.mark.parametrize("B,O,lo,hi,plo,phi", [(1, 10, 0, 10, 0, 10), (37, 55, 50, 55, 0, 55), (64, 100, 0, 100, 0, 100), (200, 100, 50, 100, 0, 100),
                                               (256, 50, 0, 50, 0, 50), (256, 130, 0, 130, 10, 120), (300, 100, 95, 100, 0, 100), (512, 60, 0, 60, 0, 60),
                                               (256, 200, 180, 200, 0, 200), (300, 200, 0, 200, 0, 200), (600, 55, 0, 55, 0, 55), (7, 300, 0, 300, 0, 300)])
@pytest.mark.parametrize("acc", [0, 1])
def test_ce_window_all_forms(B, O, lo, hi, plo, phi, acc):
    """clhip_ce_window in every dispatch form -- the 16-lane-group kernel of the training steps (B <= 512, O <= 256: ce_rows_kernel), the
    one-wave-per-row single-workgroup form (wider rows) and the multi-workgroup atomic form (B > 512) -- against fp64 math: loss, its
    gradient (overwrite and accumulate), first-maximum argmax inside the prediction window with ties, the correct count; the two
    fixed-order forms are bitwise reproducible."""
    g = torch.Generator().manual_seed(B * 1000 + O)
    logits = (torch.randn(B, O, generator=g) * 3).round_(decimals=1)          # one decimal: plenty of exact ties for the argmax
    y = torch.randint(lo, hi, (B,), generator=g)
    if B > 3:
        y[1] = (lo - 1) % O if lo > 0 else y[1]                                # a label outside the loss window contributes no loss term
    old = torch.randn(B, O, generator=g)
    w = 0.7
    ld, yd = logits.to(DEV), y.to(DEV)

    def run():
        loss = torch.full((1,), 2.5, device=DEV)
        dl = old.to(DEV).clone()
        pred = torch.empty(B, dtype=torch.int64, device=DEV)
        corr = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        call("clhip_ce_window", ld.data_ptr(), yd.data_ptr(), B, O, lo, hi, plo, phi, w, loss.data_ptr(), acc, dl.data_ptr(), acc, pred.data_ptr(),
             corr.data_ptr(), st())
        torch.cuda.synchronize()
        return loss.cpu(), dl.cpu(), pred.cpu(), corr.cpu()

    loss, dl, pred, corr = run()
    L = logits.double()
    lse = torch.logsumexp(L[:, lo:hi], dim=1)
    inwin = (y >= lo) & (y < hi)
    li = torch.where(inwin, lse - L[torch.arange(B), y], torch.zeros(B, dtype=torch.float64))
    want_loss = w * li.sum() / B + (2.5 if acc else 0.0)
    assert abs(loss.item() - want_loss.item()) <= 2e-5 * max(1.0, abs(want_loss.item()))
    gref = torch.zeros(B, O, dtype=torch.float64)
    onehot = torch.zeros(B, O, dtype=torch.float64)
    onehot[torch.arange(B), y] = 1.0
    gref[:, lo:hi] = (w / B) * (torch.softmax(L[:, lo:hi], dim=1) - onehot[:, lo:hi])
    want_g = gref + old.double() if acc else gref
    if acc:
        want_g[:, :lo] = old[:, :lo].double(); want_g[:, hi:] = old[:, hi:].double()
    assert (dl.double() - want_g).abs().max() <= 1e-6
    want_pred = L[:, plo:phi].argmax(1) + plo                                   # torch.argmax: first maximal index
    assert torch.equal(pred, want_pred)
    assert corr.item() == int((want_pred == y).sum())
    if B <= 512:
        loss2, dl2, pred2, corr2 = run()
        assert torch.equal(loss, loss2) and torch.equal(dl, dl2)


def test_lucir_head_and_losses():
    from libcontinual_amd import ops
    B, D, O, nold, K = 24, 64, 12, 9, 2
    x = rnd((B, D), 50).to(DEV).requires_grad_(True)
    w = rnd((O, D), 51).to(DEV).requires_grad_(True)
    sigma = torch.tensor([1.3], device=DEV, requires_grad=True)
    ref_f = rnd((B, D), 52).to(DEV)
    y = torch.from_numpy(np.random.RandomState(1).randint(0, O, B)).to(DEV)
    s = ops.cosine_linear(x, w)
    logit = ops.sigma_scale(s, sigma)
    loss = ops.classify_loss(logit, y) + ops.cos_embed_loss(x, ref_f, 15.81) + ops.margin_rank_loss(s, y, nold, K, 0.5, 1.0)
    loss.backward()
    xc, wc, sc = (t.detach().cpu().double().requires_grad_(True) for t in (x, w, sigma))
    s_ref = F.linear(F.normalize(xc, dim=1), F.normalize(wc, dim=1))
    lg = sc * s_ref
    yc = y.cpu()
    l_ref = F.cross_entropy(lg, yc) + torch.nn.CosineEmbeddingLoss()(xc, ref_f.cpu().double(), torch.ones(B, dtype=torch.float64)) * 15.81
    gt = s_ref.gather(1, yc.view(-1, 1)).squeeze(1)
    nov = s_ref[:, nold:].topk(K, dim=1)[0]
    hard = yc < nold
    if int(hard.sum()) > 0:
        g = gt[hard].view(-1, 1).repeat(1, K)
        l_ref = l_ref + torch.nn.MarginRankingLoss(margin=0.5)(g.view(-1, 1), nov[hard].view(-1, 1), torch.ones(int(hard.sum()) * K, 1, dtype=torch.float64))
    l_ref.backward()
    assert torch.allclose(s.detach().cpu().double(), s_ref.detach(), rtol=1e-4, atol=1e-6)
    assert abs(loss.item() - l_ref.item()) < 2e-4 * abs(l_ref.item())
    for got, want in ((x.grad, xc.grad), (w.grad, wc.grad), (sigma.grad, sc.grad)):
        assert (got.cpu().double() - want).abs().max() <= 2e-4 * want.abs().max() + 1e-7


def test_flat_elementwise_family():
    from libcontinual_amd import ops
    n = 100003
    p, ref, f, g = (rnd((n,), 60 + i).to(DEV) for i in range(4))
    f = f.abs()
    out = torch.empty(1, device=DEV)
    ops.ewc_penalty(p, ref, f, 1000.0, out, False)
    want = 1000.0 * (f.double() * (p.double() - ref.double()) ** 2).sum() / 2
    assert abs(out.item() - want.item()) < 1e-4 * want.item()
    ops.ewc_penalty(p[1:], ref[1:], f[1:], 1.0, out, True)         # misaligned pointers + accumulate
    want2 = want + (f[1:].double() * (p[1:].double() - ref[1:].double()) ** 2).sum() / 2
    assert abs(out.item() - want2.item()) < 1e-4 * want2.item()
    g0 = g.clone()
    sc = torch.tensor([0.5], device=DEV)
    ops.ewc_grad(p, ref, f, g, 1000.0, sc)
    assert torch.allclose(g, g0 + 500.0 * f * (p - ref), rtol=1e-5, atol=1e-5)
    # the multi-segment forms (EWC's backbone buffer + head weight + head bias in one launch): same values as the per-segment launches,
    # with an unaligned and an empty segment among them
    cuts = [(0, 70000), (70001, 99990), (99990, 99990), (99991, n)]
    segs = [(p[a:b], ref[a:b], f[a:b]) for a, b in cuts]
    outm = torch.empty(1, device=DEV)
    ops.ewc_penalty_multi(segs, 10.0, outm, False)
    wantm = sum(10.0 * (s[2].double() * (s[0].double() - s[1].double()) ** 2).sum() / 2 for s in segs)
    assert abs(outm.item() - wantm.item()) < 1e-4 * wantm.item()
    gm, gs = g0.clone(), g0.clone()
    ops.ewc_grad_multi([(p[a:b], ref[a:b], f[a:b], gm[a:b]) for a, b in cuts], 1000.0, sc)
    for a, b in cuts:
        if b > a:
            ops.ewc_grad(p[a:b], ref[a:b], f[a:b], gs[a:b], 1000.0, sc)
    assert torch.equal(gm, gs)
    fi = torch.zeros(n, device=DEV)
    ops.fisher_accum(fi, g0, 32.0 / 96.0)
    assert torch.allclose(fi, g0 * g0 * (32.0 / 96.0), rtol=1e-6)
    old = f.clone()
    ops.fisher_merge(fi, old, 0.9)
    assert torch.allclose(fi, 0.9 * old + 0.1 * g0 * g0 * (32.0 / 96.0), rtol=1e-5, atol=1e-7)
    # SGD (momentum, wd) for 3 steps vs torch.optim.SGD, and Adam
    for kind in ("sgd", "sgd_plain", "adam"):
        pt = rnd((n,), 70).to(DEV)
        pr = pt.clone().cpu().double().requires_grad_(True)
        if kind == "adam":
            opt = torch.optim.Adam([pr], lr=1.875e-3)
            m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        else:
            mom = 0.9 if kind == "sgd" else 0.0
            opt = torch.optim.SGD([pr], lr=0.1, momentum=mom, weight_decay=5e-4 if kind == "sgd" else 0.0)
            buf = torch.zeros(n, device=DEV) if mom else None
        for step in range(1, 4):
            gr = rnd((n,), 80 + step).to(DEV)
            pr.grad = gr.cpu().double()
            opt.step()
            if kind == "adam":
                ops.adam_step(pt, gr, m, v, 1.875e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, step)
            else:
                ops.sgd_step(pt, gr, buf, 0.1, mom, 5e-4 if kind == "sgd" else 0.0)
        assert torch.allclose(pt.cpu().double(), pr.detach(), rtol=1e-4, atol=1e-5), kind
    nrm = torch.empty(1, device=DEV)
    ops.sq_norm(g0, nrm)
    assert abs(nrm.item() - float((g0.double() ** 2).sum())) < 1e-4 * nrm.item()


def test_ncm_and_herding_match_reference_math():
    from libcontinual_amd import ops
    from oracle import methods as om
    feats = rnd((40, 64), 90) + 0.5
    lab = torch.zeros(40, dtype=torch.long)
    chosen_ref = om.herding_select(feats.clone(), lab, 12)
    fn = ops.l2_normalize_rows(feats.to(DEV))
    assert torch.allclose(fn.cpu(), feats / feats.norm(dim=1, keepdim=True), rtol=1e-5, atol=1e-6)
    chosen = ops.herding_select(fn, 12).cpu().tolist()
    assert chosen == chosen_ref
    means = rnd((7, 64), 91)
    pred = ops.ncm_classify(feats.to(DEV), means.to(DEV)).cpu()
    assert torch.equal(pred, om.ncm_distance(feats, means).argmin(1))


@pytest.mark.parametrize("n,D,m", [(500, 64, 40), (500, 512, 20), (2600, 64, 400)])
def test_herding_at_benchmark_size(n, D, m):
    """the greedy mean-matching selection at the sizes of BASELINE.json's iCaRL configuration (CIFAR-100: 500 images per class, a
    2000-exemplar buffer over 50..100 classes = 40..20 per class; ResNet-32 features 64-d, ResNet-18 512-d) and a larger case: the
    same picks as the oracle's loop (buffer/linearherdingbuffer.py:140-161) while its own selection margin is above fp32 noise, and
    in any case the same quality of the selected set (distance of its mean to the class mean)"""
    from libcontinual_amd import ops
    from oracle import methods as om
    g = torch.Generator().manual_seed(1000 + n + D)
    feats = torch.randn(n, D, generator=g) * 0.3 + torch.randn(1, D, generator=g)
    lab = torch.zeros(n, dtype=torch.long)
    ref = om.herding_select(feats.clone(), lab, m)
    fn = ops.l2_normalize_rows(feats.to(DEV))
    got = ops.herding_select(fn, m).cpu().tolist()
    assert len(got) == m and len(set(got)) == m
    first_diff = next((i for i, (a, b) in enumerate(zip(got, ref)) if a != b), m)
    f = (feats / feats.norm(dim=1, keepdim=True)).double()
    mu = f.mean(0)
    d_ref, d_got = float((f[ref].mean(0) - mu).norm()), float((f[got].mean(0) - mu).norm())
    overlap = len(set(got) & set(ref)) / m
    print(f"herding n={n} D={D} m={m}: identical picks up to #{first_diff}, overlap {overlap:.3f}, ||mean(chosen) - mean|| {d_got:.3e} (oracle {d_ref:.3e})")
    # the benchmark depths (20 / 40 picks) are reproduced exactly; a 400-deep greedy chain meets an fp32 near-tie somewhere and the two
    # chains part ways from there (the selection quality stays the same to ~10 %)
    assert first_diff >= min(m, 60)
    assert d_got <= 1.25 * d_ref + 1e-6


def test_herding_all_classes_in_one_launch():
    """ops.herding_select_classes: every class of a task by one workgroup each in ONE launch (round 4) -- the picks of per-class
    ops.herding_select calls, exactly (same arithmetic, same order), for classes of different sizes: one larger than the LDS staging
    limit (global-memory form), one smaller than the number of picks (the tail stays unpicked)."""
    from libcontinual_amd import ops
    torch.manual_seed(5)
    D, m = 64, 40
    counts = [500, 37, 700, 1, 640, 500]
    feats = ops.l2_normalize_rows(torch.randn(sum(counts), D, device=DEV))
    got = ops.herding_select_classes(feats, counts, m)
    o = 0
    for c, g in zip(counts, got):
        want = ops.herding_select(feats[o:o + c], m)
        assert g.shape[0] == min(m, c)
        assert torch.equal(g, want), (c, g.tolist(), want.tolist())
        o += c


@pytest.mark.parametrize("rep", [1, 2, 8, 16, 32, 64])
@pytest.mark.parametrize("shape", [(5, 6, 6, 16), (3, 7, 9, 64), (3, 5, 5, 128), (2, 3, 3, 512), (2, 2, 3, 2048)])
def test_batchnorm_accumulator_replicas(shape, rep):
    """The consumers of the fp64 accumulators sum the replicas themselves: every replica count the plan can choose (1 .. 64), narrow layers
    (2 C <= 128: the replicas are split over thread groups and combined through LDS) and wide ones (several channels per thread, more
    than eight loads per chain), forward (scale / shift / saved statistics / running statistics) and backward (the two means, dgamma /
    dbeta added ONCE) against fp64."""
    N, H, W, C = shape
    code, tdt = DT["bf16"]
    M = N * H * W
    z = quant(rnd((N, C, H, W), 40, 2.0) + 0.3, tdt)
    dy = quant(rnd((N, C, H, W), 41), tdt)
    gamma, beta = rnd((C,), 42) * 0.5 + 1.0, rnd((C,), 43) * 0.2
    zd, dyd, gd, bd = to_nhwc(z, tdt), to_nhwc(dy, tdt), gamma.to(DEV), beta.to(DEV)
    z2 = z.double().permute(0, 2, 3, 1).reshape(M, C)
    full = torch.stack([z2.sum(0), (z2 * z2).sum(0)])
    wts = torch.arange(1, rep + 1, dtype=torch.float64)
    wts = wts / wts.sum()
    acc = torch.stack([full * f for f in wts]).to(DEV)                              # [rep, 2, C]: the sums split unevenly over the replicas
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    mean, invstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    y = torch.empty(N, H, W, C, dtype=tdt, device=DEV)
    call("clhip_bn_apply_train", zd.data_ptr(), acc.data_ptr(), rep, M, C, gd.data_ptr(), bd.data_ptr(), rm.data_ptr(), rv.data_ptr(), 0.1, 1e-5,
         mean.data_ptr(), invstd.data_ptr(), None, y.data_ptr(), 1, code, st())
    zr = z.double().clone().requires_grad_(True)
    g64, b64 = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    rm64, rv64 = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    ybn = F.batch_norm(zr, rm64, rv64, g64, b64, True, 0.1, 1e-5)
    yref = F.relu(ybn.detach())
    assert (from_nhwc(y).double() - yref).abs().max() <= tol("bf16", yref)
    assert torch.allclose(mean.cpu().double(), z2.mean(0), rtol=1e-5, atol=1e-6)
    assert torch.allclose(rm.cpu().double(), rm64, rtol=1e-5, atol=1e-6) and torch.allclose(rv.cpu().double(), rv64, rtol=1e-4, atol=1e-6)
    (ybn * (from_nhwc(y) > 0).double()).backward(dy.double())                      # the ReLU mask of the device's stored y, as above
    for entry in ("pair", "zmask"):
        bacc = torch.zeros(rep, 2, C, dtype=torch.float64, device=DEV)
        dg, db = torch.full((C,), 0.5, device=DEV), torch.full((C,), -0.25, device=DEV)      # the launch ADDS to these
        dz = torch.empty(N, H, W, C, dtype=tdt, device=DEV)
        if entry == "pair":
            call("clhip_bn_bwd_acc", dyd.data_ptr(), y.data_ptr(), zd.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gd.data_ptr(), dg.data_ptr(),
                 db.data_ptr(), dz.data_ptr(), None, 0, M, C, 1, bacc.data_ptr(), rep, code, st())
        else:
            call("clhip_bn_bwd_acc_zmask", dyd.data_ptr(), zd.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gd.data_ptr(), bd.data_ptr(), dg.data_ptr(),
                 db.data_ptr(), dz.data_ptr(), M, C, bacc.data_ptr(), rep, code, st())
        assert (from_nhwc(dz).double() - zr.grad).abs().max() <= tol("bf16", zr.grad) * 2
        assert (dg.cpu().double() - 0.5 - g64.grad).abs().max() <= 2e-3 * (g64.grad.abs().max() + 1e-9) + 1e-4
        assert (db.cpu().double() + 0.25 - b64.grad).abs().max() <= 2e-3 * (b64.grad.abs().max() + 1e-9) + 1e-4


@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("shape", [(8, 16, 16, 64, 64, 3, 1), (4, 16, 16, 64, 128, 3, 2), (4, 8, 8, 32, 64, 1, 2), (16, 32, 32, 8, 16, 3, 1),
                                   (5, 32, 32, 8, 64, 3, 1), (3, 7, 5, 8, 32, 3, 1), (130, 32, 32, 8, 64, 3, 1),        # stem.hip (ragged last tile, odd image, many tiles per wave)
                                   (6, 16, 16, 64, 128, 1, 2), (5, 8, 8, 128, 256, 1, 2), (3, 4, 4, 256, 512, 1, 2), (7, 6, 10, 64, 64, 1, 2)])      # the shortcuts
def test_conv_fwd_stat_accumulator(mode, shape):
    """clhip_conv_fwd_acc: same z as clhip_conv_fwd, per-channel sums of z and z^2 added into a zeroed fp64 [2][K] buffer
    (= the column sums of the partial rows of the partial-buffer entry point)"""
    N, H, W, C, K, ks, stride = shape
    code, tdt = DT[mode]
    pad = 1 if ks == 3 else 0
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    x = (torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(5)) * 0.5).to(tdt).to(DEV)
    w = (torch.randn(K, ks * ks, C, generator=torch.Generator().manual_seed(6)) * 0.1).to(tdt).to(DEV)
    tiles = _lib.lib().clhip_conv_fwd_tiles(N, H, W, C, K, ks, stride, pad)
    part = torch.empty(tiles, 2, K, device=DEV)
    z1 = torch.empty(N, Ho, Wo, K, dtype=tdt, device=DEV)
    z2 = torch.empty_like(z1)
    call("clhip_conv_fwd", x.data_ptr(), w.data_ptr(), z1.data_ptr(), part.data_ptr(), N, H, W, C, K, ks, stride, pad, code, st())
    ref = part.double().sum(0)
    for rep in (1, 4):
        acc = torch.zeros(rep, 2, K, dtype=torch.float64, device=DEV)
        call("clhip_conv_fwd_acc", x.data_ptr(), w.data_ptr(), z2.data_ptr(), acc.data_ptr(), rep, N, H, W, C, K, ks, stride, pad, code, st())
        torch.cuda.synchronize()
        conv64 = mode == "bf16" and C == 64 and K == 64 and ks == 3 and stride == 1 and W <= 16 and N * H * W <= 32768      # conv3.hip's register-resident 64 -> 64 kernel
        if (mode == "bf16" and C == 8 and ks == 3 and stride == 1) or conv64:       # stem.hip / conv64 serve the accumulator form, another kernel the partial rows
            assert (z1.float() - z2.float()).abs().max() <= 2 ** -7 * z1.float().abs().max()
            xr, wr = x.float().cpu().double().permute(0, 3, 1, 2), w.float().cpu().double().reshape(K, ks, ks, C).permute(0, 3, 1, 2)
            zr = F.conv2d(xr, wr, None, stride, pad)
            assert (z2.float().cpu().double().permute(0, 3, 1, 2) - zr).abs().max() <= 2 ** -8 * zr.abs().max() + 1e-6
            assert float((acc.sum(0)[0].cpu() - zr.sum(dim=(0, 2, 3))).abs().max()) <= 1e-4 * float(zr.abs().sum(dim=(0, 2, 3)).max())
            assert float((acc.sum(0)[1].cpu() - (zr * zr).sum(dim=(0, 2, 3))).abs().max()) <= 1e-4 * float((zr * zr).sum(dim=(0, 2, 3)).max())
            assert float((acc.sum(0) - ref).abs().max()) <= 1e-4 * float(ref.abs().max())       # two kernels, two summation orders
        else:
            assert torch.equal(z1, z2)
            assert float((acc.sum(0) - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
        dedicated = mode == "bf16" and C == 8 and ks == 3 and stride == 1
        if rep > 1 and tiles >= rep and not dedicated:          # (`tiles` counts the generic kernel's workgroups)
            assert (acc.abs().amax(dim=(1, 2)) > 0).all()          # every replica received some workgroups


@pytest.mark.parametrize("shape", [(8, 16, 16, 64, 64), (4, 8, 8, 128, 256), (6, 4, 4, 512, 512), (3, 12, 20, 64, 128), (32, 8, 8, 64, 64),
                                   # the register-resident 16 -> 16 / 32 -> 32 kernels (conv3.hip conv16 / conv32): several tiles, ragged tile, odd image
                                   (9, 32, 32, 16, 16), (33, 16, 16, 32, 32), (3, 7, 5, 16, 16), (2, 5, 9, 32, 32)])
@pytest.mark.parametrize("relu,accumulate", [(1, 0), (1, 1), (0, 0)])
def test_dgrad_with_fused_batchnorm_backward_reduction(shape, relu, accumulate):
    """clhip_conv_dgrad_bn_reduce + clhip_bn_bwd_apply_acc (the dgrad epilogue accumulates sum g and sum g * xhat of the producing
    layer's BatchNorm backward from its fp32 results) against (a) the unfused pair clhip_conv_dgrad + clhip_bn_bwd_acc and (b) the
    fp64 math: dx, the two channel sums, dz, dgamma, dbeta, dres.  bf16 only (the fourth-generation kernel's domain); tiles that end
    inside an image, the K-split configurations (8x8, 4x4 images) and the accumulate path (dx += ...) included."""
    N, H, W, C, K = shape
    assert _lib.lib().clhip_conv_dgrad_bn_reduce_supported(N, H, W, C, K, 3, 1, 1, DT["bf16"][0]) == 1
    assert _lib.lib().clhip_conv_route(3, 0, N, H, W, C, C, K, 3, 1, 1, DT["bf16"][0]) != _lib.CONV_CONV9          # (off by default)
    _bnr_case(shape, relu, accumulate)


@pytest.mark.parametrize("shape", [(4, 8, 8, 128, 128), (3, 16, 16, 128, 128), (3, 32, 32, 128, 128), (6, 8, 8, 256, 256), (3, 16, 16, 256, 256)])
@pytest.mark.parametrize("relu,accumulate", [(1, 0), (1, 1), (0, 0)])
def test_dgrad_with_fused_batchnorm_backward_reduction_conv9(shape, relu, accumulate):
    """... and the same on conv9.hip (128 -> 128 / 256 -> 256 channels, CONV9=1): tiles of four / two images, one, two and four tiles per image"""
    N, H, W, C, K = shape
    L = _lib.lib()
    assert L.clhip_config(b"CONV9", b"1") == 0
    try:
        assert L.clhip_conv_route(3, 0, N, H, W, C, C, K, 3, 1, 1, DT["bf16"][0]) == _lib.CONV_CONV9
        _bnr_case(shape, relu, accumulate)
    finally:
        L.clhip_config(b"CONV9", None)


def _bnr_case(shape, relu, accumulate):
    N, H, W, C, K = shape
    code, tdt = DT["bf16"]
    M = N * H * W
    dzn = quant(rnd((N, K, H, W), 31, 0.5), tdt)                       # gradient entering the convolution's output
    wd = quant(rnd((C, 9, K), 32, 0.05), tdt)                          # dgrad weight copy [C][taps][K]
    zp = quant(rnd((N, C, H, W), 33, 1.5) + 0.2, tdt)                  # producing layer: pre-BN output, post-activation output
    yp = quant(torch.relu(rnd((N, C, H, W), 34)), tdt) if relu else quant(rnd((N, C, H, W), 34), tdt)
    old = quant(rnd((N, C, H, W), 35, 0.3), tdt)                       # what an earlier consumer left in dx
    mean, invstd = rnd((C,), 36) * 0.3, rnd((C,), 37).abs() + 0.5
    gamma, beta = rnd((C,), 38) * 0.5 + 1.0, rnd((C,), 39) * 0.2
    d = lambda t: t.to(DEV)
    dzd, wdd, zpd, ypd = to_nhwc(dzn, tdt), wd.to(tdt).to(DEV).contiguous(), to_nhwc(zp, tdt), to_nhwc(yp, tdt)
    md, isd, gd, bd = d(mean), d(invstd), d(gamma), d(beta)
    rep = 4

    def run(fused):
        dx = to_nhwc(old, tdt).clone() if accumulate else torch.full((N, H, W, C), float("nan"), dtype=tdt, device=DEV)
        acc = torch.zeros(rep, 2, C, dtype=torch.float64, device=DEV)
        dgam, dbet = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        dzo = torch.empty(N, H, W, C, dtype=tdt, device=DEV)
        if fused:
            call("clhip_conv_dgrad_bn_reduce", dzd.data_ptr(), wdd.data_ptr(), dx.data_ptr(), accumulate, zpd.data_ptr(), ypd.data_ptr() if relu else None,
                 md.data_ptr(), isd.data_ptr(), acc.data_ptr(), rep, N, H, W, C, K, 3, 1, 1, code, st())
            sums = acc.sum(0).cpu()
            call("clhip_bn_bwd_apply_acc", dx.data_ptr(), ypd.data_ptr() if relu else None, zpd.data_ptr(), md.data_ptr(), isd.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                 dgam.data_ptr(), dbet.data_ptr(), dzo.data_ptr(), None, 0, M, C, relu, acc.data_ptr(), rep, code, st())
        else:
            call("clhip_conv_dgrad", dzd.data_ptr(), wdd.data_ptr(), dx.data_ptr(), accumulate, N, H, W, C, K, 3, 1, 1, code, st())
            call("clhip_bn_bwd_acc", dx.data_ptr(), ypd.data_ptr(), zpd.data_ptr(), md.data_ptr(), isd.data_ptr(), gd.data_ptr(), dgam.data_ptr(), dbet.data_ptr(),
                 dzo.data_ptr(), None, 0, M, C, relu, acc.data_ptr(), rep, code, st())
            sums = acc.sum(0).cpu()
        torch.cuda.synchronize()
        return from_nhwc(dx).double(), sums, from_nhwc(dzo).double(), dgam.cpu().double(), dbet.cpu().double()

    dx_f, s_f, dz_f, dg_f, db_f = run(True)
    dx_u, s_u, dz_u, dg_u, db_u = run(False)
    # fp64 reference of the dgrad: dx[n,c,h,w] = sum_{r,s,o} dz[n,o,h+1-r,w+1-s] * wd[c][3r+s][o]
    w4 = wd.double().reshape(C, 3, 3, K).permute(3, 0, 1, 2).contiguous()           # [K][C][3][3] = the forward weight of a C -> K convolution
    dx_ref = F.conv_transpose2d(dzn.double(), w4, padding=1)
    if accumulate:
        dx_ref = dx_ref + old.double()
    assert torch.equal(dx_f, dx_u)                                                   # the stored gradient is the same bf16 tensor either way
    assert (dx_f - dx_ref).abs().max() <= tol("bf16", dx_ref) * 1.5
    mask = (yp.double() > 0).double() if relu else torch.ones_like(dx_ref)
    g = dx_ref * mask
    xhat = (zp.double() - mean.double().view(1, C, 1, 1)) * invstd.double().view(1, C, 1, 1)
    s_ref = torch.stack([g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))])
    scale = torch.stack([g.abs().sum((0, 2, 3)), (g * xhat).abs().sum((0, 2, 3))]) + 1e-9
    assert ((s_f - s_ref).abs() / scale).max() < 4e-3                                # sums of the fp32 results before rounding
    assert ((s_u - s_ref).abs() / scale).max() < 4e-3                                # sums of the rounded tensor (unfused pass)
    gi = (gamma * invstd).double().view(1, C, 1, 1)
    dz_ref = gi * (g - s_ref[0].view(1, C, 1, 1) / M - xhat * s_ref[1].view(1, C, 1, 1) / M)
    assert (dz_f - dz_ref).abs().max() <= tol("bf16", dz_ref) * 2.5
    assert (dz_f - dz_u).abs().max() <= tol("bf16", dz_ref) * 2.5
    assert (dg_f - s_ref[1]).abs().max() <= 4e-3 * scale[1].max()
    assert (db_f - s_ref[0]).abs().max() <= 4e-3 * scale[0].max()


PAIR_CASES = [(256, 32, 32, 64, 128), (20, 32, 32, 64, 128), (3, 32, 32, 64, 128), (70, 16, 16, 128, 256), (256, 8, 8, 256, 512), (9, 8, 8, 256, 512),
              (33, 4, 4, 64, 64), (9, 16, 8, 64, 32),
              # conv7.hip: CifarResNet-32's entries (16 -> 32 at 32 x 32, 32 -> 64 at 16 x 16), ragged last tiles, one tile, non-square maps
              (256, 32, 32, 16, 32), (256, 16, 16, 32, 64), (3, 32, 32, 16, 32), (5, 16, 16, 32, 64), (1, 4, 8, 16, 32), (7, 8, 4, 32, 64)]


@pytest.mark.parametrize("case", PAIR_CASES)
def test_stride2_dgrad_pair_one_launch(case):
    """conv6.hip: the input gradient of a down-sampling block entry -- dgrad of the 3x3 / s2 / p1 convolution + dgrad of the 1x1 / s2
    shortcut, both classes of accumulators in one launch -- against the fp64 transposed convolutions and against the two separate
    launches it replaces; with and without the shortcut operand, with accumulation; ResNet-18's three entries at batch 256, ragged
    last tiles, tiles spanning images, 256- and 128-pixel workgroups, non-square maps."""
    N, H, W, C, K = case
    code, tdt = DT["bf16"]
    L = _lib.lib()
    assert L.clhip_conv_dgrad_pair_supported(N, H, W, C, K, code) == 1
    Ho, Wo = H // 2, W // 2
    w3 = quant(rnd((K, C, 3, 3), 5, 1.0 / (K * 9) ** 0.5), tdt)
    w1 = quant(rnd((K, C, 1, 1), 8, 1.0 / K ** 0.5), tdt)
    dz = quant(rnd((N, K, Ho, Wo), 6), tdt)
    dzs = quant(rnd((N, K, Ho, Wo), 9), tdt)
    xr = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w3.double(), None, 2, 1).backward(dz.double())
    ref3 = xr.grad.clone()
    xr.grad = None
    F.conv2d(xr, w1.double(), None, 2, 0).backward(dzs.double())
    ref1 = xr.grad.clone()
    w3d = w3.permute(1, 2, 3, 0).contiguous().to(tdt).to(DEV)
    w1d = w1.permute(1, 2, 3, 0).contiguous().to(tdt).to(DEV)
    dzd, dzsd = to_nhwc(dz, tdt), to_nhwc(dzs, tdt)
    pk = torch.full((L.clhip_conv_dgrad_pair_packed_bytes(C, K),), 0x7f, dtype=torch.uint8, device=DEV)
    pk3 = torch.full_like(pk, 0x7f)                                   # (0x7f7f = a large bf16: an unwritten slot that is read shows)
    call("clhip_conv_dgrad_pair_pack", w3d.data_ptr(), w1d.data_ptr(), pk.data_ptr(), C, K, code, st())
    call("clhip_conv_dgrad_pair_pack", w3d.data_ptr(), None, pk3.data_ptr(), C, K, code, st())
    dx = torch.full((N, H, W, C), float("nan"), dtype=tdt, device=DEV)
    call("clhip_conv_dgrad_pair", dzd.data_ptr(), pk.data_ptr(), dzsd.data_ptr(), dx.data_ptr(), 0, N, H, W, C, K, code, st())
    ref = ref3 + ref1
    assert (from_nhwc(dx).double() - ref).abs().max() <= tol("bf16", ref)
    # the two launches it replaces (shortcut first, then the 3x3 layer accumulating): equal up to the bf16 rounding of the intermediate
    two = torch.full((N, H, W, C), float("nan"), dtype=tdt, device=DEV)
    call("clhip_conv_dgrad", dzsd.data_ptr(), w1d.data_ptr(), two.data_ptr(), 0, N, H, W, C, K, 1, 2, 0, code, st())
    call("clhip_conv_dgrad", dzd.data_ptr(), w3d.data_ptr(), two.data_ptr(), 1, N, H, W, C, K, 3, 2, 1, code, st())
    assert (dx.float() - two.float()).abs().max() <= 2 ** -6 * ref.abs().max()
    if L.clhip_conv_dgrad_pair_bn_reduce_supported(N, H, W, C, K, code):
        # the same launch with the BatchNorm-backward sums of the layer that produced the block input in its epilogue: dx bit-identical, the sums
        # against fp64 from the unrounded reference (sum g, sum g xhat; g = dx masked by that layer's ReLU)
        zp = quant(rnd((N, C, H, W), 31, 1.2), tdt)
        yp = quant(torch.relu(rnd((N, C, H, W), 32) + 0.1), tdt)
        mean, var = zp.double().mean((0, 2, 3)), zp.double().var((0, 2, 3), unbiased=False)
        invstd = 1.0 / torch.sqrt(var + 1e-5)
        meand, invd = mean.float().to(DEV), invstd.float().to(DEV)
        acc = torch.zeros(4, 2, C, dtype=torch.float64, device=DEV)
        dxb = torch.full((N, H, W, C), float("nan"), dtype=tdt, device=DEV)
        zpd, ypd = to_nhwc(zp, tdt), to_nhwc(yp, tdt)
        call("clhip_conv_dgrad_pair_bn_reduce", dzd.data_ptr(), pk.data_ptr(), dzsd.data_ptr(), dxb.data_ptr(), 0, zpd.data_ptr(), ypd.data_ptr(),
             meand.data_ptr(), invd.data_ptr(), acc.data_ptr(), 4, N, H, W, C, K, code, st())
        torch.cuda.synchronize()
        assert torch.equal(dxb, dx)
        g = ref * (yp.double() > 0)
        xhat = (zp.double() - meand.cpu().double().view(1, C, 1, 1)) * invd.cpu().double().view(1, C, 1, 1)
        s = acc.sum(0).cpu()
        scale = g.abs().sum((0, 2, 3)).max()
        assert (s[0] - g.sum((0, 2, 3))).abs().max() <= 1e-5 * scale + 1e-6
        assert (s[1] - (g * xhat).sum((0, 2, 3))).abs().max() <= 1e-5 * (g.abs() * xhat.abs()).sum((0, 2, 3)).max() + 1e-6
    # without the shortcut operand; with accumulation
    dx3 = torch.full((N, H, W, C), float("nan"), dtype=tdt, device=DEV)
    call("clhip_conv_dgrad_pair", dzd.data_ptr(), pk3.data_ptr(), None, dx3.data_ptr(), 0, N, H, W, C, K, code, st())
    assert (from_nhwc(dx3).double() - ref3).abs().max() <= tol("bf16", ref3)
    base = quant(rnd((N, C, H, W), 7), tdt)
    dxa = to_nhwc(base, tdt)
    call("clhip_conv_dgrad_pair", dzd.data_ptr(), pk.data_ptr(), dzsd.data_ptr(), dxa.data_ptr(), 1, N, H, W, C, K, code, st())
    ref2 = ref + base.double()
    assert (from_nhwc(dxa).double() - ref2).abs().max() <= tol("bf16", ref2) * 1.5


@pytest.mark.parametrize("shape", [(9, 32, 32, 16), (40, 16, 16, 32), (3, 7, 5, 16), (5, 8, 16, 32), (70, 16, 16, 32), (9, 8, 8, 64), (70, 8, 8, 64), (3, 16, 8, 64),
                                   (256, 8, 8, 64)])
def test_lazy_batchnorm_input_forward_and_backward(shape):
    """VERDICT r2 item 1b on the kernels that stage their operand through registers (conv16 / conv32): the consumer convolution applies its
    producer's BatchNorm + ReLU while it loads the operand.  clhip_conv_fwd_acc_bn_input(z') must equal clhip_bn_apply_train(z') followed by
    clhip_conv_fwd_acc BIT FOR BIT (output, saved statistics, coefficients, running statistics; its own fp64 sums to the atomics' order), and
    clhip_conv_dgrad_wgrad_bn_input(z', coef) the fused backward on the materialised activation (dx, dw bit-identical; the producer's
    BatchNorm-backward sums with the ReLU mask taken from z')."""
    import ctypes as C

    class BnInput(C.Structure):
        _fields_ = [("stat_acc", C.c_void_p), ("replicas", C.c_int), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("running_mean", C.c_void_p),
                    ("running_var", C.c_void_p), ("momentum", C.c_float), ("eps", C.c_float), ("mean", C.c_void_p), ("invstd", C.c_void_p), ("coef", C.c_void_p)]
    N, H, W, Cc = shape
    L = _lib.lib()
    code, tdt = DT["bf16"]
    # the lazy input needs the layer's one-launch backward as well (32-wide images at 16 channels, 16-wide at 32, 8-wide at 64): (3, 7, 5, 16) is outside by design
    inside = W == {16: 32, 32: 16, 64: 8}[Cc]
    assert L.clhip_conv_bn_input_supported(N, H, W, Cc, Cc, 3, 1, 1, code) == (1 if inside else 0)
    if not inside:
        return
    M_ = N * H * W
    zp = to_nhwc(quant(rnd((N, Cc, H, W), 71, 1.3), tdt), tdt)                    # the producer's pre-BatchNorm output
    zf = zp.float().reshape(-1, Cc).double()
    rep_in = 4
    acc_in = torch.zeros(rep_in, 2, Cc, dtype=torch.float64, device=DEV)
    acc_in[1, 0], acc_in[2, 1] = zf.sum(0), (zf * zf).sum(0)                        # the sums its convolution would have left, spread over replicas
    gamma, beta = (rnd((Cc,), 72) * 0.2 + 1.0).to(DEV), (rnd((Cc,), 73) * 0.3).to(DEV)
    w = quant(rnd((Cc, 9, Cc), 74, 0.1), tdt).to(tdt).to(DEV).contiguous()
    mom, eps, rep = 0.1, 1e-5, 8

    def fresh():
        return dict(rm=torch.full((Cc,), 0.5, device=DEV), rv=torch.full((Cc,), 2.0, device=DEV), mean=torch.empty(Cc, device=DEV), invstd=torch.empty(Cc, device=DEV),
                    coef=torch.full((2, Cc), float("nan"), device=DEV), z=torch.full((N, H, W, Cc), float("nan"), dtype=tdt, device=DEV),
                    acc=torch.zeros(rep, 2, Cc, dtype=torch.float64, device=DEV))
    e, l = fresh(), fresh()
    # eager: apply launch, then the convolution on the activation
    y = torch.full((N, H, W, Cc), float("nan"), dtype=tdt, device=DEV)
    call("clhip_bn_apply_train", zp.data_ptr(), acc_in.data_ptr(), rep_in, M_, Cc, gamma.data_ptr(), beta.data_ptr(), e["rm"].data_ptr(), e["rv"].data_ptr(), mom, eps,
         e["mean"].data_ptr(), e["invstd"].data_ptr(), None, y.data_ptr(), 1, code, st())
    call("clhip_conv_fwd_acc", y.data_ptr(), w.data_ptr(), e["z"].data_ptr(), e["acc"].data_ptr(), rep, N, H, W, Cc, Cc, 3, 1, 1, code, st())
    # lazy: one launch
    bi = BnInput(acc_in.data_ptr(), rep_in, gamma.data_ptr(), beta.data_ptr(), l["rm"].data_ptr(), l["rv"].data_ptr(), mom, eps, l["mean"].data_ptr(),
                 l["invstd"].data_ptr(), l["coef"].data_ptr())
    call("clhip_conv_fwd_acc_bn_input", zp.data_ptr(), C.byref(bi), w.data_ptr(), l["z"].data_ptr(), l["acc"].data_ptr(), rep, N, H, W, Cc, Cc, 3, 1, 1, code, st())
    torch.cuda.synchronize()
    assert torch.equal(l["z"], e["z"])
    for k in ("rm", "rv", "mean", "invstd"):
        assert torch.equal(l[k], e[k]), k
    sc = gamma * l["invstd"]
    assert torch.equal(l["coef"][0], sc) and torch.allclose(l["coef"][1], beta - l["mean"] * sc, rtol=0, atol=1e-6)      # (the kernel's shift is one fma)
    assert ((l["acc"].sum(0) - e["acc"].sum(0)).abs() <= 1e-12 * e["acc"].sum(0).abs().clamp(min=1.0)).all()
    # ---- backward of the consumer: dgrad + weight gradient in one launch, the operand relu(bn(z')) recomputed on load
    dz = to_nhwc(quant(rnd((N, Cc, H, W), 75, 0.5), tdt), tdt)
    wd = quant(rnd((Cc, 9, Cc), 76, 0.1), tdt).to(tdt).to(DEV).contiguous()
    wsb = L.clhip_conv_wgrad_ws_bytes(N, H, W, Cc, Cc, Cc, 3, 1, 1, code)
    outs = []
    for lazy in (False, True):
        dx = torch.full((N, H, W, Cc), float("nan"), dtype=tdt, device=DEV)
        dw = torch.full((Cc, 9, Cc), 0.25, device=DEV)
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        sums = torch.zeros(4, 2, Cc, dtype=torch.float64, device=DEV)
        if lazy:
            call("clhip_conv_dgrad_wgrad_bn_input", zp.data_ptr(), l["coef"].data_ptr(), dz.data_ptr(), wd.data_ptr(), dx.data_ptr(), 0, dw.data_ptr(), ws.data_ptr(),
                 l["mean"].data_ptr(), l["invstd"].data_ptr(), sums.data_ptr(), 4, N, H, W, Cc, Cc, Cc, 3, 1, 1, code, st())
        else:
            call("clhip_conv_dgrad_wgrad", y.data_ptr(), dz.data_ptr(), wd.data_ptr(), dx.data_ptr(), 0, dw.data_ptr(), ws.data_ptr(), zp.data_ptr(), y.data_ptr(),
                 e["mean"].data_ptr(), e["invstd"].data_ptr(), sums.data_ptr(), 4, N, H, W, Cc, Cc, Cc, 3, 1, 1, code, st())
        torch.cuda.synchronize()
        outs.append((dx, dw, sums.sum(0)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # mask from z' (fma > 0) against mask from the stored activation: they differ only where a positive value underflows to bf16 zero
    assert ((outs[0][2] - outs[1][2]).abs() <= 1e-9 * outs[0][2].abs().clamp(min=1.0)).all()
    # ---- the layer's OWN BatchNorm backward on the operand loads of its fused dgrad + weight-gradient launch (clhip_conv_dgrad_wgrad_bn_grad)
    # against clhip_bn_bwd_apply_acc (z-mask form) followed by clhip_conv_dgrad_wgrad: dx, dw, dgamma, dbeta bit for bit

    class BnGrad(C.Structure):
        _fields_ = [("dy", C.c_void_p), ("z", C.c_void_p), ("sums", C.c_void_p), ("replicas", C.c_int), ("mean", C.c_void_p), ("invstd", C.c_void_p),
                    ("gamma", C.c_void_p), ("beta", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("relu_mask", C.c_void_p), ("dres", C.c_void_p),
                    ("dres_accumulate", C.c_int)]
    xin = to_nhwc(quant(rnd((N, Cc, H, W), 77), tdt), tdt)                          # this layer's input
    dy = to_nhwc(quant(rnd((N, Cc, H, W), 78, 0.5), tdt), tdt)                      # gradient of its activation
    gsum = torch.zeros(4, 2, Cc, dtype=torch.float64, device=DEV)                   # sum g, sum g xhat as a consumer's epilogue leaves them
    zfl = zp.float().reshape(-1, Cc)
    gmask = (torch.addcmul(l["coef"][1], zfl, l["coef"][0]) > 0).float() * dy.float().reshape(-1, Cc)
    xhat = (zfl - l["mean"]) * l["invstd"]
    gsum[0, 0], gsum[3, 1] = gmask.double().sum(0), (gmask * xhat).double().sum(0)
    res = []
    for fused in (False, True):
        dx = torch.full((N, H, W, Cc), float("nan"), dtype=tdt, device=DEV)
        dw = torch.full((Cc, 9, Cc), 0.25, device=DEV)
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        dgam, dbet = torch.full((Cc,), 0.5, device=DEV), torch.full((Cc,), -0.25, device=DEV)
        if fused:
            bg = BnGrad(dy.data_ptr(), zp.data_ptr(), gsum.data_ptr(), 4, l["mean"].data_ptr(), l["invstd"].data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                        dgam.data_ptr(), dbet.data_ptr(), None, None, 0)
            call("clhip_conv_dgrad_wgrad_bn_grad", xin.data_ptr(), None, C.byref(bg), wd.data_ptr(), dx.data_ptr(), 0, dw.data_ptr(), ws.data_ptr(), None, None, None, None,
                 None, 1, N, H, W, Cc, Cc, Cc, 3, 1, 1, code, st())
        else:
            dzt = torch.full((N, H, W, Cc), float("nan"), dtype=tdt, device=DEV)
            call("clhip_bn_bwd_apply_acc", dy.data_ptr(), None, zp.data_ptr(), l["mean"].data_ptr(), l["invstd"].data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                 dgam.data_ptr(), dbet.data_ptr(), dzt.data_ptr(), None, 0, M_, Cc, 2, gsum.data_ptr(), 4, code, st())
            call("clhip_conv_dgrad_wgrad", xin.data_ptr(), dzt.data_ptr(), wd.data_ptr(), dx.data_ptr(), 0, dw.data_ptr(), ws.data_ptr(), None, None, None, None,
                 None, 1, N, H, W, Cc, Cc, Cc, 3, 1, 1, code, st())
        torch.cuda.synchronize()
        res.append((dx, dw, dgam, dbet))
    for a_, b_ in zip(res[0], res[1]):
        assert torch.equal(a_, b_)
    # ---- the +res form: conv -> BN -> +res -> ReLU with the forward's packed mask; the launch also writes / accumulates the residual gradient;
    # its input here is itself a lazy activation (x = relu(bn(zin)) from coefficients): everything a ResNet-32 block's second unit needs at once
    zin = to_nhwc(quant(rnd((N, Cc, H, W), 79, 1.2), tdt), tdt)
    xmat = torch.full((N, H, W, Cc), float("nan"), dtype=tdt, device=DEV)
    call("clhip_bn_apply", zin.data_ptr(), l["coef"][0].contiguous().data_ptr(), l["coef"][1].contiguous().data_ptr(), None, xmat.data_ptr(), M_, Cc, 1, code, st())
    mask = torch.randint(0, 256, (M_ * Cc // 8,), dtype=torch.uint8, device=DEV)
    mbits = ((mask.long()[:, None] >> torch.arange(8, device=DEV)) & 1).reshape(-1, Cc).float()
    gm = mbits * dy.float().reshape(-1, Cc)
    gsum2 = torch.zeros(4, 2, Cc, dtype=torch.float64, device=DEV)
    gsum2[1, 0], gsum2[2, 1] = gm.double().sum(0), (gm * xhat).double().sum(0)
    for accumulate in (0, 1):
        res = []
        for fused in (False, True):
            dx = torch.full((N, H, W, Cc), float("nan"), dtype=tdt, device=DEV)
            dw = torch.full((Cc, 9, Cc), 0.25, device=DEV)
            ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
            dgam, dbet = torch.full((Cc,), 0.5, device=DEV), torch.full((Cc,), -0.25, device=DEV)
            dres = to_nhwc(quant(rnd((N, Cc, H, W), 80, 0.4), tdt), tdt)
            psum = torch.zeros(4, 2, Cc, dtype=torch.float64, device=DEV)                  # the producer's sums out of the dgrad epilogue
            if fused:
                bg = BnGrad(dy.data_ptr(), zp.data_ptr(), gsum2.data_ptr(), 4, l["mean"].data_ptr(), l["invstd"].data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                            dgam.data_ptr(), dbet.data_ptr(), mask.data_ptr(), dres.data_ptr(), accumulate)
                call("clhip_conv_dgrad_wgrad_bn_grad", zin.data_ptr(), l["coef"].data_ptr(), C.byref(bg), wd.data_ptr(), dx.data_ptr(), 0, dw.data_ptr(), ws.data_ptr(),
                     zin.data_ptr(), None, l["mean"].data_ptr(), l["invstd"].data_ptr(), psum.data_ptr(), 4, N, H, W, Cc, Cc, Cc, 3, 1, 1, code, st())
            else:
                dzt = torch.full((N, H, W, Cc), float("nan"), dtype=tdt, device=DEV)
                call("clhip_bn_bwd_apply_acc", dy.data_ptr(), mask.data_ptr(), zp.data_ptr(), l["mean"].data_ptr(), l["invstd"].data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                     dgam.data_ptr(), dbet.data_ptr(), dzt.data_ptr(), dres.data_ptr(), accumulate, M_, Cc, 3, gsum2.data_ptr(), 4, code, st())
                call("clhip_conv_dgrad_wgrad_bn_input", zin.data_ptr(), l["coef"].data_ptr(), dzt.data_ptr(), wd.data_ptr(), dx.data_ptr(), 0, dw.data_ptr(), ws.data_ptr(),
                     l["mean"].data_ptr(), l["invstd"].data_ptr(), psum.data_ptr(), 4, N, H, W, Cc, Cc, Cc, 3, 1, 1, code, st())
            torch.cuda.synchronize()
            res.append((dx, dw, dgam, dbet, dres, psum.sum(0)))
        for k_, (a_, b_) in enumerate(zip(res[0][:5], res[1][:5])):
            assert torch.equal(a_, b_), (accumulate, k_)
        assert ((res[0][5] - res[1][5]).abs() <= 1e-12 * res[0][5].abs().clamp(min=1.0)).all()


@pytest.mark.parametrize("shape", [(9, 32, 32, 16), (40, 16, 16, 32), (3, 7, 5, 16), (5, 8, 16, 32), (70, 8, 8, 64), (3, 16, 8, 64), (256, 8, 8, 64)])
def test_lazy_batchnorm_residual_input(shape):
    """The last unit of a basic block (conv -> BN -> +res -> ReLU, resnet.py:312-316) applied by its first consumer: clhip_conv_fwd_acc_bn_res_input(z',
    res) must equal clhip_bn_apply_train_mask(z', res) followed by clhip_conv_fwd_acc BIT FOR BIT -- the convolution's output, the activation and the
    packed ReLU mask it writes for the later readers (guard elements behind both stay untouched), the saved and the running statistics."""
    import ctypes as C

    class BnInput(C.Structure):
        _fields_ = [("stat_acc", C.c_void_p), ("replicas", C.c_int), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("running_mean", C.c_void_p),
                    ("running_var", C.c_void_p), ("momentum", C.c_float), ("eps", C.c_float), ("mean", C.c_void_p), ("invstd", C.c_void_p), ("coef", C.c_void_p)]

    class BnRes(C.Structure):
        _fields_ = [("res", C.c_void_p), ("y", C.c_void_p), ("relu_mask", C.c_void_p)]
    N, H, W, Cc = shape
    L = _lib.lib()
    code, tdt = DT["bf16"]
    # the lazy input needs the layer's one-launch backward as well (32-wide images at 16 channels, 16-wide at 32, 8-wide at 64): (3, 7, 5, 16) is outside by design
    inside = W == {16: 32, 32: 16, 64: 8}[Cc]
    assert L.clhip_conv_bn_input_supported(N, H, W, Cc, Cc, 3, 1, 1, code) == (1 if inside else 0)
    if not inside:
        return
    M_ = N * H * W
    zp = to_nhwc(quant(rnd((N, Cc, H, W), 81, 1.3), tdt), tdt)
    rs_t = to_nhwc(quant(rnd((N, Cc, H, W), 82, 0.8), tdt), tdt)                   # the residual
    zf = zp.float().reshape(-1, Cc).double()
    rep_in = 4
    acc_in = torch.zeros(rep_in, 2, Cc, dtype=torch.float64, device=DEV)
    acc_in[0, 0], acc_in[3, 1] = zf.sum(0), (zf * zf).sum(0)
    gamma, beta = (rnd((Cc,), 83) * 0.2 + 1.0).to(DEV), (rnd((Cc,), 84) * 0.3).to(DEV)
    w = quant(rnd((Cc, 9, Cc), 85, 0.1), tdt).to(tdt).to(DEV).contiguous()
    mom, eps, rep = 0.1, 1e-5, 8
    nmask = M_ * Cc // 8

    def fresh():
        return dict(rm=torch.full((Cc,), 0.5, device=DEV), rv=torch.full((Cc,), 2.0, device=DEV), mean=torch.empty(Cc, device=DEV), invstd=torch.empty(Cc, device=DEV),
                    coef=torch.full((2, Cc), float("nan"), device=DEV), z=torch.full((N, H, W, Cc), float("nan"), dtype=tdt, device=DEV),
                    acc=torch.zeros(rep, 2, Cc, dtype=torch.float64, device=DEV), y=torch.full((M_ + 1, Cc), 7.0, dtype=tdt, device=DEV),
                    mask=torch.full((nmask + 16,), 0xA5, dtype=torch.uint8, device=DEV))
    e, l = fresh(), fresh()
    call("clhip_bn_apply_train_mask", zp.data_ptr(), acc_in.data_ptr(), rep_in, M_, Cc, gamma.data_ptr(), beta.data_ptr(), e["rm"].data_ptr(), e["rv"].data_ptr(), mom, eps,
         e["mean"].data_ptr(), e["invstd"].data_ptr(), rs_t.data_ptr(), e["y"].data_ptr(), e["mask"].data_ptr(), code, st())
    call("clhip_conv_fwd_acc", e["y"].data_ptr(), w.data_ptr(), e["z"].data_ptr(), e["acc"].data_ptr(), rep, N, H, W, Cc, Cc, 3, 1, 1, code, st())
    bi = BnInput(acc_in.data_ptr(), rep_in, gamma.data_ptr(), beta.data_ptr(), l["rm"].data_ptr(), l["rv"].data_ptr(), mom, eps, l["mean"].data_ptr(),
                 l["invstd"].data_ptr(), l["coef"].data_ptr())
    br = BnRes(rs_t.data_ptr(), l["y"].data_ptr(), l["mask"].data_ptr())
    call("clhip_conv_fwd_acc_bn_res_input", zp.data_ptr(), C.byref(bi), C.byref(br), w.data_ptr(), l["z"].data_ptr(), l["acc"].data_ptr(), rep, N, H, W, Cc, Cc, 3, 1, 1,
         code, st())
    torch.cuda.synchronize()
    assert torch.equal(l["y"], e["y"]) and float((l["y"][M_].float() - 7.0).abs().max()) == 0.0
    assert torch.equal(l["mask"], e["mask"]) and bool((l["mask"][nmask:] == 0xA5).all())
    assert int(e["mask"][:nmask].count_nonzero()) > 0 and int((e["y"][:M_] == 0).sum()) > 0      # both signs occur
    assert torch.equal(l["z"], e["z"])
    for k in ("rm", "rv", "mean", "invstd"):
        assert torch.equal(l[k], e[k]), k
    assert ((l["acc"].sum(0) - e["acc"].sum(0)).abs() <= 1e-12 * e["acc"].sum(0).abs().clamp(min=1.0)).all()


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("shape", [(160, 32, 32, 64, 64), (131, 32, 32, 64, 64), (256, 16, 16, 128, 128), (70, 16, 16, 128, 128), (256, 8, 8, 256, 256),
                                   (256, 4, 4, 512, 512), (32, 8, 8, 256, 256), (64, 16, 16, 64, 128), (24, 32, 32, 64, 64)])
def test_lazy_batchnorm_input_write_through(shape, with_res):
    """Round 4: the producer's BatchNorm [+ residual] + ReLU applied by the consumer convolution of a WIDE layer on its landed patch in LDS
    (conv4.hip / conv5.hip, the kernels that stage by LDS-DMA), the activation [and packed mask] written by the same launch:
    clhip_conv_fwd_acc_bn_input_wt(z', [res]) must equal clhip_bn_apply_train[_mask](z', [res]) followed by clhip_conv_fwd_acc BIT FOR BIT -- the
    convolution's output, the activation, the mask, guard elements behind them untouched, saved / running statistics (resnet.py:289-316)."""
    import ctypes as C

    class BnInput(C.Structure):
        _fields_ = [("stat_acc", C.c_void_p), ("replicas", C.c_int), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("running_mean", C.c_void_p),
                    ("running_var", C.c_void_p), ("momentum", C.c_float), ("eps", C.c_float), ("mean", C.c_void_p), ("invstd", C.c_void_p), ("coef", C.c_void_p)]

    class BnRes(C.Structure):
        _fields_ = [("res", C.c_void_p), ("y", C.c_void_p), ("relu_mask", C.c_void_p)]
    N, H, W, Cc, K = shape
    L = _lib.lib()
    code, tdt = DT["bf16"]
    assert L.clhip_config(b"BN_INPUT_WT", b"1") == 0                  # (off by default: it did not pay inside the step, profiles/r04_wt_notes.md)
    nine = Cc == K and Cc in (128, 256)                              # conv9.hip's layers: the write-through form exists on it alone (CONV9=1; conv4.hip has no lazy input)
    try:
        if nine:
            assert L.clhip_conv_bn_input_wt_supported(N, H, W, Cc, K, 3, 1, 1, code) == 0
            assert L.clhip_config(b"CONV9", b"1") == 0
            assert L.clhip_conv_route(4, 0, N, H, W, Cc, Cc, K, 3, 1, 1, code) == _lib.CONV_CONV9
        # outside the domain by design: 512 channels and 64 -> 128 channels (conv4.hip only), 64 -> 64 below conv5.hip's 512 tiles (24 x 32 x 32: 96)
        inside = nine or (Cc == 64 and K == 64 and N * H * W >= 512 * 256)
        assert L.clhip_conv_bn_input_wt_supported(N, H, W, Cc, K, 3, 1, 1, code) == (1 if inside else 0)
        if inside:
            _wt_case(L, C, BnInput, BnRes, N, H, W, Cc, K, code, tdt, with_res)
    finally:
        L.clhip_config(b"BN_INPUT_WT", None)
        L.clhip_config(b"CONV9", None)


def _wt_case(L, C, BnInput, BnRes, N, H, W, Cc, K, code, tdt, with_res):
    M_ = N * H * W
    zp = to_nhwc(quant(rnd((N, Cc, H, W), 81, 1.3), tdt), tdt)
    rs_t = to_nhwc(quant(rnd((N, Cc, H, W), 82, 0.8), tdt), tdt) if with_res else None
    zf = zp.float().reshape(-1, Cc).double()
    rep_in = 4
    acc_in = torch.zeros(rep_in, 2, Cc, dtype=torch.float64, device=DEV)
    acc_in[0, 0], acc_in[3, 1] = zf.sum(0), (zf * zf).sum(0)
    gamma, beta = (rnd((Cc,), 83) * 0.2 + 1.0).to(DEV), (rnd((Cc,), 84) * 0.3).to(DEV)
    w = quant(rnd((K, 9, Cc), 85, 0.05), tdt).to(tdt).to(DEV).contiguous()
    mom, eps, rep = 0.1, 1e-5, 8
    nmask = M_ * Cc // 8

    def fresh():
        return dict(rm=torch.full((Cc,), 0.5, device=DEV), rv=torch.full((Cc,), 2.0, device=DEV), mean=torch.empty(Cc, device=DEV), invstd=torch.empty(Cc, device=DEV),
                    coef=torch.full((2, Cc), float("nan"), device=DEV), z=torch.full((N, H, W, K), float("nan"), dtype=tdt, device=DEV),
                    acc=torch.zeros(rep, 2, K, dtype=torch.float64, device=DEV), y=torch.full((M_ + 1, Cc), 7.0, dtype=tdt, device=DEV),
                    mask=torch.full((nmask + 16,), 0xA5, dtype=torch.uint8, device=DEV))
    e, l = fresh(), fresh()
    if with_res:
        call("clhip_bn_apply_train_mask", zp.data_ptr(), acc_in.data_ptr(), rep_in, M_, Cc, gamma.data_ptr(), beta.data_ptr(), e["rm"].data_ptr(), e["rv"].data_ptr(), mom, eps,
             e["mean"].data_ptr(), e["invstd"].data_ptr(), rs_t.data_ptr(), e["y"].data_ptr(), e["mask"].data_ptr(), code, st())
    else:
        call("clhip_bn_apply_train", zp.data_ptr(), acc_in.data_ptr(), rep_in, M_, Cc, gamma.data_ptr(), beta.data_ptr(), e["rm"].data_ptr(), e["rv"].data_ptr(), mom, eps,
             e["mean"].data_ptr(), e["invstd"].data_ptr(), None, e["y"].data_ptr(), 1, code, st())
    call("clhip_conv_fwd_acc", e["y"].data_ptr(), w.data_ptr(), e["z"].data_ptr(), e["acc"].data_ptr(), rep, N, H, W, Cc, K, 3, 1, 1, code, st())
    bi = BnInput(acc_in.data_ptr(), rep_in, gamma.data_ptr(), beta.data_ptr(), l["rm"].data_ptr(), l["rv"].data_ptr(), mom, eps, l["mean"].data_ptr(),
                 l["invstd"].data_ptr(), l["coef"].data_ptr())
    br = BnRes(rs_t.data_ptr() if with_res else None, l["y"].data_ptr(), l["mask"].data_ptr() if with_res else None)
    for rerun in range(2):          # a second launch: same bits (no state left behind in the kernel's scratch); the running statistics move again
        if rerun:
            l2 = fresh()
            bi = BnInput(acc_in.data_ptr(), rep_in, gamma.data_ptr(), beta.data_ptr(), l2["rm"].data_ptr(), l2["rv"].data_ptr(), mom, eps, l2["mean"].data_ptr(),
                         l2["invstd"].data_ptr(), l2["coef"].data_ptr())
            br = BnRes(rs_t.data_ptr() if with_res else None, l2["y"].data_ptr(), l2["mask"].data_ptr() if with_res else None)
            l = l2
        call("clhip_conv_fwd_acc_bn_input_wt", zp.data_ptr(), C.byref(bi), C.byref(br), w.data_ptr(), l["z"].data_ptr(), l["acc"].data_ptr(), rep, N, H, W, Cc, K, 3, 1, 1,
             code, st())
        torch.cuda.synchronize()
        assert torch.equal(l["y"], e["y"]) and float((l["y"][M_].float() - 7.0).abs().max()) == 0.0
        if with_res:
            assert torch.equal(l["mask"], e["mask"]) and bool((l["mask"][nmask:] == 0xA5).all())
            assert int(e["mask"][:nmask].count_nonzero()) > 0
        else:
            assert bool((l["mask"] == 0xA5).all())
        assert int((e["y"][:M_] == 0).sum()) > 0 and int((e["y"][:M_] != 0).sum()) > 0      # both signs occur
        assert torch.equal(l["z"], e["z"])
        for k in ("rm", "rv", "mean", "invstd"):
            assert torch.equal(l[k], e[k]), k
        coef_want = torch.stack([gamma * e["invstd"], beta - e["mean"] * (gamma * e["invstd"])])
        assert torch.allclose(l["coef"], coef_want, rtol=1e-6, atol=1e-7)
        assert ((l["acc"].sum(0) - e["acc"].sum(0)).abs() <= 1e-12 * e["acc"].sum(0).abs().clamp(min=1.0)).all()
    return l, w          # (for tests/test_conv_routes_gpu.py: the fused launch's tensors against fp64)


@pytest.mark.parametrize("case", [(256, 32, 32, 16, 32), (256, 16, 16, 32, 64), (5, 32, 32, 16, 32), (3, 16, 16, 32, 64), (32, 32, 32, 16, 32), (130, 16, 16, 32, 64)])
def test_stride2_wgrad_pair_one_launch(case):
    """conv7.hip: the weight gradients of a down-sampling entry -- 3x3 / s2 / p1 and the 1x1 / s2 shortcut over the same block input -- in one
    launch, against the fp64 reference and the two generic launches; accumulates into the gradients; bitwise reproducible (partial blocks per image
    group + fixed-order reduce); image groups of one and of several images, a ragged last group."""
    N, H, W, C, K = case
    code, tdt = DT["bf16"]
    L = _lib.lib()
    assert L.clhip_conv_wgrad_pair_supported(N, H, W, C, K, code) == 1
    Ho, Wo = H // 2, W // 2
    x = quant(rnd((N, C, H, W), 11), tdt)
    dz = quant(rnd((N, K, Ho, Wo), 12, 0.5), tdt)
    dzs = quant(rnd((N, K, Ho, Wo), 13, 0.5), tdt)
    w3 = torch.zeros(K, C, 3, 3, dtype=torch.float64, requires_grad=True)
    w1 = torch.zeros(K, C, 1, 1, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w3, None, 2, 1).backward(dz.double())
    F.conv2d(x.double(), w1, None, 2, 0).backward(dzs.double())
    ref3 = w3.grad.permute(0, 2, 3, 1).reshape(K, 9, C)
    ref1 = w1.grad.permute(0, 2, 3, 1).reshape(K, 1, C)
    xd, dzd, dzsd = to_nhwc(x, tdt), to_nhwc(dz, tdt), to_nhwc(dzs, tdt)
    ws3 = torch.empty(L.clhip_conv_wgrad_ws_bytes(N, H, W, C, C, K, 3, 2, 1, code), dtype=torch.uint8, device=DEV)
    ws1 = torch.empty(L.clhip_conv_wgrad_ws_bytes(N, H, W, C, C, K, 1, 2, 0, code), dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        dw3 = torch.full((K, 9, C), 0.25, device=DEV)
        dw1 = torch.full((K, 1, C), -0.5, device=DEV)
        ws3.fill_(0x7f); ws1.fill_(0x7f)
        call("clhip_conv_wgrad_pair", xd.data_ptr(), dzd.data_ptr(), dzsd.data_ptr(), dw3.data_ptr(), dw1.data_ptr(), ws3.data_ptr(), ws1.data_ptr(), N, H, W, C, K, code, st())
        torch.cuda.synchronize()
        outs.append((dw3, dw1))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert ((outs[0][0].cpu().double() - 0.25) - ref3).abs().max() <= 2e-3 * ref3.abs().max() + 1e-3
    assert ((outs[0][1].cpu().double() + 0.5) - ref1).abs().max() <= 2e-3 * ref1.abs().max() + 1e-3
    # the two generic launches it replaces
    g3 = torch.full((K, 9, C), 0.25, device=DEV)
    g1 = torch.full((K, 1, C), -0.5, device=DEV)
    call("clhip_conv_wgrad", xd.data_ptr(), dzd.data_ptr(), g3.data_ptr(), ws3.data_ptr(), N, H, W, C, C, K, 3, 2, 1, code, st())
    call("clhip_conv_wgrad", xd.data_ptr(), dzsd.data_ptr(), g1.data_ptr(), ws1.data_ptr(), N, H, W, C, C, K, 1, 2, 0, code, st())
    torch.cuda.synchronize()
    assert (outs[0][0] - g3).abs().max() <= 1e-3 * ref3.abs().max() + 1e-3 and (outs[0][1] - g1).abs().max() <= 1e-3 * ref1.abs().max() + 1e-3


@pytest.mark.parametrize("case", [(256, 32, 32, 16, 32), (256, 16, 16, 32, 64), (5, 32, 32, 16, 32), (3, 16, 16, 32, 64), (1, 4, 8, 16, 32), (7, 8, 4, 32, 64)])
def test_stride2_forward_pair_one_launch(case):
    """conv7.hip: the forward of a down-sampling entry -- 3x3 / s2 / p1 and the 1x1 / s2 shortcut over the same block input, each with its BatchNorm
    sums -- in one launch, against the fp64 convolutions (outputs and the sums of the unrounded outputs) and against the two generic launches."""
    N, H, W, C, K = case
    code, tdt = DT["bf16"]
    L = _lib.lib()
    assert L.clhip_conv_fwd_acc_pair_supported(N, H, W, C, K, code) == 1
    Ho, Wo = H // 2, W // 2
    x = quant(rnd((N, C, H, W), 21), tdt)
    w3 = quant(rnd((K, C, 3, 3), 22, 1.0 / (C * 9) ** 0.5), tdt)
    w1 = quant(rnd((K, C, 1, 1), 23, 1.0 / C ** 0.5), tdt)
    r3 = F.conv2d(x.double(), w3.double(), None, 2, 1)
    r1 = F.conv2d(x.double(), w1.double(), None, 2, 0)
    xd = to_nhwc(x, tdt)
    w3d = w3.permute(0, 2, 3, 1).contiguous().to(tdt).to(DEV)          # [K][9][C]
    w1d = w1.permute(0, 2, 3, 1).contiguous().to(tdt).to(DEV)
    z3 = torch.full((N * Ho * Wo + 1, K), 7.0, dtype=tdt, device=DEV)
    z1 = torch.full((N * Ho * Wo + 1, K), 7.0, dtype=tdt, device=DEV)
    a3 = torch.zeros(8, 2, K, dtype=torch.float64, device=DEV)
    a1 = torch.zeros(4, 2, K, dtype=torch.float64, device=DEV)
    call("clhip_conv_fwd_acc_pair", xd.data_ptr(), w3d.data_ptr(), w1d.data_ptr(), z3.data_ptr(), z1.data_ptr(), a3.data_ptr(), 8, a1.data_ptr(), 4, N, H, W, C, K, code, st())
    torch.cuda.synchronize()
    M_ = N * Ho * Wo
    for z, r, a in ((z3, r3, a3), (z1, r1, a1)):
        got = z[:M_].reshape(N, Ho, Wo, K).permute(0, 3, 1, 2).cpu().double()
        assert (got - r).abs().max() <= tol("bf16", r)
        assert float((z[M_].float() - 7.0).abs().max()) == 0.0
        s = a.sum(0).cpu()
        rs, rq = r.sum((0, 2, 3)), (r * r).sum((0, 2, 3))
        assert (s[0] - rs).abs().max() <= 1e-4 * r.abs().sum((0, 2, 3)).max() + 1e-6
        assert (s[1] - rq).abs().max() <= 1e-4 * rq.max() + 1e-6
    g3 = torch.empty(M_, K, dtype=tdt, device=DEV)
    g1 = torch.empty(M_, K, dtype=tdt, device=DEV)
    b3, b1 = torch.zeros_like(a3), torch.zeros_like(a1)
    call("clhip_conv_fwd_acc", xd.data_ptr(), w3d.data_ptr(), g3.data_ptr(), b3.data_ptr(), 8, N, H, W, C, K, 3, 2, 1, code, st())
    call("clhip_conv_fwd_acc", xd.data_ptr(), w1d.data_ptr(), g1.data_ptr(), b1.data_ptr(), 4, N, H, W, C, K, 1, 2, 0, code, st())
    torch.cuda.synchronize()
    assert (z3[:M_].float() - g3.float()).abs().max() <= 2 ** -7 * float(r3.abs().max()) and (z1[:M_].float() - g1.float()).abs().max() <= 2 ** -7 * float(r1.abs().max())


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("shape", [(256, 64, 64), (33, 16, 512 // 2), (5, 49, 64), (7, 1, 128), (256, 16, 512), (3, 4, 2048)])
def test_avgpool_backward_with_batchnorm_sums(shape, dt):
    """clhip_avgpool_bwd_bn_reduce = clhip_avgpool_bwd (bit-identical gradient) + the BatchNorm-backward sums of the layer that produced the pooled
    activation (sum g, sum g xhat with g = da masked by y > 0), against fp64; with and without a ReLU."""
    N, HW, C = shape
    code, tdt = DT[dt]
    L = _lib.lib()
    assert L.clhip_avgpool_bwd_bn_reduce_supported(N, HW, C, code) == 1
    dfeat = rnd((N, C), 41).to(DEV)
    z = quant(rnd((N, HW, C), 42, 1.1), tdt).to(tdt).to(DEV)
    y = quant(torch.relu(rnd((N, HW, C), 43) + 0.2), tdt).to(tdt).to(DEV)
    mean = z.double().mean((0, 1)).float()
    invstd = (1.0 / torch.sqrt(z.double().var((0, 1), unbiased=False) + 1e-5)).float()
    ref_da = torch.empty(N, HW, C, dtype=tdt, device=DEV)
    call("clhip_avgpool_bwd", dfeat.data_ptr(), ref_da.data_ptr(), N, HW, C, code, st())
    for relu in (True, False):
        da = torch.full((N, HW, C), float("nan"), dtype=tdt, device=DEV)
        acc = torch.zeros(8, 2, C, dtype=torch.float64, device=DEV)
        call("clhip_avgpool_bwd_bn_reduce", dfeat.data_ptr(), da.data_ptr(), z.data_ptr(), y.data_ptr() if relu else None, mean.data_ptr(), invstd.data_ptr(),
             acc.data_ptr(), 8, N, HW, C, code, st())
        torch.cuda.synchronize()
        assert torch.equal(da, ref_da)
        g = (dfeat.double() / HW).view(N, 1, C).expand(N, HW, C)
        if relu:
            g = g * (y.double() > 0)
        xhat = (z.double() - mean.double()) * invstd.double()
        s = acc.sum(0)
        assert (s[0] - g.sum((0, 1))).abs().max() <= 1e-5 * g.abs().sum((0, 1)).max() + 1e-7
        assert (s[1] - (g * xhat).sum((0, 1))).abs().max() <= 1e-5 * (g.abs() * xhat.abs()).sum((0, 1)).max() + 1e-7


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_step_over_several_tensors_in_one_launch(momentum):
    """clhip_sgd_step_multi = clhip_sgd_step on each tensor, bit for bit (parameters and momentum buffers), sizes that are not multiples of 4, an empty one"""
    from libcontinual_amd import ops
    sizes = [446_042, 6400, 100, 0, 7]
    ps = [rnd((n,), 50 + i).to(DEV) for i, n in enumerate(sizes)]
    gs = [rnd((n,), 60 + i, 0.1).to(DEV) for i, n in enumerate(sizes)]
    ms = [rnd((n,), 70 + i, 0.05).to(DEV) for i, n in enumerate(sizes)]
    p1, m1 = [p.clone() for p in ps], [m.clone() for m in ms]
    p2, m2 = [p.clone() for p in ps], [m.clone() for m in ms]
    for p, g, m in zip(p1, gs, m1):
        if p.numel():
            ops.sgd_step(p, g, m if momentum else None, 0.05, momentum, 5e-4, 0.5)
    ops.sgd_step_multi([(p, g, m if momentum else None) for p, g, m in zip(p2, gs, m2)], 0.05, momentum, 5e-4, 0.5)
    torch.cuda.synchronize()
    for a, b, c, d in zip(p1, p2, m1, m2):
        assert torch.equal(a, b) and torch.equal(c, d)
    assert not torch.equal(p1[0], ps[0])


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("M_,Cc,with_res,relu", [(4096, 64, True, 1), (1000, 16, False, 1), (777, 512, False, 0), (256 * 64, 256, True, 1)])
def test_batchnorm_eval_apply_in_one_launch(dt, M_, Cc, with_res, relu):
    """clhip_bn_apply_eval = clhip_bn_eval_affine + clhip_bn_apply, bit for bit (the eval-mode forward of the reference backbones,
    resnet.py:296-316 under .eval()): one launch per unit instead of two"""
    code, tdt = DT[dt]
    z = (rnd((M_, Cc), 201) * 1.5).to(tdt).to(DEV)
    r = (rnd((M_, Cc), 202)).to(tdt).to(DEV) if with_res else None
    gamma, beta = (rnd((Cc,), 203) * 0.2 + 1.0).to(DEV), (rnd((Cc,), 204) * 0.3).to(DEV)
    rm, rv = (rnd((Cc,), 205) * 0.1).to(DEV), (rnd((Cc,), 206).abs() + 0.5).to(DEV)
    sc, sh = torch.empty(Cc, device=DEV), torch.empty(Cc, device=DEV)
    y0 = torch.full((M_ + 1, Cc), 3.0, dtype=tdt, device=DEV)
    y1 = torch.full((M_ + 1, Cc), 3.0, dtype=tdt, device=DEV)
    call("clhip_bn_eval_affine", gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1e-5, Cc, sc.data_ptr(), sh.data_ptr(), st())
    call("clhip_bn_apply", z.data_ptr(), sc.data_ptr(), sh.data_ptr(), r.data_ptr() if with_res else None, y0.data_ptr(), M_, Cc, relu, code, st())
    call("clhip_bn_apply_eval", z.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1e-5, r.data_ptr() if with_res else None, y1.data_ptr(),
         M_, Cc, relu, code, st())
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and float((y1[M_].float() - 3.0).abs().max()) == 0.0
    want = z.double() * (gamma.double() / (rv.double() + 1e-5).sqrt()) + (beta.double() - rm.double() * gamma.double() / (rv.double() + 1e-5).sqrt())
    if with_res:
        want = want + r.double()
    if relu:
        want = want.clamp(min=0)
    assert float((y1[:M_].double() - want).abs().max()) <= (2e-2 if dt == "bf16" else 1e-4) * float(want.abs().max())
