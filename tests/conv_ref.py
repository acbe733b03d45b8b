"""fp64 reference, per-element error bound and case list of the convolution entry points (csrc/conv*.hip, stem*.hip, shortcut.hip, wgrad4.hip):
clhip_conv_fwd[_acc], clhip_conv_dgrad, clhip_conv_wgrad, clhip_conv_dgrad_bn_reduce, clhip_conv_fwd_acc_bn_input_wt.

The reference works on the operands as the kernel sees them (already rounded to bf16 in the bf16 mode), in fp64 on the operands' device, as an
im2col product (unfold / fold), which is torch's conv2d / its autograd gradients written out; tests/test_conv_ref_cpu.py holds it against
F.conv2d and autograd.  Tensors are NCHW here; the layouts of the C ABI are the GPU file's business.

Beside every reference value comes S, the same operation on the operands' magnitudes (|x|, |w| / |dz|, |w| / |x|, |dz|).  The bound of one
element, in fp64:
  accumulation   (R + 8) 2^-24 S      any summation order of R fp32 products (MFMA blocks, K groups summed through LDS, split partial blocks
                                      summed afterwards, atomics) is within (R - 1) u S to first order, u = 2^-24; the 8 spare units carry the
                                      second-order terms.  R = k k C (forward), k k K (dgrad), N Ho Wo (wgrad).
  output         eps_out |ref|        2^-8 (bf16 store: the figure the project's test headers use), 2^-23 (fp32 store), 0 for the fp32 weight
                                      gradient (nothing is stored but the accumulated sum)
  accumulate     one more eps_out |ref_total| for dx += (the stored sum is rounded once more); the earlier content itself is one more addend
                 of the sum: R + 1 terms and S + |old|.  The weight gradient's += is the same: R + 1 terms, S + |old|, no output term.
The fp32 mode multiplies in full fp32 (v_mfma_f32_16x16x4_f32 in conv.hip / conv2.hip, plain FMAs in stem7.hip): products of fp32 operands are
rounded once each, which the first-order term above already counts (a product and its add are one fused step in the MFMA), so there is no
extra term.  Every element of every case is judged; nothing is left out.

BatchNorm statistics from the forward accumulators (sums of the fp32 accumulators before rounding): with b the accumulation term alone,
  |s1 - sum ref| <= sum b + 2^-50 sum |ref|,        |s2 - sum ref^2| <= sum (2 |ref| b + b^2) + 2^-50 sum ref^2
and the BatchNorm-backward sums of the dgrad epilogue the same on g = dx mask and g xhat: sum b mask, sum b mask |xhat| (the spare units of b
carry the fp32 evaluation of xhat and of the product)."""
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
OUT_EPS = {"bf16": 2.0 ** -8, "f32": 2.0 ** -23}
REL64 = 2.0 ** -50


def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _fwd(x, w, s, p):
    N, C, H, W = x.shape
    K, _, k, _ = w.shape
    Ho, Wo = out_hw(H, W, k, s, p)
    cols = F.unfold(x, k, padding=p, stride=s)                       # [N, C k k, Ho Wo]
    return (w.reshape(K, -1) @ cols).reshape(N, K, Ho, Wo)


def _dgrad(dz, w, s, p, H, W):
    N, K, Ho, Wo = dz.shape
    k = w.shape[2]
    cols = w.reshape(K, -1).T @ dz.reshape(N, K, Ho * Wo)            # [N, C k k, Ho Wo]
    return F.fold(cols, (H, W), k, padding=p, stride=s)


def _wgrad(x, dz, k, s, p):
    N, C, H, W = x.shape
    K = dz.shape[1]
    cols = F.unfold(x, k, padding=p, stride=s)                       # [N, C k k, Ho Wo]
    return torch.einsum("nkp,njp->kj", dz.reshape(N, K, -1), cols).reshape(K, C, k, k)


def conv_fwd_ref(x, w, s, p):
    """(z, S) fp64 [N, K, Ho, Wo] of x [N, C, H, W], w [K, C, k, k]"""
    x, w = x.double(), w.double()
    return _fwd(x, w, s, p), _fwd(x.abs(), w.abs(), s, p)


def conv_dgrad_ref(dz, w, s, p, H, W):
    """(dx, S) fp64 [N, C, H, W] of dz [N, K, Ho, Wo], w [K, C, k, k]"""
    dz, w = dz.double(), w.double()
    return _dgrad(dz, w, s, p, H, W), _dgrad(dz.abs(), w.abs(), s, p, H, W)


def conv_wgrad_ref(x, dz, k, s, p):
    """(dw, S) fp64 [K, C, k, k] of x [N, C, H, W], dz [N, K, Ho, Wo]"""
    x, dz = x.double(), dz.double()
    return _wgrad(x, dz, k, s, p), _wgrad(x.abs(), dz.abs(), k, s, p)


def acc_bound(S, R, old=None):
    """the accumulation term: a sum of R products (and the earlier content `old`, one more addend) in any order"""
    if old is None:
        return (R + 8) * U24 * S
    return (R + 1 + 8) * U24 * (S + old.double().abs())


def elem_bound(S, R, ref, dt, old=None):
    """allowed |got - ref_total| per element of a stored activation / gradient (dt) -- ref: the convolution alone; old: the earlier content of dx +="""
    eps = OUT_EPS[dt]
    b = acc_bound(S, R, old) + eps * ref.abs()
    if old is not None:
        b = b + eps * (ref + old.double()).abs()
    return b


def wgrad_bound(S, R, old=None):
    """allowed |got - (old + dw)| per element of the fp32 weight gradient"""
    return acc_bound(S, R, old)


def stat_bounds(ref, b, dims=(0, 2, 3), weight=None):
    """bounds of (sum ref [weight], sum ref^2) over `dims` from the elements' accumulation bounds b; weight = |xhat| for the sums of g xhat"""
    if weight is None:
        b1 = b.sum(dims) + REL64 * ref.abs().sum(dims)
    else:
        b1 = (b * weight).sum(dims) + REL64 * (ref.abs() * weight).sum(dims)
    b2 = (2 * ref.abs() * b + b * b).sum(dims) + REL64 * (ref * ref).sum(dims)
    return b1, b2


# ------------------------------------------------------------------------------------------------ kernel families of clhip_conv_route (include/clhip.h)
(STEM7, STEM, CONV64, CONV16, CONV8, CONV5, CONV9, CONV4, CONV3, CONV2, V1, SHORTCUT, W_STEM7, W_STEM, W64, W4, W3, W16, W32, W2_DET, W2_ATOMIC, W_V1,
 W_V1_NO_TR) = range(1, 24)
FAMILY_NAMES = {STEM7: "stem7", STEM: "stem", CONV64: "conv64", CONV16: "conv16", CONV8: "conv8", CONV5: "conv5", CONV9: "conv9", CONV4: "conv4", CONV3: "conv3",
                CONV2: "conv2", V1: "v1-igemm", SHORTCUT: "shortcut", W_STEM7: "wgrad-stem7", W_STEM: "wgrad-stem", W64: "wgrad64", W4: "wgrad4", W3: "wgrad3",
                W16: "wgrad16", W32: "wgrad32", W2_DET: "wgrad2-deterministic", W2_ATOMIC: "wgrad2-atomic", W_V1: "wgrad-v1", W_V1_NO_TR: "wgrad-v1-no-transpose"}
OP_FWD, OP_DGRAD, OP_WGRAD, OP_BNR, OP_WT = 0, 1, 2, 3, 4
# the families each dispatcher names.  The write-through forward (op 4) does not name conv4: conv4.hip has no lazy input, and a shape that only it would serve
# is refused (tests/test_conv_ref_cpu.py asserts the refusal)
FAMILIES = {
    OP_FWD: {STEM7, STEM, CONV64, CONV16, CONV8, CONV5, CONV9, CONV4, CONV3, CONV2, V1},
    OP_DGRAD: {SHORTCUT, CONV16, CONV64, CONV8, CONV5, CONV9, CONV4, CONV3, CONV2, V1},
    OP_WGRAD: {W_STEM7, W_STEM, W64, W4, W3, W16, W32, W2_DET, W2_ATOMIC, W_V1, W_V1_NO_TR},
    OP_BNR: {CONV64, CONV16, CONV8, CONV9, CONV4},
    OP_WT: {CONV8, CONV9, CONV5},
}
# route keys of a case -> (op, form)
KEYS = {"fwd0": (OP_FWD, 0), "fwd1": (OP_FWD, 1), "fwd2": (OP_FWD, 2), "dgrad": (OP_DGRAD, 0), "wgrad0": (OP_WGRAD, 0), "wgrad1": (OP_WGRAD, 1), "bnr": (OP_BNR, 0),
        "wt": (OP_WT, 0)}
# switches clhip_config applies at once; every other one is cached at its first use, so a case that needs one runs in a fresh process with CLHIP_<NAME> set
LIVE = {"CONV5", "CONV8", "CONV9", "CONV5_MIN_TILES", "CONV8_MIN_TILES", "CONV4_ENABLE", "BN_INPUT_WT", "CONV64_FWD"}

GEN_F32 = dict(fwd0=CONV2, fwd1=CONV2, fwd2=CONV2, dgrad=CONV2, wgrad0=W2_ATOMIC, wgrad1=W2_DET)      # the fp32 mode: the generic kernels


def _c(name, shape, bf16, f32=None, sw=None, creal=None):
    """shape = (N, H, W, C, K, k, stride, pad) with C as the call gets it (the stems' 3 channels padded to 8, Creal = 3); bf16 / f32: route key -> family
    (an absent key: that call is not part of the case); sw: the switches the case needs"""
    return dict(name=name, shape=shape, creal=creal or shape[3], routes={"bf16": bf16, "f32": f32 or {}}, sw=sw or {})


def _only(d, *keys):
    return {k: d[k] for k in keys}


_S7 = dict(fwd0=STEM7, fwd2=STEM7, wgrad1=W_STEM7)
_G = dict(fwd0=CONV2, fwd1=CONV2, fwd2=CONV2, dgrad=CONV2, wgrad0=W2_ATOMIC, wgrad1=W2_DET)
_GF = _only(GEN_F32, "fwd0", "fwd1", "fwd2", "wgrad0", "wgrad1")          # (no dgrad: fewer than 16 channels, or K no power of two)
_9 = dict(fwd0=CONV9, fwd2=CONV9, fwd1=CONV4, dgrad=CONV9, bnr=CONV9, wt=CONV9)
_94 = dict(fwd0=CONV4, fwd2=CONV4, fwd1=CONV4, dgrad=CONV4, bnr=CONV4)       # geometry9 refuses: conv4 (the write-through form has no kernel then)
_ON9 = {"CONV9": "1", "BN_INPUT_WT": "1"}

CASES = [
    # ---- the stems
    _c("stem7-2x19x23-k16", (2, 19, 23, 8, 16, 7, 2, 3), _S7, _S7, creal=3),                       # odd image, ragged everything
    _c("stem7-3x16x16-k64", (3, 16, 16, 8, 64, 7, 2, 3), _S7, _S7, creal=3),
    _c("stem-3x7x5-k32", (3, 7, 5, 8, 32, 3, 1, 1), dict(fwd0=STEM, fwd2=STEM, fwd1=CONV2, wgrad0=W2_ATOMIC, wgrad1=W2_DET), _GF, creal=3),
    _c("stem-9x16x16-k16", (9, 16, 16, 8, 16, 3, 1, 1), dict(fwd0=STEM, fwd2=STEM, fwd1=CONV2, wgrad0=W2_ATOMIC, wgrad1=W_STEM), _GF, creal=3),      # 2304 pixels >= 2048: stem.hip's weight gradient
    _c("stem-11x17x13-k64", (11, 17, 13, 8, 64, 3, 1, 1), dict(fwd0=STEM, fwd2=STEM, fwd1=CONV2, wgrad0=W2_ATOMIC, wgrad1=W_STEM), _GF, creal=3),     # odd image, ragged last 32-pixel step
    # ---- 64 -> 64 channels on small maps (conv3.hip conv64: 64-pixel tiles)
    _c("conv64-3x8x8", (3, 8, 8, 64, 64, 3, 1, 1), dict(fwd0=CONV64, fwd2=CONV64, fwd1=CONV4, dgrad=CONV64, bnr=CONV64, wgrad0=W3, wgrad1=W64), GEN_F32),
    _c("conv64-2x7x5", (2, 7, 5, 64, 64, 3, 1, 1), dict(fwd0=CONV64, fwd2=CONV64, fwd1=CONV4, dgrad=CONV64, bnr=CONV64, wgrad0=W2_ATOMIC, wgrad1=W2_DET)),      # tile spanning images, ragged, no power of two
    _c("conv64-5x16x16", (5, 16, 16, 64, 64, 3, 1, 1), dict(fwd0=CONV64, fwd2=CONV64, fwd1=CONV4, dgrad=CONV64, bnr=CONV64, wgrad0=W3, wgrad1=W4)),            # four tiles per image
    _c("conv64-2x1x9", (2, 1, 9, 64, 64, 3, 1, 1), dict(fwd0=CONV64, fwd2=CONV64, fwd1=CONV4, dgrad=CONV64, bnr=CONV64)),                                     # one-row images
    _c("conv64-5x16x8", (5, 16, 8, 64, 64, 3, 1, 1), dict(wgrad0=W3, wgrad1=W64)),                                                                       # wgrad64: 16 rows of an 8-wide image, odd image count
    # ---- 16 -> 16 / 32 -> 32 channels (conv3.hip conv16 / conv32: 256-pixel tiles)
    _c("conv16-9x7x5", (9, 7, 5, 16, 16, 3, 1, 1), dict(fwd0=CONV16, fwd1=CONV16, fwd2=CONV16, dgrad=CONV16, bnr=CONV16, wgrad0=W2_ATOMIC, wgrad1=W2_DET), GEN_F32),
    _c("conv32-2x1x9", (2, 1, 9, 32, 32, 3, 1, 1), dict(fwd0=CONV16, fwd1=CONV16, fwd2=CONV16, dgrad=CONV16, bnr=CONV16, wgrad0=W2_ATOMIC, wgrad1=W2_DET)),
    _c("conv32-5x16x16", (5, 16, 16, 32, 32, 3, 1, 1), dict(fwd0=CONV16, fwd1=CONV16, fwd2=CONV16, dgrad=CONV16, bnr=CONV16, wgrad0=W2_ATOMIC, wgrad1=W32)),
    _c("conv16-3x8x32", (3, 8, 32, 16, 16, 3, 1, 1), dict(fwd0=CONV16, fwd1=CONV16, fwd2=CONV16, dgrad=CONV16, bnr=CONV16, wgrad0=W2_ATOMIC, wgrad1=W16)),
    _c("conv32-3x7x16", (3, 7, 16, 32, 32, 3, 1, 1), dict(wgrad1=W2_DET)),                                                                                # odd row count: not wgrad32
    # ---- 64 -> 64 channels, LDS-DMA kernels forced onto small problems: conv8.hip (128-pixel tiles of whole rows) ...
    _c("conv8-3x32x32", (3, 32, 32, 64, 64, 3, 1, 1), dict(fwd0=CONV8, fwd2=CONV8, fwd1=CONV4, dgrad=CONV8, bnr=CONV8, wt=CONV8), sw={"CONV8_MIN_TILES": "1", "BN_INPUT_WT": "1"}),
    _c("conv8-2x4x32", (2, 4, 32, 64, 64, 3, 1, 1), dict(fwd0=CONV8, fwd2=CONV8, dgrad=CONV8, bnr=CONV8, wt=CONV8), sw={"CONV8_MIN_TILES": "1", "BN_INPUT_WT": "1"}),      # one tile per image
    # ... and conv5.hip (256-pixel tiles: ragged last tile, tiles spanning images, no power of two)
    _c("conv5-5x9x20", (5, 9, 20, 64, 64, 3, 1, 1), dict(fwd0=CONV5, fwd2=CONV5, fwd1=CONV4, dgrad=CONV5, bnr=CONV4, wt=CONV5), sw={"CONV5_MIN_TILES": "1", "CONV8": "0", "BN_INPUT_WT": "1"}),
    _c("conv5-2x32x32", (2, 32, 32, 64, 64, 3, 1, 1), dict(fwd0=CONV5, fwd2=CONV5, dgrad=CONV5, wt=CONV5), sw={"CONV5_MIN_TILES": "1", "CONV8": "0", "BN_INPUT_WT": "1"}),
    # ---- conv9.hip (CONV9=1; bf16, C == K): every legal geometry of geometry9.  128 channels, single-image tiles of 256 pixels ...
    _c("conv9-128-3x16x16", (3, 16, 16, 128, 128, 3, 1, 1), _9, sw=_ON9),            # one tile per image
    _c("conv9-128-3x32x16", (3, 32, 16, 128, 128, 3, 1, 1), _9, sw=_ON9),            # two tiles per image
    _c("conv9-128-3x32x32", (3, 32, 32, 128, 128, 3, 1, 1), _9, sw=_ON9),            # four tiles per image, 8 rows each
    _c("conv9-128-3x64x4", (3, 64, 4, 128, 128, 3, 1, 1), _9, sw=_ON9),
    # ... multi-image tiles
    _c("conv9-128-4x8x8", (4, 8, 8, 128, 128, 3, 1, 1), _9, sw=_ON9),                # 4 images per tile
    _c("conv9-128-8x8x8", (8, 8, 8, 128, 128, 3, 1, 1), _9, sw=_ON9),
    _c("conv9-128-4x8x16", (4, 8, 16, 128, 128, 3, 1, 1), _9, sw=_ON9),              # 2 per tile
    _c("conv9-128-4x16x8", (4, 16, 8, 128, 128, 3, 1, 1), _9, sw=_ON9),
    _c("conv9-128-8x16x4", (8, 16, 4, 128, 128, 3, 1, 1), _9, sw=_ON9),              # 4 per tile
    # ... 256 channels: 128-pixel tiles, two K groups
    _c("conv9-256-2x8x8", (2, 8, 8, 256, 256, 3, 1, 1), _9, sw=_ON9),                # 2 images per tile
    _c("conv9-256-6x8x8", (6, 8, 8, 256, 256, 3, 1, 1), _9, sw=_ON9),
    _c("conv9-256-3x8x16", (3, 8, 16, 256, 256, 3, 1, 1), _9, sw=_ON9),              # one tile per image
    _c("conv9-256-3x16x16", (3, 16, 16, 256, 256, 3, 1, 1), _9, sw=_ON9),            # two tiles per image
    _c("conv9-256-3x32x4", (3, 32, 4, 256, 256, 3, 1, 1), _9, sw=_ON9),
    # ... and what geometry9 refuses stays on conv4.hip
    _c("conv9-refused-6x8x8x128", (6, 8, 8, 128, 128, 3, 1, 1), _94, sw=_ON9),       # 6 images do not fill tiles of 4
    _c("conv9-refused-4x4x4x128", (4, 4, 4, 128, 128, 3, 1, 1), _94, sw=_ON9),
    _c("conv9-refused-4x4x4x256", (4, 4, 4, 256, 256, 3, 1, 1), _94, sw=_ON9),
    _c("conv9-refused-3x4x32x256", (3, 4, 32, 256, 256, 3, 1, 1), _94, sw=_ON9),
    # ---- conv4.hip with its defaults (64-channel multiples, 3x3 / s1)
    _c("conv4-3x16x16x128", (3, 16, 16, 128, 128, 3, 1, 1), dict(fwd0=CONV4, fwd1=CONV4, fwd2=CONV4, dgrad=CONV4, bnr=CONV4, wgrad0=W3, wgrad1=W4)),
    _c("conv4-5x8x8x256", (5, 8, 8, 256, 256, 3, 1, 1), dict(fwd0=CONV4, fwd1=CONV4, fwd2=CONV4, dgrad=CONV4, bnr=CONV4, wgrad0=W3, wgrad1=W4)),
    _c("conv4-7x4x4x512", (7, 4, 4, 512, 512, 3, 1, 1), dict(fwd0=CONV4, fwd1=CONV4, fwd2=CONV4, dgrad=CONV4, bnr=CONV4, wgrad0=W3, wgrad1=W4)),
    _c("conv4-2x6x6-64to128", (2, 6, 6, 64, 128, 3, 1, 1), dict(fwd0=CONV4, fwd1=CONV4, fwd2=CONV4, dgrad=CONV4, bnr=CONV4, wgrad0=W2_ATOMIC, wgrad1=W2_DET), GEN_F32),
    _c("wgrad4-5x4x8-64to128", (5, 4, 8, 64, 128, 3, 1, 1), dict(wgrad0=W3, wgrad1=W4)),                     # four 4x8 images per 128-pixel step, ragged last step
    _c("wgrad4-7x8x4-128to64", (7, 8, 4, 128, 64, 3, 1, 1), dict(wgrad0=W3, wgrad1=W4)),                     # two 8x4 images per step
    # ---- conv3.hip's halo kernel: where conv4.hip is off (a live switch of the micro-benchmarks) ...
    _c("conv3-2x7x5x128", (2, 7, 5, 128, 128, 3, 1, 1), dict(fwd0=CONV3, fwd1=CONV3, fwd2=CONV3, dgrad=CONV3), sw={"CONV4_ENABLE": "0"}),
    _c("conv3-5x8x8-64to128", (5, 8, 8, 64, 128, 3, 1, 1), dict(fwd0=CONV3, fwd1=CONV3, fwd2=CONV3, dgrad=CONV3), sw={"CONV4_ENABLE": "0"}),
    # ... or refuses (three 64-channel groups are no power of two)
    _c("conv3-2x6x6-64to192", (2, 6, 6, 64, 192, 3, 1, 1), dict(fwd0=CONV3, fwd1=CONV3, fwd2=CONV3)),
    # ---- the generic kernels (conv2.hip): strides, 1x1, K no power of two, one pixel, the parity-class dgrad
    _c("conv2-2x8x8-16to32-s2", (2, 8, 8, 16, 32, 3, 2, 1), _G, GEN_F32),
    _c("conv2-3x5x7-32to48", (3, 5, 7, 32, 48, 3, 1, 1), _only(_G, "fwd0", "fwd1", "fwd2", "wgrad0", "wgrad1"), _GF),
    _c("conv2-2x9x9-128to256-1x1s2", (2, 9, 9, 128, 256, 1, 2, 0), _G, GEN_F32),
    _c("conv2-1x1x1x16", (1, 1, 1, 16, 16, 3, 1, 1), _G, GEN_F32),
    _c("conv2-4x16x16-64to128-s2", (4, 16, 16, 64, 128, 3, 2, 1), _G, _only(GEN_F32, "dgrad")),                # dgrad in four parity classes
    _c("conv2-3x9x9-64to128-s2", (3, 9, 9, 64, 128, 3, 2, 1), _only(_G, "dgrad")),                                # odd image: no parity classes
    # ---- the 1x1 / s2 shortcut from 8192 output pixels on (shortcut.hip dgrad, wgrad4.hip), ragged last tile
    _c("shortcut-33x32x32-64to128", (33, 32, 32, 64, 128, 1, 2, 0), dict(dgrad=SHORTCUT, wgrad0=W2_ATOMIC, wgrad1=W4)),
    # ---- wgrad4.hip's 3x3 / s2 form (>= 32 steps)
    _c("wgrad4-20x32x32-64to128-s2", (20, 32, 32, 64, 128, 3, 2, 1), dict(wgrad0=W2_ATOMIC, wgrad1=W4)),
]

# ---- families behind switches that are cached at their first use: one fresh process per setting (CLHIP_<NAME> in its environment)
_V1 = dict(fwd0=V1, fwd1=V1, dgrad=V1, wgrad0=W_V1, wgrad1=W_V1)
_V1F = dict(fwd0=V1, fwd1=V1, dgrad=V1, wgrad0=W_V1_NO_TR, wgrad1=W_V1_NO_TR)
_V1N = dict(wgrad0=W_V1_NO_TR, wgrad1=W_V1_NO_TR)
_ND = ("fwd0", "fwd1", "wgrad0", "wgrad1")
CACHED = [
    dict(env={"CONV_V1": "1"}, cases=[
        _c("v1-2x8x8-16to32-s2", (2, 8, 8, 16, 32, 3, 2, 1), _V1, _V1F),
        _c("v1-3x5x7-32to48", (3, 5, 7, 32, 48, 3, 1, 1), _only(_V1, *_ND), _only(_V1F, *_ND)),                   # ragged everything, K no power of two
        _c("v1-2x6x6-64to128", (2, 6, 6, 64, 128, 3, 1, 1), _V1, _V1F),
        _c("v1-3x9x9-128to256-1x1s2", (3, 9, 9, 128, 256, 1, 2, 0), _V1),
    ]),
    dict(env={"CONV_V1": "1", "WGRAD_NO_TR": "1"}, cases=[
        _c("v1-notr-2x8x8-16to32-s2", (2, 8, 8, 16, 32, 3, 2, 1), _V1N),
        _c("v1-notr-3x5x7-32to48", (3, 5, 7, 32, 48, 3, 1, 1), _V1N),
        _c("v1-notr-2x6x6-64to128", (2, 6, 6, 64, 128, 3, 1, 1), _V1N),
    ]),
    dict(env={"WGRAD2_ATOMIC": "1"}, cases=[
        _c("w2atomic-2x8x8-16to32-s2", (2, 8, 8, 16, 32, 3, 2, 1), dict(wgrad1=W2_ATOMIC), dict(wgrad1=W2_ATOMIC)),
        _c("w2atomic-3x5x7-32to48", (3, 5, 7, 32, 48, 3, 1, 1), dict(wgrad1=W2_ATOMIC)),
    ]),
    dict(env={"NO_PARITY_DGRAD": "1"}, cases=[
        _c("noparity-4x16x16-64to128-s2", (4, 16, 16, 64, 128, 3, 2, 1), dict(dgrad=CONV2), dict(dgrad=CONV2)),
        _c("noparity-5x32x32-16to32-s2", (5, 32, 32, 16, 32, 3, 2, 1), dict(dgrad=CONV2)),
    ]),
    dict(env={"CONV3G": "2"}, cases=[       # the LDS-DMA weight ring: conv3g_kernel, another template than conv3_kernel (mode 1 picks the same two by size)
        _c("conv3g-2x7x5x128", (2, 7, 5, 128, 128, 3, 1, 1), dict(fwd0=CONV3, fwd1=CONV3, fwd2=CONV3, dgrad=CONV3), sw={"CONV4_ENABLE": "0"}),
        _c("conv3g-2x6x6-64to192", (2, 6, 6, 64, 192, 3, 1, 1), dict(fwd0=CONV3, fwd1=CONV3, fwd2=CONV3)),
    ]),
]

# ---- what the query, like the calls, refuses: (op, form, N, H, W, C, Creal, K, k, stride, pad, dtype code) under the default switches
BF16_CODE, F32_CODE = 0, 1
REFUSALS = [
    ("bad dtype", (0, 0, 2, 8, 8, 16, 16, 16, 3, 1, 1, 2)),
    ("bad dtype, dgrad", (1, 0, 2, 8, 8, 16, 16, 16, 3, 1, 1, -1)),
    ("bad dtype, wgrad", (2, 1, 2, 8, 8, 16, 16, 16, 3, 1, 1, 7)),
    ("bad op", (5, 0, 2, 8, 8, 16, 16, 16, 3, 1, 1, 0)),
    ("bad form", (0, 3, 2, 8, 8, 16, 16, 16, 3, 1, 1, 0)),
    ("a form on dgrad", (1, 1, 2, 8, 8, 16, 16, 16, 3, 1, 1, 0)),
    ("C no power of two", (0, 0, 1, 4, 4, 12, 12, 16, 3, 1, 1, 0)),
    ("C < 8", (0, 0, 1, 4, 4, 4, 4, 16, 3, 1, 1, 0)),
    ("K % 16", (0, 0, 1, 4, 4, 16, 16, 24, 3, 1, 1, 0)),
    ("ksize 5", (0, 0, 1, 8, 8, 16, 16, 16, 5, 1, 2, 0)),
    ("N = 0", (0, 0, 0, 8, 8, 16, 16, 16, 3, 1, 1, 0)),
    ("stride 0", (0, 0, 1, 8, 8, 16, 16, 16, 3, 0, 1, 0)),
    ("2^31 elements", (0, 0, 4096, 64, 64, 128, 128, 128, 3, 1, 1, 0)),
    ("dgrad C % 16", (1, 0, 2, 8, 8, 8, 8, 16, 3, 1, 1, 0)),
    ("dgrad K no power of two", (1, 0, 2, 8, 8, 32, 32, 48, 3, 1, 1, 0)),
    ("ksize 7 with 16 channels", (0, 0, 2, 16, 16, 16, 16, 16, 7, 2, 3, 0)),
    ("ksize 7 stride 1", (0, 0, 2, 16, 16, 8, 3, 16, 7, 1, 3, 0)),
    ("ksize 7 pad 1", (0, 2, 2, 16, 16, 8, 3, 16, 7, 2, 1, 0)),
    ("ksize 7 with 128 features", (0, 0, 2, 16, 16, 8, 3, 128, 7, 2, 3, 0)),
    ("ksize 7 partial rows", (0, 1, 2, 16, 16, 8, 3, 16, 7, 2, 3, 0)),
    ("ksize 7 dgrad", (1, 0, 2, 16, 16, 8, 3, 16, 7, 2, 3, 0)),
    ("ksize 7 wgrad without scratch", (2, 0, 2, 16, 16, 8, 3, 16, 7, 2, 3, 0)),
    ("ksize 7 wgrad Creal 0", (2, 1, 2, 16, 16, 8, 0, 16, 7, 2, 3, 0)),
    ("wgrad Creal > C", (2, 1, 2, 8, 8, 16, 17, 16, 3, 1, 1, 0)),
    ("wgrad Creal 0", (2, 0, 2, 8, 8, 16, 0, 16, 3, 1, 1, 0)),
    ("bn-reduce in fp32", (3, 0, 3, 8, 8, 64, 64, 64, 3, 1, 1, 1)),
    ("bn-reduce of a stride-2 layer", (3, 0, 3, 8, 8, 64, 64, 64, 3, 2, 1, 0)),
    ("bn-reduce of a 1x1 layer", (3, 0, 3, 8, 8, 64, 64, 64, 1, 1, 0, 0)),
    ("write-through while BN_INPUT_WT is off", (4, 0, 160, 32, 32, 64, 64, 64, 3, 1, 1, 0)),
]
# ... and with BN_INPUT_WT=1 (CONV9 left off): outside the write-through kernels' domain by design
WT_REFUSALS = [
    ("512 channels: conv4.hip has no lazy input", (4, 0, 256, 4, 4, 512, 512, 512, 3, 1, 1, 0)),
    ("64 -> 128 channels", (4, 0, 64, 16, 16, 64, 64, 128, 3, 1, 1, 0)),
    ("128 channels without CONV9", (4, 0, 256, 16, 16, 128, 128, 128, 3, 1, 1, 0)),
    ("small 64-channel maps run on conv64", (4, 0, 3, 8, 8, 64, 64, 64, 3, 1, 1, 0)),
    ("fp32", (4, 0, 160, 32, 32, 64, 64, 64, 3, 1, 1, 1)),
]


# ------------------------------------------------------------------------------------------------ the route query (host code: no device)
import contextlib


@contextlib.contextmanager
def switches(L, sw):
    """clhip_config switches of a case, set and restored (LIVE ones: the others are cached at their first use and belong in a child's environment)"""
    assert set(sw) <= LIVE, set(sw) - LIVE
    try:
        for k, v in sw.items():
            assert L.clhip_config(k.encode(), v.encode()) == 0
        yield
    finally:
        for k in sw:
            L.clhip_config(k.encode(), None)


def query(L, case, dt, key):
    """clhip_conv_route of one call of a case (under the switches in force)"""
    N, H, W, C, K, k, s, p = case["shape"]
    op, form = KEYS[key]
    return L.clhip_conv_route(op, form, N, H, W, C, case["creal"], K, k, s, p, {"bf16": BF16_CODE, "f32": F32_CODE}[dt])


def routes_of(L, case):
    """{(dt, key): family} of every call the case names"""
    with switches(L, case["sw"]):
        return {(dt, key): query(L, case, dt, key) for dt in ("bf16", "f32") for key in case["routes"][dt]}


def expected_of(case):
    return {(dt, key): fam for dt in ("bf16", "f32") for key, fam in case["routes"][dt].items()}
