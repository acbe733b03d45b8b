"""csrc/adapter.hip alone on the MI355X, in fp32 and bf16, against the fp64 restatement of tests/adapter_ref.py.

Bounds (u = 2^-24, the unit of the fp32 accumulation both modes use; v = 2^-8, bf16's):
  a product C = A B over K terms in fp32 is within K u sum|a b| of fp64 whatever the summation order (the rule of tests/test_ranpac_kernels_gpu.py),
  each product with its own K; an operand that already carries an error e adds e |b| summed; every further fp32 operation on a value c (bias, scale,
  residual add) adds u |c|.  The fp32 mode is compared with the plain fp64 formula.  The bf16 mode is compared with the fp64 formula evaluated on the
  operands the kernel really uses -- the weights rounded to bf16 on load, hd / dh rounded where they are stored -- so what is left is the same fp32
  accumulation error plus, wherever a value is STORED as bf16, the chance that the fp32 result and the fp64 one fall on different sides of a rounding
  boundary: one bf16 step, 2 v |c|.  The weight gradients read only stored bf16 tensors and write fp32: their bound has no v term at all.
"""
import pytest
import torch

import adapter_ref as A
from libcontinual_amd import _lib
from libcontinual_amd._lib import call

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U, V = 2.0 ** -24, 2.0 ** -8
DT = {"f32": (_lib.F32, torch.float32, A.ident, 0.0), "bf16": (_lib.BF16, torch.bfloat16, A.bf16, V)}
S = A.SCALE


def _st():
    return torch.cuda.current_stream().cuda_stream


def _seed(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def _inputs(M, D, R, dtype, seed=0, zero_up=False):
    """x, y (non-zero: the += must be visible), gy in the compute dtype on the device + their exact fp64 values; the fp32 masters + fp64 values"""
    g = A.gen(1000 * seed + M + D + R)
    tdt = DT[dtype][1]
    act = {k: torch.randn(M, D, generator=g, dtype=torch.float64).to(tdt) for k in ("x", "y", "gy")}
    W = [t.float() for t in A.adapter_params(D, R, seed + 1, zero_up=zero_up)]
    return {k: v.to(DEV) for k, v in act.items()}, {k: v.double() for k, v in act.items()}, [w.to(DEV) for w in W], [w.double() for w in W]


def _mask(seed_t, layer, M, R, p):
    out = torch.empty(M, R, dtype=torch.uint8, device=DEV)
    call("clhip_adapter_dropout_mask", seed_t.data_ptr() if seed_t is not None else None, layer, M, R, p, out.data_ptr(), _st())
    return out


def _fwd(dev, W, dtype, p=0.0, seed_t=None, layer=0, save=True):
    M, D = dev["x"].shape
    R = W[0].shape[0]
    y = dev["y"].clone()
    hd = torch.empty(M, R, dtype=DT[dtype][1], device=DEV) if save else None
    call("clhip_adapter_fwd", dev["x"].data_ptr(), W[0].data_ptr(), W[1].data_ptr(), W[2].data_ptr(), W[3].data_ptr(), y.data_ptr(),
         hd.data_ptr() if save else None, seed_t.data_ptr() if seed_t is not None else None, layer, p, S, M, D, R, DT[dtype][0], _st())
    return y, hd


def _bwd(gy, hd, W, dtype, p=0.0, in_place=False):
    M, D = gy.shape
    R = W[0].shape[0]
    dh = torch.empty(M, R, dtype=gy.dtype, device=DEV)
    gx = gy.clone() if in_place else torch.empty_like(gy)
    src = gx if in_place else gy
    call("clhip_adapter_bwd", src.data_ptr(), hd.data_ptr(), W[2].data_ptr(), W[0].data_ptr(), dh.data_ptr(), gx.data_ptr(), p, S, M, D, R, DT[dtype][0], _st())
    return dh, gx


def _wgrad(gy, hd, x, dh, dtype):
    M, D = gy.shape
    R = hd.shape[1]
    ws = torch.empty(_lib.lib().clhip_adapter_wgrad_ws_bytes(M, D, R), dtype=torch.uint8, device=DEV)
    dWu, dbu, dWd, dbd = (torch.full(s, 7.0, device=DEV) for s in ((D, R), (D,), (R, D), (R,)))          # written, not accumulated into
    call("clhip_adapter_wgrad", gy.data_ptr(), hd.data_ptr(), x.data_ptr(), dh.data_ptr(), dWu.data_ptr(), dbu.data_ptr(), dWd.data_ptr(), dbd.data_ptr(),
         ws.data_ptr(), S, M, D, R, DT[dtype][0], _st())
    return dWd, dbd, dWu, dbu


def _ratio(got, want, bound):
    err = (got.double().cpu() - want).abs()
    assert torch.isfinite(err).all()
    return float((err / bound.clamp_min(1e-300)).max())


def _check_all(M, D, R, dtype, p, seed_t=None, layer=0):
    q, v = DT[dtype][2], DT[dtype][3]
    dev, ref, W, W64 = _inputs(M, D, R, dtype, seed=layer)
    Wd, bd, Wu, bu = W64
    mask = _mask(seed_t, layer, M, R, p).cpu() if p > 0 else None
    # ---- forward
    y, hd = _fwd(dev, W, dtype, p, seed_t, layer)
    delta, hd64 = A.fwd(ref["x"], Wd, bd, Wu, bu, S, mask, p, q)
    y64 = q(ref["y"] + delta)
    e_hd, e_y = A.fwd_bounds(ref["x"], ref["y"], Wd, bd, Wu, bu, S, hd64, delta, y64, p, v, q)      # (the numbers live in adapter_ref: the executor's test shares them)
    r_fwd = max(_ratio(hd, hd64, e_hd), _ratio(y, y64, e_y))
    assert float((y.double().cpu() - ref["y"]).abs().max()) > 0                       # the branch did add something
    # ---- input gradient, on the restatement's own hd (the kernels are tested alone)
    hd_dev = hd64.to(DT[dtype][1]).to(DEV)
    dh, gx = _bwd(dev["gy"], hd_dev, W, dtype, p)
    dx64, dWd64, dbd64, dWu64, dbu64, dh64 = A.bwd(ref["gy"], ref["x"], hd64, Wd, Wu, S, p, q)
    gx64 = q(ref["gy"] + dx64)
    e_dh, e_gx = A.bwd_bounds(ref["gy"], hd64, Wd, Wu, S, dh64, dx64, gx64, p, v, q)
    r_bwd = max(_ratio(dh, dh64, e_dh), _ratio(gx, gx64, e_gx))
    dh2, gx2 = _bwd(dev["gy"], hd_dev, W, dtype, p, in_place=True)                    # gx may be gy
    assert torch.equal(dh2, dh) and torch.equal(gx2, gx)
    # ---- parameter gradients, on stored tensors only: fp32 accumulation over M rows, nothing else
    dh_dev = dh64.to(DT[dtype][1]).to(DEV)
    got = _wgrad(dev["gy"], hd_dev, dev["x"], dh_dev, dtype)
    bounds = A.wgrad_bounds(ref["gy"], hd64, ref["x"], dh64, S)
    r_wg = max(_ratio(a, b, c) for a, b, c in zip(got, (dWd64, dbd64, dWu64, dbu64), bounds))
    print(f"adapter M={M} D={D} R={R} {dtype} p={p}: largest error / bound  fwd {r_fwd:.3f}  bwd {r_bwd:.3f}  wgrad {r_wg:.3f}")
    assert r_fwd <= 1.0 and r_bwd <= 1.0 and r_wg <= 1.0
    return y, hd, dh, gx, got


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("R", [16, 64])
@pytest.mark.parametrize("D", [64, 768])
@pytest.mark.parametrize("M", [1, 51, 394])
def test_kernels_against_fp64(M, D, R, dtype):
    _check_all(M, D, R, dtype, 0.0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("M,D,R", [(51, 64, 16), (394, 768, 64)])
def test_dropout_against_fp64_with_the_exported_mask(M, D, R, dtype):
    """the forward and the five gradients under p = 0.1 match fp64 fed with the bytes of clhip_adapter_dropout_mask; same seed, same bits"""
    seed = _seed(0x1234567887654321)
    a = _check_all(M, D, R, dtype, 0.1, seed, layer=3)
    b = _check_all(M, D, R, dtype, 0.1, seed, layer=3)
    flat = lambda r: list(r[:4]) + list(r[4])
    assert all(torch.equal(s, t) for s, t in zip(flat(a), flat(b)))
    # dropped elements of hd are exact zeros, kept ones are scaled: the stored hd itself shows the mask
    mask = _mask(seed, 3, M, R, 0.1).bool()
    assert not a[1][~mask].any()
    torch.cuda.synchronize()


def test_dropout_mask_statistics():
    M, R, p = 2048, 64, 0.1                                             # 131072 elements
    n = M * R
    s1, s2 = _seed(11), _seed(12)
    m = _mask(s1, 0, M, R, p)
    rate, sigma = float(m.double().mean()), (p * (1 - p) / n) ** 0.5
    print(f"keep rate {rate:.5f} over {n} elements (0.9 +- {4 * sigma:.5f})")
    assert abs(rate - (1 - p)) <= 4 * sigma
    assert float((m != _mask(s1, 1, M, R, p)).double().mean()) > 0.05   # another layer
    assert float((m != _mask(s2, 0, M, R, p)).double().mean()) > 0.05   # another seed
    assert torch.equal(m, _mask(s1, 0, M, R, p))
    assert _mask(None, 0, 64, 16, 0.0).all()                            # p = 0: no seed, nothing dropped
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_zero_up_projection_leaves_y_unchanged(dtype):
    for M, D, R in ((51, 64, 16), (394, 768, 64)):
        dev, _, W, _ = _inputs(M, D, R, dtype, zero_up=True)
        for p, seed in ((0.0, None), (0.1, _seed(5))):
            y, hd = _fwd(dev, W, dtype, p, seed)
            assert torch.equal(y, dev["y"]) and hd.any()
    torch.cuda.synchronize()


def test_argument_checks():
    dev, _, W, _ = _inputs(8, 64, 16, "f32")
    L = _lib.lib()
    y, hd, seed = dev["y"].clone(), torch.empty(8, 16, device=DEV), _seed(1)
    before = y.clone()

    def fwd(D=64, R=16, p=0.0, s=None):
        return L.clhip_adapter_fwd(dev["x"].data_ptr(), W[0].data_ptr(), W[1].data_ptr(), W[2].data_ptr(), W[3].data_ptr(), y.data_ptr(), hd.data_ptr(),
                                   s.data_ptr() if s is not None else None, 0, p, S, 1, D, R, _lib.F32, _st())
    assert fwd() == 0 and fwd(p=0.1, s=seed) == 0
    y.copy_(before)
    assert fwd(R=8) == -1 and fwd(R=48) == -1 and fwd(R=128) == -1           # R in {16, 32, 64}
    assert fwd(D=96) == -1 and fwd(D=0) == -1                                # D % 64 == 0
    assert fwd(p=1.0, s=seed) == -1 and fwd(p=-0.1, s=seed) == -1            # 0 <= p < 1
    assert fwd(p=0.1) == -1 and fwd(p=0.0, s=seed) == -1                     # a seed iff p > 0
    assert b"invalid argument" in L.clhip_last_error()
    mask = torch.empty(8, 16, dtype=torch.uint8, device=DEV)
    assert L.clhip_adapter_dropout_mask(None, 0, 8, 16, 0.1, mask.data_ptr(), _st()) == -1
    assert L.clhip_adapter_dropout_mask(seed.data_ptr(), 0, 8, 16, 1.0, mask.data_ptr(), _st()) == -1
    dh = torch.empty(8, 16, device=DEV)
    assert L.clhip_adapter_bwd(dev["gy"].data_ptr(), hd.data_ptr(), W[2].data_ptr(), W[0].data_ptr(), dh.data_ptr(), y.data_ptr(), 1.0, S, 8, 64, 16, _lib.F32, _st()) == -1
    assert L.clhip_adapter_bwd(dev["gy"].data_ptr(), hd.data_ptr(), W[2].data_ptr(), W[0].data_ptr(), dh.data_ptr(), y.data_ptr(), 0.0, S, 8, 64, 24, _lib.F32, _st()) == -1
    assert L.clhip_adapter_wgrad_ws_bytes(8, 64, 24) == 0 and L.clhip_adapter_wgrad_ws_bytes(8, 96, 16) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, before)                                            # a refused call launches nothing


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("M,D,R,p", [(1, 64, 16, 0.0), (51, 64, 16, 0.1), (394, 768, 64, 0.0), (394, 768, 64, 0.1), (130, 192, 32, 0.1)])
def test_both_workgroup_heights(M, D, R, p, dtype):
    """clhip_config("ADAPTER_TM", "32" | "64"): the 64-row form meets the same fp64 bounds, and -- the k order of every sum is the same -- the same bits"""
    L = _lib.lib()
    seed = _seed(77) if p > 0 else None
    res = {}
    try:
        for tm in (b"32", b"64"):
            assert L.clhip_config(b"ADAPTER_TM", tm) == 0
            res[tm] = _check_all(M, D, R, dtype, p, seed, layer=1)
    finally:
        L.clhip_config(b"ADAPTER_TM", None)
    flat = lambda r: list(r[:4]) + list(r[4])
    assert all(torch.equal(a, b) for a, b in zip(flat(res[b"32"]), flat(res[b"64"])))
    torch.cuda.synchronize()
