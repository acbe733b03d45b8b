"""csrc/sdlora.hip alone on the MI355X, in fp32 and bf16, against the fp64 restatement of tests/sdlora_ref.py.

Bounds, by the rule of tests/test_adapter_kernels_gpu.py (u = 2^-24, the unit of the fp32 accumulation both modes use; v = 2^-8, bf16's): a product over K
terms in fp32 is within K u sum|a b| of fp64 whatever the summation order, each product with its own K; an operand that already carries an error e adds
e |b| summed; every further fp32 operation on a value c adds u |c|; a value STORED as bf16 adds one bf16 step, 2 v |c|.  The bf16 mode is compared with
the fp64 formula on the operands the kernels really use: A of every term and B of the current term rounded to bf16 where they enter the MFMA products,
the fp32 B where the magnitude gradient reads it.  P = X A^T and U = dY B are stored in the compute dtype between the K = D and the K = M products.
"""
import ctypes as C

import pytest
import torch

import sdlora_ref as R
from libcontinual_amd import _lib
from libcontinual_amd._lib import call

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U, V = 2.0 ** -24, 2.0 ** -8
DT = {"f32": (_lib.F32, torch.float32, 0.0), "bf16": (_lib.BF16, torch.bfloat16, V)}
RANKS = {"r10": [10], "r10x2": [10, 10], "r10_8_6_6": [10, 8, 6, 6], "r16x3": [16, 16, 16]}
SHAPES = [(D, M, k) for D in (64, 128) for M in (1, 65, 591) for k in RANKS] + [(768, 394, "r10x3"), (64, 1100, "r10x2")]       # the last: two slabs of rows
RANKS["r10x3"] = [10, 10, 10]
RANKS["r1"] = [1]
# the shared slab product (csrc/tn_slab.hip): one row short of, on and one row past the 1024-row slab edge, and the first M that sizes its slabs by the
# second rule (ceil(ceil(M / 16) / 64) * 64 = 1088 rows, 16 slabs)
SHAPES += [(64, M, k) for M in (1023, 1024, 1025) for k in ("r1", "r10x2")] + [(64, 16385, "r10x2")]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _q(t, dtype):
    """the value a fp32 tensor has once the kernels rounded it to the compute dtype, in fp64"""
    return t.to(DT[dtype][1]).double() if dtype == "bf16" else t.double()


def _factors(layers, D, ranks, g):
    """fp32 factors [layer][A_q, B_q, A_v, B_v][term] on the host, the same on the device, and the device pointer table [layers, 4, T + 1]"""
    host = [[[torch.empty(*((r, D) if w % 2 == 0 else (D, r))).uniform_(-0.3, 0.3, generator=g) for r in ranks] for w in range(4)] for _ in range(layers)]
    dev = [[[t.to(DEV) for t in row] for row in lay] for lay in host]
    tab = torch.tensor([[[t.data_ptr() for t in row] for row in lay] for lay in dev], dtype=torch.int64).to(DEV)
    return host, dev, tab


def _mag_inv(layers, T1, g, zero_inv):
    mag = torch.empty(T1).uniform_(0.5, 1.5, generator=g)
    inv = torch.empty(layers, 2, T1).uniform_(0.2, 0.9, generator=g)
    inv[:, :, -1] = 1.0
    if zero_inv and T1 > 1:
        inv[:, 1, 0] = 0.0                                   # a skipped term (one of its norms was 0) on the v side
    return mag, inv


def _ratio(got, want, bound):
    err = (got.double().cpu() - want).abs()
    assert torch.isfinite(err).all()
    return float((err / bound.clamp_min(1e-300)).max())


# --------------------------------------------------------------------------------------------------------------- refresh
def _refresh(D, ranks, dtype, layers=2, seed=0):
    g = torch.Generator().manual_seed(100 + seed + D + sum(ranks))
    T1, tdt, v = len(ranks), DT[dtype][1], DT[dtype][2]
    host, dev, tab = _factors(layers, D, ranks, g)
    mag, inv = _mag_inv(layers, T1, g, True)
    W = [torch.empty(3 * D, D).uniform_(-0.1, 0.1, generator=g) for _ in range(layers)]
    Wd = [w.to(DEV) for w in W]
    fill = [torch.randn(3 * D, D, generator=g).to(tdt).to(DEV) for _ in range(layers)]
    wt, wtt = [f.clone() for f in fill], [f.t().contiguous() for f in fill]
    magd, invd = mag.to(DEV), inv.to(DEV)
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    rk = (C.c_int * T1)(*ranks)
    call("clhip_sdlora_refresh", layers, arr(Wd), tab.data_ptr(), rk, T1, magd.data_ptr(), invd.data_ptr(), arr(wt), arr(wtt), D, DT[dtype][0], _st())
    worst = 0.0
    for l in range(layers):
        c = mag.double()[None, :] * inv[l].double()                                                  # [2, T1]
        for w, r0 in ((0, 0), (1, 2 * D)):
            A, B = [t.double() for t in host[l][2 * w]], [t.double() for t in host[l][2 * w + 1]]
            want = W[l][r0:r0 + D].double() + sum(c[w, i] * (B[i] @ A[i]) for i in range(T1))
            mass = W[l][r0:r0 + D].double().abs() + sum(c[w, i].abs() * (B[i].abs() @ A[i].abs()) for i in range(T1))
            bound = (sum(ranks) + 3 * T1 + 2) * U * mass + 2 * v * want.abs()
            worst = max(worst, _ratio(wt[l][r0:r0 + D], want, bound), _ratio(wtt[l][:, r0:r0 + D].t(), want, bound))
            assert torch.equal(wt[l][r0:r0 + D], wtt[l][:, r0:r0 + D].t())                          # both orientations hold the same rounded value
        assert torch.equal(wt[l][D:2 * D], fill[l][D:2 * D]) and torch.equal(wtt[l][:, D:2 * D], fill[l].t()[:, D:2 * D])      # k rows untouched
        assert not torch.equal(wt[l][:D], fill[l][:D])
    return worst, wt, wtt


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rk", ["r10", "r10x2", "r10_8_6_6", "r16x3"])
def test_refresh(D, rk, dtype):
    worst, wt, wtt = _refresh(D, RANKS[rk], dtype)
    print(f"sdlora refresh D={D} ranks={RANKS[rk]} {dtype}: largest error / bound {worst:.3f}")
    assert worst <= 1.0
    _, wt2, wtt2 = _refresh(D, RANKS[rk], dtype)
    assert all(torch.equal(a, b) for a, b in zip(wt + wtt, wt2 + wtt2))                             # bitwise reproducible


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_refresh_vit_b16_width(dtype):
    worst, _, _ = _refresh(768, RANKS["r10x3"], dtype, layers=3)
    print(f"sdlora refresh D=768 ranks=[10, 10, 10] {dtype}: largest error / bound {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------------ grad
def _grad_inputs(D, M, ranks, dtype, seed=0):
    g = torch.Generator().manual_seed(7 + seed + D + M + sum(ranks))
    tdt = DT[dtype][1]
    host, dev, tab = _factors(1, D, ranks, g)
    mag, inv = _mag_inv(1, len(ranks), g, True)
    X = torch.randn(M, D, generator=g).to(tdt)
    dY = (torch.randn(M, 3 * D, generator=g) * 0.1).to(tdt)
    return host[0], dev, tab, mag, inv[0], X, dY


def _grad_call(D, M, ranks, dtype, tab, mag, inv, X, dY):
    T1, r = len(ranks), ranks[-1]
    outs = [torch.full(s, 7.0, device=DEV) for s in ((r, D), (D, r), (r, D), (D, r), (T1,))]       # written, not accumulated into
    ws = torch.empty(_lib.lib().clhip_sdlora_grad_ws_bytes(M, D, sum(ranks)), dtype=torch.uint8, device=DEV)
    Xd, dYd, magd, invd = X.to(DEV), dY.to(DEV), mag.to(DEV), inv.to(DEV)
    call("clhip_sdlora_grad", Xd.data_ptr(), dYd.data_ptr(), tab.data_ptr(), (C.c_int * T1)(*ranks), T1, magd.data_ptr(), invd.data_ptr(),
         *[o.data_ptr() for o in outs], ws.data_ptr(), M, D, DT[dtype][0], _st())
    torch.cuda.synchronize()
    return outs


def _grad_check(D, M, ranks, dtype):
    v = DT[dtype][2]
    host, dev, tab, mag, inv, X, dY = _grad_inputs(D, M, ranks, dtype)
    got = _grad_call(D, M, ranks, dtype, tab, mag, inv, X, dY)
    X64, dY64, m64, inv64 = X.double(), dY.double(), mag.double(), inv.double()
    want, bound = R.grads_bounded(X64, dY64, host, mag, inv, lambda t: _q(t, dtype), v)       # (the numbers live in sdlora_ref: the executor's test shares them)
    ratios = [_ratio(g, w_, b_) for g, w_, b_ in zip(got, want, bound)]
    want_dm, mT = want[4], m64[-1]
    # the closed form itself (fp32 operands, no rounding model) agrees with the restatement
    ref = R.grads(X64, dY64, [_q(a, dtype) for a in host[0]], [b.double() for b in host[1]], [_q(a, dtype) for a in host[2]], [b.double() for b in host[3]],
                  m64, inv64[0], inv64[1])
    assert float((ref[4] - want_dm).abs().max()) <= 1e-12 * float(want_dm.abs().max() + 1)
    assert float((ref[1] - mT * (dY64[:, :D].T @ (X64 @ _q(host[0][-1], dtype).T))).abs().max()) < 1e-12
    if len(ranks) > 1:
        assert float(inv[1, 0]) == 0.0                                                                # the zero-inv term is among the cases
    got2 = _grad_call(D, M, ranks, dtype, tab, mag, inv, X, dY)
    assert all(torch.equal(a, b) for a, b in zip(got, got2))                                          # bitwise reproducible
    return max(ratios)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D,M,rk", SHAPES)
def test_grad(D, M, rk, dtype):
    worst = _grad_check(D, M, RANKS[rk], dtype)
    print(f"sdlora grad D={D} M={M} ranks={RANKS[rk]} {dtype}: largest error / bound {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------- refused arguments
BAD = [("rank 0", 64, 8, [10, 0]), ("rank 17", 64, 8, [17]), ("sum of ranks 528", 64, 8, [16] * 33), ("no term", 64, 8, []), ("D 96", 96, 8, [10]),
       ("M 0", 64, 0, [10])]


@pytest.mark.parametrize("what,D,M,ranks", BAD, ids=[b[0] for b in BAD])
def test_refused_arguments_launch_nothing(what, D, M, ranks):
    L = _lib.lib()
    T1, r = len(ranks), max(1, min(16, ranks[-1] if ranks else 1))
    rk = (C.c_int * max(T1, 1))(*ranks)
    tab = torch.zeros(4 * max(T1, 1), dtype=torch.int64, device=DEV)                                  # never dereferenced: the call must stop before any launch
    mag, inv = torch.ones(max(T1, 1), device=DEV), torch.ones(2 * max(T1, 1), device=DEV)
    outs = [torch.full((r * D,), 7.0, device=DEV) for _ in range(4)] + [torch.full((max(T1, 1),), 7.0, device=DEV)]
    x, dy = torch.zeros(max(M, 1), D, device=DEV), torch.zeros(max(M, 1), 3 * D, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    rc = L.clhip_sdlora_grad(x.data_ptr(), dy.data_ptr(), tab.data_ptr(), rk, T1, mag.data_ptr(), inv.data_ptr(), *[o.data_ptr() for o in outs], ws.data_ptr(), M, D,
                             _lib.F32, _st())
    assert rc != 0 and L.clhip_last_error()
    if what != "M 0":                                                                                 # (the refresh has no M)
        w = torch.zeros(3 * D, D, device=DEV)
        wt, wtt = torch.full((3 * D, D), 7.0, device=DEV), torch.full((D, 3 * D), 7.0, device=DEV)
        one = lambda t: (C.c_void_p * 1)(t.data_ptr())
        rc = L.clhip_sdlora_refresh(1, one(w), tab.data_ptr(), rk, T1, mag.data_ptr(), inv.data_ptr(), one(wt), one(wtt), D, _lib.F32, _st())
        assert rc != 0 and L.clhip_last_error()
        outs += [wt, wtt]
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)
    with pytest.raises(_lib.ClhipError):
        call("clhip_sdlora_grad", x.data_ptr(), dy.data_ptr(), tab.data_ptr(), rk, T1, mag.data_ptr(), inv.data_ptr(), *[o.data_ptr() for o in outs[:5]],
             ws.data_ptr(), M, D, _lib.F32, _st())
