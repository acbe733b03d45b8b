"""csrc/dual.hip alone on the MI355X against the fp64 restatement of tests/dual_ref.py (the literal F.normalize / topk formulas, gradients by autograd); the
query is fed directly.

Bounds, by the rule in the header of tests/test_coda_kernels_gpu.py (u = 2^-24): a product over K terms in fp32 is within K u sum|a b| of fp64 whatever the
summation order; an operand that already carries an error e adds e |b| summed; every further fp32 operation on a value c adds u |c|.  Written out for the
kernels (mq = max(|q_b|, 1e-12), mk = max(|K|, 1e-12), K the key of row task_id, g the cotangent of the key loss):
  num = <q_b, K>              e_num = D u sum|q K|
  |q_b|, |K|                  relative (D / 2 + 2) u                            (a D-term sum of squares, then the root)
  cos = num / (mq mk)         e_cos = e_num / (mq mk) + (D + 7) u |cos|
  loss = sum_l sum_b (1-cos)  sum e_cos + (B + 1) u sum_b |1 - cos| per layer, + layers u sum_l |loss_l|
  dg_p, de_p[task] = sum_b [dpk_b | dpv_b]          B u sum_b |.|             (the inputs are exact)
  s = sum_b q_b / mq          e_s = (D / 2 + 3 + B) u sum_b |q_b| / mq
  S = <s, K>                  e_S = sum e_s |K| + D u sum|s K|
  de_k[task] = g (coef K - s / mk),  coef = [|K| >= eps] S / (mk^2 |K|):
                              e_coef = e_S / (mk^2 |K|) + (1.5 D + 10) u |coef|;  |g| (e_s / mk + (D / 2 + 3) u |s| / mk + e_coef |K| + u |coef K|)
                              + 2 u |g| (|s| / mk + |coef K|)
pk / pv are copies: bit-equal to the selected rows in f32, to their round-to-nearest-even bf16 in bf16 mode.  A zero key row has norm 0 < eps: mk = eps, the
indicator is off, cos is exactly 0 and the same bounds hold relative to a gradient that is 10^12 times larger."""
import ctypes as C

import pytest
import torch

import dual_ref as R
from libcontinual_amd import _lib
from libcontinual_amd._lib import call

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
EPS = 1e-12
DT = {"f32": (_lib.F32, torch.float32), "bf16": (_lib.BF16, torch.bfloat16)}
SENTINEL = 7.0
GAP = 1e-4
# (G-layers, E-layers, B, D, pool, Lg, Le): the fixture's geometry; one layer, one sample, a pool of one and Lp 1; D above one pass of a wave (and of the
# key gradient's 256 columns) and Lp 1 on the G side; the layer table's cap
CASES = [(2, 3, 6, 64, 10, 6, 8), (0, 1, 1, 64, 1, 2, 2), (2, 3, 5, 128, 10, 2, 20), (1, 8, 3, 64, 7, 4, 4), (1, 1, 3, 320, 4, 2, 2)]
TRAIN = [(c, t) for c in CASES for t in sorted({0, c[4] // 2, c[4] - 1})]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _arr(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def make_inputs(case, seed, zero_row=None):
    """fp32 host tensors: q [B, D]; per G-layer (g_p, dpk, dpv); per E-layer (e_k, e_p, dpk, dpv); the key loss's cotangent"""
    ng, ne, B, D, pool, Lg, Le = case
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, D, generator=g)
    G = [(torch.rand(Lg, D, generator=g), torch.randn(B, Lg // 2, D, generator=g), torch.randn(B, Lg // 2, D, generator=g)) for _ in range(ng)]
    E = []
    for _ in range(ne):
        K = torch.randn(pool, D, generator=g)
        if zero_row is not None:
            K[zero_row] = 0
        E.append((K, torch.rand(pool, Le, D, generator=g), torch.randn(B, Le // 2, D, generator=g), torch.randn(B, Le // 2, D, generator=g)))
    return q, G, E, torch.tensor([0.75 + 0.5 * float(torch.rand((), generator=g))])


def fwd(case, q, G, E, train, task_id, dtype):
    """-> pk, pv (lists over G- then E-layers, [B, L/2, D]), cos [ne, B, pool], idx [ne, B], loss [1]; the rows and words past the end keep their sentinel"""
    ng, ne, B, D, pool, Lg, Le = case
    code, tdt = DT[dtype]
    qd = q.to(DEV)
    gp, ek, ep = [t[0].to(DEV) for t in G], [t[0].to(DEV) for t in E], [t[1].to(DEV) for t in E]
    pk = [torch.full((B + 1, L // 2, D), float("nan"), device=DEV, dtype=tdt) for L in [Lg] * ng + [Le] * ne]
    pv = [torch.full((B + 1, L // 2, D), float("nan"), device=DEV, dtype=tdt) for L in [Lg] * ng + [Le] * ne]
    for t in pk + pv:
        t[B:] = SENTINEL
    cos = torch.full((ne * B * pool + 8,), float("nan"), device=DEV)
    cos[ne * B * pool:] = SENTINEL
    idx = torch.full((ne * B + 8,), -5, device=DEV, dtype=torch.int32)
    loss = torch.full((9,), SENTINEL, device=DEV)
    call("clhip_dual_fwd", ng, ne, qd.data_ptr(), _arr(gp), _arr(ek), _arr(ep), _arr(pk), _arr(pv), cos.data_ptr(), idx.data_ptr(), loss.data_ptr(), B, D, pool,
         Lg, Le, int(train), task_id, code, _st())
    torch.cuda.synchronize()
    assert bool((cos[ne * B * pool:] == SENTINEL).all()) and bool((idx[ne * B:] == -5).all()) and bool((loss[1:] == SENTINEL).all())
    assert bool(loss[0] == SENTINEL) == (not train)                    # eval leaves the loss alone
    for t in pk + pv:
        assert bool((t[B:].float() == SENTINEL).all())
    return [t[:B] for t in pk], [t[:B] for t in pv], cos[:ne * B * pool].view(ne, B, pool), idx[:ne * B].view(ne, B), loss[:1]


def bwd(case, q, G, E, dloss, task_id):
    """-> dg_p, de_k, de_p (lists), every output filled with the sentinel first"""
    ng, ne, B, D, pool, Lg, Le = case
    qd, gd = q.to(DEV), dloss.to(DEV)
    ek = [t[0].to(DEV) for t in E]
    dpk = [t[1].to(DEV) for t in G] + [t[2].to(DEV) for t in E]
    dpv = [t[2].to(DEV) for t in G] + [t[3].to(DEV) for t in E]
    dg = [torch.full((Lg + 1, D), SENTINEL, device=DEV) for _ in range(ng)]
    dk = [torch.full((pool, D), SENTINEL, device=DEV) for _ in range(ne)]
    dp = [torch.full((pool, Le, D), SENTINEL, device=DEV) for _ in range(ne)]
    call("clhip_dual_bwd", ng, ne, qd.data_ptr(), _arr(ek), _arr(dpk), _arr(dpv), gd.data_ptr(), _arr(dg), _arr(dk), _arr(dp), B, D, pool, Lg, Le, task_id, _st())
    torch.cuda.synchronize()
    for t in dg:
        assert bool((t[Lg:] == SENTINEL).all())
    return [t[:Lg] for t in dg], dk, dp


def reference(q, K, P, dpk, dpv, dloss, task_id):
    """one E-layer in fp64 -> name -> (ref, bound); `loss` carries the layer's own sum and its bound"""
    q, K, P, dpk, dpv = (t.double() for t in (q, K, P, dpk, dpv))
    g = float(dloss)
    B, D = q.shape
    Kt, Pt = K.clone().requires_grad_(True), P.clone().requires_grad_(True)
    pk, pv, cos, idx, loss = R.select(q, Kt, Pt, True, task_id)
    dK, dP = torch.autograd.grad((pk * dpk).sum() + (pv * dpv).sum() + g * loss, (Kt, Pt))
    cos, k = cos.detach(), K[task_id]
    nq, nk = q.norm(dim=1), K.norm(dim=1)
    mq, mk = nq.clamp_min(EPS), nk.clamp_min(EPS)
    e_cos = D * U * (q.abs() @ K.abs().T) / (mq[:, None] * mk[None]) + (D + 7) * U * cos.abs()
    one = (1.0 - cos[:, task_id]).abs()
    e_loss = e_cos[:, task_id].sum() + (B + 1) * U * one.sum()
    b_dP = B * U * torch.cat((dpk, dpv), dim=1).abs().sum(0)
    qh = q / mq[:, None]
    s, mkt, nkt = qh.sum(0), mk[task_id], nk[task_id]
    e_s = (D / 2 + 3 + B) * U * qh.abs().sum(0)
    S = (s * k).sum()
    e_S = (e_s * k.abs()).sum() + D * U * (s * k).abs().sum()
    if float(nkt) >= EPS:
        coef = S / (mkt * mkt * nkt)
        e_coef = e_S / (mkt * mkt * nkt) + (1.5 * D + 10) * U * coef.abs()
    else:
        coef = e_coef = torch.zeros((), dtype=torch.float64)
    b_dK = abs(g) * (e_s / mkt + (D / 2 + 3) * U * s.abs() / mkt + e_coef * k.abs() + U * (coef * k).abs()) + 2 * U * abs(g) * (s.abs() / mkt + (coef * k).abs())
    return {"cos": (cos, e_cos), "loss": (loss.detach(), e_loss), "dK": (dK[task_id], b_dK), "dP": (dP[task_id], b_dP)}


def ratio(name, got, ref, bound):
    err = (got.double().cpu().reshape(ref.shape) - ref).abs()
    assert bool(torch.isfinite(err).all()), name
    pos = bound > 0
    assert not bool((err[~pos] > 0).any()), name                     # a bound of zero admits nothing
    r = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    print(f"[ratio] {name}: {r:.3g}")
    assert r <= 1.0, (name, r)


def rows_of(P, idx):
    """[pool, L, D], idx [B] -> the key half and the value half of the selected rows"""
    sel, i = P[idx.long().cpu()], P.shape[1] // 2
    return sel[:, :i], sel[:, i:]


def check_copies(case, G, E, pk, pv, idx, dtype):
    ng, ne, B = case[0], case[1], case[2]
    tdt = DT[dtype][1]
    for l, (gp, _, _) in enumerate(G):
        j = gp.shape[0] // 2
        assert torch.equal(pk[l].cpu(), gp[:j].to(tdt).expand(B, -1, -1)) and torch.equal(pv[l].cpu(), gp[j:].to(tdt).expand(B, -1, -1)), ("g", l)
    for l, lay in enumerate(E):
        wk, wv = rows_of(lay[1], idx[l])
        assert torch.equal(pk[ng + l].cpu(), wk.to(tdt)) and torch.equal(pv[ng + l].cpu(), wv.to(tdt)), ("e", l)


def run_train(case, task_id, dtype, seed, zero_row=None):
    ng, ne, B, D, pool, Lg, Le = case
    q, G, E, dloss = make_inputs(case, seed, zero_row)
    pk, pv, cos, idx, loss = fwd(case, q, G, E, True, task_id, dtype)
    dg, dk, dp = bwd(case, q, G, E, dloss, task_id)
    tag = f"dual {dtype} {case} task {task_id}"
    assert bool((idx == task_id).all())
    check_copies(case, G, E, pk, pv, idx, dtype)
    for l, (gp, gk, gv) in enumerate(G):
        ref = torch.cat((gk, gv), dim=1).double()
        ratio(f"{tag} g{l} dg_p", dg[l], ref.sum(0), B * U * ref.abs().sum(0))
    total, e_total, parts = 0.0, 0.0, 0.0
    for l, (K, P, gk, gv) in enumerate(E):
        ref = reference(q, K, P, gk, gv, dloss, task_id)
        ratio(f"{tag} e{l} cos", cos[l], *ref["cos"])
        ratio(f"{tag} e{l} de_k", dk[l][task_id], *ref["dK"])
        ratio(f"{tag} e{l} de_p", dp[l][task_id], *ref["dP"])
        others = [r for r in range(pool) if r != task_id]
        assert bool((dk[l][others] == SENTINEL).all()) and bool((dp[l][others] == SENTINEL).all()), (tag, l)
        total, e_total, parts = total + ref["loss"][0], e_total + ref["loss"][1], parts + ref["loss"][0].abs()
    ratio(f"{tag} key loss", loss, torch.as_tensor(total).reshape(1), torch.as_tensor(e_total + ne * U * parts).reshape(1))
    return cos, dk, loss


@pytest.mark.parametrize("case,task_id", TRAIN)
def test_train_selection_key_loss_and_gradients(case, task_id):
    run_train(case, task_id, "f32", 100 + 7 * case[2] + case[3] + task_id)


@pytest.mark.parametrize("case,task_id", [(CASES[0], 1), (CASES[2], 9)])
def test_bf16_mode_rounds_the_copies_and_nothing_else(case, task_id):
    run_train(case, task_id, "bf16", 31 + task_id)


def eval_inputs(case, seed):
    """inputs whose fp64 top-two cosine gap is >= GAP for every sample and layer: a condition of the construction, asserted, nothing is skipped"""
    q, G, E, _ = make_inputs(case, seed)
    want = []
    for K, _, _, _ in E:
        cos = R.select(q.double(), K.double(), E[0][1].double(), False, 0)[2]
        assert case[4] == 1 or float(R.gaps(cos).min()) >= GAP, (case, seed)
        want.append(cos.argmax(1))
    return q, G, E, torch.stack(want)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_eval_takes_the_closest_key(case, dtype):
    q, G, E, want = eval_inputs(case, 500 + case[2] + case[3])
    pk, pv, cos, idx, _ = fwd(case, q, G, E, False, 0, dtype)
    assert torch.equal(idx.cpu().long(), want)
    if case[4] > 2:
        assert len(set(idx.flatten().tolist())) >= 2                   # the selection does differ between samples
    check_copies(case, G, E, pk, pv, idx, dtype)


def test_eval_exact_tie_goes_to_the_lower_index():
    case = CASES[0]
    q, G, E, _ = make_inputs(case, 9)
    for K, _, _, _ in E:
        K[2] = q[0] * 0.5
        K[5] = K[2]                                                     # identical rows: identical cosines, and sample 0's best (cos = 1)
    pk, pv, cos, idx, _ = fwd(case, q, G, E, False, 0, "f32")
    assert bool((cos[:, :, 2] == cos[:, :, 5]).all()) and bool((idx[:, 0] == 2).all())
    for l, (K, _, _, _) in enumerate(E):
        c64 = R.select(q.double(), K.double(), E[l][1].double(), False, 0)[2]
        c64[:, 5] = -2.0                                               # the duplicate never wins; among the rest the gap condition holds
        assert float(R.gaps(c64).min()) >= GAP
        assert torch.equal(idx[l].cpu().long(), c64.argmax(1))
    check_copies(case, G, E, pk, pv, idx, "f32")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_zero_key_row(dtype):
    """the task's key row is zero: its cosines are exactly 0, the loss counts 1 per sample, everything is finite, and the gradient follows the clamp form
    x / max(|x|, eps) that torch differentiates (10^12 times the others)"""
    case = CASES[0]
    cos, dk, loss = run_train(case, 4, dtype, 5, zero_row=4)
    assert bool((cos[:, :, 4] == 0).all()) and bool((cos[:, :, 3] != 0).all())
    assert float(loss) == case[1] * case[2] and float(dk[0][4].abs().max()) > 1e6
    q, G, E, _ = make_inputs(case, 5, zero_row=4)
    _, _, cos, idx, _ = fwd(case, q, G, E, False, 0, dtype)
    assert bool(torch.isfinite(cos).all()) and bool((idx >= 0).all()) and bool((idx < case[4]).all())


def test_selection_is_bit_reproducible():
    case = CASES[2]
    q, G, E, dloss = make_inputs(case, 12)
    runs = []
    for _ in range(2):
        pk, pv, cos, idx, loss = fwd(case, q, G, E, True, 7, "bf16")
        dg, dk, dp = bwd(case, q, G, E, dloss, 7)
        ev = fwd(case, q, G, E, False, 0, "bf16")
        runs.append(pk + pv + [cos, idx, loss] + dg + dk + dp + ev[0] + ev[1] + [ev[2], ev[3]])
    for u, v in zip(*runs):
        assert torch.equal(u.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8))


def test_selection_rejects_bad_arguments():
    """D % 64 != 0, odd or zero lengths, task_id outside the pool (fwd: in train mode), more layers than the table holds, no layer, a null pointer"""
    t = torch.zeros(1 << 16, device=DEV)
    nine = _arr([t] * 9)
    two = _arr([t] * 18)
    ok = dict(ng=1, ne=1, D=64, pool=4, Lg=2, Le=4, task=1)
    bad = [dict(D=60), dict(D=0), dict(Lg=3), dict(Lg=0), dict(Le=5), dict(Le=0), dict(task=4), dict(task=-1), dict(pool=0), dict(ne=9), dict(ng=9),
           dict(ng=0, ne=0)]
    for ch in bad:
        a = dict(ok, **ch)
        with pytest.raises(_lib.ClhipError):
            call("clhip_dual_fwd", a["ng"], a["ne"], t.data_ptr(), nine, nine, nine, two, two, t.data_ptr(), t.data_ptr(), t.data_ptr(), 2, a["D"], a["pool"],
                 a["Lg"], a["Le"], 1, a["task"], _lib.F32, _st())
        with pytest.raises(_lib.ClhipError):
            call("clhip_dual_bwd", a["ng"], a["ne"], t.data_ptr(), nine, two, two, t.data_ptr(), nine, nine, nine, 2, a["D"], a["pool"], a["Lg"], a["Le"],
                 a["task"], _st())
    with pytest.raises(_lib.ClhipError):                               # a dtype that does not exist
        call("clhip_dual_fwd", 1, 1, t.data_ptr(), nine, nine, nine, two, two, t.data_ptr(), t.data_ptr(), t.data_ptr(), 2, 64, 4, 2, 4, 1, 1, 5, _st())
    with pytest.raises(_lib.ClhipError):                               # train mode without a place for the loss
        call("clhip_dual_fwd", 1, 1, t.data_ptr(), nine, nine, nine, two, two, t.data_ptr(), t.data_ptr(), None, 2, 64, 4, 2, 4, 1, 1, _lib.F32, _st())
    null = (C.c_void_p * 2)(t.data_ptr(), None)
    with pytest.raises(_lib.ClhipError):
        call("clhip_dual_fwd", 1, 1, t.data_ptr(), nine, nine, nine, null, two, t.data_ptr(), t.data_ptr(), t.data_ptr(), 2, 64, 4, 2, 4, 1, 1, _lib.F32, _st())
    with pytest.raises(_lib.ClhipError):
        call("clhip_dual_bwd", 1, 1, t.data_ptr(), nine, null, two, t.data_ptr(), nine, nine, nine, 2, 64, 4, 2, 4, 1, _st())
    with pytest.raises(_lib.ClhipError):
        call("clhip_dual_bwd", 1, 1, t.data_ptr(), nine, two, two, None, nine, nine, nine, 2, 64, 4, 2, 4, 1, _st())
    torch.cuda.synchronize()
    assert bool((t == 0).all())                                        # nothing was launched
