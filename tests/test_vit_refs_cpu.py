"""tests/vit_refs.py against torch autograd in fp64 (bound 1e-10), and the input generators against the conditions that
tests/test_vit_ops_kernels_gpu.py relies on: the shifted-logit attention inputs really hold a query row with lse < -100 and one with
lse > +100 (and a one-hot row and a uniform head), the L2P generators leave no per-sample top-k decision inside the fp32 noise, and the
constructed batch-majority tie is a tie."""
import math

import pytest
import torch
import torch.nn.functional as F

import vit_refs as V

TOL = 1e-10


def close(got, want, name, floor=1e-300):
    """relative to max|want|, or to `floor` where the expected tensor is exactly zero (dq, dk at one token)"""
    got, want = got.double(), want.double()
    err = float((got - want).abs().max()) / max(float(want.abs().max()), floor)
    assert err <= TOL, (name, err)


# ------------------------------------------------------------------------------------------------ attention
def _autograd_attention(qkv, dout, B, N, H, hd, sdpa):
    x = qkv.double().requires_grad_(True)
    q, k, v = V.split_qkv(x, B, N, H, hd)
    if sdpa:
        o = F.scaled_dot_product_attention(q, k, v)
    else:
        o = ((q @ k.transpose(-2, -1)) / math.sqrt(hd)).softmax(-1) @ v
    (o * V.heads(dout.double(), B, N, H, hd)).sum().backward()
    dq, dk, dv = V.split_qkv(x.grad, B, N, H, hd)
    lse = torch.logsumexp((q @ k.transpose(-2, -1)).detach() / math.sqrt(hd), -1)
    return o.detach(), lse, dq, dk, dv


@pytest.mark.parametrize("B,N,H,hd,sdpa", [(2, 1, 3, 64, False), (2, 17, 3, 64, True), (2, 33, 3, 32, False), (1, 50, 2, 8, True)])
def test_attn_ref_is_autograd(B, N, H, hd, sdpa):
    qkv, dout = V.attn_inputs(B, N, H, hd, 11, "f32")
    want = _autograd_attention(qkv, dout, B, N, H, hd, sdpa)
    for nm, a, b in zip(("out", "lse", "dq", "dk", "dv"), V.attn_ref(qkv, dout, B, N, H, hd), want):
        close(a, b, nm, floor=float(want[4].abs().max()) if N == 1 else 1e-300)


SHIFTED = [(197, 64), (208, 64), (224, 64), (240, 64), (197, 32)]      # every (N, hd) the GPU test feeds the construction at


@pytest.mark.parametrize("N,hd", SHIFTED)
def test_shifted_logit_generator(N, hd):
    """the reference on the shifted inputs agrees with autograd (explicit softmax), all of it finite; row 0 of (batch 0, head 0) has
    lse < -100, row 1 has lse > +100, row 2 of head 1 is one-hot on key 5, (batch 1, head 2) is uniform; and every value is bf16-exact"""
    B, H = 2, 3
    qkv, dout = V.attn_shifted_inputs(B, N, H, hd, 500 + N)
    assert torch.equal(qkv, V.rb(qkv)) and torch.equal(dout, V.rb(dout))
    ref = V.attn_ref(qkv, dout, B, N, H, hd)
    for nm, a, b in zip(("out", "lse", "dq", "dk", "dv"), ref, _autograd_attention(qkv, dout, B, N, H, hd, False)):
        assert bool(torch.isfinite(a).all()), nm
        close(a, b, nm)
    lse = ref[1]
    assert float(lse[0, 0, V.SHIFT_LOW]) < -100 and float(lse[0, 0, V.SHIFT_HIGH]) > 100
    q, k, _ = V.split_qkv(qkv.double(), B, N, H, hd)
    p = ((q @ k.transpose(-2, -1)) / math.sqrt(hd)).softmax(-1)
    assert float(p[0, 1, V.SHIFT_ONEHOT, V.SHIFT_ONEHOT_KEY]) > 0.999
    assert float((p[1, 2] - 1.0 / N).abs().max()) < 1e-12
    # the conditioning term the GPU test admits stays far below the bf16 numbers and is what it says: hd 2^-24 |logit|-ish
    cond = hd * V.U * V.attn_logit_abs(qkv, B, N, H, hd)
    assert 1e-4 < float(cond.max()) < 2e-3


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("M,D,eps,offset", [(1, 8, 1e-5, False), (5, 520, 1e-6, False), (7, 1032, 1e-5, True), (6, 64, 1e-6, True)])
def test_ln_ref_is_autograd(M, D, eps, offset):
    x, gamma, beta, dy, _ = V.ln_inputs(M, D, 21, "f32", offset)
    y, mean, rstd, dx = V.ln_ref(x, gamma, beta, dy, eps)
    xd = x.double().requires_grad_(True)
    want = F.layer_norm(xd, (D,), gamma.double(), beta.double(), eps)
    (want * dy.double()).sum().backward()
    close(y, want.detach(), "y")
    close(dx, xd.grad, "dx")
    close(mean, x.double().mean(1), "mean")
    close(rstd, 1 / torch.sqrt(x.double().var(1, unbiased=False) + eps), "rstd")
    if offset:
        assert float((mean.abs() / x.double().std(1)).min()) > 100        # |mean| >> std


@pytest.mark.parametrize("B,N,D,P", [(1, 1, 8, 1), (3, 5, 100, 5), (2, 7, 2040, 3), (3, 30, 768, 25)])
def test_ln_pool_ref_is_autograd(B, N, D, P):
    x, gamma, beta, dfeat = V.ln_pool_inputs(B, N, D, 31, "f32")
    feat, g = V.ln_pool_ref(x, gamma, beta, dfeat, B, N, D, P, 1e-6)
    xd = x.double().requires_grad_(True)
    want = F.layer_norm(xd.reshape(B, N, D), (D,), gamma.double(), beta.double(), 1e-6)[:, :P].mean(1)
    (want * dfeat.double()).sum().backward()
    close(feat, want.detach(), "feat")
    close(g.reshape(B * N, D), xd.grad, "g")
    assert float(g[:, P:].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ LoRA, Gram
@pytest.mark.parametrize("rows,cols,rank", [(96, 32, 1), (120, 40, 10), (216, 72, 16), (50, 70, 0)])
def test_weight_eff_and_lora_db_refs(rows, cols, rank):
    w, Ak, Bk, Av, Bv = V.lora_inputs(rows, cols, rank, 41)
    eff = V.weight_eff_ref(w, Ak, Bk, Av, Bv)
    if rank == 0:
        assert torch.equal(eff, w.double())
        return
    Dl = rows // 3
    close(eff[:Dl], w[:Dl].double(), "q rows")
    # the forward x W_eff^T; its autograd gradients w.r.t. B_k / B_v are the shortcut formula (square case: cols == Dl)
    M = 37
    x, dy = V.randn((M, cols), 42).double(), V.randn((M, rows), 43).double()
    bk, bv = Bk.double().requires_grad_(True), Bv.double().requires_grad_(True)
    wq = w.double()
    full = torch.cat([wq[:Dl], wq[Dl:2 * Dl] + bk @ Ak.double(), wq[2 * Dl:] + bv @ Av.double()])
    close(full.detach(), eff, "eff")
    ((x @ full.T) * dy).sum().backward()
    if cols == Dl:
        dbk, dbv = V.lora_db_ref(x, dy, Ak, Av, Dl)
        close(dbk, bk.grad, "dBk")
        close(dbv, bv.grad, "dBv")


def test_gram_ref():
    x = V.randn((130, 72), 51)
    xd = x.double().requires_grad_(True)
    close(V.gram_ref(x), torch.einsum("mi,mj->ij", xd, xd).detach(), "gram")


# ------------------------------------------------------------------------------------------------------ L2P
def _l2p_autograd(q, key, ids):
    kd = key.double().requires_grad_(True)
    kn, qn = F.normalize(kd, dim=-1), F.normalize(q.double(), dim=-1)
    val = (kn[torch.tensor(ids)].unsqueeze(0) * qn.unsqueeze(1)).sum() / q.shape[0]
    val.backward()
    return val.detach(), kd.grad, (qn @ kn.T).detach()


def _l2p_all_inputs():
    for case in V.L2P_CASES:
        B, D, pool, top_k, length = case
        yield case, V.l2p_inputs(B, D, pool, length, V.l2p_seed(B, D, pool)), None
    B, D, pool, top_k, length = V.L2P_ZERO_KEY_CASE
    yield V.L2P_ZERO_KEY_CASE, V.l2p_inputs(B, D, pool, length, V.l2p_seed(B, D, pool), V.L2P_ZERO_KEY_ROW), V.L2P_ZERO_KEY_ROW
    yield V.L2P_TIE_SHAPE, V.l2p_tie_inputs(), None


def test_l2p_ref_is_autograd_and_topk():
    for (B, D, pool, top_k, length), (q, key, _), zero_row in _l2p_all_inputs():
        r = V.l2p_ref(q, key, top_k)
        val, dkey, sim = _l2p_autograd(q, key, r["ids"])
        close(r["sim"], sim, "sim")
        close(r["reduce_sim"], val, "reduce_sim")
        close(r["dkey"], dkey, "dkey")
        assert bool(torch.isfinite(r["dkey"]).all())
        _, idx = torch.topk(sim, top_k, dim=1)
        assert torch.equal(torch.sort(idx, 1)[0], torch.sort(r["topk"], 1)[0])
        assert r["counts"].tolist() == torch.bincount(idx.reshape(-1), minlength=pool).tolist()
        assert r["ids"] == sorted(range(pool), key=lambda j: (-int(r["counts"][j]), j))[:top_k]
        if zero_row is not None:
            assert zero_row in r["ids"] and float(r["dkey"][zero_row].abs().max()) > 1e9      # sbar / 1e-12


def test_l2p_generators_leave_no_decision_inside_the_noise():
    """no sample's k-th / (k+1)-th cosine gap is inside the fp32 noise bound (the GPU test may leave out up to 2%: here none)"""
    for (B, D, pool, top_k, length), (q, key, _), _ in _l2p_all_inputs():
        r = V.l2p_ref(q, key, top_k)
        near = r["gap"] <= r["noise"]
        assert int(near.sum()) == 0, ((B, D, pool, top_k), r["gap"].min(), r["noise"].max())


def test_l2p_tie_generator_ties():
    B, D, pool, top_k, length = V.L2P_TIE_SHAPE
    q, key, _ = V.l2p_tie_inputs()
    r = V.l2p_ref(q, key, top_k)
    assert [tuple(t) for t in r["topk"].tolist()] == V.L2P_TIE_PICKS
    c = r["counts"].tolist()
    assert c[1] == c[3] == max(c) and sorted(c)[-3] < c[1]          # ids 1 and 3 tie at the top, nobody else is near
    assert r["ids"] == V.L2P_TIE_IDS
    # a scan that lets a later id replace an equal count (">=") would answer [3, 1]
    wrong = sorted(range(pool), key=lambda j: (-c[j], -j))[:top_k]
    assert wrong != r["ids"]


# --------------------------------------------------------------------------------------------------- tokens
@pytest.mark.parametrize("B,S,p", [(1, 8, 8), (3, 32, 8), (2, 48, 16)])
def test_patchify_ref_is_unfold(B, S, p):
    img = V.randn((B, 3, S, S), 61)
    want = F.unfold(img, p, stride=p).transpose(1, 2).reshape(B * (S // p) ** 2, -1)
    assert torch.equal(V.patchify_ref(img, p), want)


@pytest.mark.parametrize("B,D,n_prompt", [(1, 8, 0), (3, 128, 6), (3, 8, 1)])
def test_assemble_and_prompt_grad_refs(B, D, n_prompt):
    npch = 6
    N = n_prompt + 1 + npch
    pe, cls, pos, prompt = V.randn((B * npch, D), 71), V.randn((D,), 72), V.randn((npch + 1, D), 73), V.randn((6, D), 74)
    x = V.assemble_ref(pe, cls, pos, prompt, B, npch, n_prompt, D)
    assert x.shape == (B * N, D)
    x3 = x.reshape(B, N, D)
    close(x3[:, n_prompt], (cls.double() + pos[0].double()).expand(B, D), "cls")
    close(x3[:, n_prompt + 1:], pe.double().reshape(B, npch, D) + pos[1:].double(), "patches")
    if n_prompt:
        close(x3[:, :n_prompt], prompt[:n_prompt].double().expand(B, n_prompt, D), "prompt tokens")
        # the gradient of the prompt tokens, every sample seeing the same ones
        g = V.randn((B * N, D), 75)
        pd = prompt[:n_prompt].double().requires_grad_(True)
        (pd.expand(B, n_prompt, D) * g.double().reshape(B, N, D)[:, :n_prompt]).sum().backward()
        close(V.prompt_grad_ref(g, B, N, n_prompt, D), pd.grad, "dprompt")
