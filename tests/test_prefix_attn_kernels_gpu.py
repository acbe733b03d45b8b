"""The prefix form of csrc/attn.hip (clhip_attn_prefix_fwd / _bwd) through the C ABI on the MI355X, against the references and bounds
tests/test_vit_ops_kernels_gpu.py holds the plain form to; at the end, the two forms against each other.

No reference or bound of its own: prefix attention over (N, Lp) IS plain attention over Lp + N tokens whose first Lp rows have keys and values, an
arbitrary query and zero dout (their dS is exactly zero, they contribute nothing to dK / dV; tests/test_coda_cpu.py checks the identity in fp64).  Every
case builds that packed input, calls vit_refs.attn_ref / attn_logit_abs / attn_cancel_bound on it and holds the kernels to the bounds of
`run_attention` there, with its u, v rule (eps_o = 2^-9 in the bf16 modes, eps_ds = 2^-9 where dS is packed to bf16 for the MFMA, T 2^-24 otherwise).
Each tensor is judged per (batch, head) on the rows the kernel produces, relative to the max|ref| of THOSE rows (never looser than the packed block's).
dpk / dpv are fp32: their bound is the dk / dv bound without the final bf16 store step (half a bf16 ulp, 2^-9, off the relative part).

Both forms are instantiations of the same kernels, so the last section runs clhip_attn_fwd / _bwd on the packed form itself (T = Lp + N tokens) and
holds the token rows of the two entry-point families to each other (see test_plain_and_prefix_forms_agree)."""
import pytest
import torch

import vit_refs as V
from vit_refs import U, larger
from test_vit_ops_kernels_gpu import CODE, DEV, GUARD, TD, blocked, check, dev, guard_ok, measure, nan_out, p, st

pytestmark = pytest.mark.gpu

from libcontinual_amd import _lib           # noqa: E402
from libcontinual_amd._lib import call      # noqa: E402


def split(big, bd, B, N, Lp, D):
    """packed [B * (Lp + N), 3D] / [B * (Lp + N), D] -> qkv [B * N, 3D], pk, pv [B * Lp, D], dout [B * N, D] (the prefix rows' dout is zero)"""
    T = Lp + N
    x = big.reshape(B, T, 3, D)
    assert float(bd.reshape(B, T, D)[:, :Lp].abs().max()) == 0.0
    return (x[:, Lp:].reshape(B * N, 3 * D).contiguous(), x[:, :Lp, 1].reshape(B * Lp, D).contiguous(), x[:, :Lp, 2].reshape(B * Lp, D).contiguous(),
            bd.reshape(B, T, D)[:, Lp:].reshape(B * N, D).contiguous())


def packed_inputs(B, N, Lp, H, hd, seed, dt):
    big, bd = V.attn_inputs(B, N + Lp, H, hd, seed, dt)
    bd = bd.reshape(B, N + Lp, H * hd).clone()
    bd[:, :Lp] = 0
    return big, bd.reshape(B * (N + Lp), H * hd)


def launch(qkv, pk, pv, dout, B, N, Lp, H, hd, dt):
    D = H * hd
    q_, k_, v_, do_ = dev(qkv, dt), dev(pk, dt), dev(pv, dt), dev(dout, dt)
    out, out2 = nan_out(B * N, D, dt), nan_out(B * N, D, dt)
    lse = torch.full((B * H * N + 8,), float("nan"), device=DEV)
    lse[B * H * N:] = GUARD
    dqkv = nan_out(B * N, 3 * D, dt)
    dpk, dpv = nan_out(B * Lp, D, "f32"), nan_out(B * Lp, D, "f32")
    dsum = torch.empty(B * H * N, device=DEV)
    call("clhip_attn_prefix_fwd", p(q_), p(k_), p(v_), p(out), p(lse), B, N, Lp, H, D, CODE[dt], st())
    call("clhip_attn_prefix_fwd", p(q_), p(k_), p(v_), p(out2), None, B, N, Lp, H, D, CODE[dt], st())
    call("clhip_attn_prefix_bwd", p(q_), p(k_), p(v_), p(out), p(lse), p(do_), p(dqkv), p(dpk), p(dpv), p(dsum), B, N, Lp, H, D, CODE[dt], st())
    torch.cuda.synchronize()
    return (q_, k_, v_, do_), out, out2, lse, dqkv, dpk, dpv, dsum


def references(big, bd, B, N, Lp, H, hd, dt):
    """vit_refs.attn_references (the numbers live there: the executor's test shares them)"""
    return V.attn_references(big, bd, B, N, Lp, H, hd, dt)


def run_prefix(big, bd, B, N, Lp, H, hd, dt, tag):
    """forward (with and without lse), backward, zero-dout backward; every output against the fp64 reference of the packed form per (batch, head)"""
    D, T = H * hd, N + Lp
    qkv, pk, pv, dout = split(big, bd, B, N, Lp, D)
    ins, out, out2, lse, dqkv, dpk, dpv, dsum = launch(qkv, pk, pv, dout, B, N, Lp, H, hd, dt)
    assert guard_ok(out, B * N) and guard_ok(out2, B * N) and guard_ok(dqkv, B * N) and bool((lse[B * H * N:] == GUARD).all())
    assert guard_ok(dpk, B * Lp) and guard_ok(dpv, B * Lp)
    bits = torch.int16 if dt == "bf16" else torch.int32
    assert torch.equal(out[:B * N].view(bits), out2[:B * N].view(bits))
    for t in (out[:B * N], lse[:B * H * N], dqkv[:B * N], dpk[:B * Lp], dpv[:B * Lp]):
        assert bool(torch.isfinite(t.float()).all()), tag
    bounds, cond, ref_lse = references(big, bd, B, N, Lp, H, hd, dt)
    gq, gk, gv = V.split_qkv(V.f64(dqkv[:B * N]), B, N, H, hd)
    got = {"out": V.heads(V.f64(out[:B * N]), B, N, H, hd), "dq": gq, "dk": gk, "dv": gv,
           "dpk": V.heads(V.f64(dpk[:B * Lp]), B, Lp, H, hd), "dpv": V.heads(V.f64(dpv[:B * Lp]), B, Lp, H, hd)}
    for nm in got:
        blocked(f"{tag} {nm}", got[nm], *bounds[nm])
    tok = lambda t: t[:, :, Lp:]
    g_lse = V.f64(lse[:B * H * N]).reshape(B, H, N)
    measure(f"{tag} lse abs", g_lse, tok(ref_lse))
    check(f"{tag} lse", g_lse, tok(ref_lse), larger(torch.full_like(tok(ref_lse), V.measured(V.LSE_ABS)), V.lse_floor(cond, T, tok(ref_lse))))
    zero = torch.zeros_like(ins[3])
    dz, zk, zv = nan_out(B * N, 3 * D, dt), nan_out(B * Lp, D, "f32"), nan_out(B * Lp, D, "f32")
    call("clhip_attn_prefix_bwd", p(ins[0]), p(ins[1]), p(ins[2]), p(out), p(lse), p(zero), p(dz), p(zk), p(zv), p(dsum), B, N, Lp, H, D, CODE[dt], st())
    torch.cuda.synchronize()
    assert bool((dz[:B * N].float() == 0).all()) and guard_ok(dz, B * N), tag
    assert bool((zk[:B * Lp] == 0).all()) and bool((zv[:B * Lp] == 0).all()) and guard_ok(zk, B * Lp) and guard_ok(zv, B * Lp), tag


MFMA_CASES = [(1, 1), (12, 4), (13, 4), (16, 1), (16, 16), (197, 4), (197, 10), (197, 11), (197, 12), (222, 4), (252, 4), (255, 1)]


@pytest.mark.parametrize("N,Lp", MFMA_CASES)
def test_prefix_attention_mfma(N, Lp):
    """bf16, head dim 64, H = 3, B = 2: one key tile (12,4); the prefix pushes into a second (13,4); two key tiles over one query tile (16,1), (16,16); CODA's
    201 keys (197,4); 208 keys = 13 full tiles (197,11); 14 key tiles over 13 query tiles (197,12); 256 keys (252,4), (255,1): forward <0>, backward generic"""
    big, bd = packed_inputs(2, N, Lp, 3, 64, 700 + 3 * N + Lp, "bf16")
    run_prefix(big, bd, 2, N, Lp, 3, 64, "bf16", f"prefix bf16 hd64 N={N} Lp={Lp}")


@pytest.mark.parametrize("dt,hd", [("f32", 64), ("f32", 32), ("bf16", 32)])
@pytest.mark.parametrize("N,Lp", [(1, 1), (17, 4), (50, 5), (197, 4)])
def test_prefix_attention_generic(dt, hd, N, Lp):
    big, bd = packed_inputs(2, N, Lp, 3, hd, 900 + 3 * N + Lp, dt)
    run_prefix(big, bd, 2, N, Lp, 3, hd, dt, f"prefix {dt} hd{hd} N={N} Lp={Lp}")


def test_prefix_attention_more_workgroups_than_cus():
    """B * H = 264 workgroups at (17, 4)"""
    big, bd = packed_inputs(22, 17, 4, 12, 64, 417, "bf16")
    run_prefix(big, bd, 22, 17, 4, 12, 64, "bf16", "prefix bf16 hd64 BH=264")


@pytest.mark.parametrize("dt,hd", [("bf16", 64), ("f32", 64)])
@pytest.mark.parametrize("N,Lp", [(193, 4), (197, 4), (204, 4)])
def test_prefix_attention_shifted_logits(dt, hd, N, Lp):
    """vit_refs.attn_shifted_inputs(2, N + Lp, 3, hd, seed): a query row with every logit near -128 (lse < -100: P of a padded key overflows in the
    backward's phase A unless it is masked), one near +128, a one-hot row, a head of identical keys.  The generator puts its special QUERY rows at 0, 1, 2;
    a prefix row's query is never used, so the LAST Lp generated rows serve as the prefix (moved to the front of the packed form) and rows 0.. stay
    tokens: the softmax does not depend on the order of the keys."""
    T, D = N + Lp, 3 * hd
    x, d = V.attn_shifted_inputs(2, T, 3, hd, 500 + T)
    x, d = x.reshape(2, T, 3 * D), d.reshape(2, T, D).clone()
    d[:, N:] = 0
    big = torch.cat((x[:, N:], x[:, :N]), dim=1).reshape(2 * T, 3 * D)
    bd = torch.cat((d[:, N:], d[:, :N]), dim=1).reshape(2 * T, D)
    assert float(V.attn_ref(big, bd, 2, T, 3, hd)[1][0, 0, Lp + V.SHIFT_LOW]) < -88.7
    run_prefix(big, bd, 2, N, Lp, 3, hd, dt, f"prefix shifted {dt} hd{hd} N={N} Lp={Lp}")


@pytest.mark.parametrize("dt,hd,N,Lp", [("bf16", 64, 197, 4), ("bf16", 64, 252, 4), ("f32", 64, 50, 5)])
def test_prefix_attention_is_bit_reproducible(dt, hd, N, Lp):
    big, bd = packed_inputs(2, N, Lp, 3, hd, 31, dt)
    qkv, pk, pv, dout = split(big, bd, 2, N, Lp, 3 * hd)
    a = launch(qkv, pk, pv, dout, 2, N, Lp, 3, hd, dt)
    b = launch(qkv, pk, pv, dout, 2, N, Lp, 3, hd, dt)
    for x, y in zip(a[1:7], b[1:7]):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_prefix_attention_rejects_bad_arguments():
    """Lp = 0, N + Lp = 257, head dim 128, D % H != 0: the error code, and the NaN-filled outputs untouched"""
    for B, N, Lp, H, D in [(1, 16, 0, 1, 64), (1, 253, 4, 1, 64), (1, 16, 4, 1, 128), (1, 16, 4, 3, 64)]:
        qkv = torch.zeros(B * N, 3 * D, device=DEV, dtype=torch.bfloat16)
        pk = torch.zeros(B * max(Lp, 1), D, device=DEV, dtype=torch.bfloat16)
        out, dqkv = nan_out(B * N, D, "bf16"), nan_out(B * N, 3 * D, "bf16")
        dpk, dpv = nan_out(B * max(Lp, 1), D, "f32"), nan_out(B * max(Lp, 1), D, "f32")
        lse = torch.full((B * H * N,), float("nan"), device=DEV)
        dsum = torch.empty(B * H * N, device=DEV)
        dout = torch.zeros(B * N, D, device=DEV, dtype=torch.bfloat16)
        with pytest.raises(_lib.ClhipError):
            call("clhip_attn_prefix_fwd", p(qkv), p(pk), p(pk), p(out), p(lse), B, N, Lp, H, D, CODE["bf16"], st())
        with pytest.raises(_lib.ClhipError):
            call("clhip_attn_prefix_bwd", p(qkv), p(pk), p(pk), p(out), p(lse), p(dout), p(dqkv), p(dpk), p(dpv), p(dsum), B, N, Lp, H, D, CODE["bf16"], st())
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[:B * N].float()).all()) and bool(torch.isnan(dqkv[:B * N].float()).all()) and bool(torch.isnan(lse).all())
        assert bool(torch.isnan(dpk[:-1]).all()) and bool(torch.isnan(dpv[:-1]).all())


# ------------------------------------------------------------------------------------------- the plain and the prefix form against each other
def plain_launch(big, bd, B, T, H, hd, dt, general):
    """clhip_attn_fwd / _bwd on the packed form; general: under ATTN_BWD=1 (the general MFMA backward also where attn_bwd_mfma3_kernel is the default)"""
    D = H * hd
    x_, d_ = dev(big, dt), dev(bd, dt)
    out, dqkv = nan_out(B * T, D, dt), nan_out(B * T, 3 * D, dt)
    lse, dsum = torch.full((B * H * T,), float("nan"), device=DEV), torch.empty(B * H * T, device=DEV)
    call("clhip_attn_fwd", p(x_), p(out), p(lse), B, T, H, D, CODE[dt], st())
    if general:
        assert _lib.lib().clhip_config(b"ATTN_BWD", b"1") == 0
    try:
        call("clhip_attn_bwd", p(x_), p(out), p(lse), p(d_), p(dqkv), p(dsum), B, T, H, D, CODE[dt], st())
        torch.cuda.synchronize()
    finally:
        if general:
            _lib.lib().clhip_config(b"ATTN_BWD", None)
    return out[:B * T].float().reshape(B, T, D), lse.reshape(B, H, T), dqkv[:B * T].reshape(B, T, 3, D)


FORM_CASES = [("bf16", 64, 12, 4), ("bf16", 64, 13, 4), ("bf16", 64, 28, 4), ("bf16", 64, 29, 4), ("bf16", 64, 197, 4), ("bf16", 64, 197, 12),
              ("bf16", 64, 223, 1), ("bf16", 64, 239, 1), ("f32", 64, 17, 4), ("bf16", 32, 17, 4)]


@pytest.mark.parametrize("dt,hd,N,Lp", FORM_CASES)
def test_plain_and_prefix_forms_agree(dt, hd, N, Lp):
    """B = 2, H = 2.  clhip_attn_fwd / _bwd on the packed [B (Lp + N), 3D] input (the first Lp rows of dout zero) against clhip_attn_prefix_fwd / _bwd on its
    split form.  One key tile (12,4); the prefix opens a second key tile over one query tile (13,4); exactly one tile pair (28,4); a second pair that is all
    padding but one key (29,4); <13> and attn_bwd_mfma3_kernel against the general backward (197,4); 14 key tiles over 13 query tiles (197,12); T = 224,
    the largest MFMA backward (223,1); T = 240 (239,1): forward <0> with 15 tiles, and the backward of both forms is generic (a 256-row tile among the four
    exceeds the LDS rule); the generic kernels in both dtypes.  The plain backward runs twice, by default and under ATTN_BWD=1.
    Token rows of out, lse, dq: VALUE-EQUAL (torch.equal on floats: -0.0 == 0.0).  A query is one MFMA column in both forms, meets the same keys in the same
    tile order under the same mask (Lt = T), and the cross-lane reductions do not depend on the column or tile it sits in.
    Generic kernels: dk, dv of the token rows and dpk / dpv against the packed form's first Lp key rows are value-equal too (the zero-dout rows add exact
    zeros in front of an otherwise identical left-to-right sum); in bf16 the packed form's rows carry the bf16 store step dpk / dpv do not have, so dpk / dpv
    are rounded to bf16 (the kernel's own round-to-nearest-even store) before the comparison.
    MFMA dk, dv, dpk, dpv: the query tiles are grouped differently (shifted by Lp), so they are held to TWICE the bound run_prefix holds each tensor to
    against the fp64 reference of the packed form: both sides are within that bound of the same reference."""
    B, H, T, D = 2, 2, N + Lp, 2 * hd
    big, bd = packed_inputs(B, N, Lp, H, hd, 1300 + 3 * N + Lp, dt)
    qkv, pk, pv, dout = split(big, bd, B, N, Lp, D)
    _, out, _, lse, dqkv, dpk, dpv, _ = launch(qkv, pk, pv, dout, B, N, Lp, H, hd, dt)
    x_out, x_lse, x_dqkv = out[:B * N].float().reshape(B, N, D), lse[:B * H * N].reshape(B, H, N), dqkv[:B * N].reshape(B, N, 3, D)
    x_pre = {1: dpk[:B * Lp].reshape(B, Lp, D), 2: dpv[:B * Lp].reshape(B, Lp, D)}
    mfma = dt == "bf16" and hd == 64
    bounds = references(big, bd, B, N, Lp, H, hd, dt)[0] if mfma else None
    for general in (False, True):
        tag = f"forms {dt} hd{hd} N={N} Lp={Lp} ATTN_BWD={int(general)}"

        def within_twice(nm, a, b, rows):
            """|a - b| to twice run_prefix's bound of tensor nm (blocked() is given a - b + ref against ref)"""
            ref, rel, extra = bounds[nm]
            diff = V.heads(V.f64(a), B, rows, H, hd) - V.heads(V.f64(b), B, rows, H, hd)
            blocked(f"{tag} {nm} plain - prefix", diff + ref, ref, 2 * rel, 2 * extra)
        p_out, p_lse, p_dqkv = plain_launch(big, bd, B, T, H, hd, dt, general)
        assert torch.equal(p_out[:, Lp:], x_out), f"{tag} out"
        assert torch.equal(p_lse[:, :, Lp:], x_lse), f"{tag} lse"
        assert torch.equal(p_dqkv[:, Lp:, 0].float(), x_dqkv[:, :, 0].float()), f"{tag} dq"
        for m, nm in ((1, "k"), (2, "v")):
            if mfma:
                within_twice("d" + nm, p_dqkv[:, Lp:, m], x_dqkv[:, :, m], N)
                within_twice("dp" + nm, p_dqkv[:, :Lp, m], x_pre[m], Lp)
            else:
                assert torch.equal(p_dqkv[:, Lp:, m].float(), x_dqkv[:, :, m].float()), f"{tag} d{nm}"
                assert torch.equal(p_dqkv[:, :Lp, m].float(), x_pre[m].to(TD[dt]).float()), f"{tag} dp{nm}"
