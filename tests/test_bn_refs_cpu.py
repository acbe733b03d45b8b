"""The authority of tests/bn_refs.py: every closed form there against torch autograd in fp64 (F.batch_norm, F.relu, the residual add,
F.avg_pool2d, mean(dim) and their backward) within 1e-12 relative; the mask rule and the M = 1 rule stated; for every case of the GPU matrix
the share of ReLU-ambiguous elements under the cap and the bound tensors finite and non-negative; and the comparison helper shown to fail on
one storage ulp in one channel and on a relative 1e-4 in one channel sum."""
import pytest
import torch
import torch.nn.functional as F

import bn_refs as R

REL = 1e-12


def close(a, b, scale=None):
    """max |a - b| <= 1e-12 max |b| (or of `scale`, the magnitude of the terms, where b is a difference that cancels)"""
    a, b = a.double(), b.double()
    return float((a - b).detach().abs().max()) <= REL * max(float((b if scale is None else scale).detach().abs().max()), 1e-300)


def _rand64(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,C", [(2, 8), (75, 24), (300, 16)])
def test_train_forward_and_backward_against_autograd(M, C, relu, res):
    z = (_rand64((M, C), 1, 2.0) + 0.3).requires_grad_(True)
    r = _rand64((M, C), 2).requires_grad_(True)
    gamma, beta = (_rand64((C,), 3, 0.5) + 1.0).requires_grad_(True), _rand64((C,), 4, 0.2).requires_grad_(True)
    rm0, rv0 = _rand64((C,), 5, 0.1), _rand64((C,), 6).abs() + 0.5
    dy = _rand64((M, C), 7)
    rm, rv = rm0.clone(), rv0.clone()
    y = F.batch_norm(z.reshape(M, C, 1, 1), rm, rv, gamma, beta, True, R.MOM, R.EPS).reshape(M, C)
    if res:
        y = y + r
    ypre = y.detach().clone()
    if relu:
        y = F.relu(y)
    y.backward(dy)
    # the formulas, from the two sums
    zd = z.detach()
    mean, var, invstd = R.stats_from_sums(zd.sum(0), (zd * zd).sum(0), M)
    mine = R.bn_fwd(zd, mean, invstd, gamma.detach(), beta.detach(), r.detach() if res else None)
    assert close(mine, ypre)
    assert close(R.running_update(rm0, mean), rm)
    assert close(R.running_update(rv0, var * R.unbias_factor(M)), rv)
    mask = R.relu_mask(mine) if relu else None
    s1, s2, a1, a2 = R.bn_bwd_sums(dy, zd, mean, invstd, mask)
    dz, g = R.bn_bwd_dz(dy, zd, mean, invstd, gamma.detach(), s1, s2, M, mask)
    assert close(s1, beta.grad) and close(s2, gamma.grad)
    assert close(dz, z.grad, scale=gamma.detach() * invstd * dy)          # at M = 2 dz cancels to ~1e-5 of its terms
    if res:
        assert close(g, r.grad)
    assert bool((a1 >= s1.abs() - 1e-12).all()) and bool((a2 >= s2.abs() - 1e-12).all())


def test_mask_rule_and_m1_rule():
    # the mask: strictly positive pre-ReLU values pass the gradient, 0 does not -- F.relu's own rule
    v = torch.tensor([-1.0, -0.0, 0.0, 1e-300, 2.0], dtype=torch.float64, requires_grad=True)
    F.relu(v).sum().backward()
    assert torch.equal(R.relu_mask(v.detach()), v.grad > 0)
    assert R.relu_mask(torch.tensor([0.0]))[0].item() is False
    # M = 1: torch refuses to train BatchNorm on one value per channel; the project's rule is unbias = 1, var = 0, invstd = 1 / sqrt(eps)
    assert R.unbias_factor(1) == 1.0 and R.unbias_factor(2) == 2.0 and R.unbias_factor(101) == 101 / 100
    z = _rand64((1, 8), 9)
    mean, var, invstd = R.stats_from_sums(z.sum(0), (z * z).sum(0), 1)
    assert torch.equal(mean, z[0]) and float(var.max()) < 1e-15
    assert close(invstd, torch.full((8,), 1.0 / R.EPS ** 0.5, dtype=torch.float64))
    # a negative difference of the sums is clamped
    _, var, invstd = R.stats_from_sums(torch.tensor([300.0 * 7], dtype=torch.float64), torch.tensor([90000.0 * 7 - 1.0], dtype=torch.float64), 7)
    assert float(var) == 0.0 and abs(float(invstd) - 1.0 / R.EPS ** 0.5) < 1e-9


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_eval_against_batch_norm(relu, res):
    M, C = 40, 24
    z, r = _rand64((M, C), 11, 2.0), _rand64((M, C), 12)
    gamma, beta = _rand64((C,), 13, 0.5) + 1.0, _rand64((C,), 14, 0.2)
    rm, rv = _rand64((C,), 15, 0.3), _rand64((C,), 16).abs() + 0.2
    want = F.batch_norm(z.reshape(M, C, 1, 1), rm, rv, gamma, beta, False, R.MOM, R.EPS).reshape(M, C)
    want = want + r if res else want
    want = F.relu(want) if relu else want
    scale, shift = R.eval_affine(gamma, beta, rm, rv)
    mine = z * scale + shift
    mine = mine + r if res else mine
    assert close(mine.clamp_min(0) if relu else mine, want)
    assert close(R.bn_fwd(z, rm, 1.0 / torch.sqrt(rv + R.EPS), gamma, beta, r if res else None), want if not relu else mine)


@pytest.mark.parametrize("N,H,W,C,win", [(2, 17, 18, 8, 8), (3, 16, 24, 16, 8), (2, 5, 5, 8, 1), (2, 6, 6, 8, 6), (1, 9, 7, 3, 2)])
def test_pools_against_torch(N, H, W, C, win):
    a = _rand64((N, H, W, C), 20).requires_grad_(True)
    nchw = a.permute(0, 3, 1, 2)
    # global
    df = _rand64((N, C), 21)
    feat = nchw.mean(dim=(2, 3))
    assert close(R.avgpool_fwd(a.detach().reshape(N, H * W, C)), feat)
    (feat * df).sum().backward()
    assert close(R.avgpool_bwd(df, H * W).reshape(N, H, W, C), a.grad)
    # windowed, floor rule, NCHW flatten order
    a.grad = None
    fw = F.avg_pool2d(nchw, win).reshape(N, -1)
    assert close(R.avgpool_win_fwd(a.detach(), win), fw)
    dfw = _rand64(tuple(fw.shape), 22)
    (fw * dfw).sum().backward()
    mine = R.avgpool_win_bwd(dfw, N, H, W, C, win)
    assert close(mine, a.grad)
    Ph, Pw = H // win, W // win
    assert float(mine[:, Ph * win:].abs().sum()) == 0.0 and float(mine[:, :, Pw * win:].abs().sum()) == 0.0


def test_layout_weight_prep_mask_and_stored_sum():
    x = _rand64((2, 3, 4, 5), 30)
    y = R.nchw_to_nhwc(x, 8)
    assert y.shape == (2, 4, 5, 8) and float(y[..., 3:].abs().sum()) == 0.0
    for n in range(2):
        for c in range(3):
            assert torch.equal(y[n, :, :, c], x[n, c])
    assert torch.equal(R.nhwc_to_nchw(y)[:, :3], x)
    w = _rand64((4, 9, 3), 31)
    wf, wd = R.weight_prep(w, 8)
    assert wf.shape == (4, 9, 8) and wd.shape == (8, 9, 4) and float(wf[..., 3:].abs().sum()) == 0.0
    assert all(float(wd[c, t, k]) == float(w[k, t, c]) for k in range(4) for t in range(9) for c in range(3))
    pos = torch.zeros(2, 8, dtype=torch.bool)
    pos[0, 0] = pos[0, 7] = pos[1, 3] = True
    assert R.pack_mask(pos).tolist() == [0x81, 0x08]
    a, b = R.rnd((64,), 32).bfloat16(), R.rnd((64,), 33, 1e-3).bfloat16()
    assert torch.equal(R.add_stored(a, b, "bf16"), (a.float() + b.float()).bfloat16())
    assert torch.equal(R.add_stored(a.float(), b.float(), "f32"), a.float() + b.float())


def _all_cases():
    out = [(M, C, dt, nm) for M, C, nm in R.GEOMS_POW2 + R.GEOMS_NP2 for dt in ("bf16", "f32")]
    return out + [R.GEOM_BIG[:2] + ("bf16", R.GEOM_BIG[2])]


@pytest.mark.parametrize("M,C,dt,name", _all_cases(), ids=lambda v: str(v))
def test_gpu_cases_stay_under_the_ambiguity_cap_and_bounds_are_sane(M, C, dt, name):
    cs = R.case(M, C, dt)
    try:
        assert torch.equal(cs.z.float().to(R.TDT[dt]), cs.z)                         # quantised first
        for res in (False, True):
            n = int(cs.ambiguous(res).sum())
            share = n / (M * C)
            print(f"[ambiguous] {M}x{C} {dt} res={int(res)}: {n} of {M * C} ({share:.2e})")
            # the cap is a share of the case's elements; a case of fewer than 1 / cap elements may hold none
            assert share <= R.AMBIG_CAP
            a, e = 0, min(M, R.ROWS)
            yp = cs.ypre(res)[a:e]
            g, b = cs.gamma.double(), cs.beta.double()
            for kind in ("fp64", "rsqrt", "eval"):
                bd, fp = R.bound_y(yp, cs.z[a:e].double(), cs.mean, cs.invstd, g, b, cs.res[a:e].double() if res else None, dt, kind)
                assert bool(torch.isfinite(bd).all()) and bool((bd > 0).all()) and bool((fp > 0).all())
            for relu in (False, True):
                bw = cs.bwd(res, relu)
                for d in (1, 300):
                    for t in cs.sum_bounds(res, relu, d):
                        assert bool(torch.isfinite(t).all()) and bool((t >= 0).all())
                mu, is_ = cs.mean32.double(), cs.invstd32.double()
                dz, gg = R.bn_bwd_dz(cs.dy[a:e].double(), cs.z[a:e].double(), mu, is_, g, bw["s1"], bw["s2"], M, R.relu_mask(yp) if relu else None)
                bd = R.bound_dz(dz, gg, (cs.z[a:e].double() - mu) * is_, g * is_, bw["s1"] / M, bw["s2"] / M, dt)
                assert bool(torch.isfinite(bd).all()) and bool((bd > 0).all())
        for t in (R.bound_invstd(cs.invstd, cs.var, cs.noise, "rsqrt"), R.bound_mean(cs.mean), R.bound_running(cs.rm0.double(), cs.mean),
                  R.bound_running(cs.rv0.double(), cs.var * R.unbias_factor(M), cs.noise)):
            assert bool(torch.isfinite(t).all()) and bool((t >= 0).all())
    finally:
        if M * C > (1 << 22):
            R.drop_case(M, C, dt)


def _channel_off_by(stored, ref, c, ulp):
    """every non-zero element of channel c moved by `ulp` of its own binade, away from the reference (a stored value is already up to half an ulp off)"""
    bad = stored.clone()
    v = bad[:, c]
    away = torch.where(v >= ref[:, c], 1.0, -1.0).double()
    step = ulp * 2.0 ** torch.floor(torch.log2(v.abs().clamp_min(1e-300)))
    bad[:, c] = torch.where(v != 0, v + away * step, v)
    return bad


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_the_bounds_are_not_vacuous(dt):
    """one storage ulp in one channel of y / dz, a relative 1e-4 in one channel sum: the comparison helper must fail; the unperturbed reference passes"""
    M, C = 75, 64
    cs = R.Case(M, C, dt, seed=5)
    # bf16: one storage ulp (2^-7 of the binade).  f32: one ulp is 2 u, inside any bound that counts eight or more roundings of u on terms
    # no smaller than the result, so the f32 perturbation is 64 ulp (2^-17 of the binade, a coefficient wrong by 1e-5)
    ulp = (2.0 ** -7) if dt == "bf16" else (2.0 ** -17)
    for res in (False, True):
        y = cs.y_stored(res, True)
        cs.y_check("selftest", "unperturbed", y, res, True, "rsqrt")
        bad = _channel_off_by(y.double(), cs.ypre(res).clamp_min(0.0), 5, ulp)
        with pytest.raises(AssertionError):
            cs.y_check("selftest", "one ulp", bad, res, True, "rsqrt")
    bw = cs.bwd(True, True)
    mu, is_, g = cs.mean32.double(), cs.invstd32.double(), cs.gamma.double()
    dz, gg = R.bn_bwd_dz(cs.dy.double(), cs.z.double(), mu, is_, g, bw["s1"], bw["s2"], M, R.relu_mask(cs.ypre(True)))
    good = dz.float().to(R.TDT[dt])
    cs.dz_check("selftest", "unperturbed", good, gg.float().to(R.TDT[dt]), True, True, 1)
    bad = _channel_off_by(good.double(), dz, 9, ulp)
    with pytest.raises(AssertionError):
        cs.dz_check("selftest", "one ulp", bad, None, True, True, 0)
    wrong = gg.clone()
    wrong[3, 3] = cs.dy[3, 3].double() if float(gg[3, 3]) == 0.0 else 0.0           # a flipped mask away from 0
    assert not bool(cs.ambiguous(True)[3, 3])
    with pytest.raises(AssertionError):
        cs.dz_check("selftest", "flipped mask", good, wrong.float().to(R.TDT[dt]), True, True, 1)
    # channel sums, at the longest chain of the matrix's mid-sized cases
    d = R.bwd_chain(M, C, 3)
    b1, b2 = cs.sum_bounds(True, True, d)
    for s, b, old in ((bw["s1"], b1, cs.db0.double()), (bw["s2"], b2, cs.dg0.double())):
        bd = R.bound_grad_store(old, s, b)
        R.check("selftest", dt, "sum", (old + s).float(), old + s, bd)
        bad = s.clone()
        c = int(s.abs().argmax())
        bad[c] *= 1 + 1e-4
        with pytest.raises(AssertionError):
            R.check("selftest", dt, "sum 1e-4", old + bad, old + s, bd)
    R.RATIOS.clear()


def test_geometry_helpers():
    # 75 x 64 with 3 workgroups: rpi = 32, one row per thread, narrow: nparts = 2 -> 16 + 2
    assert R.bwd_chain(75, 64, 3) == 1 + 16 + 2
    # 12 x 2048: rpi = 1, wide
    assert R.bwd_chain(12, 2048, 12) == 1 + 1
    assert R.add_stats_chain(1000, 32, 2) == 8 + 64
    assert R.pool_bn_chain(4096, 64) == 4 + 32
