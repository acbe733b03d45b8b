"""The authority of tests/plan_ref.py without a GPU: fed the intermediates of an independent fp64 autograd network it reproduces every link to 1e-12 (the
formulas are right); fed a CPU emulator that rounds every stored tensor to bf16 every link stays inside its bound and the ambiguous share under its cap (the
bounds are satisfiable by a correct implementation); and each seeded wiring fault breaks the link it belongs to by a wide margin."""
import pytest
import torch

import bn_refs as B
import plan_ref as PR

_CACHE = {}


def _setup(name, N, seed=None):
    key = (name, N)
    if key not in _CACHE:
        units, pool_win = PR.units_of(name)
        net = PR.build_net(name, "f32")
        hw = PR.NETS[name][1]
        last_hw = net._act_dims(hw, hw)[len(units)]
        feat = units[-1].cout * (last_hw[0] // pool_win) * (last_hw[1] // pool_win) if pool_win else units[-1].cout
        _CACHE[key] = (units, pool_win) + PR.trained_like(units, 1234 + 17 * N + len(units), N, hw, feat)
    return _CACHE[key]


@pytest.mark.parametrize("case", PR.SMALLEST, ids=PR.case_id)
def test_exact_chain(case):
    units, pool_win, x, P, dfeat = _setup(*case)
    D = PR.autograd_chain(units, x, P, dfeat, pool_win)
    V = PR.judge(units, D, "f32", pool_win)
    bad = {k: v for k, v in V.rel.items() if not v <= 1e-12}
    assert not bad, bad
    assert len(V) >= 8 * sum(PR.has_bn(u) for u in units)


@pytest.mark.parametrize("epilogue", [False, True], ids=["sums-of-stored-dy", "sums-before-the-store"])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("case", PR.CASES, ids=PR.case_id)
def test_honest_chain(case, dt, epilogue):
    units, pool_win, x, P, dfeat = _setup(*case)
    D = PR.emulate(units, x, P, dfeat, dt, pool_win, epilogue=epilogue)
    V = PR.judge(units, D, dt, pool_win)
    print(f"[ratio] {PR.case_id(case)} {dt} " + " ".join(f"{k}={v:.3g}" for k, v in sorted(V.worst_by_link().items())) + f" ambig={max(V.ambig.values()):.2g}")
    V.check(PR.case_id(case))
    if case in PR.SMALLEST:                                      # a second pass accumulates onto the first one's gradients
        D2 = PR.emulate(units, x, P, dfeat, dt, pool_win, old=D, epilogue=epilogue)
        PR.judge(units, D2, dt, pool_win).check(PR.case_id(case) + " second pass")


# the link each fault belongs to: (unit -- by a rule of the unit list --, tensor)
def _expect(units, fault):
    first_res = next(i for i, u in enumerate(units) if u.res >= 0)
    first_sc = next(i for i, u in enumerate(units) if u.k == 1)
    return {
        "drop_res": (units[first_res].res - 1, "dy"),
        "dx_overwrite": (None, "dy"),
        "mask_other": (first_res, None),
        "sums_early": (PR.sums_fault(units), "dbeta"),
        # (1 / M of the variance: the fp32 mode sees it in the statistics link itself; in bf16 that link allows 2^-8 of sum z^2 for sums taken before
        #  the store, and the unit's y link -- a function of the recovered variance -- is the one that breaks)
        "biased_var": (1, None),
        "no_shortcut_dgrad": (units[first_sc].src - 1, "dy"),
        "wgrad_from_z": (2, "dw"),
        "wrong_gamma": (2, "y"),
    }[fault]


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("fault", PR.FAULTS)
def test_seeded_fault_is_caught_at_its_link(fault, dt):
    units, pool_win, x, P, dfeat = _setup("cifar14", 5)
    D = PR.emulate(units, x, P, dfeat, dt, pool_win, fault=fault)
    V = PR.judge(units, D, dt, pool_win)
    unit, what = _expect(units, fault)
    hit = {k: v for k, v in V.items() if v > 2.0 and (unit is None or k[0] == unit) and (what is None or k[1] == what)}
    print(f"[fault] {fault} {dt}: " + ", ".join(f"unit {k[0]} {k[1]} {v:.3g}" for k, v in sorted(V.items()) if v > 1.0))
    assert hit, (fault, V.failures())
    with pytest.raises(AssertionError, match=r"unit \d+ \w+"):       # the failure message names the unit and the tensor
        V.check(fault)
    # the second-pass fault: a writer that overwrites the gradient buffer instead of accumulating
    if fault == "drop_res":
        D1 = PR.emulate(units, x, P, dfeat, dt, pool_win)
        D2 = PR.emulate(units, x, P, dfeat, dt, pool_win, old=D1)
        D2["gw"][3] = D2["gw"][3] - D1["gw"][3]
        assert PR.judge(units, D2, dt, pool_win)[(3, "dw")] > 2.0


def test_recovery_bound():
    """running = momentum * new from (0, 0), in fp32, divided by the fp32 momentum in fp64: inside plan_ref.recover's stated error"""
    g = torch.Generator().manual_seed(5)
    for M in (2, 75, 5120):
        mean = (torch.randn(4096, generator=g) * 3).double()
        var = torch.rand(4096, generator=g).double() * 4 + 1e-6
        unb = B.unbias_factor(M)
        mom32 = torch.tensor(0.1, dtype=torch.float32)
        rm = (mom32 * mean.float()).double()                     # the kernel: (1 - m) * 0 + m * (float)new, fp32
        rv = (mom32 * (var * unb).float()).double()
        m2, v2, e_m, e_v = PR.recover(rm, rv, M, torch.zeros_like(var))
        assert bool(((m2 - mean).abs() <= e_m).all()) and bool(((v2 - var).abs() <= e_v).all())
        assert float((e_m / mean.abs()).max()) < 4 * B.U and float((e_v / var).max()) < 4 * B.U
