"""tests/stage_ref.py (the two references of the stage-level eval forward, csrc/stage.hip) held to an independent chain and to seeded faults, on the CPU:
  * its fp64 chains equal a chain written with F.conv2d, eval-mode F.batch_norm and F.relu;
  * the exact routing chain is integer-valued, <= 256 in magnitude and not degenerate for every seed, geometry and batch size the GPU file uses;
  * the identity probe's variance gives scale exactly 1 in torch fp32;
  * an emulation of the kernel (bf16 roundings of every pre-BatchNorm value and every activation) stays inside every link's bound;
  * FAULT INJECTION, in the manner of plan_ref.FAULTS: at every convolution position of a 16-convolution run each fault of stage_ref.FAULTS changes the exact chain's
    output bits AND pushes the matching fp64 link's err / bound above 1.  The matching link of a fault at an even position is the first-of-block probe, at an odd
    position the second-of-block probe -- except `res_from_y` from block 2 on, which the second probe cannot see by construction (the probe's Y is relu(X), and X,
    a block output, is non-negative already): there the real-block link is the matching one.  The two residual faults exist at odd positions only.  The real-block
    link is held above 1 for every fault as well.  The smallest ratio seen is printed (profiles/stage_eval.md records it)."""
import pytest
import torch
import torch.nn.functional as F

import bn_refs as B
import stage_ref as SR

GEOM_IDS = [f"C{c}-H{h}" for c, h in SR.GEOMS]
SMALLEST = {}


def _wq(c):
    return c["w"].to(torch.bfloat16).double()


def _independent(x, convs, lo, hi, var=lambda c: c["var"].double()):
    """blocks lo / 2 .. hi / 2 - 1 with torch's own operators, fp64, nothing rounded"""
    X = x.double()
    bn = lambda t, c: F.batch_norm(t, c["mean"].double(), var(c), c["gamma"].double(), c["beta"].double(), False, 0.0, B.EPS)
    for cv in range(lo, hi, 2):
        a, b = convs[cv], convs[cv + 1]
        y = F.relu(bn(F.conv2d(X, _wq(a), padding=1), a))
        X = F.relu(bn(F.conv2d(y, _wq(b), padding=1), b) + X)
    return X


def test_probe_variance_gives_scale_one_in_fp32():
    v = torch.tensor(SR.unit_var(), dtype=torch.float32)
    eps = torch.tensor(1e-5, dtype=torch.float32)
    assert float(eps) == B.EPS and float(v) == SR.unit_var()                     # (an fp32 value: the kernel receives it unchanged)
    assert float(v + eps) == 1.0
    assert float(torch.tensor(1.0) / torch.sqrt(v + eps)) == 1.0
    p = SR.ident(16)
    sc = p["gamma"] * (1.0 / torch.sqrt(p["var"] + eps))
    assert bool((sc == 1.0).all()) and bool((p["beta"] - p["mean"] * sc == 0.0).all())
    assert bool((SR.bf(p["w"]) == p["w"].double()).all())


@pytest.mark.parametrize("geom", SR.GEOMS, ids=GEOM_IDS)
def test_exact_chain_is_integer_bounded_alive_and_equals_an_independent_chain(geom):
    C, H = geom
    for N in (1, 3, 257):
        E = SR.exact_case(C, H, N, SR.EXACT_SEEDS[C])          # (asserts integers, <= 256 and the nonzero share itself)
        assert len(E["outs"]) == 8 and E["share"] >= SR.EXACT_NONZERO
        print(f"[exact] C {C} H {H} N {N}: nonzero share {E['share']:.3f}, max |value| {float(E['outs'][-1].abs().max()):.0f}")
        for c in E["convs"]:
            shift = c["beta"] - c["mean"] * c["gamma"]
            assert set(shift.tolist()) <= {0.0, -1.0, -2.0} and set(c["gamma"].tolist()) <= {1.0, -1.0}
            assert bool(((c["w"] != 0).sum(dim=(1, 2, 3)) == 1).all()) and set(c["w"].unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert set(E["x"].unique().tolist()) == {-1.0, 0.0, 1.0}
        if N == 3:
            one = torch.full((C,), 1.0, dtype=torch.float64) - B.EPS
            ind, X = [], E["x"]
            for k in range(8):
                X = _independent(X, E["convs"], 2 * k, 2 * k + 2, var=lambda c: one)
                ind.append(X)
            for o, i in zip(E["outs"], ind):
                assert float((o - i).abs().max()) < 1e-9 and torch.equal(i.round(), o)
            # the emulation's bf16 roundings change nothing on this chain
            assert torch.equal(SR.run(E["x"], E["convs"], 0, 16, rounded=True, f32sum=True), E["outs"][-1])


@pytest.mark.parametrize("geom", SR.GEOMS, ids=GEOM_IDS)
def test_link_references_equal_an_independent_chain_and_admit_the_emulated_kernel(geom):
    C, H = geom
    Lc = SR.link_case(C, H, 3, SR.LINK_SEEDS[C])
    x, convs = Lc["x"], Lc["convs"]
    for c in convs:                                              # the parameters the issue asks for
        assert bool((c["gamma"] < 0).any()) and int((c["var"] == 0).sum()) == 1 and float(c["var"][c["var"] > 0].min()) >= 0.5
        assert bool(((c["gamma"] == 0) & (c["beta"] < 0)).any()) and bool(((c["gamma"] == 0) & (c["beta"] > 0)).any())
    assert float(x[:, :, 0].abs().max()) > 2.0 and float(x[:, :, :, -1].abs().max()) > 2.0
    full, ind = SR.run(x, convs, 0, 16), _independent(x, convs, 0, 16)
    assert float(((full - ind).abs() / (1e-300 + ind.abs().max())).max()) < 1e-12
    stored = []
    SR.run(x, convs, 0, 16, rounded=True, f32sum=True, keep=stored)
    worst = {}
    for k in range(1, 9):
        xin = x if k == 1 else stored[k - 2]
        for kind in SR.KINDS:
            pc = SR.probe_convs(convs, k, kind)
            ref, bound = SR.link_ref(kind, xin, pc[2 * k - 2], pc[2 * k - 1])
            i2 = _independent(xin, pc, 2 * k - 2, 2 * k)
            assert float((ref - i2).abs().max()) <= 1e-12 * float(i2.abs().max())
            assert float(bound.min()) > 0
            got = SR.run(xin, pc, 2 * k - 2, 2 * k, rounded=True, f32sum=True)
            worst[kind] = max(worst.get(kind, 0.0), SR.ratio(got, ref, bound))
    print(f"[emulated] C {C} H {H}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("geom", SR.GEOMS, ids=GEOM_IDS)
def test_every_fault_at_every_position_breaks_both_oracles(geom):
    C, H = geom
    E = SR.exact_case(C, H, 3, SR.EXACT_SEEDS[C])
    Lc = SR.link_case(C, H, 3, SR.LINK_SEEDS[C])
    x, convs = Lc["x"], Lc["convs"]
    stored = []
    SR.run(x, convs, 0, 16, rounded=True, f32sum=True, keep=stored)
    blind, weak, smallest, sharp = [], [], (float("inf"), None), (float("inf"), None)
    for cv in range(16):
        k = cv // 2 + 1
        for f in SR.FAULTS:
            if f in SR.RES_FAULTS and not cv & 1:
                continue
            ein = E["x"] if k == 1 else E["outs"][k - 2]
            if torch.equal(SR.run(ein, E["convs"], 2 * k - 2, 16, fault=(f, cv), f32sum=True), E["outs"][-1]):
                blind.append((cv, f))
            xin = x if k == 1 else stored[k - 2]
            r = {}
            for kind in ("second" if cv & 1 else "first", "real"):
                got = SR.run(xin, SR.probe_convs(convs, k, kind), 2 * k - 2, 2 * k, fault=(f, cv), rounded=True, f32sum=True)
                r[kind] = SR.judge_link(kind, xin, convs, k, got)
            probe = r["real"] if (f == "res_from_y" and k > 1) else r["second" if cv & 1 else "first"]
            smallest = min(smallest, (probe, (cv, f, "probe")), (r["real"], (cv, f, "real")))
            sharp = min(sharp, (probe, (cv, f)))
            if not (probe > 1.0 and r["real"] > 1.0):
                weak.append((cv, f, r))
    SMALLEST[C] = smallest
    print(f"[fault] C {C} H {H}: smallest err / bound over all faults and positions {smallest[0]:.3g} at {smallest[1]}; over the matching (probe) links alone {sharp[0]:.3g} at {sharp[1]}")
    assert blind == [], f"faults that leave the exact chain's bits unchanged: {blind}"
    assert weak == [], f"faults inside a link's bound: {weak}"


def test_supported_query_admits_exactly_the_three_geometries():
    """the query is host code (no device): bf16, (C, H = W) in stage_ref.GEOMS, nconv even in 2 .. 16 -- and nothing else of a grid around them"""
    from libcontinual_amd import _lib
    L = _lib.lib()
    for C in (8, 16, 32, 64, 128):
        for H in (4, 8, 16, 32, 64):
            for W in (8, 16, 32):
                for nconv in range(-2, 21):
                    for dt in (_lib.BF16, _lib.F32, 2):
                        want = int(dt == _lib.BF16 and H == W and (C, H) in SR.GEOMS and 2 <= nconv <= SR.LMAX and nconv % 2 == 0)
                        assert L.clhip_stage_eval_supported(H, W, C, nconv, dt) == want, (C, H, W, nconv, dt)
