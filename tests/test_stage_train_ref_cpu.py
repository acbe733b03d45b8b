"""tests/stage_train_ref.py held to account on the CPU (no library, no device):
  * its references, fed the tensors of an INDEPENDENT F.conv2d / F.batch_norm fp64 autograd block (nothing rounded), reproduce every one of them to fp64 rounding:
    plain and entry block, dy and dfeat, dx written and accumulated, one block and groups of images;
  * its emulator (the kernel's rounding points) passes its own judge, with the ambiguous share under the cap;
  * every fault of FAULTS, at every table row it can sit at, pushes a link above 1;
  * for every seed and shape tests/test_stage_train_kernels_gpu.py uses, the ambiguous share -- which the reference alone determines -- stays under bn_refs.AMBIG_CAP.
The smallest faulty ratio is printed (profiles/stage_train_links.md records it)."""
import pytest
import torch
import torch.nn.functional as F

import bn_refs as B
import stage_train_ref as SR

# (C, H, N, entry) of the CPU cases: real channel counts and maps, few images
SMALL = [(16, 32, 3, False), (32, 16, 3, False), (64, 8, 5, False), (32, 16, 3, True), (64, 8, 3, True)]
IDS = [f"C{c}-H{h}-N{n}{'-entry' if e else ''}" for c, h, n, e in SMALL]
# the GPU file's batches; its last one is the largest the query reports = the device's compute units, at most 256: 256 on an MI355X (and on every part with more
# units), the other values are the unit counts of other CDNA parts, so that the seed of the largest batch is pre-checked wherever the GPU file may run
GPU_BATCHES = [1, 3, 33, 65, 130, 256, 228, 120, 110, 104, 80]
GPU_KINDS = [(c, h, False) for c, h in SR.GEOMS] + [(32, 16, True), (64, 8, True)]


def bf_rows(case):
    """the case with its weights already bf16 values, so that autograd and the reference see the same operands"""
    case = dict(case)
    case["rows"] = [dict(r, w=SR.bf(r["w"]).float()) for r in case["rows"]]
    return case


def autograd_block(case, use_dfeat, acc):
    """(G, T, O) of the block from torch autograd in fp64: what judge_fwd / judge_bwd must reproduce"""
    rows, entry = case["rows"], case["entry"]
    x = case["x"].double().clone().requires_grad_(True)
    w = [r["w"].double().clone().requires_grad_(True) for r in rows]
    ga = [r["gamma"].double().clone().requires_grad_(True) for r in rows]
    be = [r["beta"].double().clone().requires_grad_(True) for r in rows]
    n, iB = len(rows), len(rows) - 1
    z, y = [None] * n, [None] * n
    bn = lambda i: F.batch_norm(z[i], None, None, ga[i], be[i], True, 0.0, B.EPS)
    z[0] = F.conv2d(x, w[0], stride=rows[0]["s"], padding=rows[0]["p"])
    y[0] = F.relu(bn(0))
    if entry:
        z[1] = F.conv2d(x, w[1], stride=2, padding=0)
        y[1] = bn(1)
    z[iB] = F.conv2d(y[0], w[iB], stride=1, padding=1)
    y[iB] = F.relu(bn(iB) + (y[1] if entry else x))
    feat = y[iB].mean(dim=(2, 3))
    if use_dfeat:
        feat.backward(case["dfeat"].double())
    else:
        y[iB].backward(case["dy"].double())
    G = dict(z=[t.detach() for t in z], y=[t.detach() for t in y], feat=feat.detach(), mean=[], invstd=[], scale=[], shift=[], rm=[], rv=[])
    for i, r in enumerate(rows):
        zi = z[i].detach()
        M = zi.numel() // zi.shape[1]
        mean, var = zi.mean(dim=(0, 2, 3)), zi.var(dim=(0, 2, 3), unbiased=False)
        istd = 1.0 / torch.sqrt(var + B.EPS)
        G["mean"].append(mean), G["invstd"].append(istd), G["scale"].append(r["gamma"].double() * istd)
        G["shift"].append(r["beta"].double() - mean * G["scale"][-1])
        G["rm"].append((1 - B.MOM) * r["rm0"].double() + B.MOM * mean)
        G["rv"].append((1 - B.MOM) * r["rv0"].double() + B.MOM * zi.var(dim=(0, 2, 3), unbiased=True))
    O = dict(dgamma=[r["dg0"].double() + ga[i].grad for i, r in enumerate(rows)], dbeta=[r["db0"].double() + be[i].grad for i, r in enumerate(rows)],
             slab=[t.grad[None] for t in w], dx=x.grad + (case["dx0"].double() if acc else 0.0), dz=None)
    return G, O


@pytest.mark.parametrize("use_dfeat,acc", [(False, False), (True, True)])
@pytest.mark.parametrize("shape", SMALL, ids=IDS)
def test_reference_reproduces_autograd(shape, use_dfeat, acc):
    C, H, N, entry = shape
    case = bf_rows(SR.link_case(C, H, N, SR.case_seed(C, N, entry), entry))
    case["dfeat"] = SR.bf(case["dfeat"] / (H * H)) * (H * H)          # (the judge rounds dfeat / HW to bf16 as the kernel does: values that rounding keeps)
    G, O = autograd_block(case, use_dfeat, acc)
    V = SR.judge_fwd(case["x"], case["rows"], entry, G)
    assert max(V.rel.values()) < 1e-11, {k: v for k, v in V.rel.items() if v >= 1e-11}
    # the unrounded forward of the module is that chain too
    Fm = SR.forward(case["x"], case["rows"], entry, rounded=False)
    for k in ("z", "y", "mean", "invstd", "rm", "rv"):
        for a, b in zip(Fm[k], G[k]):
            assert float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max())), k
    kw = dict(dfeat=case["dfeat"]) if use_dfeat else dict(dy=case["dy"])
    Vb = SR.judge_bwd(case["x"], case["rows"], entry, G, O, dx0=case["dx0"] if acc else None, ipg=N, ipg_entry=N, **kw)
    assert max(Vb.rel.values()) < 1e-10, {k: v for k, v in Vb.rel.items() if v >= 1e-10}
    # ... and block by block: the per-image blocks add up to the same weight gradient
    Oe = SR.emulate_bwd(case["x"], case["rows"], entry, G, dx0=case["dx0"] if acc else None, ipg=1, rounded=False, **kw)
    for a, b in zip(Oe["slab"], O["slab"]):
        assert a.shape[0] == N and float((a.sum(0) - b[0]).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max()))
    assert float((Oe["dx"] - O["dx"]).abs().max()) <= 1e-10 * float(O["dx"].abs().max())


def emulated(case, ipg=1, fault=None, use_dfeat=False, acc=True):
    rows, entry = case["rows"], case["entry"]
    fwd_fault = fault if fault is not None and fault[0] in SR.FWD_FAULTS else None
    Gf = SR.forward(case["x"], rows, entry, fault=fwd_fault)
    T = SR.forward(case["x"], rows, entry)
    kw = dict(dfeat=case["dfeat"]) if use_dfeat else dict(dy=case["dy"])
    dx0 = case["dx0"] if acc else None
    O = SR.emulate_bwd(case["x"], rows, entry, T, dx0=dx0, ipg=ipg, fault=None if fwd_fault else fault, **kw)
    V = SR.judge_fwd(case["x"], rows, entry, Gf)
    SR.judge_bwd(case["x"], rows, entry, T, O, dx0=dx0, ipg=ipg, V=V, **kw)
    return V


@pytest.mark.parametrize("shape", SMALL, ids=IDS)
def test_emulator_passes_its_own_judge(shape):
    C, H, N, entry = shape
    case = SR.link_case(C, H, N, SR.case_seed(C, N, entry), entry)
    for use_dfeat, acc in ((False, True), (True, False)):
        V = emulated(case, use_dfeat=use_dfeat, acc=acc)
        V.check(f"emulator {shape}")
        print(f"[measure] emulator C{C}-H{H}-N{N} entry={int(entry)} worst err/bound {max(V.values()):.3f} ambiguous {max(V.ambig.values()):.2e}")
    for which in ([2] if entry else [1, 2]):
        probe = dict(case, rows=SR.with_identity(case["rows"], which))
        emulated(probe).check(f"emulator {shape} identity {which}")


def positions(fault, case):
    rows = case["rows"]
    n = len(rows)
    if fault in ("res_grad_drop", "res_before_mask", "dx_overwrite"):
        return [0]
    if fault == "tap_mirror":
        return [i for i, r in enumerate(rows) if r["k"] == 3]
    if fault == "entry_parity":
        return [i for i, r in enumerate(rows) if r["s"] == 2]
    if fault == "mask_other":
        return [0, n - 1]
    if fault == "group_last_twice":
        return [0, n - 1] if not case["entry"] else [n - 1]
    return list(range(n))


# (C, H, N, entry, images per weight-gradient block).  The rigorous bound of a sum over an UNSEEN gradient grows with the number of its terms (every term may carry a
# bf16 rounding of its own), so a fault that moves such a sum by 1 / N of itself is seeded at N = 3; the two 18-image cases are the ragged group form (16 + 2).
FAULT_CASES = [(16, 32, 3, False, 1), (32, 16, 3, True, 1), (64, 8, 3, False, 1), (64, 8, 3, True, 1), (64, 8, 18, False, 16), (64, 8, 18, True, 16)]


@pytest.mark.parametrize("fault", SR.FAULTS)
def test_every_fault_breaks_a_link(fault):
    smallest, seen = float("inf"), 0
    for C, H, N, entry, ipg in FAULT_CASES:
        if fault == "entry_parity" and not entry:
            continue
        if (fault == "group_last_twice") != (ipg > 1):
            continue
        case = SR.link_case(C, H, N, SR.case_seed(C, N, entry), entry)
        for pos in positions(fault, case):
            V = emulated(case, ipg=ipg, fault=(fault, pos))
            worst = max(V.values())
            assert worst > 1.0, (fault, pos, (C, H, N, entry), worst)
            smallest, seen = min(smallest, worst), seen + 1
    assert seen > 0
    print(f"[measure] fault {fault}: smallest worst-link ratio over {seen} positions {smallest:.3g}")


@pytest.mark.parametrize("kind", GPU_KINDS, ids=[f"C{c}-H{h}{'-entry' if e else ''}" for c, h, e in GPU_KINDS])
def test_ambiguous_share_of_the_gpu_cases(kind):
    C, H, entry = kind
    for N in GPU_BATCHES:
        case = SR.link_case(C, H, N, SR.case_seed(C, N, entry), entry)
        share = SR.ambiguous_share(case)
        assert share <= B.AMBIG_CAP, (C, H, N, entry, share)
        for which in ([2] if entry else [1, 2]):
            assert SR.ambiguous_share(dict(case, rows=SR.with_identity(case["rows"], which))) <= B.AMBIG_CAP


@pytest.mark.parametrize("shape", [(16, 32, 3, False), (32, 16, 3, True)], ids=["C16-H32-N3", "C32-H16-N3-entry"])
def test_chain_of_two_blocks_with_an_unseen_dy(shape):
    """the plan-level use: the block behind leaves no dx, its (reference, bound) is the dy of the block in front, and the statistics carry a recovery error"""
    C, H, N, entry = shape
    first = SR.link_case(C, H, N, SR.case_seed(C, N, entry), entry, block=0)
    second = SR.link_case(C, H, N, SR.case_seed(C, N, entry), False, block=1)
    T1 = SR.forward(first["x"], first["rows"], entry)
    x2 = T1["y"][-1]
    T2 = SR.forward(x2, second["rows"], False)
    O2 = SR.emulate_bwd(x2, second["rows"], False, T2, dfeat=first["dfeat"])
    O1 = SR.emulate_bwd(first["x"], first["rows"], entry, T1, dy=O2["dx"])
    se = lambda rows: [(1e-7 * torch.ones(C, dtype=torch.float64), 1e-7)] * len(rows)
    V = SR.judge_bwd(x2, second["rows"], False, T2, dict(O2, dx=None), dfeat=first["dfeat"], stat_err=se(second["rows"]), tag="b2:")
    ref, bound = V.dx
    assert float(((O2["dx"] - ref).abs() / bound).max()) <= 1.0
    SR.judge_bwd(first["x"], first["rows"], entry, T1, O1, dy=ref, bdy=bound, stat_err=se(first["rows"]), V=V, tag="b1:")
    V.check(f"chain {shape}")
    # ... and a fault in the block in front still shows behind the unseen dy
    bad = SR.emulate_bwd(first["x"], first["rows"], entry, T1, dy=O2["dx"], fault=("old_dgamma_ignored", 0))
    Vb = SR.judge_bwd(first["x"], first["rows"], entry, T1, bad, dy=ref, bdy=bound)
    assert max(Vb.values()) > 1.0
