"""csrc/rp.hip against fp64 torch on the CPU: clhip_rp_project, clhip_rp_gram_accum, clhip_rp_label_sum, clhip_rp_classify.

Shapes are the smallest that reach every path: one element, one ragged tile, exact tiles (32, 64), widths that are no multiple of 4 (98: element loads),
multiples of 4 but not of 32 (100, 144), more than two tiles per side with a ragged last one (272), a K that is no multiple of the K block, a base pointer
that is not 16-byte aligned, and for classify a hidden width beyond one K slice (1040 > 2 * 512).
Bounds are derived (tests/ranpac_ref.py chain_bound): K * 2^-24 * sum |a_i b_i| per element for a K-long fmaf chain, never fitted.  Every test prints
its largest error-to-bound ratio.
"""
import numpy as np
import pytest
import torch

import ranpac_ref as R
from oracle import detrand

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MS, NS, DS, CS = (1, 16, 32, 98, 100, 144, 272), (1, 31, 64, 200), (1, 24, 768), (1, 5, 200)


def _ops():
    from libcontinual_amd import ops
    return ops


def _u(tag, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(detrand.uniform(tag, shape, lo, hi))


def _ratio(got, ref, bound):
    """largest |got - ref| / bound; an element whose bound is 0 (all products exactly 0) must be exact"""
    err = (got.double().cpu() - ref).abs()
    assert bool((err[bound == 0] == 0).all())
    return float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0


def _project_ref(F, W, relu):
    F, W = F.double(), W.double()
    pre = F @ W
    return (pre.clamp(min=0) if relu else pre), torch.from_numpy(R.chain_bound(F.shape[1], (F.abs() @ W.abs()).numpy()))


@pytest.mark.parametrize("relu", [True, False])
def test_project(relu):
    ops, worst = _ops(), 0.0
    shapes = [(n, d, m) for n, d, m in ((1, 1, 1), (31, 24, 16), (64, 24, 32), (200, 768, 98), (31, 1, 100), (200, 24, 144), (64, 768, 272), (200, 24, 272),
                                        (1, 768, 100), (200, 1, 1))]
    assert {s[2] for s in shapes} == set(MS) and {s[0] for s in shapes} == set(NS) and {s[1] for s in shapes} == set(DS)
    for n, d, m in shapes:
        F, W = _u(f"rp/F/{n}/{d}", (n, d)), _u(f"rp/W/{d}/{m}", (d, m))
        ref, bound = _project_ref(F, W, relu)
        got = ops.rp_project(F.to(DEV), W.to(DEV), relu=relu)
        assert got.shape == (n, m) and got.dtype == torch.float32
        r = _ratio(got, ref, bound)          # relu is 1-Lipschitz: the bound of the pre-activation holds behind it
        assert r <= 1.0, (n, d, m, r)
        if relu:
            assert float(got.min()) >= 0.0
        else:
            assert float(got.min()) < 0.0 or n * m < 4
        worst = max(worst, r)
        assert torch.equal(got, ops.rp_project(F.to(DEV), W.to(DEV), relu=relu))        # a repeated run is bit-identical
    print(f"clhip_rp_project relu={relu}: largest error / bound {worst:.4f}")


def test_project_unaligned_base_takes_the_element_path():
    """pitches that are multiples of 4 behind base pointers that are not 16-byte aligned: same bits as the aligned call"""
    ops = _ops()
    n, d, m = 64, 24, 144
    F, W = _u("rp/Fu", (n, d)).to(DEV), _u("rp/Wu", (d, m)).to(DEV)
    Fo, Wo = torch.empty(n * d + 1, device=DEV), torch.empty(d * m + 1, device=DEV)
    Fo[1:].copy_(F.reshape(-1))
    Wo[1:].copy_(W.reshape(-1))
    Fv, Wv = Fo[1:].view(n, d), Wo[1:].view(d, m)
    assert Fv.data_ptr() % 16 == 4 and Wv.data_ptr() % 16 == 4 and Fv.is_contiguous()
    assert torch.equal(ops.rp_project(Fv, Wv), ops.rp_project(F, W))


def test_project_all_negative_is_exactly_zero():
    ops = _ops()
    X, W = _u("rp/Xpos", (31, 24), 0.1, 1.0), _u("rp/Wneg", (24, 272), -1.0, -0.1)
    H = ops.rp_project(X.to(DEV), W.to(DEV), relu=True)
    assert int(torch.count_nonzero(H)) == 0
    Wo = _u("rp/Wo0", (5, 272)).to(DEV)
    assert int(torch.count_nonzero(ops.rp_classify(X.to(DEV), W.to(DEV), Wo))) == 0
    assert float(ops.rp_project(X.to(DEV), W.to(DEV), relu=False).max()) < 0.0


def _gram_ref(H):
    Hd = H.double()
    return Hd.T @ Hd, (Hd.abs().T @ Hd.abs()).numpy()


def test_gram_single_call_symmetric_and_reproducible():
    ops, worst = _ops(), 0.0
    shapes = [(1, 1), (31, 16), (64, 32), (200, 98), (31, 100), (200, 144), (64, 272), (200, 272), (1, 272)]
    assert {s[1] for s in shapes} == set(MS) and {s[0] for s in shapes} == set(NS)
    for n, m in shapes:
        H = _u(f"rp/H/{n}/{m}", (n, m))                   # asymmetric in its columns: a transposed tile cannot pass
        ref, sabs = _gram_ref(H)
        G = ops.rp_gram_accum(H.to(DEV), torch.zeros(m, m, device=DEV))
        r = _ratio(G, ref, torch.from_numpy(R.chain_bound(n, sabs)))
        assert r <= 1.0, (n, m, r)
        assert torch.equal(G, G.T), (n, m)                # bitwise symmetric, diagonal tiles included
        assert torch.equal(G, ops.rp_gram_accum(H.to(DEV), torch.zeros(m, m, device=DEV)))
        worst = max(worst, r)
    print(f"clhip_rp_gram_accum: largest error / bound {worst:.4f}")


@pytest.mark.parametrize("cuts", [(100,), (7, 64)], ids=["two-calls", "three-unequal-chunks"])
def test_gram_accumulates_over_calls(cuts):
    """G accumulated over several calls against the fp64 Gram of all rows and against the single-call result.  Chunked bound: each call's chain rounds
    once per row and every accumulating call after the first adds one rounding of a value bounded by the same sum: (rows + calls - 1) * 2^-24 * sum."""
    ops = _ops()
    n, m = 200, 272
    H = _u("rp/Hacc", (n, m))
    ref, sabs = _gram_ref(H)
    Hd = H.to(DEV)
    G = torch.zeros(m, m, device=DEV)
    edges = (0,) + cuts + (n,)
    for a, b in zip(edges[:-1], edges[1:]):
        ops.rp_gram_accum(Hd[a:b], G)
    bound = torch.from_numpy(R.chain_bound(n, sabs, extra=len(cuts)))
    r = _ratio(G, ref, bound)
    single = ops.rp_gram_accum(Hd, torch.zeros(m, m, device=DEV))
    r2 = float(((G - single).double().abs().cpu() / (bound + torch.from_numpy(R.chain_bound(n, sabs)))).max())
    print(f"clhip_rp_gram_accum over {len(cuts) + 1} calls: error / chunked bound {r:.4f}; against the single call {r2:.4f}")
    assert r <= 1.0 and r2 <= 1.0
    assert torch.equal(G, G.T)


def _label_ref(H, labels, C):
    Y = torch.from_numpy(R.onehot(labels.numpy(), C))
    cnt = Y.sum(0)
    return H.double().T @ Y, torch.from_numpy(R.U32 * (H.double().abs().T @ Y).numpy() * cnt.numpy()[None, :])


def test_label_sum():
    ops, worst = _ops(), 0.0
    shapes = [(1, 1, 1), (31, 16, 5), (64, 32, 200), (200, 98, 5), (31, 100, 1), (200, 144, 200), (64, 272, 5), (200, 272, 200)]
    assert {s[1] for s in shapes} == set(MS) and {s[0] for s in shapes} == set(NS) and {s[2] for s in shapes} == set(CS)
    for n, m, c in shapes:
        H = _u(f"rp/HL/{n}/{m}", (n, m))
        labels = torch.from_numpy(detrand.randint(f"rp/lab/{n}/{c}", (n,), 0, c))
        ref, bound = _label_ref(H, labels, c)
        Q0 = _u(f"rp/Q0/{m}/{c}", (m, c))
        Q = ops.rp_label_sum(H.to(DEV), labels.to(DEV), Q0.clone().to(DEV))
        got = Q.cpu().double() - Q0.double()               # += : one more rounding, of a value bounded by |Q0| + sum
        bound = bound + R.U32 * (Q0.double().abs() + H.double().abs().T @ torch.from_numpy(R.onehot(labels.numpy(), c)))
        r = _ratio(got, ref, bound)
        assert r <= 1.0, (n, m, c, r)
        worst = max(worst, r)
        empty = [k for k in range(c) if not bool((labels == k).any())]
        if c == 200:
            assert empty                                    # empty classes: their columns keep Q0 bit for bit
        assert torch.equal(Q.cpu()[:, empty], Q0[:, empty])
        assert torch.equal(Q, ops.rp_label_sum(H.to(DEV), labels.to(DEV), Q0.clone().to(DEV)))
    print(f"clhip_rp_label_sum: largest error / bound {worst:.4f}")


def test_label_sum_all_rows_one_class():
    ops = _ops()
    n, m, c = 200, 100, 5
    H = _u("rp/Hone", (n, m))
    labels = torch.full((n,), 3, dtype=torch.int64)
    Q = ops.rp_label_sum(H.to(DEV), labels.to(DEV), torch.zeros(m, c, device=DEV)).cpu()
    ref, bound = _label_ref(H, labels, c)
    assert _ratio(Q, ref, bound) <= 1.0
    assert int(torch.count_nonzero(Q[:, [0, 1, 2, 4]])) == 0
    # rows are summed in ascending order: the fp32 running sum over the rows, bit for bit
    run = torch.zeros(m)
    for i in range(n):
        run = run + H[i]
    assert torch.equal(Q[:, 3], run)


@pytest.mark.parametrize("bad", [-1, 5])
def test_label_out_of_range_is_an_argument_error(bad):
    from libcontinual_amd._lib import ClhipError
    ops = _ops()
    H = _u("rp/Hbad", (31, 16)).to(DEV)
    labels = torch.from_numpy(detrand.randint("rp/labbad", (31,), 0, 5))
    labels[17] = bad
    Q = torch.zeros(16, 5, device=DEV)
    with pytest.raises(ClhipError, match="label"):
        ops.rp_label_sum(H, labels.to(DEV), Q)
    assert int(torch.count_nonzero(Q)) == 0                # refused before Q is touched


def test_classify_against_project_then_fp64_product():
    """logits against sigma * (the device's own projection, taken as fp64) @ Wo^T.  K = the hidden width; beyond one K slice (1040) the slice chains and the
    ordered sum of their partials stay inside the same K * 2^-24 * sum |h wo|.  sigma = 1 (the parameter's value, ranpac.py:47) and a power of two scale
    exactly; any other sigma is one more rounding (extra = 1)."""
    ops, worst = _ops(), 0.0
    shapes = [(1, 1, 1, 1), (31, 24, 16, 5), (64, 24, 32, 200), (48, 768, 98, 5), (31, 1, 100, 1), (48, 24, 144, 200), (64, 768, 272, 5), (200, 24, 272, 200),
              (48, 24, 1040, 5)]
    assert {s[2] for s in shapes} >= set(MS) and {s[3] for s in shapes} == set(CS) and {s[1] for s in shapes} == set(DS)
    for b, d, m, c in shapes:
        X, W, Wo = _u(f"rp/X/{b}/{d}", (b, d)), _u(f"rp/Wc/{d}/{m}", (d, m)), _u(f"rp/Wo/{c}/{m}", (c, m))
        Xd, Wd, Wod = X.to(DEV), W.to(DEV), Wo.to(DEV)
        Hd = ops.rp_project(Xd, Wd, relu=True).cpu().double()
        assert float(Hd.max()) > 0.0 or b * m < 4
        base, sabs = Hd @ Wo.double().T, (Hd.abs() @ Wo.double().abs().T).numpy()
        for sigma, extra in ((None, 0), (0.25, 0), (1.7, 1)):
            sg = None if sigma is None else torch.tensor([sigma], device=DEV)
            got = ops.rp_classify(Xd, Wd, Wod, sg)
            s = 1.0 if sigma is None else float(torch.tensor(sigma, dtype=torch.float32))
            r = _ratio(got, s * base, torch.from_numpy(R.chain_bound(m, abs(s) * sabs, extra=extra)))
            assert r <= 1.0, (b, d, m, c, sigma, r)
            worst = max(worst, r)
            assert torch.equal(got, ops.rp_classify(Xd, Wd, Wod, sg))
    print(f"clhip_rp_classify: largest error / bound {worst:.4f}")
