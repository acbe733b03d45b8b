"""The authority of tests/rapf_ref.py, without a device: it reproduces the reference's own RAPF (tests/golden/rapf_tiny.npz) in fp64 to 1e-10, its explicit
gradient agrees with torch autograd on the formula as the reference writes it, an fp32 evaluation of the same formulas stays inside the derived bounds, and
the bounds are not vacuous: three injected faults each exceed them."""
import numpy as np
import torch

import rapf_ref as R


def _inputs(B=7, M=6, Q=10, E=50, C=9, seed=3):
    g = torch.Generator().manual_seed(seed)
    W = torch.eye(E) + 0.05 * torch.randn(E, E, generator=g)
    T = torch.randn(C, E, generator=g).double()
    T = (T / T.norm(dim=1, keepdim=True)).float()
    X = torch.randn(B + M + Q, E, generator=g)
    y = torch.randint(0, C, (B + M,), generator=g)
    pos = torch.randint(0, C, (Q,), generator=g)
    neg = (pos + 1 + torch.randint(0, C - 1, (Q,), generator=g)) % C
    return X, W, T, y, pos, neg, 1.0 / 0.07, B


def test_restatement_reproduces_the_reference_fixture(golden):
    fix = golden("rapf_tiny")
    got = R.run_fixture(fix)
    d = R.deviations(got, fix)
    assert max(d[k] for k in R.FAMILIES + ("txt",)) < 1e-10 and d["preds_equal"] and d["pairs_equal"], d
    assert R.condition_a(fix) == "" and R.condition_b(fix) == "" and R.condition_c(fix, got) == ""
    assert R.check_f32(R.run_fixture(fix, torch.float32), fix) == ""
    assert fix["t1/s0/logits"].shape == (R.BATCH + 2 * 10 * R.BETA, 2 * R.INC) and fix["t1/s0/z"].shape[0] == 2 * 10 * R.BETA + 20 * R.BETA * len(fix["t1/hard_pairs"])


def test_explicit_gradient_agrees_with_autograd_on_the_reference_formula():
    X, W, T, y, pos, neg, scale, B = _inputs()
    T = T.double() / T.double().norm(dim=1, keepdim=True)                 # unit rows to fp64: the second normalisation is the identity to rounding
    ref = R.step_ref(X, W, T, scale, y, pos, neg, B)
    Wg = W.double().clone().requires_grad_(True)
    loss, logits = R.loss_autograd(X.double(), Wg, T, scale, y, pos, neg)               # the edge and text rows normalised a second time, as rapf.py:343-347
    loss.backward()
    assert abs(float(loss.detach() - ref["loss"])) < 1e-12 and float((logits.detach() - ref["logits"]).abs().max()) < 1e-12
    assert float((Wg.grad - ref["dW"]).abs().max()) < 1e-12 * float(ref["dW"].abs().max()) + 1e-15
    assert int((ref["pre"] > 0).sum()) > 0 and int((ref["pre"] < 0).sum()) > 0            # both sides of the hinge took part


def _worst(got, ref, bnd, keys, mask=None):
    w = 0.0
    for k in keys:
        err, b = (got[k].double() - ref[k]).abs(), bnd[k]
        if k == "G" and mask is not None:
            err, b = err[mask], b[mask]
        w = max(w, float((err / b.clamp(min=1e-300)).max()))
    return w


def test_fp32_evaluation_is_inside_the_bounds_and_faults_are_outside():
    X, W, T, y, pos, neg, scale, B = _inputs()
    ref, bnd = R.step_ref(X, W, T, scale, y, pos, neg, B), R.step_bound(X, W, T, scale, y, pos, neg, B)
    decided = torch.cat([torch.ones(len(y), dtype=torch.bool), ~R.undecided_edges(ref, bnd)])
    assert bool(decided.all())
    keys = ("n", "logits", "row_loss", "G", "dW", "loss_c", "loss_h", "loss")
    f32 = R.step_ref(X, W, T, scale, y, pos, neg, B, dtype=torch.float32)
    assert _worst(f32, ref, bnd, keys, decided) <= 1.0
    assert _worst(R.step_ref(X, W, T, scale, y, pos, neg, B, fault="no_proj"), ref, bnd, ("G", "dW")) > 100.0
    assert _worst(R.step_ref(X, W, T, scale, y, pos, neg, B, fault="hinge_sum"), ref, bnd, ("loss_h", "loss", "G", "dW")) > 100.0
    # the draws: fp32 inside, the upper triangle outside
    g = torch.Generator().manual_seed(11)
    E, cls, cnt = 50, [3, 0, 3], [20, 20, 40]
    mean, chol, Z = torch.randn(5, E, generator=g), 0.2 * torch.randn(5, E, E, generator=g), torch.randn(80, E, generator=g)
    want, b = R.draw_ref(mean, chol, Z, cls, cnt), R.draw_bound(mean, chol, Z, cls, cnt)
    assert float(((R.draw_ref(mean, chol, Z, cls, cnt, dtype=torch.float32).double() - want).abs() / b).max()) <= 1.0
    assert float(((R.draw_ref(mean, chol, Z, cls, cnt, upper=True) - want).abs() / b).max()) > 100.0
    assert want.shape == (80, E) and np.isfinite(want.numpy()).all()
