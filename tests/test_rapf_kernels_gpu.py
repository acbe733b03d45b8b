"""csrc/rapf.hip against the fp64 restatement and the derived per-element bounds of tests/rapf_ref.py: clhip_rapf_draw, clhip_rapf_step_fwd, clhip_rapf_step_bwd.

Step shapes (B, M, Q, E, C): one class (loss, G and dW exactly 0); the task-0 form; replay rows without edge rows; E = 50 (rows not 16-byte aligned, a ragged K
block); R at and one past a tile edge; the workload's own geometry with three hard pairs.  Every call runs on outputs pre-filled with NaN (all outputs are
written), prints `[ratio] name: max |err| / bound`, and is repeated for equal bits.  Edge rows lie on both sides of the hinge; a row whose pre-relu value is
inside its own error band is asserted through the loss only.
"""
import ctypes
import zlib

import pytest
import torch

import rapf_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 0, 0, 32, 1), (9, 0, 0, 32, 3), (5, 4, 0, 48, 7), (7, 6, 10, 50, 9), (128, 0, 0, 64, 5), (100, 20, 9, 64, 5), (100, 40, 120, 512, 100)]
EINVAL = -1


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def _step_inputs(B, M, Q, E, C):
    g = _gen("rapf/step", B, M, Q, E, C)
    W = (torch.eye(E) + 0.05 * torch.randn(E, E, generator=g)).float()
    T = torch.randn(C, E, generator=g).double()
    T = (T / T.norm(dim=1, keepdim=True)).float()
    X = torch.randn(B + M + Q, E, generator=g).float()
    labels = torch.randint(0, C, (B + M,), generator=g)
    labels[0], labels[-1] = 0, C - 1                                   # the first and the last column
    pos = neg = None
    if Q:
        pos = torch.randint(0, C, (Q,), generator=g)
        neg = (pos + 1 + torch.randint(0, C - 1, (Q,), generator=g)) % C
        # edge rows 0, 3, 6, ... are made to map onto their positive text row (A ~ T[pos]: the quiet side of the hinge), rows 1, 4, 7, ... onto their negative
        # one (the active side); rows 2, 5, 8, ... fall where they fall
        for k, src in ((0, pos), (1, neg)):
            tgt = T[src[k::3]].double() + 0.01 * torch.randn(len(src[k::3]), E, generator=g).double()
            X[B + M + k::3] = torch.linalg.solve(W.double(), tgt.T).T.float()
    return X, W, T, labels, pos, neg, 100.0 if E == 512 else 1.0 / 0.07


def _call_fwd(X, W, T, labels, pos, neg, scale, B, margin=R.MARGIN):
    """clhip_rapf_step_fwd on NaN pre-filled outputs"""
    from libcontinual_amd import _lib
    (Rr, E), C = X.shape, T.shape[0]
    nce = Rr if labels is None else labels.numel()
    Q = Rr - nce
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    o = dict(logits=nan(nce, C), n=nan(Rr, E))
    if labels is not None:
        o.update(G=nan(Rr, E), row_loss=nan(Rr), loss=nan(3), pred=torch.full((B,), -7, dtype=torch.int64, device=DEV),
                 correct=torch.full((1,), -7, dtype=torch.int32, device=DEV))
    p = lambda k: o[k].data_ptr() if k in o else None
    q = lambda t: None if t is None else t.data_ptr()
    _lib.call("clhip_rapf_step_fwd", X.data_ptr(), W.data_ptr(), T.data_ptr(), q(labels), q(pos), q(neg), scale, margin, p("logits"), p("n"), p("G"), p("row_loss"),
              p("loss"), p("pred"), p("correct"), B if labels is not None else Rr, nce - B if labels is not None else 0, Q, E, C, _st())
    return o


def _ratio(name, got, ref, bound, mask=None):
    err = (got.double().cpu() - ref).abs()
    bound = bound.expand_as(err) if bound.dim() else bound
    if mask is not None:
        err, bound = err[mask], bound[mask]
    assert bool(torch.isfinite(err).all()), name
    if err.numel() == 0:
        return 0.0
    assert bool((err[bound == 0] == 0).all()), name
    r = float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0
    print(f"[ratio] {name}: {r:.4f}")
    return r


def _check_step(shape, margin=R.MARGIN, zero_pair=False):
    from libcontinual_amd import _lib
    B, M, Q, E, C = shape
    X, W, T, labels, pos, neg, scale = _step_inputs(*shape)
    if zero_pair:
        neg[2] = pos[2]                                                # (row 2 is one of the rows that fall where they fall)
    ref = R.step_ref(X, W, T, scale, labels, pos, neg, B, margin)
    bnd = R.step_bound(X, W, T, scale, labels, pos, neg, B, margin)
    dv = lambda t: None if t is None else t.to(DEV)
    Xd, Wd, Td, ld, pd, nd = dv(X), dv(W), dv(T), dv(labels), dv(pos), dv(neg)
    o = _call_fwd(Xd, Wd, Td, ld, pd, nd, scale, B, margin)
    tag = f"step{shape}"
    nce = B + M
    worst = max(_ratio(f"{tag} n", o["n"], ref["n"], bnd["n"]), _ratio(f"{tag} logits", o["logits"], ref["logits"], bnd["logits"]),
                _ratio(f"{tag} loss_c", o["loss"][1], ref["loss_c"], bnd["loss_c"]))
    und = R.undecided_edges(ref, bnd) if Q else torch.zeros(0, dtype=torch.bool)
    rows_ok = torch.cat([torch.ones(nce, dtype=torch.bool), ~und])
    worst = max(worst, _ratio(f"{tag} row_loss", o["row_loss"], ref["row_loss"], bnd["row_loss"]),          # (relu is 1-Lipschitz: valid inside the band too)
                _ratio(f"{tag} G", o["G"], ref["G"], bnd["G"], rows_ok[:, None].expand(-1, E)))
    if Q:
        on = ref["pre"] > bnd["pre"]
        off = ref["pre"] < -bnd["pre"]
        if not zero_pair:
            assert int(on.sum()) >= 2 and int(off.sum()) >= 2, "edge rows on both sides of the hinge"
        assert bool((o["row_loss"][nce:].cpu()[off] == 0).all()) and bool((o["G"][nce:].cpu()[off] == 0).all())
        worst = max(worst, _ratio(f"{tag} loss_h", o["loss"][2], ref["loss_h"], bnd["loss_h"]))
        assert float(o["loss"][0]) == float(o["loss"][1] + o["loss"][2])
    else:
        assert float(o["loss"][2]) == 0.0 and float(o["loss"][0]) == float(o["loss"][1])
    clear = (R.top2_gap(ref["logits"][:B]) > 2 * bnd["logits"][:B].max(1).values)
    assert bool((o["pred"].cpu()[clear] == ref["pred"][clear]).all())
    if bool(clear.all()):
        assert int(o["correct"]) == ref["correct"]
    assert int(o["correct"]) == int((o["pred"] == ld[:B]).sum())
    # the weight gradient: against the fp64 chain where every edge row is decided, and always against the fp64 product of the kernel's own G
    dW = torch.full((E, E), float("nan"), device=DEV)
    _lib.call("clhip_rapf_step_bwd", o["G"].data_ptr(), Xd.data_ptr(), 1.0, dW.data_ptr(), B + M + Q, E, _st())
    own = o["G"].double().cpu().T @ X.double()
    worst = max(worst, _ratio(f"{tag} dW|G", dW, own, (B + M + Q + 3) * R.U24 * (o["G"].double().cpu().abs().T @ X.double().abs())))
    if not bool(und.any()):
        worst = max(worst, _ratio(f"{tag} dW", dW, ref["dW"], bnd["dW"]))
    assert worst <= 1.0, (shape, worst)
    # a second call: the same bits; g scales dW
    o2 = _call_fwd(Xd, Wd, Td, ld, pd, nd, scale, B, margin)
    for k in o:
        assert torch.equal(o[k], o2[k]), k
    dW2 = torch.full((E, E), float("nan"), device=DEV)
    _lib.call("clhip_rapf_step_bwd", o["G"].data_ptr(), Xd.data_ptr(), 1.0, dW2.data_ptr(), B + M + Q, E, _st())
    assert torch.equal(dW, dW2)
    _lib.call("clhip_rapf_step_bwd", o["G"].data_ptr(), Xd.data_ptr(), -0.5, dW2.data_ptr(), B + M + Q, E, _st())
    assert torch.equal(dW2, -0.5 * dW)                                 # (a power of two: exact)
    # the inference form on the CE rows: the same logits and n, bit for bit, and nothing else
    oi = _call_fwd(Xd[:nce].contiguous(), Wd, Td, None, None, None, scale, nce)
    assert torch.equal(oi["logits"], o["logits"]) and torch.equal(oi["n"], o["n"][:nce])
    return o, ref, (Xd, Wd, Td, ld, pd, nd)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step(shape):
    o, ref, _ = _check_step(shape)
    if shape[4] == 1:                                                  # one class: softmax == onehot
        assert float(o["loss"][0]) == 0.0 and bool((o["G"] == 0).all()) and bool((o["row_loss"] == 0).all())
        from libcontinual_amd import ops
        assert bool((ops.rapf_step_bwd(o["G"], torch.randn(1, shape[3], device=DEV)) == 0).all())


def test_step_hinge_exactly_zero():
    """pos == neg under margin 0: the two dots are the same chain, pre is exactly 0, and relu'(0) = 0 as in torch: no loss term, no gradient"""
    shape = (7, 6, 10, 50, 9)
    o, ref, _ = _check_step(shape, margin=0.0, zero_pair=True)
    nce = shape[0] + shape[1]
    assert float(ref["pre"][2]) == 0.0
    assert float(o["row_loss"][nce + 2]) == 0.0 and bool((o["G"][nce + 2] == 0).all())


def test_step_label_outside_the_columns_follows_ce_slice():
    """a label outside [0, C): no loss term, the softmax part of the gradient only, never correct (clhip_ce_slice's convention)"""
    shape = (9, 0, 0, 32, 3)
    X, W, T, labels, _, _, scale = _step_inputs(*shape)
    labels[2], labels[3] = 3, -1
    ref, bnd = R.step_ref(X, W, T, scale, labels, B=9), R.step_bound(X, W, T, scale, labels, B=9)
    o = _call_fwd(X.to(DEV), W.to(DEV), T.to(DEV), labels.to(DEV), None, None, scale, 9)
    assert float(o["row_loss"][2]) == 0.0 and float(o["row_loss"][3]) == 0.0
    assert max(_ratio("outside G", o["G"], ref["G"], bnd["G"]), _ratio("outside loss", o["loss"][0], ref["loss"], bnd["loss"])) <= 1.0
    assert int(o["correct"]) == int((o["pred"].cpu() == labels).sum())


def test_ops_loss_backward_fills_the_adapter_gradient():
    from libcontinual_amd import ops
    shape = (7, 6, 10, 50, 9)
    X, W, T, labels, pos, neg, scale = _step_inputs(*shape)
    ref, bnd = R.step_ref(X, W, T, scale, labels, pos, neg, 7), R.step_bound(X, W, T, scale, labels, pos, neg, 7)
    Wp = torch.nn.Parameter(W.to(DEV))
    loss, st = ops.rapf_loss(Wp, X.to(DEV), T.to(DEV), scale, labels.to(DEV), pos.to(DEV), neg.to(DEV), 7)
    loss.backward()
    assert st.pred.shape == (7,) and st.logits.shape == (13, 9)
    if not bool(R.undecided_edges(ref, bnd).any()):
        assert max(_ratio("ops dW", Wp.grad, ref["dW"], bnd["dW"]), _ratio("ops loss", loss.detach(), ref["loss"], bnd["loss"])) <= 1.0
    inf = ops.rapf_step_fwd(X[:13].to(DEV), Wp.detach(), T.to(DEV), scale)
    assert torch.equal(inf.logits, st.logits) and inf.G is None


# ------------------------------------------------------------------------------------------------ the draws
def _draw_inputs(E, Cs=5):
    g = _gen("rapf/draw", E)
    mean = torch.randn(Cs, E, generator=g).float()
    chol = torch.tril(0.2 * torch.randn(Cs, E, E, generator=g))
    i = torch.arange(E)
    chol[:, i, i] = 0.5 + chol[:, i, i].abs()
    return mean, chol.float(), g


GROUPS = {"repeat": [(3, 20), (0, 20), (3, 40)], "one": [(2, 7)], "two_row_tiles": [(1, 130), (4, 3)], "two_launches": [(i % 5, 1) for i in range(131)]}


# (the row-tile and launch splits do not depend on E: they run at E = 32 only)
@pytest.mark.parametrize("E,groups", [(E, k) for E in (32, 50, 512) for k in ("repeat", "one")] + [(32, "two_row_tiles"), (32, "two_launches")])
def test_draw(E, groups):
    from libcontinual_amd import ops
    mean, chol, g = _draw_inputs(E)
    cls, cnt = [c for c, _ in GROUPS[groups]], [n for _, n in GROUPS[groups]]
    n, row0 = sum(cnt), 9
    Z = torch.randn(n, E, generator=g).float()
    ref, bnd = R.draw_ref(mean, chol, Z, cls, cnt), R.draw_bound(mean, chol, Z, cls, cnt)
    poisoned = chol.clone()
    iu = torch.triu_indices(E, E, 1)
    poisoned[:, iu[0], iu[1]] = float("nan")                           # the strict upper triangle is never read
    X = torch.full((row0 + n + 3, E), 7.0, device=DEV)
    X[row0:row0 + n] = float("nan")
    ops.rapf_draw(mean.to(DEV), poisoned.to(DEV), Z.to(DEV), X, row0, cls, cnt)
    assert bool((X[:row0] == 7.0).all()) and bool((X[row0 + n:] == 7.0).all())      # the rows around the window are untouched
    r = _ratio(f"draw E={E} {groups}", X[row0:row0 + n], ref, bnd)
    assert r <= 1.0, (E, groups, r)
    X2 = torch.full_like(X, 7.0)
    ops.rapf_draw(mean.to(DEV), chol.to(DEV), Z.to(DEV), X2, row0, cls, cnt)
    assert torch.equal(X, X2)


# ------------------------------------------------------------------------------------------------ refusals: CLHIP_EINVAL before any launch
def test_refusals():
    from libcontinual_amd import _lib
    L = _lib.lib()
    E, C = 32, 3
    mean, chol, g = _draw_inputs(E)
    md, cd = mean.to(DEV), chol.to(DEV)
    Z = torch.randn(8, E, device=DEV)
    X = torch.full((12, E), 7.0, device=DEV)
    arr = lambda v: (ctypes.c_int32 * len(v))(*v)

    def draw(mean=md, chol=cd, Z=Z, Xo=X, cls=(1, 2), cnt=(5, 3), G=2, Cs=5, Ee=E, row0=2):
        p = lambda t: None if t is None else t.data_ptr()
        return L.clhip_rapf_draw(p(mean), p(chol), p(Z), p(Xo), None if cls is None else arr(cls), None if cnt is None else arr(cnt), G, Cs, Ee, row0, _st())

    bad = [dict(mean=None), dict(chol=None), dict(Z=None), dict(Xo=None), dict(cls=None), dict(cnt=None), dict(G=0), dict(Cs=0), dict(Ee=0), dict(row0=-1),
           dict(cls=(1, 5)), dict(cls=(-1, 2)), dict(cnt=(5, 0)), dict(cnt=(-2, 3))]
    for kw in bad:
        assert draw(**kw) == EINVAL, kw
        assert b"invalid argument" in L.clhip_last_error()
    torch.cuda.synchronize()
    assert bool((X == 7.0).all())
    assert draw() == 0

    Xs, W, T, labels, _, _, scale = _step_inputs(9, 0, 0, E, C)
    t = dict(X=Xs.to(DEV), W=W.to(DEV), T=T.to(DEV), labels=labels.to(DEV))
    out = dict(logits=torch.full((9, C), 7.0, device=DEV), n=torch.full((9, E), 7.0, device=DEV), G=torch.full((9, E), 7.0, device=DEV),
               row_loss=torch.full((9,), 7.0, device=DEV), loss=torch.full((3,), 7.0, device=DEV), pred=torch.full((9,), 7, dtype=torch.int64, device=DEV))
    idx = torch.zeros(4, dtype=torch.int64, device=DEV)

    def fwd(B=9, M=0, Q=0, Ee=E, Cc=C, pos=None, neg=None, **null):
        p = lambda k: None if k in null else {**t, **out}[k].data_ptr()
        q = lambda v: None if v is None else v.data_ptr()
        return L.clhip_rapf_step_fwd(p("X"), p("W"), p("T"), p("labels"), q(pos), q(neg), scale, 0.1, p("logits"), p("n"), p("G"), p("row_loss"), p("loss"),
                                     p("pred"), None, B, M, Q, Ee, Cc, _st())

    bad = [dict(X=1), dict(W=1), dict(T=1), dict(logits=1), dict(n=1), dict(G=1), dict(row_loss=1), dict(loss=1), dict(pred=1), dict(B=0), dict(M=-1), dict(Q=-1),
           dict(Ee=0), dict(Cc=0), dict(B=5, Q=4), dict(B=5, Q=4, pos=idx), dict(labels=1, B=5, M=4), dict(labels=1, B=5, Q=4, pos=idx, neg=idx), dict(Ee=4096, Cc=1)]
    for kw in bad:
        assert fwd(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in out.values())
    assert fwd() == 0

    dW = torch.full((E, E), 7.0, device=DEV)
    Gd = out["G"]
    for a in [(None, t["X"], dW, 9, E), (Gd, None, dW, 9, E), (Gd, t["X"], None, 9, E), (Gd, t["X"], dW, 0, E), (Gd, t["X"], dW, 9, 0)]:
        p = lambda v: None if v is None else v.data_ptr()
        assert L.clhip_rapf_step_bwd(p(a[0]), p(a[1]), 1.0, p(a[2]), a[3], a[4], _st()) == EINVAL, a
    torch.cuda.synchronize()
    assert bool((dW == 7.0).all())
