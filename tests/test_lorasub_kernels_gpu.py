"""csrc/lorasub.hip alone on the MI355X against the fp64 restatement of tests/lorasub_ref.py, each result within the fp32 bound derived there (u = 2^-24 per
counted operation on the mass of absolute terms; the bf16 mode of the factor gradients takes its operands as rounded, as tests/test_sdlora_kernels_gpu.py
does).  Each test prints the largest error / bound ratio, which must be <= 1, runs its kernel twice for bitwise equal results, and the refused arguments
must launch nothing.

Inputs of the triplet loss.  A selection (the farthest positive, the nearest negative or prototype) is only comparable between precisions where its best and
second-best candidate are apart, and a hinge where its argument is away from 0: condition (b) asks 1e-3 for both, against a distance error below 3e-4 at
D = 768 (lorasub_ref.atl_bounded).  Independent random rows cannot meet it at B = 128 (two hundred and fifty selections among distances that concentrate
within a few 1e-2), so the rows are placed: unit vectors on a great circle in a random plane of R^D, each class on its own arc with its two end members set
apart from the interior ones, the gaps between arcs growing by 3e-3 rad so that a row's left and right neighbours never tie; random interior positions,
plane, and per-row lengths (the kernel normalises).  Prototype 0 sits inside the first gap (rows next to it take it as their negative), the others leave the
plane by distinct elevations.  The interior positions are drawn until (b) holds, at most 50 times, and no case is left out.  Exact ties exist only between
bitwise equal rows (the duplicated-row case); every precision gives them to the lower index.
test_atl_random_rows runs the small batches once more on independent random rows, drawn until (b) holds.
"""
import ctypes as C
import math

import pytest
import torch

import lorasub_ref as R
from libcontinual_amd import _lib, ops
from libcontinual_amd._lib import call

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U, V = 2.0 ** -24, 2.0 ** -8
DT = {"f32": (_lib.F32, torch.float32, 0.0), "bf16": (_lib.BF16, torch.bfloat16, V)}
CLASSES = {1: 1, 2: 2, 9: 3, 33: 10, 128: 10}


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ratio(got, want, bound):
    err = (got.double().cpu() - want).abs()
    assert torch.isfinite(err).all()
    return float((err / bound.clamp_min(1e-300)).max())


# ----------------------------------------------------------------------------------------------------------------------- clhip_atl
def _counts(B, classes):
    return [B // classes + (1 if c < B % classes else 0) for c in range(classes)]


def _atl_draw(counts, D, P, g, twin=False):
    """rows [B, D], labels [B], prototypes [P, D] or None, placed as the module docstring says; counts: the rows of every class"""
    B, classes = sum(counts), len(counts)
    y = torch.repeat_interleave(torch.arange(classes), torch.tensor(counts))
    width, g0, dlt = 0.2, 0.04, 0.003
    theta, start, first_gap = torch.zeros(B, dtype=torch.float64), 0.0, None
    for c in range(classes):
        n = counts[c]
        t = torch.zeros(n, dtype=torch.float64)
        if n > 1:
            t[-1] = 1.0
            t[1:-1] = 0.2 + 0.25 * torch.rand(n - 2, generator=g, dtype=torch.float64)
        w = width if n > 1 else 0.0
        theta[y == c] = start + w * t
        if first_gap is None:
            first_gap = (start + w, g0)
        start += w + g0 + dlt * c
    assert start < math.pi
    basis, _ = torch.linalg.qr(torch.randn(D, 3, generator=g, dtype=torch.float64))
    u, w_, z = basis[:, 0], basis[:, 1], basis[:, 2]
    rows = torch.cos(theta)[:, None] * u + torch.sin(theta)[:, None] * w_
    rows = rows * (0.5 + 1.5 * torch.rand(B, 1, generator=g, dtype=torch.float64))
    if twin:
        rows[B - 1] = rows[int(torch.nonzero(y == y[B - 1])[0])]                 # the last row repeats the first row of its class, bit for bit
    protos = None
    if P:
        psi = torch.full((P,), float(theta.mean()), dtype=torch.float64)
        alpha = 0.5 + 0.6 * torch.arange(P, dtype=torch.float64) / P
        psi[0], alpha[0] = first_gap[0] + 0.4 * first_gap[1], 0.0
        protos = torch.cos(alpha)[:, None] * (torch.cos(psi)[:, None] * u + torch.sin(psi)[:, None] * w_) + torch.sin(alpha)[:, None] * z
        protos = protos * (0.5 + 1.5 * torch.rand(P, 1, generator=g, dtype=torch.float64))
    return rows.float(), y, None if protos is None else protos.float()


def _atl_case(counts, D, P, margin, weight, seed, twin=False, want_proto=None, want_inactive=False):
    """draw until condition (b) holds in fp64 (at most 50 draws), run clhip_atl twice, -> (ratio of the loss, ratio of df, info, df)"""
    g = torch.Generator().manual_seed(seed)
    B = sum(counts)
    for draw in range(50):
        f, y, pr = _atl_draw(counts, D, P, g, twin)
        loss, df, e_loss, e_df, info = R.atl_bounded(f, y, pr, margin, weight)
        ok = info["gap"] >= R.SEP
        if want_proto:
            ok = ok and any(j >= B for j in info["jn"])
        if want_inactive:
            ok = ok and any(h == 0.0 and j >= 0 for h, j in zip(info["h"], info["jn"])) and any(h > 0.0 for h in info["h"])
        if ok:
            break
    else:
        raise AssertionError(f"no draw met condition (b): B={B} D={D} P={P}")
    fd, yd, pd = f.to(DEV), y.to(DEV), None if pr is None else pr.to(DEV)
    got_loss, got_df = ops.atl(fd, yd, pd, margin, weight, df=torch.full((B, D), float("nan"), device=DEV))
    again_loss, again_df = ops.atl(fd, yd, pd, margin, weight)
    torch.cuda.synchronize()
    assert torch.equal(got_loss, again_loss) and torch.equal(got_df, again_df)                       # bitwise reproducible, and df is written
    r_loss = abs(float(got_loss) - float(loss)) / max(e_loss, 1e-300) if e_loss > 0 else (0.0 if float(got_loss) == float(loss) else math.inf)
    zero = e_df == 0
    assert bool((got_df.cpu()[zero] == 0).all())                                                     # rows nothing reaches: exactly 0
    r_df = _ratio(got_df, df, e_df.clamp_min(1e-300)) if not bool(zero.all()) else 0.0
    print(f"atl B={B} D={D} P={P} margin={margin} draw {draw}: loss {float(got_loss):.6f} (fp64 {float(loss):.6f}), error / bound: loss {r_loss:.3f} df {r_df:.3f}")
    return r_loss, r_df, info, got_df


@pytest.mark.parametrize("P", [0, 1, 7, 90])
@pytest.mark.parametrize("D", [64, 768])
@pytest.mark.parametrize("B", [1, 2, 9, 33, 128])
def test_atl(B, D, P):
    r_loss, r_df, info, _ = _atl_case(_counts(B, CLASSES[B]), D, P, 1.0, 0.05, 1000 + B + D + P, want_proto=P > 0)
    assert r_loss <= 1.0 and r_df <= 1.0
    if P == 0 and CLASSES[B] == 1:
        assert all(h == 0.0 for h in info["h"])


def _random_rows(counts, D, P, g):
    """independent random rows around random class centres, random prototypes: every pair in general position (the placed rows above lie in one plane)"""
    y = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    centres = torch.randn(len(counts), D, generator=g)
    f = centres[y] + 0.7 * torch.randn(len(y), D, generator=g)
    pr = (centres[torch.arange(P) % len(counts)] + 0.9 * torch.randn(P, D, generator=g)) if P else None
    return f, y, pr


@pytest.mark.parametrize("P", [0, 7])
@pytest.mark.parametrize("B,D", [(9, 64), (9, 768), (33, 64)])
def test_atl_random_rows(B, D, P):
    """the small batches once more on rows drawn at random until condition (b) holds (at most 50 draws): the gather on pairs in general position.  (33 rows of
    width 768 are not among them: their distances concentrate, and 50 draws do not reliably separate 66 selections by 1e-3.)"""
    g = torch.Generator().manual_seed(500 + B + D + P)
    counts = _counts(B, CLASSES[B])
    for draw in range(50):
        f, y, pr = _random_rows(counts, D, P, g)
        loss, df, e_loss, e_df, info = R.atl_bounded(f, y, pr, 1.0, 0.05)
        if info["gap"] >= R.SEP:
            break
    else:
        raise AssertionError(f"no draw met condition (b): B={B} D={D} P={P}")
    got_loss, got_df = ops.atl(f.to(DEV), y.to(DEV), None if pr is None else pr.to(DEV), 1.0, 0.05)
    again = ops.atl(f.to(DEV), y.to(DEV), None if pr is None else pr.to(DEV), 1.0, 0.05)
    assert torch.equal(got_loss, again[0]) and torch.equal(got_df, again[1])
    r_loss = abs(float(got_loss) - float(loss)) / e_loss
    r_df = _ratio(got_df, df, e_df.clamp_min(1e-300))
    partners = sum(1 for i, j in enumerate(info["jp"]) if j != i) + sum(1 for j in info["jn"] if 0 <= j < B)
    print(f"atl random rows B={B} D={D} P={P} draw {draw}: {partners} batch partners, {sum(1 for j in info['jn'] if j >= B)} prototype negatives; "
          f"error / bound: loss {r_loss:.3f} df {r_df:.3f}")
    assert r_loss <= 1.0 and r_df <= 1.0 and partners > 0


def test_atl_all_labels_equal_without_prototypes_is_exactly_zero():
    g = torch.Generator().manual_seed(5)
    f, y, _ = _atl_draw([33], 64, 0, g)
    loss, df = ops.atl(f.to(DEV), y.to(DEV), None, 1.0, 0.05, df=torch.full((33, 64), float("nan"), device=DEV))
    assert float(loss) == 0.0 and bool((df == 0).all())


def test_atl_all_labels_distinct_has_no_gradient_through_the_self_pair():
    r_loss, r_df, info, _ = _atl_case([1] * 33, 64, 7, 1.0, 0.05, 77, want_proto=True)
    assert r_loss <= 1.0 and r_df <= 1.0
    assert info["jp"] == list(range(33)) and all(abs(a - 1e-6) < 1e-12 for a in info["ap"])        # ap is the clamped self pair


def test_atl_small_margin_leaves_rows_inactive():
    # single-row classes have ap = 1e-6 and their nearest negative one gap away (0.04 + 0.003 c rad): 0.0535 lies 1.5e-3 from the two gaps around it
    r_loss, r_df, _, _ = _atl_case([3, 1, 1, 3, 1, 1, 3, 1, 1, 3, 1, 1, 1], 768, 7, 0.0535, 0.05, 78, want_inactive=True)
    assert r_loss <= 1.0 and r_df <= 1.0


def test_atl_duplicated_row():
    r_loss, r_df, info, _ = _atl_case(_counts(33, 10), 64, 7, 1.0, 0.05, 79, twin=True)
    assert r_loss <= 1.0 and r_df <= 1.0
    assert float(info["a"][32, 30]) == 0.0 and info["jp"][31] == 30                                  # row 32 repeats row 30; row 31 sees them tie and takes the lower


def test_atl_df_is_scaled_by_weight():
    a = _atl_case([3, 3, 3], 64, 1, 1.0, 1.0, 80)[3]
    b = _atl_case([3, 3, 3], 64, 1, 1.0, 0.25, 80)[3]
    assert torch.equal(a * 0.25, b)                                                                  # a power of two: exact


BAD_ATL = [("B 0", 0, 64, 0), ("B 257", 257, 64, 0), ("P 1025", 4, 64, 1025), ("P -1", 4, 64, -1), ("D 96", 4, 96, 0), ("D 0", 4, 0, 0), ("D 8256", 4, 8256, 0),
           ("P without protos", 4, 64, 3), ("protos without P", 4, 64, 0)]


@pytest.mark.parametrize("what,B,D,P", BAD_ATL, ids=[b[0] for b in BAD_ATL])
def test_atl_refused_arguments_launch_nothing(what, B, D, P):
    L = _lib.lib()
    f = torch.ones(300, 128, device=DEV)
    y = torch.zeros(300, dtype=torch.int64, device=DEV)
    pr = torch.ones(8, 128, device=DEV) if what == "protos without P" or (P > 0 and what != "P without protos") else None
    outs = [torch.full((1,), 7.0, device=DEV), torch.full((300 * 128,), 7.0, device=DEV), torch.full((4096,), 7.0, device=DEV)]
    rc = L.clhip_atl(f.data_ptr(), y.data_ptr(), None if pr is None else pr.data_ptr(), B, D, P, 1.0, 1.0, *[o.data_ptr() for o in outs], _st())
    assert rc != 0 and L.clhip_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)
    assert L.clhip_atl_ws_bytes(0, 0) == 0 and L.clhip_atl_ws_bytes(4, 1025) == 0 and L.clhip_atl_ws_bytes(256, 1024) > 0


# --------------------------------------------------------------------------------------------------------------- clhip_lora_grad_ab
def _q(t, dtype):
    return t.to(DT[dtype][1]).double() if dtype == "bf16" else t.double()


def _grad_ab(D, M, r, dtype):
    g = torch.Generator().manual_seed(11 + D + M + r)
    code, tdt, v = DT[dtype]
    host = [torch.empty(*((r, D) if w % 2 == 0 else (D, r))).uniform_(-0.3, 0.3, generator=g) for w in range(4)]
    X = torch.randn(M, D, generator=g).to(tdt)
    dY = (torch.randn(M, 3 * D, generator=g) * 0.1).to(tdt)
    Xd, dYd, dev = X.to(DEV), dY.to(DEV), [t.to(DEV) for t in host]
    runs = []
    for _ in range(2):
        outs = [torch.full(t.shape, float("nan"), device=DEV) for t in host]                         # written, not accumulated into
        ops.lora_grad_ab(Xd, dYd, *dev, outs=outs)
        runs.append(outs)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*runs))                                              # bitwise reproducible (NaN-free: fully written)
    want, bound = R.grads_ab_bounded(X.double(), dY.double(), host, lambda t: _q(t, dtype), v)
    ref = R.grads_ab(X.double(), dY.double(), *[_q(t, dtype) for t in host])                          # the closed form on the operands as rounded
    assert all(float((a - b).abs().max()) <= 1e-12 * float(b.abs().max() + 1) for a, b in zip(ref, want))
    return max(_ratio(o, w_, b_) for o, w_, b_ in zip(runs[0], want, bound))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("r", [1, 4, 10, 16])
@pytest.mark.parametrize("M", [1, 63, 394])
@pytest.mark.parametrize("D", [64, 768])
def test_lora_grad_ab(D, M, r, dtype):
    worst = _grad_ab(D, M, r, dtype)
    print(f"lora_grad_ab D={D} M={M} rank={r} {dtype}: largest error / bound {worst:.3f}")
    assert worst <= 1.0


def test_lora_grad_ab_two_slabs():
    worst = _grad_ab(64, 1100, 10, "bf16")                                                            # more than one 1024-row slab
    print(f"lora_grad_ab D=64 M=1100 rank=10 bf16: largest error / bound {worst:.3f}")
    assert worst <= 1.0


BAD_GRAD = [("rank 0", 64, 8, 0), ("rank 17", 64, 8, 17), ("D 96", 96, 8, 4), ("M 0", 64, 0, 4), ("dtype 2", 64, 8, 4)]


@pytest.mark.parametrize("what,D,M,r", BAD_GRAD, ids=[b[0] for b in BAD_GRAD])
def test_lora_grad_ab_refused_arguments_launch_nothing(what, D, M, r):
    L = _lib.lib()
    x, dy = torch.zeros(8, 128, device=DEV), torch.zeros(8, 384, device=DEV)
    fac = [torch.zeros(17 * 128, device=DEV) for _ in range(4)]
    outs = [torch.full((17 * 128,), 7.0, device=DEV) for _ in range(4)] + [torch.full((1 << 18,), 7.0, device=DEV)]
    rc = L.clhip_lora_grad_ab(x.data_ptr(), dy.data_ptr(), *[t.data_ptr() for t in fac], *[o.data_ptr() for o in outs], M, D, r,
                              2 if what == "dtype 2" else _lib.F32, _st())
    assert rc != 0 and L.clhip_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)


# ------------------------------------------------------------------------------------------------------------ clhip_proj_adam_multi
HYP = dict(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8)


def _adam_state(depth, D, r, g):
    """[4 * depth] rows (p, g, m, v) on the host, per layer A_k, B_k, A_v, B_v; m and v as some earlier steps left them"""
    rows = []
    for t in range(4 * depth):
        shape = (r, D) if t % 2 == 0 else (D, r)
        rows.append([torch.empty(shape).uniform_(-0.1, 0.1, generator=g), torch.randn(shape, generator=g) * 0.02,
                     torch.randn(shape, generator=g) * 0.01, torch.rand(shape, generator=g) * 1e-4 + 1e-6])
    return rows


def _adam_run(rows, T, D, r, wd, step):
    dev = [[t.to(DEV).clone() for t in row] for row in rows]
    table = ops.proj_adam_table(dev)
    Td = None if T is None else [t.to(DEV) for t in T]
    tt = None if T is None else torch.tensor([t.data_ptr() for t in Td], dtype=torch.int64).to(DEV)
    ws = torch.full((len(rows) * D * r,), float("nan"), device=DEV)
    ops.proj_adam_multi(table, tt, ws, D, r, weight_decay=wd, step=step, **HYP)
    torch.cuda.synchronize()
    return dev


def _adam_plain(rows, wd, step):
    dev = [[t.to(DEV).clone() for t in row] for row in rows]
    for p, g_, m, v in dev:
        ops.adam_step(p, g_, m, v, HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"], wd, 1.0, step)
    torch.cuda.synchronize()
    return dev


def _rand_T(depth, D, g, k=None):
    """T = V V^T / |V V^T|_F of k orthonormal columns, per layer (lora_sub.py:177-179)"""
    out = []
    for l in range(depth):
        Vm, _ = torch.linalg.qr(torch.randn(D, k or max(1, D // 3 + l), generator=g, dtype=torch.float64))
        T = Vm @ Vm.T
        out.append((T / T.norm()).float())
    return out


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("r", [1, 10])
@pytest.mark.parametrize("D", [64, 768])
@pytest.mark.parametrize("depth", [1, 3])
def test_proj_adam_multi(depth, D, r, step, wd):
    g = torch.Generator().manual_seed(3 + depth + D + r + step)
    rows = _adam_state(depth, D, r, g)
    plain = _adam_plain(rows, wd, step)
    # T NULL and T = I: bit for bit clhip_adam_step, moments included
    for T in (None, [torch.eye(D) for _ in range(depth)]):
        got = _adam_run(rows, T, D, r, wd, step)
        assert all(torch.equal(a, b) for ra, rb in zip(got, plain) for a, b in zip(ra, rb)), "identity" if T else "NULL"
    # a projector: against fp64 within the bound, and twice the same bits
    T = _rand_T(depth, D, g)
    got, again = _adam_run(rows, T, D, r, wd, step), _adam_run(rows, T, D, r, wd, step)
    assert all(torch.equal(a, b) for ra, rb in zip(got, again) for a, b in zip(ra, rb))
    worst = 0.0
    for t, (row, out) in enumerate(zip(rows, got)):
        want, m1, v1, bound = R.proj_adam_bounded(*row, T[t // 4], wd=wd, step=step, b1=HYP["beta1"], b2=HYP["beta2"], lr=HYP["lr"], eps=HYP["eps"])
        worst = max(worst, _ratio(out[0], want, bound))
        assert torch.equal(out[2], plain[t][2]) and torch.equal(out[3], plain[t][3]) and torch.equal(out[1], plain[t][1])      # the moments do not see T
    print(f"proj_adam_multi depth={depth} D={D} rank={r} step={step} wd={wd}: largest error / bound {worst:.3f}")
    assert worst <= 1.0


def test_proj_adam_rank_one_transform_spans_every_update():
    D, r, depth = 64, 10, 3
    g = torch.Generator().manual_seed(9)
    rows = _adam_state(depth, D, r, g)
    T = _rand_T(depth, D, g, k=1)
    got = _adam_run(rows, T, D, r, 0.0, 1)
    for t, (row, out) in enumerate(zip(rows, got)):
        vec = T[t // 4].double()[:, 0]
        vec = vec / vec.norm()
        upd = out[0].double().cpu() - row[0].double()
        upd = upd if t % 2 else upd.T                                                                  # B [D, r]: columns; A [r, D]: rows
        resid = upd - vec[:, None] * (vec @ upd)[None, :]
        # each stored p - u carries half an ulp of p (2^-27 below 0.125), and taking the component along vec out spreads the D of them: (1 + sqrt(D)) 2^-27
        assert float(resid.abs().max()) <= (1 + math.sqrt(D)) * 2.0 ** -27 and float(upd.abs().max()) > 1e-6


BAD_ADAM = [("count 0", 0, 64, 4, 1), ("count 6", 6, 64, 4, 1), ("D 48", 4, 48, 4, 1), ("rank 0", 4, 64, 0, 1), ("rank 17", 4, 64, 17, 1), ("step 0", 4, 64, 4, 0),
            ("no workspace", 4, 64, 4, 1)]


@pytest.mark.parametrize("what,count,D,r,step", BAD_ADAM, ids=[b[0] for b in BAD_ADAM])
def test_proj_adam_refused_arguments_launch_nothing(what, count, D, r, step):
    L = _lib.lib()
    rows = [[torch.full((64 * 17,), 7.0, device=DEV) for _ in range(4)] for _ in range(8)]
    table = torch.tensor([[t.data_ptr() for t in row] for row in rows], dtype=torch.int64).to(DEV)
    T = torch.eye(64, device=DEV)
    tt = torch.tensor([T.data_ptr()] * 2, dtype=torch.int64).to(DEV)
    ws = torch.full((8 * 64 * 17,), 7.0, device=DEV)
    rc = L.clhip_proj_adam_multi(count, table.data_ptr(), tt.data_ptr(), None if what == "no workspace" else ws.data_ptr(), D, r, 1e-3, 0.9, 0.999, 1e-8, 0.0,
                                 step, _st())
    assert rc != 0 and L.clhip_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for row in rows for t in row) and bool((ws == 7.0).all())
    with pytest.raises(_lib.ClhipError):
        call("clhip_proj_adam_multi", count, table.data_ptr(), tt.data_ptr(), None if what == "no workspace" else ws.data_ptr(), D, r, 1e-3, 0.9, 0.999, 1e-8,
             0.0, step, _st())
