"""The stage-level TRAINING launches (csrc/stage_train.hip + csrc/xch.h) on their own, through clhip_stage_train_fwd / clhip_stage_train_bwd, on a real MI355X:
  * links       one-block launches (nconv = 2; entry block: nconv = 1) at the three geometries and the two entry blocks, batches 1, 3, 33, 65, 130 (the ragged group
                form: 8 groups of 16 images + 2) and the largest the query reports, each judged link by link against tests/stage_train_ref.py: max over ALL elements
                of err / bound <= 1, ambiguous share under bn_refs.AMBIG_CAP.  Variants, all at every batch: the real block (dfeat + feat, dx accumulated), the real block again (dy, dx
                written), conv2 = identity (its z2 must equal the stored a1 bit for bit; the backward's unseen gradient of a1 becomes dz2), conv1 = identity (plain
                blocks; z1 must equal x bit for bit; dx - g2 becomes dz1).  Old dgamma / dbeta / running statistics are non-zero everywhere.  The test supplies every
                input of the backward itself (the fp64 forward rounded to storage), so the backward is judged whatever the forward kernel does.
  * forms       every batch is chosen for the exchange form clhip_stage_train_query reports, and the test asserts that form: one hop; two hops under the default
                switches (C = 64, N = 33); three levels with unevenly filled XCDs (N = 65, 130); two hops through STAGE_XCH3=0 at 65 and 130.  Where the device's XCD
                rule does not hold the three-level assertions are skipped with that reason.
  * composition a run of nconv = 4 and 16 (entry: 3 and 15) at N = 5 and 130 against the chain of one-block launches, each fed the previous one's stored output
                (backward: the previous dx as dy).  stage_train.hip's header puts every rounding point at a store -- a block's output and the gradient of a block's
                input pass through bf16 both in LDS / registers and in memory, statistics are per-convolution exchanges -- and reading the kernels found no value that
                crosses a block boundary unrounded, so EVERY output is held to bit equality: z, y, saved and running statistics, scale / shift, feat, dgamma, dbeta,
                every weight-gradient block, dx.
  * a forward no backward follows (z = NULL, y = NULL): feat and the running statistics bit-identical to the saving forward's.
  * every launch of a case -- one block, a long run, the lean forward -- runs twice with identical bits; ONE exchange buffer per N, zeroed once, serves every launch of this module at that N -- forward, backward, entry,
    plain, all three channel counts, in whatever order the cases run.
  * refusals    CLHIP_EINVAL and canary-filled outputs untouched.
  * status      the exchange buffer's status word is read after every case and must be 0; after a non-zero word or an abnormal end of a launch the module starts no
                further launch: the remaining tests fail at once with that reason.
The packed ReLU mask: the launch accepts mask pointers and never writes them (the backward takes the mask of a block output from y > 0, which the reference does too);
every forward here passes a canary there and asserts it untouched.
In-process; no test provokes a fault: every pointer is valid and sized.  `[measure]` lines (pytest -s): per geometry and link the worst err / bound and the ambiguous
share; profiles/stage_train_links.md holds the table of an MI355X run."""
import ctypes
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import bn_refs as B                        # noqa: E402
import stage_train_ref as SR               # noqa: E402
from libcontinual_amd import _lib          # noqa: E402

DEV = "cuda:0"
EINVAL = -1
Q_MAX, Q_XCH, Q_SLAB, Q_GROUP, Q_FORM = range(5)
KINDS = [(c, h, False) for c, h in SR.GEOMS] + [(32, 16, True), (64, 8, True)]
KIND_IDS = [f"C{c}-H{h}{'-entry' if e else ''}" for c, h, e in KINDS]
BATCHES = [1, 3, 33, 65, 130, "max"]
MEASURE, AMBIG = {}, {}
_STATE = {"dead": None}
_XCH = {}


def L():
    return _lib.lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def guard():
    if _STATE["dead"] is not None:
        pytest.fail(f"no launch after an abnormal end: {_STATE['dead']}", pytrace=False)


def max_batch():
    return int(L().clhip_stage_train_query(Q_MAX, 0, 0))


def xch(N):
    """THE exchange buffer of batch N: zeroed once, reused by every launch at that N"""
    if N not in _XCH:
        _XCH[N] = torch.zeros(int(L().clhip_stage_train_query(Q_XCH, N, 0)), dtype=torch.uint8, device=DEV)
    return _XCH[N]


def status_ok(N, what):
    s = L().clhip_stage_train_status(xch(N).data_ptr())
    if s != 0:
        _STATE["dead"] = f"status word {s} after {what}"
    assert s == 0, _STATE["dead"]


def launch(name, *args):
    """a launch + synchronize; any failure ends the module's launches"""
    guard()
    try:
        _lib.call(name, *args)
        torch.cuda.synchronize()
    except Exception as e:
        _STATE["dead"] = f"{name}: {e}"
        raise


def nhwc(t):
    return t.to(DEV).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


def as_nchw(t):
    return t.double().permute(0, 3, 1, 2)


def f32d(t):
    """a FRESH fp32 device copy (the launches update running statistics and gradients in place)"""
    return t.to(DEV).float().clone().contiguous()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def table(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def prep(r):
    """(w_fwd [K][taps][cin], w_dg [cin][taps][K]) bf16 of a row, through clhip_conv_weight_prep as a plan makes them"""
    K, cin, k = r["w"].shape[0], r["w"].shape[1], r["w"].shape[2]
    master = r["w"].float().permute(0, 2, 3, 1).reshape(K, k * k, cin).contiguous().to(DEV)
    wf = torch.empty(K, k * k, cin, dtype=torch.bfloat16, device=DEV)
    wd = torch.empty(cin, k * k, K, dtype=torch.bfloat16, device=DEV)
    _lib.call("clhip_conv_weight_prep", master.data_ptr(), wf.data_ptr(), wd.data_ptr(), K, k * k, cin, cin, _lib.BF16, st())
    return wf, wd


def nan_like(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def run_fwd(xd, rows, N, H, C, entry, ysel="all", save_z=True, feat=True):
    """one forward launch over `rows` (table order) on xd [N][h][w][c] bf16 -> dict of raw device tensors per row (None where not stored) + feat + mask canary"""
    n = len(rows)
    nconv = n - 2 if entry else n
    ws = [prep(r)[0] for r in rows]
    R = dict(gamma=[f32d(r["gamma"]) for r in rows], beta=[f32d(r["beta"]) for r in rows], rm=[f32d(r["rm0"]) for r in rows], rv=[f32d(r["rv0"]) for r in rows],
             mean=[nan_like((C,), torch.float32) for _ in rows], invstd=[nan_like((C,), torch.float32) for _ in rows], coef=[nan_like((2, C), torch.float32) for _ in rows],
             z=[nan_like((N, H, H, C), torch.bfloat16) if save_z else None for _ in rows],
             y=[nan_like((N, H, H, C), torch.bfloat16) if (ysel == "all" or i in ysel) else None for i in range(n)])
    R["feat"] = nan_like((N, C), torch.float32) if feat else None
    canary = torch.full((N * H * H * C // 8,), 0xA5, dtype=torch.uint8, device=DEV)
    tabs = [table(ws)] + [table(R[k]) for k in ("gamma", "beta", "rm", "rv", "mean", "invstd", "coef", "z", "y")] + [table([canary] * n)]
    launch("clhip_stage_train_fwd", xd.data_ptr(), N, H, H, C, nconv, *tabs, B.MOM, B.EPS, xch(N).data_ptr(), 0, int(entry),
           None if R["feat"] is None else R["feat"].data_ptr(), _lib.BF16, st())
    assert bool((canary == 0xA5).all()), "the forward wrote a packed mask"
    del ws
    return R


def fwd_dict(R):
    """the raw tensors of a forward as stage_train_ref.judge_fwd wants them"""
    d = lambda ts: [None if t is None else t.double() for t in ts]
    return dict(z=[None if t is None else as_nchw(t) for t in R["z"]], y=[None if t is None else as_nchw(t) for t in R["y"]], mean=d(R["mean"]), invstd=d(R["invstd"]),
                scale=[t[0].double() for t in R["coef"]], shift=[t[1].double() for t in R["coef"]], rm=d(R["rm"]), rv=d(R["rv"]),
                feat=None if R["feat"] is None else R["feat"].double())


def run_bwd(xd, rows, N, H, C, entry, T, dy=None, dfeat=None, dx0=None):
    """one backward launch.  T: per row the device tensors the launch READS -- z (bf16 NHWC), y (bf16 NHWC; used at the second convolution of a block), mean,
    invstd (fp32).  dx0: bf16 NHWC content dx is accumulated onto, or None: dx is written.  -> dict of raw device tensors"""
    n = len(rows)
    nconv = n - 2 if entry else n
    wds = [prep(r)[1] for r in rows]
    group = int(L().clhip_stage_train_query(Q_GROUP, N, C)) == 1
    nb = int(L().clhip_stage_train_query(Q_SLAB, N, C))
    assert nb == ((N + 15) // 16 if group else N)
    second = lambda i: (i >= 2 and (i - 2) % 2 == 0) if entry else i % 2 == 1
    strided = lambda i: entry and i < 2
    R = dict(gamma=[f32d(r["gamma"]) for r in rows], beta=[f32d(r["beta"]) for r in rows], dgamma=[f32d(r["dg0"]) for r in rows], dbeta=[f32d(r["db0"]) for r in rows],
             slab=[nan_like((N if strided(i) else nb, r["w"].numel()), torch.float32) for i, r in enumerate(rows)],
             dzg=[nan_like((C // 16, N, H, H, 16), torch.bfloat16) if (group and not strided(i)) else None for i in range(n)])
    R["dx"] = dx0.clone() if dx0 is not None else nan_like(tuple(xd.shape), torch.bfloat16)
    ys = [T["y"][i] if second(i) else None for i in range(n)]
    tabs = [table(wds), table(R["gamma"]), table(R["beta"]), table(T["mean"]), table(T["invstd"]), table(T["z"]), table(ys), table(R["dgamma"]), table(R["dbeta"]),
            table(R["slab"]), table(R["dzg"])]
    launch("clhip_stage_train_bwd", xd.data_ptr(), None if dy is None else dy.data_ptr(), R["dx"].data_ptr(), int(dx0 is not None), N, H, H, C, nconv, *tabs,
           xch(N).data_ptr(), 0, int(entry), None if dfeat is None else dfeat.data_ptr(), _lib.BF16, st())
    R["group"] = group
    del wds
    return R


def bwd_dict(R, rows):
    slabs = []
    for r, s in zip(rows, R["slab"]):
        K, cin, k = r["w"].shape[0], r["w"].shape[1], r["w"].shape[2]
        slabs.append(s.double().reshape(-1, K, k, k, cin).permute(0, 1, 4, 2, 3))
    dz = []
    for t in R["dzg"]:
        if t is None:
            dz.append(None)
        else:
            T16, N, H, W, _ = t.shape
            dz.append(t.double().permute(1, 0, 4, 2, 3).reshape(N, T16 * 16, H, W))
    return dict(dgamma=[t.double() for t in R["dgamma"]], dbeta=[t.double() for t in R["dbeta"]], slab=slabs, dx=as_nchw(R["dx"]), dz=dz)


def same_run(a, b, keys):
    bad = []
    for k in keys:
        va, vb = a[k], b[k]
        for i, (p, q) in enumerate(zip(va, vb) if isinstance(va, list) else [(va, vb)]):
            if (p is None) != (q is None) or (p is not None and not same(p, q)):
                bad.append((k, i))
    return bad


FWD_KEYS = ("z", "y", "mean", "invstd", "coef", "rm", "rv", "feat")
BWD_KEYS = ("dgamma", "dbeta", "slab", "dzg", "dx")


def teacher_dev(T):
    """the fp64 teacher forward (NCHW) as the device tensors a backward launch reads"""
    return dict(z=[nhwc(t) for t in T["z"]], y=[nhwc(t) for t in T["y"]], mean=[f32d(t) for t in T["mean"]], invstd=[f32d(t) for t in T["invstd"]])


def rule_holds():
    """three levels where the arithmetic allows them <=> the device's XCD rule holds (and STAGE_XCH3 is not 0)"""
    return int(L().clhip_stage_train_query(Q_FORM, 256, 64)) == 3


def expected_form(N, C, three):
    """the issue's statement of xch.h: one hop up to 4096 granules (N * 2 C), three levels from 64 workgroups on where the XCD rule holds, two hops otherwise"""
    if N * 2 * C <= 4096:
        return 1
    return 3 if (three and N >= 64) else 2


@pytest.fixture(scope="module", autouse=True)
def measure_table():
    yield
    for name in sorted(MEASURE):
        print(f"\n[measure] {name:34s} worst err/bound {MEASURE[name]:.4f}   ambiguous share {AMBIG.get(name.split(' ')[0], 0.0):.2e}", end="")
    print()
    _XCH.clear()


def test_query_and_exchange_forms():
    guard()
    q = L().clhip_stage_train_query
    mb = max_batch()
    assert 1 <= mb <= 256
    assert q(99, 1, 16) == -1 and q(Q_FORM, 0, 16) == -1 and q(Q_FORM, 3, 48) == -1 and q(Q_SLAB, 3, 48) == -1 and q(Q_GROUP, 3, 48) == -1 and q(Q_GROUP, 0, 64) == -1
    assert q(Q_XCH, 1, 0) > 0 and q(Q_XCH, 130, 0) > q(Q_XCH, 65, 0)
    assert [q(Q_GROUP, n, 64) for n in (127, 128, 130)] == [0, 1, 1] and q(Q_GROUP, 256, 32) == 0 and q(Q_GROUP, 256, 16) == 0
    assert q(Q_SLAB, 130, 64) == 9 and q(Q_SLAB, 127, 64) == 127 and q(Q_SLAB, 130, 32) == 130
    # one hop, and the natural two-hop window: C = 64, 33 <= N <= 63
    assert [q(Q_FORM, n, 64) for n in (1, 32, 33, 63)] == [1, 1, 2, 2]
    assert [q(Q_FORM, n, 32) for n in (3, 64)] == [1, 1] and [q(Q_FORM, n, 16) for n in (65, 128)] == [1, 1]
    big = [(64, 65), (64, 130), (32, 65), (32, 130), (16, 130)]
    assert L().clhip_config(b"STAGE_XCH3", b"0") == 0
    try:
        assert [q(Q_FORM, n, c) for c, n in big] == [2] * len(big)
    finally:
        assert L().clhip_config(b"STAGE_XCH3", None) == 0
    if not rule_holds():
        pytest.skip("this device does not place workgroup w on the XCD of workgroup w % 8: the three-level exchange is never taken")
    assert [q(Q_FORM, n, c) for c, n in big] == [3] * len(big)


def judge_case(kind, N, variants, tagx=""):
    """the links of one (geometry, batch): every variant forward + backward, twice each"""
    C, H, entry = kind
    t0 = time.time()
    form = int(L().clhip_stage_train_query(Q_FORM, N, C))
    case = SR.to_dev(SR.link_case(C, H, N, SR.case_seed(C, N, entry), entry), DEV)
    xd = nhwc(case["x"])
    name = f"C{C}-H{H}{'-entry' if entry else ''}"
    V = SR.Verdict()
    for vname, ident, use_dfeat, acc in variants:
        rows = case["rows"] if ident == 0 else SR.with_identity(case["rows"], ident)
        tag = f"{vname}:"
        iB = len(rows) - 1
        # ---- forward
        Rf = run_fwd(xd, rows, N, H, C, entry, feat=use_dfeat)
        assert same_run(Rf, run_fwd(xd, rows, N, H, C, entry, feat=use_dfeat), FWD_KEYS) == [], "two forwards differ"
        SR.judge_fwd(case["x"], rows, entry, fwd_dict(Rf), V=V, tag=tag)
        if ident == 2:
            assert same(Rf["z"][iB], Rf["y"][0]), "identity conv2: z2 is not the stored a1"
        if ident == 1:
            assert same(Rf["z"][0], xd), "identity conv1: z1 is not x"
        # ---- backward, from the fp64 teacher
        T = SR.forward(case["x"], rows, entry)
        Td = teacher_dev(T)
        kw = dict(dfeat=f32d(case["dfeat"])) if use_dfeat else dict(dy=nhwc(case["dy"]))
        dx0 = nhwc(case["dx0"]) if acc else None
        Rb = run_bwd(xd, rows, N, H, C, entry, Td, dx0=dx0, **kw)
        assert same_run(Rb, run_bwd(xd, rows, N, H, C, entry, Td, dx0=dx0, **kw), BWD_KEYS) == [], "two backwards differ"
        jk = dict(dfeat=case["dfeat"]) if use_dfeat else dict(dy=case["dy"])
        SR.judge_bwd(case["x"], rows, entry, T, bwd_dict(Rb, rows), dx0=case["dx0"] if acc else None, ipg=SR.IPG if Rb["group"] else 1, V=V, tag=tag, **jk)
        status_ok(N, f"{name} N{N} {vname}")
    for (unit, what), r in V.items():
        key = f"{name} {what}"
        MEASURE[key] = max(MEASURE.get(key, 0.0), r)
    AMBIG[name] = max(AMBIG.get(name, 0.0), max(V.ambig.values()))
    print(f"[ratio] stage_train {name} N{N}{tagx} form {form}: " + " ".join(f"{w}={v:.3g}" for w, v in sorted(V.worst_by_link().items()))
          + f" ambiguous {max(V.ambig.values()):.2e}  {time.time() - t0:.1f} s")
    V.check(f"{name} N{N}{tagx}")
    return form


# (name, identity convolution, dfeat + feat instead of dy, dx accumulated)
ALL_VARIANTS = [("real", 0, True, True), ("real", 0, False, False), ("id2", 2, False, True), ("id1", 1, True, False)]


def variants_of(kind, N):
    """every variant at every batch (conv1 = identity exists for plain blocks only): dx written and accumulated, dy and dfeat, feat present and absent and both probes
    are judged on every exchange form and in the group weight-gradient form too"""
    return [x for x in ALL_VARIANTS if not (kind[2] and x[1] == 1)]


@pytest.mark.parametrize("N", BATCHES)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_links_against_fp64(kind, N):
    guard()
    N = max_batch() if N == "max" else N
    three = rule_holds()
    form = judge_case(kind, N, variants_of(kind, N))
    assert form == expected_form(N, kind[0], three), (kind, N, form)


SWITCHED = [(k, n) for k in KINDS for n in (65, 130) if n * 2 * k[0] > 4096]          # (16 channels at 65 images go in one hop: the switch changes nothing there)


@pytest.mark.parametrize("kind,N", SWITCHED, ids=[f"{i}-N{n}" for (k, n), i in zip(SWITCHED, [KIND_IDS[KINDS.index(k)] for k, _ in SWITCHED])])
def test_links_two_hops_by_switch(kind, N):
    """STAGE_XCH3=0: the batches that take three levels by default go in two hops (another fixed summation order, the same bounds)"""
    guard()
    assert L().clhip_config(b"STAGE_XCH3", b"0") == 0
    try:
        assert judge_case(kind, N, variants_of(kind, N), " XCH3=0") == 2
    finally:
        assert L().clhip_config(b"STAGE_XCH3", None) == 0


def run_case(kind, N, nblocks):
    """x and the rows of a run of nblocks blocks (the first one the entry block where kind says so), table order"""
    C, H, entry = kind
    first = SR.link_case(C, H, N, SR.case_seed(C, N, entry), entry, block=0)
    blocks = [first["rows"]] + [SR.link_case(C, H, 1, SR.case_seed(C, N, entry), False, block=b)["rows"] for b in range(1, nblocks)]
    return first, blocks


@pytest.mark.parametrize("nblocks", [2, 8])
@pytest.mark.parametrize("N", [5, 130])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_composition_bit_equal(kind, N, nblocks):
    guard()
    C, H, entry = kind
    # (the launchers take three levels only once the device's XCD probe has run: the query runs it, so the form of this case does not depend on the tests before it)
    assert int(L().clhip_stage_train_query(Q_FORM, N, C)) == expected_form(N, C, rule_holds())
    first, blocks = run_case(kind, N, nblocks)
    rows = [r for b in blocks for r in b]
    xd = nhwc(first["x"])
    off = [0]
    for b in blocks:
        off.append(off[-1] + len(b))
    # ---- forward: the run against the chain of one-block launches
    run = run_fwd(xd, rows, N, H, C, entry)
    assert same_run(run, run_fwd(xd, rows, N, H, C, entry), FWD_KEYS) == [], "two forwards of the run differ"
    inp, bad = xd, []
    for b, brows in enumerate(blocks):
        one = run_fwd(inp, brows, N, H, C, entry and b == 0, feat=(b == nblocks - 1))
        for k in FWD_KEYS[:-1]:
            bad += [(b, k, i) for i in range(len(brows)) if not same(one[k][i], run[k][off[b] + i])]
        inp = one["y"][-1]
    if not same(one["feat"], run["feat"]):
        bad.append((nblocks - 1, "feat", 0))
    assert bad == [], f"forward: (block, tensor, row) that differ from the chain of one-block launches: {bad[:12]}"
    # ---- backward on the run's own stored tensors
    dfeat, dx0 = f32d(first["dfeat"]), nhwc(first["dx0"])
    T = {k: run[k] for k in ("z", "y", "mean", "invstd")}
    runb = run_bwd(xd, rows, N, H, C, entry, T, dfeat=dfeat, dx0=dx0)
    assert same_run(runb, run_bwd(xd, rows, N, H, C, entry, T, dfeat=dfeat, dx0=dx0), BWD_KEYS) == [], "two backwards of the run differ"
    dy = None
    for b in range(nblocks - 1, -1, -1):
        brows = blocks[b]
        Tb = {k: run[k][off[b]:off[b + 1]] for k in T}
        xin = xd if b == 0 else run["y"][off[b] - 1]
        one = run_bwd(xin, brows, N, H, C, entry and b == 0, Tb, dy=dy, dfeat=dfeat if dy is None else None, dx0=dx0 if b == 0 else None)
        for k in BWD_KEYS[:-1]:
            bad += [(b, k, i) for i in range(len(brows)) if (one[k][i] is None) != (runb[k][off[b] + i] is None) or (one[k][i] is not None and not same(one[k][i], runb[k][off[b] + i]))]
        dy = one["dx"]
    if not same(dy, runb["dx"]):
        bad.append((0, "dx", 0))
    assert bad == [], f"backward: (block, tensor, row) that differ from the chain of one-block launches: {bad[:12]}"
    status_ok(N, f"composition {kind} N{N} blocks {nblocks}")
    MEASURE[f"C{C}-H{H}{'-entry' if entry else ''} composition bit-equal"] = 0.0


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_forward_that_no_backward_follows(kind):
    guard()
    C, H, entry = kind
    N = 5
    assert int(L().clhip_stage_train_query(Q_FORM, N, C)) == 1
    first, blocks = run_case(kind, N, 2)
    rows = [r for b in blocks for r in b]
    xd = nhwc(first["x"])
    full = run_fwd(xd, rows, N, H, C, entry)
    lean = run_fwd(xd, rows, N, H, C, entry, ysel=(), save_z=False)
    assert same_run(full, lean, ("feat", "rm", "rv", "mean", "invstd", "coef")) == []
    assert same_run(lean, run_fwd(xd, rows, N, H, C, entry, ysel=(), save_z=False), ("feat", "rm", "rv", "mean", "invstd", "coef")) == [], "two lean forwards differ"
    last = run_fwd(xd, rows, N, H, C, entry, ysel=(len(rows) - 1,), save_z=False, feat=False)          # (the run's output alone: what a later launch of that forward reads)
    assert same(last["y"][-1], full["y"][-1]) and same_run(full, last, ("rm", "rv")) == []
    status_ok(N, f"forward no backward follows {kind}")


# (what, N, H, W, C, nconv, entry, dtype, with an exchange buffer)
def refusals():
    mb = max_batch()
    return [("N = largest + 1", mb + 1, 8, 8, 64, 2, 0, _lib.BF16, True), ("odd nconv", 3, 8, 8, 64, 3, 0, _lib.BF16, True), ("even nconv with entry", 3, 8, 8, 64, 4, 1, _lib.BF16, True),
            ("nconv 18", 3, 8, 8, 64, 18, 0, _lib.BF16, True), ("C = 48", 3, 8, 8, 48, 2, 0, _lib.BF16, True), ("entry at C = 16", 3, 32, 32, 16, 3, 1, _lib.BF16, True),
            ("fp32", 3, 8, 8, 64, 2, 0, _lib.F32, True), ("H != W", 3, 8, 16, 64, 2, 0, _lib.BF16, True), ("null exchange buffer", 3, 8, 8, 64, 2, 0, _lib.BF16, False)]


def test_refusals_leave_the_outputs_untouched():
    guard()
    lib = L()
    mb = max_batch()
    nmax, rows = mb + 1, 20
    # ONE canary per kind of output, shared by all table rows (nothing may be written) and sized for the largest case: 64 x 64 x 8 elements per image cover every
    # (C, H, W) of the list, an entry block's input included
    img = 64 * 64 * 8
    act = torch.full((nmax * img,), 7.5, dtype=torch.bfloat16, device=DEV)
    vec = torch.full((nmax * 64 * 9 * 64,), 7.5, dtype=torch.float32, device=DEV)
    xin = torch.ones(nmax * img, dtype=torch.bfloat16, device=DEV)
    wt = torch.ones(64 * 9 * 64, dtype=torch.bfloat16, device=DEV)
    par = torch.ones(64, dtype=torch.float32, device=DEV)
    act0, vec0 = act.clone(), vec.clone()
    xb = torch.zeros(int(lib.clhip_stage_train_query(Q_XCH, nmax, 0)), dtype=torch.uint8, device=DEV)
    t = lambda buf: table([buf] * rows)
    for what, N, H, W, C, nconv, entry, dt, with_xch in refusals():
        xp = xb.data_ptr() if with_xch else None
        rc = lib.clhip_stage_train_fwd(xin.data_ptr(), N, H, W, C, nconv, t(wt), t(par), t(par), t(vec), t(vec), t(vec), t(vec), t(vec), t(act), t(act), t(act), B.MOM, B.EPS,
                                       xp, 0, entry, vec.data_ptr(), dt, st())
        assert rc == EINVAL and lib.clhip_last_error(), ("forward", what, rc)
        rc = lib.clhip_stage_train_bwd(xin.data_ptr(), xin.data_ptr(), act.data_ptr(), 0, N, H, W, C, nconv, t(wt), t(par), t(par), t(par), t(par), t(xin), t(xin), t(vec), t(vec),
                                       t(vec), t(act), xp, 0, entry, None, dt, st())
        assert rc == EINVAL and lib.clhip_last_error(), ("backward", what, rc)
    torch.cuda.synchronize()
    assert same(act, act0) and same(vec, vec0)
    assert not bool(xb.any()), "a refused launch touched the exchange buffer"
