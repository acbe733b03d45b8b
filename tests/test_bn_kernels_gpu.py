"""Every entry point of csrc/bn.hip -- BatchNorm forward / backward / eval on the partial-buffer and on the fp64-accumulator path, add_stats,
add_inplace, global and windowed average pooling, the layout converts and conv_weight_prep -- in every form its launcher takes, at the sizes where
the launch arithmetic changes (stated in each id), against the fp64 references of tests/bn_refs.py (which tests/test_bn_refs_cpu.py holds to torch
autograd).  Bounds are the derived ones of bn_refs.py, per element or per channel; exact outputs are compared bit for bit.  Every output buffer sits
between two sentinel pads that must come back untouched, and is pre-filled with NaN where the kernel has to write all of it.  Each check prints
`[ratio] entry dtype what: max error / bound`."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from libcontinual_amd import _lib          # noqa: E402
from libcontinual_amd._lib import call     # noqa: E402
import bn_refs as R                        # noqa: E402

DEV = "cuda"
CODE = {"bf16": _lib.BF16, "f32": _lib.F32}
EINVAL = -1
DTS = ["bf16", "f32"]
PAD = 64
FWD_REPS = [1, 2, 3, 5, 16, 63, 64]        # bn_apply_train[_mask]: any count in 1..64
BWD_REPS = [1, 2, 4, 16, 64]               # the backward entries index a replica with blockIdx & (rep - 1)


def st():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    if t is None:
        return None
    return t.t.data_ptr() if isinstance(t, G) else t.data_ptr()


_LIVE = []


def dev(t):
    """upload; the tensor lives until the end of the test (a temporary freed inside an argument list would hand its block to the next upload)"""
    d = t.to(DEV).contiguous()
    _LIVE.append(d)
    return d


@pytest.fixture(autouse=True)
def _release_uploads():
    yield
    _LIVE.clear()


class G:
    """a device buffer between two sentinel pads; `fill` (NaN by default) or `init` in the payload"""

    def __init__(self, shape, dtype=torch.float32, fill=float("nan"), init=None):
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
        n = math.prod(shape)
        self.sent = 0x5A if dtype == torch.uint8 else -1024.0          # exact in every type
        self.full = torch.full((n + 2 * PAD,), self.sent, dtype=dtype, device=DEV)
        self.t = self.full[PAD:PAD + n].view(shape)
        if init is not None:
            self.t.copy_(init.reshape(shape))
        else:
            self.t.fill_(0xEE if dtype == torch.uint8 else fill)
        self.filled = self.t.clone()

    def intact(self):
        return bool((self.full[:PAD] == self.sent).all()) and bool((self.full[-PAD:] == self.sent).all())

    def untouched(self):
        return self.intact() and R.same_bits(self.t, self.filled)

    def cpu(self):
        return self.t.detach().cpu()


def guards_ok(*gs):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                # a device fault: nothing more may run on this GPU from this process
        pytest.exit(f"device error, stopping the run: {e}", returncode=3)
    for g in gs:
        if g is not None:
            assert g.intact(), "a sentinel pad was written"


def geom_id(g):
    return f"{g[0]}x{g[1]}_{g[2]}"


def cases(geoms, big=False):
    out = [pytest.param(M, C, dt, id=f"{geom_id((M, C, nm))}-{dt}") for M, C, nm in geoms for dt in DTS]
    if big:
        M, C, nm = R.GEOM_BIG
        out.append(pytest.param(M, C, "bf16", id=f"{geom_id((M, C, nm))}-bf16"))
    return out


def is_big(M, C):
    return (M, C) == R.GEOM_BIG[:2]


_DEVIN = {}


def devin(cs):
    """the case's activations on the device, uploaded once"""
    key = (cs.M, cs.C, cs.dt)
    if key not in _DEVIN:
        if cs.M * cs.C > (1 << 22):
            _DEVIN.clear()                   # one large case at a time on the device
        _DEVIN[key] = dict(z=dev(cs.z), res=dev(cs.res), dy=dev(cs.dy))
    return _DEVIN[key]


def chan_check(entry, dt, what, got, ref, bound):
    R.check(entry, dt, what, got.cpu() if isinstance(got, G) else got, ref, bound)


def stat_bounds(cs, kind):
    ex = 0.5 * cs.noise / (cs.var + R.EPS)
    return R.bound_mean(cs.mean), R.bound_invstd(cs.invstd, cs.var, cs.noise, kind), ex


def _sum_noise(parts, cs, n):
    """absolute fp64 noise of the variance from summing n given parts [n, 2, C] in fp64, in the kernel and in the reference (and, for a split made
    by the test, from forming the parts): 4 (n + 2) 2^-53 (sum |part of s2| + 2 |mean| sum |part of s1|) / M"""
    a = parts.abs().sum(0)
    return 4 * (n + 2) * R.U64 * (a[1] + 2 * cs.mean.abs() * a[0]) / cs.M


def check_saved_stats(entry, cs, kind, mean, invstd, rm, rv, what):
    bm, bi, _ = stat_bounds(cs, kind)
    chan_check(entry, cs.dt, what + " mean", mean, cs.mean, bm)
    chan_check(entry, cs.dt, what + " invstd", invstd, cs.invstd, bi)
    if rm is not None:
        new_v = cs.var * R.unbias_factor(cs.M)
        chan_check(entry, cs.dt, what + " running_mean", rm, R.running_update(cs.rm0.double(), cs.mean), R.bound_running(cs.rm0.double(), cs.mean))
        chan_check(entry, cs.dt, what + " running_var", rv, R.running_update(cs.rv0.double(), new_v),
                   R.bound_running(cs.rv0.double(), new_v, cs.noise * R.unbias_factor(cs.M)))


# ================================================================================================== size queries
def _py_bwd_blocks(M, C):
    rpi = 256 // (C // 8)
    g = -(-M // rpi)
    iters = min(max(g // 128, 1), 8)
    return max(1, min(-(-g // iters), 1024))


def _py_add_stats_blocks(M, C):
    rpi = 256 // (C // 8)
    return max(1, min(-(-(-(-M // rpi)) // 8), 2048))


def test_size_queries():
    L = _lib.lib()
    for M, C, _ in R.GEOMS_POW2 + R.GEOMS_NP2 + [R.GEOM_BIG]:
        G_ = L.clhip_bn_bwd_blocks(M, C)
        assert G_ == _py_bwd_blocks(M, C), (M, C, G_)
        assert L.clhip_bn_bwd_ws_floats(M, C) == G_ * 2 * C + 2 * C
        if 256 % (C // 8) == 0:
            assert L.clhip_add_stats_blocks(M, C) == _py_add_stats_blocks(M, C), (M, C)
    # the branches the matrix relies on
    assert L.clhip_bn_bwd_blocks(1, 8) == 1
    assert L.clhip_bn_bwd_blocks(81925, 64) == 321             # 2561 row groups, iters = 8, the last trip ragged
    assert L.clhip_bn_bwd_blocks(*R.GEOM_BIG[:2]) == 1024      # 8193 row groups / 8 = 1025, capped
    assert L.clhip_add_stats_blocks(10 ** 7, 64) == 2048


# ================================================================================================== forward: partial-buffer path
@pytest.mark.parametrize("M,C,dt", cases(R.GEOMS_POW2 + R.GEOMS_NP2, big=True))
def test_stats_finalize_and_apply(M, C, dt):
    """clhip_bn_stats_finalize from fp32 partial rows (70 of them where M allows: the second trip of the 64-lane loop), then clhip_bn_apply in
    residual x ReLU.  The reference statistics are those of the partials as given."""
    base = R.case(M, C, dt)
    tiles = min(M, 70)
    part = torch.zeros(tiles, 2, C, dtype=torch.float32)
    for t, zb in enumerate(torch.chunk(base.z, tiles, 0)):
        zb = zb.double()
        part[t, 0], part[t, 1] = zb.sum(0).float(), (zb * zb).sum(0).float()
    cs = copy.copy(base)
    cs.set_sums(part[:, 0].double().sum(0), part[:, 1].double().sum(0))
    cs.noise = cs.noise + _sum_noise(part.double(), cs, tiles)
    d = devin(cs)
    gam, bet = dev(cs.gamma), dev(cs.beta)
    rm, rv = G(C, init=dev(cs.rm0)), G(C, init=dev(cs.rv0))
    mean, invstd, scale, shift = G(C), G(C), G(C), G(C)
    call("clhip_bn_stats_finalize", ptr(dev(part)), tiles, M, C, ptr(gam), ptr(bet), ptr(rm), ptr(rv), R.MOM, R.EPS, ptr(mean), ptr(invstd),
         ptr(scale), ptr(shift), st())
    guards_ok(rm, rv, mean, invstd, scale, shift)
    check_saved_stats("bn_stats_finalize", cs, "fp64", mean, invstd, rm, rv, "")
    _, _, ex = stat_bounds(cs, "fp64")
    sc = cs.gamma.double() * cs.invstd
    msc = (cs.mean * sc).abs()
    # scale = fl(gamma istd): istd 1 + product 1; shift = fl(beta - fl((float)mean sc)): mean 1, sc 2, product 1, subtraction 1 = 5 on both terms
    chan_check("bn_stats_finalize", dt, "scale", scale, sc, sc.abs() * (2 * R.U + ex))
    chan_check("bn_stats_finalize", dt, "shift", shift, cs.beta.double() - cs.mean * sc, 5 * R.U * (cs.beta.double().abs() + msc) + ex * msc)
    forms = [(1, 1)] if is_big(M, C) else [(0, 0), (1, 0), (0, 1), (1, 1)]
    for res, relu in forms:
        y = G((M, C), R.TDT[dt])
        call("clhip_bn_apply", ptr(d["z"]), ptr(scale), ptr(shift), ptr(d["res"]) if res else None, ptr(y), M, C, relu, CODE[dt], st())
        guards_ok(y)
        cs.y_check("bn_apply", f"res={res} relu={relu}", y.t, res, relu, "fp64")


# ================================================================================================== forward: accumulator path
def _apply_train(cs, d, rep, res, relu, mask, with_running=True, seed=100):
    M, C, dt = cs.M, cs.C, cs.dt
    host = cs.split(rep, seed)
    acc = dev(host)
    view = copy.copy(cs)                     # the same case and cache; the fp64 noise of the split added to that of the variance
    view.noise = cs.noise + _sum_noise(host, cs, rep)
    gam, bet = dev(cs.gamma), dev(cs.beta)
    rm = G(C, init=dev(cs.rm0)) if with_running else None
    rv = G(C, init=dev(cs.rv0)) if with_running else None
    mean, invstd = G(C), G(C)
    y = G((M, C), R.TDT[dt])
    bits = G(M * C // 8, torch.uint8) if mask else None
    if mask:
        call("clhip_bn_apply_train_mask", ptr(d["z"]), ptr(acc), rep, M, C, ptr(gam), ptr(bet), ptr(rm), ptr(rv), R.MOM, R.EPS, ptr(mean), ptr(invstd),
             ptr(d["res"]) if res else None, ptr(y), ptr(bits), CODE[dt], st())
    else:
        call("clhip_bn_apply_train", ptr(d["z"]), ptr(acc), rep, M, C, ptr(gam), ptr(bet), ptr(rm), ptr(rv), R.MOM, R.EPS, ptr(mean), ptr(invstd),
             ptr(d["res"]) if res else None, ptr(y), relu, CODE[dt], st())
    guards_ok(rm, rv, mean, invstd, y, bits)
    return dict(y=y, bits=bits, mean=mean, invstd=invstd, rm=rm, rv=rv, view=view)


def assert_ambiguity_cap(cs, res):
    """the either-mask allowance may cover at most 1e-4 of the case's elements; a directed case names the channels it pushes to the edge on purpose
    (`cs.directed`), and the cap then holds over all the others"""
    keep = [c for c in range(cs.C) if c not in getattr(cs, "directed", ())]
    n = int(cs.ambiguous(res)[:, keep].sum())
    assert n <= R.AMBIG_CAP * cs.M * len(keep), (n, cs.M * len(keep))


def _check_apply_train(cs, out, res, relu, what, entry):
    cs = out["view"]
    kind = R.istd_kind("apply_train", cs.dt)
    if relu:
        assert_ambiguity_cap(cs, res)
    check_saved_stats(entry, cs, kind, out["mean"], out["invstd"], out["rm"], out["rv"], what)
    cs.y_check(entry, what, out["y"].t, res, relu, kind)
    if out["bits"] is not None:
        ycpu = out["y"].cpu()
        assert torch.equal(out["bits"].cpu(), R.pack_mask(ycpu.float() > 0)), "packed mask != (stored y > 0)"
        # ... and the stored sign is the true mask wherever the pre-ReLU value is outside the fp32 noise
        wrong = ((ycpu.float() > 0) != R.relu_mask(cs.ypre(res))) & ~cs.ambiguous(res, kind)
        assert not bool(wrong.any()), int(wrong.sum())


@pytest.mark.parametrize("M,C,dt", cases(R.GEOMS_POW2, big=True))
def test_apply_train_every_form(M, C, dt):
    """clhip_bn_apply_train / _mask: residual x ReLU x mask written, the replica count cycling through 1..64 (non powers of two included), sums split
    unevenly; y, the packed mask, the saved and the running statistics"""
    cs = R.case(M, C, dt)
    d = devin(cs)
    forms = [(1, 1, 1), (0, 1, 0)] if is_big(M, C) else [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 1, 1), (1, 1, 1)]
    plain = {}
    for i, (res, relu, mask) in enumerate(forms):
        k = res if relu else 2 + i               # the two ReLU forms of one `res` get the same replica count and split: the same fp64 sums
        rep = FWD_REPS[(k + M) % len(FWD_REPS)]
        out = _apply_train(cs, d, rep, res, relu, mask, seed=100 + k)
        _check_apply_train(cs, out, res, relu, f"res={res} relu={relu} mask={mask} rep={rep}", "bn_apply_train_mask" if mask else "bn_apply_train")
        if relu and not mask:
            plain[res] = out["y"].t.clone()
        if mask and res in plain:
            assert R.same_bits(out["y"].t, plain[res]), "the mask form stores another y than the plain form"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,C", [(75, 64), (12, 2048)], ids=["75x64_narrow_replica_parts", "12x2048_wide_sum_strided"])
@pytest.mark.parametrize("rep", FWD_REPS)
def test_apply_train_replicas(M, C, dt, rep):
    cs = R.case(M, C, dt)
    out = _apply_train(cs, devin(cs), rep, 1, 1, 1, seed=7 + rep)
    _check_apply_train(cs, out, 1, 1, f"rep={rep}", "bn_apply_train_mask")
    out = _apply_train(cs, devin(cs), rep, 0, 0, 0, seed=9 + rep)
    _check_apply_train(cs, out, 0, 0, f"rep={rep}", "bn_apply_train")


# ================================================================================================== eval
def _eval_view(cs):
    ev = copy.copy(cs)
    ev.mean, ev.var = cs.rm0.double(), cs.rv0.double()
    ev.invstd = 1.0 / torch.sqrt(ev.var + R.EPS)
    ev.noise = torch.zeros_like(ev.var)
    ev._cache = {}
    return ev


@pytest.mark.parametrize("M,C,dt", cases(R.GEOMS_POW2 + R.GEOMS_NP2, big=True))
def test_eval_affine_apply_and_one_launch_form(M, C, dt):
    """clhip_bn_eval_affine (+ clhip_bn_apply) and clhip_bn_apply_eval from the running statistics, residual x ReLU"""
    cs = R.case(M, C, dt)
    ev = _eval_view(cs)
    d = devin(cs)
    gam, bet, rm, rv = dev(cs.gamma), dev(cs.beta), dev(cs.rm0), dev(cs.rv0)
    scale, shift = G(C), G(C)
    call("clhip_bn_eval_affine", ptr(gam), ptr(bet), ptr(rm), ptr(rv), R.EPS, C, ptr(scale), ptr(shift), st())
    guards_ok(scale, shift)
    sc, sh = R.eval_affine(cs.gamma.double(), cs.beta.double(), ev.mean, ev.var)
    msc = (ev.mean * sc).abs()
    # scale: istd 2.5 + product 1; shift: sc 3.5, product 1, subtraction 1 on |rm scale|, subtraction 1 on |beta|
    chan_check("bn_eval_affine", dt, "scale", scale, sc, 3.5 * R.U * sc.abs())
    chan_check("bn_eval_affine", dt, "shift", shift, sh, 5.5 * R.U * msc + R.U * cs.beta.double().abs())
    forms = [(1, 1)] if is_big(M, C) else [(0, 0), (1, 0), (0, 1), (1, 1)]
    for res, relu in forms:
        y1, y2 = G((M, C), R.TDT[dt]), G((M, C), R.TDT[dt])
        call("clhip_bn_apply", ptr(d["z"]), ptr(scale), ptr(shift), ptr(d["res"]) if res else None, ptr(y1), M, C, relu, CODE[dt], st())
        call("clhip_bn_apply_eval", ptr(d["z"]), ptr(gam), ptr(bet), ptr(rm), ptr(rv), R.EPS, ptr(d["res"]) if res else None, ptr(y2), M, C, relu,
             CODE[dt], st())
        guards_ok(y1, y2)
        ev.y_check("bn_apply", f"eval res={res} relu={relu}", y1.t, res, relu, "eval")
        ev.y_check("bn_apply_eval", f"res={res} relu={relu}", y2.t, res, relu, "eval")


# ================================================================================================== backward
def _bwd_inputs(cs, res, relu_code):
    """the y argument of a backward form: nothing, the stored y, or the packed mask of the stored y"""
    if relu_code in (0, 2):
        return None
    ys = cs.y_stored(res, True)
    return dev(R.pack_mask(ys.float() > 0)) if relu_code == 3 else dev(ys)


def _check_grads(entry, cs, res, relu, dgamma, dbeta, ds, what):
    b = cs.bwd(res, relu)
    chan_check(entry, cs.dt, what + " dbeta", dbeta, cs.db0.double() + b["s1"], R.bound_grad_store(cs.db0.double(), b["s1"], ds[0]))
    chan_check(entry, cs.dt, what + " dgamma", dgamma, cs.dg0.double() + b["s2"], R.bound_grad_store(cs.dg0.double(), b["s2"], ds[1]))


BWD_FORMS = [(relu, dres) for relu in (0, 1, 3) for dres in (0, 1, 2)] + [(2, 0)]


@pytest.mark.parametrize("M,C,dt", cases(R.GEOMS_POW2 + R.GEOMS_NP2, big=True))
def test_bn_bwd_partial_buffer_path(M, C, dt):
    """clhip_bn_bwd: relu {0, 1} x dres {none, written, accumulated}; dgamma / dbeta start non-zero and get the sums once; two runs agree bit for bit
    (per-workgroup partial rows summed in a fixed order: the deterministic path)"""
    cs = R.case(M, C, dt)
    d = devin(cs)
    G_ = _lib.lib().clhip_bn_bwd_blocks(M, C)
    chain = R.bwd_chain(M, C, G_)
    gam, mu, is_ = dev(cs.gamma), dev(cs.mean32), dev(cs.invstd32)
    forms = [(1, 2), (0, 0)] if is_big(M, C) else [(relu, dres) for relu in (0, 1) for dres in (0, 1, 2)]
    for relu, dres in forms:
        res = dres != 0
        runs = []
        for rerun in range(2 if (relu, dres) == forms[0] else 1):
            yin = _bwd_inputs(cs, res, relu)
            ws = G(_lib.lib().clhip_bn_bwd_ws_floats(M, C))
            dg, db = G(C, init=dev(cs.dg0)), G(C, init=dev(cs.db0))
            dz = G((M, C), R.TDT[dt])
            dr = None if dres == 0 else (G((M, C), R.TDT[dt]) if dres == 1 else G((M, C), R.TDT[dt], init=dev(cs.dres0)))
            call("clhip_bn_bwd", ptr(d["dy"]), ptr(yin), ptr(d["z"]), ptr(mu), ptr(is_), ptr(gam), ptr(dg), ptr(db), ptr(dz), ptr(dr),
                 1 if dres == 2 else 0, M, C, relu, ptr(ws), CODE[dt], st())
            guards_ok(ws, dg, db, dz, dr)
            runs.append((dz, dr, dg, db))
        dz, dr, dg, db = runs[0]
        ds = cs.sum_bounds(res, relu, chain)
        what = f"relu={relu} dres={dres}"
        _check_grads("bn_bwd", cs, res, relu, dg, db, ds, what)
        cs.dz_check("bn_bwd", what, dz.t, None if dr is None else dr.t, res, relu, dres, ds)
        if len(runs) == 2:
            for a, b in zip(runs[0], runs[1]):
                assert (a is None and b is None) or R.same_bits(a.t, b.t), "clhip_bn_bwd is not run-to-run identical"


def _bwd_acc_form(entry, cs, d, relu, dres, rep, chain, seed=0):
    """one call of an accumulator-path backward entry and all its checks"""
    M, C, dt = cs.M, cs.C, cs.dt
    res = dres != 0
    yin = _bwd_inputs(cs, res, relu)
    gam, bet, mu, is_ = dev(cs.gamma), dev(cs.beta), dev(cs.mean32), dev(cs.invstd32)
    dg, db = G(C, init=dev(cs.dg0)), G(C, init=dev(cs.db0))
    dz = G((M, C), R.TDT[dt])
    dr = None if dres == 0 else (G((M, C), R.TDT[dt]) if dres == 1 else G((M, C), R.TDT[dt], init=dev(cs.dres0)))
    b = cs.bwd(res, relu != 0)
    if relu:
        assert_ambiguity_cap(cs, res)
    what = f"relu={relu} dres={dres} rep={rep}"
    if entry == "bn_bwd_apply_acc":
        # the sums arrive in the accumulator (as clhip_conv_dgrad_bn_reduce leaves them): the reference sums, split unevenly
        w = R.rnd((rep,), 300 + seed).double() + 0.3
        w[-1] = 1.0 - w[:-1].sum()
        host = w[:, None, None] * torch.stack([b["s1"], b["s2"]])[None]
        acc = G((rep, 2, C), torch.float64, init=dev(host))
        call("clhip_bn_bwd_apply_acc", ptr(d["dy"]), ptr(yin), ptr(d["z"]), ptr(mu), ptr(is_), ptr(gam), ptr(bet) if relu == 2 else None, ptr(dg), ptr(db),
             ptr(dz), ptr(dr), 1 if dres == 2 else 0, M, C, relu, ptr(acc), rep, CODE[dt], st())
        guards_ok(acc, dg, db, dz, dr)
        assert acc.untouched()
        noise = 4 * (rep + 2) * R.U64 * host.abs().sum(0)                # fp64: the split, and the kernel's sum over the replicas
        ds = (noise[0], noise[1])
    else:
        acc = G((rep, 2, C), torch.float64, fill=0.0)
        if entry == "bn_bwd_acc_zmask":
            call("clhip_bn_bwd_acc_zmask", ptr(d["dy"]), ptr(d["z"]), ptr(mu), ptr(is_), ptr(gam), ptr(bet), ptr(dg), ptr(db), ptr(dz), M, C, ptr(acc), rep,
                 CODE[dt], st())
        else:
            call("clhip_bn_bwd_acc", ptr(d["dy"]), ptr(yin), ptr(d["z"]), ptr(mu), ptr(is_), ptr(gam), ptr(dg), ptr(db), ptr(dz), ptr(dr),
                 1 if dres == 2 else 0, M, C, relu, ptr(acc), rep, CODE[dt], st())
        guards_ok(acc, dg, db, dz, dr)
        ds = cs.sum_bounds(res, relu != 0, chain)
        tot = acc.cpu().sum(0)
        chan_check(entry, dt, what + " acc sum g", tot[0], b["s1"], ds[0])
        chan_check(entry, dt, what + " acc sum g xhat", tot[1], b["s2"], ds[1])
    _check_grads(entry, cs, res, relu != 0, dg, db, ds, what)
    cs.dz_check(entry, what, dz.t, None if dr is None else dr.t, res, relu != 0, dres, ds)
    return dz, dr


@pytest.mark.parametrize("M,C,dt", cases(R.GEOMS_POW2, big=True))
def test_bn_bwd_accumulator_path(M, C, dt):
    """clhip_bn_bwd_acc (relu 0, 1 = y, 3 = packed mask) x dres {none, written, accumulated} and clhip_bn_bwd_acc_zmask (relu 2); the fp64 accumulator
    replicas, dgamma / dbeta = old + sum once, dz, dres"""
    cs = R.case(M, C, dt)
    d = devin(cs)
    chain = R.bwd_chain(M, C, _lib.lib().clhip_bn_bwd_blocks(M, C))
    forms = [(3, 2), (2, 0)] if is_big(M, C) else BWD_FORMS
    for i, (relu, dres) in enumerate(forms):
        rep = BWD_REPS[(i + M) % len(BWD_REPS)]
        _bwd_acc_form("bn_bwd_acc_zmask" if relu == 2 else "bn_bwd_acc", cs, d, relu, dres, rep, chain, seed=i)


@pytest.mark.parametrize("M,C,dt", cases(R.GEOMS_POW2, big=True))
def test_bn_bwd_apply_acc_every_live_form(M, C, dt):
    """clhip_bn_bwd_apply_acc, the entry the plan runs: relu {0, 1, 2, 3} x dres {none, written, accumulated (DRES == 2)}; relu = 2 without dres only"""
    cs = R.case(M, C, dt)
    d = devin(cs)
    forms = [(1, 2), (3, 1), (2, 0)] if is_big(M, C) else BWD_FORMS
    for i, (relu, dres) in enumerate(forms):
        rep = BWD_REPS[(i + M + 2) % len(BWD_REPS)]
        _bwd_acc_form("bn_bwd_apply_acc", cs, d, relu, dres, rep, 0, seed=i)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,C", [(75, 64), (37, 1024)], ids=["75x64_narrow_replica_parts", "37x1024_wide_sum_strided"])
@pytest.mark.parametrize("rep", BWD_REPS)
def test_bn_bwd_replicas(M, C, dt, rep):
    cs = R.case(M, C, dt)
    d = devin(cs)
    chain = R.bwd_chain(M, C, _lib.lib().clhip_bn_bwd_blocks(M, C))
    _bwd_acc_form("bn_bwd_acc", cs, d, 1, 2, rep, chain, seed=rep)
    _bwd_acc_form("bn_bwd_acc_zmask", cs, d, 2, 0, rep, chain, seed=rep)
    _bwd_acc_form("bn_bwd_apply_acc", cs, d, 3, 2, rep, 0, seed=rep)


# ================================================================================================== add_stats / add_inplace
@pytest.mark.parametrize("M,C,dt", cases(R.GEOMS_POW2, big=True))
def test_add_stats_and_add_inplace(M, C, dt):
    """z += r stored bit for bit; the statistics are those of the STORED sums, added onto the accumulator replicas"""
    cs = R.case(M, C, dt)
    d = devin(cs)
    want = R.add_stored(cs.z, cs.res, dt)
    a = G((M, C), R.TDT[dt], init=d["z"])
    call("clhip_add_inplace", ptr(a), ptr(d["res"]), M * C, CODE[dt], st())
    guards_ok(a)
    assert R.same_bits(a.t, want), "add_inplace"
    z2 = G((M, C), R.TDT[dt], init=d["z"])
    call("clhip_add_stats", ptr(z2), ptr(d["res"]), None, 1, M, C, CODE[dt], st())
    guards_ok(z2)
    assert R.same_bits(z2.t, want), "add_stats without accumulator"
    if is_big(M, C):
        reps = [16]
    else:
        reps = [1, 4, 16]
    s1 = torch.zeros(C, dtype=torch.float64)
    s2, a1 = torch.zeros_like(s1), torch.zeros_like(s1)
    for lo, hi in R.blocks(M):
        w = want[lo:hi].double()
        s1 += w.sum(0); s2 += (w * w).sum(0); a1 += w.abs().sum(0)
    chain = R.add_stats_chain(M, C, _lib.lib().clhip_add_stats_blocks(M, C))
    for rep in reps:
        start = R.rnd((rep, 2, C), 40 + rep, 5.0).double()
        acc = G((rep, 2, C), torch.float64, init=dev(start))
        z3 = G((M, C), R.TDT[dt], init=d["z"])
        call("clhip_add_stats", ptr(z3), ptr(d["res"]), ptr(acc), rep, M, C, CODE[dt], st())
        guards_ok(z3, acc)
        assert R.same_bits(z3.t, want), "add_stats with accumulator"
        tot = acc.cpu().sum(0)
        base = start.sum(0)
        slack = 4 * (rep + 2) * R.U64 * start.abs().sum(0)
        # terms are exact (the stored value; its square inside an fma): t = 0
        chan_check("add_stats", dt, f"rep={rep} sum", tot[0], base[0] + s1, R.bound_sum(chain, 0, a1) + slack[0])
        chan_check("add_stats", dt, f"rep={rep} sum of squares", tot[1], base[1] + s2, R.bound_sum(chain, 0, s2) + slack[1])


# ================================================================================================== pooling
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("HW", [1, 7, 8, 9, 49, 64])
def test_global_avgpool(HW, dt):
    """the unroll-by-8 loop and its tail; C = 3 for the forward (any C > 0), C = 24 for the backward, C = 64 both ways"""
    N = 5
    for C in (3, 64):
        a = R.rnd((N, HW, C), 50 + HW).to(R.TDT[dt])
        feat = G((N, C))
        call("clhip_avgpool_fwd", ptr(dev(a)), ptr(feat), N, HW, C, CODE[dt], st())
        guards_ok(feat)
        ref = R.avgpool_fwd(a.double())
        chan_check("avgpool_fwd", dt, f"HW={HW} C={C}", feat, ref, R.bound_pool_fwd(a.double().abs().sum(1), HW, ref))
    for C in (24, 64):                       # (e0 % C indexing at a C that is no power of two)
        df = R.rnd((N, C), 60 + HW)
        da = G((N, HW, C), R.TDT[dt])
        call("clhip_avgpool_bwd", ptr(dev(df)), ptr(da), N, HW, C, CODE[dt], st())
        guards_ok(da)
        ref = R.avgpool_bwd(df.double(), HW)
        chan_check("avgpool_bwd", dt, f"HW={HW} C={C}", da, ref, R.bound_pool_bwd(ref, dt))


def test_global_avgpool_bwd_second_grid_stride():
    """1049600 chunks: more than the 4096 x 256 threads of ew_blocks' cap"""
    N, HW, C, dt = 2050, 64, 64, "bf16"
    df = R.rnd((N, C), 61)
    da = G((N, HW, C), R.TDT[dt])
    call("clhip_avgpool_bwd", ptr(dev(df)), ptr(da), N, HW, C, CODE[dt], st())
    guards_ok(da)
    ref = R.avgpool_bwd(df.double(), HW)
    chan_check("avgpool_bwd", dt, "second grid stride", da, ref, R.bound_pool_bwd(ref, dt))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N,HW,C,rep,with_y", [(3, 64, 64, 4, 1), (5, 49, 8, 1, 1), (2, 16, 512, 2, 0), (37, 1, 2048, 16, 1), (300, 64, 64, 64, 1)],
                         ids=["3x64x64", "5x49x8_one_group", "2x16x512_no_relu", "37x1x2048_widest", "300x64x64_several_trips"])
def test_avgpool_bwd_bn_reduce(N, HW, C, rep, with_y, dt):
    """da = dfeat / HW and, of g = da masked by y > 0 (y an input here: no ambiguity), sum g and invstd (sum g z - mean sum g) added onto the replicas"""
    M = N * HW
    df = R.rnd((N, C), 70)
    z = (R.rnd((M, C), 71, 2.0) + 0.3).to(R.TDT[dt])
    y = R.rnd((M, C), 72).clamp_min(0.0).to(R.TDT[dt])
    mean, invstd = R.rnd((C,), 73, 0.5) + 0.3, R.rnd((C,), 74, 0.3) + 0.9
    start = R.rnd((rep, 2, C), 75, 2.0).double()
    acc = G((rep, 2, C), torch.float64, init=dev(start))
    da = G((N, HW, C), R.TDT[dt])
    call("clhip_avgpool_bwd_bn_reduce", ptr(dev(df)), ptr(da), ptr(dev(z)), ptr(dev(y)) if with_y else None, ptr(dev(mean)), ptr(dev(invstd)), ptr(acc), rep,
         N, HW, C, CODE[dt], st())
    guards_ok(acc, da)
    ref = R.avgpool_bwd(df.double(), HW)
    chan_check("avgpool_bwd_bn_reduce", dt, "da", da, ref, R.bound_pool_bwd(ref, dt))
    g = ref.reshape(M, C) * ((y.double() > 0) if with_y else 1.0)
    z64, mu, is_ = z.double(), mean.double(), invstd.double()
    s1, s2 = g.sum(0), is_ * ((g * z64).sum(0) - mu * g.sum(0))
    a1, a2 = g.abs().sum(0), (g * z64).abs().sum(0)
    d = R.pool_bn_chain(M * C // 8, C)
    slack = 4 * (rep + 2) * R.U64 * start.abs().sum(0)
    tot, base = acc.cpu().sum(0), start.sum(0)
    # g = fl(dfeat fl(1 / HW)) carries 2 roundings; sum g z adds by fma: 2 per term; then fl(istd fl(a2 - fl(mean a1))): product 1, difference 1 on
    # both, product 1 on both -> (d + 2 + 2) u sum |g z| + (d + 2 + 3) u |mean| sum |g|, times invstd
    chan_check("avgpool_bwd_bn_reduce", dt, "sum g", tot[0], base[0] + s1, R.bound_sum(d, 2, a1) + slack[0])
    chan_check("avgpool_bwd_bn_reduce", dt, "sum g xhat", tot[1], base[1] + s2, is_.abs() * (R.bound_sum(d, 4, a2) + R.bound_sum(d, 5, mu.abs() * a1)) + slack[1])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N,H,W,C,win", [(3, 17, 18, 16, 8), (2, 16, 24, 24, 8), (2, 5, 6, 40, 1), (3, 6, 6, 8, 6), (2, 9, 7, 3, 2)],
                         ids=["17x18_win8_ragged_both", "16x24_win8_C24", "win1_C40", "win_eq_H", "C3_forward_only"])
def test_windowed_avgpool(N, H, W, C, win, dt):
    """AvgPool2d(win) + flatten: the floor rule, the NCHW flatten order; the backward exactly zero on the uncovered border"""
    a = R.rnd((N, H, W, C), 80).to(R.TDT[dt])
    Ph, Pw = H // win, W // win
    feat = G((N, C * Ph * Pw))
    call("clhip_avgpool_win_fwd", ptr(dev(a)), ptr(feat), N, H, W, C, win, CODE[dt], st())
    guards_ok(feat)
    ref = R.avgpool_win_fwd(a.double(), win)
    sum_abs = R.avgpool_win_fwd(a.double().abs(), win) * (win * win)
    chan_check("avgpool_win_fwd", dt, "feat", feat, ref, R.bound_pool_fwd(sum_abs, win * win, ref))
    if C % 8:
        return
    df = R.rnd((N, C * Ph * Pw), 81)
    dfd = G((N, C * Ph * Pw), init=dev(df))                     # padded: an index computed for a border pixel stays inside the allocation
    da = G((N, H, W, C), R.TDT[dt])
    call("clhip_avgpool_win_bwd", ptr(dfd), ptr(da), N, H, W, C, win, CODE[dt], st())
    guards_ok(da)
    ref = R.avgpool_win_bwd(df.double(), N, H, W, C, win)
    chan_check("avgpool_win_bwd", dt, "da", da, ref, R.bound_pool_bwd(ref, dt))
    got = da.cpu().float()
    assert float(got[:, Ph * win:].abs().sum()) == 0.0 and float(got[:, :, Pw * win:].abs().sum()) == 0.0
    assert R.same_bits(got[:, Ph * win:], torch.zeros_like(got[:, Ph * win:])), "-0 on the border"


def test_windowed_avgpool_bwd_second_grid_stride():
    """130 x 33 x 33 x 64 in bf16: 1132560 chunks, more than the 4096 x 256 threads of ew_blocks' cap, and ragged (33 = 4 x 8 + 1): the second trip
    of the grid-stride loop redoes the e0 / C, % W, % H decomposition and meets the uncovered border too"""
    N, H, W, C, win, dt = 130, 33, 33, 64, 8, "bf16"
    assert N * H * W * C // 8 > 4096 * 256
    Ph, Pw = H // win, W // win
    df = R.rnd((N, C * Ph * Pw), 82)
    dfd = G((N, C * Ph * Pw), init=dev(df))
    da = G((N, H, W, C), R.TDT[dt])
    call("clhip_avgpool_win_bwd", ptr(dfd), ptr(da), N, H, W, C, win, CODE[dt], st())
    guards_ok(da)
    assert dfd.untouched()
    ref = R.avgpool_win_bwd(df.double(), N, H, W, C, win)
    chan_check("avgpool_win_bwd", dt, "second grid stride", da, ref, R.bound_pool_bwd(ref, dt))
    got = da.cpu()
    for border in (got[:, Ph * win:], got[:, :, Pw * win:]):
        assert R.same_bits(border, torch.zeros_like(border)), "the uncovered border is not +0"


# ================================================================================================== layout
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C,Cpad", [(3, 8), (20, 24), (16, 16)])
def test_layout_converts(C, Cpad, dt):
    N, H, W = 3, 5, 7
    x = R.rnd((N, C, H, W), 90)
    y = G((N, H, W, Cpad), R.TDT[dt])
    call("clhip_nchw_to_nhwc", ptr(dev(x)), ptr(y), N, C, H, W, Cpad, CODE[dt], st())
    guards_ok(y)
    assert R.same_bits(y.t, R.nchw_to_nhwc(x, Cpad).to(R.TDT[dt])), "nchw_to_nhwc (pad lanes +0)"
    back = G((N, Cpad, H, W))
    call("clhip_nhwc_to_nchw", ptr(y), ptr(back), N, Cpad, H, W, CODE[dt], st())
    guards_ok(back)
    assert R.same_bits(back.t, R.nhwc_to_nchw(y.cpu().float()))
    assert R.same_bits(back.t[:, :C], x.to(R.TDT[dt]).float())           # the round trip: the identity on f32, the bf16 rounding otherwise
    if dt == "f32":
        assert R.same_bits(back.t[:, :C], x)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K,taps,Creal,Cpad,with_dg", [(32, 9, 3, 8, 1), (32, 9, 3, 8, 0), (7, 1, 16, 16, 1), (5, 49, 3, 8, 1), (300, 9, 20, 24, 1)])
def test_conv_weight_prep(K, taps, Creal, Cpad, with_dg, dt):
    w = R.rnd((K, taps, Creal), 91)
    wf = G((K, taps, Cpad), R.TDT[dt])
    wd = G((Cpad, taps, K), R.TDT[dt]) if with_dg else None
    call("clhip_conv_weight_prep", ptr(dev(w)), ptr(wf), ptr(wd), K, taps, Creal, Cpad, CODE[dt], st())
    guards_ok(wf, wd)
    rf, rd = R.weight_prep(w, Cpad)
    assert R.same_bits(wf.t, rf.to(R.TDT[dt]))
    if with_dg:
        assert R.same_bits(wd.t, rd.to(R.TDT[dt]))


# ================================================================================================== directed cases
@pytest.mark.parametrize("dt,value", [("f32", 0.5), ("bf16", 0.5), ("bf16", 300.0)])
def test_zero_variance_channel(dt, value):
    """a constant channel: var = 0, invstd = 1 / sqrt(eps), y = beta (+ res), dz finite; and sums whose difference is NEGATIVE are clamped to var = 0"""
    M, C = 777, 16
    gamma, beta = torch.ones(C), torch.full((C,), 1.0)
    cs = R.Case(M, C, dt, seed=11, const={2: value, 9: value}, gamma=gamma, beta=beta)
    cs.directed = (2, 9)
    d = dict(z=dev(cs.z), res=dev(cs.res), dy=dev(cs.dy))
    assert float(cs.var[2]) < 1e-9
    for res, relu in ((0, 0), (1, 1)):
        out = _apply_train(cs, d, 4, res, relu, relu)
        _check_apply_train(cs, out, res, relu, f"const={value} res={res} relu={relu}", "bn_apply_train_mask" if relu else "bn_apply_train")
        assert bool(torch.isfinite(out["y"].cpu().float()).all())
        want = 1.0 / math.sqrt(R.EPS)
        assert abs(float(out["invstd"].cpu()[2]) - want) <= R.bound_invstd(torch.tensor(want), cs.var[2], out["view"].noise[2], R.istd_kind("apply_train", dt))
    # the clamp: the sum of squares one part in 2^20 BELOW M mean^2 (what fp32 partial rows can do to a constant channel): without the clamp
    # var + eps < 0 and invstd is NaN
    neg = copy.copy(cs)
    s2 = cs.s2.clone()
    s2[2] = cs.s1[2] ** 2 / M * (1 - 2.0 ** -20) - 1.0
    neg.set_sums(cs.s1, s2)
    assert float(neg.var[2]) == 0.0 and float(s2[2] / M - (cs.s1[2] / M) ** 2) < -R.EPS
    out = _apply_train(neg, d, 2, 0, 0, 0)
    _check_apply_train(neg, out, 0, 0, f"const={value} negative variance", "bn_apply_train")
    part = torch.stack([neg.s1, neg.s2])[None].float()
    fin = copy.copy(neg)
    fin.set_sums(part[0, 0].double(), part[0, 1].double())
    assert float(part[0, 1, 2].double() / M - (part[0, 0, 2].double() / M) ** 2) < -R.EPS, "the fp32 partials no longer give a negative variance"
    rm, rv, mean, invstd, scale, shift = G(C, init=dev(cs.rm0)), G(C, init=dev(cs.rv0)), G(C), G(C), G(C), G(C)
    call("clhip_bn_stats_finalize", ptr(dev(part)), 1, M, C, ptr(dev(gamma)), ptr(dev(beta)), ptr(rm), ptr(rv), R.MOM, R.EPS, ptr(mean), ptr(invstd),
         ptr(scale), ptr(shift), st())
    guards_ok(rm, rv, mean, invstd, scale, shift)
    check_saved_stats("bn_stats_finalize", fin, "fp64", mean, invstd, rm, rv, "negative variance")
    # backward through the constant channels: xhat = 0 there, dz = gi (g - mean g), finite
    chain = R.bwd_chain(M, C, _lib.lib().clhip_bn_bwd_blocks(M, C))
    dz, _ = _bwd_acc_form("bn_bwd_acc", cs, d, 1, 1, 4, chain)
    assert bool(torch.isfinite(dz.cpu().float()).all())


def test_large_mean_small_spread():
    """offset 50, spread 0.05, f32: the |mean scale| term of the forward bound carries the cancellation; no extra slack"""
    M, C, dt = 1000, 32, "f32"
    cs = R.Case(M, C, dt, seed=12, spread=0.05, offset=50.0)
    d = dict(z=dev(cs.z), res=dev(cs.res), dy=dev(cs.dy))
    for res in (0, 1):                       # without ReLU: at this conditioning the fp32 part of the bound (~2e-3) would make ~1e-3 of the masks ambiguous
        out = _apply_train(cs, d, 4, res, 0, 0)
        _check_apply_train(cs, out, res, 0, f"large mean res={res}", "bn_apply_train")
    chain = R.bwd_chain(M, C, _lib.lib().clhip_bn_bwd_blocks(M, C))
    _bwd_acc_form("bn_bwd_acc", cs, d, 0, 2, 4, chain)


@pytest.mark.parametrize("dt", DTS)
def test_no_running_statistics(dt):
    """rm = rv = NULL: y and the saved statistics only; rm without rv: refused, nothing written"""
    M, C = 75, 64
    cs = R.case(M, C, dt)
    d = devin(cs)
    out = _apply_train(cs, d, 2, 1, 1, 1, with_running=False)
    _check_apply_train(cs, out, 1, 1, "no running stats", "bn_apply_train_mask")
    part = torch.stack([cs.s1, cs.s2])[None].float()
    fin = copy.copy(cs)
    fin.set_sums(part[0, 0].double(), part[0, 1].double())
    gam, bet = dev(cs.gamma), dev(cs.beta)
    mean, invstd, scale, shift = G(C), G(C), G(C), G(C)
    call("clhip_bn_stats_finalize", ptr(dev(part)), 1, M, C, ptr(gam), ptr(bet), None, None, R.MOM, R.EPS, ptr(mean), ptr(invstd), ptr(scale), ptr(shift), st())
    guards_ok(mean, invstd, scale, shift)
    check_saved_stats("bn_stats_finalize", fin, "fp64", mean, invstd, None, None, "no running stats")
    L = _lib.lib()
    rm = G(C, init=dev(cs.rm0))
    mean, invstd, scale, shift, y = G(C), G(C), G(C), G(C), G((M, C), R.TDT[dt])
    acc = dev(cs.split(2))
    assert L.clhip_bn_stats_finalize(ptr(dev(part)), 1, M, C, ptr(gam), ptr(bet), ptr(rm), None, R.MOM, R.EPS, ptr(mean), ptr(invstd), ptr(scale), ptr(shift),
                                     st()) == EINVAL
    assert L.clhip_bn_apply_train(ptr(d["z"]), ptr(acc), 2, M, C, ptr(gam), ptr(bet), ptr(rm), None, R.MOM, R.EPS, ptr(mean), ptr(invstd), None, ptr(y), 1,
                                  CODE[dt], st()) == EINVAL
    torch.cuda.synchronize()
    assert all(g.untouched() for g in (rm, mean, invstd, scale, shift, y))


def test_refusals():
    """every launcher's argument check: CLHIP_EINVAL and the NaN-filled outputs untouched"""
    L = _lib.lib()
    M, dt = 16, "bf16"
    code = CODE[dt]
    big = 4096
    buf = lambda n: torch.zeros(n, dtype=torch.bfloat16, device=DEV)          # noqa: E731
    z, dy, y = buf(M * big), buf(M * big), buf(M * big)
    f = lambda n: torch.ones(n, device=DEV)                                    # noqa: E731
    mu, is_, gam, bet = f(big), f(big), f(big), f(big)
    acc = torch.zeros(64 * 2 * big, dtype=torch.float64, device=DEV)
    outs = dict(dg=G(big), db=G(big), dz=G(M * big, torch.bfloat16), dr=G(M * big, torch.bfloat16), mean=G(big), invstd=G(big), yo=G(M * big, torch.bfloat16),
                bits=G(M * big // 8, torch.uint8), ws=G(4 * big + 2 * big * 16))
    o = {k: ptr(v) for k, v in outs.items()}
    P = ptr

    def bwd_acc(C, rep, relu=0, yy=None, dtype=code, dres=None):
        return L.clhip_bn_bwd_acc(P(dy), yy, P(z), P(mu), P(is_), P(gam), o["dg"], o["db"], o["dz"], dres, 0, M, C, relu, P(acc), rep, dtype, st())

    def zmask(C, rep, beta=P(bet), dtype=code):
        return L.clhip_bn_bwd_acc_zmask(P(dy), P(z), P(mu), P(is_), P(gam), beta, o["dg"], o["db"], o["dz"], M, C, P(acc), rep, dtype, st())

    def apply_acc(C, rep, relu=0, yy=None, beta=None, dres=None, dtype=code):
        return L.clhip_bn_bwd_apply_acc(P(dy), yy, P(z), P(mu), P(is_), P(gam), beta, o["dg"], o["db"], o["dz"], dres, 0, M, C, relu, P(acc), rep, dtype, st())

    def train(C, rep, dtype=code, mask=False):
        if mask:
            return L.clhip_bn_apply_train_mask(P(z), P(acc), rep, M, C, P(gam), P(bet), None, None, R.MOM, R.EPS, o["mean"], o["invstd"], None, o["yo"],
                                               o["bits"], dtype, st())
        return L.clhip_bn_apply_train(P(z), P(acc), rep, M, C, P(gam), P(bet), None, None, R.MOM, R.EPS, o["mean"], o["invstd"], None, o["yo"], 1, dtype, st())

    refused = []
    for C in (24, 40, 4, 4096, 0):                                            # not a power of two / out of [8, 2048]
        refused += [bwd_acc(C, 4), zmask(C, 4), apply_acc(C, 4), train(C, 4), train(C, 4, mask=True)]
    for rep in (3, 5, 63, 0, 65, -1):                                          # the backward entries: powers of two in 1..64
        refused += [bwd_acc(64, rep), zmask(64, rep), apply_acc(64, rep)]
    for rep in (0, 65, -1):                                                    # the forward entries: 1..64
        refused += [train(64, rep), train(64, rep, mask=True)]
    refused += [bwd_acc(64, 4, dtype=7), zmask(64, 4, dtype=7), apply_acc(64, 4, dtype=7), train(64, 4, dtype=7), train(64, 4, dtype=7, mask=True)]
    refused += [bwd_acc(64, 4, relu=1), bwd_acc(64, 4, relu=3), apply_acc(64, 4, relu=1), apply_acc(64, 4, relu=3)]            # relu 1 / 3 without y
    refused += [apply_acc(64, 4, relu=2), apply_acc(64, 4, relu=2, beta=P(bet), dres=o["dr"]), apply_acc(64, 4, relu=4, yy=P(y)), apply_acc(64, 4, relu=-1)]
    refused += [zmask(64, 4, beta=None)]
    # the partial-buffer path
    for C in (4096, 12, 0):
        refused.append(L.clhip_bn_bwd(P(dy), None, P(z), P(mu), P(is_), P(gam), o["dg"], o["db"], o["dz"], None, 0, M, C, 0, o["ws"], code, st()))
    refused.append(L.clhip_bn_bwd(P(dy), None, P(z), P(mu), P(is_), P(gam), o["dg"], o["db"], o["dz"], None, 0, M, 64, 1, o["ws"], code, st()))      # relu without y
    refused.append(L.clhip_bn_bwd(P(dy), None, P(z), P(mu), P(is_), P(gam), o["dg"], o["db"], o["dz"], None, 0, M, 64, 0, o["ws"], 7, st()))
    refused.append(L.clhip_bn_bwd(P(dy), None, P(z), P(mu), P(is_), P(gam), o["dg"], o["db"], o["dz"], None, 0, 0, 64, 0, o["ws"], code, st()))
    refused.append(L.clhip_bn_apply(P(z), P(mu), P(is_), None, o["yo"], M, 12, 0, code, st()))
    refused.append(L.clhip_bn_apply(P(z), P(mu), P(is_), None, o["yo"], M, 64, 0, 7, st()))
    refused.append(L.clhip_bn_apply_eval(P(z), P(gam), P(bet), P(mu), P(is_), R.EPS, None, o["yo"], M, 8200, 0, code, st()))
    refused.append(L.clhip_bn_apply_eval(P(z), P(gam), P(bet), P(mu), P(is_), R.EPS, None, o["yo"], M, 64, 0, 7, st()))
    refused.append(L.clhip_bn_eval_affine(P(gam), P(bet), P(mu), None, R.EPS, 64, o["mean"], o["invstd"], st()))
    # add_stats: C / 8 must divide 256; replicas a power of two when an accumulator is given
    zz = G(M * 64, torch.bfloat16)
    for C, rep, a in ((24, 4, P(acc)), (4096, 4, P(acc)), (64, 3, P(acc)), (64, 0, P(acc))):
        refused.append(L.clhip_add_stats(P(zz), P(y), a, rep, M, C, code, st()))
    refused.append(L.clhip_add_stats(P(zz), P(y), None, 1, M, 64, 7, st()))
    refused.append(L.clhip_add_inplace(P(zz), P(y), 12, code, st()))
    refused.append(L.clhip_add_inplace(P(zz), P(y), 64, 7, st()))
    # pooling and layout
    refused.append(L.clhip_avgpool_fwd(P(z), o["mean"], 2, 4, 8, 7, st()))
    refused.append(L.clhip_avgpool_bwd(P(mu), o["dz"], 2, 4, 12, code, st()))
    refused.append(L.clhip_avgpool_bwd(P(mu), o["dz"], 2, 4, 8, 7, st()))
    refused.append(L.clhip_avgpool_bwd_bn_reduce(P(mu), o["dz"], P(z), None, P(mu), P(is_), P(acc), 3, 2, 4, 8, code, st()))
    refused.append(L.clhip_avgpool_bwd_bn_reduce(P(mu), o["dz"], P(z), None, P(mu), P(is_), P(acc), 4, 2, 4, 24, code, st()))
    refused.append(L.clhip_avgpool_bwd_bn_reduce(P(mu), o["dz"], P(z), None, P(mu), P(is_), P(acc), 4, 2, 4, 8, 7, st()))
    refused.append(L.clhip_avgpool_win_fwd(P(z), o["mean"], 2, 4, 4, 8, 5, code, st()))                    # win > H
    refused.append(L.clhip_avgpool_win_fwd(P(z), o["mean"], 2, 4, 4, 8, 0, code, st()))
    refused.append(L.clhip_avgpool_win_bwd(P(mu), o["dz"], 2, 4, 4, 12, 2, code, st()))
    refused.append(L.clhip_avgpool_win_bwd(P(mu), o["dz"], 2, 4, 4, 8, 2, 7, st()))
    refused.append(L.clhip_nchw_to_nhwc(P(mu), o["yo"], 2, 3, 4, 4, 12, code, st()))                       # Cpad % 8
    refused.append(L.clhip_nchw_to_nhwc(P(mu), o["yo"], 2, 9, 4, 4, 8, code, st()))                        # Cpad < C
    refused.append(L.clhip_nchw_to_nhwc(P(mu), o["yo"], 2, 3, 4, 4, 8, 7, st()))
    refused.append(L.clhip_nhwc_to_nchw(P(z), o["mean"], 2, 3, 4, 4, 7, st()))
    refused.append(L.clhip_conv_weight_prep(P(mu), o["yo"], None, 4, 9, 9, 8, code, st()))                # Cpad < Creal
    refused.append(L.clhip_conv_weight_prep(P(mu), o["yo"], None, 4, 9, 3, 8, 7, st()))
    torch.cuda.synchronize()
    assert all(rc == EINVAL for rc in refused), [i for i, rc in enumerate(refused) if rc != EINVAL]
    for k, v in outs.items():
        assert v.untouched(), k
    assert zz.untouched()
    assert float(acc.abs().sum()) == 0.0


def test_relu_mask_rule_at_the_storage_floor():
    """bf16, one channel with gamma = 3e-41 (an fp32 subnormal) and beta = 0: its positive outputs straddle 2^-134, half the smallest bf16 subnormal,
    below which a positive fp32 value is STORED as +0.  The packed mask (form 3) is "stored y > 0"; reading y (form 1) gives the same dz / dres bit
    for bit; and so does the mask recomputed from z (form 2), which applies the same stored-value test to its fp32 value."""
    M, C, dt = 1000, 32, "bf16"
    ch = 5
    gamma, beta = R.rnd((C,), 13, 0.5) + 1.0, R.rnd((C,), 14, 0.2)
    gamma[ch], beta[ch] = 3e-41, 0.0
    assert float(gamma[ch]) > 0.0
    cs = R.Case(M, C, dt, seed=15, gamma=gamma, beta=beta)
    cs.directed = (ch,)
    d = dict(z=dev(cs.z), res=dev(cs.res), dy=dev(cs.dy))
    out = _apply_train(cs, d, 4, 0, 1, 1)
    _check_apply_train(cs, out, 0, 1, "storage floor", "bn_apply_train_mask")
    ycpu, bits = out["y"].cpu(), out["bits"].cpu()
    stored_pos = ycpu.float() > 0
    assert torch.equal(bits, R.pack_mask(stored_pos)), "packed mask != (stored y > 0)"
    true_pos = cs.ypre(0)[:, ch] > 0
    n_true, n_stored = int(true_pos.sum()), int(stored_pos[:, ch].sum())
    print(f"[floor] channel {ch}: {n_true} outputs positive in fp64, {n_stored} stored positive")
    if n_stored == 0:
        pytest.skip("degenerate: every form masks the channel off entirely (the fp32 subnormal scale did not survive the kernels' fmaf on this build)")
    assert 0 < n_stored < n_true, "the channel does not straddle the storage floor"
    chain = R.bwd_chain(M, C, _lib.lib().clhip_bn_bwd_blocks(M, C))
    gam, bet = dev(cs.gamma), dev(cs.beta)
    got = {}
    for relu, yin in ((1, out["y"].t), (3, out["bits"].t), (2, None)):
        acc = G((4, 2, C), torch.float64, fill=0.0)
        dg, db = G(C, fill=0.0), G(C, fill=0.0)
        dz = G((M, C), R.TDT[dt])
        if relu == 2:
            call("clhip_bn_bwd_acc_zmask", ptr(d["dy"]), ptr(d["z"]), ptr(out["mean"]), ptr(out["invstd"]), ptr(gam), ptr(bet), ptr(dg), ptr(db), ptr(dz), M, C,
                 ptr(acc), 4, CODE[dt], st())
        else:
            call("clhip_bn_bwd_acc", ptr(d["dy"]), ptr(yin), ptr(d["z"]), ptr(out["mean"]), ptr(out["invstd"]), ptr(gam), ptr(dg), ptr(db), ptr(dz), None, 0, M, C,
                 relu, ptr(acc), 4, CODE[dt], st())
        guards_ok(acc, dg, db, dz)
        got[relu] = (dz.cpu(), db.cpu())
        # the apply-only entry on the sums just reduced
        dg2, db2, dz2 = G(C, fill=0.0), G(C, fill=0.0), G((M, C), R.TDT[dt])
        dr2 = G((M, C), R.TDT[dt]) if relu != 2 else None
        call("clhip_bn_bwd_apply_acc", ptr(d["dy"]), ptr(yin), ptr(d["z"]), ptr(out["mean"]), ptr(out["invstd"]), ptr(gam), ptr(bet), ptr(dg2), ptr(db2), ptr(dz2),
             ptr(dr2), 0, M, C, relu, ptr(acc), 4, CODE[dt], st())
        guards_ok(dg2, db2, dz2, dr2)
        got[relu] += (dz2.cpu(), None if dr2 is None else dr2.cpu())
    assert R.same_bits(got[1][0], got[3][0]) and R.same_bits(got[1][2], got[3][2]) and R.same_bits(got[1][3], got[3][3]), "forms 1 and 3 differ"
    # dres (form 1 / 3) is dy under the stored mask, exactly
    assert R.same_bits(got[1][3], torch.where(stored_pos, cs.dy, torch.zeros_like(cs.dy)))
    # form 2.  In this channel dz itself is below the storage floor (gamma is), so a wrong mask shows as the sign of a zero in dz and, plainly, in
    # dbeta = sum g: 61 terms under the stored mask, 495 under "fp32 value > 0".  (Before stored_positive<T> was applied to the RELU == 2 branches
    # the bit comparison of dz below failed on this case, on signs of zeros only.)
    ds1, _ = cs.sum_bounds(0, False, chain)                       # the unmasked sum |dy| bounds either mask's
    db1, db2 = got[1][1].double(), got[2][1].double()
    print(f"[floor] dbeta[{ch}]: mask from y {float(db1[ch]):.6g}, mask from z {float(db2[ch]):.6g}; allowed difference {2 * float(ds1[ch]):.3g}")
    assert bool(((db1 - db2).abs() <= 2 * ds1 + 2 * R.U * db1.abs()).all()), "form 2 sums another mask than form 1"
    diff = int((got[2][0].view(torch.int16) != got[1][0].view(torch.int16)).sum())
    print(f"[floor] dz elements whose bits differ between the mask from z and the mask from y: {diff}")
    assert R.same_bits(got[2][0], got[1][0]) and R.same_bits(got[2][2], got[1][2]), f"form 2 differs from form 1 in {diff} elements"
