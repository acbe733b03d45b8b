"""The entry-block body of csrc/conv2.hip (3x3 / stride 2 / pad 1, bf16, Cd = 2 Cs, inside the generic family, behind the ENTRY_S2 switch) on a real MI355X.

The body stages its operands by LDS-DMA but multiplies and reduces exactly as the generic kernel does (same workgroup tile, same MFMAs in the same order, same
statistics reduction), so its z is the generic kernel's bit for bit, and so are the fp64 accumulators (one atomic per workgroup, channel and sum of the same fp32
values; fp64 sums of that few fp32 addends are exact, whatever their order).  That is what the tests hold it to, beside the fp64 reference:
z of every case against the per-element bound of tests/conv_ref.py (R = 9 Cs fp32 products, one bf16 store); the statistics against the fp64 sums of the kernel's
OWN stored z, the form tests/plan_ref.py uses,
    |s1 - sum z|   <= r (1 + r) sum |z| + b1,        |s2 - sum z^2| <= 2 r (1 + r) sum z^2 + b2,        r = 2^-8, (b1, b2) = conv_ref.stat_bounds(z, acc_bound)
and against the fp64 reference sums with conv_ref.stat_bounds as tests/conv_run.py does.

Since both kernels give the same bits, the outputs cannot tell which one ran.  clhip_conv_entry_s2_launches() counts the body's launches in this process, and
every test asserts the count it expects: one more per call inside the domain with the switch on (default, or "1" again after "0": the switch is read on every
call, not cached), none with ENTRY_S2=0, none outside the domain, none where the generic kernel takes its 128-pixel tile (256 images of 32x32: that tile has no
body), three per training forward of the `wide` net through the plan and none there with the switch off."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_ref as R                       # noqa: E402
import conv_run as CR                      # noqa: E402
from libcontinual_amd import _lib          # noqa: E402
from libcontinual_amd._lib import call     # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
HALF = 2.0 ** -8
# (N, H, W, Cs): the three shapes of ResNet-18's entry blocks, and 80 output pixels of 4x4 maps -- the second 64-pixel tile is ragged and the first holds four images
SHAPES = [(3, 8, 8, 256), (3, 16, 16, 128), (2, 32, 32, 64), (5, 8, 8, 64)]
_CACHE = {}
_ids = lambda v: "x".join(map(str, v))


def body_launches():
    return int(_lib.lib().clhip_conv_entry_s2_launches())


def _new_case(name, shape):
    """a case as tests/conv_ref.py's list holds them: shape = (N, H, W, C, K, k, stride, pad)"""
    return dict(name=name, shape=shape, creal=shape[3], routes={"bf16": dict(fwd2=R.CONV2), "f32": {}}, sw={})


def _stat_ratios(ref, b, s1, s2):
    """the statistics against the fp64 reference sums, bounds from conv_ref.stat_bounds (what tests/conv_run.py does)"""
    b1, b2 = R.stat_bounds(ref, b)
    return CR.ratio(s1, ref.sum((0, 2, 3)), b1), CR.ratio(s2, (ref * ref).sum((0, 2, 3)), b2)


def _case(shape):
    N, H, W, C = shape
    return _new_case(f"entry-{N}x{H}x{W}x{C}", (N, H, W, C, 2 * C, 3, 2, 1))


def _operands(shape):
    """operands and fp64 reference of a shape, computed once and shared (nothing writes to them)"""
    if shape not in _CACHE:
        o = CR.Operands(_case(shape), "bf16", seed=40)
        o.fwd_ref()
        _CACHE[shape] = o
    return _CACHE[shape]


def _launch(o, rep, switch=None):
    """clhip_conv_fwd_acc into NaN-filled z and zeroed accumulators; switch: None (default) / "0" / "1" """
    L = _lib.lib()
    N, H, W, C, K, k, s, p = o.dims()
    z = CR.Guarded((N, o.Ho, o.Wo, K), o.tdt, float("nan"))
    acc = CR.Guarded((rep, 2, K), torch.float64, 0.0)
    try:
        if switch is not None:
            assert L.clhip_config(b"ENTRY_S2", switch.encode()) == 0
        call("clhip_conv_fwd_acc", o.xd.data_ptr(), o.wfd.data_ptr(), z.ptr(), acc.ptr(), rep, N, H, W, C, K, k, s, p, o.code, CR.st())
        torch.cuda.synchronize()
    finally:
        if switch is not None:
            L.clhip_config(b"ENTRY_S2", None)
    assert z.guard_ok() and acc.guard_ok()
    return z.t, acc.t


def _judge(o, z, acc, tag):
    N, H, W, C, K, k, s, p = o.dims()
    ref, S = o.fwd_ref()
    Rn = k * k * C
    zz = CR.nchw64(z)
    out = {"z": CR.ratio(zz, ref, R.elem_bound(S, Rn, ref, o.dt))}
    b = R.acc_bound(S, Rn)
    s1, s2 = acc[:, 0].sum(0), acc[:, 1].sum(0)
    out["s1 vs ref"], out["s2 vs ref"] = _stat_ratios(ref, b, s1, s2)
    b1, b2 = R.stat_bounds(zz, b)
    out["s1 vs stored z"] = CR.ratio(s1, zz.sum((0, 2, 3)), HALF * (1 + HALF) * zz.abs().sum((0, 2, 3)) + b1)
    out["s2 vs stored z"] = CR.ratio(s2, (zz * zz).sum((0, 2, 3)), 2 * HALF * (1 + HALF) * (zz * zz).sum((0, 2, 3)) + b2)
    for what, r in out.items():
        print(f"[ratio] {o.case['name']} {tag} {what} {r:.4g}")
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_and_statistics_against_fp64(shape):
    o = _operands(shape)
    assert R.query(_lib.lib(), o.case, "bf16", "fwd2") == R.CONV2            # the route does not name the body: it lives inside the family
    for rep in (1, 8):
        n0 = body_launches()
        z, acc = _launch(o, rep)
        assert body_launches() == n0 + 1, "the body did not run"
        out = _judge(o, z, acc, f"rep{rep}")
        assert all(v <= 1.0 for v in out.values()), out


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_same_call_twice_same_bits(shape):
    o = _operands(shape)
    z1, a1 = _launch(o, 8)
    z2, a2 = _launch(o, 8)
    assert torch.equal(z1.view(torch.int16), z2.view(torch.int16))
    assert torch.equal(a1, a2)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_switch_is_read_on_every_call(shape):
    """default (the body) first, then ENTRY_S2=0, toggled after that first call: the generic kernel answers (the body's counter stands still), so the switch is not
    cached; then 1 again: the body.  The outputs differ by nothing -- inside the bound a fortiori"""
    o = _operands(shape)
    n0 = body_launches()
    z_on, a_on = _launch(o, 8)
    assert body_launches() == n0 + 1
    z_off, a_off = _launch(o, 8, "0")
    assert body_launches() == n0 + 1, "ENTRY_S2=0 after a first call still ran the body: the switch is cached"
    z_on2, a_on2 = _launch(o, 8, "1")
    assert body_launches() == n0 + 2
    assert all(v <= 1.0 for v in _judge(o, z_off, a_off, "ENTRY_S2=0").values())
    assert all(v <= 1.0 for v in _judge(o, z_on, a_on, "default").values())
    assert torch.equal(z_on.view(torch.int16), z_off.view(torch.int16)) and torch.equal(a_on, a_off)
    assert torch.equal(z_on.view(torch.int16), z_on2.view(torch.int16)) and torch.equal(a_on, a_on2)


def test_layer2_entry_at_batch_256_stays_on_the_generic_kernel():
    """65536 output pixels x 128 channels: the generic kernel takes its 128-pixel tile (512 workgroups), for which there is no body -- the launcher must fall
    through, whatever the switch says: no body launch, the same bits"""
    g = torch.Generator().manual_seed(7)
    N, H, C = 256, 32, 64
    x = (torch.rand(N, H, H, C, generator=g) * 2 - 1).to(torch.bfloat16).to(CR.DEV)
    w = ((torch.rand(2 * C, 3, 3, C, generator=g) * 2 - 1) / 24).to(torch.bfloat16).to(CR.DEV)
    L = _lib.lib()
    out = {}
    n0 = body_launches()
    for sw in ("1", "0"):
        z = CR.Guarded((N, H // 2, H // 2, 2 * C), torch.bfloat16, float("nan"))
        acc = CR.Guarded((16, 2, 2 * C), torch.float64, 0.0)
        try:
            assert L.clhip_config(b"ENTRY_S2", sw.encode()) == 0
            call("clhip_conv_fwd_acc", x.data_ptr(), w.data_ptr(), z.ptr(), acc.ptr(), 16, N, H, H, C, 2 * C, 3, 2, 1, _lib.BF16, CR.st())
            torch.cuda.synchronize()
        finally:
            L.clhip_config(b"ENTRY_S2", None)
        assert z.guard_ok() and acc.guard_ok() and not torch.isnan(z.t.float()).any()
        out[sw] = (z.t, acc.t)
    assert body_launches() == n0
    assert torch.equal(out["1"][0].view(torch.int16), out["0"][0].view(torch.int16))
    assert torch.equal(out["1"][1], out["0"][1])


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_partial_row_and_plain_forms_keep_the_same_z(shape):
    """clhip_conv_fwd with partial rows runs the body as well (tests/test_kernels_gpu.py holds the forms of one layer to the same bits): same z as the
    accumulator form, every allocated row written, column sums of the rows = the accumulators' (fp32 values summed in fp64: exact at this many tiles)"""
    o = _operands(shape)
    L = _lib.lib()
    N, H, W, C, K, k, s, p = o.dims()
    z_acc, acc = _launch(o, 1)
    n0 = body_launches()
    tiles = L.clhip_conv_fwd_tiles(N, H, W, C, K, k, s, p)
    assert tiles > 0
    z = CR.Guarded((N, o.Ho, o.Wo, K), o.tdt, float("nan"))
    part = CR.Guarded((tiles, 2, K), torch.float32, float("nan"))
    call("clhip_conv_fwd", o.xd.data_ptr(), o.wfd.data_ptr(), z.ptr(), part.ptr(), N, H, W, C, K, k, s, p, o.code, CR.st())
    torch.cuda.synchronize()
    assert z.guard_ok() and part.guard_ok()
    assert torch.equal(z.t.view(torch.int16), z_acc.view(torch.int16))
    assert not torch.isnan(part.t).any()
    assert torch.equal(part.t.double().sum(0), acc.sum(0))
    z0 = CR.Guarded((N, o.Ho, o.Wo, K), o.tdt, float("nan"))          # and the statistics-free call of eval forwards
    call("clhip_conv_fwd", o.xd.data_ptr(), o.wfd.data_ptr(), z0.ptr(), None, N, H, W, C, K, k, s, p, o.code, CR.st())
    torch.cuda.synchronize()
    assert z0.guard_ok() and torch.equal(z0.t.view(torch.int16), z_acc.view(torch.int16))
    assert body_launches() == n0 + 2


@pytest.mark.parametrize("shape", [(3, 8, 8, 128, 128), (2, 9, 9, 64, 128)], ids=["Cd=Cs", "odd-H"])
def test_outside_the_domain_the_switch_changes_nothing(shape):
    N, H, W, C, K = shape
    o = CR.Operands(_new_case("outside", (N, H, W, C, K, 3, 2, 1)), "bf16", seed=41)
    n0 = body_launches()
    z_on, a_on = _launch(o, 8, "1")
    z_off, a_off = _launch(o, 8, "0")
    assert body_launches() == n0
    assert torch.equal(z_on.view(torch.int16), z_off.view(torch.int16))
    # both calls are the generic kernel, which adds several workgroups' sums into one accumulator with fp64 atomics in no fixed order (csrc/bn.hip's header:
    # "equal to ~1e-16 relative, not bit for bit"): z is held to the same bits, the accumulators to 1e-12 relative
    assert CR.ratio(a_on, a_off, 1e-12 * a_off.abs()) <= 1.0
    assert all(v <= 1.0 for v in _judge(o, z_on, a_on, "outside").values())


@pytest.mark.parametrize("switch", ["1", "0"], ids=["ENTRY_S2=1", "ENTRY_S2=0"])
def test_plan_step_of_the_wide_net(switch):
    """one training step (and a second onto its gradients, and an eval forward) of the `wide` net at batch 16 through the plan, every stored link -- z, statistics, y,
    feat, every dy, dw, dgamma, dbeta -- inside the bf16 bounds tests/plan_ref.py derives, with the body and with the generic kernel (tests/plan_unit_worker.py, a
    fresh process per setting as in tests/test_plan_units_gpu.py)"""
    env = dict(os.environ, CLHIP_STAGE_TRAIN="0", CLHIP_STAGE_EVAL="0", CLHIP_ENTRY_S2=switch)
    r = subprocess.run([sys.executable, os.path.join(HERE, "plan_unit_worker.py"), "bf16", "wide-b16"], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert "RATIOS " in r.stdout and not [ln for ln in r.stdout.splitlines() if ln.startswith("FAIL ")]


def test_plan_forward_runs_the_body_three_times():
    """a training forward of the `wide` net at batch 16 through the plan in THIS process: its three entry forwards run the body with the default switch, the
    generic kernel with ENTRY_S2=0 set between two forwards (the plan reads the switch with every launch), the body again afterwards; same features every time"""
    import plan_ref as PR
    L = _lib.lib()
    net = PR.build_net("wide", "bf16").to(CR.DEV).train()
    net._ensure_flat(torch.device(CR.DEV))
    x = torch.randn(16, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(CR.DEV)

    def forward():
        net._stats.zero_()
        net._nbt.zero_()
        n0 = body_launches()
        out = net(x)
        torch.cuda.synchronize()
        feat = out if torch.is_tensor(out) else out["features"]
        return body_launches() - n0, feat.detach().float().clone()
    n_on, f_on = forward()
    try:
        assert L.clhip_config(b"ENTRY_S2", b"0") == 0
        n_off, f_off = forward()
    finally:
        L.clhip_config(b"ENTRY_S2", None)
    n_on2, f_on2 = forward()
    assert (n_on, n_off, n_on2) == (3, 0, 3), (n_on, n_off, n_on2)
    assert torch.equal(f_on, f_off) and torch.equal(f_on, f_on2)
