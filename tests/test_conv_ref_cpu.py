"""tests/conv_ref.py checks itself on the CPU: its im2col reference against F.conv2d and autograd in fp64, its accumulation bound against a plain fp32
emulation of the convolution in three summation orders, and -- through clhip_conv_route, host code that needs no device -- that the cases of
tests/test_conv_routes_gpu.py take the routes named for them and together reach every kernel family of every convolution entry point."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
from libcontinual_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("shape", [(2, 5, 7, 3, 4, 3, 1, 1), (3, 8, 8, 4, 6, 3, 2, 1), (2, 9, 9, 5, 3, 1, 2, 0), (2, 19, 23, 3, 4, 7, 2, 3), (1, 1, 1, 4, 4, 3, 1, 1)])
def test_reference_is_conv2d_and_its_autograd_gradients(shape):
    N, H, W, C, K, k, s, p = shape
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(K, C, k, k, generator=g, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    z = F.conv2d(xr, wr, None, s, p)
    dz = torch.randn(z.shape, generator=g, dtype=torch.float64)
    z.backward(dz)
    zr, S = R.conv_fwd_ref(x, w, s, p)
    assert torch.allclose(zr, z.detach(), rtol=1e-12, atol=1e-12) and bool((S >= zr.abs() - 1e-12).all())
    dx, S = R.conv_dgrad_ref(dz, w, s, p, H, W)
    assert torch.allclose(dx, xr.grad, rtol=1e-12, atol=1e-12) and bool((S >= dx.abs() - 1e-12).all())
    dw, S = R.conv_wgrad_ref(x, dz, k, s, p)
    assert torch.allclose(dw, wr.grad, rtol=1e-12, atol=1e-12) and bool((S >= dw.abs() - 1e-12).all())


def _emulate(cols, wm, order):
    """fp32 products summed in fp32, one reduction element at a time: wm [K, R] . cols [R, P]"""
    Rn = wm.shape[1]
    ks = {"forward": [range(Rn)], "reversed": [range(Rn - 1, -1, -1)], "two groups": [range(0, Rn // 2), range(Rn // 2, Rn)]}[order]
    parts = []
    for sl in ks:
        acc = np.zeros((wm.shape[0], cols.shape[1]), np.float32)
        for r in sl:
            acc = acc + wm[:, r:r + 1] * cols[r][None, :]
        parts.append(acc)
    out = parts[0]
    for q in parts[1:]:
        out = out + q
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("C", [16, 128])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_accumulation_bound_holds_for_an_fp32_emulation(C, dt):
    N, H, W, K, k = 2, 5, 6, 24, 3
    g = torch.Generator().manual_seed(C)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, k, k, generator=g) / (C * k * k) ** 0.5
    if dt == "bf16":
        x, w = x.bfloat16().float(), w.bfloat16().float()
    ref, S = R.conv_fwd_ref(x, w, 1, 1)
    allowed = R.acc_bound(S, k * k * C)
    cols = F.unfold(x, k, padding=1)                      # fp32 copies of the operands: the products are fp32 products
    for order in ("forward", "reversed", "two groups"):
        got = torch.stack([torch.from_numpy(_emulate(cols[n].numpy(), w.reshape(K, -1).numpy(), order)) for n in range(N)]).reshape(N, K, H, W).double()
        over = (got - ref).abs() > allowed
        assert int(over.sum()) == 0, (order, int(over.sum()))
        assert float((got - ref).abs().max()) > 0.0          # the emulation does round
        # the statistics' bounds follow from the elements'
        b1, b2 = R.stat_bounds(ref, allowed)
        assert bool(((got.sum((0, 2, 3)) - ref.sum((0, 2, 3))).abs() <= b1).all())
        assert bool((((got * got).sum((0, 2, 3)) - (ref * ref).sum((0, 2, 3))).abs() <= b2).all())


def test_bound_terms():
    S, ref, old = torch.full((3,), 2.0, dtype=torch.float64), torch.tensor([1.0, -1.0, 0.0], dtype=torch.float64), torch.tensor([0.5, 0.5, -4.0])
    b = R.elem_bound(S, 72, ref, "bf16")
    assert torch.equal(b, 80 * R.U24 * S + 2.0 ** -8 * ref.abs())
    ba = R.elem_bound(S, 72, ref, "bf16", old)
    assert torch.equal(ba, 81 * R.U24 * (S + old.double().abs()) + 2.0 ** -8 * ref.abs() + 2.0 ** -8 * (ref + old.double()).abs())
    assert torch.equal(R.elem_bound(S, 72, ref, "f32"), 80 * R.U24 * S + 2.0 ** -23 * ref.abs())
    assert torch.equal(R.wgrad_bound(S, 100), 108 * R.U24 * S)


# ------------------------------------------------------------------------------------------------ the route query (host code: no device)
@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_each_case_takes_the_route_named_for_it(case):
    got = R.routes_of(_lib.lib(), case)
    want = R.expected_of(case)
    assert got == want, {k: (R.FAMILY_NAMES.get(got[k], got[k]), R.FAMILY_NAMES[want[k]]) for k in want if got[k] != want[k]}


def _child_routes(gi):
    group = R.CACHED[gi]
    env = dict(os.environ)
    for k, v in group["env"].items():
        env["CLHIP_" + k] = v
    r = subprocess.run([sys.executable, os.path.join(HERE, "conv_route_worker.py"), str(gi)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ROUTES ")][-1]
    raw = json.loads(line[len("ROUTES "):])
    return {name: {tuple(k.split("/")): fam for k, fam in d.items()} for name, d in raw.items()}


@pytest.fixture(scope="module")
def cached_routes():
    """the routes of the CACHED groups, each asked in a fresh child process with the group's switches in its environment"""
    return [_child_routes(gi) for gi in range(len(R.CACHED))]


@pytest.mark.parametrize("gi", range(len(R.CACHED)), ids=["+".join(g["env"]) for g in R.CACHED])
def test_cached_switch_cases_take_their_routes_in_a_fresh_process(gi, cached_routes):
    for case in R.CACHED[gi]["cases"]:
        assert cached_routes[gi][case["name"]] == R.expected_of(case), case["name"]


def test_the_cases_reach_every_family_of_every_entry_point(cached_routes):
    """a set EQUALITY per entry point: a kernel family without a case fails here, and so does a case on a family the list does not know"""
    L = _lib.lib()
    seen = {op: set() for op in R.FAMILIES}
    for case in R.CASES:
        for (dt, key), fam in R.routes_of(L, case).items():
            seen[R.KEYS[key][0]].add(fam)
    for group, routes in zip(R.CACHED, cached_routes):
        for case in group["cases"]:
            for (dt, key), fam in routes[case["name"]].items():
                seen[R.KEYS[key][0]].add(fam)
    assert seen == R.FAMILIES, {op: (seen[op] ^ R.FAMILIES[op]) for op in seen if seen[op] != R.FAMILIES[op]}
    assert set().union(*R.FAMILIES.values()) == set(R.FAMILY_NAMES) == set(range(1, 24))          # every CLHIP_CONV_* constant of include/clhip.h
    # the binding's constants are the header's and this module's
    import re
    with open(_lib.HEADER_PATH) as f:
        hdr = dict(re.findall(r"#define CLHIP_CONV_([A-Z0-9_]+) (\d+)", f.read()))
    assert len(hdr) == 23 and sorted(int(v) for v in hdr.values()) == list(range(1, 24))
    for name, v in hdr.items():
        assert getattr(_lib, "CONV_" + name) == int(v), name
    assert (R.STEM7, R.CONV9, R.CONV4, R.SHORTCUT, R.W_STEM7, R.W2_DET, R.W_V1_NO_TR) == (_lib.CONV_STEM7, _lib.CONV_CONV9, _lib.CONV_CONV4, _lib.CONV_SHORTCUT,
                                                                                             _lib.CONV_WGRAD_STEM7, _lib.CONV_WGRAD2_DET, _lib.CONV_WGRAD_V1_NO_TR)


@pytest.mark.parametrize("what,args", R.REFUSALS, ids=[r[0] for r in R.REFUSALS])
def test_route_query_refuses_what_the_call_refuses(what, args):
    L = _lib.lib()
    assert L.clhip_conv_route(*args) == -1, what
    assert len(L.clhip_last_error()) > 0


def test_write_through_domain_and_the_conv4_stub():
    L = _lib.lib()
    with R.switches(L, {"BN_INPUT_WT": "1"}):
        for what, args in R.WT_REFUSALS:
            assert L.clhip_conv_route(*args) == -1, what
            assert L.clhip_conv_bn_input_wt_supported(*args[2:6], *args[7:]) == 0, what
        assert L.clhip_conv_route(4, 0, 160, 32, 32, 64, 64, 64, 3, 1, 1, 0) == R.CONV8            # ResNet-18 layer1 at batch 160
        assert L.clhip_conv_bn_input_wt_supported(160, 32, 32, 64, 64, 3, 1, 1, 0) == 1
    assert L.clhip_conv_bn_input_wt_supported(160, 32, 32, 64, 64, 3, 1, 1, 0) == 0


def test_the_calls_refuse_through_the_same_check():
    """the entry points ask the route first: a refused shape never reaches a pointer (none is valid here) or a device"""
    L = _lib.lib()
    assert L.clhip_conv_fwd(1, 1, 1, None, 1, 4, 4, 12, 16, 3, 1, 1, 0, None) == -1
    assert L.clhip_conv_dgrad(1, 1, 1, 0, 2, 8, 8, 32, 48, 3, 1, 1, 0, None) == -1
    assert L.clhip_conv_wgrad(1, 1, 1, None, 2, 16, 16, 8, 3, 16, 7, 2, 3, 0, None) == -1          # the 7x7 stem has no atomic form
    assert L.clhip_conv_dgrad_bn_reduce_supported(3, 8, 8, 64, 64, 3, 2, 1, 0) == 0
    assert L.clhip_conv_dgrad_bn_reduce_supported(3, 8, 8, 64, 64, 3, 1, 1, 0) == 1
