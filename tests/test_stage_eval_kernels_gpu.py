"""The stage-level eval forward (csrc/stage.hip) on its own, through clhip_stage_eval, held to the two references of tests/stage_ref.py on a real MI355X:
  * routing, BIT-EQUAL: the exact integer chain at all three geometries the kernel admits, nconv = 2 .. 16, N = 1, 3 and 257 (one workgroup per image; 257 is one
    more than the chip's 256 CUs, so a workgroup starts after another has retired), the N = 257 run a second time into a fresh buffer;
  * fp64 links: N = 3, L = 16, all 8 blocks times the three runs (first-of-block probe, second-of-block probe, the real block) per geometry, max over ALL elements
    of err / bound <= 1; the stored input of block k is the output of the prefix run of length 2k - 2 (stage_ref's docstring states the assumption);
  * refusals: CLHIP_EINVAL from the entry, 0 from the query, the output buffer untouched.
In-process: the direct entry reads no switch.  No test provokes a fault: every pointer passed is valid and sized.  The weight copies are made with
clhip_conv_weight_prep, so a plan and these tests hold the same bits.  `[ratio]` lines as in test_plan_units_gpu.py (pytest -s); profiles/stage_eval.md holds the
table of an MI355X run."""
import ctypes
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import bn_refs as B                        # noqa: E402
import stage_ref as SR                     # noqa: E402
from libcontinual_amd import _lib          # noqa: E402

DEV = "cuda:0"
EINVAL = -1
GEOM_IDS = [f"C{c}-H{h}" for c, h in SR.GEOMS]
MEASURE = {}
_PREP = {}


def st():
    return torch.cuda.current_stream().cuda_stream


def dev_params(c):
    """device copies of one convolution's parameters, made once: the bf16 [C][9][C] forward copy through clhip_conv_weight_prep, the four fp32 BatchNorm arrays"""
    ent = _PREP.get(id(c))
    if ent is None:
        C = c["w"].shape[0]
        master = c["w"].float().permute(0, 2, 3, 1).reshape(C, 9, C).contiguous().to(DEV)
        wf = torch.empty(C, 9, C, dtype=torch.bfloat16, device=DEV)
        _lib.call("clhip_conv_weight_prep", master.data_ptr(), wf.data_ptr(), None, C, 9, C, C, _lib.BF16, st())
        ent = (c, wf) + tuple(c[k].float().contiguous().to(DEV) for k in ("gamma", "beta", "mean", "var"))
        _PREP[id(c)] = ent                 # (holds c: its id stays unique)
    return ent[1:]


def tables(convs, n):
    cols = list(zip(*[dev_params(c) for c in convs[:n]]))
    return [(ctypes.c_void_p * n)(*[t.data_ptr() for t in col]) for col in cols], cols


def nhwc(x):
    """NCHW fp64 (bf16 values) -> the kernel's [N][H][W][C] bf16"""
    return x.to(DEV).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


def launch(xd, convs, nconv):
    """y [N][H][W][C] bf16 of a run of the first nconv convolutions of `convs` on xd; the buffer is fresh and pre-filled with NaN patterns"""
    N, H, W, C = xd.shape
    y = torch.full_like(xd, float("nan"))
    tabs, keep = tables(convs, nconv)
    _lib.call("clhip_stage_eval", xd.data_ptr(), y.data_ptr(), N, H, W, C, nconv, *tabs, B.EPS, _lib.BF16, st())
    torch.cuda.synchronize()
    del keep
    return y


def as_nchw(y):
    return y.double().permute(0, 3, 1, 2)


@pytest.fixture(scope="module", autouse=True)
def measure_table():
    yield
    for name, (worst, secs) in MEASURE.items():
        print(f"\n[measure] {name:28s} " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()) + f"   {secs:.1f} s", end="")
    print()


@pytest.mark.parametrize("N", [1, 3, 257])
@pytest.mark.parametrize("geom", SR.GEOMS, ids=GEOM_IDS)
def test_routing_bit_equal(geom, N):
    C, H = geom
    t0 = time.time()
    assert all(_lib.lib().clhip_stage_eval_supported(H, H, C, n, _lib.BF16) == 1 for n in range(2, 17, 2))
    E = SR.exact_case(C, H, N, SR.EXACT_SEEDS[C], dev=DEV)
    xd = nhwc(E["x"])
    wrong = []
    for nconv in range(2, 17, 2):
        got, want = launch(xd, E["convs"], nconv), nhwc(E["outs"][nconv // 2 - 1])
        if not B.same_bits(got, want):
            d = (got.double() != want.double()) | ~torch.isfinite(got.double())
            wrong.append((nconv, int(d.sum()), [tuple(i) for i in d.nonzero()[:4].tolist()]))
    assert wrong == [], f"(nconv, differing elements, first [n, y, x, c] indices): {wrong}"
    if N == 257:
        assert B.same_bits(launch(xd, E["convs"], 16), nhwc(E["outs"][-1]))
    MEASURE[f"routing C{C}-H{H} N{N}"] = ({"bit-equal": 1.0}, time.time() - t0)


@pytest.mark.parametrize("geom", SR.GEOMS, ids=GEOM_IDS)
def test_links_against_fp64(geom):
    C, H = geom
    t0 = time.time()
    Lc = SR.link_case(C, H, 3, SR.LINK_SEEDS[C], dev=DEV)
    x, convs = Lc["x"], Lc["convs"]
    xd = nhwc(x)
    stored = [as_nchw(launch(xd, convs, 2 * k)) for k in range(1, 9)]          # the prefix runs: stored[k - 1] = the input of block k + 1, and block k's real output
    worst, bad = {}, []
    for k in range(1, 9):
        xin = x if k == 1 else stored[k - 2]
        r = {}
        for kind in SR.KINDS:
            got = stored[k - 1] if kind == "real" else as_nchw(launch(xd, SR.probe_convs(convs, k, kind), 2 * k))
            r[kind] = SR.judge_link(kind, xin, convs, k, got)
            worst[kind] = max(worst.get(kind, 0.0), r[kind])
            if not r[kind] <= 1.0:
                bad.append((k, kind, r[kind]))
        print(f"[ratio] stage_eval C{C}-H{H} block {k} " + " ".join(f"{kind}={v:.3g}" for kind, v in r.items()))
    MEASURE[f"links C{C}-H{H}"] = (worst, time.time() - t0)
    assert bad == [], f"links outside their bound (block, kind, err / bound): {bad}"


# (what, N, H, W, C, nconv, dtype); the query has no N, so the last case has no query to ask
REFUSALS = [("nconv 3", 3, 32, 32, 16, 3, _lib.BF16), ("nconv 15", 3, 16, 16, 32, 15, _lib.BF16), ("nconv 0", 3, 8, 8, 64, 0, _lib.BF16), ("nconv 18", 3, 32, 32, 16, 18, _lib.BF16),
            ("fp32", 3, 32, 32, 16, 4, _lib.F32), ("H != W", 3, 32, 16, 16, 4, _lib.BF16), ("(C, H) = (16, 16)", 3, 16, 16, 16, 4, _lib.BF16), ("N = 0", 0, 32, 32, 16, 4, _lib.BF16)]


def test_refusals_leave_the_output_untouched():
    L = _lib.lib()
    convs = [SR.ident(64) for _ in range(2)] * 9               # 18 valid rows of the widest geometry: no table is too short for any case
    tabs, keep = tables(convs, 18)
    n = 3 * 32 * 32 * 64                                       # more than any case could touch
    xd = torch.ones(n, dtype=torch.bfloat16, device=DEV)
    y = torch.full((n,), 7.5, dtype=torch.bfloat16, device=DEV)
    pattern = y.clone()
    for what, N, H, W, C, nconv, dt in REFUSALS:
        if N > 0:
            assert L.clhip_stage_eval_supported(H, W, C, nconv, dt) == 0, what
        rc = L.clhip_stage_eval(xd.data_ptr(), y.data_ptr(), N, H, W, C, nconv, *tabs, B.EPS, dt, st())
        assert rc == EINVAL, (what, rc)
        assert L.clhip_last_error()
    torch.cuda.synchronize()
    assert B.same_bits(y, pattern)
    del keep
