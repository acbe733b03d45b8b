"""Runs the cases of tests/conv_ref.py on the GPU and judges every element against the fp64 reference and its bound (a helper of
tests/test_conv_routes_gpu.py and of its child processes, not a test).  Every call returns {what: largest err / bound}; a value above 1, a NaN
left in an output or a touched guard element is a failure of the caller's assertion."""
import torch

import conv_ref as R
from libcontinual_amd import _lib
from libcontinual_amd._lib import call

DEV = "cuda"
DT = {"bf16": (_lib.BF16, torch.bfloat16), "f32": (_lib.F32, torch.float32)}
GUARD = 64


def st():
    return torch.cuda.current_stream().cuda_stream


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def nhwc(t, tdt, cpad=None):
    """NCHW fp32 (already rounded) -> device NHWC in tdt, channels zero-padded to cpad"""
    n, c, h, w = t.shape
    y = torch.zeros(n, h, w, cpad or c)
    y[..., :c] = t.permute(0, 2, 3, 1)
    return y.to(tdt).to(DEV).contiguous()


def nchw64(t):
    return t.double().permute(0, 3, 1, 2)


class Guarded:
    """a device buffer with GUARD sentinel elements behind it, the payload filled with `fill` (NaN: every element must be written)"""
    def __init__(self, shape, dtype, fill):
        n = 1
        for d in shape:
            n *= d
        self.n, self.shape = n, shape
        self.sentinel = 3 if dtype == torch.uint8 else 7.0
        self.buf = torch.full((n + GUARD,), self.sentinel, dtype=dtype, device=DEV)
        if isinstance(fill, torch.Tensor):
            self.buf[:n] = fill.reshape(-1)
        else:
            self.buf[:n] = fill
        self.t = self.buf[:n].view(shape)

    def ptr(self):
        return self.buf.data_ptr()

    def guard_ok(self):
        return bool((self.buf[self.n:] == self.sentinel).all())


def ratio(got, ref, bound):
    """largest |got - ref| / bound over all elements; inf for a NaN or an error where the bound is 0"""
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    r = torch.nan_to_num(r, nan=float("inf"))
    return float(r.max())


class Operands:
    def __init__(self, case, dt, seed=0):
        N, H, W, C, K, k, s, p = case["shape"]
        self.case, self.dt = case, dt
        self.code, self.tdt = DT[dt]
        cr = case["creal"]
        self.Ho, self.Wo = R.out_hw(H, W, k, s, p)
        q = lambda t: t.to(self.tdt).float()
        self.x = q(rnd((N, cr, H, W), seed + 1))
        self.w = q(rnd((K, cr, k, k), seed + 2, 1.0 / (cr * k * k) ** 0.5))
        self.dz = q(rnd((N, K, self.Ho, self.Wo), seed + 3))
        self.wb = q(rnd((K, cr, k, k), seed + 4, 1.0 / (K * k * k) ** 0.5))          # the dgrad's weight
        self.xd = nhwc(self.x, self.tdt, C)
        wk = torch.zeros(K, k, k, C)
        wk[..., :cr] = self.w.permute(0, 2, 3, 1)
        self.wfd = wk.to(self.tdt).to(DEV).contiguous()
        self.dzd = nhwc(self.dz, self.tdt)
        self.wdg = self.wb.permute(1, 2, 3, 0).contiguous().to(self.tdt).to(DEV)      # [C][R][S][K]
        self._fwd = self._dg = self._wg = None

    def dims(self):
        return self.case["shape"]

    def fwd_ref(self):
        if self._fwd is None:
            _, _, _, _, _, k, s, p = self.dims()
            self._fwd = R.conv_fwd_ref(self.x.to(DEV), self.w.to(DEV), s, p)
        return self._fwd

    def dgrad_ref(self):
        if self._dg is None:
            N, H, W, C, K, k, s, p = self.dims()
            self._dg = R.conv_dgrad_ref(self.dz.to(DEV), self.wb.to(DEV), s, p, H, W)
        return self._dg

    def wgrad_ref(self):
        if self._wg is None:
            _, _, _, _, _, k, s, p = self.dims()
            self._wg = R.conv_wgrad_ref(self.x.to(DEV), self.dz.to(DEV), k, s, p)
        return self._wg


def _stats(ref, b, s1, s2):
    b1, b2 = R.stat_bounds(ref, b)
    return ratio(s1, ref.sum((0, 2, 3)), b1), ratio(s2, (ref * ref).sum((0, 2, 3)), b2)


def _conv9_replicas(o, ref, b, acc, rep):
    """conv9.hip: pixel tile t (256 consecutive pixels at 128 channels, 128 at 256) adds into replica t & (rep - 1) -- each replica against the fp64 sums of
    ITS tiles, so an addend in another replica shows although the sum over the replicas does not change"""
    N, H, W, C, K, k, s, p = o.dims()
    tp = 256 // (C // 128)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, tp, K)                   # [tile][pixel][channel]
    r_t, b_t = rows(ref), rows(b)
    worst = 0.0
    for r in range(rep):
        mine = r_t[r::rep]
        if mine.shape[0] == 0:
            assert float(acc[r].abs().max()) == 0.0
            continue
        bm = b_t[r::rep]
        worst = max(worst, ratio(acc[r, 0], mine.sum((0, 1)), bm.sum((0, 1)) + R.REL64 * mine.abs().sum((0, 1))),
                    ratio(acc[r, 1], (mine * mine).sum((0, 1)), (2 * mine.abs() * bm + bm * bm).sum((0, 1)) + R.REL64 * (mine * mine).sum((0, 1))))
    return worst


def run_fwd(L, o, form, fam=None):
    """form 0: no statistics; 1: partial rows; 2: the fp64 accumulators with 1 and 8 replicas"""
    N, H, W, C, K, k, s, p = o.dims()
    ref, S = o.fwd_ref()
    Rn = k * k * o.case["creal"]
    bound = R.elem_bound(S, Rn, ref, o.dt)
    out = {}
    if form == 0:
        z = Guarded((N, o.Ho, o.Wo, K), o.tdt, float("nan"))
        call("clhip_conv_fwd", o.xd.data_ptr(), o.wfd.data_ptr(), z.ptr(), None, N, H, W, C, K, k, s, p, o.code, st())
        torch.cuda.synchronize()
        assert z.guard_ok()
        out["z"] = ratio(nchw64(z.t), ref, bound)
    elif form == 1:
        tiles = L.clhip_conv_fwd_tiles(N, H, W, C, K, k, s, p)
        assert tiles > 0
        z = Guarded((N, o.Ho, o.Wo, K), o.tdt, float("nan"))
        part = Guarded((tiles, 2, K), torch.float32, float("nan"))
        call("clhip_conv_fwd", o.xd.data_ptr(), o.wfd.data_ptr(), z.ptr(), part.ptr(), N, H, W, C, K, k, s, p, o.code, st())
        torch.cuda.synchronize()
        assert z.guard_ok() and part.guard_ok()
        out["z"] = ratio(nchw64(z.t), ref, bound)
        out["s1"], out["s2"] = _stats(ref, R.acc_bound(S, Rn), part.t[:, 0].double().sum(0), part.t[:, 1].double().sum(0))
    else:
        for rep in (1, 8):
            z = Guarded((N, o.Ho, o.Wo, K), o.tdt, float("nan"))
            acc = Guarded((rep, 2, K), torch.float64, 0.0)
            call("clhip_conv_fwd_acc", o.xd.data_ptr(), o.wfd.data_ptr(), z.ptr(), acc.ptr(), rep, N, H, W, C, K, k, s, p, o.code, st())
            torch.cuda.synchronize()
            assert z.guard_ok() and acc.guard_ok()
            out[f"z/rep{rep}"] = ratio(nchw64(z.t), ref, bound)
            out[f"s1/rep{rep}"], out[f"s2/rep{rep}"] = _stats(ref, R.acc_bound(S, Rn), acc.t[:, 0].sum(0), acc.t[:, 1].sum(0))
            if fam == R.CONV9:
                out[f"each replica/rep{rep}"] = _conv9_replicas(o, ref, R.acc_bound(S, Rn), acc.t, rep)
    return out


def _old(o, seed=9):
    N, H, W, C, K, k, s, p = o.dims()
    return rnd((N, C, H, W), seed, 0.5).to(o.tdt).float()


def run_dgrad(L, o):
    """accumulate 0 into a NaN-filled buffer, accumulate 1 onto earlier content"""
    N, H, W, C, K, k, s, p = o.dims()
    ref, S = o.dgrad_ref()
    Rn = k * k * K
    out = {}
    dx = Guarded((N, H, W, C), o.tdt, float("nan"))
    call("clhip_conv_dgrad", o.dzd.data_ptr(), o.wdg.data_ptr(), dx.ptr(), 0, N, H, W, C, K, k, s, p, o.code, st())
    torch.cuda.synchronize()
    assert dx.guard_ok()
    out["dx"] = ratio(nchw64(dx.t), ref, R.elem_bound(S, Rn, ref, o.dt))
    old = _old(o)
    dx = Guarded((N, H, W, C), o.tdt, nhwc(old, o.tdt))
    call("clhip_conv_dgrad", o.dzd.data_ptr(), o.wdg.data_ptr(), dx.ptr(), 1, N, H, W, C, K, k, s, p, o.code, st())
    torch.cuda.synchronize()
    assert dx.guard_ok()
    oldd = old.to(DEV)
    out["dx+="] = ratio(nchw64(dx.t), ref + oldd.double(), R.elem_bound(S, Rn, ref, o.dt, oldd))
    return out


def run_wgrad(L, o, form, fam):
    """into zeros, += onto earlier content, and (where the kernel uses the scratch: every family but the atomic ones) once more for the same bits"""
    N, H, W, C, K, k, s, p = o.dims()
    cr = o.case["creal"]
    ref, S = o.wgrad_ref()                                     # [K, cr, k, k]
    Rn = N * o.Ho * o.Wo
    wsb = int(L.clhip_conv_wgrad_ws_bytes(N, H, W, C, cr, K, k, s, p, o.code)) if form == 1 else 0
    ws = Guarded((max(wsb, 16),), torch.uint8, 0x7F) if form == 1 else None          # (no zeroed scratch)

    def launch(dw):
        call("clhip_conv_wgrad", o.xd.data_ptr(), o.dzd.data_ptr(), dw.ptr(), ws.ptr() if ws else None, N, H, W, C, cr, K, k, s, p, o.code, st())
        torch.cuda.synchronize()
        assert dw.guard_ok() and (ws is None or ws.guard_ok())
        return dw.t.double().permute(0, 3, 1, 2)

    out = {}
    d0 = Guarded((K, k, k, cr), torch.float32, 0.0)
    out["dw"] = ratio(launch(d0), ref, R.wgrad_bound(S, Rn))
    old = rnd((K, cr, k, k), 10, 0.5)
    d1 = Guarded((K, k, k, cr), torch.float32, old.permute(0, 2, 3, 1).contiguous().to(DEV))
    oldd = old.to(DEV)
    out["dw+="] = ratio(launch(d1), ref + oldd.double(), R.wgrad_bound(S, Rn, oldd))
    if form == 1 and fam not in (R.W2_ATOMIC, R.W_V1, R.W_V1_NO_TR):
        d2 = Guarded((K, k, k, cr), torch.float32, 0.0)
        launch(d2)
        assert torch.equal(d2.t, d0.t), "the weight gradient with scratch is not bitwise repeatable"
    return out


def run_bnr(L, o):
    """clhip_conv_dgrad_bn_reduce: dx (bit for bit the plain dgrad's where that runs on the same kernel) and the producer's BatchNorm-backward sums, accumulate 0 / 1, 1 and 8 replicas"""
    N, H, W, C, K, k, s, p = o.dims()
    ref, S = o.dgrad_ref()
    Rn = k * k * K
    zp = (rnd((N, C, H, W), 21, 1.5) + 0.2).to(o.tdt).float()
    yp = torch.relu(rnd((N, C, H, W), 22)).to(o.tdt).float()
    mean, invstd = rnd((C,), 23) * 0.3, rnd((C,), 24).abs() + 0.5
    zpd, ypd, md, isd = nhwc(zp, o.tdt), nhwc(yp, o.tdt), mean.to(DEV), invstd.to(DEV)
    mask = (yp > 0).double().to(DEV)
    xhat = (zp.double().to(DEV) - mean.double().to(DEV).view(1, C, 1, 1)) * invstd.double().to(DEV).view(1, C, 1, 1)
    same_kernel = R.query(L, o.case, o.dt, "dgrad") == R.query(L, o.case, o.dt, "bnr")      # (conv5.hip has no such epilogue: its layers reduce on conv4.hip)
    out = {}
    for accumulate, rep in ((0, 1), (1, 8), (0, 8)):
        old = _old(o) if accumulate else None
        oldd = old.to(DEV) if accumulate else None
        total = ref + oldd.double() if accumulate else ref
        fill = nhwc(old, o.tdt) if accumulate else float("nan")
        dx, dxp = Guarded((N, H, W, C), o.tdt, fill), Guarded((N, H, W, C), o.tdt, fill)
        acc = Guarded((rep, 2, C), torch.float64, 0.0)
        call("clhip_conv_dgrad_bn_reduce", o.dzd.data_ptr(), o.wdg.data_ptr(), dx.ptr(), accumulate, zpd.data_ptr(), ypd.data_ptr(), md.data_ptr(), isd.data_ptr(),
             acc.ptr(), rep, N, H, W, C, K, k, s, p, o.code, st())
        call("clhip_conv_dgrad", o.dzd.data_ptr(), o.wdg.data_ptr(), dxp.ptr(), accumulate, N, H, W, C, K, k, s, p, o.code, st())
        torch.cuda.synchronize()
        assert dx.guard_ok() and acc.guard_ok()
        tag = f"acc{accumulate}/rep{rep}"
        if same_kernel:
            assert torch.equal(dx.t, dxp.t), f"{tag}: dx differs from the plain dgrad's"
        out[f"dx/{tag}"] = ratio(nchw64(dx.t), total, R.elem_bound(S, Rn, ref, o.dt, oldd))
        b = R.acc_bound(S, Rn, oldd) * mask
        g = total * mask
        b1, _ = R.stat_bounds(g, b)
        bx, _ = R.stat_bounds(g, b, weight=xhat.abs())
        sums = acc.t.sum(0)
        out[f"sum g/{tag}"] = ratio(sums[0], g.sum((0, 2, 3)), b1)
        out[f"sum g xhat/{tag}"] = ratio(sums[1], (g * xhat).sum((0, 2, 3)), bx)
    return out


def run_wt(L, o):
    """clhip_conv_fwd_acc_bn_input_wt without and with the residual: bit for bit clhip_bn_apply_train[_mask] + clhip_conv_fwd_acc (the property and the code of
    tests/test_kernels_gpu.py), and the convolution of the activation the launch wrote against fp64"""
    import ctypes as C_

    import test_kernels_gpu as TK

    class BnInput(C_.Structure):
        _fields_ = [("stat_acc", C_.c_void_p), ("replicas", C_.c_int), ("gamma", C_.c_void_p), ("beta", C_.c_void_p), ("running_mean", C_.c_void_p),
                    ("running_var", C_.c_void_p), ("momentum", C_.c_float), ("eps", C_.c_float), ("mean", C_.c_void_p), ("invstd", C_.c_void_p), ("coef", C_.c_void_p)]

    class BnRes(C_.Structure):
        _fields_ = [("res", C_.c_void_p), ("y", C_.c_void_p), ("relu_mask", C_.c_void_p)]
    N, H, W, C, K, k, s, p = o.dims()
    out = {}
    for with_res in (False, True):
        l, w = TK._wt_case(L, C_, BnInput, BnRes, N, H, W, C, K, o.code, o.tdt, with_res)
        y = l["y"][:N * H * W].view(N, H, W, C).permute(0, 3, 1, 2)                       # the operand as the kernel formed (and wrote) it
        ref, S = R.conv_fwd_ref(y, w.view(K, 3, 3, C).permute(0, 3, 1, 2), 1, 1)
        tag = "res" if with_res else "plain"
        out[f"z/{tag}"] = ratio(nchw64(l["z"]), ref, R.elem_bound(S, 9 * C, ref, o.dt))
        out[f"s1/{tag}"], out[f"s2/{tag}"] = _stats(ref, R.acc_bound(S, 9 * C), l["acc"][:, 0].sum(0), l["acc"][:, 1].sum(0))
    return out


def run_key(L, o, key, fam):
    if key.startswith("fwd"):
        return run_fwd(L, o, int(key[3]), fam)
    if key == "dgrad":
        return run_dgrad(L, o)
    if key.startswith("wgrad"):
        return run_wgrad(L, o, int(key[5]), fam)
    if key == "bnr":
        return run_bnr(L, o)
    return run_wt(L, o)


def run_case(L, case, measure=None):
    """every call the case names, in both modes: the route is asserted before each launch.  Returns {(dt, key, what): err / bound}"""
    res = {}
    with R.switches(L, case["sw"]):
        for dt in ("bf16", "f32"):
            if not case["routes"][dt]:
                continue
            o = Operands(case, dt)
            for key, fam in case["routes"][dt].items():
                got = R.query(L, case, dt, key)
                assert got == fam, (case["name"], dt, key, R.FAMILY_NAMES.get(got, got), R.FAMILY_NAMES[fam])
                for what, r in run_key(L, o, key, fam).items():
                    res[(dt, key, what)] = r
                    print(f"[ratio] {case['name']} {dt} {key} {R.FAMILY_NAMES[fam]} {what} {r:.4g}")
                    if measure is not None:
                        m = measure.setdefault(R.FAMILY_NAMES[fam], (0.0, ""))
                        if r > m[0]:
                            measure[R.FAMILY_NAMES[fam]] = (r, f"{case['name']} {dt} {key} {what}")
    return res
