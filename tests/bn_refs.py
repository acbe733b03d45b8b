"""fp64 references, seeded inputs and derived error bounds of csrc/bn.hip (a helper module, not a conftest): BatchNorm2d forward / backward /
eval with residual add and ReLU (nn.BatchNorm2d(momentum=0.1, eps=1e-5), backbone/resnet.py:296-316), the pre-activation residual sum of
ResNet_BIC (resnet.py:589-617), AdaptiveAvgPool2d(1) / AvgPool2d(win) + flatten (:160, :344, :675-676), the NCHW <-> NHWC converts and the
convolution weight shadows.  Plain torch fp64 on the CPU, every formula written out by hand; the project is not imported.
tests/test_bn_refs_cpu.py holds each formula to torch autograd in fp64; tests/test_bn_kernels_gpu.py holds the kernels to them.

Conventions.  Activations are NHWC matrices [M, C] (M = N*H*W) in the storage type ("bf16" / "f32"), quantised BEFORE the oracle sees them.
The statistics entry points receive per-channel sums, so the reference statistics are functions of those sums: mean = s1 / M,
var = max(s2 / M - mean^2, 0), unbiased factor M / (M - 1) and, the project's rule, 1 at M = 1.  eps and momentum are the fp32 values the
C ABI receives.  The backward receives the SAVED fp32 mean / invstd, so its reference is a function of those fp32 values.

Bounds.  u = 2^-24 is the unit roundoff of fp32, r = 2^-8 that of bf16.  Every bound below counts the roundings of the path it covers (the count
stands next to the constant) and is a tensor per element or per channel.  None was fitted to a kernel's output."""
import math

import torch

U = 2.0 ** -24                   # fp32 unit roundoff
U64 = 2.0 ** -53                 # fp64 unit roundoff
R = {"bf16": 2.0 ** -8, "f32": 0.0}                      # storage rounding, relative
FLOOR = {"bf16": 2.0 ** -134, "f32": 2.0 ** -150}        # storage rounding in the subnormal range: half the smallest subnormal
TDT = {"bf16": torch.bfloat16, "f32": torch.float32}
EPS = float(torch.tensor(1e-5, dtype=torch.float32))     # what `float eps` holds
MOM = float(torch.tensor(0.1, dtype=torch.float32))      # what `float momentum` holds
AMBIG_CAP = 1e-4                 # largest share of a case's elements whose ReLU mask may be inside the fp32 noise
ROWS = 1 << 16                   # row block of the blockwise evaluations (keeps the 16.8 M-element case under ~1 GB)

# fp32 roundings between the fp64 variance and invstd, relative:
#   fp64 expression (bn_finalize_kernel, f32 mode of bn_apply_train_kernel): istd = (float)(1 / sqrt(var + eps))            -> 1 rounding = 1 u
#   bf16 mode of bn_apply_train_kernel: rsqrtf((float)var + eps): (float)var and the add each move the argument by u, i.e. invstd by u / 2
#   each (1 u together), rsqrtf is good to 2 ulp = 4 u                                                                       -> 5 u
#   eval (bn_eval_affine_kernel, bn_apply_eval_kernel): 1.f / sqrtf(rv + eps): the add u / 2, sqrtf (correctly rounded) u, the divide u -> 2.5 u
E_ISTD = {"fp64": 1.0, "rsqrt": 5.0, "eval": 2.5}


def istd_kind(entry, dt):
    return "rsqrt" if (entry == "apply_train" and dt == "bf16") else ("eval" if entry == "eval" else "fp64")


def rnd(shape, seed, scale=1.0):
    """fp32 uniform in (-scale, scale), seeded"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def f64(t):
    return t.detach().cpu().double()


def blocks(M):
    return [(a, min(a + ROWS, M)) for a in range(0, M, ROWS)]


# ================================================================================================== closed forms
def unbias_factor(M):
    """nn.BatchNorm2d's M / (M - 1); the project defines 1 at M = 1 (torch refuses a single value per channel in training)"""
    return M / (M - 1.0) if M > 1 else 1.0


def stats_from_sums(s1, s2, M):
    """(mean, biased var, invstd) of a channel from its sum and sum of squares; a negative difference is clamped to 0"""
    mean = s1 / M
    var = (s2 / M - mean * mean).clamp_min(0.0)
    return mean, var, 1.0 / torch.sqrt(var + EPS)


def running_update(old, new, mom=MOM):
    return (1.0 - mom) * old + mom * new


def bn_fwd(z, mean, invstd, gamma, beta, res=None):
    """pre-ReLU output: gamma (z - mean) invstd + beta (+ res), written as z scale + shift like the kernels"""
    scale = gamma * invstd
    y = z * scale + (beta - mean * scale)
    return y if res is None else y + res


def eval_affine(gamma, beta, rm, rv):
    scale = gamma / torch.sqrt(rv + EPS)
    return scale, beta - rm * scale


def relu_mask(ypre):
    """THE mask rule: an element passes the ReLU's gradient iff its pre-ReLU value is > 0 (0 itself does not, as F.relu)"""
    return ypre > 0


def bn_bwd_sums(dy, z, mean, invstd, mask=None):
    """(sum g, sum g xhat, sum |g|, sum |g xhat|) per channel, g = dy masked"""
    g = dy if mask is None else dy * mask
    t = g * ((z - mean) * invstd)
    return g.sum(0), t.sum(0), g.abs().sum(0), t.abs().sum(0)


def bn_bwd_dz(dy, z, mean, invstd, gamma, s1, s2, M, mask=None):
    """dz = gamma invstd (g - mean(g) - xhat mean(g xhat)); dres = g"""
    g = dy if mask is None else dy * mask
    xhat = (z - mean) * invstd
    return gamma * invstd * (g - s1 / M - xhat * (s2 / M)), g


def avgpool_fwd(a):
    """a [N, HW, C] -> [N, C]"""
    return a.sum(1) / a.shape[1]


def avgpool_bwd(dfeat, HW):
    """dfeat [N, C] -> [N, HW, C]"""
    return (dfeat / HW)[:, None, :].expand(dfeat.shape[0], HW, dfeat.shape[1])


def avgpool_win_fwd(a, win):
    """a [N, H, W, C] -> [N, C*Ph*Pw] in the NCHW flatten order, floor rule: rows / columns past Ph*win, Pw*win are not read"""
    N, H, W, C = a.shape
    Ph, Pw = H // win, W // win
    t = a[:, :Ph * win, :Pw * win].reshape(N, Ph, win, Pw, win, C).sum(dim=(2, 4)) / (win * win)          # [N, Ph, Pw, C]
    return t.permute(0, 3, 1, 2).reshape(N, C * Ph * Pw)


def avgpool_win_bwd(dfeat, N, H, W, C, win):
    """dfeat [N, C*Ph*Pw] -> [N, H, W, C]; exactly zero on the uncovered border"""
    Ph, Pw = H // win, W // win
    d = dfeat.reshape(N, C, Ph, Pw).permute(0, 2, 3, 1) / (win * win)                                        # [N, Ph, Pw, C]
    out = torch.zeros(N, H, W, C, dtype=dfeat.dtype)
    out[:, :Ph * win, :Pw * win] = d[:, :, None, :, None, :].expand(N, Ph, win, Pw, win, C).reshape(N, Ph * win, Pw * win, C)
    return out


def nchw_to_nhwc(x, Cpad):
    N, C, H, W = x.shape
    y = torch.zeros(N, H, W, Cpad, dtype=x.dtype)
    y[..., :C] = x.permute(0, 2, 3, 1)
    return y


def nhwc_to_nchw(y):
    return y.permute(0, 3, 1, 2).contiguous()


def weight_prep(w, Cpad):
    """master [K, taps, Creal] -> (w_fwd [K, taps, Cpad] zero-padded, w_dg [Cpad, taps, K] its transpose)"""
    K, taps, Creal = w.shape
    wf = torch.zeros(K, taps, Cpad, dtype=w.dtype)
    wf[..., :Creal] = w
    return wf, wf.permute(2, 1, 0).contiguous()


def add_stored(a, b, dt):
    """what `a += b` stores: the fp32 sum (the fp64 sum of two storage values rounded once to fp32 IS the fp32 sum), rounded to the storage type"""
    return (a.double() + b.double()).float().to(TDT[dt])


def pack_mask(pos):
    """[M, C] bool -> uint8 [M*C/8], bit e of byte i = element 8 i + e"""
    b = pos.reshape(-1, 8).to(torch.int32)
    return (b << torch.arange(8, dtype=torch.int32)).sum(1).to(torch.uint8)


# ================================================================================================== launch geometry (for the sum bounds)
def bwd_chain(M, C, G):
    """longest fp32 addition chain of bn_bwd_reduce_kernel before a value becomes fp64.  G = clhip_bn_bwd_blocks(M, C); rows per
    iteration rpi = 256 / (C / 8); a thread adds ceil(M / (G rpi)) rows; then LDS: narrow layers (2C <= 128) in two steps over
    nparts = 256 / 2C slices, ceil(rpi / nparts) + nparts additions; wide layers serially over the rpi rows"""
    cpr = C // 8
    rpi = 256 // cpr
    rows = -(-M // (G * rpi))
    if 2 * C <= 128:
        nparts = 256 // (2 * C)
        return rows + -(-rpi // nparts) + nparts
    return rows + rpi


def add_stats_chain(M, C, G):
    """add_stats_kernel: ceil(M / (G rpi)) rows per thread, then the rpi rows serially through LDS; G = clhip_add_stats_blocks(M, C)"""
    rpi = 256 // (C // 8)
    return -(-M // (G * rpi)) + rpi


def pool_bn_chain(nchunks, C):
    """avgpool_bwd_bn_kernel: min(1024, ceil(nchunks / 1024)) workgroups (about four chunks per thread, the launcher's rule), grid-stride
    trips per thread, then 256 / (C / 8) threads of a channel group serially through LDS"""
    G = max(1, min(1024, -(-nchunks // 1024)))
    return -(-nchunks // (G * 256)) + max(1, 256 // (C // 8))


# ================================================================================================== bounds
def var_noise(s1, s2, M):
    """absolute fp64 noise of s2 / M - mean^2 on either side (kernel and reference each round 1 / M or the quotients, the square and the
    difference: at most 5 roundings of magnitude <= E[z^2] + mean^2 each) -- it matters only where the variance cancels to ~0"""
    mean = s1 / M
    return 10 * U64 * (s2 / M + mean * mean)


def bound_invstd(invstd, var, noise, kind):
    """per channel: E_ISTD fp32 roundings, plus the fp64 cancellation noise of var carried through 1 / sqrt (d invstd / invstd = dvar / 2 (var + eps))"""
    return invstd.abs() * (E_ISTD[kind] * U + 0.5 * noise / (var + EPS))


def bound_mean(mean):
    return U * mean.abs() + 4 * U64 * mean.abs()          # one fp32 rounding of the fp64 value


def bound_running(old, new, new_noise=0.0, mom=MOM):
    """(1 - m) old + m (float)new in fp32: (1.f - m) u and its product u on the first term; (float)new u and its product u on the second;
    the add u of the result <= u (|first| + |second|) -> 3 u on each term.  new_noise: absolute fp64 noise of `new` (the variance)"""
    return 3 * U * (((1.0 - mom) * old).abs() + (mom * new).abs()) + mom * new_noise


def bound_y(ref, z, mean, invstd, gamma, beta, res, dt, kind, e_extra=0.0):
    """forward y, per element.  Path: sc = fl(gamma istd); sh = fl(beta - fl((float)mean sc)); o = fma(z, sc, sh); o += res.  The SAME sc multiplies z
    and mean, so its error acts on their difference:
      on |(z - mean) scale|: istd E_ISTD, the product gamma istd 1                               = E + 1  (+ e_extra)
      on |z scale|:          fma 1, residual add 1                                               = 2
      on |mean scale|:       (float)mean 1, product 1, subtraction 1, fma 1, add 1               = 5
      on |beta|:             subtraction 1, fma 1, add 1                                         = 3
      on |res|:              add 1                                                               = 1
    each + 1 for the second-order products of these roundings.  The issue's k u (|z scale| + |mean scale| + |beta| + |res|) with k = E + 8 is an upper
    bound of this one (|z - mean| <= |z| + |mean|); the split matters on a constant channel, where z - mean = 0 and the invstd error cancels.
    Eval: the running mean is an exact fp32 input, which only lowers the count.  e_extra: relative fp64 noise of invstd per channel (bound_invstd's
    second term).  Storage: r |x| + the subnormal floor for the fp32 value x, |x| <= |ref| + fp32 part.
    Returns (bound, fp32 part): the second decides which ReLU masks are ambiguous."""
    scale = (gamma * invstd).abs()
    fp = ((E_ISTD[kind] + 2) * U + e_extra) * (z - mean).abs() * scale + 3 * U * z.abs() * scale + 6 * U * mean.abs() * scale + 4 * U * beta.abs()
    if res is not None:
        fp = fp + 2 * U * res.abs()
    fp = fp + FLOOR[dt]
    return R[dt] * ref.abs() + (1 + R[dt]) * fp, fp


def bound_dz(ref, g, xhat, gi, k0, k1, dt, dk0=0.0, dk1=0.0):
    """dz, per element.  Path: gi = fl(gamma istd) 1; xh = fl(fl(z - mu) istd) 2; k0, k1 = (float)(s / M) 1 each;
    t1 = fl(g - k0); p = fl(xh k1); o = fl(gi fl(t1 - p)).
      on |g|:       t1 1, t1 - p 1, final product 1, gi 1                 = 4
      on |k0|:      (float) 1, t1 1, t1 - p 1, product 1, gi 1            = 5
      on |xhat k1|: xh 2, (float)k1 1, p 1, t1 - p 1, product 1, gi 1     = 7
    k = 7 on all three + 1 for second order = 8.  dk0, dk1: per-channel absolute error of the two means the kernel works with (the bound of
    the channel sums / M where the kernel reduced them itself; 0 where the test supplies them in fp64)."""
    mag = gi.abs() * (g.abs() + k0.abs() + (xhat * k1).abs())
    fp = 8 * U * mag + gi.abs() * (dk0 + xhat.abs() * dk1) + FLOOR[dt]
    return R[dt] * ref.abs() + (1 + R[dt]) * fp


def bound_dres_acc(ref, dt):
    """dres accumulated: one fp32 add of two storage values (u) and one storage rounding; dres WRITTEN is exact (a copy of g)"""
    fp = U * ref.abs() + FLOOR[dt]
    return R[dt] * ref.abs() + (1 + R[dt]) * fp


def bound_sum(d, t, sum_abs, ambig_abs=0.0):
    """an fp32 partial sum that becomes fp64: (d + t) u sum |term| for a chain of d additions of terms that carry t roundings each; the fp64
    atomics and the fp64 finalize add <= 2^-40 relative on top (up to 4096 additions at 2^-53).  ambig_abs: sum |term| over the elements whose
    ReLU mask is ambiguous -- either mask value is right there"""
    return (d + t) * U * sum_abs + 4096 * U64 * sum_abs + ambig_abs


def bound_grad_store(old, s, ds):
    """dgamma / dbeta = old + (float)s: the conversion u |s|, the add u |old + s|, on top of the error ds of s itself"""
    return ds + U * s.abs() + U * (old + s).abs() + U * ds


T_SUM1, T_SUM2 = 0, 3            # roundings inside one term: g is exact; g (z - mu) istd is fl(fl(g fl(z - mu)) istd)


def bound_pool_fwd(a_abs_sum, n, ref):
    """mean of n storage values summed serially in fp32 (chain n), then one fp32 division"""
    return n * U * a_abs_sum / n + U * ref.abs()


def bound_pool_bwd(ref, dt):
    """dfeat * fl(1 / n): the reciprocal u, the product u, then storage"""
    fp = 2 * U * ref.abs() + FLOOR[dt]
    return R[dt] * ref.abs() + (1 + R[dt]) * fp


# ================================================================================================== comparison
def err_ratio(got, ref, bound, alt=None, ambig=None):
    """max over elements of |got - ref| / bound; on the `ambig` elements the smaller of the errors against ref and alt counts.
    A NaN or an infinity anywhere in `got` is an infinite ratio."""
    got, ref = f64(got).reshape(ref.shape), ref.double()
    err = (got - ref).abs()
    if ambig is not None and bool(ambig.any()):
        err = torch.where(ambig, torch.minimum(err, (got - alt.double()).abs()), err)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    if err.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    q = err / bound
    q = torch.where(err == 0, torch.zeros_like(q), q)          # 0 / 0 at an exact element with a zero bound
    return float("inf") if bool(torch.isnan(q).any()) else float(q.max())


RATIOS = {}                      # (entry, dt) -> worst ratio seen in this process


def check(entry, dt, what, got, ref, bound, alt=None, ambig=None):
    q = err_ratio(got, ref, bound, alt, ambig)
    RATIOS[(entry, dt)] = max(RATIOS.get((entry, dt), 0.0), q)
    print(f"[ratio] {entry} {dt} {what}: {q:.3g}")
    assert q <= 1.0, (entry, dt, what, q)
    return q


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    w = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.view(w), b.view(w))


# ================================================================================================== cases
class Case:
    """Seeded inputs of one geometry and storage type, and its references, each computed once (blockwise in fp64) and kept.
    z uniform in +-spread plus a per-channel offset, gamma about 1, beta in +-0.2 (the density of |y| near 0 is then ~0.1 per unit, and the
    fp32 part of the forward bound ~1e-6: an ambiguous share near 1e-6).  `const` = {channel: value} makes channels constant."""

    def __init__(self, M, C, dt, seed=0, spread=2.0, offset=0.3, const=None, gamma=None, beta=None):
        self.M, self.C, self.dt = M, C, dt
        q = TDT[dt]
        off = rnd((C,), seed + 9, 0.5) + offset
        z = rnd((M, C), seed, spread) + off
        for c, v in (const or {}).items():
            z[:, c] = v
        self.z = z.to(q)
        del z
        self.res = rnd((M, C), seed + 1).to(q)
        self.dy = rnd((M, C), seed + 2).to(q)
        self.dres0 = rnd((M, C), seed + 3, 0.5).to(q)
        self.gamma = (rnd((C,), seed + 4, 0.5) + 1.0) if gamma is None else gamma.float().clone()
        self.beta = rnd((C,), seed + 5, 0.2) if beta is None else beta.float().clone()
        self.rm0, self.rv0 = rnd((C,), seed + 6, 0.1), rnd((C,), seed + 7).abs() + 0.5
        self.dg0, self.db0 = rnd((C,), seed + 8, 3.0), rnd((C,), seed + 10, 3.0)
        s1, s2 = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
        for a, b in blocks(M):
            zb = self.z[a:b].double()
            s1 += zb.sum(0)
            s2 += (zb * zb).sum(0)
        self.set_sums(s1, s2)
        self._cache = {}

    def set_sums(self, s1, s2):
        """the statistics the entry points are GIVEN (fp64 sums, or the fp64 total of fp32 partials)"""
        self.s1, self.s2 = s1.double().clone(), s2.double().clone()
        self.mean, self.var, self.invstd = stats_from_sums(self.s1, self.s2, self.M)
        self.noise = var_noise(self.s1, self.s2, self.M)
        self.mean32, self.invstd32 = self.mean.float(), self.invstd.float()          # what the forward saves for the backward
        self._cache = {}

    def split(self, rep, seed=100):
        """[rep, 2, C] fp64 whose sum over the replicas is (s1, s2) to ~1e-16, split unevenly (weights of either sign)"""
        w = rnd((rep,), seed).double() + 0.3
        w[-1] = 1.0 - w[:-1].sum()
        return w[:, None, None] * torch.stack([self.s1, self.s2])[None]

    # ---- forward
    def ypre(self, res):
        key = ("ypre", bool(res))
        if key not in self._cache:
            g, b = self.gamma.double(), self.beta.double()
            out = torch.empty(self.M, self.C, dtype=torch.float64)
            for a, e in blocks(self.M):
                out[a:e] = bn_fwd(self.z[a:e].double(), self.mean, self.invstd, g, b, self.res[a:e].double() if res else None)
            self._cache[key] = out
        return self._cache[key]

    def y_check(self, entry, what, got, res, relu, kind):
        """device y [M, C] (storage type) against relu?(ypre) under bound_y, by row blocks; returns the worst ratio"""
        g, b = self.gamma.double(), self.beta.double()
        ex = 0.5 * self.noise / (self.var + EPS)
        yp = self.ypre(res)
        worst = 0.0
        got = got.detach().cpu().reshape(self.M, self.C)
        for a, e in blocks(self.M):
            ref = yp[a:e].clamp_min(0.0) if relu else yp[a:e]
            bd, _ = bound_y(ref, self.z[a:e].double(), self.mean, self.invstd, g, b, self.res[a:e].double() if res else None, self.dt, kind, ex)
            worst = max(worst, err_ratio(got[a:e], ref, bd))
        RATIOS[(entry, self.dt)] = max(RATIOS.get((entry, self.dt), 0.0), worst)
        print(f"[ratio] {entry} {self.dt} {what}: {worst:.3g}")
        assert worst <= 1.0, (entry, self.dt, what, worst)
        return worst

    def ambiguous(self, res, kind="rsqrt"):
        """[M, C] bool: |ypre| no larger than the fp32 part of the forward bound (the widest of the forward kinds unless told otherwise)"""
        key = ("ambig", bool(res), kind)
        if key not in self._cache:
            g, b = self.gamma.double(), self.beta.double()
            ex = 0.5 * self.noise / (self.var + EPS)
            yp = self.ypre(res)
            out = torch.empty(self.M, self.C, dtype=torch.bool)
            for a, e in blocks(self.M):
                _, fp = bound_y(yp[a:e], self.z[a:e].double(), self.mean, self.invstd, g, b, self.res[a:e].double() if res else None, self.dt, kind, ex)
                out[a:e] = yp[a:e].abs() <= fp
            self._cache[key] = out
        return self._cache[key]

    def y_stored(self, res, relu):
        """the reference output rounded to the storage type: the y a backward test hands to the kernels"""
        key = ("ystored", bool(res), bool(relu))
        if key not in self._cache:
            yp = self.ypre(res)
            self._cache[key] = (yp.clamp_min(0.0) if relu else yp).float().to(TDT[self.dt])
        return self._cache[key]

    # ---- backward (functions of the saved fp32 statistics)
    def bwd(self, res, relu):
        """dict: s1, s2 (channel sums), a1, a2 (sums of |term|), m1, m2 (sums of |term| over the ambiguous elements), n_ambig"""
        key = ("bwd", bool(res), bool(relu))
        if key not in self._cache:
            mu, is_ = self.mean32.double(), self.invstd32.double()
            acc = [torch.zeros(self.C, dtype=torch.float64) for _ in range(6)]
            n_amb = 0
            for a, e in blocks(self.M):
                dy, z = self.dy[a:e].double(), self.z[a:e].double()
                mask = relu_mask(self.ypre(res)[a:e]) if relu else None
                for i, v in enumerate(bn_bwd_sums(dy, z, mu, is_, mask)):
                    acc[i] += v
                if relu:
                    amb = self.ambiguous(res)[a:e]
                    if bool(amb.any()):
                        n_amb += int(amb.sum())
                        t = dy * ((z - mu) * is_)
                        acc[4] += (dy.abs() * amb).sum(0)
                        acc[5] += (t.abs() * amb).sum(0)
            self._cache[key] = dict(s1=acc[0], s2=acc[1], a1=acc[2], a2=acc[3], m1=acc[4], m2=acc[5], n_ambig=n_amb)
        return self._cache[key]

    def sum_bounds(self, res, relu, d):
        """(bound of sum g, bound of sum g xhat) for a reduction of chain length d"""
        b = self.bwd(res, relu)
        return bound_sum(d, T_SUM1, b["a1"], b["m1"]), bound_sum(d, T_SUM2, b["a2"], b["m2"])

    def dz_check(self, entry, what, got_dz, got_dres, res, relu, dres_mode, ds=(0.0, 0.0)):
        """device dz (and dres: mode 1 written, 2 accumulated onto dres0) against the reference, by row blocks.  ds: the absolute error bounds of the
        two channel sums the kernel worked with"""
        b = self.bwd(res, relu)
        mu, is_, g64 = self.mean32.double(), self.invstd32.double(), self.gamma.double()
        gi = g64 * is_
        k0, k1 = b["s1"] / self.M, b["s2"] / self.M
        dk0, dk1 = ds[0] / self.M, ds[1] / self.M
        worst = [0.0, 0.0]
        got_dz = got_dz.detach().cpu().reshape(self.M, self.C)
        got_dres = None if got_dres is None else got_dres.detach().cpu().reshape(self.M, self.C)
        for a, e in blocks(self.M):
            dy, z = self.dy[a:e].double(), self.z[a:e].double()
            mask = relu_mask(self.ypre(res)[a:e]) if relu else None
            amb = self.ambiguous(res)[a:e] if relu else None
            ref, g = bn_bwd_dz(dy, z, mu, is_, g64, b["s1"], b["s2"], self.M, mask)
            alt = alt_g = None
            if relu and bool(amb.any()):
                alt, alt_g = bn_bwd_dz(dy, z, mu, is_, g64, b["s1"], b["s2"], self.M, mask ^ amb)
            xhat = (z - mu) * is_
            has_alt = alt is not None
            gmag = torch.where(amb, dy.abs(), g.abs()) if has_alt else g.abs()          # an ambiguous element: the bound of the unmasked gradient
            bd = bound_dz(ref, gmag, xhat, gi, k0, k1, self.dt, dk0, dk1)
            worst[0] = max(worst[0], err_ratio(got_dz[a:e], ref, bd, alt, amb if has_alt else None))
            if dres_mode == 1:                                                          # a copy of g: exact
                gd = got_dres[a:e].double()
                exact = (gd == g) | (((gd == alt_g) & amb) if has_alt else False)
                worst[1] = max(worst[1], 0.0 if bool(exact.all()) else float("inf"))
            elif dres_mode == 2:
                r0 = self.dres0[a:e].double()
                mag = (r0 + g).abs()
                if has_alt:
                    mag = torch.where(amb, torch.maximum(mag, (r0 + alt_g).abs()), mag)
                worst[1] = max(worst[1], err_ratio(got_dres[a:e], r0 + g, bound_dres_acc(mag, self.dt),
                                                   r0 + alt_g if has_alt else None, amb if has_alt else None))
        for i, nm in enumerate(("dz", "dres")):
            if i == 1 and dres_mode == 0:
                continue
            RATIOS[(entry, self.dt)] = max(RATIOS.get((entry, self.dt), 0.0), worst[i])
            print(f"[ratio] {entry} {self.dt} {what} {nm}: {worst[i]:.3g}")
            assert worst[i] <= 1.0, (entry, self.dt, what, nm, worst[i])

    def ambiguous_share(self, res):
        return float(self.ambiguous(res).sum()) / (self.M * self.C)


# the GPU matrix (tests/test_bn_kernels_gpu.py); the CPU test walks the same list for the ambiguity cap
GEOMS_POW2 = [
    (1, 8, "M1_unbias_C8_single_chunk"), (2, 16, "single_chunk"),
    (75, 64, "narrow_finalize_rpi32_ragged"), (75, 128, "wide_finalize_rpi16_ragged"), (12, 2048, "widest_rpi1"), (37, 1024, "wide_rpi2_ragged"),
    (777, 8, "narrow_C8_all_thread_lds"), (1000, 32, "narrow_C32_all_thread_lds"),
    (32771, 64, "262168_chunks_partial_first_trip"), (81925, 64, "655400_chunks_second_trip_bwd_iters8"),
]
GEOM_BIG = (262154, 64, "2097232_chunks_second_grid_stride_bwd_cap1024")          # bf16 only, reduced forms
GEOMS_NP2 = [(75, 24, "np2_C24_nparts5"), (50, 40, "np2_C40_nparts3"), (9, 1000, "np2_C1000_wide")]

_CASES = {}


def case(M, C, dt):
    """the one Case of a geometry and type in this process"""
    if (M, C, dt) not in _CASES:
        _CASES[(M, C, dt)] = Case(M, C, dt, seed=1000 + 7 * C + M % 97)
    return _CASES[(M, C, dt)]


def drop_case(M, C, dt):
    _CASES.pop((M, C, dt), None)
