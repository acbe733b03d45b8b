// rapf.hip -- the adapter step of RAPF (reference core/model/rapf.py): the class-Gaussian draws that stand in for old data (sample(), :37-44, as called
// from :318-322 and :328-334), the adapter + normalisation + CLIP logits + cross entropy + hinge of one step (:143-153, :341-353) with the gradient
// at the adapter's output, and the adapter's weight gradient.  The rules are those of rp.hip and ca.hip: fp32 in / fp32 accumulate, the three
// matrix-shaped products on v_mfma_f32_32x32x2_f32 through the operand staging of rp_tile.h, no atomics, every summation order a function of the
// shapes only (two calls give the same bits), ragged edges the normal case, every output WRITTEN.
//
// One tile body (tile_product) serves the three products:
//   draw : X[row0 + r] = mean[cls] + Z[r] L[cls]^T, one row tile per 128 rows of a GROUP (a class and a count, chosen by the host per step; the table
//          travels in the kernel arguments, so nothing is copied or synchronised).  L is lower triangular: the K loop of a column tile stops at its
//          last column and fetch_lower never reads above the diagonal, as in ca_sample.
//   A    : A = X W^T (W in nn.Linear layout: both operands k-contiguous), written into the `n` output ...
//   rows : ... which one workgroup per row then normalises in place, forms the logits, the softmax, the row's loss term and G = dloss/dA: the whole
//          loss is known here, so the backward is one product ...
//   dW   : dW = g G^T X (both operands k-major, k = the row), the rows in ascending order inside ONE workgroup per tile: R is a few hundred, no slabs.
// A fourth, one-workgroup launch adds the row terms in a fixed order (loss_c, loss_h, the correct count); the inference form stops after `rows`.
#include "rp_tile.h"

using namespace rp_tile;

namespace {

constexpr int kMaxGroups = 128;         // groups per draw launch (the table is a kernel argument: 1 KB)
constexpr int kRowMaxFloats = 8192;     // 2 E + C floats of LDS per row workgroup (32 KB at the limit)

struct DrawGroups {
    int n;
    int cls[kMaxGroups];
    int cnt[kMaxGroups];
};

// acc += a(i0.., k) b(j0.., k) over k in [0, K): rp.hip's loop.  A is k-major or k-contiguous; B likewise, or LOWER (k-contiguous, row j read up to k = j)
template <bool A_KMAJOR, bool B_KMAJOR, bool LOWER>
__device__ __forceinline__ void tile_product(const float* __restrict__ a, size_t lda, bool avec, int I, int i0, const float* __restrict__ b, size_t ldb, bool bvec,
                                             int J, int j0, int K, float* As, float* Bs, f32x16 (&acc)[2][2]) {
    using OA = Operand<A_KMAJOR>;
    using OB = Operand<B_KMAJOR>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    const int lr = lane & 31, lk = lane >> 5;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][q][r] = 0.f;
    float4 ra[2], rb[2];
    OA::fetch(a, lda, I, K, i0, 0, avec, ra);
    if (LOWER) fetch_lower(b, ldb, J, K, j0, 0, bvec, rb);
    else OB::fetch(b, ldb, J, K, j0, 0, bvec, rb);
    for (int k0 = 0; k0 < K; k0 += kBK) {
        __syncthreads();
        OA::stash(As, ra);
        OB::stash(Bs, rb);
        __syncthreads();
        if (k0 + kBK < K) {
            OA::fetch(a, lda, I, K, i0, k0 + kBK, avec, ra);
            if (LOWER) fetch_lower(b, ldb, J, K, j0, k0 + kBK, bvec, rb);
            else OB::fetch(b, ldb, J, K, j0, k0 + kBK, bvec, rb);
        }
#pragma unroll
        for (int s = 0; s < kBK / 2; ++s) {
            const int k = 2 * s + lk;
            float av[2], bv[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) av[m] = As[k * OA::LD + wi + m * 32 + lr];
#pragma unroll
            for (int q = 0; q < 2; ++q) bv[q] = Bs[k * OB::LD + wj + q * 32 + lr];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int q = 0; q < 2; ++q) acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[q], acc[m][q], 0, 0, 0);
        }
    }
}

// out[(i, j)] = alpha * acc + (bias ? bias[j] : 0) for the tile at (i0, j0) of an I x J matrix.
// C/D map of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
__device__ __forceinline__ void tile_store(const f32x16 (&acc)[2][2], float* __restrict__ out, size_t ldo, int I, int J, int i0, int j0, float alpha,
                                           const float* __restrict__ bias) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    const int lr = lane & 31, lk = lane >> 5;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int j = j0 + wj + q * 32 + lr;
            if (j >= J) continue;
            const float loc = bias ? bias[j] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = i0 + wi + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (i >= I) continue;
                out[(size_t)i * ldo + j] = bias ? loc + acc[m][q][r] : alpha * acc[m][q][r];
            }
        }
}

// blockIdx = (column tile, row tile over all groups of this launch).  Z and X point at the first row of the launch's first group.
__global__ __launch_bounds__(kThreads) void rapf_draw_kernel(const float* __restrict__ mean, const float* __restrict__ chol, const float* __restrict__ Z,
                                                              float* __restrict__ X, int E, int vec, const DrawGroups G) {
    using O = Operand<false>;
    __shared__ __attribute__((aligned(16))) float As[kBK * O::LD];
    __shared__ __attribute__((aligned(16))) float Bs[kBK * O::LD];
    int t = blockIdx.y, g = 0, row = 0;
    while (g < G.n - 1 && t >= (G.cnt[g] + kTile - 1) / kTile) {      // (the host sized the grid: t lands inside group g)
        t -= (G.cnt[g] + kTile - 1) / kTile;
        row += G.cnt[g];
        ++g;
    }
    const int cnt = G.cnt[g];
    const size_t c = (size_t)G.cls[g];
    const int i0 = t * kTile, j0 = blockIdx.x * kTile;
    const int kend = min(E, j0 + kTile);               // the K blocks past the tile's last column lie wholly above the diagonal
    f32x16 acc[2][2];
    tile_product<false, false, true>(Z + (size_t)row * E, (size_t)E, vec != 0, cnt, i0, chol + c * E * E, (size_t)E, vec != 0, E, j0, kend, As, Bs, acc);
    tile_store(acc, X + (size_t)row * E, (size_t)E, cnt, E, i0, j0, 1.f, mean + c * E);
}

// out [I, J] = alpha * a b^T-or-so: the plain product of the step.  NT: a [I, K] and b [J, K] k-contiguous (A = X W^T); TN: a [K, I] and b [K, J] k-major (G^T X)
template <bool KMAJOR>
__global__ __launch_bounds__(kThreads) void rapf_gemm_kernel(const float* __restrict__ a, size_t lda, int avec, const float* __restrict__ b, size_t ldb, int bvec,
                                                              float* __restrict__ out, size_t ldo, int I, int J, int K, float alpha) {
    using O = Operand<KMAJOR>;
    __shared__ __attribute__((aligned(16))) float As[kBK * O::LD];
    __shared__ __attribute__((aligned(16))) float Bs[kBK * O::LD];
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    f32x16 acc[2][2];
    tile_product<KMAJOR, KMAJOR, false>(a, lda, avec != 0, I, i0, b, ldb, bvec != 0, J, j0, K, As, Bs, acc);
    tile_store(acc, out, ldo, I, J, i0, j0, alpha, nullptr);
}

// (value, index) of the first maximum over the workgroup; every thread brings its own candidate (index 0x7fffffff: none)
__device__ __forceinline__ void block_argmax_256(float& bv, int& bi, float* redv, int* redi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { redv[threadIdx.x >> 6] = bv; redi[threadIdx.x >> 6] = bi; }
    __syncthreads();
    bv = redv[0]; bi = redi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (redv[w] > bv || (redv[w] == bv && redi[w] < bi)) { bv = redv[w]; bi = redi[w]; }
}

// One workgroup per row r of nbuf [R, E], which holds A = X W^T on entry and n = A / |A| on exit.
//   r <  nce (= B + M): logits[r] = scale n . T^T; with labels: row_loss[r] = CE, pred[r] (r < B), G[r] from (softmax - onehot) scale / nce
//   r >= nce (edge row q = r - nce): pre = -n . T[pos[q]] + n . T[neg[q]] + margin, row_loss[r] = relu(pre), G[r] from 1[pre > 0] (T[neg] - T[pos]) / Q
// G[r] = (g_n - n (n . g_n)) / |A_r|.  labels == nullptr: the inference form, logits and n only.
__global__ __launch_bounds__(256) void rapf_row_kernel(float* __restrict__ nbuf, const float* __restrict__ T, const int64_t* __restrict__ labels,
                                                        const int64_t* __restrict__ pos, const int64_t* __restrict__ neg, float scale, float margin,
                                                        float* __restrict__ logits, float* __restrict__ G, float* __restrict__ row_loss,
                                                        int64_t* __restrict__ pred, int B, int nce, int Q, int E, int C) {
    extern __shared__ float lds[];
    float* n = lds;                 // [E]
    float* gn = lds + E;            // [E]
    float* lg = lds + 2 * E;        // [C]
    __shared__ float red[4];
    __shared__ int redi[4];
    const int r = blockIdx.x, t = threadIdx.x, lane = t & 63;
    float* nr = nbuf + (size_t)r * E;
    float ss = 0.f;
    for (int e = t; e < E; e += 256) {
        const float a = nr[e];
        n[e] = a;
        ss = fmaf(a, a, ss);
    }
    ss = block_sum_256(ss, red);
    const float inv = 1.0f / sqrtf(ss);      // no eps, as in the reference: a zero row gives inf / NaN and is the caller's problem
    for (int e = t; e < E; e += 256) {
        const float v = n[e] * inv;
        n[e] = v;
        nr[e] = v;
    }
    __syncthreads();
    const bool train = labels != nullptr;
    if (r < nce) {
        for (int c = t >> 6; c < C; c += 4) {
            float a = 0.f;
            for (int e = lane; e < E; e += 64) a = fmaf(n[e], T[(size_t)c * E + e], a);
            a = wave_sum(a);
            if (lane == 0) {
                lg[c] = scale * a;
                logits[(size_t)r * C + c] = scale * a;
            }
        }
        if (!train) return;
        __syncthreads();
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int c = t; c < C; c += 256)
            if (lg[c] > bv) { bv = lg[c]; bi = c; }
        block_argmax_256(bv, bi, red, redi);      // the first maximum: also the softmax's shift
        float se = 0.f;
        for (int c = t; c < C; c += 256) se += expf(lg[c] - bv);
        se = block_sum_256(se, red);
        const float lse = bv + logf(se);
        const int64_t y = labels[r];
        const bool in = y >= 0 && y < C;          // clhip_ce_slice's convention: a label outside the columns gives no loss term and no onehot
        if (t == 0) {
            row_loss[r] = in ? lse - lg[y] : 0.f;
            if (r < B) pred[r] = bi;
        }
        __syncthreads();                          // every read of lg[y] and of the logits is done
        const float sc = scale / (float)nce;
        for (int c = t; c < C; c += 256) lg[c] = sc * (expf(lg[c] - lse) - (c == y ? 1.f : 0.f));
        __syncthreads();
        for (int e = t; e < E; e += 256) {
            float a = 0.f;
            for (int c = 0; c < C; ++c) a = fmaf(lg[c], T[(size_t)c * E + e], a);
            gn[e] = a;
        }
    } else {
        if (!train) return;
        const int q = r - nce;
        const int64_t p = pos[q], m = neg[q];
        const bool ok = p >= 0 && p < C && m >= 0 && m < C;      // a pair outside the text rows is inactive: no loss term, no gradient
        float dp = 0.f, dm = 0.f;
        if (ok)
            for (int e = t; e < E; e += 256) {
                dp = fmaf(n[e], T[(size_t)p * E + e], dp);
                dm = fmaf(n[e], T[(size_t)m * E + e], dm);
            }
        dp = block_sum_256(dp, red);
        dm = block_sum_256(dm, red);
        const float pre = (-dp + dm) + margin;
        const bool on = ok && pre > 0.f;                         // relu'(0) = 0, as torch
        if (t == 0) row_loss[r] = on ? pre : 0.f;
        const float w = 1.0f / (float)Q;
        for (int e = t; e < E; e += 256) gn[e] = on ? w * (T[(size_t)m * E + e] - T[(size_t)p * E + e]) : 0.f;
    }
    float ng = 0.f;
    for (int e = t; e < E; e += 256) ng = fmaf(n[e], gn[e], ng);      // (each thread reads the gn it wrote)
    ng = block_sum_256(ng, red);
    for (int e = t; e < E; e += 256) G[(size_t)r * E + e] = (gn[e] - n[e] * ng) * inv;
}

// loss[1] = mean of the CE terms, loss[2] = mean of the hinge terms (0 without edge rows), loss[0] = their sum, correct = #(pred == label) over the
// image rows: thread t adds rows t, t + 256, ... in order, then the butterfly and the four waves in order
__global__ __launch_bounds__(256) void rapf_finish_kernel(const float* __restrict__ row_loss, const int64_t* __restrict__ pred, const int64_t* __restrict__ labels,
                                                           float* __restrict__ loss, int32_t* __restrict__ correct, int B, int nce, int Q) {
    __shared__ float red[4];
    const int t = threadIdx.x;
    float sc = 0.f, sh = 0.f, ok = 0.f;
    for (int r = t; r < nce; r += 256) sc += row_loss[r];
    for (int r = t; r < Q; r += 256) sh += row_loss[nce + r];
    for (int r = t; r < B; r += 256) ok += pred[r] == labels[r] ? 1.f : 0.f;      // (B < 2^24: exact)
    sc = block_sum_256(sc, red);
    sh = block_sum_256(sh, red);
    ok = block_sum_256(ok, red);
    if (t == 0) {
        const float lc = sc / (float)nce, lh = Q > 0 ? sh / (float)Q : 0.f;
        loss[0] = Q > 0 ? lc + lh : lc;
        loss[1] = lc;
        loss[2] = lh;
        if (correct) *correct = (int32_t)ok;
    }
}

}  // namespace

extern "C" int clhip_rapf_draw(const float* mean, const float* chol, const float* Z, float* X, const int32_t* cls, const int32_t* cnt, int G, int Cs, int E,
                               int row0, void* stream) {
    CLHIP_CHECK_ARG(mean && chol && Z && X && cls && cnt && G >= 1 && Cs >= 1 && E >= 1 && row0 >= 0);
    long long rows = 0;
    for (int g = 0; g < G; ++g) {
        if (cls[g] < 0 || cls[g] >= Cs || cnt[g] < 1) {
            clhip_set_error("clhip_rapf_draw: invalid argument: group %d draws %d rows of class %d; %d classes are stored", g, cnt[g], cls[g], Cs);
            return CLHIP_EINVAL;
        }
        rows += cnt[g];
    }
    CLHIP_CHECK_ARG(row0 + rows <= 0x7fffffffLL);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // chol and Z share the pitch E, and a class or a row starts a multiple of E floats in: one alignment test serves all of them
    const int vec = vec_ok(Z, E) && vec_ok(chol, E);
    size_t row = 0;
    for (int g0 = 0; g0 < G; g0 += kMaxGroups) {
        DrawGroups dg;
        dg.n = min(kMaxGroups, G - g0);
        long long nt = 0, nr = 0;
        for (int g = 0; g < dg.n; ++g) {
            dg.cls[g] = cls[g0 + g];
            dg.cnt[g] = cnt[g0 + g];
            nt += tiles(cnt[g0 + g]);
            nr += cnt[g0 + g];
        }
        for (int g = dg.n; g < kMaxGroups; ++g) dg.cls[g] = dg.cnt[g] = 0;
        CLHIP_CHECK_ARG(nt <= 65535);
        rapf_draw_kernel<<<dim3(tiles(E), (unsigned)nt, 1), kThreads, 0, st>>>(mean, chol, Z + row * E, X + ((size_t)row0 + row) * E, E, vec, dg);
        CLHIP_LAUNCH_CHECK();
        row += (size_t)nr;
    }
    return CLHIP_OK;
}

extern "C" int clhip_rapf_step_fwd(const float* X, const float* W, const float* T, const int64_t* labels, const int64_t* pos, const int64_t* neg, float scale,
                                   float margin, float* logits, float* n, float* G, float* row_loss, float* loss, int64_t* pred, int32_t* correct, int B, int M,
                                   int Q, int E, int C, void* stream) {
    CLHIP_CHECK_ARG(X && W && T && logits && n && B >= 1 && M >= 0 && Q >= 0 && E >= 1 && C >= 1);
    CLHIP_CHECK_ARG((long long)B + M + Q <= 0x7fffffLL && 2LL * E + C <= kRowMaxFloats);
    if (labels) CLHIP_CHECK_ARG(G && row_loss && loss && pred && (Q == 0 || (pos && neg)));
    else CLHIP_CHECK_ARG(M == 0 && Q == 0);                     // the inference form
    const int R = B + M + Q;
    CLHIP_CHECK_ARG(tiles(R) <= 65535);
    hipStream_t st = static_cast<hipStream_t>(stream);
    rapf_gemm_kernel<false><<<dim3(tiles(E), tiles(R), 1), kThreads, 0, st>>>(X, (size_t)E, vec_ok(X, E), W, (size_t)E, vec_ok(W, E), n, (size_t)E, R, E, E, 1.f);
    CLHIP_LAUNCH_CHECK();
    rapf_row_kernel<<<dim3(R), dim3(256), (size_t)(2 * E + C) * sizeof(float), st>>>(n, T, labels, pos, neg, scale, margin, logits, G, row_loss, pred, B, B + M, Q,
                                                                                     E, C);
    CLHIP_LAUNCH_CHECK();
    if (labels) {
        rapf_finish_kernel<<<1, 256, 0, st>>>(row_loss, pred, labels, loss, correct, B, B + M, Q);
        CLHIP_LAUNCH_CHECK();
    }
    return CLHIP_OK;
}

extern "C" int clhip_rapf_step_bwd(const float* G, const float* X, float g, float* dW, int R, int E, void* stream) {
    CLHIP_CHECK_ARG(G && X && dW && R >= 1 && E >= 1 && tiles(E) <= 65535);
    const int vec = vec_ok(G, E) && vec_ok(X, E);
    rapf_gemm_kernel<true><<<dim3(tiles(E), tiles(E), 1), kThreads, 0, static_cast<hipStream_t>(stream)>>>(G, (size_t)E, vec, X, (size_t)E, vec, dW, (size_t)E, E, E,
                                                                                                           R, g);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}
