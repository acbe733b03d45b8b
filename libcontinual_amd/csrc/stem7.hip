// stem7.hip -- the ImageNet stem of the reference ResNets (core/model/backbone/resnet.py:136-149): conv1 = Conv2d(3, 64, 7, stride 2,
// pad 3) -> BatchNorm -> ReLU -> MaxPool2d(3, stride 2, pad 1), gfx950.
//
//  * forward, bf16: v_mfma_f32_16x16x32_bf16 with the reduction index = (tap, channel) exactly as in stem.hip: one K step is four taps x
//    the 8 padded channels, so the B operand of a lane (pixel = lane & 15, tap = 4 ks + (lane >> 4)) is ONE 16-byte load of that
//    pixel's input neighbour; 49 taps -> 13 K steps (taps 49..51 multiply zeros).  Packing the 21 real (kx, c) pairs of a kernel row
//    densely (7 K steps) would halve the MFMAs, but every operand would become a 6-byte gather that straddles pixels; the stem is
//    bound by its loads and stores, not by its 13 MFMAs per 16 pixels and 16 output channels.  The weights (64 x 49 x 8 bf16 = 50 KB)
//    do not fit in registers: each workgroup stages them in LDS once (53-tap pitch: 16 lanes of a ds_read_b128 cover all 64 banks);
//    the BatchNorm sums come from the fp32 accumulators into the plan's replicated fp64 accumulators like stem.hip.
//  * weight gradient, bf16: wgrad_stem_kernel's scheme (stem.hip) per kernel ROW: a workgroup (split, ky) walks 32-pixel steps, im2col
//    rows of the 7 taps of row ky (+ one zero slot) and the gradient rows go into wave-private LDS tiles, both operands come back
//    through transposing reads; partial blocks [split][K][49][Creal] are summed in a fixed order by wgrad3_reduce_kernel: deterministic.
//  * fp32 parity mode: plain per-thread kernels for both (the same statistics / partial-block contracts).
//  * BatchNorm + ReLU + 3x3 / s2 / p1 max-pool, fused: each thread reads its window of z once (8 channels), applies the BatchNorm of the
//    batch statistics (training: from the accumulators, like bn_apply_train_kernel) or of the running statistics (eval), and writes the
//    pooled value and the window position of the maximum (first maximum in row-major order, padding never wins: torch's `val > maxval`).
//  * max-pool backward as a gather: each stem pixel sums the <= 4 pooled gradients whose argmax points at it (fixed order, no atomics),
//    applies the ReLU mask (recomputed from z with the forward's scale / shift) and accumulates the two BatchNorm-backward sums.
#include <stdlib.h>

#include "kernels.h"

namespace {

constexpr int kTaps = 49, kSteps = 13, kPitch = 53;     // taps, K steps of four taps, LDS pitch in taps (16 bytes each)

struct Stem7Params {
    const void* x;       // [N,H,W,8]
    const void* w;       // [K][49][8]
    void* z;             // [N,Ho,Wo,K]
    double* acc;         // [rep][2][K] or nullptr
    int rep;
    int N, H, W, Ho, Wo, K, M;
};

template <int KT>
__global__ __launch_bounds__(256) void conv_stem7_kernel(const Stem7Params p) {
    extern __shared__ __attribute__((aligned(16))) char wsm[];          // [KT*16][kPitch][16 B]
    __shared__ float red[4][2][KT * 16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const bf16_t* x = static_cast<const bf16_t*>(p.x);
    const bf16_t* w = static_cast<const bf16_t*>(p.w);
    for (int i = tid; i < KT * 16 * kPitch; i += 256) {
        const int o = i / kPitch, t = i - o * kPitch;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (t < kTaps) v = *reinterpret_cast<const uint4*>(w + ((size_t)o * kTaps + t) * 8);
        *reinterpret_cast<uint4*>(wsm + (size_t)i * 16) = v;
    }
    __syncthreads();
    int ky[kSteps], kx[kSteps];
#pragma unroll
    for (int ks = 0; ks < kSteps; ++ks) { const int tap = 4 * ks + g; ky[ks] = tap < kTaps ? tap / 7 : 99; kx[ks] = tap % 7; }
    float s1[KT][4], s2[KT][4];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int e = 0; e < 4; ++e) { s1[kt][e] = 0.f; s2[kt][e] = 0.f; }
    const int H = p.H, W = p.W, HWo = p.Ho * p.Wo;
    const int ntile = (p.M + 15) / 16;                        // 16 output pixels per wave and iteration
    for (int tile = blockIdx.x * 4 + wave; tile < ntile; tile += gridDim.x * 4) {
        const int px = tile * 16 + l15;
        const bool valid = px < p.M;
        const int n = px / HWo, r = px - n * HWo, ho = r / p.Wo, wo = r - ho * p.Wo;
        const int h0 = 2 * ho - 3, w0 = 2 * wo - 3;
        bf16x8_t b[kSteps];
#pragma unroll
        for (int ks = 0; ks < kSteps; ++ks) {
            const int hh = h0 + ky[ks], ww = w0 + kx[ks];
            uint4 v = make_uint4(0, 0, 0, 0);
            if (valid && ky[ks] < 7 && (unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W)
                v = *reinterpret_cast<const uint4*>(x + (((size_t)n * H + hh) * W + ww) * 8);
            b[ks] = __builtin_bit_cast(bf16x8_t, v);
        }
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
            const char* arow = wsm + (size_t)(kt * 16 + l15) * kPitch * 16 + g * 16;
#pragma unroll
            for (int ks = 0; ks < kSteps; ++ks) {
                const bf16x8_t a = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(arow + ks * 64));
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[ks], c, 0, 0, 0);
            }
            if (valid)
                *reinterpret_cast<uint2*>(static_cast<bf16_t*>(p.z) + (size_t)px * p.K + kt * 16 + 4 * g) = make_uint2(pack_bf16x2(c[0], c[1]), pack_bf16x2(c[2], c[3]));
#pragma unroll
            for (int e = 0; e < 4; ++e) { s1[kt][e] += c[e]; s2[kt][e] = fmaf(c[e], c[e], s2[kt][e]); }     // pixels behind M multiplied zeros
        }
    }
    if (p.acc == nullptr) return;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
        float v[8] = {s1[kt][0], s1[kt][1], s1[kt][2], s1[kt][3], s2[kt][0], s2[kt][1], s2[kt][2], s2[kt][3]};
        row16_sum_n(v);
        if (l15 == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { red[wave][0][kt * 16 + 4 * g + e] = v[e]; red[wave][1][kt * 16 + 4 * g + e] = v[4 + e]; }
        }
    }
    __syncthreads();
    for (int i = tid; i < 2 * KT * 16; i += 256) {
        const int which = i / (KT * 16), ch = i - which * (KT * 16);
        const float t = red[0][which][ch] + red[1][which][ch] + red[2][which][ch] + red[3][which][ch];
        atomicAdd(p.acc + ((size_t)(blockIdx.x & (p.rep - 1)) * 2 + which) * p.K + ch, (double)t);
    }
}

// fp32 parity mode: one thread = one output pixel x 8 output channels (the thread's channel group is fixed: the grid stride is a multiple of K / 8)
__global__ __launch_bounds__(256) void conv_stem7_f32_kernel(const Stem7Params p) {
    __shared__ float red[256][17];
    const float* x = static_cast<const float*>(p.x);
    const float* w = static_cast<const float*>(p.w);
    const int cpp = p.K / 8, HWo = p.Ho * p.Wo;
    const int64_t nchunks = (int64_t)p.M * cpp, stride = (int64_t)gridDim.x * blockDim.x;
    float s[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nchunks; i += stride) {
        const int px = (int)(i / cpp), o0 = (int)(i - (int64_t)px * cpp) * 8;
        const int n = px / HWo, r = px - n * HWo, ho = r / p.Wo, wo = r - ho * p.Wo;
        float a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0.f;
        for (int ky = 0; ky < 7; ++ky) {
            const int hh = 2 * ho - 3 + ky;
            if ((unsigned)hh >= (unsigned)p.H) continue;
            for (int kx = 0; kx < 7; ++kx) {
                const int ww = 2 * wo - 3 + kx;
                if ((unsigned)ww >= (unsigned)p.W) continue;
                float xv[8];
                load8<float>(x + (((size_t)n * p.H + hh) * p.W + ww) * 8, xv);
                const int tap = ky * 7 + kx;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float wv[8];
                    load8<float>(w + ((size_t)(o0 + e) * kTaps + tap) * 8, wv);
#pragma unroll
                    for (int c = 0; c < 8; ++c) a[e] = fmaf(wv[c], xv[c], a[e]);
                }
            }
        }
        store8<float>(static_cast<float*>(p.z) + (size_t)px * p.K + o0, a);
#pragma unroll
        for (int e = 0; e < 8; ++e) { s[e] += a[e]; s[8 + e] = fmaf(a[e], a[e], s[8 + e]); }
    }
    if (p.acc == nullptr) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) red[threadIdx.x][e] = s[e];
    __syncthreads();
    for (int c = threadIdx.x; c < p.K; c += 256) {
        const int grp = c >> 3, e = c & 7;
        float a1 = 0.f, a2 = 0.f;
        for (int t = grp; t < 256; t += cpp) { a1 += red[t][e]; a2 += red[t][8 + e]; }
        double* acc = p.acc + (size_t)(blockIdx.x & (p.rep - 1)) * 2 * p.K;
        atomicAdd(acc + c, (double)a1);
        atomicAdd(acc + p.K + c, (double)a2);
    }
}

// ------------------------------------------------------------------------------------------------------------ weight gradient
struct Stem7WParams { const void* x; const void* dz; float* slab; int N, H, W, Ho, Wo, K, M, Creal, nstep; };

// grid (splits, 7): workgroup (s, ky) accumulates dw[o][ky][kx][c] over the 32-pixel steps s * 4 + wave, + 4 splits, ...
template <int KT>
__global__ __launch_bounds__(256) void wgrad_stem7_kernel(const Stem7WParams p) {
    constexpr int PZ = KT * 32 + 16, PX = 144;               // LDS pitches: gradient row (16 KT channels), im2col row (8 x 16 B + pad)
    constexpr int WAVE_LDS = 32 * PZ + 32 * PX;
    constexpr int RED = KT * 16 * 64 * 4;
    __shared__ __attribute__((aligned(16))) char smem[4 * WAVE_LDS > RED ? 4 * WAVE_LDS : RED];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int H = p.H, W = p.W, K = p.K, HWo = p.Ho * p.Wo, ky = blockIdx.y;
    const bf16_t* x = static_cast<const bf16_t*>(p.x);
    const bf16_t* dzp = static_cast<const bf16_t*>(p.dz);
    char* zs = smem + wave * WAVE_LDS;
    char* xs = zs + 32 * PZ;
    if (lane < 32) *reinterpret_cast<uint4*>(xs + lane * PX + 112) = make_uint4(0, 0, 0, 0);      // the eighth tap slot stays zero
    f32x4 acc[KT][4];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[kt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int col = fg * 8 + (fr >> 2), seg = (fr & 3) * 8;
    const int gw = blockIdx.x * 4 + wave, nw = gridDim.x * 4;
    uint4 zr[KT], xr[4];
    auto fetch = [&](int s) {
        const int p0 = s * 32;
#pragma unroll
        for (int i = 0; i < KT; ++i) {
            const int id = lane + 64 * i, px = id / (2 * KT), part = id - px * (2 * KT);
            zr[i] = make_uint4(0, 0, 0, 0);
            if (p0 + px < p.M) zr[i] = *reinterpret_cast<const uint4*>(dzp + (size_t)(p0 + px) * K + part * 8);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int id = lane + 64 * i;
            xr[i] = make_uint4(0, 0, 0, 0);
            if (id < 224) {
                const int px = id / 7, kx = id - px * 7, gp = p0 + px;
                const int n = gp / HWo, r = gp - n * HWo, ho = r / p.Wo, wo = r - ho * p.Wo;
                const int hh = 2 * ho - 3 + ky, ww = 2 * wo - 3 + kx;
                if (gp < p.M && (unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W)
                    xr[i] = *reinterpret_cast<const uint4*>(x + (((size_t)n * H + hh) * W + ww) * 8);
            }
        }
    };
    if (gw < p.nstep) fetch(gw);
    for (int s = gw; s < p.nstep; s += nw) {
#pragma unroll
        for (int i = 0; i < KT; ++i) {
            const int id = lane + 64 * i, px = id / (2 * KT), part = id - px * (2 * KT);
            *reinterpret_cast<uint4*>(zs + px * PZ + part * 16) = zr[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int id = lane + 64 * i;
            if (id < 224) { const int px = id / 7, kx = id - px * 7; *reinterpret_cast<uint4*>(xs + px * PX + kx * 16) = xr[i]; }
        }
        if (s + nw < p.nstep) fetch(s + nw);
        bf16x8_t zf[KT], xf[4];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) zf[kt] = tr8b(zs, col * PZ + kt * 32 + seg, 4 * PZ);
#pragma unroll
        for (int j = 0; j < 4; ++j) xf[j] = tr8b(xs, col * PX + j * 32 + seg, 4 * PX);
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[kt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(zf[kt], xf[j], acc[kt][j], 0, 0, 0);
        __builtin_amdgcn_s_waitcnt(0xC07F);                  // the tiles are overwritten by the next step's stores
    }
    // D[row = out channel 4 fg + e][col = 16 j + fr = (kx 2 j + fr / 8, channel fr % 8)] -> red[o][64], the four waves in a fixed order
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float* q = red + (kt * 16 + fg * 4 + e) * 64 + j * 16 + fr;
                        *q = w == 0 ? acc[kt][j][e] : *q + acc[kt][j][e];
                    }
        }
        __syncthreads();
    }
    float* out = p.slab + (size_t)blockIdx.x * K * kTaps * p.Creal;
    for (int i = tid; i < K * 7 * p.Creal; i += 256) {
        const int c = i % p.Creal, kx = (i / p.Creal) % 7, o = i / (p.Creal * 7);
        out[((size_t)o * kTaps + ky * 7 + kx) * p.Creal + c] = red[o * 64 + kx * 8 + c];
    }
}

// fp32 parity mode: workgroup (split, o), a thread = (tap, channel) entries j, j + 256, ... (49 * Creal is up to 392), each over its pixels in order
__global__ __launch_bounds__(256) void wgrad_stem7_f32_kernel(const Stem7WParams p, int pps) {
    const float* x = static_cast<const float*>(p.x);
    const float* dz = static_cast<const float*>(p.dz);
    const int o = blockIdx.y, HWo = p.Ho * p.Wo;
    const int g0 = blockIdx.x * pps, g1 = min(p.M, g0 + pps);
    for (int j = threadIdx.x; j < kTaps * p.Creal; j += blockDim.x) {
        const int tap = j / p.Creal, c = j - tap * p.Creal, ky = tap / 7, kx = tap % 7;
        float a = 0.f;
        for (int gp = g0; gp < g1; ++gp) {
            const int n = gp / HWo, r = gp - n * HWo, ho = r / p.Wo, wo = r - ho * p.Wo;
            const int hh = 2 * ho - 3 + ky, ww = 2 * wo - 3 + kx;
            if ((unsigned)hh < (unsigned)p.H && (unsigned)ww < (unsigned)p.W)
                a = fmaf(dz[(size_t)gp * p.K + o], x[(((size_t)n * p.H + hh) * p.W + ww) * 8 + c], a);
        }
        p.slab[((size_t)blockIdx.x * p.K + o) * kTaps * p.Creal + j] = a;
    }
}

int stem7_fwd_grid(int M) {
    const int ntile = (M + 15) / 16;
    int grid = (ntile + 15) / 16;                            // >= 4 tiles per wave
    static const int cap = clhip_cfg("STEM7_GRID") ? atoi(clhip_cfg("STEM7_GRID")) : 512;
    if (grid > cap) grid = cap;
    return grid < 1 ? 1 : grid;
}

int stem7_wgrad_splits(int M, int dtype) {
    if (dtype == CLHIP_F32) { const int s = (M + 255) / 256; return s < 1 ? 1 : (s > 256 ? 256 : s); }
    const int nstep = (M + 31) / 32;
    int grid = (nstep + 15) / 16;                            // >= 4 steps per wave
    static const int cap = clhip_cfg("STEM7_WGRAD_GRID") ? atoi(clhip_cfg("STEM7_WGRAD_GRID")) : 128;
    if (grid > cap) grid = cap;
    return grid < 1 ? 1 : grid;
}

// ------------------------------------------------------------------------------------------ BatchNorm + ReLU + max-pool
template <typename T, bool TRAIN>
__global__ __launch_bounds__(256) void bn_relu_maxpool_kernel(const T* __restrict__ z, const double* __restrict__ acc, int rep, double invM, double unbias,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, float* rm, float* rv, float momentum,
                                                              float eps, float* __restrict__ mean_o, float* __restrict__ invstd_o, T* __restrict__ y,
                                                              unsigned char* __restrict__ argmax, int N, int H, int W, int Hp, int Wp, int C) {
    extern __shared__ __attribute__((aligned(16))) float coefs[];       // [2][C]: scale, shift
    __shared__ double sred[256];
    if (TRAIN) {
        // batch statistics from the accumulators: bn_apply_train_kernel's finalize, expression for expression
        const bool narrow = 2 * C <= 128;
        if (narrow) replica_parts(acc, rep, C, sred);
        for (int c = threadIdx.x; c < C; c += 256) {
            const bool upd = blockIdx.x == 0 && rm != nullptr;
            const float rm_old = upd ? rm[c] : 0.f, rv_old = upd ? rv[c] : 0.f;
            double s1 = 0.0, s2 = 0.0;
            if (narrow) { for (int q = 0; q < 256 / (2 * C); ++q) { s1 += sred[q * 2 * C + c]; s2 += sred[q * 2 * C + C + c]; } }
            else sum_strided2(acc + c, acc + C + c, rep, 2 * (size_t)C, s1, s2);
            const double mean = s1 * invM;
            double var = s2 * invM - mean * mean;
            if (var < 0.0) var = 0.0;
            float istd;
            if constexpr (sizeof(T) == 4) istd = (float)(1.0 / sqrt(var + (double)eps));
            else istd = rsqrtf((float)var + eps);
            const float sc = gamma[c] * istd;
            coefs[c] = sc;
            coefs[C + c] = beta[c] - (float)mean * sc;
            if (blockIdx.x == 0) {
                mean_o[c] = (float)mean;
                invstd_o[c] = istd;
                if (rm != nullptr) {
                    rm[c] = (1.f - momentum) * rm_old + momentum * (float)mean;
                    rv[c] = (1.f - momentum) * rv_old + momentum * (float)(var * unbias);
                }
            }
        }
    } else {
        for (int c = threadIdx.x; c < C; c += 256) {                   // bn_apply_eval_kernel's expressions
            const float istd = 1.f / sqrtf(rv[c] + eps);
            const float sc = gamma[c] * istd;
            coefs[c] = sc;
            coefs[C + c] = beta[c] - rm[c] * sc;
        }
    }
    __syncthreads();
    const int cpp = C >> 3;
    const int64_t nchunks = (int64_t)N * Hp * Wp * cpp, stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c0 = ((int)i0 & (cpp - 1)) * 8;                          // fixed per thread: the grid stride is a multiple of C / 8
    float sc[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { sc[e] = coefs[c0 + e]; sh[e] = coefs[C + c0 + e]; }
    for (int64_t i = i0; i < nchunks; i += stride) {
        const int64_t q = i / cpp;
        const int n = (int)(q / ((int64_t)Hp * Wp)), r = (int)(q - (int64_t)n * Hp * Wp), hp = r / Wp, wp = r - hp * Wp;
        float best[8];
        unsigned pos[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { best[e] = -INFINITY; pos[e] = 0; }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int hh = 2 * hp - 1 + t / 3, ww = 2 * wp - 1 + t % 3;
            if ((unsigned)hh >= (unsigned)H || (unsigned)ww >= (unsigned)W) continue;      // padding never wins
            float v[8];
            load8<T>(z + (((size_t)n * H + hh) * W + ww) * C + c0, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float o = fmaxf(fmaf(v[e], sc[e], sh[e]), 0.f);
                if (o > best[e]) { best[e] = o; pos[e] = (unsigned)t; }             // ties: the first in row-major window order
            }
        }
        store8<T>(y + q * C + c0, best);
        if (argmax != nullptr) {
            uint2 m;
            m.x = pos[0] | (pos[1] << 8) | (pos[2] << 16) | (pos[3] << 24);
            m.y = pos[4] | (pos[5] << 8) | (pos[6] << 16) | (pos[7] << 24);
            *reinterpret_cast<uint2*>(argmax + q * C + c0) = m;
        }
    }
}

// gather backward: g = relu'(the stem pixel) * sum of dy over the pooled outputs whose argmax is this pixel; sums of g and g * xhat into acc
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_bn_kernel(const T* __restrict__ dy, const unsigned char* __restrict__ argmax, const T* __restrict__ z,
                                                             const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, T* __restrict__ g_out, double* __restrict__ acc, int rep, int N,
                                                             int H, int W, int Hp, int Wp, int C) {
    __shared__ float red[256][17];
    const int cpp = C >> 3;
    const int64_t nchunks = (int64_t)N * H * W * cpp, stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c0 = ((int)i0 & (cpp - 1)) * 8;
    float sc[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {                                        // the forward's scale / shift (bn_relu_maxpool_kernel): the same sign test
        const int c = c0 + e;
        sc[e] = gamma[c] * invstd[c];
        sh[e] = beta[c] - mean[c] * sc[e];
    }
    float s[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.f;
    for (int64_t i = i0; i < nchunks; i += stride) {
        const int64_t pix = i / cpp;
        const int n = (int)(pix / ((int64_t)H * W)), r = (int)(pix - (int64_t)n * H * W), h = r / W, w = r - h * W;
        float g[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = 0.f;
        // pooled rows whose window (2 hp - 1 .. 2 hp + 1) holds h: hp = h / 2 for even h, (h - 1) / 2 and (h + 1) / 2 for odd h
        const int hp0 = h >> 1, hp1 = (h + 1) >> 1, wp0 = w >> 1, wp1 = (w + 1) >> 1;
        for (int hp = hp0; hp <= hp1 && hp < Hp; ++hp)
            for (int wp = wp0; wp <= wp1 && wp < Wp; ++wp) {
                const unsigned want = (unsigned)((h - 2 * hp + 1) * 3 + (w - 2 * wp + 1));
                const size_t o = (((size_t)n * Hp + hp) * Wp + wp) * C + c0;
                const uint2 m = *reinterpret_cast<const uint2*>(argmax + o);
                float d[8];
                load8<T>(dy + o, d);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const unsigned a = ((e < 4 ? m.x : m.y) >> (8 * (e & 3))) & 0xffu;
                    if (a == want) g[e] += d[e];
                }
            }
        float zz[8];
        load8<T>(z + pix * C + c0, zz);
#pragma unroll
        for (int e = 0; e < 8; ++e) if (!(fmaf(zz[e], sc[e], sh[e]) > 0.f)) g[e] = 0.f;
        store8<T>(g_out + pix * C + c0, g);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            // (the sums of the stored, rounded values: what the apply pass reads back)
            float gs = g[e];
            if constexpr (sizeof(T) == 2) gs = bf16_to_f32((bf16_t)(pack_bf16x2(gs, 0.f) & 0xffffu));
            s[e] += gs; s[8 + e] = fmaf(gs, zz[e], s[8 + e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) red[threadIdx.x][e] = s[e];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        const int grp = c >> 3, e = c & 7;
        float a1 = 0.f, a2 = 0.f;
        for (int t = grp; t < 256; t += cpp) { a1 += red[t][e]; a2 += red[t][8 + e]; }
        double* a = acc + (size_t)(blockIdx.x & (rep - 1)) * 2 * C;
        atomicAdd(a + c, (double)a1);
        atomicAdd(a + C + c, (double)(invstd[c] * (a2 - mean[c] * a1)));
    }
}

int pool_blocks(int64_t nchunks) {
    int64_t b = (nchunks + 256 * 8 - 1) / (256 * 8);
    if (b < 512) { b = (nchunks + 255) / 256; if (b > 512) b = 512; }
    if (b > 4096) b = 4096;
    return b < 1 ? 1 : (int)b;
}

bool pool_c_ok(int C) { return C >= 8 && C <= 2048 && (C & (C - 1)) == 0; }

}  // namespace

// ------------------------------------------------------------------------------------------------ entries (conv.hip routes ksize 7 here)
bool clhip_stem7_supported(int N, int H, int W, int C, int K, int stride, int pad) {
    return N >= 1 && H >= 1 && W >= 1 && C == 8 && stride == 2 && pad == 3 && (K == 16 || K == 32 || K == 64) &&
           (int64_t)N * H * W * 8 < ((int64_t)1 << 31) && (int64_t)N * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1) * K < ((int64_t)1 << 31);
}

int clhip_stem7_fwd_tiles(int N, int H, int W) { return stem7_fwd_grid(N * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1)); }

int clhip_stem7_fwd_launch(const void* x, const void* w, void* z, double* acc, int rep, int N, int H, int W, int K, int dtype, hipStream_t st) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    Stem7Params p{x, w, z, acc, rep > 0 ? rep : 1, N, H, W, Ho, Wo, K, N * Ho * Wo};
    if (dtype == CLHIP_F32) {
        const int64_t nch = (int64_t)p.M * (K / 8);
        int grid = (int)((nch + 255) / 256);
        if (grid > 2048) grid = 2048;
        hipLaunchKernelGGL(conv_stem7_f32_kernel, dim3(grid), dim3(256), 0, st, p);
    } else {
        const int grid = stem7_fwd_grid(p.M);
        const size_t lds = (size_t)K * kPitch * 16;
        if (K == 16) hipLaunchKernelGGL(conv_stem7_kernel<1>, dim3(grid), dim3(256), lds, st, p);
        else if (K == 32) hipLaunchKernelGGL(conv_stem7_kernel<2>, dim3(grid), dim3(256), lds, st, p);
        else hipLaunchKernelGGL(conv_stem7_kernel<4>, dim3(grid), dim3(256), lds, st, p);
    }
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

size_t clhip_stem7_wgrad_ws_bytes(int N, int H, int W, int Creal, int K, int dtype) {
    const int M = N * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
    return (size_t)stem7_wgrad_splits(M, dtype) * K * kTaps * Creal * sizeof(float);
}

int clhip_stem7_wgrad_launch(const void* x, const void* dz, float* dw, float* ws, int N, int H, int W, int Creal, int K, int dtype, hipStream_t st) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, M = N * Ho * Wo;
    Stem7WParams p{x, dz, ws, N, H, W, Ho, Wo, K, M, Creal, (M + 31) / 32};
    const int splits = stem7_wgrad_splits(M, dtype);
    if (dtype == CLHIP_F32) {
        const int pps = (M + splits - 1) / splits;
        hipLaunchKernelGGL(wgrad_stem7_f32_kernel, dim3(splits, K), dim3(256), 0, st, p, pps);
    } else if (K == 16) hipLaunchKernelGGL(wgrad_stem7_kernel<1>, dim3(splits, 7), dim3(256), 0, st, p);
    else if (K == 32) hipLaunchKernelGGL(wgrad_stem7_kernel<2>, dim3(splits, 7), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(wgrad_stem7_kernel<4>, dim3(splits, 7), dim3(256), 0, st, p);
    CLHIP_LAUNCH_CHECK();
    return clhip_wgrad_reduce_launch(ws, dw, (int64_t)K * kTaps * Creal / 4, splits, st);
}

extern "C" int clhip_maxpool_out_dim(int H) { return H >= 1 ? (H + 2 - 3) / 2 + 1 : 0; }

extern "C" int clhip_bn_relu_maxpool_fwd(const void* z, const double* stat_acc, int replicas, const float* gamma, const float* beta, float* running_mean,
                                         float* running_var, float momentum, float eps, float* mean, float* invstd, void* y, void* argmax, int N, int H, int W, int C,
                                         int training, int dtype, void* stream) {
    CLHIP_CHECK_ARG(z && gamma && beta && y && N > 0 && H > 0 && W > 0 && pool_c_ok(C) && (dtype == CLHIP_BF16 || dtype == CLHIP_F32));
    CLHIP_CHECK_ARG(training ? (stat_acc && mean && invstd && replicas >= 1 && replicas <= 64 && (running_mean == nullptr) == (running_var == nullptr))
                             : (running_mean && running_var));
    const int Hp = clhip_maxpool_out_dim(H), Wp = clhip_maxpool_out_dim(W);
    const int64_t M = (int64_t)N * H * W;
    CLHIP_CHECK_ARG(M * C < ((int64_t)1 << 31));
    const int64_t nch = (int64_t)N * Hp * Wp * (C / 8);
    dim3 g(pool_blocks(nch)), b(256);
    const size_t lds = 2 * (size_t)C * sizeof(float);
    const double invM = 1.0 / (double)M, unbias = M > 1 ? (double)M / (double)(M - 1) : 1.0;
    unsigned char* am = static_cast<unsigned char*>(argmax);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define POOL(T, TR) hipLaunchKernelGGL((bn_relu_maxpool_kernel<T, TR>), g, b, lds, st, (const T*)z, stat_acc, replicas, invM, unbias, gamma, beta, running_mean, running_var, \
                                       momentum, eps, mean, invstd, (T*)y, am, N, H, W, Hp, Wp, C)
    if (dtype == CLHIP_BF16) { if (training) POOL(bf16_t, true); else POOL(bf16_t, false); }
    else { if (training) POOL(float, true); else POOL(float, false); }
#undef POOL
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

extern "C" int clhip_maxpool_bwd_bn_reduce(const void* dy, const void* argmax, const void* z, const float* mean, const float* invstd, const float* gamma,
                                           const float* beta, void* g, double* acc, int replicas, int N, int H, int W, int C, int dtype, void* stream) {
    CLHIP_CHECK_ARG(dy && argmax && z && mean && invstd && gamma && beta && g && acc && N > 0 && H > 0 && W > 0 && pool_c_ok(C));
    CLHIP_CHECK_ARG(replicas >= 1 && replicas <= 64 && (replicas & (replicas - 1)) == 0 && (dtype == CLHIP_BF16 || dtype == CLHIP_F32));
    CLHIP_CHECK_ARG((int64_t)N * H * W * C < ((int64_t)1 << 31));
    const int Hp = clhip_maxpool_out_dim(H), Wp = clhip_maxpool_out_dim(W);
    const int64_t nch = (int64_t)N * H * W * (C / 8);
    dim3 gr(pool_blocks(nch)), b(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned char* am = static_cast<const unsigned char*>(argmax);
    if (dtype == CLHIP_BF16)
        hipLaunchKernelGGL(maxpool_bwd_bn_kernel<bf16_t>, gr, b, 0, st, (const bf16_t*)dy, am, (const bf16_t*)z, mean, invstd, gamma, beta, (bf16_t*)g, acc, replicas, N, H, W,
                           Hp, Wp, C);
    else
        hipLaunchKernelGGL(maxpool_bwd_bn_kernel<float>, gr, b, 0, st, (const float*)dy, am, (const float*)z, mean, invstd, gamma, beta, (float*)g, acc, replicas, N, H, W,
                           Hp, Wp, C);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}
