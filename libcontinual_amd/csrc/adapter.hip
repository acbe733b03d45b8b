// adapter.hip -- the AdaptFormer bottleneck branch of the adapter ViT (core/model/backbone/petl/vision_transformer_adapter.py:31-90, :165-183;
// the backbone of the reference's RanPAC first session): per block, parallel to the MLP,
//     h = relu(x Wd^T + bd),   hd = dropout(h, p),   y += s (hd Wu^T + bu)          Wd [R, D], Wu [D, R], R in {16, 32, 64}
// as ONE launch each for the forward, the input gradient and the four parameter gradients.  The shape is a GEMM with N = R followed by one with
// K = R, and the whole branch moves ~3 M D elements for 4 M D R flops: it is bound by the activation traffic, so a workgroup owns 32 rows (64 selectable, measured
// slower at ViT-B/16), keeps their hidden tile in LDS between the two products, touches x / y once and writes every output as 16-byte row pieces.  D is walked in chunks of 256 (bf16) / 128 (fp32) elements
// with every load of a chunk issued before the first LDS store: a ViT-B/16 row tile is three round trips to memory per product, not twelve.
// bf16 runs on mfma_f32_16x16x32_bf16, the fp32 parity mode on the exact mfma_f32_16x16x4f32; both take lane l's operand from row l & 15, k-group l >> 4 of a K-contiguous LDS tile, so one tile routine serves
// the five products (the transposed ones are transposed while they are staged).  The weights are the fp32 masters, converted on load: they move
// every step and are 64 x 768, a compute-dtype copy would only add staleness logic.  No atomics, fixed summation order: repeated runs are bit-identical.
//
// Dropout is a counter-based hash of (seed, layer, row, column) -- a pure function, no generator state; the seed is one 64-bit word in device memory.
// The backward never re-draws it: hd > 0 <=> (h > 0 and kept), and bf16 rounding keeps a positive fp32 positive, so the saved hd IS the mask.
#include <stdlib.h>

#include "common.h"

#ifndef ADAPTER_TM_DEFAULT
#define ADAPTER_TM_DEFAULT 32
#endif

namespace {
// A workgroup of the forward / input gradient owns TM rows (32 or 64, a template parameter: 64 rows halve how often the two fp32 weight matrices
// are read and converted, 32 rows give twice the workgroups).  Elements of D per staged chunk (K of the first product), for the LDS budget:
template <typename T, int TM> constexpr int chunk_of() { return (sizeof(T) == 2 ? 256 : 128) * 32 / TM; }

template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
    static constexpr int KS = 32, KE = 8;
    __device__ static __forceinline__ f32x4 mma(const bf16_t* a, const bf16_t* b, f32x4 c) {
        const uint4 ua = *reinterpret_cast<const uint4*>(a), ub = *reinterpret_cast<const uint4*>(b);
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, ua), __builtin_bit_cast(bf16x8_t, ub), c, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    static constexpr int KS = 4, KE = 1;
    __device__ static __forceinline__ f32x4 mma(const float* a, const float* b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(*a, *b, c, 0, 0, 0); }
};
template <typename T> constexpr int pad_of() { return 16 / (int)sizeof(T); }       // one 16-byte slot per LDS row: conflict-free operand reads

// acc[e] += sum_k a[4 (lane >> 4) + e][k] b[lane & 15][k]: a, b = 16 K-contiguous rows each (pitches lda, ldb elements), K % Mma<T>::KS == 0
template <typename T>
__device__ __forceinline__ f32x4 tile_mma(const T* a, int lda, const T* b, int ldb, int K, f32x4 acc) {
    const int lane = threadIdx.x & 63, r = lane & 15, kg = lane >> 4;
    const T* pa = a + r * lda + kg * Mma<T>::KE;
    const T* pb = b + r * ldb + kg * Mma<T>::KE;
    for (int k = 0; k < K; k += Mma<T>::KS) acc = Mma<T>::mma(pa + k, pb + k, acc);
    return acc;
}

// dst[r][c] = src[r * ld + c] for r < nrows, c < ncols (zero where r >= valid); columns [ncols, kpad) are zeroed.  ncols, kpad % 8 == 0.
template <typename T, typename S>
__device__ __forceinline__ void stage_rows(T* dst, int pitch, const S* src, size_t ld, int valid, int nrows, int ncols, int kpad) {
    const int cw = kpad >> 3, n = nrows * cw;
    for (int i0 = threadIdx.x; i0 < n; i0 += 1024) {                 // four loads in flight per thread before the first store
        float v[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * 256, r = i / cw, c = (i - r * cw) * 8;
#pragma unroll
            for (int q = 0; q < 8; ++q) v[u][q] = 0.f;
            if (i < n && r < valid && c < ncols) load8<S>(src + (size_t)r * ld + c, v[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * 256, r = i / cw, c = (i - r * cw) * 8;
            if (i < n) store8<T>(dst + r * pitch + c, v[u]);
        }
    }
}
// dst[c][r] = src[r * ld + c] for r < nrows, c < ncols (zero where r >= valid); dst rows [nrows, kpad) are zeroed
template <typename T, typename S>
__device__ __forceinline__ void stage_cols(T* dst, int pitch, const S* src, size_t ld, int valid, int nrows, int ncols, int kpad) {
    const int cw = ncols >> 3, n = kpad * cw;
    for (int i0 = threadIdx.x; i0 < n; i0 += 1024) {
        float v[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * 256, r = i / cw, c = (i - r * cw) * 8;
#pragma unroll
            for (int q = 0; q < 8; ++q) v[u][q] = 0.f;
            if (i < n && r < valid && r < nrows) load8<S>(src + (size_t)r * ld + c, v[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * 256, r = i / cw, c = (i - r * cw) * 8;
            if (i < n) {
#pragma unroll
                for (int q = 0; q < 8; ++q) Elem<T>::st(dst + (c + q) * pitch + r, v[u][q]);
            }
        }
    }
}

// rows [0, rows) of an LDS tile [.., ncols] (pitch elements) -> global [.., ld], 16 bytes per lane
template <typename T>
__device__ __forceinline__ void tile_out(T* dst, size_t ld, const T* tile, int pitch, int rows, int ncols) {
    const int cw = ncols >> 3;
    for (int i = threadIdx.x; i < rows * cw; i += 256) {
        const int r = i / cw, c = (i - r * cw) * 8;
        float v[8];
        load8<T>(tile + r * pitch + c, v);
        store8<T>(dst + (size_t)r * ld + c, v);
    }
}
// dst[r][c] = src[r][c] + os[r][c] for r < rows, c < ncols: row-contiguous 16-byte accesses (dst may be src)
template <typename T>
__device__ __forceinline__ void tile_add_out(T* dst, const T* src, size_t ld, const float* os, int OP, int rows, int ncols) {
    const int cw = ncols >> 3;
    for (int i = threadIdx.x; i < rows * cw; i += 256) {
        const int r = i / cw, c = (i - r * cw) * 8;
        float v[8], o[8];
        load8<T>(src + (size_t)r * ld + c, v);
        load8<float>(os + r * OP + c, o);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] += o[q];
        store8<T>(dst + (size_t)r * ld + c, v);
    }
}

// 24 uniform bits of element (row, col) of layer `layer` under `seed`: two splitmix64 finalisers over the seed / layer word and the position
__device__ __forceinline__ unsigned drop_bits(unsigned long long seed, int layer, int row, int col) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(layer + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    z ^= ((unsigned long long)(unsigned)row << 32) | (unsigned)col;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (unsigned)(z >> 40);
}
// an element is KEPT iff its 24 bits are >= thresh = p 2^24
__host__ __device__ inline unsigned drop_thresh(float p) { return (unsigned)(p * 16777216.f); }

template <typename T, int TM>
__global__ __launch_bounds__(256) void adapter_fwd_kernel(const T* __restrict__ x, const float* __restrict__ Wd, const float* __restrict__ bd,
                                                           const float* __restrict__ Wu, const float* __restrict__ bu, T* __restrict__ y,
                                                           T* __restrict__ hd_out, const unsigned long long* __restrict__ seed_p, int layer,
                                                           unsigned thresh, float keep_scale, float s, int M, int D, int R) {
    constexpr int KC = chunk_of<T, TM>(), PC = KC + pad_of<T>(), PHM = 64 + pad_of<T>();
    constexpr int OC = KC * (int)sizeof(T) / 4, OP = OC + 4;     // columns / fp32 LDS pitch of one output tile of the second product: the x tile's bytes
    constexpr int WR = TM / 16, WC = 4 / WR, NJ = 4 / WC;        // waves along the rows / along the column blocks; column blocks of R per wave
    __shared__ __attribute__((aligned(16))) T as[TM * PC];
    __shared__ __attribute__((aligned(16))) T bs[64 * PC > OC * PHM ? 64 * PC : OC * PHM];
    __shared__ __attribute__((aligned(16))) T hs[TM * PHM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, kg = lane >> 4;
    const int rb = wave % WR, nh = wave / WR;               // a wave: 16 of the TM rows, every WC-th column block
    const int m0 = blockIdx.x * TM, rows = min(TM, M - m0);
    const int ncb = R >> 4, RP = R < Mma<T>::KS ? Mma<T>::KS : R, PH = RP + pad_of<T>();
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = zero;
    for (int d0 = 0; d0 < D; d0 += KC) {
        __syncthreads();
        const int kc = min(KC, D - d0);
        stage_rows<T, T>(as, PC, x + (size_t)m0 * D + d0, D, rows, TM, kc, kc);
        stage_rows<T, float>(bs, PC, Wd + d0, D, R, R, kc, kc);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (nh + WC * j < ncb) acc[j] = tile_mma<T>(as + rb * 16 * PC, PC, bs + (nh + WC * j) * 16 * PC, PC, kc, acc[j]);
    }
    const unsigned long long seed = thresh ? *seed_p : 0ull;
    if (RP > R)                                             // the bf16 MFMA is 32 deep: columns [R, 32) of the hidden tile are zero
        for (int i = threadIdx.x; i < TM * 16; i += 256) Elem<T>::st(hs + (i >> 4) * PH + 16 + (i & 15), 0.f);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cb = nh + WC * j;
        if (cb >= ncb) continue;
        const int col = cb * 16 + l15;
        const float b = bd[col];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = rb * 16 + kg * 4 + e;
            float v = fmaxf(acc[j][e] + b, 0.f);
            if (thresh) v = drop_bits(seed, layer, m0 + row, col) >= thresh ? v * keep_scale : 0.f;
            Elem<T>::st(hs + row * PH + col, v);
        }
    }
    __syncthreads();                                        // hs is complete; the x tile is dead: its LDS becomes the fp32 output tile
    if (hd_out != nullptr) tile_out<T>(hd_out + (size_t)m0 * R, R, hs, PH, rows, R);
    float* os = reinterpret_cast<float*>(as);
    static_assert(TM * OP * sizeof(float) <= sizeof(as), "output tile must fit the x tile");
    for (int d0 = 0; d0 < D; d0 += OC) {
        const int dc = min(OC, D - d0);
        stage_rows<T, float>(bs, PH, Wu + (size_t)d0 * R, R, dc, dc, R, RP);
        __syncthreads();
        for (int cb = nh; cb < (dc >> 4); cb += WC) {
            const f32x4 o = tile_mma<T>(hs + rb * 16 * PH, PH, bs + cb * 16 * PH, PH, RP, zero);
            const float b = bu[d0 + cb * 16 + l15];
#pragma unroll
            for (int e = 0; e < 4; ++e) os[(rb * 16 + kg * 4 + e) * OP + cb * 16 + l15] = s * (o[e] + b);
        }
        __syncthreads();
        T* yp = y + (size_t)m0 * D + d0;
        tile_add_out<T>(yp, yp, D, os, OP, rows, dc);         // y += s (hd Wu^T + bu), whole 16-byte pieces of a row per lane
        __syncthreads();
    }
}

// dh = ((s gy) Wu) * [hd > 0] * keep_scale  -> dh_out [M, R];  gx = gy + dh Wd  (gx may be gy: a workgroup has read its rows of gy before it writes)
template <typename T, int TM>
__global__ __launch_bounds__(256) void adapter_bwd_kernel(const T* gy, const T* __restrict__ hd, const float* __restrict__ Wu,
                                                           const float* __restrict__ Wd, T* __restrict__ dh_out, T* gx, float s, float keep_scale,
                                                           int M, int D, int R) {
    constexpr int KC = chunk_of<T, TM>(), PC = KC + pad_of<T>(), PHM = 64 + pad_of<T>();
    constexpr int OC = KC * (int)sizeof(T) / 4, OP = OC + 4;     // columns / fp32 LDS pitch of one output tile of the second product: the x tile's bytes
    constexpr int WR = TM / 16, WC = 4 / WR, NJ = 4 / WC;        // waves along the rows / along the column blocks; column blocks of R per wave
    __shared__ __attribute__((aligned(16))) T as[TM * PC];
    __shared__ __attribute__((aligned(16))) T bs[64 * PC > OC * PHM ? 64 * PC : OC * PHM];
    __shared__ __attribute__((aligned(16))) T hs[TM * PHM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, kg = lane >> 4;
    const int rb = wave % WR, nh = wave / WR;
    const int m0 = blockIdx.x * TM, rows = min(TM, M - m0);
    const int ncb = R >> 4, RP = R < Mma<T>::KS ? Mma<T>::KS : R, PH = RP + pad_of<T>();
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = zero;
    for (int d0 = 0; d0 < D; d0 += KC) {
        __syncthreads();
        const int kc = min(KC, D - d0);
        stage_rows<T, T>(as, PC, gy + (size_t)m0 * D + d0, D, rows, TM, kc, kc);
        stage_cols<T, float>(bs, PC, Wu + (size_t)d0 * R, R, kc, kc, R, kc);          // bs[r][d] = Wu[d0 + d][r]
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (nh + WC * j < ncb) acc[j] = tile_mma<T>(as + rb * 16 * PC, PC, bs + (nh + WC * j) * 16 * PC, PC, kc, acc[j]);
    }
    if (RP > R)
        for (int i = threadIdx.x; i < TM * 16; i += 256) Elem<T>::st(hs + (i >> 4) * PH + 16 + (i & 15), 0.f);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cb = nh + WC * j;
        if (cb >= ncb) continue;
        const int col = cb * 16 + l15;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = rb * 16 + kg * 4 + e;
            const bool in = row < rows;
            const float h = in ? Elem<T>::ld(hd + (size_t)(m0 + row) * R + col) : 0.f;
            const float v = h > 0.f ? s * acc[j][e] * keep_scale : 0.f;
            Elem<T>::st(hs + row * PH + col, v);
        }
    }
    __syncthreads();
    tile_out<T>(dh_out + (size_t)m0 * R, R, hs, PH, rows, R);
    float* os = reinterpret_cast<float*>(as);
    static_assert(TM * OP * sizeof(float) <= sizeof(as), "output tile must fit the gy tile");
    for (int d0 = 0; d0 < D; d0 += OC) {
        const int dc = min(OC, D - d0);
        stage_cols<T, float>(bs, PH, Wd + d0, D, R, R, dc, RP);                      // bs[d][r] = Wd[r][d0 + d]
        __syncthreads();
        for (int cb = nh; cb < (dc >> 4); cb += WC) {
            const f32x4 o = tile_mma<T>(hs + rb * 16 * PH, PH, bs + cb * 16 * PH, PH, RP, zero);
#pragma unroll
            for (int e = 0; e < 4; ++e) os[(rb * 16 + kg * 4 + e) * OP + cb * 16 + l15] = o[e];
        }
        __syncthreads();
        tile_add_out<T>(gx + (size_t)m0 * D + d0, gy + (size_t)m0 * D + d0, D, os, OP, rows, dc);
        __syncthreads();
    }
}

// row-slab partials of the two [D, R] products and the two column sums.  grid (D / 64, slabs, 2): z = 0 -> Y = gy, Z = hd (dWu, dbu);
// z = 1 -> Y = x, Z = dh (dWd transposed, dbd).  part = [2][slabs][D][R] products, then [slabs][D + R] column sums.
template <typename T>
__global__ __launch_bounds__(256) void adapter_wgrad_kernel(const T* __restrict__ gy, const T* __restrict__ hd, const T* __restrict__ x,
                                                             const T* __restrict__ dh, float* __restrict__ part, int M, int D, int R,
                                                             int rows_per_slab) {
    constexpr int KM = 32, PT = KM + pad_of<T>();
    __shared__ __attribute__((aligned(16))) T yt[64 * PT];
    __shared__ __attribute__((aligned(16))) T zt[64 * PT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kg = lane >> 4;
    const int which = blockIdx.z, slab = blockIdx.y, nslab = gridDim.y, d0 = blockIdx.x * 64;
    const T* Y = which ? x : gy;
    const T* Z = which ? dh : hd;
    const int m0 = slab * rows_per_slab, m1 = min(M, m0 + rows_per_slab);
    const int ncb = R >> 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[4] = {zero, zero, zero, zero};
    // column sums: dbu from the Y tile of every column block (z = 0), dbd from the Z tile of column block 0 (z = 1)
    const bool sum_y = which == 0 && tid < 64, sum_z = which == 1 && blockIdx.x == 0 && tid >= 64 && tid < 64 + R;
    float bsum = 0.f;
    for (int mb = m0; mb < m1; mb += KM) {
        __syncthreads();
        stage_cols<T, T>(yt, PT, Y + (size_t)mb * D + d0, D, m1 - mb, KM, 64, KM);    // yt[d][m]
        stage_cols<T, T>(zt, PT, Z + (size_t)mb * R, R, m1 - mb, KM, R, KM);          // zt[r][m]
        __syncthreads();
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
            if (cb < ncb) acc[cb] = tile_mma<T>(yt + wave * 16 * PT, PT, zt + cb * 16 * PT, PT, KM, acc[cb]);
        if (sum_y || sum_z) {
            const T* row = sum_y ? yt + tid * PT : zt + (tid - 64) * PT;
            for (int k = 0; k < KM; ++k) bsum += Elem<T>::ld(row + k);
        }
    }
    float* mat = part + ((size_t)which * nslab + slab) * D * R;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
        if (cb < ncb) {
#pragma unroll
            for (int e = 0; e < 4; ++e) mat[(size_t)(d0 + wave * 16 + kg * 4 + e) * R + cb * 16 + l15] = acc[cb][e];
        }
    float* cs = part + (size_t)2 * nslab * D * R + (size_t)slab * (D + R);
    if (sum_y) cs[d0 + tid] = bsum;
    if (sum_z) cs[D + tid - 64] = bsum;
}

// slabs summed in slab order: dWu [D, R] = s sum, dWd [R, D] = (sum)^T, dbu [D] = s sum, dbd [R] = sum
__global__ __launch_bounds__(256) void adapter_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dWu, float* __restrict__ dbu,
                                                                    float* __restrict__ dWd, float* __restrict__ dbd, float s, int D, int R, int nslab) {
    const int idx = blockIdx.x * 256 + threadIdx.x, DR = D * R;
    if (idx >= 2 * DR + D + R) return;
    float a = 0.f;
    if (idx < 2 * DR) {
        for (int q = 0; q < nslab; ++q) a += part[((size_t)(idx >= DR ? nslab : 0) + q) * DR + (idx % DR)];
        if (idx < DR) dWu[idx] = s * a;
        else { const int i = idx - DR, d = i / R, r = i - d * R; dWd[(size_t)r * D + d] = a; }
    } else {
        const int i = idx - 2 * DR;
        const float* cs = part + (size_t)2 * nslab * DR;
        for (int q = 0; q < nslab; ++q) a += cs[(size_t)q * (D + R) + i];
        if (i < D) dbu[i] = s * a;
        else dbd[i - D] = a;
    }
}

__global__ __launch_bounds__(256) void adapter_mask_kernel(const unsigned long long* __restrict__ seed_p, int layer, int M, int R, unsigned thresh,
                                                            unsigned char* __restrict__ out) {
    const size_t n = (size_t)M * R;
    const unsigned long long seed = thresh ? *seed_p : 0ull;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int row = (int)(i / R), col = (int)(i - (size_t)row * R);
        out[i] = thresh == 0 || drop_bits(seed, layer, row, col) >= thresh ? 1 : 0;
    }
}

bool shape_ok(int M, int D, int R) { return M > 0 && D > 0 && D % 64 == 0 && (R == 16 || R == 32 || R == 64); }
bool p_ok(float p) { return p == 0.f || (p < 1.f && drop_thresh(p) > 0); }      // (a p below 2^-24 cannot be told from 0 by 24 hash bits: refused)

// rows per workgroup of the forward / input gradient: clhip_config("ADAPTER_TM", "32" | "64") pins it (read at every call: the tests run both)
int tile_rows(int M) {
    const char* c = clhip_cfg("ADAPTER_TM");
    if (c && atoi(c) == 64) return 64;
    if (c && atoi(c) == 32) return 32;
    return ADAPTER_TM_DEFAULT;
}

void wgrad_slabs(int M, int& rows, int& nslab) {
    // ~24 slabs (x 2 D / 64 workgroups each: a few hundred workgroups at ViT-B/16), 32-row steps
    const int want = (M + 31) / 32 < 24 ? (M + 31) / 32 : 24;
    rows = ((M + want - 1) / want + 31) / 32 * 32;
    nslab = (M + rows - 1) / rows;
}
}  // namespace

extern "C" int clhip_adapter_fwd(const void* x, const float* down_w, const float* down_b, const float* up_w, const float* up_b, void* y, void* hd,
                                 const unsigned long long* seed, int layer, float p, float scale, int M, int D, int R, int dtype, void* stream) {
    CLHIP_CHECK_ARG(x && down_w && down_b && up_w && up_b && y);
    CLHIP_CHECK_ARG(dtype == CLHIP_BF16 || dtype == CLHIP_F32);
    CLHIP_CHECK_ARG(shape_ok(M, D, R));
    CLHIP_CHECK_ARG(p_ok(p));
    CLHIP_CHECK_ARG((p > 0.f) == (seed != nullptr));
    CLHIP_CHECK_ARG(layer >= 0);
    const unsigned thresh = drop_thresh(p);
    const float ks = thresh ? 1.f / (1.f - p) : 1.f;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int TM = tile_rows(M);
    const dim3 grid((M + TM - 1) / TM);
#define ADAPTER_FWD(T, TMv) hipLaunchKernelGGL((adapter_fwd_kernel<T, TMv>), grid, dim3(256), 0, s, (const T*)x, down_w, down_b, up_w, up_b, (T*)y, (T*)hd, \
                                               seed, layer, thresh, ks, scale, M, D, R)
    if (dtype == CLHIP_BF16) { if (TM == 64) ADAPTER_FWD(bf16_t, 64); else ADAPTER_FWD(bf16_t, 32); }
    else { if (TM == 64) ADAPTER_FWD(float, 64); else ADAPTER_FWD(float, 32); }
#undef ADAPTER_FWD
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

extern "C" int clhip_adapter_bwd(const void* gy, const void* hd, const float* up_w, const float* down_w, void* dh, void* gx, float p, float scale, int M,
                                 int D, int R, int dtype, void* stream) {
    CLHIP_CHECK_ARG(gy && hd && up_w && down_w && dh && gx);
    CLHIP_CHECK_ARG(dtype == CLHIP_BF16 || dtype == CLHIP_F32);
    CLHIP_CHECK_ARG(shape_ok(M, D, R));
    CLHIP_CHECK_ARG(p_ok(p));
    const float ks = drop_thresh(p) ? 1.f / (1.f - p) : 1.f;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int TM = tile_rows(M);
    const dim3 grid((M + TM - 1) / TM);
#define ADAPTER_BWD(T, TMv) hipLaunchKernelGGL((adapter_bwd_kernel<T, TMv>), grid, dim3(256), 0, s, (const T*)gy, (const T*)hd, up_w, down_w, (T*)dh, (T*)gx, \
                                               scale, ks, M, D, R)
    if (dtype == CLHIP_BF16) { if (TM == 64) ADAPTER_BWD(bf16_t, 64); else ADAPTER_BWD(bf16_t, 32); }
    else { if (TM == 64) ADAPTER_BWD(float, 64); else ADAPTER_BWD(float, 32); }
#undef ADAPTER_BWD
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

extern "C" size_t clhip_adapter_wgrad_ws_bytes(int M, int D, int R) {
    if (!shape_ok(M, D, R)) return 0;
    int rows, nslab;
    wgrad_slabs(M, rows, nslab);
    return (size_t)nslab * ((size_t)2 * D * R + D + R) * sizeof(float);
}

extern "C" int clhip_adapter_wgrad(const void* gy, const void* hd, const void* x, const void* dh, float* d_up_w, float* d_up_b, float* d_down_w,
                                   float* d_down_b, void* ws, float scale, int M, int D, int R, int dtype, void* stream) {
    CLHIP_CHECK_ARG(gy && hd && x && dh && d_up_w && d_up_b && d_down_w && d_down_b && ws);
    CLHIP_CHECK_ARG(dtype == CLHIP_BF16 || dtype == CLHIP_F32);
    CLHIP_CHECK_ARG(shape_ok(M, D, R));
    int rows, nslab;
    wgrad_slabs(M, rows, nslab);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(ws);
    const dim3 grid(D / 64, nslab, 2);
    if (dtype == CLHIP_BF16)
        hipLaunchKernelGGL(adapter_wgrad_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)gy, (const bf16_t*)hd, (const bf16_t*)x, (const bf16_t*)dh, part, M,
                           D, R, rows);
    else
        hipLaunchKernelGGL(adapter_wgrad_kernel<float>, grid, dim3(256), 0, s, (const float*)gy, (const float*)hd, (const float*)x, (const float*)dh, part, M, D,
                           R, rows);
    CLHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(adapter_wgrad_reduce_kernel, dim3((2 * D * R + D + R + 255) / 256), dim3(256), 0, s, part, d_up_w, d_up_b, d_down_w, d_down_b, scale, D,
                       R, nslab);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

extern "C" int clhip_adapter_dropout_mask(const unsigned long long* seed, int layer, int M, int R, float p, unsigned char* out, void* stream) {
    CLHIP_CHECK_ARG(out && M > 0 && R > 0 && layer >= 0);
    CLHIP_CHECK_ARG(p_ok(p));
    CLHIP_CHECK_ARG((p > 0.f) == (seed != nullptr));
    const size_t n = (size_t)M * R;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(adapter_mask_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), seed, layer, M, R, drop_thresh(p), out);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}
