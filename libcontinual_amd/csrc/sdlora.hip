// sdlora.hip -- SD-LoRA (core/model/sd_lora.py, MultiHeadAttention_SDLoRA at core/model/backbone/transformer.py:276-357): the low-rank branch on
// q and v is a SUM over all tasks so far, past terms normalised to unit Frobenius "direction" and every term scaled by a trainable scalar
// magnitude.  The branch is linear in the layer input, so the forward runs with an effective qkv weight
//     W_eff[q rows] = W[q rows] + sum_i c_i B_i A_i,   c_i = mag_i * inv_i   (inv_T = 1, inv_i = 1 / (|B_i|_F |A_i|_F) or 0 for i < T)
// (v rows likewise, k rows untouched) that clhip_sdlora_refresh rewrites every step, and clhip_sdlora_grad produces the gradients of the
// current term's A and B and of every magnitude from rank-sized products only -- no dense [D, D] weight gradient.  No atomics anywhere:
// every sum over the M token rows is slab partials (clhip_tn_slabs, tn_slab.hip: the routine the LoRA B gradient of vit_ops.hip uses) reduced
// in slab order, so two runs are bitwise equal.
// Factor table of one layer: 4 * nterms device pointers, [A_q terms | B_q terms | A_v terms | B_v terms]; A_i [r_i, D], B_i [D, r_i] fp32.
#include <algorithm>

#include "common.h"

namespace {
constexpr int kMaxTerms = 512, kMaxLayers = 32;
struct SdTerms { unsigned char r[kMaxTerms]; };                 // ranks by value: sum r_i <= 512 bounds the term count
struct SdLayer { const float* w; void* wt; void* wtT; };
struct SdLayerTable { SdLayer e[kMaxLayers]; };

size_t al256(size_t v) { return (v + 255) / 256 * 256; }

// q and v rows of all layers' effective qkv copies: blockIdx = (column tile, row tile of [q rows | v rows], layer)
template <typename T>
__global__ __launch_bounds__(256) void sdlora_refresh_kernel(SdLayerTable t, SdTerms tr, const float* const* __restrict__ factors, int l0, int nterms,
                                                              const float* __restrict__ mag, const float* __restrict__ inv, int D) {
    __shared__ float bs[32][17], as[16][33], tile[32][33];
    const SdLayer& d = t.e[blockIdx.z];
    const int layer = l0 + blockIdx.z;
    const int which = (int)blockIdx.y >= D / 32 ? 1 : 0;                       // 0: q rows [0, D), 1: v rows [2D, 3D)
    const int rl0 = ((int)blockIdx.y - which * (D / 32)) * 32, r0 = which * 2 * D + rl0, c0 = blockIdx.x * 32;
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const float* const* fa = factors + ((size_t)layer * 4 + 2 * which) * nterms;
    const float* const* fb = fa + nterms;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < nterms; ++i) {                                         // term order 0..T, fp32
        const int r = tr.r[i];
        const float c = mag[i] * inv[((size_t)layer * 2 + which) * nterms + i];
        if (c == 0.f) continue;                                                // (uniform over the workgroup) a skipped term: transformer.py:325, :331
        const float* A = fa[i];
        const float* B = fb[i];
        __syncthreads();
        for (int idx = tid; idx < 32 * r; idx += 256) {
            const int row = idx / r, q = idx - row * r;
            bs[row][q] = B[(size_t)(rl0 + row) * r + q];
        }
        for (int idx = tid; idx < 32 * r; idx += 256) as[idx >> 5][idx & 31] = A[(size_t)(idx >> 5) * D + c0 + (idx & 31)];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float a = 0.f;
            for (int q = 0; q < r; ++q) a += bs[ty + 8 * j][q] * as[q][tx];
            acc[j] += c * a;
        }
    }
    T* wt = static_cast<T*>(d.wt);
    T* wtT = static_cast<T*>(d.wtT);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = r0 + ty + 8 * j, c = c0 + tx;
        const float v = d.w[(size_t)r * D + c] + acc[j];
        Elem<T>::st(wt + (size_t)r * D + c, v);
        tile[ty + 8 * j][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = c0 + ty + 8 * j, r = r0 + tx;
        Elem<T>::st(wtT + (size_t)c * 3 * D + r, tile[tx][ty + 8 * j]);
    }
}

// compute-dtype operands of the two K = D products: acat [2 Rp, D] = rows [A_0^q .. A_T^q, 0 | A_0^v .. A_T^v, 0] (R = sum r_i rows, padded to Rp)
// and bcat [32, D] = rows [B_T^q transposed, 0 | B_T^v transposed, 0] (16 rows each)
template <typename T>
__global__ __launch_bounds__(256) void sdlora_pack_kernel(const float* const* __restrict__ f, SdTerms tr, int nterms, int R, int Rp, int D, T* __restrict__ acat,
                                                           T* __restrict__ bcat) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= (2 * Rp + 32) * D) return;
    const int row = idx / D, c = idx - row * D;
    float v = 0.f;
    if (row < 2 * Rp) {
        const int which = row >= Rp ? 1 : 0;
        int j = row - which * Rp;
        if (j < R) {
            int i = 0;
            while (j >= tr.r[i]) { j -= tr.r[i]; ++i; }
            v = f[2 * which * nterms + i][(size_t)j * D + c];
        }
        Elem<T>::st(acat + idx, v);
    } else {
        const int rb = row - 2 * Rp, which = rb >> 4, q = rb & 15, rT = tr.r[nterms - 1];
        if (q < rT) v = f[(2 * which + 1) * nterms + nterms - 1][(size_t)c * rT + q];
        Elem<T>::st(bcat + (size_t)rb * D + c, v);
    }
}

// slabs in slab order -> S [2, D, Rp] (kept for the magnitude gradients), dB_T = m_T S_T and dA_T = m_T (U^T X) of q and v, all WRITTEN
__global__ __launch_bounds__(256) void sdlora_reduce_kernel(const float* __restrict__ slabS, const float* __restrict__ slabA, int nslab, int D, int Rp, int offT,
                                                             int rT, const float* __restrict__ mag, int nterms, float* __restrict__ S, float* __restrict__ dAq,
                                                             float* __restrict__ dBq, float* __restrict__ dAv, float* __restrict__ dBv) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, nS = (size_t)2 * D * Rp, nA = (size_t)D * 32;
    if (idx >= nS + nA) return;
    const float mT = mag[nterms - 1];
    float a = 0.f;
    if (idx < nS) {
        for (int s = 0; s < nslab; ++s) a += slabS[(size_t)s * nS + idx];
        S[idx] = a;
        const int j = (int)(idx % Rp) - offT, o = (int)((idx / Rp) % D);
        if (j >= 0 && j < rT) (idx >= nS / 2 ? dBv : dBq)[(size_t)o * rT + j] = mT * a;
    } else {
        const size_t k = idx - nS;
        const int d = (int)(k >> 5), q = (int)(k & 15);
        if (q >= rT) return;
        for (int s = 0; s < nslab; ++s) a += slabA[(size_t)s * nA + k];
        ((k & 16) ? dAv : dAq)[(size_t)q * D + d] = mT * a;
    }
}

// dmag_row[i] = inv_q[i] <S_i^q, B_i^q>_F + inv_v[i] <S_i^v, B_i^v>_F: one workgroup per term, fixed order
__global__ __launch_bounds__(256) void sdlora_dmag_kernel(const float* __restrict__ S, const float* const* __restrict__ f, SdTerms tr, int nterms, int D, int Rp,
                                                           const float* __restrict__ inv, float* __restrict__ dmag_row) {
    __shared__ float red[4];
    const int i = blockIdx.x, r = tr.r[i];
    int off = 0;
    for (int k = 0; k < i; ++k) off += tr.r[k];
    float tot = 0.f;
    for (int w = 0; w < 2; ++w) {
        const float* B = f[(2 * w + 1) * nterms + i];
        float a = 0.f;
        for (int idx = threadIdx.x; idx < D * r; idx += 256) {
            const int o = idx / r, q = idx - o * r;
            a += S[((size_t)w * D + o) * Rp + off + q] * B[idx];
        }
        tot += inv[w * nterms + i] * block_sum_256(a, red);
    }
    if (threadIdx.x == 0) dmag_row[i] = tot;
}

__global__ __launch_bounds__(256) void sdlora_mag_reduce_kernel(const float* __restrict__ rows, int depth, int nterms, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nterms) return;
    float a = 0.f;
    for (int l = 0; l < depth; ++l) a += rows[(size_t)l * nterms + i];          // layer order
    out[i] = a;
}

// ranks -> (sum, packed copy); false (with the error set) when a limit is broken
bool check_terms(const char* who, const int* ranks, int nterms, SdTerms& tr, int& R) {
    if (!ranks || nterms < 1 || nterms > kMaxTerms) { clhip_set_error("%s: 1 .. %d terms with their ranks are required (got %d)", who, kMaxTerms, nterms); return false; }
    R = 0;
    for (int i = 0; i < nterms; ++i) {
        if (ranks[i] < 1 || ranks[i] > 16) { clhip_set_error("%s: rank %d of term %d is outside 1..16", who, ranks[i], i); return false; }
        tr.r[i] = (unsigned char)ranks[i];
        R += ranks[i];
    }
    if (R > 512) { clhip_set_error("%s: the ranks sum to %d, more than 512", who, R); return false; }
    return true;
}

int slab_rows(int M) { return M <= 16384 ? 1024 : ((M + 15) / 16 + 63) / 64 * 64; }
}  // namespace

extern "C" int clhip_sdlora_refresh(int layers, const float* const* qkv_w, const float* const* factors, const int* ranks, int nterms, const float* mag,
                                    const float* inv, void* const* wt, void* const* wt_t, int D, int dtype, void* stream) {
    CLHIP_CHECK_ARG(layers > 0 && qkv_w && factors && mag && inv && wt && wt_t);
    CLHIP_CHECK_ARG(dtype == CLHIP_BF16 || dtype == CLHIP_F32);
    if (D <= 0 || D % 64) { clhip_set_error("clhip_sdlora_refresh: D = %d is not a positive multiple of 64", D); return CLHIP_EINVAL; }
    SdTerms tr;
    int R;
    if (!check_terms("clhip_sdlora_refresh", ranks, nterms, tr, R)) return CLHIP_EINVAL;
    for (int l = 0; l < layers; ++l) CLHIP_CHECK_ARG(qkv_w[l] && wt[l] && wt_t[l]);
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int l0 = 0; l0 < layers; l0 += kMaxLayers) {
        const int n = std::min(kMaxLayers, layers - l0);
        SdLayerTable t;
        for (int i = 0; i < n; ++i) t.e[i] = SdLayer{qkv_w[l0 + i], wt[l0 + i], wt_t[l0 + i]};
        dim3 grid(D / 32, 2 * D / 32, n);
        if (dtype == CLHIP_BF16) hipLaunchKernelGGL(sdlora_refresh_kernel<bf16_t>, grid, dim3(256), 0, s, t, tr, factors, l0, nterms, mag, inv, D);
        else hipLaunchKernelGGL(sdlora_refresh_kernel<float>, grid, dim3(256), 0, s, t, tr, factors, l0, nterms, mag, inv, D);
        CLHIP_LAUNCH_CHECK();
    }
    return CLHIP_OK;
}

// workspace: acat, bcat, P [M, 2 Rp], U [M, 32] (sized for fp32), S [2, D, Rp], the two slab sets
extern "C" size_t clhip_sdlora_grad_ws_bytes(int M, int D, int sum_r) {
    if (M < 1 || D < 1 || sum_r < 1 || sum_r > 512) return 0;
    const size_t Rp = (sum_r + 31) / 32 * 32, nslab = (M + slab_rows(M) - 1) / slab_rows(M);
    return al256((2 * Rp + 32) * D * 4) + al256((size_t)M * 2 * Rp * 4) + al256((size_t)M * 32 * 4) + al256(2 * D * Rp * 4) + al256(nslab * 2 * D * Rp * 4) +
           al256(nslab * D * 32 * 4);
}

extern "C" int clhip_sdlora_grad(const void* x, const void* dqkv, const float* const* factors, const int* ranks, int nterms, const float* mag, const float* inv,
                                 float* d_a_q, float* d_b_q, float* d_a_v, float* d_b_v, float* d_mag_row, void* ws, int M, int D, int dtype, void* stream) {
    CLHIP_CHECK_ARG(x && dqkv && factors && mag && inv && d_a_q && d_b_q && d_a_v && d_b_v && d_mag_row && ws);
    CLHIP_CHECK_ARG(dtype == CLHIP_BF16 || dtype == CLHIP_F32);
    if (M < 1) { clhip_set_error("clhip_sdlora_grad: M = %d rows", M); return CLHIP_EINVAL; }
    if (D <= 0 || D % 64) { clhip_set_error("clhip_sdlora_grad: D = %d is not a positive multiple of 64", D); return CLHIP_EINVAL; }
    SdTerms tr;
    int R;
    if (!check_terms("clhip_sdlora_grad", ranks, nterms, tr, R)) return CLHIP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Rp = (R + 31) / 32 * 32, rT = ranks[nterms - 1], offT = R - rT, rows = slab_rows(M), nslab = (M + rows - 1) / rows;
    const size_t e = dtype == CLHIP_BF16 ? 2 : 4;
    char* p = static_cast<char*>(ws);
    char* acat = p; p += al256((size_t)(2 * Rp + 32) * D * 4);
    char* bcat = acat + (size_t)2 * Rp * D * e;
    char* P = p; p += al256((size_t)M * 2 * Rp * 4);
    char* U = p; p += al256((size_t)M * 32 * 4);
    float* S = reinterpret_cast<float*>(p); p += al256((size_t)2 * D * Rp * 4);
    float* slabS = reinterpret_cast<float*>(p); p += al256((size_t)nslab * 2 * D * Rp * 4);
    float* slabA = reinterpret_cast<float*>(p);
    const int npack = ((2 * Rp + 32) * D + 255) / 256;
    if (dtype == CLHIP_BF16) hipLaunchKernelGGL(sdlora_pack_kernel<bf16_t>, dim3(npack), dim3(256), 0, s, factors, tr, nterms, R, Rp, D, (bf16_t*)acat, (bf16_t*)bcat);
    else hipLaunchKernelGGL(sdlora_pack_kernel<float>, dim3(npack), dim3(256), 0, s, factors, tr, nterms, R, Rp, D, (float*)acat, (float*)bcat);
    CLHIP_LAUNCH_CHECK();
    // K = D: P = X Acat^T [M, 2 Rp]; U = [dQ B_T^q | dV B_T^v] [M, 32]  (MFMA GEMM in both modes)
    if (int rc = clhip_gemm_nt(x, acat, P, nullptr, nullptr, nullptr, M, 2 * Rp, D, D, D, 2 * Rp, 0, 0, 0, dtype, stream)) return rc;
    const char* dq = static_cast<const char*>(dqkv);
    if (int rc = clhip_gemm_nt(dq, bcat, U, nullptr, nullptr, nullptr, M, 16, D, 3 * D, D, 32, 0, 0, 0, dtype, stream)) return rc;
    if (int rc = clhip_gemm_nt(dq + (size_t)2 * D * e, bcat + (size_t)16 * D * e, U + 16 * e, nullptr, nullptr, nullptr, M, 16, D, 3 * D, D, 32, 0, 0, 0, dtype, stream))
        return rc;
    // K = M (tn_slab.hip): S_w = dY_w^T P_w [D, Rp] (w = q, v) and [dA_q^T | dA_v^T] = X^T U [D, 32]; MFMA in bf16, plain FMA in fp32
    if (int rc = clhip_tn_slabs(dqkv, dtype, 3 * D, 2 * D, P, dtype, 2 * Rp, Rp, 0, slabS, M, D, Rp, 2, rows, s)) return rc;
    if (int rc = clhip_tn_slabs(x, dtype, D, 0, U, dtype, 32, 0, 0, slabA, M, D, 32, 1, rows, s)) return rc;
    const size_t nred = (size_t)2 * D * Rp + (size_t)D * 32;
    hipLaunchKernelGGL(sdlora_reduce_kernel, dim3((unsigned)((nred + 255) / 256)), dim3(256), 0, s, slabS, slabA, nslab, D, Rp, offT, rT, mag, nterms, S, d_a_q, d_b_q,
                       d_a_v, d_b_v);
    hipLaunchKernelGGL(sdlora_dmag_kernel, dim3(nterms), dim3(256), 0, s, S, factors, tr, nterms, D, Rp, inv, d_mag_row);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

extern "C" int clhip_sdlora_mag_reduce(const float* rows, int depth, int nterms, float* d_mag, void* stream) {
    CLHIP_CHECK_ARG(rows && d_mag && depth > 0 && nterms > 0);
    hipLaunchKernelGGL(sdlora_mag_reduce_kernel, dim3((nterms + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), rows, depth, nterms, d_mag);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}
