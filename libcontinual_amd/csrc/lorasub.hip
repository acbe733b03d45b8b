// lorasub.hip -- LoRA-Sub-DRS (core/model/lora_sub.py, MultiHeadAttention_LoRA_Sub at core/model/backbone/transformer.py:359-444): the three pieces of the
// method that had no kernel.  clhip_atl is the augmented triplet loss (lora_sub.py:34-68, a Python double loop over batch x prototypes) with its gradient with
// respect to the un-normalised features; clhip_lora_grad_ab the gradients of all four k / v factors of one layer when A trains too; clhip_proj_adam_multi
// the Adam step whose update is multiplied by a per-layer [D, D] transform (lora_sub.py:120-157).  Exact fp32, no atomics anywhere, every sum in a fixed
// order (lane-strided partials + the xor-shuffle tree, slab partials in slab order, k ascending): two runs are bitwise equal.
#include <math.h>

#include "common.h"

namespace {
constexpr int kAtlMaxB = 256, kAtlMaxP = 1024, kAtlMaxD = 8192;
// workspace of clhip_atl (floats): what the select launch leaves for the gather launch
struct AtlWs {
    float* finv;     // [256]  1 / |f_i|
    float* cinv;     // [1024] 1 / |proto_p|
    float* cpos;     // [256]  1 / ap_i where row i is active and ap_i is not clamped, else 0
    float* cneg;     // [256]  1 / an_i where row i is active, has a negative and an_i is not clamped, else 0
    float* hinge;    // [256]  max(0, ap_i - an_i + margin), 0 for a row without any negative
    int* jpos;       // [256]  the batch row that gave ap_i
    int* jneg;       // [256]  the candidate that gave an_i: batch row j, or B + p for prototype p, or -1
};
__host__ __device__ inline AtlWs atl_ws(void* ws) {
    float* p = static_cast<float*>(ws);
    AtlWs w;
    w.finv = p; w.cinv = p + 256; w.cpos = p + 1280; w.cneg = p + 1536; w.hinge = p + 1792;
    w.jpos = reinterpret_cast<int*>(p + 2048); w.jneg = reinterpret_cast<int*>(p + 2304);
    return w;
}
constexpr size_t kAtlWsBytes = 2560 * 4;

// sum of squares of one row by ONE wave, lane-strided: the only way a norm is formed, so every workgroup holds the same n_j
__device__ __forceinline__ float wave_sumsq(const float* __restrict__ row, int D, int lane) {
    float s = 0.f;
    for (int d = lane; d < D; d += 64) { const float v = row[d]; s += v * v; }
    return wave_sum(s);
}

// launch 1: workgroup i forms the distances of row i to every batch row and prototype (a wave per candidate) and selects ap_i and an_i
__global__ __launch_bounds__(256) void atl_select_kernel(const float* __restrict__ f, const int64_t* __restrict__ labels, const float* __restrict__ protos, int B,
                                                          int D, int P, float margin, AtlWs w) {
    extern __shared__ float ni[];                                   // [D] n_i
    __shared__ float dd[kAtlMaxB + kAtlMaxP], aa[kAtlMaxB + kAtlMaxP];      // the clamped distance and the raw sum of squares of every candidate
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* fi = f + (size_t)i * D;
    const float inv_i = 1.f / sqrtf(wave_sumsq(fi, D, lane));
    for (int d = tid; d < D; d += 256) ni[d] = fi[d] * inv_i;
    __syncthreads();
    for (int c = wave; c < B + P; c += 4) {
        const float* row = c < B ? f + (size_t)c * D : protos + (size_t)(c - B) * D;
        const float inv = 1.f / sqrtf(wave_sumsq(row, D, lane));
        float a = 0.f;
        for (int d = lane; d < D; d += 64) { const float t = ni[d] - row[d] * inv; a += t * t; }
        a = wave_sum(a);
        if (lane == 0) {
            if (c < B) { aa[c] = a; dd[c] = sqrtf(fmaxf(a, 1e-12f)); }                    // dist.clamp(min=1e-12).sqrt(), lora_sub.py:45
            else { const float e = sqrtf(a); aa[c] = e; dd[c] = fmaxf(e, 1e-12f); }       // torch.norm(...).clamp(min=1e-12), :62
            if (c == i) w.finv[i] = inv;
            if (c >= B && (c - B) % (int)gridDim.x == i) w.cinv[c - B] = inv;
        }
    }
    __syncthreads();
    if (wave != 0) return;
    const int64_t yi = labels[i];
    // ap: the largest distance among the rows of the same label (j = i included), an: the smallest among the others; ties to the lower index
    float pv = -1.f, nv = INFINITY, ev = INFINITY;
    int pj = B, nj = B, ej = B + P;
    for (int j = lane; j < B; j += 64) {
        const float d = dd[j];
        if (labels[j] == yi) { if (d > pv) { pv = d; pj = j; } }
        else if (d < nv) { nv = d; nj = j; }
    }
    for (int c = B + lane; c < B + P; c += 64)
        if (dd[c] < ev) { ev = dd[c]; ej = c; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float opv = __shfl_xor(pv, o, 64), onv = __shfl_xor(nv, o, 64), oev = __shfl_xor(ev, o, 64);
        const int opj = __shfl_xor(pj, o, 64), onj = __shfl_xor(nj, o, 64), oej = __shfl_xor(ej, o, 64);
        if (opv > pv || (opv == pv && opj < pj)) { pv = opv; pj = opj; }
        if (onv < nv || (onv == nv && onj < nj)) { nv = onv; nj = onj; }
        if (oev < ev || (oev == ev && oej < ej)) { ev = oev; ej = oej; }
    }
    if (lane != 0) return;
    const float ap = pv;
    float an = nj < B ? nv : ap + margin;                           // lora_sub.py:53-56
    int jn = nj < B ? nj : -1;
    if (ej < B + P && ev < an) { an = ev; jn = ej; }                // :60-63, strict, ascending p
    const float h = (ap - an) + margin;                             // MarginRankingLoss(an, ap, 1)
    const bool active = pj < B && jn >= 0 && h > 0.f;               // (pj == B: every distance of the row is NaN)
    w.hinge[i] = active ? h : (pj < B ? 0.f : NAN);
    w.jpos[i] = pj < B ? pj : i;
    w.jneg[i] = jn;
    w.cpos[i] = active && aa[pj] >= 1e-12f ? 1.f / ap : 0.f;        // clamp passes the gradient where the argument is >= the bound
    w.cneg[i] = active && aa[jn] >= 1e-12f ? 1.f / an : 0.f;
}

// launch 2: workgroup j gathers d loss / d n_j (its own two pairs and, in ascending i, the rows that selected j), then passes it through the normalisation
__global__ __launch_bounds__(256) void atl_gather_kernel(const float* __restrict__ f, const float* __restrict__ protos, int B, int D, float weight, AtlWs w,
                                                          float* __restrict__ loss, float* __restrict__ df) {
    __shared__ float finv[kAtlMaxB], cpos[kAtlMaxB], cneg[kAtlMaxB], red[4];
    __shared__ int jpos[kAtlMaxB], jneg[kAtlMaxB];
    const int j = blockIdx.x, tid = threadIdx.x;
    if (tid < B) { finv[tid] = w.finv[tid]; cpos[tid] = w.cpos[tid]; cneg[tid] = w.cneg[tid]; jpos[tid] = w.jpos[tid]; jneg[tid] = w.jneg[tid]; }
    __syncthreads();
    if (j == 0 && tid == 0) {
        float s = 0.f;
        for (int i = 0; i < B; ++i) s += w.hinge[i];
        loss[0] = s / (float)B;
    }
    const float* fj = f + (size_t)j * D;
    float* dj = df + (size_t)j * D;
    const float invj = finv[j];
    float dot = 0.f;
    for (int d = tid; d < D; d += 256) {
        const float nj = fj[d] * invj;
        float g = 0.f;
        for (int i = 0; i < B; ++i) {
            if (i == j) {
                if (cpos[j] != 0.f) { const int p = jpos[j]; g += cpos[j] * (nj - f[(size_t)p * D + d] * finv[p]); }
                if (cneg[j] != 0.f) {
                    const int c = jneg[j];
                    const float nc = c < B ? f[(size_t)c * D + d] * finv[c] : protos[(size_t)(c - B) * D + d] * w.cinv[c - B];
                    g -= cneg[j] * (nj - nc);
                }
            } else {
                if (jpos[i] == j && cpos[i] != 0.f) g -= cpos[i] * (f[(size_t)i * D + d] * finv[i] - nj);
                if (jneg[i] == j && cneg[i] != 0.f) g += cneg[i] * (f[(size_t)i * D + d] * finv[i] - nj);
            }
        }
        dj[d] = g;                                                  // (read back below by the thread that wrote it)
        dot += nj * g;
    }
    dot = block_sum_256(dot, red);
    const float s = weight / (float)B;
    for (int d = tid; d < D; d += 256) dj[d] = s * ((dj[d] - fj[d] * invj * dot) * invj);
}

// ---------------------------------------------------------------------------------------------------------------- gradients of A and B
size_t al256(size_t v) { return (v + 255) / 256 * 256; }
int slab_rows(int M) { return M <= 16384 ? 1024 : ((M + 15) / 16 + 63) / 64 * 64; }

// compute-dtype operands of the two K = D products: acat [32, D] = rows [A_k, 0 | A_v, 0] and bcat [32, D] = rows [B_k transposed, 0 | B_v transposed, 0]
template <typename T>
__global__ __launch_bounds__(256) void lorasub_pack_kernel(const float* __restrict__ ak, const float* __restrict__ bk, const float* __restrict__ av,
                                                            const float* __restrict__ bv, int r, int D, T* __restrict__ acat, T* __restrict__ bcat) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 64 * D) return;
    const int row = idx / D, c = idx - row * D, q = row & 15, v = (row >> 4) & 1;
    float val = 0.f;
    if (row < 32) {
        if (q < r) val = (v ? av : ak)[(size_t)q * D + c];
        Elem<T>::st(acat + idx, val);
    } else {
        if (q < r) val = (v ? bv : bk)[(size_t)c * r + q];
        Elem<T>::st(bcat + (size_t)(row - 32) * D + c, val);
    }
}

// slabs in slab order -> d_b [D, r] of k and v (slabS [s][w][D][16]) and d_a [r, D] of k and v (slabA [s][D][32], columns [k | v]); all WRITTEN
__global__ __launch_bounds__(256) void lorasub_reduce_kernel(const float* __restrict__ slabS, const float* __restrict__ slabA, int nslab, int D, int r,
                                                              float* __restrict__ dak, float* __restrict__ dbk, float* __restrict__ dav, float* __restrict__ dbv) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, nS = (size_t)2 * D * 16, nA = (size_t)D * 32;
    if (idx >= nS + nA) return;
    float a = 0.f;
    if (idx < nS) {
        const int q = (int)(idx & 15), o = (int)((idx >> 4) % D);
        if (q >= r) return;
        for (int s = 0; s < nslab; ++s) a += slabS[(size_t)s * nS + idx];
        (idx >= nS / 2 ? dbv : dbk)[(size_t)o * r + q] = a;
    } else {
        const size_t k = idx - nS;
        const int d = (int)(k >> 5), q = (int)(k & 15);
        if (q >= r) return;
        for (int s = 0; s < nslab; ++s) a += slabA[(size_t)s * nA + k];
        ((k & 16) ? dav : dak)[(size_t)q * D + d] = a;
    }
}

// ------------------------------------------------------------------------------------------------------------------- projected Adam
struct AdamT { float* p; const float* g; float* m; float* v; };

// launch 1: moments of every tensor (the arithmetic of adam_kernel, elementwise.hip); plain: the parameter too, else q = m / denom for launch 2
template <bool kPlain>
__global__ __launch_bounds__(256) void proj_adam_moments_kernel(const AdamT* __restrict__ t, int n, float lr, float b1, float b2, float eps, float wd, float bc1,
                                                                 float bc2s, float* __restrict__ q) {
    const AdamT e = t[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float pv = e.p[i];
    const float d = fmaf(wd, pv, e.g[i]);
    const float mi = b1 * e.m[i] + (1.f - b1) * d;
    const float vi = b2 * e.v[i] + (1.f - b2) * d * d;
    e.m[i] = mi; e.v[i] = vi;
    const float denom = sqrtf(vi) / bc2s + eps;
    if (kPlain) e.p[i] = pv - (lr / bc1) * (mi / denom);
    else q[(size_t)blockIdx.y * n + i] = mi / denom;
}

// launch 2: blockIdx = (32-wide block of the D axis, 0: the two B of a layer, 1: the two A, layer).  out[a][c] = sum_k Tt[a][k] qs[k][c], k ascending, c < 2 r
// (k then v); B: Tt[a][k] = T[i0 + a][k], A: Tt[a][k] = T[k][i0 + a].  p <- p - (lr / bc1) out.
__global__ __launch_bounds__(256) void proj_adam_apply_kernel(const AdamT* __restrict__ t, const float* const* __restrict__ transforms, const float* __restrict__ q,
                                                               int D, int r, float lr, float bc1) {
    __shared__ float ts[32][33], qs[32][33];
    const int i0 = blockIdx.x * 32, isA = blockIdx.y, layer = blockIdx.z, tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const float* T = transforms[layer];
    const int n = D * r, tk = layer * 4 + (isA ? 0 : 1), tv = tk + 2;          // per layer: A_k, B_k, A_v, B_v
    const float* qk = q + (size_t)tk * n;
    const float* qv = q + (size_t)tv * n;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < D; k0 += 32) {
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int row = ty + 8 * jj;
            if (isA) ts[tx][row] = T[(size_t)(k0 + row) * D + i0 + tx];
            else ts[row][tx] = T[(size_t)(i0 + row) * D + k0 + tx];
        }
        for (int idx = tid; idx < 32 * 2 * r; idx += 256) {
            int k, c;
            if (isA) { k = idx & 31; c = idx >> 5; } else { c = idx % (2 * r); k = idx / (2 * r); }
            const float* src = c < r ? qk : qv;
            const int cc = c < r ? c : c - r;
            qs[k][c] = isA ? src[(size_t)cc * D + k0 + k] : src[(size_t)(k0 + k) * r + cc];
        }
        __syncthreads();
        if (tx < 2 * r) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                for (int k = 0; k < 32; ++k) acc[jj] += ts[ty + 8 * jj][k] * qs[k][tx];
        }
    }
    if (tx >= 2 * r) return;
    float* p = t[tx < r ? tk : tv].p;
    const int cc = tx < r ? tx : tx - r;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int a = i0 + ty + 8 * jj;
        float* dst = isA ? p + (size_t)cc * D + a : p + (size_t)a * r + cc;
        const float pv = *dst;
        *dst = pv - (lr / bc1) * acc[jj];
    }
}
}  // namespace

extern "C" size_t clhip_atl_ws_bytes(int B, int P) { return B >= 1 && B <= kAtlMaxB && P >= 0 && P <= kAtlMaxP ? kAtlWsBytes : 0; }

extern "C" int clhip_atl(const float* f, const int64_t* labels, const float* protos, int B, int D, int P, float margin, float weight, float* loss, float* df,
                         void* ws, void* stream) {
    CLHIP_CHECK_ARG(f && labels && loss && df && ws);
    if (B < 1 || B > kAtlMaxB) { clhip_set_error("clhip_atl: B = %d is outside 1..%d", B, kAtlMaxB); return CLHIP_EINVAL; }
    if (P < 0 || P > kAtlMaxP) { clhip_set_error("clhip_atl: P = %d is outside 0..%d", P, kAtlMaxP); return CLHIP_EINVAL; }
    if (D <= 0 || D % 64 || D > kAtlMaxD) { clhip_set_error("clhip_atl: D = %d is not a positive multiple of 64 up to %d", D, kAtlMaxD); return CLHIP_EINVAL; }
    if ((P > 0) != (protos != nullptr)) { clhip_set_error("clhip_atl: protos must be given exactly when P > 0 (P = %d)", P); return CLHIP_EINVAL; }
    if (!isfinite(margin) || !isfinite(weight)) { clhip_set_error("clhip_atl: margin and weight must be finite"); return CLHIP_EINVAL; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const AtlWs w = atl_ws(ws);
    hipLaunchKernelGGL(atl_select_kernel, dim3(B), dim3(256), (size_t)D * sizeof(float), s, f, labels, protos, B, D, P, margin, w);
    hipLaunchKernelGGL(atl_gather_kernel, dim3(B), dim3(256), 0, s, f, protos, B, D, weight, w, loss, df);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

// workspace: acat, bcat, P [M, 32], U [M, 32] (sized for fp32), the two slab sets
extern "C" size_t clhip_lora_grad_ab_ws_bytes(int M, int D) {
    if (M < 1 || D < 1) return 0;
    const size_t nslab = (M + slab_rows(M) - 1) / slab_rows(M);
    return al256((size_t)64 * D * 4) + 2 * al256((size_t)M * 32 * 4) + al256(nslab * 2 * D * 16 * 4) + al256(nslab * D * 32 * 4);
}

extern "C" int clhip_lora_grad_ab(const void* x, const void* dqkv, const float* lora_a_k, const float* lora_b_k, const float* lora_a_v, const float* lora_b_v,
                                  float* d_a_k, float* d_b_k, float* d_a_v, float* d_b_v, void* ws, int M, int D, int rank, int dtype, void* stream) {
    CLHIP_CHECK_ARG(x && dqkv && lora_a_k && lora_b_k && lora_a_v && lora_b_v && d_a_k && d_b_k && d_a_v && d_b_v && ws);
    CLHIP_CHECK_ARG(dtype == CLHIP_BF16 || dtype == CLHIP_F32);
    if (M < 1) { clhip_set_error("clhip_lora_grad_ab: M = %d rows", M); return CLHIP_EINVAL; }
    if (D <= 0 || D % 64) { clhip_set_error("clhip_lora_grad_ab: D = %d is not a positive multiple of 64", D); return CLHIP_EINVAL; }
    if (rank < 1 || rank > 16) { clhip_set_error("clhip_lora_grad_ab: rank %d is outside 1..16", rank); return CLHIP_EINVAL; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rows = slab_rows(M), nslab = (M + rows - 1) / rows;
    const size_t e = dtype == CLHIP_BF16 ? 2 : 4;
    char* p = static_cast<char*>(ws);
    char* acat = p; p += al256((size_t)64 * D * 4);
    char* bcat = acat + (size_t)32 * D * e;
    char* P = p; p += al256((size_t)M * 32 * 4);
    char* U = p; p += al256((size_t)M * 32 * 4);
    float* slabS = reinterpret_cast<float*>(p); p += al256((size_t)nslab * 2 * D * 16 * 4);
    float* slabA = reinterpret_cast<float*>(p);
    const int npack = (64 * D + 255) / 256;
    if (dtype == CLHIP_BF16)
        hipLaunchKernelGGL(lorasub_pack_kernel<bf16_t>, dim3(npack), dim3(256), 0, s, lora_a_k, lora_b_k, lora_a_v, lora_b_v, rank, D, (bf16_t*)acat, (bf16_t*)bcat);
    else hipLaunchKernelGGL(lorasub_pack_kernel<float>, dim3(npack), dim3(256), 0, s, lora_a_k, lora_b_k, lora_a_v, lora_b_v, rank, D, (float*)acat, (float*)bcat);
    CLHIP_LAUNCH_CHECK();
    // K = D: P = X [A_k; A_v]^T [M, 32]; U = [dK B_k | dV B_v] [M, 32]  (MFMA GEMM in both modes)
    if (int rc = clhip_gemm_nt(x, acat, P, nullptr, nullptr, nullptr, M, 32, D, D, D, 32, 0, 0, 0, dtype, stream)) return rc;
    const char* dk = static_cast<const char*>(dqkv) + (size_t)D * e;
    if (int rc = clhip_gemm_nt(dk, bcat, U, nullptr, nullptr, nullptr, M, 16, D, 3 * D, D, 32, 0, 0, 0, dtype, stream)) return rc;
    if (int rc = clhip_gemm_nt(dk + (size_t)D * e, bcat + (size_t)16 * D * e, U + 16 * e, nullptr, nullptr, nullptr, M, 16, D, 3 * D, D, 32, 0, 0, 0, dtype, stream))
        return rc;
    // K = M (tn_slab.hip): S_w = dY_w^T P[:, 16 w .. 16 w + 16) [D, 16] (w = k, v) and [d_a_k^T | d_a_v^T] = X^T U [D, 32]
    if (int rc = clhip_tn_slabs(dk, dtype, 3 * D, D, P, dtype, 32, 0, 16, slabS, M, D, 16, 2, rows, s)) return rc;
    if (int rc = clhip_tn_slabs(x, dtype, D, 0, U, dtype, 32, 0, 0, slabA, M, D, 32, 1, rows, s)) return rc;
    const size_t nred = (size_t)2 * D * 16 + (size_t)D * 32;
    hipLaunchKernelGGL(lorasub_reduce_kernel, dim3((unsigned)((nred + 255) / 256)), dim3(256), 0, s, slabS, slabA, nslab, D, rank, d_a_k, d_b_k, d_a_v, d_b_v);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

extern "C" int clhip_proj_adam_multi(int count, void* const* tensors, const float* const* transforms, float* ws, int D, int rank, float lr, float beta1,
                                     float beta2, float eps, float weight_decay, int step, void* stream) {
    CLHIP_CHECK_ARG(tensors && step >= 1);
    if (count < 4 || count % 4 || count > 65532) { clhip_set_error("clhip_proj_adam_multi: count = %d is not 4 per layer, up to 65532 (one grid row per tensor)", count); return CLHIP_EINVAL; }
    if (D <= 0 || D % 32) { clhip_set_error("clhip_proj_adam_multi: D = %d is not a positive multiple of 32", D); return CLHIP_EINVAL; }
    if (rank < 1 || rank > 16) { clhip_set_error("clhip_proj_adam_multi: rank %d is outside 1..16", rank); return CLHIP_EINVAL; }
    if (transforms && !ws) { clhip_set_error("clhip_proj_adam_multi: a projected step needs its workspace"); return CLHIP_EINVAL; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const AdamT* t = reinterpret_cast<const AdamT*>(tensors);
    const int n = D * rank;
    const float bc1 = 1.f - powf(beta1, (float)step);
    const float bc2s = sqrtf(1.f - powf(beta2, (float)step));
    const dim3 grid((n + 255) / 256, count);
    if (!transforms) {
        hipLaunchKernelGGL(proj_adam_moments_kernel<true>, grid, dim3(256), 0, s, t, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, (float*)nullptr);
        CLHIP_LAUNCH_CHECK();
        return CLHIP_OK;
    }
    hipLaunchKernelGGL(proj_adam_moments_kernel<false>, grid, dim3(256), 0, s, t, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, ws);
    hipLaunchKernelGGL(proj_adam_apply_kernel, dim3(D / 32, 2, count / 4), dim3(256), 0, s, t, transforms, ws, D, rank, lr, bc1);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}
