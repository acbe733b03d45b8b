// coda.hip -- CODA-Prompt's prompt assembly (reference core/model/backbone/prompt.py:158-220, CodaPrompt.forward) for all prompted layers at once, exact fp32.
// Per layer, with K, A [pool, D], P [pool, L, D] and the query q [B, D] (the cls feature of a prompt-free forward), over the components k < f:
//     c[b,k]  = <q_b * A_k, K_k> / (max(|q_b * A_k|, eps) max(|K_k|, eps))        (prompt.py:190-194: F.normalize on both factors, eps 1e-12)
//     P_[b]   = sum_{k<f} c[b,k] P[k]                                             (prompt.py:196)
//     ek = P_[:, :L/2], ev = P_[:, L/2:]                                          (prompt.py:199-201), stored in the compute dtype as [B, L/2, D]:
// what clhip_attn_prefix_fwd takes as pk / pv.  The backward takes dpk, dpv (fp32, [B, L/2, D]) and writes rows [s, f) of dK, dA, dP -- the components the
// running task trains (prompt.py:174-182: rows below s are detached) -- and nothing else.  Every sum runs in a fixed order: no atomics.
// The clamp is differentiated as torch does: y = x / max(|x|, eps) has dy/dx = 1 / m - [|x| >= eps] x x^T / (m^2 |x|), m = max(|x|, eps).
#include "common.h"

namespace {

constexpr int kMaxLayers = 8;
constexpr float kEps = 1e-12f;

struct CodaTable {
    const float* K[kMaxLayers]; const float* A[kMaxLayers]; const float* P[kMaxLayers];
    void* ek[kMaxLayers]; void* ev[kMaxLayers];
    const float* dpk[kMaxLayers]; const float* dpv[kMaxLayers];
    float* dK[kMaxLayers]; float* dA[kMaxLayers]; float* dP[kMaxLayers];
};

// the three sums of one (sample, component): <q*A, K>, |q*A|^2, |K|^2, every lane of the wave gets all three
__device__ __forceinline__ void coda_sums(const float* q, const float* A, const float* K, int D, int lane, float& num, float& na2, float& nk2) {
    num = na2 = nk2 = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float a = q[d] * A[d], k = K[d];
        num += a * k; na2 += a * a; nk2 += k * k;
    }
    num = wave_sum(num); na2 = wave_sum(na2); nk2 = wave_sum(nk2);
}

// grid (B, layers): the f coefficients of one sample (a wave per component), then its L x D mixed prompt (a thread per element, k in order)
template <typename T>
__global__ __launch_bounds__(256) void coda_fwd_kernel(CodaTable t, const float* __restrict__ q, float* __restrict__ c, int l0, int B, int D, int L, int f) {
    const int b = blockIdx.x, l = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* qb = q + (size_t)b * D;
    float* cb = c + ((size_t)(l0 + l) * B + b) * f;
    for (int k = wave; k < f; k += 4) {
        float num, na2, nk2;
        coda_sums(qb, t.A[l] + (size_t)k * D, t.K[l] + (size_t)k * D, D, lane, num, na2, nk2);
        if (lane == 0) cb[k] = num / (fmaxf(sqrtf(na2), kEps) * fmaxf(sqrtf(nk2), kEps));
    }
    __syncthreads();                                              // (a workgroup-scope fence as well: cb is read back below)
    const int Lp = L >> 1, LD = L * D;
    const float* P = t.P[l];
    for (int i = threadIdx.x; i < LD; i += 256) {
        float acc = 0.f;
        for (int k = 0; k < f; ++k) acc += cb[k] * P[(size_t)k * LD + i];
        const int r = i / D, d = i - r * D;
        T* dst = r < Lp ? static_cast<T*>(t.ek[l]) + ((size_t)b * Lp + r) * D + d : static_cast<T*>(t.ev[l]) + ((size_t)b * Lp + (r - Lp)) * D + d;
        Elem<T>::st(dst, acc);
    }
}

// workspace of the backward, per layer: dc, num, na [B, f - s] each, then nk [f - s]
__host__ __device__ inline size_t coda_ws_layer(int B, int n) { return (size_t)3 * B * n + n; }

// grid (B, layers): per component k in [s, f) of one sample dc = <dP_[b], P[k]> and the forward's sums
__global__ __launch_bounds__(256) void coda_bwd_coef_kernel(CodaTable t, const float* __restrict__ q, float* __restrict__ ws, int l0, int B, int D, int L, int s,
                                                            int f) {
    const int b = blockIdx.x, l = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = f - s, Lp = L >> 1, half = Lp * D, LD = L * D;
    float* w = ws + (size_t)(l0 + l) * coda_ws_layer(B, n);
    const float* qb = q + (size_t)b * D;
    const float* gk = t.dpk[l] + (size_t)b * half;
    const float* gv = t.dpv[l] + (size_t)b * half;
    for (int k = s + wave; k < f; k += 4) {
        const float* P = t.P[l] + (size_t)k * LD;
        float dc = 0.f;
        for (int i = lane; i < half; i += 64) dc += gk[i] * P[i];
        for (int i = lane; i < half; i += 64) dc += gv[i] * P[half + i];
        dc = wave_sum(dc);
        float num, na2, nk2;
        coda_sums(qb, t.A[l] + (size_t)k * D, t.K[l] + (size_t)k * D, D, lane, num, na2, nk2);
        if (lane == 0) {
            const int j = k - s;
            w[(size_t)b * n + j] = dc;
            w[(size_t)(B + b) * n + j] = num;
            w[(size_t)(2 * B + b) * n + j] = sqrtf(na2);
            if (b == 0) w[(size_t)3 * B * n + j] = sqrtf(nk2);
        }
    }
}

// grid (chunks of 256 over D + L*D, f - s, layers): a thread owns column d of dA / dK of its component, or one element of its dP; batch in order
__global__ __launch_bounds__(256) void coda_bwd_param_kernel(CodaTable t, const float* __restrict__ q, const float* __restrict__ c, const float* __restrict__ ws,
                                                             int l0, int B, int D, int L, int s, int f) {
    const int j = blockIdx.y, k = s + j, l = blockIdx.z, n = f - s;
    const int i = blockIdx.x * 256 + threadIdx.x, Lp = L >> 1, half = Lp * D, LD = L * D;
    const float* w = ws + (size_t)(l0 + l) * coda_ws_layer(B, n);
    if (i < D) {
        const float Kd = t.K[l][(size_t)k * D + i], Ad = t.A[l][(size_t)k * D + i];
        const float nk = w[(size_t)3 * B * n + j], mk = fmaxf(nk, kEps);
        float dA = 0.f, dKa = 0.f, S = 0.f;
        for (int b = 0; b < B; ++b) {
            const float dc = w[(size_t)b * n + j], num = w[(size_t)(B + b) * n + j], na = w[(size_t)(2 * B + b) * n + j];
            const float ma = fmaxf(na, kEps), qd = q[(size_t)b * D + i], aq = qd * Ad;
            const float tt = na >= kEps ? num / (ma * na) : 0.f;       // the norm's own derivative, where the clamp lets it through
            dA += qd * (dc / (ma * mk)) * (Kd - tt * aq);
            dKa += (dc / ma) * aq;
            S += dc * num / ma;
        }
        t.dA[l][(size_t)k * D + i] = dA;
        t.dK[l][(size_t)k * D + i] = dKa / mk - (nk >= kEps ? S / (mk * mk * nk) * Kd : 0.f);
    } else if (i - D < LD) {
        const int e = i - D;
        const float* g = e < half ? t.dpk[l] + e : t.dpv[l] + (e - half);
        const float* ck = c + (size_t)(l0 + l) * B * f + k;
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += ck[(size_t)b * f] * g[(size_t)b * half];
        t.dP[l][(size_t)k * LD + e] = acc;
    }
}

int coda_check(int layers, int B, int D, int pool, int L, int s, int f) {
    CLHIP_CHECK_ARG(layers > 0 && B > 0 && D > 0 && D % 64 == 0 && pool > 0 && L >= 2 && L % 2 == 0 && f >= 1 && f <= pool && s >= 0 && s < f);
    return CLHIP_OK;
}

}  // namespace

extern "C" size_t clhip_coda_ws_bytes(int layers, int B, int s, int f) {
    if (layers <= 0 || B <= 0 || s < 0 || f <= s) return 0;
    return (size_t)layers * coda_ws_layer(B, f - s) * sizeof(float);
}

extern "C" int clhip_coda_fwd(int layers, const float* q, const float* const* K, const float* const* A, const float* const* P, void* const* ek, void* const* ev,
                              float* c, int B, int D, int pool, int L, int f, int dtype, void* stream) {
    CLHIP_CHECK_ARG(q && K && A && P && ek && ev && c);
    if (int rc = coda_check(layers, B, D, pool, L, 0, f)) return rc;
    CLHIP_CHECK_ARG(dtype == CLHIP_BF16 || dtype == CLHIP_F32);
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int l0 = 0; l0 < layers; l0 += kMaxLayers) {
        const int n = layers - l0 < kMaxLayers ? layers - l0 : kMaxLayers;
        CodaTable t = {};
        for (int i = 0; i < n; ++i) {
            CLHIP_CHECK_ARG(K[l0 + i] && A[l0 + i] && P[l0 + i] && ek[l0 + i] && ev[l0 + i]);
            t.K[i] = K[l0 + i]; t.A[i] = A[l0 + i]; t.P[i] = P[l0 + i]; t.ek[i] = ek[l0 + i]; t.ev[i] = ev[l0 + i];
        }
        if (dtype == CLHIP_BF16) hipLaunchKernelGGL(coda_fwd_kernel<bf16_t>, dim3(B, n), dim3(256), 0, st, t, q, c, l0, B, D, L, f);
        else hipLaunchKernelGGL(coda_fwd_kernel<float>, dim3(B, n), dim3(256), 0, st, t, q, c, l0, B, D, L, f);
        CLHIP_LAUNCH_CHECK();
    }
    return CLHIP_OK;
}

extern "C" int clhip_coda_bwd(int layers, const float* q, const float* const* K, const float* const* A, const float* const* P, const float* c,
                              const float* const* dpk, const float* const* dpv, float* const* dK, float* const* dA, float* const* dP, float* ws, int B, int D,
                              int pool, int L, int s, int f, void* stream) {
    CLHIP_CHECK_ARG(q && K && A && P && c && dpk && dpv && dK && dA && dP && ws);
    if (int rc = coda_check(layers, B, D, pool, L, s, f)) return rc;
    CLHIP_CHECK_ARG(f - s <= 65535);
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int l0 = 0; l0 < layers; l0 += kMaxLayers) {
        const int n = layers - l0 < kMaxLayers ? layers - l0 : kMaxLayers;
        CodaTable t = {};
        for (int i = 0; i < n; ++i) {
            const int l = l0 + i;
            CLHIP_CHECK_ARG(K[l] && A[l] && P[l] && dpk[l] && dpv[l] && dK[l] && dA[l] && dP[l]);
            t.K[i] = K[l]; t.A[i] = A[l]; t.P[i] = P[l]; t.dpk[i] = dpk[l]; t.dpv[i] = dpv[l]; t.dK[i] = dK[l]; t.dA[i] = dA[l]; t.dP[i] = dP[l];
        }
        hipLaunchKernelGGL(coda_bwd_coef_kernel, dim3(B, n), dim3(256), 0, st, t, q, ws, l0, B, D, L, s, f);
        hipLaunchKernelGGL(coda_bwd_param_kernel, dim3((D + L * D + 255) / 256, f - s, n), dim3(256), 0, st, t, q, c, ws, l0, B, D, L, s, f);
        CLHIP_LAUNCH_CHECK();
    }
    return CLHIP_OK;
}
