// dual.hip -- DualPrompt's prompt selection (reference core/model/backbone/prompt.py:269-337, DualPrompt.forward) for all prompted layers at once, exact fp32.
// G-layers (prompt.py:310-316): g_p [Lg, D] is every sample's prefix, rows [0, Lg/2) the keys, rows [Lg/2, Lg) the values.
// E-layers (prompt.py:272-306), with the keys e_k [pool, D], the prompts e_p [pool, Le, D] and the query q [B, D] (the cls feature of a prompt-free forward):
//     cos[b,k] = <q_b, K_k> / (max(|q_b|, eps) max(|K_k|, eps))                     (prompt.py:279-281: F.normalize on both sides, eps 1e-12)
//     train:  idx[b] = task_id,  loss_l = sum_b (1 - cos[b, task_id])               (prompt.py:285-287, task_id_bootstrap)
//     eval:   idx[b] = argmax_k cos[b,k], ties to the lowest k                      (prompt.py:294-296, top-1)
//     pk = e_p[idx[b]][:Le/2], pv = e_p[idx[b]][Le/2:]                              (prompt.py:299-306), stored in the compute dtype as [B, Le/2, D]:
// what clhip_attn_prefix_fwd takes as pk / pv.  The key loss is the sum of loss_l over the E-layers in order, each summed over b in order (transformer.py:2279).
// The backward takes dpk, dpv (fp32, [B, L/2, D]) and writes dg_p = sum_b [dpk_b | dpv_b], row task_id of de_p by the same sum, and row task_id of de_k, the
// gradient of the key loss times its cotangent -- and nothing else.  Every sum runs in a fixed order: no atomics.
// The clamp is differentiated as torch does: y = x / max(|x|, eps) has dy/dx = 1 / m - [|x| >= eps] x x^T / (m^2 |x|), m = max(|x|, eps).  With
// s = sum_b q_b / max(|q_b|, eps) and K the task's key:  d loss_l / dK = -s / m + [|K| >= eps] <s, K> K / (m^2 |K|).
#include "common.h"

namespace {

constexpr int kMaxLayers = 8;          // of each kind
constexpr float kEps = 1e-12f;

struct DualFwdTable {
    const float* g_p[kMaxLayers]; const float* e_k[kMaxLayers]; const float* e_p[kMaxLayers];
    void* pk[2 * kMaxLayers]; void* pv[2 * kMaxLayers];                // G-layers first, then E-layers
};

struct DualBwdTable {
    const float* e_k[kMaxLayers];
    const float* dpk[2 * kMaxLayers]; const float* dpv[2 * kMaxLayers];
    float* dg_p[kMaxLayers]; float* de_k[kMaxLayers]; float* de_p[kMaxLayers];
};

// the cosine of one (sample, key), every lane of the wave gets it
__device__ __forceinline__ float dual_cos(const float* q, const float* K, int D, int lane) {
    float num = 0.f, nq2 = 0.f, nk2 = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float a = q[d], k = K[d];
        num += a * k; nq2 += a * a; nk2 += k * k;
    }
    num = wave_sum(num); nq2 = wave_sum(nq2); nk2 = wave_sum(nk2);
    return num / (fmaxf(sqrtf(nq2), kEps) * fmaxf(sqrtf(nk2), kEps));
}

// rows [0, L/2) of src [L, D] -> pk[b], rows [L/2, L) -> pv[b]: a thread per element
template <typename T>
__device__ __forceinline__ void dual_copy(const float* src, void* pk, void* pv, int b, int L, int D) {
    const int Lp = L >> 1, LD = L * D;
    for (int i = threadIdx.x; i < LD; i += 256) {
        const int r = i / D, d = i - r * D;
        T* dst = r < Lp ? static_cast<T*>(pk) + ((size_t)b * Lp + r) * D + d : static_cast<T*>(pv) + ((size_t)b * Lp + (r - Lp)) * D + d;
        Elem<T>::st(dst, src[i]);
    }
}

// grid (B, n_g + n_e [+ 1 in train mode]): row y < n_g copies a G-prompt; the next n_e rows compute the pool cosines of one sample (a wave per key), select and
// copy; the last row's first workgroup sums the key loss, b in order per layer, then the layers in order
template <typename T>
__global__ __launch_bounds__(256) void dual_fwd_kernel(DualFwdTable t, const float* __restrict__ q, float* __restrict__ cos, int* __restrict__ idx,
                                                       float* __restrict__ loss, int n_g, int n_e, int B, int D, int pool, int Lg, int Le, int train, int task_id) {
    const int b = blockIdx.x, y = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ float part[256];
    __shared__ int sel;
    if (y < n_g) {
        dual_copy<T>(t.g_p[y], t.pk[y], t.pv[y], b, Lg, D);
        return;
    }
    if (y == n_g + n_e) {
        if (b) return;
        float total = 0.f;
        for (int l = 0; l < n_e; ++l) {
            const float* K = t.e_k[l] + (size_t)task_id * D;
            float layer = 0.f;
            for (int b0 = 0; b0 < B; b0 += 256) {
                const int nb = B - b0 < 256 ? B - b0 : 256;
                for (int j = wave; j < nb; j += 4) {
                    const float c = dual_cos(q + (size_t)(b0 + j) * D, K, D, lane);
                    if (lane == 0) part[j] = 1.f - c;
                }
                __syncthreads();
                if (threadIdx.x == 0)
                    for (int j = 0; j < nb; ++j) layer += part[j];
                __syncthreads();
            }
            total += layer;
        }
        if (threadIdx.x == 0) *loss = total;
        return;
    }
    const int l = y - n_g;
    const float* qb = q + (size_t)b * D;
    float* cb = cos + ((size_t)l * B + b) * pool;
    for (int k = wave; k < pool; k += 4) {
        const float c = dual_cos(qb, t.e_k[l] + (size_t)k * D, D, lane);
        if (lane == 0) cb[k] = c;
    }
    __syncthreads();                                              // (a workgroup-scope fence as well: cb is read back below)
    if (threadIdx.x == 0) {
        int best = task_id;
        if (!train) {
            best = 0;
            float top = cb[0];
            for (int k = 1; k < pool; ++k)
                if (cb[k] > top) { top = cb[k]; best = k; }      // strict: an exact tie stays with the lower index
        }
        sel = best;
        idx[(size_t)l * B + b] = best;
    }
    __syncthreads();
    dual_copy<T>(t.e_p[l] + (size_t)sel * Le * D, t.pk[y], t.pv[y], b, Le, D);
}

// grid (nx + 1, n_g + n_e): the first nx columns own one element of dg_p / of row task_id of de_p each (a thread per element, batch in order); the last
// column's workgroup of an E-layer writes row task_id of de_k
__global__ __launch_bounds__(256) void dual_bwd_kernel(DualBwdTable t, const float* __restrict__ q, const float* __restrict__ dloss, int n_g, int nx, int B, int D,
                                                       int Lg, int Le, int task_id) {
    const int y = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool is_e = y >= n_g;
    if ((int)blockIdx.x < nx) {
        const int L = is_e ? Le : Lg, half = (L >> 1) * D, LD = L * D;
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i >= LD) return;
        const float* g = i < half ? t.dpk[y] + i : t.dpv[y] + (i - half);
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += g[(size_t)b * half];
        float* out = is_e ? t.de_p[y - n_g] + (size_t)task_id * LD : t.dg_p[y];
        out[i] = acc;
        return;
    }
    if (!is_e) return;
    const int l = y - n_g;
    const float* K = t.e_k[l] + (size_t)task_id * D;
    float* dK = t.de_k[l] + (size_t)task_id * D;
    __shared__ float mq[256];
    __shared__ float red[8];
    float S = 0.f, nk2 = 0.f;
    for (int d0 = 0; d0 < D; d0 += 256) {
        const int d = d0 + threadIdx.x;
        float s = 0.f;                                            // column d of sum_b q_b / max(|q_b|, eps)
        for (int b0 = 0; b0 < B; b0 += 256) {
            const int nb = B - b0 < 256 ? B - b0 : 256;
            __syncthreads();                                      // the readers of the previous chunk are done
            for (int j = wave; j < nb; j += 4) {
                const float* qb = q + (size_t)(b0 + j) * D;
                float nq2 = 0.f;
                for (int e = lane; e < D; e += 64) nq2 += qb[e] * qb[e];
                nq2 = wave_sum(nq2);
                if (lane == 0) mq[j] = fmaxf(sqrtf(nq2), kEps);
            }
            __syncthreads();
            if (d < D)
                for (int j = 0; j < nb; ++j) s += q[(size_t)(b0 + j) * D + d] / mq[j];
        }
        if (d < D) {
            const float kd = K[d];
            dK[d] = s;                                            // parked in the output row: the same thread reads it back below
            S += s * kd; nk2 += kd * kd;
        }
    }
    S = wave_sum(S); nk2 = wave_sum(nk2);
    if (lane == 0) { red[wave] = S; red[4 + wave] = nk2; }
    __syncthreads();
    S = red[0] + red[1] + red[2] + red[3];
    nk2 = red[4] + red[5] + red[6] + red[7];
    const float nk = sqrtf(nk2), mk = fmaxf(nk, kEps), g = *dloss;
    const float coef = nk >= kEps ? S / (mk * mk * nk) : 0.f;     // the norm's own derivative, where the clamp lets it through
    for (int d = threadIdx.x; d < D; d += 256) dK[d] = g * (coef * K[d] - dK[d] / mk);
}

int dual_check(int n_g, int n_e, int B, int D, int pool, int Lg, int Le, int task_id) {
    CLHIP_CHECK_ARG(n_g >= 0 && n_e >= 0 && n_g + n_e > 0 && n_g <= kMaxLayers && n_e <= kMaxLayers);
    CLHIP_CHECK_ARG(B > 0 && D > 0 && D % 64 == 0);
    CLHIP_CHECK_ARG(n_g == 0 || (Lg >= 2 && Lg % 2 == 0));
    CLHIP_CHECK_ARG(n_e == 0 || (Le >= 2 && Le % 2 == 0 && pool > 0 && task_id >= 0 && task_id < pool));
    CLHIP_CHECK_ARG((n_g == 0 || (long long)Lg * D < (1LL << 30)) && (n_e == 0 || (long long)Le * D < (1LL << 30)));      // element indices are ints
    return CLHIP_OK;
}

}  // namespace

extern "C" int clhip_dual_fwd(int n_g, int n_e, const float* q, const float* const* g_p, const float* const* e_k, const float* const* e_p, void* const* pk,
                              void* const* pv, float* cos, int* idx, float* loss, int B, int D, int pool, int Lg, int Le, int train, int task_id, int dtype,
                              void* stream) {
    if (int rc = dual_check(n_g, n_e, B, D, pool, Lg, Le, n_e > 0 && train ? task_id : 0)) return rc;
    CLHIP_CHECK_ARG(pk && pv && (n_g == 0 || g_p) && (n_e == 0 || (q && e_k && e_p && cos && idx)) && (!train || loss));
    CLHIP_CHECK_ARG(dtype == CLHIP_BF16 || dtype == CLHIP_F32);
    DualFwdTable t = {};
    for (int i = 0; i < n_g; ++i) {
        CLHIP_CHECK_ARG(g_p[i]);
        t.g_p[i] = g_p[i];
    }
    for (int i = 0; i < n_e; ++i) {
        CLHIP_CHECK_ARG(e_k[i] && e_p[i]);
        t.e_k[i] = e_k[i]; t.e_p[i] = e_p[i];
    }
    for (int i = 0; i < n_g + n_e; ++i) {
        CLHIP_CHECK_ARG(pk[i] && pv[i]);
        t.pk[i] = pk[i]; t.pv[i] = pv[i];
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(B, n_g + n_e + (train ? 1 : 0));
    if (dtype == CLHIP_BF16)
        hipLaunchKernelGGL(dual_fwd_kernel<bf16_t>, grid, dim3(256), 0, st, t, q, cos, idx, loss, n_g, n_e, B, D, pool, Lg, Le, train ? 1 : 0, task_id);
    else
        hipLaunchKernelGGL(dual_fwd_kernel<float>, grid, dim3(256), 0, st, t, q, cos, idx, loss, n_g, n_e, B, D, pool, Lg, Le, train ? 1 : 0, task_id);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

extern "C" int clhip_dual_bwd(int n_g, int n_e, const float* q, const float* const* e_k, const float* const* dpk, const float* const* dpv, const float* dloss,
                              float* const* dg_p, float* const* de_k, float* const* de_p, int B, int D, int pool, int Lg, int Le, int task_id, void* stream) {
    if (int rc = dual_check(n_g, n_e, B, D, pool, Lg, Le, task_id)) return rc;
    CLHIP_CHECK_ARG(dpk && dpv && (n_g == 0 || dg_p) && (n_e == 0 || (q && e_k && dloss && de_k && de_p)));
    DualBwdTable t = {};
    for (int i = 0; i < n_g; ++i) {
        CLHIP_CHECK_ARG(dg_p[i]);
        t.dg_p[i] = dg_p[i];
    }
    for (int i = 0; i < n_e; ++i) {
        CLHIP_CHECK_ARG(e_k[i] && de_k[i] && de_p[i]);
        t.e_k[i] = e_k[i]; t.de_k[i] = de_k[i]; t.de_p[i] = de_p[i];
    }
    for (int i = 0; i < n_g + n_e; ++i) {
        CLHIP_CHECK_ARG(dpk[i] && dpv[i]);
        t.dpk[i] = dpk[i]; t.dpv[i] = dpv[i];
    }
    const int Lmax = (n_g && (!n_e || Lg > Le)) ? Lg : Le;
    const int nx = (Lmax * D + 255) / 256;
    hipLaunchKernelGGL(dual_bwd_kernel, dim3(nx + 1, n_g + n_e), dim3(256), 0, static_cast<hipStream_t>(stream), t, q, dloss, n_g, nx, B, D, Lg, Le, task_id);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}
