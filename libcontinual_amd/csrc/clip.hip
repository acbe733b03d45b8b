// clip.hip -- the image side of CLIP's logits (core/model/backbone/clip.py:405-412): the pooled ln_post features through visual.proj, the
// L2 normalisation and the scaled cosine product against ALREADY normalised text features, and the input gradient of all three.  Exact fp32, no
// atomics, every sum in a fixed order (ascending index per thread, then the xor butterfly of a wave, then the four waves in order): two runs are
// bitwise equal.  One launch each way; `linear` + `cosine_linear` would normalise the text rows a second time (not the reference's arithmetic)
// and take three launches and two scratch buffers each way.  One workgroup per image: the tensors are a few hundred KB and stay in L2.
#include "common.h"

namespace {

constexpr int CLIP_MAX_DIM = 4096;      // D + E floats of LDS per workgroup (16 KB at the limit)

// u = feat[b] . proj, n = u / |u|, logits[b] = scale * n . txt^T
__global__ __launch_bounds__(256) void clip_logits_fwd_kernel(const float* __restrict__ feat, const float* __restrict__ proj, const float* __restrict__ txt,
                                                               float scale, float* __restrict__ logits, float* __restrict__ u_out, float* __restrict__ inv_out,
                                                               int D, int E, int C) {
    extern __shared__ float lds[];
    float* f = lds;                      // [D]
    float* n = lds + D;                  // [E]: u, then u / |u|
    __shared__ float red[4];
    const int b = blockIdx.x, t = threadIdx.x;
    for (int d = t; d < D; d += 256) f[d] = feat[(size_t)b * D + d];
    __syncthreads();
    float ss = 0.f;
    for (int e = t; e < E; e += 256) {
        float a = 0.f;
        for (int d = 0; d < D; ++d) a = fmaf(f[d], proj[(size_t)d * E + e], a);
        n[e] = a;
        u_out[(size_t)b * E + e] = a;
        ss = fmaf(a, a, ss);
    }
    ss = block_sum_256(ss, red);         // (its barriers also publish n)
    const float inv = 1.0f / sqrtf(ss);  // no eps, as in the reference: a zero row gives inf / NaN logits and is the caller's problem
    if (t == 0) inv_out[b] = inv;
    for (int e = t; e < E; e += 256) n[e] *= inv;
    __syncthreads();
    const int lane = t & 63;
    for (int c = t >> 6; c < C; c += 4) {
        float a = 0.f;
        for (int e = lane; e < E; e += 64) a = fmaf(n[e], txt[(size_t)c * E + e], a);
        a = wave_sum(a);
        if (lane == 0) logits[(size_t)b * C + c] = scale * a;
    }
}

// g = scale * dlogits[b] . txt, du = (g - n (n . g)) / |u|, dfeat[b] = proj . du
__global__ __launch_bounds__(256) void clip_logits_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ proj, const float* __restrict__ txt,
                                                               float scale, const float* __restrict__ u, const float* __restrict__ inv_in,
                                                               float* __restrict__ dfeat, int D, int E, int C) {
    extern __shared__ float lds[];
    float* du = lds;                     // [E]
    float* dl = lds + E;                 // [C]
    __shared__ float red[4];
    const int b = blockIdx.x, t = threadIdx.x;
    for (int c = t; c < C; c += 256) dl[c] = dlogits[(size_t)b * C + c];
    __syncthreads();
    const float inv = inv_in[b];
    float ng = 0.f;
    for (int e = t; e < E; e += 256) {
        float g = 0.f;
        for (int c = 0; c < C; ++c) g = fmaf(dl[c], txt[(size_t)c * E + e], g);
        g *= scale;
        du[e] = g;
        ng = fmaf(u[(size_t)b * E + e] * inv, g, ng);
    }
    ng = block_sum_256(ng, red);
    for (int e = t; e < E; e += 256) du[e] = (du[e] - u[(size_t)b * E + e] * inv * ng) * inv;      // (each thread rewrites its own elements)
    __syncthreads();
    const int lane = t & 63;
    for (int d = t >> 6; d < D; d += 4) {
        float a = 0.f;
        for (int e = lane; e < E; e += 64) a = fmaf(proj[(size_t)d * E + e], du[e], a);
        a = wave_sum(a);
        if (lane == 0) dfeat[(size_t)b * D + d] = a;
    }
}

}  // namespace

extern "C" int clhip_clip_logits_fwd(const float* feat, const float* proj, const float* txt, float scale, float* logits, float* u, float* inv_norm, int B, int D,
                                     int E, int C, void* stream) {
    CLHIP_CHECK_ARG(feat && proj && txt && logits && u && inv_norm);
    CLHIP_CHECK_ARG(B > 0 && D > 0 && E > 0 && C > 0 && D + E <= CLIP_MAX_DIM && E + C <= CLIP_MAX_DIM);      // (E + C: what the backward of this call needs)
    hipLaunchKernelGGL(clip_logits_fwd_kernel, dim3(B), dim3(256), (size_t)(D + E) * sizeof(float), static_cast<hipStream_t>(stream), feat, proj, txt, scale, logits, u,
                       inv_norm, D, E, C);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

extern "C" int clhip_clip_logits_bwd(const float* dlogits, const float* proj, const float* txt, float scale, const float* u, const float* inv_norm, float* dfeat,
                                     int B, int D, int E, int C, void* stream) {
    CLHIP_CHECK_ARG(dlogits && proj && txt && u && inv_norm && dfeat);
    CLHIP_CHECK_ARG(B > 0 && D > 0 && E > 0 && C > 0 && D + E <= CLIP_MAX_DIM && E + C <= CLIP_MAX_DIM);
    hipLaunchKernelGGL(clip_logits_bwd_kernel, dim3(B), dim3(256), (size_t)(E + C) * sizeof(float), static_cast<hipStream_t>(stream), dlogits, proj, txt, scale, u,
                       inv_norm, dfeat, D, E, C);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}
