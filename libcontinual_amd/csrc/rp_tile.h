// rp_tile.h -- the operand staging of the exact-fp32 MFMA tile kernels (rp.hip, ca.hip, rapf.hip): a workgroup of kThreads owns a kTile x kTile output tile and
// advances K by kBK through LDS images stored k-major ([k][row]).  See rp.hip for the layout and its reasons.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(16))) float f32x16;

namespace rp_tile {

constexpr int kTile = 128;        // output tile edge
constexpr int kBK = 16;           // K block
constexpr int kThreads = 256;

template <bool KMAJOR> struct Operand {
    static constexpr int LD = KMAJOR ? kTile : kTile + 2;

    // this thread's share (two 4-element groups) of the [kBK x kTile] block at (k0, i0); rows >= I and k >= kend read as zero
    __device__ static __forceinline__ void fetch(const float* __restrict__ p, size_t ld, int I, int kend, int i0, int k0, bool vec, float4 (&r)[2]) {
        const int t = threadIdx.x;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (KMAJOR) {
                const int f = t + kThreads * h, k = k0 + (f >> 5), i = i0 + (f & 31) * 4;
                if (k < kend) {
                    const float* q = p + (size_t)k * ld + i;
                    if (vec && i + 4 <= I) {
                        const float4 u = *reinterpret_cast<const float4*>(q);
                        v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (i + e < I) v[e] = q[e];
                    }
                }
            } else {
                const int i = i0 + (t >> 2) + 64 * h, k = k0 + (t & 3) * 4;
                if (i < I) {
                    const float* q = p + (size_t)i * ld + k;
                    if (vec && k + 4 <= kend) {
                        const float4 u = *reinterpret_cast<const float4*>(q);
                        v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (k + e < kend) v[e] = q[e];
                    }
                }
            }
            r[h] = make_float4(v[0], v[1], v[2], v[3]);
        }
    }

    __device__ static __forceinline__ void stash(float* S, const float4 (&r)[2]) {
        const int t = threadIdx.x;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (KMAJOR) {
                const int f = t + kThreads * h;
                *reinterpret_cast<float4*>(S + (f >> 5) * LD + (f & 31) * 4) = r[h];
            } else {
                const int i = (t >> 2) + 64 * h, k = (t & 3) * 4;
                S[(k + 0) * LD + i] = r[h].x;
                S[(k + 1) * LD + i] = r[h].y;
                S[(k + 2) * LD + i] = r[h].z;
                S[(k + 3) * LD + i] = r[h].w;
            }
        }
    }
};

// Operand<false>::fetch for a lower-triangular operand (the Cholesky factors of ca.hip and rapf.hip): row j is read up to k = j only
__device__ __forceinline__ void fetch_lower(const float* __restrict__ p, size_t ld, int J, int kend, int j0, int k0, bool vec, float4 (&r)[2]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        const int j = j0 + (t >> 2) + 64 * h, k = k0 + (t & 3) * 4;
        if (j < J) {
            const int ke = min(kend, j + 1);
            const float* q = p + (size_t)j * ld + k;
            if (vec && k + 4 <= ke) {
                const float4 u = *reinterpret_cast<const float4*>(q);
                v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k + e < ke) v[e] = q[e];
            }
        }
        r[h] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

inline int vec_ok(const float* p, size_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; }
inline int tiles(int n) { return (n + kTile - 1) / kTile; }

}  // namespace rp_tile
