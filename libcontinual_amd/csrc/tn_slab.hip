// tn_slab.hip -- clhip_tn_slabs (contract: common.h): the K = M ("TN") products of the LoRA family.  The weight gradient of a low-rank factor is a sum over
// the M token rows of an activation-gradient column times a rank-sized projection column; one fp32 partial per row slab and no atomics, the caller sums the slabs
// in slab order (lora_db_reduce_kernel, sdlora_reduce_kernel), so two runs are bitwise equal.  Callers: clhip_lora_grad (vit_ops.hip), clhip_sdlora_grad (sdlora.hip).
#include "common.h"

namespace {
// Z in fp32: plain FMA, one thread per o, 16 columns j per workgroup, m ascending in 64-row LDS blocks of Z -- the fp32 parity mode, and
// bf16 Y where no bf16 Z exists.  Only the jn columns of the window are loaded: the last row of the last window may end the buffer.
template <typename T>
__global__ __launch_bounds__(256) void tn_slab_kernel(const T* __restrict__ Y, int ldy, int ystep, const float* __restrict__ Z, int ldz, int zstep, int j0step,
                                                       float* __restrict__ slab, int M, int O, int jn, int nw, int nt, int rows_per_slab) {
    __shared__ float ps[64][16];
    const int jt = blockIdx.z % nt, w = blockIdx.z / nt;
    const int jc = min(16, jn - jt * 16);                          // columns of this tile
    Y += (size_t)w * ystep;
    Z += (size_t)w * zstep + w * j0step + jt * 16;
    const int o = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    const int m0 = s * rows_per_slab, m1 = min(M, m0 + rows_per_slab);
    float acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    for (int mb = m0; mb < m1; mb += 64) {
        __syncthreads();
        for (int i = threadIdx.x; i < 64 * 16; i += 256) {
            const int r = i >> 4, q = i & 15;
            ps[r][q] = ((mb + r) < m1 && q < jc) ? Z[(size_t)(mb + r) * ldz + q] : 0.f;
        }
        __syncthreads();
        if (o < O) {
            const int nr = min(64, m1 - mb);
            for (int r = 0; r < nr; ++r) {
                const float dy = Elem<T>::ld(Y + (size_t)(mb + r) * ldy + o);
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[q] += dy * ps[r][q];
            }
        }
    }
    if (o < O) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (q < jc) slab[(((size_t)s * nw + w) * O + o) * jn + jt * 16 + q] = acc[q];
    }
}

// Y and Z in bf16 (O % 64 == 0): the same product on the bf16 MFMA.  Both operands are read with the transposing LDS read from row-major
// tiles (rows = m), 32 rows per step, k-slot j of lane group g <-> row 4 g + (j & 3) + 16 (j >> 2) on BOTH operands (the slot order of an
// MFMA is free), which keeps the reads bank-conflict free at these pitches.  Workgroup = 64 columns o x the 32 columns [32 jt, 32 jt + 32) of
// Z_w, read whole; wave v owns o in [16 v, 16 v + 16); the columns inside the window [j0_w, j0_w + jn) are stored.
constexpr int YP = 160, PP = 96;      // LDS pitches (bytes) of the Y tile rows (64 bf16) and the Z tile rows (32 bf16)

__global__ __launch_bounds__(256) void tn_slab_mfma_kernel(const bf16_t* __restrict__ Y, int ldy, int ystep, const bf16_t* __restrict__ Z, int ldz, int zstep,
                                                            int j0step, float* __restrict__ slab, int M, int O, int jn, int nw, int nt, int rows_per_slab) {
    __shared__ __attribute__((aligned(16))) char ys[2][32 * YP];
    __shared__ __attribute__((aligned(16))) char ps[2][32 * PP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int jt = blockIdx.z % nt, w = blockIdx.z / nt;
    const int o0 = blockIdx.x * 64;
    const int m0 = blockIdx.y * rows_per_slab, m1 = min(M, m0 + rows_per_slab);
    const int yr = tid >> 3, yc = tid & 7;                          // Y tile: 32 rows x 8 chunks
    const int pr = tid >> 2, pc = tid & 3;                          // Z tile: 32 rows x 4 chunks (threads < 128)
    const bf16_t* ysrc = Y + (size_t)w * ystep + o0 + yc * 8;
    const bf16_t* zsrc = Z + (size_t)w * zstep + jt * 32 + pc * 8;
    uint4 ry, rp;
    auto gload = [&](int mb) {
        const int my = mb + yr, mp = mb + pr;
        ry = my < m1 ? *reinterpret_cast<const uint4*>(ysrc + (size_t)my * ldy) : make_uint4(0, 0, 0, 0);
        if (tid < 128) rp = mp < m1 ? *reinterpret_cast<const uint4*>(zsrc + (size_t)mp * ldz) : make_uint4(0, 0, 0, 0);
    };
    auto sstore = [&](int st) {
        *reinterpret_cast<uint4*>(ys[st] + yr * YP + yc * 16) = ry;
        if (tid < 128) *reinterpret_cast<uint4*>(ps[st] + pr * PP + pc * 16) = rp;
    };
    const int ya = (g * 4 + (l15 >> 2)) * YP + (wave * 16 + (l15 & 3) * 4) * 2;
    const int pa = (g * 4 + (l15 >> 2)) * PP + (l15 & 3) * 8;
    f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
    if (m0 < m1) {
        gload(m0);
        sstore(0);
        __syncthreads();
        int st = 0;
        for (int mb = m0; mb < m1; mb += 32, st ^= 1) {
            const bool more = mb + 32 < m1;
            if (more) gload(mb + 32);
            const uint4 a = tr8(ys[st], ya, 16 * YP);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const uint4 b = tr8(ps[st], pa + t * 32, 16 * PP);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc[t], 0, 0, 0);
            }
            if (more) sstore(st ^ 1);
            __syncthreads();
        }
    }
    // D[row = o (4 g + e)][col = column l15 + 16 t of the Z tile]; keep the window
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int j = jt * 32 + l15 + 16 * t - w * j0step;
        if (j >= 0 && j < jn) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int o = o0 + wave * 16 + g * 4 + e;
                slab[(((size_t)blockIdx.y * nw + w) * O + o) * jn + j] = acc[t][e];
            }
        }
    }
}
}  // namespace

int clhip_tn_slabs(const void* Y, int ydtype, int ldy, int ystep, const void* Z, int zdtype, int ldz, int zstep, int j0step, float* slab, int M, int O, int jn,
                   int nw, int rows_per_slab, hipStream_t s) {
    CLHIP_CHECK_ARG(Y && Z && slab && M > 0 && O > 0 && jn > 0 && nw > 0 && rows_per_slab > 0 && j0step >= 0 && zstep >= 0 && ystep >= 0);
    CLHIP_CHECK_ARG((ydtype == CLHIP_BF16 || ydtype == CLHIP_F32) && (zdtype == CLHIP_F32 || (zdtype == CLHIP_BF16 && ydtype == CLHIP_BF16)));
    const int nslab = (M + rows_per_slab - 1) / rows_per_slab;
    if (zdtype == CLHIP_BF16) {
        const int nt = ((nw - 1) * j0step + jn + 31) / 32;          // whole 32-column tiles of Z_w, 16-byte loads
        CLHIP_CHECK_ARG(O % 64 == 0 && ldy % 8 == 0 && ystep % 8 == 0 && ldz % 8 == 0 && zstep % 8 == 0 && (nw - 1) * zstep + nt * 32 <= ldz);
        hipLaunchKernelGGL(tn_slab_mfma_kernel, dim3(O / 64, nslab, nw * nt), dim3(256), 0, s, (const bf16_t*)Y, ldy, ystep, (const bf16_t*)Z, ldz, zstep, j0step, slab,
                           M, O, jn, nw, nt, rows_per_slab);
    } else {
        const int nt = (jn + 15) / 16;
        CLHIP_CHECK_ARG((nw - 1) * (zstep + j0step) + jn <= ldz);
        const dim3 grid((O + 255) / 256, nslab, nw * nt);
        if (ydtype == CLHIP_BF16)
            hipLaunchKernelGGL(tn_slab_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)Y, ldy, ystep, (const float*)Z, ldz, zstep, j0step, slab, M, O, jn, nw, nt,
                               rows_per_slab);
        else
            hipLaunchKernelGGL(tn_slab_kernel<float>, grid, dim3(256), 0, s, (const float*)Y, ldy, ystep, (const float*)Z, ldz, zstep, j0step, slab, M, O, jn, nw, nt,
                               rows_per_slab);
    }
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}
