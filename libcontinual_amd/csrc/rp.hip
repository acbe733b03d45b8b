// rp.hip -- RanPAC's random-projection ridge classifier (reference core/model/ranpac.py:49-63, 214-266) on the exact fp32 MFMA of gfx950.
//
// Every product here is fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32, whose result is bit for bit a k-ordered fmaf chain: the ridge solves that
// consume G and Q amplify operand errors, so the bf16 MFMA kernels of gemm.hip are no option.  No kernel uses atomics and every summation order is a
// function of the shapes only, so repeated runs give the same bits.
//
// One tile kernel serves the three products.  A workgroup of 4 waves owns a 128 x 128 output tile, each wave a 64 x 64 quarter as 2 x 2 MFMA tiles of
// 32 x 32 (4 independent accumulators per wave: the 64-cycle issue interval of the instruction is covered).  K advances 16 at a time through LDS images
// stored k-major ([k][row]), which is what the MFMA operand map wants: lane l reads element [k = l >> 5][l & 31], 32 consecutive floats per half wave,
// conflict-free for ds_read_b32 whatever the row pitch.  The next K block is fetched into registers while the current one is multiplied.
// An operand is either "k-major" in memory (element (k, i) at p[k * ld + i]: W_rand, and H for both sides of H^T H) and goes to LDS with 16-byte
// stores, or "k-contiguous" (element (i, k) at p[i * ld + k]: the feature rows, the hidden rows, Wo) and is transposed on its way in; pitch 130 makes
// those transposing ds_write_b32 conflict-free (the four k-quads of a half wave land 8 banks apart).
// The ragged edge is the normal case (M = 10000 = 78 * 128 + 16): loads outside the matrix read as zero, stores are guarded, and the 16-byte global
// loads are taken only where the pitch is a multiple of 4, the base is 16-byte aligned and the whole vector is inside -- element loads otherwise.
#include <mutex>

#include "rp_tile.h"

using namespace rp_tile;

namespace {

constexpr int kSplitK = 512;      // K slice of the classify product (partials are summed in slice order)
constexpr int kLabelCols = 256;   // columns of H per label-sum workgroup
constexpr int kLabelClasses = 8;  // classes per label-sum workgroup

enum { MODE_STORE = 0, MODE_GRAM = 1 };

// out tile (i, j) = sum_k a(i, k) * b(k, j) over k in [z * kslice, min(K, (z + 1) * kslice)), z = blockIdx.z.
// MODE_STORE: out[z * zstride + i * ldo + j] = (relu ? max(., 0) : .).
// MODE_GRAM : a == b == H (k-major, I == J == M); blockIdx.x enumerates the tiles on or above the diagonal; G(i, j) += tile, and the SAME sum is
//             written to G(j, i) for an off-diagonal tile.  A diagonal tile is symmetric by construction: its (i, j) and (j, i) elements are the same
//             k-ordered chain of the same (commutative) products.
template <bool A_KMAJOR, bool B_KMAJOR, int MODE>
__global__ __launch_bounds__(kThreads) void rp_tile_kernel(const float* __restrict__ a, size_t lda, int avec, const float* __restrict__ b, size_t ldb,
                                                           int bvec, float* __restrict__ out, size_t ldo, size_t zstride, int I, int J, int K,
                                                           int kslice, int relu) {
    using OA = Operand<A_KMAJOR>;
    using OB = Operand<B_KMAJOR>;
    __shared__ __attribute__((aligned(16))) float As[kBK * OA::LD];
    __shared__ __attribute__((aligned(16))) float Bs[kBK * OB::LD];
    int ti, tj;
    if (MODE == MODE_GRAM) {
        const int T = (I + kTile - 1) / kTile;
        int t = blockIdx.x;
        ti = 0;
        while (t >= T - ti) {
            t -= T - ti;
            ++ti;
        }
        tj = ti + t;
    } else {
        tj = blockIdx.x;
        ti = blockIdx.y;
    }
    const int i0 = ti * kTile, j0 = tj * kTile;
    const int kbeg = blockIdx.z * kslice;
    const int kend = min(K, kbeg + kslice);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    const int lr = lane & 31, lk = lane >> 5;

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    float4 ra[2], rb[2];
    OA::fetch(a, lda, I, kend, i0, kbeg, avec != 0, ra);
    OB::fetch(b, ldb, J, kend, j0, kbeg, bvec != 0, rb);
    for (int k0 = kbeg; k0 < kend; k0 += kBK) {
        __syncthreads();
        OA::stash(As, ra);
        OB::stash(Bs, rb);
        __syncthreads();
        if (k0 + kBK < kend) {
            OA::fetch(a, lda, I, kend, i0, k0 + kBK, avec != 0, ra);
            OB::fetch(b, ldb, J, kend, j0, k0 + kBK, bvec != 0, rb);
        }
#pragma unroll
        for (int s = 0; s < kBK / 2; ++s) {
            const int k = 2 * s + lk;
            float av[2], bv[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) av[m] = As[k * OA::LD + wi + m * 32 + lr];
#pragma unroll
            for (int n = 0; n < 2; ++n) bv[n] = Bs[k * OB::LD + wj + n * 32 + lr];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[n], acc[m][n], 0, 0, 0);
        }
    }

    // C/D map of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float* o = out + (size_t)blockIdx.z * zstride;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int j = j0 + wj + n * 32 + lr;
            if (j >= J) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = i0 + wi + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (i >= I) continue;
                float v = acc[m][n][r];
                if (MODE == MODE_GRAM) {
                    v += o[(size_t)i * ldo + j];
                    o[(size_t)i * ldo + j] = v;
                    if (ti != tj) o[(size_t)j * ldo + i] = v;
                } else {
                    o[(size_t)i * ldo + j] = relu ? fmaxf(v, 0.f) : v;
                }
            }
        }
}

// Q[m, c] += sum over the rows n with labels[n] == c of H[n, m], rows in ascending order.  One thread per column m and kLabelClasses classes per
// workgroup; the label of a row is wave-uniform, so a workgroup loads only the rows of its own classes and H is read once in total.
__global__ __launch_bounds__(kLabelCols) void rp_label_sum_kernel(const float* __restrict__ H, const int64_t* __restrict__ labels, float* __restrict__ Q,
                                                                  int N, int M, int C) {
    const int m = blockIdx.x * kLabelCols + threadIdx.x;
    const int c0 = blockIdx.y * kLabelClasses;
    float acc[kLabelClasses];
#pragma unroll
    for (int q = 0; q < kLabelClasses; ++q) acc[q] = 0.f;
    for (int n = 0; n < N; ++n) {
        const int64_t lab = labels[n];
        if (lab < c0 || lab >= c0 + kLabelClasses) continue;
        const float h = m < M ? H[(size_t)n * M + m] : 0.f;
        const int ql = (int)(lab - c0);
#pragma unroll
        for (int q = 0; q < kLabelClasses; ++q)
            if (q == ql) acc[q] += h;
    }
    if (m >= M) return;
#pragma unroll
    for (int q = 0; q < kLabelClasses; ++q)
        if (c0 + q < C) Q[(size_t)m * C + c0 + q] += acc[q];
}

__global__ void rp_label_check_kernel(const int64_t* __restrict__ labels, int N, int C, int* __restrict__ bad) {
    for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
        const int64_t lab = labels[n];
        if (lab < 0 || lab >= C) *bad = 1;
    }
}

// logits[e] = sigma * (partial[0][e] + partial[1][e] + ...), slices in ascending order
__global__ void rp_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ sigma, float* __restrict__ logits, int n, int slices) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    float s = 0.f;
    for (int z = 0; z < slices; ++z) s += partial[(size_t)z * n + e];
    logits[e] = (sigma ? *sigma : 1.f) * s;
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// the word the label check reports through: one per device, allocated at the first call
int* label_flag() {
    static std::mutex mu;
    static int* flags[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!flags[dev] && hipMalloc(reinterpret_cast<void**>(&flags[dev]), sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        flags[dev] = nullptr;
    }
    return flags[dev];
}

int project(const float* F, const float* W, float* H, int N, int D, int M, int relu, hipStream_t st) {
    dim3 grid(tiles(M), tiles(N), 1);
    rp_tile_kernel<false, true, MODE_STORE><<<grid, kThreads, 0, st>>>(F, (size_t)D, vec_ok(F, D), W, (size_t)M, vec_ok(W, M), H, (size_t)M, 0, N, M, D, D,
                                                                        relu);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

}  // namespace

extern "C" int clhip_rp_project(const float* F, const float* W, float* H, int N, int D, int M, int relu, void* stream) {
    CLHIP_CHECK_ARG(F && W && H && N >= 1 && D >= 1 && M >= 1);
    CLHIP_CHECK_ARG(tiles(N) <= 65535);
    return project(F, W, H, N, D, M, relu, static_cast<hipStream_t>(stream));
}

extern "C" int clhip_rp_gram_accum(const float* H, float* G, int N, int M, void* stream) {
    CLHIP_CHECK_ARG(H && G && N >= 1 && M >= 1);
    const long long T = tiles(M);
    CLHIP_CHECK_ARG(T * (T + 1) / 2 <= 0x7fffffffLL);
    dim3 grid((unsigned)(T * (T + 1) / 2), 1, 1);
    const int vec = vec_ok(H, M);
    rp_tile_kernel<true, true, MODE_GRAM><<<grid, kThreads, 0, static_cast<hipStream_t>(stream)>>>(H, (size_t)M, vec, H, (size_t)M, vec, G, (size_t)M, 0, M, M,
                                                                                                   N, N, 0);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

extern "C" int clhip_rp_label_sum(const float* H, const int64_t* labels, float* Q, int N, int M, int C, void* stream) {
    CLHIP_CHECK_ARG(H && labels && Q && N >= 1 && M >= 1 && C >= 1);
    CLHIP_CHECK_ARG((C + kLabelClasses - 1) / kLabelClasses <= 65535);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* flag = label_flag();
    if (!flag) {
        clhip_set_error("clhip_rp_label_sum: cannot allocate the label-check word");
        return CLHIP_EHIP;
    }
    int bad = 0;
    if (hipMemsetAsync(flag, 0, sizeof(int), st) != hipSuccess) return CLHIP_EHIP;
    rp_label_check_kernel<<<min((N + 255) / 256, 256), 256, 0, st>>>(labels, N, C, flag);
    CLHIP_LAUNCH_CHECK();
    if (hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        clhip_set_error("clhip_rp_label_sum: reading the label check failed");
        return CLHIP_EHIP;
    }
    if (bad) {
        clhip_set_error("clhip_rp_label_sum: invalid argument: a label lies outside [0, %d)", C);
        return CLHIP_EINVAL;
    }
    dim3 grid((M + kLabelCols - 1) / kLabelCols, (C + kLabelClasses - 1) / kLabelClasses, 1);
    rp_label_sum_kernel<<<grid, kLabelCols, 0, st>>>(H, labels, Q, N, M, C);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

extern "C" size_t clhip_rp_classify_ws_bytes(int B, int M, int C) {
    if (B < 1 || M < 1 || C < 1) return 0;
    const size_t slices = (size_t)(M + kSplitK - 1) / kSplitK;
    return align256((size_t)B * M * sizeof(float)) + align256(slices * B * C * sizeof(float));
}

// hidden = relu(X W) goes through ws (B x M floats); the second product is cut into K slices of kSplitK, one workgroup each, and the
// slice partials are summed in slice order by a last launch that also applies sigma
extern "C" int clhip_rp_classify(const float* X, const float* W, const float* Wo, const float* sigma, float* logits, void* ws, int B, int D, int M, int C,
                                 void* stream) {
    CLHIP_CHECK_ARG(X && W && Wo && logits && ws && B >= 1 && D >= 1 && M >= 1 && C >= 1);
    CLHIP_CHECK_ARG(tiles(B) <= 65535);
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* hidden = static_cast<float*>(ws);
    float* partial = reinterpret_cast<float*>(static_cast<char*>(ws) + align256((size_t)B * M * sizeof(float)));
    if (int rc = project(X, W, hidden, B, D, M, 1, st)) return rc;
    const int slices = (M + kSplitK - 1) / kSplitK;
    dim3 grid(tiles(C), tiles(B), slices);
    rp_tile_kernel<false, false, MODE_STORE><<<grid, kThreads, 0, st>>>(hidden, (size_t)M, vec_ok(hidden, M), Wo, (size_t)M, vec_ok(Wo, M), partial,
                                                                         (size_t)C, (size_t)B * C, B, C, M, kSplitK, 0);
    CLHIP_LAUNCH_CHECK();
    const int n = B * C;
    rp_reduce_kernel<<<(n + 255) / 256, 256, 0, st>>>(partial, sigma, logits, n, slices);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}
