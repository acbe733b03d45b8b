// ca.hip -- classifier alignment of InfLoRA_OPT (reference core/model/InfLoRA_opt.py:371-456): the per-class Gaussians over the backbone features and
// the sampler that draws the rows the heads are re-trained on, both on the exact fp32 MFMA of gfx950 with the operand staging of rp_tile.h.
//
// The rules are those of rp.hip: fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain), no atomics, every summation order a
// function of the shapes only, ragged edges the normal case, 16-byte loads only where pitch and alignment allow.
//
// class_moments: phase 1 sums each column of a class's rows in row order (one thread per column) and divides by the count; phase 2 is, per class, the
//   Gram of the centred rows over the tiles on or above the diagonal.  Both operands are the class's rows, k-major (k = the row inside the class); the
//   mean is subtracted in registers between the global load and the LDS store, so the centred rows never exist in memory.  The epilogue divides by
//   n_c - 1, adds eps on the diagonal and writes an off-diagonal tile to both places.
// ca_sample: per class X = scale * mean + Z L^T, an S x D x D product whose second operand is lower triangular: an output column tile starting at j0
//   needs k < j0 + 128 only, so the K loop stops there, and inside the diagonal block the loads of row j of L stop at k = j -- the strict upper
//   triangle is never read (torch.linalg.cholesky leaves zeros there, other factorisations leave anything).  The epilogue scatters the rows to
//   their places after the shuffle.
#include <mutex>
#include <vector>

#include "rp_tile.h"

using namespace rp_tile;

namespace {

constexpr int kMeanCols = 64;     // columns per mean workgroup (768 columns x 10 classes = 120 workgroups)

// mean[c, j] = (sum over the rows k of class c, ascending, of F[off_c + k, j]) / n_c
__global__ __launch_bounds__(kMeanCols) void ca_mean_kernel(const float* __restrict__ F, const int32_t* __restrict__ offsets, float* __restrict__ mean,
                                                            int D) {
    const int j = blockIdx.x * kMeanCols + threadIdx.x, c = blockIdx.y;
    if (j >= D) return;
    const int off = offsets[c], n = offsets[c + 1] - off;
    const float* p = F + (size_t)off * D + j;
    float s = 0.f;
    for (int k0 = 0; k0 < n; k0 += 8) {          // eight independent loads in flight, added in row order
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = k0 + e < n ? p[(size_t)(k0 + e) * D] : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (k0 + e < n) s += v[e];
    }
    mean[(size_t)c * D + j] = s / (float)n;
}

// x - mean on this thread's share of a k-major block (Operand<true>::fetch: rows k0 + (t >> 5) + 8 h, columns i0 + (t & 31) * 4 .. + 3, the same four
// columns in every block); rows past the class stay zero, and m[] is zero for the columns past D
__device__ __forceinline__ void centre(float4 (&r)[2], const float (&m)[4], int k0, int kend) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (k0 + (int)(threadIdx.x >> 5) + 8 * h < kend) {
            r[h].x -= m[0];
            r[h].y -= m[1];
            r[h].z -= m[2];
            r[h].w -= m[3];
        }
}

// cov[c] tile (i, j) = sum_k (x(k, i) - mean(i)) (x(k, j) - mean(j)) / (n_c - 1) [+ eps where i == j]; blockIdx.x enumerates the tiles on or above
// the diagonal, blockIdx.y the classes.  A diagonal tile is symmetric by construction (rp.hip, MODE_GRAM); an off-diagonal one is written twice.
__global__ __launch_bounds__(kThreads) void ca_cov_kernel(const float* __restrict__ F, const int32_t* __restrict__ offsets,
                                                           const float* __restrict__ mean, float* __restrict__ cov, int D, int vec, float eps) {
    using O = Operand<true>;
    __shared__ __attribute__((aligned(16))) float As[kBK * O::LD];
    __shared__ __attribute__((aligned(16))) float Bs[kBK * O::LD];
    const int c = blockIdx.y;
    const int off = offsets[c], n = offsets[c + 1] - off;
    const int T = (D + kTile - 1) / kTile;
    int t = blockIdx.x, ti = 0;
    while (t >= T - ti) {
        t -= T - ti;
        ++ti;
    }
    const int tj = ti + t;
    const int i0 = ti * kTile, j0 = tj * kTile;
    const float* p = F + (size_t)off * D;
    const float* mu = mean + (size_t)c * D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    const int lr = lane & 31, lk = lane >> 5;

    float ma[4], mb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = i0 + (threadIdx.x & 31) * 4 + e, j = j0 + (threadIdx.x & 31) * 4 + e;
        ma[e] = i < D ? mu[i] : 0.f;
        mb[e] = j < D ? mu[j] : 0.f;
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][q][r] = 0.f;

    float4 ra[2], rb[2];
    O::fetch(p, (size_t)D, D, n, i0, 0, vec != 0, ra);
    O::fetch(p, (size_t)D, D, n, j0, 0, vec != 0, rb);
    for (int k0 = 0; k0 < n; k0 += kBK) {
        centre(ra, ma, k0, n);
        centre(rb, mb, k0, n);
        __syncthreads();
        O::stash(As, ra);
        O::stash(Bs, rb);
        __syncthreads();
        if (k0 + kBK < n) {
            O::fetch(p, (size_t)D, D, n, i0, k0 + kBK, vec != 0, ra);
            O::fetch(p, (size_t)D, D, n, j0, k0 + kBK, vec != 0, rb);
        }
#pragma unroll
        for (int s = 0; s < kBK / 2; ++s) {
            const int k = 2 * s + lk;
            float av[2], bv[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) av[m] = As[k * O::LD + wi + m * 32 + lr];
#pragma unroll
            for (int q = 0; q < 2; ++q) bv[q] = Bs[k * O::LD + wj + q * 32 + lr];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int q = 0; q < 2; ++q) acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[q], acc[m][q], 0, 0, 0);
        }
    }

    // C/D map of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float* o = cov + (size_t)c * D * D;
    const float denom = (float)(n - 1);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int j = j0 + wj + q * 32 + lr;
            if (j >= D) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = i0 + wi + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (i >= D) continue;
                float v = acc[m][q][r] / denom;
                if (i == j) v += eps;
                o[(size_t)i * D + j] = v;
                if (ti != tj) o[(size_t)j * D + i] = v;
            }
        }
}

// X[dest[c S + s], j] = scale[c] mean[c, j] + sum_{k <= j} Z[c S + s, k] L[c, j, k]; blockIdx = (column tile, row tile, class)
__global__ __launch_bounds__(kThreads) void ca_sample_kernel(const float* __restrict__ mean, const float* __restrict__ scale, const float* __restrict__ chol,
                                                              const float* __restrict__ Z, const int64_t* __restrict__ dest, float* __restrict__ X,
                                                              int64_t* __restrict__ labels, int S, int D, int vec, int64_t class_lo) {
    using O = Operand<false>;
    __shared__ __attribute__((aligned(16))) float As[kBK * O::LD];
    __shared__ __attribute__((aligned(16))) float Bs[kBK * O::LD];
    __shared__ int64_t sdest[kTile];
    const int c = blockIdx.z;
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    const float* a = Z + (size_t)c * S * D;
    const float* b = chol + (size_t)c * D * D;
    const int kend = min(D, j0 + kTile);          // the K blocks past the tile's last column lie wholly above the diagonal
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    const int lr = lane & 31, lk = lane >> 5;

    if (threadIdx.x < kTile && i0 + (int)threadIdx.x < S) {
        const int64_t d = dest[(size_t)c * S + i0 + threadIdx.x];
        sdest[threadIdx.x] = d;
        if (blockIdx.x == 0) labels[d] = class_lo + c;
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][q][r] = 0.f;

    float4 ra[2], rb[2];
    O::fetch(a, (size_t)D, S, kend, i0, 0, vec != 0, ra);
    fetch_lower(b, (size_t)D, D, kend, j0, 0, vec != 0, rb);
    for (int k0 = 0; k0 < kend; k0 += kBK) {
        __syncthreads();
        O::stash(As, ra);
        O::stash(Bs, rb);
        __syncthreads();
        if (k0 + kBK < kend) {
            O::fetch(a, (size_t)D, S, kend, i0, k0 + kBK, vec != 0, ra);
            fetch_lower(b, (size_t)D, D, kend, j0, k0 + kBK, vec != 0, rb);
        }
#pragma unroll
        for (int s = 0; s < kBK / 2; ++s) {
            const int k = 2 * s + lk;
            float av[2], bv[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) av[m] = As[k * O::LD + wi + m * 32 + lr];
#pragma unroll
            for (int q = 0; q < 2; ++q) bv[q] = Bs[k * O::LD + wj + q * 32 + lr];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int q = 0; q < 2; ++q) acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[q], acc[m][q], 0, 0, 0);
        }
    }

    const float sc = scale[c];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int j = j0 + wj + q * 32 + lr;
            if (j >= D) continue;
            const float loc = sc * mean[(size_t)c * D + j];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int il = wi + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (i0 + il >= S) continue;
                X[(size_t)sdest[il] * D + j] = loc + acc[m][q][r];
            }
        }
}

// dest is a permutation of [0, n) iff every entry is in range and, after inv[dest[i]] = i, every i reads itself back: of two entries with the same
// value only the writer that landed last does.  Two launches; inv is the caller's scratch (n words of 8 bytes).
__global__ void ca_perm_scatter_kernel(const int64_t* __restrict__ dest, int64_t* __restrict__ inv, int n, int* __restrict__ bad) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int64_t d = dest[i];
        if (d < 0 || d >= n) *bad = 1;
        else inv[d] = i;
    }
}

__global__ void ca_perm_verify_kernel(const int64_t* __restrict__ dest, const int64_t* __restrict__ inv, int n, int* __restrict__ bad) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int64_t d = dest[i];
        if (d >= 0 && d < n && inv[d] != i) *bad = 1;
    }
}

// the word the permutation check reports through: one per device, allocated at the first call
int* perm_flag() {
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

}  // namespace

extern "C" int clhip_class_moments(const float* F, const int32_t* offsets, float* mean, float* cov, int N, int D, int C, float eps, void* stream) {
    CLHIP_CHECK_ARG(F && offsets && mean && cov && N >= 1 && D >= 1 && C >= 1 && C <= 65535);
    const long long T = tiles(D);
    CLHIP_CHECK_ARG(T * (T + 1) / 2 <= 0x7fffffffLL);
    hipStream_t st = static_cast<hipStream_t>(stream);
    std::vector<int32_t> offs((size_t)C + 1);
    if (hipMemcpyAsync(offs.data(), offsets, offs.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        clhip_set_error("clhip_class_moments: reading the class offsets failed");
        return CLHIP_EHIP;
    }
    if (offs[0] != 0 || offs[C] != N) {
        clhip_set_error("clhip_class_moments: invalid argument: the offsets run from %d to %d, not from 0 to N = %d", offs[0], offs[C], N);
        return CLHIP_EINVAL;
    }
    for (int c = 0; c < C; ++c)
        if ((long long)offs[c + 1] - offs[c] < 2) {
            clhip_set_error("clhip_class_moments: invalid argument: class %d has %lld rows (offsets %d, %d); the unbiased covariance needs 2", c,
                            (long long)offs[c + 1] - offs[c], offs[c], offs[c + 1]);
            return CLHIP_EINVAL;
        }
    ca_mean_kernel<<<dim3((D + kMeanCols - 1) / kMeanCols, C, 1), kMeanCols, 0, st>>>(F, offsets, mean, D);
    CLHIP_LAUNCH_CHECK();
    ca_cov_kernel<<<dim3((unsigned)(T * (T + 1) / 2), C, 1), kThreads, 0, st>>>(F, offsets, mean, cov, D, vec_ok(F, D), eps);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

extern "C" int clhip_ca_sample(const float* mean, const float* scale, const float* chol, const float* Z, const int64_t* dest, float* X, int64_t* labels,
                               int C, int S, int D, int64_t class_lo, void* stream) {
    CLHIP_CHECK_ARG(mean && scale && chol && Z && dest && X && labels && C >= 1 && S >= 1 && D >= 1);
    CLHIP_CHECK_ARG(C <= 65535 && tiles(S) <= 65535 && (long long)C * S <= 0x7fffffffLL);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n = C * S;
    int* flag = perm_flag();
    if (!flag) {
        clhip_set_error("clhip_ca_sample: cannot allocate the permutation-check word");
        return CLHIP_EHIP;
    }
    int bad = 0;
    if (hipMemsetAsync(flag, 0, sizeof(int), st) != hipSuccess) return CLHIP_EHIP;
    const int blocks = min((n + 255) / 256, 256);
    ca_perm_scatter_kernel<<<blocks, 256, 0, st>>>(dest, labels, n, flag);
    CLHIP_LAUNCH_CHECK();
    ca_perm_verify_kernel<<<blocks, 256, 0, st>>>(dest, labels, n, flag);
    CLHIP_LAUNCH_CHECK();
    if (hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        clhip_set_error("clhip_ca_sample: reading the permutation check failed");
        return CLHIP_EHIP;
    }
    if (bad) {
        clhip_set_error("clhip_ca_sample: invalid argument: dest is not a permutation of [0, %d)", n);
        return CLHIP_EINVAL;
    }
    // chol and Z share the pitch D, and a class starts a multiple of D floats in: one alignment test serves every class
    const int vec = vec_ok(Z, D) && vec_ok(chol, D);
    ca_sample_kernel<<<dim3(tiles(D), tiles(S), C), kThreads, 0, st>>>(mean, scale, chol, Z, dest, X, labels, S, D, vec, class_lo);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}
