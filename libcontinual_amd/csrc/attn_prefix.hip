// attn_prefix.hip -- prefix-tuning attention of the ViT path (reference core/model/backbone/transformer.py:169-197 with `prompt` given, :175-180): every
// sample brings Lp extra key and value rows (pk, pv: [B, Lp, D], column = head*d + i) that have NO query.  Per (batch, head) the N token queries attend over
// the Lp + N keys [prefix | tokens]; the reference concatenates k and v ([B,H,Lp+N,d]) and runs the plain product.  The backward returns dqkv for the tokens
// and the prefix gradients dpk, dpv [B, Lp, D] in fp32 (written, not accumulated; no atomics: each key row has one owner).
//
// The formulation is attn.hip's (one workgroup per (batch, head), K and V staged once in LDS with pitch KP, v_mfma_f32_16x16x32_bf16, S^T in registers,
// padded keys zero in LDS), with two differences that run through every loop: K and V are staged from TWO sources, and the key-tile count
// ceil((N + Lp) / 16) is not the query-tile count ceil(N / 16).  LDS row r of K / V is key r: r < Lp the prefix, r - Lp the token.
// fp32 (parity mode), head sizes other than 64 and a backward whose four tiles do not fit the LDS use the generic one-wave-per-row kernels below.
#include "common.h"

namespace {

struct PrefixParams {
    const void* qkv; const void* pk; const void* pv; void* out; float* lse;
    const void* dout; void* dqkv; float* dpk; float* dpv; float* dsum;      // backward only (dsum: [B,H,N] scratch, generic path)
    int B, N, Lp, H, D;
    float scale;
};

constexpr int KP = 160;      // LDS pitch (bytes) of a 64-element bf16 row, as attn.hip: ds_read_b128 and the transposed reads are conflict-free

__device__ __forceinline__ f32x4 mfma_bf16(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ uint4 pack8(const f32x4& a, const f32x4& b) {
    return make_uint4(pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]), pack_bf16x2(b[0], b[1]), pack_bf16x2(b[2], b[3]));
}
__device__ __forceinline__ uint4 ldsq(const char* base, int off) { return *reinterpret_cast<const uint4*>(base + off); }

// 16-byte chunk c of key row `row` of one head: the prefix (row pitch D) below Lp, the token row - Lp (row pitch ld) below Lp + N, zero beyond
__device__ __forceinline__ uint4 key_chunk(const bf16_t* pre, size_t D, const bf16_t* tok, size_t ld, int Lp, int Lt, int row, int c) {
    if (row < Lp) return *reinterpret_cast<const uint4*>(pre + (size_t)row * D + c * 8);
    if (row < Lt) return *reinterpret_cast<const uint4*>(tok + (size_t)(row - Lp) * ld + c * 8);
    return make_uint4(0, 0, 0, 0);
}

// NKT = number of 16-key tiles (compile time: 13 / 14 for 197..208 / 209..224 keys; 0 = run-time count, up to 16).  The arithmetic per query tile is
// attn_fwd_mfma_kernel's: scale folded into the exponent, only the last key tile masked, P unnormalised in bf16, 1 / sum applied to the output.
template <int NKT>
__global__ __launch_bounds__(256) void prefix_fwd_mfma_kernel(PrefixParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int bh = blockIdx.x, b = bh / p.H, h = bh - b * p.H;
    const int N = p.N, D = p.D, Lp = p.Lp, Lt = N + Lp;
    const int nKT = NKT > 0 ? NKT : (Lt + 15) >> 4, nQT = (N + 15) >> 4;
    constexpr int KTMAX = NKT > 0 ? NKT : 16;
    const int NK2 = ((nKT + 1) & ~1) * 16;
    const size_t ld = 3 * (size_t)D;
    const bf16_t* base = static_cast<const bf16_t*>(p.qkv) + (size_t)b * N * ld + h * 64;
    const bf16_t* pkb = static_cast<const bf16_t*>(p.pk) + (size_t)b * Lp * D + h * 64;
    const bf16_t* pvb = static_cast<const bf16_t*>(p.pv) + (size_t)b * Lp * D + h * 64;
    char* Ks = smem;
    char* Vs = smem + NK2 * KP;
    for (int idx = tid; idx < NK2 * 8; idx += 256) {
        const int row = idx >> 3, cc = idx & 7;
        *reinterpret_cast<uint4*>(Ks + row * KP + cc * 16) = key_chunk(pkb, D, base + D, ld, Lp, Lt, row, cc);
        *reinterpret_cast<uint4*>(Vs + row * KP + cc * 16) = key_chunk(pvb, D, base + 2 * D, ld, Lp, Lt, row, cc);
    }
    __syncthreads();
    const float c = p.scale * 1.4426950408889634f;          // scores -> exp2 domain
    const int last0 = (nKT - 1) * 16 + g * 4;               // first key this lane holds in the last tile

    for (int qt = wave; qt < nQT; qt += 4) {
        const int qrow = qt * 16 + l15;
        const bool qok = qrow < N;
        uint4 qf[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
            qf[kk] = qok ? *reinterpret_cast<const uint4*>(base + (size_t)qrow * ld + (g + 4 * kk) * 8) : make_uint4(0, 0, 0, 0);
        f32x4 s[KTMAX + 1];
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < KTMAX; ++kt) {
            s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (NKT > 0 || kt < nKT) {
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) s[kt] = mfma_bf16(ldsq(Ks, (kt * 16 + l15) * KP + (g + 4 * kk) * 16), qf[kk], s[kt]);
                if (kt == nKT - 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (last0 + e >= Lt) s[kt][e] = -INFINITY;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) mx = fmaxf(mx, s[kt][e]);
            }
        }
        s[KTMAX] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mc = mx * c;
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < KTMAX; ++kt) {
            if (NKT > 0 || kt < nKT) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float e_ = __builtin_amdgcn_exp2f(fmaf(s[kt][e], c, -mc)); s[kt][e] = e_; sum += e_; }
            }
        }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        if (g == 0 && qok && p.lse) p.lse[((size_t)b * p.H + h) * N + qrow] = mx * p.scale + __logf(sum);
        f32x4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < (KTMAX + 1) / 2; ++ks) {
            if (NKT > 0 || 2 * ks < nKT) {
                const uint4 pb = pack8(s[2 * ks], s[2 * ks + 1]);           // tiles >= nKT are zero
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const uint4 vt = tr8(Vs, (2 * ks * 16 + g * 4 + (l15 >> 2)) * KP + (dt * 16 + (l15 & 3) * 4) * 2, 16 * KP);
                    o[dt] = mfma_bf16(vt, pb, o[dt]);
                }
            }
        }
        if (qok) {
            const float inv = 1.0f / sum;
            bf16_t* orow = static_cast<bf16_t*>(p.out) + ((size_t)b * N + qrow) * D + h * 64 + g * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<uint2*>(orow + dt * 16) = make_uint2(pack_bf16x2(o[dt][0] * inv, o[dt][1] * inv), pack_bf16x2(o[dt][2] * inv, o[dt][3] * inv));
        }
    }
}

constexpr int BWD_WAVES = 16;     // one workgroup per CU (the LDS holds Q, dO, K, V of the head): 16 waves, as attn.hip

// LDS: Q and dO have NQ2 rows (query tiles rounded to a pair), K and V have NK2 rows (key tiles rounded to a pair).  Every global read of the prologue is
// issued before the first LDS write (attn_bwd_mfma3_kernel's one round trip).  Phase A (wave <- query tile) walks the key-tile pairs, phase B (wave <- key tile)
// the query-tile pairs; phase B owns the prefix key rows too and stores their dK / dV columns to dpk / dpv in fp32.
// Masks: a padded QUERY has lse = +inf, so P = 0.  A padded KEY meets a real query row in phase A, where P = exp2(0 - lse log2 e) overflows for lse < -88.7
// and dS = inf * x is not finite (attn.hip:284-287): the last key tile and the padding tile behind it set P = 0 by key index.  In phase B a padded key column
// is computed as zero (kok) and never stored.
__global__ __launch_bounds__(64 * BWD_WAVES) void prefix_bwd_mfma_kernel(PrefixParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int bh = blockIdx.x, b = bh / p.H, h = bh - b * p.H;
    const int N = p.N, D = p.D, Lp = p.Lp, Lt = N + Lp;
    const int nQT = (N + 15) >> 4, nKT = (Lt + 15) >> 4;
    const int NQ2 = ((nQT + 1) & ~1) * 16, NK2 = ((nKT + 1) & ~1) * 16, nQPair = NQ2 >> 5, nKPair = NK2 >> 5;
    const size_t ld = 3 * (size_t)D;
    const bf16_t* base = static_cast<const bf16_t*>(p.qkv) + (size_t)b * N * ld + h * 64;
    const bf16_t* pkb = static_cast<const bf16_t*>(p.pk) + (size_t)b * Lp * D + h * 64;
    const bf16_t* pvb = static_cast<const bf16_t*>(p.pv) + (size_t)b * Lp * D + h * 64;
    const bf16_t* dob = static_cast<const bf16_t*>(p.dout) + (size_t)b * N * D + h * 64;
    const bf16_t* ob = static_cast<const bf16_t*>(p.out) + (size_t)b * N * D + h * 64;
    bf16_t* dqb = static_cast<bf16_t*>(p.dqkv) + (size_t)b * N * ld + h * 64;
    char* Qs = smem;
    char* Gs = Qs + NQ2 * KP;                                  // dO
    char* Ks = Gs + NQ2 * KP;
    char* Vs = Ks + NK2 * KP;
    float* lse_s = reinterpret_cast<float*>(Vs + NK2 * KP);    // [NQ2]  lse * log2(e)  (+inf beyond N -> P = 0)
    float* dq_s = lse_s + NQ2;                                 // [NQ2]  rowsum(dO * O)
    constexpr int CH = (256 * 8) / (64 * BWD_WAVES);           // chunks per thread of the largest tile (256 rows)
    uint4 sq[CH], sg[CH], sk[CH], sv[CH], orow[8];
    float lraw = INFINITY;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int idx = tid + i * 64 * BWD_WAVES, row = idx >> 3, cc = idx & 7;
        sq[i] = sg[i] = make_uint4(0, 0, 0, 0);
        if (row < N) {
            sq[i] = *reinterpret_cast<const uint4*>(base + (size_t)row * ld + cc * 8);
            sg[i] = *reinterpret_cast<const uint4*>(dob + (size_t)row * D + cc * 8);
        }
        sk[i] = key_chunk(pkb, D, base + D, ld, Lp, Lt, row, cc);
        sv[i] = key_chunk(pvb, D, base + 2 * D, ld, Lp, Lt, row, cc);
    }
    if (tid < N) {
        lraw = p.lse[((size_t)b * p.H + h) * N + tid];
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) orow[cc] = *reinterpret_cast<const uint4*>(ob + (size_t)tid * D + cc * 8);
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int idx = tid + i * 64 * BWD_WAVES, row = idx >> 3, cc = idx & 7;
        if (row < NQ2) {
            *reinterpret_cast<uint4*>(Qs + row * KP + cc * 16) = sq[i];
            *reinterpret_cast<uint4*>(Gs + row * KP + cc * 16) = sg[i];
        }
        if (row < NK2) {
            *reinterpret_cast<uint4*>(Ks + row * KP + cc * 16) = sk[i];
            *reinterpret_cast<uint4*>(Vs + row * KP + cc * 16) = sv[i];
        }
    }
    __syncthreads();
    if (tid < NQ2) {
        float dsum = 0.f;
        if (tid < N) {
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) {
                const uint4 xg = ldsq(Gs, tid * KP + cc * 16);
                const unsigned xw[4] = {xg.x, xg.y, xg.z, xg.w}, yw[4] = {orow[cc].x, orow[cc].y, orow[cc].z, orow[cc].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    dsum += __uint_as_float(xw[j] << 16) * __uint_as_float(yw[j] << 16);
                    dsum += __uint_as_float(xw[j] & 0xffff0000u) * __uint_as_float(yw[j] & 0xffff0000u);
                }
            }
        }
        lse_s[tid] = lraw * 1.4426950408889634f;
        dq_s[tid] = dsum;
    }
    __syncthreads();
    const float c = p.scale * 1.4426950408889634f;          // scores -> exp2 domain

    // ---- phase A: dQ.  wave <- query tile; per key-tile pair: S^T, dP^T (D layout: rows key g*4+e, col q l15)
    for (int qt = wave; qt < nQT; qt += BWD_WAVES) {
        const int qrow = qt * 16 + l15;
        uint4 qf[2], gf[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            qf[kk] = ldsq(Qs, qrow * KP + (g + 4 * kk) * 16);
            gf[kk] = ldsq(Gs, qrow * KP + (g + 4 * kk) * 16);
        }
        const float lq = lse_s[qrow], dq = dq_s[qrow];
        f32x4 acc[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) acc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < nKPair; ++ks) {
            f32x4 ds[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int krow = (2 * ks + t) * 16 + l15;
                f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    s = mfma_bf16(ldsq(Ks, krow * KP + (g + 4 * kk) * 16), qf[kk], s);
                    dp = mfma_bf16(ldsq(Vs, krow * KP + (g + 4 * kk) * 16), gf[kk], dp);
                }
                const bool tail = (2 * ks + t) >= nKT - 1;               // only the last key tile and the padding tile hold keys >= Lt
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pr = __builtin_amdgcn_exp2f(fmaf(s[e], c, -lq));
                    if (tail && (2 * ks + t) * 16 + g * 4 + e >= Lt) pr = 0.f;
                    ds[t][e] = pr * (dp[e] - dq);
                }
            }
            const uint4 db = pack8(ds[0], ds[1]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const uint4 kt_ = tr8(Ks, (2 * ks * 16 + g * 4 + (l15 >> 2)) * KP + (dt * 16 + (l15 & 3) * 4) * 2, 16 * KP);
                acc[dt] = mfma_bf16(kt_, db, acc[dt]);
            }
        }
        if (qrow < N) {
            bf16_t* r = dqb + (size_t)qrow * ld + g * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<uint2*>(r + dt * 16) = make_uint2(pack_bf16x2(acc[dt][0] * p.scale, acc[dt][1] * p.scale),
                                                                    pack_bf16x2(acc[dt][2] * p.scale, acc[dt][3] * p.scale));
        }
    }

    // ---- phase B: dK, dV.  wave <- key tile (prefix rows included); per query-tile pair: S, dP (D layout: rows q g*4+e, col key l15)
    for (int kt = wave; kt < nKT; kt += BWD_WAVES) {
        const int krow = kt * 16 + l15;
        const bool kok = krow < Lt;
        uint4 kf[2], vf[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            kf[kk] = ldsq(Ks, krow * KP + (g + 4 * kk) * 16);
            vf[kk] = ldsq(Vs, krow * KP + (g + 4 * kk) * 16);
        }
        f32x4 dk[4], dv[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) { dk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
        for (int qs = 0; qs < nQPair; ++qs) {
            f32x4 pr[2], ds[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int qr = (2 * qs + t) * 16 + l15;
                f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    s = mfma_bf16(ldsq(Qs, qr * KP + (g + 4 * kk) * 16), kf[kk], s);
                    dp = mfma_bf16(ldsq(Gs, qr * KP + (g + 4 * kk) * 16), vf[kk], dp);
                }
                const int q0 = (2 * qs + t) * 16 + g * 4;
                const float4 l4 = *reinterpret_cast<const float4*>(lse_s + q0);
                const float4 d4 = *reinterpret_cast<const float4*>(dq_s + q0);
                const float le[4] = {l4.x, l4.y, l4.z, l4.w}, de[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pe = kok ? __builtin_amdgcn_exp2f(fmaf(s[e], c, -le[e])) : 0.f;      // lse = +inf beyond N -> 0
                    pr[t][e] = pe;
                    ds[t][e] = pe * (dp[e] - de[e]);
                }
            }
            const uint4 pb = pack8(pr[0], pr[1]), db = pack8(ds[0], ds[1]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const int a = (2 * qs * 16 + g * 4 + (l15 >> 2)) * KP + (dt * 16 + (l15 & 3) * 4) * 2;
                dv[dt] = mfma_bf16(tr8(Gs, a, 16 * KP), pb, dv[dt]);
                dk[dt] = mfma_bf16(tr8(Qs, a, 16 * KP), db, dk[dt]);
            }
        }
        if (kok && krow < Lp) {                                           // a prefix key: fp32, no rounding step
            float* rk = p.dpk + ((size_t)b * Lp + krow) * D + h * 64 + g * 4;
            float* rv = p.dpv + ((size_t)b * Lp + krow) * D + h * 64 + g * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                *reinterpret_cast<float4*>(rk + dt * 16) = make_float4(dk[dt][0] * p.scale, dk[dt][1] * p.scale, dk[dt][2] * p.scale, dk[dt][3] * p.scale);
                *reinterpret_cast<float4*>(rv + dt * 16) = make_float4(dv[dt][0], dv[dt][1], dv[dt][2], dv[dt][3]);
            }
        } else if (kok) {
            bf16_t* r = dqb + (size_t)(krow - Lp) * ld + g * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                *reinterpret_cast<uint2*>(r + D + dt * 16) = make_uint2(pack_bf16x2(dk[dt][0] * p.scale, dk[dt][1] * p.scale),
                                                                        pack_bf16x2(dk[dt][2] * p.scale, dk[dt][3] * p.scale));
                *reinterpret_cast<uint2*>(r + 2 * D + dt * 16) = make_uint2(pack_bf16x2(dv[dt][0], dv[dt][1]), pack_bf16x2(dv[dt][2], dv[dt][3]));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ generic path
// One wave per (batch, head, row); lane = key while scoring, lane = d while accumulating (attn.hip's generic kernels over the Lp + N keys).
template <typename T>
struct HeadPtrs {
    const T *q, *k, *v, *pk, *pv;      // token rows (pitch 3D) and prefix rows (pitch D) of one (batch, head)
    size_t ld, D;
    int Lp;
    __device__ __forceinline__ HeadPtrs(const PrefixParams& p, int b, int h, int hd) {
        ld = 3 * (size_t)p.D; D = p.D; Lp = p.Lp;
        q = static_cast<const T*>(p.qkv) + (size_t)b * p.N * ld + h * hd;
        k = q + p.D; v = q + 2 * p.D;
        pk = static_cast<const T*>(p.pk) + (size_t)b * p.Lp * p.D + h * hd;
        pv = static_cast<const T*>(p.pv) + (size_t)b * p.Lp * p.D + h * hd;
    }
    __device__ __forceinline__ const T* key(int j) const { return j < Lp ? pk + (size_t)j * D : k + (size_t)(j - Lp) * ld; }
    __device__ __forceinline__ const T* val(int j) const { return j < Lp ? pv + (size_t)j * D : v + (size_t)(j - Lp) * ld; }
};

template <typename T>
__global__ __launch_bounds__(256) void prefix_fwd_generic_kernel(PrefixParams p, int hd) {
    __shared__ float ps[4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;                       // (b*H + h)*N + q
    if (row >= p.B * p.H * p.N) return;
    const int q = row % p.N, bh = row / p.N, h = bh % p.H, b = bh / p.H, Lt = p.N + p.Lp;
    const HeadPtrs<T> hp(p, b, h, hd);
    const T* qp = hp.q + (size_t)q * hp.ld;
    float s[4], mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int key = lane + 64 * i;
        s[i] = -INFINITY;
        if (key < Lt) {
            const T* kp = hp.key(key);
            float a = 0.f;
            for (int d = 0; d < hd; ++d) a += Elem<T>::ld(qp + d) * Elem<T>::ld(kp + d);
            s[i] = a * p.scale;
        }
        mx = fmaxf(mx, s[i]);
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { s[i] = (lane + 64 * i) < Lt ? expf(s[i] - mx) : 0.f; sum += s[i]; }
    sum = wave_sum(sum);
#pragma unroll
    for (int i = 0; i < 4; ++i) ps[wave][lane + 64 * i] = s[i] / sum;
    if (lane == 0 && p.lse) p.lse[row] = mx + logf(sum);
    __builtin_amdgcn_wave_barrier();
    if (lane < hd) {
        float o = 0.f;
        for (int key = 0; key < Lt; ++key) o += ps[wave][key] * Elem<T>::ld(hp.val(key) + lane);
        Elem<T>::st(static_cast<T*>(p.out) + ((size_t)b * p.N + q) * p.D + h * hd + lane, o);
    }
}

// pass 1 (row = query, B*H*N rows): dsum[row] = sum_d dO*O; dQ.   pass 2 (row = key, B*H*(Lp+N) rows): dK, dV of a token, dpk, dpv of a prefix row
template <typename T, int PASS>
__global__ __launch_bounds__(256) void prefix_bwd_generic_kernel(PrefixParams p, int hd) {
    __shared__ float ps[4][256], ds_[4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    const int Lt = p.N + p.Lp, R = PASS == 1 ? p.N : Lt;
    if (row >= p.B * p.H * R) return;
    const int r = row % R, bh = row / R, h = bh % p.H, b = bh / p.H;
    const HeadPtrs<T> hp(p, b, h, hd);
    const size_t ld = hp.ld;
    const T* dob = static_cast<const T*>(p.dout) + (size_t)b * p.N * p.D + h * hd;
    const T* ob = static_cast<const T*>(p.out) + (size_t)b * p.N * p.D + h * hd;
    T* dqb = static_cast<T*>(p.dqkv) + (size_t)b * p.N * ld + h * hd;
    const float* lse = p.lse + (size_t)bh * p.N;
    float* dsum = p.dsum + (size_t)bh * p.N;
    if constexpr (PASS == 1) {
        float dd = lane < hd ? Elem<T>::ld(dob + (size_t)r * p.D + lane) * Elem<T>::ld(ob + (size_t)r * p.D + lane) : 0.f;
        dd = wave_sum(dd);
        if (lane == 0) dsum[r] = dd;
        const float l = lse[r];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = lane + 64 * i;
            float v = 0.f;
            if (key < Lt) {
                const T *kp = hp.key(key), *vp = hp.val(key);
                float a = 0.f, dp = 0.f;
                for (int d = 0; d < hd; ++d) {
                    a += Elem<T>::ld(hp.q + (size_t)r * ld + d) * Elem<T>::ld(kp + d);
                    dp += Elem<T>::ld(dob + (size_t)r * p.D + d) * Elem<T>::ld(vp + d);
                }
                v = expf(a * p.scale - l) * (dp - dd);
            }
            ds_[wave][key] = v;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < hd) {
            float a = 0.f;
            for (int key = 0; key < Lt; ++key) a += ds_[wave][key] * Elem<T>::ld(hp.key(key) + lane);
            Elem<T>::st(dqb + (size_t)r * ld + lane, a * p.scale);
        }
    } else {
        const T *kp = hp.key(r), *vp = hp.val(r);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = lane + 64 * i;
            float pv = 0.f, dv = 0.f;
            if (q < p.N) {
                float a = 0.f, dp = 0.f;
                for (int d = 0; d < hd; ++d) {
                    a += Elem<T>::ld(hp.q + (size_t)q * ld + d) * Elem<T>::ld(kp + d);
                    dp += Elem<T>::ld(dob + (size_t)q * p.D + d) * Elem<T>::ld(vp + d);
                }
                pv = expf(a * p.scale - lse[q]);
                dv = pv * (dp - dsum[q]);
            }
            ps[wave][q] = pv;
            ds_[wave][q] = dv;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < hd) {
            float ak = 0.f, av = 0.f;
            for (int q = 0; q < p.N; ++q) {
                ak += ds_[wave][q] * Elem<T>::ld(hp.q + (size_t)q * ld + lane);
                av += ps[wave][q] * Elem<T>::ld(dob + (size_t)q * p.D + lane);
            }
            if (r < p.Lp) {
                p.dpk[((size_t)b * p.Lp + r) * p.D + h * hd + lane] = ak * p.scale;
                p.dpv[((size_t)b * p.Lp + r) * p.D + h * hd + lane] = av;
            } else {
                Elem<T>::st(dqb + p.D + (size_t)(r - p.Lp) * ld + lane, ak * p.scale);
                Elem<T>::st(dqb + 2 * p.D + (size_t)(r - p.Lp) * ld + lane, av);
            }
        }
    }
}

bool force_generic() {
    static int v = -1;
    if (v < 0) { const char* e = clhip_cfg("ATTN_GENERIC"); v = (e && e[0] == '1') ? 1 : 0; }
    return v == 1;
}

int check(int B, int N, int Lp, int H, int D, int dtype) {
    CLHIP_CHECK_ARG(B > 0 && H > 0 && N > 0 && Lp >= 1 && N + Lp <= 256 && D % H == 0 && D / H <= 64 && D % 8 == 0);
    CLHIP_CHECK_ARG(dtype == CLHIP_BF16 || dtype == CLHIP_F32);
    return CLHIP_OK;
}

}  // namespace

extern "C" int clhip_attn_prefix_fwd(const void* qkv, const void* pk, const void* pv, void* out, float* lse, int B, int N, int Lp, int H, int D, int dtype,
                                     void* stream) {
    CLHIP_CHECK_ARG(qkv && pk && pv && out);
    if (int rc = check(B, N, Lp, H, D, dtype)) return rc;
    const int hd = D / H;
    PrefixParams p{qkv, pk, pv, out, lse, nullptr, nullptr, nullptr, nullptr, nullptr, B, N, Lp, H, D, 1.0f / sqrtf((float)hd)};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == CLHIP_BF16 && hd == 64 && !force_generic()) {
        const int nkt = (N + Lp + 15) >> 4;
        const size_t smem = 2 * (size_t)(((nkt + 1) & ~1) * 16) * KP;
        static bool done = false;
        if (!done) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(prefix_fwd_mfma_kernel<13>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 256 * KP);
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(prefix_fwd_mfma_kernel<14>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 256 * KP);
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(prefix_fwd_mfma_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 256 * KP);
            done = true;
        }
        if (nkt == 13) hipLaunchKernelGGL(prefix_fwd_mfma_kernel<13>, dim3(B * H), dim3(256), smem, s, p);
        else if (nkt == 14) hipLaunchKernelGGL(prefix_fwd_mfma_kernel<14>, dim3(B * H), dim3(256), smem, s, p);
        else hipLaunchKernelGGL(prefix_fwd_mfma_kernel<0>, dim3(B * H), dim3(256), smem, s, p);
    } else {
        const int rows = B * H * N;
        if (dtype == CLHIP_BF16) hipLaunchKernelGGL(prefix_fwd_generic_kernel<bf16_t>, dim3((rows + 3) / 4), dim3(256), 0, s, p, hd);
        else hipLaunchKernelGGL(prefix_fwd_generic_kernel<float>, dim3((rows + 3) / 4), dim3(256), 0, s, p, hd);
    }
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

extern "C" int clhip_attn_prefix_bwd(const void* qkv, const void* pk, const void* pv, const void* out, const float* lse, const void* dout, void* dqkv,
                                     float* dpk, float* dpv, float* dsum_ws, int B, int N, int Lp, int H, int D, int dtype, void* stream) {
    CLHIP_CHECK_ARG(qkv && pk && pv && out && lse && dout && dqkv && dpk && dpv);
    if (int rc = check(B, N, Lp, H, D, dtype)) return rc;
    const int hd = D / H;
    PrefixParams p{qkv, pk, pv, const_cast<void*>(out), const_cast<float*>(lse), dout, dqkv, dpk, dpv, dsum_ws, B, N, Lp, H, D, 1.0f / sqrtf((float)hd)};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int NQ2 = ((((N + 15) >> 4) + 1) & ~1) * 16, NK2 = ((((N + Lp + 15) >> 4) + 1) & ~1) * 16;
    const size_t smem = 2 * (size_t)(NQ2 + NK2) * KP + 2 * NQ2 * sizeof(float);
    constexpr size_t kLdsMax = 160 * 1024;       // Q, dO, K, V of one head must fit the CU's LDS; else the generic path
    if (dtype == CLHIP_BF16 && hd == 64 && smem <= kLdsMax && !force_generic()) {
        static bool done = false;
        if (!done) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(prefix_bwd_mfma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax);
            done = true;
        }
        hipLaunchKernelGGL(prefix_bwd_mfma_kernel, dim3(B * H), dim3(64 * BWD_WAVES), smem, s, p);
    } else {
        CLHIP_CHECK_ARG(dsum_ws != nullptr);
        const int rq = B * H * N, rk = B * H * (N + Lp);
        if (dtype == CLHIP_BF16) {
            hipLaunchKernelGGL((prefix_bwd_generic_kernel<bf16_t, 1>), dim3((rq + 3) / 4), dim3(256), 0, s, p, hd);
            hipLaunchKernelGGL((prefix_bwd_generic_kernel<bf16_t, 2>), dim3((rk + 3) / 4), dim3(256), 0, s, p, hd);
        } else {
            hipLaunchKernelGGL((prefix_bwd_generic_kernel<float, 1>), dim3((rq + 3) / 4), dim3(256), 0, s, p, hd);
            hipLaunchKernelGGL((prefix_bwd_generic_kernel<float, 2>), dim3((rk + 3) / 4), dim3(256), 0, s, p, hd);
        }
    }
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}
