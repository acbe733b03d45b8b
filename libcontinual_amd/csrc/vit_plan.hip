// vit_plan.hip -- whole-backbone executor for the ViT path: one C call runs the complete forward (patch embedding,
// token assembly with optional L2P prompt tokens, depth x [LN -> qkv -> attention -> proj(+res) -> LN -> fc1(GELU)
// -> fc2(+res)], final LN + pooling; CLIP's visual tower through clhip_vit_set_clip: ln_pre, QuickGELU, its own final eps) or the complete activation-gradient backward (every weight of the backbone is
// frozen in L2P and InfLoRA_OPT; the only parameter gradients are the prompt tokens, the LoRA B matrices and, with adapter_dim > 0, the
// AdaptFormer adapters of csrc/adapter.hip -- RanPAC's first session).
// Replaces VisionTransformer.forward / Transformer.forward / ResidualAttentionBlock.forward
// (core/model/backbone/transformer.py:2222-2294, 2006-2018, 1331-1336) and the autograd graph behind
// loss.backward() (l2p.py:103, trainer.py:604).  Nothing here allocates or synchronises: fixed workspace offsets.
#include <new>
#include <vector>

#include "common.h"

namespace {
size_t al(size_t v) { return (v + 255) / 256 * 256; }

enum { EPI_NONE = 0, EPI_BIAS = 1, EPI_BIAS_RES = 2, EPI_BIAS_GELU = 3, EPI_MUL = 4, EPI_BIAS_QGELU = 6 };

struct LayerShadow { size_t qkv_f, qkv_b, proj_f, proj_b, fc1_f, fc1_b, fc2_f, fc2_b, acat; };

struct Layout {          // byte offsets into the workspace for one (B, n_prompt, save) configuration
    int B, P, N, M, save;
    bool h1_own;             // h1 has a region of its own (keep_h1, or bit 1 of the flags); else it aliases ln_out, which LN2 rewrites
    size_t patches, pe_out, ln_out, act, g, dtmp, dbig, dqkv, dsum, lora_ws, g2, ad_dh, ad_ws, sd_ws, total;
    std::vector<size_t> x_in, x_mid, qkv, attn_o, hpre, h1, st1, st2, lse, ad_hd;   // per layer (x_in has depth+1 entries)
    std::vector<int> pf_lp;                  // prefix mode of the forward that filled this layout (empty = off): per layer the prefix length ...
    std::vector<const void*> pf_pk, pf_pv;   // ... and the caller's key / value rows, which the backward reads again
    float final_eps;                         // eps of the pooled final LN of that forward (1e-6, or clhip_vit_set_clip's)
};

template <typename T>
__global__ __launch_bounds__(256) void to_f32_kernel(const T* __restrict__ x, float* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = Elem<T>::ld(x + i);
}
}  // namespace

struct clhip_vit {
    clhip_vit_desc d;
    int dtype, esize, np, Kp;
    size_t shadow_bytes, pe_f;
    std::vector<LayerShadow> sh;
    Layout last;          // configuration of the most recent forward
    bool have_last;
    hipStream_t side;     // stream of the LoRA weight gradients (leaves of the backward chain), created on first use
    hipEvent_t ev_q, ev_l;
    const unsigned long long* drop_seed;   // adapter dropout of the next forward (clhip_vit_set_adapter_dropout) ...
    float drop_p;
    float last_p;                          // ... and of the forward the backward belongs to
    int sd_terms, sd_sum;                  // SD-LoRA mode (clhip_vit_set_sdlora): term count (0 = off), sum of the ranks ...
    std::vector<int> sd_ranks;
    const float* const* sd_factors;        // ... and the caller's device tables
    const float *sd_mag, *sd_inv;
    std::vector<int> pf_lp;                // prefix mode (clhip_vit_set_prefix): per layer the prefix length (empty = off) ...
    std::vector<const void*> pf_pk, pf_pv; // ... and the caller's buffers
    float* tap;                            // gradient tap (clhip_vit_set_tap; nullptr = off): host bookkeeping and copies only
    size_t tap_cap;
    int info_side, info_lowest;            // what the last backward did (clhip_vit_last_backward_info; -1 = none yet)
    bool clip_on;                          // CLIP mode (clhip_vit_set_clip): ln_pre on the assembled tokens (NULL = none), QuickGELU in the MLP, ...
    const float *clip_ln_w, *clip_ln_b;
    float clip_final_eps;                  // ... and the eps of the pooled final LN
    int clip_qgelu;
};

// The tap's slot map for the layout of the last saved forward, in floats.  Slot 0 holds g after ln_pool_bwd [M, D]; layer l's slots follow at
// M D + l * stride in the order of tap_slot_off: dbig [M, mlp] | ad_dh [M, R] | the adapter's output gradient [M, D] (both absent when R = 0) |
// dtmp after the fc1 dgrad | g after the LN2 backward | dtmp after the proj dgrad [M, D each] | dqkv [M, 3D] | dtmp after the qkv dgrad | g after the
// LN1 backward [M, D each].  A slot the backward does not write (a layer below the lowest one it runs) is left as the caller filled it.
enum { TAP_DBIG = 0, TAP_AD_DH, TAP_AD_GX, TAP_DFC1, TAP_G_LN2, TAP_DPROJ, TAP_DQKV, TAP_DQKV_IN, TAP_G_LN1, TAP_SLOTS };
static size_t tap_slot_floats(const clhip_vit* v, const Layout& L, int slot) {
    const size_t M = L.M, D = v->d.dim, R = v->d.adapter_dim;
    switch (slot) {
        case TAP_DBIG: return M * v->d.mlp;
        case TAP_AD_DH: return M * R;
        case TAP_AD_GX: return R > 0 ? M * D : 0;
        case TAP_DQKV: return M * 3 * D;
        default: return M * D;
    }
}
static size_t tap_slot_off(const clhip_vit* v, const Layout& L, int layer, int slot) {      // layer < 0: slot 0; slot == TAP_SLOTS: the layer's end
    size_t stride = 0, in = 0;
    for (int s = 0; s < TAP_SLOTS; ++s) { if (s < slot) in += tap_slot_floats(v, L, s); stride += tap_slot_floats(v, L, s); }
    if (layer < 0) return 0;
    return (size_t)L.M * v->d.dim + (size_t)layer * stride + in;
}

// `flags`: bit 0 = keep what the backward needs; bit 1 (CLHIP_VIT_KEEP_ATTN_IN) = keep every layer's attention input (LN1 output) until the
// end of the forward -- the Gram pass multiplies all of them in one launch
static void make_layout(const clhip_vit* v, int B, int P, int flags, Layout& L) {
    const clhip_vit_desc& d = v->d;
    const size_t e = v->esize;
    const int save = flags & 1;
    L.B = B; L.P = P; L.N = P + 1 + v->np; L.M = B * L.N; L.save = save;
    const size_t M = L.M, D = d.dim;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al(bytes); return o; };
    L.patches = take((size_t)B * v->np * v->Kp * e);
    L.pe_out = take((size_t)B * v->np * D * e);
    L.ln_out = take(M * D * e);
    L.act = take(M * d.mlp * e);
    const int sets = save ? d.depth : 1;
    L.x_in.assign(d.depth + 1, 0); L.x_mid.assign(d.depth, 0); L.qkv.assign(d.depth, 0); L.attn_o.assign(d.depth, 0);
    L.hpre.assign(d.depth, 0); L.h1.assign(d.depth, 0); L.st1.assign(d.depth, 0); L.st2.assign(d.depth, 0); L.lse.assign(d.depth, 0);
    const bool keep_h1 = save && (d.lora_rank > 0 || v->sd_terms > 0);
    for (int s = 0; s < sets; ++s) {
        L.x_mid[s] = take(M * D * e);
        L.qkv[s] = take(M * 3 * D * e);
        L.attn_o[s] = take(M * D * e);
        L.hpre[s] = save ? take(M * d.mlp * e) : 0;
        L.h1[s] = keep_h1 ? take(M * D * e) : L.ln_out;
        L.st1[s] = take(2 * M * sizeof(float));
        L.st2[s] = take(2 * M * sizeof(float));
        L.lse[s] = take((size_t)B * d.heads * L.N * sizeof(float));
    }
    if (save) {
        for (int l = 0; l <= d.depth; ++l) L.x_in[l] = take(M * D * e);
    } else {
        const size_t a = take(M * D * e), b = take(M * D * e);
        for (int l = 0; l <= d.depth; ++l) L.x_in[l] = (l & 1) ? b : a;
        for (int l = 1; l < d.depth; ++l) {
            L.x_mid[l] = L.x_mid[0]; L.qkv[l] = L.qkv[0]; L.attn_o[l] = L.attn_o[0]; L.hpre[l] = 0; L.h1[l] = L.ln_out;
            L.st1[l] = L.st1[0]; L.st2[l] = L.st2[0]; L.lse[l] = L.lse[0];
        }
    }
    L.h1_own = keep_h1 || (flags & 2);
    if ((flags & 2) && !keep_h1) {                       // one contiguous region, layer stride M * D elements
        const size_t base = take((size_t)d.depth * al(M * D * e));
        for (int l = 0; l < d.depth; ++l) L.h1[l] = base + (size_t)l * al(M * D * e);
    }
    if (save) {
        L.g = take(M * D * e);
        L.dtmp = take(M * D * e);
        L.dbig = take(M * d.mlp * e);
        L.dqkv = take(M * 3 * D * e);
        L.dsum = take((size_t)B * d.heads * L.N * sizeof(float));
        L.lora_ws = d.lora_rank > 0 ? take(clhip_lora_grad_ws_bytes(L.M, d.dim, d.lora_rank)) : 0;
    } else {
        L.g = L.dtmp = L.dbig = L.dqkv = L.dsum = L.lora_ws = 0;
    }
    // adapters (appended: without them every offset above and the total are what they were): the dropped hidden rows of every layer, dh, the
    // second gradient buffer (the adapter's input gradient is written out of place, so its weight gradient still reads dL/dx_out) and the slabs
    L.ad_hd.assign(d.depth, 0);
    L.g2 = L.ad_dh = L.ad_ws = 0;
    if (save && d.adapter_dim > 0) {
        for (int l = 0; l < d.depth; ++l) L.ad_hd[l] = take(M * d.adapter_dim * e);
        L.ad_dh = take(M * d.adapter_dim * e);
        L.g2 = take(M * D * e);
        L.ad_ws = take(clhip_adapter_wgrad_ws_bytes(L.M, d.dim, d.adapter_dim));
    }
    L.sd_ws = save && v->sd_terms > 0 ? take(clhip_sdlora_grad_ws_bytes(L.M, d.dim, v->sd_sum)) : 0;      // (appended, like the adapters' part)
    L.total = off;
}

extern "C" clhip_vit* clhip_vit_create(const clhip_vit_desc* desc, int dtype) {
    if (!desc || (dtype != CLHIP_BF16 && dtype != CLHIP_F32) || desc->dim <= 0 || desc->depth <= 0 || desc->heads <= 0 || desc->dim % desc->heads ||
        desc->patch <= 0 || desc->img % desc->patch || desc->dim % 64 || desc->mlp % 64 || (3 * desc->patch * desc->patch) % 64 ||
        desc->dim / desc->heads > 64 || desc->lora_rank < 0 || desc->lora_rank > 16 ||
        (desc->adapter_dim != 0 && desc->adapter_dim != 16 && desc->adapter_dim != 32 && desc->adapter_dim != 64)) {
        clhip_set_error("clhip_vit_create: invalid descriptor (dim, mlp and 3*patch^2 must be multiples of 64; head dim <= 64; rank <= 16; adapter_dim 0, 16, 32 or 64)");
        return nullptr;
    }
    clhip_vit* v = new (std::nothrow) clhip_vit();
    if (!v) { clhip_set_error("out of host memory"); return nullptr; }
    v->d = *desc; v->dtype = dtype; v->esize = dtype == CLHIP_BF16 ? 2 : 4;
    const int g = desc->img / desc->patch;
    v->np = g * g; v->Kp = 3 * desc->patch * desc->patch;
    if (v->np + 1 > 256) { clhip_set_error("clhip_vit_create: more than 256 tokens"); delete v; return nullptr; }
    const size_t e = v->esize, D = desc->dim, H = desc->mlp;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al(bytes); return o; };
    v->pe_f = take(D * v->Kp * e);
    v->sh.resize(desc->depth);
    for (auto& s : v->sh) {
        s.qkv_f = take(3 * D * D * e); s.qkv_b = take(3 * D * D * e);
        s.proj_f = take(D * D * e); s.proj_b = take(D * D * e);
        s.fc1_f = take(H * D * e); s.fc1_b = take(H * D * e);
        s.fc2_f = take(H * D * e); s.fc2_b = take(H * D * e);
        s.acat = desc->lora_rank > 0 ? take(32 * D * e) : 0;
    }
    v->shadow_bytes = off;
    v->have_last = false;
    v->drop_seed = nullptr; v->drop_p = 0.f; v->last_p = 0.f;
    v->sd_terms = v->sd_sum = 0; v->sd_factors = nullptr; v->sd_mag = v->sd_inv = nullptr;
    v->tap = nullptr; v->tap_cap = 0; v->info_side = v->info_lowest = -1;
    v->clip_on = false; v->clip_ln_w = v->clip_ln_b = nullptr; v->clip_final_eps = 1e-6f; v->clip_qgelu = 0;
    return v;
}

extern "C" void clhip_vit_destroy(clhip_vit* v) {
    if (v && v->side) {
        (void)hipStreamSynchronize(v->side);
        (void)hipEventDestroy(v->ev_q);
        (void)hipEventDestroy(v->ev_l);               // (the stream is the process-wide one: clhip_shared_stream)
    }
    delete v;
}
extern "C" size_t clhip_vit_shadow_bytes(const clhip_vit* v) { return v ? v->shadow_bytes : 0; }
extern "C" size_t clhip_vit_workspace_bytes(const clhip_vit* v, int B, int n_prompt, int save) {
    if (!v || B <= 0 || n_prompt < 0 || n_prompt + 1 + v->np > 256) return 0;
    Layout L;
    make_layout(v, B, n_prompt, save, L);
    return L.total;
}

#define TRY(x) do { int rc_ = (x); if (rc_ != CLHIP_OK) return rc_; } while (0)

static int vit_to_f32(const void* src, float* out, size_t n, int dtype, hipStream_t s) {
    const int blocks = (int)((n + 255) / 256 < 65536 ? (n + 255) / 256 : 65536);
    if (dtype == CLHIP_BF16) hipLaunchKernelGGL(to_f32_kernel<bf16_t>, dim3(blocks), dim3(256), 0, s, (const bf16_t*)src, out, n);
    else hipLaunchKernelGGL(to_f32_kernel<float>, dim3(blocks), dim3(256), 0, s, (const float*)src, out, n);
    CLHIP_LAUNCH_CHECK();
    return CLHIP_OK;
}

extern "C" int clhip_vit_set_adapter_dropout(clhip_vit* v, const unsigned long long* seed, float p) {
    CLHIP_CHECK_ARG(v && v->d.adapter_dim > 0);
    CLHIP_CHECK_ARG(p == 0.f || (p < 1.f && p * 16777216.f >= 1.f));     // the kernels' rule: 24 hash bits cannot tell a smaller p from 0
    CLHIP_CHECK_ARG((p > 0.f) == (seed != nullptr));
    v->drop_seed = seed; v->drop_p = p;
    return CLHIP_OK;
}

extern "C" int clhip_vit_set_sdlora(clhip_vit* v, int nterms, const int* ranks, const float* const* factors, const float* mag, const float* inv) {
    CLHIP_CHECK_ARG(v && nterms >= 0 && v->d.lora_rank == 0);
    if (nterms == 0) { v->sd_terms = v->sd_sum = 0; v->sd_ranks.clear(); v->sd_factors = nullptr; v->sd_mag = v->sd_inv = nullptr; v->have_last = false; return CLHIP_OK; }
    CLHIP_CHECK_ARG(ranks && factors && mag && inv && nterms <= 512);
    int sum = 0;
    for (int i = 0; i < nterms; ++i) { CLHIP_CHECK_ARG(ranks[i] >= 1 && ranks[i] <= 16); sum += ranks[i]; }
    CLHIP_CHECK_ARG(sum <= 512);
    v->sd_terms = nterms; v->sd_sum = sum; v->sd_ranks.assign(ranks, ranks + nterms);
    v->sd_factors = factors; v->sd_mag = mag; v->sd_inv = inv;
    v->have_last = false;                                    // a saved forward of another term set cannot be continued
    return CLHIP_OK;
}

extern "C" int clhip_vit_set_prefix(clhip_vit* v, const int* Lp, const void* const* pk, const void* const* pv) {
    CLHIP_CHECK_ARG(v != nullptr);
    if (Lp == nullptr) { v->pf_lp.clear(); v->pf_pk.clear(); v->pf_pv.clear(); return CLHIP_OK; }
    CLHIP_CHECK_ARG(pk && pv);
    const int n = v->d.depth;
    bool any = false;
    for (int l = 0; l < n; ++l) {
        CLHIP_CHECK_ARG(Lp[l] >= 0 && Lp[l] < 256 && (Lp[l] == 0 || (pk[l] && pv[l])));
        any = any || Lp[l] > 0;
    }
    CLHIP_CHECK_ARG(any);
    v->pf_lp.assign(Lp, Lp + n); v->pf_pk.assign(pk, pk + n); v->pf_pv.assign(pv, pv + n);
    return CLHIP_OK;
}

extern "C" int clhip_vit_set_clip(clhip_vit* v, const float* ln_pre_w, const float* ln_pre_b, float final_eps, int quick_gelu) {
    CLHIP_CHECK_ARG(v != nullptr && (ln_pre_w != nullptr) == (ln_pre_b != nullptr) && (quick_gelu == 0 || quick_gelu == 1));
    if (ln_pre_w == nullptr && quick_gelu == 0) {             // off: the executor is what it was
        v->clip_on = false; v->clip_ln_w = v->clip_ln_b = nullptr; v->clip_final_eps = 1e-6f; v->clip_qgelu = 0;
        return CLHIP_OK;
    }
    CLHIP_CHECK_ARG(final_eps > 0.f);
    CLHIP_CHECK_ARG(v->d.adapter_dim == 0 && v->sd_terms == 0 && v->pf_lp.empty());      // (a forward checks again: those modes may be set afterwards)
    v->clip_on = true; v->clip_ln_w = ln_pre_w; v->clip_ln_b = ln_pre_b; v->clip_final_eps = final_eps; v->clip_qgelu = quick_gelu;
    return CLHIP_OK;
}

extern "C" int clhip_vit_sdlora_refresh(clhip_vit* v, const clhip_vit_params* P, void* shadow, void* stream) {
    CLHIP_CHECK_ARG(v && P && P->layers && shadow && v->sd_terms > 0);
    char* sh = static_cast<char*>(shadow);
    const int n = v->d.depth;
    std::vector<const float*> w(n);
    std::vector<void*> wt(n), wtt(n);
    for (int l = 0; l < n; ++l) { w[l] = P->layers[l].qkv_w; wt[l] = sh + v->sh[l].qkv_f; wtt[l] = sh + v->sh[l].qkv_b; }
    return clhip_sdlora_refresh(n, w.data(), v->sd_factors, v->sd_ranks.data(), v->sd_terms, v->sd_mag, v->sd_inv, wt.data(), wtt.data(), v->d.dim, v->dtype, stream);
}

extern "C" int clhip_vit_prep_weights(clhip_vit* v, const clhip_vit_params* P, void* shadow, int apply_lora, int qkv_only, void* stream) {
    CLHIP_CHECK_ARG(v && P && P->layers && shadow);
    char* sh = static_cast<char*>(shadow);
    const int D = v->d.dim, H = v->d.mlp, r = apply_lora ? v->d.lora_rank : 0;
    if (qkv_only && r > 0) {
        // between optimizer steps only lora_B moves: refresh the k / v rows of all layers' qkv copies in one launch
        const int n = v->d.depth;
        std::vector<const float*> w(n), ak(n), bk(n), av(n), bv(n);
        std::vector<void*> wt(n), wtt(n);
        for (int l = 0; l < n; ++l) {
            const clhip_vit_layer_params& p = P->layers[l];
            w[l] = p.qkv_w; ak[l] = p.lora_a_k; bk[l] = p.lora_b_k; av[l] = p.lora_a_v; bv[l] = p.lora_b_v;
            wt[l] = sh + v->sh[l].qkv_f; wtt[l] = sh + v->sh[l].qkv_b;
        }
        return clhip_lora_qkv_refresh(n, w.data(), ak.data(), bk.data(), av.data(), bv.data(), wt.data(), wtt.data(), D, r, v->dtype, stream);
    }
    if (!qkv_only) TRY(clhip_weight_prep2(P->pe_w, sh + v->pe_f, nullptr, D, v->Kp, nullptr, nullptr, nullptr, nullptr, 0, v->dtype, stream));
    for (int l = 0; l < v->d.depth; ++l) {
        const clhip_vit_layer_params& p = P->layers[l];
        const LayerShadow& s = v->sh[l];
        if (r > 0) {
            CLHIP_CHECK_ARG(p.lora_a_k && p.lora_b_k && p.lora_a_v && p.lora_b_v);
            TRY(clhip_lora_acat(p.lora_a_k, p.lora_a_v, sh + s.acat, D, r, v->dtype, stream));
        }
        TRY(clhip_weight_prep2(p.qkv_w, sh + s.qkv_f, sh + s.qkv_b, 3 * D, D, p.lora_a_k, p.lora_b_k, p.lora_a_v, p.lora_b_v, r, v->dtype, stream));
        if (qkv_only) continue;
        TRY(clhip_weight_prep2(p.proj_w, sh + s.proj_f, sh + s.proj_b, D, D, nullptr, nullptr, nullptr, nullptr, 0, v->dtype, stream));
        TRY(clhip_weight_prep2(p.fc1_w, sh + s.fc1_f, sh + s.fc1_b, H, D, nullptr, nullptr, nullptr, nullptr, 0, v->dtype, stream));
        TRY(clhip_weight_prep2(p.fc2_w, sh + s.fc2_f, sh + s.fc2_b, D, H, nullptr, nullptr, nullptr, nullptr, 0, v->dtype, stream));
    }
    return CLHIP_OK;
}

extern "C" int clhip_vit_lora_refresh_ab(clhip_vit* v, const clhip_vit_params* P, void* shadow, void* stream) {
    // A and B both moved: the k / v rows of all layers' qkv copies in one launch; nothing else depends on them (clhip_lora_grad_ab packs its own operands)
    CLHIP_CHECK_ARG(v && P && P->layers && shadow && v->d.lora_rank > 0);
    for (int l = 0; l < v->d.depth; ++l) {
        const clhip_vit_layer_params& p = P->layers[l];
        CLHIP_CHECK_ARG(p.qkv_w && p.lora_a_k && p.lora_b_k && p.lora_a_v && p.lora_b_v);
    }
    return clhip_vit_prep_weights(v, P, shadow, 1, 1, stream);
}

extern "C" int clhip_vit_forward(clhip_vit* v, const clhip_vit_params* P, const void* shadow, void* workspace, const float* images, int B,
                                 const float* prompt_tokens, int n_prompt, int save, float* gram, float* feat, void* stream) {
    CLHIP_CHECK_ARG(v && P && P->layers && shadow && workspace && images && feat && B > 0 && n_prompt >= 0);
    CLHIP_CHECK_ARG(n_prompt == 0 || prompt_tokens != nullptr);
    CLHIP_CHECK_ARG(n_prompt + 1 + v->np <= 256);
    const clhip_vit_desc& d = v->d;
    const bool clip = v->clip_on;
    // CLIP mode: no prompt tokens, prefixes, adapters or SD-LoRA (none of the reference's CLIP methods combines them); refused before any launch
    if (clip) CLHIP_CHECK_ARG(n_prompt == 0 && v->pf_lp.empty() && d.adapter_dim == 0 && v->sd_terms == 0);
    CLHIP_CHECK_ARG(clip || P->pe_b != nullptr);
    Layout& L = v->last;
    make_layout(v, B, n_prompt, (save ? 1 : 0) | (gram ? 2 : 0), L);
    L.final_eps = clip ? v->clip_final_eps : 1e-6f;
    L.pf_lp = v->pf_lp; L.pf_pk = v->pf_pk; L.pf_pv = v->pf_pv;                  // (make_layout leaves them alone: the mode of THIS forward)
    v->have_last = true;
    char* ws = static_cast<char*>(workspace);
    const char* sh = static_cast<const char*>(shadow);
    const int D = d.dim, Hm = d.mlp, M = L.M, N = L.N, dt = v->dtype;
    const float beps = d.block_ln_eps > 0.f ? d.block_ln_eps : 1e-5f;
    const int R = d.adapter_dim;
    const unsigned long long* drop_seed = v->drop_seed;
    const float drop_p = v->drop_p;
    v->drop_seed = nullptr; v->drop_p = 0.f; v->last_p = drop_p;             // the dropout state is consumed by this forward
    // patch embedding (timm PatchEmbed = Conv2d(3, D, p, stride p)) as patchify + GEMM, then token assembly
    TRY(clhip_patchify(images, ws + L.patches, B, d.img, d.patch, dt, stream));
    // (CLIP's conv1 has no bias, transformer.py:2107: pe_b == NULL there)
    TRY(clhip_gemm_nt(ws + L.patches, sh + v->pe_f, ws + L.pe_out, P->pe_b, nullptr, nullptr, B * v->np, D, v->Kp, v->Kp, v->Kp, D, 0, 0,
                      P->pe_b ? EPI_BIAS : EPI_NONE, dt, stream));
    if (clip && v->clip_ln_w) {
        // ln_pre (transformer.py:2127, eps 1e-5): the assembled rows land in the LN scratch, which nothing owns before layer 0, and x_in[0] is their
        // normalised form.  Nothing below it takes a gradient (no prompt tokens in this mode), so no statistics are kept and there is no backward.
        TRY(clhip_vit_assemble(ws + L.pe_out, P->cls_token, P->pos_embed, nullptr, ws + L.ln_out, B, v->np, 0, D, dt, stream));
        TRY(clhip_ln_fwd(ws + L.ln_out, v->clip_ln_w, v->clip_ln_b, ws + L.x_in[0], nullptr, nullptr, M, D, 1e-5f, dt, stream));
    } else
        TRY(clhip_vit_assemble(ws + L.pe_out, P->cls_token, P->pos_embed, prompt_tokens, ws + L.x_in[0], B, v->np, n_prompt, D, dt, stream));
    const int epi_act = clip && v->clip_qgelu ? EPI_BIAS_QGELU : EPI_BIAS_GELU;
    for (int l = 0; l < d.depth; ++l) {
        const clhip_vit_layer_params& p = P->layers[l];
        const LayerShadow& s = v->sh[l];
        float* st1 = reinterpret_cast<float*>(ws + L.st1[l]);
        float* st2 = reinterpret_cast<float*>(ws + L.st2[l]);
        char* h1 = ws + L.h1[l];
        TRY(clhip_ln_fwd(ws + L.x_in[l], p.ln1_w, p.ln1_b, h1, st1, st1 + M, M, D, beps, dt, stream));
        TRY(clhip_gemm_nt(h1, sh + s.qkv_f, ws + L.qkv[l], p.qkv_b, nullptr, nullptr, M, 3 * D, D, D, D, 3 * D, 0, 0, EPI_BIAS, dt, stream));
        if (!L.pf_lp.empty() && L.pf_lp[l] > 0)
            TRY(clhip_attn_prefix_fwd(ws + L.qkv[l], L.pf_pk[l], L.pf_pv[l], ws + L.attn_o[l], reinterpret_cast<float*>(ws + L.lse[l]), B, N, L.pf_lp[l], d.heads, D,
                                      dt, stream));
        else
            TRY(clhip_attn_fwd(ws + L.qkv[l], ws + L.attn_o[l], reinterpret_cast<float*>(ws + L.lse[l]), B, N, d.heads, D, dt, stream));
        TRY(clhip_gemm_nt(ws + L.attn_o[l], sh + s.proj_f, ws + L.x_mid[l], p.proj_b, ws + L.x_in[l], nullptr, M, D, D, D, D, D, D, 0, EPI_BIAS_RES, dt, stream));
        TRY(clhip_ln_fwd(ws + L.x_mid[l], p.ln2_w, p.ln2_b, ws + L.ln_out, st2, st2 + M, M, D, beps, dt, stream));
        TRY(clhip_gemm_nt(ws + L.ln_out, sh + s.fc1_f, ws + L.act, p.fc1_b, nullptr, save ? ws + L.hpre[l] : nullptr, M, Hm, D, D, D, Hm, 0, Hm, epi_act, dt,
                          stream));
        TRY(clhip_gemm_nt(ws + L.act, sh + s.fc2_f, ws + L.x_in[l + 1], p.fc2_b, ws + L.x_mid[l], nullptr, M, D, Hm, Hm, Hm, D, D, 0, EPI_BIAS_RES, dt, stream));
        if (R > 0) {                                         // x_out += s * adapter(x_mid), parallel to the MLP (vision_transformer_adapter.py:165-183)
            CLHIP_CHECK_ARG(p.ad_down_w && p.ad_down_b && p.ad_up_w && p.ad_up_b);
            TRY(clhip_adapter_fwd(ws + L.x_mid[l], p.ad_down_w, p.ad_down_b, p.ad_up_w, p.ad_up_b, ws + L.x_in[l + 1], save ? ws + L.ad_hd[l] : nullptr,
                                  drop_seed, l, drop_p, d.adapter_scale, M, D, R, dt, stream));
        }
    }
    if (gram) {
        // every layer's attention input is still there (make_layout bit 1, or the backward's own copies): X_l^T X_l of all layers, one launch
        bool strided = true;
        for (int l = 1; l < d.depth; ++l) strided = strided && (L.h1[l] - L.h1[l - 1]) == (L.h1[1] - L.h1[0]) && (L.h1[1] - L.h1[0]) % v->esize == 0;
        if (strided && d.depth > 1) TRY(clhip_gram_accum_batched(ws + L.h1[0], (L.h1[1] - L.h1[0]) / v->esize, d.depth, gram, M, D, dt, stream));
        else for (int l = 0; l < d.depth; ++l) TRY(clhip_gram_accum(ws + L.h1[l], gram + (size_t)l * D * D, M, D, dt, stream));
    }
    return clhip_ln_pool_fwd(ws + L.x_in[d.depth], P->norm_w, P->norm_b, feat, B, N, D, n_prompt > 0 ? n_prompt : 1, L.final_eps, dt, stream);
}

// the leaves (d_lora_b, d_sd, d_ab) exclude one another; dpk / dpv are required exactly when the saved forward ran in prefix mode
extern "C" int clhip_vit_backward(clhip_vit* v, const clhip_vit_params* P, const void* shadow, void* workspace, const float* dfeat, const clhip_vit_grads* out,
                                  void* stream) {
    const clhip_vit_grads G = out ? *out : clhip_vit_grads{};
    float* const dprompt_tokens = G.dprompt_tokens;
    const auto d_lora_b = G.d_lora_b, d_adapter = G.d_adapter, d_sd = G.d_sd, d_ab = G.d_ab, dpk = G.dpk, dpv = G.dpv;
    CLHIP_CHECK_ARG(v && P && P->layers && shadow && workspace && dfeat);
    CLHIP_CHECK_ARG(d_sd == nullptr || (v->sd_terms > 0 && G.d_mag_rows && G.d_mag && d_lora_b == nullptr && v->last.sd_ws != 0));
    CLHIP_CHECK_ARG(d_adapter == nullptr || v->d.adapter_dim > 0);
    CLHIP_CHECK_ARG(v->have_last && v->last.save);
    const clhip_vit_desc& d = v->d;
    const Layout& L = v->last;
    CLHIP_CHECK_ARG(dprompt_tokens == nullptr || L.P > 0);
    CLHIP_CHECK_ARG(d_lora_b == nullptr || d.lora_rank > 0);
    CLHIP_CHECK_ARG(d_ab == nullptr || (d.lora_rank > 0 && G.ab_ws != nullptr && d_lora_b == nullptr && d_sd == nullptr));
    CLHIP_CHECK_ARG((dpk != nullptr) == !L.pf_lp.empty() && (dpk != nullptr) == (dpv != nullptr));
    CLHIP_CHECK_ARG(v->tap == nullptr || v->tap_cap >= tap_slot_off(v, L, v->d.depth, 0));
    int lowest = 0;                                            // the lowest layer whose attention backward somebody needs
    if (dpk && !dprompt_tokens && !d_lora_b && !d_adapter && !d_sd && !d_ab)
        while (L.pf_lp[lowest] == 0) ++lowest;
    char* ws = static_cast<char*>(workspace);
    const char* sh = static_cast<const char*>(shadow);
    const int D = d.dim, Hm = d.mlp, M = L.M, N = L.N, B = L.B, dt = v->dtype;
    char* g = ws + L.g;
    char* g2 = ws + L.g2;
    const int R = d.adapter_dim;
    // the lora_B gradients are leaves of the chain: they run on a side stream (ordered by events against the single dqkv buffer)
    static const bool two_streams = !(clhip_cfg("WGRAD_STREAM") && atoi(clhip_cfg("WGRAD_STREAM")) == 0);
    hipStream_t main_s = static_cast<hipStream_t>(stream);
    // (inside a stream capture everything stays on the captured stream, as plan.hip does: no fork / join nodes, no stream probe)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(main_s, &cap);
    const bool side_on = two_streams && (d_lora_b != nullptr || d_sd != nullptr || d_ab != nullptr) && cap == hipStreamCaptureStatusNone;
    hipStream_t shared_side = side_on ? clhip_shared_stream(0, main_s, false) : nullptr;
    if (side_on && shared_side == nullptr) { clhip_set_error("clhip_vit_backward: cannot create the side stream"); return CLHIP_EHIP; }
    const bool first_side = side_on && !v->side;
    if (side_on) v->side = shared_side;
    if (first_side) {
        (void)hipEventCreateWithFlags(&v->ev_q, hipEventDisableTiming);
        (void)hipEventCreateWithFlags(&v->ev_l, hipEventDisableTiming);
    }
    bool lora_pending = false;
    // a leaf that reads dqkv: on the side stream once the caller's stream has written dqkv (ev_q), its end marked for the next writer (ev_l); else in line
    auto leaf = [&](auto&& run) -> int {
        if (!side_on) return run(stream);
        (void)hipEventRecord(v->ev_q, main_s);
        (void)hipStreamWaitEvent(v->side, v->ev_q, 0);
        TRY(run(v->side));
        (void)hipEventRecord(v->ev_l, v->side);
        lora_pending = true;
        return CLHIP_OK;
    };
    // the tap: a copy of a chain buffer to fp32 on the caller's stream right after the launch that wrote it (one more reader ahead of the next writer)
    auto tap = [&](const void* src, int layer, int slot) -> int {
        if (!v->tap) return CLHIP_OK;
        const size_t n = layer < 0 ? (size_t)M * D : tap_slot_floats(v, L, slot);
        return n ? vit_to_f32(src, v->tap + tap_slot_off(v, L, layer, slot), n, dt, main_s) : CLHIP_OK;
    };
    v->info_side = side_on ? 1 : 0; v->info_lowest = -1;
    TRY(clhip_ln_pool_bwd(dfeat, ws + L.x_in[d.depth], P->norm_w, g, B, N, D, L.P > 0 ? L.P : 1, L.final_eps, dt, stream));
    TRY(tap(g, -1, 0));
    for (int l = d.depth - 1; l >= 0; --l) {
        const clhip_vit_layer_params& p = P->layers[l];
        const LayerShadow& s = v->sh[l];
        const float* st1 = reinterpret_cast<const float*>(ws + L.st1[l]);
        const float* st2 = reinterpret_cast<const float*>(ws + L.st2[l]);
        // MLP branch: x_out = x_mid + fc2(gelu(fc1(LN2(x_mid))))
        v->info_lowest = l;
        TRY(clhip_gemm_nt(g, sh + s.fc2_b, ws + L.dbig, nullptr, nullptr, ws + L.hpre[l], M, Hm, D, D, D, Hm, 0, Hm, EPI_MUL, dt, stream));
        TRY(tap(ws + L.dbig, l, TAP_DBIG));
        if (R > 0) {
            // adapter branch: g is dL/dx_out here (the fc2 dgrad above has read it, LN2's += comes below).  g2 = g + dh Wd, then the two buffers
            // swap roles: the chain goes on in g2 and the weight gradient still finds dL/dx_out in the old one.  One stream: one summation order.
            CLHIP_CHECK_ARG(p.ad_down_w && p.ad_up_w);
            TRY(clhip_adapter_bwd(g, ws + L.ad_hd[l], p.ad_up_w, p.ad_down_w, ws + L.ad_dh, g2, v->last_p, d.adapter_scale, M, D, R, dt, stream));
            TRY(tap(ws + L.ad_dh, l, TAP_AD_DH));
            TRY(tap(g2, l, TAP_AD_GX));
            if (d_adapter) {
                float* const* ga = d_adapter + 4 * l;
                CLHIP_CHECK_ARG(ga[0] && ga[1] && ga[2] && ga[3]);
                TRY(clhip_adapter_wgrad(g, ws + L.ad_hd[l], ws + L.x_mid[l], ws + L.ad_dh, ga[2], ga[3], ga[0], ga[1], ws + L.ad_ws, d.adapter_scale, M, D, R,
                                        dt, stream));
            }
            char* t = g; g = g2; g2 = t;
        }
        TRY(clhip_gemm_nt(ws + L.dbig, sh + s.fc1_b, ws + L.dtmp, nullptr, nullptr, nullptr, M, D, Hm, Hm, Hm, D, 0, 0, EPI_NONE, dt, stream));
        TRY(tap(ws + L.dtmp, l, TAP_DFC1));
        TRY(clhip_ln_bwd(ws + L.dtmp, ws + L.x_mid[l], p.ln2_w, st2, st2 + M, g, M, D, dt, stream));
        TRY(tap(g, l, TAP_G_LN2));
        // attention branch: x_mid = x_in + proj(attn(qkv(LN1(x_in))))
        TRY(clhip_gemm_nt(g, sh + s.proj_b, ws + L.dtmp, nullptr, nullptr, nullptr, M, D, D, D, D, D, 0, 0, EPI_NONE, dt, stream));
        TRY(tap(ws + L.dtmp, l, TAP_DPROJ));
        if (lora_pending) { (void)hipStreamWaitEvent(main_s, v->ev_l, 0); lora_pending = false; }     // the previous layer's dB has read dqkv
        if (dpk && L.pf_lp[l] > 0) {
            CLHIP_CHECK_ARG(dpk[l] && dpv[l]);
            TRY(clhip_attn_prefix_bwd(ws + L.qkv[l], L.pf_pk[l], L.pf_pv[l], ws + L.attn_o[l], reinterpret_cast<const float*>(ws + L.lse[l]), ws + L.dtmp,
                                      ws + L.dqkv, dpk[l], dpv[l], reinterpret_cast<float*>(ws + L.dsum), B, N, L.pf_lp[l], d.heads, D, dt, stream));
        } else
            TRY(clhip_attn_bwd(ws + L.qkv[l], ws + L.attn_o[l], reinterpret_cast<const float*>(ws + L.lse[l]), ws + L.dtmp, ws + L.dqkv,
                               reinterpret_cast<float*>(ws + L.dsum), B, N, d.heads, D, dt, stream));
        TRY(tap(ws + L.dqkv, l, TAP_DQKV));
        if (d_lora_b) {
            CLHIP_CHECK_ARG(p.lora_a_k && p.lora_a_v && d_lora_b[2 * l] && d_lora_b[2 * l + 1]);
            TRY(leaf([&](void* ls) {
                return clhip_lora_grad(ws + L.h1[l], ws + L.dqkv, p.lora_a_k, p.lora_a_v, sh + s.acat, d_lora_b[2 * l], d_lora_b[2 * l + 1], ws + L.lora_ws, M, D,
                                       d.lora_rank, dt, ls);
            }));
        }
        if (d_sd) {
            float* const* gs = d_sd + 4 * l;
            CLHIP_CHECK_ARG(gs[0] && gs[1] && gs[2] && gs[3]);
            TRY(leaf([&](void* ls) {
                return clhip_sdlora_grad(ws + L.h1[l], ws + L.dqkv, v->sd_factors + (size_t)l * 4 * v->sd_terms, v->sd_ranks.data(), v->sd_terms, v->sd_mag,
                                         v->sd_inv + (size_t)l * 2 * v->sd_terms, gs[0], gs[1], gs[2], gs[3], G.d_mag_rows + (size_t)l * v->sd_terms, ws + L.sd_ws, M,
                                         D, dt, ls);
            }));
        }
        if (d_ab) {
            float* const* ga = d_ab + 4 * l;
            CLHIP_CHECK_ARG(p.lora_a_k && p.lora_b_k && p.lora_a_v && p.lora_b_v && ga[0] && ga[1] && ga[2] && ga[3]);
            TRY(leaf([&](void* ls) {
                return clhip_lora_grad_ab(ws + L.h1[l], ws + L.dqkv, p.lora_a_k, p.lora_b_k, p.lora_a_v, p.lora_b_v, ga[0], ga[1], ga[2], ga[3], G.ab_ws, M, D,
                                          d.lora_rank, dt, ls);
            }));
        }
        if (l == lowest && dprompt_tokens == nullptr) break;      // nothing below the first block (or the lowest prefixed one) needs a gradient
        TRY(clhip_gemm_nt(ws + L.dqkv, sh + s.qkv_b, ws + L.dtmp, nullptr, nullptr, nullptr, M, D, 3 * D, 3 * D, 3 * D, D, 0, 0, EPI_NONE, dt, stream));
        TRY(tap(ws + L.dtmp, l, TAP_DQKV_IN));
        TRY(clhip_ln_bwd(ws + L.dtmp, ws + L.x_in[l], p.ln1_w, st1, st1 + M, g, M, D, dt, stream));
        TRY(tap(g, l, TAP_G_LN1));
    }
    if (dprompt_tokens) TRY(clhip_vit_prompt_grad(g, dprompt_tokens, B, N, L.P, D, dt, stream));
    if (lora_pending) (void)hipStreamWaitEvent(main_s, v->ev_l, 0);          // the caller's stream owns the gradients again
    return d_sd ? clhip_sdlora_mag_reduce(G.d_mag_rows, d.depth, v->sd_terms, G.d_mag, stream) : CLHIP_OK;
}

extern "C" int clhip_vit_read_act(clhip_vit* v, void* workspace, int layer, int which, float* out, void* stream) {
    CLHIP_CHECK_ARG(v && workspace && out && v->have_last);
    CLHIP_CHECK_ARG(layer >= 0 && layer <= v->d.depth && which >= 0 && which <= 9 && (layer < v->d.depth || which == 0));
    const Layout& L = v->last;
    // a forward that did not save keeps one set of buffers for all layers: only the attention inputs of a Gram pass (which 5) are still there
    CLHIP_CHECK_ARG(L.save || which == 5);
    const size_t D = v->d.dim, M = L.M;
    size_t off, n;
    int dt = v->dtype;
    switch (which) {
        case 0: off = L.x_in[layer]; n = M * D; break;
        case 1: off = L.qkv[layer]; n = M * 3 * D; break;
        case 2: off = L.attn_o[layer]; n = M * D; break;
        case 3: off = L.x_mid[layer]; n = M * D; break;
        case 4: off = L.hpre[layer]; n = M * v->d.mlp; break;
        case 5:
            if (!L.h1_own) { clhip_set_error("clhip_vit_read_act: the LN1 output aliases the LN2 scratch in this layout"); return CLHIP_EINVAL; }
            off = L.h1[layer]; n = M * D; break;
        case 6: off = L.lse[layer]; n = (size_t)L.B * v->d.heads * L.N; dt = CLHIP_F32; break;
        case 7: off = L.st1[layer]; n = 2 * M; dt = CLHIP_F32; break;
        case 8: off = L.st2[layer]; n = 2 * M; dt = CLHIP_F32; break;
        default:
            if (v->d.adapter_dim <= 0) { clhip_set_error("clhip_vit_read_act: no adapters in this executor"); return CLHIP_EINVAL; }
            off = L.ad_hd[layer]; n = M * v->d.adapter_dim; break;
    }
    return vit_to_f32(static_cast<const char*>(workspace) + off, out, n, dt, static_cast<hipStream_t>(stream));
}

extern "C" int clhip_vit_set_tap(clhip_vit* v, float* buf, size_t floats) {
    CLHIP_CHECK_ARG(v && (buf != nullptr) == (floats > 0));
    v->tap = buf; v->tap_cap = floats;
    return CLHIP_OK;
}

extern "C" size_t clhip_vit_tap_floats(const clhip_vit* v) {
    return v && v->have_last && v->last.save ? tap_slot_off(v, v->last, v->d.depth, 0) : 0;
}

extern "C" int clhip_vit_last_backward_info(const clhip_vit* v, int* side_stream_used, int* lowest_layer_run) {
    CLHIP_CHECK_ARG(v && side_stream_used && lowest_layer_run && v->info_side >= 0);
    *side_stream_used = v->info_side; *lowest_layer_run = v->info_lowest;
    return CLHIP_OK;
}
