// kernels.h -- the host functions one .hip file of libclhip defines for another (predicates, launchers, scratch sizes, tuning hooks; not part of the C ABI of
// include/clhip.h), declared ONCE and grouped by the file that defines them.  build.sh compiles with -Werror=missing-prototypes, so a definition that is missing
// here does not build, and no .hip declares one by hand (tests/test_csrc_layout_cpu.py).
#pragma once
#include "common.h"

// ---- the arguments of a 3x3 / stride-1 / pad-1 launch (conv3 / conv4 / conv5 / conv8 / conv9 / conv16+32 / conv64): named, so that an optional group is one
//      pointer that is either there or not.  A launcher that is handed a group it has no kernel for refuses (CLHIP_EINVAL); it never ignores one.
// BnSums: the BatchNorm-backward sums of the layer that PRODUCED the tensor whose gradient a dgrad launch completes (sum g and sum g * xhat per channel, g = dy masked by
// the producer's ReLU), reduced from the fp32 results in the epilogue
struct BnSums {
    const void* z = nullptr;         // [N,H,W,Cd] pre-BatchNorm output of that layer; nullptr: no reduction
    const void* y = nullptr;         // its post-activation output (ReLU mask y > 0), or nullptr: no ReLU
    const void* mask = nullptr;      // cheaper mask sources (conv8.hip only): its packed ReLU mask [N*H*W][Cd/8] ...
    const float* gamma = nullptr; const float* beta = nullptr;      // ... or its weight / bias, for a ReLU straight behind the BatchNorm (the mask from z)
    const float* mean = nullptr; const float* invstd = nullptr;
    const float* coef = nullptr;     // [2][Cd] scale, shift of that layer: its ReLU mask from z when y == nullptr (conv16 / conv32 / conv64; the activation was never written)
    double* acc = nullptr;           // [rep][2][Cd]
    int rep = 1;
};

struct ConvCall {
    const void* src = nullptr;       // [N,H,W,Cs]   (forward: x; dgrad: dz)
    const void* wt = nullptr;        // [Cd][9][Cs]
    void* dst = nullptr;             // [N,H,W,Cd]
    float* stats = nullptr;          // BatchNorm statistics of dst as partial rows [tiles_m][2][Cd] (conv3 / conv4 / conv16+32), or nullptr
    double* stat_acc = nullptr;      // ... or as fp64 accumulators [stat_rep][2][Cd], or nullptr
    int stat_rep = 1;
    int N = 0, H = 0, W = 0, Cs = 0, Cd = 0;
    int accumulate = 0;              // dst += result
    int mode = 0;                    // 0: forward; 1: dgrad
    // forward with a "lazy" BatchNorm input: src is the producer's pre-BatchNorm output and the operand is relu(bn(src) [+ res]) ...
    const LazyIn* in = nullptr;                 // ... formed in LDS and written to in->y (the LDS-DMA kernels: conv5 / conv8 / conv9)
    const clhip_bn_input* bn_in = nullptr;      // ... applied while the patch is staged through registers (conv16 / conv32 / conv64) ...
    const clhip_bn_res_input* rs = nullptr;     // ... of a conv -> BN -> +res -> ReLU producer: the launch also writes its activation and packed mask (with bn_in only)
    const BnSums* bnr = nullptr;                // dgrad with the producer's BatchNorm-backward sums in the epilogue (conv4 / conv8 / conv9 / conv16+32 / conv64)
};

// ---- bn.hip
void clhip_bn_set_fwd_stop_event(hipEvent_t ev);      // one-shot completion event of the next accumulator-path forward apply launch
void clhip_bn_set_stop_event(hipEvent_t ev);          // ... of the next accumulator-path backward apply launch
hipEvent_t clhip_bn_pending_stop_event();

// ---- conv2.hip: the generic kernels (any ksize / stride / pad, both dtypes)
int clhip_conv2_tiles_m(int M, int Cd);
int clhip_conv2_launch(const void* src, const void* wt, void* dst, float* stats, double* stat_acc, int stat_rep, int N, int Hs, int Ws, int Cs, int Hd, int Wd,
                       int Cd, int ksize, int stride, int pad, int accumulate, int mode, int dtype, hipStream_t st);
size_t clhip_wgrad2_ws_bytes(int N, int H, int W, int C, int Creal, int K, int ksize, int stride, int pad);
int clhip_wgrad2_launch(const void* x, const void* dz, float* dw, float* ws, int N, int H, int W, int C, int Creal, int K, int ksize, int stride,
                        int pad, int dtype, hipStream_t st);

// ---- conv3.hip: the halo kernel (conv3), the register-resident 16 -> 16 / 32 -> 32 (conv16) and 64 -> 64 (conv64) kernels, their weight gradients
bool clhip_conv16_supported(int H, int W, int Cs, int Cd, int ksize, int stride, int pad, int dtype);
int clhip_conv16_tiles_m(int M);
int clhip_conv16_launch(const ConvCall& c, hipStream_t st);      // Cs == Cd == 16 or 32
bool clhip_conv64_supported(int N, int H, int W, int Cs, int Cd, int ksize, int stride, int pad, int dtype);
int clhip_conv64_launch(const ConvCall& c, hipStream_t st);
bool clhip_conv3_supported(int H, int W, int Cs, int Cd, int ksize, int stride, int pad, int dtype);
int clhip_conv3_tiles_m(int M, int Cd);
int clhip_conv3_launch(const ConvCall& c, hipStream_t st);
bool clhip_wgrad32_supported(int N, int H, int W, int C, int Creal, int K, int ksize, int stride, int pad, int dtype);
size_t clhip_wgrad32_ws_bytes(int N);
int clhip_wgrad32_launch(const void* x, const void* dz, float* dw, float* ws, int N, int H, const float* x_coef, hipStream_t st);
bool clhip_wgrad64_supported(int N, int H, int W, int C, int Creal, int K, int ksize, int stride, int pad, int dtype);
size_t clhip_wgrad64_ws_bytes(int N);
int clhip_wgrad64_launch(const void* x, const void* dz, float* dw, float* ws, int N, int H, const float* x_coef, hipStream_t st);
bool clhip_wgrad16_supported(int N, int H, int W, int C, int Creal, int K, int ksize, int stride, int pad, int dtype);
size_t clhip_wgrad16_ws_bytes(int N);
int clhip_wgrad16_launch(const void* x, const void* dz, float* dw, float* ws, int N, int H, const float* x_coef, hipStream_t st);
bool clhip_wgrad3_supported(int N, int H, int W, int C, int Creal, int K, int ksize, int stride, int pad, int dtype);
size_t clhip_wgrad3_ws_bytes(int N, int H, int W, int C, int K);
int clhip_wgrad3_launch(const void* x, const void* dz, float* dw, float* ws, int N, int H, int W, int C, int Creal, int K, hipStream_t st);
// a layer's input gradient and weight gradient in one launch (conv16 / conv32 / conv64 shapes).  bnr: z / y / mean / invstd / acc / rep of the dgrad epilogue;
// x_coef: x is the producer's z (lazy), its scale / shift [2][C] (the epilogue's ReLU mask comes from z as well); lz: dz = the layer's own BatchNorm backward
bool clhip_bwd_fused_supported(int N, int H, int W, int C, int Creal, int K, int ksize, int stride, int pad, int dtype);
int clhip_bwd_fused_launch(const void* x, const void* dz, const void* w_dg, void* dx, int accumulate, float* dw, float* ws, int N, int H, int W, int C,
                           const BnSums& bnr, const float* x_coef, const clhip_bn_grad* lz, hipStream_t st);
void clhip_wgrad_defer_begin();                         // collect the partial-block reduces of the weight-gradient launches ...
void clhip_wgrad_defer_abort();
void clhip_wgrad_defer_pause(bool paused);
int clhip_wgrad_defer_flush(hipStream_t st, bool end);  // ... and run them as one launch
int clhip_wgrad_reduce_launch(const float* slab, float* dw, int64_t n4, int splits, hipStream_t st);      // dw += the `splits` partial blocks of a workspace, fixed order

// ---- conv4.hip: LDS-DMA rings, channel multiples of 64
bool clhip_conv4_supported(int N, int H, int W, int Cs, int Cd, int ksize, int stride, int pad, int dtype);
int clhip_conv4_tiles_m(int M, int Cs, int Cd, int W);
int clhip_conv4_launch(const ConvCall& c, hipStream_t st);
// hooks that take effect at once (tools/ubench; api.hip's configuration table)
void clhip_conv4_set_cfg(int wm, int wn, int kg, int ck);
void clhip_conv4_enable(int on);
void clhip_conv4_set_debug(int bits);
void clhip_conv4_set_trace(unsigned long long* dev_buf);

// ---- conv5.hip: 64 -> 64 channels, weight-stationary
bool clhip_conv5_supported(int N, int H, int W, int Cs, int Cd, int ksize, int stride, int pad, int dtype);
void clhip_conv5_enable(int on);
void clhip_conv5_min_tiles(int n);
int clhip_conv5_tiles_m(int M);
int clhip_conv5_launch(const ConvCall& c, hipStream_t st);      // (mode / in as for conv8; no bnr)

// ---- conv6.hip: the input gradient of a down-sampling block entry (3x3 / s2 + 1x1 / s2 shortcut) in one launch
bool clhip_dgrad6_supported(int N, int H, int W, int C, int K, int dtype);
void clhip_conv6_enable(int on);
void clhip_conv6_set_trace(unsigned long long* buf, int wg);
size_t clhip_dgrad6_packed_bytes(int C, int K);
int clhip_dgrad6_pack(const void* w_dg, const void* w_sc_dg, void* packed, int C, int K, hipStream_t st);
int clhip_dgrad6_launch(const void* dz, const void* w_packed, const void* dz_sc, void* dx, int accumulate, int N, int H, int W, int C, int K, hipStream_t st);

// ---- conv7.hip: the same for 16 -> 32 and 32 -> 64 channels (CifarResNet-32), packed [C][10][K]; the entry's weight gradients and forward in one launch each
bool clhip_dgrad7_supported(int N, int H, int W, int C, int K, int dtype);
size_t clhip_dgrad7_packed_bytes(int C, int K);
int clhip_dgrad7_pack(const void* w_dg, const void* w_sc_dg, void* packed, int C, int K, hipStream_t st);
int clhip_dgrad7_launch(const void* dz, const void* w_packed, const void* dz_sc, void* dx, int accumulate, int N, int H, int W, int C, int K, hipStream_t st,
                        const void* bn_z = nullptr, const void* bn_y = nullptr, const float* bn_mean = nullptr, const float* bn_invstd = nullptr, double* bn_acc = nullptr,
                        int bn_rep = 1);
bool clhip_wgrad7_supported(int N, int H, int W, int C, int K, int dtype);
size_t clhip_wgrad7_ws_bytes(int N, int C, int K, int which);
int clhip_wgrad7_launch(const void* x, const void* dz, const void* dz_sc, float* dw, float* dw_sc, float* ws3, float* ws_sc, int N, int C, hipStream_t st);
bool clhip_fwd7_supported(int N, int H, int W, int C, int K, int dtype);
int clhip_fwd7_launch(const void* x, const void* w3, const void* wsc, void* z3, void* zsc, double* acc3, int rep3, double* accsc, int repsc, int N, int H, int W, int C,
                      hipStream_t st);

// ---- conv8.hip: 64 -> 64 channels on large maps, two four-wave workgroups per CU
bool clhip_conv8_supported(int N, int H, int W, int Cs, int Cd, int ksize, int stride, int pad, int dtype);
void clhip_conv8_enable(int on);
void clhip_conv8_min_tiles(int n);
void clhip_conv8_set_trace(unsigned long long* dev_buf);
int clhip_conv8_tiles_m(int M);
// mode 0: forward (stat_acc may be nullptr); mode 1: dgrad, with the producer's BatchNorm-backward sums when bnr->z != nullptr.
// in != nullptr (forward only): src is the producer's pre-BatchNorm output, the operand relu(bn(src) [+ in->res]) is formed in LDS and written to in->y
int clhip_conv8_launch(const ConvCall& c, hipStream_t st);

// ---- conv9.hip: 128 -> 128 / 256 -> 256 channels, resident patch (mode / in / bnr as for conv8, without the cheaper mask sources)
bool clhip_conv9_supported(int N, int H, int W, int Cs, int Cd, int ksize, int stride, int pad, int dtype);
void clhip_conv9_enable(int on);
void clhip_conv9_set_trace(unsigned long long* dev_buf);
int clhip_conv9_tiles_m(int N, int H, int W, int C);
int clhip_conv9_launch(const ConvCall& c, hipStream_t st);      // Cs == Cd

// ---- gemm8.hip
int clhip_gemm8_rows(int M, int N, int K, int lda, int ldb, int ldc, int ldr, int ldh, int dtype);
int clhip_gemm8_launch(const void* A, const void* B, void* C, const float* bias, const void* R, void* H, int M, int N, int K,
                       int lda, int ldb, int ldc, int ldr, int ldh, int epilogue, hipStream_t st);

// ---- shortcut.hip: the input gradient of a 1x1 / s2 shortcut convolution
bool clhip_shortcut_supported(int N, int H, int W, int C, int K, int ksize, int stride, int pad, int dtype);
int clhip_shortcut_dgrad(const void* dz, const void* w_dg, void* dx, int accumulate, int N, int H, int W, int C, int K, hipStream_t st);

// ---- stage.hip (its predicate clhip_stage_eval_supported is part of the C ABI: include/clhip.h)
int clhip_stage_eval_launch(const void* x, void* y, int N, int H, int W, int C, int nconv, const void* const* w, const float* const* gamma, const float* const* beta,
                            const float* const* mean, const float* const* var, float eps, int dtype, hipStream_t st);

// ---- stage_train.hip (its direct entries clhip_stage_train_fwd / _bwd / _query / _status are part of the C ABI: include/clhip.h)
int clhip_stage_train_max_batch();
bool clhip_stage_train_supported(int N, int H, int W, int C, int nconv, int dtype);
size_t clhip_stage_train_xch_bytes(int N);
bool clhip_stage_train_xcd_rule(bool probe);
int clhip_stage_train_slab_blocks(int N, int C);
int clhip_stage_train_fwd_launch(const void* x, int N, int H, int W, int C, int nconv, const void* const* w, const float* const* gamma, const float* const* beta,
                                 float* const* rm, float* const* rv, float* const* mean, float* const* invstd, float* const* coef, void* const* z, void* const* y,
                                 void* const* mask, float momentum, float eps, void* xch, int trace, int entry, float* feat, int dtype, hipStream_t st);
int clhip_stage_train_bwd_launch(const void* x, const void* dy, void* dx, int dx_accumulate, int N, int H, int W, int C, int nconv, const void* const* wd,
                                 const float* const* gamma, const float* const* beta, const float* const* mean, const float* const* invstd, const void* const* z,
                                 const void* const* y, float* const* dgamma, float* const* dbeta, float* const* slab, void* const* dzg, void* xch, int trace, int entry, const float* dfeat, int dtype, hipStream_t st);
int clhip_stage_train_status(void* xch);      // (plan.hip's use of it; the C ABI declares it first, so this keeps its C linkage)
int clhip_stage_train_trace(void* xch, unsigned long long* out24);

// ---- stem.hip: <= 8 padded input channels, 3x3
bool clhip_stem_wgrad_supported(int N, int H, int W, int C, int Creal, int K, int ksize, int stride, int pad, int dtype);
size_t clhip_stem_wgrad_ws_bytes(int N, int H, int W, int Creal, int K);
int clhip_stem_wgrad_launch(const void* x, const void* dz, float* dw, float* ws, int N, int H, int W, int Creal, int K, hipStream_t st);
bool clhip_stem_supported(int N, int H, int W, int C, int K, int ksize, int stride, int pad, int dtype);
int clhip_stem_launch(const void* x, const void* w, void* z, double* acc, int rep, int N, int H, int W, int K, hipStream_t st);

// ---- stem7.hip: the ImageNet stem (7x7 / s2 / p3)
bool clhip_stem7_supported(int N, int H, int W, int C, int K, int stride, int pad);
int clhip_stem7_fwd_tiles(int N, int H, int W);
int clhip_stem7_fwd_launch(const void* x, const void* w, void* z, double* acc, int rep, int N, int H, int W, int K, int dtype, hipStream_t st);
size_t clhip_stem7_wgrad_ws_bytes(int N, int H, int W, int Creal, int K, int dtype);
int clhip_stem7_wgrad_launch(const void* x, const void* dz, float* dw, float* ws, int N, int H, int W, int Creal, int K, int dtype, hipStream_t st);

// ---- wgrad4.hip: the LDS-DMA weight gradient
bool clhip_wgrad4_supported(int N, int H, int W, int C, int Creal, int K, int ksize, int stride, int pad, int dtype);
size_t clhip_wgrad4_ws_bytes(int N, int H, int W, int C, int K, int ksize, int stride);
int clhip_wgrad4_launch(const void* x, const void* dz, float* dw, float* ws, int N, int H, int W, int C, int K, int ksize, int stride, hipStream_t st);
void clhip_wgrad4_set_trace(unsigned long long* dev_buf);
