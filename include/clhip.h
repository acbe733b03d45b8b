/*
 * clhip.h -- C ABI of libclhip.so, the MI355X (gfx950) hot-path library of libcontinual_amd.
 *
 * The reference (RL-VIG/LibContinual) is 100 % Python on torch and has no FFI of its own
 * (SURVEY.md section 2.6): every FLOP of its hot path is a torch op called from
 *   core/trainer.py:585-612            (the batch loop)
 *   core/model/{finetune,ewc,lwf,icarl,lucir}.py  (observe / inference / Fisher)
 *   core/model/backbone/resnet.py      (ResNet forward)
 *   core/model/backbone/{transformer,vit,prompt}.py  (the frozen ViT, its prompted forward and the prompt pools
 *                                       of L2P, CODA-Prompt and DualPrompt: clhip_vit_*, clhip_l2p_*, clhip_coda_*, clhip_dual_*)
 * The entry points below are what those call sites bind to in the drop-in (INTEGRATION.md shows
 * the ctypes stubs); each declaration cites the reference lines whose arithmetic it replaces.
 *
 * Conventions
 *   - plain C, no torch types; all pointers are DEVICE pointers borrowed for the call (the caller
 *     -- torch's caching allocator -- keeps ownership), except where marked "host".
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *   - return 0 on success, a negative CLHIP_E* code otherwise; never throws.  clhip_last_error()
 *     gives a thread-local message.  Functions are re-entrant per stream; no global mutable state.
 *   - activations are NHWC in `dtype` (CLHIP_BF16 = bf16 storage / bf16 MFMA / fp32 accumulate,
 *     CLHIP_F32 = fp32 storage / fp32 MFMA: the exact-arithmetic parity mode); parameters,
 *     gradients, optimizer state, Fisher, BN statistics and losses are always fp32.
 *   - conv weights (fp32 master) are stored K,R,S,C ("channels_last" strides of a [K,C,R,S] tensor).
 */
#ifndef CLHIP_H
#define CLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLHIP_OK 0
#define CLHIP_EINVAL (-1)   /* bad argument / unsupported shape */
#define CLHIP_EHIP (-2)     /* a HIP runtime call failed */
#define CLHIP_ENOMEM (-3)

#define CLHIP_BF16 0
#define CLHIP_F32 1

const char* clhip_last_error(void);
int clhip_version(void);

/* ------------------------------------------------------------------------------------------------
 * Layout / precision conversion.
 * x: fp32 NCHW [N,C,H,W] (the batch dict's "image", core/data/dataset.py:266)  ->  y: NHWC `dtype`
 * with channels zero-padded to Cpad (multiple of 8).                                               */
int clhip_nchw_to_nhwc(const float* x, void* y, int N, int C, int H, int W, int Cpad, int dtype, void* stream);
/* y: NHWC `dtype` [N,H,W,C] -> x: fp32 NCHW (for 'fmaps', backbone/resnet.py:392-395) */
int clhip_nhwc_to_nchw(const void* y, float* x, int N, int C, int H, int W, int dtype, void* stream);

/* fp32 master conv weight [K][taps][Creal] -> `dtype` shadows:
 *   w_fwd [K][taps][Cpad]   (forward / wgrad operand)
 *   w_dg  [Cpad][taps][K]   (dgrad operand), may be NULL                                           */
int clhip_conv_weight_prep(const float* w, void* w_fwd, void* w_dg, int K, int taps, int Creal, int Cpad,
                           int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Convolution as implicit GEMM on MFMA (replaces nn.Conv2d fwd / dgrad / wgrad, reference
 * backbone/resnet.py:17-24, 295-298, 337, 367).  ksize in {1,3}; C, K multiples of 8 (pad the
 * 3-channel stem to 8); H,W arbitrary.  Ho = (H + 2*pad - ksize)/stride + 1.
 * ksize 7 (fwd, wgrad and their sizing queries only): the ImageNet stem conv1 = Conv2d(3, 64, 7, stride 2, pad 3)
 * (resnet.py:136-137) with C == 8 (padded), stride 2, pad 3, K in {16, 32, 64}, both dtypes; the forward takes the
 * statistics through stat_acc only (stat_partials must be NULL) and the weight gradient needs `ws` (deterministic
 * partial blocks).  Any other 7x7 call, and every 7x7 dgrad, returns CLHIP_EINVAL.
 *
 * fwd : z[N,Ho,Wo,K] = conv(x[N,H,W,C], w_fwd).  If stat_partials != NULL it receives per-tile
 *       partial sums for train-mode BatchNorm: float[tiles][2][K] (sum, sum of squares of the fp32
 *       accumulators), tiles = clhip_conv_fwd_tiles(); *not* atomics -> deterministic.
 * dgrad: dx[N,H,W,C] (+)= conv^T(dz[N,Ho,Wo,K], w_dg);  accumulate!=0 adds to the existing dx.
 * wgrad: dw[K][taps][Creal] += sum_pixels dz * x   (fp32).  `ws` (nullable) is scratch of
 *        clhip_conv_wgrad_ws_bytes() bytes: with it the 3x3/s1 kernel writes per-split partial blocks and reduces
 *        them in a fixed order (bitwise reproducible); without it partial sums are combined with fp32 atomics. */
int clhip_conv_fwd_tiles(int N, int H, int W, int C, int K, int ksize, int stride, int pad);
int clhip_conv_fwd(const void* x, const void* w_fwd, void* z, float* stat_partials, int N, int H, int W, int C, int K,
                   int ksize, int stride, int pad, int dtype, void* stream);
/* same forward, but the per-channel sums of z and z^2 are ADDED into stat_acc[replicas][2][K] (fp64, hardware atomics; zeroed
 * by the caller; a workgroup uses replica blockIdx & (replicas-1), replicas = power of two <= 64) instead of written as per-tile
 * partial rows: the consumer (clhip_bn_apply_train) sums the replicas itself and needs no finalize launch */
int clhip_conv_fwd_acc(const void* x, const void* w_fwd, void* z, double* stat_acc, int replicas, int N, int H, int W, int C, int K,
                       int ksize, int stride, int pad, int dtype, void* stream);
int clhip_conv_dgrad(const void* dz, const void* w_dg, void* dx, int accumulate, int N, int H, int W, int C, int K,
                     int ksize, int stride, int pad, int dtype, void* stream);
/* clhip_conv_dgrad whose epilogue also reduces the BatchNorm backward of the layer that PRODUCED the tensor x (the two per-channel
 * sums of autograd's batch-norm backward, resnet.py:296-316: sum g and sum g * xhat with g = dx * (y_prod > 0), xhat =
 * (z_prod - mean) * invstd), from the fp32 results before they are rounded: the separate reduction pass over dx and z_prod
 * (first launch of clhip_bn_bwd_acc) disappears.  Valid when this launch COMPLETES dx (it is the last writer / accumulator).
 * z_prod, y_prod: [N,H,W,C] pre- / post-activation outputs of the producing layer (y_prod NULL: no ReLU); acc[replicas][2][C] fp64,
 * zeroed by the caller.  3x3 / stride 1 / pad 1 bf16 layers the fourth-generation kernel covers:
 * clhip_conv_dgrad_bn_reduce_supported() != 0. */
int clhip_conv_dgrad_bn_reduce_supported(int N, int H, int W, int C, int K, int ksize, int stride, int pad, int dtype);
/* != 0: the layer runs on a kernel that hides this epilogue (conv8.hip: two workgroups per CU, one multiplies while the other reduces), so the
 * fused form pays on large maps as well -- the plan fuses such layers whatever their pixel count */
int clhip_conv_dgrad_bn_reduce_overlapped(int N, int H, int W, int C, int K, int ksize, int stride, int pad, int dtype);
int clhip_conv_dgrad_bn_reduce(const void* dz, const void* w_dg, void* dx, int accumulate, const void* z_prod, const void* y_prod /*nullable*/,
                               const float* mean, const float* invstd, double* acc, int replicas, int N, int H, int W, int C, int K,
                               int ksize, int stride, int pad, int dtype, void* stream);
/* ... with cheaper sources for the producer's ReLU mask (both nullable; kernels that cannot use them fall back to y_prod): mask_prod = its packed mask
 * [N*H*W][C/8] (bit e of byte c/8 = element c%8 > 0, what clhip_bn_apply_train_mask writes), gamma_prod / beta_prod = its weight / bias for a ReLU straight
 * behind the BatchNorm (mask = scale z + shift > 0, scale = gamma * invstd, shift = beta - mean * scale as in the forward) */
int clhip_conv_dgrad_bn_reduce_ex(const void* dz, const void* w_dg, void* dx, int accumulate, const void* z_prod, const void* y_prod /*nullable*/,
                                  const void* mask_prod /*nullable*/, const float* gamma_prod /*nullable*/, const float* beta_prod, const float* mean, const float* invstd, double* acc,
                                  int replicas, int N, int H, int W, int C, int K, int ksize, int stride, int pad, int dtype, void* stream);
size_t clhip_conv_wgrad_ws_bytes(int N, int H, int W, int C, int Creal, int K, int ksize, int stride, int pad, int dtype);
int clhip_conv_wgrad(const void* x, const void* dz, float* dw, void* ws, int N, int H, int W, int C, int Creal, int K, int ksize,
                     int stride, int pad, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm2d (+ residual add + ReLU), reference backbone/resnet.py:296-316 (nn.BatchNorm2d,
 * momentum 0.1, eps 1e-5; train = batch statistics + running-stat update with unbiased variance).
 *
 * bn_stats_finalize: reduce the conv's stat partials -> mean/invstd (saved for backward) and the
 *   fused affine scale = gamma*invstd, shift = beta - mean*scale; updates running_mean/var.
 * bn_eval_affine: scale/shift from the running statistics (eval mode).
 * bn_apply: y = [relu]( z*scale[c] + shift[c] [+ res] ).
 * bn_bwd: given dy (grad wrt y), y (ReLU mask), z:  dgamma,dbeta (+= into fp32 grads), dz, and the
 *   residual-branch gradient dres (= masked dy; written or accumulated).  `ws` = float scratch of
 *   clhip_bn_bwd_ws_floats(M, C) floats.                                                            */
int clhip_bn_stats_finalize(const float* stat_partials, int tiles, int64_t M, int C, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, float momentum, float eps, float* mean,
                            float* invstd, float* scale, float* shift, void* stream);
int clhip_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                         float eps, int C, float* scale, float* shift, void* stream);
int clhip_bn_apply(const void* z, const float* scale, const float* shift, const void* res, void* y, int64_t M, int C,
                   int relu, int dtype, void* stream);
/* eval-mode BatchNorm (running statistics) [+ residual] [+ ReLU] in ONE launch: clhip_bn_eval_affine + clhip_bn_apply with the per-channel
 * scale / shift derived per workgroup (same expressions, same values).  nn.BatchNorm2d.eval() of the reference backbones (resnet.py:296-316). */
int clhip_bn_apply_eval(const void* z, const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                        const void* res /*nullable*/, void* y, int64_t M, int C, int relu, int dtype, void* stream);
/* training-mode BatchNorm straight from the fp64 sums of clhip_conv_fwd_acc: y = relu?(bn(z) + res?), batch mean / invstd saved
 * for the backward, running statistics updated (momentum, unbiased variance) -- bn_stats_finalize + bn_apply in ONE launch.
 * C must be a power of two. */
int clhip_bn_apply_train(const void* z, const double* stat_acc, int replicas, int64_t M, int C, const float* gamma, const float* beta, float* rm,
                         float* rv, float momentum, float eps, float* mean, float* invstd, const void* res /*nullable*/, void* y,
                         int relu, int dtype, void* stream);
/* clhip_bn_apply_train with ReLU that also writes the packed ReLU mask the backward can read instead of y: relu_mask[M * C / 8] bytes,
 * bit j of byte i = (stored y[8 i + j] > 0).  The mask of `out = F.relu(out + residual)` (resnet.py:316) costs the backward 1/16 of the
 * bytes of the activation. */
int clhip_bn_apply_train_mask(const void* z, const double* stat_acc, int replicas, int64_t M, int C, const float* gamma, const float* beta, float* rm,
                              float* rv, float momentum, float eps, float* mean, float* invstd, const void* res /*nullable*/, void* y,
                              void* relu_mask, int dtype, void* stream);
/* clhip_bn_bwd with the two per-channel sums accumulated into acc[replicas][2][C] (fp64 atomics, zeroed by the caller) and
 * consumed directly by the apply pass: no partial buffer, no finalize launch.  relu: 0 none, 1 mask = (y > 0), 3: `y` points to the
 * packed mask of clhip_bn_apply_train_mask. */
int clhip_bn_bwd_acc(const void* dy, const void* y, const void* z, const float* mean, const float* invstd, const float* gamma,
                     float* dgamma, float* dbeta, void* dz, void* dres, int dres_accumulate, int64_t M, int C, int relu, double* acc,
                     int replicas, int dtype, void* stream);
/* the same for a unit whose ReLU follows the BatchNorm directly (no residual): the ReLU mask is recomputed from z with the forward's
 * own scale / shift expressions (gamma * invstd, beta - mean * scale), so the activation tensor is not read                          */
int clhip_bn_bwd_acc_zmask(const void* dy, const void* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                           float* dgamma, float* dbeta, void* dz, int64_t M, int C, double* acc, int replicas, int dtype, void* stream);
/* The apply half alone: acc[replicas][2][C] already holds sum g and sum g * xhat -- accumulated by the launch that produced dy
 * (clhip_conv_dgrad_bn_reduce).  relu: 0 none, 1 mask = (y > 0), 2 mask recomputed from z, gamma, beta (then beta is required and
 * dres must be NULL), 3: `y` points to the packed mask of clhip_bn_apply_train_mask.  Same arithmetic as the second launch of clhip_bn_bwd_acc (autograd of nn.BatchNorm2d + ReLU + residual add,
 * core/model/backbone/resnet.py:296-316). */
int clhip_bn_bwd_apply_acc(const void* dy, const void* y /*nullable*/, const void* z, const float* mean, const float* invstd, const float* gamma,
                           const float* beta /*nullable*/, float* dgamma, float* dbeta, void* dz, void* dres /*nullable*/, int dres_accumulate,
                           int64_t M, int C, int relu, const double* acc, int replicas, int dtype, void* stream);
/* number of reduction workgroups clhip_bn_bwd / clhip_bn_bwd_acc launch (= producers adding into the accumulator) */
int clhip_bn_bwd_blocks(int64_t M, int C);
size_t clhip_bn_bwd_ws_floats(int64_t M, int C);
int clhip_bn_bwd(const void* dy, const void* y, const void* z, const float* mean, const float* invstd, const float* gamma,
                 float* dgamma, float* dbeta, void* dz, void* dres, int dres_accumulate, int64_t M, int C, int relu,
                 float* ws, int dtype, void* stream);

/* global average pool: feat[N,C] (fp32) = mean_hw a[N,HW,C]; backward broadcasts dfeat/HW           */
int clhip_avgpool_fwd(const void* a, float* feat, int N, int HW, int C, int dtype, void* stream);
int clhip_avgpool_bwd(const float* dfeat, void* da, int N, int HW, int C, int dtype, void* stream);
/* clhip_avgpool_bwd that also reduces the BatchNorm backward of the layer that PRODUCED the pooled activation (the backbone's last unit; the pooling
 * is that activation's only reader): z_prod, y_prod (nullable: no ReLU), mean, invstd, acc [replicas][2][C] fp64 as clhip_conv_dgrad_bn_reduce.
 * C a power of two in [8, 2048].  _supported: 1 / 0. */
int clhip_avgpool_bwd_bn_reduce_supported(int N, int HW, int C, int dtype);
int clhip_avgpool_bwd_bn_reduce(const float* dfeat, void* da, const void* z_prod, const void* y_prod /*nullable*/, const float* mean, const float* invstd,
                                double* acc, int replicas, int N, int HW, int C, int dtype, void* stream);

/* The ImageNet stem's BatchNorm -> ReLU -> MaxPool2d(kernel_size=3, stride=2, padding=1) (reference resnet.py:138-149, 217-218), fused.
 * clhip_maxpool_out_dim(H) = (H - 1) / 2 + 1 (nn.MaxPool2d's floor rule for these settings).
 * fwd: z [N,H,W,C] (the stem conv's raw output) -> y [N,Hp,Wp,C] = maxpool(relu(bn(z))) and argmax [N,Hp,Wp,C] uint8 (nullable) = the window position
 *   (ky * 3 + kx, row-major from the top-left corner at (2 hp - 1, 2 wp - 1)) of the first maximum -- torch's `val > maxval` rule: ties go to the
 *   earliest position, padding never wins.  training != 0: batch statistics from stat_acc [replicas][2][C] (the conv's sums, as clhip_bn_apply_train),
 *   mean / invstd saved, running statistics updated when non-NULL; training == 0: running statistics (nn.BatchNorm2d eval), stat_acc / mean / invstd
 *   ignored.  C a power of two in [8, 2048].
 * bwd (gather form, no atomics on the tensor): g [N,H,W,C] = (bn(z) > 0) * sum of dy [N,Hp,Wp,C] over the <= 4 pooled outputs whose argmax is
 *   the pixel (MaxPool2d + ReLU backward), and the two BatchNorm-backward sums (sum g, sum g * xhat) ADDED into acc [replicas][2][C] as
 *   clhip_conv_dgrad_bn_reduce does: clhip_bn_bwd_apply_acc(relu = 0) on g then forms dz. */
int clhip_maxpool_out_dim(int H);
int clhip_bn_relu_maxpool_fwd(const void* z, const double* stat_acc, int replicas, const float* gamma, const float* beta, float* running_mean,
                              float* running_var, float momentum, float eps, float* mean, float* invstd, void* y, void* argmax /*nullable*/, int N, int H,
                              int W, int C, int training, int dtype, void* stream);
int clhip_maxpool_bwd_bn_reduce(const void* dy, const void* argmax, const void* z, const float* mean, const float* invstd, const float* gamma,
                                const float* beta, void* g, double* acc, int replicas, int N, int H, int W, int C, int dtype, void* stream);

/* AvgPool2d(win) + NCHW flatten: feat[n][(c*Ph + ph)*Pw + pw] (fp32), Ph = H/win, Pw = W/win (resnet.py:643, 675-676) */
int clhip_avgpool_win_fwd(const void* a, float* feat, int N, int H, int W, int C, int win, int dtype, void* stream);
int clhip_avgpool_win_bwd(const float* dfeat, void* da, int N, int H, int W, int C, int win, int dtype, void* stream);

/* z[M,C] += r[M,C] in place and, when stat_acc != NULL, the per-channel sum / sum of squares of the result added into the fp64
 * accumulator [replicas][2][C] that clhip_bn_apply_train reads: `out += residual` of BasicBlock2 (resnet.py:615) followed by the
 * next block's bn1 (:602).  clhip_add_stats_blocks = number of producer workgroups (for sizing `replicas`).                         */
int clhip_add_stats_blocks(int64_t M, int C);
int clhip_add_stats(void* z, const void* r, double* stat_acc, int replicas, int64_t M, int C, int dtype, void* stream);
/* a[n] += b[n] (n % 8 == 0): joins the two gradient paths of a raw sum (autograd's accumulation at `out += residual`) */
int clhip_add_inplace(void* a, const void* b, int64_t n, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Whole-backbone plan: a static list of (conv -> BN -> +res -> ReLU) units + global avg-pool, run
 * with ONE call per direction (replaces the per-op dispatch of CifarResNet.forward / ResNet._forward_impl
 * / modified_ResNet.forward, backbone/resnet.py:381-395, 215-223, 549-560, and autograd's backward).  */
/* bits of clhip_unit_desc.relu.  The last three re-associate pre-activation blocks (ResNet_BIC / BasicBlock2, backbone/resnet.py:589-680:
 * BN -> ReLU -> conv, the shortcut added to the RAW conv output, BN-free 1x1 shortcut convs) onto the same unit list: a unit is then
 * conv -> (+ raw sum of unit res-1) -> BatchNorm of the FOLLOWING block -> ReLU.                                                      */
enum {
    CLHIP_UNIT_RELU = 1,     /* ReLU after the BatchNorm (+ residual)                                                                 */
    CLHIP_UNIT_PRE_RES = 2,  /* `res` names a unit whose raw (pre-BatchNorm) sum is added to this conv's output BEFORE the BatchNorm  */
    CLHIP_UNIT_RAW_SRC = 4,  /* the conv reads the raw sum of activation `src` instead of its normalised output                       */
    CLHIP_UNIT_NO_BN = 8,    /* conv only (gamma/beta/rm/rv offsets ignored); the result is consumed through PRE_RES / RAW_SRC         */
    CLHIP_UNIT_MAXPOOL = 16  /* the ImageNet stem (resnet.py:136-149, 217-218): conv -> BN -> ReLU -> MaxPool2d(3, 2, 1).  Unit 0 only, src 0,
                                RELU set, no residual; activation 1 is the pooled map (z and the argmax map stay in the workspace).  This unit
                                may also be 7x7 / stride 2 / pad 3 (Cin <= 8); a 7x7 unit without this bit is refused.  Training needs the
                                accumulator path (the default).                                                                        */
};

typedef struct {
    int32_t cin, cout, ksize, stride, pad;
    int32_t src;      /* activation index consumed: 0 = network input, i+1 = output of unit i */
    int32_t res;      /* activation index added before the ReLU, or -1 */
    int32_t relu;     /* CLHIP_UNIT_* bits (1 = plain ReLU, 0 = none: the values older callers pass) */
    int64_t w_off;    /* element offsets into the flat fp32 parameter / gradient buffers */
    int64_t gamma_off;
    int64_t beta_off;
    int64_t rm_off;   /* element offsets into the flat fp32 BN-statistics buffer */
    int64_t rv_off;
} clhip_unit_desc;

typedef struct clhip_plan clhip_plan;

clhip_plan* clhip_plan_create(const clhip_unit_desc* units /*host*/, int n_units, int N, int H, int W, int Cin, int dtype);
/* pool_win > 0: nn.AvgPool2d(pool_win) + flatten of the NCHW result instead of the global pool (ResNet_BIC.forward, resnet.py:675-676;
 * feat_dim = C * (H/win) * (W/win)) */
clhip_plan* clhip_plan_create_ex(const clhip_unit_desc* units /*host*/, int n_units, int N, int H, int W, int Cin, int dtype, int pool_win);
void clhip_plan_destroy(clhip_plan*);
size_t clhip_plan_workspace_bytes(const clhip_plan*);      /* activations + saved tensors + grads + scratch */
size_t clhip_plan_shadow_bytes(const clhip_plan*);         /* `dtype` copies of the conv weights */
int clhip_plan_feat_dim(const clhip_plan*);
/* (round 6) Runs of BasicBlocks of the CIFAR ResNet-32s (core/model/backbone/resnet.py:289-316, 381-392) execute as ONE launch per direction in training mode
 * when the batch fits the device one image per compute unit (bf16 plans, N <= number of CUs; clhip_config("STAGE_TRAIN", "0") keeps one launch per unit).
 * Those launches need every workgroup resident at once, so: (1) a plan's training passes must not run on two streams concurrently, nor beside the training
 * passes of another plan of the same device on another stream (the library serialises stream switches outside a capture; inside a capture the caller must);
 * (2) several PROCESSES sharing one GPU must switch STAGE_TRAIN off.  Every in-launch wait is bounded: a violation ends in wrong results plus a sticky error
 * word, not a hung device.  clhip_plan_stage_status returns that word (0 = clean; synchronises the device -- call it at epoch / task boundaries).
 * The batch statistics of grids of 64+ workgroups are exchanged XCD-first (xch.h: plain stores inside an XCD's L2, the XCDs' partial sums across): that form is used
 * only on a device where a probe at plan creation found workgroup w on the XCD of workgroup w % 8 for every grid size it tries; clhip_config("STAGE_XCH3", "0")
 * keeps the two-hop form (another fixed summation order: the two forms agree to fp64 rounding, not bit for bit). */
int clhip_plan_stage_status(clhip_plan*);
/* what: 0 = units of the plan that run inside stage-level training launches, 1 / 2 = such forward / backward launches made so far (tests, diagnostics) */
long long clhip_plan_stage_info(const clhip_plan*, int what);
/* diagnostic (clhip_config("STAGE_TRACE", "<channels>:<convolution>")): 24 phase stamps (s_memtime ticks: shader cycles on this part) of workgroup 0's last traced forward [0..7] / backward [8..23] unit */
int clhip_plan_stage_trace(clhip_plan*, unsigned long long* out24);
/* refresh the `dtype` weight shadows from the fp32 masters (call after every optimizer step) */
int clhip_plan_prep_weights(clhip_plan*, const float* params, void* shadow, void* stream);
/* x: fp32 NCHW input; feat: fp32 [N, feat_dim].  training!=0: batch statistics, running stats updated,
 * activations saved in `workspace` for clhip_plan_backward.  training == 2: the same forward with the promise that NO backward (and no clhip_plan_read_act)
 * follows -- a frozen teacher that runs on batch statistics: the stage-level launches then skip the stores of z and of the activations inside a run
 * (same features, same statistics); launches that do not know the hint ignore it.                      */
int clhip_plan_forward(clhip_plan*, const float* x, const float* params, float* bn_stats, const void* shadow,
                       void* workspace, float* feat, int training, void* stream);
/* the same with nn.BatchNorm2d's `num_batches_tracked += 1` (torch/nn/modules/batchnorm.py, one int64 counter per unit, slot i = unit i;
 * nullable) folded into the forward's first launch when training != 0 -- no separate host-side add per step */
int clhip_plan_forward_ex(clhip_plan*, const float* x, const float* params, float* bn_stats, const void* shadow,
                          void* workspace, float* feat, int training, int64_t* num_batches_tracked, void* stream);
/* dfeat: fp32 [N, feat_dim]; grads: flat fp32 buffer laid out like params, accumulated into (+=).      */
int clhip_plan_backward(clhip_plan*, const float* dfeat, const float* params, const void* shadow, void* workspace,
                        float* grads, void* stream);
/* the same backward in pieces: units [unit_lo, unit_hi) in reverse order (unit_hi == number of units starts from dfeat).  Lets
 * the data-parallel host start the all-reduce of the deepest layers' gradients (the tail of the flat gradient buffer: the
 * parameters are laid out in unit order) while the backward of the shallower layers is still running. */
int clhip_plan_num_units(const clhip_plan* p);
/* tests: which branch of the executor's dispatch unit `unit` took in the plan's LAST forward (fwd_bits) and LAST backward (bwd_bits; units outside a
 * clhip_plan_backward_range keep their earlier word).  Host-side bookkeeping only: no device work, nothing launched differently.  Either pointer may be NULL. */
#define CLHIP_FORM_FWD_LAZY_INPUT 1u      /* the producer's BatchNorm + ReLU applied on this convolution's operand load */
#define CLHIP_FORM_FWD_LAZY_RES_INPUT 2u  /* ... of a block's last unit (+ residual), this launch writing the activation and its packed mask */
#define CLHIP_FORM_FWD_WRITE_THROUGH 4u   /* ... on the patch landed in LDS (BN_INPUT_WT) */
#define CLHIP_FORM_FWD_PAIR 8u            /* a down-sampling entry's two convolutions as one launch (on both units) */
#define CLHIP_FORM_FWD_EVAL_LAZY 16u      /* eval forward: the producer's running-statistics BatchNorm applied on the operand load */
#define CLHIP_FORM_BWD_BOTH 1u            /* dgrad and weight gradient as one launch */
#define CLHIP_FORM_BWD_BN_GRAD 2u         /* ... which also applies the unit's BatchNorm backward on its operand loads (dz never written) */
#define CLHIP_FORM_BWD_BN_GRAD_RES 4u     /* ... and writes the residual gradient from the packed mask */
#define CLHIP_FORM_BWD_LAZY_INPUT 8u      /* the weight gradient's operand rebuilt from the producer's z (lazy activation) */
#define CLHIP_FORM_BWD_EPILOGUE_SUMS 16u  /* the unit's BatchNorm-backward sums came from the launch that completed its dy (dgrad / pooling epilogue) */
#define CLHIP_FORM_BWD_PAIR_DGRAD 32u     /* a down-sampling entry's two input gradients as one launch (on both units) */
#define CLHIP_FORM_BWD_PAIR_BN_SUMS 64u   /* ... which also reduced the producer's BatchNorm-backward sums */
#define CLHIP_FORM_BWD_WGRAD_PAIR 128u    /* ... and their two weight gradients as one launch (on both units) */
#define CLHIP_FORM_BWD_SIDE_STREAM 256u   /* the weight gradient ran on the side stream */
#define CLHIP_FORM_BWD_BRANCH 512u        /* the whole unit ran on the branch stream */
#define CLHIP_FORM_BWD_EVENT_HOOK 1024u   /* the BatchNorm-backward launch completed the dz event itself */
#define CLHIP_FORM_BWD_POOL_FUSED 2048u   /* (last unit) the pooling's backward reduced its BatchNorm-backward sums */
int clhip_plan_unit_forms(const clhip_plan* p, int unit, unsigned* fwd_bits, unsigned* bwd_bits);
int clhip_plan_backward_range(clhip_plan* p, const float* dfeat, const float* params, const void* shadow, void* workspace,
                              float* grads, int unit_hi, int unit_lo, void* stream);
/* debugging / tests: copy activation `idx` (0=input) as fp32 NCHW; which: 0 = y, 1 = pre-BN z (idx>=1), 2 = dy,
 * 3 = the pre-pool z of the max-pool stem unit at its own size [N, C, Ho, Wo] (which = 1 is refused there: another shape than the activation).
 * Not every intermediate is written by the fast paths.  An activation whose BatchNorm the consumer applies on its operand load (training: the first convolution
 * of a block, also inside a stage-level run of stage_train.hip; eval: EVAL_LAZY) is REBUILT here from its z and coefficients by the apply launch the eager path
 * would have made -- which is why `workspace` is written to despite the const, and why the call must not be made between a forward and its backward on another
 * stream.  An activation INSIDE a run the eval forward executed as one launch (stage.hip) was never produced: CLHIP_EINVAL (clhip_config("STAGE_EVAL", "0") keeps
 * one launch per unit).  dy (which = 2) exists for the per-unit backward only: inside a stage-level training run the gradient of an activation never leaves LDS
 * (clhip_config("STAGE_TRAIN", "0") before the forward keeps the per-unit backward). */
int clhip_plan_read_act(clhip_plan*, const void* workspace, int idx, int which, float* out_nchw, void* stream);

/* A run of nconv / 2 BasicBlocks (conv3x3 C -> C, stride 1 -> BN -> ReLU -> conv3x3 -> BN -> + block input -> ReLU) in eval mode as ONE launch, the image
 * resident in LDS (csrc/stage.hip) -- what the eval forward of a bf16 plan makes of such a run (clhip_config("STAGE_EVAL", "0") keeps one launch per unit); the
 * direct entry reads no switch.  x, y: [N][H][W][C] bf16 (y may not alias x); w[i]: the [C][9][C] bf16 forward copy of convolution i exactly as
 * clhip_conv_weight_prep writes w_fwd; gamma / beta / mean / var[i]: its BatchNorm weight, bias and running statistics (fp32, C each); the five tables are host
 * arrays of nconv device pointers.  Every pre-BatchNorm value is rounded to bf16 as the per-unit path stores it.  Supported (the query returns 1, else 0): bf16,
 * (C, H = W) = (16, 32), (32, 16) or (64, 8), nconv even in 2 .. 16; the call also needs N >= 1.  Anything else is CLHIP_EINVAL before a launch. */
int clhip_stage_eval_supported(int H, int W, int C, int nconv, int dtype);
int clhip_stage_eval(const void* x, void* y, int N, int H, int W, int C, int nconv, const void* const* w, const float* const* gamma, const float* const* beta,
                     const float* const* mean, const float* const* var, float eps, int dtype, void* stream);

/* The same run in TRAINING mode as ONE launch per direction (csrc/stage_train.hip, csrc/xch.h): one workgroup per image, all of them resident at once, the batch
 * statistics of every BatchNorm through an in-launch all-reduce.  These are the launches a bf16 plan makes of such a run (see clhip_plan_stage_status above for the
 * rules a process must keep); the direct entries read no switch except STAGE_XCH3.  One entry per convolution in every table (host arrays of device pointers).
 *   forward   x [N][H][W][C] bf16; w[i] the [C][9][C] forward copy of clhip_conv_weight_prep; gamma / beta[i] fp32 [C]; rm / rv[i] the running statistics, updated
 *             in place (momentum, unbiased variance; factor 1 at N H W = 1); mean / invstd[i] [C] and coef[i] [2][C] (scale, shift) are written; z[i] [N][H][W][C]
 *             bf16 the pre-BatchNorm output (entry NULL: not stored -- a forward no backward follows); y[i] the activation behind convolution i (NULL: not stored;
 *             the launch itself needs none of them); mask[i] is accepted for the plan's sake and never written: the backward takes the ReLU mask of a block
 *             output from y > 0.  feat (nullable) [N][C] fp32: the global average of the run's output.
 *   backward  x as above, dy [N][H][W][C] bf16 the gradient of the run's output (not read when dfeat [N][C] is given: the gradient is then dfeat / (H W) at every
 *             pixel), dx the gradient of x (dx_accumulate: added to what dx holds); wd[i] the [C][9][C] dgrad copy (w_dg of clhip_conv_weight_prep); mean / invstd /
 *             z[i] as the forward left them, y[i] at the second convolution of every block (odd i), NULL elsewhere; dgamma / dbeta[i] are accumulated into;
 *             slab[i]: clhip_stage_train_query(SLAB_BLOCKS) blocks of C * 9 * C floats, one per image or per group of 16 images, which the caller sums in block
 *             order; dzg[i] [C / 16][N][H][W][16] bf16 scratch where the query reports the group form, NULL otherwise.
 *   entry != 0: the launch starts with the stage's down-sampling block: nconv odd, C >= 32, the tables hold nconv + 2 entries -- [0] its 3x3 / stride-2 convolution
 *             (w [C][9][C / 2], wd [C / 2][9][C], slab N blocks of C * 9 * C / 2), [1] its 1x1 / stride-2 shortcut (w [C][1][C / 2], wd [C / 2][1][C], slab N blocks of
 *             C * C / 2; y[1] may receive the shortcut's BatchNorm output), [2] its second convolution, [3 ...] the blocks behind it; x / dx are [N][2 H][2 W][C / 2].
 *   xch       clhip_stage_train_query(XCH_BYTES, N) bytes, zeroed ONCE by the caller and then reused by every launch at that N, whatever its direction or geometry.
 *             clhip_stage_train_status returns its sticky error word (0 = clean; synchronises the device).
 * Supported: bf16, (C, H = W) = (16, 32), (32, 16) or (64, 8), 1 <= N <= query(MAX_BATCH), nconv even in 2 .. 16 (entry: odd in 1 .. 15).  Anything else, or a NULL
 * xch, is CLHIP_EINVAL before a launch. */
#define CLHIP_STAGE_TRAIN_Q_MAX_BATCH 0   /* the largest N */
#define CLHIP_STAGE_TRAIN_Q_XCH_BYTES 1   /* bytes of the exchange buffer for N */
#define CLHIP_STAGE_TRAIN_Q_SLAB_BLOCKS 2 /* weight-gradient blocks per convolution that a backward of N images at C channels leaves */
#define CLHIP_STAGE_TRAIN_Q_GROUP 3       /* 1: that backward takes the group weight gradient (and needs dzg) */
#define CLHIP_STAGE_TRAIN_Q_FORM 4        /* the exchange of N workgroups at C channels under the current switches: 1 one hop, 2 two hops, 3 three levels (XCD-first) */
/* -1: unknown `what`, N < 1, or (SLAB_BLOCKS, GROUP, FORM) a C other than 16 / 32 / 64; XCH_BYTES answers for any N >= 1, also beyond MAX_BATCH.
 * The three-level form is taken only on a device whose XCD probe has RUN and found the rule to hold: clhip_plan_create runs it, and so does query(FORM) -- which
 * is why FORM must not be asked inside a stream capture.  The launches themselves never probe: a host that uses the direct entries without either call gets the
 * two-hop form wherever FORM would have said 3 (another fixed summation order, the same totals to fp64 rounding).  Ask FORM once before the first launch. */
long long clhip_stage_train_query(int what, int N, int C);
int clhip_stage_train_status(void* xch);
int clhip_stage_train_fwd(const void* x, int N, int H, int W, int C, int nconv, const void* const* w, const float* const* gamma, const float* const* beta,
                          float* const* rm, float* const* rv, float* const* mean, float* const* invstd, float* const* coef, void* const* z, void* const* y,
                          void* const* mask, float momentum, float eps, void* xch, int trace, int entry, float* feat, int dtype, void* stream);
int clhip_stage_train_bwd(const void* x, const void* dy, void* dx, int dx_accumulate, int N, int H, int W, int C, int nconv, const void* const* wd,
                          const float* const* gamma, const float* const* beta, const float* const* mean, const float* const* invstd, const void* const* z,
                          const void* const* y, float* const* dgamma, float* const* dbeta, float* const* slab, void* const* dzg, void* xch, int trace, int entry,
                          const float* dfeat, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Heads and losses (fp32).
 * linear: out[B,O] = x[B,D] W[O,D]^T + b   (nn.Linear heads: ewc.py:50, lwf.py:29-40, icarl.py:31)      */
int clhip_linear_fwd(const float* x, const float* w, const float* b /*nullable*/, float* out, int B, int D, int O, void* stream);
int clhip_linear_bwd(const float* x, const float* w, const float* dout, float* dx /*nullable*/, float* dw, float* db /*nullable*/,
                     int B, int D, int O, int accumulate, void* stream);
/* cross entropy over the column slice [lo,hi) with labels offset by lo (F.cross_entropy(logit[:, old:], y-old),
 * ewc.py:99, lwf.py:62, icarl.py:209) fused with argmax over [0,pred_hi) and the correct-count
 * (ewc.py:102-108).  loss_out[0] (+)= weight*mean CE ; dlogits[B,O] (+)= weight*dCE (zero outside the slice);
 * pred[B] int64 ; correct[0] int32.                                                                   */
int clhip_ce_slice(const float* logits, const int64_t* labels, int B, int O, int lo, int hi, int pred_hi, float weight,
                   float* loss_out, int loss_accumulate, float* dlogits /*nullable*/, int grad_accumulate,
                   int64_t* pred /*nullable*/, int32_t* correct /*nullable*/, void* stream);
/* same with the argmax restricted to [pred_lo, pred_hi): L2P's logits masked to -inf outside the current task's classes
 * (l2p.py:92-106) are CE over [lo,hi) and argmax over [lo,hi) */
int clhip_ce_window(const float* logits, const int64_t* labels, int B, int O, int lo, int hi, int pred_lo, int pred_hi, float weight,
                    float* loss_out, int loss_accumulate, float* dlogits /*nullable*/, int grad_accumulate,
                    int64_t* pred /*nullable*/, int32_t* correct /*nullable*/, void* stream);
/* distillation: -(softmax(soft/T) * log_softmax(pred/T)).sum()/B over the first k columns
 * (lwf.py:75-78, icarl.py:198-206); strides are the row pitches (O) of the two logit matrices.         */
int clhip_kd_loss(const float* pred, int pred_stride, const float* soft, int soft_stride, int B, int k, float T,
                  float weight, float* loss_out, int loss_accumulate, float* dpred /*nullable*/, int grad_accumulate,
                  void* stream);

/* LUCIR heads/losses (backbone/resnet.py:418-463, lucir.py:175-210) */
int clhip_cosine_linear_fwd(const float* x, const float* w, float* out, float* xnorm, float* wnorm, int B, int D, int O, void* stream);
int clhip_cosine_linear_bwd(const float* x, const float* w, const float* out, const float* xnorm, const float* wnorm,
                            const float* dout, float* dx, float* dw, int B, int D, int O, int accumulate, void* stream);
/* mean(1 - cos(a,b)) * weight ; da (+)= grad ; b is the detached teacher feature */
int clhip_cos_embed_loss(const float* a, const float* b, int B, int D, float weight, float* loss_out, int loss_accumulate,
                         float* da, int grad_accumulate, void* stream);
/* margin ranking on old-class samples: for rows with label < num_old, over the top-K novel scores:
 * mean(max(0, margin - (gt - novel))) * weight; scores[B,O] are the pre-sigma cosine scores.            */
int clhip_margin_rank_loss(const float* scores, const int64_t* labels, int B, int O, int num_old, int K, float margin,
                           float weight, float* loss_out, int loss_accumulate, float* dscores, int grad_accumulate,
                           int32_t* hard_count, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Flat-buffer (multi-tensor) elementwise family, fp32.
 * ewc_penalty: loss_out (+)= weight * sum_i F_i (p_i - ref_i)^2 / 2       (ewc.py:221-225)
 * ewc_grad   : g_i += weight * F_i (p_i - ref_i)                          (its autograd gradient)
 * fisher_accum: fisher_i += g_i^2 * scale                                 (ewc.py:171-174)
 * fisher_merge: new_i = alpha*old_i + (1-alpha)*new_i                     (ewc.py:128-131)
 * sgd_step : torch.optim.SGD semantics (trainer.py:159-166): d = g*grad_scale + wd*p [+ ewc term];
 *            m = momentum*m + d; p -= lr*m.  `mom` may be NULL when momentum == 0.
 * adam_step: torch.optim.Adam (no amsgrad); step = 1-based step count.
 * sq_norm  : out[0] (+)= sum g_i^2   (clip_grad_norm_, l2p.py:104); scale: g *= s                       */
int clhip_ewc_penalty(const float* p, const float* ref, const float* fisher, int64_t n, float weight, float* loss_out,
                      int loss_accumulate, void* stream);
/* dev_scale (nullable): device scalar multiplied into `weight` (the upstream autograd gradient, no host sync) */
int clhip_ewc_grad(const float* p, const float* ref, const float* fisher, float* g, int64_t n, float weight,
                   const float* dev_scale, void* stream);
/* the same over up to 4 (p, ref, fisher[, g]) segments in ONE launch (host arrays of device pointers / lengths): EWC's parameters are the backbone's
 * flat buffer plus the head's weight and bias prefixes (ewc.py:207-225 loops over named_parameters) */
int clhip_ewc_penalty_multi(int count, const float* const* p, const float* const* ref, const float* const* fisher, const int64_t* n, float weight,
                            float* loss_out, int loss_accumulate, void* stream);
int clhip_ewc_grad_multi(int count, const float* const* p, const float* const* ref, const float* const* fisher, float* const* g, const int64_t* n,
                         float weight, const float* dev_scale, void* stream);
int clhip_fisher_accum(float* fisher, const float* g, int64_t n, float scale, void* stream);
int clhip_fisher_merge(float* new_f, const float* old_f, int64_t n, float alpha, void* stream);
int clhip_sgd_step(float* p, const float* g, float* mom, int64_t n, float lr, float momentum, float weight_decay,
                   float grad_scale, const float* ewc_ref, const float* ewc_fisher, float ewc_weight, void* stream);
/* the same update (without the EWC term) over `count` <= 8 tensors in ONE launch: p[k], g[k], mom[k] (mom NULL when momentum == 0), n[k] elements each.
 * Element for element the arithmetic of clhip_sgd_step. */
int clhip_sgd_step_multi(int count, float* const* p, const float* const* g, float* const* mom /*nullable*/, const int64_t* n, float lr, float momentum,
                         float weight_decay, float grad_scale, void* stream);
/* ... and, for the tensors whose bit is set in zero_grad_mask, g <- 0 once it has been consumed: the flat gradient buffer of a backbone then
 * enters the next backward already zeroed (every writer of it accumulates) and the per-step 44.7-MB fill launch of ResNet-18 disappears
 * (trainer.train_steps opts in: between optimizer.step() and the next zero_grad() nothing reads the gradients there). */
int clhip_sgd_step_multi_zero(int count, float* const* p, float* const* g, float* const* mom /*nullable*/, const int64_t* n, float lr, float momentum,
                              float weight_decay, float grad_scale, unsigned zero_grad_mask, void* stream);
int clhip_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, float grad_scale, int step, void* stream);
int clhip_sq_norm(const float* g, int64_t n, float* out, int accumulate, void* stream);
int clhip_scale(float* g, int64_t n, float s, void* stream);
/* out_i = g_i * s * (*dev_scale)  (out may alias g); chains a precomputed loss gradient with the upstream grad */
int clhip_scale_dev(const float* g, float* out, int64_t n, float s, const float* dev_scale, void* stream);
/* LUCIR sigma: logits = sigma*scores ; backward: dscores = sigma*dlogits, dsigma (+)= sum dlogits*scores
 * (backbone/resnet.py:439-441, 459-463) */
int clhip_sigma_scale_fwd(const float* scores, const float* sigma_dev, float* logits, int64_t n, void* stream);
int clhip_sigma_scale_bwd(const float* scores, const float* sigma_dev, const float* dlogits, float* dscores, float* dsigma,
                          int dsigma_accumulate, int64_t n, void* stream);

/* iCaRL nearest-class-mean: dist[B,M] = sum_d (f[b,d]-means[m,d])^2 ; pred = argmin (icarl.py:122-152);
 * herding step: idx = argmin_i || mu - (S + f_i)/(k+1) ||_2 over rows with taken[i]==0
 * (buffer/linearherdingbuffer.py:140-161)                                                              */
/* out[r] = x[r] / ||x[r]||_2  (feats / feats.norm(dim=1), linearherdingbuffer.py:133, icarl.py:256) */
int clhip_l2_normalize_rows(const float* x, float* out, int R, int D, void* stream);
int clhip_ncm_classify(const float* feats, const float* means, int B, int M, int D, int64_t* pred, void* stream);
int clhip_herding_select(const float* feats /*[n,D], L2-normalised*/, int n, int D, int m, int32_t* chosen /*[m]*/,
                         float* ws /*[2*D + n]*/, void* stream);
/* the same for every class of a task in ONE launch (one block per class): class c = rows [offsets[c], offsets[c+1]) of feats (offsets: n_classes + 1
 * int32 on the device, max_rows = the largest class), picks are class-local indices in chosen[c * m ...] (-1 beyond a class's row count);
 * ws: 2 * D * n_classes + offsets[n_classes] floats.  Same arithmetic, same picks as n_classes calls of clhip_herding_select. */
int clhip_herding_select_batched(const float* feats, const int32_t* offsets, int n_classes, int max_rows, int D, int m, int32_t* chosen, float* ws,
                                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * ViT path: frozen ViT-B/16 backbone with L2P prompt tokens or InfLoRA's
 * LoRA branch.  Token activations are [B*N, D] row-major in the compute dtype (batch-first: the reference's
 * seq-first [N,B,D] layout and its two permutes per block, transformer.py:1322-1329, do not exist here).
 *
 * clhip_gemm_nt: C[M,N] = epi(A[M,K] . B[N,K]^T); replaces every F.linear on the path (transformer.py:172,194,
 *   255,1267-1271) and, with the [in,out] copy of a frozen weight as B, its input gradient.  Epilogues:
 *   0 none | 1 +bias | 2 +bias +R (residual add, :1333-1334) | 3 +bias, then C <- GELU(.) (:1268) and H <- GELU'(.)
 *   (nullable; saved for the backward) | 4 C <- (.) * H (backward of 3 and 6) | 6 +bias, then CLIP's QuickGELU (transformer.py:137-139): with
 *   s = sigmoid(1.702 x), C <- x s and H <- s (1 + 1.702 x (1 - s)) (nullable; C has the same bits with and without H); one exp of -|1.702 x| gives s
 *   and 1 - s, so no |x| overflows or forms 0 * inf.  (5 is not an epilogue: it stays CLHIP_EINVAL.)  bias fp32; R, H in the compute dtype.
 *   K % 64 == 0, N % 4 == 0, lda and ldb % 8 == 0.  Output-side pitches (ldc; ldr when R is given; ldh when H is given): % 4 == 0, and % 8 == 0 for a
 *   bf16 product with N % 8 == 0 -- its kernels move C, R and H as 16-byte chunks at row * ld + 8 c, so every row must start 16-byte aligned (bf16 with
 *   N % 8 == 4 stores 8 bytes at a time and fp32 rows of ld % 4 == 0 are 16-byte aligned: both keep % 4).  Anything else is CLHIP_EINVAL before a launch.
 *   Products with fewer than 256 tiles of 128 x 128 and K >= 3072 (bf16) run as 2-4 K slices + one fixed-order
 *   reduce / epilogue pass through a library-owned fp32 scratch (per stream, allocated at the first such call outside stream capture, never
 *   freed while a graph may hold it); results are bitwise reproducible either way.                                                          */
int clhip_gemm_nt(const void* A, const void* B, void* C, const float* bias, const void* R, void* H, int M, int N, int K,
                  int lda, int ldb, int ldc, int ldr, int ldh, int epilogue, int dtype, void* stream);
/* The launches clhip_gemm_nt would make for this call, in order (host code only, no device needed): launches[4 i .. 4 i + 3] = kernel family
 * (below), first row, row count, K slices (> 1: split-K, the 128 x 128 tile per slice + the reduce / epilogue pass) for i < min(return value,
 * max_launches).  Returns the number of launches (at most 3: gemm8 rows, one 256 x 256 head, the small-tile rest) or CLHIP_EINVAL for a shape or
 * pitch clhip_gemm_nt rejects (the same check; ldr and ldh are judged as in a call that gives R and H, so pass 0 or N for an absent one).  clhip_gemm_nt switches on the same decision; the current clhip_gemm8_config mode and CLHIP_GEMM_* switches apply.  A split-K
 * launch is the intent: a call that finds no scratch (stream capture) runs those rows unsplit. */
#define CLHIP_GEMM_GEMM8 1    /* gemm8.hip, 256 x 256 persistent */
#define CLHIP_GEMM_256 2      /* register-staged 256 x 256, 8 waves */
#define CLHIP_GEMM_160 3      /* 160 x 128 */
#define CLHIP_GEMM_128 4      /* 128 x 128 */
#define CLHIP_GEMM_64 5       /* 64 x 64 */
#define CLHIP_GEMM_F32_128 6  /* fp32 parity mode, 128 x 128 */
int clhip_gemm_nt_route(int M, int N, int K, int lda, int ldb, int ldc, int ldr, int ldh, int dtype, int* launches, int max_launches);
/* The input gradient AND the weight gradient of one layer in ONE launch (both consume dz and nothing of each other): the layers whose two
 * backward convolutions are launches at their latency floor -- 3x3/s1/p1 with 16 -> 16 channels on 32-wide or 32 -> 32 channels on 16-wide
 * images, bf16 (CifarResNet-32 stages 1 and 2, core/model/backbone/resnet.py:289-316 under autograd).  Same arguments and results (bit for
 * bit) as clhip_conv_dgrad [or clhip_conv_dgrad_bn_reduce when z_prod != NULL: then y_prod (nullable), mean, invstd, acc, replicas as there]
 * followed by clhip_conv_wgrad with scratch `ws` (clhip_conv_wgrad_ws_bytes; required: the weight gradient is the deterministic form). */
int clhip_conv_dgrad_wgrad_supported(int N, int H, int W, int C, int Creal, int K, int ksize, int stride, int pad, int dtype);
int clhip_conv_dgrad_wgrad(const void* x, const void* dz, const void* w_dg, void* dx, int accumulate, float* dw, void* ws,
                           const void* z_prod, const void* y_prod, const float* mean, const float* invstd, double* acc, int replicas,
                           int N, int H, int W, int C, int Creal, int K, int ksize, int stride, int pad, int dtype, void* stream);

/* "Lazy" BatchNorm input (core/model/backbone/resnet.py:289-316: conv -> bn -> relu -> conv inside a basic block).  The consumer
 * convolution reads its producer's PRE-BatchNorm output z' and applies relu(scale * z' + shift) while it stages the operand: the
 * producer's BatchNorm-apply launch and its activation tensor do not exist (the values are bit for bit the ones clhip_bn_apply_train would
 * have stored).  Every workgroup derives scale / shift from the producer's statistics accumulators as clhip_bn_apply_train does;
 * the launch also leaves `mean`, `invstd` (for clhip_bn_bwd_*) and `coef` = [2][C] scale, shift, and updates the running statistics.
 * Served by the kernels that stage their operand through registers: 3x3/s1/p1 with 16 -> 16 or 32 -> 32 channels, bf16 (CifarResNet-32
 * stages 1 and 2).  The backward of that consumer takes the same tensor and `coef`: clhip_conv_dgrad_wgrad_bn_input = clhip_conv_dgrad_wgrad
 * with x = relu(coef[0] * x_z + coef[1]) and, when acc != NULL, the producer's BatchNorm-backward sums reduced in the dgrad epilogue
 * with its ReLU mask taken from x_z (z_prod == x_z). */
typedef struct clhip_bn_input {
    const double* stat_acc; int replicas;     /* the producer's [replicas][2][C] fp64 sums (clhip_conv_fwd_acc); NULL = the producer's BatchNorm is in EVAL mode:
                                                 scale / shift come from running_mean / running_var (required, read only), mean / invstd / coef are not written
                                                 (nullable), and the launch takes stat_acc == NULL for its own output too (no statistics in eval mode) */
    const float* gamma; const float* beta;
    float* running_mean; float* running_var;  /* nullable pair */
    float momentum, eps;
    float* mean; float* invstd;               /* out [C] */
    float* coef;                              /* out [2][C] */
} clhip_bn_input;
/* The same in the backward for the layer's OWN BatchNorm: clhip_conv_dgrad_wgrad_bn_grad = clhip_bn_bwd_apply_acc (ReLU mask from z, no residual)
 * followed by clhip_conv_dgrad_wgrad, with the BatchNorm-backward result dz = scale * (g - mean(g) - xhat * mean(g xhat)) computed from dy and
 * z on both bodies' operand loads instead of being written and re-read; `sums` are the [replicas][2][C] accumulators a consumer's dgrad
 * epilogue filled (clhip_conv_dgrad_bn_reduce / clhip_conv_dgrad_wgrad*), one workgroup adds them to dgamma / dbeta.  Same domain. */
typedef struct clhip_bn_grad {
    const void* dy; const void* z;            /* [N,H,W,K] gradient of the layer's activation, its pre-BatchNorm output */
    const double* sums; int replicas;
    const float* mean; const float* invstd; const float* gamma; const float* beta;
    float* dgamma; float* dbeta;              /* accumulated into */
    const void* relu_mask;                    /* NULL: ReLU straight after the BatchNorm, mask from z; else the packed mask of a conv -> BN -> +res -> ReLU layer
                                                 (clhip_bn_apply_train_mask) and ... */
    void* dres; int dres_accumulate;          /* ... its residual gradient g = dy * mask, written / accumulated by the launch (NULL: none) */
} clhip_bn_grad;
int clhip_conv_dgrad_wgrad_bn_grad(const void* x, const float* x_coef /*nullable: x is a lazy BatchNorm input, z_prod == x, y_prod unused*/,
                                   const clhip_bn_grad* bn /*host*/, const void* w_dg, void* dx, int accumulate, float* dw, void* ws,
                                   const void* z_prod, const void* y_prod, const float* mean, const float* invstd, double* acc, int replicas, int N,
                                   int H, int W, int C, int Creal, int K, int ksize, int stride, int pad, int dtype, void* stream);
int clhip_conv_bn_input_supported(int N, int H, int W, int C, int K, int ksize, int stride, int pad, int dtype);
int clhip_conv_fwd_acc_bn_input(const void* z_in, const clhip_bn_input* bn /*host*/, const void* w_fwd, void* z, double* stat_acc, int replicas,
                                int N, int H, int W, int C, int K, int ksize, int stride, int pad, int dtype, void* stream);
/* The same when the producer is a conv -> BN -> +res -> ReLU layer (the last unit of a basic block, resnet.py:312-316): the operand is
 * relu(scale * z_in + shift + res), and because that activation has later readers (the next block's residual add, the backward) the
 * launch also WRITES it and its packed ReLU mask -- each pixel by the workgroup that owns it -- exactly as clhip_bn_apply_train_mask would
 * have: the apply launch disappears, the convolution's read of the activation becomes the read of z_in and res.  Same domain. */
typedef struct clhip_bn_res_input {
    const void* res;                          /* [N,H,W,C] the residual */
    void* y;                                  /* out [N,H,W,C] relu(bn(z_in) + res) */
    void* relu_mask;                          /* out [N*H*W*C/8] bytes, bit e = (stored element e > 0); nullable when the producer is in eval mode (bn->stat_acc == NULL) */
} clhip_bn_res_input;
int clhip_conv_fwd_acc_bn_res_input(const void* z_in, const clhip_bn_input* bn /*host*/, const clhip_bn_res_input* rs /*host*/, const void* w_fwd, void* z,
                                    double* stat_acc, int replicas, int N, int H, int W, int C, int K, int ksize, int stride, int pad, int dtype,
                                    void* stream);
/* The write-through form for the LDS-DMA kernels of the wide layers (64 ... 512 channels, 3x3 / stride 1: ResNet-18's BasicBlocks,
 * resnet.py:289-316; conv4.hip / conv5.hip): LDS-DMA has no arithmetic on the way, so the patch lands RAW (z_in) and the wave that issued a
 * DMA piece rewrites its slots in LDS with relu(scale * z_in + shift [+ res]) before the patch is published; the workgroup that owns a pixel
 * writes rs->y (always: the consumer's weight gradient reads it) and, for a conv -> BN -> +res -> ReLU producer, rs->relu_mask.
 * rs->res / rs->relu_mask NULL: plain relu(bn(z_in)).  Values bit for bit those of clhip_bn_apply_train[_mask]; bf16 only. */
int clhip_conv_bn_input_wt_supported(int N, int H, int W, int C, int K, int ksize, int stride, int pad, int dtype);
int clhip_conv_fwd_acc_bn_input_wt(const void* z_in, const clhip_bn_input* bn /*host*/, const clhip_bn_res_input* rs /*host*/, const void* w_fwd, void* z,
                                   double* stat_acc, int replicas, int N, int H, int W, int C, int K, int ksize, int stride, int pad, int dtype,
                                   void* stream);
/* Which kernel a convolution call would run (host code only: no device, no pointers).  op: 0 clhip_conv_fwd / _acc, 1 clhip_conv_dgrad, 2 clhip_conv_wgrad,
 * 3 clhip_conv_dgrad_bn_reduce[_ex], 4 clhip_conv_fwd_acc_bn_input_wt.  form: forward 0 no statistics, 1 partial rows (stat_partials), 2 fp64 accumulators
 * (_acc); wgrad 0 ws == NULL, 1 scratch given; otherwise 0.  Returns one kernel family below (> 0), or CLHIP_EINVAL with clhip_last_error set where the call
 * would refuse these shapes (the same check; pointer arguments are the call's own business).  The five entry points switch on this function's result; the
 * current clhip_config switches apply (most are cached at their first use). */
#define CLHIP_CONV_STEM7 1         /* stem7.hip forward (7x7 / s2 / p3) */
#define CLHIP_CONV_STEM 2          /* stem.hip forward (3x3, 8 padded input channels) */
#define CLHIP_CONV_CONV64 3        /* conv3.hip conv64_kernel */
#define CLHIP_CONV_CONV16 4        /* conv3.hip conv16_kernel / conv32_kernel */
#define CLHIP_CONV_CONV8 5         /* conv8.hip */
#define CLHIP_CONV_CONV5 6         /* conv5.hip */
#define CLHIP_CONV_CONV9 7         /* conv9.hip */
#define CLHIP_CONV_CONV4 8         /* conv4.hip */
#define CLHIP_CONV_CONV3 9         /* conv3.hip conv3_kernel / conv3g_kernel */
#define CLHIP_CONV_CONV2 10        /* conv2.hip conv_igemm2_kernel (the generic kernel) */
#define CLHIP_CONV_V1 11           /* conv.hip conv_igemm_kernel (CONV_V1) */
#define CLHIP_CONV_SHORTCUT 12     /* shortcut.hip (dgrad of the 1x1 / s2 shortcut) */
#define CLHIP_CONV_WGRAD_STEM7 13  /* stem7.hip weight gradient */
#define CLHIP_CONV_WGRAD_STEM 14   /* stem.hip weight gradient */
#define CLHIP_CONV_WGRAD64 15      /* conv3.hip wgrad64_kernel */
#define CLHIP_CONV_WGRAD4 16       /* wgrad4.hip */
#define CLHIP_CONV_WGRAD3 17       /* conv3.hip conv_wgrad3_kernel */
#define CLHIP_CONV_WGRAD16 18      /* conv3.hip wgrad16_kernel */
#define CLHIP_CONV_WGRAD32 19      /* conv3.hip wgrad32_kernel */
#define CLHIP_CONV_WGRAD2_DET 20   /* conv2.hip conv_wgrad2_kernel, partial blocks + fixed-order reduce */
#define CLHIP_CONV_WGRAD2_ATOMIC 21 /* conv2.hip conv_wgrad2_kernel, fp32 atomics */
#define CLHIP_CONV_WGRAD_V1 22     /* conv.hip conv_wgrad_kernel (CONV_V1), LDS transpose read in bf16 */
#define CLHIP_CONV_WGRAD_V1_NO_TR 23 /* conv.hip conv_wgrad_kernel without the transpose read (WGRAD_NO_TR; fp32 always) */
int clhip_conv_route(int op, int form, int N, int H, int W, int C, int Creal, int K, int ksize, int stride, int pad, int dtype);
/* Number of launches, in this process, of the entry-block body of conv2.hip (the 3x3/s2 forwards behind ENTRY_S2).  The body stores the generic kernel's
 * bits, so its outputs cannot tell which kernel ran: tests and A/B runs read this counter instead. */
long long clhip_conv_entry_s2_launches(void);
int clhip_conv_dgrad_wgrad_bn_input(const void* x_z, const float* x_coef, const void* dz, const void* w_dg, void* dx, int accumulate, float* dw,
                                    void* ws, const float* mean, const float* invstd, double* acc /*nullable*/, int replicas, int N, int H, int W,
                                    int C, int Creal, int K, int ksize, int stride, int pad, int dtype, void* stream);

/* The input gradient of a DOWN-SAMPLING block entry in one launch (core/model/backbone/resnet.py:226-234: `conv1` 3x3/s2/p1 and
 * `downsample[0]` 1x1/s2/p0 both read the block input x [N,H,W,C]):  dx (+)= dgrad3x3s2(dz, W) + dgrad1x1s2(dz_sc, W_sc).
 * dz, dz_sc [N,H/2,W/2,K]; dz_sc NULL: the 3x3 convolution alone.  The weights come as ONE packed buffer of
 * clhip_conv_dgrad_pair_packed_bytes(C, K) bytes made by clhip_conv_dgrad_pair_pack from the dgrad copies w_dg [C][9][K] and
 * w_sc_dg [C][1][K] (nullable) of clhip_conv_weight_prep -- per (64-channel tile, 16-wide K chunk) the LDS image of that chunk's ten
 * taps (csrc/conv6.hip); a plan writes this layout in its own weight preparation.  Same result as clhip_conv_dgrad of the shortcut
 * followed by clhip_conv_dgrad(accumulate) of the 3x3 layer up to the bf16 rounding of the intermediate (here the two are summed
 * in fp32).  bf16, C % 64 == 0, K % 32 == 0, H/2 and W/2 powers of two, W/2 <= 16 (ResNet-18's three entries; csrc/conv6.hip), or
 * C in {16, 32} with K = 2 C (CifarResNet-32's two; csrc/conv7.hip, packed [C][10][K]).  _supported: 1 / 0. */
int clhip_conv_dgrad_pair_supported(int N, int H, int W, int C, int K, int dtype);
size_t clhip_conv_dgrad_pair_packed_bytes(int C, int K);
int clhip_conv_dgrad_pair_pack(const void* w_dg, const void* w_sc_dg /*nullable*/, void* packed, int C, int K, int dtype, void* stream);
int clhip_conv_dgrad_pair(const void* dz, const void* w_packed, const void* dz_sc /*nullable*/, void* dx, int accumulate, int N, int H,
                          int W, int C, int K, int dtype, void* stream);

/* clhip_conv_dgrad_pair whose epilogue also reduces the BatchNorm backward of the layer that PRODUCED the block input (z_prod, y_prod, mean, invstd,
 * acc, replicas exactly as clhip_conv_dgrad_bn_reduce; valid when this launch completes dx, i.e. the two layers are the activation's only readers).
 * The small-channel entries (C in {16, 32}, K = 2 C).  _supported: 1 / 0. */
int clhip_conv_dgrad_pair_bn_reduce_supported(int N, int H, int W, int C, int K, int dtype);
int clhip_conv_dgrad_pair_bn_reduce(const void* dz, const void* w_packed, const void* dz_sc /*nullable*/, void* dx, int accumulate, const void* z_prod,
                                    const void* y_prod /*nullable*/, const float* mean, const float* invstd, double* acc, int replicas, int N, int H,
                                    int W, int C, int K, int dtype, void* stream);
/* The WEIGHT gradients of the same two layers in one launch (csrc/conv7.hip): dw [K][9][C] += the 3x3/s2 layer's, dw_sc [K][1][C] += the
 * shortcut's, both over the block input x [N,H,W,C]; dz, dz_sc [N,H/2,W/2,K].  ws / ws_sc: scratch of clhip_conv_wgrad_ws_bytes() bytes of
 * the 3x3 / the 1x1 layer (partial blocks per image group, summed in a fixed order: bitwise reproducible).  bf16; CifarResNet-32's two
 * entries (32 x 32 x 16 -> 32 channels, 16 x 16 x 32 -> 64).  _supported: 1 / 0. */
int clhip_conv_wgrad_pair_supported(int N, int H, int W, int C, int K, int dtype);
/* ... and their two FORWARD convolutions in one launch: z [N,H/2,W/2,K] = conv3x3/s2/p1(x, w_fwd [K][9][C]), z_sc = conv1x1/s2(x, w_sc_fwd [K][1][C]),
 * each with its BatchNorm statistics added into its own fp64 accumulators exactly as clhip_conv_fwd_acc does.  Same domain as the small-channel
 * clhip_conv_dgrad_pair (C in {16, 32}, K = 2 C). */
int clhip_conv_fwd_acc_pair_supported(int N, int H, int W, int C, int K, int dtype);
int clhip_conv_fwd_acc_pair(const void* x, const void* w_fwd, const void* w_sc_fwd, void* z, void* z_sc, double* stat_acc, int replicas,
                            double* stat_acc_sc, int replicas_sc, int N, int H, int W, int C, int K, int dtype, void* stream);
int clhip_conv_wgrad_pair(const void* x, const void* dz, const void* dz_sc, float* dw, float* dw_sc, void* ws, void* ws_sc, int N, int H, int W,
                          int C, int K, int dtype, void* stream);

/* ---- run-time configuration ------------------------------------------------------------------------------------------------
 * ONE entry point for every dispatch switch, tuning value and micro-benchmark hook of the library (there are no other steering
 * exports).  `key` is a name from the list below (a leading "CLHIP_" is accepted), `value` its new value as text; value == NULL
 * returns the switch to its default, which is the environment variable CLHIP_<key> if that is set and the built-in default
 * otherwise.  Unknown keys fail with CLHIP_EINVAL.  Most switches are read once, at the first launch or plan creation that
 * consults them: configure before that.  The product never needs a call: the defaults ARE the product; tests use the switches to
 * pin a code path, tools/ to sweep.
 *   dispatch (0 / 1 unless noted):
 *     CONV4 (0: 3x3/s1 layers stay on conv3.hip), CONV5 (0: the 64 -> 64-channel 3x3/s1 layers stay on conv4.hip), CONV64 (0: 64 -> 64 channels on small maps stay on conv4 / wgrad4; CONV64_FWD 0: only their backward; CONV64_BM 64 | 128), CONV6 (0: no fused stride-2 dgrad pair kernel), CONV6_PAIR (0: plans keep the two separate input-gradient launches), CONV7 (0: no small-channel entry kernels; FWD7 0 / WGRAD7 0: not their forward / weight-gradient pairs; CONV7_TPW n: tiles per wave), BN_INPUT (0: no lazy BatchNorm inputs), BN_INPUT_WT (0: not on the LDS-DMA kernels of the wide layers), BN_RES_INPUT (0: block outputs keep their own apply launch), EVAL_LAZY (0: eval-mode forwards keep one BatchNorm apply launch per unit instead of the consumer-side forms), BN_GRAD (0: no BatchNorm backward on the operand loads; BN_GRAD_MINC n: only for layers of >= n channels, BN_GRAD_RES 0: not for the +res layers), CONV_V1,
 *     ENTRY_S2 (0: the 3x3/s2 entry forwards of 64 / 128 / 256 -> twice as many channels stay on the generic kernel of conv2.hip; read on every call),
 *     NO_CONV3, NO_CONV16, NO_STEM, NO_SHORTCUT, NO_PARITY_DGRAD, CONV3G, WGRAD4 (0 off, 2 stride-1 layers only), WGRAD5, WGRAD32,
 *     WGRAD_NO_TR, WGRAD2_ATOMIC (1: the generic weight-gradient kernel keeps fp32 atomics even when scratch is handed in), BWD_FUSED (0: dgrad and weight gradient of the 16 / 32-channel layers as two launches), WGRAD_DEFER_SIDE (n > 0: plans WITH a weight-gradient stream reduce in groups of n launches), WGRAD_DEFER (0: plans without a weight-gradient stream reduce their partial blocks per layer instead of once per backward), GEMM_NO_SPLIT, GEMM_TAIL, GEMM_SPLITK (0: no split-K for the few-tile / long-K products; n > 1: the minimum K that splits, default 3072), ATTN_GENERIC, CE_ROWS,
 *     BN_PARTIALS (partial rows + finalize launches instead of the fp64 accumulators), BN_FUSE (0 never, 1 everywhere; default: small
 *     activations), BN_FUSE_MAX_M, BN_MASK_BITS, BN_MASK_FROM_Y, BN_ONEPASS, PREP_NARROW,
 *     WGRAD_STREAM (0: weight gradients on the caller's stream), BRANCH_STREAM (shortcut branches on a third stream: 0 never, 1 forward and backward, 2 forward only = default, 3 backward only), WGRAD_ALWAYS_QUEUE, SIDE_PRIO, EVENT_FLAGS, EVENT_RECORD
 *     round 5: CONV8 (0: the 64 -> 64-channel 3x3/s1 layers with >= CONV8_MIN_TILES [1024] tiles of 128 pixels stay on conv5.hip), CONV8_BNR (1: conv8's dgrad epilogue
 *     reduces the producer's BatchNorm backward -- measured slower, off), CONV9 (1: 128 / 256-channel 3x3/s1 layers on conv9.hip -- equal in the step, off),
 *     STREAM_PROBE (0: the executors' extra stream is the first one created, not the first one MEASURED to run beside the caller's stream)
 *   tuning values:
 *     DZ_BUFFERS (2..4 rotating gradient buffers of the two-stream backward, default 4), CONV8_GRID, CONV8_OPT, CONV64_MAX_W, CONV64_MAX_M,
 *     WGRAD_TARGET (workgroups of the weight-gradient kernels), WGRAD_NET_GFLOP, WGRAD4_MIN_STEPS, WGRAD4_MIN_TOTAL, CONV3_CFG "wm,wn",
 *     CONV4_CFG "wm,wn,kg,ck", CONV4_GRID, CONV5_MIN_TILES, CONV5_GRID, PLAN_SKIP (timing ablations: 1 no forward BatchNorm apply, 2 no BatchNorm backward, 4 no weight gradients -- results invalid), IGEMM_TILE "bm,bn", GEMM_MT, GEMM_GROUP_M, STEM_GRID,
 *     STEM_WGRAD_GRID, SHORTCUT_MIN_PIXELS, BN_ACC_CPT, BN_BWD_ITERS
 *   micro-benchmark / ablation hooks (tools/ubench; take effect at once): CONV4_FORCE_CFG "wm,wn,kg,ck", CONV4_ENABLE, CONV4_DEBUG, CONV6_DEBUG (read once),
 *     CONV3_DEBUG, WGRAD_DEBUG (bit masks of phases to skip), CONV4_TRACE, WGRAD4_TRACE, CONV8_TRACE, CONV9_TRACE (device address of
 *     a stamp buffer as a number; ablation builds only) */
int clhip_config(const char* key, const char* value);
/* the value clhip_config() last set for `key` (NULL: never set or erased -- the environment's value applies).  For callers that flip a
 * switch around a region and must put back what was there (ops.TeacherPass).  The pointer stays valid for the process' life. */
const char* clhip_config_get(const char* key);
/* the 256 x 256 eight-phase kernel with 64-deep K tiles (gemm8.hip, round 5; bf16, N % 256 == 0, K % 128 == 0, K >= 256): 0 never, 1 (the default) the
 * row panels that fill whole rounds of its 256 persistent workgroups -- the remaining rows go to the register-staged kernel --, 2 wherever it is
 * supported (tests); -1 = from $CLHIP_GEMM8.  Same epilogues as clhip_gemm_nt's other kernels
 * (core/model/backbone/transformer.py:172, 194, 1259-1271). */
void clhip_gemm8_config(int mode);
/* workgroups the LDS-DMA weight-gradient kernel (wgrad4.hip) aims for: 0 = the default (160 -- 128 until round 4 --, chosen for the training step, where the
 * launch shares the chip with the dgrad / BatchNorm chain of the caller's stream; $CLHIP_WGRAD_TARGET), 256 = one per CU (the kernel
 * alone: bench.py's `full_chip` figures).  The scratch size (clhip_conv_wgrad_ws_bytes) follows the setting. */
void clhip_wgrad4_config(int target_workgroups);
/* softmax(q k^T / sqrt(d)) v per (batch, head) on the packed qkv [B*N, 3D] (column = which*D + head*d + i), out [B*N, D],
 * lse [B,H,N] (nullable in forward-only use); MultiHeadAttention.forward, transformer.py:169-197.  N <= 256, d <= 64. */
int clhip_attn_fwd(const void* qkv, void* out, float* lse, int B, int N, int H, int D, int dtype, void* stream);
/* dqkv [B*N, 3D] from dout [B*N, D]; dsum_ws: [B,H,N] floats (only used by the generic fp32 path) */
int clhip_attn_bwd(const void* qkv, const void* out, const float* lse, const void* dout, void* dqkv, float* dsum_ws, int B, int N,
                   int H, int D, int dtype, void* stream);
/* Prefix-tuning attention: MultiHeadAttention.forward with `prompt` given (transformer.py:175-180: k = cat(pk, k), v = cat(pv, v) per sample and head).
 * qkv, out, lse, dout, dqkv exactly as in clhip_attn_fwd / _bwd; pk, pv [B, Lp, D] in the compute dtype (column = head*d + i): per-sample key and value
 * rows that have no query.  Per (batch, head) the N token queries attend over the Lp + N keys [prefix | tokens].  dpk, dpv [B, Lp, D] fp32 are WRITTEN
 * (not accumulated); deterministic, no atomics.  1 <= Lp, N + Lp <= 256, d <= 64; anything else is CLHIP_EINVAL.  csrc/attn.hip (the prefix
 * instantiation of the kernels behind clhip_attn_fwd / _bwd). */
int clhip_attn_prefix_fwd(const void* qkv, const void* pk, const void* pv, void* out, float* lse, int B, int N, int Lp, int H, int D, int dtype, void* stream);
int clhip_attn_prefix_bwd(const void* qkv, const void* pk, const void* pv, const void* out, const float* lse, const void* dout, void* dqkv, float* dpk,
                          float* dpv, float* dsum_ws, int B, int N, int Lp, int H, int D, int dtype, void* stream);
/* CODA-Prompt's prompt assembly, CodaPrompt.forward (prompt.py:158-220) for `layers` prompted layers in one launch, exact fp32.  K, A, P, ek, ev, dpk, dpv,
 * dK, dA, dP: HOST arrays of `layers` device pointers.  Per layer K, A [pool, D], P [pool, L, D] (fp32 masters), q [B, D] fp32 (shared by the layers).
 * fwd: c[l,b,k] = <q_b * A_k, K_k> / (max(|q_b * A_k|, 1e-12) max(|K_k|, 1e-12)) for k < f (prompt.py:190-194), kept as c [layers, B, f] fp32;
 *      P_[b] = sum_{k<f} c[b,k] P[k] (prompt.py:196); rows [0, L/2) -> ek [B, L/2, D], rows [L/2, L) -> ev (prompt.py:199-201), compute dtype:
 *      the pk / pv of clhip_attn_prefix_fwd.
 * bwd: from dpk, dpv [B, L/2, D] fp32 writes rows [s, f) of dK, dA [pool, D] and dP [pool, L, D] (the components the running task trains,
 *      prompt.py:174-182) and nothing outside them; q gets no gradient; the batch is summed in order (bit-reproducible).  ws: clhip_coda_ws_bytes.
 * D % 64 == 0, L even, 1 <= f <= pool, 0 <= s < f. */
size_t clhip_coda_ws_bytes(int layers, int B, int s, int f);
int clhip_coda_fwd(int layers, const float* q, const float* const* K, const float* const* A, const float* const* P, void* const* ek, void* const* ev, float* c,
                   int B, int D, int pool, int L, int f, int dtype, void* stream);
int clhip_coda_bwd(int layers, const float* q, const float* const* K, const float* const* A, const float* const* P, const float* c, const float* const* dpk,
                   const float* const* dpv, float* const* dK, float* const* dA, float* const* dP, float* ws, int B, int D, int pool, int L, int s, int f,
                   void* stream);
/* DualPrompt's prompt selection, DualPrompt.forward (prompt.py:269-337) for n_g G-layers and n_e E-layers in one launch, exact fp32.  g_p, e_k, e_p, dg_p,
 * de_k, de_p: HOST arrays of n_g / n_e device pointers; pk, pv, dpk, dpv: HOST arrays of n_g + n_e device pointers, the G-layers first.  Per G-layer
 * g_p [Lg, D]; per E-layer e_k [pool, D], e_p [pool, Le, D] (fp32 masters); q [B, D] fp32 (shared by the layers).
 * fwd: G-layer (prompt.py:310-316): pk[b] = g_p[:Lg/2], pv[b] = g_p[Lg/2:] for every sample.
 *      E-layer: cos[l,b,k] = <q_b, K_k> / (max(|q_b|, 1e-12) max(|K_k|, 1e-12)) for all k < pool (prompt.py:279-281), kept as cos [n_e, B, pool] fp32;
 *      idx[l,b] (int32, [n_e, B]) = task_id when `train` (prompt.py:285-287), else the arg-max of cos[l,b,:], an exact tie going to the lowest index
 *      (prompt.py:294-296, top-1); pk[b] = e_p[idx][:Le/2], pv[b] = e_p[idx][Le/2:] (prompt.py:299-306).  pk, pv [B, L/2, D] in the compute dtype: the
 *      pk / pv of clhip_attn_prefix_fwd; a copy (bf16: one rounding).
 *      train: loss[0] = sum over the E-layers in order of sum_b (1 - cos[l,b,task_id]), b in order (prompt.py:286, transformer.py:2279); eval: not written.
 * bwd: from dpk, dpv [B, L/2, D] fp32 writes dg_p = sum_b [dpk_b | dpv_b] ([Lg, D]), row task_id of de_p [pool, Le, D] by the same sum, and row task_id of
 *      de_k [pool, D] = dloss[0] * d(key loss)/d e_k (dloss: one fp32 on the device) -- and nothing outside them; q gets no gradient; the batch is summed
 *      in order (bit-reproducible).
 * D % 64 == 0, Lg / Le even and >= 2, 0 <= task_id < pool (fwd: in train mode), n_g, n_e <= 8 and not both 0. */
int clhip_dual_fwd(int n_g, int n_e, const float* q, const float* const* g_p, const float* const* e_k, const float* const* e_p, void* const* pk, void* const* pv,
                   float* cos, int* idx, float* loss, int B, int D, int pool, int Lg, int Le, int train, int task_id, int dtype, void* stream);
int clhip_dual_bwd(int n_g, int n_e, const float* q, const float* const* e_k, const float* const* dpk, const float* const* dpv, const float* dloss,
                   float* const* dg_p, float* const* de_k, float* const* de_p, int B, int D, int pool, int Lg, int Le, int task_id, void* stream);
/* nn.LayerNorm over the last dim (transformer.py:1331-1336): y = (x-mean)*rstd*gamma+beta; mean/rstd [M] saved when given */
int clhip_ln_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int M, int D, float eps,
                 int dtype, void* stream);
/* g += dLN/dx^T dy  (gamma/beta are frozen on this path: input gradient only) */
int clhip_ln_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* g, int M, int D,
                 int dtype, void* stream);
/* final LN (eps 1e-6) + mean over the first P tokens of each sample -> feat [B,D] fp32 (P = 1: cls token;
 * P = top_k*length: L2P's prompt-token mean, transformer.py:2254-2261) and its backward into g [B*N, D] (rows >= P zeroed) */
int clhip_ln_pool_fwd(const void* x, const float* gamma, const float* beta, float* feat, int B, int N, int D, int P, float eps,
                      int dtype, void* stream);
int clhip_ln_pool_bwd(const float* dfeat, const void* x, const float* gamma, void* g, int B, int N, int D, int P, float eps,
                      int dtype, void* stream);
/* images fp32 NCHW [B,3,img,img] -> patch rows [B*(img/patch)^2, 3*patch^2] (timm PatchEmbed's Conv2d as a GEMM operand) */
int clhip_patchify(const float* images, void* patches, int B, int img, int patch, int dtype, void* stream);
/* x [B, P+1+np, D]: prompt tokens (no pos-embed) | cls + pos[0] | patch_emb + pos[1..]   (transformer.py:2239-2243, 2010-2014) */
int clhip_vit_assemble(const void* patch_emb, const float* cls_token, const float* pos_embed, const float* prompt_tokens, void* x,
                       int B, int n_patches, int n_prompt, int D, int dtype, void* stream);
/* dprompt_tokens[t] = sum_b g[b, t]  (t < n_prompt) */
int clhip_vit_prompt_grad(const void* g, float* dprompt, int B, int N, int n_prompt, int D, int dtype, void* stream);
/* fp32 master [rows, cols] (+ LoRA: rows [rows/3, 2rows/3) += B_k A_k, [2rows/3, rows) += B_v A_v, transformer.py:249-255)
 * -> compute-dtype copies wt [rows, cols] and wt_t [cols, rows] (either nullable) */
int clhip_weight_prep2(const float* w, void* wt, void* wt_t, int rows, int cols, const float* lora_a_k, const float* lora_b_k,
                       const float* lora_a_v, const float* lora_b_v, int rank, int dtype, void* stream);
/* per-step refresh of the k / v rows of the effective qkv copies (W + B A) of `layers` layers in ONE launch: arrays of `layers`
 * device pointers (fp32 masters and LoRA factors; wt [3D, D] and wt_t [D, 3D] in the compute dtype); q rows are left untouched */
int clhip_lora_qkv_refresh(int layers, const float* const* qkv_w, const float* const* lora_a_k, const float* const* lora_b_k,
                           const float* const* lora_a_v, const float* const* lora_b_v, void* const* wt, void* const* wt_t, int D, int rank,
                           int dtype, void* stream);
/* merge_weight (transformer.py:228-234) on the fp32 master qkv weight [3D, D] */
int clhip_lora_merge(float* qkv_w, const float* lora_a_k, const float* lora_b_k, const float* lora_a_v, const float* lora_b_v, int D,
                     int rank, void* stream);
/* d lora_B_k [D, r] += dK^T (X A_k^T), d lora_B_v likewise, dK/dV = columns [D,2D) / [2D,3D) of dqkv; x = the attention
 * input [M, D].  ws: clhip_lora_grad_ws_bytes(M, D, rank) bytes.  Deterministic (slab partials + ordered reduce). */
size_t clhip_lora_grad_ws_bytes(int M, int D, int rank);
/* a_cat (nullable): [32, D] compute-dtype matrix [A_k; A_v; 0] from clhip_lora_acat -- enables the bf16 MFMA path */
int clhip_lora_acat(const float* lora_a_k, const float* lora_a_v, void* a_cat, int D, int rank, int dtype, void* stream);
int clhip_lora_grad(const void* x, const void* dqkv, const float* lora_a_k, const float* lora_a_v, const void* a_cat, float* d_b_k,
                    float* d_b_v, void* ws, int M, int D, int rank, int dtype, void* stream);
/* G [D, D] fp32 += X^T X  (MultiHeadAttention_LoRA get_input_matrix, transformer.py:241-244; the running mean is the caller's) */
int clhip_gram_accum(const void* x, float* G, int M, int D, int dtype, void* stream);
/* the same for n_layers inputs of one pass in ONE launch: layer l reads x + l * layer_stride_elems and adds into G + l * D * D.  bf16: an
 * MFMA "TN" product, one workgroup per (layer, 128 x 128 tile) over all rows -- no atomics, bitwise reproducible; fp32: the scalar kernel per layer */
int clhip_gram_accum_batched(const void* x, size_t layer_stride_elems, int n_layers, float* G, int M, int D, int dtype, void* stream);
/* prompt.L2P.forward (prompt.py:369-406): cosine top-k per sample, batch-majority top-k ids (ties: lowest id), gathered
 * prompt tokens [top_k*length, D], reduce_sim (scalar) and d reduce_sim / d prompt_key [pool, D].  scratch: B+pool+D+B*pool floats. */
int clhip_l2p_select(const float* cls_feat, const float* prompt_key, const float* prompt, int B, int D, int pool, int top_k, int length,
                     int* ids, float* prompt_tokens, float* reduce_sim, float* dkey, float* scratch, void* stream);
int clhip_l2p_scatter(const float* dtokens, const int* ids, float* dprompt_pool, int pool, int top_k, int length, int D, void* stream);

/* AdaptFormer adapter branch (csrc/adapter.hip; petl/vision_transformer_adapter.py:31-90): x, y, hd, dh, gy, gx in the compute dtype, the
 * weights fp32 masters (down_w [R, D], down_b [R], up_w [D, R], up_b [D]); R in {16, 32, 64}, D % 64 == 0, 0 <= p < 1, any M >= 1.  No atomics,
 * bitwise reproducible.
 * fwd  : y [M, D] += scale * (drop(relu(x down_w^T + down_b)) up_w^T + up_b) in one launch; hd (nullable) [M, R] = the dropped hidden rows.
 *        Dropout keeps element (row, col) iff a hash of (*seed, layer, row, col) says so and scales it by 1 / (1 - p); seed: one 64-bit word in
 *        device memory, required iff p > 0.  p == 0: nothing is drawn or scaled.
 *        0 < p < 2^-24 is refused (24 hash bits).  fwd / bwd: a workgroup owns 32 or 64 rows; clhip_config("ADAPTER_TM", "32" | "64") pins it.
 * bwd  : dh [M, R] = ((scale * gy) up_w) * [hd > 0] / (1 - p);  gx [M, D] = gy + dh down_w  (gx may be gy)
 * wgrad: d_up_w = scale * gy^T hd, d_up_b = scale * sum_rows gy, d_down_w = dh^T x, d_down_b = sum_rows dh (written, not accumulated);
 *        ws: clhip_adapter_wgrad_ws_bytes(M, D, R) bytes (row-slab partials, reduced in slab order)
 * dropout_mask: out [M, R] bytes, 1 = kept -- the mask clhip_adapter_fwd applies for the same (seed, layer, p) */
int clhip_adapter_fwd(const void* x, const float* down_w, const float* down_b, const float* up_w, const float* up_b, void* y, void* hd,
                      const unsigned long long* seed, int layer, float p, float scale, int M, int D, int R, int dtype, void* stream);
int clhip_adapter_bwd(const void* gy, const void* hd, const float* up_w, const float* down_w, void* dh, void* gx, float p, float scale, int M,
                      int D, int R, int dtype, void* stream);
size_t clhip_adapter_wgrad_ws_bytes(int M, int D, int R);
int clhip_adapter_wgrad(const void* gy, const void* hd, const void* x, const void* dh, float* d_up_w, float* d_up_b, float* d_down_w,
                        float* d_down_b, void* ws, float scale, int M, int D, int R, int dtype, void* stream);
int clhip_adapter_dropout_mask(const unsigned long long* seed, int layer, int M, int R, float p, unsigned char* out, void* stream);

/* SD-LoRA (core/model/sd_lora.py; MultiHeadAttention_SDLoRA, core/model/backbone/transformer.py:276-357; csrc/sdlora.hip).  Per attention layer and for
 * q and v separately the low-rank branch is a sum over nterms = T + 1 terms: term i has rank ranks[i] (HOST array, each 1..16, sum <= 512; ranks may
 * differ), A_i [r_i, D] and B_i [D, r_i] fp32.  The factor table of a layer is 4 * nterms DEVICE-resident pointers [A^q terms | B^q terms | A^v
 * terms | B^v terms]; `factors` of the refresh holds one such table per layer, back to back.  mag [nterms] and inv [layers, 2, nterms] (q then v;
 * inv of the current term = 1, of a past term 1 / (|B_i|_F |A_i|_F) or 0) are device vectors; c_i = mag[i] * inv[l, w, i].  D % 64 == 0, any M >= 1.
 * refresh: replaces qq / vv of transformer.py:317-336 by the effective weight W + sum_i c_i B_i A_i on the q and v rows of wt [3D, D] and wt_t
 *          [D, 3D] (compute dtype) of ALL layers in one launch: fp32 accumulation in term order 0..T, one rounding on the store; k rows untouched.
 * grad   : replaces autograd through transformer.py:317-332 for one layer: with X [M, D] the attention input and dQ / dV the q / v column blocks of
 *          dqkv [M, 3D], P_i = X A_i^T, S_i = dQ^T P_i:  d_b = m_T S_T [D, r_T], d_a = m_T (dQ B_T)^T X [r_T, D] (q and v), and
 *          d_mag_row[i] = sum_{q, v} inv_i <S_i, B_i>_F, this layer's row of partials.  All outputs are WRITTEN.  The K = D products run on the MFMA GEMM
 *          and the K = M products on the bf16 MFMA (plain FMA in fp32 mode), as slab partials reduced in slab order: no atomics, bitwise reproducible.
 *          ws: clhip_sdlora_grad_ws_bytes(M, D, sum of ranks) bytes.
 * mag_reduce: d_mag [nterms] = the rows [depth, nterms] summed in layer order. */
int clhip_sdlora_refresh(int layers, const float* const* qkv_w, const float* const* factors, const int* ranks, int nterms, const float* mag,
                         const float* inv, void* const* wt, void* const* wt_t, int D, int dtype, void* stream);
size_t clhip_sdlora_grad_ws_bytes(int M, int D, int sum_r);
int clhip_sdlora_grad(const void* x, const void* dqkv, const float* const* factors, const int* ranks, int nterms, const float* mag, const float* inv,
                      float* d_a_q, float* d_b_q, float* d_a_v, float* d_b_v, float* d_mag_row, void* ws, int M, int D, int dtype, void* stream);
int clhip_sdlora_mag_reduce(const float* rows, int depth, int nterms, float* d_mag, void* stream);

/* LoRA-Sub-DRS (core/model/lora_sub.py; MultiHeadAttention_LoRA_Sub, core/model/backbone/transformer.py:359-444; csrc/lorasub.hip).  Exact fp32, no atomics,
 * every sum in a fixed order: two runs are bitwise equal.  Every call refuses bad arguments before it launches anything.
 * atl     : AugmentedTripletLoss.forward (lora_sub.py:34-68, the Python double loop over batch x prototypes at :51-63) and its autograd backward in two
 *           launches.  f [B, D] the UN-normalised features, labels [B], protos [P, D] un-normalised (NULL iff P == 0).  With n_i = f_i / |f_i| and
 *           c_p = proto_p / |proto_p|:  d_ij = sqrt(max(|n_i - n_j|^2, 1e-12)), e_ip = max(|n_i - c_p|, 1e-12), both summed from the DIFFERENCES (the
 *           expansion |a|^2 + |b|^2 - 2ab of :41-43 loses the self and near pairs in fp32);  ap_i = max over {j: y_j == y_i} (j = i included),
 *           an_i = min over {j: y_j != y_i}, or ap_i + margin when there is none, then the smallest e_ip if it is < an_i;  ties go to the lower index,
 *           batch rows before prototypes.  loss[0] = mean_i max(0, ap_i - an_i + margin) (unweighted; a row without any negative counts 0),
 *           df [B, D] = weight * d loss / d f, WRITTEN: through both ends of a selected batch pair (row j gathers, in ascending i, the rows that
 *           selected it), the n_i end of a prototype pair, nothing through a clamped distance, and through the normalisation as (g - n (n.g)) / |f|.
 *           1 <= B <= 256, 0 <= P <= 1024, D % 64 == 0 and D <= 8192 (one normalised row in LDS).  ws: clhip_atl_ws_bytes(B, P) bytes.
 * lora_grad_ab: replaces autograd through transformer.py:401-424 for one layer when A and B both train: X [M, D] the attention input, dK / dV the k / v
 *           column blocks of dqkv [M, 3D] (compute dtype), the factors fp32 (A [r, D], B [D, r]):  d_b = dK^T (X A^T) [D, r], d_a = (dK B)^T X [r, D], the
 *           same for v.  All four WRITTEN.  The K = D products run on clhip_gemm_nt, the K = M products are slab partials (csrc/tn_slab.hip) reduced in slab
 *           order.  Rank 1..16, any M >= 1, D % 64 == 0.  ws: clhip_lora_grad_ab_ws_bytes(M, D) bytes.
 * proj_adam_multi: the projected Adam step of lora_sub.py:120-157, :193-233 over `count` = 4 * layers factor tensors in at most two launches.  tensors:
 *           DEVICE table [count][4] of pointers (p, g, m, v), per layer in the order A_k [r, D], B_k [D, r], A_v, B_v;  transforms: DEVICE table [layers] of
 *           T_l [D, D] fp32, or NULL = plain Adam (task 0: one launch, element for element clhip_adam_step with grad_scale 1).  Moments and bias
 *           correction as clhip_adam_step (weight_decay joins the gradient first); with q = m / (sqrt(v) / sqrt(bc2) + eps), the scalar step factored out
 *           of the product:  B <- B - (lr / bc1) (T_l q),  A <- A - (lr / bc1) (q T_l), each element accumulated in ascending index.  T_l is read once
 *           for the two B and once for the two A of a layer.  Rank 1..16, D % 32 == 0.  ws: count * D * rank floats. */
size_t clhip_atl_ws_bytes(int B, int P);
int clhip_atl(const float* f, const int64_t* labels, const float* protos /*nullable*/, int B, int D, int P, float margin, float weight, float* loss,
              float* df, void* ws, void* stream);
size_t clhip_lora_grad_ab_ws_bytes(int M, int D);
int clhip_lora_grad_ab(const void* x, const void* dqkv, const float* lora_a_k, const float* lora_b_k, const float* lora_a_v, const float* lora_b_v,
                       float* d_a_k, float* d_b_k, float* d_a_v, float* d_b_v, void* ws, int M, int D, int rank, int dtype, void* stream);
int clhip_proj_adam_multi(int count, void* const* tensors, const float* const* transforms /*nullable*/, float* ws, int D, int rank, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int step, void* stream);

/* Whole-backbone executor: one C call per forward / backward (VisionTransformer.forward, transformer.py:2222-2294, and
 * the autograd backward of L2P.observe / the trainer's loss.backward()). */
typedef struct clhip_vit_desc {
    int32_t img, patch, dim, depth, heads, mlp, lora_rank;
    float block_ln_eps;   /* eps of the per-block LayerNorms: 0 -> 1e-5 (transformer.py nn.LayerNorm default); timm-style trees
                           * (vit_inflora.py:375) use 1e-6 everywhere.  The final norm is 1e-6 in both. */
    int32_t adapter_dim;  /* AdaptFormer bottleneck width R in {16, 32, 64}; 0: no adapters (the executor is then exactly what it was) */
    float adapter_scale;  /* s of x_out = x_mid + mlp(LN2(x_mid)) + s * adapter(x_mid) */
} clhip_vit_desc;
typedef struct clhip_vit_layer_params {
    const float *qkv_w, *qkv_b, *proj_w, *proj_b, *ln1_w, *ln1_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b, *ln2_w, *ln2_b;
    const float *lora_a_k, *lora_b_k, *lora_a_v, *lora_b_v;          /* NULL without LoRA */
    const float *ad_down_w, *ad_down_b, *ad_up_w, *ad_up_b;          /* adapter [R, D], [R], [D, R], [D]; NULL without adapters */
} clhip_vit_layer_params;
typedef struct clhip_vit_params {
    const float *cls_token, *pos_embed, *pe_w, *pe_b, *norm_w, *norm_b;
    const clhip_vit_layer_params* layers;                            /* [depth] */
} clhip_vit_params;
typedef struct clhip_vit clhip_vit;
clhip_vit* clhip_vit_create(const clhip_vit_desc* desc, int dtype);
void clhip_vit_destroy(clhip_vit* v);
size_t clhip_vit_shadow_bytes(const clhip_vit* v);
size_t clhip_vit_workspace_bytes(const clhip_vit* v, int B, int n_prompt, int save_for_backward);
/* fp32 masters -> compute-dtype weight copies in `shadow`; apply_lora folds B A into the k/v rows; qkv_only != 0 refreshes
 * just the qkv copies (what changes between InfLoRA steps) */
int clhip_vit_prep_weights(clhip_vit* v, const clhip_vit_params* P, void* shadow, int apply_lora, int qkv_only, void* stream);
/* images fp32 [B,3,img,img]; prompt_tokens fp32 [n_prompt, D] (NULL / 0: none); feat [B, D] fp32 = final LN pooled over the
 * prompt tokens (n_prompt > 0) or at the cls token; gram (nullable) [depth, D, D] += X^T X of every attention input */
int clhip_vit_forward(clhip_vit* v, const clhip_vit_params* P, const void* shadow, void* workspace, const float* images, int B,
                      const float* prompt_tokens, int n_prompt, int save_for_backward, float* gram, float* feat, void* stream);
/* The backward of the last forward that ran with save_for_backward, and every parameter gradient of the ViT path.  Each member of clhip_vit_grads is nullable:
 * NULL = that gradient is not asked for (out == NULL: none of them; the chain still runs).  Every argument rule is checked before the first launch.
 * dprompt_tokens: [n_prompt, D], written; needs n_prompt > 0 in the saved forward.  Without it the chain stops after the lowest layer's attention backward.
 * d_lora_b : [2*depth] pointers (k, v per layer) to [D, r], ACCUMULATED into; for a fixed A (InfLoRA; lora_rank > 0).  It reads the [A_k; A_v] operand that
 *            clhip_vit_prep_weights packed, which clhip_vit_lora_refresh_ab does NOT refresh: it must not follow that call without a full prep_weights.
 * d_adapter: [4*depth] pointers (d down_w [R, D], d down_b [R], d up_w [D, R], d up_b [D] per layer), written (adapter_dim > 0).  With adapters the input
 *            gradient of every adapter branch is part of the chain either way.
 * d_sd     : SD-LoRA (clhip_vit_set_sdlora): [4*depth] pointers (d A_q, d B_q, d A_v, d B_v of the current term per layer), written by clhip_sdlora_grad per
 *            layer; requires d_mag_rows [depth, nterms] (scratch) and d_mag [nterms] = its rows summed in layer order, after the chain, on the caller's stream.
 * d_ab     : LoRA-Sub-DRS (A and B both train): [4*depth] pointers (d A_k, d B_k, d A_v, d B_v of the layer), written by clhip_lora_grad_ab per layer; requires
 *            ab_ws: clhip_lora_grad_ab_ws_bytes(M, D) bytes of the caller's, M = B * tokens of the saved forward (lora_rank > 0).
 *            d_lora_b, d_sd and d_ab exclude one another.  They are leaves of the chain: outside a stream capture (and unless WGRAD_STREAM=0) they run on a
 *            side stream, ordered by events against the one dqkv buffer; the caller's stream owns the gradients again when the call returns.
 * dpk, dpv : the prefix gradients of a forward that ran in prefix mode (clhip_vit_set_prefix): both required for one, refused otherwise.  [depth] host arrays
 *            of fp32 [B, Lp[l], D] buffers, written (entries of plain layers are ignored).  Without any other gradient the chain stops at the lowest
 *            prefixed layer's attention backward. */
typedef struct clhip_vit_grads {
    float* dprompt_tokens;
    float *const *d_lora_b, *const *d_adapter;
    float *const *d_sd, *d_mag_rows, *d_mag;
    float* const* d_ab;
    void* ab_ws;
    float *const *dpk, *const *dpv;
} clhip_vit_grads;
int clhip_vit_backward(clhip_vit* v, const clhip_vit_params* P, const void* shadow, void* workspace, const float* dfeat, const clhip_vit_grads* out,
                       void* stream);
/* adapter dropout of the NEXT clhip_vit_forward (and of the backward that follows it): probability p in [0, 1) and the 64-bit seed in device
 * memory (required iff p > 0; read when the kernels run, so it must stay alive until then).  The forward consumes the state: forwards after it
 * run without dropout until this is called again. */
int clhip_vit_set_adapter_dropout(clhip_vit* v, const unsigned long long* seed, float p);
/* SD-LoRA mode of the executor (new entry points; descriptors and parameter tables are untouched, so every other caller gets the executor it had).
 * set_sdlora: nterms > 0 switches the mode on -- ranks (host, copied), factors = [depth] factor tables back to back, mag [nterms], inv [depth, 2,
 *          nterms] on the device, all alive until replaced; forwards that save for the backward then keep every layer's attention input.  nterms = 0
 *          switches it off.  Requires lora_rank == 0 in the descriptor.
 * sdlora_refresh: clhip_sdlora_refresh on the executor's qkv copies (after clhip_vit_prep_weights without LoRA, and then once per step).
 *          Its gradients: the d_sd member of clhip_vit_grads. */
int clhip_vit_set_sdlora(clhip_vit* v, int nterms, const int* ranks, const float* const* factors, const float* mag, const float* inv);
int clhip_vit_sdlora_refresh(clhip_vit* v, const clhip_vit_params* P, void* shadow, void* stream);
/* LoRA-Sub-DRS: A and B of the k / v LoRA terms both train (lora_rank > 0; the layers' qkv_w point at the caller's composed fp32 masters).
 * lora_refresh_ab: the per-step refresh when A moves too -- the k / v rows of all layers' qkv copies (W + B A, one launch); the q rows and every other weight
 *   copy keep the rounding of the last clhip_vit_prep_weights.  The [A_k; A_v] operand of clhip_lora_grad is NOT refreshed: clhip_vit_backward's d_lora_b is
 *   for a fixed A (InfLoRA) and must not follow this call without a full clhip_vit_prep_weights.  Its gradients: the d_ab member of clhip_vit_grads. */
int clhip_vit_lora_refresh_ab(clhip_vit*, const clhip_vit_params* params, void* shadow, void* stream);
/* Prefix mode of the executor (VisionTransformer.forward with `prompt`, transformer.py:2272-2288: blocks whose prompt is not None attend over
 * [prefix | tokens]).  Descriptors and parameter tables are untouched.
 * set_prefix: Lp [depth] (host, copied; 0 = a plain layer, at least one > 0), pk / pv [depth] host arrays of device pointers to [B, Lp[l], D] in the
 *          compute dtype (copied; the BUFFERS are the caller's and must outlive the backward).  The state PERSISTS: every forward after it runs in prefix
 *          mode until Lp == NULL switches it off (CODA-Prompt's query pass runs with the mode off).  A forward remembers the prefixes it ran with, so
 *          switching afterwards does not disturb its backward.  The saved lse stays [B, H, N]; the workspace size does not change.
 *          Its gradients: the dpk / dpv members of clhip_vit_grads. */
int clhip_vit_set_prefix(clhip_vit* v, const int* Lp, const void* const* pk, const void* const* pv);
/* CLIP mode of the executor: the visual tower of the reference's CLIP backbone (VisualTransformer.forward, transformer.py:2121-2140) is this ViT with
 * four differences.  Descriptors and parameter tables are untouched; a caller that never calls this gets the executor it had.
 * set_clip: ln_pre_w / ln_pre_b [D] fp32 on the device (alive while the mode is on; both NULL = no ln_pre), final_eps = eps of the pooled final LN
 *          (ln_post: 1e-5; the executor's own is 1e-6), quick_gelu 0 / 1.  NULL ln_pre together with quick_gelu == 0 switches the mode off (final_eps is
 *          then ignored and 1e-6 again).  The state PERSISTS.  In the mode:
 *            - pe_b == NULL in clhip_vit_params means a patch convolution without bias (:2107); outside the mode a NULL pe_b is refused;
 *            - the assembled token rows (class embedding + pos[0] | patches + pos[1..], :2125-2126) are normalised by ln_pre (eps 1e-5, :2127): layer 0's
 *              saved x_in (clhip_vit_read_act which 0) is the ln_pre OUTPUT.  The un-normalised rows pass through the LN scratch: no workspace change;
 *            - fc1 runs epilogue 6 of clhip_gemm_nt (QuickGELU, :137-139); its backward is epilogue 4 on the saved derivative as before;
 *            - clhip_ln_pool_fwd / _bwd run with final_eps (a backward uses the eps of the forward it belongs to).
 *          block_ln_eps = 0 in the descriptor already gives the blocks' 1e-5.  The Gram accumulation and d_lora_b work unchanged.  Without prompt tokens
 *          the backward stops at the lowest layer's attention backward, so ln_pre has no backward.
 *          Prompt tokens, prefix mode, adapters and SD-LoRA do not combine with the mode: set_clip refuses an executor that has them, and a forward in
 *          the mode refuses them, with CLHIP_EINVAL before any launch. */
int clhip_vit_set_clip(clhip_vit* v, const float* ln_pre_w, const float* ln_pre_b, float final_eps, int quick_gelu);
/* CLIP's image-side logits (CLIP.forward, core/model/backbone/clip.py:405-412; csrc/clip.hip).  Exact fp32, no atomics, every sum in a fixed order: two
 * runs are bitwise equal.  One workgroup per image, one launch each way.
 * fwd: feat [B, D] (the executor's pooled ln_post output), proj [D, E] (visual.proj), txt [C, E] text features that are ALREADY L2-normalised (they are
 *      not normalised again), scale = exp(logit_scale):  u = feat . proj,  n = u / |u|,  logits [B, C] = scale * n . txt^T.  Saves u [B, E] and
 *      inv_norm [B] = 1 / |u| for the backward.  As in the reference NO eps guards the norm: a row with u = 0 gives inf / NaN and is the caller's problem.
 * bwd: dlogits [B, C] -> dfeat [B, D] = proj . ((g - n (n . g)) / |u|),  g = scale * dlogits . txt.  proj and txt take no gradient here (the text tower
 *      and visual.proj are frozen on this path).
 * All outputs are WRITTEN.  B, D, E, C >= 1, D + E <= 4096 and E + C <= 4096 (one row of each in LDS).  CE and predictions stay on clhip_ce_slice /
 * the argmax of the head (ties to the lower index). */
int clhip_clip_logits_fwd(const float* feat, const float* proj, const float* txt, float scale, float* logits, float* u, float* inv_norm, int B, int D, int E,
                          int C, void* stream);
int clhip_clip_logits_bwd(const float* dlogits, const float* proj, const float* txt, float scale, const float* u, const float* inv_norm, float* dfeat, int B,
                          int D, int E, int C, void* stream);
/* debug/test: copy one saved tensor of layer l of the last forward to fp32: 0 x_in [M, D] (layer == depth: the last block's output), 1 qkv [M, 3D],
 * 2 attn out, 3 x_mid, 4 GELU derivative of the mlp [M, mlp], 5 h1 = the LN1 output [M, D], 6 lse [B, H, N], 7 the LN1 statistics [2, M] (mean row, rstd
 * row), 8 the LN2 statistics likewise, 9 the adapter's dropped hidden rows [M, R].  0..4 and 6..9 need a forward that saved for the backward; 5 needs h1 to
 * have a region of its own (LoRA or SD-LoRA with a saving forward, or any forward with a Gram buffer): where it aliases the LN2 scratch the call is
 * refused, as is 9 without adapters.  Host bookkeeping and one copy; nothing of a step changes. */
int clhip_vit_read_act(clhip_vit* v, void* workspace, int layer, int which, float* out, void* stream);
/* debug/test: a gradient tap.  While buf != NULL every backward copies each buffer of its chain to fp32 in buf right after the launch that wrote it,
 * on the caller's stream (the copy of dqkv is one more reader ahead of the next layer's writer on that stream: no new event).  With M = B * tokens of
 * the last saved forward, in floats: [0, M D) = g after the pooled-LN backward; layer l's slots start at M D + l * stride, stride = M (mlp + 8 D) (+ M (R + D)
 * with adapters), in this order: dbig [M, mlp] | with adapters: ad_dh [M, R], the adapter's output gradient g + dh Wd [M, D] | dtmp after the fc1 dgrad |
 * g after the LN2 backward | dtmp after the proj dgrad [M, D each] | dqkv [M, 3D] | dtmp after the qkv dgrad | g after the LN1 backward [M, D each].
 * Slots of launches a backward does not run are left untouched.  tap_floats: the size for the last saved forward (0: none).  A backward whose tap is
 * smaller is refused.  set_tap(v, NULL, 0) switches it off. */
int clhip_vit_set_tap(clhip_vit* v, float* buf, size_t floats);
size_t clhip_vit_tap_floats(const clhip_vit* v);
/* host bookkeeping of the last backward that passed its argument checks: did its leaves (LoRA / SD-LoRA weight gradients) run on the side stream, and the
 * lowest layer it ran (the prefix-only backward stops at the lowest prefixed layer) */
int clhip_vit_last_backward_info(const clhip_vit* v, int* side_stream_used, int* lowest_layer_run);

/* ------------------------------------------------------------------------------------------------
 * Input pipeline on the GPU.  store: uint8 [Nimg, H, W, 3] resident in HBM; index [B]: rows
 * of the store that form the batch; out: fp32 NCHW [B, 3, S, S].  mean3 / std3 are HOST pointers (3 floats each).
 * crop_flip = RandomCrop(S, padding=pad) + RandomHorizontalFlip + ColorJitter(brightness) + ToTensor + Normalize of the
 *   reference's CIFAR ResNet pipeline (core/data/data.py:4-19); params [B,3] = (dy, dx in [0, H+2pad-S], flip 0/1) drawn by the
 *   caller; brightness [B] factors or NULL.  (dy = dx = pad, flip = 0, brightness NULL = the test transform.)
 * rrc_flip  = RandomResizedCrop(S) (bilinear) + RandomHorizontalFlip + ToTensor [+ Normalize] of the ViT configs
 *   (config/l2p-...yaml train_trfms); params [B,5] = (y0, x0, h, w, flip): the crop box in source pixels. */
int clhip_augment_crop_flip(const uint8_t* store, const int64_t* index, const int32_t* params, const float* brightness /*nullable*/,
                            float* out, int B, int H, int W, int S, int pad, const float* mean3, const float* std3, void* stream);
int clhip_augment_rrc_flip(const uint8_t* store, const int64_t* index, const int32_t* params, float* out, int B, int H, int W, int S,
                           const float* mean3, const float* std3, void* stream);
/* rrc_aa = the same pipeline for stores whose images are LARGER than S (ImageNet-R, config/InfLoRA_opt-vit-imagenetr-b20-20-10.yaml
 *   :28-35), where torchvision's resize on PIL images anti-aliases: Pillow's two fixed-point passes (triangle filter of support
 *   max(scale, 1), 22-bit weights, uint8 intermediate image), reproduced bit for bit.  The store may be RAGGED: image i = uint8
 *   [hw[2i], hw[2i+1], 3] at store + offsets[i] (offsets / hw NULL: a uniform [Nimg, H, W, 3] store).  max_box >= the largest
 *   crop-box side of the batch (sizes the coefficient table: ws of clhip_augment_rrc_aa_ws_bytes(B, S, max_box) bytes). */
size_t clhip_augment_rrc_aa_ws_bytes(int B, int S, int max_box);
int clhip_augment_rrc_aa(const uint8_t* store, const int64_t* offsets /*nullable*/, const int32_t* hw /*nullable*/, const int64_t* index,
                         const int32_t* params, float* out, void* ws, int B, int H, int W, int S, int max_box, const float* mean3,
                         const float* std3, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RanPAC: random-projection ridge classifier (core/model/ranpac.py) in exact fp32 on the f32-input MFMA (csrc/rp.hip).  Everything is fp32,
 * row-major and dense; no atomics, fixed summation order (bitwise reproducible); any N, D, M, C, B >= 1.
 * project   : H [N, M] = F [N, D] W [D, M], through a ReLU when relu != 0  (ranpac.py:248 and :55; W_rand as :221 stores it)
 * gram_accum: G [M, M] += H^T H  (ranpac.py:251, :257).  Only the tiles on or above the diagonal are computed and each is written to both places:
 *             G stays exactly symmetric.  No split along N; successive calls accumulate (read-modify-write of the tile).
 * label_sum : Q [M, C] += H^T onehot(labels), a per-class column sum with the rows in ascending order (ranpac.py:246, :250, :256); labels: int64
 *             [N] on the device.  A label outside [0, C) makes the call return CLHIP_EINVAL before Q is touched (checked on the device copy; this
 *             call synchronises the stream).
 * classify  : logits [B, C] = sigma * relu(X [B, D] W [D, M]) Wo [C, M]^T, the use_RP branch of CosineLinear.forward (ranpac.py:53-61).  sigma: one
 *             float on the device (NULL: 1).  ws: clhip_rp_classify_ws_bytes(B, M, C) bytes (the hidden rows and the K-slice partials, which are
 *             summed in slice order). */
int clhip_rp_project(const float* F, const float* W, float* H, int N, int D, int M, int relu, void* stream);
int clhip_rp_gram_accum(const float* H, float* G, int N, int M, void* stream);
int clhip_rp_label_sum(const float* H, const int64_t* labels, float* Q, int N, int M, int C, void* stream);
size_t clhip_rp_classify_ws_bytes(int B, int M, int C);
int clhip_rp_classify(const float* X, const float* W, const float* Wo, const float* sigma /*nullable*/, float* logits, void* ws, int B, int D, int M,
                      int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * InfLoRA_OPT classifier alignment (core/model/InfLoRA_opt.py:371-456) in exact fp32 on the f32-input MFMA (csrc/ca.hip), under the rules of the
 * RanPAC kernels: fp32, row-major, dense; no atomics, summation order a function of the shapes only; any D, C, S >= 1.
 * class_moments: the Gaussians of InfLoRA_opt.py:392-397.  F [N, D] holds the feature rows grouped by class, offsets int32 [C + 1] on the device
 *             (offsets[0] = 0, offsets[C] = N) where each class starts.  mean [C, D] = the column means of the class's rows, summed in row order
 *             (:396); cov [C, D, D] = sum (x - mean)(x - mean)^T / (n_c - 1) + eps on the diagonal (:397, torch.cov's unbiased estimate).  The mean is
 *             subtracted as the rows enter LDS; only the tiles on or above the diagonal are computed and each is written to both places, so cov[c]
 *             is exactly symmetric.  The offsets are read back and checked on the host (this call synchronises the stream): a class with fewer than
 *             2 rows, offsets that do not increase, offsets[0] != 0 or offsets[C] != N return CLHIP_EINVAL before anything is launched.
 * ca_sample : the draws of InfLoRA_opt.py:418-437 for C classes with S rows each, given the Cholesky factors chol [C, D, D] (lower, row-major) and
 *             standard normals Z [C * S, D]:  X[dest[c * S + s], j] = scale[c] * mean[c, j] + sum_{k <= j} Z[c * S + s, k] * chol[c, j, k]
 *             (MultivariateNormal.sample = loc + L z with loc = mean * (0.9 + decay), :421-427) and labels[dest[c * S + s]] = class_lo + c (:429);
 *             dest is the place of a row after the shuffle of :435-437.  One triangular product per class: K blocks above the diagonal are skipped,
 *             and the strict upper triangle of chol is never read.  dest int64 [C * S] must be a permutation of [0, C * S): otherwise the call
 *             returns CLHIP_EINVAL with X untouched (checked on the device, with `labels` as the scratch of the check; this call synchronises
 *             the stream). */
int clhip_class_moments(const float* F, const int32_t* offsets, float* mean, float* cov, int N, int D, int C, float eps, void* stream);
int clhip_ca_sample(const float* mean, const float* scale, const float* chol, const float* Z, const int64_t* dest, float* X, int64_t* labels, int C,
                    int S, int D, int64_t class_lo, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RAPF's adapter step (core/model/rapf.py; csrc/rapf.hip) under the same rules: fp32 in / fp32 accumulate, the matrix-shaped products on the f32-input
 * MFMA, row-major and dense, no atomics, every sum in an order fixed by the shapes (two calls give the same bits), every output WRITTEN.
 * Notation: X [R, E] the step's rows, R = B + M + Q: B image rows | M replay rows | Q edge rows; W [E, E] the adapter in nn.Linear layout (out x in);
 * T [C, E] the text rows, ALREADY L2-normalised (they are not normalised again); scale = exp(logit_scale).
 * rapf_draw    : sample() (rapf.py:37-44) as called from :318-322 and :328-334.  G groups; group g draws cnt[g] rows of class cls[g]:
 *                X[row0 + r, j] = mean[cls[g], j] + sum_{k <= j} Z[r, k] * chol[cls[g], j, k], r counting through the groups in order.  mean [Cs, E],
 *                chol [Cs, E, E] (lower, row-major, one factor per STORED class: the covariance does not change after after_task, so it is factored there,
 *                not in every step as :41 does), Z [sum cnt, E] standard normals.  The draws land behind the image rows of the step's row matrix: nothing
 *                is concatenated, and rows outside [row0, row0 + sum cnt) are untouched.  A class may appear in several groups and the counts may
 *                differ.  The strict upper triangle of chol is never read.  cls / cnt are HOST arrays (int32 [G]): a class outside [0, Cs) or a count
 *                < 1 returns CLHIP_EINVAL before any launch, with no synchronisation; the table travels in the kernel arguments (128 groups per launch).
 * rapf_step_fwd: ClassIncrementalCLIP.forward (:143-153) and the losses (:341-353).  A = X W^T, n_r = A_r / |A_r| -- NO eps, as in the reference: a zero
 *                row gives inf / NaN and is the caller's problem.  Rows r < B + M: logits[r, c] = scale * n_r . T_c and the mean over those rows of
 *                CE(logits_r, labels[r]) is loss_c.  Edge row q (r = B + M + q): h_q = relu(margin - n . T[pos[q]] + n . T[neg[q]]) (margin 0.1 at
 *                :348), loss_h = mean_q h_q.  The reference's second normalisation of the edge and text rows (:343-347) is the identity on unit
 *                vectors, in value and in Jacobian, and is done once.  Outputs: logits [B + M, C]; n [R, E]; loss [3] = (loss_c + loss_h if Q > 0
 *                else loss_c, loss_c, loss_h); row_loss [R] (the CE term of a row, h_q of an edge row); pred int64 [B] (argmax of the image rows, ties to
 *                the lower index); correct int32 [1] (nullable); and G [R, E] = dloss/dA:
 *                    g_n = scale / (B + M) * (softmax - onehot) . T on CE rows, 1[h_q > 0] / Q * (T[neg] - T[pos]) on edge rows (h_q == 0: 0, torch's relu),
 *                    G_r = (g_n - n_r (n_r . g_n)) / |A_r|.
 *                labels int64 [B + M], pos / neg int64 [Q] live on the device.  A label outside [0, C) is treated as clhip_ce_slice treats one outside its
 *                slice: no loss term, no onehot in the gradient (the softmax part stays), never counted correct.  An edge pair with pos or neg outside
 *                [0, C) is inactive: h_q = 0 and G_r = 0.  M = 0 and Q = 0 are ordinary cases (pos / neg may then be NULL).
 *                INFERENCE form: labels == NULL (then M = Q = 0): only logits and n are written; G, row_loss, loss, pred, correct may be NULL.
 *                2 E + C <= 8192 (one row of n, g_n and the logits in LDS).
 * rapf_step_bwd: dW [E, E] = g * G^T X, dW[o, i] = g * sum_r G[r, o] * X[r, i] with r ascending inside one workgroup per tile (no slabs at R of a few
 *                hundred); g is the upstream scalar. */
int clhip_rapf_draw(const float* mean, const float* chol, const float* Z, float* X, const int32_t* cls, const int32_t* cnt, int G, int Cs, int E, int row0,
                    void* stream);
int clhip_rapf_step_fwd(const float* X, const float* W, const float* T, const int64_t* labels /*nullable*/, const int64_t* pos /*nullable*/,
                        const int64_t* neg /*nullable*/, float scale, float margin, float* logits, float* n, float* G, float* row_loss, float* loss,
                        int64_t* pred, int32_t* correct /*nullable*/, int B, int M, int Q, int E, int C, void* stream);
int clhip_rapf_step_bwd(const float* G, const float* X, float g, float* dW, int R, int E, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLHIP_H */
