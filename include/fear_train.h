/*
 * fear_train.h — C ABI of the MI355X (gfx950) operators of the FEAR head TRAINING step (SURVEY.md §8f N3,
 * BASELINE.json configs[4] "training step: backbone + xcorr fwd/bwd"; first slice = BoxTower + FEARLoss).
 *
 * What the reference does with torch autograd + cuDNN is spelled out here as explicit forward / backward operators:
 *     SepConv (depthwise 3x3 -> pointwise 1x1)         model_training/model/blocks.py:45-72
 *     nn.BatchNorm2d in training mode (+ ReLU)         model/blocks.py:98-101, 115-119, 150-158
 *     MobileCorrelation  s = z^T x, cat[x, s]          model/blocks.py:121-126
 *     exp(adjust * x + bias), 0.1 * cls                model/blocks.py:186-192
 *     FEARLoss (BCE-with-logits halves + 1 - IoU)      model_training/train/loss.py:13-96
 * feartracker_amd/train_head.py composes them into `BoxTower.forward` + loss + backward (host code stays Python, like the
 * reference's Lightning step train/fear_lightning_model.py:60-66); gradients of all ranks are averaged by ONE RCCL
 * all-reduce of the flat gradient buffer (the reference: Lightning DDP, train/trainer.py:50-52).
 *
 * Conventions: plain C; every tensor pointer is a DEVICE pointer, fp32, "rows x channels" NHWC ([M = batch*H*W][ld], channels
 * contiguous, ld = row stride in floats) unless it says NCHW; `stream` is a hipStream_t passed as void*; calls are
 * asynchronous on it; 0 on success, negative FEAR_TRAIN_ERR_* otherwise.  `workspace` is caller-owned scratch of at least
 * fear_train_workspace_bytes(rows, max_channels) bytes; every reduction is two-stage in a fixed order (no atomics).
 */
#ifndef FEAR_TRAIN_H
#define FEAR_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#include "fear_hip.h"   /* fear_frame */

#ifdef __cplusplus
extern "C" {
#endif

#define FEAR_TRAIN_OK 0
#define FEAR_TRAIN_ERR_NULL (-1)
#define FEAR_TRAIN_ERR_SHAPE (-2)
#define FEAR_TRAIN_ERR_HIP (-4)
#define FEAR_TRAIN_ERR_WORKSPACE (-7)   /* workspace missing or too small */
#define FEAR_TRAIN_ERR_SYNC (-8)        /* the SyncBatchNorm all-reduce callback failed, or its buffer is too small (fear_train_sync_bind) */
#define FEAR_TRAIN_ERR_FORMAT (-9)      /* fear_jpeg_parse, fear_jpeg_entropy_decode: the bytes are no complete baseline JPEG */
#define FEAR_TRAIN_ERR_UNSUPPORTED (-10) /* the same two: a valid JPEG of a kind the decoder declines */
/* After FEAR_TRAIN_ERR_SYNC a caller may rely on this: the call returned right after the failed all-reduce, without launching what
 * would have read the un-reduced buffer — running_mean, running_var and `vec` of the failed BatchNorm and of every BatchNorm behind it
 * in the call are NOT written (a block's BatchNorms that completed before it keep their update); every other output of the call
 * (raw tensors, local d gamma / d beta, scratch, workspace) is unspecified.  The failure is not remembered: the next call on the same
 * host thread, bound or not, starts clean, so the step can be retried once the collective works again. */

size_t fear_train_workspace_bytes(long rows, int max_channels);

/* Layout rules for every operator below: activations are row-major [rows][ld] fp32 with 16-byte-aligned bases; channel
 * counts and leading dimensions are multiples of 4 floats (rows are read and written as float4s), ld >= the row's width;
 * violations return FEAR_TRAIN_ERR_SHAPE. */
/* Empty calls: every operator from here to fear_dw_backward_weight_act returns FEAR_TRAIN_OK for M == 0 (B == 0 for the depthwise ones)
 * before it looks at any other argument, launches nothing and writes nothing — not even the zeros of an empty sum; negative counts are
 * FEAR_TRAIN_ERR_SHAPE.  (fear_bn_finalize takes no rows: count < 1 is FEAR_TRAIN_ERR_SHAPE.) */
/* nn.Conv2d(K, N, 1): y[m][n] = sum_k x[m][k] w[n][k] (+ bias[n]); K, N multiples of 4 (v_mfma_f32_16x16x4_f32) */
int fear_pw_forward(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, long M, int K, int N,
                    void* stream);
/* its input gradient dx[m][k] = (add ? add[m][k] : 0) + sum_n dy[m][n] w[n][k] */
int fear_pw_backward_data(const float* dy, int lddy, const float* w, const float* add, int ldadd, float* dx, int lddx, long M,
                          int K, int N, void* stream);
/* its weight gradient dw[n][k] = sum_m dy[m][n] x[m][k] (MFMA, reduction over the rows); N, K, lddy, ldx multiples of 4 */
int fear_pw_backward_weight(const float* dy, int lddy, const float* x, int ldx, float* dw, float* workspace, size_t ws_bytes,
                            long M, int K, int N, void* stream);
/* bias gradients: out[c] = sum_m dy[m][c] */
int fear_col_sum(const float* dy, int lddy, float* out, float* workspace, size_t ws_bytes, long M, int C, void* stream);

/* nn.Conv2d(C, C, k, groups=C, padding=k/2, stride=stride), k in {3,5}, stride in {1,2}: taps laid out [k*k][C] (tap-major) */
int fear_dw_forward(const float* x, int ldx, const float* w_taps, const float* bias, float* y, int ldy, int B, int H, int W,
                    int C, int k, int stride, void* stream);
/* input gradient (B, H, W = the INPUT map; dy is the (H/stride, W/stride) output-side gradient) */
int fear_dw_backward_data(const float* dy, int lddy, const float* w_taps, float* dx, int lddx, int B, int H, int W, int C, int k,
                          int stride, void* stream);
/* weight gradient dw_taps[t][c] = sum_{b,oy,ox} dy[b,oy,ox,c] * x[b, oy*stride+ky-k/2, ox*stride+kx-k/2, c] */
int fear_dw_backward_weight(const float* dy, int lddy, const float* x, int ldx, float* dw_taps, float* workspace,
                            size_t ws_bytes, int B, int H, int W, int C, int k, int stride, void* stream);

/* stem conv 3x3 stride 2 pad 1 (3 -> 16) as a GEMM: im2col of an NCHW image batch into rows of 28 floats
 * (k = (ci*3+ky)*3+kx, column 27 zero) -> fear_pw_forward / fear_pw_backward_weight with K = 28 */
int fear_stem_im2col(const float* x_nchw, float* rows28, long n, int H, int W, void* stream);

/* nn.BatchNorm2d(C) in training mode (+ optional ReLU): batch statistics over the M rows; mean / rstd are saved for the
 * backward; running_mean / running_var (may be NULL) follow torch: (1 - momentum) * running + momentum * stat, unbiased var */
int fear_bn_train_forward(const float* x, int ldx, const float* gamma, const float* beta, float* y, int ldy, float* mean,
                          float* rstd, float* running_mean, float* running_var, double momentum, double eps, long M, int C,
                          int relu, float* workspace, size_t ws_bytes, void* stream);
/* backward through (ReLU o BatchNorm): y_act = the forward output when a ReLU followed (its mask), else NULL */
int fear_bn_train_backward(const float* dy, int lddy, const float* y_act, int ldy, const float* x, int ldx, const float* mean,
                           const float* rstd, const float* gamma, float* dx, int lddx, float* dgamma, float* dbeta, long M,
                           int C, float* workspace, size_t ws_bytes, void* stream);

/* SyncBatchNorm (the reference's multi-GPU backends train with sync_bn: True, config/backend/{2,4}gpu.yaml -> trainer.py:52):
 * the same BatchNorm with its two reductions exposed, so that the ranks can add their float64 sums ([2][C] doubles on the
 * device: forward sum x | sum x^2, backward sum g | sum g * xhat with g = the ReLU-masked dy) with one all-reduce each:
 *   forward : fear_bn_reduce -> all-reduce(sums) -> fear_bn_forward_from_sums(count = rows of all ranks)
 *   backward: fear_bn_backward_reduce -> copy = local sums, all-reduce(sums) -> fear_bn_backward_from_sums
 * d gamma / d beta come from the LOCAL sums (they are averaged with every other gradient), dx from the global ones — the
 * split torch.nn.SyncBatchNorm makes.  With one rank the pair equals fear_bn_train_forward / _backward. */
int fear_bn_reduce(const float* x, int ldx, double* sums, long M, int C, float* workspace, size_t ws_bytes, void* stream);
int fear_bn_forward_from_sums(const float* x, int ldx, const double* sums, double count, const float* gamma, const float* beta,
                              float* y, int ldy, float* mean, float* rstd, float* running_mean, float* running_var,
                              double momentum, double eps, long M, int C, int relu, void* stream);
int fear_bn_backward_reduce(const float* dy, int lddy, const float* y_act, int ldy, const float* x, int ldx, const float* mean,
                            const float* rstd, double* sums, long M, int C, float* workspace, size_t ws_bytes, void* stream);
int fear_bn_backward_from_sums(const float* dy, int lddy, const float* y_act, int ldy, const float* x, int ldx, const float* mean,
                               const float* rstd, const float* gamma, const double* sums_all, double count,
                               const double* sums_local, float* dx, int lddx, float* dgamma, float* dbeta, float* workspace,
                               size_t ws_bytes, long M, int C, void* stream);

/* ---- fused conv + BatchNorm training operators (the trunk's step; model/blocks.py:27-35 over mobile_cv's conv-BN-ReLU units) ----
 * A BatchNorm'd activation is never written out.  A PRODUCER writes the convolution's raw output y and, from the same pass, the
 * float64 column sums of it (sums = [2][C]: sum y | sum y^2 — exactly what SyncBatchNorm all-reduces); fear_bn_finalize turns the
 * (possibly all-reduced) sums into mean / rstd / running statistics and the affine a = gamma * rstd, b = beta - mean * a; every
 * CONSUMER applies act(x) = fma(x, a, b) [then max(., 0)] to the raw tensor as it loads it: in_a / in_b / in_relu below (in_a = NULL:
 * the input is used as it is).  The ReLU mask of the backward is recomputed from the raw tensor with the same expression, so the
 * forward and the backward agree bit for bit on which elements are active.  Zero padding of a depthwise conv pads the
 * ACTIVATION (stays zero).  fear_bn_act materialises act(x) [+ residual] where a tensor is needed (block outputs).
 * Against the unfused operators above: 11 instead of 16 passes over every saved tensor, half the saved memory. */
int fear_pw_forward_stats(const float* x, int ldx, const float* in_a, const float* in_b, int in_relu, const float* w, float* y,
                          int ldy, long M, int K, int N, double* sums, float* workspace, size_t ws_bytes, void* stream);
int fear_dw_forward_stats(const float* x, int ldx, const float* in_a, const float* in_b, int in_relu, const float* w_taps, float* y,
                          int ldy, int B, int H, int W, int C, int k, int stride, double* sums, float* workspace, size_t ws_bytes,
                          void* stream);
/* bytes of workspace the two producers need for `rows` output rows of `channels` channels (partial sums per workgroup).  The depthwise
 * producer deals one thread a strip of four output rows: for maps of ONE output row with rows x channels / 4 > 32 768 it launches more
 * workgroups than this allows for and returns FEAR_TRAIN_ERR_WORKSPACE before launching anything; it then needs
 * ceil(B * ceil(Ho / 4) * Wo * (C / 4) / 256) * 2 * C doubles (tests/test_train_layer_ops_gpu.py pins both). */
size_t fear_train_stats_workspace_bytes(long rows, int channels);
int fear_bn_finalize(const double* sums, double count, const float* gamma, const float* beta, float* mean, float* rstd, float* a_out,
                     float* b_out, float* running_mean, float* running_var, double momentum, double eps, int C, void* stream);
int fear_bn_act(const float* x, int ldx, const float* a, const float* b, int relu, const float* residual, int ldr, float* y, int ldy,
                long M, int C, void* stream);
/* backward through (ReLU? o BatchNorm) of a raw tensor x: sums = [2][C] float64 (sum g | sum g * xhat, g = dy where act(x) > 0 when
 * relu); then dx from the (all ranks') sums and row count, d gamma / d beta from the local sums — the split of
 * fear_bn_backward_reduce / _from_sums above, with the mask taken from x instead of a stored activation */
int fear_bn_backward_reduce_x(const float* dy, int lddy, const float* x, int ldx, const float* act_a, const float* act_b, int relu,
                              const float* mean, const float* rstd, double* sums, long M, int C, float* workspace, size_t ws_bytes,
                              void* stream);
int fear_bn_backward_apply_x(const float* dy, int lddy, const float* x, int ldx, const float* act_a, const float* act_b, int relu,
                             const float* mean, const float* rstd, const float* gamma, const double* sums_all, double count,
                             const double* sums_local, float* dx, int lddx, float* dgamma, float* dbeta, float* workspace,
                             size_t ws_bytes, long M, int C, void* stream);
/* the layer-wise step's BatchNorm in the same affine form, activation written out (y = act(x) [+ residual]), and its backward with
 * the ReLU mask recomputed from x — the stored activation is not read on the way back; three launches each, one rank */
int fear_bn_train_forward_ab(const float* x, int ldx, const float* gamma, const float* beta, int relu, const float* residual, int ldr,
                             float* y, int ldy, float* mean, float* rstd, float* a_out, float* b_out, float* running_mean,
                             float* running_var, double momentum, double eps, long M, int C, float* workspace, size_t ws_bytes,
                             void* stream);
int fear_bn_train_backward_x(const float* dy, int lddy, const float* x, int ldx, const float* act_a, const float* act_b, int relu,
                             const float* mean, const float* rstd, const float* gamma, float* dx, int lddx, float* dgamma, float* dbeta,
                             long M, int C, float* workspace, size_t ws_bytes, void* stream);
/* weight gradients whose x operand is act(raw x) applied on load */
int fear_pw_backward_weight_act(const float* dy, int lddy, const float* x, int ldx, const float* in_a, const float* in_b, int in_relu,
                                float* dw, float* workspace, size_t ws_bytes, long M, int K, int N, void* stream);
int fear_dw_backward_weight_act(const float* dy, int lddy, const float* x, int ldx, const float* in_a, const float* in_b, int in_relu,
                                float* dw_taps, float* workspace, size_t ws_bytes, int B, int H, int W, int C, int k, int stride,
                                void* stream);

/* MobileCorrelation (blocks.py:121-123): s[b][p][j] = sum_c x[b][p][c] z[b][c][j]; z_nchw = (B, C, J) as the reference holds it.
 * Both directions return FEAR_TRAIN_ERR_SHAPE before anything is launched unless C >= 4, J >= 4, C % 4 == J % 4 == 0 and every
 * leading dimension is a multiple of 4 floats that covers its row (ldx >= C, lds / ldds >= J, lddx >= C, ldadd >= C where
 * dx_add is given): rows are read and written as float4s.  P % 32 == 0 forward (a wave's 32 rows share one crop's z),
 * P % 128 == 0 backward (a 128-row tile must not straddle crops).  s_out may be columns of x's own buffer past column C. */
int fear_xcorr_forward(const float* x, int ldx, const float* z_nchw, float* s_out, int lds, int B, int P, int C, int J,
                       void* stream);
/* dx[b][p][c] = (dx_add ? dx_add[b][p][c] : 0) + sum_j ds[b][p][j] z[b][c][j];   dz[b][c][j] = sum_p x[b][p][c] ds[b][p][j] */
int fear_xcorr_backward(const float* ds, int ldds, const float* x, int ldx, const float* z_nchw, const float* dx_add, int ldadd,
                        float* dx, int lddx, float* dz_nchw, int B, int P, int C, int J, void* stream);

/* bbox = exp(adjust * p + bias[c]) on rows of 4 (blocks.py:186-187), and its backward (dp, d adjust, d bias) */
int fear_exp_head_forward(const float* p, const float* adjust, const float* bias4, float* bbox, long M, void* stream);
int fear_exp_head_backward(const float* p, const float* adjust, const float* bbox, const float* dbbox, float* dp, float* dadjust,
                           float* dbias4, float* workspace, size_t ws_bytes, long M, void* stream);

/* FEARLoss forward + gradient (train/loss.py:45-96): bbox / gt_reg rows of 4 (ltrb), cls / gt_cls / gt_weight one value per row.
 * losses2 = {classification, regression} (each times its coefficient); dbbox / dcls = d(sum of both) / d(bbox, cls).
 * Selections of one or no cell: the reference indexes with `label.eq(1).nonzero().squeeze()` (loss.py:77-78), so exactly ONE
 * positive (or one negative) cell makes `_weighted_cls_loss` return a constant 0 for that half — mirrored: no loss, no gradient.
 * With NO positive / negative / weighted cell torch yields NaN (mean over nothing); this operator yields 0 for that term — the
 * one deliberate deviation (a NaN would poison the all-reduced gradient buffer of every rank).                                */
int fear_head_loss(const float* bbox, const float* cls, const float* gt_reg, const float* gt_cls, const float* gt_weight,
                   float coef_cls, float coef_reg, float* losses2, float* dbbox, float* dcls, float* workspace, size_t ws_bytes,
                   long M, void* stream);

/* boundary layout changes (the reference's tensors are NCHW): out[(b*HW + p)*ld_out + ch_off + c] = in[(b*C + c)*HW + p], and back */
int fear_nchw_to_nhwc(const float* in, float* out, long n, int C, int HW, int ld_out, int ch_off, void* stream);
int fear_nhwc_to_nchw(const float* in, float* out, long n, int C, int HW, int ld_in, int ch_off, void* stream);

/* out[m*ld_out + col_out] = scale * in[m*ld_in + col_in]  (cls = 0.1 * cls_pred(c), blocks.py:192, forward and backward) */
int fear_scale_column(const float* in, int ld_in, int col_in, float scale, float* out, int ld_out, int col_out, long M,
                      void* stream);
/* out = a + b over n floats: gradient accumulation where the two branches of the head meet */
int fear_add(const float* a, const float* b, float* out, long n, void* stream);

/* One torch.optim.Adam update (no amsgrad; weight_decay is the L2 form added to the gradient) of n parameters in place — the
 * reference's optimiser is Adam(lr = 1e-4) (train/base_lightning_model.py:63-64).  `step` counts from 1 (bias corrections
 * 1 - beta^step are taken in double on the host, like torch's Python scalars); exp_avg / exp_avg_sq start at zero. */
int fear_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, double lr, double beta1, double beta2,
                   double eps, double weight_decay, int step, void* stream);

/* ---- the optimiser family and gradient-norm clipping (csrc/fear_train_optim.h) ---------------------------------------------------
 * The reference's config/optimizer/{adam,adamw,sgd}.yaml and `gradient_clip_val` (train/trainer.py:59: Lightning's clip_grad_norm_
 * over all parameters) on flat fp32 buffers, without a host round trip: sum of squares -> norm and coefficient -> update.
 *
 * The 2-norm in a fixed order: each workgroup adds the squares of one chunk of FEAR_GRAD_SUMSQ_CHUNK consecutive floats in float64
 * (16-byte loads from the first 16-byte boundary on, the head and the tail scalar) and writes one partial; the count of partials for n
 * elements comes from the first function (0 for n <= 0).  No floating-point atomics: the same input gives the same bits.  `grad`
 * must be 4-byte aligned. */
#define FEAR_GRAD_SUMSQ_CHUNK 4096
long fear_grad_sumsq_partials(long n);
int fear_grad_sumsq(const float* grad, long n, double* partials, void* stream);
/* One workgroup adds `count` partials in a fixed order — they may come from several sum-of-squares calls that wrote consecutive
 * ranges (a model updated tensor by tensor) — and writes out2[0] = norm = (float)sqrt(sum) and out2[1] = the clipping coefficient
 * min(1, max_norm / (norm + 1e-6)) in fp32, as torch.nn.utils.clip_grad_norm_(norm_type = 2) forms it (the reciprocal of the fp32
 * sum, times max_norm); max_norm <= 0 writes 1.
 * A non-finite norm gives a NaN coefficient, as in torch. */
int fear_grad_norm_finalize(const double* partials, long count, double max_norm, float* out2, void* stream);

#define FEAR_OPT_ADAM 0
#define FEAR_OPT_ADAMW 1
#define FEAR_OPT_SGD 2
typedef struct {
    int kind;                 /* FEAR_OPT_ADAM | FEAR_OPT_ADAMW | FEAR_OPT_SGD */
    int nesterov;             /* SGD */
    double lr, beta1, beta2, eps, weight_decay, momentum, dampening;
} FearOptim;
/* One update of n parameters in place by torch.optim.Adam / AdamW / SGD's rule (no amsgrad; the fp32 operations in torch's
 * order; scalars formed in double on the host).  `step` counts from 1.  `clip_coef`: device pointer to the coefficient (out2 + 1
 * above) or NULL; the kernel forms g = grad * coef in a register and does NOT write the gradient buffer (torch scales it in place).
 *   ADAM    as fear_adam_step: state1 = exp_avg, state2 = exp_avg_sq (same bits with clip_coef NULL)
 *   ADAMW   p *= 1 - lr * weight_decay, then Adam without the L2 term
 *   SGD     g += weight_decay * p; buf = g at step 1, else momentum * buf + (1 - dampening) * g; g = g + momentum * buf with
 *           nesterov, else buf; p -= lr * g.  state1 = the momentum buffer (may be NULL when momentum == 0), state2 unused.
 * FEAR_TRAIN_ERR_SHAPE, before anything is launched: an unknown kind, step < 1, n < 0, betas outside [0, 1), momentum < 0, nesterov
 * with momentum <= 0 or dampening != 0 (torch's rule); FEAR_TRAIN_ERR_NULL: a missing descriptor, parameter, gradient or required
 * state.  Four elements per lane where all bases are 16-byte aligned, element by element otherwise. */
int fear_optim_step(const FearOptim* o, float* param, const float* grad, float* state1, float* state2, long n, int step,
                    const float* clip_coef, void* stream);

/* ---- block-fused operators of the trunk's training step (round 5; csrc/fear_train_block.h) --------------------------------------
 * One call per inverted-residual block and direction — model_training/model/blocks.py:22-35 over mobile_cv's conv-BN-ReLU units:
 * expand 1x1 + BN + ReLU (absent when `expand` = 0: cexp = cin), depthwise kxk stride s + BN + ReLU, project 1x1 + BN [+ input when
 * `residual`].  The call sequences its kernels itself; BatchNorm'd activations, BatchNorm input gradients and ReLU masks are formed
 * in registers by whichever kernel needs them (forward: statistics in the producing pass, normalisation on load in the consumer;
 * backward: the BatchNorm backward applied on load from the pair (gradient, raw tensor)); what is written is the raw conv outputs
 * e / d / p (saved for the backward) and, in the backward, two masked gradients in `scratch`.  Same arithmetic as the operators
 * above composed unit by unit (tests/test_train_head.py pins both against autograd).  SyncBatchNorm: fear_train_sync_bind below. */
/* The expansion's backward without its raw output (e = x W1^T is linear in the block input: BatchNorm1's input gradient folds into
 * the two consumers' own algebra, a cin x cin matrix each — csrc/fear_train.hip BnbIn): chosen by the call where it pays (up to 32
 * input channels: the large maps); these flags force it wherever it applies (cexp % 16 == 0, cin <= 128) or forbid it. */
#define FEAR_IRB_LINEAR_BN1 1
#define FEAR_IRB_NO_LINEAR_BN1 2
/* ... and the expansion never written at all (FearIrbSaved.e may be NULL): the depthwise kernels of both directions form the channels
 * they own from the pixel's inputs on the spot, BatchNorm1's batch statistics come from the input's Gram matrix.  For the shapes
 * fear_irb_virtual_ok() accepts (16 ... 32 input channels, stride 2, cexp a multiple of 16 from 64 up — FEAR-XS's 16 -> 96 at 128 x 128
 * (0.8 GB per 128 crops), 24 -> 144 at 64 x 64, 32 -> 192 at 32 x 32); the same flag in the forward and the backward call. */
#define FEAR_IRB_VIRTUAL_E 4
/* blocks of at most 32 channels throughout: the projection's weight gradient is summed inside the masked-gradient pass that reads the
 * same three tensors (0.9 GB less traffic per 128-pair step; off by default: it lengthens the chain of input gradients, see
 * csrc/fear_train_block.h irb_w3g) */
#define FEAR_IRB_FUSE_W3 8
typedef struct FearIrbBlock {
    int cin, cexp, cout, k, stride, expand, residual;
    int flags;                     /* 0 = let the call choose; FEAR_IRB_LINEAR_BN1 / FEAR_IRB_NO_LINEAR_BN1 (below) */
    const float* w_pw;             /* [cexp][cin]   (NULL without expansion) */
    const float* w_dw;             /* [k*k][cexp]   depthwise taps, tap-major */
    const float* w_pwl;            /* [cout][cexp] */
    const float* gamma[3];         /* BatchNorm of the expand | depthwise | project unit ([0] unused without expansion) */
    const float* beta[3];
    float* running_mean[3];        /* updated by the forward like fear_bn_train_forward (may be NULL) */
    float* running_var[3];
} FearIrbBlock;
typedef struct FearIrbSaved {      /* written by the forward, read by the backward; caller-allocated */
    float* e;                      /* [B*H*W][cexp]            raw expansion (NULL without expansion) */
    float* d;                      /* [B*(H/s)*(W/s)][cexp]    raw depthwise output */
    float* p;                      /* [B*(H/s)*(W/s)][cout]    raw projection */
    float* vec[3];                 /* per BatchNorm 4*C floats: mean | rstd | a = gamma*rstd | b = beta - mean*a */
} FearIrbSaved;
typedef struct FearIrbGrads {      /* parameter gradients, kernel layouts of FearIrbBlock */
    float* w_pw;
    float* w_dw;
    float* w_pwl;
    float* gamma[3];
    float* beta[3];
} FearIrbGrads;
size_t fear_irb_workspace_bytes(const FearIrbBlock* blk, int B, int H, int W);     /* 0: unsupported shape */
int fear_irb_virtual_ok(const FearIrbBlock* blk);                                   /* 1: FEAR_IRB_VIRTUAL_E may be set for this block */
size_t fear_irb_scratch_floats(const FearIrbBlock* blk, int B, int H, int W);      /* `scratch` of the backward; it begins with the two
                                                                                       masked gradients, exact zeros where a ReLU is shut:
                                                                                       g2 [B*(H/s)*(W/s)][cexp], then with an expansion
                                                                                       g1 [B*H*W][cexp] */
/* x [B*H*W][cin] -> out [B*(H/s)*(W/s)][cout] */
int fear_irb_train_forward(const FearIrbBlock* blk, const FearIrbSaved* saved, const float* x, float* out, int B, int H, int W,
                           double momentum, double eps, float* workspace, size_t ws_bytes, void* stream);
/* dout = gradient w.r.t. `out`; dx (may be NULL when the block has an expansion and its input needs no gradient) = gradient w.r.t. x */
/* `wgrad_stream` (may be NULL = `stream`): the block's two pointwise weight gradients do not feed dx; given a second stream they are
 * issued there — ordered behind the kernels that produce their operands by events — and overlap the rest of the backward pass.  The
 * caller then keeps `scratch` private to this call, and makes whatever consumes the gradients (or reuses scratch / workspace / the
 * tensors handed in) wait for that stream. */
int fear_irb_train_backward(const FearIrbBlock* blk, const FearIrbSaved* saved, const FearIrbGrads* grads, const float* x, const float* dout,
                            float* dx, float* scratch, int B, int H, int W, float* workspace, size_t ws_bytes, void* stream,
                            void* wgrad_stream);
/* What the two calls above would launch for this block and shape — host only: nothing is launched and no device is needed.  The
 * kernels and grids are chosen from the row counts B*H*W and B*(H/s)*(W/s) (csrc/fear_train_block.h: gemm_lds_applies, stat_grid,
 * dgrad_grid, col_rows_per_block, wgrad_plan, dw_geom, gram_rows_per_wg); the query asks the same helpers the launches ask, so that a
 * test can state which of them its shapes reach (tests/test_train_block.py::test_cases_reach_the_paths_they_claim). */
typedef struct FearGemmPlan {      /* one row-tiled pointwise GEMM */
    int32_t present;               /* 0: the block has no such launch (every other field is 0) */
    int32_t lds;                   /* 1: the LDS-staged kernel (csrc/fear_train_gemm.h); 0: the first generation, on the grid below */
    int32_t rows, k, n;            /* rows, reduction length (both operands), output columns */
    int32_t x2;                    /* 1: the reduction runs over two operands (the E-free input gradient: [g1 | x]) */
    int32_t row_tiles;             /* first generation: 128-row tiles per workgroup */
    int32_t grid_x, grid_y, nt;    /* first generation: row blocks, column passes, 16-column tiles per pass */
} FearGemmPlan;
typedef struct FearWgradPlan {     /* one pointwise weight gradient dW[n][k] over `rows` rows */
    int32_t present;               /* 0: none; 1: a launch of its own; 2: summed inside another kernel's pass (FEAR_IRB_FUSE_W3 in the
                                      masked-gradient GEMM; a virtual 3 x 3 expansion's in the depthwise backward): `slices` partials */
    int32_t rows, k, n;
    int32_t swapped, lds_tile;     /* the kernel variant: operands traded / 128 x 128 tiles staged through LDS */
    int32_t rows_per_slice, slices;
} FearWgradPlan;
typedef struct FearDwPlan {        /* one depthwise launch: persistent workgroups walk tiles of the map */
    int32_t tiles_x, tiles_y, tile_side, nslab, wgs_per_slab;
    int32_t items_per_wg;          /* the most tiles a workgroup walks */
    int32_t small_map;             /* 1: the 8 x 8-tile kernel of the 5 x 5 stride-1 blocks on maps of at most 8 x 8 */
} FearDwPlan;
typedef struct FearIrbPlanInfo {
    int32_t rows_in, rows_out;
    int32_t lin, virtual_e;        /* BatchNorm1's backward in the E-free form / the expansion never written */
    FearGemmPlan expand, project;  /* forward (expand: absent without an expansion or with a virtual one) */
    FearGemmPlan g2, dx;           /* backward: the masked gradient; the input gradient of an expansion (what a non-NULL dx launches) */
    int32_t col_rows_in, col_rows_out;      /* rows per column-reduction workgroup at either row count (the block's own column
                                               reduction, BatchNorm3's backward sums, runs over rows_out) */
    int32_t wgrad_rows_per_slice;  /* the coarse weight-gradient slice the workspace is sized by; a launch may cut finer: w3, w1 */
    FearWgradPlan w3, w1;          /* the projection's / the expansion's weight gradient */
    FearDwPlan dw_fwd, dw_bwd;
    int32_t gram_rows_per_wg;      /* rows per workgroup of the input's Gram matrix (virtual forward; E-free backward up to 32 input
                                      channels); 0: no such launch */
} FearIrbPlanInfo;
int fear_irb_plan_info(const FearIrbBlock* blk, int B, int H, int W, FearIrbPlanInfo* out);
/* ... and of fear_pwbn_train_* over M rows, or (stem = 1: K = 28, N = 16, relu = 1) of fear_stem_train_* over M = n*(H/2)*(W/2) rows */
typedef struct FearPwbnPlanInfo {
    int32_t rows;
    FearGemmPlan forward, dx;      /* (dx: what a non-NULL dx launches; absent for the stem) */
    int32_t col_rows;
    FearWgradPlan w;
} FearPwbnPlanInfo;
int fear_pwbn_plan_info(long M, int K, int N, int relu, int stem, FearPwbnPlanInfo* out);
/* ... and of the layer operators at the top of this file (fear_pw_forward ... fear_dw_backward_weight_act) for M rows, K input and N
 * output channels — and, when `dw` is given, for one depthwise shape.  Host only; a record of its own (FearGemmPlan's layout is held by
 * the block tests).  tests/test_train_layer_ops_gpu.py::test_cases_reach_the_branches_they_claim holds every case of that file to it. */
typedef struct FearLayerGemmPlan {     /* fear_pw_forward (reduction K, N columns) or fear_pw_backward_data (reduction N, K columns) */
    int32_t lds;                       /* 1: gemm_lds_kernel (csrc/fear_train_gemm.h); 0: the first generation, pw_mfma_kernel */
    int32_t row_tile, ntw, col_blocks; /* LDS: rows per workgroup (64 or 128), 16-column tiles per workgroup, column blocks (gridDim.y) */
    int32_t grid_x, grid_y, nt;        /* first generation: row workgroups, column passes dealt over gridDim.y, tiles per pass */
} FearLayerGemmPlan;
typedef struct FearLayerWgradPlan {    /* fear_pw_backward_weight[_act] with `ws_bytes` of workspace */
    int32_t swapped, lds_tile;         /* operands traded (narrow dY) / 128 x 128 tiles staged through LDS */
    int32_t small_k;                   /* 16-column k-blocks of pw_wgrad_smallk_kernel (1 or 2); 0: a 64 x 64 or staged tile */
    int32_t n_tiles, k_tiles, rows_per_slice, slices;
} FearLayerWgradPlan;
typedef struct FearLayerDwShape { int32_t B, H, W, C, k, stride, ld; } FearLayerDwShape;      /* ld: pitch of x (forward), of dy (input gradient) */
typedef struct FearLayerDwPlan {
    int32_t strips, workgroups;        /* forward and _stats: 4-row strips per image column, workgroups (= partial rows of _stats) */
    int32_t dgrad_workgroups;
    int32_t wgrad_rows, wgrad_workgroups, wgrad_row_run;      /* output pixels per workgroup, workgroups, 1: runs of T pixels (Wo % T == 0) */
    int32_t fwd_plain, dgrad_plain;    /* 1: the tensor's span reaches 2^31 bytes, plain loads instead of buffer loads */
} FearLayerDwPlan;
typedef struct FearLayerPlanInfo {
    FearLayerGemmPlan forward, dx;
    int32_t stats_blocks, stats_nt;    /* fear_pw_forward_stats: workgroups (partial rows), tiles per pass */
    FearLayerWgradPlan w, w_act;
    int32_t col_rows, col_blocks;      /* the column reductions over M rows: rows per workgroup, workgroups */
    FearLayerDwPlan dw;                /* zeros without `dw` */
} FearLayerPlanInfo;
int fear_layer_plan_info(long M, int K, int N, size_t ws_bytes, const FearLayerDwShape* dw, FearLayerPlanInfo* out);
/* The running statistics of one BatchNorm from the `vec` its forward saved (mean | rstd | a | b), for forwards that ran with
 * running_mean = NULL: the shared trunk's two passes (template, search: model/fear_net.py:83-88) may then overlap on two streams,
 * and torch's update order — template pass first — is restored by applying the search pass's update afterwards. */
int fear_bn_running_update(const float* vec, double count, float* running_mean, float* running_var, double momentum, double eps, int C,
                           void* stream);
/* ... for a whole pass's BatchNorms in ONE launch (n items; the search pass's 47 deferred updates were 47 launches) */
typedef struct FearBnRunning { const float* vec; float* running_mean; float* running_var; int C; double count; } FearBnRunning;
int fear_bn_running_update_multi(const FearBnRunning* items, int n, double momentum, double eps, void* stream);
/* a lone pointwise conv + BatchNorm [+ ReLU] in the same style (the stem on its im2col rows, the AdjustLayer neck blocks.py:75-88):
 * raw = x w^T, vec as above, out = act(raw) materialised;  backward from dy = gradient w.r.t. out */
size_t fear_pwbn_workspace_bytes(long M, int K, int N);
int fear_pwbn_train_forward(const float* x, int ldx, const float* w, const float* gamma, const float* beta, float* running_mean,
                            float* running_var, float* raw, float* vec, int relu, float* out, long M, int K, int N, double momentum, double eps,
                            float* workspace, size_t ws_bytes, void* stream);
int fear_pwbn_train_backward(const float* dy, const float* raw, const float* vec, int relu, const float* x, int ldx, const float* w,
                             const float* gamma, float* dw, float* dgamma, float* dbeta, float* dx, long M, int K, int N, float* workspace,
                             size_t ws_bytes, void* stream, void* wgrad_stream);

/* the stem (3x3 stride-2 conv 3 -> 16 + BatchNorm + ReLU: the FBNet-C first stage behind model/fear_net.py:83-88) on the NCHW image —
 * fear_pwbn_train_* over fear_stem_im2col's rows without ever materialising them (w [16][28]: k = (ci*3 + ky)*3 + kx, column 27 = 0;
 * raw, out [n*(H/2)*(W/2)][16]; the image needs no gradient) */
size_t fear_stem_workspace_bytes(long n, int H, int W);
int fear_stem_train_forward(const float* x_nchw, const float* w, const float* gamma, const float* beta, float* running_mean,
                            float* running_var, float* raw, float* vec, float* out, long n, int H, int W, double momentum, double eps,
                            float* workspace, size_t ws_bytes, void* stream);
int fear_stem_train_backward(const float* dy, const float* raw, const float* vec, const float* x_nchw, const float* gamma, float* dw,
                             float* dgamma, float* dbeta, long n, int H, int W, float* workspace, size_t ws_bytes, void* stream,
                             void* wgrad_stream);

/* ---- SyncBatchNorm for the block-fused operators (round 6) -----------------------------------------------------------------------
 * The reference's multi-GPU backends train with `sync_bn: True` (model_training/config/backend/2gpu.yaml:5, 4gpu.yaml:5 ->
 * train/trainer.py:50-52).  In fear_irb_train_* / fear_pwbn_train_* / fear_stem_train_* / fear_sepbn_train_* a BatchNorm's two
 * reductions sit INSIDE one call (producer -> float64 column sums -> finalize -> consumer), so the ranks' all-reduce is a hook:
 * a stream is bound to a FearSync, and every BatchNorm finalize enqueued on that stream becomes
 *     local float64 sums [2][C] -> sync.buf        (forward: sum y | sum y^2;  backward: sum g | sum g * xhat, with d gamma / d beta
 *                                                    taken from the LOCAL sums — they are averaged with every other gradient)
 *     sync.all_reduce(user, buf, 2 C, 0, stream)   the caller's collective (RCCL through torch.distributed in feartracker_amd/train_net.py),
 *                                                    in place, ordered on `stream`; returns 0 on success
 *     finalize from the summed buffer with count = local rows * sync.world
 * (a virtual expansion's BatchNorm1 — statistics from the input's Gram matrix — all-reduces that fp32 matrix instead: is_f32 = 1).
 * Every rank must enqueue the same sequence of operators with the same row counts (DDP's equal batches), and a FearSync serves ONE
 * stream: two passes on two streams bind two of them (two buffers); their collectives then reach the communicator in the host's
 * issue order, which is the same on every rank.  Streams without a binding run the one-rank form; with world = 1 the bound form gives
 * the same numbers bit for bit.  Binding copies *sync; NULL unbinds.  At most 16 streams are bound at a time. */
typedef int (*fear_allreduce_fn)(void* user, void* buf, long n, int is_f32, void* stream);
typedef struct FearSync {
    fear_allreduce_fn all_reduce;
    void* user;
    double* buf;                   /* device scratch of this binding alone, >= FEAR_SYNC_BUF_BYTES */
    size_t buf_bytes;
    int world;                     /* ranks of the group (>= 1) */
} FearSync;
#define FEAR_SYNC_BUF_BYTES 16384  /* 2 x 1024 channels x 8 bytes */
int fear_train_sync_bind(void* stream, const FearSync* sync);

/* SepConv (depthwise 3x3 + pointwise, both with bias) + BatchNorm + ReLU: the layer of the head's encoders and towers
 * (SepConv + BatchNorm2d + ReLU: model_training/model/blocks.py:97-101 MatrixMobile, :115-119 MobileCorrelation, :151-161 BoxTower's towers), one call per direction.  Kernel layouts: depthwise taps
 * [9][cin], pointwise [cout][cin].  The pointwise bias sits in front of the BatchNorm: it cancels in the normalisation (its gradient
 * and the depthwise bias's are exactly zero and are not written) and only shifts the tracked running mean — `raw` is saved without it. */
typedef struct FearSepLayer {
    int cin, cout;
    const float* w_dw;  const float* b_dw;        /* b_dw, b_pw may be NULL */
    const float* w_pw;  const float* b_pw;
    const float* gamma; const float* beta;
    float* running_mean; float* running_var;      /* may be NULL: not tracked by this call */
} FearSepLayer;
typedef struct FearSepGrads { float* w_dw; float* w_pw; float* gamma; float* beta; } FearSepGrads;
size_t fear_sepbn_workspace_bytes(const FearSepLayer* layer, int B, int H, int W);      /* 0: unsupported shape */
/* x [B*H*W][ldx] -> saved d [M][cin], raw [M][cout], vec [4*cout] (mean | rstd | a | b) and out [M][ldo] = relu(a raw + b) */
int fear_sepbn_train_forward(const FearSepLayer* layer, const float* x, int ldx, float* d, float* raw, float* vec, float* out, int ldo,
                             int B, int H, int W, double momentum, double eps, float* workspace, size_t ws_bytes, void* stream);
/* dy [M][cout] = gradient w.r.t. out -> dx [M][cin] and the four parameter gradients.  `dd` [M][cin] (the depthwise output's gradient)
 * and `coef` [4*cout] are scratch PRIVATE to this call.  `wgrad_stream` (may be NULL = `stream`): the two weight gradients do not feed
 * dx; given a second stream they are issued there, ordered behind the kernels that produce their operands.  The caller then makes
 * whatever consumes the gradients — or reuses dd / coef / the tensors handed in — wait for that stream, and hands every call that
 * shares this workspace the same weight-gradient stream (its partial sums live there). */
int fear_sepbn_train_backward(const FearSepLayer* layer, const FearSepGrads* grads, const float* x, int ldx, const float* d,
                              const float* raw, const float* vec, const float* dy, float* dd, float* coef, float* dx, int B, int H,
                              int W, float* workspace, size_t ws_bytes, void* stream, void* wgrad_stream);

/* ---- training pairs from frames: the data stage in front of the step (feartracker_amd/train_data.py) ----
 * SiameseTrackingDataset._transform of the reference (model_training/dataset/siam_dataset.py:33-61) for a batch of pairs, with the
 * scalar per-pair work (context boxes, jitter, the moved box, the inverse warp, the colour lookup tables) done on the host and
 * handed in as one FearPairGeom per pair.  Frames are fear_frame (include/fear_hip.h): uint8 RGB (h, w, 3), any sizes. */
#define FEAR_TP_TEMPLATE 128    /* template crop side                                        */
#define FEAR_TP_CONTEXT 512     /* stage-1 search crop side (get_extended_crop, 2 x search)  */
#define FEAR_TP_SEARCH 256      /* search crop side after the jitter warp                     */
#define FEAR_TP_SCORE 16        /* target map side; cell centres (k - 8) * 16 + 128           */

/* One pair.  96 bytes, no padding. */
typedef struct FearPairGeom {
    int32_t t_frame, s_frame;   /* frame-table indices of the template and the search frame; outside [0, n_frames): all-zero crop */
    int32_t t_ctx[4];           /* template context box x, y, w, h in frame pixels (extend_bbox(box, 0.2); may leave the frame)   */
    int32_t s_ctx[4];           /* search context box, resized to the 512 x 512 stage-1 crop                                        */
    int32_t box[4];             /* search_bbox inside the 256 x 256 search crop, xywh (the targets are encoded from it)            */
    int32_t presence;           /* 0: gt_reg, gt_cls, gt_weight are zeros                                                           */
    int32_t tone;               /* 0 none, 1 gray (cv2 RGB2GRAY), 2 sepia (albumentations ToSepia)                                  */
    double inv[4];              /* inverse warp 512 -> 256 (cv2.warpAffine's inverted matrix): x_src = inv[0] x + inv[1],
                                   y_src = inv[2] y + inv[3]                                                                        */
} FearPairGeom;
#ifdef __cplusplus
static_assert(sizeof(FearPairGeom) == 96, "FearPairGeom is 96 bytes");
#else
_Static_assert(sizeof(FearPairGeom) == 96, "FearPairGeom is 96 bytes");
#endif

/* The frames' mean colours as cv2.copyMakeBorder writes them: per frame exact integer channel sums, then sum / (h w) in double,
 * rounded half to even and saturated (border_color_u8(np.mean(frame, (0, 1))) bit for bit).  One launch for all frames.  A frame
 * with no pixels (null data, h or w < 1) gets (0, 0, 0).
 *   frames : (n_frames) fear_frame, device     out_rgb_u8 : (n_frames, 3) uint8, device                                         */
int fear_frame_border_u8(const fear_frame* frames, int n_frames, uint8_t* out_rgb_u8, void* stream);

/* Template crop, search crop and targets of n pairs (one launch):
 *   template_out (n, 3, 128, 128) : get_extended_crop of frames[t_frame] (border border_rgb[t_frame]) -> colour -> normalise
 *   search_out   (n, 3, 256, 256) : get_extended_crop of frames[s_frame] to 512 (computed per tap, never stored) -> cv2.warpAffine
 *                                   INTER_LINEAR, BORDER_CONSTANT 0 (10-bit AB, 5-bit table, 15-bit weights) -> colour -> normalise
 *   gt_reg (n, 4, 16, 16), gt_cls (n, 1, 16, 16), gt_weight (n, 16, 16) : FEARBoxCoder.encode / get_regression_weight_label(r_pos 2)
 * The colour stage acts on a pixel's uint8 RGB: the pair's tone (gray / sepia), then lut[pair][channel][value].  Normalisation is
 * fear_normalize_u8's (px - 255 mean) * (1 / (255 std)), fp32 NCHW.  All outputs are fp32.
 *   frames : (n_frames) fear_frame, device     border_rgb : (n_frames, 3) uint8, device (fear_frame_border_u8)
 *   geom : (n) FearPairGeom, device            lut : (n, 3, 256) uint8, device                                                   */
int fear_train_pairs(const fear_frame* frames, int n_frames, const uint8_t* border_rgb, const FearPairGeom* geom, const uint8_t* lut,
                     int n, float* template_out, float* search_out, float* gt_reg, float* gt_cls, float* gt_weight, void* stream);

/* fear_train_pairs with the crops left as the colour stage made them — after the tone and the lookup table, before the normalisation —
 * as uint8 HWC, the input of fear_photometric_u8.  The same kernel body with another store policy; the targets are fear_train_pairs'.
 *   template_u8 (n, 128, 128, 3), search_u8 (n, 256, 256, 3) uint8, device                                                          */
int fear_train_pairs_u8(const fear_frame* frames, int n_frames, const uint8_t* border_rgb, const FearPairGeom* geom, const uint8_t* lut,
                        int n, uint8_t* template_u8, uint8_t* search_u8, float* gt_reg, float* gt_cls, float* gt_weight, void* stream);

/* fear_train_pairs and fear_train_pairs_u8 for frames of which only a rectangle is stored (JpegStore.decode_windows): the same kernel
 * body with another frame-fetch policy.  `h`, `w` stay the FRAME's shape, so the inside / outside-the-frame test and the border colour
 * are unchanged; a pixel (x, y) inside the frame is read at data[((y - y0) ww + (x - x0)) 3], with y - y0 clamped to [0, wh) and
 * x - x0 to [0, ww): a window that does not cover what the pairs read gives wrong pixels, never a read outside its wh ww 3 bytes.  A
 * window without pixels (null data, wh or ww < 1) reads as the border colour.  The checks are fear_train_pairs'.
 *   windows : (n_frames) fear_frame_window, device                                                                                  */
typedef struct fear_frame_window {
    const uint8_t* data;        /* device: contiguous (wh, ww, 3) uint8, the frame's pixels [y0, y0 + wh) x [x0, x0 + ww)            */
    int32_t h, w;               /* the frame's shape                                                                                */
    int32_t y0, x0;             /* the frame coordinates of the window's first pixel                                                */
    int32_t wh, ww;             /* the window's shape                                                                               */
} fear_frame_window;
#ifdef __cplusplus
static_assert(sizeof(fear_frame_window) == 32, "fear_frame_window is 32 bytes");
#else
_Static_assert(sizeof(fear_frame_window) == 32, "fear_frame_window is 32 bytes");
#endif
int fear_train_pairs_windows(const fear_frame_window* windows, int n_frames, const uint8_t* border_rgb, const FearPairGeom* geom,
                             const uint8_t* lut, int n, float* template_out, float* search_out, float* gt_reg, float* gt_cls,
                             float* gt_weight, void* stream);
int fear_train_pairs_windows_u8(const fear_frame_window* windows, int n_frames, const uint8_t* border_rgb, const FearPairGeom* geom,
                                const uint8_t* lut, int n, uint8_t* template_u8, uint8_t* search_u8, float* gt_reg, float* gt_cls,
                                float* gt_weight, void* stream);

/* ---- the photometric stage: PHOTOMETRIC_AUGMENTATIONS of the reference (model_training/dataset/aug.py:8-25) on each crop on its
 * own, between the colour stage and the normalisation.  Per crop, in this order:
 *   blur       1 Blur          (sum of the k x k window + k k / 2) / (k k) in integers, BORDER_REFLECT_101
 *              2 GaussianBlur  sigma 0: 8-bit weights [64,128,64] / [16,64,96,64,16] / [8,28,56,72,56,28,8] on both axes,
 *                              (sum_y sum_x w_y w_x p + 32768) >> 16, BORDER_REFLECT_101
 *              3 MedianBlur    the exact median of the k x k window per channel, BORDER_REPLICATE
 *              4 MotionBlur    cv2.filter2D with row `tap_row` of `taps`: a 7 x 7 fp32 kernel, row-major (a k x k kernel sits centred
 *                              in it, zeros around): correlation, anchor at the centre, fp32 accumulation over the non-zero taps in
 *                              row-major order, every product and sum rounded on its own, rint half to even, saturated,
 *                              BORDER_REFLECT_101
 *   noise      1 MultiplicativeNoise  trunc(clip(fp32(v) * scale, 0, 255)), one multiplier per crop
 *              2 GaussNoise           trunc(clip(fp32(v) + scale * qtable[i], 0, 255)) per channel, scale = sigma; i = the top 12 bits of
 *                                     word c of Philox4x32-10(counter (x, y, 0, 0), key) for channel c = 0, 1, 2
 *   downscale  Downscale(0.5, INTER_NEAREST) and back: pixel (y, x) takes the value of (2 floor(y / 2), 2 floor(x / 2)); blur and
 *              noise — the noise counter included — are evaluated at that even pixel, so a 2 x 2 block shares one value
 * then fear_train_pairs' normalisation.  `qtable` is the caller's table of 4096 normal quantiles (train_data.normal_quantiles).
 * The records live in device memory, where the call cannot read them: a record with an unknown blur or noise kind, a ksize outside
 * {3, 5, 7}, or a MotionBlur with tap_row < 0 or a null `taps` has that member treated as "none" by the kernel.  A tap_row past the
 * table's last row is the caller's error (the call does not know the table's length).  H and W must be even and >= 4 (one reflection
 * at radius 3 stays inside), n <= 65535: FEAR_TRAIN_ERR_SHAPE otherwise.  n == 0 returns FEAR_TRAIN_OK without a launch.  A null
 * crops_u8, ops, qtable or out_f32 returns FEAR_TRAIN_ERR_NULL; `taps` may be null.
 *   crops_u8 : (n, H, W, 3) uint8, device      ops : (n) FearPhotoOp, device        taps : (m, 49) fp32, device, or NULL
 *   qtable : (4096) fp32, device               out_f32 : (n, 3, H, W) fp32, device                                                 */
#define FEAR_PHOTO_BLUR_NONE 0
#define FEAR_PHOTO_BLUR_BOX 1
#define FEAR_PHOTO_BLUR_GAUSSIAN 2
#define FEAR_PHOTO_BLUR_MEDIAN 3
#define FEAR_PHOTO_BLUR_MOTION 4
#define FEAR_PHOTO_BLUR_GLASS 5          /* GlassBlur: "none" to fear_photometric_u8, applied by fear_glass_u8 (below)         */
#define FEAR_PHOTO_NOISE_NONE 0
#define FEAR_PHOTO_NOISE_MULTIPLICATIVE 1
#define FEAR_PHOTO_NOISE_GAUSS 2
#define FEAR_PHOTO_NOISE_JPEG 3          /* ImageCompression: "none" to fear_photometric_u8, applied by fear_jpeg_u8 (below) */
#define FEAR_PHOTO_NOISE_ISO 4           /* ISONoise: "none" to fear_photometric_u8, applied by fear_hls_u8 (below)            */
#define FEAR_PHOTO_QUANTILES 4096

/* One crop.  32 bytes, no padding. */
typedef struct FearPhotoOp {
    int32_t blur;               /* FEAR_PHOTO_BLUR_*                                                                  */
    int32_t ksize;              /* 3, 5 or 7 (read only with a blur)                                                  */
    int32_t noise;              /* FEAR_PHOTO_NOISE_*                                                                 */
    float scale;                /* the multiplier m, or sigma = fp32(sqrt(var))                                       */
    uint32_t key[2];            /* the crop's Philox key (GaussNoise, GlassBlur)                                      */
    int32_t downscale;          /* non-zero: Downscale(0.5)                                                           */
    int32_t tap_row;            /* MotionBlur's row of `taps`, -1 otherwise                                           */
} FearPhotoOp;
#ifdef __cplusplus
static_assert(sizeof(FearPhotoOp) == 32, "FearPhotoOp is 32 bytes");
#else
_Static_assert(sizeof(FearPhotoOp) == 32, "FearPhotoOp is 32 bytes");
#endif

int fear_photometric_u8(const uint8_t* crops_u8, int n, int H, int W, const FearPhotoOp* ops, const float* taps, const float* qtable,
                        float* out_f32, void* stream);

/* fear_photometric_u8 with the crops left as the chain made them — after blur, noise and Downscale, before the normalisation — as uint8
 * HWC, the input of fear_jpeg_u8.  The same kernel body with another store policy, the same records and argument checks; and
 * crops_u8 != out_u8 (a blur reads its neighbours): FEAR_TRAIN_ERR_SHAPE.
 *   out_u8 : (n, H, W, 3) uint8, device                                                                                              */
int fear_photometric_stage_u8(const uint8_t* crops_u8, int n, int H, int W, const FearPhotoOp* ops, const float* taps, const float* qtable,
                              uint8_t* out_u8, void* stream);

/* ---- ImageCompression, the third member of the reference's noise group (model_training/dataset/aug.py:19-22): the lossy part of a
 * baseline JPEG round trip on uint8 HWC crops, as libjpeg computes it and without the entropy coding, which is lossless (DESIGN.md
 * section 11 states the contract; train_data.jpeg_roundtrip_u8_host restates it in numpy, the two agree bit for bit, and the numpy
 * form equals Pillow's libjpeg-turbo byte for byte).  cv2 reads albumentations' RGB crop as BGR: libjpeg's R is channel 2, its B channel 0.
 *   forward colour   Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *                    Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *                    Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 *   downsample       Cb, Cr 4:2:0: (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2, ... along a row of the downsampled plane
 *   forward DCT      level shift -128, jfdctint (CONST_BITS 13, PASS1_BITS 2, rows then columns, output scaled by 8)
 *   quantise         q[k] = clamp((base[k] scale + 50) / 100, 1, 255), scale = 5000 / quality below 50, else 200 - 2 quality, base the
 *                    standard luminance / chrominance table; coef = sign(v) ((|v| + (q[k] << 3 >> 1)) / (q[k] << 3))
 *   inverse DCT      coef q[k], jidctint islow (columns then rows, descale by CONST_BITS + PASS1_BITS + 3), + 128, clamp to 0..255
 *   upsample         h2v2 fancy: 3 near + far vertically (the first and last rows are their own far rows), then (3 this + left + 8) >> 4
 *                    and (3 this + right + 7) >> 4 (the first and last columns are their own neighbours), across block and MCU borders
 *   colour back      R = Y + ((91881 (Cr - 128) + 32768) >> 16), B = Y + ((116130 (Cb - 128) + 32768) >> 16),
 *                    G = Y + ((-22554 (Cb - 128) - 46802 (Cr - 128) + 32768) >> 16), each clamped to 0..255
 * `quality` lives in device memory, where the call cannot read it: the kernels copy a crop whose quality is outside 1..100.  Two launches
 * inside the call (fancy upsampling reads chroma across MCU borders): the first leaves the decoded Y, Cb and Cr planes in `workspace`
 * (fear_jpeg_workspace_bytes: 1.5 H W bytes per crop and 16 for alignment; 0 for a shape the call refuses), the second upsamples,
 * converts back and stores.  No atomics.  H and W must be positive multiples of 16 (whole MCUs), n <= 65535, crops_in != crops_out:
 * FEAR_TRAIN_ERR_SHAPE otherwise.  n == 0 returns FEAR_TRAIN_OK without a launch.  A null crops_in, quality or crops_out returns
 * FEAR_TRAIN_ERR_NULL, a null or too small workspace FEAR_TRAIN_ERR_WORKSPACE.
 *   crops_in, crops_out : (n, H, W, 3) uint8, device, distinct      quality : (n) int32, device                                     */
int fear_jpeg_u8(const uint8_t* crops_in, int n, int H, int W, const int32_t* quality, void* workspace, size_t workspace_bytes,
                 uint8_t* crops_out, void* stream);
size_t fear_jpeg_workspace_bytes(int n, int H, int W);

/* ---- JPEG frames: what the reference reads with cv2.imread (model_training/dataset/utils.py:35-43) — libjpeg with its defaults, islow
 * IDCT and fancy upsampling — decoded for the stages above (DESIGN.md section 14 states the contract; jpeg_frames.jpeg_decode_host restates
 * it in numpy and equals Pillow's libjpeg-turbo byte for byte).  The host parses the file and runs the Huffman stage; the device does the
 * arithmetic and never sees the bitstream.
 * Accepted: SOF0 (baseline sequential, 8-bit), one component or three in one interleaved scan, chroma sampling 1 x 1 and luma sampling
 * (h, v) of (1, 1), (2, 1) or (2, 2), 8-bit DQT, up to four DC and four AC Huffman tables, DRI with RST0-7, sides of 1..8192; APPn, COM and
 * fill bytes are skipped, EXIF orientation is ignored.  FEAR_TRAIN_ERR_UNSUPPORTED: the other SOF kinds, arithmetic coding, 12-bit samples,
 * 16-bit DQT, other sampling factors, 2 or 4 components, a scan with part of the components, Adobe APP14 with transform 0 (RGB), DNL.
 * FEAR_TRAIN_ERR_FORMAT: a truncated stream, a code in no table, a coefficient index past 63, a missing or out-of-order restart marker, a
 * table a component selects but no segment defined, a segment length past the end, a Huffman table with more than 256 symbols or an
 * over-subscribed code length.  A file whose entropy data is complete decodes without its EOI.
 *
 * fear_jpeg_parse reads the segments up to the scan and fills `info`.  Component i has blocks_w[i] x blocks_h[i] = mcus_x h[i] x mcus_y v[i]
 * blocks, mcus_x = ceil(width / (8 h[0])); a single component has h = v = 1 whatever the file says (its scan is not interleaved).
 * fear_jpeg_entropy_decode runs T.81 F.2 over the scan (DC prediction per component; at a restart interval the bits are dropped to the byte
 * boundary, the marker checked, the predictions reset) and writes the quantised coefficients PACKED: blocks component by component,
 * row-major within a component; block b owns coef[block_start[b] .. block_start[b + 1]), its coefficients in zigzag order from the DC term
 * through its last non-zero one (at least the DC term, at most 64 values), the rest of the block is zero.  `block_start` takes
 * total_blocks + 1 entries, `coef` up to fear_jpeg_packed_bound(info) = 64 total_blocks values; a shorter coef_cap that the file overruns
 * returns FEAR_TRAIN_ERR_WORKSPACE, an `info` that is not the file's FEAR_TRAIN_ERR_SHAPE.  Both calls are host code (no HIP call, no
 * global state; any number of threads may run them at once), check every read against `n` and every write against `coef_cap`.      */
#define FEAR_JPEG_MAX_SIDE 8192
typedef struct FearJpegInfo {
    int32_t width, height;
    int32_t components;          /* 1 or 3                                                                               */
    int32_t restart_interval;    /* MCUs between restart markers, 0: none                                                */
    int32_t mcus_x, mcus_y;
    int32_t h[3], v[3];          /* sampling factors; h[0], v[0] are the largest                                         */
    int32_t blocks_w[3], blocks_h[3];
    uint32_t total_blocks;       /* the sum over the components                                                          */
    int32_t reserved;
    uint16_t qt[3][64];          /* each component's quantiser table, natural (row-major) order                          */
} FearJpegInfo;
#ifdef __cplusplus
static_assert(sizeof(FearJpegInfo) == 464, "FearJpegInfo is 464 bytes");
#else
_Static_assert(sizeof(FearJpegInfo) == 464, "FearJpegInfo is 464 bytes");
#endif

int fear_jpeg_parse(const uint8_t* data, size_t n, FearJpegInfo* info);
size_t fear_jpeg_packed_bound(const FearJpegInfo* info);
int fear_jpeg_entropy_decode(const uint8_t* data, size_t n, const FearJpegInfo* info, int16_t* coef, size_t coef_cap, uint32_t* block_start,
                             size_t* coef_used);

/* Progressive files (SOF2), host code as the three calls above (csrc/fear_jpeg_progressive.h; DESIGN.md section 14, "Progressive files";
 * jpeg_progressive.py restates them in Python).  Opt-in: fear_jpeg_parse keeps answering FEAR_TRAIN_ERR_UNSUPPORTED for SOF2.
 * Accepted: what fear_jpeg_parse accepts of a frame header, with SOF2 in place of SOF0 (any other SOF: FEAR_TRAIN_ERR_UNSUPPORTED), and up
 * to 100 scans by T.81 G.1: a scan's components are a subset of the frame's in frame order; a DC scan (Ss = Se = 0) may interleave, an AC
 * scan (1 <= Ss <= Se <= 63) has one component; Al <= 13 and Ah is 0 or Al + 1; a first scan needs its DC or AC table (anything else:
 * FEAR_TRAIN_ERR_FORMAT).  DHT and DRI between scans are honoured.  A scan of one component walks that component's own
 * ceil(ceil(width h / h[0]) / 8) x ceil(ceil(height v / v[0]) / 8) blocks and its restart interval counts them.  After the last block the
 * next marker follows the padded byte at once.  Truncated entropy data, a missing EOI, a code in no table, a run past Se, a refinement
 * symbol of a size other than 1: FEAR_TRAIN_ERR_FORMAT.
 * FEAR_TRAIN_ERR_UNSUPPORTED: a DQT after the first SOS; an inconsistent progression (a refinement whose Ah is not the Al the coefficient
 * has reached, a first scan of a coefficient already coded, an AC scan in front of the component's DC scan); an incomplete one (at EOI
 * some coefficient has not reached Al = 0: libjpeg would smooth such blocks); a 101st scan; coefficients beyond the baseline alphabet (an
 * AC term outside +-1023, or a DC difference outside +-2047 in the layout fear_jpeg_progressive_to_baseline writes) - one rule for both
 * calls, so they always give one verdict.
 *
 * fear_jpeg_progressive_parse fills the FearJpegInfo a baseline file of that frame gets, restart_interval 0.
 * fear_jpeg_progressive_decode decodes every scan and writes fear_jpeg_entropy_decode's packed stream, which fear_jpeg_decode_u8 reads
 * unchanged; statuses and capacities as fear_jpeg_entropy_decode's.  The padded blocks a scan of one component does not visit stay zero.
 * fear_jpeg_progressive_to_baseline writes the same coefficients as a complete baseline file of at most fear_jpeg_baseline_bound(info)
 * bytes (a shorter out_cap that the file overruns: FEAR_TRAIN_ERR_WORKSPACE): SOI, the source's JFIF APP0 and Adobe APP14 segments from in
 * front of its first SOS, one DQT per table a component selects, SOF0 with the source's component ids, sampling factors and table
 * selectors, four DHT (two for one component: DC and AC for luma, then for chroma; T.81 K.2 on this file's symbol counts), DRI = mcus_x,
 * one interleaved SOS, the entropy data with RSTn after every MCU row, EOI.  EXIF, COM and the other APPn segments are dropped. */
int fear_jpeg_progressive_parse(const uint8_t* data, size_t n, FearJpegInfo* info);
int fear_jpeg_progressive_decode(const uint8_t* data, size_t n, const FearJpegInfo* info, int16_t* coef, size_t coef_cap,
                                 uint32_t* block_start, size_t* coef_used);
size_t fear_jpeg_baseline_bound(const FearJpegInfo* info);
int fear_jpeg_progressive_to_baseline(const uint8_t* data, size_t n, uint8_t* out, size_t out_cap, size_t* out_used);

/* The device half: n images of any sizes and sampling modes in one call, two launches.
 *   per block   the stored values un-zigzagged into a zeroed block, coef q in natural order, jidctint islow (columns, then rows), + 128,
 *               clamp to 0..255 — the clamp is the contract: libjpeg's C range-limit table wraps beyond +-512 of the centre where its
 *               SIMD paths saturate, and ordinary encoders stay inside — stored to the component's padded plane in `workspace`
 *   upsample    on the true [ch, cw] part of a chroma plane, cw = ceil(width / 2), ch = ceil(height / 2) for (2, 2): the edge rules apply at
 *               those edges, not at the padded blocks'.  (2, 2): fear_jpeg_u8's h2v2 rule.  (2, 1): (3 this + left + 1) >> 2 and
 *               (3 this + right + 2) >> 2, the first and last columns are their own neighbours.  A plane with cw <= 2 is replicated
 *               instead, as libjpeg does (jdsample.c)
 *   colour      fear_jpeg_u8's "colour back", stored in R, G, B order (fear_jpeg_u8 reverses it, this call does not); one component
 *               gives R = G = B = Y.  Only pixels inside [height, width] are stored.
 * `images` is a HOST array of n records holding device pointers; the call reads it for its checks, the grid sizes and nothing else.  The
 * kernels read `group_start`, a DEVICE table the caller uploads with the coefficients:
 *     uint32 [n + 1]  prefix sums of ceil(total_blocks / FEAR_JPEG_GROUP_BLOCKS) per image (jpeg_decode_blocks_kernel's workgroups)
 *     uint32 [n + 1]  prefix sums of ceil(height width / FEAR_JPEG_GROUP_PIXELS) per image (jpeg_decode_merge_kernel's)
 *     padding to FEAR_JPEG_TABLE_RECORDS(n) bytes, then a copy of the n records
 * A workgroup finds its image by a bounded binary search of its prefix table (uniform: scalar loads).  A device copy that differs from
 * `images` is the caller's error, as a wrong `block_start` is.  An image's planes lie at workspace + 16-byte alignment + plane_offset:
 * component i takes 64 blocks_w[i] blocks_h[i] bytes, an image the sum rounded up to 16 (what fear_jpeg_decode_workspace_bytes adds up,
 * plus 16).  No atomics, bounded loops only.
 * FEAR_TRAIN_ERR_SHAPE: n < 0 or n > 65535, sides outside 1..8192, components other than 1 or 3, another sampling mode, a plane_offset
 * that is no multiple of 16.  n == 0 returns FEAR_TRAIN_OK without a launch.  A null images, group_start or a null pointer in a record
 * returns FEAR_TRAIN_ERR_NULL; a null workspace, or one too short for a record's planes, FEAR_TRAIN_ERR_WORKSPACE.                   */
#define FEAR_JPEG_GROUP_BLOCKS 32
#define FEAR_JPEG_GROUP_PIXELS 256
#define FEAR_JPEG_TABLE_RECORDS(n) (((size_t)(n) * 8 + 8 + 15) & ~(size_t)15)

/* One image.  448 bytes. */
typedef struct FearJpegImage {
    const int16_t* coef;         /* device: the packed coefficients                                                      */
    const uint32_t* block_start; /* device: total_blocks + 1 offsets into coef                                           */
    uint8_t* out;                /* device: (height, width, 3) uint8, contiguous                                         */
    uint64_t plane_offset;       /* bytes from the aligned workspace to this image's planes, a multiple of 16            */
    int32_t width, height;
    int32_t components;          /* 1 or 3                                                                               */
    int32_t h, v;                /* the luma sampling factors: (1, 1), (2, 1) or (2, 2); (1, 1) with one component       */
    int32_t reserved[3];         /* [0]: the record's scale, read by fear_jpeg_decode_mixed_u8 alone (below); [1..2]: reserved */
    uint16_t qt[3][64];          /* FearJpegInfo's                                                                    */
} FearJpegImage;
#ifdef __cplusplus
static_assert(sizeof(FearJpegImage) == 448, "FearJpegImage is 448 bytes");
#else
_Static_assert(sizeof(FearJpegImage) == 448, "FearJpegImage is 448 bytes");
#endif

int fear_jpeg_decode_u8(const FearJpegImage* images, int n, const uint32_t* group_start, void* workspace, size_t workspace_bytes,
                        void* stream);
/* fear_jpeg_decode_u8 for the pixel rows [y0, y1) of each image, taken from DEVICE memory: `rows_dev` holds n pairs of int32 that only
 * the kernels read (they may still be in flight on `stream`), clipped there to [0, height]; y0 >= y1 stores nothing for the image.  The
 * records, the table, the grids and the workspace are fear_jpeg_decode_u8's, of the whole images.  jpeg_decode_blocks_kernel skips a
 * block whose MCU row lies outside the band a .. b), a = y0 / (8 v), b = ceil(y1 / (8 v)), one more on each side where v == 2 (the
 * fancy upsampling reads a chroma row above and below), clipped to the image; a workgroup all of whose 32 blocks are skipped returns in
 * front of its work.  jpeg_decode_merge_kernel stores the pixels of the rows [y0, y1) alone: their luma lies in the MCU rows of the
 * band without its halo and the chroma rows they read in the band with it, so every plane byte that is read was written by this call,
 * and the image keeps its true size, so the edge rules apply at the true edges.  The rows [y0, y1) of `out` are fear_jpeg_decode_u8's
 * byte for byte when the coefficients of the band's blocks are; all other rows of `out` keep what they held.
 * The checks are fear_jpeg_decode_u8's; a null rows_dev is FEAR_TRAIN_ERR_NULL.                                                       */
int fear_jpeg_decode_u8_rows_dev(const FearJpegImage* images, int n, const uint32_t* group_start, const int32_t* rows_dev, void* workspace,
                                 size_t workspace_bytes, void* stream);
size_t fear_jpeg_decode_workspace_bytes(const FearJpegInfo* infos, int n);
/* fear_jpeg_decode_u8 at 1 / scale of the size, scale 2, 4 or 8, as libjpeg decodes with scale_denom (Pillow's Image.draft): two
 * launches whatever n is.  With m = 8 / scale, `out` is the SCALED frame, (ceil(height m / 8), ceil(width m / 8), 3); width, height and
 * the sampling of a record stay the file's.  Component c runs an ss x ss inverse transform (jidctred.c: 4 x 4, 2 x 2, 1 x 1; ss == 8 is
 * islow): ss starts at m and doubles while ss < 8 and (h_max m) % (h_c ss 2) == 0 and (v_max m) % (v_c ss 2) == 0 — luma m; 4:2:0 chroma
 * 2 m, and no upsampling; 4:2:2 chroma m, upsampled horizontally by the (2, 1) rule above on its true width ceil(width m / 16) when
 * m > 1 and that width is above 2, replicated otherwise (libjpeg turns fancy upsampling off at 1/8).  Dequantisation, + 128, clamp and
 * colour are fear_jpeg_decode_u8's.  The transforms run in 32-bit integers where libjpeg uses `long`: equal while the dequantised
 * coefficients stay within +-2^13, as an encoder's do.
 * The table is fear_jpeg_decode_u8's: its first prefix table is the same (32 blocks per workgroup), the second counts SCALED pixels,
 * ceil(ceil(height m / 8) ceil(width m / 8) / FEAR_JPEG_GROUP_PIXELS).  An image's planes lie one after another at plane_offset, ss ss
 * bytes per block: never more than the 64 bytes per block of fear_jpeg_decode_workspace_bytes, which stays the bound to allocate and
 * is what the call checks.  A band of MCU rows is decoded as fear_jpeg_decode_u8 decodes one: `height` the band's full-size height,
 * `out` at the band's first scaled row.
 * FEAR_TRAIN_ERR_SHAPE: a scale other than 2, 4 or 8; every other check is fear_jpeg_decode_u8's; n == 0 returns FEAR_TRAIN_OK
 * without a launch.  No atomics, bounded loops only, a block reads at most 64 stored values.                                          */
int fear_jpeg_decode_scaled_u8(const FearJpegImage* images, int n, const uint32_t* group_start, int scale, void* workspace,
                               size_t workspace_bytes, void* stream);
/* fear_jpeg_decode_scaled_u8 with a scale PER RECORD, full size included: two launches whatever the mix and whatever n is.  Record i
 * carries its scale s_i in reserved[0] (byte 52 of the record): 0 or 1 is full size, 2, 4 and 8 are the scales, anything else is
 * FEAR_TRAIN_ERR_SHAPE; reserved[1..2] stay reserved, and the three entry points above go on ignoring the word.  Record i is exactly
 * the record the uniform call at s_i would carry — width, height and the sampling the file's, or the band's or window's full-size
 * ones, `out` the scaled frame or the band's first scaled row — and its pixels are that call's, byte for byte: fear_jpeg_decode_u8's at
 * full size (h2v2 and h2v1 fancy upsampling at the true chroma edges, replication for cw <= 2), fear_jpeg_decode_scaled_u8's otherwise.
 * The table's first prefix table is unchanged (32 blocks per workgroup); the second counts each image's OWN scaled pixels,
 * ceil(ceil(height m_i / 8) ceil(width m_i / 8) / FEAR_JPEG_GROUP_PIXELS) with m_i = 8 / max(s_i, 1).  A workgroup belongs to one image
 * and reads its m once from the record (a scalar load, a uniform branch).  The planes of a full-size record take 64 bytes per block,
 * those of a scaled one less: fear_jpeg_decode_workspace_bytes stays the bound to allocate and is what the call checks.
 * The checks and their order are fear_jpeg_decode_u8's, the scale being part of a record's shape; n == 0 returns FEAR_TRAIN_OK without
 * a launch.  No atomics, bounded loops only, a block reads at most 64 stored values.                                                  */
int fear_jpeg_decode_mixed_u8(const FearJpegImage* images, int n, const uint32_t* group_start, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ---- the Huffman stage on the device (jpeg_huffman.jpeg_entropy_parallel_host restates it in Python, step for
 * step).  A baseline scan has no index, but Huffman streams re-synchronise by themselves: the self-synchronising parallel decode of
 * Weissenberger and Schmidt (ICPP 2018; 2021), in a variant that is exact with bounded work and in which no workgroup waits for another.
 *
 * fear_jpeg_scan_prepare is the host's part, all it does per file besides fear_jpeg_parse: from the first byte of the scan it copies the
 * entropy-coded bytes to `bytes_out` with the FF 00 stuffing removed and splits them at the restart markers; segment s owns
 * bytes_out[seg_start[s] .. seg_start[s + 1]).  Without a restart interval there is one segment; with one there are ceil(MCUs / interval),
 * and the marker behind segment k < last must be RST(k mod 8): a missing, surplus or out-of-order marker, or a file cut in front of or
 * inside one, is FEAR_TRAIN_ERR_FORMAT.  The last segment ends at any FF xx with xx != 0 or with the file, which is where
 * fear_jpeg_entropy_decode's reader ends the data (a marker that cuts it short is found by the device: blocks are missing).  It fills
 * `scan` with the geometry and the Huffman tables the scan's components select (component c decodes with dc[c] and ac[c]); the caller
 * sets the three device addresses.  `bytes_cap` bytes and `seg_cap` entries are the capacities: the file's length and segments + 1
 * always do; FEAR_TRAIN_ERR_WORKSPACE where the file needs more.  A file whose `info` is not its own: FEAR_TRAIN_ERR_SHAPE.  Host code, no
 * HIP call, no global state, every read checked against `n` and every write against the capacities.
 *
 * fear_jpeg_huffman decodes n scans: one workgroup of 256 lanes per segment.  The segment's bits are cut into subsequences of
 * 8 subsequence_bytes bits, 256 consecutive subsequences are a sequence, and the workgroup walks its sequences in order.  A state is
 * (bit position, slot = block within the MCU, z = zigzag index, 0: a DC code is next).  Per sequence: lane 0 enters with the true state,
 * every other lane i guesses (start of subsequence i, 0, 0); each lane decodes its subsequence and stores the exit state; in round r a
 * lane still active decodes subsequence i + r from the state it carries, stops if its exit equals the one stored there and overwrites it
 * otherwise — after at most 255 rounds every stored state is the true one, whatever the file.  Then each lane decodes its subsequence
 * again and counts the blocks that begin in it and the DC differences per component modulo 2^16; an exclusive prefix carried from
 * sequence to sequence gives it the ordinal of its first block and the predictors at its entry; a last decode writes the coefficients
 * DENSE: block b (fear_jpeg_entropy_decode's component-major, row-major index) owns coef[coef_offset + 64 b ..+ 64) in zigzag order, the
 * DC term as its predicted value, every position written by exactly one lane.  Blocks past the segment's count are dropped.
 * status_dev[i] is FEAR_TRAIN_OK or FEAR_TRAIN_ERR_FORMAT: on the true chain and inside the segment's blocks a code in no table, a DC size
 * above 15, an index past 63, a symbol or its magnitude bits not wholly inside the segment; fewer blocks than the segment owes; whole
 * bytes between the last block and a restart marker — the verdict of fear_jpeg_entropy_decode, file by file.  The coefficients of a
 * failed image are unspecified; nothing is read or written out of range for it.
 * Two launches (the statuses' zeros, the decode), only workgroup barriers, no atomics; every loop is bounded by the segment's length.
 * `scans` is a HOST array the call reads for its checks and the grid size; the kernels read `table_dev`, a DEVICE copy the caller uploads:
 *     uint32 [n + 1]  prefix sums of n_seg per image
 *     padding to FEAR_JPEG_SCAN_TABLE_RECORDS(n) bytes, then a copy of the n records
 * `bytes` of a record is 4-byte aligned and readable up to n_bytes rounded up to 4.
 * FEAR_TRAIN_ERR_SHAPE: n < 0 or n > 65535, subsequence_bytes no multiple of 4 in 4..1024, a record whose geometry is not one
 * fear_jpeg_parse gives, whose n_seg or total_blocks do not follow from it, whose bytes are misaligned or whose largest segment exceeds
 * FEAR_JPEG_DEVICE_SCAN_MAX (such a file goes through fear_jpeg_entropy_decode).  n == 0 returns FEAR_TRAIN_OK without a launch.  A null
 * scans, table_dev, coef, status_dev or address in a record: FEAR_TRAIN_ERR_NULL.
 * fear_jpeg_dense_block_start writes 0, 64, 128, ... 64 total_blocks to `block_start`: the table every dense image's FearJpegImage record
 * points at, so that the dense coefficients feed fear_jpeg_decode_u8 as they are.                                                     */
#define FEAR_JPEG_DEVICE_SCAN_MAX (16u << 20)
#define FEAR_JPEG_SCAN_TABLE_RECORDS(n) (((size_t)(n) * 4 + 4 + 15) & ~(size_t)15)

/* One Huffman table in fear_jpeg::Huffman's layout.  1440 bytes. */
typedef struct FearJpegHuff {
    uint16_t look[512];          /* (length << 8 | symbol) for codes of at most 9 bits, 0 otherwise                      */
    int32_t first[17], index[17];/* the first code of a length and its place in `values`                                 */
    uint8_t values[256];
    uint8_t counts[17];          /* codes of each length 1..16                                                           */
    uint8_t reserved[7];
} FearJpegHuff;

/* One image's scan.  8704 bytes. */
typedef struct FearJpegScan {
    const uint8_t* bytes;        /* device: the unstuffed bytes of all segments                                          */
    const uint32_t* seg_start;   /* device: n_seg + 1 offsets into bytes                                                 */
    uint64_t coef_offset;        /* values from `coef` to this image's 64 total_blocks dense coefficients                */
    uint32_t n_bytes, n_seg;
    uint32_t max_seg_bytes;      /* the longest segment                                                                  */
    uint32_t total_blocks;
    int32_t components;          /* 1 or 3                                                                               */
    int32_t h, v;                /* the luma sampling factors, as in FearJpegImage                                       */
    int32_t mcus_x, mcus_y;
    int32_t restart_interval;
    FearJpegHuff dc[3], ac[3];   /* by component                                                                         */
} FearJpegScan;
#ifdef __cplusplus
static_assert(sizeof(FearJpegHuff) == 1440, "FearJpegHuff is 1440 bytes");
static_assert(sizeof(FearJpegScan) == 8704, "FearJpegScan is 8704 bytes");
#else
_Static_assert(sizeof(FearJpegHuff) == 1440, "FearJpegHuff is 1440 bytes");
_Static_assert(sizeof(FearJpegScan) == 8704, "FearJpegScan is 8704 bytes");
#endif

int fear_jpeg_scan_prepare(const uint8_t* data, size_t n, const FearJpegInfo* info, uint8_t* bytes_out, size_t bytes_cap,
                           uint32_t* seg_start, size_t seg_cap, FearJpegScan* scan);
int fear_jpeg_huffman(const FearJpegScan* scans, int n, const void* table_dev, int16_t* coef, int32_t* status_dev, int subsequence_bytes,
                      void* stream);
int fear_jpeg_dense_block_start(uint32_t* block_start, uint32_t total_blocks, void* stream);

/* ---- scans resident on the device, with the index a baseline scan lacks ("The resident store";
 * jpeg_huffman.jpeg_scan_index_host and jpeg_entropy_indexed_host restate the two calls in Python; jpeg_store.JpegStore is their user).
 * A file that is decoded again and again is prepared and uploaded once, and the true entry of every subsequence — what fear_jpeg_huffman
 * finds anew in every call by synchronising, counting and a prefix — is stored next to its bytes: FearJpegSubseq, 16 bytes per
 * subsequence.  Subsequences are numbered per image, segment after segment: segment s owns the entries sub_start[s] .. sub_start[s + 1]),
 * ceil(segment bytes / subsequence_bytes) of them; sub_start has n_seg + 1 entries.  fear_jpeg_sub_start computes it on the host from
 * the seg_start that fear_jpeg_scan_prepare wrote: it reads seg_start[0 .. n_seg], writes sub_start[0 .. n_seg] (sub_cap entries are the
 * capacity: FEAR_TRAIN_ERR_WORKSPACE below n_seg + 1; a null sub_start only counts) and the total to *n_sub.  FEAR_TRAIN_ERR_SHAPE: a bad
 * subsequence_bytes, n_seg == 0, offsets that do not start at 0, decrease or do not end at n_bytes; FEAR_TRAIN_ERR_NULL: a null seg_start
 * or n_sub.  Host code, no HIP call, no global state.
 *
 * fear_jpeg_index_build is fear_jpeg_huffman with one more output: the same kernel in a second instantiation, the same algorithm, the
 * same coefficients (to `coef`, a scratch buffer the caller may throw away) and the same verdict in status_dev; in front of its write
 * pass each lane stores its entry, one 16-byte store checked against n_sub.  `indexes` is a HOST array the call reads for its checks,
 * `index_table_dev` a DEVICE copy of the same n records for the kernel.  The checks are fear_jpeg_huffman's, and the index's capacity:
 * seg_start_host of a record is the HOST copy of the scan's seg_start (what fear_jpeg_scan_prepare wrote), non-decreasing and ending at
 * n_bytes, and n_sub must equal the sum of ceil((seg_start[s + 1] - seg_start[s]) / subsequence_bytes), else FEAR_TRAIN_ERR_SHAPE; an
 * index not 16-byte aligned or a sub_start not 4-byte aligned is FEAR_TRAIN_ERR_SHAPE too, a null index, sub_start, seg_start_host,
 * indexes or index_table_dev FEAR_TRAIN_ERR_NULL (an image with n_sub == 0 may have a null index).  A refused call launches nothing.
 *
 * fear_jpeg_huffman_indexed decodes n resident scans from their indexes: 256 lanes, ceil(n_sub / 256) workgroups per image, one lane
 * per subsequence.  A workgroup copies its image's six tables to LDS and meets one barrier; each lane then loads its entry, finds its
 * segment by a search of sub_start bounded by 21 steps, decodes once from the entry to the subsequence's end with the write pass's
 * rules and stores what it decodes: no rounds, no count pass, no prefix, no atomics, no workgroup waits for another, every coefficient
 * position is stored by exactly one lane.  The verdict is fear_jpeg_huffman's: a lane that finds a fault stores FEAR_TRAIN_ERR_FORMAT to
 * its image's status (the lane of a segment's last subsequence judges the segment's block count, the lane of its first an empty segment
 * in front, the lane of the image's last subsequence empty segments behind; an image with n_sub == 0 fails in the first launch).
 * `images` is a HOST array of per-call records the call reads for its checks and the grid size; `scan` of a record is a DEVICE-resident
 * FearJpegScan whose own coef_offset is ignored.  The kernel reads `table_dev`, a DEVICE copy the caller uploads:
 *     uint32 [n + 1]  prefix sums of ceil(n_sub / 256) per image
 *     padding to FEAR_JPEG_SCAN_TABLE_RECORDS(n) bytes, then a copy of the n records
 * Two launches: the statuses' zeros and the decode.  n == 0 returns FEAR_TRAIN_OK without a launch.  FEAR_TRAIN_ERR_SHAPE: n < 0 or
 * n > 65535, subsequence_bytes no multiple of 4 in 4..1024, an index or a scan not 16-byte aligned, a sub_start not 4-byte aligned, more
 * than 2^31 - 1 workgroups; FEAR_TRAIN_ERR_NULL: a null images, table_dev, coef, status_dev, or scan, index (unless n_sub == 0) or
 * sub_start of a record.  The scan's geometry was checked when its index was built and lives in device memory, where the call cannot
 * read it: a wrong index, sub_start or resident record is the caller's error, as a wrong block_start is to fear_jpeg_decode_u8.  Even
 * so every read stays inside the segment and the image's n_bytes, every write inside the image's 64 total_blocks values from its
 * coef_offset, an entry's slot and z are clamped to the tables, and every loop is bounded by the subsequence's length.
 *
 * fear_jpeg_huffman_indexed_rows is fear_jpeg_huffman_indexed for a band of MCU rows per image, [mcu_row0, mcu_row0 + mcu_rows) clipped
 * to the image (JpegStore.decode_rows; jpeg_huffman.jpeg_entropy_indexed_host with a band restates it).  Only the record's subsequences
 * sub0 .. sub0 + sub_count) get a lane: ceil(sub_count / 256) workgroups per image, which is what the prefix sums of `table_dev` count.
 * The caller takes them from the file's row table (jpeg_huffman.scan_row_sub: row_sub[r] is the subsequence in which the first block of
 * MCU row r begins, row_sub[mcus_y] = n_sub): row_sub[mcu_row0] .. min(row_sub[mcu_row0 + mcu_rows], n_sub - 1), so that every block of
 * the band lies wholly in lanes that run.  A lane decodes exactly as fear_jpeg_huffman_indexed's and judges all that lane judges; a block
 * whose MCU row lies outside the band (an explicit range test) is decoded and not stored.  The band's blocks are stored BAND-DENSE: the
 * component-major, row-major layout of an image that consists of those MCU rows alone, 64 (mcu_rows mcus_x blocks-per-MCU) values from
 * coef_offset, every position written by exactly one lane, nothing outside them.  Lanes that do not run judge nothing: status_dev[i] is
 * the verdict of the lanes that ran (an image with n_sub == 0 fails as above), and a band without rows or lanes leaves FEAR_TRAIN_OK.
 * The checks are fear_jpeg_huffman_indexed's, and FEAR_TRAIN_ERR_SHAPE for sub_count > 0 with sub0 + sub_count > n_sub, or
 * mcu_row0 + mcu_rows > FEAR_JPEG_MAX_SIDE / 8.  Two launches, no atomics, one barrier, plain vector stores.
 *
 * fear_jpeg_huffman_indexed_rows_dev is the band of rows taken from DEVICE memory (JpegStore.decode_rows with a device tensor;
 * jpeg_huffman.jpeg_entropy_rows_device_host restates it in Python): `rows_dev` holds n pairs of int32, the pixel rows [y0, y1) of
 * image i at rows_dev[2 i], and only kernels read them — they may still be in flight on `stream` when the call is made.  The host does
 * not know the band, so the grid, `table_dev` and coef_offset are fear_jpeg_huffman_indexed's: ceil(n_sub / 256) workgroups per image
 * and the FULL-IMAGE dense layout.  Per image the kernel clips y0 and y1 to [0, 8 v mcus_y] (the rows of the MCU grid: the resident
 * record does not hold the height; fear_jpeg_decode_u8_rows_dev, which does, clips to it), y0 >= y1 is the empty band; else the band is
 * the MCU rows a .. b), a = y0 / (8 v), b = ceil(y1 / (8 v)), one more on each side where v == 2, clipped to mcus_y — the halo rule of
 * JpegStore.decode_rows.  A lane runs only if its subsequence lies in row_sub[a] .. min(row_sub[b], n_sub - 1); `row_sub` of a record is
 * the file's row table resident on the device, mcus_y + 1 values (jpeg_huffman.scan_row_sub).  A workgroup none of whose 256
 * subsequences lies in that interval returns in front of its copy of the tables and its barrier: it costs a few loads.  A lane that
 * runs decodes and judges as fear_jpeg_huffman_indexed's; a block of the band is stored at its FULL-IMAGE place, a block of another row
 * is decoded, judged and not stored.  Every stored position is written by exactly one lane, nothing is written outside the image's
 * 64 total_blocks values, all other positions keep what the buffer held, and every loop bound is independent of the data.  The checks
 * are fear_jpeg_huffman_indexed's; a null rows_dev, or a null row_sub in a record, is FEAR_TRAIN_ERR_NULL, a row_sub not 4-byte
 * aligned FEAR_TRAIN_ERR_SHAPE.
 *
 * fear_jpeg_huffman_indexed_windows is fear_jpeg_huffman_indexed_rows for a range of MCU columns as well (JpegStore.decode_windows;
 * jpeg_huffman.jpeg_entropy_indexed_host with a band and `cols` restates it).  The record is fear_jpeg_huffman_indexed_rows' — the band
 * mcu_row0, mcu_rows and the lanes sub0, sub_count from the row table — and its `reserved` word holds the columns as two 16-bit halves:
 * mcu_col0 in the low half, mcu_cols in the high one (mcus_x <= 1024), the range [mcu_col0, mcu_col0 + mcu_cols) clipped to mcus_x.
 * A lane of the band runs only if it can touch the window.  It loads its own entry and the next subsequence's, or takes the segment's
 * block count where the next subsequence lies in another segment; the blocks it stores have the segment ordinals lo .. hi),
 * lo = begun - (1 if a block is open at its entry), hi = min(the next begun, the segment's count); they lie in the consecutive MCUs
 * first_mcu + lo / slots .. first_mcu + (hi - 1) / slots, and the lane runs if one of those has its column in the range — all of a
 * row's columns if they are mcus_x or more, else the interval of columns from the first MCU's, the part that wraps over the row's end
 * tested on its own.  No loop, no bound that depends on the data; the rule may run a lane that stores nothing (its MCUs of the range lie
 * outside the band), never the reverse.  Lanes that do not run judge nothing, as in the rows form.  A lane that runs decodes and judges
 * exactly as fear_jpeg_huffman_indexed_rows' and stores a block only when its MCU row is in the band and its MCU column in the range,
 * WINDOW-DENSE: the component-major, row-major layout of an image made of those mcu_rows x mcu_cols MCUs alone,
 * 64 (mcu_rows mcu_cols blocks-per-MCU) values from coef_offset, every position written by exactly one lane, nothing outside them.
 * The checks are fear_jpeg_huffman_indexed_rows'; mcu_cols == 0, or mcu_col0 + mcu_cols > FEAR_JPEG_MAX_SIDE / 8, is
 * FEAR_TRAIN_ERR_SHAPE.  Two launches, no atomics, one barrier, plain vector stores.                                                  */
typedef struct FearJpegSubseq {
    uint32_t p;                  /* the true entry bit position in the segment, up to 30 bits behind the subsequence's first: < 2^27 + 31 */
    uint32_t begun;              /* blocks begun in the segment in front of the subsequence                              */
    uint16_t sz;                 /* slot << 8 | z at the entry                                                           */
    uint16_t dc[3];              /* the predictors at the entry, modulo 2^16, by component                               */
} FearJpegSubseq;

/* One image of a fear_jpeg_index_build call.  32 bytes. */
typedef struct FearJpegIndex {
    FearJpegSubseq* index;           /* device: n_sub entries, 16-byte aligned                                           */
    const uint32_t* sub_start;       /* device: n_seg + 1 prefix sums of the segments' subsequence counts                */
    const uint32_t* seg_start_host;  /* HOST: the scan's seg_start, for the call's checks; the kernel does not read it   */
    uint32_t n_sub;
    uint32_t reserved;
} FearJpegIndex;

/* One image of a fear_jpeg_huffman_indexed call.  64 bytes. */
typedef struct FearJpegIndexed {
    const FearJpegScan* scan;        /* device: the resident record; its coef_offset is ignored                          */
    const FearJpegSubseq* index;     /* device                                                                           */
    const uint32_t* sub_start;       /* device                                                                           */
    uint64_t coef_offset;            /* values from `coef` to this image's 64 total_blocks dense coefficients            */
    uint32_t n_sub;
    uint32_t sub0, sub_count;        /* fear_jpeg_huffman_indexed_rows alone: the subsequences that get a lane, sub0 .. sub0 + sub_count) */
    uint32_t mcu_row0, mcu_rows;     /* fear_jpeg_huffman_indexed_rows alone: the band of MCU rows whose blocks are stored             */
    uint32_t reserved;               /* fear_jpeg_huffman_indexed_windows alone: mcu_col0 | mcu_cols << 16, the MCU columns whose blocks are stored */
    const uint32_t* row_sub;         /* fear_jpeg_huffman_indexed_rows_dev alone: device, the file's row table, mcus_y + 1 values; offset 56 */
} FearJpegIndexed;
#ifdef __cplusplus
static_assert(sizeof(FearJpegSubseq) == 16, "FearJpegSubseq is 16 bytes");
static_assert(sizeof(FearJpegIndex) == 32, "FearJpegIndex is 32 bytes");
static_assert(sizeof(FearJpegIndexed) == 64 && offsetof(FearJpegIndexed, row_sub) == 56, "FearJpegIndexed is 64 bytes, row_sub at 56");
#else
_Static_assert(sizeof(FearJpegSubseq) == 16, "FearJpegSubseq is 16 bytes");
_Static_assert(sizeof(FearJpegIndex) == 32, "FearJpegIndex is 32 bytes");
_Static_assert(sizeof(FearJpegIndexed) == 64 && offsetof(FearJpegIndexed, row_sub) == 56, "FearJpegIndexed is 64 bytes, row_sub at 56");
#endif

int fear_jpeg_sub_start(const uint32_t* seg_start, uint32_t n_seg, uint32_t n_bytes, int subsequence_bytes, uint32_t* sub_start,
                        size_t sub_cap, uint32_t* n_sub);
int fear_jpeg_index_build(const FearJpegScan* scans, int n, const void* table_dev, const FearJpegIndex* indexes, const void* index_table_dev,
                          int16_t* coef, int32_t* status_dev, int subsequence_bytes, void* stream);
int fear_jpeg_huffman_indexed(const FearJpegIndexed* images, int n, const void* table_dev, int16_t* coef, int32_t* status_dev,
                              int subsequence_bytes, void* stream);
int fear_jpeg_huffman_indexed_rows(const FearJpegIndexed* images, int n, const void* table_dev, int16_t* coef, int32_t* status_dev,
                                   int subsequence_bytes, void* stream);
int fear_jpeg_huffman_indexed_rows_dev(const FearJpegIndexed* images, int n, const void* table_dev, const int32_t* rows_dev, int16_t* coef,
                                       int32_t* status_dev, int subsequence_bytes, void* stream);
int fear_jpeg_huffman_indexed_windows(const FearJpegIndexed* images, int n, const void* table_dev, int16_t* coef, int32_t* status_dev,
                                      int subsequence_bytes, void* stream);

/* ---- scans whose bytes lie in pinned host memory ("Bytes on the host"; JpegStore(residence="host")).
 * The four calls above, each with the STAGED byte fetch: the same records, checks, grids, launch counts and results, but `bytes` of a
 * record's resident FearJpegScan is the DEVICE-SIDE address of pinned, mapped host memory (fear_host_mapped_pointer), which the kernels
 * read in place; everything else of the record stays in device memory.  A workgroup's running lanes cover consecutive subsequences,
 * hence one byte range (fear_jpeg_stage_range).  In front of its barrier the workgroup copies that range into LDS with 16-byte loads:
 * from the 16-byte aligned address at or in front of the range's first byte to two words behind its end (the last lane's 64-bit
 * window), at most min(256 subsequence_bytes + 32, 65536) bytes — the launch's dynamic LDS — and never a word at or behind
 * 4 ceil(n_bytes / 4) bytes from `bytes` nor one in front of it.  A lane takes a word from LDS where it was staged and from `bytes`
 * otherwise: above subsequence_bytes 256 a range can exceed the cap, its tail is then read directly, slower and as exact.  Form rows_dev
 * stages the range of the band's lanes alone (an idle workgroup returns in front of it), form windows that of all the band's lanes of
 * the workgroup, whether or not one of them touches the window.  FEAR_TRAIN_ERR_HIP where the runtime refuses the kernels' LDS size.
 *
 * fear_host_mapped_pointer asks hipPointerGetAttributes for the device-side address of `host`, a pointer into a pinned, mapped host
 * allocation, and stores it to *device.  FEAR_TRAIN_ERR_SHAPE (and a null *device) for anything else: pageable memory, device or managed
 * memory, a null `host`; FEAR_TRAIN_ERR_NULL for a null `device`; FEAR_TRAIN_ERR_HIP where there is no device to ask.
 *
 * fear_jpeg_stage_range is the range rule on the host, before alignment and cap: the bytes byte0 .. byte1) of the scan that the
 * subsequences sub_first .. sub_first + sub_count) cover — the union of [seg_start[s] + k subsequence_bytes, min(that +
 * subsequence_bytes, seg_start[s + 1])) over them, one range because consecutive subsequences are consecutive bytes; 0, 0 for
 * sub_count == 0.  The kernels and this function share one helper; jpeg_huffman.stage_range_host restates it.  Host code, no HIP call.
 * FEAR_TRAIN_ERR_NULL: a null pointer; FEAR_TRAIN_ERR_SHAPE: fear_jpeg_sub_start's refusals of seg_start, a sub_start that is not
 * its prefix sums, sub_first + sub_count > n_sub.                                                                                      */
int fear_jpeg_huffman_indexed_host(const FearJpegIndexed* images, int n, const void* table_dev, int16_t* coef, int32_t* status_dev,
                                   int subsequence_bytes, void* stream);
int fear_jpeg_huffman_indexed_rows_host(const FearJpegIndexed* images, int n, const void* table_dev, int16_t* coef, int32_t* status_dev,
                                        int subsequence_bytes, void* stream);
int fear_jpeg_huffman_indexed_rows_dev_host(const FearJpegIndexed* images, int n, const void* table_dev, const int32_t* rows_dev,
                                            int16_t* coef, int32_t* status_dev, int subsequence_bytes, void* stream);
int fear_jpeg_huffman_indexed_windows_host(const FearJpegIndexed* images, int n, const void* table_dev, int16_t* coef, int32_t* status_dev,
                                           int subsequence_bytes, void* stream);
int fear_host_mapped_pointer(const void* host, void** device);
int fear_jpeg_stage_range(const uint32_t* seg_start, const uint32_t* sub_start, uint32_t n_seg, uint32_t n_bytes, uint32_t sub_first,
                          uint32_t sub_count, int subsequence_bytes, uint32_t* byte0, uint32_t* byte1);

/* ---- the colour stage's members that are no lookup table: Equalize, HueSaturationValue, ColorJitter and Emboss of the reference's
 * p = 0.5 OneOf (model_training/dataset/aug.py:35-48), on uint8 HWC crops between fear_train_pairs_u8 (tone, then the lookup-table
 * members) and fear_photometric_u8 (DESIGN.md section 11 states every contract; train_data.colour_u8_host restates them in numpy and the
 * two agree bit for bit).  Per crop, by the record's kind:
 *   5 Equalize            cv2.equalizeHist per channel over the crop: i0 the first non-empty bin, lut[i] = saturate(rint(fp32(sum of
 *                         hist(i0, i]) * (fp32(255) / fp32(H W - hist[i0])))), a channel with a single value keeps it
 *   6 HueSaturationValue  RGB -> HSV (cv2's 8-bit path, H in [0, 180)), aux_lut rows lh | ls | lv, HSV -> RGB (cv2's fp32 path)
 *   7 ColorJitter         `order` is a permutation of 0 brightness (aux_lut row 0), 1 contrast (trunc(clip(i contrast + mean (1 -
 *                         contrast), 0, 255)) in float64, mean = that of the gray plane of the crop as the operations in front left
 *                         it), 2 saturation (rint(fp32(c) alpha + fp32(gray) beta)), 3 hue (RGB -> HSV, aux_lut row 1 on H, HSV -> RGB);
 *                         each operation works on the previous one's uint8 result
 *   8 Emboss              cv2.filter2D with the nine `taps` (row-major 3 x 3): correlation, anchor at the centre, BORDER_REFLECT_101,
 *                         the non-zero taps in row-major order, fp32 accumulation, rint half to even, saturated
 * Any other kind, and a ColorJitter whose order is no permutation, copies the crop (the records live in device memory, where the call
 * cannot read them).  Per-crop statistics are per crop: one workgroup per crop, integer sums in LDS, no global atomics.
 * H and W must be even and >= 4, n <= 65535, crops_in != crops_out (Emboss reads neighbours): FEAR_TRAIN_ERR_SHAPE otherwise.  n == 0
 * returns FEAR_TRAIN_OK without a launch.  A null crops_in, ops, aux_lut or crops_out returns FEAR_TRAIN_ERR_NULL.
 *   crops_in, crops_out : (n, H, W, 3) uint8, device, distinct      ops : (n) FearColourOp, device      aux_lut : (n, 3, 256) uint8, device */
#define FEAR_COLOUR_EQUALIZE 5
#define FEAR_COLOUR_HSV 6
#define FEAR_COLOUR_JITTER 7
#define FEAR_COLOUR_EMBOSS 8

/* One crop.  64 bytes. */
typedef struct FearColourOp {
    int32_t kind;               /* FEAR_COLOUR_*, anything else: copy                                                  */
    uint8_t order[4];           /* ColorJitter: the operations in the order they run                                   */
    double contrast;            /* ColorJitter: the contrast factor                                                    */
    float alpha, beta;          /* ColorJitter: fp32(saturation), fp32(1 - saturation) (the difference in float64)     */
    float taps[9];              /* Emboss: the 3 x 3 kernel, row-major                                                 */
    int32_t reserved;
} FearColourOp;
#ifdef __cplusplus
static_assert(sizeof(FearColourOp) == 64, "FearColourOp is 64 bytes");
#else
_Static_assert(sizeof(FearColourOp) == 64, "FearColourOp is 64 bytes");
#endif

int fear_colour_u8(const uint8_t* crops_in, int n, int H, int W, const FearColourOp* ops, const uint8_t* aux_lut, uint8_t* crops_out,
                   void* stream);

/* ---- the photometric stage's members that work in HLS: ISONoise, the fourth member of the reference's noise group, and its weather
 * group OneOf([RandomRain, RandomShadow]) (model_training/dataset/aug.py:8-25), on uint8 HWC crops between fear_photometric_stage_u8 (or
 * fear_jpeg_u8) and fear_photometric_u8 (DESIGN.md section 11 states every contract; train_data.hls_u8_host restates them in numpy and the
 * two agree bit for bit).  RGB <-> HLS is cv2's, through fp32 with every operation rounded on its own.  Per crop, by the record's kind:
 *   1 ISONoise      S1 = sum(max + min), S2 = sum((max + min)^2) over the crop's pixels in integers; in float64 sigma_L = sqrt(max(S2 / N
 *                   - (S1 / N)^2, 0)) / 510, lambda = sigma_L intensity 255, quantised to rint(16 lambda) / 16 and cut to [0, 64]; the CDF
 *                   p_0 = exp_table[16 lambda], p_j = p_{j-1} lambda / j over 160 terms, summed in order.  Per pixel, Philox4x32-10 at
 *                   counter (x, y, 0, 0) with `key`: k = the number of CDF entries <= word 0 / 2^32 (at most 159), noise = qtable[word 1
 *                   >> 20] hue_scale.  On the fp32 HLS of the crop times fp32(1 / 255): h += noise, + 360 when negative, then - 360 when
 *                   above 360; l += (fp32(k) fp32(1 / 255)) (1 - l); back to RGB, times 255, trunc(clip(., 0, 255))
 *   2 RandomRain    rows seg_offset .. + seg_count of `segments` are drops (x0, y0, x1, y1): 200 in all channels along each one's raster
 *                   (OpenCV's 8-connected line, clipped to the crop), fear_photometric_u8's Blur at k = 7, then on every pixel RGB -> HLS
 *                   (8-bit), L = trunc(fp32(L) fp32(0.7)), HLS -> RGB
 *   3 RandomShadow  those rows are polygons: a row (n, 0, 0, 0), then the polygon's n edges (x0, y0, x1, y1).  A pixel is in shadow when
 *                   it lies on the raster of an edge or inside a polygon by the even-odd rule on integer pixel coordinates (an edge counts
 *                   when y0 <= y < y1, its ends ordered by y, and (x - x0) (y1 - y0) < (y - y0) (x1 - x0)); there RGB -> HLS (8-bit),
 *                   L = L >> 1, HLS -> RGB
 * Any other kind, and a rain or shadow record with a negative seg_offset or seg_count, copies the crop (the records live in device
 * memory, where the call cannot read them); rows past the table's end are the caller's error.  One workgroup per crop: the mask, the
 * sums and the CDF live in LDS, no global atomics.
 * H and W must be even, >= 4 and <= 256 (the mask holds 256 x 256 bits), n <= 65535, crops_in != crops_out (rain reads neighbours):
 * FEAR_TRAIN_ERR_SHAPE otherwise.  n == 0 returns FEAR_TRAIN_OK without a launch.  A null crops_in, ops, segments, qtable, exp_table or
 * crops_out returns FEAR_TRAIN_ERR_NULL.
 *   crops_in, crops_out : (n, H, W, 3) uint8, device, distinct      ops : (n) FearHlsOp, device      segments : (m, 4) int16, device
 *   qtable : (4096) fp32, device (train_data.normal_quantiles)     exp_table : (1025) float64, device: exp(-i / 16)                 */
#define FEAR_HLS_COPY 0
#define FEAR_HLS_ISO 1
#define FEAR_HLS_RAIN 2
#define FEAR_HLS_SHADOW 3
#define FEAR_HLS_MAX_SIDE 256
#define FEAR_HLS_EXP_ENTRIES 1025

/* One crop.  32 bytes, no padding. */
typedef struct FearHlsOp {
    int32_t kind;               /* FEAR_HLS_*, anything else: copy                                                     */
    int32_t seg_offset;         /* rain, shadow: the first row of `segments`                                           */
    int32_t seg_count;          /* rain: the drops; shadow: the rows of all polygons, their count rows included        */
    float hue_scale;            /* ISONoise: fp32(color_shift 360 intensity)                                           */
    double intensity;           /* ISONoise                                                                            */
    uint32_t key[2];            /* ISONoise: the crop's Philox key                                                     */
} FearHlsOp;
#ifdef __cplusplus
static_assert(sizeof(FearHlsOp) == 32, "FearHlsOp is 32 bytes");
#else
_Static_assert(sizeof(FearHlsOp) == 32, "FearHlsOp is 32 bytes");
#endif

int fear_hls_u8(const uint8_t* crops_in, int n, int H, int W, const FearHlsOp* ops, const int16_t* segments, const float* qtable,
                const double* exp_table, uint8_t* crops_out, void* stream);

/* ---- GlassBlur, the fifth member of the reference's blur group (model_training/dataset/aug.py:8-25), with albumentations' defaults
 * (sigma 0.7, max_delta 4, iterations 2, mode "fast"), on uint8 HWC crops in front of fear_photometric_stage_u8 / fear_photometric_u8,
 * to which a record of this kind is "none" (DESIGN.md section 11 states the contract; train_data.glass_u8_host restates it in numpy
 * and the two agree bit for bit).  A crop whose record's blur is FEAR_PHOTO_BLUR_GLASS takes, all three channels alike:
 *   1  cv2.GaussianBlur(ksize (0, 0), sigma 0.7) on 8 bits: 5 x 5, the weights (2, 53, 146, 53, 2) on both axes,
 *      (sum_y sum_x w_y w_x p + 32768) >> 16, BORDER_REFLECT_101
 *   2  for i = 0, 1: over the pixels h in [5, H - 4], w in [5, W - 4], element n = (H - 4 - h) + (H - 8) (W - 4 - w), with dy = (word & 7)
 *      - 4 and dx = ((word >> 3) & 7) - 4 of word 0 of Philox4x32-10(counter (w, h, 1 + i, 0), the record's key):
 *      x[h, w], x[h + dy, w + dx] = x[h + dy, w + dx], x[h, w], both right-hand sides read before the iteration, the first assignment
 *      made for every n before the second, and the largest n winning where the second assignment's targets repeat.  No such pixel
 *      when H <= 8 or W <= 8
 *   3  the Gaussian of 1 again
 * Every other crop is copied.  One workgroup per 32 x 32 tile with its neighbourhood of 12 pixels in LDS; the scatter of 2 is a gather
 * over the 8 x 8 sources that can reach a pixel: no atomics, no workspace.
 * H and W must be even, >= 4 and <= 256, n <= 65535, crops_u8 != out_u8: FEAR_TRAIN_ERR_SHAPE otherwise (fear_hls_u8's checks).  n == 0
 * returns FEAR_TRAIN_OK without a launch.  A null crops_u8, ops or out_u8 returns FEAR_TRAIN_ERR_NULL.
 *   crops_u8, out_u8 : (n, H, W, 3) uint8, device, distinct      ops : (n) FearPhotoOp, device (blur and key are read)               */
int fear_glass_u8(const uint8_t* crops_u8, int n, int H, int W, const FearPhotoOp* ops, uint8_t* out_u8, void* stream);

/* ---- step metrics: the training telemetry of the reference's `_training_step` (train/fear_lightning_model.py:66-87) on the device
 * (feartracker_amd/metrics.py).  Per pair: FEARBoxCoder.decode of the step's own output maps (fear_decode's
 * arithmetic: fp32 sigmoid, first maximum, float64 grid), box_convert(xywh -> xyxy) of the decoded and the ground-truth box, and
 * torchvision's box_iou of the two in float64, every operation rounded on its own.  Then BoxIoUMetric / TrackingFailureRateMetric
 * (metrics/tracking.py) and DatasetAwareMetric (metrics/dataset_aware_metric.py), summed in pair-index order (two launches, no atomics):
 *   cls (B,1,16,16), bbox (B,4,16,16) fp32 : the step's outputs          gt_box (B,4) int32 xywh in the 256 x 256 search crop
 *   visible (B) int32 : 0 = the pair takes no part                        dataset_id (B) int32 in [0, n_datasets)
 *   iou (B) float64 out : the pair's IoU, -1 for an invisible pair
 *   step3 (3) float64 out : mean IoU over the visible pairs | failure rate = 1 - count_nonzero(iou) / n_visible | n_visible
 *   accum (3 + 2 n_datasets) float64, updated in place (zero it to start an epoch):
 *       sum of step mean IoUs | sum of step failure rates | steps counted | per dataset sum of IoUs | per dataset pair count
 * A step with NO visible pair makes the reference take a mean over nothing (NaN, which then stays in its epoch mean); here such a
 * step writes step3 = {0, 0, 0} and adds nothing to any accumulator — the same kind of deliberate deviation as fear_head_loss's. */
#define FEAR_METRICS_MAX_DATASETS 64
int fear_train_metrics(const float* cls, const float* bbox, const int32_t* gt_box, const int32_t* visible, const int32_t* dataset_id,
                       int B, int n_datasets, double* iou, double* step3, double* accum, void* stream);

/* ---- pictures made on the device (csrc/fear_train_visuals.h; feartracker_amd/visuals.py restates both calls in
 * numpy, `draw_boxes_host` and `miner_host`, and the two agree byte for byte).
 *
 * The rectangle contract.  A box is (x, y, w, h) int32 with corners x0 = min(x, x + w), x1 = max(x, x + w), likewise y0, y1: pt2 =
 * (x + w, y + h) is inclusive.  For thickness t, o = t / 2 and i = (t - 1) / 2: a pixel belongs to the box's band iff it lies in the outer
 * rectangle [x0 - o, x1 + o] x [y0 - o, y1 + o] and not in the inner rectangle [x0 + i + 1, x1 - i - 1] x [y0 + i + 1, y1 - i - 1], which is
 * empty when either range is reversed.  The outline is t pixels wide with square corners, the band is clipped to the image, a box wholly
 * outside draws nothing, a box thinner than the band is filled.  Boxes on one frame are drawn in index order: the LAST box in index order
 * whose band holds a pixel gives it its colour.  This is the project's own statement, not cv2.rectangle's thick lines.
 *
 * fear_draw_boxes_u8 draws K boxes into uint8 frames in place.  Every argument is read on the device only:
 *   frames : (n_frames) fear_frame, device: contiguous (h, w, 3) uint8, any sizes; the pixels are WRITTEN (a frame with h <= 0, w <= 0 or
 *            a null pointer is skipped)
 *   boxes : (K, 4) int32, device      frame_of : (K) int32, device: the frame of each box, outside [0, n_frames) the box is skipped
 *   colours : (K, 3) uint8, device
 * One workgroup of 256 lanes per (box, side): the top and bottom strips over the outer rectangle's width, the left and right strips of
 * the rows between.  "The last box wins" is a gather: a workgroup first compacts into LDS the later boxes of its frame whose outer
 * rectangle meets its strip (flags and popcounts, up to 512 boxes; where more meet it, the rest are read from memory per pixel), then a
 * lane skips a pixel that one of them holds.  Two strips of one box may store the same value to a shared pixel.  No atomics, no order
 * between workgroups, the same bytes on every run.  Every workgroup reads the K - k - 1 later boxes: the call is meant for hundreds of
 * boxes, not for 65535 on one frame.
 * FEAR_TRAIN_ERR_SHAPE: K < 0 or K > 65535, n_frames < 0, thickness outside 1..32.  K == 0 or n_frames == 0 returns FEAR_TRAIN_OK
 * without a launch.  A null frames, boxes, frame_of or colours returns FEAR_TRAIN_ERR_NULL.                                          */
int fear_draw_boxes_u8(const fear_frame* frames, int n_frames, const int32_t* boxes, const int32_t* frame_of, const uint8_t* colours, int K,
                       int thickness, void* stream);

/* The best / worst batch miner: BestWorstMinerCallback of the reference (model_training/train/callbacks.py:95-230) with get_visuals
 * (train/fear_lightning_model.py:217-258), one call per training step, two launches, nothing read by the host.
 *   decide   one wave.  s = (double)(fp32 score_a[0] (+ score_b[0] when score_b is given)).  For each side, [0] best and [1] worst: a
 *            side with has == 0 takes the step; otherwise, mode min (mode_max == 0), best takes s <= score - min_delta and worst takes
 *            s >= score + min_delta; mode max mirrors them.  A NaN on either side of a comparison takes nothing, so a NaN enters only
 *            as a first step and then stays.  take[side] is written for every call; a side that takes sets has, score, step =
 *            step_index.  When either side takes, the first n = min(B, n_images) pairs are decoded (fear_train_metrics's decode), each of
 *            x, y, w, h truncated toward zero (a NaN is 0, a magnitude above 2^20 is cut to it), into pred.
 *   render   grid (16, n, 2); a workgroup of a side with take == 0 returns after that load.  Otherwise item k fills rows 256 k ..
 *            256 k + 255 of the side's sheet: the template in columns 0..127 of the top 128 rows, zeros below it, the search crop in
 *            columns 128..383.  A normalised value x of channel c becomes 255.0 * ((double)x * std_c + mean_c) in float64, every
 *            operation rounded on its own, truncated toward zero and cut to 0..255 (a NaN is 0).  On the search crop, clipped to it,
 *            at thickness 2 by the contract above: first pred[k] in (0, 250, 0), then gt_box[k] in (250, 0, 0) where visible[k] != 0,
 *            else (0, 0, 250).
 *   templ (B,3,128,128), search (B,3,256,256) fp32 normalised      cls (B,1,16,16), bbox (B,4,16,16) fp32: the step's outputs
 *   gt_box (B,4) int32, visible (B) int32      score_a, score_b : device scalars, score_b may be null
 *   state : device, zeroed to start an epoch      sheets : (2, n 256, 384, 3) uint8, device: [0] best, [1] worst
 * FEAR_TRAIN_ERR_SHAPE: B < 0 or B > 65535, n_images outside 1..FEAR_MINER_MAX_IMAGES.  B == 0 returns FEAR_TRAIN_OK without a launch.
 * A null pointer other than score_b returns FEAR_TRAIN_ERR_NULL.                                                                       */
#define FEAR_MINER_MAX_IMAGES 64

/* The miner's state.  1072 bytes. */
typedef struct FearMinerState {
    int32_t has[2];             /* [0] best, [1] worst: the side holds a batch                                          */
    int32_t step[2];            /* the step_index of that batch                                                        */
    double score[2];            /* its score                                                                           */
    int32_t take[2];            /* the last call's decision                                                            */
    int32_t reserved[2];
    int32_t pred[FEAR_MINER_MAX_IMAGES][4];   /* the decoded boxes x, y, w, h of the last step that was taken          */
} FearMinerState;
#ifdef __cplusplus
static_assert(sizeof(FearMinerState) == 1072, "FearMinerState is 1072 bytes");
#else
_Static_assert(sizeof(FearMinerState) == 1072, "FearMinerState is 1072 bytes");
#endif

int fear_miner_update(const float* templ, const float* search, const float* cls, const float* bbox, const int32_t* gt_box,
                      const int32_t* visible, const float* score_a, const float* score_b, int B, int n_images, int mode_max, double min_delta,
                      int step_index, FearMinerState* state, uint8_t* sheets, void* stream);

/* ---- JPEG files written on the device (csrc/fear_jpeg_encode.h; DESIGN.md section 14, "Writing JPEG files"; jpeg_encode.jpeg_encode_host
 * restates the whole call in numpy and equals Pillow's libjpeg-turbo byte for byte).  uint8 RGB frames of any size 1..FEAR_JPEG_MAX_SIDE
 * become baseline SOF0 files: 8-bit, three components, 4:2:0, jpeg_set_quality(quality, force_baseline)'s tables, the islow FDCT, the
 * standard Huffman tables of T.81 K.3 to K.6, a restart interval in MCUs if restart_interval != 0.  Channel 0 is R (fear_jpeg_u8 keeps
 * cv2's reading, in which it is B).
 *
 * A record is host data.  The caller fills src, out, out_cap, header, header_bytes, width, height, quality (1..100) and restart_interval
 * (0..65535); fear_jpeg_encode_plan fills the rest: where the image's scratch lies in the workspace and at which workgroup of each pass
 * the image begins.  The header — everything from SOI to the end of the SOS segment — is built on the host: fear_jpeg_encode_header
 * writes it (at most FEAR_JPEG_ENC_HEADER_MAX bytes; a smaller out_cap that it overruns: FEAR_TRAIN_ERR_WORKSPACE; a side, quality or
 * interval out of range: FEAR_TRAIN_ERR_SHAPE).  The first FEAR_JPEG_ENC_TABLE_BYTES(n) bytes of the workspace are the CALLER's to write:
 * a device copy of the n planned records, uploaded with the header bytes before the call, so that the call itself transfers nothing
 * and never waits.
 *
 * fear_jpeg_encode_u8: a memset of the bit streams and eight launches, whatever n is.
 *   transform  4 MCUs per workgroup: colour conversion, the edge rules (luma replicated right and down to whole blocks; chroma columns
 *              replicated at full size, the last row only to an even height, then the last DOWNSAMPLED row replicated down), h2v2
 *              downsampling, FDCT, quantiser; int16 coefficients in zigzag order, blocks in MCU order (Y00 Y01 Y10 Y11 Cb Cr).  A luma
 *              block outside the component has no AC terms and the DC term of the block before it in that order.
 *   sizes      one lane per block, FEAR_JPEG_ENC_GROUP_BLOCKS per workgroup: the DC difference to the previous block of the component
 *              (0 at a restart boundary) and the block's exact bit count.
 *   segments   one workgroup per restart segment: the exclusive scan of its blocks' bit counts, its length in bytes.
 *   offsets    one workgroup per image: the exclusive scan of the segments' bytes; the length of the unstuffed stream.
 *   write      one lane per block: the codes into the image's unstuffed byte stream, MSB first.  Words a block covers whole are stored;
 *              its first and last words are merged with an integer OR into the zeroed stream, which does not depend on arrival order.
 *              The pad bits of a segment's last byte are 1.
 *   count      one workgroup per FEAR_JPEG_ENC_CHUNK_BYTES of the stream: its FF bytes.
 *   lengths    one workgroup per image: the exclusive scan of the chunks' counts; the file's length, and whether it fits the slot.
 *   assemble   one workgroup per chunk: byte i of the stream lands at header_bytes + i + (FF bytes before it) + 2 (restart markers before
 *              it), a 00 behind each FF; the markers FF D0+((k-1)&7), the header's copy and the EOI.
 * length_dev[i] is the file's length and status_dev[i] FEAR_TRAIN_OK, or 0 and FEAR_JPEG_ENC_OVERFLOW for a file longer than out_cap: its
 * slot is then not written at all, and no byte at or past a slot's end is ever written.  The other images are unaffected.
 * fear_jpeg_encode_bound is the longest file a frame can give: header, 1244 bytes per MCU and one of padding per segment, every byte
 * stuffed, the markers and the EOI; 0 for arguments out of range.  fear_jpeg_encode_workspace_bytes is 0 for a call that would be refused.
 * FEAR_TRAIN_ERR_SHAPE: n < 0 or n > 65535, a side outside 1..FEAR_JPEG_MAX_SIDE, a quality outside 1..100, a restart_interval outside
 * 0..65535, header_bytes outside 1..4096, a source that overlaps its or another image's slot, plan fields that are not
 * fear_jpeg_encode_plan's.  n == 0 returns FEAR_TRAIN_OK without a launch.  A null images, length_dev, status_dev, src, out or header:
 * FEAR_TRAIN_ERR_NULL.  A null workspace or one below fear_jpeg_encode_workspace_bytes: FEAR_TRAIN_ERR_WORKSPACE.
 * fear_jpeg_encode_header, _plan, _workspace_bytes and _bound are host code.
 *
 * The other layouts.  A record's `sampling` (0 in a zeroed record: 4:2:0 from RGB, all of the above) selects 4:2:2, 4:4:4 or one gray
 * component; fear_jpeg_encode_plan keeps it and refuses any other value as FEAR_TRAIN_ERR_SHAPE.  Per layout: the MCU in pixels, its
 * blocks in scan order, MCUs per transform workgroup, the longest MCU in bits.
 *   4:2:0  16 x 16  Y00 Y01 Y10 Y11 Cb Cr  4   9952      4:2:2  16 x 8  Y0 Y1 Cb Cr  6   6636
 *   4:4:4   8 x 8   Y Cb Cr                8   4978      gray    8 x 8  Y            24  1658
 * 4:2:2 is h2v1: chroma is (a + b + bias) >> 1 with bias 0, 1, 0, 1 along a row, columns replicated at full size, rows below the frame
 * repeat the last row; Y1 of the last MCU column is a dummy block (the DC term of Y0, no AC terms) when ceil(width / 8) is odd.  4:4:4
 * and gray replicate right and down and have no dummy blocks.  Gray is one non-interleaved component with table 0 only; its header is
 * 328 bytes (334 with DRI), the colour layouts' 623 (629).  A restart interval counts the layout's MCUs.  A gray source is width x height
 * bytes unless FEAR_JPEG_ENC_GRAY_RGB is set.  fear_jpeg_encode_header and fear_jpeg_encode_bound mean 4:2:0; the _mode forms take the
 * sampling (for the header without FEAR_JPEG_ENC_GRAY_RGB, which does not change the file's layout) and are FEAR_TRAIN_ERR_SHAPE or 0
 * for an unknown one.
 *
 * Per-file Huffman tables.  A record whose `flags` have FEAR_JPEG_ENC_OPTIMIZE gets the file libjpeg writes with optimize_coding: its
 * tables are built from the scan's own symbol counts by T.81 K.2 as jpeg_gen_optimal_table does it (a reserved 257th symbol of
 * frequency 1; the two smallest non-zero frequencies merged, in a tie the larger symbol first; lengths limited to 16 by Adjust_BITS; the
 * reserved symbol taken from the longest length in use; symbols sorted by depth, then value; codes by annex C).  All-zero flags are the
 * record described above, unknown bits FEAR_TRAIN_ERR_SHAPE, and flags changed after fear_jpeg_encode_plan are refused like a changed
 * sampling.  For such a record the caller passes the header WITHOUT its DHT segments (fear_jpeg_encode_header_flags); they belong
 * 177 bytes in (gray: 102), behind SOF0, where the device puts the segments it built: DC 0, AC 0 and, but for gray, DC 1, AC 1; DRI and
 * SOS follow.  The header's length is then a device value; it never exceeds the standard header's, since a table lists the symbols its
 * scan has.  A call with at least one such record runs two more launches between transform and sizes:
 *   stats      sizes' grid, one lane per block: the symbols the coder will emit (dummy blocks, ZRL and EOB included, DC differences
 *              restarting at segment boundaries) counted in LDS per workgroup and added to the image's 4 x 256 uint32 counts with integer
 *              atomics: the sums do not depend on the order.  The counts stand in front of the image's stream, where the call's one
 *              memset zeroes them.  Workgroups of plain images return.
 *   tables     one wave per (image, table): the rule above, each merge two wave-wide searches for the smallest frequency; the image's
 *              code table, which sizes and write then read in place of the standard one, and the table's DHT segment.
 * A call without such a record is the memset and the eight launches above, unchanged.  A tree deeper than 32 before limiting is what
 * libjpeg refuses (JERR_HUFF_CLEN_OVERFLOW): the image's status is FEAR_JPEG_ENC_HUFF_DEPTH, its length 0 and its slot untouched; the
 * other images are unaffected.  fear_jpeg_encode_bound_flags is the bound of a record with these flags: with per-file tables any code
 * may be 16 bits long, so a block is at most 16 + 11 + 63 x 26 = 1665 bits, luma or chroma (MCUs of 9990, 6660, 4995 and 1665 bits), and
 * the header at most the standard one.
 * fear_jpeg_huff_optimal runs the table stage alone on n histograms of 256 uint32 counts on the device: counts_dev (n, 16) codes per
 * length, values_dev (n, 256) of which nvalues_dev[i] are written, codes_dev (n, 256) length << 16 | code per symbol (0: no code),
 * status_dev[i] FEAR_TRAIN_OK or FEAR_JPEG_ENC_HUFF_DEPTH (counts, codes and nvalues zeroed).  Any counts are safe.  n outside
 * 0..4 x 65535 (the tables of the largest encode call): FEAR_TRAIN_ERR_SHAPE; n == 0 returns FEAR_TRAIN_OK without a launch; a null
 * pointer with n > 0: FEAR_TRAIN_ERR_NULL.                                                                                        */
#define FEAR_JPEG_ENC_OVERFLOW 1
#define FEAR_JPEG_ENC_HUFF_DEPTH 2
#define FEAR_JPEG_ENC_OPTIMIZE 1u        /* a record's flags: per-file Huffman tables */
#define FEAR_JPEG_ENC_HEADER_MAX 640
#define FEAR_JPEG_ENC_GROUP_BLOCKS 256
#define FEAR_JPEG_ENC_CHUNK_BYTES 4096
#define FEAR_JPEG_ENC_TABLE_BYTES(n) (((size_t)(n) * 96 + 15) & ~(size_t)15)
/* A record's sampling: the file's layout.  FEAR_JPEG_ENC_GRAY writes one component from a (height, width) uint8 source, or, with
 * FEAR_JPEG_ENC_GRAY_RGB or-ed in, from the luma of a (height, width, 3) RGB source. */
#define FEAR_JPEG_ENC_420 0
#define FEAR_JPEG_ENC_422 1
#define FEAR_JPEG_ENC_444 2
#define FEAR_JPEG_ENC_GRAY 3
#define FEAR_JPEG_ENC_GRAY_RGB 0x100

/* One image of a fear_jpeg_encode_u8 call.  96 bytes. */
typedef struct FearJpegEncImage {
    const uint8_t* src;              /* device: (height, width, 3) uint8 RGB, contiguous; (height, width) for plain gray    */
    uint8_t* out;                    /* device: the file's slot                                                            */
    const uint8_t* header;           /* device: header_bytes bytes, SOI to the end of SOS                                  */
    uint64_t stream_offset;          /* plan: the unstuffed stream, bytes from the workspace's start; offset 24             */
    uint64_t work_offset;            /* plan: coefficients, bit offsets, segment and chunk tables                          */
    int32_t width, height, quality, restart_interval;        /* offset 40                                                  */
    uint32_t out_cap, header_bytes;  /* offset 56                                                                          */
    uint32_t stream_cap;             /* plan: the stream's capacity in bytes; offset 64                                    */
    uint32_t start[4];               /* plan: the image's first workgroup of transform, sizes / write, segments, count / assemble */
    uint32_t sampling;               /* FEAR_JPEG_ENC_420 .. _GRAY, | FEAR_JPEG_ENC_GRAY_RGB; 0: 4:2:0 from RGB; offset 84      */
    uint32_t plan_sampling;          /* plan: the sampling | flags << 16 the plan was made for: a later change is refused     */
    uint32_t flags;                  /* 0 or FEAR_JPEG_ENC_OPTIMIZE; offset 92                                                 */
} FearJpegEncImage;
#ifdef __cplusplus
static_assert(sizeof(FearJpegEncImage) == 96, "FearJpegEncImage is 96 bytes");
#else
_Static_assert(sizeof(FearJpegEncImage) == 96, "FearJpegEncImage is 96 bytes");
#endif

int fear_jpeg_encode_header(int width, int height, int quality, int restart_interval, uint8_t* out, size_t out_cap, size_t* out_used);
size_t fear_jpeg_encode_bound(int width, int height, int restart_interval);
int fear_jpeg_encode_header_mode(int width, int height, int quality, int restart_interval, int sampling, uint8_t* out, size_t out_cap,
                                 size_t* out_used);
size_t fear_jpeg_encode_bound_mode(int width, int height, int restart_interval, int sampling);
int fear_jpeg_encode_header_flags(int width, int height, int quality, int restart_interval, int sampling, uint32_t flags, uint8_t* out,
                                  size_t out_cap, size_t* out_used);
size_t fear_jpeg_encode_bound_flags(int width, int height, int restart_interval, int sampling, uint32_t flags);
int fear_jpeg_encode_plan(FearJpegEncImage* images, int n);
size_t fear_jpeg_encode_workspace_bytes(const FearJpegEncImage* images, int n);
int fear_jpeg_encode_u8(const FearJpegEncImage* images, int n, void* workspace, size_t workspace_bytes, int32_t* length_dev,
                        int32_t* status_dev, void* stream);
int fear_jpeg_huff_optimal(const uint32_t* freq_dev, int n, uint8_t* counts_dev, uint8_t* values_dev, int32_t* nvalues_dev,
                           uint32_t* codes_dev, int32_t* status_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FEAR_TRAIN_H */
