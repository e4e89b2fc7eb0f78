/*
 * usseg.h - C ABI of libusseg_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * ResNeSt/UNet segmentation hot path of silverlight6/Ultrasound_Modeling.
 *
 * The reference (TensorFlow/Keras) has no FFI or operator boundary of its own: every
 * kernel it runs is implicit inside tf.keras.layers.*.  Each entry point below therefore cites the
 * reference call sites whose implicit framework kernel it replaces (paths relative to the reference
 * repo root).  INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Contract (all functions)
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated otherwise;
 *  - the caller owns every buffer, including workspaces; the library allocates no device memory,
 *    never synchronises and never throws.  Mutable host state is THREAD-LOCAL: the error string; the queue of
 *    deferred finishing reductions of every stream between usseg_defer_begin() and usseg_defer_end() (defer.hip);
 *    the opt-in launch timer of usseg_prof_* (runtime.hip) - so host threads that drive different streams do not
 *    share any of it (a stream's begin / launches / flush / end come from one thread).  Process-wide state: the USSEG_*
 *    planner switches, each read from the environment at its first use and kept, five test knobs on every call; and the
 *    dynamic-LDS opt-in table (runtime.hip), guarded by a mutex, which records per (device, kernel) the largest size
 *    granted - a failed opt-in is returned by the call that needed it;
 *  - one producer per destination between two flushes is NOT required: deferred finishes that share a
 *    destination are issued as separate, stream-ordered launches (defer.hip);
 *  - all work is enqueued on the hipStream_t passed in (graph-capture safe);
 *  - return value: 0 on success, negative UssegStatus on error (usseg_last_error() has the text).
 *
 * Data layout
 *  - activations: NHWC, bf16, channel stride `ld` (elements) >= C; C and ld are multiples of 8 and
 *    the base pointer is 16-byte aligned, so a pixel's channels can be read 8 at a time.  Channels
 *    beyond the layer's logical width are kept exactly zero by every kernel ("pad channels").
 *  - packed conv operand ("Wp"): bf16 matrix [Nrows][Kw], Nrows = roundup(N,16), K index =
 *    tap*Cin + c  (Cin = physical input channels of the op), row stride Kw = ntaps*Cin.
 *    Built from the fp32 Keras-layout master weights by usseg_pack_weight().
 *  - per-channel vectors (bias, gamma, beta, ...) are fp32, padded with zeros to the physical width.
 */
#ifndef USSEG_H
#define USSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* usseg_stream_t; /* a hipStream_t */

typedef enum UssegStatus {
  USSEG_OK = 0,
  USSEG_ERR_BAD_ARG = -1,
  USSEG_ERR_UNSUPPORTED = -2,
  USSEG_ERR_LAUNCH = -3
} UssegStatus;

typedef enum UssegAct { USSEG_ACT_NONE = 0, USSEG_ACT_LRELU = 1, USSEG_ACT_RELU = 2, USSEG_ACT_ELU = 3, USSEG_ACT_GELU = 4 } UssegAct;

enum {
  USSEG_OUT_F32 = 1,   /* y is float* (ldy counted in floats); default bf16 */
  USSEG_ACCUMULATE = 2 /* y += result (residual pointer == y is also allowed) */
};

/* Geometry of one Conv2D (stride 1, SAME, dilation d) or Conv2DTranspose (stride 2, SAME). */
typedef struct UssegConvDesc {
  int32_t B, H, W;     /* batch and INPUT spatial size of the forward op (tconv output is 2H x 2W) */
  int32_t Cin, Cout;   /* physical channel counts (multiples of 8) of the forward input / output */
  int32_t ldx, ldy;    /* channel strides (elements) of the forward input / output buffers */
  int32_t ksize;       /* conv: 1 or 3; tconv: 3 or 4 */
  int32_t dilation;    /* conv only */
  int32_t act;         /* UssegAct fused into the forward epilogue */
  float alpha;         /* LeakyReLU / ELU alpha */
  int32_t flags;       /* USSEG_OUT_F32 | USSEG_ACCUMULATE */
} UssegConvDesc;

const char* usseg_last_error(void);
int usseg_version(void);

/* ---- convolution: Conv2D 3x3 / dilated 3x3 / 1x1, stride 1, SAME -------------------------------
 * replaces tf.keras.layers.Conv2D at ResNest.py:14,17,21,77,82,122,128,160,166; Decoder.py:11-25,
 * 36-50,103; VisionTransformer.py:106; TBI_ResNest.py:83,85,88,140,143,162,167,189,195.
 * y = act(conv(x, Wp) + bias) (+ residual).  bias may be NULL; residual (bf16, stride ldr) may be NULL. */
int usseg_conv2d_fwd(const UssegConvDesc* d, const void* x, const void* wp_fwd, const float* bias,
                     const void* residual, int32_t ldr, void* y, usseg_stream_t stream);
/* Conv2D followed by an inference-mode BatchNormalization and the activation in ONE pass (ResNest.py:17-23; Decoder.py:67-76):
 * y = act(scale[n] * conv(x, Wp)[n] + shift[n]) with scale = gamma*rsqrt(var+eps), shift = beta - mean*scale + scale*conv_bias
 * (usseg_bn_fold_batched builds both).  The pre-normalisation tensor is never written; the backward recovers what it needs
 * from y (usseg_norm_act_bwd mode 2). */
int usseg_conv2d_fwd_affine(const UssegConvDesc* d, const void* x, const void* wp_fwd, const float* scale, const float* shift,
                            const void* residual, int32_t ldr, void* y, usseg_stream_t stream);
typedef struct UssegBnFoldJob {   /* one BatchNormalization layer (device pointers; C logical, Cp physical channels) */
  const float *gamma, *beta, *mean, *var;
  const float* bias;               /* bias of the conv in front of it, or NULL */
  float *scale, *shift;            /* outputs, Cp floats each (zero past C) */
  int32_t C, Cp;
  float eps;
  int32_t reserved;
} UssegBnFoldJob;
int usseg_bn_fold_batched(const UssegBnFoldJob* jobs_dev, int32_t njobs, usseg_stream_t stream);
/* dx = conv_transpose(dy, W) (+ residual): the backward-data of the op above.  wp_dgrad is the operand
 * packed with in/out swapped (K index = tap*Cout + co).  dx has d->Cin channels, stride d->ldx. */
int usseg_conv2d_dgrad(const UssegConvDesc* d, const void* dy, const void* wp_dgrad, const void* residual,
                       int32_t ldr, void* dx, usseg_stream_t stream);
/* dW[tap][ci][co] += sum_pixels x * dy, accumulated into a [ntaps][Cin][Cout] fp32 buffer (zeroed or holding a
 * running sum).  ws (may be NULL) is a caller-owned fp32 workspace of ws_floats floats for the split-K partial slabs of
 * the 3x3 kernel (any size helps; 9*Cin*Cout*512 is always enough); without it the partials are combined with atomics. */
int usseg_conv2d_wgrad(const UssegConvDesc* d, const void* x, const void* dy, float* dw_scratch, float* ws,
                       int64_t ws_floats, usseg_stream_t stream);

/* Backward-data of several parallel convolutions that read the SAME input (Decoder.py:67-75,79-87: conv*_1 1x1 and the three
 * dilated 3x3 convs) in one pass: dx = sum_b dgrad_b(dy[..., ch_off[b] : ch_off[b]+Cb]).  d: B,H,W, Cin/ldx of dx, ldy = channel
 * stride of the concatenated dy tensor.  wp_cat: bf16 [roundup(Cin,16)][Ktot], Ktot = sum_b ksize_b^2 * Cb, branch b's taps at
 * columns (taps before b)*Cb + tap*Cb + co (tap = kh*k + kw of the forward kernel).  At most 32 taps in total. */
int usseg_conv2d_dgrad_branches(const UssegConvDesc* d, int32_t nbranches, const int32_t* ksize, const int32_t* dilation,
                                const int32_t* ch_off, int32_t Cb, const void* dy, const void* wp_cat, const void* residual,
                                int32_t ldr, void* dx, usseg_stream_t stream);

/* Weight gradient written straight into the framework's variables: up to 4 rectangular blocks of the physical
 * [ntaps][Cin_phys][Cout_phys] gradient go to strided destinations (Keras kernel [k,k,Cin,Cout] / [k,k,Cout,Cin] with the
 * LOGICAL channel counts; one block per cardinal path for the block-diagonal grouped convs, ResNest.py:91-96).  Elements
 * outside every block (channel padding, off-diagonal blocks) are dropped.  dst[t*sT + i*sI + o*sO] += dW[t][i_off+i][o_off+o]. */
typedef struct UssegWgradBlock {
  float* dst;
  int64_t sT, sI, sO;          /* element strides of the destination per tap / input channel / output channel */
  int32_t i_off, o_off, ni, no; /* the block: input channels [i_off, i_off+ni), output channels [o_off, o_off+no) */
} UssegWgradBlock;
typedef struct UssegWgradDst {
  int32_t nblocks;             /* 1..4 */
  int32_t reserved;
  UssegWgradBlock blk[4];
} UssegWgradDst;
int usseg_conv2d_wgrad_mapped(const UssegConvDesc* d, const void* x, const void* dy, const UssegWgradDst* dst, float* ws,
                              int64_t ws_floats, usseg_stream_t stream);
int usseg_tconv2d_wgrad_mapped(const UssegConvDesc* d, const void* x, const void* dy, const UssegWgradDst* dst, float* ws,
                               int64_t ws_floats, usseg_stream_t stream);

/* Several independent 3x3 weight gradients in one launch (the DecoderBlock's dilation branches; the stem's three convs, ResNest.py:39-44): same
 * semantics as usseg_conv2d_wgrad / usseg_conv2d_wgrad_mapped per job (dst NULL: accumulate into dw; dst set: dw ignored).  The jobs share one
 * grid when they have the same (B, H, W), the same number of 128-pixel groups and - channel counts may differ - the same tile shape and tile
 * count of the halo kernel; otherwise they are launched one after the other. */
typedef struct UssegWgradJob {
  UssegConvDesc desc;
  const void* x;
  const void* dy;
  float* dw;
  const UssegWgradDst* dst;
} UssegWgradJob;
int usseg_conv2d_wgrad_multi(int32_t njobs, const UssegWgradJob* jobs, float* ws, int64_t ws_floats, usseg_stream_t stream);

/* Deferred finishing reductions.  Between usseg_defer_begin(stream, ...) and usseg_defer_end(stream) the small kernels
 * that add per-workgroup partial sums into gradient variables (the tail of usseg_norm_act_bwd, usseg_colsum,
 * usseg_conv2d_wgrad[_mapped], usseg_tconv2d_wgrad_mapped on that stream) are queued and run as a few batched launches at
 * usseg_defer_flush / _end (or earlier when a workspace fills).  The gradients those calls produce are therefore complete only
 * after the flush: flush before anything on the stream reads them (the optimiser; training-mode BatchNorm's backward fix).
 * The two workspaces (fp32, caller-owned, must outlive the end call) replace the per-call ws arguments while deferring;
 * either may be NULL to keep that family immediate.  One context per stream. */
int usseg_defer_begin(usseg_stream_t stream, float* reduce_ws, int64_t reduce_floats, float* wgrad_ws, int64_t wgrad_floats);
int usseg_defer_flush(usseg_stream_t stream);
int usseg_defer_end(usseg_stream_t stream);

/* Several independent 3x3 convolutions in ONE launch: the DecoderBlock's parallel dilation branches
 * (Decoder.py:14-25,39-50: the conv2_x / conv3_x / conv4_x layers read the same input and write disjoint channel slices of the
 * concatenated output, Decoder.py:67-75,79-87).  Semantics = usseg_conv2d_fwd / usseg_conv2d_dgrad called once per job
 * in order; the jobs must not depend on each other (disjoint outputs).  1 <= njobs <= 4.  Jobs that cannot share a
 * grid are launched one after the other.  Forward only: a 1x1 job (ksize 1, dilation 1: the block's conv1_x, Decoder.py:11-13) beside at
 * least one 3x3 job on the same input rides in their launch as a centre-tap-only job of the 3x3 geometry (its wp is the 1x1 conv's own
 * [N][Cin] operand). */
typedef struct UssegConvJob {
  UssegConvDesc desc;
  const void* x;        /* fwd: input x;  dgrad: dy */
  const void* wp;       /* packed operand (forward packing for fwd, in/out-swapped packing for dgrad) */
  const float* bias;    /* fwd only, may be NULL */
  const void* residual; /* bf16, may be NULL */
  int32_t ldr;
  int32_t reserved;
  void* y;              /* fwd: y;  dgrad: dx */
  const float* scale;   /* fwd only, may be NULL: y = act(scale[n]*conv + bias[n]) (folded inference BatchNorm, see _affine) */
} UssegConvJob;
int usseg_conv2d_fwd_multi(int32_t njobs, const UssegConvJob* jobs, usseg_stream_t stream);
int usseg_conv2d_dgrad_multi(int32_t njobs, const UssegConvJob* jobs, usseg_stream_t stream);

/* ---- transposed convolution: Conv2DTranspose 3x3 s2 (Decoder.py:57,120) and 4x4 s2 (TBI_ResNest.py:124,210),
 * padding 'same' (k=3: out[2i+k] += x[i] w[k], last row/col cropped; k=4: out[2i+k-1]).  Four parity-class
 * implicit GEMMs, no zero insertion. */
int usseg_tconv2d_fwd(const UssegConvDesc* d, const void* x, const void* wp_fwd, const float* bias, void* y,
                      usseg_stream_t stream);
int usseg_tconv2d_dgrad(const UssegConvDesc* d, const void* dy, const void* wp_dgrad, const void* residual,
                        int32_t ldr, void* dx, usseg_stream_t stream);
int usseg_tconv2d_wgrad(const UssegConvDesc* d, const void* x, const void* dy, float* dw_scratch,
                        usseg_stream_t stream);

/* ---- operand packing -------------------------------------------------------------------------
 * dst[(n_off+n)*Kw + tap*tap_stride + k_off + k] = bf16(src[tap*sT + n*sN + k*sK]),  n<Nn, k<Kk, tap<T.
 * Inverse (gradient gather): dst_f32[tap*sT + n*sN + k*sK] (+)= scale * scratch[tap][k_off+k][n_off+n],
 * scratch being the [T][Mrows][Ncols] fp32 output of a *_wgrad call. */
int usseg_pack_weight(const float* src, int64_t sT, int64_t sN, int64_t sK, int32_t T, int32_t Nn, int32_t Kk,
                      void* dst, int32_t Kw, int32_t tap_stride, int32_t n_off, int32_t k_off,
                      usseg_stream_t stream);
/* All packs of a model in one launch: `jobs_dev` is a DEVICE array of njobs descriptors (same fields as above).  usseg_pack_weight refuses
 * k_off + Kk > tap_stride and T*tap_stride > Kw; the two batched forms cannot read the device table and check nothing: a job may place its
 * segment at any k_off with Kk <= tap_stride and k_off + (T-1)*tap_stride + Kk <= Kw (the quad operands and the decoder's concatenated
 * backward-data operand do), and the jobs of one launch must write disjoint elements. */
typedef struct UssegPackJob {
  const float* src;
  void* dst;
  int64_t sT, sN, sK;
  int32_t T, Nn, Kk, Kw, tap_stride, n_off, k_off, reserved;
  const float* nscale; /* optional fp32 multiplier per row n (NULL = none): an inference BatchNormalization folded into the
                          FORWARD operand, W'[n][..] = W[n][..] * gamma[n]*rsqrt(var[n]+eps) (the conv then runs its plain
                          bias + activation epilogue with bias' = beta - mean*scale + scale*bias) */
} UssegPackJob;
int usseg_pack_weights_batched(const UssegPackJob* jobs_dev, int32_t njobs, usseg_stream_t stream);
/* Same packs, flat grid: tilemap = nblocks triples (job index, first 32x32 tile of that job, tile count) that cover every tile of
 * every job exactly once (tiles of a job are numbered tap-major, then 32-row blocks of n, then 32-column blocks of k). */
int usseg_pack_weights_flat(const UssegPackJob* jobs_dev, const int32_t* tilemap_dev, int32_t nblocks, usseg_stream_t stream);
int usseg_unpack_wgrad(const float* scratch, int32_t Mrows, int32_t Ncols, int32_t T, int32_t Nn, int32_t Kk,
                       int32_t n_off, int32_t k_off, float* dst, int64_t sT, int64_t sN, int64_t sK,
                       float scale, int32_t accumulate, usseg_stream_t stream);
/* Several unpacks in one launch (device-resident job table, static pointers): the per-branch blocks of a grouped gradient. */
typedef struct UssegUnpackJob {
  const float* scratch;
  float* dst;
  int64_t sT, sN, sK;
  int32_t Mrows, Ncols, T, Nn, Kk, n_off, k_off, accumulate;
  float scale;
  int32_t reserved;
} UssegUnpackJob;
int usseg_unpack_wgrad_batched(const UssegUnpackJob* jobs_dev, int32_t njobs, int32_t max_elems, usseg_stream_t stream);

/* ---- normalisation + activation (bf16 rows of C channels, G groups of Cg = C/G) ---------------
 * mode 0: LayerNormalization(axis=-1, eps) per pixel and per group (ResNest.py:86,125,132,164; Decoder.py:112)
 * mode 1: BatchNormalization in inference mode = per-channel affine with moving statistics
 *         (ResNest.py:19,23; Decoder.py:32-35,51-54; TBI_ResNest.py:90,144,164,169,190,213)
 * followed by act (LeakyReLU / ReLU / ELU / none).  mult scales the activated output (Arch A dropout = 2*mask). */
typedef struct UssegNormDesc {
  int64_t M;          /* pixels */
  int32_t C, Cphys;   /* logical channels, physical channels (multiple of 8; pad channels written as 0) */
  int32_t ldx, ldy;   /* channel strides of input and output */
  int32_t G;          /* groups (LN only), C % G == 0 */
  int32_t mode;       /* 0 LN, 1 affine, 2 (usseg_norm_act_bwd only) affine whose input x is the ACTIVATED output of usseg_conv2d_fwd_affine */
  float eps;
  int32_t act;
  float alpha;
  int32_t lddx;       /* usseg_norm_act_bwd: channel stride of dx (0 = ldx) */
} UssegNormDesc;
/* mask (may be NULL): bf16 tensor [M][ldm] multiplied into the ACTIVATED output (dropout: 0 or 1/keep; since the mask is
 * non-negative relu(bn(x)*mask) == relu(bn(x))*mask, TBI_ResNest.py:213-218); the backward applies it to dy.
 * gamma / beta / mean / var: fp32, 16-byte aligned, readable up to Cphys floats (only the first C are used). */
int usseg_norm_act_fwd(const UssegNormDesc* d, const void* x, const float* gamma, const float* beta,
                       const float* mean, const float* var, const void* mask, int32_t ldm, void* y, usseg_stream_t stream);
/* tf.nn.dropout mask (TBI_ResNest.py:216): mask = keep ? 1/(1-rate) : 0 from a counter-based hash of (seed, index). */
int usseg_dropout_mask(void* mask, int64_t M, int32_t C, int32_t ld, uint64_t seed, float rate, usseg_stream_t stream);
/* Same, with a device-resident step counter mixed into the seed (the optimiser's step variable): a captured HIP graph of the
 * training step then draws a fresh mask at every replay. */
int usseg_dropout_mask_step(void* mask, int64_t M, int32_t C, int32_t ld, uint64_t seed, const int32_t* step_dev, float rate,
                            usseg_stream_t stream);
/* *counter += inc on the device (one thread): advances a counter that usseg_dropout_mask_step reads, eagerly or inside a captured HIP graph. */
int usseg_counter_add(int32_t* counter, int32_t inc, usseg_stream_t stream);
/* dx, and dgamma/dbeta accumulated.  x is the SAME pre-normalisation input as in fwd. */
int usseg_norm_act_bwd(const UssegNormDesc* d, const void* x, const void* dy, const float* gamma, const float* beta,
                       const float* mean, const float* var, const void* mask, int32_t ldm, void* dx, float* dgamma,
                       float* dbeta, float* dbias, float* ws, usseg_stream_t stream);
/* LayerNormalization backward (mode 0, G = 1) + the residual branch around a pre-norm transformer block in one pass
 * (VisionTransformer.py:137-146, SwinTransformer.py:224-257: x = x + f(norm(x))): dx = bf16(bf16(LN backward) + dres) - the bits of
 * usseg_norm_act_bwd followed by usseg_copy_channels(accumulate).  dres: bf16 [M][lddres].  dbias (may be NULL) += the column sums
 * of the STORED dx: the bias gradient of the Dense layer whose output (plus a shortcut) this gradient belongs to (attention
 * projection / the previous block's fc2) - no usseg_colsum pass for it. */
int usseg_norm_act_bwd_res(const UssegNormDesc* d, const void* x, const void* dy, const float* gamma, const float* beta,
                           const void* dres, int32_t lddres, void* dx, float* dgamma, float* dbeta, float* dbias, float* ws,
                           usseg_stream_t stream);
/* The split attention of a residual_S stage (ResNest.py:171-199) folded into the norms on either side of it:
 *  - usseg_norm_act_fwd_gap: the norm + activation that produces the cardinal output ALSO writes, per image and workgroup, the
 *    partial sums of its (bf16) output over the pixels: gap_rows [B][nb][Cphys] - the global average pool of ResNest.py:179
 *    without a pass over the tensor (usseg_splitattn_mlp_fwd adds the nb rows);
 *  - usseg_norm_act_bwd_sa: the norm backward whose incoming gradient is the re-weighting's backward
 *    dy = sa_mult * sa_s[b][c] * dout + sa_dg[b][c]  (identical radix branches: R == 1 in the descriptor), formed in registers
 *    (replaces usseg_splitattn_apply_bwd_dy + the tensor it wrote).  d->M must be B * pixels-per-image. */
int usseg_norm_act_fwd_gap(const UssegNormDesc* d, const void* x, const float* gamma, const float* beta, const float* mean,
                           const float* var, void* y, int32_t B, int32_t nb, float* gap_rows, usseg_stream_t stream);
int usseg_norm_act_bwd_sa(const UssegNormDesc* d, const void* x, const void* dout, const float* gamma, const float* beta,
                          const float* mean, const float* var, int32_t B, const float* sa_s, const float* sa_dg, float sa_mult,
                          void* dx, float* dgamma, float* dbeta, float* dbias, float* ws, usseg_stream_t stream);
/* Two INDEPENDENT LayerNormalization + LeakyReLU backward passes as ONE launch: A plain (a residual_S stage's shortcut norm, ResNest.py:100-101),
 * B with the split-attention re-weighting's backward folded in as in usseg_norm_act_bwd_sa (conv2_bn, ResNest.py:143-144 behind :194-197).
 * Same results as the two calls (bitwise: the same tile kernel runs both roles).  USSEG_ERR_UNSUPPORTED, and nothing launched, when the pair
 * has no instantiation (channel widths other than a stage of ResNest.py, tensors below 32k pixels): the caller then makes the two calls. */
int usseg_norm_act_bwd_pair(const UssegNormDesc* da, const void* xa, const void* dya, const float* gamma_a, const float* beta_a, void* dxa,
                            float* dgamma_a, float* dbeta_a, float* dbias_a, const UssegNormDesc* db, const void* xb, const void* doutb,
                            const float* gamma_b, const float* beta_b, int32_t B, const float* sa_s, const float* sa_dg, float sa_mult, void* dxb,
                            float* dgamma_b, float* dbeta_b, float* dbias_b, float* ws, usseg_stream_t stream);
/* The encoder stem as ONE launch (ResNest.py:39-47): Conv2D(1->16) + LeakyReLU -> Conv2D(16->32) + inference BatchNormalization (its scale
 * folded into the packed operand w2, its shift = b2) + LeakyReLU -> Conv2D(32->32) -> BatchNormalization + LeakyReLU -> AveragePooling2D(2,2).
 * x [B,H,W,8 physical channels]; w1 [16][72], w2 [32][144], w3 [32][288]: the packed forward operands of usseg_conv2d_fwd; b1 [16], b2 [32],
 * b3 [32], gamma / beta / mean / var [32] fp32.  Outputs, all kept for the backward pass: y1 [B,H,W,16] and t1 [B,H,W,32] (activated),
 * c2 [B,H,W,32] (pre-norm convtmp_2 output), pooled [B,H/2,W/2,32].  A workgroup owns a 16x16 tile and recomputes the two inner convs on
 * its halo, so no intermediate is re-read from HBM; rounding points are those of the four unfused launches. */
int usseg_stem_fwd(int32_t B, int32_t H, int32_t W, const void* x, int32_t ldx, const void* w1, const float* b1, const void* w2, const float* b2,
                   const void* w3, const float* b3, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                   float alpha, void* y1, void* t1, void* c2, void* pooled, usseg_stream_t stream);
/* The same launch for inference: same inputs and checks, ONE output, pooled [B,H/2,W/2,32], bit-identical to what usseg_stem_fwd writes.
 * y1, t1 and c2 (the tensors only the backward pass reads, 80 of the 112 bf16 channels written per pixel) are not stored. */
int usseg_stem_fwd_infer(int32_t B, int32_t H, int32_t W, const void* x, int32_t ldx, const void* w1, const float* b1, const void* w2,
                         const float* b2, const void* w3, const float* b3, const float* gamma, const float* beta, const float* mean,
                         const float* var, float eps, float alpha, void* pooled, usseg_stream_t stream);
/* A stem conv's 3x3 backward-data pass + the backward of the layer in front of it, in ONE launch (GradientTape through ResNest.py:41-44 /
 * :39-41): dy [B,H,W,32] -> dx_in = conv3x3_backward_data(dy, wd) (wd = the packed operand of usseg_conv2d_dgrad, [Co][9*32]) -> then
 *   mode 2 (Co = 32): the folded inference BatchNormalization + LeakyReLU backward from the ACTIVATED tensor yact the forward stored
 *                     (= usseg_norm_act_bwd mode 2: dx, dgamma += , dbeta +=, dbias += sum dx);
 *   mode 0 (Co = 16): LeakyReLU backward from the activated tensor + column sums (= usseg_act_bwd_colsum: dx, dbias +=).
 * The intermediate gradient never goes to HBM (it stays fp32 in registers: the unfused pair rounds it to bf16 in between).
 * USSEG_ERR_UNSUPPORTED - nothing launched - for any other (Co, mode).  ws: usseg_reduce_ws_floats() floats. */
int usseg_conv3_dgrad_actbwd(int32_t B, int32_t H, int32_t W, const void* dy, int32_t lddy, const void* wd, int32_t Co, const void* yact, int32_t ldy,
                             int32_t mode, const float* gamma, const float* beta, const float* var, float eps, float alpha, void* dx,
                             int32_t lddx, float* dgamma, float* dbeta, float* dbias, float* ws, usseg_stream_t stream);
/* One residual_S stage's cardinal group AND shortcut as ONE launch (SURVEY.md section 2.2 "K3"; ResNest.py:136-147 per path - the `kpaths`
 * paths share the input, :99-101 shortcut): replaces, in the implicit TensorFlow graph of the reference, Conv2D(1x1) -> LayerNormalization ->
 * LeakyReLU -> Conv2D(3x3) -> LayerNormalization -> LeakyReLU (+ the reduce_mean of :179) per path and Conv2D(1x1) -> LayerNormalization ->
 * LeakyReLU of the shortcut.  One workgroup owns an 8x8-pixel tile (+1 halo) of one image in LDS.
 *   x [B,H,W,Cin] bf16; w1 [roundup(Up,16)][Cin], w2 [roundup(Vp,16)][9*Up] (block diagonal over the paths), wsc [Oc][Cin]: the packed
 *   forward operands of usseg_conv2d_fwd; b1/g1/be1 [Up]/[P*cv11], b2/g2/be2 [Vp]/[P*cvkk], bsc/gsc/besc [Oc] fp32 (per-path vectors back to back);
 *   outputs (all kept for the backward pass): u_raw, u [B,H,W,Up]; v_raw, y [B,H,W,Vp]; sc_raw, sc [B,H,W,Oc];
 *   gap_rows [B][ceil(H/8)*ceil(W/8)][Vp] fp32: per-tile sums of y over its pixels (consumed by usseg_splitattn_mlp_fwd).
 * Values are rounded to bf16 where the unfused launches round them.  usseg_cardinal_supported: 1 if a fused kernel exists for the
 * channel configuration (the four stages of ResNest.py with radix 3 / kpaths 3), else the caller runs the unfused launches. */
typedef struct UssegCardinalDesc {
  int32_t B, H, W;
  int32_t Cin;              /* physical input channels */
  int32_t P, cv11, cvkk;    /* paths; logical channels per path after the 1x1 / the 3x3 (ResNest.py:120-121) */
  int32_t Up, Vp, Oc;       /* physical widths roundup(P*cv11, 8), roundup(P*cvkk, 8); shortcut / stage output channels */
  int32_t ldx, ldu, ldv, ldsc;
  float eps, alpha;         /* LayerNormalization epsilon, LeakyReLU slope */
} UssegCardinalDesc;
int32_t usseg_cardinal_supported(const UssegCardinalDesc* d);
int usseg_cardinal_fwd(const UssegCardinalDesc* d, const void* x, const void* w1, const float* b1, const float* g1, const float* be1,
                       const void* w2, const float* b2, const float* g2, const float* be2, const void* wsc, const float* bsc,
                       const float* gsc, const float* besc, void* u_raw, void* u, void* v_raw, void* y, float* gap_rows, void* sc_raw,
                       void* sc, usseg_stream_t stream);
/* The same launch for inference: the same descriptor (ldu is not read), weights and checks, and three outputs - y [B,H,W,Vp], gap_rows and
 * sc [B,H,W,Oc] - bit-identical to what usseg_cardinal_fwd writes.  u_raw, u, v_raw and sc_raw (read only by the backward pass) are not
 * stored.  usseg_cardinal_supported decides support for both entry points. */
int usseg_cardinal_fwd_infer(const UssegCardinalDesc* d, const void* x, const void* w1, const float* b1, const float* g1, const float* be1,
                             const void* w2, const float* b2, const float* g2, const float* be2, const void* wsc, const float* bsc,
                             const float* gsc, const float* besc, void* y, float* gap_rows, void* sc, usseg_stream_t stream);
/* The backward pass of the same stage half as ONE launch (K3 backward; GradientTape through ResNest.py:136-147 and :100-101): replaces the
 * split-attention re-weighting's backward + LayerNormalization/LeakyReLU backward of conv2_bn, the grouped 3x3's backward-data pass, the
 * LayerNormalization/LeakyReLU backward of conv1_bn, and the shortcut norm's backward.
 *   dout [B,H,W,Vp] (stride ldo): gradient w.r.t. the split-attention output (concats_1); sa_s / sa_dg [B][P*cvkk] fp32 from
 *   usseg_splitattn_bwd_fused: the gradient w.r.t. y is sa_mult*sa_s[b][c]*dout + sa_dg[b][c], formed in registers;
 *   dsc [B,H,W,Oc] (stride lddsc): gradient w.r.t. the activated shortcut; v_raw, u_raw, sc_raw: saved by usseg_cardinal_fwd;
 *   w2d [roundup(Up,16)][9*Vp]: the packed backward-data operand of the grouped 3x3 (block diagonal, as usseg_conv2d_dgrad takes it);
 *   outputs: dv [B,H,W,Vp] (stride d->ldv; gradient w.r.t. v_raw - the grouped 3x3's weight gradient reads it) and
 *   dcat [B,H,W,ldc] = [du_raw (Up) | dsc_raw (Oc)]: the gradients w.r.t. both 1x1 outputs, the operand of ONE backward-data GEMM and ONE
 *   weight-gradient launch (both 1x1 convs read the stage input);
 *   dg2/dbe2/db2, dg1/dbe1/db1, dgsc/dbesc/dbsc: gamma / beta gradients of the three norms and the bias gradients of the convs in front of
 *   them, ACCUMULATED (one partial row per workgroup + an ordered finishing reduction: bitwise reproducible);
 *   ws: usseg_reduce_ws_floats() floats.  A workgroup owns an 8x8 tile and recomputes the first norm's backward on its one-pixel halo. */
int usseg_cardinal_bwd(const UssegCardinalDesc* d, const void* dout, int32_t ldo, const void* dsc, int32_t lddsc, const void* v_raw,
                       const void* u_raw, const void* sc_raw, const void* w2d, const float* g2, const float* be2, const float* g1,
                       const float* be1, const float* gsc, const float* besc, const float* sa_s, const float* sa_dg, float sa_mult, void* dv,
                       void* dcat, int32_t ldc, float* dg2, float* dbe2, float* db2, float* dg1, float* dbe1, float* db1, float* dgsc,
                       float* dbesc, float* dbsc, float* ws, usseg_stream_t stream);
/* Inference BatchNormalization + activation + AveragePooling2D(2,2) in one pass - the stem's convtmp_2bn -> LeakyReLU ->
 * conv1_pool (ResNest.py:45-47) and conv2_1_2bn -> ELU -> pool_1 (TBI_ResNest.py:90-92): the activated full-resolution tensor
 * feeds the pool only, so it is never written.  x [B,H,W,Cphys] pre-norm; y / dy [B,H/2,W/2,Cphys]; dx [B,H,W,Cphys] is the
 * gradient w.r.t. x; dgamma / dbeta / dbias (= sum of dx: the producing conv's bias gradient, may be NULL) accumulate.
 * Bit-identical to usseg_norm_act_fwd + usseg_avgpool2_fwd (resp. avgpool2_bwd + norm_act_bwd). */
int usseg_bn_act_pool_fwd(const void* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Cphys, int32_t ldx, const float* gamma,
                          const float* beta, const float* mean, const float* var, float eps, int32_t act, float alpha, void* y,
                          int32_t ldy, usseg_stream_t stream);
int usseg_bn_act_pool_bwd(const void* x, const void* dy, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Cphys, int32_t ldx,
                          int32_t lddy, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                          int32_t act, float alpha, void* dx, int32_t lddx, float* dgamma, float* dbeta, float* dbias, float* ws,
                          usseg_stream_t stream);
/* Every per-channel reduction (norm backward, colsum, channel_stats, split-attention reductions) writes one partial
 * row per workgroup into the caller's fp32 workspace `ws` (at least usseg_reduce_ws_floats() floats) and a finishing
 * kernel ADDS the column sums to the destination: no atomics, bitwise reproducible.
 * usseg_norm_act_bwd: dgamma/dbeta += ...; dbias (may be NULL) += sum over pixels of dx, i.e. the bias gradient of
 * the convolution that produced x. */
int64_t usseg_reduce_ws_floats(void);
/* BatchNormalization training mode statistics: sum[c] += sum_m x, sumsq[c] += sum_m x^2. */
int usseg_channel_stats(const void* x, int64_t M, int32_t C, int32_t ldx, float* sum, float* sumsq, float* ws,
                        usseg_stream_t stream);

/* BatchNormalization TRAINING mode (Keras semantics: batch mean, biased variance, moving statistics *= momentum).
 * forward : usseg_bn_batch_stats (or usseg_channel_stats -> usseg_bn_finalize_stats) -> usseg_norm_act_fwd(mode 1, mean/var = batch statistics);
 * backward: usseg_norm_act_bwd(mode 1) with ZEROED scratch tg/tb as dgamma/dbeta, then usseg_bn_train_bwd_fix
 *           (dx -= gamma*rstd*(tb + xhat*tg)/M), then add tg/tb to the real gradients. */
int usseg_bn_finalize_stats(const float* sum, const float* sumsq, int64_t M, int32_t C, float momentum, float* mean, float* var,
                            float* moving_mean, float* moving_var, usseg_stream_t stream);
/* The forward's statistics in one call: mean / var (C floats each) are OVERWRITTEN with the batch mean and biased variance, taken as sums
 * of x - x[pixel 0] (no cancellation when |mean| >> std, which the one-pass sum x^2 / M - mean^2 of usseg_bn_finalize_stats has);
 * moving statistics (both or neither) *= momentum as above; ws: usseg_reduce_ws_floats() floats. */
int usseg_bn_batch_stats(const void* x, int64_t M, int32_t C, int32_t ldx, float momentum, float* mean, float* var, float* moving_mean,
                         float* moving_var, float* ws, usseg_stream_t stream);
int usseg_bn_train_bwd_fix(const void* x, void* dx, int64_t M, int32_t C, int32_t Cphys, int32_t ldx, int32_t lddx, const float* gamma,
                           const float* mean, const float* var, float eps, const float* tg, const float* tb, usseg_stream_t stream);

/* ---- plain activation (conv1 + LeakyReLU, ResNest.py:39-40; TBI_ResNest.py:83-87) -------------
 * y may be x, and dx may be dy (same stride): every 16-byte chunk is read and written by exactly one thread, once. */
int usseg_act_fwd(const void* x, int64_t M, int32_t C, int32_t ldx, int32_t ldy, int32_t act, float alpha, void* y,
                  usseg_stream_t stream);
int usseg_act_bwd(const void* x, const void* dy, int64_t M, int32_t C, int32_t ldx, int32_t lddy, int32_t lddx,
                  int32_t act, float alpha, void* dx, usseg_stream_t stream);
/* act_bwd that also accumulates db[c] += sum_m dx[m][c] (C logical channels): the bias gradient of the conv whose fused
 * activation it undoes (ResNest.py:39-40), in the same pass.  ws: usseg_reduce_ws_floats() floats. */
int usseg_act_bwd_colsum(const void* x, const void* dy, int64_t M, int32_t C, int32_t ldx, int32_t lddy, int32_t lddx, int32_t act,
                         float alpha, void* dx, float* db, float* ws, usseg_stream_t stream);

/* ---- AveragePooling2D(2,2) (ResNest.py:25-28,47-53; TBI_ResNest.py:92-107) -------------------- */
int usseg_avgpool2_fwd(const void* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldx, int32_t ldy, void* y,
                       usseg_stream_t stream);
/* dx = 0.25 * dy[h/2,w/2] (+ add, bf16 stride ldadd, may be NULL) */
int usseg_avgpool2_bwd(const void* dy, int32_t B, int32_t H, int32_t W, int32_t C, int32_t lddy, int32_t lddx,
                       const void* add, int32_t ldadd, void* dx, usseg_stream_t stream);
/* avgpool2_bwd that also accumulates db[c] += sum over the pixels of dx: dx is the gradient w.r.t. the output of the conv in front of
 * the pool (a residual_S stage's concats_2, ResNest.py:98,49-54), so this is that conv's bias gradient.  C <= 512. */
int usseg_avgpool2_bwd_colsum(const void* dy, int32_t B, int32_t H, int32_t W, int32_t C, int32_t lddy, int32_t lddx, const void* add,
                              int32_t ldadd, void* dx, float* db, float* ws, usseg_stream_t stream);

/* ---- channel-slice copy / accumulate: tf.concat(axis=3) and the raw reshape re-injection
 * (ResNest.py:96; Decoder.py:66,75,87,140-141; TBI_ResNest.py:110-122,139) ---------------------- */
int usseg_copy_channels(const void* src, int64_t M, int32_t C, int32_t lds, void* dst, int32_t ldd, int32_t accumulate,
                        usseg_stream_t stream);
/* fp32/fp64 NHWC host-layout input -> bf16 with the channel count padded to Cphys (ResNest.py:39 input cast) */
int usseg_cast_input(const void* src, int32_t src_is_f64, int64_t M, int32_t C, void* dst, int32_t Cphys,
                     usseg_stream_t stream);
int usseg_cast_bf16_to_f32(const void* src, int64_t M, int32_t C, int32_t lds, float* dst, usseg_stream_t stream);

/* ---- split attention (ResNest.py:171-199; TBI_ResNest.py:175-207) ----------------------------
 * Tensors: y [B,HW,P*R*Cg] bf16 (P cardinal paths, R distinct radix branches, Cg=cvkk channels each).
 * gap:    g[b][c] = sum_hw y[b,hw,c]                                  (fp32, zeroed by caller)
 * mlp:    per (b,path): a = act(norm(dense1(mult/HW * sum_r g))) ; z_r = dense2_r(a) ; s_r = softmax_c(z_r)
 * apply:  out[b,hw,p,c] = mult * sum_r y[b,hw,p,r,c] * s[b,p,r,c]
 * In the reference's Arch B the R branches share weights and are identical: R=1, mult=radix. */
typedef struct UssegSplitAttnDesc {
  int32_t B, HW;
  int32_t P, R, Cg, Hd;     /* paths, distinct radix branches, channels per branch, hidden = Cg/2 */
  int32_t ldy, ldo;         /* channel strides of y and out */
  int32_t Cy_phys, Co_phys; /* physical widths of y and out (pads written as zero in out) */
  float mult;               /* radix multiplicity of identical branches (Arch B) or 1 (Arch A) */
  int32_t norm_mode;        /* 0 LN (Arch B), 1 affine/BN-inference (Arch A) */
  float eps;
  int32_t act;              /* LeakyReLU (B) / ELU (A) */
  float alpha;
  int32_t use_sigmoid;      /* radix == 1 (ResNest.py:189-190) */
} UssegSplitAttnDesc;
/* parameter block for the tiny MLP, all fp32, per path p: w1[p][Cg][Hd], b1[p][Hd], gamma/beta/mean/var[p][Hd],
 * w2[p][R][Hd][Cg], b2[p][R][Cg] */
typedef struct UssegSplitAttnParams {
  const float *w1, *b1, *gamma, *beta, *mean, *var, *w2, *b2;
} UssegSplitAttnParams;
typedef struct UssegSplitAttnGrads {
  float *w1, *b1, *gamma, *beta, *w2, *b2;
} UssegSplitAttnGrads;
/* g[b][c] = sum_hw y[b,hw,c] (g is OVERWRITTEN: no pre-zeroing needed) */
int usseg_splitattn_gap(const UssegSplitAttnDesc* d, const void* y, float* g, float* ws, usseg_stream_t stream);
/* ws: fp32 workspace of usseg_splitattn_ws_floats(d) floats holding the saved MLP intermediates */
int64_t usseg_splitattn_ws_floats(const UssegSplitAttnDesc* d);
/* g = pooled sums as [B][g_rows][g_stride] partial rows which the kernel adds up: (1, Cy) for the vector usseg_splitattn_gap
 * wrote, or the rows usseg_norm_act_fwd_gap produced (g_rows = its nb, g_stride = Cphys) - no pooling pass, no finishing launch */
int usseg_splitattn_mlp_fwd(const UssegSplitAttnDesc* d, const float* g, int32_t g_rows, int32_t g_stride,
                            const UssegSplitAttnParams* p, float* s, float* ws, usseg_stream_t stream);
int usseg_splitattn_apply_fwd(const UssegSplitAttnDesc* d, const void* y, const float* s, void* out,
                              usseg_stream_t stream);
/* backward: (1) ds[b][p][r][c] = sum_hw mult*y*dout (ds is OVERWRITTEN) (2) MLP backward -> dg, param grads
 * (3) dy = mult*s*dout + dg*mult/HW */
int usseg_splitattn_apply_bwd_reduce(const UssegSplitAttnDesc* d, const void* y, const void* dout, int32_t lddo,
                                     float* ds, float* ws, usseg_stream_t stream);
/* grad_ws: usseg_splitattn_mlp_bwd_ws_floats(d) floats - one row of parameter-gradient partials per (path, image); the rows
 * are added into the variables in image order by a finishing reduction (no float atomics: bitwise reproducible). */
int64_t usseg_splitattn_mlp_bwd_ws_floats(const UssegSplitAttnDesc* d);
int usseg_splitattn_mlp_bwd(const UssegSplitAttnDesc* d, const float* g, int32_t g_rows, int32_t g_stride,
                            const UssegSplitAttnParams* p, const float* s, const float* ws, const float* ds, float* dg,
                            const UssegSplitAttnGrads* grads, float* grad_ws, usseg_stream_t stream);
/* usseg_splitattn_apply_bwd_reduce + usseg_splitattn_mlp_bwd as one call with no finishing launch between them: the MLP kernel adds the
 * reduce kernel's per-workgroup rows (in `reduce_ws`, usseg_reduce_ws_floats()) itself.  Outputs: dg [B][P*R*Cg] and the parameter gradients. */
int usseg_splitattn_bwd_fused(const UssegSplitAttnDesc* d, const void* y, const void* dout, int32_t lddo, const float* g, int32_t g_rows,
                              int32_t g_stride, const UssegSplitAttnParams* p, const float* s, const float* ws, float* dg,
                              const UssegSplitAttnGrads* grads, float* reduce_ws, float* grad_ws, usseg_stream_t stream);
int usseg_splitattn_apply_bwd_dy(const UssegSplitAttnDesc* d, const void* dout, int32_t lddo, const float* s,
                                 const float* dg, void* dy, int32_t lddy, usseg_stream_t stream);

/* ---- head softmax + loss ---------------------------------------------------------------------
 * logits fp32 [M][ldl] (C classes) -> probs fp32 [M][C] (Decoder.py:121; TBI_ResNest.py:125).
 * loss_kind 0: CategoricalCrossentropy(label_smoothing, reduction NONE) summed and divided by the GLOBAL batch
 *              (VisionTransformer.py:205,225-227); loss[0] receives the scalar.
 * loss_kind 1: my_loss_cat (TBI_ResNest.py:234-248) with precomputed per-pixel-per-class scale[HW][C];
 *              loss_map [HW] is overwritten.
 * dlogits (bf16 [M][lddl], may be NULL) = d(sum loss)/d logits. */
typedef struct UssegLossDesc {
  int64_t M;            /* B*H*W pixels */
  int32_t HW;           /* pixels per image */
  int32_t C, ldl, lddl; /* classes, logits stride (floats), dlogits stride (bf16 elements) */
  int32_t loss_kind;
  float label_smoothing;
  float clip_eps;       /* 1e-7 */
  float inv_global_batch;
  int32_t quad_w;       /* 0: logits/dlogits are [M][ldl]; W (full-resolution width): they are in the space-to-depth layout
                           [B][H/2][W/2][16] that the 2x2-tap form of the stride-2 head produces, pixel (y,x) in slot
                           4*((y&1)*2+(x&1)) (ldl = lddl = 16, C <= 4).  probs and y_true are always [M][C]. */
} UssegLossDesc;
/* Reproducible scalar accumulators (loss of loss_kind 0, usseg_sumsq): the pointer names USSEG_ACC_FLOATS floats -
 * [0] the result (OVERWRITTEN by every call), [1] a ticket counter (zero between calls), [2..] one partial per workgroup; the
 * last workgroup to arrive adds the partials in workgroup order, so no float atomics and the same bits on every run.  Zero the
 * whole buffer once at allocation; no per-call zeroing.  The loss map of loss_kind 1 is [HW] floats, each pixel owned by one
 * thread and OVERWRITTEN. */
#define USSEG_ACC_FLOATS 2050
int usseg_softmax_loss_fwd_bwd(const UssegLossDesc* d, const float* logits, const float* y_true, const float* scale,
                               float* probs, float* loss, void* dlogits, usseg_stream_t stream);
/* The quad-form head conv (bias included), its softmax and the loss of loss_kind 0 in ONE launch: replaces usseg_quad_bias_expand +
 * usseg_conv2d_fwd (fp32 quad logits) + usseg_softmax_loss_fwd_bwd (quad_w != 0) - the reference's
 * Conv2DTranspose(num_classes, 3, strides 2) -> Softmax -> CategoricalCrossentropy (Decoder.py:119-121,142; VisionTransformer.py:205,225-229).
 *   x [B,h,w,Cin_phys] bf16 (stride ldx); wq [16][9*Cin_phys] bf16: the quad operand (rows = parity class*4 + class, K = stencil tap*Cin_phys + channel);
 *   bias [C]; y_true [B,2h,2w,C] fp32 or NULL (probabilities only); probs [B,2h,2w,C] fp32; loss: USSEG_ACC_FLOATS floats ([0] is overwritten);
 *   dlogits [B,h,w,16] bf16 in the quad layout or NULL.  USSEG_ERR_UNSUPPORTED (nothing launched) when ceil(h/16)*ceil(w/16)*B exceeds the
 *   slots of the ordered sum, or Cin_phys is neither 72 (Decoder.py: the last block's 16 channels + the 56 re-injected ones) nor 16: the caller
 *   then runs the three calls. */
int usseg_head_quad_softmax_loss(const void* x, int32_t B, int32_t h, int32_t w, int32_t Cin_phys, int32_t ldx, const void* wq, const float* bias, int32_t C,
                                 const float* y_true, float* probs, float* loss, void* dlogits, float label_smoothing, float clip_eps,
                                 float inv_global_batch, usseg_stream_t stream);
/* The same two losses evaluated on PROBABILITIES, as the reference's public methods take them:
 * loss_kind 0 = VisionTransformer.compute_loss(y_true, y_pred) (VisionTransformer.py:225-227: Keras normalises the
 * probabilities by their class sum, clips to [clip_eps, 1-clip_eps], -sum_c y_smoothed*log p, summed / global batch into *loss);
 * loss_kind 1 = ResNest.my_loss_cat(y_true, y_pred) (TBI_ResNest.py:234-248: loss map [HW] -= y*log(p+1e-7)*scale[hw][c]).
 * probs, y_true fp32 [M][C]; only M, HW, C, loss_kind, label_smoothing, clip_eps, inv_global_batch of the descriptor are read.
 * loss is overwritten (loss_kind 0: a USSEG_ACC_FLOATS accumulator, [0] = the scalar). */
/* Accuracy metric of a step (TBI_ResNest.py:48-51; VisionTransformer.py:256-262): acc[0] = fraction of the M pixels whose
 * argmax(probs) equals argmax(y_true) (first maximum, as tf.argmax); probs, y_true fp32 [M][C].  acc is a USSEG_ACC_FLOATS
 * accumulator (zeroed once by the caller), [0] OVERWRITTEN.  One pass instead of the reference's four framework reductions. */
int usseg_accuracy(const float* probs, const float* y_true, int64_t M, int32_t C, float* acc, usseg_stream_t stream);
/* ---- validation metrics (metrics.hip) ---------------------------------------------------------
 * The counters behind the drivers' Keras Precision / Recall / MeanIoU objects and their `c2` pair (MainNumpy.py:20-27,49-53,
 * 100-106; TBI_ResNest.py:9-12,421-426; TBI_TransUNet.py:749-756,947-956; MainParallel.py:86-114,148-176), as exact integers:
 * one streaming pass over y_true and y_pred, contiguous fp32 [B][H][W][C] (the layout of probs and label2vec).  Per element:
 *  - round = 1: both values first go through tf.math.round, half to even (rintf): a label of exactly 0.5 - label2vec of a raw
 *    label 1.5 - counts as 0 (MainNumpy.py:49-50,100-101).  round = 0: the values as they are (TBI_ResNest.py:423-426);
 *  - a true value is positive when it is non-zero (Precision / Recall cast y_true to bool), a prediction when it is > 0.5 (their
 *    default threshold);
 *  - the confusion-matrix class of a value is the value truncated to an integer (tf.math.confusion_matrix casts to int64; MeanIoU
 *    flattens its inputs and takes no argmax: MainNumpy.py:53,106);
 *  - the element is INVALID when either class lies outside [0, num_classes) or the prediction outside [0, 1] (TF raises for both).
 * counts: USSEG_SEG_COUNTS uint64, ADDED INTO (never cleared: the caller zeroes the buffer once, e.g. per epoch):
 *   [0..2] TP, FP, FN over every element;  [3..5] TP, FP, FN over the elements with w == W-1 only - the reference's
 *   `c2` metrics index y[:, :, -1] of a 4-D tensor, the last image COLUMN, not class 2 (MainNumpy.py:104-105);
 *   [6 .. 6+nc*nc) the confusion matrix cm[true][pred];  [6+nc*nc] the count of invalid elements.
 * 1 <= num_classes <= 4; B, H >= 0; W, C >= 1.  Integer adds: bitwise reproducible; no allocation, no synchronisation. */
typedef struct UssegSegCountDesc {
  int32_t B, H, W, C;
  int32_t num_classes; /* of the confusion matrix, 1..4 */
  int32_t round;       /* 0 or 1 */
} UssegSegCountDesc;
#define USSEG_SEG_COUNTS 23 /* 6 + 4*4 + 1 */
int usseg_seg_counts(const UssegSegCountDesc* d, const float* y_true, const float* y_pred, uint64_t* counts, usseg_stream_t stream);
/* ---- brain-mask cascade (cascade.hip; TBIEvaluator.py:221-252, use_brainMask=True) --------------------------------------------
 * The step between the brain-mask model and the bleed model, on the device.  probs: the mask model's fp32 [M][C_mask] (2 <= C_mask <= 4);
 * x: the bf16 input [M][ldx] as usseg_cast_input wrote it (ldx a positive multiple of 8; x and x_gated 16-byte aligned).  Pixel m is
 * gated iff probs[m*C_mask] > 0.5f, which is the reference's np.round(mask)[..., 0] == 1 (:224-225): round-half-to-even sends exactly
 * 0.5 to 0, and NaN is not gated.  A gated row of x_gated is ldx zeros, any other row a copy of x's (:226-227 zero all ten input
 * channels; 0.0 is exact in bf16, so zeroing after the cast gives the bits of the reference's zero-then-cast).  x_gated == x (in place)
 * is allowed and then rewrites only the gated rows.  mask (may be NULL): the gate as u8 [M]. */
int usseg_cascade_gate(const float* probs, int32_t C_mask, int64_t M, const void* x, int32_t ldx, void* x_gated, uint8_t* mask,
                       usseg_stream_t stream);
/* The evaluator's two maps of the bleed model's probabilities, fp32 [M][C] with C == 3: prob_map[m] = ((1 - p0) - 0.5f*p1) + p2 in fp32,
 * rounded in that order (:249-252; the reference evaluates it in float64), bleed_prob[m] = p2 (:239). */
int usseg_cascade_maps(const float* probs, int32_t C, int64_t M, float* prob_map, float* bleed_prob, usseg_stream_t stream);
int usseg_loss_from_probs(const UssegLossDesc* d, const float* probs, const float* y_true, const float* scale, float* loss,
                          usseg_stream_t stream);
/* ---- class loss: VisionTransformer.my_loss_cat and its focal variant (VisionTransformer.py:259-280) ----------------------------
 * The reference's second loss for Arch B, as executed.  Per pixel, with probabilities p[c], labels y[c], s = label_smoothing:
 *     ys[c] = y[c]*(1 - s) + s/C
 *     pc[c] = clip(p[c], clip_eps, 1 - clip_eps)            (:266; NOT divided by the class sum, unlike Keras' CCE of loss_kind 0)
 *     l     = -factor * sum_c w[c] * ys[c] * (1 - pc[c])^gamma * log(pc[c])
 *     d l / d p[c] = factor*w[c]*ys[c]*(gamma*(1-pc)^(gamma-1)*log(pc) - (1-pc)^gamma/pc) for clip_eps < p[c] < 1 - clip_eps, else 0
 * my_loss_cat as committed (:270): factor 3, w = class_factor, gamma 0.  Its focal line (:272-273,277): factor 1, w = 1, gamma = alpha.
 * gamma is 0 (no pow and no 1 - pc evaluated) or lies in [1, 8] (below 1 the derivative is unbounded at the clip edge); w[c] and factor
 * are finite and >= 0; only w[0..C) is read.  The struct is passed by reference and copied into the launch (it travels BY VALUE with it), so a captured graph holds its numbers.
 * The three entry points below are the class-loss forms of the three above; the descriptor must say loss_kind 2 and its
 * label_smoothing, clip_eps, inv_global_batch and geometry mean what they mean there.  The scalar is
 * inv_global_batch * sum over all pixels of l, through the same ordered sum (loss: USSEG_ACC_FLOATS floats, [0] OVERWRITTEN);
 * dlogits = d scalar / d logits. */
typedef struct UssegClassLoss {
  float w[8];   /* per-class weight */
  float gamma;  /* focal exponent: 0, or 1..8 */
  float factor; /* the reference's 3 ("if using class factor") or 1 */
} UssegClassLoss;
int usseg_softmax_loss_fwd_bwd_cl(const UssegLossDesc* d, const UssegClassLoss* cl, const float* logits, const float* y_true, float* probs,
                                  float* loss, void* dlogits, usseg_stream_t stream);
/* Fused head: gamma == 0 and gamma > 0 are separate instantiations of the kernel (the loss is a compile-time property of it).
 * USSEG_ERR_UNSUPPORTED - nothing launched - under the same conditions as the function above. */
int usseg_head_quad_softmax_loss_cl(const void* x, int32_t B, int32_t h, int32_t w, int32_t Cin_phys, int32_t ldx, const void* wq, const float* bias,
                                    int32_t C, const float* y_true, float* probs, float* loss, void* dlogits, float label_smoothing, float clip_eps,
                                    float inv_global_batch, const UssegClassLoss* cl, usseg_stream_t stream);
/* On PROBABILITIES (fp32 [M][C], like y_true).  as_map == 0: the scalar (compute_loss with this loss).  as_map != 0: loss is [HW] floats,
 * map[hw] = sum_b l[b][hw] (what my_loss_cat returns, :270 axis=[0,3]); inv_global_batch is not applied; one thread owns a pixel and walks
 * the batch in order. */
int usseg_loss_from_probs_cl(const UssegLossDesc* d, const UssegClassLoss* cl, const float* probs, const float* y_true, float* loss,
                             int32_t as_map, usseg_stream_t stream);
/* ---- region-overlap losses: soft Dice / Tversky, optionally plus CategoricalCrossentropy (csrc/overlap_loss.hip) ------------------
 * Not in the reference: the loss family people training a segmenter on rare classes reach for first.  On the head's fp32 probabilities
 * p[m][c] and the labels y[m][c] exactly as passed (no label smoothing in the overlap term; soft labels allowed), m over the M pixels
 * of THIS call, s = smooth, a = alpha, b = beta, g = power:
 *     I_c = sum_m p*y      P_c = sum_m p      Y_c = sum_m y
 *     N_c = I_c + s        D_c = (1-a-b)*I_c + a*P_c + b*Y_c + s        T_c = N_c / D_c
 *     L_ov = sum_c w[c] * (1 - T_c)^g
 *     loss = ce_weight * CCE + ov_weight * ov_scale * L_ov
 * CCE is loss_kind 0 above, exactly: Keras normalisation, clip_eps, label_smoothing, times inv_global_batch.  a = b = 0.5 is soft Dice
 * in the convention (2*I + 2*s)/(P + Y + 2*s): s is added to the numerator and to the denominator of the HALVED textbook fraction, so
 * the textbook smoothing constant is 2*s.  power is 1, or lies in [1, 4] (below 1, (1-T)^(g-1) is unbounded at T = 1: refused);
 * smooth > 0; alpha, beta, w[c], ov_weight, ce_weight finite and >= 0; only w[0..C) is read; C <= 4.  ov_scale (finite, >= 0) is the
 * caller's data-parallel weight of this call's overlap term: with the replicas' gradients SUM-reduced, B_local / global batch makes the
 * result the batch-weighted mean of the replicas' overlap losses (1 on one device).
 *     d loss / d p_c(m) = A_c*y_c(m) + B_c (+ the CCE term),   k_c = ov_weight*ov_scale*w[c]*g*(1-T_c)^(g-1),
 *     A_c = -k_c*(D_c - (1-a-b)*N_c)/D_c^2,   B_c = k_c*a*N_c/D_c^2;   dlogit_j = p_j*(G_j - sum_c p_c*G_c), fp32, ONE bf16 rounding.
 * The gradient at a pixel depends on sums over all pixels, so there are two launches behind a probabilities-only forward
 * (usseg_head_quad_softmax_loss / usseg_softmax_loss_fwd_bwd with y_true = NULL):
 *   usseg_overlap_loss_sums   reads probs and y_true (fp32 [M][C], 16-byte aligned) once; acc[0] = the scalar loss (OVERWRITTEN);
 *                             acc[2] = the CCE pixel sum; acc[4+c] = A_c; acc[8+c] = B_c; acc[16+c], [20+c], [24+c], [28+c] = I_c, P_c, Y_c, T_c.
 *   usseg_overlap_loss_bwd    reads probs, y_true and acc[4..12); writes dlogits bf16 [M][8] (lddl 8), or with quad_w the
 *                             space-to-depth layout [B][H/2][W/2][16] (lddl 16) of UssegLossDesc; pad channels are exactly zero.
 * acc names acc_floats floats, USSEG_OVERLAP_ACC_FLOATS to hold every grid: [1] is a ticket counter (zero between calls), [32 + 16*b + k]
 * workgroup b's partial of value k.  The 3C + 1 totals are bitwise reproducible: fixed per-thread, per-wave and per-workgroup orders, the
 * partials published by a returning agent-scope exchange, and the last workgroup to arrive adds them in workgroup order (no float atomics,
 * no workgroup waits for another).  Zero the buffer once at allocation; no per-call zeroing.  The grid rule, part of the contract because
 * the rounding-error bound of the totals follows from it: usseg_overlap_loss_grid(M) = clamp(ceil(ceil(M/4)/256), 1, 512) workgroups of
 * 256 threads; a thread adds groups of 4 consecutive pixels, group index striding by 256*grid.
 * Of the descriptor only M, HW, C, lddl, quad_w, label_smoothing, clip_eps and inv_global_batch are read (M <= 2^29, a multiple of HW; M = 0
 * gives loss 0 and no backward launch).  The struct is passed by reference and copied into the launches (it travels BY VALUE with them), so a captured graph holds its numbers.  Every
 * argument is checked before any launch (USSEG_ERR_BAD_ARG with usseg_last_error text), an accumulator too small for the grid included. */
typedef struct UssegOverlapLoss {
  float w[8];      /* per-class weight */
  float alpha;     /* weight of the false positives (P - I) in the denominator */
  float beta;      /* weight of the false negatives (Y - I) */
  float smooth;    /* s > 0 */
  float power;     /* g: 1, or in [1, 4] */
  float ov_weight; /* weight of the overlap term */
  float ce_weight; /* weight of the CCE term; 0: not evaluated */
} UssegOverlapLoss;
#define USSEG_OVERLAP_ACC_FLOATS 8224 /* 32 + 16 * 512 workgroups */
int usseg_overlap_loss_grid(int64_t M);
int usseg_overlap_loss_sums(const UssegLossDesc* d, const UssegOverlapLoss* ol, float ov_scale, const float* probs, const float* y_true,
                            float* acc, int64_t acc_floats, usseg_stream_t stream);
int usseg_overlap_loss_bwd(const UssegLossDesc* d, const UssegOverlapLoss* ol, const float* probs, const float* y_true, const float* acc,
                           int64_t acc_floats, void* dlogits, usseg_stream_t stream);
/* ---- exact Euclidean distance maps (csrc/sdf.hip) ------------------------------------------------------------------------------------
 * usseg_sdf_labels: y_true fp32 [B,H,W,C] - the labels exactly as the loss kernels get them, C <= 4, soft labels allowed - -> phi fp32
 * [B,H,W,C], the layout of probs.  Per image and class the mask is y_c > thr (NaN is outside the mask).  With d(A) at a pixel the Euclidean
 * distance to the nearest pixel of the set A:
 *     outside the mask  phi = d(mask)              (the first pixel outside is 1)
 *     inside the mask   phi = 1 - d(not mask)      (the first pixel inside is 0)
 * which is Kervadec et al.'s signed distance map, scipy form  edt(~m)*~m - (edt(m) - 1)*m.  A class with no mask pixel in that image has
 * phi = 0 everywhere - and so has a class that covers the WHOLE image: a deliberate deviation (SciPy's distance_transform_edt of an image
 * without a background pixel is an arbitrary ramp; a class without a boundary has no boundary term).  Exactness is part of the contract:
 * squared distances are computed in int32 and are exact, and phi is the fp64 value (the square root of that integer; 1 minus it inside the
 * mask) rounded ONCE to fp32 - outside the mask the correctly rounded fp32 square root (double rounding is innocuous for square roots of
 * integers below 2^31).  A second call gives the same bits.
 * H and W each lie in [1, 8192], B in [0, 65535], B*H*W <= 2^29; anything else is USSEG_ERR_BAD_ARG before any launch, like a workspace
 * (16-byte aligned) of fewer than usseg_sdf_ws_bytes(B,H,W,C) bytes (-1 for a shape the transform refuses).  Nothing allocates; two launches.
 *
 * usseg_surface_dist: a, b uint8 [N,H,W] masks, nonzero = inside.  The surface S(m) is the set of mask pixels with at least one 4-neighbour
 * outside the mask, out-of-image counting as outside (medpy's / SciPy's  m & ~binary_erosion(m, border_value=0)).  Per image
 *     counters int64 [N,4] = |S(a)|, |S(b)|, max over S(a) of the SQUARED distance to S(b), max over S(b) of the squared distance to S(a)
 *     sums     fp64  [N,2] = sum over S(a) of the distance to S(b), sum over S(b) of the distance to S(a)
 * When either surface is empty both maxima are -1 and both sums 0.  The sums are bitwise reproducible: one workgroup per image and
 * direction, a thread adds its pixels in index order, the 256 partial sums are added as a fixed tree; no float atomics.  Hausdorff distance
 * = sqrt(max of the two maxima); average symmetric surface distance (medpy) = mean of sums[0]/|S(a)| and sums[1]/|S(b)|.  HD95 and the
 * surface Dice need a per-image selection: usseg_surface_stats below.  Same limits as above with N for B; workspace
 * usseg_surface_ws_bytes(N,H,W).
 *
 * usseg_surface_stats: usseg_surface_dist plus order statistics of the distances and counts within a tolerance - what HD95 (the 95th
 * percentile Hausdorff distance) and the surface Dice at a tolerance (normalised surface Dice, NSD; Nikolov et al., pixel-count form) need.
 * Per image, with S(a), S(b) as above:
 *     D_ab   the multiset of SQUARED Euclidean distances from each pixel of S(a) to the nearest pixel of S(b): exact int32, below 2^27
 *     D_ba   the same from S(b) to S(a);   D_pool  their multiset union;   all three empty if either surface is empty.
 * Order statistics.  For a set of size n >= 1 and a quantile t in [0, 1]:  pos = t * (double)(n - 1)  (ONE fp64 multiply),  k = floor(pos),
 * k1 = min(k + 1, n - 1).  The host passes t = q / 100 computed in fp64, so pos is Python's  q / 100 * (n - 1).  The device returns the pair
 * of squared distances of rank k and rank k1 (rank 0 the smallest), (-1, -1) for an empty set.  The host computes  g = pos - k,
 * lo = sqrt(d2_k), hi = sqrt(d2_k1)  in fp64 and  value = lo + (hi - lo) * g  - NumPy's linear percentile; q = 100 is the Hausdorff
 * distance, q = 0 the smallest distance.  Two conventions come from the one call:  pooled = the percentile of D_pool (medpy's hd95:
 * np.percentile(np.hstack((d_ab, d_ba)), 95));  directed = the larger of the percentiles of D_ab and D_ba (MONAI's).  NaN where either
 * surface is empty, as hd and assd.
 * Surface Dice at tolerance tau = (|{D_ab <= t2}| + |{D_ba <= t2}|) / (|S(a)| + |S(b)|) with t2 the largest integer whose square root
 * (the fp64 value, the distance as it is reported) is <= tau - the host computes it in integer arithmetic and passes it as an int32, which
 * makes d <= tau exact.  Both surfaces empty: NaN;
 * exactly one empty: 0.0 (no distance exists and the denominator is positive).
 *     quant  fp64  [P] HOST array, P in [0, 4], each finite and in [0, 1];   tol2 int32 [T] HOST array, T in [0, 4], each >= 0
 *            (both are copied by value into the kernel arguments: a captured graph holds them)
 *     counters int64 [N,4], sums fp64 [N,2]   usseg_surface_dist's, bit for bit (the same per-thread index order and tree)
 *     sel    int32 [N,3,P,2]   sets D_ab, D_ba, D_pool x quantile x (d2_k, d2_k1)
 *     within int64 [N,T,2]     |{D_ab <= tol2[t]}|, |{D_ba <= tol2[t]}|
 * With P == 0 (T == 0) quant and sel (tol2 and within) may be null.  Every output is a function of the inputs: the selection is an integer
 * radix select (most significant digit first, 8-bit digits, integer atomics in LDS), no sort, no float atomics, no host round trip.  Three
 * launches whatever the data; nothing allocates.  Limits as usseg_surface_dist; workspace usseg_surface_stats_ws_bytes(N,H,W) =
 * round16(4*N*H*W) + round16(8*N*H*W) bytes (the row distances, then the int32 [N,2,H,W] plane of squared distances), 16-byte aligned;
 * counters, sums and within 8-byte, sel 4-byte aligned; anything else is USSEG_ERR_BAD_ARG before any launch.  N == 0 launches nothing.
 * (A source pixel of an image whose OTHER surface is empty costs one read per image row: the emptiness is known only after the scan.) */
int64_t usseg_sdf_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t C);
int usseg_sdf_labels(const float* y_true, int32_t B, int32_t H, int32_t W, int32_t C, float thr, float* phi, void* ws, int64_t ws_bytes,
                     usseg_stream_t stream);
int64_t usseg_surface_ws_bytes(int32_t N, int32_t H, int32_t W);
int usseg_surface_dist(const uint8_t* a, const uint8_t* b, int32_t N, int32_t H, int32_t W, int64_t* counters, double* sums, void* ws,
                       int64_t ws_bytes, usseg_stream_t stream);
int64_t usseg_surface_stats_ws_bytes(int32_t N, int32_t H, int32_t W);
int usseg_surface_stats(const uint8_t* a, const uint8_t* b, int32_t N, int32_t H, int32_t W, const double* quant, int32_t P, const int32_t* tol2,
                        int32_t T, int64_t* counters, double* sums, int32_t* sel, int64_t* within, void* ws, int64_t ws_bytes,
                        usseg_stream_t stream);
/* ---- connected components (csrc/components.hip) ----------------------------------------------------------------------------------------
 * Masks are uint8 [N,H,W], nonzero = inside; components are 4- or 8-connected (any other connectivity is refused) and never cross an image.
 * H and W each lie in [1, 8192], N in [0, 65535], N*H*W <= 2^29; labels, count, prob and the hit tables are 4-byte, stats 8-byte and the
 * workspace 16-byte aligned; anything else is USSEG_ERR_BAD_ARG before any launch, like a workspace of fewer than
 * usseg_components_ws_bytes(N,H,W) bytes (-1 for a refused shape; 12 bytes per pixel plus 4 per image row).  N == 0 returns 0 without a
 * launch.  Nothing allocates and nothing synchronises with the host: every launch goes to `stream` in order, so a call captures as one
 * linear chain.  Every result is an integer sum, minimum or maximum: a second call gives the same bits.
 *
 * usseg_label_components: labels int32 [N,H,W] = 0 outside the mask and 1..K_n inside, the components of image n numbered in raster order
 * of their first (smallest linear index) pixel - scipy.ndimage.label's numbering, element for element; count int32 [N] = K_n.
 *
 * usseg_component_stats: stats int64 [N,cap,8]; row k-1 of image n describes the component with id k <= cap:
 *     area, y_min, x_min, y_max, x_max, sum of y, sum of x, peak
 * peak = the largest prob (fp32 [N,H,W], values in [0, 1]) over the component as its fp32 bit pattern widened to int64; a NaN never wins;
 * 0 when prob is null.  Rows of ids that do not exist are zero; ids above cap are skipped.  0 <= cap <= H*W.
 *
 * usseg_clean_mask: out uint8 [N,H,W] = 1 where the pixel belongs to a component of at least min_area pixels whose peak of prob is at least
 * min_peak (prob null: the area alone decides), else 0.  Areas and peaks are kept per component root in the workspace, not in a capped table:
 * right for any number of components.  out may alias mask.  min_area <= 1 with min_peak <= 0 (or no prob) copies the binarised mask.
 * A NaN min_peak is refused.
 *
 * usseg_component_overlap: two label images of one shape; hit_a int32 [N,cap_a], hit_a[n][k-1] = the number of pixels of a's component k
 * that lie inside any component of b; hit_b [N,cap_b] the other way round.  Ids above the caps are skipped. */
int64_t usseg_components_ws_bytes(int32_t N, int32_t H, int32_t W);
int usseg_label_components(const uint8_t* mask, int32_t N, int32_t H, int32_t W, int32_t connectivity, int32_t* labels, int32_t* count, void* ws,
                           int64_t ws_bytes, usseg_stream_t stream);
int usseg_component_stats(const int32_t* labels, const float* prob, int32_t N, int32_t H, int32_t W, int32_t cap, int64_t* stats,
                          usseg_stream_t stream);
int usseg_clean_mask(const uint8_t* mask, const float* prob, int32_t N, int32_t H, int32_t W, int32_t connectivity, int32_t min_area,
                     float min_peak, uint8_t* out, void* ws, int64_t ws_bytes, usseg_stream_t stream);
int usseg_component_overlap(const int32_t* labels_a, const int32_t* labels_b, int32_t N, int32_t H, int32_t W, int32_t cap_a, int32_t cap_b,
                            int32_t* hit_a, int32_t* hit_b, usseg_stream_t stream);
/* ---- the boundary term on top of the region-overlap losses (Kervadec et al.; csrc/overlap_loss.hip) ------------------------------------
 *     L_B = wb * ov_scale * (1/M) * sum_m sum_c u[c] * p_c(m) * phi_c(m)          loss = (the overlap loss above) + L_B
 * phi fp32 [M][C] (16-byte aligned) is usseg_sdf_labels' map of the same labels, M the pixels of this call, u[c] per-class weights (finite,
 * >= 0; only u[0..C) is read), ov_scale the same data-parallel factor the overlap term takes, and wb the boundary weight - read from DEVICE
 * memory when the kernel runs, so a captured graph follows a weight that grows during training.  The two entry points take everything
 * usseg_overlap_loss_sums / _bwd take and are further instantiations of the same two kernels:
 *   usseg_overlap_boundary_loss_sums   acc[0] = overlap loss + L_B;  acc[12] = L_B alone;  acc[13] = wb*ov_scale/M, the coefficient of
 *                                      u[c]*phi_c(m) in G_c(m);  every other slot as usseg_overlap_loss_sums leaves it.  The one extra total
 *                                      rides in the same ordered reduction (3C + 2 values a workgroup).
 *   usseg_overlap_boundary_loss_bwd    G_c(m) = A_c*y_c(m) + B_c + acc[13]*u[c]*phi_c(m) (+ the CCE term) in dlogit_j = p_j*(G_j - sum_c p_c*G_c):
 *                                      still ONE bf16 rounding of the fp32 value.  Reads acc[4..12) and acc[13].
 * With *wb == 0 the loss and every dlogits element equal the plain pair's bit for bit (pass 2 skips the summand when acc[13] is zero). */
typedef struct UssegBoundaryLoss {
  float u[8]; /* per-class weight of the boundary term */
} UssegBoundaryLoss; /* passed by reference, copied into the launches */
int usseg_overlap_boundary_loss_sums(const UssegLossDesc* d, const UssegOverlapLoss* ol, float ov_scale, const float* probs, const float* y_true,
                                     const float* phi, const UssegBoundaryLoss* bl, const float* wb, float* acc, int64_t acc_floats,
                                     usseg_stream_t stream);
int usseg_overlap_boundary_loss_bwd(const UssegLossDesc* d, const UssegOverlapLoss* ol, const float* probs, const float* y_true, const float* phi,
                                    const UssegBoundaryLoss* bl, const float* acc, int64_t acc_floats, void* dlogits, usseg_stream_t stream);
/* ---- a stable segmented radix sort of (key, value) pairs (csrc/lovasz.hip) --------------------------------------------------------------
 * usseg_sort_pairs_u32: S segments of n (key, value) uint32 pairs, segment s at [s*n, (s+1)*n) of every array.  The order is ascending on the
 * low key_bits bits of the key and STABLE: pairs whose low bits agree keep their input order.  Bits above key_bits are ignored for the order
 * and kept in the output.  An LSD radix sort with digits of USSEG_SORT_DIGIT_BITS = 8 bits over tiles of USSEG_SORT_TILE = 2048 pairs (256
 * threads x 8), segments in grid.y; a digit pass is tile histograms, their offsets, and a scatter that is stable inside a tile (a wave ranks
 * 64 pairs at a time with one 64-lane ballot per digit bit and keeps its running digit counts in LDS).  The number of launches is fixed by
 * (S, n, key_bits) - 3 * ceil(key_bits / 8) - and never by the data, so a captured graph holds the call.  No host synchronisation, no
 * allocation: the workspace (16-byte aligned, usseg_sort_ws_bytes(S, n) bytes; -1 for a refused shape) comes from the caller.  No workgroup
 * waits for another: a pass boundary is a launch boundary.  Only integer atomics are used, so the result is a function of the inputs alone.
 * 0 <= S <= 65535, 0 <= n <= 2^29, 1 <= key_bits <= 32; the outputs must not alias the inputs or each other; S == 0 or n == 0 returns 0
 * without a launch.  Every argument is checked before any launch (USSEG_ERR_BAD_ARG with usseg_last_error text), a workspace that is too
 * small included. */
#define USSEG_SORT_TILE 2048
#define USSEG_SORT_DIGIT_BITS 8
int64_t usseg_sort_ws_bytes(int32_t S, int64_t n);
int usseg_sort_pairs_u32(const uint32_t* keys_in, const uint32_t* vals_in, int32_t S, int64_t n, int32_t key_bits, uint32_t* keys_out,
                         uint32_t* vals_out, void* ws, int64_t ws_bytes, usseg_stream_t stream);
/* ---- the Lovasz-softmax loss (Berman, Triki, Blaschko, CVPR 2018; csrc/lovasz.hip) -------------------------------------------------------
 * Not in the reference: the surrogate of the intersection over union the drivers report.  Batch-level (the paper's per_image = False), on the
 * head's fp32 probabilities p[m][c] and the labels y[m][c] exactly as passed, m over the M pixels of THIS call, C <= 4, M <= 2^29.  Per class c:
 *     fg(m) = y_c(m) > threshold          (a NaN is not foreground: usseg_sdf_labels' rule)
 *     e(m)  = fg ? 1 - p_c(m) : p_c(m)    (one fp32 operation)
 *     key   = the uint32 bit pattern of |e|, clamped to 0x3F800000: every input, NaN or out of range, has a defined place
 *     order = key descending, ties by ascending pixel index m - a strict order, so the result is a function of the inputs alone
 * With r(m) the 0-based rank, F(m) the number of foreground pixels of rank <= r(m), Y = sum fg, I = Y - F, U = Y + r + 1 - F, the Lovasz
 * gradient of the Jaccard loss is built from the exact integers in closed form (never as a difference of two Jaccard values):
 *     g(m) = 1 / U  at a foreground pixel,   I / (U * (U - 1))  at a background pixel (the product in int64);
 *     Y = 0:  g = 1 at rank 0 and 0 elsewhere.
 *     L_c = sum_m e(m) * g(m)                 L_lv = (1/|S|) * sum_{c in S} w[c] * L_c
 *     loss = ce_weight * CCE + lv_weight * ov_scale * L_lv
 * S is the set of classes with Y_c > 0 (all_classes = 0: "present", the paper's default) or every class (all_classes = 1); |S| is counted on
 * the device; an empty S gives L_lv = 0 and a zero gradient.  CCE is loss_kind 0 exactly as the overlap losses carry it, ov_scale their
 * data-parallel factor.
 *     G_c(m) = k_c * (fg ? -1 : +1) * g_c(m) (+ the CCE term),   k_c = lv_weight * ov_scale * w[c] / |S| in S, 0 outside;
 *     dlogit_j = p_j*(G_j - sum_c p_c*G_c), fp32, ONE bf16 rounding.
 * Three calls behind a probabilities-only forward:
 *   usseg_lovasz_coeffs      writes g fp32 [M][C] (the layout of probs) and counts int32 [C] = Y_c: keys and payloads, usseg_sort_pairs_u32's
 *                            passes with S = C, n = M on the key 0x3F800000 - clamped bits (30 key bits; ascending and stable on it is
 *                            "descending, ties by index"), a scan of fg along the sorted order, the scatter back to pixel order.  16 launches.
 *                            ws: 16-byte aligned, usseg_lovasz_ws_bytes(M, C) bytes (-1 for a refused shape).
 *   usseg_lovasz_loss_sums   acc[0] = the scalar loss (OVERWRITTEN); acc[2] = the CCE pixel sum; acc[4+c] = k_c; acc[16+c] = L_c.  The ordered,
 *                            ticketed grid reduction of usseg_overlap_loss_sums under the same grid rule usseg_overlap_loss_grid(M) and the
 *                            same accumulator geometry ([1] the ticket, zero between calls; [32 + 16*b + k] workgroup b's partial): the
 *                            totals are bitwise reproducible and the same depth bound applies.  USSEG_OVERLAP_ACC_FLOATS holds every grid.
 *   usseg_lovasz_loss_bwd    reads probs, y_true, g and acc[4..8); writes dlogits bf16 [M][8] (lddl 8) or the quad layout (lddl 16) of
 *                            UssegLossDesc; pad channels are exactly zero.
 * M = 0 gives loss 0, counts 0 and no further launch.  With lv_weight = 0 and ce_weight = 1 the loss and dlogits equal the loss_kind 0
 * launch as the overlap pair does in that limit.  w[c], lv_weight, ce_weight finite and >= 0 (only w[0..C) is read); threshold finite;
 * probs, y_true and g 16-byte aligned.  Of the descriptor the fields the overlap entry points read.  The struct travels BY VALUE, into the
 * calls and with the launches, so a captured graph holds its numbers.  Nothing allocates and nothing synchronises with the host.  Every
 * argument is checked before any launch (USSEG_ERR_BAD_ARG with usseg_last_error text), a workspace or accumulator that is too small included. */
typedef struct UssegLovaszLoss {
  float w[8];          /* per-class weight */
  float lv_weight;     /* weight of the Lovasz term */
  float ce_weight;     /* weight of the CCE term; 0: not evaluated */
  float threshold;     /* foreground is y > threshold */
  int32_t all_classes; /* 0: average over the classes present in this call; 1: over all classes */
} UssegLovaszLoss;
int64_t usseg_lovasz_ws_bytes(int64_t M, int32_t C);
int usseg_lovasz_coeffs(const UssegLossDesc* d, UssegLovaszLoss ll, const float* probs, const float* y_true, float* g, int32_t* counts, void* ws,
                        int64_t ws_bytes, usseg_stream_t stream);
int usseg_lovasz_loss_sums(const UssegLossDesc* d, UssegLovaszLoss ll, float ov_scale, const float* probs, const float* y_true, const float* g,
                           const int32_t* counts, float* acc, int64_t acc_floats, usseg_stream_t stream);
int usseg_lovasz_loss_bwd(const UssegLossDesc* d, UssegLovaszLoss ll, const float* probs, const float* y_true, const float* g, const float* acc,
                          int64_t acc_floats, void* dlogits, usseg_stream_t stream);
/* ---- an exact grid-wide selection, and the top-k (hard-pixel) cross-entropy on it (csrc/topk_loss.hip) ----------------------------------
 * usseg_topk_select: S segments of n uint32 keys, segment s at [s*n, (s+1)*n).  With k the count below, per segment
 *     t = the k-th largest key,   ngt = |{key > t}|,   neq = |{key == t}|       sel int32 [S][4] = {t, ngt, neq, k} (t: the key's bits)
 * as exact integers.  The count: k = max(1, min(n, floor((double)f * n))) with f the fp32 fraction widened to double (the product is exact),
 * f read from DEVICE memory when the kernels run - or, with fraction == NULL, the explicit k (1 <= k <= n).  Give one of the two (k = 0 with
 * a fraction).  On the device the clamp is the whole rule: a fraction that does not compare (NaN) gives k = 1.  An MSD radix select with 8-bit
 * digits over a table int32 [S][4][256] in the workspace (16-byte aligned, usseg_topk_select_ws_bytes(S) bytes; -1 for a refused S): the table
 * is zeroed inside the call (a memset node under capture), one launch per digit adds the histogram of the keys that carry the prefix chosen
 * so far - every workgroup re-derives that prefix and the remaining rank from the tables of the digits before (a 256-entry scan in LDS) -
 * and a fifth launch writes sel.  Five kernels and one memset, fixed by (S, n) and never by the data, so a captured graph holds the call and
 * follows the fraction.  No host synchronisation, no allocation.  No workgroup waits for another: a digit boundary is a launch boundary.
 * Only integer atomics are used, so the result is a function of the inputs alone.  0 <= S <= 2^29, 1 <= n <= 2^29; S == 0 returns 0 without
 * a launch.  Every argument is checked before any launch (USSEG_ERR_BAD_ARG with usseg_last_error text), a workspace that is too small included.
 *
 * The top-k cross-entropy (nnU-Net's TopKLoss; online hard example mining), not in the reference: the mean of the k largest per-pixel losses.
 * On the head's fp32 probabilities and the labels, probs / y_true fp32 [M][C], C <= 4, 16-byte aligned, M <= 2^29:
 *     l(m)  = the CategoricalCrossentropy of pixel m, loss_kind 0's arithmetic exactly (divide by the class sum, clip, log, label smoothing),
 *             stored as fp32;   key(m) = the uint32 bits of l(m) with the sign bit cleared (l >= 0, so bit order is value order; a NaN sorts
 *             above every finite value, is therefore selected, and makes the loss NaN as CCE's would)
 *     scope = 0 ("batch"): one segment of n = M pixels;   scope = 1 ("image"): M/HW segments of n = HW
 *     t_s, ngt_s, neq_s, k as above per segment s,   r_s = k - ngt_s  (1 <= r_s <= neq_s)
 *     a(m)  = 1 if key > t_s,   r_s / neq_s (one fp32 division) if key == t_s,   0 otherwise
 * Ties are shared, not broken by index: the loss is the mean of exactly k values (what torch.topk(...).mean() returns), the gradient is the
 * average of all valid subgradients, nothing depends on pixel order.
 *     L_tk   = tk_weight * inv_global_batch * (n/k) * sum_m a(m) * l(m)
 *     G_c(m) = (tk_weight * inv_global_batch * (n/k) * a(m)) * dLdp_c(m),   dLdp the gradient of l (zero where the quotient was clipped);
 *     dlogit_j = p_j*(G_j - sum_c p_c*G_c), fp32, ONE bf16 rounding.  A pixel with a(m) = 0 stores exact zeros in all its slots.
 * With fraction 1 every pixel is selected and L_tk is loss_kind 0's loss.  Data-parallel reading: with scope 0 a replica selects among ITS
 * pixels (the replica reading of the overlap term), with scope 1 the selection is per image and independent of how the batch is split;
 * inv_global_batch gives the SUM all-reduce the right weight.
 * Dice + top-k (nnU-Net's DC_and_topk_loss): usseg_overlap_loss_sums runs unchanged with ce_weight = 0 into an accumulator of its own, which
 * the two calls below take as overlap_acc (NULL: plain top-k): the sums pass adds its [0] to the scalar, the backward pass adds
 * A_c*y_c(m) + B_c from its [4..12) to G_c(m) before the one rounding.
 * Three calls behind a probabilities-only forward, the workspace (16-byte aligned, usseg_topk_ws_bytes(M, HW, scope) bytes; -1 for a refused
 * shape) carrying l fp32 [M] at offset 0, the select table at the next multiple of 256 bytes, sel behind it (again on a multiple of 256):
 *   usseg_topk_pixel_loss   l, the top digit's histogram in the same launch, the three further digits, sel: five kernels and one memset.
 *   usseg_topk_loss_sums    reads l and sel: acc[0] = L_tk (+ overlap_acc[0]) (OVERWRITTEN); acc[2] = the plain CCE pixel sum sum_m l(m);
 *                           acc[4] = the coefficient tk_weight * inv_global_batch * n / k; acc[5] = sum_m a(m)*l(m).  The ordered, ticketed
 *                           grid reduction of usseg_overlap_loss_sums under the same grid rule usseg_overlap_loss_grid(M) and accumulator
 *                           geometry ([1] the ticket, zero between calls): bitwise reproducible.  USSEG_OVERLAP_ACC_FLOATS holds every grid.
 *   usseg_topk_loss_bwd     reads probs, y_true, l, sel, acc[4] (and overlap_acc[4..12)); writes dlogits bf16 [M][8] (lddl 8) or the quad
 *                           layout (lddl 16) of UssegLossDesc; pad channels are exactly zero.
 * Seven kernels and one memset for a training step, whatever the data.  M = 0 gives loss 0: the sums pass alone runs (as the other region
 * losses' does) and nothing else launches.  tk_weight finite and >= 0; of the descriptor the fields the overlap entry points read.  The
 * struct travels BY VALUE; the fraction is a device pointer, so a captured graph follows it without a recapture.  Every argument is checked
 * before any launch (USSEG_ERR_BAD_ARG with usseg_last_error text), a workspace one byte short and M > 2^29 included. */
typedef struct UssegTopkLoss {
  float tk_weight; /* weight of the top-k term */
  int32_t scope;   /* 0: one selection over the call's pixels ("batch"); 1: one per image ("image") */
} UssegTopkLoss;
int64_t usseg_topk_select_ws_bytes(int64_t S);
int usseg_topk_select(const uint32_t* keys, int32_t S, int64_t n, const float* fraction, int32_t k, int32_t* sel, void* ws, int64_t ws_bytes,
                      usseg_stream_t stream);
int64_t usseg_topk_ws_bytes(int64_t M, int32_t HW, int32_t scope);
int usseg_topk_pixel_loss(const UssegLossDesc* d, UssegTopkLoss tk, const float* fraction, const float* probs, const float* y_true, void* ws,
                          int64_t ws_bytes, usseg_stream_t stream);
int usseg_topk_loss_sums(const UssegLossDesc* d, UssegTopkLoss tk, const void* ws, int64_t ws_bytes, const float* overlap_acc, float* acc,
                         int64_t acc_floats, usseg_stream_t stream);
int usseg_topk_loss_bwd(const UssegLossDesc* d, UssegTopkLoss tk, const float* probs, const float* y_true, const void* ws, int64_t ws_bytes,
                        const float* acc, int64_t acc_floats, const float* overlap_acc, void* dlogits, usseg_stream_t stream);
/* The <= 4-class head Conv2DTranspose(k x k, stride 2, 'same') (Decoder.py:120 k=3; TBI_ResNest.py:124 k=4) in "quad" form: a
 * stride-1 convolution at the INPUT resolution whose 16 output channels are (output parity class)*4 + n, run by
 * usseg_conv2d_fwd/dgrad/wgrad as a 3x3 conv (each parity uses <= 2x2 of the stencil taps, the rest are zero).  With
 * pad = (k==4): kernel tap kh feeds output parity a = (kh+pad)&1 from source offset di = (a+pad-kh)/2.  These helpers move
 * the bias and the gradients between the Keras variables and that form: bias16[cls*4+n] = bias[n];
 * dbias[n] += sum_cls d16[cls*4+n] (head, Np = 4);  grad[kh][kw][n][c] += dq[(di+1)*3+(dj+1)][c][(a*2+b)*Np+n], dq = [9][Cin_phys][4*Np]. */
int usseg_quad_bias_expand(const float* bias, int32_t C, int32_t Np, float* out /* [4*Np] */, usseg_stream_t stream);
/* d16 is [4][4] - the head's own Np = 4, whatever Np the other helpers are given: dbias[n] += d16[n] + d16[4+n] + d16[8+n] + d16[12+n], n < C <= 4.
 * (usseg_quad_head_fold strides its d16 by the Np it is passed; the two agree bit for bit at Np = 4.) */
int usseg_quad_bias_fold(const float* d16 /* [4][4] */, int32_t C, float* dbias, usseg_stream_t stream);
int usseg_tconv_quad_unpack(const float* dq, int32_t Cin_phys, int32_t Cin, int32_t Cout, int32_t Np, int32_t ksize, float* grad,
                            usseg_stream_t stream);
/* usseg_tconv_quad_unpack + usseg_quad_bias_fold (with d16 = [4][Np] column sums) as ONE launch: the tail of the quad-form head's backward. */
int usseg_quad_head_fold(const float* dq, int32_t Cin_phys, int32_t Cin, int32_t Cout, int32_t Np, int32_t ksize, float* grad, const float* d16,
                         float* dbias, usseg_stream_t stream);
/* General quad-form transposed conv (any channel count; Np = physical output channels per parity class, the 16 of the head = 4*4):
 * y4 / dy4 are [B,H,W,4*Np] space-to-depth tensors of the [B,2H,2W,Np] output (usseg_space_to_depth2 converts either way);
 * the descriptor is that of the 3x3 stride-1 conv (ksize 3, Cout = 4*Np).  Each parity class only uses <= 2x2 of the nine stencil
 * taps: the conv kernels skip the others per channel class (tap masks), so no multiply is wasted on the structural zeros.
 * Replaces tf.keras.layers.Conv2DTranspose(k=4, strides 2) of TBI_ResNest.py:124,210 (and k=3 of Decoder.py:120). */
int usseg_space_to_depth2(const void* full, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ld_full, void* quad, int32_t Np,
                          int32_t ld_quad, int32_t to_quad, usseg_stream_t stream);
int usseg_tconv_quad_fwd(const UssegConvDesc* d, int32_t ksize, int32_t Np, const void* x, const void* wq_f, const float* bias_q, void* y4,
                         usseg_stream_t stream);
int usseg_tconv_quad_dgrad(const UssegConvDesc* d, int32_t ksize, int32_t Np, const void* dy4, const void* wq_d, void* dx, usseg_stream_t stream);
int usseg_tconv_quad_wgrad(const UssegConvDesc* d, int32_t ksize, int32_t Np, const void* x, const void* dy4, float* dq, float* ws,
                           int64_t ws_floats, usseg_stream_t stream);

/* my_loss_cat scale[hw][c] = 1/(sum_b y[b,hw,c] + 1)/(H*W)  (TBI_ResNest.py:240-241) */
int usseg_loss_cat_scale(const float* y_true, int32_t B, int32_t HW, int32_t C, float* scale, usseg_stream_t stream);

/* ---- host input pipeline on the device -----------------------------------------------------
 * label2vec (Dataset_2.py:6-20): label [M] fp32 -> soft class maps [M][num_classes] (3: c2 = clip(l-1,0,1) where l >= 1.05,
 * c1 = (l > 0.95) ? 1-c2 : 0, c0 = l <= 0.95; 2: (1-l, l)). */
int usseg_label2vec(const float* label, int64_t M, int32_t num_classes, float* out, usseg_stream_t stream);
/* dataAug (DataAugs.py:82-102) AS EXECUTED for a batch, one fused pass: imageReduc (zeroes the image where the label is 0,
 * DataAugs.py:76-78), up to 2 clip boxes (:27-38), shift (:6-24, last row/column stay zero) and noisy (:41-51, unit Gaussian
 * / 5000: from `noise` [B,H,W,C] if given, else a counter-based generator seeded per sample), then label2vec and the cast
 * to the model's input.  The draws are made on the host in the reference's order and passed per sample.
 * do_flip (TBI_TransUNet.py:840-842; 0 in DataAugs' draws) mirrors image and label left-right FIRST: every later step (reduc,
 * clip boxes, shift) works in the frame of the flipped image, and the noise field stays in output coordinates. */
typedef struct UssegAugSample {
  int32_t do_reduc, nclip;
  int32_t clip[2][4];        /* r, c, ra, ca per box */
  int32_t do_shift, shift_r, shift_c, shift_dir;
  int32_t do_noise, do_flip;
  uint64_t seed;
} UssegAugSample;
typedef struct UssegAugDesc {
  int32_t B, H, W, C;        /* x: [B,H,W,C] fp32 or fp64, y: [B,H,W] fp32 */
  int32_t Cphys;             /* channels of the bf16 output (multiple of 8, zero padded) */
  int32_t num_classes;       /* for y_vec */
} UssegAugDesc;
/* outputs (any may be NULL except one of the x outputs): x_out_bf16 [B,H,W,Cphys], x_out_f32 [B,H,W,C], y_out [B,H,W],
 * y_vec [B,H,W,num_classes] */
int usseg_augment(const UssegAugDesc* d, const UssegAugSample* samples_dev, const void* x, int32_t x_is_f64, const float* y,
                  const float* noise, void* x_out_bf16, float* x_out_f32, float* y_out, float* y_vec, usseg_stream_t stream);

/* ---- Decoder.py:140-141: the hidden state [B][N][hidden] is re-injected at every decoder scale through a RAW row-major
 * reshape to [B][gh*s][gw*s][c0_i] and concatenated behind the block output.  bufs[i] = first element of scale i's channel
 * slice (pixel stride ld[i], c0[i] channels, c0 % 8 == 0), n <= 4 scales in one launch.
 * backward == 0: scatter `hidden` into the n slices; backward == 1: hidden = sum_i slice_i (fp32 sum, one rounding). */
int usseg_reinject_hidden(void* hidden, int64_t numel, int32_t n, void* const* bufs, const int32_t* c0, const int32_t* ld,
                          int32_t backward, usseg_stream_t stream);

/* ---- windowed-attention encoder (SwinTransformer.py: PatchEmbed :341-365, WindowAttention :60-141, SwinTransformerBlock :162-261,
 * PatchMerging :264-290, GlobalAveragePooling1D :451).  Tokens are NHWC bf16 tensors [B][H][W][C] (the reference's [B, H*W, C]).
 *
 * usseg_patchify: x fp32/fp64 [B][H][W][C] -> bf16 [B][H/p][W/p][Cp], channel (ph*p + pw)*C + c (zero pad up to Cp): the
 *   space-to-depth half of Conv2D(kernel = stride = p); the other half is a 1x1 conv whose kernel is the Keras [p][p][C][E] variable
 *   read as [p*p*C][E] (same memory).
 * usseg_patch_merge: merged[b][i][j][(a + 2*bb)*C + c] = full[b][2i+a][2j+bb][c] (:280-284); backward != 0 scatters merged -> full.
 * usseg_ln_wide_*: LayerNormalization over C <= 4096 channels (C % 8 == 0) of M tokens; backward accumulates dgamma / dbeta
 *   (ws: >= 2*C floats per workgroup, ws_floats total - more is faster up to 512 workgroups).
 * usseg_window_attn_*: qkv [B][H][W][3C] (q | k | v, each [heads][C/heads]) -> out [B][H][W][C]; window side ws in {2,4,8}, cyclic
 *   shift `shift` (0 <= shift < ws) with the -100 region mask of :192-217, relative-position bias table [(2ws-1)^2][heads] (:78-99),
 *   q scaled by (C/heads)^-0.5.  Backward writes dqkv (same layout as qkv) and ACCUMULATES the table gradient;
 *   ws_rows: usseg_window_attn_bwd_ws_floats() floats.
 * usseg_token_mean_*: out[b][c] = mean over the L tokens; backward dx[b][t][c] = dy[b][c] / L. */
int usseg_patchify(const void* x, int32_t x_is_f64, int32_t B, int32_t H, int32_t W, int32_t C, int32_t patch, void* out, int32_t Cp,
                   usseg_stream_t stream);
int usseg_patch_merge(void* full, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldf, void* merged, int32_t ldm, int32_t backward,
                      usseg_stream_t stream);
int usseg_ln_wide_fwd(const void* x, int64_t M, int32_t C, int32_t ldx, const float* gamma, const float* beta, float eps, void* y,
                      int32_t ldy, usseg_stream_t stream);
int usseg_ln_wide_bwd(const void* x, const void* dy, int64_t M, int32_t C, int32_t ldx, int32_t lddy, const float* gamma, float eps,
                      void* dx, int32_t lddx, float* dgamma, float* dbeta, float* ws, int64_t ws_floats, usseg_stream_t stream);
int usseg_window_attn_fwd(const void* qkv, int32_t ldq, const float* table, int32_t B, int32_t H, int32_t W, int32_t C, int32_t heads,
                          int32_t ws, int32_t shift, void* out, int32_t ldo, usseg_stream_t stream);
int64_t usseg_window_attn_bwd_ws_floats(int32_t B, int32_t H, int32_t W, int32_t heads, int32_t ws);
int usseg_window_attn_bwd(const void* qkv, int32_t ldq, const void* dout, int32_t ldo, const float* table, int32_t B, int32_t H, int32_t W,
                          int32_t C, int32_t heads, int32_t ws, int32_t shift, void* dqkv, float* dtable, float* ws_rows,
                          usseg_stream_t stream);
int usseg_token_mean_fwd(const void* x, int32_t B, int32_t L, int32_t C, int32_t ld, float* out, usseg_stream_t stream);
int usseg_token_mean_bwd(const float* dy, int32_t B, int32_t L, int32_t C, int32_t ld, void* dx, usseg_stream_t stream);

/* ---- bias gradient: db[c] += sum_pixels dy[m][c] --------------------------------------------- */
int usseg_colsum(const void* dy, int64_t M, int32_t C, int32_t ld, float* db, float* ws, usseg_stream_t stream);

/* ---- optimiser: tf.clip_by_global_norm(1.0) + Adam (VisionTransformer.py:204,244-245; TBI_ResNest.py:28,46)
 * sumsq: out[0] = sum g^2 over n floats (OVERWRITTEN).  `out` is a USSEG_ACC_FLOATS accumulator (zeroed by the caller once; see below),
 *        so the sum - and with it the clip factor of every update - is bitwise reproducible from run to run.
 * adam:  scale = clip_norm > 0 ? clip_norm / max(sqrt(*sumsq), clip_norm) : 1;  g' = g*scale*grad_scale;
 *        Keras Adam with bias-corrected lr_t (host-computed from the device step counter is avoided: the caller
 *        passes lr_t = lr*sqrt(1-b2^t)/(1-b1^t) through a device scalar so a captured graph can be replayed). */
int usseg_sumsq(const float* g, int64_t n, float* out, usseg_stream_t stream);
/* out[0] = sum of n floats through a USSEG_ACC_FLOATS accumulator (see above): the scalar of TBI_ResNest.py's [H,W] loss map
 * (my_loss_cat, :234-248) that the mirrored step reduces (MainParallel.py:131-134) - reproducible, no framework reduction. */
int usseg_sum_f32(const float* x, int64_t n, float* out, usseg_stream_t stream);
/* the same launch also advances the optimiser's device step counter (usseg_adam_advance) in its last workgroup */
int usseg_sumsq_advance(const float* g, int64_t n, float* out, int32_t* step, float* lr_t_dev, float lr, float beta1, float beta2,
                        usseg_stream_t stream);
int usseg_adam_clip_step(float* p, const float* g, float* m, float* v, int64_t n, const float* sumsq, float clip_norm,
                         const float* lr_t_dev, float beta1, float beta2, float eps, usseg_stream_t stream);
/* device-side step counter: *step += 1; *lr_t = lr*sqrt(1-b2^step)/(1-b1^step) */
int usseg_adam_advance(int32_t* step, float* lr_t_dev, float lr, float beta1, float beta2, usseg_stream_t stream);
int usseg_fill_f32(float* p, int64_t n, float value, usseg_stream_t stream);
int usseg_scale_f32(float* p, int64_t n, const float* sumsq, float clip_norm, usseg_stream_t stream);

/* ---- learning-rate / weight-decay schedule on the device + decoupled weight decay (AdamW)
 * The table lives in DEVICE memory and is never a kernel argument, so a captured graph reads whatever the table holds when it
 * replays.  PiecewiseConstantDecay(boundary[0..n-2], lr/wd[0..n-1]), 1 <= n <= USSEG_SCHED_MAX_PIECES, boundaries strictly increasing:
 * at step x (= *step BEFORE the increment, as Keras evaluates a schedule at optimizer.iterations) the piece is #{i : x > boundary[i]}. */
#define USSEG_SCHED_MAX_PIECES 16
typedef struct UssegLrSchedule {
  int32_t n;                                   /* number of pieces */
  int32_t boundary[USSEG_SCHED_MAX_PIECES - 1];
  float lr[USSEG_SCHED_MAX_PIECES];            /* learning rate of each piece */
  float wd[USSEG_SCHED_MAX_PIECES];            /* decoupled weight decay of each piece (0 = none) */
} UssegLrSchedule;
/* x = *step; *step = t = x + 1; *lr_t = lr[piece]*sqrt(1-b2^t)/(1-b1^t) (usseg_adam_advance's expression); *wd_t = wd[piece] */
int usseg_sched_advance(int32_t* step, const UssegLrSchedule* sched_dev, float* lr_t_dev, float* wd_t_dev, float beta1, float beta2,
                        usseg_stream_t stream);
/* usseg_sumsq (same grid, same bits of out[0]) with usseg_sched_advance done by the workgroup that performs the final addition */
int usseg_sumsq_sched_advance(const float* g, int64_t n, float* out, int32_t* step, const UssegLrSchedule* sched_dev, float* lr_t_dev,
                              float* wd_t_dev, float beta1, float beta2, usseg_stream_t stream);
/* tfa AdamW: if *wd_t != 0 and (decay_mask == NULL or decay_mask[i] != 0): p[i] = p[i] - wd_t*p[i] (fp32, two roundings); then
 * usseg_adam_clip_step's arithmetic on the decayed p.  wd_t is NOT multiplied by the learning rate.  p, g, m, v 16-byte aligned,
 * decay_mask (u8 per element, nullable) 4-byte aligned, any n >= 0. */
int usseg_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, const float* sumsq, float clip_norm, const float* lr_t_dev,
                     const float* wd_t_dev, const uint8_t* decay_mask, float beta1, float beta2, float eps, usseg_stream_t stream);

/* ---- weight averaging inside the optimiser step (tfa.optimizers.MovingAverage / tfa.optimizers.SWA)
 * The descriptor lives in DEVICE memory and is never a kernel argument, so a captured graph reads whatever it holds when it replays.
 * Every thread derives the blend coefficient c from t = *step_dev AFTER the step's increment (the t of Adam's bias correction):
 *   EMA: c = 1 for t <= start (the average tracks the weights), else c = 1 - d_t, d_t = decay, or min(decay, (1+t)/(10+t)) with
 *        dynamic_decay;
 *   SWA: c = 1/(k+1) if t >= start and (t-start) % period == 0, k = (t-start)/period (the first snapshot replaces the average), else 0;
 * and avg[i] = fmaf(c, p[i] - avg[i], avg[i]).  c == 0 writes nothing (no byte of avg moves), c == 1 stores p[i] itself. */
#define USSEG_AVERAGE_OFF 0
#define USSEG_AVERAGE_EMA 1
#define USSEG_AVERAGE_SWA 2
typedef struct UssegAverage {
  int32_t mode;                                /* USSEG_AVERAGE_* */
  float decay;                                 /* EMA: 0 <= decay < 1 */
  int32_t dynamic_decay;                       /* EMA: nonzero = min(decay, (1+t)/(10+t)) */
  int32_t start;                               /* EMA: start_step; SWA: the step of the first snapshot */
  int32_t period;                              /* SWA: steps between snapshots, >= 1 */
} UssegAverage;
/* usseg_adamw_step and the average of the UPDATED p in one pass (36 bytes per parameter instead of 28): p, m and v get the bits
 * usseg_adamw_step gives them.  wd_t_dev may be NULL: no decay, the arithmetic of usseg_adam_clip_step.  p, g, m, v, avg 16-byte aligned,
 * decay_mask (u8 per element, nullable) 4-byte aligned, any n >= 0. */
int usseg_adamw_avg_step(float* p, const float* g, float* m, float* v, float* avg, int64_t n, const float* sumsq, float clip_norm,
                         const float* lr_t_dev, const float* wd_t_dev, const uint8_t* decay_mask, float beta1, float beta2, float eps,
                         const int32_t* step_dev, const UssegAverage* avg_desc_dev, usseg_stream_t stream);
/* the average alone, for a p updated elsewhere: the same bits of avg as the fused launch.  avg, p 16-byte aligned, any n >= 0. */
int usseg_average_update(float* avg, const float* p, int64_t n, const int32_t* step_dev, const UssegAverage* avg_desc_dev,
                         usseg_stream_t stream);
/* exchanges two disjoint buffers in place (the averaged weights go where every kernel reads its weights, and back).  a, b 16-byte
 * aligned, any n >= 0. */
int usseg_swap_f32(float* a, float* b, int64_t n, usseg_stream_t stream);

/* ---- ViT bottleneck helpers (VisionTransformer.py:9-79,127-174) ------------------------
 * Batched GEMMs on the conv kernels (bf16 operands, fp32 accumulate), 2-level batch (image, head) with element strides:
 *   nt: Y[b1,b2][m][n]  = sum_k X[b1,b2][m][k] * W[b1,b2][n][k]   (M rows, K contiguous in both operands)
 *   tn: O[b1,b2][m][n] += sum_r A[b1,b2][r][m] * B[b1,b2][r][n]   (K = number of rows r; fp32 atomics, zero O first)
 * For tn, ldx and ldw are the row strides of A and B, and xs1, xs2, ws1, ws2 their batch strides. */
typedef struct UssegGemmDesc {
  int32_t M, N, K;
  int32_t ldx, ldw, ldy;
  int32_t nb1, nb2;
  int64_t xs1, xs2, ws1, ws2, ys1, ys2;
  int32_t flags;   /* USSEG_OUT_F32 (nt only) */
} UssegGemmDesc;
int usseg_gemm_nt_batched(const UssegGemmDesc* d, const void* x, const void* w, void* y, usseg_stream_t stream);
int usseg_gemm_tn_batched(const UssegGemmDesc* d, const void* a, const void* b, float* out, usseg_stream_t stream);
/* Row softmax of scale*S (fp32 [rows][ld]) -> P fp32 (the attention weights the reference returns, :44) and P bf16;
 * backward: dS = scale * P * (dP - sum_k dP*P)  (bf16 out). */
int usseg_softmax_rows_fwd(const float* s, int64_t rows, int32_t n, float scale, float* p32, void* pbf, usseg_stream_t stream);
int usseg_softmax_rows_bwd(const float* p32, const float* dp, int64_t rows, int32_t n, float scale, void* ds_bf, usseg_stream_t stream);
/* dst[b][c][r] = src[b][r][c]: bf16, src row stride lds, batch strides ss1/ss2 (2-level), dst dense [nb1*nb2][C][R]. */
int usseg_transpose_batched(const void* src, int32_t R, int32_t C, int32_t lds, int32_t nb1, int32_t nb2, int64_t ss1, int64_t ss2,
                            void* dst, usseg_stream_t stream);
/* dst_bf16[b1,b2][r][c] = src_f32[(b1*nb2+b2)][r][c] with dst row stride ldd and batch strides ds1/ds2 */
int usseg_cast_f32_to_bf16_batched(const float* src, int32_t R, int32_t C, int32_t nb1, int32_t nb2, void* dst, int32_t ldd, int64_t ds1,
                                   int64_t ds2, usseg_stream_t stream);

/* ---- fused multi-head attention (VisionTransformer.py:38-50, TBI_TransUNet.py:44-62; head size 128) -------------------------
 * O = softmax(scale * Q K^T) V per (image, head) without the [B, heads, N, N] score tensors in memory.  q / k / v point at head 0
 * of image 0 inside the fused projection output (bf16, row stride ld_qkv elements, image stride N*ld_qkv, head h at columns
 * h*128); o / d_o are [B][N][ld_o] bf16 with the same head columns.  lse (fp32 [B*H][N], base-2 log-sum-exp of the scaled scores)
 * is written by the forward and read by the backward; delta (fp32 [B*H][N]) is backward workspace.  o32 (optional, may be NULL)
 * is an fp32 copy of O, dense [B][N][H*128]: with it the backward's delta = sum_d dO*O is free of O's bf16 rounding, which keeps
 * the rows of dS summing to zero to rounding noise (the key bias gradient, exactly zero in the reference, stays at noise level).  dq / dk / dv are written
 * (not accumulated) with row stride ld_qkv - normally the three slices of one [B][N][3*hidden] gradient tensor.  The backward
 * recomputes the probabilities (two kernels: by query tile and by key tile), uses no atomics and is bitwise reproducible.
 * The attention weights the reference also returns (:44,56) are not produced: callers that want them use the unfused
 * usseg_gemm_nt_batched + usseg_softmax_rows_fwd path. */
typedef struct UssegFlashDesc {
  int32_t B, N, H, head_dim; /* images, tokens, heads, head size (128) */
  int32_t ld_qkv, ld_o;      /* row strides in elements */
  float scale;               /* 1/sqrt(num_heads) in the reference (VisionTransformer.py:42) */
} UssegFlashDesc;
int usseg_flash_attn_fwd(const UssegFlashDesc* d, const void* q, const void* k, const void* v, void* o, float* o32, float* lse,
                         usseg_stream_t stream);
int usseg_flash_attn_bwd(const UssegFlashDesc* d, const void* q, const void* k, const void* v, const void* o, const float* o32,
                         const void* d_o, const float* lse, float* delta, void* dq, void* dk, void* dv, usseg_stream_t stream);

/* ---- opt-in per-launch timing (bench.py roofline leg) ------------------------------------------
 * When enabled, every launch of the selected kernel family is bracketed by hipEventRecord on ITS stream.
 * kinds (bits): 1 = conv / tconv forward + backward-data launches, 2 = weight-gradient launches, 4 = fused tile kernels (usseg_cardinal_fwd /
 * _bwd, usseg_stem_fwd: convs AND their norms in one launch).  Events are created by
 * usseg_prof_enable (never inside a launch function); usseg_prof_read synchronises the recorded events and
 * returns the summed duration and the launch count.  Not graph-capture safe: disable before capturing. */
int usseg_prof_enable(int32_t kind_mask, int32_t capacity);
int usseg_prof_read(int32_t kind, double* total_ms, int64_t* launches);
int usseg_prof_disable(void);

/* ---- offline preprocessing of one raw scan (prep.hip; DataFilePlayGround.output2DImages mode 1, DataFilePlayGround.py:286-393) ----------
 * Every cardiac cycle of one .mat file in one chain of launches, fp64 like the reference; the cv2 resize / GaussianBlur rules the kernels
 * restate are in DESIGN.md section 4h.  Output size USSEG_PREP_H x USSEG_PREP_W (cv2.resize(.., (80, 256))).  Every value is written by
 * one lane with a fixed operation order: bitwise reproducible.  All buffers are dense and row-major.
 * frames: fp64 [C][10][H0][W0], plane c*10+k = displacement[:, :, start_c + k] (k < 5: the "real" frames, else "imag"; :312-318).
 * usseg_prep_cycle_stats -> stats fp64 [C*10][2]: the plane's mean (numpy's x.mean(axis=0).mean(axis=0): an ordered column sum / H0,
 *   then an ordered sum of the column means / W0) and safe_max = max|x - mean| with 0 -> 1 (:368-376).  col_ws: fp64 [C*10][3][W0]. */
#define USSEG_PREP_H 256
#define USSEG_PREP_W 80
int usseg_prep_cycle_stats(const double* frames, int32_t C, int32_t H0, int32_t W0, double* col_ws, double* stats, usseg_stream_t stream);
/* The label and the gate at USSEG_PREP_H x USSEG_PREP_W (:330-343).  brain: fp64 [Hb][Wb]; gate[p] = 1 where the resized brain mask is
 * exactly 0.  objective 0: label = gate ? 0 : 1 (blood, normal, ws unused, may be NULL).  objective 1: blood, normal fp64 [Hm][Wm]; the
 * fp32 label where(blood > normal, 2, 1) (NaN compares false) goes through GaussianBlur 9x9 sigma 4, the re-set to 2 where blood > normal,
 * GaussianBlur 3x3 sigma 2, the re-set, a fp32 resize and label = gate ? 0 : that.  ws: fp32 [2][Hm*Wm] (objective 1 only). */
int usseg_prep_label(const double* brain, int32_t Hb, int32_t Wb, const double* blood, const double* normal, int32_t Hm, int32_t Wm,
                     int32_t objective, float* ws, float* label, uint8_t* gate, usseg_stream_t stream);
/* The thick-mask label of PizzaPlayGround.py (:92-97) and DataPreprocessing.py (:134-146): label fp32 and gate uint8 at
 * USSEG_PREP_H x USSEG_PREP_W from brain fp64 [Hb][Wb] and blood (bloodMaskThick) fp64 [Hm][Wm], no blur and no normal mask.  gate[p] = 1
 * where the fp64-resized brain mask is exactly 0, as usseg_prep_label; label = gate ? 0 : v with
 *   order 0 (PizzaPlayGround): each tap float(blood + 1.0), then the resize in float32 arithmetic (cv2's float32 path);
 *   order 1 (DataPreprocessing, objective 1): the resize of blood with the weights applied in double, then v = float(that + 1.0).
 * NaN in blood propagates through the taps it reaches (a NaN tap of weight 0 included).  One lane per output pixel, no workspace, one
 * launch.  Errors: a null pointer, Hb, Wb, Hm or Wm < 1, order other than 0 or 1. */
int usseg_prep_label_thick(const double* brain, int32_t Hb, int32_t Wb, const double* blood, int32_t Hm, int32_t Wm, int32_t order,
                           float* label, uint8_t* gate, usseg_stream_t stream);
/* out fp64 [C][USSEG_PREP_H][USSEG_PREP_W][12], the reference's image per cycle (:393): 0 the label; 1..10 plane c*10+k resized, each
 * bilinear tap normalised with stats before the blend and 0 where gate is set for objective 1 (:384-388); 11 the resized map
 * mean_f log10(bmode[c][.][.][f]), never gated (:327, :351, :381).  bmode: fp64 [C][Hq][Wq][F], cycle c = bModeNorm[:, :, :, c]. */
int usseg_prep_assemble(const double* frames, const double* stats, int32_t C, int32_t H0, int32_t W0, const double* bmode, int32_t Hq,
                        int32_t Wq, int32_t F, const float* label, const uint8_t* gate, int32_t objective, double* out, usseg_stream_t stream);

/* ---- DataFilePlayGround.dataAug on the device (prep_aug.hip; DataFilePlayGround.py:177-246 of the reference, as executed) ---------------
 * Records are dense fp64 [N][H][W][C], H, W >= 4, C >= 3: channel 0 the label, 1..C-2 the displacement frames, C-1 the B-mode image.
 * DESIGN.md section 4h defines every step.  All arithmetic fp64 without fused multiply-adds, the order statistics exact: bitwise
 * reproducible.
 *
 * usseg_select_ranks_f64: x fp64 [N][n] -> out fp64 [N][R], out[s][i] = the value of rank ranks[i] (0 = the smallest) of segment s, by a
 *   radix select on the order-preserving 64-bit key of a double with -0.0 folded onto +0.0 (a zero is returned as +0.0; NaNs sort by
 *   their bits, positive ones last).  ranks is a HOST array of R <= 4 values in [0, n), the same for every segment.  active (device int32
 *   [N], nullable): a segment whose entry is 0 is skipped and its out row left untouched.  One workgroup per (segment, rank), LDS integer
 *   histograms, no grid-wide wait.  Errors: a null pointer, N outside [1, 65535], n outside [1, 2^31), R outside [1, 4], a rank outside
 *   [0, n). */
int usseg_select_ranks_f64(const double* x, int32_t N, int64_t n, const int32_t* ranks, int32_t R, const int32_t* active, double* out,
                           usseg_stream_t stream);
#define USSEG_PREP_AUG_PARTIALS 64
typedef struct UssegPrepAugSample {
  int32_t do_flip, do_reduc, do_contrast, do_clip;
  int32_t clip[4];                               /* r, c, ra, ca */
  int32_t do_rotate, rot_slot;                   /* rot_slot: this sample's place in rot_list / the coefficient buffer */
  int32_t do_shift, shift_r, shift_c, shift_dir;
  int32_t do_noise, reserved;
  uint64_t seed;                                 /* of the generated noise */
  double rot[6];                                 /* R00, R01, R10, R11, offset0, offset1: source (y, x) = R (i, j) + offset */
} UssegPrepAugSample;
typedef struct UssegPrepAugDesc {
  int32_t N, H, W, C;
  int32_t n_rot;                                 /* entries of rot_list: the samples that rotate */
  int32_t k_lo, k_hi;                            /* floor of the 2nd / 98th percentile's position among the H*W*C values ... */
  double g_lo, g_hi;                             /* ... and its fraction (numpy's linear rule) */
  double zH, zW;                                 /* z^(H-1), z^(W-1), z = sqrt(3) - 2 */
} UssegPrepAugDesc;
/* The workspace of usseg_prep_aug in doubles, -1 on a bad argument. */
int64_t usseg_prep_aug_ws_doubles(int32_t N, int32_t H, int32_t W, int32_t C, int32_t n_rot);
/* out[n] = dataAug(x[n]) with the draws samples_dev[n] (device table), seven launches whatever N and the draws are.  x is not modified.
 * rot_list_dev: device int32, its first n_rot entries the samples with do_rotate in rising order (at least one readable entry).  noise:
 * the unit Gaussian field fp64 [N][H][W][C-1] or NULL (then a counter-based generator seeded per sample); noise_out (nullable, same shape)
 * receives the field that was used, 0 where a sample takes none.  Errors: a null pointer, geometry, H*W*C >= 2^31, n_rot outside [0, N],
 * ranks outside the record, weights outside [0, 1), non-finite zH / zW, a workspace below usseg_prep_aug_ws_doubles. */
int usseg_prep_aug(const UssegPrepAugDesc* d, const UssegPrepAugSample* samples_dev, const int32_t* rot_list_dev, const double* x,
                   const double* noise, double* ws, int64_t ws_doubles, double* out, double* noise_out, usseg_stream_t stream);

/* ---- the evaluator's cone figures (cone.hip; TBIEvaluator.Display, TBIEvaluator.py:276-355 of the reference) ---------------------------
 * pcolormesh(X, Y, C[:-1, :-1], shading='flat') scan-converted at px_per_unit pixels per axis unit, then colour-mapped; DESIGN.md
 * section 4h-2.  All arithmetic fp64 without fused multiply-adds; every result is order-independent: bitwise reproducible.
 * usseg_cone_index: X, Y fp64 [H][W] (H, W >= 2); quad q = i*(W-1) + j has the vertices (i,j), (i,j+1), (i+1,j+1), (i+1,j).  Pixel
 * (r, c) of index int32 [Hp][Wp] samples (xmin + (c+0.5)/ppu, ymin + (r+0.5)/ppu) and holds the largest q whose nonzero winding number
 * there is not 0 (half-open crossing rule), or -1.  Hp*Wp*4 bytes must fit int32.  Non-finite quads cover nothing. */
int usseg_cone_index(const double* X, const double* Y, int32_t H, int32_t W, double xmin, double ymin, double ppu, int32_t Hp, int32_t Wp,
                     int32_t* index, usseg_stream_t stream);
/* bmode fp64 [B][HW] -> range fp64 [B][2]: np.histogram(bmode[b], bins=25)[1][[2, -2]] (first + k*((last-first)/25), first/last = min/max
 * widened by 0.5 when equal); nonfinite int32 [B]: bit 0 where the image holds a NaN or an infinity, bit 1 where the 26 edges do not
 * strictly increase (np.histogram raises on both). */
int usseg_cone_range(const double* bmode, int32_t B, int32_t HW, double* range, int32_t* nonfinite, usseg_stream_t stream);
/* out uint8 [B][2*Hp+gap][2*Wp+gap][3], white background: panel 0 (top left) prob_map fp32, 1 label fp64, 2 bleed fp32 (all [B][H][W],
 * LUT 0, ranges[2p], ranges[2p+1] (a HOST array fp64 [3][2])), 3 (bottom right) bmode fp64 [B][H][W], LUT 1, bmode_range [B][2] on the
 * device (usseg_cone_range's output).  luts: uint8 [2][256][3] on the device.  The pixel of quad (i, j) shows the value at (i, j);
 * k = clamp(floor((v - vmin)/(vmax - vmin) * 256), 0, 255), 0 when vmax == vmin; a NaN or infinite value is white. */
int usseg_cone_render(const int32_t* index, int32_t Hp, int32_t Wp, int32_t gap, const float* prob_map, const double* label, const float* bleed,
                      const double* bmode, int32_t B, int32_t H, int32_t W, const double* ranges, const double* bmode_range, const uint8_t* luts,
                      uint8_t* out, usseg_stream_t stream);

/* ---- ensemble prediction, uncertainty maps and calibration counters (ensemble.hip; not in the reference) -------------------------------
 * usseg_ensemble_merge merges K member probability tensors in ONE pass: every member is read once, every output written once,
 * (K*C + C + 2 [+ C]) * 4 bytes per pixel.  Members and outputs are fp32 [B][H][W][C] (entropy, mutual_info: [B][H][W]), 1 <= C <= 4,
 * 1 <= K <= USSEG_ENSEMBLE_MAX.  members: a HOST array of K device pointers; they and flip_w travel BY VALUE in the kernel arguments, so a
 * captured graph holds them.  Member k contributes to pixel (b,h,w) its value at (b,h,W-1-w) when bit k of flip_w is set (it was
 * computed on the mirrored input).  Per pixel, members in ascending k, all fp32 without fused multiply-adds:
 *     mean_c      = (((p_0c + p_1c) + ...) + p_(K-1)c) / (float)K                 (an IEEE division)
 *     entropy     = -sum_c t(mean_c),   t(p) = p*logf(p) for p > 0, 0 for p <= 0, NaN for a NaN           (predictive entropy H)
 *     EH          = -(sum_k sum_c t(p_kc)) / (float)K
 *     mutual_info = H - EH, 0 where that is negative                               (the BALD term; a NaN stays a NaN)
 *     variance_c  = sum_k p_kc^2 / (float)K - mean_c^2, 0 where that is negative   (variance may be NULL)
 * Groups of four pixels as float4 for C = 3 when every base is 16-byte aligned, one pixel per lane otherwise and for the ragged tail.
 * usseg_ensemble_image_scores: scores fp32 [B][4] = the mean entropy, the mean mutual information, the maximum mutual information (a NaN
 * wins), and the mean entropy over the pixels whose mean_probs arg-max (first maximum; a NaN is never larger) is class C-1 - 0 when there
 * is none; counts int32 [B] = the number of those pixels.  One workgroup per image and a fixed summation order: bitwise reproducible.
 * B, H, W >= 1 and H*W < 2^31 for both.
 * usseg_calibration_bins: reliability counters of probs against y_true (both fp32 [B][H][W][C], 1 <= C <= 4) in one streaming pass.
 * cls = -1 (top label): conf = max_c p_c, a hit when the first-maximum index of p equals that of y_true.  cls = k in [0, C): conf = p_k, a
 * hit when y_true's first-maximum index is k.  A pixel whose conf is NaN or outside [0, 1] is INVALID and only counted as such.  Otherwise
 * bin = min(bins-1, (int)(conf*(float)bins)) in fp32, 1 <= bins <= USSEG_CALIB_MAX_BINS.  counts: int64 [bins*3 + 2], ADDED INTO (the
 * caller zeroes it once): per bin the pixel count, the hit count and sum rintf(conf*2^24); then sum rintf(v*2^24) over the valid pixels
 * with v = sum_c (p_c - onehot_c)^2 (the Brier sum; a v that is NaN or above C counts as C); then the invalid count.  B, H >= 0; W >= 1.
 * Integer adds only: bitwise reproducible.
 * All three: every argument is checked before any launch, nothing allocates and nothing synchronises with the host. */
#define USSEG_ENSEMBLE_MAX 16
#define USSEG_CALIB_MAX_BINS 64
typedef struct UssegEnsembleDesc {
  int32_t B, H, W, C;
  int32_t K; /* members, 1..USSEG_ENSEMBLE_MAX (image_scores ignores it) */
} UssegEnsembleDesc;
int usseg_ensemble_merge(const UssegEnsembleDesc* d, const float* const* members, uint32_t flip_w, float* mean_probs, float* entropy,
                         float* mutual_info, float* variance, usseg_stream_t stream);
int usseg_ensemble_image_scores(const UssegEnsembleDesc* d, const float* mean_probs, const float* entropy, const float* mutual_info,
                                float* scores, int32_t* counts, usseg_stream_t stream);
typedef struct UssegCalibDesc {
  int32_t B, H, W, C;
  int32_t bins; /* 1..USSEG_CALIB_MAX_BINS */
  int32_t cls;  /* -1: top label; 0..C-1: that class */
} UssegCalibDesc;
int usseg_calibration_bins(const UssegCalibDesc* d, const float* probs, const float* y_true, int64_t* counts, usseg_stream_t stream);

/* ---- threshold sweeps and temperature scaling (operating_point.hip; not in the reference) ---------------------------------------------
 * probs, y_true and out are fp32 [B][H][W][C], 1 <= C <= 4, B, H >= 0, W >= 1 and M = B*H*W <= 2^31; M = 0 returns USSEG_OK without a launch.
 * The label of a pixel is the first-maximum class of y_true (a NaN is never larger), as in usseg_calibration_bins.
 * usseg_score_sweep: per score bin the negatives and the positives of class cls (0..C-1) in one streaming pass.  The score is
 * s = probs[p][cls]; a pixel is POSITIVE when its label is cls.  A pixel whose s is NaN or outside [0, 1] is INVALID and only counted as such
 * (the test comes before any index is formed).  Otherwise bin = min(bins-1, (int)(s*(float)bins)) in fp32, clamped at 0 as well; bins is a
 * power of two, 2 <= bins <= USSEG_SWEEP_MAX_BINS, so s*bins is exact and "bin >= k" is "s >= k/bins" for k < bins (s = 1 lies in the last bin).  counts: int64 [2*bins + 1], ADDED
 * INTO (the caller zeroes it once): counts[2b] the negatives of bin b, counts[2b+1] its positives, counts[2*bins] the invalid pixels.  Each
 * workgroup counts into two histograms of 32-bit LDS counters (32 KB, sized by the constant), a wave whose lanes all hold one (bin,
 * positive) key adds its population count once, and the workgroup then issues one 64-bit atomic per non-zero counter.  Integer adds only:
 * bitwise reproducible and independent of the grid.
 * usseg_temperature_nll: the summed negative log-likelihood of n_beta candidate inverse temperatures, 1 <= n_beta <= USSEG_TEMP_MAX_BETAS,
 * every pixel read once for all of them.  betas: a HOST array, every entry finite with 0 < beta <= 16; it travels BY VALUE in the kernel
 * arguments, so a captured graph holds it.  Per pixel, all fp32 without fused multiply-adds, the accurate logf / expf, classes ascending:
 *     z_c   = logf(p_c + 1e-7f)                                              (the CCE's epsilon)
 *     m     = max_c beta_j*z_c
 *     nll_j = (m + logf(sum_c expf(beta_j*z_c - m))) - beta_j*z_y,           y the pixel's label
 * A pixel with any p_c that is NaN or outside [0, 1] is INVALID and contributes nothing.  counts: int64 [n_beta + 2], ADDED INTO:
 * counts[j] += (int64)rintf(min(max(nll_j, 0), USSEG_TEMP_NLL_CAP) * 2^20), counts[n_beta] the valid and counts[n_beta+1] the invalid
 * pixels.  No overflow: 2^10 (the cap) * 2^20 (the unit) * 2^31 (pixels per call) = 2^61 < 2^63; a caller that accumulates calls keeps
 * their pixel total below 2^33.  64-bit sums per lane, one LDS tree per workgroup, one 64-bit atomic per counter: bitwise reproducible.
 * usseg_apply_temperature: out_c = expf(beta*z_c - m) / sum_c expf(beta*z_c - m) with z and m as above and an IEEE division (n_beta is
 * ignored).  beta_dev: a DEVICE float, read by the kernel on every launch - a captured graph follows it; beta == 1 is NOT special-cased.
 * A pixel with a NaN z_c (a NaN p_c, or one below -1e-7) is NaN in all its classes.  out may alias probs.  Groups of four pixels as float4 for
 * C = 3 when both bases are 16-byte aligned, one pixel per lane otherwise and for the ragged tail.
 * All three: every argument is checked before any launch, nothing allocates and nothing synchronises with the host. */
#define USSEG_SWEEP_MAX_BINS 4096
#define USSEG_TEMP_MAX_BETAS 16
#define USSEG_TEMP_NLL_CAP 1024
typedef struct UssegSweepDesc {
  int32_t B, H, W, C;
  int32_t bins; /* a power of two, 2..USSEG_SWEEP_MAX_BINS */
  int32_t cls;  /* 0..C-1: the class whose score is swept */
} UssegSweepDesc;
int usseg_score_sweep(const UssegSweepDesc* d, const float* probs, const float* y_true, int64_t* counts, usseg_stream_t stream);
typedef struct UssegTempDesc {
  int32_t B, H, W, C;
  int32_t n_beta; /* candidates, 1..USSEG_TEMP_MAX_BETAS (apply_temperature ignores it) */
} UssegTempDesc;
int usseg_temperature_nll(const UssegTempDesc* d, const float* probs, const float* y_true, const float* betas, int64_t* counts,
                          usseg_stream_t stream);
int usseg_apply_temperature(const UssegTempDesc* d, const float* probs, const float* beta_dev, float* out, usseg_stream_t stream);

/* ---- elastic and affine warp of a training batch (not in the reference; csrc/warp.hip) --------------
 * x [B,H,W,C] fp32 or fp64 and y [B,H,W] fp32 -> x_out, y_out of the same shapes and dtypes, every output pixel (i, j) sampled at a source
 * coordinate that an affine map and a smoothed random displacement give.  Two launches whatever B, the sizes and the draws are; nothing
 * allocates or synchronises with the host; the sample table and the weights are read from the device on every launch, so a captured graph
 * follows them.  All coordinate and interpolation arithmetic is fp64 without fused multiply-adds, every sum in the stated order:
 *   field     u[b][k][i][j], k = 0 rows / 1 columns: `field` as it is if given, else h * 2^-31 - 1 with h the low 32 bits of the 64-bit
 *             finaliser of usseg_augment's noise applied to seed * 0x9e3779b97f4a7c15 + ((k*H + i)*W + j) (wrapping): uniform on [-1, 1).
 *   smoothing a separable Gaussian with zero padding, along H and then along W: s[p] = sum over k = -radius..radius ascending of
 *             w[|k|] * u[p + k], starting from +0.0, taps outside the image skipped; radius == 0 passes u through unchanged.
 *   source    src0 = ((A00*i + A01*j) + o0) + alpha[0]*s0, src1 = ((A10*i + A11*j) + o1) + alpha[1]*s1, each operation rounded.
 *   image     bilinear: i0 = floor(src0), f0 = src0 - i0 (likewise src1); out = ((w00*v00 + w01*v01) + w10*v10) + w11*v11 with
 *             w00 = (1-f0)*(1-f1), w01 = (1-f0)*f1, w10 = f0*(1-f1), w11 = f0*f1; a tap outside the image is 0 and is not read; a coordinate
 *             that is not finite or not inside (-1, H) x (-1, W) gives 0 (tested in fp64 before any integer is formed); rounded ONCE to x's dtype.
 *   label     nearest: y[floor(src0 + 0.5)][floor(src1 + 0.5)], 0 outside; never interpolated.
 *   inactive  active == 0: x_out and y_out are copies of that sample's x and y, bit for bit; its disp_out and field_out are 0.
 * disp_out (alpha[k]*s_k) and field_out (the field that was used) are optional [B][2][H][W] fp64 outputs.  x_out / y_out must not
 * overlap x / y.  Every argument is checked before any launch (USSEG_ERR_BAD_ARG with usseg_last_error text): a null pointer, B, H, W or C
 * below 1, B*H*W*C >= 2^31, a radius outside [0, USSEG_WARP_MAX_RADIUS], a workspace below usseg_warp_ws_bytes, overlapping buffers. */
#define USSEG_WARP_MAX_RADIUS 64
typedef struct UssegWarpSample {
  int32_t active, reserved;
  uint64_t seed;
  double alpha[2];   /* rows, cols */
  double aff[6];     /* A00, A01, A10, A11, o0, o1 */
} UssegWarpSample; /* one sample's draws; a device table of them is read on every launch */
typedef struct UssegWarpDesc { int32_t B, H, W, C, x_is_f64, radius; } UssegWarpDesc;

int64_t usseg_warp_ws_bytes(int32_t B, int32_t H, int32_t W);   /* 0 for a B, H or W below 1 */
int usseg_elastic_warp(const UssegWarpDesc* d, const UssegWarpSample* samples_dev,
                       const double* weights_dev /* [radius+1], w[0] the centre tap */,
                       const double* field /* nullable, [B][2][H][W] */,
                       const void* x, const float* y,
                       void* ws, int64_t ws_bytes,
                       void* x_out, float* y_out,
                       double* disp_out /* nullable, [B][2][H][W] */,
                       double* field_out /* nullable, [B][2][H][W] */,
                       usseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* USSEG_H */
