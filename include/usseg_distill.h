/*
 * usseg_distill.h - third header of libusseg_hip.so's C ABI: the knowledge-distillation loss (csrc/distill.hip).  usseg.h declares the
 * training and inference kernels, usseg_scores.h the evaluator's scores; this header stands alone beside them (a program may include any of
 * the three) and the contract of usseg.h holds for every function here:
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated; the caller owns every buffer;
 *  - the library allocates no device memory, never synchronises with the host and never throws;
 *  - all work is enqueued on the hipStream_t passed in, in order: a call captures into a HIP graph as one linear chain;
 *  - return value: 0 on success, USSEG_ERR_BAD_ARG (-1) when an argument is refused - every argument is checked BEFORE any launch - and
 *    USSEG_ERR_LAUNCH (-3) when a launch fails; usseg_last_error() (usseg.h) has the text.
 *
 * Nothing here exists in the reference (silverlight6/Ultrasound_Modeling).  The loss is Hinton et al.'s (2015): a student is trained against
 * a teacher's softened probabilities as well as the labels.
 *
 * Definition.  p: the student's probabilities, q: the teacher's (a model's, or the mean of an ensemble's members), y: the labels, all fp32
 * [M][C]; T > 0 the temperature.  ONE device function softens both sides, the arithmetic of usseg_apply_temperature:
 *     soften(r)_c  = softmax_c( log(r_c + 1e-7) / T )                       pT = soften(p), qT = soften(q)
 *     soft(pixel)  = T^2 * sum_c qT_c * (log qT_c - log pT_c)               the logs as s_c - logsumexp(s), s_c = log(r_c + 1e-7) / T
 *     hard(pixel)  = CategoricalCrossentropy(label_smoothing, clip_eps)     the arithmetic of usseg.h's loss_kind 0
 *     loss         = inv_global_batch * ( hard_weight * sum_pixels hard + soft_weight * sum_pixels soft )
 * Gradient with respect to the logits z (p = softmax(z)), for the soft term:
 *     r_c = T * (pT_c - qT_c) * p_c / (p_c + 1e-7),    dz_j = r_j - p_j * sum_c r_c
 * i.e. dz_j = p_j * (G_j - sum_c p_c * G_c) with G_c = T * (pT_c - qT_c) / (p_c + 1e-7): no division by a small number.  The hard term's G
 * is the CCE's d loss / d p; both are added in fp32 before the ONE bf16 rounding of dlogits.  Because both sides pass through the same
 * function, q == p (the same bits) gives a soft sum of exactly 0.0 and an exactly zero soft gradient.
 *
 * The settings are a DEVICE table of USSEG_DISTILL_SETTINGS floats, read when the kernel runs, so a captured graph follows a change without
 * a recapture: [0] T, [1] soft_weight, [2] hard_weight, [3] reserved (0).  The library does not check them (it never reads device memory
 * from the host): the caller keeps T finite and > 0 and the weights finite and >= 0 (distill.distill_config).
 *
 * The accumulator: USSEG_DISTILL_ACC_FLOATS floats, zeroed ONCE at allocation and never by the caller again:
 *     [0] the loss (OVERWRITTEN by every call)   [1] a ticket counter, zero between calls   [2] sum_pixels hard   [3] sum_pixels soft
 *     [4] inv_global_batch * hard_weight * [2]   [5] inv_global_batch * soft_weight * [3]   [32 + 16*b + k] the partials of workgroup b
 * The two sums are added in a fixed order (a thread its pixels in index order; lanes, waves and workgroups by the ticketed grid reduction of
 * usseg_overlap_loss_sums), so they and the loss are bitwise reproducible.  usseg_distill_grid(M) = clamp(ceil(ceil(M/4)/256), 1, 512)
 * workgroups of 256 threads; a thread owns groups of four consecutive pixels.
 *
 * ONE launch per call: the gradient needs no grid-wide coefficient, so the same kernel that forms the sums writes dlogits.
 * Limits: 1 <= C <= 4, 0 <= M <= 2^29, M a multiple of HW.  M == 0 launches no kernel: the accumulator's header is set to zero (loss 0).
 */
#ifndef USSEG_DISTILL_H
#define USSEG_DISTILL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* usseg_stream_t; /* a hipStream_t; the same typedef as usseg.h's (C11 and C++ allow the repeat) */

#define USSEG_DISTILL_ACC_FLOATS 8224 /* 32 + 16 * 512 workgroups */
#define USSEG_DISTILL_SETTINGS 4

typedef struct UssegDistillDesc {
  int64_t M;             /* B*H*W pixels */
  int32_t HW;            /* pixels per image */
  int32_t C;             /* classes, 1..4 */
  int32_t lddl;          /* dlogits stride in bf16 elements: 8, or 16 in the quad layout */
  int32_t quad_w;        /* 0: dlogits is [M][8]; W (the full-resolution width, even, H even too): the space-to-depth layout
                            [B][H/2][W/2][16], pixel (y,x) in slot 4*((y&1)*2+(x&1)), as UssegLossDesc.quad_w */
  float label_smoothing; /* [0, 1) */
  float clip_eps;        /* 1e-7 */
  float inv_global_batch; /* the loss's scale: 1 / global batch, or 1 / (B*H*W) for a mean over pixels; finite, >= 0 */
} UssegDistillDesc;

/* The workgroups of the launch for M pixels (the grid rule above; part of the ABI because the accumulator's size follows from it). */
int usseg_distill_grid(int64_t M);

/* probs, y_true, q: fp32 [M][C], 16-byte aligned.  settings_dev: the device table above, 4-byte aligned.  acc: acc_floats floats, at least
 * 32 + 16 * usseg_distill_grid(M), 4-byte aligned.  dlogits: bf16, 16-byte aligned, every element written (pad channels exactly zero), or
 * null for the loss alone (lddl and quad_w are checked all the same). */
int usseg_distill_loss(const UssegDistillDesc* desc, const float* probs, const float* y_true, const float* q, const float* settings_dev,
                       float* acc, int64_t acc_floats, void* dlogits, usseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* USSEG_DISTILL_H */
