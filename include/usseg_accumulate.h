/*
 * usseg_accumulate.h - fourth header of libusseg_hip.so's C ABI: gradient accumulation (csrc/accumulate.hip).  usseg.h declares the training
 * and inference kernels, usseg_scores.h the evaluator's scores, usseg_distill.h the distillation loss; this header stands alone beside them
 * (a program may include any of the four) and the contract of usseg.h holds for the function here:
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer; the caller owns every buffer;
 *  - the library allocates no device memory, never synchronises with the host and never throws;
 *  - all work is enqueued on the hipStream_t passed in, in order: a call captures into a HIP graph as one node;
 *  - return value: 0 on success, USSEG_ERR_BAD_ARG (-1) when an argument is refused - every argument is checked BEFORE the launch - and
 *    USSEG_ERR_LAUNCH (-3) when the launch fails; usseg_last_error() (usseg.h) has the text.
 *
 * Nothing here exists in the reference (silverlight6/Ultrasound_Modeling): one optimiser step on the gradient of N micro-batches (DESIGN.md
 * section 4g-3).  acc is one more flat fp32 buffer of the gradient's shape, zero before the first micro-step of a group.  One launch, a pure
 * stream (16 bytes per lane, no atomics, no LDS):
 *     finish == 0:  acc[i] = acc[i] + grad[i]
 *     finish == 1:  t = acc[i] + grad[i];  grad[i] = t / divisor;  acc[i] = 0            divisor = (float)N >= 1
 * Each operation is one separately rounded IEEE fp32 operation - an addition, and a true division: no reciprocal multiply, nothing
 * contracted, denormals kept - so the result is a function of the micro-batch gradients and their order alone and NumPy fp32 restates it bit
 * for bit for every N.  acc is +0.0 again after a finish: no device counter is needed, and one captured micro-step serves every micro-step of
 * a group.  The clip, the data-parallel exchange and the Adam update of usseg.h then run on grad exactly as they do without accumulation.
 */
#ifndef USSEG_ACCUMULATE_H
#define USSEG_ACCUMULATE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* usseg_stream_t; /* a hipStream_t; the same typedef as usseg.h's (C11 and C++ allow the repeat) */

/* acc, grad: n floats each, 16-byte aligned, disjoint; any n >= 0 (n == 0 launches nothing).  finish: 0 or 1.  divisor is read only with
 * finish == 1.  The grid is usseg_adam_clip_step's: ceil(n / 1024) workgroups of 256 threads, at most 4096, in a grid-stride loop. */
int usseg_grad_accumulate(float* acc, float* grad, int64_t n, int32_t finish, float divisor, usseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* USSEG_ACCUMULATE_H */
