/*
 * usseg_scores.h - second header of libusseg_hip.so's C ABI: the evaluator's per-image scores in pixels and in physical units
 * (csrc/scores.hip).  usseg.h declares everything else; this header stands alone beside it (a program may include either or both) and the
 * contract of usseg.h holds for every function here:
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer; the caller owns every buffer;
 *  - the library allocates no device memory, never synchronises with the host and never throws;
 *  - all work is enqueued on the hipStream_t passed in, in order: a call captures into a HIP graph as one linear chain;
 *  - return value: 0 on success, USSEG_ERR_BAD_ARG (-1) when an argument is refused - every argument is checked BEFORE any launch - and
 *    USSEG_ERR_LAUNCH (-3) when a launch fails; usseg_last_error() (usseg.h) has the text.
 *
 * Nothing here exists in the reference (silverlight6/Ultrasound_Modeling): its evaluator draws figures and prints pooled Keras metrics.
 * These entry points give the numbers a segmentation paper prints first - an overlap table per image, an interval from a (cluster)
 * bootstrap, and the bleed's size in the units of axis/xAxis.npy and axis/yAxis.npy - as EXACT INTEGERS: every result is an integer
 * sum, minimum or maximum, independent of the order in which the threads arrive, so a second call gives the same bits and a test can
 * compare with ==.  No float atomics: sums use vector 64-bit integer atomics (global_atomic_add_x2 and its min / max kin) after a
 * reduction inside the wave, or no atomics at all (usseg_bootstrap_sums).  The caller zeroes nothing: every output word is written.
 *
 * Shapes (the limits of usseg_component_stats): H and W each lie in [1, 8192], N in [0, 65535], N*H*W <= 2^29.  pred, truth: any
 * alignment; weight, labels, xq, yq 4-byte, every int64 table 8-byte aligned.  N == 0, R == 0 and U == 0 launch nothing and return 0.
 *
 * Fixed point and overflow.  The physical quantities are carried as integers that metrics.ScanGeometry prepares on the host:
 *     weight (wq) < 2^20    the area of the cell around a sample, in units of quantum = max area / (2^20 - 1)
 *     xq, yq in [0, 65535]  the sample's position, in units of xstep = (x_max - x_min) / 65535 (ystep alike) above the minimum
 * One image has H*W <= 8192 * 8192 = 2^26 samples, so the largest sum a call can form, sum of w * xq over one image, stays below
 * 2^20 * 2^16 * 2^26 = 2^62 < 2^63: no int64 sum can overflow.  (usseg_image_confusion takes any uint32 weight: 2^32 * 2^26 = 2^58.)
 * An area summed over n pixels is off by at most n * quantum / 2 (each cell is rounded to the nearest quantum once).
 */
#ifndef USSEG_SCORES_H
#define USSEG_SCORES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* usseg_stream_t; /* a hipStream_t; the same typedef as usseg.h's (C11 and C++ allow the repeat) */

/* ---- the confusion table of every image --------------------------------------------------------------------------------------------
 * pred, truth: uint8 [N,H,W] class ids; C in [2, 4].  weight: uint32 [H,W], one table shared by all images, or null.
 *     cm      int64 [N,C,C]   cm[n][t][p] = the number of pixels of image n with truth t and prediction p (rows = truth, columns =
 *                             prediction: the orientation of usseg_seg_counts' matrix, which metrics.SegMetrics reads)
 *     wcm     int64 [N,C,C]   the same cells, each pixel counted weight[y][x] times; null exactly when weight is null (one without the
 *                             other is refused)
 *     invalid int64 [N]       the pixels where either id is >= C; they are counted in no cell of cm or wcm
 * so sum(cm[n]) + invalid[n] == H*W for every image. */
int usseg_image_confusion(const uint8_t* pred, const uint8_t* truth, const uint32_t* weight, int32_t N, int32_t H, int32_t W, int32_t C,
                          int64_t* cm, int64_t* wcm, int64_t* invalid, usseg_stream_t stream);

/* ---- the size, position and extent of every component in physical units ---------------------------------------------------------------
 * labels: the int32 [N,H,W] of usseg_label_components (0 outside, ids 1..K_n inside).  weight uint32 [H,W] (< 2^20), xq and yq int32
 * [H,W] (in [0, 65535]): the tables above, shared by all images, none null.  0 <= cap <= H*W.
 *     out int64 [N,cap,8]; row k-1 of image n describes the component with id k <= cap:
 *         pixels, sum of w, sum of w*xq, sum of w*yq, xq_min, xq_max, yq_min, yq_max
 * so area = (sum of w) * quantum and the area-weighted centroid is x_min + xstep * (sum of w*xq) / (sum of w).  Rows of ids that do not
 * exist hold 0 in the first four fields and the EMPTY MARKER in the extents: xq_min = yq_min = 65536 (USSEG_SCORES_EMPTY_MIN) and
 * xq_max = yq_max = -1.  Ids above cap are skipped, as in usseg_component_stats; cap == 0 launches nothing (out may then be null). */
#define USSEG_SCORES_MEASURE_FIELDS 8
#define USSEG_SCORES_EMPTY_MIN 65536
int usseg_component_measure(const int32_t* labels, const uint32_t* weight, const int32_t* xq, const int32_t* yq, int32_t N, int32_t H,
                            int32_t W, int32_t cap, int64_t* out, usseg_stream_t stream);

/* ---- bootstrap replicates of column sums ---------------------------------------------------------------------------------------------------
 * rows: int64 [U,K], one row of K integer columns per resampling unit (an image, or a patient for a cluster bootstrap).
 *     out int64 [R,K]   out[r] = the sum of U rows drawn with replacement
 * Draw d (0 <= d < U) of replicate r (0 <= r < R) is defined bit for bit, in arithmetic modulo 2^64 (splitmix64's finaliser on a counter):
 *     z = seed + 0x9E3779B97F4A7C15 * (1 + r*U + d)
 *     z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 *     index = ((z >> 32) * U) >> 32
 * so a replicate depends on (seed, r, U) alone, not on R or on the launch.  The multiply-shift maps 2^32 equally likely values onto U
 * indices: one index is at most U / 2^32 more likely than another (2^-12 at the largest U), far below the bootstrap's own Monte-Carlo error.
 * Limits: 1 <= K <= 16; R <= 2^20; 1 <= U <= 2^20 whenever R > 0 (U == 0 with R == 0 is an empty call).  The sums are formed in
 * int64 without a check: the caller keeps |v| <= 2^62 / U (ops.bootstrap_sums refuses anything larger).  No atomics: one wave per
 * replicate, reduced in registers. */
#define USSEG_SCORES_BOOT_MAX_K 16
#define USSEG_SCORES_BOOT_MAX 1048576
int usseg_bootstrap_sums(const int64_t* rows, int32_t U, int32_t K, uint64_t seed, int32_t R, int64_t* out, usseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* USSEG_SCORES_H */
