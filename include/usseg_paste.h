/*
 * usseg_paste.h - fifth header of libusseg_hip.so's C ABI: lesion copy-paste augmentation of a training batch (csrc/paste.hip).  usseg.h
 * declares the training and inference kernels, usseg_scores.h the evaluator's scores, usseg_distill.h the distillation loss,
 * usseg_accumulate.h gradient accumulation; this header stands alone beside them (a program may include any of the five) and the contract of
 * usseg.h holds for the function here:
 *  - plain pointers and sizes only; every pointer but the descriptor's is a DEVICE pointer; the caller owns every buffer;
 *  - the library allocates no device memory, never synchronises with the host and never throws;
 *  - all work is enqueued on the hipStream_t passed in, in order: the call captures into a HIP graph as a chain of two nodes;
 *  - return value: 0 on success, USSEG_ERR_BAD_ARG (-1) when an argument is refused - every argument the host can see is checked BEFORE any
 *    launch - and USSEG_ERR_LAUNCH (-3) when a launch fails; usseg_last_error() (usseg.h) has the text.
 *
 * Nothing here exists in the reference (silverlight6/Ultrasound_Modeling): copy-paste augmentation (Ghiasi et al., "Simple Copy-Paste", CVPR
 * 2021; TumorCP and CarveMix for lesions) puts a labelled lesion of one training record into another record's brain.
 * The bank IS the resident training set: x_bank [N][H][W][C] in x's element type, y_bank fp32 [N][H][W], and labels_bank int32 [N][H][W], the
 * connected components of `y_bank >= 1.05f` (usseg_label_components).  x is [B][H][W][C] fp32 or fp64, y fp32 [B][H][W].
 *
 * Definitions - integer comparisons and bit copies only, apart from the two label thresholds:
 *   mapping     item i of sample b maps a target pixel q = (r', c') to the donor pixel p = (r' - dr, c): cf = c' - dc, c = flip ? W-1-cf : cf;
 *   member_i(q) p lies inside the image AND inside the item's donor box [r0, r1] x [c0, c1] (inclusive; the bounding box of the component, from
 *               usseg_component_stats) AND labels_bank[record][p] == comp.  A box that holds the whole component leaves the test to the label;
 *   ok(q)       y[b][q] > 0.95f and, with protect, not y[b][q] >= 1.05f: the recipient's ORIGINAL label says brain (and no bleed of its own).
 *               A NaN label is never ok;
 *   landed_i    the number of q with member_i(q) && ok(q); item i is ACCEPTED iff landed_i >= max(need_i, 1);
 *   output      at each q the LAST accepted item with member && ok wins: x_out[b][q][:] = x_bank[record][p][:], y_out[b][q] = y_bank[record][p];
 *               every other pixel, and every pixel of a sample with active == 0, is a copy of x and y bit for bit (NaN payloads, -0.0);
 *   absent      an item with record outside [0, N) or comp < 1, and the items at and beyond n_items (clamped to [0, USSEG_PASTE_MAX_ITEMS]), do
 *               not exist: landed 0, never accepted, never read through.  The table lives on the device, so the host cannot check it; no
 *               value in it makes a launch read or write out of bounds.
 * landed_out int32 [B][USSEG_PASTE_MAX_ITEMS] is overwritten (0 for absent items and inactive samples).  counts int64 [2] is ADDED into with
 * integer atomics: [0] items accepted, [1] pixels pasted (a pixel two items cover counts once).  The sample table is read on every launch, so a
 * captured graph follows new draws.
 *
 * Two launches whatever the draws are: pass 1, one workgroup per (sample, item), walks the item's target box and writes landed; pass 2 decides
 * every output pixel once (the recipient's label, then at most USSEG_PASTE_MAX_ITEMS bank labels, read only inside item boxes) and copies its
 * C elements 16, 8 or 4 bytes at a time, whichever C * element size and the pointers allow, in a grid-stride loop of at most 2048 workgroups.
 * No float arithmetic, no float atomics; no workgroup waits for another.
 *
 * Refused before any launch: a null pointer; B, H, W, C or N below 1; B*H*W*C >= 2^31; N*H*W*C*8 beyond 2^62; x, x_bank or x_out not aligned to
 * the element, y / y_bank / labels_bank / y_out / landed_out / samples_dev to 4 bytes, counts to 8; an output (x_out, y_out, landed_out, counts)
 * that overlaps an input, the bank, the table or another output.
 */
#ifndef USSEG_PASTE_H
#define USSEG_PASTE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* usseg_stream_t; /* a hipStream_t; the same typedef as usseg.h's (C11 and C++ allow the repeat) */

#define USSEG_PASTE_MAX_ITEMS 4

typedef struct UssegPasteItem {
  int32_t record, comp;   /* the donor: training record and component id in labels_bank (>= 1) */
  int32_t dr, dc;         /* target = donor + (dr, dc), the columns after the flip */
  int32_t flip;           /* nonzero: the donor is mirrored left-right first */
  int32_t need;           /* accepted iff landed >= max(need, 1) */
  int32_t r0, c0, r1, c1; /* the donor component's bounding box, inclusive */
} UssegPasteItem;

typedef struct UssegPasteSample {
  int32_t active;  /* 0: the sample is copied bit for bit */
  int32_t n_items; /* items[0 .. n_items) exist; clamped to [0, USSEG_PASTE_MAX_ITEMS] */
  UssegPasteItem items[USSEG_PASTE_MAX_ITEMS];
} UssegPasteSample;

typedef struct UssegPasteDesc {
  int32_t B, H, W, C;
  int32_t x_is_f64; /* x, x_bank and x_out: 1 fp64, 0 fp32 */
  int32_t N;        /* records of the bank */
  int32_t protect;  /* nonzero: a recipient pixel with a label >= 1.05f is never pasted over */
} UssegPasteDesc;

int usseg_lesion_paste(const UssegPasteDesc* d, const UssegPasteSample* samples_dev, const void* x, const float* y, const void* x_bank,
                       const float* y_bank, const int32_t* labels_bank, void* x_out, float* y_out, int32_t* landed_out, int64_t* counts,
                       usseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* USSEG_PASTE_H */
