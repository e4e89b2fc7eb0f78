// Lesion copy-paste augmentation of a training batch (include/usseg_paste.h; not in the reference): a labelled lesion of
// one resident training record is put into another record's brain, ahead of usseg_elastic_warp and usseg_augment.  Two launches:
//   paste_count_kernel   one workgroup per (sample, item): the item's target box, clipped to the image, is walked once; landed = the pixels with
//                        member && ok.  An absent item, an inactive sample and an empty box write 0;
//   paste_gather_kernel  one decision per output pixel (one lane per pixel: the recipient's label, then the items from the last to the first,
//                        a bank label only inside an item's box), then the copy of the pixel's C elements with one lane per 16 / 8 / 4 bytes:
//                        loads and stores are contiguous over the neighbouring lanes of a pixel, and of the run of pixels where nothing is pasted.
// The definitions are the header's.  Integer comparisons and bit copies, apart from the two label thresholds; integer atomics only; no
// allocation, no synchronisation, the sample table read from the device: graph-capture safe.  No value of the device table can make a launch
// read or write out of bounds: every index is formed from numbers tested against B, H, W, N first, in 64-bit arithmetic.
//
// Bytes at B=16 x 256x80x10 fp64: x is read or replaced by bank pixels (26 MB) and written (26 MB) once, y 1.3 MB each way, and a label of the
// bank per pixel and item inside the item boxes, twice (once per pass).
#include "common.h"
#include "../../include/usseg_paste.h"

namespace {
constexpr int kThreads = 256;
constexpr int kGridCap = 2048;                                     // memory-bound: at most 8 workgroups per CU, the rest by grid stride
static_assert(sizeof(UssegPasteItem) == 40 && sizeof(UssegPasteSample) == 8 + 40 * USSEG_PASTE_MAX_ITEMS, "paste: the table's layout");

struct PasteBox {                                                  // an item that exists, its boxes clipped to the image
  int64_t base;                                                    // record * H * W
  int r0, c0, r1, c1;                                              // donor box, inclusive, inside the image (empty if r0 > r1 or c0 > c1)
};

__device__ __forceinline__ bool recipient_ok(float yv, int protect) {
  return yv > 0.95f && !(protect && yv >= 1.05f);                  // a NaN compares false: never ok
}

// Whether item `it` exists, and its donor box clipped to the image.  SAFETY: record in [0, N) before base is formed.
__device__ __forceinline__ bool paste_item_box(const UssegPasteDesc& d, const UssegPasteItem& it, PasteBox& bx) {
  if (it.record < 0 || it.record >= d.N || it.comp < 1) return false;
  bx.base = (int64_t)it.record * d.H * d.W;
  bx.r0 = it.r0 > 0 ? it.r0 : 0;
  bx.c0 = it.c0 > 0 ? it.c0 : 0;
  bx.r1 = it.r1 < d.H - 1 ? it.r1 : d.H - 1;
  bx.c1 = it.c1 < d.W - 1 ? it.c1 : d.W - 1;
  return true;
}

// The donor pixel index (within the record) of target pixel (r, c), or -1 when it lies outside the clipped donor box.
__device__ __forceinline__ int64_t paste_donor(const UssegPasteDesc& d, const UssegPasteItem& it, const PasteBox& bx, int r, int c) {
  const int64_t pr = (int64_t)r - it.dr, cf = (int64_t)c - it.dc;
  const int64_t pc = it.flip ? (int64_t)d.W - 1 - cf : cf;
  if (pr < bx.r0 || pr > bx.r1 || pc < bx.c0 || pc > bx.c1) return -1;       // SAFETY: inside the box means inside the image
  return pr * d.W + pc;
}

__device__ __forceinline__ int clamp_n_items(int n) { return n < 0 ? 0 : (n > USSEG_PASTE_MAX_ITEMS ? USSEG_PASTE_MAX_ITEMS : n); }

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

template <int VB> struct PasteVec;
template <> struct PasteVec<16> { using type = uint4; };
template <> struct PasteVec<8> { using type = uint2; };
template <> struct PasteVec<4> { using type = uint32_t; };
}  // namespace

// Named outside the anonymous namespace: the profiler reports kernels of an anonymous namespace with an empty name.
//
// Workgroup blockIdx.x = b * USSEG_PASTE_MAX_ITEMS + i.  Every branch below depends on the workgroup's own item alone: the barrier is uniform.
__global__ __launch_bounds__(256) void paste_count_kernel(const UssegPasteDesc d, const UssegPasteSample* __restrict__ samples,
                                                          const float* __restrict__ y, const int32_t* __restrict__ labels,
                                                          int32_t* __restrict__ landed_out, unsigned long long* __restrict__ counts) {
  __shared__ int total;
  const int b = blockIdx.x / USSEG_PASTE_MAX_ITEMS, i = blockIdx.x % USSEG_PASTE_MAX_ITEMS;     // SAFETY: the grid is B * USSEG_PASTE_MAX_ITEMS
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  int cnt = 0;
  int need = 1;
  if (samples[b].active && i < clamp_n_items(samples[b].n_items)) {
    const UssegPasteItem it = samples[b].items[i];
    PasteBox bx;
    if (paste_item_box(d, it, bx) && bx.r0 <= bx.r1 && bx.c0 <= bx.c1) {
      need = it.need > 1 ? it.need : 1;
      // the target box: the donor box moved by (dr, dc), its columns mirrored first with flip; clipped to the image in 64 bits
      int64_t tr0 = (int64_t)bx.r0 + it.dr, tr1 = (int64_t)bx.r1 + it.dr;
      int64_t tc0 = (it.flip ? (int64_t)d.W - 1 - bx.c1 : (int64_t)bx.c0) + it.dc, tc1 = (it.flip ? (int64_t)d.W - 1 - bx.c0 : (int64_t)bx.c1) + it.dc;
      if (tr0 < 0) tr0 = 0;
      if (tc0 < 0) tc0 = 0;
      if (tr1 > d.H - 1) tr1 = d.H - 1;
      if (tc1 > d.W - 1) tc1 = d.W - 1;
      if (tr0 <= tr1 && tc0 <= tc1) {
        const int bw = (int)(tc1 - tc0 + 1), n = (int)(tr1 - tr0 + 1) * bw;                  // <= H*W < 2^31
        const int64_t ybase = (int64_t)b * d.H * d.W;
        for (int idx = threadIdx.x; idx < n; idx += kThreads) {
          const int r = (int)tr0 + idx / bw, c = (int)tc0 + idx % bw;                         // SAFETY: 0 <= r < H, 0 <= c < W
          const int64_t p = paste_donor(d, it, bx, r, c);
          if (p >= 0 && labels[bx.base + p] == it.comp && recipient_ok(y[ybase + (int64_t)r * d.W + c], d.protect)) ++cnt;
        }
      }
    }
  }
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&total, cnt);
  __syncthreads();
  if (threadIdx.x == 0) {
    landed_out[blockIdx.x] = total;
    if (total >= need) atomicAdd(counts, 1ULL);                    // need >= 1: an item that does not exist has total 0
  }
}

// VB bytes per lane of the copy; `units` = C * element size / VB lanes per pixel.
template <int VB>
__global__ __launch_bounds__(256) void paste_gather_kernel(const UssegPasteDesc d, const UssegPasteSample* __restrict__ samples,
                                                           const char* __restrict__ x, const uint32_t* __restrict__ y,
                                                           const char* __restrict__ x_bank, const uint32_t* __restrict__ y_bank,
                                                           const int32_t* __restrict__ labels, const int32_t* __restrict__ landed,
                                                           char* __restrict__ x_out, uint32_t* __restrict__ y_out,
                                                           unsigned long long* __restrict__ counts, int units) {
  using V = typename PasteVec<VB>::type;
  __shared__ int64_t src[kThreads];                                // bank pixel index of the pixel's source, or -1: its own x
  __shared__ int total;
  if (threadIdx.x == 0) total = 0;
  const int64_t plane = (int64_t)d.H * d.W, M = (int64_t)d.B * plane;            // M * C < 2^31 (checked by the entry point)
  const int64_t row_bytes = (int64_t)units * VB;
  int pasted = 0;
  for (int64_t m0 = (int64_t)blockIdx.x * kThreads; m0 < M; m0 += (int64_t)gridDim.x * kThreads) {   // uniform trip count: the barriers are uniform
    __syncthreads();                                               // the previous trip's readers of src are done (first trip: total is written)
    const int64_t m = m0 + threadIdx.x;
    if (m < M) {
      const int b = (int)(m / plane);
      const int rem = (int)(m - (int64_t)b * plane);
      const int r = rem / d.W, c = rem - r * d.W;
      const uint32_t ybits = y[m];
      int64_t s = -1;
      if (samples[b].active && recipient_ok(__uint_as_float(ybits), d.protect)) {
        for (int i = clamp_n_items(samples[b].n_items) - 1; i >= 0; --i) {                     // the LAST accepted item wins
          const UssegPasteItem it = samples[b].items[i];
          PasteBox bx;
          if (!paste_item_box(d, it, bx)) continue;
          const int64_t p = paste_donor(d, it, bx, r, c);
          if (p < 0) continue;
          if (landed[b * USSEG_PASTE_MAX_ITEMS + i] < (it.need > 1 ? it.need : 1)) continue;   // rejected by pass 1
          if (labels[bx.base + p] != it.comp) continue;            // SAFETY: bx.base + p < N*H*W
          s = bx.base + p;
          break;
        }
      }
      y_out[m] = s >= 0 ? y_bank[s] : ybits;
      pasted += s >= 0;
      src[threadIdx.x] = s;
    }
    __syncthreads();
    const int64_t left = M - m0;
    const int npix = left < kThreads ? (int)left : kThreads;
    const int64_t e0 = m0 * row_bytes;
    for (int u = threadIdx.x; u < npix * units; u += kThreads) {   // SAFETY: e0 + u*VB + VB <= M * row_bytes; pl < npix <= kThreads
      const int pl = u / units, k = u - pl * units;
      const int64_t s = src[pl];
      const char* from = s >= 0 ? x_bank + s * row_bytes + (int64_t)k * VB : x + e0 + (int64_t)u * VB;
      *reinterpret_cast<V*>(x_out + e0 + (int64_t)u * VB) = *reinterpret_cast<const V*>(from);       // the bits: no arithmetic, no conversion
    }
  }
  pasted = wave_sum(pasted);
  if ((threadIdx.x & 63) == 0 && pasted) atomicAdd(&total, pasted);
  __syncthreads();
  if (threadIdx.x == 0 && total) atomicAdd(counts + 1, (unsigned long long)total);
}

static bool paste_overlaps(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

extern "C" int usseg_lesion_paste(const UssegPasteDesc* d, const UssegPasteSample* samples_dev, const void* x, const float* y, const void* x_bank,
                                  const float* y_bank, const int32_t* labels_bank, void* x_out, float* y_out, int32_t* landed_out, int64_t* counts,
                                  usseg_stream_t stream) {
  USSEG_CHECK_ARG(d && samples_dev && x && y && x_bank && y_bank && labels_bank && x_out && y_out && landed_out && counts, "lesion_paste: null pointer");
  USSEG_CHECK_ARG(d->B >= 1 && d->H >= 1 && d->W >= 1 && d->C >= 1 && d->N >= 1, "lesion_paste: bad descriptor (B, H, W, C, N >= 1)");
  const int64_t M = (int64_t)d->B * d->H;                          // < 2^62
  USSEG_CHECK_ARG(M < ((int64_t)1 << 31) && M * d->W < ((int64_t)1 << 31) && M * d->W * d->C < ((int64_t)1 << 31),
                  "lesion_paste: bad descriptor (B*H*W*C < 2^31)");
  USSEG_CHECK_ARG(d->B < (1 << 29), "lesion_paste: bad descriptor (B < 2^29: one workgroup per sample and item)");
  const int es = d->x_is_f64 ? 8 : 4;
  const int64_t plane = (int64_t)d->H * d->W, pixels = M * d->W;   // plane * C <= B*H*W*C < 2^31
  USSEG_CHECK_ARG((int64_t)d->N * (plane * d->C) <= ((int64_t)1 << 59), "lesion_paste: bad descriptor (N*H*W*C*8 <= 2^62)");
  const uintptr_t xa = (uintptr_t)x | (uintptr_t)x_bank | (uintptr_t)x_out;
  USSEG_CHECK_ARG(xa % es == 0, "lesion_paste: x, x_bank and x_out must be aligned to their element (%d bytes)", es);
  USSEG_CHECK_ARG(((uintptr_t)y | (uintptr_t)y_bank | (uintptr_t)labels_bank | (uintptr_t)y_out | (uintptr_t)landed_out | (uintptr_t)samples_dev) % 4 == 0,
                  "lesion_paste: y, y_bank, labels_bank, y_out, landed_out and the sample table must be 4-byte aligned");
  USSEG_CHECK_ARG((uintptr_t)counts % 8 == 0, "lesion_paste: counts must be 8-byte aligned");
  const int64_t row_bytes = (int64_t)d->C * es;
  struct Span { const void* p; int64_t n; };
  const Span outs[4] = {{x_out, pixels * row_bytes}, {y_out, pixels * 4}, {landed_out, (int64_t)d->B * USSEG_PASTE_MAX_ITEMS * 4}, {counts, 16}};
  const Span ins[6] = {{x, pixels * row_bytes}, {y, pixels * 4}, {x_bank, (int64_t)d->N * plane * row_bytes}, {y_bank, (int64_t)d->N * plane * 4},
                       {labels_bank, (int64_t)d->N * plane * 4}, {samples_dev, (int64_t)d->B * (int64_t)sizeof(UssegPasteSample)}};
  for (int o = 0; o < 4; ++o) {
    for (int i = 0; i < 6; ++i)
      USSEG_CHECK_ARG(!paste_overlaps(outs[o].p, outs[o].n, ins[i].p, ins[i].n),
                      "lesion_paste: x_out / y_out / landed_out / counts must not overlap x / y, the bank or the sample table");
    for (int q = o + 1; q < 4; ++q)
      USSEG_CHECK_ARG(!paste_overlaps(outs[o].p, outs[o].n, outs[q].p, outs[q].n), "lesion_paste: x_out / y_out / landed_out / counts must not overlap each other");
  }
  hipLaunchKernelGGL(paste_count_kernel, dim3((unsigned)(d->B * USSEG_PASTE_MAX_ITEMS)), dim3(kThreads), 0, (hipStream_t)stream, *d, samples_dev, y,
                     labels_bank, landed_out, (unsigned long long*)counts);
  if (int rc = usseg_check_launch("lesion_paste (count)")) return rc;
  int64_t g = cdiv64(pixels, kThreads);
  if (g > kGridCap) g = kGridCap;
  const int vb = (row_bytes % 16 == 0 && xa % 16 == 0) ? 16 : (row_bytes % 8 == 0 && xa % 8 == 0) ? 8 : 4;    // the widest copy the pixel and the pointers allow
  const int units = (int)(row_bytes / vb);
#define USSEG_PASTE_LAUNCH(VB)                                                                                                                       \
  hipLaunchKernelGGL(paste_gather_kernel<VB>, dim3((unsigned)g), dim3(kThreads), 0, (hipStream_t)stream, *d, samples_dev, (const char*)x,           \
                     (const uint32_t*)y, (const char*)x_bank, (const uint32_t*)y_bank, labels_bank, (const int32_t*)landed_out, (char*)x_out,       \
                     (uint32_t*)y_out, (unsigned long long*)counts, units)
  if (vb == 16) USSEG_PASTE_LAUNCH(16);
  else if (vb == 8) USSEG_PASTE_LAUNCH(8);
  else USSEG_PASTE_LAUNCH(4);
#undef USSEG_PASTE_LAUNCH
  return usseg_check_launch("lesion_paste (gather)");
}
