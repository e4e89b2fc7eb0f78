// Validation metrics of the reference's drivers (MainNumpy.py:49-53,100-106; TBI_ResNest.py:421-426; TBI_TransUNet.py:947-956;
// MainParallel.py:86-114,148-176) as exact integer counters: one streaming pass over the probabilities and labels that are already in
// HBM.  The five Keras metric objects (Precision, Recall, their `c2` pair and MeanIoU) become the counters of usseg.h
// (USSEG_SEG_COUNTS): TP / FP / FN over every element, the same three over the last image column, the confusion matrix and a count
// of the elements Keras would reject.  Counters live in registers (uint32) and are reduced across the wave and the workgroup; each
// workgroup then adds its totals into the uint64 block with ONE atomic wave-instruction.  Integer adds do not depend on arrival
// order: the result is bitwise reproducible without an ordered sum.  No allocation, no synchronisation: graph-capture safe.
#include "common.h"

namespace {

constexpr int kThreads = 512;     // 8 waves
constexpr int kMaxGrid = 256;     // one workgroup per CU: each arrival on the counter block costs ~12 ns at the memory side (fan-in)

template <int NC>
struct SegCnt {
  static constexpr int NPC = NC < 2 ? NC : 2;      // a valid prediction lies in [0, 1]: its class is 0 or 1 (1 only for exactly 1.0)
  static constexpr int N = 7 + NC * NC;            // [0..5] TP FP FN (all, last column), [6..) cm[true][pred], [6+NC*NC] invalid
  uint32_t v[N];
};

// One element, as Keras scores it.  `last`: the element lies in the image's last column (the reference's y[:, :, -1] on a 4-D tensor).
template <int NC>
__device__ __forceinline__ void seg_elem(float t, float p, bool last, bool rnd, SegCnt<NC>& k) {
  if (rnd) { t = rintf(t); p = rintf(p); }            // tf.math.round: half to even
  const bool tpos = t != 0.f;                          // Precision / Recall cast y_true to bool
  const bool ppos = p > 0.5f;                          // default threshold
  const uint32_t tp = tpos & ppos, fp = !tpos & ppos, fn = tpos & !ppos;
  k.v[0] += tp; k.v[1] += fp; k.v[2] += fn;
  k.v[3] += tp & last; k.v[4] += fp & last; k.v[5] += fn & last;
  // confusion_matrix casts to int64 (truncation) and rejects classes outside [0, NC); Precision / Recall reject predictions outside [0, 1]
  const bool tval = t > -1.f && t < (float)NC;
  const bool pval = p >= 0.f && p <= 1.f && p < (float)NC;
  const bool ok = tval && pval;
  const int idx = ok ? (int)t * NC + (int)p : -1;
#pragma unroll
  for (int a = 0; a < NC; ++a)
#pragma unroll
    for (int b = 0; b < SegCnt<NC>::NPC; ++b) k.v[6 + a * NC + b] += idx == a * NC + b;
  k.v[6 + NC * NC] += !ok;
}

// The generic path: one pixel per thread and trip, scalar loads (any C, any alignment; the ragged tail of the fast path).
template <int NC>
__device__ __forceinline__ void seg_pixels(const float* __restrict__ yt, const float* __restrict__ yp, int64_t p_begin, int64_t M, int W, int C,
                                           bool rnd, SegCnt<NC>& k) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t p = p_begin + (int64_t)blockIdx.x * kThreads + threadIdx.x; p < M; p += stride) {
    const bool last = mod_w(p, W, M <= 0x7fffffff) == W - 1;
    for (int c = 0; c < C; ++c) seg_elem<NC>(yt[p * C + c], yp[p * C + c], last, rnd, k);
  }
}

// Four pixels of the reference's three classes = twelve floats = three float4 per tensor (16-byte aligned when both bases are).
template <int NC>
__device__ __forceinline__ void seg_group3(const float4 (&t)[3], const float4 (&p)[3], int w, int W, bool rnd, SegCnt<NC>& k) {
  const float tv[12] = {t[0].x, t[0].y, t[0].z, t[0].w, t[1].x, t[1].y, t[1].z, t[1].w, t[2].x, t[2].y, t[2].z, t[2].w};
  const float pv[12] = {p[0].x, p[0].y, p[0].z, p[0].w, p[1].x, p[1].y, p[1].z, p[1].w, p[2].x, p[2].y, p[2].z, p[2].w};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const bool last = w == W - 1;
#pragma unroll
    for (int c = 0; c < 3; ++c) seg_elem<NC>(tv[u * 3 + c], pv[u * 3 + c], last, rnd, k);
    w = w + 1 == W ? 0 : w + 1;
  }
}

template <int NC>
__global__ __launch_bounds__(kThreads) void seg_counts_kernel(const float* __restrict__ yt, const float* __restrict__ yp, int64_t M, int W, int C,
                                                               int rnd, int vec3, unsigned long long* __restrict__ counts) {
  SegCnt<NC> k;
#pragma unroll
  for (int i = 0; i < SegCnt<NC>::N; ++i) k.v[i] = 0u;
  int64_t p_tail = 0;
  const bool small = M <= 0x7fffffff;     // 32-bit column arithmetic (uniform branch)
  if (vec3) {        // C == 3, both bases 16-byte aligned: groups of four pixels, two groups per thread and trip (12 loads in flight)
    const int64_t G = M >> 2, stride = (int64_t)gridDim.x * kThreads;
    const float4* t4 = reinterpret_cast<const float4*>(yt);
    const float4* p4 = reinterpret_cast<const float4*>(yp);
    int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    for (; g + stride < G; g += 2 * stride) {
      float4 ta[3], pa[3], tb[3], pb[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        ta[i] = t4[g * 3 + i]; pa[i] = p4[g * 3 + i];
        tb[i] = t4[(g + stride) * 3 + i]; pb[i] = p4[(g + stride) * 3 + i];
      }
      seg_group3<NC>(ta, pa, mod_w(g * 4, W, small), W, rnd, k);
      seg_group3<NC>(tb, pb, mod_w((g + stride) * 4, W, small), W, rnd, k);
    }
    if (g < G) {
      float4 ta[3], pa[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) { ta[i] = t4[g * 3 + i]; pa[i] = p4[g * 3 + i]; }
      seg_group3<NC>(ta, pa, mod_w(g * 4, W, small), W, rnd, k);
    }
    p_tail = G * 4;
  }
  seg_pixels<NC>(yt, yp, p_tail, M, W, C, rnd, k);

  // wave -> workgroup -> one atomic wave-instruction into the uint64 block
  __shared__ uint32_t red[kThreads / 64][SegCnt<NC>::N];
#pragma unroll
  for (int i = 0; i < SegCnt<NC>::N; ++i) {
    uint32_t s = k.v[i];
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) s += __shfl_xor(s, msk, 64);
    k.v[i] = s;
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < SegCnt<NC>::N; ++i) red[threadIdx.x >> 6][i] = k.v[i];
  }
  __syncthreads();
  if (threadIdx.x < SegCnt<NC>::N) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += red[w][threadIdx.x];
    if (s) atomicAdd(counts + threadIdx.x, s);      // device scope: the workgroups of every XCD add into the same block
  }
}

template <int NC>
void launch(const UssegSegCountDesc& d, const float* yt, const float* yp, uint64_t* counts, int64_t M, int vec3, hipStream_t s) {
  const int64_t work = vec3 ? (M >> 2) : M;
  int64_t g = cdiv64(work > 0 ? work : 1, kThreads);
  if (g > kMaxGrid) g = kMaxGrid;
  hipLaunchKernelGGL(seg_counts_kernel<NC>, dim3((unsigned)g), dim3(kThreads), 0, s, yt, yp, M, (int)d.W, (int)d.C, (int)d.round, vec3,
                     reinterpret_cast<unsigned long long*>(counts));
}

}  // namespace

extern "C" int usseg_seg_counts(const UssegSegCountDesc* d, const float* y_true, const float* y_pred, uint64_t* counts, usseg_stream_t stream) {
  USSEG_CHECK_ARG(d && y_true && y_pred && counts, "seg_counts: null pointer");
  USSEG_CHECK_ARG(d->B >= 0 && d->H >= 0 && d->W >= 1 && d->C >= 1, "seg_counts: bad descriptor (B, H >= 0; W, C >= 1)");
  USSEG_CHECK_ARG(d->num_classes >= 1 && d->num_classes <= 4, "seg_counts: bad descriptor (1 <= num_classes <= 4)");
  USSEG_CHECK_ARG(d->round == 0 || d->round == 1, "seg_counts: bad descriptor (round is 0 or 1)");
  const int64_t M = (int64_t)d->B * d->H * d->W;
  if (M == 0) return USSEG_OK;
  const int vec3 = d->C == 3 && ((reinterpret_cast<uintptr_t>(y_true) | reinterpret_cast<uintptr_t>(y_pred)) & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  switch (d->num_classes) {
    case 1: launch<1>(*d, y_true, y_pred, counts, M, vec3, s); break;
    case 2: launch<2>(*d, y_true, y_pred, counts, M, vec3, s); break;
    case 3: launch<3>(*d, y_true, y_pred, counts, M, vec3, s); break;
    default: launch<4>(*d, y_true, y_pred, counts, M, vec3, s); break;
  }
  return usseg_check_launch("seg_counts");
}
