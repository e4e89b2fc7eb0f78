// Ensemble prediction (include/usseg.h, "ensemble prediction, uncertainty maps and calibration counters"; not in the reference):
//   usseg_ensemble_merge         K member probability tensors -> mean, predictive entropy, mutual information (BALD), variance in ONE pass;
//   usseg_ensemble_image_scores  four scores per image of those maps, one workgroup per image, a fixed summation order;
//   usseg_calibration_bins       reliability counters (per-bin count / hits / confidence sum, Brier sum, invalid count) as exact integers.
// All three are streaming passes over tensors the previous launch wrote.  No allocation, no synchronisation: graph-capture safe.
//
// Roofline of the merge (HBM3E at 6.3 TB/s, the MI355X's measured float4-copy rate): (K*C + C + 2 + C) * 4 bytes per pixel, every member read
// once and every output written once = 80 B/pixel at K = 4, C = 3 with the variance: 26.2 MB at B=16 x 256x80 -> 4.2 us.  The accumulate
// form (one launch per member) would read a member and read and rewrite the 2C + 1 accumulators in each of its K launches:
// K*(C + 2*(2C + 1)) * 4 = 272 B/pixel before its finishing pass, 3.4x as much.  The pass evaluates K*C + C logf per pixel.
#include "common.h"

// BY VALUE in the kernel arguments: a captured graph holds the member pointers and the flip mask.  (Outside the anonymous namespace, like the
// kernels: the profiler reports a kernel whose name involves an anonymous namespace with an empty name.)
struct EnsembleMergeArgs {
  const float* m[USSEG_ENSEMBLE_MAX];
  float *mean, *ent, *mi, *var;
  int64_t M;                       // pixels
  int32_t W, C, K;
  uint32_t flip_w;
  int32_t vec3;
};

namespace {
using MergeArgs = EnsembleMergeArgs;
constexpr int kThreads = 256;
constexpr int kMaxGrid = 2048;
constexpr int kCalibSlots = USSEG_CALIB_MAX_BINS * 3 + 2;

// t(p) = p*logf(p): 0 for p <= 0, NaN for a NaN
__device__ __forceinline__ float plogp(float p) { return p > 0.f ? p * logf(p) : (p <= 0.f ? 0.f : p); }
// max(d, 0) that keeps a NaN (fmaxf would drop it)
__device__ __forceinline__ float clamp0(float d) { return d < 0.f ? 0.f : d; }

// One pixel's accumulators over the members: the class sums (member 0 starts them: no 0 + p_0), the sums of squares and sum t(p).
template <int NC>
struct PixAcc {
  float s[NC], q[NC], e;
};
template <int NC>
__device__ __forceinline__ void pix_add(PixAcc<NC>& a, const float (&p)[NC], bool first) {
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    a.s[c] = first ? p[c] : a.s[c] + p[c];
    a.q[c] = first ? p[c] * p[c] : a.q[c] + p[c] * p[c];
    a.e = (first && c == 0) ? plogp(p[c]) : a.e + plogp(p[c]);
  }
}
// -> mean[NC], var[NC], entropy, mutual information
template <int NC>
__device__ __forceinline__ void pix_finish(const PixAcc<NC>& a, float fK, float (&mean)[NC], float (&var)[NC], float& ent, float& mi) {
#pragma clang fp contract(off)
  float h = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    mean[c] = a.s[c] / fK;
    h = c == 0 ? plogp(mean[c]) : h + plogp(mean[c]);
    var[c] = clamp0(a.q[c] / fK - mean[c] * mean[c]);
  }
  ent = -h;
  mi = clamp0(ent - (-(a.e / fK)));
}

// The generic path: one pixel per lane and trip, scalar loads (any C <= 4 through NC, any alignment; the ragged tail of the fast path).
template <int NC>
__device__ __forceinline__ void merge_pixels(const MergeArgs& a, int64_t p_begin) {
  const bool small = a.M <= 0x7fffffff;
  const float fK = (float)a.K;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t p = p_begin + (int64_t)blockIdx.x * kThreads + threadIdx.x; p < a.M; p += stride) {
    const int w = mod_w(p, a.W, small);
    const int64_t pf = p + (a.W - 1 - 2 * w);          // the same row's pixel W-1-w: 0 <= W-1-w < W, so pf stays inside the row of p
    PixAcc<NC> acc;
    for (int k = 0; k < a.K; ++k) {
      const float* src = a.m[k] + (((a.flip_w >> k) & 1u) ? pf : p) * NC;
      float v[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) v[c] = src[c];
      pix_add<NC>(acc, v, k == 0);
    }
    float mean[NC], var[NC], ent, mi;
    pix_finish<NC>(acc, fK, mean, var, ent, mi);
#pragma unroll
    for (int c = 0; c < NC; ++c) a.mean[p * NC + c] = mean[c];
    a.ent[p] = ent;
    a.mi[p] = mi;
    if (a.var) {
#pragma unroll
      for (int c = 0; c < NC; ++c) a.var[p * NC + c] = var[c];
    }
  }
}

// C == 3, every base 16-byte aligned: groups of four pixels = twelve floats = three float4 per tensor.  An un-mirrored member is read as three
// float4; a mirrored member pixel by pixel (its four source pixels run backwards and are 16-byte aligned only by chance), each with the
// column of ITS pixel: a group that straddles two image rows mirrors each part inside its own row.
__device__ __forceinline__ void merge_groups3(const MergeArgs& a) {
  const bool small = a.M <= 0x7fffffff;
  const float fK = (float)a.K;
  const int64_t G = a.M >> 2, stride = (int64_t)gridDim.x * kThreads;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < G; g += stride) {
    const int64_t p0 = g * 4;
    int wu[4];
    wu[0] = mod_w(p0, a.W, small);
#pragma unroll
    for (int u = 1; u < 4; ++u) wu[u] = wu[u - 1] + 1 == a.W ? 0 : wu[u - 1] + 1;
    PixAcc<3> acc[4];
    for (int k = 0; k < a.K; ++k) {            // (unrolling this loop by two - six float4 loads in flight - measured no faster: DESIGN.md section 8)
      float v[12];
      if ((a.flip_w >> k) & 1u) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float* src = a.m[k] + (p0 + u + (a.W - 1 - 2 * wu[u])) * 3;      // inside the row of pixel p0 + u (< M): in bounds
#pragma unroll
          for (int c = 0; c < 3; ++c) v[u * 3 + c] = src[c];
        }
      } else {
        const float4* s4 = reinterpret_cast<const float4*>(a.m[k]) + g * 3;
        const float4 x = s4[0], y = s4[1], z = s4[2];
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
        v[8] = z.x; v[9] = z.y; v[10] = z.z; v[11] = z.w;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float pv[3] = {v[u * 3], v[u * 3 + 1], v[u * 3 + 2]};
        pix_add<3>(acc[u], pv, k == 0);
      }
    }
    float mean[12], var[12], ent[4], mi[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float mu[3], vu[3];
      pix_finish<3>(acc[u], fK, mu, vu, ent[u], mi[u]);
#pragma unroll
      for (int c = 0; c < 3; ++c) { mean[u * 3 + c] = mu[c]; var[u * 3 + c] = vu[c]; }
    }
    float4* m4 = reinterpret_cast<float4*>(a.mean) + g * 3;
    m4[0] = make_float4(mean[0], mean[1], mean[2], mean[3]);
    m4[1] = make_float4(mean[4], mean[5], mean[6], mean[7]);
    m4[2] = make_float4(mean[8], mean[9], mean[10], mean[11]);
    reinterpret_cast<float4*>(a.ent)[g] = make_float4(ent[0], ent[1], ent[2], ent[3]);
    reinterpret_cast<float4*>(a.mi)[g] = make_float4(mi[0], mi[1], mi[2], mi[3]);
    if (a.var) {
      float4* v4 = reinterpret_cast<float4*>(a.var) + g * 3;
      v4[0] = make_float4(var[0], var[1], var[2], var[3]);
      v4[1] = make_float4(var[4], var[5], var[6], var[7]);
      v4[2] = make_float4(var[8], var[9], var[10], var[11]);
    }
  }
}
}  // namespace

// Named outside the anonymous namespace: the profiler reports kernels of an anonymous namespace with an empty name.
template <int NC>
__global__ __launch_bounds__(256) void ensemble_merge_kernel(const MergeArgs a) {
  int64_t p_tail = 0;
  if constexpr (NC == 3) {
    if (a.vec3) {
      merge_groups3(a);
      p_tail = (a.M >> 2) * 4;
    }
  }
  merge_pixels<NC>(a, p_tail);
}

// One workgroup of kScoreThreads per image.  A lane adds its pixels (tid, tid + kScoreThreads, ...) in ascending order; the lane totals are
// combined by a fixed halving tree in LDS: the same additions in the same order on every run.  The maximum keeps a NaN once it has met one.
// 1024 lanes, the pixel loop unrolled: an image is one workgroup's work, so what hides the load latency is the number of loads it has in flight.
constexpr int kScoreThreads = 1024;
__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }

__global__ __launch_bounds__(kScoreThreads) void ensemble_image_scores_kernel(const float* __restrict__ mean, const float* __restrict__ ent,
                                                                     const float* __restrict__ mi, int HW, int C, float* __restrict__ scores,
                                                                     int32_t* __restrict__ counts) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* mb = mean + (int64_t)b * HW * C;
  const float* eb = ent + (int64_t)b * HW;
  const float* ib = mi + (int64_t)b * HW;
  float se = 0.f, sm = 0.f, mx = -INFINITY, sl = 0.f;
  int n = 0;
#pragma unroll 4
  for (int i = tid; i < HW; i += kScoreThreads) {
    const float e = eb[i], m = ib[i];
    float best = mb[(int64_t)i * C];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
      const float v = mb[(int64_t)i * C + c];
      if (v > best) { best = v; arg = c; }            // first maximum; a NaN is never larger
    }
    se += e;
    sm += m;
    mx = max_nan(mx, m);
    if (arg == C - 1) { sl += e; ++n; }
  }
  __shared__ float r[4][kScoreThreads];
  __shared__ int rn[kScoreThreads];
  r[0][tid] = se; r[1][tid] = sm; r[2][tid] = mx; r[3][tid] = sl; rn[tid] = n;
  __syncthreads();
  for (int h = kScoreThreads / 2; h >= 1; h >>= 1) {
    if (tid < h) {
      r[0][tid] += r[0][tid + h];
      r[1][tid] += r[1][tid + h];
      r[2][tid] = max_nan(r[2][tid], r[2][tid + h]);
      r[3][tid] += r[3][tid + h];
      rn[tid] += rn[tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float fn = (float)HW;
    scores[b * 4 + 0] = r[0][0] / fn;
    scores[b * 4 + 1] = r[1][0] / fn;
    scores[b * 4 + 2] = r[2][0];
    scores[b * 4 + 3] = rn[0] ? r[3][0] / (float)rn[0] : 0.f;
    counts[b] = rn[0];
  }
}

// Reliability counters.  Per workgroup a histogram of 64-bit counters in LDS (integer atomics), then one 64-bit integer atomic per non-zero
// counter: integer adds do not depend on arrival order, so the result is bitwise reproducible without an ordered sum.
template <int NC>
__global__ __launch_bounds__(256) void calibration_bins_kernel(const float* __restrict__ probs, const float* __restrict__ yt, int64_t M, int bins,
                                                                int cls, unsigned long long* __restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ unsigned long long h[kCalibSlots];
  const int slots = bins * 3 + 2;               // bins <= USSEG_CALIB_MAX_BINS (checked by the entry point): slots <= kCalibSlots
  for (int i = threadIdx.x; i < slots; i += kThreads) h[i] = 0ull;
  __syncthreads();
  unsigned long long brier = 0ull;
  unsigned int invalid = 0u;
  const float fbins = (float)bins;
  for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < M; p += (int64_t)gridDim.x * kThreads) {
    float pv[NC], tv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { pv[c] = probs[p * NC + c]; tv[c] = yt[p * NC + c]; }
    int ap = 0, at = 0;                          // first maxima; a NaN is never larger
    float pbest = pv[0], tbest = tv[0];
#pragma unroll
    for (int c = 1; c < NC; ++c) {
      if (pv[c] > pbest) { pbest = pv[c]; ap = c; }
      if (tv[c] > tbest) { tbest = tv[c]; at = c; }
    }
    float conf = pbest;
    bool hit = ap == at;
    if (cls >= 0) {
      conf = pv[0];
#pragma unroll
      for (int c = 1; c < NC; ++c) conf = c == cls ? pv[c] : conf;
      hit = at == cls;
    }
    // SAFETY: the validity test and the clamp come BEFORE any LDS index is formed.  A NaN, a negative or a greater-than-1 confidence
    // fails `valid` (a NaN compares false) and touches no bin; a valid one gives 0 <= (int)(conf*bins) <= bins, clamped into [0, bins-1].
    const bool valid = conf >= 0.f && conf <= 1.f;
    if (!valid) { ++invalid; continue; }
    int bin = (int)(conf * fbins);
    bin = bin > bins - 1 ? bins - 1 : bin;
    bin = bin < 0 ? 0 : bin;
    float v = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float d = pv[c] - (c == at ? 1.f : 0.f);
      v = c == 0 ? d * d : v + d * d;
    }
    if (!(v <= (float)NC)) v = (float)NC;        // a NaN or out-of-range neighbour class: counted as the largest in-range value
    brier += (unsigned long long)rintf(v * 16777216.f);
    atomicAdd(&h[bin * 3 + 0], 1ull);
    if (hit) atomicAdd(&h[bin * 3 + 1], 1ull);
    atomicAdd(&h[bin * 3 + 2], (unsigned long long)rintf(conf * 16777216.f));
  }
  if (brier) atomicAdd(&h[bins * 3], brier);
  if (invalid) atomicAdd(&h[bins * 3 + 1], (unsigned long long)invalid);
  __syncthreads();
  for (int i = threadIdx.x; i < slots; i += kThreads) {
    const unsigned long long s = h[i];
    if (s) atomicAdd(counts + i, s);             // device scope: the workgroups of every XCD add into the same block
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int usseg_ensemble_merge(const UssegEnsembleDesc* d, const float* const* members, uint32_t flip_w, float* mean_probs, float* entropy,
                                    float* mutual_info, float* variance, usseg_stream_t stream) {
  USSEG_CHECK_ARG(d && members && mean_probs && entropy && mutual_info, "ensemble_merge: null pointer");
  USSEG_CHECK_ARG(d->B >= 1 && d->H >= 1 && d->W >= 1 && (int64_t)d->H * d->W <= 0x7fffffff, "ensemble_merge: bad descriptor (B, H, W >= 1; H*W < 2^31)");
  USSEG_CHECK_ARG(d->C >= 1 && d->C <= 4, "ensemble_merge: bad descriptor (1 <= C <= 4)");
  USSEG_CHECK_ARG(d->K >= 1 && d->K <= USSEG_ENSEMBLE_MAX, "ensemble_merge: bad descriptor (1 <= K <= %d)", USSEG_ENSEMBLE_MAX);
  USSEG_CHECK_ARG((flip_w >> d->K) == 0u, "ensemble_merge: flip_w has bits at or above K");
  MergeArgs a = {};
  bool al = aligned16(mean_probs) && aligned16(entropy) && aligned16(mutual_info) && aligned16(variance);
  for (int k = 0; k < d->K; ++k) {
    USSEG_CHECK_ARG(members[k], "ensemble_merge: null pointer (member %d)", k);
    a.m[k] = members[k];
    al = al && aligned16(members[k]);
  }
  a.mean = mean_probs; a.ent = entropy; a.mi = mutual_info; a.var = variance;
  a.M = (int64_t)d->B * d->H * d->W;
  a.W = d->W; a.C = d->C; a.K = d->K; a.flip_w = flip_w;
  a.vec3 = d->C == 3 && al;
  const int64_t work = a.vec3 && a.M >= 4 ? a.M >> 2 : a.M;      // (grid-stride loops: any grid covers the groups and the tail)
  int64_t g = cdiv64(work, kThreads);
  if (g > kMaxGrid) g = kMaxGrid;
  auto k = d->C == 1 ? ensemble_merge_kernel<1> : d->C == 2 ? ensemble_merge_kernel<2> : d->C == 3 ? ensemble_merge_kernel<3> : ensemble_merge_kernel<4>;
  hipLaunchKernelGGL(k, dim3((unsigned)g), dim3(kThreads), 0, (hipStream_t)stream, a);
  return usseg_check_launch("ensemble_merge");
}

extern "C" int usseg_ensemble_image_scores(const UssegEnsembleDesc* d, const float* mean_probs, const float* entropy, const float* mutual_info,
                                           float* scores, int32_t* counts, usseg_stream_t stream) {
  USSEG_CHECK_ARG(d && mean_probs && entropy && mutual_info && scores && counts, "ensemble_image_scores: null pointer");
  USSEG_CHECK_ARG(d->B >= 1 && d->H >= 1 && d->W >= 1 && (int64_t)d->H * d->W <= 0x7fffffff,
                  "ensemble_image_scores: bad descriptor (B, H, W >= 1; H*W < 2^31)");
  USSEG_CHECK_ARG(d->C >= 1 && d->C <= 4, "ensemble_image_scores: bad descriptor (1 <= C <= 4)");
  hipLaunchKernelGGL(ensemble_image_scores_kernel, dim3((unsigned)d->B), dim3(kScoreThreads), 0, (hipStream_t)stream, mean_probs, entropy, mutual_info,
                     d->H * d->W, (int)d->C, scores, counts);
  return usseg_check_launch("ensemble_image_scores");
}

extern "C" int usseg_calibration_bins(const UssegCalibDesc* d, const float* probs, const float* y_true, int64_t* counts, usseg_stream_t stream) {
  USSEG_CHECK_ARG(d && probs && y_true && counts, "calibration_bins: null pointer");
  USSEG_CHECK_ARG(d->B >= 0 && d->H >= 0 && d->W >= 1, "calibration_bins: bad descriptor (B, H >= 0; W >= 1)");
  USSEG_CHECK_ARG(d->C >= 1 && d->C <= 4, "calibration_bins: bad descriptor (1 <= C <= 4)");
  USSEG_CHECK_ARG(d->bins >= 1 && d->bins <= USSEG_CALIB_MAX_BINS, "calibration_bins: bad descriptor (1 <= bins <= %d)", USSEG_CALIB_MAX_BINS);
  USSEG_CHECK_ARG(d->cls >= -1 && d->cls < d->C, "calibration_bins: bad descriptor (cls is -1 or a class below C)");
  const int64_t M = (int64_t)d->B * d->H * d->W;
  if (M == 0) return USSEG_OK;
  int64_t g = cdiv64(M, kThreads);
  if (g > 256) g = 256;           // one workgroup per CU: every arrival on the counter block costs at the memory side (metrics.hip)
  auto k = d->C == 1 ? calibration_bins_kernel<1> : d->C == 2 ? calibration_bins_kernel<2> : d->C == 3 ? calibration_bins_kernel<3> : calibration_bins_kernel<4>;
  hipLaunchKernelGGL(k, dim3((unsigned)g), dim3(kThreads), 0, (hipStream_t)stream, probs, y_true, M, (int)d->bins, (int)d->cls,
                     reinterpret_cast<unsigned long long*>(counts));
  return usseg_check_launch("calibration_bins");
}
