// Operating points and temperature scaling (include/usseg.h, "threshold sweeps and temperature scaling"; not in the reference):
//   usseg_score_sweep        per score bin the negatives and the positives of one class, as exact integers: the one table ROC, PR, AUC, average
//                            precision and Dice against the threshold come from (metrics.sweep_from_counts);
//   usseg_temperature_nll    the negative log-likelihood of up to 16 candidate inverse temperatures in ONE read of the batch, as exact integers;
//   usseg_apply_temperature  probs -> softmax(beta * log(probs + 1e-7)), beta a DEVICE float a captured graph follows.
// All three are streaming passes after the pattern of calibration_bins_kernel (ensemble.hip): integer counters, a validity test and a clamp
// before any index is formed, LDS of a fixed size the entry point checks against, no data-dependent loop bound.  No allocation, no
// synchronisation: graph-capture safe.  Accurate logf / expf / IEEE division throughout (the tests' bounds rest on their error).
//
// Bytes at B=16 x 256x80, C=3: the two counting passes read probs and y_true once, 24 B/pixel = 7.9 MB (1.2 us at the 6.3 TB/s float4-copy rate
// of HBM3E; the L2 / MALL hold both tensors when the previous launch wrote them); apply reads and writes probs, 24 B/pixel.
#include "common.h"

// Build switch of tools/time_sweep.py ONLY (it compiles this file a second time with -DUSSEG_SWEEP_AGGREGATE=0 to time the plain path, and with
// -DUSSEG_SWEEP_TOOL_PROBE to read the device's logf / expf): the product is built with neither and has one form of each kernel.
#ifndef USSEG_SWEEP_AGGREGATE
#define USSEG_SWEEP_AGGREGATE 1
#endif

// BY VALUE in the kernel arguments: a captured graph holds the candidates.
struct TemperatureBetas {
  float b[USSEG_TEMP_MAX_BETAS];
};

namespace {
constexpr int kThreads = 256;
constexpr int kCountGrid = 256;       // one workgroup per CU: every arrival on the counter block costs at the memory side (calibration_bins)
constexpr int kApplyGrid = 2048;
constexpr int kSweepSlots = 2 * USSEG_SWEEP_MAX_BINS;      // 8192 32-bit counters = 32 KB of static LDS (the default limit is 64 KB)
constexpr int kTempSlots = USSEG_TEMP_MAX_BETAS + 2;
constexpr float kEps = 1e-7f;         // the CCE's epsilon (attn_loss_optim.hip)
static_assert(kSweepSlots * sizeof(unsigned int) + sizeof(unsigned int) <= 64 * 1024, "score_sweep: the histograms must fit the default static LDS limit");
static_assert(kTempSlots * kThreads * sizeof(unsigned long long) <= 64 * 1024, "temperature_nll: the reduction tree must fit the default static LDS limit");

// the first-maximum class of y_true; a NaN is never larger (calibration_bins_kernel's `at`)
template <int NC>
__device__ __forceinline__ int first_max(const float (&t)[NC]) {
  int at = 0;
  float best = t[0];
#pragma unroll
  for (int c = 1; c < NC; ++c) {
    if (t[c] > best) { best = t[c]; at = c; }
  }
  return at;
}

// One pixel of the temperature: out_c = expf(beta*z_c - m) / sum_c expf(beta*z_c - m), z_c = logf(p_c + 1e-7f), m = max_c beta*z_c, the sum in
// ascending class order.  A z_c that is NaN (a NaN input, or one below -1e-7) makes every class of the pixel NaN.
template <int NC>
__device__ __forceinline__ void temper_pixel(const float (&p)[NC], float beta, float (&o)[NC]) {
#pragma clang fp contract(off)
  float t[NC], m = 0.f;
  bool nan = false;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    t[c] = beta * logf(p[c] + kEps);
    nan = nan || t[c] != t[c];
    m = (c == 0 || t[c] > m) ? t[c] : m;
  }
  float e[NC], s = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    e[c] = expf(t[c] - m);
    s = c == 0 ? e[c] : s + e[c];
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) o[c] = nan ? __builtin_nanf("") : e[c] / s;
}
}  // namespace

// Named outside the anonymous namespace: the profiler reports kernels of an anonymous namespace with an empty name.
//
// Sweep counters.  Per workgroup two interleaved histograms of 32-bit counters in LDS (slot 2*bin + positive), then one 64-bit integer global
// atomic per non-zero counter: integer adds do not depend on arrival order or on the grid, so the result is bitwise reproducible.
// A 32-bit LDS counter cannot wrap: a workgroup counts at most ceil(M / gridDim.x) <= 2^31 / 256 pixels when the grid is capped, and fewer than
// 256 * 256 otherwise.
template <int NC, bool AGG>
__global__ __launch_bounds__(256) void score_sweep_kernel(const float* __restrict__ probs, const float* __restrict__ yt, int64_t M, int bins,
                                                           int cls, unsigned long long* __restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ unsigned int h[kSweepSlots];
  __shared__ unsigned int h_invalid;
  const int slots = 2 * bins;                   // bins <= USSEG_SWEEP_MAX_BINS (checked by the entry point): slots <= kSweepSlots
  for (int i = threadIdx.x; i < slots; i += kThreads) h[i] = 0u;
  if (threadIdx.x == 0) h_invalid = 0u;
  __syncthreads();
  unsigned int invalid = 0u;
  const float fbins = (float)bins;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  // The trip count depends on blockIdx alone, so every lane of a wave stays in the loop for the same trips and the wave votes as a whole;
  // a lane past M (the last, partial trip) holds key -1 like an invalid pixel.
  for (int64_t base = (int64_t)blockIdx.x * kThreads; base < M; base += stride) {
    const int64_t p = base + threadIdx.x;
    int key = -1;
    if (p < M) {
      float tv[NC];
      float s = probs[p * NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        tv[c] = yt[p * NC + c];
        if (c > 0) s = c == cls ? probs[p * NC + c] : s;
      }
      const int positive = first_max<NC>(tv) == cls ? 1 : 0;
      // SAFETY: the validity test and the clamp come BEFORE any LDS index is formed.  A NaN, a negative or a greater-than-1 score fails
      // `valid` (a NaN compares false) and touches no bin; a valid one gives 0 <= (int)(s*bins) <= bins, clamped into [0, bins-1], so
      // 0 <= key = 2*bin + positive <= 2*bins - 1 < slots <= kSweepSlots.
      const bool valid = s >= 0.f && s <= 1.f;
      if (valid) {
        int bin = (int)(s * fbins);
        bin = bin > bins - 1 ? bins - 1 : bin;
        bin = bin < 0 ? 0 : bin;
        key = 2 * bin + positive;
      } else {
        ++invalid;
      }
    }
    if constexpr (AGG) {
      // The bleed class is skewed: most waves hold one key (bin 0, negative) in every lane, and 64 LDS atomics on one address serialise.
      // When every lane that has a key holds the key of the first such lane, that lane adds the population count; otherwise each lane
      // adds its own 1.  Both forms add the same integers.
      const unsigned long long has = __ballot(key >= 0);
      if (has != 0ull) {                                              // wave-uniform
        const int first = __ffsll(has) - 1;                           // SAFETY: has != 0, so 0 <= first <= 63: a lane of this wave
        const int key0 = __shfl(key, first);                          // SAFETY: lane `first` voted key >= 0, so key0 is ITS checked key, in [0, slots)
        const unsigned long long same = __ballot(key == key0);
        if (same == has) {
          if (lane == first) atomicAdd(&h[key0], (unsigned int)__popcll(has));
        } else if (key >= 0) {
          atomicAdd(&h[key], 1u);                                     // SAFETY: key >= 0 only from the checked branch above
        }
      }
    } else {
      if (key >= 0) atomicAdd(&h[key], 1u);                           // SAFETY: key >= 0 only from the checked branch above
    }
  }
  if (invalid) atomicAdd(&h_invalid, invalid);
  __syncthreads();
  for (int i = threadIdx.x; i < slots; i += kThreads) {                // SAFETY: i < slots = 2*bins; counts holds 2*bins + 1 elements
    const unsigned int s = h[i];
    if (s) atomicAdd(counts + i, (unsigned long long)s);               // device scope: the workgroups of every XCD add into the same block
  }
  if (threadIdx.x == 0 && h_invalid) atomicAdd(counts + slots, (unsigned long long)h_invalid);
}

// NLL counters of n_beta candidates.  A lane keeps 64-bit sums; one halving tree in LDS per workgroup; one 64-bit global atomic per counter.
template <int NC>
__global__ __launch_bounds__(256) void temperature_nll_kernel(const float* __restrict__ probs, const float* __restrict__ yt, int64_t M, int n_beta,
                                                               const TemperatureBetas betas, unsigned long long* __restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ unsigned long long red[kTempSlots][kThreads];
  unsigned long long acc[USSEG_TEMP_MAX_BETAS];
#pragma unroll
  for (int j = 0; j < USSEG_TEMP_MAX_BETAS; ++j) acc[j] = 0ull;
  unsigned long long n_valid = 0ull, n_invalid = 0ull;
  for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < M; p += (int64_t)gridDim.x * kThreads) {
    float z[NC], tv[NC];
    bool valid = true;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float pv = probs[p * NC + c];
      tv[c] = yt[p * NC + c];
      valid = valid && pv >= 0.f && pv <= 1.f;          // a NaN compares false
      z[c] = logf(pv + kEps);
    }
    if (!valid) { ++n_invalid; continue; }
    ++n_valid;
    const int y = first_max<NC>(tv);
    float zy = z[0];
#pragma unroll
    for (int c = 1; c < NC; ++c) zy = c == y ? z[c] : zy;
#pragma unroll
    for (int j = 0; j < USSEG_TEMP_MAX_BETAS; ++j) {                 // a fixed trip count with a uniform predicate: acc[] stays in registers
      if (j < n_beta) {
        const float beta = betas.b[j];
        float t[NC], m = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          t[c] = beta * z[c];
          m = (c == 0 || t[c] > m) ? t[c] : m;
        }
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const float e = expf(t[c] - m);
          s = c == 0 ? e : s + e;
        }
        float nll = (m + logf(s)) - beta * zy;
        nll = nll > 0.f ? nll : 0.f;                                   // (also a NaN, which a valid pixel cannot give)
        nll = nll < (float)USSEG_TEMP_NLL_CAP ? nll : (float)USSEG_TEMP_NLL_CAP;
        acc[j] += (unsigned long long)rintf(nll * 1048576.f);
      }
    }
  }
  // SAFETY: every index below is a compile-time slot (< kTempSlots) and threadIdx.x (+ h with threadIdx.x < h): inside red[kTempSlots][kThreads].
#pragma unroll
  for (int j = 0; j < USSEG_TEMP_MAX_BETAS; ++j) red[j][threadIdx.x] = acc[j];
  red[USSEG_TEMP_MAX_BETAS][threadIdx.x] = n_valid;
  red[USSEG_TEMP_MAX_BETAS + 1][threadIdx.x] = n_invalid;
  __syncthreads();
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) {
#pragma unroll
      for (int j = 0; j < kTempSlots; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + h];
    }
    __syncthreads();
  }
  // SAFETY: lane j < n_beta <= 16 writes counts[j]; lanes 16 and 17 write counts[n_beta] and counts[n_beta + 1]: counts holds n_beta + 2.
  const int j = threadIdx.x;
  if (j < kTempSlots) {
    const unsigned long long s = red[j][0];
    if (j < n_beta) {
      if (s) atomicAdd(counts + j, s);
    } else if (j >= USSEG_TEMP_MAX_BETAS) {
      if (s) atomicAdd(counts + n_beta + (j - USSEG_TEMP_MAX_BETAS), s);
    }
  }
}

// probs -> out (may alias): the generic path, one pixel per lane and trip from pixel p_begin on; and for C == 3 with 16-byte aligned bases
// groups of four pixels = three float4 (ensemble_merge's layout).  A lane reads all of its pixels before it writes them, and no lane reads
// another's: in place is safe.  beta is read from the device on every launch and never compared with 1.
template <int NC>
__global__ __launch_bounds__(256) void apply_temperature_kernel(const float* probs, const float* __restrict__ beta_dev, float* out, int64_t M,
                                                                 int vec3) {
#pragma clang fp contract(off)
  const float beta = *beta_dev;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  int64_t p_tail = 0;
  if constexpr (NC == 3) {
    if (vec3) {
      const int64_t G = M >> 2;
      for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < G; g += stride) {      // SAFETY: g < M/4: floats 12g .. 12g+11 < 3M
        const float4* s4 = reinterpret_cast<const float4*>(probs) + g * 3;
        const float4 x = s4[0], y = s4[1], w = s4[2];
        const float v[12] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w, w.x, w.y, w.z, w.w};
        float o[12];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float pv[3] = {v[u * 3], v[u * 3 + 1], v[u * 3 + 2]};
          float ov[3];
          temper_pixel<3>(pv, beta, ov);
          o[u * 3] = ov[0]; o[u * 3 + 1] = ov[1]; o[u * 3 + 2] = ov[2];
        }
        float4* d4 = reinterpret_cast<float4*>(out) + g * 3;
        d4[0] = make_float4(o[0], o[1], o[2], o[3]);
        d4[1] = make_float4(o[4], o[5], o[6], o[7]);
        d4[2] = make_float4(o[8], o[9], o[10], o[11]);
      }
      p_tail = G * 4;
    }
  }
  for (int64_t p = p_tail + (int64_t)blockIdx.x * kThreads + threadIdx.x; p < M; p += stride) {   // SAFETY: p < M: floats NC*p .. NC*p+NC-1 < NC*M
    float pv[NC], ov[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) pv[c] = probs[p * NC + c];
    temper_pixel<NC>(pv, beta, ov);
#pragma unroll
    for (int c = 0; c < NC; ++c) out[p * NC + c] = ov[c];
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int usseg_score_sweep(const UssegSweepDesc* d, const float* probs, const float* y_true, int64_t* counts, usseg_stream_t stream) {
  USSEG_CHECK_ARG(d && probs && y_true && counts, "score_sweep: null pointer");
  USSEG_CHECK_ARG(d->B >= 0 && d->H >= 0 && d->W >= 1, "score_sweep: bad descriptor (B, H >= 0; W >= 1)");
  USSEG_CHECK_ARG(d->C >= 1 && d->C <= 4, "score_sweep: bad descriptor (1 <= C <= 4)");
  USSEG_CHECK_ARG(d->bins >= 2 && d->bins <= USSEG_SWEEP_MAX_BINS && (d->bins & (d->bins - 1)) == 0,
                  "score_sweep: bad descriptor (bins is a power of two, 2 <= bins <= %d)", USSEG_SWEEP_MAX_BINS);
  USSEG_CHECK_ARG(d->cls >= 0 && d->cls < d->C, "score_sweep: bad descriptor (cls is a class below C)");
  const int64_t BH = (int64_t)d->B * d->H;           // < 2^62
  USSEG_CHECK_ARG(BH <= ((int64_t)1 << 31) / d->W, "score_sweep: bad descriptor (B*H*W <= 2^31)");
  const int64_t M = BH * d->W;
  if (M == 0) return USSEG_OK;
  int64_t g = cdiv64(M, kThreads);
  if (g > kCountGrid) g = kCountGrid;
  constexpr bool kAgg = USSEG_SWEEP_AGGREGATE != 0;
  auto k = d->C == 1 ? score_sweep_kernel<1, kAgg> : d->C == 2 ? score_sweep_kernel<2, kAgg> : d->C == 3 ? score_sweep_kernel<3, kAgg>
                                                                                                        : score_sweep_kernel<4, kAgg>;
  hipLaunchKernelGGL(k, dim3((unsigned)g), dim3(kThreads), 0, (hipStream_t)stream, probs, y_true, M, (int)d->bins, (int)d->cls,
                     reinterpret_cast<unsigned long long*>(counts));
  return usseg_check_launch("score_sweep");
}

static int temp_desc_pixels(const UssegTempDesc* d, const char* what, int64_t* M) {
  USSEG_CHECK_ARG(d->B >= 0 && d->H >= 0 && d->W >= 1, "%s: bad descriptor (B, H >= 0; W >= 1)", what);
  USSEG_CHECK_ARG(d->C >= 1 && d->C <= 4, "%s: bad descriptor (1 <= C <= 4)", what);
  const int64_t BH = (int64_t)d->B * d->H;
  USSEG_CHECK_ARG(BH <= ((int64_t)1 << 31) / d->W, "%s: bad descriptor (B*H*W <= 2^31)", what);
  *M = BH * d->W;
  return USSEG_OK;
}

extern "C" int usseg_temperature_nll(const UssegTempDesc* d, const float* probs, const float* y_true, const float* betas, int64_t* counts,
                                     usseg_stream_t stream) {
  USSEG_CHECK_ARG(d && probs && y_true && betas && counts, "temperature_nll: null pointer");
  int64_t M = 0;
  if (int rc = temp_desc_pixels(d, "temperature_nll", &M)) return rc;
  USSEG_CHECK_ARG(d->n_beta >= 1 && d->n_beta <= USSEG_TEMP_MAX_BETAS, "temperature_nll: bad descriptor (1 <= n_beta <= %d)", USSEG_TEMP_MAX_BETAS);
  TemperatureBetas b = {};
  for (int j = 0; j < d->n_beta; ++j) {
    USSEG_CHECK_ARG(betas[j] > 0.f && betas[j] <= 16.f, "temperature_nll: beta %d must be finite with 0 < beta <= 16", j);    // (a NaN compares false)
    b.b[j] = betas[j];
  }
  if (M == 0) return USSEG_OK;
  int64_t g = cdiv64(M, kThreads);
  if (g > kCountGrid) g = kCountGrid;
  auto k = d->C == 1 ? temperature_nll_kernel<1> : d->C == 2 ? temperature_nll_kernel<2> : d->C == 3 ? temperature_nll_kernel<3> : temperature_nll_kernel<4>;
  hipLaunchKernelGGL(k, dim3((unsigned)g), dim3(kThreads), 0, (hipStream_t)stream, probs, y_true, M, (int)d->n_beta, b,
                     reinterpret_cast<unsigned long long*>(counts));
  return usseg_check_launch("temperature_nll");
}

extern "C" int usseg_apply_temperature(const UssegTempDesc* d, const float* probs, const float* beta_dev, float* out, usseg_stream_t stream) {
  USSEG_CHECK_ARG(d && probs && beta_dev && out, "apply_temperature: null pointer");
  int64_t M = 0;
  if (int rc = temp_desc_pixels(d, "apply_temperature", &M)) return rc;
  if (M == 0) return USSEG_OK;
  const int vec3 = d->C == 3 && aligned16(probs) && aligned16(out);
  const int64_t work = vec3 && M >= 4 ? M >> 2 : M;                  // (grid-stride loops: any grid covers the groups and the tail)
  int64_t g = cdiv64(work, kThreads);
  if (g > kApplyGrid) g = kApplyGrid;
  auto k = d->C == 1 ? apply_temperature_kernel<1> : d->C == 2 ? apply_temperature_kernel<2> : d->C == 3 ? apply_temperature_kernel<3> : apply_temperature_kernel<4>;
  hipLaunchKernelGGL(k, dim3((unsigned)g), dim3(kThreads), 0, (hipStream_t)stream, probs, beta_dev, out, M, vec3);
  return usseg_check_launch("apply_temperature");
}

#ifdef USSEG_SWEEP_TOOL_PROBE
// tools/time_sweep.py --probe: the logf and expf this file is compiled with, element by element, to measure their error against fp64.
__global__ __launch_bounds__(256) void tool_logf_expf_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ lg, float* __restrict__ ex) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    lg[i] = logf(x[i]);
    ex[i] = expf(x[i]);
  }
}
extern "C" int usseg_tool_logf_expf(const float* x, int64_t n, float* lg, float* ex, usseg_stream_t stream) {
  USSEG_CHECK_ARG(x && lg && ex && n >= 1, "tool_logf_expf: bad arguments");
  hipLaunchKernelGGL(tool_logf_expf_kernel, dim3(256), dim3(kThreads), 0, (hipStream_t)stream, x, n, lg, ex);
  return usseg_check_launch("tool_logf_expf");
}
#endif
