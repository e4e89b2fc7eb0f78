// Per-image scores in pixels and in physical units (usseg_scores.h: usseg_image_confusion, usseg_component_measure, usseg_bootstrap_sums).
// Every result is an integer sum, minimum or maximum, so it does not depend on the order of the threads: a second call gives the same bits.
//   sc_zero_kernel / sc_measure_init_kernel   write every output word first (the caller zeroes nothing).
//   sc_confusion_kernel   grid (blocks per image, N): a thread keeps the C*C + 1 cells of its pixels in registers (one compare per cell and
//                         pixel - no indexed register file, no LDS atomics that an all-background image would serialise on one word), the
//                         wave and then the workgroup reduce them, and one lane per non-zero cell sends ONE 64-bit atomic.
//   sc_measure_kernel     one thread per pixel, like cc_stats_kernel (components.hip): the lanes of a wave that fall into the same table row
//                         are reduced in registers, then one lane sends the row's eight 64-bit atomics.
//   sc_bootstrap_kernel   one wave per replicate: the lanes draw indices d = lane, lane + 64, ..., keep K sums in registers and a butterfly
//                         adds them.  No atomics, every out word written once.
// The atomics are vector 64-bit integer atomics at agent scope (the batch spans all XCDs); nothing allocates, nothing synchronises with the
// host, every launch goes to the one stream in order (a linear chain under graph capture).
#include "common.h"
#include "../../include/usseg_scores.h"

#define SC_MAX_DIM 8192
#define SC_RLX __ATOMIC_RELAXED
#define SC_AGENT __HIP_MEMORY_SCOPE_AGENT
#define SC_PIX_PER_THREAD 8

__global__ __launch_bounds__(256) void sc_zero_kernel(long long* __restrict__ a, int64_t na, long long* __restrict__ b, int64_t nb, long long* __restrict__ c,
                                                      int64_t nc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < na) a[i] = 0;
  if (b && i < nb) b[i] = 0;
  if (i < nc) c[i] = 0;
}

__device__ __forceinline__ unsigned long long sc_wave_sum_u64(unsigned long long v) {
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, off, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), off, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}
__device__ __forceinline__ int sc_wave_sum(int v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int sc_wave_min(int v) {
  for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ int sc_wave_max(int v) {
  for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
  return v;
}

// grid (bpi, N) x 256 threads; block b of image n takes the pixels b*256 + tid, + bpi*256, ... of that image.  A thread sees at most
// ceil(HW / 256) <= 2^18 pixels: its counts fit an int.  Cell CC (the last) counts the invalid pixels.
template <int C, bool WEIGHTED>
__global__ __launch_bounds__(256) void sc_confusion_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth,
                                                           const unsigned* __restrict__ weight, long long* cm, long long* wcm, long long* invalid, int HW) {
  constexpr int CC = C * C;
  __shared__ unsigned long long part[4][2 * CC + 1];
  const int n = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint8_t* p = pred + (int64_t)n * HW;
  const uint8_t* t = truth + (int64_t)n * HW;
  int cnt[CC + 1];
  unsigned long long ws[CC];
#pragma unroll
  for (int c = 0; c <= CC; ++c) cnt[c] = 0;
#pragma unroll
  for (int c = 0; c < CC; ++c) ws[c] = 0ull;
  const int stride = gridDim.x * 256;
  for (int i = blockIdx.x * 256 + tid; i < HW; i += stride) {
    const int a = t[i], b = p[i];
    const int cell = (a < C && b < C) ? a * C + b : CC;
    const unsigned long long w = WEIGHTED ? (unsigned long long)weight[i] : 0ull;
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      const bool hit = cell == c;
      cnt[c] += hit ? 1 : 0;
      if (WEIGHTED) ws[c] += hit ? w : 0ull;
    }
    cnt[CC] += cell == CC ? 1 : 0;
  }
#pragma unroll
  for (int c = 0; c <= CC; ++c) {
    const int s = sc_wave_sum(cnt[c]);
    if (lane == 0) part[wave][c] = (unsigned long long)s;
  }
  if (WEIGHTED) {
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      const unsigned long long s = sc_wave_sum_u64(ws[c]);
      if (lane == 0) part[wave][CC + 1 + c] = s;
    }
  }
  __syncthreads();
  const int cells = WEIGHTED ? 2 * CC + 1 : CC + 1;
  if (tid < cells) {
    const unsigned long long s = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
    if (s) {
      long long* dst = tid < CC ? cm + (int64_t)n * CC + tid : tid == CC ? invalid + n : wcm + (int64_t)n * CC + (tid - CC - 1);
      __hip_atomic_fetch_add(dst, (long long)s, SC_RLX, SC_AGENT);
    }
  }
}

__global__ __launch_bounds__(256) void sc_measure_init_kernel(long long* __restrict__ out, int64_t rows) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * USSEG_SCORES_MEASURE_FIELDS) return;
  const int f = (int)(i % USSEG_SCORES_MEASURE_FIELDS);
  out[i] = f < 4 ? 0ll : (f == 4 || f == 6) ? (long long)USSEG_SCORES_EMPTY_MIN : -1ll;      // the empty marker stays in rows nobody adds to
}

// One thread per pixel; at most 64 rounds, one per distinct table row in the wave.  64 values below 2^36 (w * q) sum to less than 2^42.
__global__ __launch_bounds__(256) void sc_measure_kernel(const int* __restrict__ labels, const unsigned* __restrict__ weight, const int* __restrict__ xq,
                                                         const int* __restrict__ yq, long long* out, int total, int HW, int cap) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int row = -1, x = 0, y = 0;
  unsigned long long w = 0ull;
  if (g < total) {
    const int k = labels[g];
    if (k >= 1 && k <= cap) {                                           // ids above the cap are skipped: nothing is written outside the table
      const int n = g / HW, i = g - n * HW;
      row = n * cap + (k - 1);                                          // < N*H*W <= 2^29
      w = weight[i];
      x = xq[i];
      y = yq[i];
    }
  }
  uint64_t todo = __ballot(row >= 0);
  for (int it = 0; it < 64 && todo; ++it) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const int lrow = __shfl(row, leader, 64);
    const bool mine = row == lrow;
    const uint64_t same = __ballot(mine) & todo;
    const unsigned long long sw = sc_wave_sum_u64(mine ? w : 0ull);
    const unsigned long long swx = sc_wave_sum_u64(mine ? w * (unsigned long long)(long long)x : 0ull);
    const unsigned long long swy = sc_wave_sum_u64(mine ? w * (unsigned long long)(long long)y : 0ull);
    const int x_min = sc_wave_min(mine ? x : 0x7fffffff), x_max = sc_wave_max(mine ? x : (int)0x80000000);
    const int y_min = sc_wave_min(mine ? y : 0x7fffffff), y_max = sc_wave_max(mine ? y : (int)0x80000000);
    if (lane == leader) {
      long long* s = out + (int64_t)lrow * USSEG_SCORES_MEASURE_FIELDS;
      __hip_atomic_fetch_add(s + 0, (long long)__popcll(same), SC_RLX, SC_AGENT);
      __hip_atomic_fetch_add(s + 1, (long long)sw, SC_RLX, SC_AGENT);
      __hip_atomic_fetch_add(s + 2, (long long)swx, SC_RLX, SC_AGENT);
      __hip_atomic_fetch_add(s + 3, (long long)swy, SC_RLX, SC_AGENT);
      __hip_atomic_fetch_min(s + 4, (long long)x_min, SC_RLX, SC_AGENT);
      __hip_atomic_fetch_max(s + 5, (long long)x_max, SC_RLX, SC_AGENT);
      __hip_atomic_fetch_min(s + 6, (long long)y_min, SC_RLX, SC_AGENT);
      __hip_atomic_fetch_max(s + 7, (long long)y_max, SC_RLX, SC_AGENT);
    }
    todo &= ~same;
  }
}

__device__ __forceinline__ unsigned sc_draw(unsigned long long seed, unsigned long long counter, unsigned U) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * counter;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (unsigned)(((z >> 32) * (unsigned long long)U) >> 32);         // < U
}

// grid ceil(R / 4) x 256 threads: wave = one replicate.  Sums are formed modulo 2^64 (unsigned): with |v| <= 2^62 / U they are the exact int64.
__global__ __launch_bounds__(256) void sc_bootstrap_kernel(const long long* __restrict__ rows, int U, int K, unsigned long long seed, int R,
                                                           long long* __restrict__ out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + wave;
  if (r >= R) return;                                                   // (whole waves leave: the shuffles below see all 64 lanes)
  unsigned long long acc[USSEG_SCORES_BOOT_MAX_K];
#pragma unroll
  for (int k = 0; k < USSEG_SCORES_BOOT_MAX_K; ++k) acc[k] = 0ull;
  const unsigned long long base = 1ull + (unsigned long long)r * (unsigned long long)U;
  for (int d = lane; d < U; d += 64) {
    const unsigned idx = sc_draw(seed, base + (unsigned long long)d, (unsigned)U);
    const long long* src = rows + (int64_t)idx * K;                     // idx < U: inside the table
#pragma unroll
    for (int k = 0; k < USSEG_SCORES_BOOT_MAX_K; ++k)
      if (k < K) acc[k] += (unsigned long long)src[k];
  }
#pragma unroll
  for (int k = 0; k < USSEG_SCORES_BOOT_MAX_K; ++k) {
    if (k < K) {                                                        // K is uniform: no lane skips a shuffle another lane takes
      const unsigned long long s = sc_wave_sum_u64(acc[k]);
      if (lane == 0) out[(int64_t)r * K + k] = (long long)s;
    }
  }
}

// ---- entry points: every argument is checked before any launch ------------------------------------------------------------------------
#define SC_CHECK_SHAPE(what)                                                                                                              \
  USSEG_CHECK_ARG(H >= 1 && H <= SC_MAX_DIM && W >= 1 && W <= SC_MAX_DIM, what ": H and W must lie in [1, %d], got %d x %d", SC_MAX_DIM, H, W); \
  USSEG_CHECK_ARG(N >= 0 && N <= 65535, what ": 0 <= N <= 65535");                                                                        \
  USSEG_CHECK_ARG((int64_t)N * H * W <= (1 << 29), what ": more than 2^29 pixels")

template <int C>
static void sc_launch_confusion(dim3 grid, hipStream_t s, const uint8_t* pred, const uint8_t* truth, const uint32_t* weight, long long* cm, long long* wcm,
                                long long* invalid, int HW) {
  if (weight)
    hipLaunchKernelGGL((sc_confusion_kernel<C, true>), grid, dim3(256), 0, s, pred, truth, (const unsigned*)weight, cm, wcm, invalid, HW);
  else
    hipLaunchKernelGGL((sc_confusion_kernel<C, false>), grid, dim3(256), 0, s, pred, truth, (const unsigned*)nullptr, cm, (long long*)nullptr, invalid, HW);
}

extern "C" int usseg_image_confusion(const uint8_t* pred, const uint8_t* truth, const uint32_t* weight, int32_t N, int32_t H, int32_t W, int32_t C,
                                     int64_t* cm, int64_t* wcm, int64_t* invalid, usseg_stream_t stream) {
  SC_CHECK_SHAPE("image_confusion");
  USSEG_CHECK_ARG(C >= 2 && C <= 4, "image_confusion: C must lie in [2, 4], got %d", C);
  USSEG_CHECK_ARG(pred && truth && cm && invalid, "image_confusion: null pointer");
  USSEG_CHECK_ARG((weight != nullptr) == (wcm != nullptr), "image_confusion: wcm goes with weight: both or neither, got %s without %s",
                  weight ? "weight" : "wcm", weight ? "wcm" : "weight");
  USSEG_CHECK_ARG(((uintptr_t)weight & 3) == 0 && ((uintptr_t)cm & 7) == 0 && ((uintptr_t)wcm & 7) == 0 && ((uintptr_t)invalid & 7) == 0,
                  "image_confusion: weight must be 4-byte, cm, wcm and invalid 8-byte aligned");
  if (N == 0) return USSEG_OK;
  const int HW = H * W;                                                  // <= 2^26
  const int64_t cells = (int64_t)N * C * C;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sc_zero_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, (long long*)cm, cells, (long long*)wcm, cells, (long long*)invalid,
                     (int64_t)N);
  int bpi = (HW + 256 * SC_PIX_PER_THREAD - 1) / (256 * SC_PIX_PER_THREAD);
  if (bpi > 1024) bpi = 1024;
  const dim3 grid(bpi, N);
  if (C == 2)
    sc_launch_confusion<2>(grid, s, pred, truth, weight, (long long*)cm, (long long*)wcm, (long long*)invalid, HW);
  else if (C == 3)
    sc_launch_confusion<3>(grid, s, pred, truth, weight, (long long*)cm, (long long*)wcm, (long long*)invalid, HW);
  else
    sc_launch_confusion<4>(grid, s, pred, truth, weight, (long long*)cm, (long long*)wcm, (long long*)invalid, HW);
  return usseg_check_launch("image_confusion");
}

extern "C" int usseg_component_measure(const int32_t* labels, const uint32_t* weight, const int32_t* xq, const int32_t* yq, int32_t N, int32_t H,
                                       int32_t W, int32_t cap, int64_t* out, usseg_stream_t stream) {
  SC_CHECK_SHAPE("component_measure");
  USSEG_CHECK_ARG(cap >= 0 && cap <= H * W, "component_measure: the cap must lie in [0, H*W], got %d", cap);
  USSEG_CHECK_ARG(labels && weight && xq && yq && (out || cap == 0), "component_measure: null pointer");
  USSEG_CHECK_ARG(((uintptr_t)labels & 3) == 0 && ((uintptr_t)weight & 3) == 0 && ((uintptr_t)xq & 3) == 0 && ((uintptr_t)yq & 3) == 0 &&
                      ((uintptr_t)out & 7) == 0,
                  "component_measure: labels, weight, xq and yq must be 4-byte, out 8-byte aligned");
  if (N == 0 || cap == 0) return USSEG_OK;
  const int total = N * H * W;
  const int64_t rows = (int64_t)N * cap;                                 // <= 2^29
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sc_measure_init_kernel, dim3((unsigned)((rows * USSEG_SCORES_MEASURE_FIELDS + 255) / 256)), dim3(256), 0, s, (long long*)out, rows);
  hipLaunchKernelGGL(sc_measure_kernel, dim3((total + 255) / 256), dim3(256), 0, s, labels, (const unsigned*)weight, xq, yq, (long long*)out, total, H * W,
                     cap);
  return usseg_check_launch("component_measure");
}

extern "C" int usseg_bootstrap_sums(const int64_t* rows, int32_t U, int32_t K, uint64_t seed, int32_t R, int64_t* out, usseg_stream_t stream) {
  USSEG_CHECK_ARG(K >= 1 && K <= USSEG_SCORES_BOOT_MAX_K, "bootstrap_sums: K must lie in [1, %d], got %d", USSEG_SCORES_BOOT_MAX_K, K);
  USSEG_CHECK_ARG(R >= 0 && R <= USSEG_SCORES_BOOT_MAX, "bootstrap_sums: R must lie in [0, 2^20], got %d", R);
  USSEG_CHECK_ARG(U >= 0 && U <= USSEG_SCORES_BOOT_MAX, "bootstrap_sums: U must lie in [0, 2^20], got %d", U);
  USSEG_CHECK_ARG(U >= 1 || R == 0, "bootstrap_sums: %d replicates of an empty table (U = 0)", R);
  USSEG_CHECK_ARG((rows || U == 0) && (out || R == 0), "bootstrap_sums: null pointer");
  USSEG_CHECK_ARG(((uintptr_t)rows & 7) == 0 && ((uintptr_t)out & 7) == 0, "bootstrap_sums: rows and out must be 8-byte aligned");
  if (R == 0 || U == 0) return USSEG_OK;
  hipLaunchKernelGGL(sc_bootstrap_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const long long*)rows, U, K,
                     (unsigned long long)seed, R, (long long*)out);
  return usseg_check_launch("bootstrap_sums");
}
