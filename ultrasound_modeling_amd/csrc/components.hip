// Connected-component labelling on the device (usseg.h: usseg_label_components, usseg_component_stats, usseg_clean_mask,
// usseg_component_overlap): integer work, data-dependent access, and no arithmetic but atomic min / add / max.
// A plane is a [H][W] binary image (mask != 0 = inside); components are 4- or 8-connected and never cross an image of the batch.
// Union-find on a parent array P of GLOBAL linear indices g = (n*H + y)*W + x (int32: N*H*W <= 2^29), -1 outside the mask.  Invariants, held
// at every instant of every kernel: P[g] <= g, and P[g] is a pixel of g's own component - so any value ever stored in a word, a stale one
// included, leads DOWN to a smaller index of the same component, and the root of a finished component is its smallest linear index.
//   cc_init_kernel     one wave per image row, 64 pixels per ballot: P[g] = the start of g's horizontal run INSIDE its 64-pixel word (clz of
//                      the zero bits below the lane), so the only unions left are across word borders and between rows.
//   cc_merge_kernel    one union per adjacency that is not implied by the others: left across a word border; up unless left and up-left are
//                      both set; (8) up-left if neither up nor left is set; (8) up-right if up is not set.  cc_union links the LARGER root
//                      under the smaller with an agent-scope atomicMin (the batch spans all XCDs).  No workgroup waits for another: every
//                      iteration of the union loop lowers a + b by at least one (see cc_union), whatever the other threads do.
//   cc_flatten_kernel  P[g] = root(g) for every pixel, and the number of roots of each row (ballot + popcount, no atomics).
//   cc_scan_kernel     one workgroup per image: exclusive scan of the at most 8192 row counts, K_n = their sum.
//   cc_assign_kernel   a root's id = 1 + roots before it in raster order (row base + popcount of the lower lanes), stored at ids[root].
//   cc_relabel_kernel  labels[g] = ids[P[g]] (0 outside).  `labels` itself is P up to here.
// usseg_clean_mask runs init / merge / flatten on a parent array in the workspace, adds every pixel into ITS ROOT's area and peak words
// (wave-aggregated atomicAdd and atomicMax of the non-negative fp32 bit pattern - integer order = float order), and writes the decision per
// pixel: no table, no cap.  The statistics and overlap tables are integer sums, minima and maxima: independent of the order of the atomics.
// Nothing allocates, nothing synchronises with the host, every launch goes to the one stream in order (a linear chain under graph capture).
#include "common.h"
#include <cmath>

#define CC_MAX_DIM 8192
#define CC_RLX __ATOMIC_RELAXED
#define CC_AGENT __HIP_MEMORY_SCOPE_AGENT

// the root above x.  Terminates: P[x] < x at every step that does not stop (the invariant), so at most `bound` = H*W steps inside one image.
// The loads are agent-scope (served by L2, not a CU's L1); a stale value is an EARLIER value of the same word and still a valid ancestor.
__device__ __forceinline__ int cc_find(const int* P, int x, int bound) {
  for (int it = 0; it < bound; ++it) {
    const int p = __hip_atomic_load(P + x, CC_RLX, CC_AGENT);
    if (p == x || p < 0) break;                       // (p < 0 cannot occur on a mask pixel; it keeps a wrong caller inside the array)
    x = p;
  }
  return x;
}

// Makes a and b one tree.  Lock-free, and no thread waits for another: each iteration either ends the loop or replaces the larger of (a, b) by
// a STRICTLY smaller index (old < a when a was no longer a root; cc_find only goes down), so a + b falls by at least one per iteration and the
// loop ends after at most 2*H*W iterations - the bound written in the for statement - whether or not other threads run.  A failed atomicMin
// (old != a) has still stored min(old, b) in P[a]: a stays below its component, and the loop goes on to join old and b.
__device__ __forceinline__ void cc_union(int* P, int a, int b, int bound) {
  a = cc_find(P, a, bound);
  b = cc_find(P, b, bound);
  for (int it = 0; it < 2 * bound; ++it) {
    if (a == b) break;
    if (a < b) { const int t = a; a = b; b = t; }     // a > b: the larger index goes under the smaller
    const int old = __hip_atomic_fetch_min(P + a, b, CC_RLX, CC_AGENT);
    if (old == a) break;                              // a was a root and now points at b
    a = cc_find(P, old, bound);                       // old < a
  }
}

// grid ceil(rows / 4) x 256 threads: wave = one row of one image.  zero0 / zero1 (may be null): per-pixel accumulators cleared on the way.
__global__ __launch_bounds__(256) void cc_init_kernel(const uint8_t* __restrict__ mask, int* __restrict__ P, int* __restrict__ zero0,
                                                      unsigned* __restrict__ zero1, int rows, int W) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const int nw = (W + 63) >> 6;
  const int base = row * W;                           // rows * W <= 2^29
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    const bool in = x < W && mask[base + x] != 0;
    const uint64_t bal = __ballot(in);
    if (x >= W) continue;
    int p = -1;
    if (in) {
      const uint64_t lower = (1ull << lane) - 1ull;
      const uint64_t zeros = ~bal & lower;            // clear bits below this lane: the run starts just above the highest of them
      p = base + w * 64 + (zeros ? 64 - __clzll((long long)zeros) : 0);
    }
    P[base + x] = p;
    if (zero0) zero0[base + x] = 0;
    if (zero1) zero1[base + x] = 0u;
  }
}

template <bool CONN8>
__global__ __launch_bounds__(256) void cc_merge_kernel(const uint8_t* __restrict__ mask, int* P, int rows, int H, int W) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const int nw = (W + 63) >> 6;
  const int y = row % H;
  const int base = row * W, bound = H * W;
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    if (x >= W) break;
    const int g = base + x;
    if (!mask[g]) continue;
    const bool L = x > 0 && mask[g - 1];
    const bool U = y > 0 && mask[g - W];
    const bool UL = y > 0 && x > 0 && mask[g - W - 1];
    if (lane == 0 && L) cc_union(P, g, g - 1, bound);                 // inside a word the run is already one tree
    if (U && !(L && UL)) cc_union(P, g, g - W, bound);                // L & UL: the left pixel joins this row's run to the run above
    if (CONN8) {
      const bool UR = y > 0 && x + 1 < W && mask[g - W + 1];
      if (UL && !U && !L) cc_union(P, g, g - W - 1, bound);           // U: up-left is in up's run; L: up-left is the left pixel's up
      if (UR && !U) cc_union(P, g, g - W + 1, bound);                 // U: up-right is in up's run
    }
  }
}

// rowcnt (may be null): the number of roots in each row
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* P, int* __restrict__ rowcnt, int rows, int H, int W) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const int nw = (W + 63) >> 6;
  const int base = row * W, bound = H * W;
  int roots = 0;
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    bool is_root = false;
    if (x < W) {
      const int g = base + x;
      const int p = __hip_atomic_load(P + g, CC_RLX, CC_AGENT);
      if (p >= 0) {
        const int r = cc_find(P, p, bound);
        if (r != p) __hip_atomic_store(P + g, r, CC_RLX, CC_AGENT);    // (a root is never rewritten: P[r] == r throughout this kernel)
        is_root = r == g;
      }
    }
    roots += __popcll(__ballot(is_root));
  }
  if (rowcnt && lane == 0) rowcnt[row] = roots;
}

// grid N x 256 threads: rowcnt [N][H] -> exclusive prefix in place, count[n] = the total.  A thread owns ceil(H/256) <= 32 consecutive rows.
__global__ __launch_bounds__(256) void cc_scan_kernel(int* __restrict__ rowcnt, int* __restrict__ count, int H) {
  __shared__ int part[256];
  const int n = blockIdx.x, tid = threadIdx.x;
  int* rc = rowcnt + (int64_t)n * H;
  const int per = (H + 255) / 256;
  const int lo = tid * per, hi = lo + per < H ? lo + per : H;
  int s = 0;
  for (int r = lo; r < hi; ++r) s += rc[r];
  part[tid] = s;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {                                   // inclusive scan of the 256 partial sums, 8 steps
    const int v = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - s;
  for (int r = lo; r < hi; ++r) { const int c = rc[r]; rc[r] = run; run += c; }
  if (tid == 255) count[n] = part[255];
}

__global__ __launch_bounds__(256) void cc_assign_kernel(const int* __restrict__ P, const int* __restrict__ rowbase, int* __restrict__ ids, int rows, int W) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const int nw = (W + 63) >> 6;
  const int base = row * W;
  int before = rowbase[row];
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    const bool is_root = x < W && P[base + x] == base + x;
    const uint64_t bal = __ballot(is_root);
    if (is_root) ids[base + x] = before + __popcll(bal & ((1ull << lane) - 1ull)) + 1;
    before += __popcll(bal);
  }
}

__global__ __launch_bounds__(256) void cc_relabel_kernel(int* __restrict__ labels, const int* __restrict__ ids, int total) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int r = labels[g];
  labels[g] = r < 0 ? 0 : ids[r];
}

// the bit pattern of a probability as an unsigned integer whose order is the float order: NaN, zero and negative values give 0
__device__ __forceinline__ unsigned cc_peak_bits(float p) { return p > 0.f ? __float_as_uint(p) : 0u; }

// clean_mask: every mask pixel adds 1 to area[root] and raises peak[root].  The lanes of a wave that share a root add ONCE and raise ONCE: at
// most 64 rounds, one per distinct root in the wave, each with a 6-step butterfly maximum over the lanes of that root (a large component
// would otherwise send every pixel's atomic to one word).  The maximum is skipped when the word already holds as much (a stale read is an
// earlier, smaller value).
__global__ __launch_bounds__(256) void cc_accumulate_kernel(const int* __restrict__ P, const float* __restrict__ prob, int* area, unsigned* peak, int total) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int r = g < total ? P[g] : -1;
  const unsigned b = (prob && r >= 0) ? cc_peak_bits(prob[g]) : 0u;
  uint64_t todo = __ballot(r >= 0);
  for (int it = 0; it < 64 && todo; ++it) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const int lr = __shfl(r, leader, 64);
    const uint64_t same = __ballot(r == lr) & todo;
    unsigned m = r == lr ? b : 0u;
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned o = (unsigned)__shfl_xor((int)m, off, 64);
      m = o > m ? o : m;
    }
    if (lane == leader) {
      __hip_atomic_fetch_add(area + lr, (int)__popcll(same), CC_RLX, CC_AGENT);
      if (m > __hip_atomic_load(peak + lr, CC_RLX, CC_AGENT)) __hip_atomic_fetch_max(peak + lr, m, CC_RLX, CC_AGENT);
    }
    todo &= ~same;
  }
}

__global__ __launch_bounds__(256) void cc_decide_kernel(const int* __restrict__ P, const int* __restrict__ area, const unsigned* __restrict__ peak,
                                                        int min_area, unsigned min_peak_bits, int use_peak, uint8_t* out, int total) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int r = P[g];
  bool keep = false;
  if (r >= 0) keep = area[r] >= min_area && (!use_peak || peak[r] >= min_peak_bits);
  out[g] = keep ? 1 : 0;
}

__global__ __launch_bounds__(256) void cc_binarise_kernel(const uint8_t* mask, uint8_t* out, int total) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g < total) out[g] = mask[g] ? 1 : 0;
}

// ---- tables -----------------------------------------------------------------------------------------------------------------------------
#define CC_STAT_FIELDS 8
__global__ __launch_bounds__(256) void cc_stats_init_kernel(long long* __restrict__ stats, int64_t rows) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * CC_STAT_FIELDS) return;
  const int f = (int)(i % CC_STAT_FIELDS);
  stats[i] = (f == 1 || f == 2) ? 0x7fffffffffffffffll : 0ll;           // y_min, x_min start high; the last pass zeroes them in empty rows
}

// butterfly reductions over the 64 lanes; a lane outside the group passes the neutral value
__device__ __forceinline__ int cc_wave_min(int v) {
  for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ int cc_wave_max(int v) {
  for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ int cc_wave_sum(int v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// One thread per pixel.  The lanes of a wave that fall into the same table row are reduced in registers first (at most 64 rounds, one per
// distinct row in the wave; 64 coordinates below 8192 sum to less than 2^19), then ONE lane sends the eight atomics of the row.
__global__ __launch_bounds__(256) void cc_stats_kernel(const int* __restrict__ labels, const float* __restrict__ prob, long long* stats, int total, int H,
                                                       int W, int cap) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int row = -1, y = 0, x = 0;
  unsigned b = 0u;
  if (g < total) {
    const int k = labels[g];
    if (k >= 1 && k <= cap) {                                           // ids above the cap are skipped: nothing is written outside the table
      const int HW = H * W;
      const int n = g / HW, i = g - n * HW;
      y = i / W;
      x = i - y * W;
      row = n * cap + (k - 1);                                          // < N*cap <= 2^29
      if (prob) b = cc_peak_bits(prob[g]);
    }
  }
  uint64_t todo = __ballot(row >= 0);
  for (int it = 0; it < 64 && todo; ++it) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const int lrow = __shfl(row, leader, 64);
    const bool mine = row == lrow;
    const uint64_t same = __ballot(mine) & todo;
    const int y_min = cc_wave_min(mine ? y : 0x7fffffff), x_min = cc_wave_min(mine ? x : 0x7fffffff);
    const int y_max = cc_wave_max(mine ? y : -1), x_max = cc_wave_max(mine ? x : -1);
    const int y_sum = cc_wave_sum(mine ? y : 0), x_sum = cc_wave_sum(mine ? x : 0);
    const int peak = cc_wave_max(mine ? (int)b : 0);                    // (the bits of a value in [0, 1] are a non-negative int)
    if (lane == leader) {
      long long* s = stats + (int64_t)lrow * CC_STAT_FIELDS;
      __hip_atomic_fetch_add(s + 0, (long long)__popcll(same), CC_RLX, CC_AGENT);
      __hip_atomic_fetch_min(s + 1, (long long)y_min, CC_RLX, CC_AGENT);
      __hip_atomic_fetch_min(s + 2, (long long)x_min, CC_RLX, CC_AGENT);
      __hip_atomic_fetch_max(s + 3, (long long)y_max, CC_RLX, CC_AGENT);
      __hip_atomic_fetch_max(s + 4, (long long)x_max, CC_RLX, CC_AGENT);
      __hip_atomic_fetch_add(s + 5, (long long)y_sum, CC_RLX, CC_AGENT);
      __hip_atomic_fetch_add(s + 6, (long long)x_sum, CC_RLX, CC_AGENT);
      if (peak > 0) __hip_atomic_fetch_max(s + 7, (long long)peak, CC_RLX, CC_AGENT);
    }
    todo &= ~same;
  }
}

__global__ __launch_bounds__(256) void cc_stats_final_kernel(long long* __restrict__ stats, int64_t rows) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  long long* s = stats + r * CC_STAT_FIELDS;
  if (s[0] == 0) { s[1] = 0; s[2] = 0; }
}

__global__ __launch_bounds__(256) void cc_zero_i32_kernel(int* __restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0;
}

__global__ __launch_bounds__(256) void cc_overlap_kernel(const int* __restrict__ la, const int* __restrict__ lb, int* hit_a, int* hit_b, int total, int HW,
                                                         int cap_a, int cap_b) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int a = la[g], b = lb[g];
  if (a < 1 || b < 1) return;
  const int n = g / HW;
  if (a <= cap_a) __hip_atomic_fetch_add(hit_a + (int64_t)n * cap_a + (a - 1), 1, CC_RLX, CC_AGENT);
  if (b <= cap_b) __hip_atomic_fetch_add(hit_b + (int64_t)n * cap_b + (b - 1), 1, CC_RLX, CC_AGENT);
}

// ---- entry points: every argument is checked before any launch ------------------------------------------------------------------------
static inline int64_t cc_round16(int64_t v) { return (v + 15) / 16 * 16; }

static inline bool cc_shape_ok(int32_t N, int32_t H, int32_t W) {
  return N >= 0 && N <= 65535 && H >= 1 && W >= 1 && H <= CC_MAX_DIM && W <= CC_MAX_DIM && (int64_t)N * H * W <= (1 << 29);
}

extern "C" int64_t usseg_components_ws_bytes(int32_t N, int32_t H, int32_t W) {
  if (!cc_shape_ok(N, H, W)) return -1;
  return 3 * cc_round16((int64_t)4 * N * H * W) + cc_round16((int64_t)4 * N * H);
}

#define CC_CHECK_SHAPE(what)                                                                                                              \
  USSEG_CHECK_ARG(H >= 1 && H <= CC_MAX_DIM && W >= 1 && W <= CC_MAX_DIM, what ": H and W must lie in [1, %d], got %d x %d", CC_MAX_DIM, H, W); \
  USSEG_CHECK_ARG(N >= 0 && N <= 65535, what ": 0 <= N <= 65535");                                                                        \
  USSEG_CHECK_ARG((int64_t)N * H * W <= (1 << 29), what ": more than 2^29 pixels")

static void cc_launch_trees(const uint8_t* mask, int* P, int* zero0, unsigned* zero1, int* rowcnt, int N, int H, int W, int connectivity, hipStream_t s) {
  const int rows = N * H;
  const dim3 grid((rows + 3) / 4), block(256);
  hipLaunchKernelGGL(cc_init_kernel, grid, block, 0, s, mask, P, zero0, zero1, rows, W);
  if (connectivity == 8)
    hipLaunchKernelGGL((cc_merge_kernel<true>), grid, block, 0, s, mask, P, rows, H, W);
  else
    hipLaunchKernelGGL((cc_merge_kernel<false>), grid, block, 0, s, mask, P, rows, H, W);
  hipLaunchKernelGGL(cc_flatten_kernel, grid, block, 0, s, P, rowcnt, rows, H, W);
}

extern "C" int usseg_label_components(const uint8_t* mask, int32_t N, int32_t H, int32_t W, int32_t connectivity, int32_t* labels, int32_t* count, void* ws,
                                      int64_t ws_bytes, usseg_stream_t stream) {
  CC_CHECK_SHAPE("label_components");
  USSEG_CHECK_ARG(connectivity == 4 || connectivity == 8, "label_components: connectivity must be 4 or 8, got %d", connectivity);
  USSEG_CHECK_ARG(mask && labels && count && ws, "label_components: null pointer");
  USSEG_CHECK_ARG(((uintptr_t)labels & 3) == 0 && ((uintptr_t)count & 3) == 0 && ((uintptr_t)ws & 15) == 0,
                  "label_components: labels and count must be 4-byte, the workspace 16-byte aligned");
  USSEG_CHECK_ARG(ws_bytes >= usseg_components_ws_bytes(N, H, W), "label_components: the workspace holds %lld bytes, %lld needed", (long long)ws_bytes,
                  (long long)usseg_components_ws_bytes(N, H, W));
  if (N == 0) return USSEG_OK;
  const int total = N * H * W, rows = N * H;
  int* ids = (int*)ws;
  int* rowcnt = (int*)((char*)ws + 3 * cc_round16((int64_t)4 * total));
  hipStream_t s = (hipStream_t)stream;
  cc_launch_trees(mask, labels, nullptr, nullptr, rowcnt, N, H, W, connectivity, s);
  hipLaunchKernelGGL(cc_scan_kernel, dim3(N), dim3(256), 0, s, rowcnt, count, H);
  hipLaunchKernelGGL(cc_assign_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, (const int*)labels, (const int*)rowcnt, ids, rows, W);
  hipLaunchKernelGGL(cc_relabel_kernel, dim3((total + 255) / 256), dim3(256), 0, s, labels, (const int*)ids, total);
  return usseg_check_launch("label_components");
}

extern "C" int usseg_component_stats(const int32_t* labels, const float* prob, int32_t N, int32_t H, int32_t W, int32_t cap, int64_t* stats,
                                     usseg_stream_t stream) {
  CC_CHECK_SHAPE("component_stats");
  USSEG_CHECK_ARG(cap >= 0 && cap <= H * W, "component_stats: the cap must lie in [0, H*W], got %d", cap);
  USSEG_CHECK_ARG(labels && (stats || cap == 0), "component_stats: null pointer");
  USSEG_CHECK_ARG(((uintptr_t)labels & 3) == 0 && ((uintptr_t)prob & 3) == 0 && ((uintptr_t)stats & 7) == 0,
                  "component_stats: labels and prob must be 4-byte, stats 8-byte aligned");
  if (N == 0 || cap == 0) return USSEG_OK;
  const int total = N * H * W;
  const int64_t rows = (int64_t)N * cap;                                 // <= 2^29
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_stats_init_kernel, dim3((unsigned)((rows * CC_STAT_FIELDS + 255) / 256)), dim3(256), 0, s, (long long*)stats, rows);
  hipLaunchKernelGGL(cc_stats_kernel, dim3((total + 255) / 256), dim3(256), 0, s, labels, prob, (long long*)stats, total, H, W, cap);
  hipLaunchKernelGGL(cc_stats_final_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, (long long*)stats, rows);
  return usseg_check_launch("component_stats");
}

extern "C" int usseg_clean_mask(const uint8_t* mask, const float* prob, int32_t N, int32_t H, int32_t W, int32_t connectivity, int32_t min_area,
                                float min_peak, uint8_t* out, void* ws, int64_t ws_bytes, usseg_stream_t stream) {
  CC_CHECK_SHAPE("clean_mask");
  USSEG_CHECK_ARG(connectivity == 4 || connectivity == 8, "clean_mask: connectivity must be 4 or 8, got %d", connectivity);
  USSEG_CHECK_ARG(!std::isnan(min_peak), "clean_mask: min_peak is NaN");
  USSEG_CHECK_ARG(mask && out && ws, "clean_mask: null pointer");
  USSEG_CHECK_ARG(((uintptr_t)prob & 3) == 0 && ((uintptr_t)ws & 15) == 0, "clean_mask: prob must be 4-byte, the workspace 16-byte aligned");
  USSEG_CHECK_ARG(ws_bytes >= usseg_components_ws_bytes(N, H, W), "clean_mask: the workspace holds %lld bytes, %lld needed", (long long)ws_bytes,
                  (long long)usseg_components_ws_bytes(N, H, W));
  if (N == 0) return USSEG_OK;
  const int total = N * H * W;
  hipStream_t s = (hipStream_t)stream;
  const bool use_peak = prob != nullptr && min_peak > 0.f;
  if (min_area <= 1 && !use_peak) {
    hipLaunchKernelGGL(cc_binarise_kernel, dim3((total + 255) / 256), dim3(256), 0, s, mask, out, total);
    return usseg_check_launch("clean_mask");
  }
  const int64_t region = cc_round16((int64_t)4 * total);
  int* P = (int*)ws;
  int* area = (int*)((char*)ws + region);
  unsigned* peak = (unsigned*)((char*)ws + 2 * region);
  unsigned min_bits;                                                     // min_peak > 0 here when it is used: its bit pattern orders as the float
  { const float mp = use_peak ? min_peak : 0.f; __builtin_memcpy(&min_bits, &mp, 4); }
  cc_launch_trees(mask, P, area, peak, nullptr, N, H, W, connectivity, s);
  hipLaunchKernelGGL(cc_accumulate_kernel, dim3((total + 255) / 256), dim3(256), 0, s, (const int*)P, use_peak ? prob : (const float*)nullptr, area, peak,
                     total);
  hipLaunchKernelGGL(cc_decide_kernel, dim3((total + 255) / 256), dim3(256), 0, s, (const int*)P, (const int*)area, (const unsigned*)peak, min_area, min_bits,
                     use_peak ? 1 : 0, out, total);
  return usseg_check_launch("clean_mask");
}

extern "C" int usseg_component_overlap(const int32_t* labels_a, const int32_t* labels_b, int32_t N, int32_t H, int32_t W, int32_t cap_a, int32_t cap_b,
                                       int32_t* hit_a, int32_t* hit_b, usseg_stream_t stream) {
  CC_CHECK_SHAPE("component_overlap");
  USSEG_CHECK_ARG(cap_a >= 0 && cap_a <= H * W && cap_b >= 0 && cap_b <= H * W, "component_overlap: the caps must lie in [0, H*W], got %d and %d", cap_a,
                  cap_b);
  USSEG_CHECK_ARG(labels_a && labels_b && (hit_a || cap_a == 0) && (hit_b || cap_b == 0), "component_overlap: null pointer");
  USSEG_CHECK_ARG(((uintptr_t)labels_a & 3) == 0 && ((uintptr_t)labels_b & 3) == 0 && ((uintptr_t)hit_a & 3) == 0 && ((uintptr_t)hit_b & 3) == 0,
                  "component_overlap: labels and hit tables must be 4-byte aligned");
  if (N == 0 || (cap_a == 0 && cap_b == 0)) return USSEG_OK;
  const int total = N * H * W;
  hipStream_t s = (hipStream_t)stream;
  const int64_t na = (int64_t)N * cap_a, nb = (int64_t)N * cap_b;
  if (na) hipLaunchKernelGGL(cc_zero_i32_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, s, hit_a, na);
  if (nb) hipLaunchKernelGGL(cc_zero_i32_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, hit_b, nb);
  hipLaunchKernelGGL(cc_overlap_kernel, dim3((total + 255) / 256), dim3(256), 0, s, labels_a, labels_b, hit_a, hit_b, total, H * W, cap_a, cap_b);
  return usseg_check_launch("component_overlap");
}
