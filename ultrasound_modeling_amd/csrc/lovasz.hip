// A stable segmented LSD radix sort of (key, value) uint32 pairs, and the Lovasz-softmax loss (Berman, Triki, Blaschko, CVPR 2018) built on
// it: usseg.h, usseg_sort_pairs_u32 and UssegLovaszLoss.
//
// Sort.  8-bit digits, tiles of SORT_TILE = 2048 pairs (256 threads x 8), segments in grid.y.  One digit pass is three launches:
//   sort_hist_kernel     hist[seg][tile][digit] = the tile's digit counts (LDS integer atomics; integer sums have one value in any order);
//   sort_offsets_kernel  one workgroup per segment: the exclusive scan of the table in (digit, tile) order, in place - four threads per digit;
//   sort_scatter_kernel  a tile's pairs go to offset[tile][digit] + their rank among the tile's pairs of that digit IN INDEX ORDER.  A wave
//                        owns 512 consecutive pairs and ranks them 64 at a time: the lanes holding one digit find each other with one
//                        __ballot per digit bit, the rank inside the group is a popcount below the lane, and the wave's running count of
//                        the digit lives in LDS.  The four waves' counts are then chained in wave order, the tile is put in sorted order
//                        in LDS and leaves from there, so a digit's run is written by neighbouring threads.
// The number of launches depends on (S, n, key_bits) alone - 3 * ceil(key_bits / 8) - and a pass boundary is a launch boundary: no
// workgroup waits for another, nothing allocates, nothing synchronises with the host.
//
// Loss.  Per class the pixels are ordered by error, descending, ties by pixel index; the Lovasz gradient of the Jaccard loss at rank r is a
// closed form in exact integers (usseg.h), so the launches are: keys and payloads (1), the sort (12 at 30 key bits), foreground counts per
// tile of the sorted order (1), their exclusive scan and Y_c (1), the coefficients scattered back to pixel order (1).  The sums pass and the
// backward pass restate overlap_loss.hip's two kernels (its ordered, ticketed grid reduction under the same grid rule; its CCE arithmetic;
// its dlogits layouts) rather than sharing them through a header: that file's kernels stay instruction for instruction what they were.
#include "common.h"
#include <cmath>

#define SORT_TILE USSEG_SORT_TILE
#define SORT_RADIX (1 << USSEG_SORT_DIGIT_BITS)
static_assert(SORT_TILE == 2048 && SORT_RADIX == 256, "the kernels below are written for 256 threads x 8 pairs and one digit per thread");

static inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }
static inline int64_t sort_tiles(int64_t n) { return cdiv64(n, SORT_TILE); }

__device__ __forceinline__ unsigned sort_digit(unsigned key, int shift, unsigned mask) { return (key >> shift) & mask; }

__global__ __launch_bounds__(256) void sort_hist_kernel(const unsigned* __restrict__ keys, unsigned* __restrict__ hist, int n, int ntiles, int shift,
                                                         unsigned mask) {
  __shared__ unsigned h[SORT_RADIX];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t seg = blockIdx.y;
  const int t0 = blockIdx.x * SORT_TILE;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int i = t0 + r * 256 + threadIdx.x;
    if (i < n) atomicAdd(&h[sort_digit(keys[seg * n + i], shift, mask)], 1u);
  }
  __syncthreads();
  hist[(seg * ntiles + blockIdx.x) * SORT_RADIX + threadIdx.x] = h[threadIdx.x];
}

// in place: hist[seg][tile][d] becomes the number of the segment's pairs with a smaller digit, or with digit d in an earlier tile.  1024 threads:
// thread (d, q) owns digit d over the q-th quarter of the tiles and keeps 16 independent loads in flight, so the chain of dependent memory
// round trips is ntiles / 64 long, twice (the totals, then the running offsets) - one thread per digit over all tiles took 55 us at 160 tiles.
#define SORT_SCAN_UN 16
__global__ __launch_bounds__(1024) void sort_offsets_kernel(unsigned* __restrict__ hist, int ntiles) {
  __shared__ unsigned part[4][SORT_RADIX];
  __shared__ unsigned tot[SORT_RADIX];
  const int d = threadIdx.x & (SORT_RADIX - 1), q = threadIdx.x >> USSEG_SORT_DIGIT_BITS;
  const int per = (ntiles + 3) / 4, lo = q * per, hi = lo + per < ntiles ? lo + per : ntiles;
  unsigned* const h = hist + (int64_t)blockIdx.x * ntiles * SORT_RADIX + d;
  unsigned s = 0u;
  for (int t = lo; t < hi; t += SORT_SCAN_UN) {
    unsigned v[SORT_SCAN_UN];
#pragma unroll
    for (int i = 0; i < SORT_SCAN_UN; ++i) v[i] = t + i < hi ? h[(int64_t)(t + i) * SORT_RADIX] : 0u;
#pragma unroll
    for (int i = 0; i < SORT_SCAN_UN; ++i) s += v[i];
  }
  part[q][d] = s;
  __syncthreads();
  if (q == 0) tot[d] = (part[0][d] + part[1][d]) + (part[2][d] + part[3][d]);
  __syncthreads();
  unsigned run = 0u;
  for (int k = 0; k < d; ++k) run += tot[k];
  for (int k = 0; k < q; ++k) run += part[k][d];
  for (int t = lo; t < hi; t += SORT_SCAN_UN) {
    unsigned v[SORT_SCAN_UN];
#pragma unroll
    for (int i = 0; i < SORT_SCAN_UN; ++i) v[i] = t + i < hi ? h[(int64_t)(t + i) * SORT_RADIX] : 0u;
#pragma unroll
    for (int i = 0; i < SORT_SCAN_UN; ++i) {
      if (t + i < hi) h[(int64_t)(t + i) * SORT_RADIX] = run;
      run += v[i];
    }
  }
}

__global__ __launch_bounds__(256) void sort_scatter_kernel(const unsigned* __restrict__ keys_in, const unsigned* __restrict__ vals_in,
                                                            unsigned* __restrict__ keys_out, unsigned* __restrict__ vals_out,
                                                            const unsigned* __restrict__ offs, int n, int ntiles, int shift, unsigned mask, int bits) {
  __shared__ unsigned cnt[4][SORT_RADIX];       // a wave's running count of each digit; afterwards where the wave's first pair of it sits in the sorted tile
  __shared__ unsigned goff[SORT_RADIX], wtot[4];
  __shared__ unsigned sk[SORT_TILE], sv[SORT_TILE];      // the tile in sorted order
  volatile unsigned* const vc = &cnt[0][0];
#pragma unroll
  for (int w = 0; w < 4; ++w) cnt[w][threadIdx.x] = 0u;
  __syncthreads();
  const int64_t seg = blockIdx.y, base = seg * n;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int i0 = blockIdx.x * SORT_TILE + wave * 512 + lane;
  unsigned key[8], val[8], rank[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int i = i0 + r * 64;
    const bool ok = i < n;
    key[r] = ok ? keys_in[base + i] : 0u;
    val[r] = ok ? vals_in[base + i] : 0u;
    const unsigned d = sort_digit(key[r], shift, mask);
    unsigned long long same = __ballot(ok);                   // (every lane takes part in every ballot; lanes past n match nobody)
    for (int b = 0; b < bits; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long v = __ballot(bit);
      same &= bit ? v : ~v;
    }
    const unsigned before = (unsigned)__popcll(same & below);
    const unsigned old = vc[wave * SORT_RADIX + d];          // the wave's LDS accesses execute in program order: every lane of a group reads
    if (ok && before == 0u) vc[wave * SORT_RADIX + d] = old + (unsigned)__popcll(same);      // the count before the group's first lane bumps it
    rank[r] = old + before;
  }
  __syncthreads();
  {   // thread d: where digit d starts inside the sorted tile (a scan over the 256 digit totals: shuffles in a wave, the four waves through LDS)
    const int d = threadIdx.x;
    unsigned c[4], total = 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) { c[w] = cnt[w][d]; total += c[w]; }
    unsigned x = total;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_up(x, o, 64);
      if (lane >= o) x += up;
    }
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    unsigned start = x - total;
    for (int w = 0; w < wave; ++w) start += wtot[w];
    goff[d] = offs[(seg * ntiles + blockIdx.x) * SORT_RADIX + d] - start;      // (mod 2^32) global position = goff[digit] + position in the sorted tile
#pragma unroll
    for (int w = 0; w < 4; ++w) { cnt[w][d] = start; start += c[w]; }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    if (i0 + r * 64 < n) {
      const unsigned at = cnt[wave][sort_digit(key[r], shift, mask)] + rank[r];      // < the tile's pair count <= SORT_TILE
      sk[at] = key[r];
      sv[at] = val[r];
    }
  }
  __syncthreads();
  const int left = n - blockIdx.x * SORT_TILE, have = left < SORT_TILE ? left : SORT_TILE;
#pragma unroll
  for (int r = 0; r < 8; ++r) {      // the sorted tile leaves in order: neighbouring threads write neighbouring words of one digit's run
    const int at = r * 256 + threadIdx.x;
    if (at < have) {
      const unsigned k = sk[at];
      const unsigned pos = goff[sort_digit(k, shift, mask)] + (unsigned)at;          // < n: offsets and ranks count pairs of this segment
      keys_out[base + pos] = k;
      vals_out[base + pos] = sv[at];
    }
  }
}

extern "C" int64_t usseg_sort_ws_bytes(int32_t S, int64_t n) {
  if (S < 0 || S > 65535 || n < 0 || n > ((int64_t)1 << 29)) return -1;
  return 2 * align256((int64_t)S * n * 4) + align256((int64_t)S * sort_tiles(n) * SORT_RADIX * 4);
}

static int sort_args(const char* who, const void* keys_in, const void* vals_in, int32_t S, int64_t n, int32_t key_bits, const void* keys_out,
                     const void* vals_out, const void* ws, int64_t ws_bytes) {
  USSEG_CHECK_ARG(S >= 0 && S <= 65535, "%s: 0 <= S <= 65535 segments", who);
  USSEG_CHECK_ARG(n >= 0 && n <= ((int64_t)1 << 29), "%s: 0 <= n <= 2^29 pairs a segment", who);
  USSEG_CHECK_ARG(key_bits >= 1 && key_bits <= 32, "%s: 1 <= key_bits <= 32", who);
  if (S == 0 || n == 0) return USSEG_OK;
  USSEG_CHECK_ARG(keys_in && vals_in && keys_out && vals_out && ws, "%s: null pointer", who);
  USSEG_CHECK_ARG((((uintptr_t)keys_in | (uintptr_t)vals_in | (uintptr_t)keys_out | (uintptr_t)vals_out) & 3) == 0 && ((uintptr_t)ws & 15) == 0,
                  "%s: keys and values must be 4-byte, the workspace 16-byte aligned", who);
  USSEG_CHECK_ARG(keys_in != keys_out && vals_in != vals_out && keys_out != vals_out, "%s: the outputs must not alias the inputs or each other", who);
  USSEG_CHECK_ARG(ws_bytes >= usseg_sort_ws_bytes(S, n), "%s: the workspace holds %lld bytes, %lld needed", who, (long long)ws_bytes,
                  (long long)usseg_sort_ws_bytes(S, n));
  return USSEG_OK;
}

// (arguments already checked)
static void sort_launch(const unsigned* keys_in, const unsigned* vals_in, int S, int n, int key_bits, unsigned* keys_out, unsigned* vals_out, void* ws,
                        hipStream_t s) {
  char* const w = (char*)ws;
  const int64_t pb = align256((int64_t)S * n * 4);
  unsigned* const tk = (unsigned*)w;
  unsigned* const tv = (unsigned*)(w + pb);
  unsigned* const hist = (unsigned*)(w + 2 * pb);
  const int ntiles = (int)sort_tiles(n), passes = (key_bits + USSEG_SORT_DIGIT_BITS - 1) / USSEG_SORT_DIGIT_BITS;
  const dim3 grid((unsigned)ntiles, (unsigned)S);
  const unsigned *ki = keys_in, *vi = vals_in;
  for (int p = 0; p < passes; ++p) {          // the last pass writes keys_out; the passes before it alternate with the workspace
    const bool to_out = ((passes - 1 - p) & 1) == 0;
    unsigned* const ko = to_out ? keys_out : tk;
    unsigned* const vo = to_out ? vals_out : tv;
    const int shift = p * USSEG_SORT_DIGIT_BITS;
    const int bits = key_bits - shift < USSEG_SORT_DIGIT_BITS ? key_bits - shift : USSEG_SORT_DIGIT_BITS;
    const unsigned mask = (1u << bits) - 1u;
    hipLaunchKernelGGL(sort_hist_kernel, grid, dim3(256), 0, s, ki, hist, n, ntiles, shift, mask);
    hipLaunchKernelGGL(sort_offsets_kernel, dim3((unsigned)S), dim3(1024), 0, s, hist, ntiles);
    hipLaunchKernelGGL(sort_scatter_kernel, grid, dim3(256), 0, s, ki, vi, ko, vo, hist, n, ntiles, shift, mask, bits);
    ki = ko; vi = vo;
  }
}

extern "C" int usseg_sort_pairs_u32(const uint32_t* keys_in, const uint32_t* vals_in, int32_t S, int64_t n, int32_t key_bits, uint32_t* keys_out,
                                    uint32_t* vals_out, void* ws, int64_t ws_bytes, usseg_stream_t stream) {
  const int rc = sort_args("sort_pairs_u32", keys_in, vals_in, S, n, key_bits, keys_out, vals_out, ws, ws_bytes);
  if (rc) return rc;
  if (S == 0 || n == 0) return USSEG_OK;
  sort_launch(keys_in, vals_in, S, (int)n, key_bits, keys_out, vals_out, ws, (hipStream_t)stream);
  return usseg_check_launch("sort_pairs_u32");
}

// ---- the Lovasz-softmax loss ---------------------------------------------------------------------------------------------------------
#define LV_ONE_BITS 0x3F800000u     // fp32 1.0: the clamp of the sort key; keys take 30 bits
#define LV_KEY_BITS 30
#define LV_HDR 32        // acc[0] loss, [1] ticket, [2] CCE pixel sum, [4..8) k_c, [16..20) L_c
#define LV_STRIDE 16     // floats per workgroup row of partials (C + 1 <= 5 used): acc[LV_HDR + 16*b + k], the overlap accumulator's geometry
#define LV_MAX_BLOCKS ((USSEG_OVERLAP_ACC_FLOATS - LV_HDR) / LV_STRIDE)

__device__ __forceinline__ bool lv_fg(float y, float thr) { return y > thr; }      // (a NaN is not foreground)

// keys [C][M] = 0x3F800000 - min(bits(|e|), 0x3F800000): ascending and stable on it is "error descending, ties by pixel index";
// payloads [C][M] = m | fg << 31
template <int C>
__global__ __launch_bounds__(256) void lovasz_keys_kernel(const float* __restrict__ probs, const float* __restrict__ y_true, unsigned* __restrict__ keys,
                                                           unsigned* __restrict__ vals, int M, float thr) {
  for (int m = blockIdx.x * 256 + threadIdx.x; m < M; m += gridDim.x * 256) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float p = probs[(int64_t)m * C + c];
      const bool fg = lv_fg(y_true[(int64_t)m * C + c], thr);
      const float e = fg ? 1.f - p : p;
      const unsigned b = __float_as_uint(e) & 0x7FFFFFFFu;
      keys[(int64_t)c * M + m] = LV_ONE_BITS - (b < LV_ONE_BITS ? b : LV_ONE_BITS);
      vals[(int64_t)c * M + m] = (unsigned)m | (fg ? 0x80000000u : 0u);
    }
  }
}

// foreground pairs per tile of the sorted order: tcnt[c][tile]
__global__ __launch_bounds__(256) void lovasz_tile_fg_kernel(const unsigned* __restrict__ vals, int* __restrict__ tcnt, int M, int ntiles) {
  __shared__ int wsum[4];
  const int64_t base = (int64_t)blockIdx.y * M;
  int s = 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int i = blockIdx.x * SORT_TILE + r * 256 + threadIdx.x;
    if (i < M) s += (int)(vals[base + i] >> 31);
  }
  for (int msk = 32; msk >= 1; msk >>= 1) s += __shfl_xor(s, msk, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) tcnt[(int64_t)blockIdx.y * ntiles + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// one workgroup per class: tcnt[c][.] becomes its exclusive scan, counts[c] = Y_c
__global__ __launch_bounds__(256) void lovasz_tile_scan_kernel(int* __restrict__ tcnt, int* __restrict__ counts, int ntiles) {
  __shared__ int part[256];
  int* const t = tcnt + (int64_t)blockIdx.x * ntiles;
  const int per = (ntiles + 255) / 256, lo = threadIdx.x * per, hi = lo + per < ntiles ? lo + per : ntiles;
  int s = 0;
  for (int i = lo; i < hi; ++i) s += t[i];
  part[threadIdx.x] = s;
  __syncthreads();
  int run = 0;
  for (int j = 0; j < (int)threadIdx.x; ++j) run += part[j];
  if (threadIdx.x == 255) counts[blockIdx.x] = run + s;
  for (int i = lo; i < hi; ++i) {
    const int c = t[i];
    t[i] = run;
    run += c;
  }
}

// rank r = the position in the sorted order, F = foreground pairs of rank <= r, Y = counts[c]: g by the closed form, to pixel order
__global__ __launch_bounds__(256) void lovasz_coeffs_kernel(const unsigned* __restrict__ vals, const int* __restrict__ tcnt, const int* __restrict__ counts,
                                                             float* __restrict__ g, int M, int ntiles, int C) {
  __shared__ int wcnt[8][4];
  const int c = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t base = (int64_t)c * M;
  const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
  unsigned v[8];
  int f[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int i = blockIdx.x * SORT_TILE + r * 256 + threadIdx.x;
    v[r] = i < M ? vals[base + i] : 0u;
    const unsigned long long b = __ballot((v[r] >> 31) != 0u);
    f[r] = __popcll(b & upto);
    if (lane == 0) wcnt[r][wave] = __popcll(b);
  }
  __syncthreads();
  const int Y = counts[c];
  int run = tcnt[(int64_t)c * ntiles + blockIdx.x];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int before = run;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) before += wcnt[r][w];
      run += wcnt[r][w];
    }
    const int i = blockIdx.x * SORT_TILE + r * 256 + threadIdx.x;
    if (i >= M) continue;
    const int F = before + f[r];
    const bool fg = (v[r] >> 31) != 0u;
    const int64_t I = (int64_t)Y - F, U = (int64_t)Y + i + 1 - F;
    float gv;
    if (Y == 0) gv = i == 0 ? 1.f : 0.f;
    else if (fg) gv = 1.f / (float)U;
    else gv = (float)I / (float)(U * (U - 1));        // U - 1 >= Y >= 1 at a background pixel; the product is exact in int64
    g[(int64_t)(v[r] & 0x7FFFFFFFu) * C + c] = gv;
  }
}

// the parameters as the kernels take them, by value: lvk = lv_weight * ov_scale and cek = ce_weight * inv_global_batch folded on the host
struct LovaszK { float w[4]; float lvk, cek, thr; int all; };

template <int C>
__device__ __forceinline__ void lv_load_group(const float* __restrict__ base, int g, int M, float (&v)[4 * C]) {
  if (4 * g + 4 <= M) {
    const float4* q = reinterpret_cast<const float4*>(base) + (int64_t)g * C;
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const float4 t = q[i];
      v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
    }
  } else {
    const int n = (M - 4 * g) * C;      // floats that exist in the last, partial group
#pragma unroll
    for (int i = 0; i < 4 * C; ++i) v[i] = i < n ? base[(int64_t)g * (4 * C) + i] : 0.f;
  }
}

// CategoricalCrossentropy(label_smoothing) on probabilities, one pixel: overlap_loss.hip's ov_cce_pixel, the arithmetic of loss_kind 0
template <int C, bool GRAD>
__device__ __forceinline__ float lv_cce_pixel(const float* p, const float* y, float ls, float eps, float* dLdp) {
  float S = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) S += p[c];
  float l = 0.f, u[C], ubar = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float ys = y[c] * (1.f - ls) + ls / (float)C;
    const float q = p[c] / S;
    const float qc = fminf(fmaxf(q, eps), 1.f - eps);
    l -= ys * __logf(qc);
    if (GRAD) {
      u[c] = (q > eps && q < 1.f - eps) ? -ys / qc : 0.f;
      ubar += u[c] * q;
    }
  }
  if (GRAD) {
#pragma unroll
    for (int c = 0; c < C; ++c) dLdp[c] = (u[c] - ubar) / S;
  }
  return l;
}

// K = C + 1 totals (L_c, the CCE pixel sum) by overlap_sums_kernel's ordered reduction: per thread in index order, a wave by a butterfly, the
// four waves as (0+1)+(2+3), the workgroups' rows published by ONE returning agent-scope exchange each and folded into the operand of the
// ticket add, the LAST workgroup to arrive adding them in a fixed order.  tools/check_ordered_sum.py checks the ISA of this sequence.
template <int C, bool CE>
__global__ __launch_bounds__(256) void lovasz_sums_kernel(const LovaszK k, const float* __restrict__ probs, const float* __restrict__ y_true,
                                                           const float* __restrict__ gco, const int* __restrict__ counts, float* acc, int M, int ngroups,
                                                           float ls, float eps) {
  constexpr int K = C + 1;
  __shared__ float red[4][LV_STRIDE];
  __shared__ float fin[16][LV_STRIDE + 1];
  __shared__ float tot[LV_STRIDE];
  __shared__ int s_last;
  float s[K];
#pragma unroll
  for (int i = 0; i < K; ++i) s[i] = 0.f;
  for (int g = blockIdx.x * 256 + threadIdx.x; g < ngroups; g += gridDim.x * 256) {
    float p[4 * C], y[4 * C], gc[4 * C];
    lv_load_group<C>(probs, g, M, p);
    lv_load_group<C>(y_true, g, M, y);
    lv_load_group<C>(gco, g, M, gc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (4 * g + j >= M) break;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float e = lv_fg(y[j * C + c], k.thr) ? 1.f - p[j * C + c] : p[j * C + c];
        s[c] += e * gc[j * C + c];
      }
      if (CE) s[C] += lv_cce_pixel<C, false>(p + j * C, y + j * C, ls, eps, nullptr);
    }
  }
#pragma unroll
  for (int i = 0; i < K; ++i) {
    float v = s[i];
    for (int msk = 32; msk >= 1; msk >>= 1) v += __shfl_xor(v, msk, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = v;
  }
  __syncthreads();
  const int nb = gridDim.x;
  if (threadIdx.x < 64) {
    unsigned zero = 0u;
    if (threadIdx.x < K) {
      const float t = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
      const float old = __hip_atomic_exchange(acc + LV_HDR + blockIdx.x * LV_STRIDE + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("; ticket after the partials are at the memory side" : "+v"(zero) : "v"(old));
    }
    for (int msk = 8; msk >= 1; msk >>= 1) zero |= __shfl_xor(zero, msk, 64);     // lane 0 holds a value that depends on all K returns (K <= 5)
    if (threadIdx.x == 0) {
      const unsigned tk = __hip_atomic_fetch_add(reinterpret_cast<unsigned*>(acc + 1), 1u + zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_last = (tk == (unsigned)nb - 1u);
    }
  }
  __syncthreads();
  if (!s_last) return;
  {
    const int kk = threadIdx.x & 15, j = threadIdx.x >> 4;
    float v = 0.f;
    for (int b0 = j; b0 < nb; b0 += 16 * 8) {     // eight independent loads in flight, added in workgroup order
      float t[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int b = b0 + 16 * i;
        t[i] = (b < nb && kk < K) ? __hip_atomic_load(acc + LV_HDR + b * LV_STRIDE + kk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) v += t[i];
    }
    fin[j][kk] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int c = threadIdx.x;
    float a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = fin[2 * i][c] + fin[2 * i + 1][c];
    tot[c] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int ns = 0;
    bool in[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { in[c] = M > 0 && (k.all || counts[c] > 0); ns += in[c] ? 1 : 0; }
    const float inv = ns > 0 ? 1.f / (float)ns : 0.f;
    float lv = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (in[c]) lv += k.w[c] * tot[c];
      acc[4 + c] = in[c] ? k.lvk * k.w[c] * inv : 0.f;
      acc[16 + c] = tot[c];
    }
    const float ce = CE ? tot[C] : 0.f;
    acc[2] = ce;
    acc[0] = k.cek * ce + k.lvk * (lv * inv);       // OVERWRITES: no zero-fill launch in front of the kernel
    __hip_atomic_store(reinterpret_cast<unsigned*>(acc + 1), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// dlogit_j = p_j*(G_j - sum_c p_c*G_c), G_c = k_c*(fg ? -g : +g) (+ the CCE term): overlap_bwd_kernel's layouts, one bf16 rounding
template <int C, bool CE, bool QUAD>
__global__ __launch_bounds__(256) void lovasz_bwd_kernel(const float cek, const float thr, const float* __restrict__ probs, const float* __restrict__ y_true,
                                                          const float* __restrict__ gco, const float* __restrict__ acc, bf16_t* __restrict__ dl, int M,
                                                          int ngroups, int HW, int W, float ls, float eps) {
  float kc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) kc[c] = acc[4 + c];
  for (int g = blockIdx.x * 256 + threadIdx.x; g < ngroups; g += gridDim.x * 256) {
    float p[4 * C], y[4 * C], gc[4 * C];
    lv_load_group<C>(probs, g, M, p);
    lv_load_group<C>(y_true, g, M, y);
    lv_load_group<C>(gco, g, M, gc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = 4 * g + j;
      if (m >= M) break;
      float G[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float t = kc[c] * gc[j * C + c];
        G[c] = lv_fg(y[j * C + c], thr) ? -t : t;
      }
      if (CE) {
        float dce[C];
        lv_cce_pixel<C, true>(p + j * C, y + j * C, ls, eps, dce);
#pragma unroll
        for (int c = 0; c < C; ++c) G[c] += dce[c] * cek;
      }
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) dot += G[c] * p[j * C + c];
      float o[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = c < C ? p[j * C + (c < C ? c : 0)] * (G[c < C ? c : 0] - dot) : 0.f;
      if (QUAD) {
        const unsigned b = (unsigned)m / (unsigned)HW, hw = (unsigned)m - b * (unsigned)HW;
        const unsigned yy = hw / (unsigned)W, xx = hw - yy * (unsigned)W;
        const int64_t q = ((int64_t)b * (HW / W / 2) + (yy >> 1)) * (W / 2) + (xx >> 1);
        uint2 v;
        v.x = pack2bf(o[0], o[1]); v.y = pack2bf(o[2], o[3]);
        *reinterpret_cast<uint2*>(dl + q * 16 + 4 * ((yy & 1) * 2 + (xx & 1))) = v;
      } else {
        uint4 v;
        v.x = pack2bf(o[0], o[1]); v.y = pack2bf(o[2], o[3]); v.z = 0u; v.w = 0u;
        *reinterpret_cast<uint4*>(dl + (int64_t)m * 8) = v;
      }
    }
  }
}

// ---- entry points: every argument is checked before any launch ------------------------------------------------------------------------
extern "C" int64_t usseg_lovasz_ws_bytes(int64_t M, int32_t C) {
  if (M < 0 || M > ((int64_t)1 << 29) || C < 1 || C > 4) return -1;
  return 4 * align256(C * M * 4) + align256(C * sort_tiles(M) * 4) + usseg_sort_ws_bytes(C, M);
}

static int lovasz_args(const char* who, const UssegLossDesc* d, const UssegLovaszLoss* ll, const float* probs, const float* y_true, const float* g) {
  USSEG_CHECK_ARG(d, "%s: null descriptor", who);
  USSEG_CHECK_ARG(probs && y_true && g, "%s: null pointer", who);
  USSEG_CHECK_ARG(d->C >= 1 && d->C <= 4, "%s: 1 <= C <= 4", who);
  USSEG_CHECK_ARG(d->HW > 0 && d->M >= 0 && d->M % d->HW == 0, "%s: M must be a non-negative multiple of HW", who);
  USSEG_CHECK_ARG(d->M <= (1 << 29), "%s: more than 2^29 pixels", who);
  USSEG_CHECK_ARG((((uintptr_t)probs | (uintptr_t)y_true | (uintptr_t)g) & 15) == 0, "%s: probs, y_true and g must be 16-byte aligned", who);
  USSEG_CHECK_ARG(std::isfinite(ll->threshold), "%s: threshold must be finite", who);
  USSEG_CHECK_ARG(ll->all_classes == 0 || ll->all_classes == 1, "%s: all_classes must be 0 or 1", who);
  USSEG_CHECK_ARG(std::isfinite(ll->lv_weight) && ll->lv_weight >= 0.f && std::isfinite(ll->ce_weight) && ll->ce_weight >= 0.f,
                  "%s: lv_weight and ce_weight must be finite and >= 0", who);
  for (int c = 0; c < d->C; ++c) USSEG_CHECK_ARG(std::isfinite(ll->w[c]) && ll->w[c] >= 0.f, "%s: class weights must be finite and >= 0", who);
  USSEG_CHECK_ARG(std::isfinite(d->inv_global_batch) && d->inv_global_batch >= 0.f, "%s: inv_global_batch must be finite and >= 0", who);
  if (ll->ce_weight != 0.f) {
    USSEG_CHECK_ARG(d->label_smoothing >= 0.f && d->label_smoothing < 1.f, "%s: label_smoothing must lie in [0, 1)", who);
    USSEG_CHECK_ARG(d->clip_eps > 0.f && 1.f - d->clip_eps < 1.f && d->clip_eps < 0.5f, "%s: clip_eps must be > 0 and representable below 1 in fp32", who);
  }
  return USSEG_OK;
}
static inline int lovasz_groups(const UssegLossDesc* d) { return (int)((d->M + 3) / 4); }

extern "C" int usseg_lovasz_coeffs(const UssegLossDesc* d, UssegLovaszLoss ll, const float* probs, const float* y_true, float* g, int32_t* counts,
                                   void* ws, int64_t ws_bytes, usseg_stream_t stream) {
  const char* who = "lovasz_coeffs";
  const int rc = lovasz_args(who, d, &ll, probs, y_true, g);
  if (rc) return rc;
  USSEG_CHECK_ARG(counts && ((uintptr_t)counts & 3) == 0, "%s: counts must be a 4-byte aligned pointer", who);
  USSEG_CHECK_ARG(ws && ((uintptr_t)ws & 15) == 0, "%s: the workspace must be a 16-byte aligned pointer", who);
  USSEG_CHECK_ARG(ws_bytes >= usseg_lovasz_ws_bytes(d->M, d->C), "%s: the workspace holds %lld bytes, %lld needed", who, (long long)ws_bytes,
                  (long long)usseg_lovasz_ws_bytes(d->M, d->C));
  hipStream_t s = (hipStream_t)stream;
  const int C = d->C, M = (int)d->M;
  if (M == 0) {                                   // Y_c = 0; nothing to rank
    if (hipMemsetAsync(counts, 0, sizeof(int32_t) * C, s) != hipSuccess) return usseg_check_launch(who);
    return USSEG_OK;
  }
  char* w = (char*)ws;
  const int64_t pb = align256((int64_t)C * M * 4);
  const int ntiles = (int)sort_tiles(M);
  unsigned* const keys = (unsigned*)w;
  unsigned* const vals = (unsigned*)(w + pb);
  unsigned* const skeys = (unsigned*)(w + 2 * pb);
  unsigned* const svals = (unsigned*)(w + 3 * pb);
  int* const tcnt = (int*)(w + 4 * pb);
  void* const sws = w + 4 * pb + align256((int64_t)C * ntiles * 4);
  int64_t gk = cdiv64(M, 256);
  if (gk > 2048) gk = 2048;
#define LV_KEYS(CC) hipLaunchKernelGGL(lovasz_keys_kernel<CC>, dim3((unsigned)gk), dim3(256), 0, s, probs, y_true, keys, vals, M, ll.threshold)
  switch (C) {
    case 1: LV_KEYS(1); break;
    case 2: LV_KEYS(2); break;
    case 3: LV_KEYS(3); break;
    default: LV_KEYS(4); break;
  }
#undef LV_KEYS
  sort_launch(keys, vals, C, M, LV_KEY_BITS, skeys, svals, sws, s);
  const dim3 grid((unsigned)ntiles, (unsigned)C);
  hipLaunchKernelGGL(lovasz_tile_fg_kernel, grid, dim3(256), 0, s, svals, tcnt, M, ntiles);
  hipLaunchKernelGGL(lovasz_tile_scan_kernel, dim3((unsigned)C), dim3(256), 0, s, tcnt, counts, ntiles);
  hipLaunchKernelGGL(lovasz_coeffs_kernel, grid, dim3(256), 0, s, svals, tcnt, counts, g, M, ntiles, C);
  return usseg_check_launch(who);
}

extern "C" int usseg_lovasz_loss_sums(const UssegLossDesc* d, UssegLovaszLoss ll, float ov_scale, const float* probs, const float* y_true, const float* g,
                                      const int32_t* counts, float* acc, int64_t acc_floats, usseg_stream_t stream) {
  const char* who = "lovasz_loss_sums";
  const int rc = lovasz_args(who, d, &ll, probs, y_true, g);
  if (rc) return rc;
  USSEG_CHECK_ARG(counts && ((uintptr_t)counts & 3) == 0, "%s: counts must be a 4-byte aligned pointer", who);
  USSEG_CHECK_ARG(acc && ((uintptr_t)acc & 3) == 0, "%s: acc must be a 4-byte aligned pointer", who);
  USSEG_CHECK_ARG(std::isfinite(ov_scale) && ov_scale >= 0.f, "%s: ov_scale must be finite and >= 0", who);
  const int grid = usseg_overlap_loss_grid(d->M);
  USSEG_CHECK_ARG(grid <= LV_MAX_BLOCKS && acc_floats >= LV_HDR + (int64_t)LV_STRIDE * grid, "%s: a grid of %d workgroups needs %d accumulator floats",
                  who, grid, LV_HDR + LV_STRIDE * grid);
  LovaszK k = {};
  for (int c = 0; c < d->C; ++c) k.w[c] = ll.w[c];
  k.lvk = ll.lv_weight * ov_scale;
  k.cek = ll.ce_weight * d->inv_global_batch;
  k.thr = ll.threshold;
  k.all = ll.all_classes;
  const bool ce = ll.ce_weight != 0.f;
  const int M = (int)d->M, ng = lovasz_groups(d);
  hipStream_t s = (hipStream_t)stream;
#define LV_SUMS2(CC, CEB)                                                                                                                  \
  hipLaunchKernelGGL((lovasz_sums_kernel<CC, CEB>), dim3(grid), dim3(256), 0, s, k, probs, y_true, g, counts, acc, M, ng, CEB ? d->label_smoothing : 0.f, \
                     CEB ? d->clip_eps : 0.f)
#define LV_SUMS(CC) \
  if (ce) LV_SUMS2(CC, true); else LV_SUMS2(CC, false)
  switch (d->C) {
    case 1: LV_SUMS(1); break;
    case 2: LV_SUMS(2); break;
    case 3: LV_SUMS(3); break;
    default: LV_SUMS(4); break;
  }
#undef LV_SUMS
#undef LV_SUMS2
  return usseg_check_launch(who);
}

extern "C" int usseg_lovasz_loss_bwd(const UssegLossDesc* d, UssegLovaszLoss ll, const float* probs, const float* y_true, const float* g, const float* acc,
                                     int64_t acc_floats, void* dlogits, usseg_stream_t stream) {
  const char* who = "lovasz_loss_bwd";
  const int rc = lovasz_args(who, d, &ll, probs, y_true, g);
  if (rc) return rc;
  USSEG_CHECK_ARG(acc && ((uintptr_t)acc & 3) == 0 && acc_floats >= LV_HDR, "%s: acc must hold its %d header floats", who, LV_HDR);
  USSEG_CHECK_ARG(dlogits && ((uintptr_t)dlogits & 15) == 0, "%s: dlogits must be a 16-byte aligned pointer", who);
  USSEG_CHECK_ARG(d->quad_w == 0 || (d->quad_w > 0 && d->quad_w % 2 == 0 && d->HW % (2 * d->quad_w) == 0), "%s: quad layout needs even H and W", who);
  USSEG_CHECK_ARG(d->lddl == (d->quad_w ? 16 : 8), "%s: dlogits stride must be 8 (16 in the quad layout)", who);
  if (d->M == 0) return USSEG_OK;
  const float cek = ll.ce_weight * d->inv_global_batch;
  const bool ce = ll.ce_weight != 0.f;
  const int M = (int)d->M, ng = lovasz_groups(d);
  int64_t gb = cdiv64(ng, 256);
  if (gb > 2048) gb = 2048;
  const dim3 grid((unsigned)gb);
  bf16_t* dl = (bf16_t*)dlogits;
  hipStream_t s = (hipStream_t)stream;
#define LV_BWD2(CC, CEB, Q)                                                                                                              \
  hipLaunchKernelGGL((lovasz_bwd_kernel<CC, CEB, Q>), grid, dim3(256), 0, s, cek, ll.threshold, probs, y_true, g, acc, dl, M, ng, d->HW, \
                     d->quad_w ? d->quad_w : 1, d->label_smoothing, d->clip_eps)
#define LV_BWD(CC)                                                                  \
  if (ce) { if (d->quad_w) LV_BWD2(CC, true, true); else LV_BWD2(CC, true, false); } \
  else { if (d->quad_w) LV_BWD2(CC, false, true); else LV_BWD2(CC, false, false); }
  switch (d->C) {
    case 1: LV_BWD(1) break;
    case 2: LV_BWD(2) break;
    case 3: LV_BWD(3) break;
    default: LV_BWD(4) break;
  }
#undef LV_BWD
#undef LV_BWD2
  return usseg_check_launch(who);
}
