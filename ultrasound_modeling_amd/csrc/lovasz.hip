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
// backward pass are the two passes of a region loss as overlap_loss.hip has them, under the same grid rule: the ordered, ticketed grid
// reduction is grid_ordered_sums (common.h); the group loader, the CCE arithmetic, the dlogits store and the shared checks are region_loss.h's.
#include "region_loss.h"

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
// the accumulator header (region_loss.h has its geometry): acc[0] loss, [1] ticket, [2] CCE pixel sum, [4..8) k_c, [16..20) L_c; C + 1 <= 5
// floats of a workgroup's row of partials are used

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

// K = C + 1 totals (L_c, the CCE pixel sum): a thread adds its pixels in index order, grid_ordered_sums (common.h) the threads, waves and
// workgroups in a fixed order; thread 0 of the last workgroup to arrive finishes and puts the ticket back to zero.
template <int C, bool CE>
__global__ __launch_bounds__(256) void lovasz_sums_kernel(const LovaszK k, const float* __restrict__ probs, const float* __restrict__ y_true,
                                                           const float* __restrict__ gco, const int* __restrict__ counts, float* acc, int M, int ngroups,
                                                           float ls, float eps) {
  constexpr int K = C + 1;
  __shared__ float red[4][REGION_STRIDE];
  __shared__ float fin[16][REGION_STRIDE + 1];
  __shared__ float tot[REGION_STRIDE];
  __shared__ int s_last;
  float s[K];
#pragma unroll
  for (int i = 0; i < K; ++i) s[i] = 0.f;
  for (int g = blockIdx.x * 256 + threadIdx.x; g < ngroups; g += gridDim.x * 256) {
    float p[4 * C], y[4 * C], gc[4 * C];
    region_load_group<C>(probs, g, M, p);
    region_load_group<C>(y_true, g, M, y);
    region_load_group<C>(gco, g, M, gc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (4 * g + j >= M) break;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float e = lv_fg(y[j * C + c], k.thr) ? 1.f - p[j * C + c] : p[j * C + c];
        s[c] += e * gc[j * C + c];
      }
      if (CE) s[C] += region_cce_pixel<C, false>(p + j * C, y + j * C, ls, eps, nullptr);
    }
  }
  if (!grid_ordered_sums<K, REGION_HDR, REGION_STRIDE>(s, acc, red, fin, tot, s_last)) return;
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

// dlogit_j = p_j*(G_j - sum_c p_c*G_c), G_c = k_c*(fg ? -g : +g) (+ the CCE term), one bf16 rounding (region_store_dlogits)
template <int C, bool CE, bool QUAD>
__global__ __launch_bounds__(256) void lovasz_bwd_kernel(const float cek, const float thr, const float* __restrict__ probs, const float* __restrict__ y_true,
                                                          const float* __restrict__ gco, const float* __restrict__ acc, bf16_t* __restrict__ dl, int M,
                                                          int ngroups, int HW, int W, float ls, float eps) {
  float kc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) kc[c] = acc[4 + c];
  for (int g = blockIdx.x * 256 + threadIdx.x; g < ngroups; g += gridDim.x * 256) {
    float p[4 * C], y[4 * C], gc[4 * C];
    region_load_group<C>(probs, g, M, p);
    region_load_group<C>(y_true, g, M, y);
    region_load_group<C>(gco, g, M, gc);
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
        region_cce_pixel<C, true>(p + j * C, y + j * C, ls, eps, dce);
#pragma unroll
        for (int c = 0; c < C; ++c) G[c] += dce[c] * cek;
      }
      region_store_dlogits<C, QUAD>(G, p + j * C, dl, m, HW, W);
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
  const int rc = region_shape_args(who, d);
  if (rc) return rc;
  USSEG_CHECK_ARG((((uintptr_t)probs | (uintptr_t)y_true | (uintptr_t)g) & 15) == 0, "%s: probs, y_true and g must be 16-byte aligned", who);
  USSEG_CHECK_ARG(std::isfinite(ll->threshold), "%s: threshold must be finite", who);
  USSEG_CHECK_ARG(ll->all_classes == 0 || ll->all_classes == 1, "%s: all_classes must be 0 or 1", who);
  USSEG_CHECK_ARG(std::isfinite(ll->lv_weight) && ll->lv_weight >= 0.f && std::isfinite(ll->ce_weight) && ll->ce_weight >= 0.f,
                  "%s: lv_weight and ce_weight must be finite and >= 0", who);
  for (int c = 0; c < d->C; ++c) USSEG_CHECK_ARG(std::isfinite(ll->w[c]) && ll->w[c] >= 0.f, "%s: class weights must be finite and >= 0", who);
  return region_scale_args(who, d, ll->ce_weight);
}

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
  USSEG_CHECK_ARG(grid <= REGION_MAX_BLOCKS && acc_floats >= REGION_HDR + (int64_t)REGION_STRIDE * grid,
                  "%s: a grid of %d workgroups needs %d accumulator floats", who, grid, REGION_HDR + REGION_STRIDE * grid);
  LovaszK k = {};
  for (int c = 0; c < d->C; ++c) k.w[c] = ll.w[c];
  k.lvk = ll.lv_weight * ov_scale;
  k.cek = ll.ce_weight * d->inv_global_batch;
  k.thr = ll.threshold;
  k.all = ll.all_classes;
  const bool ce = ll.ce_weight != 0.f;
  const int M = (int)d->M, ng = region_groups(d);
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
  int rc = lovasz_args(who, d, &ll, probs, y_true, g);
  if (rc) return rc;
  USSEG_CHECK_ARG(acc && ((uintptr_t)acc & 3) == 0 && acc_floats >= REGION_HDR, "%s: acc must hold its %d header floats", who, REGION_HDR);
  if ((rc = region_bwd_args(who, d, dlogits))) return rc;
  if (d->M == 0) return USSEG_OK;
  const float cek = ll.ce_weight * d->inv_global_batch;
  const bool ce = ll.ce_weight != 0.f;
  const int M = (int)d->M, ng = region_groups(d);
  const dim3 grid = region_bwd_grid(ng);
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
