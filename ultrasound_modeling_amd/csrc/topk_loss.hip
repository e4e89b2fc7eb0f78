// An exact grid-wide selection of the k-th largest of n uint32 keys per segment, and the top-k (hard-pixel) cross-entropy built on it:
// usseg.h, usseg_topk_select and UssegTopkLoss.
//
// Select.  An MSD radix select with 8-bit digits over the table hist int32 [S][4][256].  Level L (0 = bits 31..24) is ONE launch of
// topk_refine_kernel: every workgroup re-derives the prefix chosen so far and the rank that remains from the tables of the levels before it
// (a 256-entry scan in LDS per level), and adds the digit-L histogram of the keys that carry the prefix: a wave shares one LDS atomic among
// the lanes that agree with its first matching lane, a workgroup flushes one global integer atomic per non-empty bin.  The same kernel at
// level 4 histograms nothing: one workgroup per segment writes sel[s] = {t, ngt, neq, k}.  Integer atomics only, so the result is a function
// of the inputs; a level boundary is a launch boundary, so no workgroup waits for another; the launches are fixed by (S, n) and never by the
// data; the fraction is read from device memory by every launch.
//
// Loss.  The per-pixel CCE l(m) (region_cce_pixel<C, false>: the arithmetic of loss_kind 0) is written once as fp32, its bits with the sign
// cleared are the keys.  The launches: zero the table (a memset node), l and the level-0 histogram (1), levels 1..3 (3), sel (1) - then the two
// passes of a region loss as overlap_loss.hip and lovasz.hip have them, under the same grid rules: the sums pass (grid_ordered_sums, common.h)
// and the backward pass (region_store_dlogits, region_loss.h).  Seven kernels and one memset whatever the data.
#include "region_loss.h"

#define TK_BINS 256
#define TK_LEVELS 4
#define TK_TILE 2048        // keys a workgroup reads per step of a refinement: 256 threads x 8
#define TK_SEG_MAX ((int64_t)1 << 29)

static inline int64_t tk_align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// k = max(1, min(n, floor((double)f * n))): the product of a 24-bit and a 30-bit number is exact in fp64.  Anything that does not compare
// (a NaN fraction) gives 1.  Without a fraction pointer the explicit k, clamped the same way.  n >= 1.
__device__ __forceinline__ int tk_count(const float* __restrict__ frac, int k_explicit, int n) {
  if (!frac) return k_explicit < 1 ? 1 : (k_explicit > n ? n : k_explicit);
  const double v = floor((double)frac[0] * (double)n);
  return v >= (double)n ? n : (v >= 1.0 ? (int)v : 1);
}

// one more count in bin `bin` of the LDS table h for every lane with `match`; the lanes that agree with the first matching lane share one
// atomic.  Called by whole waves.
__device__ __forceinline__ void tk_hist_add(int* h, int bin, bool match) {
  const unsigned long long m = __ballot(match);
  if (!m) return;
  const int first = __shfl(bin, __ffsll(m) - 1, 64);
  const unsigned long long same = __ballot(match && bin == first);
  if (!match) return;
  if (bin != first) atomicAdd(&h[bin], 1);
  else if ((int)(threadIdx.x & 63) == __ffsll(same) - 1) atomicAdd(&h[first], __popcll(same));
}

// The state of the select after `levels` digits, from the tables of segment `seg`: the prefix of the k-th largest key, the keys above the
// prefix (ngt), the keys in the last chosen bin (neq; n before the first digit).  Thread tid owns digit 255 - tid, so an inclusive scan over
// the threads counts the keys whose digit is >= its own.  Called by whole workgroups of 256 threads; the result is the same in every thread.
struct TkState { unsigned prefix; int ngt, neq, krem; };
__device__ __forceinline__ TkState tk_descend(const int* __restrict__ hist, int64_t seg, int levels, int k, int n, int (&s_w)[4], int (&s_pick)[3]) {
  TkState st = {0u, 0, n, k};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, digit = TK_BINS - 1 - (int)threadIdx.x;
  int cnts[TK_LEVELS];
#pragma unroll
  for (int L = 0; L < TK_LEVELS; ++L) cnts[L] = L < levels ? hist[(seg * TK_LEVELS + L) * TK_BINS + digit] : 0;      // every level's load in flight at once
#pragma unroll
  for (int L = 0; L < TK_LEVELS; ++L) {
    if (L >= levels) break;
    const int cnt = cnts[L];
    int x = cnt;
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(x, o, 64);
      if (lane >= o) x += up;
    }
    if (lane == 63) s_w[wave] = x;
    if (threadIdx.x == 0) { s_pick[0] = 0; s_pick[1] = 0; s_pick[2] = 0; }
    __syncthreads();
    for (int w = 0; w < wave; ++w) x += s_w[w];
    const int above = x - cnt;                      // keys with the prefix and a larger digit
    if (cnt > 0 && above < st.krem && st.krem <= x) { s_pick[0] = digit; s_pick[1] = above; s_pick[2] = cnt; }      // exactly one thread
    __syncthreads();
    st.prefix = (st.prefix << 8) | (unsigned)s_pick[0];
    st.ngt += s_pick[1];
    st.krem -= s_pick[1];
    st.neq = s_pick[2];
    __syncthreads();
  }
  return st;
}

// grid (x, y): segments blockIdx.y, blockIdx.y + gridDim.y, ...; the workgroups of a row share a segment's keys in steps of TK_TILE.
// level < 4: hist[seg][level][.] += the digit counts of the keys that carry the prefix of the levels before.  level == 4 (gridDim.x == 1): sel.
// A key is keys[i] & mask: all 32 bits for usseg_topk_select, the sign bit cleared for the loss values.
__global__ __launch_bounds__(256) void topk_refine_kernel(const unsigned* __restrict__ keys, int* __restrict__ hist, int* __restrict__ sel,
                                                           const float* __restrict__ frac, int k_explicit, int n, int S, int level, unsigned mask) {
  __shared__ int h[TK_BINS];
  __shared__ int s_w[4], s_pick[3];
  const int k = tk_count(frac, k_explicit, n);
  for (int64_t seg = blockIdx.y; seg < S; seg += gridDim.y) {
    const TkState st = tk_descend(hist, seg, level, k, n, s_w, s_pick);
    if (level == TK_LEVELS) {
      if (threadIdx.x == 0) {
        int* o = sel + seg * 4;
        o[0] = (int)st.prefix; o[1] = st.ngt; o[2] = st.neq; o[3] = k;
      }
      continue;
    }
    h[threadIdx.x] = 0;
    __syncthreads();
    const unsigned* kp = keys + seg * n;
    const int shift = 24 - 8 * level;
    for (int t0 = blockIdx.x * TK_TILE; t0 < n; t0 += gridDim.x * TK_TILE) {       // (uniform in the workgroup: every wave reaches every ballot)
      unsigned key[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int i = t0 + r * 256 + (int)threadIdx.x;
        key[r] = i < n ? (kp[i] & mask) : 0u;
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const bool in = t0 + r * 256 + (int)threadIdx.x < n;
        const bool match = in && (level == 0 || (key[r] >> (shift + 8)) == st.prefix);
        tk_hist_add(h, (int)((key[r] >> shift) & 255u), match);
      }
    }
    __syncthreads();
    const int c = h[threadIdx.x];
    if (c) atomicAdd(&hist[(seg * TK_LEVELS + level) * TK_BINS + threadIdx.x], c);
    __syncthreads();
  }
}

// l[m] = the CCE of pixel m; hist[seg(m)][0][.] += the top digit of its key.  Workgroup b owns the groups [b*chunk, (b+1)*chunk) (chunk a
// multiple of 256): the pixels of the segment its first pixel lies in are counted in LDS, any others (image scope, where a workgroup's
// range crosses an image boundary) go to the table directly.
template <int C>
__global__ __launch_bounds__(256) void topk_pixel_loss_kernel(const float* __restrict__ probs, const float* __restrict__ y_true, float* __restrict__ l,
                                                               int* __restrict__ hist, int M, int ngroups, int chunk, int n, float ls, float eps) {
  __shared__ int h[TK_BINS];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int g0 = blockIdx.x * chunk, g1 = g0 + chunk < ngroups ? g0 + chunk : ngroups;
  const int seg0 = (int)((unsigned)(4 * g0) / (unsigned)n);
  for (int gb = g0; gb < g1; gb += 256) {              // (uniform in the workgroup)
    const int g = gb + (int)threadIdx.x;
    const bool have = g < g1;
    float p[4 * C], y[4 * C], lv[4] = {0.f, 0.f, 0.f, 0.f};
    if (have) {
      region_load_group<C>(probs, g, M, p);
      region_load_group<C>(y_true, g, M, y);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = 4 * g + j;
      const bool ok = have && m < M;
      if (ok) lv[j] = region_cce_pixel<C, false>(p + j * C, y + j * C, ls, eps, nullptr);
      const int bin = (int)((__float_as_uint(lv[j]) & 0x7FFFFFFFu) >> 24);
      const int seg = ok ? (int)((unsigned)m / (unsigned)n) : seg0;
      tk_hist_add(h, bin, ok && seg == seg0);
      if (ok && seg != seg0) atomicAdd(&hist[(int64_t)seg * TK_LEVELS * TK_BINS + bin], 1);
    }
    if (have) {
      if (4 * g + 4 <= M) *reinterpret_cast<float4*>(l + 4 * (int64_t)g) = make_float4(lv[0], lv[1], lv[2], lv[3]);
      else
        for (int j = 0; 4 * g + j < M; ++j) l[4 * (int64_t)g + j] = lv[j];
    }
  }
  __syncthreads();
  const int c = h[threadIdx.x];
  if (c && g0 < ngroups) atomicAdd(&hist[(int64_t)seg0 * TK_LEVELS * TK_BINS + threadIdx.x], c);
}

// a(m) from the key of l and the segment's sel: 1 above t, r/neq at t (r = k - ngt, one fp32 division), 0 below
__device__ __forceinline__ float tk_weight_of(float lv, const int4 q) {
  const unsigned key = __float_as_uint(lv) & 0x7FFFFFFFu, t = (unsigned)q.x;
  if (key > t) return 1.f;
  if (key < t) return 0.f;
  return (float)(q.w - q.y) / (float)q.z;
}
// ... of the four pixels of group g (0 past M): one row of sel per group, and one more wherever an image boundary runs through it - no
// division per pixel, and none at all with one segment (n >= M)
__device__ __forceinline__ void tk_group_weights(const float (&lv)[4], const int* __restrict__ sel, int g, int M, int n, float (&a)[4]) {
  const int m0 = 4 * g;
  int seg = n >= M ? 0 : (int)((unsigned)m0 / (unsigned)n);
  int next = n >= M ? M : (seg + 1) * n;                // the first pixel of the next segment
  int4 q = *reinterpret_cast<const int4*>(sel + (int64_t)seg * 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = m0 + j;
    a[j] = 0.f;
    if (m >= M) continue;
    if (m >= next) {
      while (m >= next) { ++seg; next += n; }
      q = *reinterpret_cast<const int4*>(sel + (int64_t)seg * 4);
    }
    a[j] = tk_weight_of(lv[j], q);
  }
}

__device__ __forceinline__ void tk_load_l(const float* __restrict__ l, int g, int M, float (&v)[4]) {
  if (4 * g + 4 <= M) {
    const float4 t = *reinterpret_cast<const float4*>(l + 4 * (int64_t)g);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = 4 * g + j < M ? l[4 * (int64_t)g + j] : 0.f;
  }
}

// K = 2 totals (sum_m a(m)*l(m), sum_m l(m)): a thread adds its pixels in index order, grid_ordered_sums (common.h) the threads, waves and
// workgroups in a fixed order; thread 0 of the last workgroup to arrive finishes and puts the ticket back to zero.
__global__ __launch_bounds__(256) void topk_sums_kernel(const float* __restrict__ l, const int* __restrict__ sel, const float* __restrict__ ov_acc, float* acc,
                                                         int M, int ngroups, int n, float scale /* tk_weight * inv_global_batch */) {
  __shared__ float red[4][REGION_STRIDE];
  __shared__ float fin[16][REGION_STRIDE + 1];
  __shared__ float tot[REGION_STRIDE];
  __shared__ int s_last;
  float s[2] = {0.f, 0.f};
  for (int g = blockIdx.x * 256 + threadIdx.x; g < ngroups; g += gridDim.x * 256) {
    float lv[4], a[4];
    tk_load_l(l, g, M, lv);
    tk_group_weights(lv, sel, g, M, n, a);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (4 * g + j >= M) break;
      if (a[j] != 0.f) s[0] += a[j] * lv[j];      // (an unselected NaN cannot exist: a NaN key is above every finite one)
      s[1] += lv[j];
    }
  }
  if (!grid_ordered_sums<2, REGION_HDR, REGION_STRIDE>(s, acc, red, fin, tot, s_last)) return;
  if (threadIdx.x == 0) {
    const float coef = M > 0 ? (float)((double)scale * (double)n / (double)sel[3]) : 0.f;      // n and f are the same in every segment: so is k
    acc[2] = tot[1];
    acc[4] = coef;
    acc[5] = tot[0];
    acc[0] = coef * tot[0] + (ov_acc ? ov_acc[0] : 0.f);       // OVERWRITES: no zero-fill launch in front of the kernel
    __hip_atomic_store(reinterpret_cast<unsigned*>(acc + 1), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// dlogit_j = p_j*(G_j - sum_c p_c*G_c), G_c = (coef * a) * dLdp_c (+ A_c*y_c + B_c of the Dice term), one bf16 rounding (region_store_dlogits)
template <int C, bool QUAD, bool OV>
__global__ __launch_bounds__(256) void topk_bwd_kernel(const float* __restrict__ probs, const float* __restrict__ y_true, const float* __restrict__ l,
                                                        const int* __restrict__ sel, const float* __restrict__ acc, const float* __restrict__ ov_acc,
                                                        bf16_t* __restrict__ dl, int M, int ngroups, int n, int HW, int W, float ls, float eps) {
  const float coef = acc[4];
  float A[C], B[C];
#pragma unroll
  for (int c = 0; c < C; ++c) { A[c] = OV ? ov_acc[4 + c] : 0.f; B[c] = OV ? ov_acc[8 + c] : 0.f; }
  for (int g = blockIdx.x * 256 + threadIdx.x; g < ngroups; g += gridDim.x * 256) {
    float p[4 * C], y[4 * C], lv[4], aw[4];
    region_load_group<C>(probs, g, M, p);
    region_load_group<C>(y_true, g, M, y);
    tk_load_l(l, g, M, lv);
    tk_group_weights(lv, sel, g, M, n, aw);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = 4 * g + j;
      if (m >= M) break;
      const float a = aw[j];
      float G[C];
#pragma unroll
      for (int c = 0; c < C; ++c) G[c] = 0.f;
      if (a != 0.f) {
        float dce[C];
        region_cce_pixel<C, true>(p + j * C, y + j * C, ls, eps, dce);
        const float sc = coef * a;
#pragma unroll
        for (int c = 0; c < C; ++c) G[c] = sc * dce[c];
      }
      if (OV) {
#pragma unroll
        for (int c = 0; c < C; ++c) G[c] += A[c] * y[j * C + c] + B[c];
      }
      region_store_dlogits<C, QUAD>(G, p + j * C, dl, m, HW, W);
    }
  }
}

// ---- entry points: every argument is checked before any launch ------------------------------------------------------------------------
extern "C" int64_t usseg_topk_select_ws_bytes(int64_t S) {
  if (S < 0 || S > TK_SEG_MAX) return -1;
  return S * TK_LEVELS * TK_BINS * 4;
}

extern "C" int64_t usseg_topk_ws_bytes(int64_t M, int32_t HW, int32_t scope) {
  if (M < 0 || M > TK_SEG_MAX || HW <= 0 || M % HW != 0 || (scope != 0 && scope != 1)) return -1;
  if (M == 0) return 0;
  const int64_t S = scope ? M / HW : 1;
  return tk_align256(M * 4) + tk_align256(usseg_topk_select_ws_bytes(S)) + tk_align256(S * 16);
}

// (arguments already checked; S >= 1, n >= 1)  level_from = 1 when the level-0 histogram is in the table already
static void tk_select_launch(const unsigned* keys, int S, int n, const float* frac, int k, int* hist, int* sel, int level_from, unsigned mask,
                             hipStream_t s) {
  const int64_t gx = cdiv64(n, TK_TILE);
  const dim3 grid((unsigned)(gx > 512 ? 512 : gx), (unsigned)(S > 65535 ? 65535 : S));
  for (int level = level_from; level < TK_LEVELS; ++level)
    hipLaunchKernelGGL(topk_refine_kernel, grid, dim3(256), 0, s, keys, hist, sel, frac, k, n, S, level, mask);
  hipLaunchKernelGGL(topk_refine_kernel, dim3(1, grid.y), dim3(256), 0, s, keys, hist, sel, frac, k, n, S, TK_LEVELS, mask);
}

extern "C" int usseg_topk_select(const uint32_t* keys, int32_t S, int64_t n, const float* fraction, int32_t k, int32_t* sel, void* ws, int64_t ws_bytes,
                                 usseg_stream_t stream) {
  const char* who = "topk_select";
  USSEG_CHECK_ARG(S >= 0 && (int64_t)S <= TK_SEG_MAX, "%s: 0 <= S <= 2^29 segments", who);
  USSEG_CHECK_ARG(n >= 1 && n <= TK_SEG_MAX, "%s: 1 <= n <= 2^29 keys a segment", who);
  USSEG_CHECK_ARG((fraction != nullptr) != (k != 0), "%s: give the device fraction or an explicit k, not both and not neither", who);
  USSEG_CHECK_ARG(fraction || (k >= 1 && k <= n), "%s: 1 <= k <= n", who);
  if (S == 0) return USSEG_OK;
  USSEG_CHECK_ARG(keys && sel && ws, "%s: null pointer", who);
  USSEG_CHECK_ARG((((uintptr_t)keys | (uintptr_t)fraction) & 3) == 0 && (((uintptr_t)sel | (uintptr_t)ws) & 15) == 0,
                  "%s: keys and the fraction must be 4-byte, sel and the workspace 16-byte aligned", who);
  USSEG_CHECK_ARG(ws_bytes >= usseg_topk_select_ws_bytes(S), "%s: the workspace holds %lld bytes, %lld needed", who, (long long)ws_bytes,
                  (long long)usseg_topk_select_ws_bytes(S));
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(ws, 0, (size_t)usseg_topk_select_ws_bytes(S), s) != hipSuccess) return usseg_check_launch(who);
  tk_select_launch(keys, S, (int)n, fraction, k, (int*)ws, sel, 0, 0xFFFFFFFFu, s);
  return usseg_check_launch(who);
}

struct TkWs { float* l; int* hist; int* sel; int S, n; };
static TkWs tk_ws(const UssegLossDesc* d, int scope, void* ws) {
  TkWs w;
  w.S = scope ? (int)(d->M / d->HW) : 1;
  w.n = scope ? d->HW : (int)d->M;
  char* b = (char*)ws;
  w.l = (float*)b;
  w.hist = (int*)(b + tk_align256(d->M * 4));
  w.sel = (int*)(b + tk_align256(d->M * 4) + tk_align256(usseg_topk_select_ws_bytes(w.S)));
  return w;
}

static int topk_args(const char* who, const UssegLossDesc* d, const UssegTopkLoss* tk, const void* ws, int64_t ws_bytes) {
  USSEG_CHECK_ARG(d, "%s: null descriptor", who);
  int rc = region_shape_args(who, d);
  if (rc) return rc;
  USSEG_CHECK_ARG(std::isfinite(tk->tk_weight) && tk->tk_weight >= 0.f, "%s: tk_weight must be finite and >= 0", who);
  USSEG_CHECK_ARG(tk->scope == 0 || tk->scope == 1, "%s: scope must be 0 (batch) or 1 (image)", who);
  if ((rc = region_scale_args(who, d, 1.f))) return rc;
  if (d->M == 0) return USSEG_OK;
  USSEG_CHECK_ARG(ws && ((uintptr_t)ws & 15) == 0, "%s: the workspace must be a 16-byte aligned pointer", who);
  USSEG_CHECK_ARG(ws_bytes >= usseg_topk_ws_bytes(d->M, d->HW, tk->scope), "%s: the workspace holds %lld bytes, %lld needed", who, (long long)ws_bytes,
                  (long long)usseg_topk_ws_bytes(d->M, d->HW, tk->scope));
  return USSEG_OK;
}

extern "C" int usseg_topk_pixel_loss(const UssegLossDesc* d, UssegTopkLoss tk, const float* fraction, const float* probs, const float* y_true, void* ws,
                                     int64_t ws_bytes, usseg_stream_t stream) {
  const char* who = "topk_pixel_loss";
  const int rc = topk_args(who, d, &tk, ws, ws_bytes);
  if (rc) return rc;
  USSEG_CHECK_ARG(fraction && ((uintptr_t)fraction & 3) == 0, "%s: fraction must be a 4-byte aligned device pointer", who);
  USSEG_CHECK_ARG(probs && y_true, "%s: null pointer", who);
  USSEG_CHECK_ARG((((uintptr_t)probs | (uintptr_t)y_true) & 15) == 0, "%s: probs and y_true must be 16-byte aligned", who);
  if (d->M == 0) return USSEG_OK;
  const TkWs w = tk_ws(d, tk.scope, ws);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(w.hist, 0, (size_t)usseg_topk_select_ws_bytes(w.S), s) != hipSuccess) return usseg_check_launch(who);
  const int M = (int)d->M, ng = region_groups(d);
  const int64_t tiles = cdiv64(ng, 256);
  const int64_t per = cdiv64(tiles, 1024);          // tiles of 256 groups a workgroup owns: at most 1024 workgroups, none of them empty
  const int grid = (int)cdiv64(tiles, per), chunk = (int)(per * 256);
#define TK_PIX(CC) \
  hipLaunchKernelGGL(topk_pixel_loss_kernel<CC>, dim3(grid), dim3(256), 0, s, probs, y_true, w.l, w.hist, M, ng, chunk, w.n, d->label_smoothing, d->clip_eps)
  switch (d->C) {
    case 1: TK_PIX(1); break;
    case 2: TK_PIX(2); break;
    case 3: TK_PIX(3); break;
    default: TK_PIX(4); break;
  }
#undef TK_PIX
  tk_select_launch((const unsigned*)w.l, w.S, w.n, fraction, 0, w.hist, w.sel, 1, 0x7FFFFFFFu, s);
  return usseg_check_launch(who);
}

extern "C" int usseg_topk_loss_sums(const UssegLossDesc* d, UssegTopkLoss tk, const void* ws, int64_t ws_bytes, const float* overlap_acc, float* acc,
                                    int64_t acc_floats, usseg_stream_t stream) {
  const char* who = "topk_loss_sums";
  const int rc = topk_args(who, d, &tk, ws, ws_bytes);
  if (rc) return rc;
  USSEG_CHECK_ARG(acc && ((uintptr_t)acc & 3) == 0, "%s: acc must be a 4-byte aligned pointer", who);
  USSEG_CHECK_ARG(((uintptr_t)overlap_acc & 3) == 0 && overlap_acc != acc, "%s: overlap_acc must be a 4-byte aligned pointer other than acc", who);
  const int grid = usseg_overlap_loss_grid(d->M);
  USSEG_CHECK_ARG(grid <= REGION_MAX_BLOCKS && acc_floats >= REGION_HDR + (int64_t)REGION_STRIDE * grid,
                  "%s: a grid of %d workgroups needs %d accumulator floats", who, grid, REGION_HDR + REGION_STRIDE * grid);
  TkWs w = {};
  if (d->M > 0) w = tk_ws(d, tk.scope, const_cast<void*>(ws));
  else w.n = 1;
  hipLaunchKernelGGL(topk_sums_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w.l, w.sel, overlap_acc, acc, (int)d->M, region_groups(d), w.n,
                     tk.tk_weight * d->inv_global_batch);
  return usseg_check_launch(who);
}

extern "C" int usseg_topk_loss_bwd(const UssegLossDesc* d, UssegTopkLoss tk, const float* probs, const float* y_true, const void* ws, int64_t ws_bytes,
                                   const float* acc, int64_t acc_floats, const float* overlap_acc, void* dlogits, usseg_stream_t stream) {
  const char* who = "topk_loss_bwd";
  int rc = topk_args(who, d, &tk, ws, ws_bytes);
  if (rc) return rc;
  USSEG_CHECK_ARG(probs && y_true, "%s: null pointer", who);
  USSEG_CHECK_ARG((((uintptr_t)probs | (uintptr_t)y_true) & 15) == 0, "%s: probs and y_true must be 16-byte aligned", who);
  USSEG_CHECK_ARG(acc && ((uintptr_t)acc & 3) == 0 && acc_floats >= REGION_HDR, "%s: acc must hold its %d header floats", who, REGION_HDR);
  USSEG_CHECK_ARG(((uintptr_t)overlap_acc & 3) == 0, "%s: overlap_acc must be a 4-byte aligned pointer", who);
  if ((rc = region_bwd_args(who, d, dlogits))) return rc;
  if (d->M == 0) return USSEG_OK;
  const TkWs w = tk_ws(d, tk.scope, const_cast<void*>(ws));
  const int M = (int)d->M, ng = region_groups(d);
  const dim3 grid = region_bwd_grid(ng);
  bf16_t* dl = (bf16_t*)dlogits;
  hipStream_t s = (hipStream_t)stream;
#define TK_BWD2(CC, Q, OV)                                                                                                                        \
  hipLaunchKernelGGL((topk_bwd_kernel<CC, Q, OV>), grid, dim3(256), 0, s, probs, y_true, w.l, w.sel, acc, overlap_acc, dl, M, ng, w.n, d->HW, \
                     d->quad_w ? d->quad_w : 1, d->label_smoothing, d->clip_eps)
#define TK_BWD(CC)                                                                          \
  if (overlap_acc) { if (d->quad_w) TK_BWD2(CC, true, true); else TK_BWD2(CC, false, true); } \
  else { if (d->quad_w) TK_BWD2(CC, true, false); else TK_BWD2(CC, false, false); }
  switch (d->C) {
    case 1: TK_BWD(1) break;
    case 2: TK_BWD(2) break;
    case 3: TK_BWD(3) break;
    default: TK_BWD(4) break;
  }
#undef TK_BWD
#undef TK_BWD2
  return usseg_check_launch(who);
}
