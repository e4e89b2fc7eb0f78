// Exact Euclidean distance maps on the device (usseg.h: usseg_sdf_labels, usseg_surface_dist, usseg_surface_stats): the signed distance map of the
// labels for the boundary loss, and the surface-to-surface distances behind the Hausdorff / average-symmetric-surface-distance scores, their
// percentiles (HD95) and the surface Dice at a tolerance.
// One transform, two uses.  A plane is a [H][W] binary image; every pixel wants the squared distance to the nearest pixel of a TARGET set.
//   row pass     sdf_row_kernel: one wave per image row.  The lanes ballot 64 pixels at a time into a bit row in LDS; a pixel then finds the
//                nearest set (or clear) bit to its left and right with clz / ffs over at most ceil(W/64) words.  It writes g, the distance
//                along the row to the nearest target pixel (0xFFFF: the row holds none), for TWO target sets packed in one uint32 per pixel:
//                labels   lo = mask, hi = complement of the mask, per class ([B][H][W][C], the layout of y_true), plus one byte per (row, class)
//                         that says whether the row holds a mask pixel (bit 0) and a non-mask pixel (bit 1);
//                surfaces lo = S(a), hi = S(b) ([N][H][W]).
//                g == 0 says the pixel itself is in the set, so the second pass needs no other input.
//   column pass  min over rows r of (y-r)^2 + g(r, x)^2, scanning outward from the pixel's own row and stopping once dy^2 >= best: exact, every
//                loop bounded by H, all int32 (g <= 8191, dy <= 8191: at most 2 * 8191^2 < 2^27).  Lanes of a wave read neighbouring (x, c) of
//                the same row: coalesced, and served by L2 (the intermediate of 16 x 256 x 80 x 3 is 3.9 MB).
//                sdf_col_kernel   one thread per (pixel, class): a pixel outside the mask asks for the mask, a pixel inside for the complement;
//                                 a plane WITHOUT the asked-for set (class absent, or class filling the plane) gives phi = 0 - the row bytes,
//                                 OR-ed over the plane by the workgroup, say so before any scan starts.
//                sdf_surface_kernel   one workgroup per (image, direction): counts both surfaces, then each thread walks its pixels in index
//                                 order (max of d^2 in int32, sum of sqrt in fp64) and the workgroup adds the 256 partial sums as a fixed
//                                 tree - bitwise reproducible, no float atomics.
//                sdf_plane_kernel     (usseg_surface_stats) one thread per pixel over all images: the squared distance of every surface pixel to the
//                                 other surface into an int32 [N][2][H][W] plane, for the selection that follows.
//   selection    sdf_select_kernel    one workgroup per (image, set): sdf_surface_kernel's counters and sums again, from the plane, in the same order
//                                 (the same bits), the counts within each tolerance, and an integer radix select of the asked-for ranks - most
//                                 significant digit first, 8-bit digits, a 256-bin histogram in LDS per distinct prefix, four levels.
// phi =the fp64 value - the square root of the exact integer, 1 minus it inside the mask - rounded ONCE to fp32: outside the mask that is the
// correctly rounded fp32 root for every integer below 2^31.
// Nothing here allocates; the intermediate lives in the caller's workspace (usseg_sdf_ws_bytes / usseg_surface_ws_bytes / usseg_surface_stats_ws_bytes).
#include "common.h"
#include <cmath>

#define SDF_INF 0xFFFFu
#define SDF_MAX_DIM 8192
#define SDF_MAX_WORDS (SDF_MAX_DIM / 64)

// distance along the row from x to the nearest set bit of m (inv: the nearest CLEAR bit among the W valid ones), SDF_INF if there is none.
// Both loops run over at most nw words.
__device__ __forceinline__ unsigned sdf_row_near(const uint64_t* m, int nw, int W, int x, bool inv) {
  const int w0 = x >> 6, b0 = x & 63;
  const uint64_t tail = (W & 63) ? ((1ull << (W & 63)) - 1ull) : ~0ull;      // valid bits of the last word
  unsigned best = SDF_INF;
  for (int w = w0; w >= 0; --w) {
    uint64_t v = inv ? ~m[w] : m[w];
    if (w == nw - 1) v &= tail;
    if (w == w0) v &= (2ull << b0) - 1ull;                                     // bits <= b0 (b0 = 63: 2 << 63 wraps to 0, minus 1 = all)
    if (v) { best = (unsigned)(x - (w * 64 + 63 - __clzll((long long)v))); break; }
  }
  for (int w = w0; w < nw; ++w) {
    uint64_t v = inv ? ~m[w] : m[w];
    if (w == nw - 1) v &= tail;
    if (w == w0) v &= ~0ull << b0;                                             // bits >= b0
    if (v) {
      const unsigned d = (unsigned)(w * 64 + __ffsll((unsigned long long)v) - 1 - x);
      best = d < best ? d : best;
      break;
    }
  }
  return best;
}

// SURF = false: y [rows][W][C] fp32 labels, set s = class s, inside = y > thr (NaN compares false: outside).
// SURF = true:  a, b [rows][W] uint8 masks, set 0 = S(a), set 1 = S(b): a mask pixel with a 4-neighbour outside the mask or outside the image.
template <bool SURF>
__global__ __launch_bounds__(256) void sdf_row_kernel(const float* __restrict__ y, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, float thr,
                                                      uint32_t* __restrict__ g, uint8_t* __restrict__ rowflags, int rows, int H, int W, int C) {
  __shared__ uint64_t bits[4][4][SDF_MAX_WORDS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  const bool live = row < rows;
  const int nw = (W + 63) >> 6;
  const int NS = SURF ? 2 : C;
  const int yy = live ? row % H : 0;
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    const bool px = live && x < W;
    for (int s = 0; s < NS; ++s) {
      bool in = false;
      if (px) {
        if (SURF) {
          const uint8_t* m = (s ? b : a) + (int64_t)row * W;
          if (m[x]) {
            const bool up = yy > 0 && m[x - W], dn = yy < H - 1 && m[x + W];
            const bool lf = x > 0 && m[x - 1], rt = x < W - 1 && m[x + 1];
            in = !(up && dn && lf && rt);
          }
        } else {
          in = y[((int64_t)row * W + x) * C + s] > thr;
        }
      }
      const uint64_t bal = __ballot(in);
      if (lane == 0) bits[wave][s][w] = bal;
    }
  }
  __syncthreads();
  if (!live) return;
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    if (x >= W) break;
    if (SURF) {
      const unsigned ga = sdf_row_near(bits[wave][0], nw, W, x, false), gb = sdf_row_near(bits[wave][1], nw, W, x, false);
      g[(int64_t)row * W + x] = ga | (gb << 16);
    } else {
      for (int s = 0; s < NS; ++s) {
        const unsigned gm = sdf_row_near(bits[wave][s], nw, W, x, false), gn = sdf_row_near(bits[wave][s], nw, W, x, true);
        g[((int64_t)row * W + x) * C + s] = gm | (gn << 16);
        if (x == 0) rowflags[(int64_t)row * 4 + s] = (uint8_t)((gm != SDF_INF ? 1 : 0) | (gn != SDF_INF ? 2 : 0));
      }
    }
  }
}

// min over the rows r of (yy - r)^2 + g(r)^2 with g = (word >> shift) & 0xFFFF read at p[r * stride]; -1 if no row holds a target.
__device__ __forceinline__ int sdf_col_scan(const uint32_t* __restrict__ p, int64_t stride, int yy, int H, int shift) {
  int best = 0x7fffffff;
  {
    const unsigned g0 = (p[(int64_t)yy * stride] >> shift) & 0xFFFFu;
    if (g0 != SDF_INF) best = (int)(g0 * g0);
  }
  for (int dy = 1; dy < H; ++dy) {
    const int d2 = dy * dy;
    if (d2 >= best) break;
    const int r0 = yy - dy, r1 = yy + dy;
    if (r0 < 0 && r1 >= H) break;
    const unsigned u0 = r0 >= 0 ? (p[(int64_t)r0 * stride] >> shift) & 0xFFFFu : SDF_INF;
    const unsigned u1 = r1 < H ? (p[(int64_t)r1 * stride] >> shift) & 0xFFFFu : SDF_INF;
    const unsigned u = u0 < u1 ? u0 : u1;
    if (u != SDF_INF) {
      const int cand = d2 + (int)(u * u);
      best = cand < best ? cand : best;
    }
  }
  return best == 0x7fffffff ? -1 : best;
}

// grid (ceil(W*C / 256), H, B): thread = one (x, c) of row blockIdx.y of image blockIdx.z
__global__ __launch_bounds__(256) void sdf_col_kernel(const uint32_t* __restrict__ g, const uint8_t* __restrict__ rowflags, float* __restrict__ phi, int H,
                                                      int W, int C) {
  const int bimg = blockIdx.z, yy = blockIdx.y;
  // which sets the planes of this image hold: byte c of `have` = OR over the rows of rowflags[row][c]
  __shared__ unsigned s_have;
  if (threadIdx.x == 0) s_have = 0u;
  __syncthreads();
  unsigned have = 0u;
  const uint32_t* rf = reinterpret_cast<const uint32_t*>(rowflags) + (int64_t)bimg * H;
  for (int r = threadIdx.x; r < H; r += 256) have |= rf[r];
  for (int msk = 32; msk >= 1; msk >>= 1) have |= (unsigned)__shfl_xor((int)have, msk, 64);
  if ((threadIdx.x & 63) == 0 && have) atomicOr(&s_have, have);      // (an integer OR in LDS: the order does not matter)
  __syncthreads();
  have = s_have;
  const int j = blockIdx.x * 256 + threadIdx.x, WC = W * C;
  if (j >= WC) return;
  const int c = j % C;
  const uint32_t* col = g + (int64_t)bimg * H * WC + j;
  const bool inside = (col[(int64_t)yy * WC] & 0xFFFFu) == 0u;
  float out = 0.f;
  if ((have >> (8 * c)) & (inside ? 2u : 1u)) {
    const int d2 = sdf_col_scan(col, WC, yy, H, inside ? 16 : 0);
    const double d = sqrt((double)(d2 < 0 ? 0 : d2));
    out = (float)(inside ? 1.0 - d : d);          // ONE rounding to fp32, of the fp64 value
  }
  phi[((int64_t)bimg * H + yy) * WC + j] = out;
}

// grid (2, N): direction 0 = S(a) -> S(b), 1 = S(b) -> S(a)
__global__ __launch_bounds__(256) void sdf_surface_kernel(const uint32_t* __restrict__ g, int64_t* __restrict__ counters, double* __restrict__ sums, int H, int W) {
  __shared__ int64_t cnt[2][256];
  __shared__ double red[256];
  __shared__ int mxs[256];
  const int dir = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const int HW = H * W;
  const uint32_t* p = g + (int64_t)n * HW;
  int64_t ca = 0, cb = 0;
  for (int i = tid; i < HW; i += 256) {
    const uint32_t u = p[i];
    ca += (u & 0xFFFFu) == 0u;
    cb += (u >> 16) == 0u;
  }
  cnt[0][tid] = ca; cnt[1][tid] = cb;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) { cnt[0][tid] += cnt[0][tid + s]; cnt[1][tid] += cnt[1][tid + s]; }
    __syncthreads();
  }
  const int64_t na = cnt[0][0], nb = cnt[1][0];
  if (dir == 0 && tid == 0) { counters[4 * n] = na; counters[4 * n + 1] = nb; }
  if (na == 0 || nb == 0) {
    if (tid == 0) { counters[4 * n + 2 + dir] = -1; sums[2 * n + dir] = 0.0; }
    return;
  }
  const int src = dir ? 16 : 0, tgt = dir ? 0 : 16;
  double s = 0.0;
  int mx = -1;
  for (int i = tid; i < HW; i += 256) {
    if (((p[i] >> src) & 0xFFFFu) != 0u) continue;
    const int yy = i / W, xx = i - yy * W;
    const int d2 = sdf_col_scan(p + xx, W, yy, H, tgt);      // (>= 0: the target surface is not empty)
    mx = d2 > mx ? d2 : mx;
    s += sqrt((double)d2);
  }
  red[tid] = s; mxs[tid] = mx;
  __syncthreads();
  for (int k = 128; k >= 1; k >>= 1) {                        // a fixed tree: the same bits on every run
    if (tid < k) { red[tid] += red[tid + k]; mxs[tid] = mxs[tid] > mxs[tid + k] ? mxs[tid] : mxs[tid + k]; }
    __syncthreads();
  }
  if (tid == 0) { counters[4 * n + 2 + dir] = mxs[0]; sums[2 * n + dir] = red[0]; }
}

// ---- surface statistics (usseg.h: usseg_surface_stats): the distances materialised, then an exact integer radix select ------------------
// plane int32 [N][2][H][W]: [n][0] = squared distance from a pixel of S(a) to S(b), [n][1] = from a pixel of S(b) to S(a); SDF_NOT_SOURCE
// where the pixel is not on the source surface, -1 (sdf_col_scan's) where it is and the target surface is empty.
#define SDF_NOT_SOURCE (-2)
#define SDF_MAX_Q 4
#define SDF_MAX_RANKS (2 * SDF_MAX_Q)
#define SDF_SEL_THREADS 1024          // sdf_select_kernel's workgroup: the first 256 threads are sdf_surface_kernel's, all of them fill the histograms

struct SurfStatsArgs {                 // by value in the kernel arguments: a captured graph holds them
  double quant[SDF_MAX_Q];
  int32_t tol2[SDF_MAX_Q];
  int32_t P, T;
};

// grid (ceil(H*W / 256), N): thread = one pixel, lanes along x
__global__ __launch_bounds__(256) void sdf_plane_kernel(const uint32_t* __restrict__ g, int32_t* __restrict__ plane, int H, int W) {
  const int n = blockIdx.y, HW = H * W;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const uint32_t* p = g + (int64_t)n * HW;
  const uint32_t u = p[i];
  const int yy = i / W, xx = i - yy * W;
  int dab = SDF_NOT_SOURCE, dba = SDF_NOT_SOURCE;
  if ((u & 0xFFFFu) == 0u) dab = sdf_col_scan(p + xx, W, yy, H, 16);
  if ((u >> 16) == 0u) dba = sdf_col_scan(p + xx, W, yy, H, 0);
  int32_t* out = plane + (int64_t)n * 2 * HW;
  out[i] = dab;
  out[HW + i] = dba;
}

// one more count in bin `bin` of h for every lane with `match`; the lanes that agree with the first matching lane share one atomic (a surface
// that lies on the other one is all zeros).  Called by whole waves.
__device__ __forceinline__ void sdf_hist_add(int* h, int bin, bool match, int lane) {
  const uint64_t m = __ballot(match);
  if (!m) return;
  const int first = __shfl(bin, __ffsll((unsigned long long)m) - 1, 64);
  const uint64_t same = __ballot(match && bin == first);
  if (!match) return;
  if (bin != first) atomicAdd(&h[bin], 1);
  else if (lane == __ffsll((unsigned long long)same) - 1) atomicAdd(&h[first], __popcll(same));
}

// grid (P ? 3 : 2, N): set 0 = D_ab, 1 = D_ba, 2 = their union.  Sets 0 and 1 also give usseg_surface_dist's counters and sums of their
// direction - sdf_surface_kernel's per-thread index order and tree, on the first 256 threads - and the counts within each tolerance.
__global__ __launch_bounds__(SDF_SEL_THREADS) void sdf_select_kernel(const int32_t* __restrict__ plane, SurfStatsArgs A, int64_t* __restrict__ counters,
                                                         double* __restrict__ sums, int32_t* __restrict__ sel, int64_t* __restrict__ within, int H, int W) {
  __shared__ int hist[SDF_MAX_RANKS][256];
  __shared__ double red[256];
  __shared__ int mxs[256];
  __shared__ int s_cnt[2], s_within[SDF_MAX_Q];
  __shared__ int s_prefix[SDF_MAX_RANKS], s_rem[SDF_MAX_RANKS], s_owner[SDF_MAX_RANKS], s_uniq[SDF_MAX_RANKS], s_nu;
  const int set = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HW = H * W;
  const int32_t* pl = plane + (int64_t)n * 2 * HW;
  if (tid < 2) s_cnt[tid] = 0;
  if (tid < SDF_MAX_Q) s_within[tid] = 0;
  __syncthreads();
  {
    int ca = 0, cb = 0;
    for (int i = tid; i < HW; i += SDF_SEL_THREADS) {
      ca += pl[i] != SDF_NOT_SOURCE;
      cb += pl[HW + i] != SDF_NOT_SOURCE;
    }
    for (int msk = 32; msk >= 1; msk >>= 1) { ca += __shfl_xor(ca, msk, 64); cb += __shfl_xor(cb, msk, 64); }
    if (lane == 0) { atomicAdd(&s_cnt[0], ca); atomicAdd(&s_cnt[1], cb); }
  }
  __syncthreads();
  const int na = s_cnt[0], nb = s_cnt[1];
  const bool empty = na == 0 || nb == 0;
  if (set == 0 && tid == 0) { counters[4 * n] = na; counters[4 * n + 1] = nb; }
  if (set < 2) {
    const int32_t* e = pl + (int64_t)set * HW;
    double s = 0.0;
    int mx = -1, wc[SDF_MAX_Q] = {0, 0, 0, 0};
    if (!empty && tid < 256) {
      for (int i = tid; i < HW; i += 256) {
        const int d2 = e[i];
        if (d2 < 0) continue;
        mx = d2 > mx ? d2 : mx;
        s += sqrt((double)d2);
#pragma unroll
        for (int t = 0; t < SDF_MAX_Q; ++t) wc[t] += (t < A.T && d2 <= A.tol2[t]) ? 1 : 0;
      }
    }
    if (tid < 256) { red[tid] = s; mxs[tid] = mx; }
    __syncthreads();
    for (int k = 128; k >= 1; k >>= 1) {                        // sdf_surface_kernel's tree
      if (tid < k) { red[tid] += red[tid + k]; mxs[tid] = mxs[tid] > mxs[tid + k] ? mxs[tid] : mxs[tid + k]; }
      __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < SDF_MAX_Q; ++t) {
      int v = wc[t];
      for (int msk = 32; msk >= 1; msk >>= 1) v += __shfl_xor(v, msk, 64);
      if (lane == 0 && v) atomicAdd(&s_within[t], v);
    }
    __syncthreads();
    if (tid == 0) { counters[4 * n + 2 + set] = empty ? -1 : mxs[0]; sums[2 * n + set] = empty ? 0.0 : red[0]; }
    if (tid < A.T) within[((int64_t)n * A.T + tid) * 2 + set] = s_within[tid];
  }
  const int P = A.P, R = 2 * P;
  if (P == 0) return;
  int32_t* out = sel + ((int64_t)n * 3 + set) * P * 2;
  if (empty) {
    if (tid < R) out[tid] = -1;
    return;
  }
  const int32_t* e = pl + (set == 1 ? HW : 0);
  const int len = set == 2 ? 2 * HW : HW;
  const int cnt = set == 0 ? na : set == 1 ? nb : na + nb;
  if (tid < R) {
    double t = A.quant[0];                                      // (constant indices: the argument struct stays in registers)
#pragma unroll
    for (int p = 1; p < SDF_MAX_Q; ++p) t = (tid >> 1) == p ? A.quant[p] : t;
    const double pos = t * (double)(cnt - 1);
    int k = (int)floor(pos);
    if (tid & 1) k = k + 1 < cnt - 1 ? k + 1 : cnt - 1;
    s_prefix[tid] = 0; s_rem[tid] = k; s_owner[tid] = 0;
  }
  if (tid == 0) { s_nu = 1; s_uniq[0] = 0; }
  __syncthreads();
  for (int shift = 24; shift >= 0; shift -= 8) {
    const int nu = s_nu;
    for (int j = tid; j < nu * 256; j += SDF_SEL_THREADS) (&hist[0][0])[j] = 0;
    __syncthreads();
    for (int base = 0; base < len; base += 4 * SDF_SEL_THREADS) {      // four loads in flight; most of the plane is not a source
      int xs[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = base + j * SDF_SEL_THREADS + tid;
        xs[j] = i < len ? e[i] : -1;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = xs[j];
        if (!__ballot(x >= 0)) continue;                                // (the whole wave)
        const int hi = shift == 24 ? 0 : x >> (shift + 8);
        const int bin = (x >> shift) & 255;
        for (int u = 0; u < nu; ++u) sdf_hist_add(hist[u], bin, x >= 0 && hi == s_uniq[u], lane);
      }
    }
    __syncthreads();
    // the bin that holds rank s_rem[r] among the values under s_prefix[r]: a wave per rank, four bins per lane
    for (int r = wave; r < R; r += SDF_SEL_THREADS / 64) {
      const int* h = hist[s_owner[r]];
      const int rem = s_rem[r];
      const int b0 = h[4 * lane], b1 = h[4 * lane + 1], b2 = h[4 * lane + 2], b3 = h[4 * lane + 3];
      const int mine = b0 + b1 + b2 + b3;
      int incl = mine;
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
      }
      const int excl = incl - mine;
      if (excl <= rem && rem < incl) {
        int q = rem - excl, b = 0;
        if (q >= b0) { q -= b0; b = 1; if (q >= b1) { q -= b1; b = 2; if (q >= b2) { q -= b2; b = 3; } } }
        s_prefix[r] = (s_prefix[r] << 8) | (4 * lane + b);
        s_rem[r] = q;
      }
    }
    __syncthreads();
    if (tid == 0) {                                             // ranks whose prefixes agree share the next level's histogram
      int m = 0;
      for (int r = 0; r < R; ++r) {
        int o = -1;
        for (int u = 0; u < m; ++u) if (s_uniq[u] == s_prefix[r]) o = u;
        if (o < 0) { o = m; s_uniq[m++] = s_prefix[r]; }
        s_owner[r] = o;
      }
      s_nu = m;
    }
    __syncthreads();
  }
  if (tid < R) out[tid] = s_prefix[tid];
}

// ---- entry points: every argument is checked before any launch ------------------------------------------------------------------------
static inline int64_t round16(int64_t v) { return (v + 15) / 16 * 16; }

extern "C" int64_t usseg_sdf_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t C) {
  if (B < 0 || H < 1 || W < 1 || C < 1 || C > 4 || H > SDF_MAX_DIM || W > SDF_MAX_DIM) return -1;
  return round16((int64_t)4 * B * H * W * C) + round16((int64_t)4 * B * H);
}

extern "C" int64_t usseg_surface_ws_bytes(int32_t N, int32_t H, int32_t W) {
  if (N < 0 || H < 1 || W < 1 || H > SDF_MAX_DIM || W > SDF_MAX_DIM) return -1;
  return round16((int64_t)4 * N * H * W);
}

extern "C" int usseg_sdf_labels(const float* y_true, int32_t B, int32_t H, int32_t W, int32_t C, float thr, float* phi, void* ws, int64_t ws_bytes,
                                usseg_stream_t stream) {
  USSEG_CHECK_ARG(H >= 1 && H <= SDF_MAX_DIM && W >= 1 && W <= SDF_MAX_DIM, "sdf_labels: H and W must lie in [1, %d], got %d x %d", SDF_MAX_DIM, H, W);
  USSEG_CHECK_ARG(C >= 1 && C <= 4, "sdf_labels: 1 <= C <= 4");
  USSEG_CHECK_ARG(B >= 0 && B <= 65535, "sdf_labels: 0 <= B <= 65535");
  USSEG_CHECK_ARG((int64_t)B * H * W <= (1 << 29), "sdf_labels: more than 2^29 pixels");
  USSEG_CHECK_ARG(!std::isnan(thr), "sdf_labels: the threshold is NaN");
  USSEG_CHECK_ARG(y_true && phi && ws, "sdf_labels: null pointer");
  USSEG_CHECK_ARG(((uintptr_t)y_true & 3) == 0 && ((uintptr_t)phi & 3) == 0 && ((uintptr_t)ws & 15) == 0,
                  "sdf_labels: y_true and phi must be 4-byte, the workspace 16-byte aligned");
  USSEG_CHECK_ARG(ws_bytes >= usseg_sdf_ws_bytes(B, H, W, C), "sdf_labels: the workspace holds %lld bytes, %lld needed", (long long)ws_bytes,
                  (long long)usseg_sdf_ws_bytes(B, H, W, C));
  if (B == 0) return USSEG_OK;
  uint32_t* g = (uint32_t*)ws;
  uint8_t* rowflags = (uint8_t*)ws + round16((int64_t)4 * B * H * W * C);
  hipStream_t s = (hipStream_t)stream;
  const int rows = B * H;
  hipLaunchKernelGGL((sdf_row_kernel<false>), dim3((rows + 3) / 4), dim3(256), 0, s, y_true, (const uint8_t*)nullptr, (const uint8_t*)nullptr, thr, g, rowflags,
                     rows, H, W, C);
  hipLaunchKernelGGL(sdf_col_kernel, dim3((W * C + 255) / 256, H, B), dim3(256), 0, s, (const uint32_t*)g, (const uint8_t*)rowflags, phi, H, W, C);
  return usseg_check_launch("sdf_labels");
}

extern "C" int usseg_surface_dist(const uint8_t* a, const uint8_t* b, int32_t N, int32_t H, int32_t W, int64_t* counters, double* sums, void* ws,
                                  int64_t ws_bytes, usseg_stream_t stream) {
  USSEG_CHECK_ARG(H >= 1 && H <= SDF_MAX_DIM && W >= 1 && W <= SDF_MAX_DIM, "surface_dist: H and W must lie in [1, %d], got %d x %d", SDF_MAX_DIM, H, W);
  USSEG_CHECK_ARG(N >= 0 && N <= 65535, "surface_dist: 0 <= N <= 65535");
  USSEG_CHECK_ARG((int64_t)N * H * W <= (1 << 29), "surface_dist: more than 2^29 pixels");
  USSEG_CHECK_ARG(a && b && counters && sums && ws, "surface_dist: null pointer");
  USSEG_CHECK_ARG(((uintptr_t)counters & 7) == 0 && ((uintptr_t)sums & 7) == 0 && ((uintptr_t)ws & 15) == 0,
                  "surface_dist: counters and sums must be 8-byte, the workspace 16-byte aligned");
  USSEG_CHECK_ARG(ws_bytes >= usseg_surface_ws_bytes(N, H, W), "surface_dist: the workspace holds %lld bytes, %lld needed", (long long)ws_bytes,
                  (long long)usseg_surface_ws_bytes(N, H, W));
  if (N == 0) return USSEG_OK;
  uint32_t* g = (uint32_t*)ws;
  hipStream_t s = (hipStream_t)stream;
  const int rows = N * H;
  hipLaunchKernelGGL((sdf_row_kernel<true>), dim3((rows + 3) / 4), dim3(256), 0, s, (const float*)nullptr, a, b, 0.f, g, (uint8_t*)nullptr, rows, H, W, 1);
  hipLaunchKernelGGL(sdf_surface_kernel, dim3(2, N), dim3(256), 0, s, (const uint32_t*)g, counters, sums, H, W);
  return usseg_check_launch("surface_dist");
}

extern "C" int64_t usseg_surface_stats_ws_bytes(int32_t N, int32_t H, int32_t W) {
  if (N < 0 || H < 1 || W < 1 || H > SDF_MAX_DIM || W > SDF_MAX_DIM) return -1;
  return round16((int64_t)4 * N * H * W) + round16((int64_t)8 * N * H * W);      // g, then the plane of squared distances
}

extern "C" int usseg_surface_stats(const uint8_t* a, const uint8_t* b, int32_t N, int32_t H, int32_t W, const double* quant, int32_t P, const int32_t* tol2,
                                   int32_t T, int64_t* counters, double* sums, int32_t* sel, int64_t* within, void* ws, int64_t ws_bytes,
                                   usseg_stream_t stream) {
  USSEG_CHECK_ARG(H >= 1 && H <= SDF_MAX_DIM && W >= 1 && W <= SDF_MAX_DIM, "surface_stats: H and W must lie in [1, %d], got %d x %d", SDF_MAX_DIM, H, W);
  USSEG_CHECK_ARG(N >= 0 && N <= 65535, "surface_stats: 0 <= N <= 65535");
  USSEG_CHECK_ARG((int64_t)N * H * W <= (1 << 29), "surface_stats: more than 2^29 pixels");
  USSEG_CHECK_ARG(P >= 0 && P <= SDF_MAX_Q, "surface_stats: 0 <= P <= %d quantiles, got %d", SDF_MAX_Q, P);
  USSEG_CHECK_ARG(T >= 0 && T <= SDF_MAX_Q, "surface_stats: 0 <= T <= %d tolerances, got %d", SDF_MAX_Q, T);
  USSEG_CHECK_ARG(a && b && counters && sums && ws && (P == 0 || (quant && sel)) && (T == 0 || (tol2 && within)), "surface_stats: null pointer");
  SurfStatsArgs A = {};
  for (int p = 0; p < P; ++p) {
    USSEG_CHECK_ARG(std::isfinite(quant[p]) && quant[p] >= 0.0 && quant[p] <= 1.0, "surface_stats: quantile %d must be finite and lie in [0, 1], got %.17g", p,
                    quant[p]);
    A.quant[p] = quant[p];
  }
  for (int t = 0; t < T; ++t) {
    USSEG_CHECK_ARG(tol2[t] >= 0, "surface_stats: squared tolerance %d must be >= 0, got %d", t, tol2[t]);
    A.tol2[t] = tol2[t];
  }
  A.P = P;
  A.T = T;
  USSEG_CHECK_ARG(((uintptr_t)counters & 7) == 0 && ((uintptr_t)sums & 7) == 0 && ((uintptr_t)within & 7) == 0 && ((uintptr_t)sel & 3) == 0 &&
                      ((uintptr_t)ws & 15) == 0,
                  "surface_stats: counters, sums and within must be 8-byte, sel 4-byte, the workspace 16-byte aligned");
  USSEG_CHECK_ARG(ws_bytes >= usseg_surface_stats_ws_bytes(N, H, W), "surface_stats: the workspace holds %lld bytes, %lld needed", (long long)ws_bytes,
                  (long long)usseg_surface_stats_ws_bytes(N, H, W));
  if (N == 0) return USSEG_OK;
  uint32_t* g = (uint32_t*)ws;
  int32_t* plane = (int32_t*)((uint8_t*)ws + round16((int64_t)4 * N * H * W));
  hipStream_t s = (hipStream_t)stream;
  const int rows = N * H;
  hipLaunchKernelGGL((sdf_row_kernel<true>), dim3((rows + 3) / 4), dim3(256), 0, s, (const float*)nullptr, a, b, 0.f, g, (uint8_t*)nullptr, rows, H, W, 1);
  hipLaunchKernelGGL(sdf_plane_kernel, dim3((H * W + 255) / 256, N), dim3(256), 0, s, (const uint32_t*)g, plane, H, W);
  hipLaunchKernelGGL(sdf_select_kernel, dim3(P ? 3 : 2, N), dim3(SDF_SEL_THREADS), 0, s, (const int32_t*)plane, A, counters, sums, sel, within, H, W);
  return usseg_check_launch("surface_stats");
}
