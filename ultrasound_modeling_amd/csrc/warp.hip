// Elastic and affine warp of a training batch (include/usseg.h, "elastic and affine warp"; not in the reference):
// random elastic deformation (Simard et al. 2003) with a small rotation, scale and translation, ahead of usseg_augment.  Two launches:
//   warp_blur_h_kernel   the random field u (generated from the sample's seed, or injected) of one [kTH + 2*radius] x kTW tile in LDS, blurred
//                        along H into the workspace - a tile generates each field value once for its kTH rows, not once per tap;
//   warp_gather_kernel   the blur along W, the source coordinate and the label per output pixel (one lane per pixel), then the bilinear gather with
//                        one lane per (pixel, channel) element: the four taps and the store are contiguous over the channels of neighbouring lanes.
// The displacement never leaves the chip unless disp_out is asked for.  All coordinate and interpolation arithmetic is fp64 with
// `#pragma clang fp contract(off)` (prep.hip, cone.hip, operating_point.hip): tests/warp_restatement.py follows it bit for bit.
// No allocation, no synchronisation, the sample table and the weights read from the device: graph-capture safe.
//
// Bytes at B=16 x 256x80x10 fp64: x is read (26 MB, the four taps of a pixel share cache lines) and written (26 MB) once; the workspace is 5.2 MB
// written and read (2r+1) times out of the caches; y 1.3 MB each way.  No fp32 VALU arithmetic in this file (it is not in NOPK_SRCS).
#include "common.h"

namespace {
constexpr int kThreads = 256;
constexpr int kTH = 32, kTW = 32;                                  // output rows x columns of a blur tile: 8 row groups x 32 lanes
constexpr int kTileRows = kTH + 2 * USSEG_WARP_MAX_RADIUS;         // 160 rows x 32 doubles = 40 KB of static LDS (the default limit is 64 KB)
constexpr int kGridCap = 4096;
static_assert(kThreads == kTW * 8 && kTH % 8 == 0, "warp_blur_h: a thread owns column tx of rows ty, ty + 8, ...");
static_assert((kTileRows * kTW + USSEG_WARP_MAX_RADIUS + 1) * sizeof(double) <= 64 * 1024, "warp_blur_h: the tile must fit the default static LDS limit");

enum : int32_t { kPixZero = 0, kPixCopy = 1, kPixInterp = 2 };     // WarpPix::mode; an interpolated pixel carries its tap mask in bits 4..7
struct WarpPix {
  double w00, w01, w10, w11;
  int64_t p00;              // pixel index (b*H + i0)*W + j0 of the upper-left tap; i0 or j0 may be -1: only the taps of `mode`'s mask are read
  int32_t mode, pad;
};
static_assert(kThreads * sizeof(WarpPix) <= 16 * 1024, "warp_gather: the pixel table");
}  // namespace

// Named outside the anonymous namespace: the profiler reports kernels of an anonymous namespace with an empty name.
//
// Tile t of n_tiles = 2*B * tiles_h * tiles_w (columns fastest, then rows, then (b, k)).  LDS row `row` holds image row i0 - radius + row.
__global__ __launch_bounds__(256) void warp_blur_h_kernel(const UssegWarpDesc d, const UssegWarpSample* __restrict__ samples,
                                                          const double* __restrict__ wts, const double* __restrict__ field,
                                                          double* __restrict__ ws, double* __restrict__ field_out, int tiles_h, int tiles_w,
                                                          int64_t n_tiles) {
#pragma clang fp contract(off)
  __shared__ double tile[kTileRows][kTW];
  __shared__ double w_s[USSEG_WARP_MAX_RADIUS + 1];
  const int r = d.radius;                                          // 0 <= r <= USSEG_WARP_MAX_RADIUS (checked by the entry point)
  for (int t = threadIdx.x; t <= r; t += kThreads) w_s[t] = wts[t];
  const int tx = threadIdx.x % kTW, ty = threadIdx.x / kTW;
  const int64_t plane = (int64_t)d.H * d.W;
  const int rows = kTH + 2 * r;                                    // <= kTileRows
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {      // (b, k) and the trip count depend on blockIdx alone: the barriers are uniform
    const int tw = (int)(t % tiles_w);
    const int64_t q = t / tiles_w;
    const int th = (int)(q % tiles_h);
    const int64_t bk = q / tiles_h;                                // < 2*B
    const int b = (int)(bk >> 1), k = (int)(bk & 1);
    const int i0 = th * kTH, j0 = tw * kTW;
    const int64_t base = bk * plane;                               // SAFETY: element (b, k, i, j) = base + i*W + j < 2*B*H*W, the size of ws / field / field_out
    const int active = samples[b].active;
    const uint64_t seed = samples[b].seed;
    if (!active) {                                                 // the sample is copied: its field is 0 and its workspace is never read
      if (field_out) {
#pragma unroll
        for (int g = 0; g < kTH / 8; ++g) {
          const int i = i0 + ty + 8 * g, j = j0 + tx;
          if (i < d.H && j < d.W) field_out[base + (int64_t)i * d.W + j] = 0.0;
        }
      }
      continue;
    }
    __syncthreads();                                               // the previous trip's readers are done (first trip: w_s is written)
    for (int idx = threadIdx.x; idx < rows * kTW; idx += kThreads) {
      const int row = idx / kTW, col = idx % kTW;                  // SAFETY: row < rows <= kTileRows, col < kTW
      const int gi = i0 - r + row, gj = j0 + col;
      double u = 0.0;
      if (gi >= 0 && gi < d.H && gj < d.W) {                       // SAFETY: only elements inside the image are read or written
        const int64_t e = (int64_t)gi * d.W + gj;
        if (field) {
          u = field[base + e];
        } else {
          const uint32_t h = aug_hash(seed * 0x9e3779b97f4a7c15ULL + (uint64_t)((int64_t)k * plane + e));
          u = (double)h * 0x1p-31 - 1.0;                           // exact: 32 bits
        }
        if (field_out && row >= r && row < r + kTH) field_out[base + e] = u;      // this tile's own rows
      }
      tile[row][col] = u;
    }
    __syncthreads();
    const int j = j0 + tx;
#pragma unroll
    for (int g = 0; g < kTH / 8; ++g) {
      const int li = ty + 8 * g, i = i0 + li;
      if (i < d.H && j < d.W) {
        double acc;
        if (r == 0) {
          acc = tile[li][tx];
        } else {
          const int lo = -r > -i ? -r : -i, hi = r < d.H - 1 - i ? r : d.H - 1 - i;       // taps inside the image
          acc = 0.0;
          for (int kk = lo; kk <= hi; ++kk) acc = acc + w_s[kk < 0 ? -kk : kk] * tile[li + r + kk][tx];   // SAFETY: 0 <= li + r + kk < rows
        }
        ws[base + (int64_t)i * d.W + j] = acc;
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void warp_gather_kernel(const UssegWarpDesc d, const UssegWarpSample* __restrict__ samples,
                                                          const double* __restrict__ wts, const double* __restrict__ ws, const T* __restrict__ x,
                                                          const float* __restrict__ y, T* __restrict__ x_out, float* __restrict__ y_out,
                                                          double* __restrict__ disp_out) {
#pragma clang fp contract(off)
  __shared__ WarpPix pix[kThreads];
  __shared__ double w_s[USSEG_WARP_MAX_RADIUS + 1];
  const int r = d.radius;
  for (int t = threadIdx.x; t <= r; t += kThreads) w_s[t] = wts[t];
  const int64_t plane = (int64_t)d.H * d.W, M = (int64_t)d.B * plane;            // M * C < 2^31 (checked by the entry point)
  const double Hd = (double)d.H, Wd = (double)d.W;
  for (int64_t m0 = (int64_t)blockIdx.x * kThreads; m0 < M; m0 += (int64_t)gridDim.x * kThreads) {   // uniform trip count: the barriers are uniform
    __syncthreads();                                               // the previous trip's readers of pix are done (first trip: w_s is written)
    const int64_t m = m0 + threadIdx.x;
    if (m < M) {
      const int b = (int)(m / plane);
      const int rem = (int)(m - (int64_t)b * plane);
      const int i = rem / d.W, j = rem - i * d.W;
      WarpPix p = {0.0, 0.0, 0.0, 0.0, 0, kPixCopy, 0};
      float lab;
      double disp[2] = {0.0, 0.0};
      if (!samples[b].active) {
        lab = y[m];
      } else {
        const UssegWarpSample s = samples[b];
        for (int k = 0; k < 2; ++k) {                              // the blur along W of the workspace row
          const double* row = ws + ((int64_t)b * 2 + k) * plane + (int64_t)i * d.W;
          double acc;
          if (r == 0) {
            acc = row[j];
          } else {
            const int lo = -r > -j ? -r : -j, hi = r < d.W - 1 - j ? r : d.W - 1 - j;     // SAFETY: 0 <= j + kk < W
            acc = 0.0;
            for (int kk = lo; kk <= hi; ++kk) acc = acc + w_s[kk < 0 ? -kk : kk] * row[j + kk];
          }
          disp[k] = s.alpha[k] * acc;
        }
        const double di = (double)i, dj = (double)j;
        const double src0 = ((s.aff[0] * di + s.aff[1] * dj) + s.aff[4]) + disp[0];
        const double src1 = ((s.aff[2] * di + s.aff[3] * dj) + s.aff[5]) + disp[1];
        // SAFETY: every range test is made in fp64 (a NaN compares false) BEFORE a double is converted to an integer.
        const double n0 = floor(src0 + 0.5), n1 = floor(src1 + 0.5);
        lab = 0.f;
        if (n0 >= 0.0 && n0 < Hd && n1 >= 0.0 && n1 < Wd) lab = y[(int64_t)b * plane + (int64_t)(int)n0 * d.W + (int)n1];
        p.mode = kPixZero;
        if (src0 > -1.0 && src0 < Hd && src1 > -1.0 && src1 < Wd) {
          const double fi = floor(src0), fj = floor(src1);         // -1 <= fi <= H-1, -1 <= fj <= W-1
          const double f0 = src0 - fi, f1 = src1 - fj;
          const int ti = (int)fi, tj = (int)fj;
          const double g0 = 1.0 - f0, g1 = 1.0 - f1;
          p.w00 = g0 * g1; p.w01 = g0 * f1; p.w10 = f0 * g1; p.w11 = f0 * f1;
          p.p00 = (int64_t)b * plane + (int64_t)ti * d.W + tj;
          const int r0 = ti >= 0, r1 = ti + 1 < d.H, c0 = tj >= 0, c1 = tj + 1 < d.W;
          p.mode = kPixInterp | ((r0 & c0) << 4) | ((r0 & c1) << 5) | ((r1 & c0) << 6) | ((r1 & c1) << 7);
        }
      }
      y_out[m] = lab;
      if (disp_out) {
        disp_out[((int64_t)b * 2) * plane + rem] = disp[0];
        disp_out[((int64_t)b * 2 + 1) * plane + rem] = disp[1];
      }
      pix[threadIdx.x] = p;
    }
    __syncthreads();
    const int64_t left = M - m0;
    const int npix = left < kThreads ? (int)left : kThreads;
    const int64_t e0 = m0 * d.C;
    for (int e = threadIdx.x; e < npix * d.C; e += kThreads) {     // SAFETY: e0 + e < M*C; pl < npix <= kThreads
      const int pl = e / d.C, c = e - pl * d.C;
      const WarpPix p = pix[pl];
      if (p.mode == kPixCopy) {
        x_out[e0 + e] = x[e0 + e];                                 // the bits, a NaN's payload included: no arithmetic, no conversion
      } else if (p.mode == kPixZero) {
        x_out[e0 + e] = (T)0.0;
      } else {                                                     // SAFETY: a tap is read only if the mask says it lies inside the image
        const int64_t a = p.p00 * d.C + c, dw = (int64_t)d.W * d.C;
        const double v00 = (p.mode & 0x10) ? (double)x[a] : 0.0;
        const double v01 = (p.mode & 0x20) ? (double)x[a + d.C] : 0.0;
        const double v10 = (p.mode & 0x40) ? (double)x[a + dw] : 0.0;
        const double v11 = (p.mode & 0x80) ? (double)x[a + dw + d.C] : 0.0;
        const double o = ((p.w00 * v00 + p.w01 * v01) + p.w10 * v10) + p.w11 * v11;
        x_out[e0 + e] = (T)o;                                      // rounded once
      }
    }
  }
}

extern "C" int64_t usseg_warp_ws_bytes(int32_t B, int32_t H, int32_t W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  return (int64_t)B * 2 * H * W * (int64_t)sizeof(double);         // the H-blurred field, [B][2][H][W]
}

static bool overlaps(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

extern "C" int usseg_elastic_warp(const UssegWarpDesc* d, const UssegWarpSample* samples_dev, const double* weights_dev, const double* field,
                                  const void* x, const float* y, void* ws, int64_t ws_bytes, void* x_out, float* y_out, double* disp_out,
                                  double* field_out, usseg_stream_t stream) {
  USSEG_CHECK_ARG(d && samples_dev && weights_dev && x && y && ws && x_out && y_out, "elastic_warp: null pointer");
  USSEG_CHECK_ARG(d->B >= 1 && d->H >= 1 && d->W >= 1 && d->C >= 1, "elastic_warp: bad descriptor (B, H, W, C >= 1)");
  const int64_t M = (int64_t)d->B * d->H;                          // < 2^62
  USSEG_CHECK_ARG(M < ((int64_t)1 << 31) && M * d->W < ((int64_t)1 << 31) && M * d->W * d->C < ((int64_t)1 << 31),
                  "elastic_warp: bad descriptor (B*H*W*C < 2^31)");
  USSEG_CHECK_ARG(d->radius >= 0 && d->radius <= USSEG_WARP_MAX_RADIUS, "elastic_warp: bad descriptor (0 <= radius <= %d)", USSEG_WARP_MAX_RADIUS);
  const int64_t need = usseg_warp_ws_bytes(d->B, d->H, d->W);
  USSEG_CHECK_ARG(ws_bytes >= need, "elastic_warp: workspace of %lld bytes, need %lld (usseg_warp_ws_bytes)", (long long)ws_bytes, (long long)need);
  const int64_t pixels = M * d->W, xb = pixels * d->C * (d->x_is_f64 ? 8 : 4), yb = pixels * 4;
  USSEG_CHECK_ARG(!overlaps(x_out, xb, x, xb) && !overlaps(x_out, xb, y, yb) && !overlaps(y_out, yb, x, xb) && !overlaps(y_out, yb, y, yb),
                  "elastic_warp: x_out / y_out must not overlap x / y");
  const int tiles_h = (d->H + kTH - 1) / kTH, tiles_w = (d->W + kTW - 1) / kTW;
  const int64_t n_tiles = (int64_t)d->B * 2 * tiles_h * tiles_w;   // <= 2*B*H*W < 2^32
  const int64_t g1 = n_tiles < kGridCap ? n_tiles : kGridCap;
  hipLaunchKernelGGL(warp_blur_h_kernel, dim3((unsigned)g1), dim3(kThreads), 0, (hipStream_t)stream, *d, samples_dev, weights_dev, field,
                     (double*)ws, field_out, tiles_h, tiles_w, n_tiles);
  if (int rc = usseg_check_launch("elastic_warp (blur along H)")) return rc;
  int64_t g2 = cdiv64(pixels, kThreads);
  if (g2 > kGridCap) g2 = kGridCap;
  if (d->x_is_f64)
    hipLaunchKernelGGL(warp_gather_kernel<double>, dim3((unsigned)g2), dim3(kThreads), 0, (hipStream_t)stream, *d, samples_dev, weights_dev,
                       (const double*)ws, (const double*)x, y, (double*)x_out, y_out, disp_out);
  else
    hipLaunchKernelGGL(warp_gather_kernel<float>, dim3((unsigned)g2), dim3(kThreads), 0, (hipStream_t)stream, *d, samples_dev, weights_dev,
                       (const double*)ws, (const float*)x, y, (float*)x_out, y_out, disp_out);
  return usseg_check_launch("elastic_warp (gather)");
}
