// The evaluator's cone figures (TBIEvaluator.Display of the reference, TBIEvaluator.py:276-355): four pcolormesh panels per test image,
// scan-converted and colour-mapped on the device so the host only compresses PNGs.  DESIGN.md section 4i has the rules and the numbers.
//   usseg_cone_index   once per geometry: which quad of the [H][W] vertex grid each pixel of a panel shows (-1: background)
//   usseg_cone_range   once per batch: each image's bMode colour range, np.histogram(bMode, bins=25) edges [2] and [-2]
//   usseg_cone_render  once per batch: all four panels of every image into uint8 RGB, reading the range from the device
// All arithmetic is fp64 with `fp contract(off)` (the separate roundings of the NumPy restatement, tests/cone_restatement.py); the
// index image is an atomicMax over quads and every other value is written by one lane, so every result is bitwise reproducible.
#include "common.h"
#include <cmath>

namespace {
constexpr int kThreads = 256;
constexpr int kRangeThreads = 1024;
constexpr int kPixPerLane = 4;     // 4 RGB pixels = 12 bytes = three dword stores per lane

unsigned cone_grid(int64_t items) {
  int64_t g = cdiv64(items, kThreads);
  if (g > 65535) g = 65535;
  return (unsigned)(g < 1 ? 1 : g);
}

struct PanelRanges {               // vmin / vmax of panels 0..2 (Prediction, label, Probability Bleed), by value
  double lo[3], hi[3];
};
}  // namespace

// ---------------------------------------------------------------------------------------------------------------- index image
// One lane per quad q = i*(W-1) + j over the pixel bounding box of its four vertices (widened by one pixel: the winding test alone
// decides).  A pixel centre (px, py) is covered when the quad's nonzero winding number there is not 0, counted with the half-open
// crossing rule: an upward edge (y0 <= py < y1) with the point strictly left of it +1, a downward edge (y1 <= py < y0) with the point
// strictly right of it -1.  atomicMax keeps the last quad in row-major draw order whatever order the lanes run in.
__global__ __launch_bounds__(256) void cone_index_kernel(const double* __restrict__ X, const double* __restrict__ Y, int H, int W, double xmin,
                                                         double ymin, double ppu, int Hp, int Wp, int* __restrict__ index) {
#pragma clang fp contract(off)
  const int Wq = W - 1;
  const int64_t nq = (int64_t)(H - 1) * Wq;
  for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < nq; q += (int64_t)gridDim.x * kThreads) {
    const int i = (int)(q / Wq), j = (int)(q - (int64_t)i * Wq);
    const int64_t a = (int64_t)i * W + j;
    const double vx[4] = {X[a], X[a + 1], X[a + W + 1], X[a + W]};
    const double vy[4] = {Y[a], Y[a + 1], Y[a + W + 1], Y[a + W]};
    bool finite = true;
    double x0 = vx[0], x1 = vx[0], y0 = vy[0], y1 = vy[0];
    for (int e = 0; e < 4; ++e) {
      finite = finite && isfinite(vx[e]) && isfinite(vy[e]);
      x0 = fmin(x0, vx[e]);
      x1 = fmax(x1, vx[e]);
      y0 = fmin(y0, vy[e]);
      y1 = fmax(y1, vy[e]);
    }
    if (!finite) continue;
    const double cl = floor((x0 - xmin) * ppu - 0.5) - 1.0, ch = ceil((x1 - xmin) * ppu - 0.5) + 1.0;
    const double rl = floor((y0 - ymin) * ppu - 0.5) - 1.0, rh = ceil((y1 - ymin) * ppu - 0.5) + 1.0;
    const int c_lo = cl < 0.0 ? 0 : (int)cl, c_hi = ch > (double)(Wp - 1) ? Wp - 1 : (int)ch;
    const int r_lo = rl < 0.0 ? 0 : (int)rl, r_hi = rh > (double)(Hp - 1) ? Hp - 1 : (int)rh;
    for (int r = r_lo; r <= r_hi; ++r) {
      const double py = ymin + ((double)r + 0.5) / ppu;
      for (int c = c_lo; c <= c_hi; ++c) {
        const double px = xmin + ((double)c + 0.5) / ppu;
        int wn = 0;
        for (int e = 0; e < 4; ++e) {
          const double ex0 = vx[e], ey0 = vy[e], ex1 = vx[(e + 1) & 3], ey1 = vy[(e + 1) & 3];
          const double il = (ex1 - ex0) * (py - ey0) - (px - ex0) * (ey1 - ey0);
          if (ey0 <= py) {
            if (py < ey1 && il > 0.0) ++wn;
          } else if (ey1 <= py && il < 0.0) {
            --wn;
          }
        }
        if (wn != 0) atomicMax(index + (int64_t)r * Wp + c, (int)q);
      }
    }
  }
}

extern "C" int usseg_cone_index(const double* X, const double* Y, int32_t H, int32_t W, double xmin, double ymin, double ppu, int32_t Hp,
                                int32_t Wp, int32_t* index, usseg_stream_t stream) {
  USSEG_CHECK_ARG(X && Y && index, "cone_index: null pointer");
  USSEG_CHECK_ARG(H >= 2 && W >= 2, "cone_index: the vertex grid needs H, W >= 2 (got %d x %d)", (int)H, (int)W);
  USSEG_CHECK_ARG((int64_t)H * W * 8 <= INT32_MAX, "cone_index: a %d x %d fp64 grid overflows int32 byte offsets", (int)H, (int)W);
  USSEG_CHECK_ARG(Hp >= 1 && Wp >= 1 && (int64_t)Hp * Wp * 4 <= INT32_MAX, "cone_index: panel %d x %d is empty or overflows int32 byte offsets",
                  (int)Hp, (int)Wp);
  USSEG_CHECK_ARG(std::isfinite(xmin) && std::isfinite(ymin) && std::isfinite(ppu) && ppu > 0.0, "cone_index: bad origin or px_per_unit");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(index, 0xFF, (size_t)Hp * Wp * sizeof(int32_t), s) != hipSuccess) {      // every pixel -1: background
    usseg_set_error("cone_index: hipMemsetAsync failed");
    return USSEG_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(cone_index_kernel, dim3(cone_grid((int64_t)(H - 1) * (W - 1))), dim3(kThreads), 0, s, X, Y, (int)H, (int)W, xmin, ymin,
                     ppu, (int)Hp, (int)Wp, index);
  return usseg_check_launch("cone_index");
}

// ---------------------------------------------------------------------------------------------------------------- bMode range
// One workgroup per image: min / max of the finite values (exact, order-free) and a non-finite flag, then numpy's edges: when
// min == max both move by 0.5; step = (last - first) / 25; edge k = k*step + first (np.linspace; (k/25)*delta + first when step is 0),
// the last edge = last.  Flag bit 0: a NaN or an infinity; bit 1: edges that do not strictly increase (a range of a few ulps).  Both
// make np.histogram raise.
__global__ __launch_bounds__(1024) void cone_range_kernel(const double* __restrict__ bmode, int HW, double* __restrict__ range,
                                                          int* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  __shared__ double smn[kRangeThreads], smx[kRangeThreads];
  __shared__ int sbad[kRangeThreads];
  const int b = blockIdx.x, t = threadIdx.x;
  const double* p = bmode + (int64_t)b * HW;
  double mn = INFINITY, mx = -INFINITY;
  int bad = 0;
#pragma unroll 4
  for (int k = t; k < HW; k += kRangeThreads) {      // a few loads in flight per lane: one workgroup per image is latency-bound
    const double v = p[k];
    if (isfinite(v)) {
      mn = fmin(mn, v);
      mx = fmax(mx, v);
    } else {
      bad = 1;
    }
  }
  smn[t] = mn;
  smx[t] = mx;
  sbad[t] = bad;
  __syncthreads();
  for (int w = kRangeThreads / 2; w > 0; w >>= 1) {
    if (t < w) {
      smn[t] = fmin(smn[t], smn[t + w]);
      smx[t] = fmax(smx[t], smx[t + w]);
      sbad[t] |= sbad[t + w];
    }
    __syncthreads();
  }
  if (t == 0) {
    double first = smn[0], last = smx[0];
    if (first == last) {
      first = first - 0.5;
      last = last + 0.5;
    }
    const double delta = last - first, step = delta / 25.0;
    double prev = first, e2 = first, e24 = first;
    int flag = sbad[0];
    for (int k = 1; k <= 25; ++k) {        // every edge, to refuse what np.histogram refuses: edges that do not strictly increase
      const double e = k == 25 ? last : step == 0.0 ? ((double)k / 25.0) * delta + first : (double)k * step + first;
      if (!(prev < e)) flag |= 2;
      if (k == 2) e2 = e;
      if (k == 24) e24 = e;
      prev = e;
    }
    range[2 * b] = e2;
    range[2 * b + 1] = e24;
    nonfinite[b] = flag;
  }
}

extern "C" int usseg_cone_range(const double* bmode, int32_t B, int32_t HW, double* range, int32_t* nonfinite, usseg_stream_t stream) {
  USSEG_CHECK_ARG(bmode && range && nonfinite, "cone_range: null pointer");
  USSEG_CHECK_ARG(B >= 1 && HW >= 1 && B <= 65535, "cone_range: bad batch (1 <= B <= 65535, HW >= 1)");
  hipLaunchKernelGGL(cone_range_kernel, dim3(B), dim3(kRangeThreads), 0, (hipStream_t)stream, bmode, (int)HW, range, (int*)nonfinite);
  return usseg_check_launch("cone_range");
}

// ---------------------------------------------------------------------------------------------------------------- render
struct RenderArgs {
  const int* index;
  const float *prob, *bleed;
  const double *label, *bmode, *bm_range;
  const uint8_t* luts;
  int Hp, Wp, gap, B, H, W, OH, OW;
};

// Four consecutive pixels of the flat [B][OH][OW] pixel sequence per lane: 12 bytes, stored as three dwords (the buffer is 4-byte
// aligned and 12*g is a multiple of 4).  The last lane of a sequence whose length is not a multiple of 4 stores bytes.  The chain per
// pixel is index -> value -> colour; the four pixels' loads go out together at each step and the tables sit in LDS, so a lane waits on
// two rounds of global loads instead of twelve dependent ones.
__global__ __launch_bounds__(256) void cone_render_kernel(RenderArgs a, PanelRanges rg, uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ uint8_t lut[2 * 256 * 3];
  for (int k = threadIdx.x; k < 2 * 256 * 3; k += kThreads) lut[k] = a.luts[k];
  __syncthreads();
  const int ppi = a.OH * a.OW, Wq = a.W - 1, nq = (a.H - 1) * Wq;
  const int64_t npix = (int64_t)a.B * ppi;
  const int64_t lanes = (npix + kPixPerLane - 1) / kPixPerLane;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < lanes; g += (int64_t)gridDim.x * kThreads) {
    const int64_t p0 = g * kPixPerLane;
    int b = (int)(p0 / ppi);
    const int rem = (int)(p0 - (int64_t)b * ppi);
    int y = rem / a.OW, x = rem - y * a.OW;
    int img[kPixPerLane], panel[kPixPerLane], q[kPixPerLane];
#pragma unroll
    for (int k = 0; k < kPixPerLane; ++k) {             // step 1: which panel, and the index image (-1: gap, background, past the end)
      const int pr = y < a.Hp ? 0 : y >= a.Hp + a.gap ? 1 : -1;
      const int pc = x < a.Wp ? 0 : x >= a.Wp + a.gap ? 1 : -1;
      const bool in = p0 + k < npix && (pr | pc) >= 0;
      img[k] = b;
      panel[k] = pr * 2 + pc;
      q[k] = in ? a.index[(y - pr * (a.Hp + a.gap)) * a.Wp + (x - pc * (a.Wp + a.gap))] : -1;
      if (++x == a.OW) {
        x = 0;
        if (++y == a.OH) {
          y = 0;
          ++b;
        }
      }
    }
    double v[kPixPerLane], lo[kPixPerLane], hi[kPixPerLane];
#pragma unroll
    for (int k = 0; k < kPixPerLane; ++k) {             // step 2: the quad's value and the panel's range
      v[k] = NAN;
      lo[k] = hi[k] = 0.0;
      if (q[k] < 0 || q[k] >= nq) continue;             // (an index image of another grid reads nothing)
      const int i = q[k] / Wq, j = q[k] - i * Wq;
      const int64_t off = ((int64_t)img[k] * a.H + i) * a.W + j;
      const int p = panel[k];
      if (p == 3) {
        v[k] = a.bmode[off];
        lo[k] = a.bm_range[2 * img[k]];
        hi[k] = a.bm_range[2 * img[k] + 1];
      } else {
        v[k] = p == 0 ? (double)a.prob[off] : p == 1 ? a.label[off] : (double)a.bleed[off];
        lo[k] = p == 0 ? rg.lo[0] : p == 1 ? rg.lo[1] : rg.lo[2];
        hi[k] = p == 0 ? rg.hi[0] : p == 1 ? rg.hi[1] : rg.hi[2];
      }
    }
    uint32_t px[kPixPerLane];
#pragma unroll
    for (int k = 0; k < kPixPerLane; ++k) {             // step 3: colour.  Gaps, background, NaN and inf (pcolormesh masks them): white
      if (!isfinite(v[k])) {
        px[k] = 0xFFFFFFu;
        continue;
      }
      int c = 0;                                        // Normalize maps everything to 0 when vmin == vmax
      if (hi[k] != lo[k]) {
        const double f = floor((v[k] - lo[k]) / (hi[k] - lo[k]) * 256.0);
        c = f >= 255.0 ? 255 : f >= 0.0 ? (int)f : 0;   // under -> entry 0, over -> entry 255
      }
      const uint8_t* e = lut + (panel[k] == 3 ? 768 : 0) + 3 * c;
      px[k] = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16);
    }
    uint8_t* o = out + p0 * 3;
    if (p0 + kPixPerLane <= npix) {
      uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
      o32[0] = px[0] | (px[1] << 24);
      o32[1] = (px[1] >> 8) | (px[2] << 16);
      o32[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
      for (int k = 0; p0 + k < npix; ++k) {
        o[3 * k] = (uint8_t)px[k];
        o[3 * k + 1] = (uint8_t)(px[k] >> 8);
        o[3 * k + 2] = (uint8_t)(px[k] >> 16);
      }
    }
  }
}

extern "C" int usseg_cone_render(const int32_t* index, int32_t Hp, int32_t Wp, int32_t gap, const float* prob_map, const double* label,
                                 const float* bleed, const double* bmode, int32_t B, int32_t H, int32_t W, const double* ranges,
                                 const double* bmode_range, const uint8_t* luts, uint8_t* out, usseg_stream_t stream) {
  USSEG_CHECK_ARG(index && prob_map && label && bleed && bmode && ranges && bmode_range && luts && out, "cone_render: null pointer");
  USSEG_CHECK_ARG(((uintptr_t)out & 3) == 0, "cone_render: out must be 4-byte aligned");
  USSEG_CHECK_ARG(B >= 1 && H >= 2 && W >= 2 && (int64_t)H * W * 8 <= INT32_MAX, "cone_render: bad value planes (B >= 1, H, W >= 2)");
  USSEG_CHECK_ARG(Hp >= 1 && Wp >= 1 && gap >= 0 && (int64_t)Hp * Wp * 4 <= INT32_MAX, "cone_render: bad panel geometry");
  const int64_t OH = 2 * (int64_t)Hp + gap, OW = 2 * (int64_t)Wp + gap;
  USSEG_CHECK_ARG(OH * OW * 3 <= INT32_MAX, "cone_render: a %lld x %lld figure overflows int32 byte offsets", (long long)OH, (long long)OW);
  PanelRanges rg;
  for (int p = 0; p < 3; ++p) {
    rg.lo[p] = ranges[2 * p];
    rg.hi[p] = ranges[2 * p + 1];
  }
  RenderArgs a{index, prob_map, bleed, label, bmode, bmode_range, luts, (int)Hp, (int)Wp, (int)gap, (int)B, (int)H, (int)W, (int)OH, (int)OW};
  const int64_t lanes = cdiv64((int64_t)B * OH * OW, kPixPerLane);
  hipLaunchKernelGGL(cone_render_kernel, dim3(cone_grid(lanes)), dim3(kThreads), 0, (hipStream_t)stream, a, rg, out);
  return usseg_check_launch("cone_render");
}
