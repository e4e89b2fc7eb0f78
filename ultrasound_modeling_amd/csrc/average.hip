// Weight averaging inside the optimiser step for gfx950: tfa.optimizers.MovingAverage (EMA) and tfa.optimizers.SWA kept by the same
// elementwise launch that applies AdamW.  The kernels stream 16 bytes per lane; the descriptor and the step counter
// are read from device memory, so a captured graph follows every stream-ordered rewrite of them.
#include "common.h"
#include "optim_elem.h"
#include <cmath>

// The blend coefficient c of step t (= *step AFTER the increment, the t of Adam's bias correction): avg += c*(p - avg).
//   EMA: t <= start -> 1 (the average tracks the weights); else 1 - d_t, d_t = decay or min(decay, (1+t)/(10+t)) with dynamic_decay
//   SWA: t >= start and (t-start) % period == 0 -> 1/(k+1), k = (t-start)/period (the first snapshot replaces the average); else 0
__device__ __forceinline__ float average_coeff(const UssegAverage* d, int t) {
  const int mode = d->mode, start = d->start;
  if (mode == USSEG_AVERAGE_EMA) {
    if (t <= start) return 1.f;
    float dt = d->decay;
    if (d->dynamic_decay) dt = fminf(dt, (float)(1 + t) / (float)(10 + t));
    return 1.f - dt;
  }
  if (mode == USSEG_AVERAGE_SWA) {
    const int period = max(d->period, 1);
    if (t < start || (t - start) % period != 0) return 0.f;
    return 1.f / (float)((t - start) / period + 1);
  }
  return 0.f;
}
// one element, 0 < c < 1: the fused multiply-add is written out, not left to contraction
__device__ __forceinline__ float average_elem(float avg, float p, float c) { return fmaf(c, p - avg, avg); }
__device__ __forceinline__ float4 average_elem4(float4 a, float4 p, float c) {
  return make_float4(average_elem(a.x, p.x, c), average_elem(a.y, p.y, c), average_elem(a.z, p.z, c), average_elem(a.w, p.w, c));
}

__global__ __launch_bounds__(256) void average_kernel(float* __restrict__ avg, const float* __restrict__ p, int64_t n, const int32_t* step,
                                                       const UssegAverage* desc) {
  const float c = average_coeff(desc, *step);
  if (c == 0.f) return;                  // no snapshot at this step: no byte of avg moves
  const bool copy = c == 1.f;            // avg = p itself ((p - avg) + avg need not round back to p)
  const int64_t n4 = n >> 2;
  float4* a4 = reinterpret_cast<float4*>(avg);
  const float4* p4 = reinterpret_cast<const float4*>(p);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 pi = p4[i];
    a4[i] = copy ? pi : average_elem4(a4[i], pi, c);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = n4 * 4 + threadIdx.x;
    avg[i] = copy ? p[i] : average_elem(avg[i], p[i], c);
  }
}
extern "C" int usseg_average_update(float* avg, const float* p, int64_t n, const int32_t* step_dev, const UssegAverage* avg_desc_dev,
                                    usseg_stream_t stream) {
  USSEG_CHECK_ARG(avg && p && step_dev && avg_desc_dev, "average_update: null pointer");
  USSEG_CHECK_ARG(n >= 0, "average_update: n < 0");
  USSEG_CHECK_ARG(((uintptr_t)avg | (uintptr_t)p) % 16 == 0, "average_update: avg and p must be 16-byte aligned");
  if (n == 0) return USSEG_OK;
  int64_t grid = cdiv64(n >> 2 > 0 ? n >> 2 : 1, 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(average_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, avg, p, n, step_dev, avg_desc_dev);
  return usseg_check_launch("average_update");
}

// adamw_kernel (attn_loss_optim.hip) with the average of the updated p kept in the same pass: 36 bytes per parameter instead of 28, no
// second launch.  wd_t_dev == NULL is the fixed-rate step (no decay): adamw_elem without decay is adam_kernel's arithmetic.
__global__ __launch_bounds__(256) void adamw_avg_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, float* __restrict__ avg, int64_t n, const float* sumsq,
                                                         float clip_norm, const float* lr_t_dev, const float* wd_t_dev,
                                                         const uint8_t* __restrict__ mask, float b1, float b2, float eps, const int32_t* step,
                                                         const UssegAverage* desc) {
  float scale = 1.f;
  if (clip_norm > 0.f) scale = clip_norm / fmaxf(sqrtf(*sumsq), clip_norm);  // tf.clip_by_global_norm
  const float lr_t = *lr_t_dev, wd_t = wd_t_dev ? *wd_t_dev : 0.f;
  const bool wd_on = wd_t != 0.f;        // p - 0*p would turn -0 into +0: no decay at all
  const float c = average_coeff(desc, *step);
  const bool blend = c != 0.f, copy = c == 1.f;
  const int64_t n4 = n >> 2;
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  float4* a4 = reinterpret_cast<float4*>(avg);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const uchar4* k4 = reinterpret_cast<const uchar4*>(mask);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    float4 pi = p4[i], mi = m4[i], vi = v4[i];
    const float4 gi = g4[i];
    float4 ai = make_float4(0.f, 0.f, 0.f, 0.f);
    if (blend && !copy) ai = a4[i];
    uchar4 k = make_uchar4(1, 1, 1, 1);
    if (mask && wd_on) k = k4[i];
    adamw_elem(pi.x, gi.x, mi.x, vi.x, wd_on && k.x, scale, lr_t, wd_t, b1, b2, eps);
    adamw_elem(pi.y, gi.y, mi.y, vi.y, wd_on && k.y, scale, lr_t, wd_t, b1, b2, eps);
    adamw_elem(pi.z, gi.z, mi.z, vi.z, wd_on && k.z, scale, lr_t, wd_t, b1, b2, eps);
    adamw_elem(pi.w, gi.w, mi.w, vi.w, wd_on && k.w, scale, lr_t, wd_t, b1, b2, eps);
    p4[i] = pi;
    m4[i] = mi;
    v4[i] = vi;
    if (blend) a4[i] = copy ? pi : average_elem4(ai, pi, c);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {       // scalar tail: n need not be a multiple of 4
    const int64_t i = n4 * 4 + threadIdx.x;
    const bool decay = wd_on && (mask == nullptr || mask[i] != 0);
    float pi = p[i];
    adamw_elem(pi, g[i], m[i], v[i], decay, scale, lr_t, wd_t, b1, b2, eps);
    p[i] = pi;
    if (blend) avg[i] = copy ? pi : average_elem(avg[i], pi, c);
  }
}
extern "C" int usseg_adamw_avg_step(float* p, const float* g, float* m, float* v, float* avg, int64_t n, const float* sumsq, float clip_norm,
                                    const float* lr_t_dev, const float* wd_t_dev, const uint8_t* decay_mask, float beta1, float beta2, float eps,
                                    const int32_t* step_dev, const UssegAverage* avg_desc_dev, usseg_stream_t stream) {
  USSEG_CHECK_ARG(p && g && m && v && avg && lr_t_dev && step_dev && avg_desc_dev, "adamw_avg_step: null pointer");
  USSEG_CHECK_ARG(clip_norm <= 0.f || sumsq, "adamw_avg_step: clip_norm > 0 needs sumsq");
  USSEG_CHECK_ARG(n >= 0, "adamw_avg_step: n < 0");
  USSEG_CHECK_ARG(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)avg) % 16 == 0,
                  "adamw_avg_step: p, g, m, v and avg must be 16-byte aligned");
  USSEG_CHECK_ARG((uintptr_t)decay_mask % 4 == 0, "adamw_avg_step: decay_mask must be 4-byte aligned");
  if (n == 0) return USSEG_OK;
  int64_t grid = cdiv64(n >> 2 > 0 ? n >> 2 : 1, 256);      // adamw_step's grid
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(adamw_avg_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, avg, n, sumsq, clip_norm, lr_t_dev,
                     wd_t_dev, decay_mask, beta1, beta2, eps, step_dev, avg_desc_dev);
  return usseg_check_launch("adamw_avg_step");
}

__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n) {
  const int64_t n4 = n >> 2;
  float4* a4 = reinterpret_cast<float4*>(a);
  float4* b4 = reinterpret_cast<float4*>(b);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 x = a4[i], y = b4[i];
    a4[i] = y;
    b4[i] = x;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = n4 * 4 + threadIdx.x;
    const float x = a[i], y = b[i];
    a[i] = y;
    b[i] = x;
  }
}
extern "C" int usseg_swap_f32(float* a, float* b, int64_t n, usseg_stream_t stream) {
  USSEG_CHECK_ARG(a && b, "swap_f32: null pointer");
  USSEG_CHECK_ARG(n >= 0, "swap_f32: n < 0");
  USSEG_CHECK_ARG(((uintptr_t)a | (uintptr_t)b) % 16 == 0, "swap_f32: a and b must be 16-byte aligned");
  USSEG_CHECK_ARG(a + n <= b || b + n <= a, "swap_f32: a and b overlap");
  if (n == 0) return USSEG_OK;
  int64_t grid = cdiv64(n >> 2 > 0 ? n >> 2 : 1, 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(swap_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a, b, n);
  return usseg_check_launch("swap_f32");
}
