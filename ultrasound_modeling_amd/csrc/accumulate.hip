// Gradient accumulation for gfx950 (include/usseg_accumulate.h, usseg_grad_accumulate): the sum of N micro-batch gradients kept in one more flat fp32 buffer, and on the N-th the mean handed
// back in the gradient buffer for the unchanged clip / exchange / Adam tail.  A pure stream: 16 bytes per lane,
// no atomics, no LDS, no device counter - acc is zero again after every finish, so one captured micro-step serves a whole group.
#include "common.h"
#include "../../include/usseg_accumulate.h"

// Every operation is one separately rounded IEEE fp32 operation (an add, and on the finish a true division: no reciprocal multiply, nothing
// to contract), so NumPy fp32 restates both behaviours bit for bit for any N.
template <bool FINISH>
__device__ __forceinline__ void accumulate_elem(float& a, float& g, float divisor) {
  const float t = __fadd_rn(a, g);
  if (FINISH) {
    g = __fdiv_rn(t, divisor);
    a = 0.f;
  } else {
    a = t;
  }
}

template <bool FINISH>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, float* __restrict__ grad, int64_t n, float divisor) {
  const int64_t n4 = n >> 2;
  float4* a4 = reinterpret_cast<float4*>(acc);
  float4* g4 = reinterpret_cast<float4*>(grad);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    float4 ai = a4[i], gi = g4[i];
    accumulate_elem<FINISH>(ai.x, gi.x, divisor);
    accumulate_elem<FINISH>(ai.y, gi.y, divisor);
    accumulate_elem<FINISH>(ai.z, gi.z, divisor);
    accumulate_elem<FINISH>(ai.w, gi.w, divisor);
    a4[i] = ai;
    if (FINISH) g4[i] = gi;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {       // scalar tail: n need not be a multiple of 4
    const int64_t i = n4 * 4 + threadIdx.x;
    float ai = acc[i], gi = grad[i];
    accumulate_elem<FINISH>(ai, gi, divisor);
    acc[i] = ai;
    if (FINISH) grad[i] = gi;
  }
}

extern "C" int usseg_grad_accumulate(float* acc, float* grad, int64_t n, int32_t finish, float divisor, usseg_stream_t stream) {
  USSEG_CHECK_ARG(n >= 0, "grad_accumulate: n < 0");
  if (n == 0) return USSEG_OK;             // (an empty tensor has no address)
  USSEG_CHECK_ARG(acc && grad, "grad_accumulate: null pointer");
  USSEG_CHECK_ARG(((uintptr_t)acc | (uintptr_t)grad) % 16 == 0, "grad_accumulate: acc and grad must be 16-byte aligned");
  USSEG_CHECK_ARG(acc + n <= grad || grad + n <= acc, "grad_accumulate: acc and grad overlap");
  USSEG_CHECK_ARG(finish == 0 || finish == 1, "grad_accumulate: finish must be 0 or 1");
  USSEG_CHECK_ARG(!finish || divisor >= 1.f, "grad_accumulate: divisor must be the number of micro-steps, >= 1");
  int64_t grid = cdiv64(n, 256 * 4);       // usseg_adam_clip_step's grid
  if (grid > 4096) grid = 4096;
  if (finish)
    hipLaunchKernelGGL(grad_accumulate_kernel<true>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, acc, grad, n, divisor);
  else
    hipLaunchKernelGGL(grad_accumulate_kernel<false>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, acc, grad, n, divisor);
  return usseg_check_launch("grad_accumulate");
}
