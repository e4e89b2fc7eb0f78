// The device step between the two models of the brain-mask cascade (TBIEvaluator.py:221-231 with use_brainMask=True) and the two maps
// the evaluator derives from the bleed model's probabilities (:239, :249-252).  Both kernels are streaming pointwise passes: one pixel
// per lane (the gate: one 16-byte vector of the bf16 input row per lane), a grid-stride loop.  No allocation, no synchronisation:
// graph-capture safe.
//
// Roofline (HBM3E at 6.3 TB/s, the MI355X's measured float4-copy rate):
//   gate: M * (4*C_mask + 2*ldx + 2*ldx + 1) bytes = 73 B/pixel at C_mask 2, ldx 16: 23.9 MB at B=16 x 256x80 -> 3.8 us.  The in-place
//         form (x_gated == x) neither reads nor rewrites an ungated row, so it moves 4*C_mask + 1 bytes for such a pixel.
//   maps: M * (12 + 4 + 4) bytes = 6.6 MB at B=16 x 256x80 -> 1.0 us.
// Both inputs were written by the previous launch and fit the 256 MiB Infinity Cache, so the HBM figures are upper bounds.
#include "common.h"

namespace {
constexpr int kThreads = 256;

unsigned cascade_grid(int64_t items) {
  int64_t g = cdiv64(items, kThreads);
  if (g > 2048) g = 2048;
  return (unsigned)(g < 1 ? 1 : g);
}
}  // namespace

// Named outside the anonymous namespace: the profiler reports kernels of an anonymous namespace with an empty name.
// gate = p0 > 0.5f is np.round(p0) == 1 for every fp32 p0 (round-half-to-even sends 0.5 to 0; NaN compares false; p0 >= 1.5 cannot
// come out of a softmax).
// One 16-byte vector of a row per lane (VC vectors per pixel: 1 for ldx 8, 2 for ldx 16 - every 1..16-channel input; 0: ldx/8 counted at
// run time), so a wave's loads and stores cover contiguous bytes; the VC lanes of a pixel read the same probability.
template <int VC>
__global__ __launch_bounds__(256) void cascade_gate_kernel(const float* __restrict__ probs, int C_mask, int64_t M, const uint4* x, int ldx,
                                                           uint4* x_gated, uint8_t* __restrict__ mask) {
  const int V = VC ? VC : ldx / 8;
  const bool inplace = x == x_gated;
  const int64_t total = M * V;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t m = i / V;
    const bool gate = probs[m * C_mask] > 0.5f;
    if (gate) x_gated[i] = make_uint4(0u, 0u, 0u, 0u);
    else if (!inplace) x_gated[i] = x[i];
    if (mask && i - m * V == 0) mask[m] = (uint8_t)gate;
  }
}

__global__ __launch_bounds__(256) void cascade_maps_kernel(const float* __restrict__ probs, int64_t M, float* __restrict__ prob_map,
                                                           float* __restrict__ bleed_prob) {
#pragma clang fp contract(off)       // three roundings, as the reference's three statements: 0.5f*p1 is not fused into the subtraction
  for (int64_t m = (int64_t)blockIdx.x * kThreads + threadIdx.x; m < M; m += (int64_t)gridDim.x * kThreads) {
    const float p0 = probs[m * 3], p1 = probs[m * 3 + 1], p2 = probs[m * 3 + 2];
    prob_map[m] = ((1.0f - p0) - 0.5f * p1) + p2;        // :249-252, in that order
    bleed_prob[m] = p2;                                  // :239
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int usseg_cascade_gate(const float* probs, int32_t C_mask, int64_t M, const void* x, int32_t ldx, void* x_gated, uint8_t* mask,
                                  usseg_stream_t stream) {
  USSEG_CHECK_ARG(probs && x && x_gated, "cascade_gate: null pointer");
  USSEG_CHECK_ARG(M > 0 && ldx > 0 && ldx % 8 == 0, "cascade_gate: bad geometry (M > 0, ldx a positive multiple of 8)");
  USSEG_CHECK_ARG(C_mask >= 2 && C_mask <= 4, "cascade_gate: C_mask must be 2..4");
  USSEG_CHECK_ARG(aligned16(x) && aligned16(x_gated), "cascade_gate: x and x_gated must be 16-byte aligned");
  auto k = ldx == 16 ? cascade_gate_kernel<2> : ldx == 8 ? cascade_gate_kernel<1> : cascade_gate_kernel<0>;
  hipLaunchKernelGGL(k, dim3(cascade_grid(M * (ldx / 8))), dim3(kThreads), 0, (hipStream_t)stream, probs, (int)C_mask, M, (const uint4*)x, (int)ldx,
                     (uint4*)x_gated, mask);
  return usseg_check_launch("cascade_gate");
}

extern "C" int usseg_cascade_maps(const float* probs, int32_t C, int64_t M, float* prob_map, float* bleed_prob, usseg_stream_t stream) {
  USSEG_CHECK_ARG(probs && prob_map && bleed_prob, "cascade_maps: null pointer");
  USSEG_CHECK_ARG(C == 3, "cascade_maps: C must be 3");
  USSEG_CHECK_ARG(M > 0, "cascade_maps: bad geometry (M > 0)");
  hipLaunchKernelGGL(cascade_maps_kernel, dim3(cascade_grid(M)), dim3(kThreads), 0, (hipStream_t)stream, probs, M, prob_map, bleed_prob);
  return usseg_check_launch("cascade_maps");
}
