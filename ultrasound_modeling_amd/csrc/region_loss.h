// What the two passes of the region losses share (overlap_loss.hip: soft Dice / Tversky, the boundary term; lovasz.hip: Lovasz-softmax), each
// optionally plus CategoricalCrossentropy.  Both read probs / y_true (fp32 [M][C], C <= 4) behind the probabilities-only head launch:
//   pass 1  K grid-wide totals by grid_ordered_sums (common.h) into the accumulator laid out below; the last workgroup writes loss and coefficients;
//   pass 2  d loss / d logits = p_j*(G_j - sum_c p_c*G_c) from the loss's own G, one bf16 rounding, row or quad layout.
// A thread owns GROUPS of four consecutive pixels: 4*C floats = C 16-byte loads per tensor whatever C is (the base pointers are 16-byte
// aligned, checked by the entry points); the last group of an M that is no multiple of 4 takes guarded scalar loads.
// NOT shared with attn_loss_optim.hip: softmax_loss_pixel and the fused head kernel keep their own statement of the CCE arithmetic, because that
// file's kernels are on the benchmarked step and stay instruction for instruction what they are.
#pragma once
#include "common.h"
#include <cmath>

// The accumulator (usseg.h, USSEG_OVERLAP_ACC_FLOATS): acc[0] loss, [1] ticket, [2] CCE pixel sum, the rest of the header as each loss documents
// it; behind the header one row of partials per workgroup, acc[REGION_HDR + REGION_STRIDE*b + k].
#define REGION_HDR 32
#define REGION_STRIDE 16
#define REGION_MAX_BLOCKS ((USSEG_OVERLAP_ACC_FLOATS - REGION_HDR) / REGION_STRIDE)
static_assert(REGION_MAX_BLOCKS == 512, "usseg.h documents the grid rule with 512 workgroups");

template <int C>
__device__ __forceinline__ void region_load_group(const float* __restrict__ base, int g, int M, float (&v)[4 * C]) {
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

// CategoricalCrossentropy(label_smoothing) on probabilities, one pixel: the arithmetic of loss_kind 0 (Keras: divide by the class sum,
// clip, log; the gradient is zero where the quotient was clipped).  Returns the loss term; dLdp (if asked for) is unscaled.
template <int C, bool GRAD>
__device__ __forceinline__ float region_cce_pixel(const float* p, const float* y, float ls, float eps, float* dLdp) {
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

// The tail of pass 2 for pixel m: G = d loss / d p, p its probabilities -> dlogits.  Row layout: dl[m*8 + c], one 16-byte store per pixel with
// the pad channels zero.  Quad layout (UssegLossDesc.quad_w = W): pixel (y, x) in slot 4*((y&1)*2 + (x&1)) of the 16-channel pixel (y/2, x/2),
// one 8-byte store per pixel - the four pixels of a 2x2 block fill all 16.
template <int C, bool QUAD>
__device__ __forceinline__ void region_store_dlogits(const float (&G)[C], const float* p, bf16_t* __restrict__ dl, int m, int HW, int W) {
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) dot += G[c] * p[c];
  float o[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = c < C ? p[c < C ? c : 0] * (G[c < C ? c : 0] - dot) : 0.f;
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

// ---- host side: the checks on UssegLossDesc that every entry point of the family makes, in the pieces their order of refusal needs -----------
static inline int region_shape_args(const char* who, const UssegLossDesc* d) {
  USSEG_CHECK_ARG(d->C >= 1 && d->C <= 4, "%s: 1 <= C <= 4", who);
  USSEG_CHECK_ARG(d->HW > 0 && d->M >= 0 && d->M % d->HW == 0, "%s: M must be a non-negative multiple of HW", who);
  USSEG_CHECK_ARG(d->M <= (1 << 29), "%s: more than 2^29 pixels", who);
  return USSEG_OK;
}
static inline int region_scale_args(const char* who, const UssegLossDesc* d, float ce_weight) {
  USSEG_CHECK_ARG(std::isfinite(d->inv_global_batch) && d->inv_global_batch >= 0.f, "%s: inv_global_batch must be finite and >= 0", who);
  if (ce_weight != 0.f) {
    USSEG_CHECK_ARG(d->label_smoothing >= 0.f && d->label_smoothing < 1.f, "%s: label_smoothing must lie in [0, 1)", who);
    USSEG_CHECK_ARG(d->clip_eps > 0.f && 1.f - d->clip_eps < 1.f && d->clip_eps < 0.5f, "%s: clip_eps must be > 0 and representable below 1 in fp32", who);
  }
  return USSEG_OK;
}
static inline int region_bwd_args(const char* who, const UssegLossDesc* d, const void* dlogits) {
  USSEG_CHECK_ARG(dlogits && ((uintptr_t)dlogits & 15) == 0, "%s: dlogits must be a 16-byte aligned pointer", who);
  USSEG_CHECK_ARG(d->quad_w == 0 || (d->quad_w > 0 && d->quad_w % 2 == 0 && d->HW % (2 * d->quad_w) == 0), "%s: quad layout needs even H and W", who);
  USSEG_CHECK_ARG(d->lddl == (d->quad_w ? 16 : 8), "%s: dlogits stride must be 8 (16 in the quad layout)", who);
  return USSEG_OK;
}
static inline int region_groups(const UssegLossDesc* d) { return (int)((d->M + 3) / 4); }
// pass 2: a thread per group, at most 2048 workgroups (pass 1's grid is usseg_overlap_loss_grid, part of the ABI)
static inline dim3 region_bwd_grid(int ngroups) {
  const int64_t g = cdiv64(ngroups, 256);
  return dim3((unsigned)(g > 2048 ? 2048 : g));
}
