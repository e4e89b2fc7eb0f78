// Region-overlap losses (soft Dice / Tversky, optionally plus CategoricalCrossentropy) on the head's probabilities: usseg.h, UssegOverlapLoss.
// The gradient at one pixel depends on sums over every pixel of the call, so the loss cannot ride in the fused head launch the way the
// per-pixel losses do.  Two passes over probs / y_true (fp32 [M][C], C <= 4) behind today's probabilities-only head launch:
//   pass 1  overlap_sums_kernel: 3C + 1 grid-wide totals (I_c, P_c, Y_c, the CCE pixel sum), reduced bitwise reproducibly by
//           grid_ordered_sums (common.h); the last workgroup to arrive writes the scalar loss and the 2C coefficients A_c, B_c;
//   pass 2  overlap_bwd_kernel: d loss / d logits = p_j*(G_j - sum_c p_c*G_c), G_c = A_c*y_c + B_c (+ the CCE term), one bf16 rounding.
// What the two passes have in common with the Lovasz loss (lovasz.hip) is in region_loss.h: the loader of a thread's group of four pixels, the
// CCE arithmetic, the dlogits store, the accumulator's geometry and the checks on UssegLossDesc.  This file keeps what is Dice / Tversky.
// The boundary term (usseg.h, UssegBoundaryLoss; BD instantiations of the same two kernels): L_B = wb*ov_scale/M * sum_m sum_c u_c*p_c*phi_c with
// phi the signed distance map of the labels (sdf.hip).  Pass 1 carries one more total, reads wb from DEVICE memory, adds L_B to acc[0] and leaves
// L_B in acc[12] and the coefficient wb*ov_scale/M in acc[13]; pass 2 adds acc[13]*u_c*phi_c(m) to G_c(m) in front of the ONE bf16 rounding - and
// skips that summand when the coefficient is zero, so wb = 0 gives the bits of the plain pair.
#include "region_loss.h"

// the accumulator header (region_loss.h has its geometry): acc[0] loss, [1] ticket, [2] CCE pixel sum, [4..8) A_c, [8..12) B_c, [12] L_B,
// [13] wb*ov_scale/M, [16..20) I_c, [20..24) P_c, [24..28) Y_c, [28..32) T_c; 3C + 2 <= 14 floats of a workgroup's row of partials are used

// the parameters as the kernels take them, by value: ovk = ov_weight * ov_scale and cek = ce_weight * inv_global_batch folded on the host
struct OverlapK { float w[4]; float alpha, beta, smooth, power, ovk, cek; };
// the boundary term's arguments (BD instantiations only): u_c, bscale = ov_scale / M folded on the host, phi [M][C], the device float wb
struct BoundaryK { float u[4]; float bscale; const float* phi; const float* wb; };

// ---- pass 1 -------------------------------------------------------------------------------------------------------------------------
// K = 3C + 1 totals.  A thread adds its pixels in index order; grid_ordered_sums (common.h) adds the threads, waves and workgroups in a fixed
// order and leaves the totals with the last workgroup to arrive, whose thread 0 finishes and puts the ticket back to zero.
template <int C, bool CE, bool BD>
__global__ __launch_bounds__(256) void overlap_sums_kernel(const OverlapK k, const BoundaryK bk, const float* __restrict__ probs,
                                                            const float* __restrict__ y_true, float* acc, int M, int ngroups, float ls, float eps) {
  constexpr int K = 3 * C + 1 + (BD ? 1 : 0);       // (the boundary total is value 3C + 1, behind the CCE sum)
  __shared__ float red[4][REGION_STRIDE];
  __shared__ float fin[16][REGION_STRIDE + 1];
  __shared__ float tot[REGION_STRIDE];
  __shared__ int s_last;
  float s[K];
#pragma unroll
  for (int i = 0; i < K; ++i) s[i] = 0.f;
  for (int g = blockIdx.x * 256 + threadIdx.x; g < ngroups; g += gridDim.x * 256) {
    float p[4 * C], y[4 * C];
    region_load_group<C>(probs, g, M, p);
    region_load_group<C>(y_true, g, M, y);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int c = 0; c < C; ++c) {     // (pixels past M were loaded as zeros)
        s[c] += p[j * C + c] * y[j * C + c];
        s[C + c] += p[j * C + c];
        s[2 * C + c] += y[j * C + c];
      }
      if (CE && 4 * g + j < M) s[3 * C] += region_cce_pixel<C, false>(p + j * C, y + j * C, ls, eps, nullptr);
    }
    if constexpr (BD) {
      float f[4 * C];
      region_load_group<C>(bk.phi, g, M, f);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float t = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) t += bk.u[c] * (p[j * C + c] * f[j * C + c]);
        s[3 * C + 1] += t;
      }
    }
  }
  if (!grid_ordered_sums<K, REGION_HDR, REGION_STRIDE>(s, acc, red, fin, tot, s_last)) return;
  if (threadIdx.x == 0) {
    float lov = 0.f;
    const float r = 1.f - k.alpha - k.beta;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float I = tot[c], P = tot[C + c], Y = tot[2 * C + c];
      const float N = I + k.smooth, D = r * I + k.alpha * P + k.beta * Y + k.smooth;     // D >= N > 0 for probabilities and labels in [0, 1]
      const float T = N / D;
      const float om = fmaxf(1.f - T, 0.f);                                             // (rounding may put T one ulp above 1)
      const float pw1 = k.power == 1.f ? 1.f : powf(om, k.power - 1.f);                 // (1 - T)^(g - 1), g >= 1
      lov += k.w[c] * (pw1 * om);
      const float kc = k.ovk * k.w[c] * k.power * pw1, d2 = 1.f / (D * D);
      acc[4 + c] = -kc * (D - r * N) * d2;
      acc[8 + c] = kc * k.alpha * N * d2;
      acc[16 + c] = I; acc[20 + c] = P; acc[24 + c] = Y; acc[28 + c] = T;
    }
    const float ce = CE ? tot[3 * C] : 0.f;
    acc[2] = ce;
    float loss = k.cek * ce + k.ovk * lov;
    if constexpr (BD) {
      const float kb = *bk.wb * bk.bscale, lb = kb * tot[3 * C + 1];
      acc[12] = lb; acc[13] = kb;
      loss += lb;                                  // (wb = 0: lb is a zero, the sum the bits of the plain loss)
    }
    acc[0] = loss;                                 // OVERWRITES: no zero-fill launch in front of the kernel
    __hip_atomic_store(reinterpret_cast<unsigned*>(acc + 1), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- pass 2 -------------------------------------------------------------------------------------------------------------------------
// (the row and the quad layout of dlogits: region_store_dlogits)
template <int C, bool CE, bool QUAD, bool BD>
__global__ __launch_bounds__(256) void overlap_bwd_kernel(const float cek, const BoundaryK bk, const float* __restrict__ probs,
                                                           const float* __restrict__ y_true, const float* __restrict__ acc, bf16_t* __restrict__ dl, int M,
                                                           int ngroups, int HW, int W, float ls, float eps) {
  float A[C], B[C], U[C];
#pragma unroll
  for (int c = 0; c < C; ++c) { A[c] = acc[4 + c]; B[c] = acc[8 + c]; U[c] = BD ? acc[13] * bk.u[c] : 0.f; }
  const bool bd = BD && acc[13] != 0.f;
  for (int g = blockIdx.x * 256 + threadIdx.x; g < ngroups; g += gridDim.x * 256) {
    float p[4 * C], y[4 * C];
    region_load_group<C>(probs, g, M, p);
    region_load_group<C>(y_true, g, M, y);
    float f[BD ? 4 * C : 1];
    if constexpr (BD) {
      if (bd) region_load_group<C>(bk.phi, g, M, f);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = 4 * g + j;
      if (m >= M) break;
      float G[C];
#pragma unroll
      for (int c = 0; c < C; ++c) G[c] = A[c] * y[j * C + c] + B[c];
      if constexpr (BD) {
        if (bd) {
#pragma unroll
          for (int c = 0; c < C; ++c) G[c] += U[c] * f[j * C + c];
        }
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
static int overlap_args(const char* who, const UssegLossDesc* d, const UssegOverlapLoss* ol, const float* probs, const float* y_true,
                        const float* acc, int64_t acc_floats) {
  USSEG_CHECK_ARG(d, "%s: null descriptor", who);
  USSEG_CHECK_ARG(ol, "%s: null overlap-loss struct", who);
  USSEG_CHECK_ARG(probs && y_true && acc, "%s: null pointer", who);
  int rc = region_shape_args(who, d);
  if (rc) return rc;
  USSEG_CHECK_ARG(((uintptr_t)probs & 15) == 0 && ((uintptr_t)y_true & 15) == 0 && ((uintptr_t)acc & 3) == 0,
                  "%s: probs and y_true must be 16-byte aligned", who);
  USSEG_CHECK_ARG(std::isfinite(ol->alpha) && ol->alpha >= 0.f && std::isfinite(ol->beta) && ol->beta >= 0.f,
                  "%s: alpha and beta must be finite and >= 0", who);
  USSEG_CHECK_ARG(std::isfinite(ol->smooth) && ol->smooth > 0.f, "%s: smooth must be finite and > 0", who);
  USSEG_CHECK_ARG(ol->power >= 1.f && ol->power <= 4.f, "%s: power must lie in [1, 4]", who);
  USSEG_CHECK_ARG(std::isfinite(ol->ov_weight) && ol->ov_weight >= 0.f && std::isfinite(ol->ce_weight) && ol->ce_weight >= 0.f,
                  "%s: ov_weight and ce_weight must be finite and >= 0", who);
  for (int c = 0; c < d->C; ++c) USSEG_CHECK_ARG(std::isfinite(ol->w[c]) && ol->w[c] >= 0.f, "%s: class weights must be finite and >= 0", who);
  if ((rc = region_scale_args(who, d, ol->ce_weight))) return rc;
  USSEG_CHECK_ARG(acc_floats >= REGION_HDR, "%s: the accumulator holds fewer than its %d header floats", who, REGION_HDR);
  return USSEG_OK;
}

extern "C" int usseg_overlap_loss_grid(int64_t M) {
  const int64_t g = cdiv64(cdiv64(M > 0 ? M : 0, 4), 256);
  return (int)(g < 1 ? 1 : g > REGION_MAX_BLOCKS ? REGION_MAX_BLOCKS : g);
}

// the boundary term's arguments, checked like the rest (d->C is known to be valid here)
static int boundary_args(const char* who, const UssegLossDesc* d, const float* phi, const UssegBoundaryLoss* bl, const float* wb) {
  USSEG_CHECK_ARG(bl, "%s: null boundary-loss struct", who);
  USSEG_CHECK_ARG(phi && wb, "%s: null pointer (phi, wb)", who);
  USSEG_CHECK_ARG(((uintptr_t)phi & 15) == 0 && ((uintptr_t)wb & 3) == 0, "%s: phi must be 16-byte, wb 4-byte aligned", who);
  for (int c = 0; c < d->C; ++c) USSEG_CHECK_ARG(std::isfinite(bl->u[c]) && bl->u[c] >= 0.f, "%s: boundary class weights must be finite and >= 0", who);
  return USSEG_OK;
}
static BoundaryK boundary_k(const UssegLossDesc* d, const float* phi, const UssegBoundaryLoss* bl, const float* wb, float ov_scale) {
  BoundaryK bk = {};
  for (int c = 0; c < d->C; ++c) bk.u[c] = bl->u[c];
  bk.bscale = d->M > 0 ? (float)((double)ov_scale / (double)d->M) : 0.f;
  bk.phi = phi; bk.wb = wb;
  return bk;
}

static int overlap_sums_impl(const char* who, const UssegLossDesc* d, const UssegOverlapLoss* ol, float ov_scale, const float* probs, const float* y_true,
                             const float* phi, const UssegBoundaryLoss* bl, const float* wb, bool bd, float* acc, int64_t acc_floats,
                             usseg_stream_t stream) {
  int rc = overlap_args(who, d, ol, probs, y_true, acc, acc_floats);
  if (rc) return rc;
  if (bd && (rc = boundary_args(who, d, phi, bl, wb))) return rc;
  USSEG_CHECK_ARG(std::isfinite(ov_scale) && ov_scale >= 0.f, "%s: ov_scale must be finite and >= 0", who);
  const int grid = usseg_overlap_loss_grid(d->M);
  USSEG_CHECK_ARG(acc_floats >= REGION_HDR + (int64_t)REGION_STRIDE * grid, "%s: a grid of %d workgroups needs %d accumulator floats", who, grid,
                  REGION_HDR + REGION_STRIDE * grid);
  const BoundaryK bk = bd ? boundary_k(d, phi, bl, wb, ov_scale) : BoundaryK{};
  OverlapK k = {};
  for (int c = 0; c < d->C; ++c) k.w[c] = ol->w[c];
  k.alpha = ol->alpha; k.beta = ol->beta; k.smooth = ol->smooth; k.power = ol->power;
  k.ovk = ol->ov_weight * ov_scale;
  k.cek = ol->ce_weight * d->inv_global_batch;
  const bool ce = ol->ce_weight != 0.f;
  const int M = (int)d->M, ng = region_groups(d);
  hipStream_t s = (hipStream_t)stream;
#define OV_SUMS2(CC, CEB, BDB)                                                                                                               \
  hipLaunchKernelGGL((overlap_sums_kernel<CC, CEB, BDB>), dim3(grid), dim3(256), 0, s, k, bk, probs, y_true, acc, M, ng, CEB ? d->label_smoothing : 0.f, \
                     CEB ? d->clip_eps : 0.f)
#define OV_SUMS(CC)                                                            \
  if (ce) { if (bd) OV_SUMS2(CC, true, true); else OV_SUMS2(CC, true, false); } \
  else { if (bd) OV_SUMS2(CC, false, true); else OV_SUMS2(CC, false, false); }
  switch (d->C) {
    case 1: OV_SUMS(1) break;
    case 2: OV_SUMS(2) break;
    case 3: OV_SUMS(3) break;
    default: OV_SUMS(4) break;
  }
#undef OV_SUMS
#undef OV_SUMS2
  return usseg_check_launch(who);
}

extern "C" int usseg_overlap_loss_sums(const UssegLossDesc* d, const UssegOverlapLoss* ol, float ov_scale, const float* probs, const float* y_true,
                                       float* acc, int64_t acc_floats, usseg_stream_t stream) {
  return overlap_sums_impl("overlap_loss_sums", d, ol, ov_scale, probs, y_true, nullptr, nullptr, nullptr, false, acc, acc_floats, stream);
}

extern "C" int usseg_overlap_boundary_loss_sums(const UssegLossDesc* d, const UssegOverlapLoss* ol, float ov_scale, const float* probs, const float* y_true,
                                                const float* phi, const UssegBoundaryLoss* bl, const float* wb, float* acc, int64_t acc_floats,
                                                usseg_stream_t stream) {
  return overlap_sums_impl("overlap_boundary_loss_sums", d, ol, ov_scale, probs, y_true, phi, bl, wb, true, acc, acc_floats, stream);
}

static int overlap_bwd_impl(const char* who, const UssegLossDesc* d, const UssegOverlapLoss* ol, const float* probs, const float* y_true, const float* phi,
                            const UssegBoundaryLoss* bl, bool bd, const float* acc, int64_t acc_floats, void* dlogits, usseg_stream_t stream) {
  int rc = overlap_args(who, d, ol, probs, y_true, acc, acc_floats);
  if (rc) return rc;
  if (bd && (rc = boundary_args(who, d, phi, bl, acc))) return rc;      // (pass 2 reads the coefficient from acc[13], not wb)
  if ((rc = region_bwd_args(who, d, dlogits))) return rc;
  if (d->M == 0) return USSEG_OK;
  const BoundaryK bk = bd ? boundary_k(d, phi, bl, acc, 0.f) : BoundaryK{};
  const float cek = ol->ce_weight * d->inv_global_batch;
  const bool ce = ol->ce_weight != 0.f;
  const int M = (int)d->M, ng = region_groups(d);
  const dim3 grid = region_bwd_grid(ng);
  bf16_t* dl = (bf16_t*)dlogits;
  hipStream_t s = (hipStream_t)stream;
#define OV_BWD3(CC, CEB, Q, BDB)                                                                                                             \
  hipLaunchKernelGGL((overlap_bwd_kernel<CC, CEB, Q, BDB>), grid, dim3(256), 0, s, cek, bk, probs, y_true, acc, dl, M, ng, d->HW,              \
                     d->quad_w ? d->quad_w : 1, d->label_smoothing, d->clip_eps)
#define OV_BWD2(CC, CEB, Q) \
  if (bd) OV_BWD3(CC, CEB, Q, true); else OV_BWD3(CC, CEB, Q, false)
#define OV_BWD(CC)                                                \
  if (ce) { if (d->quad_w) { OV_BWD2(CC, true, true); } else { OV_BWD2(CC, true, false); } } \
  else { if (d->quad_w) { OV_BWD2(CC, false, true); } else { OV_BWD2(CC, false, false); } }
  switch (d->C) {
    case 1: OV_BWD(1) break;
    case 2: OV_BWD(2) break;
    case 3: OV_BWD(3) break;
    default: OV_BWD(4) break;
  }
#undef OV_BWD
#undef OV_BWD2
#undef OV_BWD3
  return usseg_check_launch(who);
}

extern "C" int usseg_overlap_loss_bwd(const UssegLossDesc* d, const UssegOverlapLoss* ol, const float* probs, const float* y_true, const float* acc,
                                      int64_t acc_floats, void* dlogits, usseg_stream_t stream) {
  return overlap_bwd_impl("overlap_loss_bwd", d, ol, probs, y_true, nullptr, nullptr, false, acc, acc_floats, dlogits, stream);
}

extern "C" int usseg_overlap_boundary_loss_bwd(const UssegLossDesc* d, const UssegOverlapLoss* ol, const float* probs, const float* y_true, const float* phi,
                                               const UssegBoundaryLoss* bl, const float* acc, int64_t acc_floats, void* dlogits, usseg_stream_t stream) {
  return overlap_bwd_impl("overlap_boundary_loss_bwd", d, ol, probs, y_true, phi, bl, true, acc, acc_floats, dlogits, stream);
}
