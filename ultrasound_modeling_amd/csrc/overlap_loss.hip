// Region-overlap losses (soft Dice / Tversky, optionally plus CategoricalCrossentropy) on the head's probabilities: usseg.h, UssegOverlapLoss.
// The gradient at one pixel depends on sums over every pixel of the call, so the loss cannot ride in the fused head launch the way the
// per-pixel losses do.  Two passes over probs / y_true (fp32 [M][C], C <= 4) behind today's probabilities-only head launch:
//   pass 1  overlap_sums_kernel: 3C + 1 grid-wide totals (I_c, P_c, Y_c, the CCE pixel sum), reduced bitwise reproducibly with the K-value
//           form of grid_ordered_sum (common.h); the last workgroup to arrive writes the scalar loss and the 2C coefficients A_c, B_c;
//   pass 2  overlap_bwd_kernel: d loss / d logits = p_j*(G_j - sum_c p_c*G_c), G_c = A_c*y_c + B_c (+ the CCE term), one bf16 rounding.
// A thread owns GROUPS of four consecutive pixels: 4*C floats = C 16-byte loads per tensor whatever C is (the base pointers are 16-byte
// aligned, checked by the entry points); the last group of an M that is no multiple of 4 takes guarded scalar loads.
// The CCE arithmetic restates loss_kind 0 of attn_loss_optim.hip (softmax_loss_pixel) rather than sharing it through a header: that
// file's kernels stay instruction for instruction what they were.
// The boundary term (usseg.h, UssegBoundaryLoss; BD instantiations of the same two kernels): L_B = wb*ov_scale/M * sum_m sum_c u_c*p_c*phi_c with
// phi the signed distance map of the labels (sdf.hip).  Pass 1 carries one more total, reads wb from DEVICE memory, adds L_B to acc[0] and leaves
// L_B in acc[12] and the coefficient wb*ov_scale/M in acc[13]; pass 2 adds acc[13]*u_c*phi_c(m) to G_c(m) in front of the ONE bf16 rounding - and
// skips that summand when the coefficient is zero, so wb = 0 gives the bits of the plain pair.
#include "common.h"
#include <cmath>

#define OV_HDR 32        // acc[0] loss, [1] ticket, [2] CCE pixel sum, [4..8) A_c, [8..12) B_c, [12] L_B, [13] wb*ov_scale/M, [16..20) I_c, [20..24) P_c, [24..28) Y_c, [28..32) T_c
#define OV_STRIDE 16     // floats per workgroup row of partials (3C + 2 <= 14 used): acc[OV_HDR + 16*b + k]
#define OV_MAX_BLOCKS ((USSEG_OVERLAP_ACC_FLOATS - OV_HDR) / OV_STRIDE)
static_assert(OV_MAX_BLOCKS == 512, "usseg.h documents the grid rule with 512 workgroups");

// the parameters as the kernels take them, by value: ovk = ov_weight * ov_scale and cek = ce_weight * inv_global_batch folded on the host
struct OverlapK { float w[4]; float alpha, beta, smooth, power, ovk, cek; };
// the boundary term's arguments (BD instantiations only): u_c, bscale = ov_scale / M folded on the host, phi [M][C], the device float wb
struct BoundaryK { float u[4]; float bscale; const float* phi; const float* wb; };

template <int C>
__device__ __forceinline__ void ov_load_group(const float* __restrict__ base, int g, int M, float (&v)[4 * C]) {
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
__device__ __forceinline__ float ov_cce_pixel(const float* p, const float* y, float ls, float eps, float* dLdp) {
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

// ---- pass 1 -------------------------------------------------------------------------------------------------------------------------
// K = 3C + 1 totals.  Within a workgroup: a thread adds its pixels in index order, a wave its lanes by a butterfly, thread k < K the four
// waves as (0+1)+(2+3).  Across workgroups, grid_ordered_sum's construction for K values: lanes 0..K-1 of wave 0 publish the K totals with
// ONE returning agent-scope exchange instruction, all K return values are folded into the operand of the ticket add (so the add cannot
// issue before every partial is at the memory side), and the LAST workgroup to arrive adds the rows in a fixed order - thread (j, k) the
// workgroups j, j+16, j+32, ... of value k, then thread k the sixteen j as a balanced tree.  No workgroup waits for another; no float
// atomics; the ticket is back at zero when the kernel ends.  tools/check_ordered_sum.py checks the ISA of this sequence on every build.
template <int C, bool CE, bool BD>
__global__ __launch_bounds__(256) void overlap_sums_kernel(const OverlapK k, const BoundaryK bk, const float* __restrict__ probs,
                                                            const float* __restrict__ y_true, float* acc, int M, int ngroups, float ls, float eps) {
  constexpr int K = 3 * C + 1 + (BD ? 1 : 0);       // (the boundary total is value 3C + 1, behind the CCE sum)
  __shared__ float red[4][OV_STRIDE];
  __shared__ float fin[16][OV_STRIDE + 1];
  __shared__ float tot[OV_STRIDE];
  __shared__ int s_last;
  float s[K];
#pragma unroll
  for (int i = 0; i < K; ++i) s[i] = 0.f;
  for (int g = blockIdx.x * 256 + threadIdx.x; g < ngroups; g += gridDim.x * 256) {
    float p[4 * C], y[4 * C];
    ov_load_group<C>(probs, g, M, p);
    ov_load_group<C>(y_true, g, M, y);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int c = 0; c < C; ++c) {     // (pixels past M were loaded as zeros)
        s[c] += p[j * C + c] * y[j * C + c];
        s[C + c] += p[j * C + c];
        s[2 * C + c] += y[j * C + c];
      }
      if (CE && 4 * g + j < M) s[3 * C] += ov_cce_pixel<C, false>(p + j * C, y + j * C, ls, eps, nullptr);
    }
    if constexpr (BD) {
      float f[4 * C];
      ov_load_group<C>(bk.phi, g, M, f);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float t = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) t += bk.u[c] * (p[j * C + c] * f[j * C + c]);
        s[3 * C + 1] += t;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < K; ++i) {
    float v = s[i];
    for (int msk = 32; msk >= 1; msk >>= 1) v += __shfl_xor(v, msk, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = v;
  }
  __syncthreads();
  const int nb = gridDim.x;
  if (threadIdx.x < 64) {
    unsigned zero = 0u;
    if (threadIdx.x < K) {
      const float t = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
      const float old = __hip_atomic_exchange(acc + OV_HDR + blockIdx.x * OV_STRIDE + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("; ticket after the partials are at the memory side" : "+v"(zero) : "v"(old));
    }
    for (int msk = 8; msk >= 1; msk >>= 1) zero |= __shfl_xor(zero, msk, 64);     // lane 0 holds a value that depends on all K returns (K <= 14)
    if (threadIdx.x == 0) {
      const unsigned tk = __hip_atomic_fetch_add(reinterpret_cast<unsigned*>(acc + 1), 1u + zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_last = (tk == (unsigned)nb - 1u);
    }
  }
  __syncthreads();
  if (!s_last) return;
  {
    const int kk = threadIdx.x & 15, j = threadIdx.x >> 4;
    float v = 0.f;
    for (int b0 = j; b0 < nb; b0 += 16 * 8) {     // eight independent loads in flight, added in workgroup order
      float t[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int b = b0 + 16 * i;
        t[i] = (b < nb && kk < K) ? __hip_atomic_load(acc + OV_HDR + b * OV_STRIDE + kk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) v += t[i];
    }
    fin[j][kk] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int c = threadIdx.x;
    float a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = fin[2 * i][c] + fin[2 * i + 1][c];
    tot[c] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  }
  __syncthreads();
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
// Row layout: dl[m*8 + c], one 16-byte store per pixel with the pad channels zero.  Quad layout (UssegLossDesc.quad_w): pixel (y, x) in
// slot 4*((y&1)*2 + (x&1)) of the 16-channel pixel (y/2, x/2), one 8-byte store per pixel - the four pixels of a 2x2 block fill all 16.
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
    ov_load_group<C>(probs, g, M, p);
    ov_load_group<C>(y_true, g, M, y);
    float f[BD ? 4 * C : 1];
    if constexpr (BD) {
      if (bd) ov_load_group<C>(bk.phi, g, M, f);
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
        ov_cce_pixel<C, true>(p + j * C, y + j * C, ls, eps, dce);
#pragma unroll
        for (int c = 0; c < C; ++c) G[c] += dce[c] * cek;
      }
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) dot += G[c] * p[j * C + c];
      float o[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = c < C ? p[j * C + (c < C ? c : 0)] * (G[c < C ? c : 0] - dot) : 0.f;
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
  }
}

// ---- entry points: every argument is checked before any launch ------------------------------------------------------------------------
static int overlap_args(const char* who, const UssegLossDesc* d, const UssegOverlapLoss* ol, const float* probs, const float* y_true,
                        const float* acc, int64_t acc_floats) {
  USSEG_CHECK_ARG(d, "%s: null descriptor", who);
  USSEG_CHECK_ARG(ol, "%s: null overlap-loss struct", who);
  USSEG_CHECK_ARG(probs && y_true && acc, "%s: null pointer", who);
  USSEG_CHECK_ARG(d->C >= 1 && d->C <= 4, "%s: 1 <= C <= 4", who);
  USSEG_CHECK_ARG(d->HW > 0 && d->M >= 0 && d->M % d->HW == 0, "%s: M must be a non-negative multiple of HW", who);
  USSEG_CHECK_ARG(d->M <= (1 << 29), "%s: more than 2^29 pixels", who);
  USSEG_CHECK_ARG(((uintptr_t)probs & 15) == 0 && ((uintptr_t)y_true & 15) == 0 && ((uintptr_t)acc & 3) == 0,
                  "%s: probs and y_true must be 16-byte aligned", who);
  USSEG_CHECK_ARG(std::isfinite(ol->alpha) && ol->alpha >= 0.f && std::isfinite(ol->beta) && ol->beta >= 0.f,
                  "%s: alpha and beta must be finite and >= 0", who);
  USSEG_CHECK_ARG(std::isfinite(ol->smooth) && ol->smooth > 0.f, "%s: smooth must be finite and > 0", who);
  USSEG_CHECK_ARG(ol->power >= 1.f && ol->power <= 4.f, "%s: power must lie in [1, 4]", who);
  USSEG_CHECK_ARG(std::isfinite(ol->ov_weight) && ol->ov_weight >= 0.f && std::isfinite(ol->ce_weight) && ol->ce_weight >= 0.f,
                  "%s: ov_weight and ce_weight must be finite and >= 0", who);
  for (int c = 0; c < d->C; ++c) USSEG_CHECK_ARG(std::isfinite(ol->w[c]) && ol->w[c] >= 0.f, "%s: class weights must be finite and >= 0", who);
  USSEG_CHECK_ARG(std::isfinite(d->inv_global_batch) && d->inv_global_batch >= 0.f, "%s: inv_global_batch must be finite and >= 0", who);
  if (ol->ce_weight != 0.f) {
    USSEG_CHECK_ARG(d->label_smoothing >= 0.f && d->label_smoothing < 1.f, "%s: label_smoothing must lie in [0, 1)", who);
    USSEG_CHECK_ARG(d->clip_eps > 0.f && 1.f - d->clip_eps < 1.f && d->clip_eps < 0.5f, "%s: clip_eps must be > 0 and representable below 1 in fp32", who);
  }
  USSEG_CHECK_ARG(acc_floats >= OV_HDR, "%s: the accumulator holds fewer than its %d header floats", who, OV_HDR);
  return USSEG_OK;
}
static inline int overlap_groups(const UssegLossDesc* d) { return (int)((d->M + 3) / 4); }

extern "C" int usseg_overlap_loss_grid(int64_t M) {
  const int64_t g = cdiv64(cdiv64(M > 0 ? M : 0, 4), 256);
  return (int)(g < 1 ? 1 : g > OV_MAX_BLOCKS ? OV_MAX_BLOCKS : g);
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
  USSEG_CHECK_ARG(acc_floats >= OV_HDR + (int64_t)OV_STRIDE * grid, "%s: a grid of %d workgroups needs %d accumulator floats", who, grid,
                  OV_HDR + OV_STRIDE * grid);
  const BoundaryK bk = bd ? boundary_k(d, phi, bl, wb, ov_scale) : BoundaryK{};
  OverlapK k = {};
  for (int c = 0; c < d->C; ++c) k.w[c] = ol->w[c];
  k.alpha = ol->alpha; k.beta = ol->beta; k.smooth = ol->smooth; k.power = ol->power;
  k.ovk = ol->ov_weight * ov_scale;
  k.cek = ol->ce_weight * d->inv_global_batch;
  const bool ce = ol->ce_weight != 0.f;
  const int M = (int)d->M, ng = overlap_groups(d);
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
  USSEG_CHECK_ARG(dlogits && ((uintptr_t)dlogits & 15) == 0, "%s: dlogits must be a 16-byte aligned pointer", who);
  USSEG_CHECK_ARG(d->quad_w == 0 || (d->quad_w > 0 && d->quad_w % 2 == 0 && d->HW % (2 * d->quad_w) == 0), "%s: quad layout needs even H and W", who);
  USSEG_CHECK_ARG(d->lddl == (d->quad_w ? 16 : 8), "%s: dlogits stride must be 8 (16 in the quad layout)", who);
  if (d->M == 0) return USSEG_OK;
  const BoundaryK bk = bd ? boundary_k(d, phi, bl, acc, 0.f) : BoundaryK{};
  const float cek = ol->ce_weight * d->inv_global_batch;
  const bool ce = ol->ce_weight != 0.f;
  const int M = (int)d->M, ng = overlap_groups(d);
  int64_t g = cdiv64(ng, 256);
  if (g > 2048) g = 2048;
  const dim3 grid((unsigned)g);
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
