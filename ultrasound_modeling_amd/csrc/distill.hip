// Knowledge distillation (Hinton et al. 2015; not in the reference): include/usseg_distill.h, usseg_distill_loss.
//
//   loss = scale * ( hard_weight * sum_pixels CCE(p, y) + soft_weight * sum_pixels T^2 * KL( soften(q) || soften(p) ) )
//   soften(r)_c = softmax_c( log(r_c + 1e-7) / T )        (usseg_apply_temperature's arithmetic, operating_point.hip: temper_pixel)
//
// ONE launch behind the probabilities-only head: the gradient G_c = hard_weight*scale*dCCE/dp_c + soft_weight*scale*T*(pT_c - qT_c)/(p_c + 1e-7)
// needs no grid-wide coefficient, so the kernel that forms the two pixel sums (grid_ordered_sums, common.h) also writes dlogits
// (region_store_dlogits, region_loss.h).  A thread owns groups of four pixels: C 16-byte loads for each of p, y and q (region_load_group).
// T, soft_weight and hard_weight come from a DEVICE table read once per thread, so a captured graph follows a change of them.
//
// Bytes at 16 x 256 x 256, C = 3 (M = 2^20), quad layout: 3 tensors x 12 B + 8 B of dlogits = 44 B/pixel = 46 MB.
//
// logf / expf, not __logf / __expf, in the softening.  The soft gradient is a DIFFERENCE pT_c - qT_c of two softmax outputs whose
// exponents reach |log(1e-7)| / T = 129 at the smallest T (1/8): an absolute error d in an exponent is a RELATIVE error d in pT_c.  OCML's
// logf and expf are documented within 1 ulp, so d <= about 3 ulp(129) = 3 * 2^-16 (the log, the product with 1/T, the subtraction of the
// maximum) - a thirtieth of the bf16 unit 2^-9 the tests' bound is built on, and 3 * 2^-18 at the smallest temperature they use (0.5).  The __ forms carry no documented bound to derive a test bound
// from, and the launch is limited by its 46 MB, not by the 2C + 2 logs and 2C exps of a pixel; operating_point.hip made the same choice
// for the same function.  The hard term keeps region_cce_pixel as it is (its __logf included): it stays the arithmetic of the other
// region losses.
// fp contraction is OFF in the softening and the KL term so that both sides are the same instruction sequence: q == p (the same bits) then
// gives pT == qT and log pT == log qT bit for bit, a soft sum of exactly 0.0 and G_soft of exactly 0.
#include "region_loss.h"
#include "../../include/usseg_distill.h"

static_assert(USSEG_DISTILL_ACC_FLOATS == USSEG_OVERLAP_ACC_FLOATS, "the distillation accumulator has the region losses' geometry");
static_assert(USSEG_DISTILL_SETTINGS == 4, "usseg_distill.h documents a table of four floats");

#define DISTILL_EPS 1e-7f

// soften(r): t[c] = r_T[c], lg[c] = log r_T[c] = s_c - logsumexp(s), s_c = logf(r_c + 1e-7f) * invT; the sum in ascending class order
template <int C>
__device__ __forceinline__ void distill_soften(const float* r, float invT, float (&t)[C], float (&lg)[C]) {
#pragma clang fp contract(off)
  float s[C], m = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    s[c] = logf(r[c] + DISTILL_EPS) * invT;
    m = (c == 0 || s[c] > m) ? s[c] : m;
  }
  float e[C], sum = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    e[c] = expf(s[c] - m);
    sum += e[c];
  }
  const float lse = m + logf(sum);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    t[c] = e[c] / sum;
    lg[c] = s[c] - lse;
  }
}

// MODE 0: the loss alone; 1: dlogits in the row layout; 2: in the quad layout.
// `scale` (inv_global_batch), ls and eps are by value: nothing set_distill changes.
template <int C, int MODE>
__global__ __launch_bounds__(256) void distill_kernel(const float* __restrict__ probs, const float* __restrict__ y_true, const float* __restrict__ teacher,
                                                       const float* __restrict__ settings, float* acc, bf16_t* __restrict__ dl, int M, int ngroups, int HW,
                                                       int W, float ls, float eps, float scale) {
  __shared__ float red[4][REGION_STRIDE];
  __shared__ float fin[16][REGION_STRIDE + 1];
  __shared__ float tot[REGION_STRIDE];
  __shared__ int s_last;
  const float T = settings[0], invT = 1.f / T;                 // once per thread
  const float ks = settings[1] * scale * T, kh = settings[2] * scale;
  float s[2] = {0.f, 0.f};                                     // sum hard, sum KL (without T^2)
  for (int g = blockIdx.x * 256 + threadIdx.x; g < ngroups; g += gridDim.x * 256) {
    float p[4 * C], y[4 * C], q[4 * C];
    region_load_group<C>(probs, g, M, p);
    region_load_group<C>(y_true, g, M, y);
    region_load_group<C>(teacher, g, M, q);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = 4 * g + j;
      if (m >= M) break;
      float dce[C];
      s[0] += region_cce_pixel<C, MODE != 0>(p + j * C, y + j * C, ls, eps, dce);
      float pT[C], qT[C], lp[C], lq[C];
      distill_soften<C>(p + j * C, invT, pT, lp);
      distill_soften<C>(q + j * C, invT, qT, lq);
      {
#pragma clang fp contract(off)
        float kl = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) kl += qT[c] * (lq[c] - lp[c]);
        s[1] += kl;
      }
      if (MODE != 0) {
        float G[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
          float gs;
          {
#pragma clang fp contract(off)
            gs = ks * ((pT[c] - qT[c]) / (p[j * C + c] + DISTILL_EPS));
          }
          G[c] = kh * dce[c] + gs;
        }
        region_store_dlogits<C, MODE == 2>(G, p + j * C, dl, m, HW, W);
      }
    }
  }
  if (!grid_ordered_sums<2, REGION_HDR, REGION_STRIDE>(s, acc, red, fin, tot, s_last)) return;
  if (threadIdx.x == 0) {
    const float soft = (T * T) * tot[1];
    const float lh = kh * tot[0], lsft = (settings[1] * scale) * soft;
    acc[2] = tot[0];
    acc[3] = soft;
    acc[4] = lh;
    acc[5] = lsft;
    acc[0] = lh + lsft;                              // OVERWRITES: no zero-fill launch in front of the kernel
    __hip_atomic_store(reinterpret_cast<unsigned*>(acc + 1), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- entry points: every argument is checked before any launch ------------------------------------------------------------------------
extern "C" int usseg_distill_grid(int64_t M) { return usseg_overlap_loss_grid(M); }

extern "C" int usseg_distill_loss(const UssegDistillDesc* desc, const float* probs, const float* y_true, const float* q, const float* settings_dev,
                                  float* acc, int64_t acc_floats, void* dlogits, usseg_stream_t stream) {
  const char* who = "distill_loss";
  USSEG_CHECK_ARG(desc, "%s: null descriptor", who);
  UssegLossDesc d = {};
  d.M = desc->M; d.HW = desc->HW; d.C = desc->C; d.ldl = desc->C; d.lddl = desc->lddl; d.loss_kind = 0;
  d.label_smoothing = desc->label_smoothing; d.clip_eps = desc->clip_eps; d.inv_global_batch = desc->inv_global_batch; d.quad_w = desc->quad_w;
  int rc = region_shape_args(who, &d);
  if (rc) return rc;
  USSEG_CHECK_ARG(probs && y_true && q && settings_dev && acc, "%s: null pointer", who);
  USSEG_CHECK_ARG((((uintptr_t)probs | (uintptr_t)y_true | (uintptr_t)q) & 15) == 0, "%s: probs, y_true and q must be 16-byte aligned", who);
  USSEG_CHECK_ARG((((uintptr_t)settings_dev | (uintptr_t)acc) & 3) == 0, "%s: the settings table and acc must be 4-byte aligned", who);
  USSEG_CHECK_ARG(dlogits == nullptr || ((uintptr_t)dlogits & 15) == 0, "%s: dlogits must be a 16-byte aligned pointer", who);
  USSEG_CHECK_ARG(d.quad_w == 0 || (d.quad_w > 0 && d.quad_w % 2 == 0 && d.HW % (2 * d.quad_w) == 0), "%s: quad layout needs even H and W", who);
  USSEG_CHECK_ARG(d.lddl == (d.quad_w ? 16 : 8), "%s: dlogits stride must be 8 (16 in the quad layout)", who);
  if ((rc = region_scale_args(who, &d, 1.f))) return rc;
  const int grid = usseg_distill_grid(d.M);
  USSEG_CHECK_ARG(grid <= REGION_MAX_BLOCKS && acc_floats >= REGION_HDR + (int64_t)REGION_STRIDE * grid,
                  "%s: a grid of %d workgroups needs %d accumulator floats", who, grid, REGION_HDR + REGION_STRIDE * grid);
  hipStream_t s = (hipStream_t)stream;
  if (d.M == 0) {      // no kernel: a memset node puts the header (loss, ticket, sums, terms) to zero
    if (hipMemsetAsync(acc, 0, REGION_HDR * sizeof(float), s) != hipSuccess) return usseg_check_launch(who);
    return usseg_check_launch(who);
  }
  const int M = (int)d.M, ng = region_groups(&d);
  bf16_t* dl = (bf16_t*)dlogits;
#define DS_RUN(CC, MODE)                                                                                                                      \
  hipLaunchKernelGGL((distill_kernel<CC, MODE>), dim3(grid), dim3(256), 0, s, probs, y_true, q, settings_dev, acc, dl, M, ng, d.HW, \
                     d.quad_w ? d.quad_w : 1, d.label_smoothing, d.clip_eps, d.inv_global_batch)
#define DS_C(CC) \
  if (!dl) DS_RUN(CC, 0); else if (d.quad_w) DS_RUN(CC, 2); else DS_RUN(CC, 1)
  switch (d.C) {
    case 1: DS_C(1); break;
    case 2: DS_C(2); break;
    case 3: DS_C(3); break;
    default: DS_C(4); break;
  }
#undef DS_C
#undef DS_RUN
  return usseg_check_launch(who);
}
