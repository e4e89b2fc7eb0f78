// The per-element arithmetic of the AdamW update, shared by adamw_kernel (attn_loss_optim.hip) and the update fused with the weight
// average (average.hip): one definition, so both launches give the same bits of p, m and v.
#pragma once

// tfa DecoupledWeightDecayExtension: p - wd_t*p, two roundings (a fused multiply-add would round once)
__device__ __forceinline__ float decoupled_decay(float p, float wd_t) {
#pragma clang fp contract(off)
  return p - wd_t * p;
}
// one element of the update: the decay (if on), then adam_kernel's arithmetic on the decayed p.  adam_kernel's two moment statements
// compile to fma(b1, m, (1-b1)*g') and fma(b2, v, ((1-b2)*g')*g'); left to contraction, the scalar tail here fused the OTHER product
// (fma((1-b1), g', b1*m)), which differs in the last bit now and then, so the contraction is written out
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, bool decay, float scale, float lr_t, float wd_t, float b1, float b2,
                                           float eps) {
  float pi = decay ? decoupled_decay(p, wd_t) : p;
  float gi = g * scale;
  float mi = fmaf(b1, m, (1.f - b1) * gi);
  float vi = fmaf(b2, v, (1.f - b2) * gi * gi);
  m = mi;
  v = vi;
  pi -= lr_t * mi / (sqrtf(vi) + eps);
  p = pi;
}
