// The body of stem_fwd_kernel / stem_fwd_infer_kernel (stem.hip): included inside each kernel, with `constexpr bool STASH` and `p` in scope.
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char lds[];
  bf16_t* const XT = reinterpret_cast<bf16_t*>(lds);
  bf16_t* const Y1T = reinterpret_cast<bf16_t*>(lds + XS_B);
  bf16_t* const T1T = reinterpret_cast<bf16_t*>(lds + XS_B + Y1_B);
  bf16_t* const C2T = reinterpret_cast<bf16_t*>(lds);          // reuses the x + y1 region once convtmp_1 has read them
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  // (a persistent form that keeps all 31 weight fragments in registers across tiles was measured: 264 VGPRs = one workgroup per CU, 133 us
  // against 80 us - the tile is a chain of five barrier-separated phases and needs its three co-resident workgroups more than it needs
  // the 125 KB of fragment reloads per tile removed)
  WFrag<1, 1> wf1;
  WFrag<2, 2> wf2;
  wf1.load(p.w1, r, q);
  wf2.load(p.w2, r, q);
  {
  const int b = blockIdx.y, tile = blockIdx.x;
  const int tyi = tile / p.tiles_x, txi = tile - tyi * p.tiles_x;
  const int ty0 = tyi * TH, tx0 = txi * T;
  const int64_t img = (int64_t)b * p.H * p.W;
  // ---- x tile + 3-pixel halo (zeros outside the image): both loads of a thread before its LDS stores
  {
    uint4 v[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int hp = tid + 256 * i;
      const int hy = hp / XW, hx = hp - hy * XW;
      const int gy = ty0 - 3 + hy, gx = tx0 - 3 + hx;
      v[i] = (hp < XW * XH && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W)
                 ? *reinterpret_cast<const uint4*>(p.x + (img + (int64_t)gy * p.W + gx) * p.ldx) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int hp = tid + 256 * i;
      if (hp < XW * XH) *reinterpret_cast<uint4*>(XT + hp * XS) = v[i];
    }
  }
  __syncthreads();
  // ---- conv1 + LeakyReLU on the 20x20 pixels convtmp_1 needs (ResNest.py:39-40)
  conv_phase<1, 1, Y1W, Y1H, XS, Y1S, true, true>(XT, Y1T, wf1, p.b1, p.alpha, ty0 - 2, tx0 - 2, p.H, p.W, wv, r, q);
  WFrag<4, 2> wf3;
  wf3.load(p.w3, r, q);                   // in flight during convtmp_1
  __syncthreads();
  if constexpr (STASH) store_interior<Y1W, 2, 2, Y1S>(Y1T, p.y1, img, 16, ty0, tx0, p.H, p.W, tid);
  // ---- convtmp_1 + folded BatchNorm + LeakyReLU on the 18x18 pixels convtmp_2 needs (:41-43)
  conv_phase<2, 2, T1W, T1H, Y1S, T1S, true, true>(Y1T, T1T, wf2, p.b2, p.alpha, ty0 - 1, tx0 - 1, p.H, p.W, wv, r, q);
  __syncthreads();
  if constexpr (STASH) store_interior<T1W, 1, 4, T1S>(T1T, p.t1, img, 32, ty0, tx0, p.H, p.W, tid);
  // ---- convtmp_2 (:44): the pre-norm output, kept for the BatchNorm backward
  conv_phase<4, 2, T, TH, T1S, C2S, false, false>(T1T, C2T, wf3, p.b3, 0.f, ty0, tx0, p.H, p.W, wv, r, q);
  __syncthreads();
  if constexpr (STASH) store_interior<T, 0, 4, C2S>(C2T, p.c2, img, 32, ty0, tx0, p.H, p.W, tid);
  // ---- BatchNorm + LeakyReLU + 2x2 average pool (:45-47): one (pooled pixel, 8-channel chunk) per thread; the activation is rounded to
  //      bf16 before the pool, as the two-launch form stores it
  if (tid < (T / 2) * (TH / 2) * 4) {
    const int pp = tid >> 2, c = tid & 3;
    const int oy = pp >> 3, ox = pp & 7;
    const int gy = (ty0 >> 1) + oy, gx = (tx0 >> 1) + ox;
    float ga[8], be[8], mu[8], rs[8];
    *reinterpret_cast<float4*>(ga) = *reinterpret_cast<const float4*>(p.gamma + c * 8);
    *reinterpret_cast<float4*>(ga + 4) = *reinterpret_cast<const float4*>(p.gamma + c * 8 + 4);
    *reinterpret_cast<float4*>(be) = *reinterpret_cast<const float4*>(p.beta + c * 8);
    *reinterpret_cast<float4*>(be + 4) = *reinterpret_cast<const float4*>(p.beta + c * 8 + 4);
    *reinterpret_cast<float4*>(mu) = *reinterpret_cast<const float4*>(p.mean + c * 8);
    *reinterpret_cast<float4*>(mu + 4) = *reinterpret_cast<const float4*>(p.mean + c * 8 + 4);
    *reinterpret_cast<float4*>(rs) = *reinterpret_cast<const float4*>(p.var + c * 8);
    *reinterpret_cast<float4*>(rs + 4) = *reinterpret_cast<const float4*>(p.var + c * 8 + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) rs[j] = rsqrtf(rs[j] + p.eps);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int iy = 2 * oy + (s >> 1), ix = 2 * ox + (s & 1);
      float xv[8], o[8], r8[8];
      unpack8(*reinterpret_cast<const uint4*>(C2T + (iy * T + ix) * C2S + c * 8), xv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = ga[j] * ((xv[j] - mu[j]) * rs[j]) + be[j];
        o[j] = v >= 0.f ? v : p.alpha * v;
      }
      unpack8(pack8(o), r8);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += r8[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= 0.25f;
    if (gy < (p.H >> 1) && gx < (p.W >> 1))
      *reinterpret_cast<uint4*>(p.pooled + ((int64_t)b * (p.H >> 1) * (p.W >> 1) + (int64_t)gy * (p.W >> 1) + gx) * 32 + c * 8) = pack8(acc);
  }
  }
#endif
