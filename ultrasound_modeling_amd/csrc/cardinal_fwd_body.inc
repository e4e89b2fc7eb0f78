// The body of cardinal_fwd_kernel / cardinal_fwd_infer_kernel (cardinal.hip): included inside each kernel, with the template parameters
// CIN, CV11, CVKK, OC, `constexpr bool STASH` and `p` in scope.
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char lds[];
  using Cfg = CardCfg<CIN, CV11, CVKK, OC>;
  constexpr int UP = Cfg::UP, VP = Cfg::VP;
  constexpr int CX = Cfg::CX, CU = Cfg::CU, S1 = Cfg::S1, S2 = Cfg::S2, S3 = Cfg::S3;

  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int b = blockIdx.y, tile = blockIdx.x;
  const int tyi = tile / p.tiles_x, txi = tile - tyi * p.tiles_x;
  const int ty0 = tyi * TILE, tx0 = txi * TILE;
  const int64_t img = (int64_t)b * p.H * p.W;
  constexpr int KS1 = CIN / 32;

  if (blockIdx.z == 1) {
    // ================================================================ shortcut: sc_raw = x . Wsc^T + bsc -> LayerNorm -> LeakyReLU (ResNest.py:99-101)
    bf16_t* const XS = reinterpret_cast<bf16_t*>(lds);
    bf16_t* const SS = reinterpret_cast<bf16_t*>(lds + NPIX * CX * 2);
    float* const STAT = reinterpret_cast<float*>(lds + NPIX * CX * 2 + NPIX * S3 * 2);
    constexpr int NTS = OC / 16, NPASS = NTS > 16 ? NTS / 16 : 1, NTWS = (NTS > 16 ? 16 : NTS) / 4;
    CARD_STAMP(0);
    bf16x8_t a3[PF][NTWS];
    auto wsc_frag = [&](int pass, int ks, int j) -> bf16x8_t {
      const int nt = pass * 16 + wv + 4 * j;
      return ldg_frag(p.wsc + (int64_t)(nt * 16 + r) * CIN + ks * 32 + q * 8);
    };
#pragma unroll
    for (int s = 0; s < PF; ++s)
#pragma unroll
      for (int j = 0; j < NTWS; ++j) a3[s][j] = s < KS1 ? wsc_frag(0, s, j) : zero_frag();
    load_rows<NPIX, CIN, CX>(XS, tid, [&](int pp) -> const bf16_t* {
      const int gy = ty0 + (pp >> 3), gx = tx0 + (pp & 7);
      return (gy < p.H && gx < p.W) ? p.x + (img + (int64_t)gy * p.W + gx) * p.ldx : nullptr;
    });
    __syncthreads();
    CARD_STAMP(1);
#pragma unroll 1
    for (int pass = 0; pass < NPASS; ++pass) {
      f32x4_t acc[4][NTWS];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NTWS; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      if (pass > 0) {
#pragma unroll
        for (int s = 0; s < PF; ++s)
#pragma unroll
          for (int j = 0; j < NTWS; ++j) a3[s][j] = s < KS1 ? wsc_frag(pass, s, j) : zero_frag();
      }
#pragma unroll
      for (int ks0 = 0; ks0 < KS1; ks0 += PF)
#pragma unroll
        for (int s = 0; s < PF; ++s) {
          const int ks = ks0 + s;
          if (ks < KS1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const bf16x8_t bx = *reinterpret_cast<const bf16x8_t*>(XS + (i * 16 + r) * CX + ks * 32 + q * 8);
#pragma unroll
              for (int j = 0; j < NTWS; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a3[s][j], bx, acc[i][j], 0, 0, 0);
            }
            if (ks + PF < KS1) {
#pragma unroll
              for (int j = 0; j < NTWS; ++j) a3[s][j] = wsc_frag(pass, ks + PF, j);
            }
          }
        }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int pp = i * 16 + r;
#pragma unroll
        for (int j = 0; j < NTWS; ++j) {
          const int ch = (pass * 16 + wv + 4 * j) * 16 + 4 * q;
          const float4 bb = *reinterpret_cast<const float4*>(p.bsc + ch);
          uint2 o;
          o.x = pack2bf(acc[i][j][0] + bb.x, acc[i][j][1] + bb.y);
          o.y = pack2bf(acc[i][j][2] + bb.z, acc[i][j][3] + bb.w);
          *reinterpret_cast<uint2*>(SS + pp * S3 + ch) = o;
        }
      }
    }
    __syncthreads();
    CARD_STAMP(2);
    constexpr int NCH3 = OC / 8;
    auto rowptr = [&](bf16_t* base, int pp) -> bf16_t* {
      const int gy = ty0 + (pp >> 3), gx = tx0 + (pp & 7);
      return (gy < p.H && gx < p.W) ? base + (img + (int64_t)gy * p.W + gx) * p.ldsc : nullptr;
    };
    if constexpr (STASH) {
      for (int it = tid; it < NPIX * NCH3; it += 256) {       // sc_raw -> HBM, whole rows, before the norm overwrites the staging tile
        const int pp = it / NCH3, c = it - pp * NCH3;
        bf16_t* dst = rowptr(p.sc_raw, pp);
        if (dst) *reinterpret_cast<uint4*>(dst + c * 8) = *reinterpret_cast<const uint4*>(SS + pp * S3 + c * 8);
      }
    }
    CARD_STAMP(3);
    tile_layernorm<1, NCH3, OC, 1>(SS, S3, NPIX, STAT, p.gsc, p.besc, p.eps, p.alpha, wv, lane, SS, S3, true);
    __syncthreads();
    CARD_STAMP(4);
    for (int it = tid; it < NPIX * NCH3; it += 256) {
      const int pp = it / NCH3, c = it - pp * NCH3;
      bf16_t* dst = rowptr(p.sc, pp);
      if (dst) *reinterpret_cast<uint4*>(dst + c * 8) = *reinterpret_cast<const uint4*>(SS + pp * S3 + c * 8);
    }
    CARD_STAMP(5);
    return;
  }

  // ================================================================== cardinal chain (ResNest.py:136-147, all paths)
  bf16_t* const XS = reinterpret_cast<bf16_t*>(lds);
  bf16_t* const US = reinterpret_cast<bf16_t*>(lds + Cfg::XS_B);
  bf16_t* const SS = reinterpret_cast<bf16_t*>(lds + Cfg::XS_B + Cfg::US_B);
  float* const STAT = reinterpret_cast<float*>(lds + Cfg::XS_B + Cfg::US_B + Cfg::SSA_E * 2);

  CARD_STAMP(0);
  // ---- GEMM 1 weight fragments, ALL K steps, issued before anything else (their latency hides under the tile load).  Up to three channel
  //      tiles: wave w takes pixel tiles w and w+4 and every channel tile; six (the 256-channel stage): wave w takes channel tiles w and w+4
  //      and every pixel tile, so that its K-step fragments (2 x 8) fit in registers up front
  constexpr int NT1 = (UP + 15) / 16;
  constexpr bool NSPLIT = NT1 >= 4;
  constexpr int NA1 = NSPLIT ? 2 : NT1, MA1 = NSPLIT ? 7 : 2;
  static_assert(KS1 <= 8 && (NSPLIT || KS1 <= 4), "GEMM 1 keeps every K step's weight fragments in registers");
  bf16x8_t a1[KS1][NA1];
#pragma unroll
  for (int s = 0; s < KS1; ++s)
#pragma unroll
    for (int j = 0; j < NA1; ++j) {
      const int nt = NSPLIT ? wv + 4 * j : j;
      a1[s][j] = nt < NT1 ? ldg_frag(p.w1 + (int64_t)(nt * 16 + r) * CIN + s * 32 + q * 8) : zero_frag();
    }

  // ---- A: x tile + one-pixel halo -> LDS (zeros outside the image)
  load_rows<NHALO, CIN, CX>(XS, tid, [&](int hp) -> const bf16_t* {
    const int hy = hp / LW, hx = hp - hy * LW;
    const int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
    return (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) ? p.x + (img + (int64_t)gy * p.W + gx) * p.ldx : nullptr;
  });
  __syncthreads();
  CARD_STAMP(1);

  // ---- B: u_raw[halo pixel][Up] = x . W1^T + b1 for the 100 halo pixels (7 pixel tiles of 16)
  {
    f32x4_t acc[MA1][NA1];
#pragma unroll
    for (int i = 0; i < MA1; ++i)
#pragma unroll
      for (int j = 0; j < NA1; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    int prow[MA1];
#pragma unroll
    for (int i = 0; i < MA1; ++i) {
      const int pp = (NSPLIT ? i : wv + 4 * i) * 16 + r;
      prow[i] = (pp < NHALO ? pp : NHALO - 1) * CX;
    }
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks)
#pragma unroll
      for (int i = 0; i < MA1; ++i)
        if (NSPLIT || wv + 4 * i < 7) {
          const bf16x8_t bx = *reinterpret_cast<const bf16x8_t*>(XS + prow[i] + ks * 32 + q * 8);
#pragma unroll
          for (int j = 0; j < NA1; ++j)
            if (!NSPLIT || wv + 4 * j < NT1) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[ks][j], bx, acc[i][j], 0, 0, 0);
        }
#pragma unroll
    for (int i = 0; i < MA1; ++i) {
      const int mt = NSPLIT ? i : wv + 4 * i;
      const int pp = mt * 16 + r;
      if (mt < 7 && pp < NHALO) {
#pragma unroll
        for (int j = 0; j < NA1; ++j) {
          const int ch = (NSPLIT ? wv + 4 * j : j) * 16 + 4 * q;
          if (ch < UP) {
            const float4 bb = *reinterpret_cast<const float4*>(p.b1 + ch);
            uint2 o;
            o.x = pack2bf(acc[i][j][0] + bb.x, acc[i][j][1] + bb.y);
            o.y = pack2bf(acc[i][j][2] + bb.z, acc[i][j][3] + bb.w);
            *reinterpret_cast<uint2*>(SS + pp * S1 + ch) = o;
          }
        }
      }
    }
  }
  // GEMM 2 = the grouped 3x3: block diagonal, so wave g < 3 computes PATH g only - its CVKK output channels from its CV11 input channels
  // (the 8-channel chunks that cover them; the foreign channels inside those chunks meet zero weights), all four pixel tiles: 1 / 2.4 of the
  // dense K x N work and weight bytes, and each weight fragment is pulled through this CU's L1 exactly once (the workgroup is bound by its
  // ~20 B/clk of L2 -> L1 traffic, not by MFMA).  Its first K steps' weight fragments are in flight during the row pass.
  constexpr int TPP = (CVKK + 15) / 16, PF2 = TPP > 4 ? 3 : PF;
  const int pcb = (wv * CV11) / 8, pnck = ((wv + 1) * CV11 + 7) / 8 - pcb, pn0 = wv * CVKK;     // chunk base / chunks per tap / first channel
  const int pnch = 9 * pnck, KSg = (pnch + 3) / 4;
  // No select on the loaded value (`ok ? v : 0` made the compiler wait for every fragment right behind its load - vmcnt(0) - so nothing was
  // ever in flight): a K chunk past the path's last one re-reads the last chunk and meets a ZEROED pixel fragment below, a row past the
  // path's last channel re-reads the last row and lands in accumulator rows that are never stored.
  auto w2_frag = [&](int ks, int j) -> bf16x8_t {
    int chunk = 4 * ks + q, row = 16 * j + r;
    chunk = chunk < pnch ? chunk : pnch - 1;
    row = row < CVKK ? row : CVKK - 1;
    const int tap = chunk / pnck, choff = chunk - tap * pnck;
    return ldg_frag(p.w2 + (int64_t)(pn0 + row) * (9 * UP) + tap * UP + (pcb + choff) * 8);
  };
  bf16x8_t a2[PF2][TPP];
  if (wv < 3) {
#pragma unroll
    for (int s = 0; s < PF2; ++s)
#pragma unroll
      for (int j = 0; j < TPP; ++j) a2[s][j] = w2_frag(s, j);
  }
  __syncthreads();
  CARD_STAMP(2);

  // ---- C: per-path LayerNorm + LeakyReLU of the 100 halo pixels: u -> LDS (ZERO outside the image: the 3x3 conv pads the normalised
  //         tensor); u_raw / u of the interior pixels -> HBM in whole rows
  {
    const int hp = (wv & 1) * 64 + lane;
    const int hy = hp / LW, hx = hp - hy * LW;
    const int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
    const bool inimg = hp < NHALO && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
    tile_layernorm<2, UP / 8, CV11, 3>(SS, S1, NHALO, STAT, p.g1, p.be1, p.eps, p.alpha, wv, lane, US, CU, inimg);
  }
  __syncthreads();
  CARD_STAMP(3);
  constexpr int CPT = UP / 8;
  if constexpr (STASH) {
    for (int it = tid; it < NPIX * CPT; it += 256) {
      const int pp = it / CPT, c = it - pp * CPT;
      const int gy = ty0 + (pp >> 3), gx = tx0 + (pp & 7);
      if (gy < p.H && gx < p.W) {
        const int hp = ((pp >> 3) + 1) * LW + (pp & 7) + 1;
        const int64_t gp = (img + (int64_t)gy * p.W + gx) * p.ldu + c * 8;
        *reinterpret_cast<uint4*>(p.u_raw + gp) = *reinterpret_cast<const uint4*>(SS + hp * S1 + c * 8);
        *reinterpret_cast<uint4*>(p.u + gp) = *reinterpret_cast<const uint4*>(US + hp * CU + c * 8);
      }
    }
  }

  CARD_STAMP(4);
  // ---- D: v_raw[interior pixel][path channels] = conv3x3(u) + b2: implicit GEMM over K = (tap, 8-channel chunk of the path) from the LDS u tile
  {
    f32x4_t acc[4][TPP];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < TPP; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (wv < 3) {
      int pbase[4];   // halo index of the (0,0) tap of this lane's pixel in each pixel tile
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int pp = i * 16 + r;
        pbase[i] = (pp >> 3) * LW + (pp & 7);
      }
#pragma unroll 1
      for (int ks0 = 0; ks0 < KSg; ks0 += PF2) {
#pragma unroll
        for (int s = 0; s < PF2; ++s) {
          const int ks = ks0 + s;
          {   // (no `ks < KSg` branch: a step past the end multiplies clamped weights with zeroed pixel fragments; a branch here makes the
              //  compiler drain every weight load in flight - vmcnt(0) - at its join)
            const int chunk = 4 * ks + q;
            const bool kv = chunk < pnch;
            const int tap = kv ? chunk / pnck : 0, choff = kv ? chunk - tap * pnck : 0;
            const int dy = tap / 3, dx = tap - dy * 3;
            const int toff = (dy * LW + dx) * CU + (pcb + choff) * 8;
            bf16x8_t bu[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              bu[i] = *reinterpret_cast<const bf16x8_t*>(US + pbase[i] * CU + toff);
              if (!kv) bu[i] = zero_frag();
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < TPP; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2[s][j], bu[i], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < TPP; ++j) a2[s][j] = w2_frag(ks + PF2, j);      // (unconditional, clamped: the compiler's vmcnt count stays exact)
          }
        }
      }
    }
    CARD_STAMP(5);
    __syncthreads();      // every thread is done copying u_raw out of the staging tile
    if (wv < 3) {
      // a path starts at any channel (85, 170, ...): 2-byte LDS stores
#pragma unroll
      for (int j = 0; j < TPP; ++j) {
        float bb[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int cl = 16 * j + 4 * q + e;
          bb[e] = p.b2[pn0 + (cl < CVKK ? cl : 0)];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int pp = i * 16 + r;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int cl = 16 * j + 4 * q + e;
            if (cl < CVKK) SS[pp * S2 + pn0 + cl] = f2bf(acc[i][j][e] + bb[e]);
          }
        }
      }
    } else if (VP > 3 * CVKK) {     // the pad channels of the staged rows
      for (int c = 3 * CVKK; c < VP; ++c) SS[lane * S2 + c] = 0;
    }
  }
  __syncthreads();
  CARD_STAMP(6);

  // ---- E: v_raw -> HBM; per-path LayerNorm + LeakyReLU of the 64 interior pixels in place; y -> HBM; pooled partial row of this tile
  constexpr int NCV = VP / 8;
  if constexpr (STASH) {
    for (int it = tid; it < NPIX * NCV; it += 256) {
      const int pp = it / NCV, c = it - pp * NCV;
      const int gy = ty0 + (pp >> 3), gx = tx0 + (pp & 7);
      if (gy < p.H && gx < p.W)
        *reinterpret_cast<uint4*>(p.v_raw + (img + (int64_t)gy * p.W + gx) * p.ldv + c * 8) = *reinterpret_cast<const uint4*>(SS + pp * S2 + c * 8);
    }
  }
  CARD_STAMP(7);
  tile_layernorm<1, NCV, CVKK, 3>(SS, S2, NPIX, STAT, p.g2, p.be2, p.eps, p.alpha, wv, lane, SS, S2, true);
  __syncthreads();
  CARD_STAMP(8);
  for (int it = tid; it < NPIX * NCV; it += 256) {
    const int pp = it / NCV, c = it - pp * NCV;
    const int gy = ty0 + (pp >> 3), gx = tx0 + (pp & 7);
    if (gy < p.H && gx < p.W)
      *reinterpret_cast<uint4*>(p.y + (img + (int64_t)gy * p.W + gx) * p.ldv + c * 8) = *reinterpret_cast<const uint4*>(SS + pp * S2 + c * 8);
  }
  if (tid < VP) {       // the pool sums the STORED (bf16) values in pixel order, as a pass over y would
    float a = 0.f;
#pragma unroll 8
    for (int pp = 0; pp < NPIX; ++pp) {
      const bool in = ty0 + (pp >> 3) < p.H && tx0 + (pp & 7) < p.W;
      const float t = bf2f(SS[pp * S2 + tid]);
      a += in ? t : 0.f;
    }
    p.gap[((int64_t)b * p.ntiles + tile) * VP + tid] = a;
  }
  CARD_STAMP(9);
#endif
