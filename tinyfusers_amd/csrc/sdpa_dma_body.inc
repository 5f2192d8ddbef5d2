// Body of the LDS-DMA attention kernels, #included into k_sdpa_dma (sdpa_dma.h; KS = 1, SR = 0 as local constants), k_sdpa_split (sdpa_split.hip), k_sdpa_dual
// (sdpa_dual.hip) and k_sdpa_pag (sdpa_pag.hip): one text, four __global__ functions -- a shared __device__ function, even force-inlined, changed the code of the
// shipped k_sdpa_dma instances.  So did, later, a __device__ function for the piece-offset arithmetic alone, which voff[] and the dual form's image tile both spell
// out below (profiles/sdpa_refactor_code_identity.txt): the two copies stay.
// In scope: template parameters HS, QT, DBG, NW, BF; constants KS (key slices), SR (stages per ring when KS > 1); the kernel argument `p`.
//
// TF_SDPA_BODY_DUAL (a compile-time flag, #defined to 1 around the #include in k_sdpa_dual only; KS = 1, DBG = 0, no causal mask; also in scope: `pd`,
// the SdpaDualP that holds `p`): o = softmax(q k^T) v + s softmax(q k2^T) v2 with a second key set of at most 64 keys.  The second set is one more
// tile of the same ring -- local tile `ntiles`, fetched through descriptors of its own -- and one more trip of the same loop (`img`): the text
// row sums l are set aside first, the tile takes its own maximum and its own row sums l2 (fp32, a lane-group sum), its P fragments are scaled per
// query by s l / l2 before the 16-bit rounding, and its P.V MFMAs accumulate onto the text accumulators, so that the plain epilogue's one multiply by
// 1 / l finishes both terms -- and at s = 0 stores what the plain kernel stores, value for value.  Without the flag every line below preprocesses to
// what it was.
#ifndef TF_SDPA_BODY_DUAL
#define TF_SDPA_BODY_DUAL 0
#endif
  static_assert(!(BF && DBG), "the ablation instances are fp16");
  static_assert(NW % KS == 0 && (KS == 1 || (DBG == 0 && SR >= 2)), "key slices: whole query groups, a ring each, no ablation form");
  constexpr int NQ = NW / KS;                                // query groups (waves per slice)
  constexpr int QW = 16 * QT, QB = NQ * QW, NT = NW * 64;   // queries per wave / per block, threads
  using C = SdpaDma<HS>;
  constexpr int NKS = C::NKS, NDT = C::NDT, CK = C::CK, KPC = C::KPC, VPC = C::VPC, KP = C::KP, VP = C::VP, VSK = C::VSK, VGC = C::VGC;
  constexpr int STAGE_B = C::STAGE_B, NI = C::NI, LPW = (C::NI + NQ - 1) / NQ;
  constexpr int S = KS == 1 ? sdpa_ring(STAGE_B, NW, C::S) : SR;   // stages per ring; KS rings back to back
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];

  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qg = KS == 1 ? wid : wid % NQ, sl = KS == 1 ? 0 : wid / NQ;   // query group, key slice (wave-uniform)
  const int lr = lane & 15, lg = lane >> 4;
  const SdpaBlk blk = sdpa_block(p, QB);
  const int b = blk.b, h = blk.h;
  const int qblk = blk.qb * QB + qg * QW;
  const half_t* qb = p.q + b * p.q_sb + h * p.q_sh;
  const half_t* kb = p.k + b * p.k_sb + h * p.k_sh;
  const half_t* vb = p.v + b * p.v_sb + h * p.v_sh;

  typedef unsigned u4 __attribute__((ext_vector_type(4)));
  for (int i = tid; i < KS * S * STAGE_B / 16; i += NT) reinterpret_cast<u4*>(smem_raw)[i] = (u4){0, 0, 0, 0};
  constexpr bool HAS_PAD = C::HAS_PAD;
  if constexpr (HAS_PAD) {
    __syncthreads();                     // ones column of V (column HS of every key row, every ring stage): written once
    for (int i = tid; i < KS * S * 64; i += NT) {
      int st_ = i >> 6, R = i & 63;
      reinterpret_cast<half_t*>(smem_raw + st_ * STAGE_B + C::K_BYTES)[(R >> 3) * VGC * 8 + (R & 7) * VP + HS] = f2e<BF>(1.0f);
    }
  }

  h8 qf[QT][NKS];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    int qi = qblk + qt * 16 + lr;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      int d0 = ks * 32 + lg * 8;
      h8 qv = (qi < p.Tq && d0 < HS) ? *reinterpret_cast<const h8*>(qb + qi * p.q_st + d0) : (h8){0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 8; ++j) qv[j] = f2e<BF>(e2f<BF>(qv[j]) * p.scale_log2e);
      qf[qt][ks] = qv;
    }
  }

  int ntiles = (p.Tk + 63) / 64;
  if (p.causal) {
    int last_q = min(p.Tq, blk.qb * QB + QB) - 1;
    ntiles = min(ntiles, last_q / 64 + 1);
  }
  // this slice's tiles: global tiles t0 .. t0 + n_my - 1, walked as local tiles 0 .. n_my - 1 of its ring; `trip` iterations for every wave of the block
#if TF_SDPA_BODY_DUAL
  static_assert(KS == 1 && DBG == 0, "the dual form has no key slices and no ablation build");
  const int trip = ntiles + 1, t0 = 0, n_my = ntiles + 1;      // the image tile is local tile `ntiles`
  const float scale2 = *pd.scale2;
  float l_txt[QT] = {};                                           // the text row sums, set when the image tile begins
#else
  const int trip = KS == 1 ? ntiles : (ntiles + KS - 1) / KS;
  const int t0 = KS == 1 ? 0 : sl * trip;
  const int n_my = KS == 1 ? ntiles : max(0, min(trip, ntiles - t0));
#endif

  // this wave's 1-KiB pieces of a tile: piece j = qg + NQ i (clamped: the spare slots of the last round repeat piece
  // NI-1, same bytes to the same place); j < KPC -> K image, else V image
  const i4v rs_k = sdpa_rsrc(kb, (unsigned)(((long long)(p.Tk - 1) * p.k_st + HS) * 2));
  const i4v rs_v = sdpa_rsrc(vb, (unsigned)(((long long)(p.Tk - 1) * p.v_st + HS) * 2));
  unsigned voff[LPW];
  const unsigned k_adv = 64u * (unsigned)p.k_st * 2u, v_adv = 64u * (unsigned)p.v_st * 2u;
#pragma unroll
  for (int i = 0; i < LPW; ++i) {
    int j = min(qg + NQ * i, NI - 1);
    if (j < KPC) {
      int x = 64 * j + lane, r = x / KPC, cc = x - r * KPC;
      int kt = r >> 4, rr = r & 15;
      int key = 32 * (kt >> 1) + 8 * (rr >> 2) + 4 * (kt & 1) + (rr & 3);
      voff[i] = cc < CK ? (unsigned)(key * (int)p.k_st + cc * 8) * 2u : 0x80000000u;
    } else {
      // V image: groups of 8 rows (VPC chunks each) followed by VSC skew chunks; pad / skew / tail chunks are fetched out of range
      int x = 64 * (j - KPC) + lane, grp = x / VGC, rem = x - grp * VGC;
      int rr = rem / VPC, cc = rem - rr * VPC, r = 8 * grp + rr;
      voff[i] = (rr < 8 && grp < 8 && cc < CK) ? (unsigned)(r * (int)p.v_st + cc * 8) * 2u : 0x80000000u;
      if (HAS_PAD && rr < 8 && grp < 8 && cc == CK) voff[i] = 0xFFFFFFFFu;     // the preset ones column: this lane stays out of the DMA
    }
  }
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem_raw + (unsigned)(sl * S) * STAGE_B;
  auto issue = [&](int lt_) {             // local tile lt_ of this slice -> stage lt_ % S of its ring
    const unsigned base = lds0 + (unsigned)(lt_ % S) * STAGE_B;
    const int tt = t0 + lt_;
#if TF_SDPA_BODY_DUAL
    if (lt_ == ntiles) {
      // the image tile: the same pieces to the same places through descriptors of its own (rows >= Tk2 lie beyond num_records and come back as zeros,
      // as a ragged text tile's do); voff's arithmetic with the image strides, done here, once per kernel
      const i4v rs_k2 = sdpa_rsrc(pd.k2 + b * pd.k2_sb + h * pd.k2_sh, (unsigned)(((long long)(pd.Tk2 - 1) * pd.k2_st + HS) * 2));
      const i4v rs_v2 = sdpa_rsrc(pd.v2 + b * pd.v2_sb + h * pd.v2_sh, (unsigned)(((long long)(pd.Tk2 - 1) * pd.v2_st + HS) * 2));
#pragma unroll
      for (int i = 0; i < LPW; ++i) {
        const int j = min(qg + NQ * i, NI - 1);
        if (j < KPC) {
          int x = 64 * j + lane, r = x / KPC, cc = x - r * KPC;
          int kt = r >> 4, rr = r & 15;
          int key = 32 * (kt >> 1) + 8 * (rr >> 2) + 4 * (kt & 1) + (rr & 3);
          sdpa_dma16(rs_k2, cc < CK ? (unsigned)(key * (int)pd.k2_st + cc * 8) * 2u : 0x80000000u, base + j * 1024);
        } else {
          int x = 64 * (j - KPC) + lane, grp = x / VGC, rem = x - grp * VGC;
          int rr = rem / VPC, cc = rem - rr * VPC, r = 8 * grp + rr;
          const unsigned off = (rr < 8 && grp < 8 && cc < CK) ? (unsigned)(r * (int)pd.v2_st + cc * 8) * 2u : 0x80000000u;
          if (!(HAS_PAD && rr < 8 && grp < 8 && cc == CK)) sdpa_dma16(rs_v2, off, base + j * 1024);     // (the preset ones column stays out of the DMA)
        }
      }
      return;
    }
#endif
#pragma unroll
    for (int i = 0; i < LPW; ++i) {
      int j = min(qg + NQ * i, NI - 1);
      if (j < KPC) sdpa_dma16(rs_k, voff[i] + (unsigned)tt * k_adv, base + j * 1024);
      else if (!HAS_PAD) sdpa_dma16(rs_v, voff[i] + (unsigned)tt * v_adv, base + j * 1024);
      else if (voff[i] != 0xFFFFFFFFu) sdpa_dma16(rs_v, voff[i] + (unsigned)tt * v_adv, base + j * 1024);   // (EXEC-masked: the skipped lanes write nothing)
    }
  };

  f4 ot[NDT][QT], lt[QT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) { for (int q_ = 0; q_ < QT; ++q_) ot[dt][q_] = (f4){0, 0, 0, 0}; }
  for (int q_ = 0; q_ < QT; ++q_) lt[q_] = (f4){0, 0, 0, 0};
  float m_run[QT];
  for (int q_ = 0; q_ < QT; ++q_) m_run[q_] = 0.f;
  const half_t one1 = f2e<BF>(1.f);
  const h8 ones = {one1, one1, one1, one1, one1, one1, one1, one1};

  __syncthreads();                       // zero fill done (and drained) before the first DMA lands
#pragma unroll
  for (int tt = 0; tt < S - 1; ++tt)
    if (tt < n_my) issue(tt);

  for (int i = 0; i < trip; ++i) {
    const int t = t0 + i;
    // tile t landed (this wave's pieces), leaving the younger tiles in flight; the barrier extends that to every wave
    // and tells that all of them are done reading tile t-1, whose slot the next issue refills
    {
      int younger = min(S - 2, n_my - 1 - i);
      if (younger >= 4 && S >= 6 && 4 * LPW <= 63) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * LPW > 63 ? 63 : 4 * LPW) : "memory");
      else if (younger >= 3 && S >= 5 && 3 * LPW <= 63) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * LPW > 63 ? 63 : 3 * LPW) : "memory");
      else if (younger >= 2 && S >= 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPW > 63 ? 63 : 2 * LPW) : "memory");
      else if (younger >= 1 && S >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPW > 63 ? 63 : LPW) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (!(DBG & 8)) __builtin_amdgcn_s_barrier();
    if (i + S - 1 < n_my && !(DBG & 16)) issue(i + S - 1);
    if constexpr (KS > 1) { if (i >= n_my) continue; }     // out of tiles: the barrier above was this iteration's only duty

    const half_t* ks_ = reinterpret_cast<const half_t*>(smem_raw + (sl * S + i % S) * STAGE_B);
    const half_t* vs_ = ks_ + C::K_BYTES / 2;

#if TF_SDPA_BODY_DUAL
    const bool img = i == ntiles;                          // (wave-uniform)
    const int key0 = img ? 0 : t * 64, nkeys = img ? pd.Tk2 : p.Tk;
    if (img) {
      // the text softmax is complete.  Its row sum l is taken out of the accumulators' reach (at d = 40 the image tile's P.V adds to the row that
      // holds it) and both are scaled by the power of two that brings l into [1, 2): exact, so the epilogue's o * (1 / l) -- the plain kernel's own
      // expression -- rounds to what the plain kernel stores, and the image tile's P, scaled by s l / l2 below, stays <= 2 |s|.  The image tile's own
      // softmax starts from nothing.
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        float l = lt[qt][0];
        if constexpr (HAS_PAD) l = __shfl(ot[(HS / 16) % NDT][qt][0], lr + 16 * ((HS % 16) / 4), 64);
        const float e2 = __uint_as_float(0x7f000000u - (__float_as_uint(l) & 0x7f800000u));      // 2^-floor(log2 l)
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) ot[dt][qt] *= e2;
        l_txt[qt] = l * e2;
        m_run[qt] = 0.f;
      }
    }
#else
    constexpr bool img = false;
    const int key0 = t * 64, nkeys = p.Tk;
#endif
    f4 st[4][QT];
    f4 init4[QT];
#pragma unroll
    for (int q_ = 0; q_ < QT; ++q_) init4[q_] = (f4){-m_run[q_], -m_run[q_], -m_run[q_], -m_run[q_]};
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        h8 kf = *reinterpret_cast<const h8*>(ks_ + (16 * kt + lr) * KP + ks * 32 + lg * 8);
#pragma unroll
        for (int q_ = 0; q_ < QT; ++q_) {
          if (DBG & 4) { if (ks == 0) st[kt][q_] = init4[q_] + (f4){(float)kf[0], (float)kf[1], (float)kf[2], (float)kf[3]}; }
          else st[kt][q_] = mfma16<BF>(kf, qf[q_][ks], ks == 0 ? init4[q_] : st[kt][q_]);
        }
      }
    }
    const int kbase = key0 + 8 * lg;
    if (key0 + 64 > nkeys || p.causal) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          int key = kbase + 32 * (kt >> 1) + 4 * (kt & 1) + e;
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) {
            int qi = qblk + qt * 16 + lr;
            if (key >= nkeys || (p.causal && key > qi)) st[kt][qt][e] = -INFINITY;
          }
        }
    }
    constexpr float RESCALE_THR = 6.0f;
    float mx[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      if (DBG & 64) { mx[qt] = st[0][qt][0]; continue; }
      float m0_ = fmaxf(fmaxf(st[0][qt][0], st[0][qt][1]), fmaxf(st[0][qt][2], st[0][qt][3]));
#pragma unroll
      for (int kt = 1; kt < 4; ++kt) {
        m0_ = fmaxf(fmaxf(m0_, st[kt][qt][0]), st[kt][qt][1]);
        m0_ = fmaxf(fmaxf(m0_, st[kt][qt][2]), st[kt][qt][3]);
      }
      m0_ = max_over_lane_groups(m0_);
      mx[qt] = m0_;
    }
    bool over = false;
#pragma unroll
    for (int q_ = 0; q_ < QT; ++q_) over = over || (mx[q_] > RESCALE_THR);
    if (i == 0 || img || __any(over)) {
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        float delta = mx[qt] == -INFINITY ? 0.f : (i == 0 || img ? mx[qt] : fmaxf(mx[qt], 0.f));
        m_run[qt] += delta;
        if (i != 0 && !img) {
          float alpha = __builtin_amdgcn_exp2f(-delta);
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) ot[dt][qt] *= alpha;
          lt[qt] *= alpha;
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int e = 0; e < 4; ++e) st[kt][qt][e] -= delta;
      }
    }
    h8 pf[2][QT];
#if TF_SDPA_BODY_DUAL
    if (img) {
      // own row sums in fp32 (this lane's 16 keys, then the four lane groups); P is scaled by s l / l2 per query -- the query is the lane's own
      // column; l: the text row sum the epilogue divides by -- and rounded to 16 bits once
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        float l2 = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int e = 0; e < 4; ++e) { st[kt][qt][e] = __builtin_amdgcn_exp2f(st[kt][qt][e]); l2 += st[kt][qt][e]; }
        const float c2 = scale2 * l_txt[qt] / sum_over_lane_groups(l2);      // l2 >= 1: Tk2 >= 1 and the maximum's own term is 2^0
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int e = 0; e < 4; ++e) pf[kt >> 1][qt][(kt & 1) * 4 + e] = f2e<BF>(st[kt][qt][e] * c2);
      }
    } else
#endif
    {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int e = 0; e < 4; ++e) pf[kt >> 1][qt][(kt & 1) * 4 + e] = (DBG & 1) ? (half_t)st[kt][qt][e] : f2e<BF>(__builtin_amdgcn_exp2f(st[kt][qt][e]));
    }
    if constexpr (!HAS_PAD) {
      if (!img) {
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
#pragma unroll
        for (int q_ = 0; q_ < QT; ++q_) lt[q_] = mfma16<BF>(ones, pf[kc][q_], lt[q_]);
      }
      }
    }
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        const half_t* va = vs_ + (32 * kc + 8 * lg + (lr >> 2)) * VP + (4 * kc + lg) * VSK + dt * 16 + 4 * (lr & 3);
        union { struct { s4v a, b; } s; h8 h; } u;
        if (DBG & 32) u.h = pf[kc][0];
        else { u.s.a = lds_tr16(va); u.s.b = lds_tr16(va + 4 * VP); }
#pragma unroll
        for (int q_ = 0; q_ < QT; ++q_) {
          if (DBG & 2) ot[dt][q_] += (f4){(float)u.h[0] * (float)pf[kc][q_][0], (float)u.h[1], (float)u.h[2], (float)pf[kc][q_][7]};
          else ot[dt][q_] = mfma16<BF>(u.h, pf[kc][q_], ot[dt][q_]);
        }
      }
    }
  }

  if constexpr (KS > 1) {
    // merge the slices through the (dead) rings, lane to lane: the waves of one query group hold the same queries in the same lanes
    constexpr int NF = (NDT + (HAS_PAD ? 0 : 1)) * QT;      // f4 per lane: O^T (row HS of it is the row sum at d = 40), else + the ones-MFMA's row sums
    constexpr int MO_B = (KS - 1) * NQ * NF * 64 * 16, MM_B = (KS - 1) * NQ * QT * 64 * 4;
    static_assert(MO_B + MM_B <= KS * S * STAGE_B, "merge scratch must fit the rings (else merge in rounds)");
    f4* mo = reinterpret_cast<f4*>(smem_raw);
    float* mm = reinterpret_cast<float*>(smem_raw + MO_B);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                     // every wave is done with its ring: nothing in flight, nothing left to read
    if (sl > 0) {
      const int w = (sl - 1) * NQ + qg;
#pragma unroll
      for (int q_ = 0; q_ < QT; ++q_) {
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) mo[(w * NF + dt * QT + q_) * 64 + lane] = ot[dt][q_];
        if constexpr (!HAS_PAD) mo[(w * NF + NDT * QT + q_) * 64 + lane] = lt[q_];
        mm[(w * QT + q_) * 64 + lane] = m_run[q_];
      }
    }
    __syncthreads();
    if (sl > 0) return;
#pragma unroll
    for (int s_ = 1; s_ < KS; ++s_) {
      if (ntiles - s_ * trip <= 0) break;                  // an empty slice (and every one after it) contributes nothing
      const int w = (s_ - 1) * NQ + qg;
#pragma unroll
      for (int q_ = 0; q_ < QT; ++q_) {
        const float ms = mm[(w * QT + q_) * 64 + lane], M = fmaxf(m_run[q_], ms);
        const float a0 = __builtin_amdgcn_exp2f(m_run[q_] - M), as = __builtin_amdgcn_exp2f(ms - M);   // scores are in log2 units
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) ot[dt][q_] = ot[dt][q_] * a0 + mo[(w * NF + dt * QT + q_) * 64 + lane] * as;
        if constexpr (!HAS_PAD) lt[q_] = lt[q_] * a0 + mo[(w * NF + NDT * QT + q_) * 64 + lane] * as;
        m_run[q_] = M;
      }
    }
  }

  half_t* ob = p.o + b * p.o_sb + h * p.o_sh;
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    // row sum: the ones-MFMA's accumulator, or row HS of O^T (the preset ones column of V): accumulator tile HS / 16, lane group (HS % 16) / 4
#if TF_SDPA_BODY_DUAL
    float l = l_txt[qt];                 // the text row sum, saved (and scaled into [1, 2) with the accumulators) in front of the image tile
#else
    float l = lt[qt][0];
    if constexpr (HAS_PAD) l = __shfl(ot[(HS / 16) % NDT][qt][0], lr + 16 * ((HS % 16) / 4), 64);
#endif
    float inv = l > 0.f ? 1.0f / l : 0.f;
    int qi = qblk + qt * 16 + lr;
    if (qi < p.Tq) {
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        int d = dt * 16 + lg * 4;
        if (d < HS) {
          h4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = f2e<BF>(ot[dt][qt][e] * inv);
          *reinterpret_cast<h4*>(ob + qi * p.o_st + d) = o;
        }
      }
    }
  }
