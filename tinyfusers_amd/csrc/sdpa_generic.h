// Fused flash-style scaled-dot-product attention for gfx950 (wave64, MFMA 16x16x32 f16, online softmax): k_sdpa, the register-staged kernel for any
// head size up to 160 -- what runs where the LDS-DMA family (sdpa_dma.h) has no instance, or under TF_SDPA_GENERIC.
// Replaces attention/sdpa.py:53-77 (cp.matmul -> softmax_kernel -> cp.matmul with the (B,NH,Tq,Tk) fp32
// score matrix materialised twice in HBM): scores never leave registers.
//
// Block = 4 waves, 128 query rows (32 per wave); K/V tiles of 64 keys staged through LDS (register-staged
// prefetch, two LDS stages).  Per wave and tile:
//   S^T (64 keys x 32 queries) = K_tile . Q^T      -- K rows are the MFMA A operand (ds_read_b128),
//                                                     Q fragments stay in registers for the whole kernel;
//   softmax along keys is lane-local (query = lane & 15) plus two xor-shuffles across the 4 lane groups.  The loop is
//   VALU-issue bound at d = 40 (v_exp 8 cycles, everything else 4), so the softmax is cut to max3 + exp2 + cvt per
//   score: Q is pre-scaled by log2(e)/sqrt(d), the running reference maximum enters as the INITIAL ACCUMULATOR of
//   the QK^T chain (S' = K Q^T - m needs no subtract), and the row sums come out of the PV product itself through
//   a column of ones in the padding of the V tile (column DV-1 >= HS), rescaled together with O for free;
//   O^T (d x 32 queries) += V^T . P^T              -- P^T is already in B-operand layout (accumulator ->
//                                                     operand, keys permuted so each lane group owns 8
//                                                     consecutive keys), V^T comes from the row-major V
//                                                     tile with ds_read_b64_tr_b16.
#pragma once
#include "sdpa_common.h"

template <int DQK, int DV, bool BF = false>   // BF: bfloat16 q / k / v / o (sdpa_bf16.hip)
__global__ void __launch_bounds__(256) k_sdpa(const SdpaP p) {
  constexpr int KS = DQK + 8;                 // K row stride (halves); 16-B multiple
  constexpr int VS = DV + 8;                  // V row stride (halves); 16-B multiple
  constexpr int NKS = DQK / 32;               // k-steps of QK^T
  constexpr int NDT = DV / 16;                // d tiles of PV (the last one holds the ones column: DV > HS)
  constexpr int CPR = DV / 8;                 // 16-B chunks per staged row (covers HS <= DV)
  constexpr int NCH = (64 * CPR + 255) / 256; // staging rounds per tensor
  constexpr int STAGE_H = 64 * KS + 64 * VS;  // halves per stage
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  half_t* smem = reinterpret_cast<half_t*>(smem_raw);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const SdpaBlk blk = sdpa_block(p);
  const int b = blk.b, h = blk.h;
  const int qblk = blk.qb * 128 + wid * 32;
  const half_t* qb = p.q + b * p.q_sb + h * p.q_sh;
  const half_t* kb = p.k + b * p.k_sb + h * p.k_sh;
  const half_t* vb = p.v + b * p.v_sb + h * p.v_sh;

  // zero both stages once: padding columns [HS, DQK) of K and [HS, DV) of V are never written afterwards
  for (int i = tid; i < 2 * STAGE_H / 8; i += 256) reinterpret_cast<h8*>(smem)[i] = (h8){0, 0, 0, 0, 0, 0, 0, 0};

  // Q fragments (B operand of S^T = K Q^T): lane holds Q[query lr][d = 32 ks + 8 lg + j]
  h8 qf[2][NKS];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    int qi = qblk + qt * 16 + lr;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      int d0 = ks * 32 + lg * 8;
      h8 qv = (qi < p.Tq && d0 < p.HS) ? *reinterpret_cast<const h8*>(qb + qi * p.q_st + d0) : (h8){0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 8; ++j) qv[j] = f2e<BF>(e2f<BF>(qv[j]) * p.scale_log2e);
      qf[qt][ks] = qv;
    }
  }

  f4 ot[NDT][2];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) { ot[dt][0] = (f4){0, 0, 0, 0}; ot[dt][1] = (f4){0, 0, 0, 0}; }
  float m_run[2] = {0.f, 0.f};    // reference maximum (log2 units); set from the first tile, then only raised

  int ntiles = (p.Tk + 63) / 64;
  if (p.causal) {   // keys beyond the block's last query are never needed
    int last_q = min(p.Tq, blk.qb * 128 + 128) - 1;
    ntiles = min(ntiles, last_q / 64 + 1);
  }

  // K/V tiles: raw buffer loads with 32-bit offsets; rows >= Tk and padding columns fall outside the range check
  // and come back as zeros (no branches, no 64-bit address math)
  const __amdgpu_buffer_rsrc_t rs_k = __builtin_amdgcn_make_buffer_rsrc((void*)kb, 0, (unsigned)(((long long)(p.Tk - 1) * p.k_st + p.HS) * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc((void*)vb, 0, (unsigned)(((long long)(p.Tk - 1) * p.v_st + p.HS) * 2), 0x00020000);
  typedef unsigned u4 __attribute__((ext_vector_type(4)));
  union U4H8 { u4 u; h8 h; };
  h8 kreg[NCH], vreg[NCH];
  int st_row[NCH], st_col[NCH];
#pragma unroll
  for (int r = 0; r < NCH; ++r) {
    int idx = tid + 256 * r;
    st_row[r] = idx / CPR;
    st_col[r] = (idx - st_row[r] * CPR) * 8;
  }
  auto load_tile = [&](int t) {
#pragma unroll
    for (int r = 0; r < NCH; ++r) {
      int key = t * 64 + st_row[r];
      bool ok = st_row[r] < 64 && key < p.Tk && st_col[r] < p.HS;
      unsigned ko = ok ? (unsigned)(key * (int)p.k_st + st_col[r]) * 2u : 0x80000000u;
      unsigned vo = ok ? (unsigned)(key * (int)p.v_st + st_col[r]) * 2u : 0x80000000u;
      U4H8 a, b2;
      a.u = __builtin_amdgcn_raw_buffer_load_b128(rs_k, ko, 0, 0);
      b2.u = __builtin_amdgcn_raw_buffer_load_b128(rs_v, vo, 0, 0);
      kreg[r] = a.h; vreg[r] = b2.h;
    }
  };
  auto store_tile = [&](int buf) {
    half_t* ks_ = smem + buf * STAGE_H;
    half_t* vs_ = ks_ + 64 * KS;
#pragma unroll
    for (int r = 0; r < NCH; ++r) {
      if (st_row[r] < 64 && st_col[r] < p.HS) {
        *reinterpret_cast<h8*>(ks_ + st_row[r] * KS + st_col[r]) = kreg[r];
        *reinterpret_cast<h8*>(vs_ + st_row[r] * VS + st_col[r]) = vreg[r];
      }
    }
  };

  load_tile(0);
  __syncthreads();           // zero-fill complete before the first tile lands on top of it
  store_tile(0);
  if (tid < 128) smem[(tid >> 6) * STAGE_H + 64 * KS + (tid & 63) * VS + DV - 1] = f2e<BF>(1.0f);   // ones column -> row sums
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1;
    if (t + 1 < ntiles) load_tile(t + 1);
    const half_t* ks_ = smem + buf * STAGE_H;
    const half_t* vs_ = ks_ + 64 * KS;

    // ---- S^T = K Q^T : st[kt][qt], key(kt, row) = 32 (kt>>1) + 8 (row>>2) + 4 (kt&1) + (row&3)
    f4 st[4][2];
    const f4 init4[2] = {{-m_run[0], -m_run[0], -m_run[0], -m_run[0]}, {-m_run[1], -m_run[1], -m_run[1], -m_run[1]}};
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      int krow = 32 * (kt >> 1) + 8 * (lr >> 2) + 4 * (kt & 1) + (lr & 3);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        h8 kf = *reinterpret_cast<const h8*>(ks_ + krow * KS + ks * 32 + lg * 8);
        st[kt][0] = mfma16<BF>(kf, qf[0][ks], ks == 0 ? init4[0] : st[kt][0]);
        st[kt][1] = mfma16<BF>(kf, qf[1][ks], ks == 0 ? init4[1] : st[kt][1]);
      }
    }
    // ---- masks: this lane's keys are t*64 + 32 (kt>>1) + 8 lg + 4 (kt&1) + reg
    const int kbase = t * 64 + 8 * lg;
    if (t * 64 + 64 > p.Tk || p.causal) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          int key = kbase + 32 * (kt >> 1) + 4 * (kt & 1) + e;
#pragma unroll
          for (int qt = 0; qt < 2; ++qt) {
            int qi = qblk + qt * 16 + lr;
            if (key >= p.Tk || (p.causal && key > qi)) st[kt][qt][e] = -INFINITY;
          }
        }
    }
    // ---- online softmax (per query column) in log2 units, P^T fragments.  st already holds s - m_run.  The reference
    // max is set by the first tile and afterwards only moves when some query's tile max exceeds it by more than
    // RESCALE_THR (then every accumulator of the wave is rescaled once), so P <= 2^RESCALE_THR: harmless in fp16 (fp32
    // accumulation), and the O-wide multiply leaves the steady state.
    constexpr float RESCALE_THR = 6.0f;
    float mx[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      float m0_ = fmaxf(fmaxf(st[0][qt][0], st[0][qt][1]), fmaxf(st[0][qt][2], st[0][qt][3]));
#pragma unroll
      for (int kt = 1; kt < 4; ++kt) {
        m0_ = fmaxf(fmaxf(m0_, st[kt][qt][0]), st[kt][qt][1]);
        m0_ = fmaxf(fmaxf(m0_, st[kt][qt][2]), st[kt][qt][3]);
      }
      m0_ = max_over_lane_groups(m0_);
      mx[qt] = m0_;
    }
    if (t == 0 || __any((mx[0] > RESCALE_THR) || (mx[1] > RESCALE_THR))) {
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        // first tile: adopt its max whatever the sign (O is still zero, nothing to rescale); later: raise only
        float delta = mx[qt] == -INFINITY ? 0.f : (t == 0 ? mx[qt] : fmaxf(mx[qt], 0.f));
        m_run[qt] += delta;
        if (t != 0) {
          float alpha = __builtin_amdgcn_exp2f(-delta);
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) ot[dt][qt] *= alpha;
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int e = 0; e < 4; ++e) st[kt][qt][e] -= delta;
      }
    }
    h8 pf[2][2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int e = 0; e < 4; ++e) pf[kt >> 1][qt][(kt & 1) * 4 + e] = f2e<BF>(__builtin_amdgcn_exp2f(st[kt][qt][e]));
    // ---- O^T += V^T P^T
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        const half_t* va = vs_ + (32 * kc + 8 * lg + (lr >> 2)) * VS + dt * 16 + 4 * (lr & 3);
        s4v v0 = lds_tr16(va), v1 = lds_tr16(va + 4 * VS);
        union { struct { s4v a, b; } s; h8 h; } u;
        u.s.a = v0; u.s.b = v1;
        ot[dt][0] = mfma16<BF>(u.h, pf[kc][0], ot[dt][0]);
        ot[dt][1] = mfma16<BF>(u.h, pf[kc][1], ot[dt][1]);
      }
    }
    if (t + 1 < ntiles) store_tile(buf ^ 1);
    __syncthreads();
  }

  // ---- normalise and store: lane holds O[query lr][d = 16 dt + 4 lg + {0..3}]
  half_t* ob = p.o + b * p.o_sb + h * p.o_sh;
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    // row sum = O^T row DV-1 (the ones column of V): last accumulator tile, lane group 3, register 3
    float l = __shfl(ot[NDT - 1][qt][3], lr + 48, 64);
    float inv = l > 0.f ? 1.0f / l : 0.f;
    int qi = qblk + qt * 16 + lr;
    if (qi < p.Tq) {
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        int d = dt * 16 + lg * 4;
        if (d < p.HS) {
          h4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = f2e<BF>(ot[dt][qt][e] * inv);
          *reinterpret_cast<h4*>(ob + qi * p.o_st + d) = o;
        }
      }
    }
  }
}

// BF as a template argument, not the unit's kBF: a template is instantiated where sdpa.hip's launch calls it, which keeps this family's kernels behind the
// LDS-DMA family's in the code object, where they always were
template <int DQK, int DV, bool BF>
static int launch_sdpa_dv(const SdpaP& p, hipStream_t st) {
  constexpr int smem = 2 * (64 * (DQK + 8) + 64 * (DV + 8)) * 2;      // two stages of a K and a V tile
  return launch_sdpa_kernel<k_sdpa<DQK, DV, BF>>(p, p, smem, 128, 4, st);
}
// (DQK, DV) = (HS rounded up to 32, HS + 1 rounded up to 16): the V tile always has room for the ones column
template <bool BF>
static int launch_sdpa(const SdpaP& p, hipStream_t st) {
  const int HS = p.HS;
  if (HS <= 32) return launch_sdpa_dv<32, 48, BF>(p, st);
  if (HS <= 40) return launch_sdpa_dv<64, 48, BF>(p, st);
  if (HS <= 56) return launch_sdpa_dv<64, 64, BF>(p, st);
  if (HS <= 64) return launch_sdpa_dv<64, 80, BF>(p, st);
  if (HS <= 88) return launch_sdpa_dv<96, 96, BF>(p, st);
  if (HS <= 96) return launch_sdpa_dv<96, 112, BF>(p, st);
  if (HS <= 120) return launch_sdpa_dv<128, 128, BF>(p, st);
  if (HS <= 128) return launch_sdpa_dv<128, 144, BF>(p, st);
  return launch_sdpa_dv<160, 176, BF>(p, st);
}
