// Temporal attention of a video latent (tf_sdpa_temporal_16): for every video g, pixel p and head h the F <= 32 frames of that pixel attend to each
// other, o[g, f, p, h, :] = softmax_f'(q' k'^T / sqrt HS) v'.  Tens of thousands of tiny (pixel, head) problems whose rows lie a whole frame apart in
// memory: nothing for the key-tile kernels of sdpa.hip (64-key tiles, a linear batch stride), so this unit stands alone.
//
// Work split: one block per (video, pixel, group of NW <= 4 adjacent heads), one wave per head.
//   stage   all waves together walk (frame, head of the group, 8 channels) once and read q, k and v with 16-byte loads (adjacent heads of a pixel are
//           contiguous, so a frame's row of NW HS channels is one run), widen to fp32, add the positional tables' rows (fp32) and park q', k', v' in
//           LDS, one region per head, rows RS = HS + 4 floats apart (RS / 4 odd: 16 lanes of a ds_read_b128 group on 16 rows hit 64 different banks)
//   scores  lane (i, jg) of the head's wave: query frame i against the keys jg, jg + LJ, ... (LJ = the largest power of two with LJ F <= 64 adjacent
//           lanes per query), four keys per pass so that one read of q serves four of k; fp32 FMAs in channel order, scaled into log2 units
//   softmax inside the LJ lanes of a row: maximum by a butterfly, every lane's own scores -> exp2 in place, the sum by the same butterfly, 1 / sum
//   P V     lane (i, jg): 8 channels at a time, keys in order, fp32; times 1 / sum; the fp32 row replaces q' row i (no longer read)
//   store   all waves together: fp32 -> 16 bits (the ONE rounding of the output), 16-byte stores, the channel run of the group per frame
// No atomics, every sum in a fixed order: the launch is deterministic.  LDS per head: (3 F RS + F (F + 1 | 1)) floats -- 9.6 KB at F = 16, HS = 40,
// 67 KB at F = 32, HS = 160; NW is lowered until the block's share stays inside SDPA_T_LDS_MAX.  The operands sit in LDS as fp32 (the tables make
// them fp32 values) and the products run on the vector ALU, not the MFMA: DESIGN 4.3 has the roofline and what that costs.
#include "common.h"

#include <math.h>

#include "../../include/tinyfusers_hip.h"

#define SDPA_T_LDS_MAX (144 * 1024)

struct SdpaTP {
  const half_t *q, *k, *v;
  half_t* o;
  const float *pe_q, *pe_k, *pe_v;     // (F, NH HS) fp32 or null
  int G, F, P, NH, HS;
  int NW, per, lj_shift;               // heads per block; floats of LDS per head; log2 of the lanes per query frame
  long long q_sf, q_sp, q_sh, k_sf, k_sp, k_sh, v_sf, v_sp, v_sh, o_sf, o_sp, o_sh;     // frame, pixel, head strides in elements
  float scale_log2e;
};

// floats between staged rows and between score rows, and the floats of LDS one head takes (a multiple of 4: every region starts 16-byte aligned)
__host__ __device__ constexpr int sdpa_t_rs(int HS) { return HS + 4; }
__host__ __device__ constexpr int sdpa_t_ss(int F) { return (F + 1) | 1; }
__host__ __device__ constexpr int sdpa_t_per(int F, int HS) { return 3 * F * sdpa_t_rs(HS) + ((F * sdpa_t_ss(F) + 3) & ~3); }

// one operand's 8 channels: 16 bytes from global memory, widened, plus the table's 8 floats (pe: null or the table's address for this frame and channel)
template <bool BF>
__device__ __forceinline__ void sdpa_t_load(const half_t* src, const float* pe, f4& a, f4& b) {
  const h8 x = *reinterpret_cast<const h8*>(src);
  a = f4{e2f<BF>(x[0]), e2f<BF>(x[1]), e2f<BF>(x[2]), e2f<BF>(x[3])};
  b = f4{e2f<BF>(x[4]), e2f<BF>(x[5]), e2f<BF>(x[6]), e2f<BF>(x[7])};
  if (pe) {
    const f4* t = reinterpret_cast<const f4*>(pe);
    a += t[0];
    b += t[1];
  }
}

// The block's work.  HSC / FC: the head size and frame count as compile-time constants (0: read from the launch) -- with them every loop has a fixed
// trip count and every LDS offset is an immediate; the results are the same bits either way (the same operations in the same order).
template <bool BF, int HSC, int FC>
__device__ __forceinline__ void sdpa_t_body(const SdpaTP& p, float* smem) {
  const int F = FC ? FC : p.F, HS = HSC ? HSC : p.HS, RS = sdpa_t_rs(HS), SS = sdpa_t_ss(F), per = sdpa_t_per(F, HS);
  const int lj_shift = FC == 16 ? 2 : p.lj_shift;          // (16 frames: four lanes per query frame)
  const int ngrp = (p.NH + p.NW - 1) / p.NW;
  const unsigned bid = blockIdx.x;
  const int hg = bid % ngrp, gp = bid / ngrp, pix = gp % p.P, g = gp / p.P;
  const int h0 = hg * p.NW, nh = min(p.NW, p.NH - h0);
  const int C8 = HS >> 3, row_items = nh * C8, items = F * row_items;

  // stage: one walk over (frame, head of the group, 8 channels) loads q, k and v together (three 16-byte loads in flight per lane)
  for (int idx = threadIdx.x; idx < items; idx += blockDim.x) {
    const int f = idx / row_items, r = idx - f * row_items, hl = r / C8, c = (r - hl * C8) * 8;
    const long long fr = (long long)g * F + f, hd = h0 + hl;
    const long long pe_off = ((long long)f * p.NH + hd) * HS + c;
    f4 qa, qb, ka, kb, va, vb;
    sdpa_t_load<BF>(p.q + fr * p.q_sf + (long long)pix * p.q_sp + hd * p.q_sh + c, p.pe_q ? p.pe_q + pe_off : nullptr, qa, qb);
    sdpa_t_load<BF>(p.k + fr * p.k_sf + (long long)pix * p.k_sp + hd * p.k_sh + c, p.pe_k ? p.pe_k + pe_off : nullptr, ka, kb);
    sdpa_t_load<BF>(p.v + fr * p.v_sf + (long long)pix * p.v_sp + hd * p.v_sh + c, p.pe_v ? p.pe_v + pe_off : nullptr, va, vb);
    float* dst = smem + hl * per + f * RS + c;
    *reinterpret_cast<f4*>(dst) = qa;
    *reinterpret_cast<f4*>(dst + 4) = qb;
    *reinterpret_cast<f4*>(dst + F * RS) = ka;
    *reinterpret_cast<f4*>(dst + F * RS + 4) = kb;
    *reinterpret_cast<f4*>(dst + 2 * F * RS) = va;
    *reinterpret_cast<f4*>(dst + 2 * F * RS + 4) = vb;
  }
  __syncthreads();

  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* Q = smem + w * per;
  const float* K = Q + F * RS;
  const float* V = K + F * RS;
  float* S = Q + 3 * F * RS;
  const int LJ = 1 << lj_shift, i = lane >> lj_shift, jg = lane & (LJ - 1);      // LJ adjacent lanes share query frame i
  const bool work = w < nh && i < F;          // (w < nh: a ragged last group leaves waves idle; they still meet the barriers)
  float* sr = S + (work ? i : 0) * SS;

  // scores: this lane's keys jg, jg + LJ, ..., four per pass; each lands in the row's score line, the largest stays in mx
  float mx = -INFINITY;
  if (work) {
    const float* qi = Q + i * RS;
    for (int jb = jg; jb < F; jb += 4 * LJ) {
      const int j0 = jb, j1 = jb + LJ, j2 = jb + 2 * LJ, j3 = jb + 3 * LJ;
      const float *k0 = K + j0 * RS, *k1 = K + min(j1, F - 1) * RS, *k2 = K + min(j2, F - 1) * RS, *k3 = K + min(j3, F - 1) * RS;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      for (int c = 0; c < HS; c += 4) {
        const f4 qv = *reinterpret_cast<const f4*>(qi + c);
        const f4 x0 = *reinterpret_cast<const f4*>(k0 + c), x1 = *reinterpret_cast<const f4*>(k1 + c);
        const f4 x2 = *reinterpret_cast<const f4*>(k2 + c), x3 = *reinterpret_cast<const f4*>(k3 + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a0 = fmaf(qv[e], x0[e], a0);
          a1 = fmaf(qv[e], x1[e], a1);
          a2 = fmaf(qv[e], x2[e], a2);
          a3 = fmaf(qv[e], x3[e], a3);
        }
      }
      a0 *= p.scale_log2e; a1 *= p.scale_log2e; a2 *= p.scale_log2e; a3 *= p.scale_log2e;
      sr[j0] = a0;
      mx = fmaxf(mx, a0);
      if (j1 < F) { sr[j1] = a1; mx = fmaxf(mx, a1); }
      if (j2 < F) { sr[j2] = a2; mx = fmaxf(mx, a2); }
      if (j3 < F) { sr[j3] = a3; mx = fmaxf(mx, a3); }
    }
  }
  // softmax inside the LJ lanes of a row (every lane of the wave takes part in the exchanges; idle lanes carry -inf and 0): the row's maximum,
  // each lane's own scores -> exp2 in place, the row's sum in a fixed butterfly order
  for (int o = LJ >> 1; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float sum = 0.f;
  if (work) {
    for (int j = jg; j < F; j += LJ) {
      const float e = __builtin_amdgcn_exp2f(sr[j] - mx);
      sr[j] = e;
      sum += e;
    }
  }
  for (int o = LJ >> 1; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  const float inv = 1.0f / sum;
  __syncthreads();

  if (work) {
    for (int c = jg * 8; c < HS; c += LJ * 8) {
      f4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < F; ++j) {
        const float pj = sr[j];
        const float* vr = V + j * RS + c;
        const f4 va = *reinterpret_cast<const f4*>(vr), vb = *reinterpret_cast<const f4*>(vr + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[e] = fmaf(pj, va[e], a[e]);
          b[e] = fmaf(pj, vb[e], b[e]);
        }
      }
      *reinterpret_cast<f4*>(Q + i * RS + c) = a * inv;
      *reinterpret_cast<f4*>(Q + i * RS + c + 4) = b * inv;
    }
  }
  __syncthreads();

  for (int idx = threadIdx.x; idx < items; idx += blockDim.x) {
    const int f = idx / row_items, r = idx - f * row_items, hl = r / C8, c = (r - hl * C8) * 8;
    const float* s = smem + hl * per + f * RS + c;
    const f4 a = *reinterpret_cast<const f4*>(s), b = *reinterpret_cast<const f4*>(s + 4);
    const h8 y = {f2e<BF>(a[0]), f2e<BF>(a[1]), f2e<BF>(a[2]), f2e<BF>(a[3]), f2e<BF>(b[0]), f2e<BF>(b[1]), f2e<BF>(b[2]), f2e<BF>(b[3])};
    *reinterpret_cast<h8*>(p.o + ((long long)g * F + f) * p.o_sf + (long long)pix * p.o_sp + (long long)(h0 + hl) * p.o_sh + c) = y;
  }
}

// ONE kernel per element type (the library's kernel census stays small); the shapes of the motion modules -- 16 frames, head sizes 40 / 80 / 160 --
// take a body with constant loop bounds behind a branch that is uniform over the launch, every other shape the general body
template <bool BF>
__global__ void __launch_bounds__(256) k_sdpa_temporal(const SdpaTP p) {
  extern __shared__ __attribute__((aligned(16))) float sdpa_t_smem[];
  if (p.F == 16 && p.HS == 40) sdpa_t_body<BF, 40, 16>(p, sdpa_t_smem);
  else if (p.F == 16 && p.HS == 80) sdpa_t_body<BF, 80, 16>(p, sdpa_t_smem);
  else if (p.F == 16 && p.HS == 160) sdpa_t_body<BF, 160, 16>(p, sdpa_t_smem);
  else sdpa_t_body<BF, 0, 0>(p, sdpa_t_smem);
}

int tfk_sdpa_temporal_bf16(const SdpaTP& p, unsigned nblk, hipStream_t st);
int TFK(tfk_sdpa_temporal)(const SdpaTP& p, unsigned nblk, hipStream_t st) {
  static bool attr_set = false;
  if (!attr_set) {
    TF_HIP(hipFuncSetAttribute((const void*)k_sdpa_temporal<kBF>, hipFuncAttributeMaxDynamicSharedMemorySize, SDPA_T_LDS_MAX));
    attr_set = true;
  }
  hipLaunchKernelGGL((k_sdpa_temporal<kBF>), dim3(nblk), dim3(64 * p.NW), (size_t)p.NW * p.per * sizeof(float), st, p);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

#if !TF_TU_BF
extern "C" int tf_sdpa_temporal_16(int dtype, void* o, const void* q, const void* k, const void* v, const float* pe_q, const float* pe_k, const float* pe_v, int G, int F,
                                   int P, int NH, int HS, long long q_sf, long long q_sp, long long q_sh, long long k_sf, long long k_sp, long long k_sh, long long v_sf,
                                   long long v_sp, long long v_sh, long long o_sf, long long o_sp, long long o_sh, tfStream_t s) {
  TF_REQUIRE(dtype == TF_DTYPE_F16 || dtype == TF_DTYPE_BF16, "tf_sdpa_temporal_16: dtype=%d (0 = float16, 1 = bfloat16)", dtype);
  TF_REQUIRE(o && q && k && v, "tf_sdpa_temporal_16: null tensor");
  TF_REQUIRE(G >= 0 && P >= 0 && NH >= 1 && F >= 1, "tf_sdpa_temporal_16: bad sizes G=%d F=%d P=%d NH=%d", G, F, P, NH);
  if (F > 32) {
    tf_set_error("tf_sdpa_temporal_16: %d frames: one launch attends over at most 32 (no sliding window)", F);
    return TF_E_UNSUPPORTED;
  }
  TF_REQUIRE(HS >= 8 && HS % 8 == 0 && HS <= 160, "tf_sdpa_temporal_16: head size %d must be a multiple of 8 in [8, 160]", HS);
  const long long str[] = {q_sf, q_sp, q_sh, k_sf, k_sp, k_sh, v_sf, v_sp, v_sh, o_sf, o_sp, o_sh};
  for (int i = 0; i < 12; ++i) TF_REQUIRE(str[i] % 8 == 0, "tf_sdpa_temporal_16: q / k / v / o strides must be multiples of 8 elements (16-B rows)");
  const void* ptr[] = {o, q, k, v, pe_q, pe_k, pe_v};
  for (int i = 0; i < 7; ++i) TF_REQUIRE(((uintptr_t)ptr[i] & 15) == 0, "tf_sdpa_temporal_16: tensors and tables must be 16-byte aligned");
  SdpaTP p;
  p.NW = NH < 4 ? NH : 4;
  p.per = sdpa_t_per(F, HS);
  p.lj_shift = 0;
  while ((2 << p.lj_shift) * F <= 64) ++p.lj_shift;       // the largest power of two of lanes per query frame that fits a wave
  while ((size_t)p.NW * p.per * sizeof(float) > SDPA_T_LDS_MAX) --p.NW;       // (one head takes 67 KB at most: NW >= 2 always)
  const long long nblk = (long long)G * P * ((NH + p.NW - 1) / p.NW);
  TF_REQUIRE(nblk < (1ll << 31), "tf_sdpa_temporal_16: too many (video, pixel, head group) work items");
  if (G == 0 || P == 0) return TF_OK;
  p.q = (const half_t*)q; p.k = (const half_t*)k; p.v = (const half_t*)v; p.o = (half_t*)o;
  p.pe_q = pe_q; p.pe_k = pe_k; p.pe_v = pe_v;
  p.G = G; p.F = F; p.P = P; p.NH = NH; p.HS = HS;
  p.q_sf = q_sf; p.q_sp = q_sp; p.q_sh = q_sh; p.k_sf = k_sf; p.k_sp = k_sp; p.k_sh = k_sh;
  p.v_sf = v_sf; p.v_sp = v_sp; p.v_sh = v_sh; p.o_sf = o_sf; p.o_sp = o_sp; p.o_sh = o_sh;
  p.scale_log2e = (1.0f / sqrtf((float)HS)) * 1.4426950408889634f;
  hipStream_t st = tf_hs(s);
  TfProfScope prof_(TF_PROF_FAM_SDPA, 4.0 * G * P * NH * (double)F * F * HS, st);
  return dtype == TF_DTYPE_BF16 ? tfk_sdpa_temporal_bf16(p, (unsigned)nblk, st) : tfk_sdpa_temporal(p, (unsigned)nblk, st);
}
#endif
