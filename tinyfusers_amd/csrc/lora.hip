// LoRA adapters (storage/lora.py; variants/sd.py::set_adapters): the device-side merge of up to 8 low-rank pairs into a fresh copy of one
// weight matrix.  Own translation unit: no existing kernel's code changes.
#include "common.h"
#include "../../include/tinyfusers_hip.h"

#define LM_MAX 8                         // adapters of one launch
#define LM_BLOCK 256                     // 4 waves
#define LM_TN 16                         // rows of dst (N) per wave: the MFMA's column index
#define LM_SUB 4                         // 16-wide MFMA tiles along Kd per wave
#define LM_TK (16 * LM_SUB)              // columns of dst (Kd) per wave
#define LM_BK (LM_TK * (LM_BLOCK / 64))  // columns of dst per block

// The whole table travels by value in the kernel arguments (as k_control_add's does): nothing is uploaded.
struct LoraTable {
  const void* up[LM_MAX];                // (N, Rp_i), contiguous along the rank
  const void* down_t[LM_MAX];            // (Kd, Rp_i), contiguous along the rank
  int rp[LM_MAX];                        // padded rank, a multiple of 32
  float s[LM_MAX];
  int n;
};

// dst[n, k] = round16(base[n, k] + sum_i s_i * sum_j up_i[n, j] * down_i[j, k]).
// One wave owns a 16 (N) x 64 (Kd) tile of dst and computes it TRANSPOSED: D (Kd x N) = down_t (Kd x Rp) . up^T (Rp x N) on
// mfma_f32_16x16x32, so that the A fragment of lane l is 8 consecutive rank elements of down_t's row k0 + (l & 15), the B fragment 8 consecutive
// rank elements of up's row n0 + (l & 15) -- one 16-byte global load each, no LDS -- and the four accumulator values of a lane are
// dst[n0 + (l & 15)][k0 + 4 (l >> 4) + 0..3]: consecutive along Kd, one 8-byte store.  Products of two 16-bit values are exact in fp32; every
// adapter has an accumulator of its own, s_i is applied to it with one fma into the running fp32 sum that starts at the base value, and the sum
// is rounded to 16 bits once.  s_i == 0 skips the adapter (a uniform branch: 0 * inf would be NaN), so with every scale 0 dst gets base's bits.
// Rows past N / Kd read a clamped (valid) row and are never stored.  No atomics: the same bits on every run.
template <bool BF>
__global__ void __launch_bounds__(LM_BLOCK) k_lora_merge(half_t* __restrict__ dst, const half_t* __restrict__ base, const LoraTable t, int N, int Kd, int vec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.y * LM_TN;
  const int k0 = blockIdx.x * LM_BK + wave * LM_TK;
  if (k0 >= Kd) return;                  // (wave-uniform)
  const int r = lane & 15, q = lane >> 4;
  const int n = n0 + r;                  // this lane's dst row, and the row of `up` it loads
  const size_t nrow = (size_t)(n < N ? n : N - 1);
  size_t krow[LM_SUB];                   // the rows of `down_t` it loads
#pragma unroll
  for (int u = 0; u < LM_SUB; ++u) {
    const int k = k0 + 16 * u + r;
    krow[u] = (size_t)(k < Kd ? k : Kd - 1);
  }
  const size_t row = (size_t)nrow * (size_t)Kd;
  f4 sum[LM_SUB];
#pragma unroll
  for (int u = 0; u < LM_SUB; ++u) {
    const int k = k0 + 16 * u + 4 * q;   // this lane's four dst columns k .. k + 3
    if (vec) {                           // Kd % 4 == 0, 8-byte aligned: the four are in range together or not at all
      const size_t kk = (size_t)(k < Kd ? k : 0);
      const h4 b = *reinterpret_cast<const h4*>(base + row + kk);
#pragma unroll
      for (int e = 0; e < 4; ++e) sum[u][e] = e2f<BF>(b[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) sum[u][e] = e2f<BF>(base[row + (size_t)(k + e < Kd ? k + e : 0)]);
    }
  }
#pragma unroll
  for (int i = 0; i < LM_MAX; ++i) {     // (every index into the table is a compile-time constant: it stays in scalar registers)
    if (i < t.n && t.s[i] != 0.0f) {
      const int rp = t.rp[i];
      const half_t* up = reinterpret_cast<const half_t*>(t.up[i]) + nrow * (size_t)rp + 8 * q;
      const half_t* dn = reinterpret_cast<const half_t*>(t.down_t[i]) + 8 * q;
      f4 acc[LM_SUB];
#pragma unroll
      for (int u = 0; u < LM_SUB; ++u) acc[u] = f4{0.0f, 0.0f, 0.0f, 0.0f};
      for (int j = 0; j < rp; j += 32) {
        const h8 b = *reinterpret_cast<const h8*>(up + j);
        h8 a[LM_SUB];
#pragma unroll
        for (int u = 0; u < LM_SUB; ++u) a[u] = *reinterpret_cast<const h8*>(dn + krow[u] * (size_t)rp + j);
#pragma unroll
        for (int u = 0; u < LM_SUB; ++u) acc[u] = mfma16<BF>(a[u], b, acc[u]);
      }
      const float s = t.s[i];
#pragma unroll
      for (int u = 0; u < LM_SUB; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) sum[u][e] = fmaf(s, acc[u][e], sum[u][e]);
    }
  }
  if (n >= N) return;
#pragma unroll
  for (int u = 0; u < LM_SUB; ++u) {
    const int k = k0 + 16 * u + 4 * q;
    if (vec) {
      if (k < Kd) {
        h4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f2e<BF>(sum[u][e]);
        *reinterpret_cast<h4*>(dst + row + k) = o;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (k + e < Kd) dst[row + k + e] = f2e<BF>(sum[u][e]);
    }
  }
}

extern "C" {

int tf_lora_merge_16(int dtype, void* dst, const void* base, const void* table, int n_adapters, int N, int Kd, tfStream_t s) {
  TF_REQUIRE(dtype == TF_DTYPE_F16 || dtype == TF_DTYPE_BF16, "tf_lora_merge_16: dtype=%d (0 = float16, 1 = bfloat16)", dtype);
  TF_REQUIRE(dst && base && table, "tf_lora_merge_16: null pointer (dst, base or table)");
  TF_REQUIRE(dst != base, "tf_lora_merge_16: dst and base must be distinct buffers");
  TF_REQUIRE(n_adapters >= 1 && n_adapters <= LM_MAX, "tf_lora_merge_16: n_adapters=%d (1..%d)", n_adapters, LM_MAX);
  TF_REQUIRE(N >= 1 && Kd >= 1, "tf_lora_merge_16: N=%d Kd=%d (both >= 1)", N, Kd);
  TF_REQUIRE((((uintptr_t)dst | (uintptr_t)base) & 1) == 0, "tf_lora_merge_16: dst and base must be 2-byte aligned");
  TF_REQUIRE((N + LM_TN - 1) / LM_TN <= 65535, "tf_lora_merge_16: N=%d exceeds one launch (%d rows)", N, 65535 * LM_TN);
  const tfLoraEntry* in = (const tfLoraEntry*)table;
  LoraTable t = {};
  t.n = n_adapters;
  for (int i = 0; i < n_adapters; ++i) {
    TF_REQUIRE(in[i].up && in[i].down_t, "tf_lora_merge_16: adapter %d holds a null pointer", i);
    TF_REQUIRE(in[i].rp >= 32 && in[i].rp % 32 == 0, "tf_lora_merge_16: adapter %d has Rp=%d (a positive multiple of 32)", i, in[i].rp);
    TF_REQUIRE((((uintptr_t)in[i].up | (uintptr_t)in[i].down_t) & 15) == 0, "tf_lora_merge_16: adapter %d is not 16-byte aligned", i);
    t.up[i] = in[i].up; t.down_t[i] = in[i].down_t; t.rp[i] = in[i].rp; t.s[i] = in[i].scale;
  }
  const int vec = Kd % 4 == 0 && (((uintptr_t)dst | (uintptr_t)base) & 7) == 0;
  const dim3 grid((unsigned)((Kd + LM_BK - 1) / LM_BK), (unsigned)((N + LM_TN - 1) / LM_TN));
  hipLaunchKernelGGL(dtype == TF_DTYPE_BF16 ? k_lora_merge<true> : k_lora_merge<false>, grid, dim3(LM_BLOCK), 0, tf_hs(s),
                     (half_t*)dst, (const half_t*)base, t, N, Kd, vec);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

}  // extern "C"
