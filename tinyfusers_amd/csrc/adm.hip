// Vector conditioning of an SDXL UNet (vision/unet.py: emb = time_embed(t) + label_emb(y), y = [pooled text | Fourier(size ids)]) and the row
// gather of the pooled text vector (vae/open_clip_text.py).  All three run in start() / encode_prompt, outside the captured step.  Own translation
// unit: no existing kernel's code changes.  Plain vector stores, no atomics: a launch computes the same bits every time.
#include "common.h"
#include "../../include/tinyfusers_hip.h"

#define ADM_BLOCK EW_BLOCK

// out (R, P + 6 D): row r = [pooled[r] | emb(ids[r, 0]) .. emb(ids[r, 5])], emb(t) = [cos(t f_i) | sin(t f_i)], i < D / 2 -- k_timestep_embedding's
// expression (csrc/elementwise.hip) for one scalar, term for term: the same fp32 operations in the same order, one rounding to 16 bits.  The pooled
// elements are moved as 16-bit words.  One block per row.  bf: the element type, a launch-uniform argument (these run once per start(): one
// kernel for both types keeps the library's kernel count down).
__global__ void __launch_bounds__(ADM_BLOCK) k_adm_vector(half_t* __restrict__ out, const unsigned short* __restrict__ pooled, const float* __restrict__ ids,
                                                          int P, int D, float max_period, bool bf) {
  const int r = blockIdx.x, half_dim = D / 2;
  const long long W = (long long)P + 6LL * D;
  half_t* o = out + r * W;
  unsigned short* ow = reinterpret_cast<unsigned short*>(o);
  const unsigned short* pr = pooled + (long long)r * P;
  for (int j = threadIdx.x; j < P; j += ADM_BLOCK) ow[j] = pr[j];
  for (int q = threadIdx.x; q < 6 * half_dim; q += ADM_BLOCK) {
    const int k = q / half_dim, i = q - k * half_dim;
    const float t = ids[r * 6 + k];
    float f = expf(-logf(max_period) * (float)i / (float)half_dim);
    float a = t * f;
    const float c = cosf(a), sn = sinf(a);
    o[P + (long long)k * D + i] = bf ? f2e<true>(c) : f2e<false>(c);
    o[P + (long long)k * D + half_dim + i] = bf ? f2e<true>(sn) : f2e<false>(sn);
  }
}

// out[s R + r, :] = round16(t_emb[s, :] + y_emb[r, :]): one fp32 add, one rounding; 8 elements (16 bytes) per lane and step
__global__ void __launch_bounds__(ADM_BLOCK) k_adm_emb_rows(h8* __restrict__ out, const h8* __restrict__ t_emb, const h8* __restrict__ y_emb,
                                                            long long vecs, int R, int E8, bool bf) {
  const long long gs = (long long)gridDim.x * ADM_BLOCK;
  for (long long v = (long long)blockIdx.x * ADM_BLOCK + threadIdx.x; v < vecs; v += gs) {
    const long long row = v / E8;
    const int c = (int)(v - row * E8);
    const long long s = row / R;
    const int r = (int)(row - s * R);
    const h8 a = t_emb[s * E8 + c], b = y_emb[(long long)r * E8 + c];
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = bf ? f2e<true>(e2f<true>(a[j]) + e2f<true>(b[j])) : f2e<false>(e2f<false>(a[j]) + e2f<false>(b[j]));
    out[v] = o;
  }
}

// out[b, :] = src[idx[b], :] as 16-byte vectors; an index outside [0, rows) writes zeros (nothing is read out of bounds)
__global__ void __launch_bounds__(ADM_BLOCK) k_gather_rows(uint4* __restrict__ out, const uint4* __restrict__ src, const int* __restrict__ idx,
                                                           long long vecs, int W8, int rows) {
  const long long gs = (long long)gridDim.x * ADM_BLOCK;
  for (long long v = (long long)blockIdx.x * ADM_BLOCK + threadIdx.x; v < vecs; v += gs) {
    const long long b = v / W8;
    const int c = (int)(v - b * W8);
    const int i = idx[b];
    out[v] = (i >= 0 && i < rows) ? src[(long long)i * W8 + c] : make_uint4(0u, 0u, 0u, 0u);
  }
}

extern "C" {

int tf_adm_vector_16(int dtype, void* out, const void* pooled, const void* ids_f32, int R, int P, int D, float max_period, tfStream_t s) {
  TF_REQUIRE(dtype == TF_DTYPE_F16 || dtype == TF_DTYPE_BF16, "tf_adm_vector_16: dtype=%d (0 = float16, 1 = bfloat16)", dtype);
  TF_REQUIRE(out && ids_f32 && R >= 1 && R <= 65535 && P >= 0 && (pooled || P == 0) && D >= 2 && D % 2 == 0 && D <= (1 << 20) && P <= (1 << 24),
             "tf_adm_vector_16: bad arguments (R=%d in 1..65535, P=%d >= 0, D=%d even and >= 2)", R, P, D);
  TF_REQUIRE(max_period > 0.0f, "tf_adm_vector_16: max_period=%g must be positive", (double)max_period);
  TF_REQUIRE((((uintptr_t)out | (uintptr_t)pooled) & 1) == 0 && ((uintptr_t)ids_f32 & 3) == 0, "tf_adm_vector_16: out / pooled must be 2-byte, ids 4-byte aligned");
  const unsigned short* pw = (const unsigned short*)pooled;
  const float* ids = (const float*)ids_f32;
  hipLaunchKernelGGL(k_adm_vector, dim3(R), dim3(ADM_BLOCK), 0, tf_hs(s), (half_t*)out, pw, ids, P, D, max_period, dtype == TF_DTYPE_BF16);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

int tf_adm_emb_rows_16(int dtype, void* out, const void* t_emb, const void* y_emb, int S, int R, int E, tfStream_t s) {
  TF_REQUIRE(dtype == TF_DTYPE_F16 || dtype == TF_DTYPE_BF16, "tf_adm_emb_rows_16: dtype=%d (0 = float16, 1 = bfloat16)", dtype);
  TF_REQUIRE(out && t_emb && y_emb && S >= 1 && R >= 1 && E >= 8 && E % 8 == 0, "tf_adm_emb_rows_16: bad arguments (S=%d >= 1, R=%d >= 1, E=%d a positive multiple of 8)", S, R, E);
  TF_REQUIRE((((uintptr_t)out | (uintptr_t)t_emb | (uintptr_t)y_emb) & 15) == 0, "tf_adm_emb_rows_16: every tensor must be 16-byte aligned");
  const long long vecs = (long long)S * R * (E / 8);
  TF_REQUIRE(vecs < (1LL << 40), "tf_adm_emb_rows_16: %lld 16-byte vectors", vecs);
  hipLaunchKernelGGL(k_adm_emb_rows, dim3(ew_grid(vecs)), dim3(ADM_BLOCK), 0, tf_hs(s), (h8*)out, (const h8*)t_emb, (const h8*)y_emb, vecs, R, E / 8, dtype == TF_DTYPE_BF16);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

int tf_gather_rows_16(void* out, const void* src, const void* idx_i32, int B, int W, int rows, tfStream_t s) {
  TF_REQUIRE(out && src && idx_i32 && B >= 1 && rows >= 1 && W >= 8 && W % 8 == 0, "tf_gather_rows_16: bad arguments (B=%d >= 1, rows=%d >= 1, W=%d a positive multiple of 8)", B, rows, W);
  TF_REQUIRE((((uintptr_t)out | (uintptr_t)src) & 15) == 0 && ((uintptr_t)idx_i32 & 3) == 0, "tf_gather_rows_16: out / src must be 16-byte, idx 4-byte aligned");
  const long long vecs = (long long)B * (W / 8);
  hipLaunchKernelGGL(k_gather_rows, dim3(ew_grid(vecs)), dim3(ADM_BLOCK), 0, tf_hs(s), (uint4*)out, (const uint4*)src, (const int*)idx_i32, vecs, W / 8, rows);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

}  // extern "C"
