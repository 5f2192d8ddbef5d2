// ControlNet on the captured SD-1.x step (vision/controlnet.py): the seam where the control residuals enter the UNet's skip connections
// (vision/unet.py:72: cat(x, saved.pop() + residual) in the controlled model) and the input edge of the hint stem.  Own translation unit: no
// existing kernel's code changes.
#include "common.h"
#include "../../include/tinyfusers_hip.h"

#define CT_MAX 16                        // entries of one launch (SD-1.5: 12 skip tensors + the middle block's output)
#define CT_BLOCK EW_BLOCK                // (k_hint_from_u8 launches on ew_grid)
#define CT_VPL 4                         // 16-byte vectors per lane and stream
#define CT_CHUNK (CT_BLOCK * CT_VPL)     // vectors of one block

// The whole table travels by value in the kernel arguments: nothing is uploaded, and a captured graph node owns its copy.
struct ControlTable {
  void* dst[CT_MAX];
  const void* skip[CT_MAX];
  const void* res[CT_MAX];
  unsigned vecs[CT_MAX];                 // 16-byte vectors of entry i (n / 8)
  unsigned first[CT_MAX + 1];            // prefix sum of the vectors, every entry rounded up to whole blocks: entry i owns [first[i], first[i+1])
  int n;
};

// dst_i = round16(fmaf(s_i, res_i, skip_i)), s_i = scales[i] read from device memory.  A block finds its entry from the prefix sums (every index
// into the table is a compile-time constant: the table stays in scalar registers); each lane moves CT_VPL 16-byte vectors per stream.
// dst may alias skip: every element is read, then written, by the same lane (all loads of a lane come first).  s_i == 0 copies the skip's
// bits (a uniform branch): 0 * inf would be NaN.  No atomics: a replay computes what the eager launch computes, bit for bit.
template <bool BF>
__global__ void __launch_bounds__(CT_BLOCK) k_control_add(const ControlTable t, const float* __restrict__ scales) {
  const unsigned g0 = blockIdx.x * (unsigned)CT_CHUNK;
  int e = 0;
  void* dst = t.dst[0];
  const void* skip = t.skip[0];
  const void* res = t.res[0];
  unsigned vecs = t.vecs[0], first = 0;
#pragma unroll
  for (int i = 1; i < CT_MAX; ++i) {
    if (i < t.n && g0 >= t.first[i]) {
      e = i; dst = t.dst[i]; skip = t.skip[i]; res = t.res[i]; vecs = t.vecs[i]; first = t.first[i];
    }
  }
  const float s = scales[e];
  const unsigned v0 = g0 - first + threadIdx.x;
  const h8* sk = reinterpret_cast<const h8*>(skip);
  const h8* rs = reinterpret_cast<const h8*>(res);
  h8* ds = reinterpret_cast<h8*>(dst);
  h8 a[CT_VPL], r[CT_VPL];
  if (s == 0.0f) {
    if (dst == skip) return;
#pragma unroll
    for (int j = 0; j < CT_VPL; ++j) if (v0 + j * CT_BLOCK < vecs) a[j] = sk[v0 + j * CT_BLOCK];
#pragma unroll
    for (int j = 0; j < CT_VPL; ++j) if (v0 + j * CT_BLOCK < vecs) ds[v0 + j * CT_BLOCK] = a[j];
    return;
  }
#pragma unroll
  for (int j = 0; j < CT_VPL; ++j) {
    if (v0 + j * CT_BLOCK < vecs) { a[j] = sk[v0 + j * CT_BLOCK]; r[j] = rs[v0 + j * CT_BLOCK]; }
  }
#pragma unroll
  for (int j = 0; j < CT_VPL; ++j) {
    if (v0 + j * CT_BLOCK < vecs) {
      h8 o;
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = f2e<BF>(fmaf(s, e2f<BF>(r[j][k]), e2f<BF>(a[j][k])));
      ds[v0 + j * CT_BLOCK] = o;
    }
  }
}

// uint8 -> x / 255 in the step's 16-bit type: one correctly rounded fp32 division of two exact integers, then one rounding to 16 bits.
// 8 elements per thread (8 bytes in, 16 out) when VEC, one otherwise
template <typename T, bool VEC>
__global__ void __launch_bounds__(CT_BLOCK) k_hint_from_u8(T* __restrict__ out, const unsigned char* __restrict__ in, long long n) {
  typedef T T8 __attribute__((ext_vector_type(8)));
  const long long gs = (long long)gridDim.x * CT_BLOCK;
  if (VEC) {
    const long long nv = n >> 3;
    for (long long i = (long long)blockIdx.x * CT_BLOCK + threadIdx.x; i < nv; i += gs) {
      const uint2 v = reinterpret_cast<const uint2*>(in)[i];
      T8 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = (T)((float)((v.x >> (8 * j)) & 0xffu) / 255.0f);
        o[4 + j] = (T)((float)((v.y >> (8 * j)) & 0xffu) / 255.0f);
      }
      reinterpret_cast<T8*>(out)[i] = o;
    }
  } else {
    for (long long i = (long long)blockIdx.x * CT_BLOCK + threadIdx.x; i < n; i += gs) out[i] = (T)((float)in[i] / 255.0f);
  }
}

extern "C" {

int tf_control_add_16(int dtype, const void* table, int n_entries, const void* scales_f32, tfStream_t s) {
  TF_REQUIRE(dtype == TF_DTYPE_F16 || dtype == TF_DTYPE_BF16, "tf_control_add_16: dtype=%d (0 = float16, 1 = bfloat16)", dtype);
  TF_REQUIRE(table && scales_f32 && n_entries >= 1 && n_entries <= CT_MAX, "tf_control_add_16: bad arguments (n_entries=%d, 1..%d)", n_entries, CT_MAX);
  TF_REQUIRE(((uintptr_t)scales_f32 & 3) == 0, "tf_control_add_16: scales must be 4-byte aligned");
  const tfControlEntry* in = (const tfControlEntry*)table;
  ControlTable t = {};
  t.n = n_entries;
  long long first = 0;
  for (int i = 0; i < n_entries; ++i) {
    TF_REQUIRE(in[i].dst && in[i].skip && in[i].residual, "tf_control_add_16: entry %d holds a null pointer", i);
    TF_REQUIRE(in[i].n > 0 && in[i].n % 8 == 0, "tf_control_add_16: entry %d has n=%lld (a positive multiple of 8)", i, in[i].n);
    TF_REQUIRE((((uintptr_t)in[i].dst | (uintptr_t)in[i].skip | (uintptr_t)in[i].residual) & 15) == 0, "tf_control_add_16: entry %d is not 16-byte aligned", i);
    const long long v = in[i].n >> 3;
    t.dst[i] = in[i].dst; t.skip[i] = in[i].skip; t.res[i] = in[i].residual;
    t.first[i] = (unsigned)first;
    first += (v + CT_CHUNK - 1) / CT_CHUNK * CT_CHUNK;
    TF_REQUIRE(first < (1LL << 31), "tf_control_add_16: %lld 16-byte vectors exceed one launch (2^31)", first);
    t.vecs[i] = (unsigned)v;
  }
  for (int i = n_entries; i <= CT_MAX; ++i) t.first[i] = (unsigned)first;
  const bool bf = dtype == TF_DTYPE_BF16;
  hipLaunchKernelGGL(bf ? k_control_add<true> : k_control_add<false>, dim3((unsigned)(first / CT_CHUNK)), dim3(CT_BLOCK), 0, tf_hs(s), t, (const float*)scales_f32);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

int tf_hint_from_u8_16(int dtype, void* out, const void* x_u8, long long n, tfStream_t s) {
  TF_REQUIRE(dtype == TF_DTYPE_F16 || dtype == TF_DTYPE_BF16, "tf_hint_from_u8_16: dtype=%d (0 = float16, 1 = bfloat16)", dtype);
  TF_REQUIRE(out && x_u8 && n >= 0, "tf_hint_from_u8_16: bad arguments (n=%lld)", n);
  TF_REQUIRE(((uintptr_t)out & 1) == 0, "tf_hint_from_u8_16: out must be 2-byte aligned");
  if (n == 0) return TF_OK;
  const bool vec = n % 8 == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)x_u8 & 7) == 0;
  const unsigned char* in = (const unsigned char*)x_u8;
  if (dtype == TF_DTYPE_BF16) {
    if (vec) hipLaunchKernelGGL((k_hint_from_u8<bf16_t, true>), dim3(ew_grid(n >> 3)), dim3(CT_BLOCK), 0, tf_hs(s), (bf16_t*)out, in, n);
    else hipLaunchKernelGGL((k_hint_from_u8<bf16_t, false>), dim3(ew_grid(n)), dim3(CT_BLOCK), 0, tf_hs(s), (bf16_t*)out, in, n);
  } else {
    if (vec) hipLaunchKernelGGL((k_hint_from_u8<half_t, true>), dim3(ew_grid(n >> 3)), dim3(CT_BLOCK), 0, tf_hs(s), (half_t*)out, in, n);
    else hipLaunchKernelGGL((k_hint_from_u8<half_t, false>), dim3(ew_grid(n)), dim3(CT_BLOCK), 0, tf_hs(s), (half_t*)out, in, n);
  }
  TF_LAUNCH_CHECK();
  return TF_OK;
}

}  // extern "C"
