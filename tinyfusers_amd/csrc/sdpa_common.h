// What the attention translation units share (sdpa.hip, sdpa_split.hip, sdpa_dual.hip, sdpa_pag.hip and their _bf16 twins): the launch arguments, the
// block decode, the wave reductions, the LDS-DMA pieces and layouts of the DMA family (sdpa_dma_body.inc), and the host side every entry repeats -- the
// SdpaP builder, the argument checks, the addressability rule and its refusal, the kernel launcher and the head-size dispatch.
// The kernels themselves: sdpa_generic.h (k_sdpa), sdpa_dma.h (k_sdpa_dma), and one unit each for k_sdpa_split, k_sdpa_dual and k_sdpa_pag.
#pragma once
#include <type_traits>
#include "common.h"
#include "../../include/tinyfusers_hip.h"

struct SdpaP {
  const half_t* q; const half_t* k; const half_t* v; half_t* o;
  int B, NH, Tq, Tk, HS;
  long long q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, o_sb, o_sh, o_st;
  float scale_log2e;
  int causal;
  int dbg;              // ablation build only (TF_SDPA_DBG, tools/sdpa_dbg.py): 1 no exp, 2 no P.V MFMAs, 4 no Q.K MFMAs, 8 no barrier, 16 no DMA in the loop, 32 no V reads, 64 no max
};

// max over the four 16-lane groups of the wave (lanes l, l^16, l^32, l^48), result in every lane: gfx950's v_permlane16_swap /
// v_permlane32_swap exchange rows between two registers in the VALU -- swap(x, x) leaves (row0,row0,row2,row2) and (row1,row1,row3,row3),
// whose max is the xor-16 butterfly; the 32-lane swap finishes it.  The ds_bpermute form (__shfl_xor) put two dependent LDS round trips
// in front of every tile's exponentials (self-attention 64 x 64, d = 40: 88.4 -> 85.3 us).
__device__ __forceinline__ float max_over_lane_groups(float v) {
  typedef unsigned u2v __attribute__((ext_vector_type(2)));
  u2v r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  float m = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  u2v q = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  return fmaxf(__uint_as_float(q[0]), __uint_as_float(q[1]));
}
// sum over the four 16-lane groups of the wave, result in every lane (the same order in every lane): max_over_lane_groups' two swaps with an add
__device__ __forceinline__ float sum_over_lane_groups(float v) {
  typedef unsigned u2v __attribute__((ext_vector_type(2)));
  u2v r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  float m = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  u2v q = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  return __uint_as_float(q[0]) + __uint_as_float(q[1]);
}

__device__ __forceinline__ s4v lds_tr16(const half_t* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)p);
}

// 1-D grid, XCD-aware: blocks i and i+8 share an XCD (and its L2).  Every XCD gets a contiguous run of work items with
// the query block fastest, so all query blocks of one (batch, head) sit on one XCD and its K/V stream through that
// L2 once instead of through all eight (bijective remap, any grid size).
struct SdpaBlk { int qb, h, b; };
__device__ __forceinline__ SdpaBlk sdpa_block(const SdpaP& p, const int QB = 128) {
  const int nqb = (p.Tq + QB - 1) / QB, nblk = nqb * p.NH * p.B;
  int bid = blockIdx.x;
  int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, idx = bid >> 3;
  bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  SdpaBlk o;
  int bh = bid / nqb;
  o.qb = bid - bh * nqb;
  o.b = bh / p.NH;
  o.h = bh - o.b * p.NH;
  return o;
}

// ---------------------------------------------------------------------------------------------------------------
// The LDS-DMA family (k_sdpa_dma and the kernels that share its body) for the head sizes of the SD UNets (40 / 80 / 160, plus 64 / 128).  In k_sdpa
// (sdpa_generic.h) a third of the time at d = 40 goes to moving K/V tiles global -> VGPR -> LDS (buffer loads, ds_writes, the vmcnt stall in front of
// them).  Here the tiles go global -> LDS directly (buffer_load_dwordx4 ... lds, 1 KiB per wave-instruction, no
// registers) into a ring of S stages, S-1 tiles in flight, one s_barrier per tile behind a counted vmcnt.
//   K image: row r = 16 kt + lr holds key 32 (kt>>1) + 8 (lr>>2) + 4 (kt&1) + (lr&3) (the key each MFMA A-row needs, so
//            a 16-lane read walks 16 consecutive rows); pitch = an odd number of 16-B chunks -> conflict-free b128 reads.
//   V image: natural key order, pitch chosen so the 4 rows x 32 B of a transposed read fall in distinct banks.
//   Pad chunks are fetched "out of range" (zeros).  Columns >= HS read by the 32-deep QK^T steps hold finite data of
//   the neighbouring row and meet zero Q columns; the LDS is zeroed once so no stale NaN pattern can be there.
//   Row sums: one extra MFMA per (key half, query tile) against an all-ones A fragment.
typedef int i4v __attribute__((ext_vector_type(4)));

// raw buffer descriptor in SGPRs (base, no stride, num_records in bytes, 32-bit raw format word of gfx9)
__device__ __forceinline__ i4v sdpa_rsrc(const void* base, unsigned bytes) {
  unsigned long long a = (unsigned long long)base;
  i4v r;
  r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
  r[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32) & 0xffff);
  r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
  r[3] = 0x00020000;
  return r;
}

// LDS-DMA issued from inline asm: the compiler does not see an LDS write, so it puts no vmcnt(0) in front of the
// ds_read_tr of the tile being consumed (it cannot tell the ring stages apart); ordering is the kernel's own
// counted s_waitcnt vmcnt + s_barrier.  16 B per lane, LDS destination = M0 + lane * 16, out-of-range lanes write 0.
__device__ __forceinline__ void sdpa_dma16(i4v rsrc, unsigned voffset_bytes, unsigned lds_base) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
               :: "s"(__builtin_amdgcn_readfirstlane((int)lds_base)), "v"(voffset_bytes), "s"(rsrc) : "memory");   // M0 has no other user in k_sdpa_dma (gfx9 DS ops do not read it)
}

// LDS layouts are chosen against the real bank model of the chip (64 banks x 4 B; a ds_read_b128 is served in four groups of
// 16 NON-contiguous lanes, a ds_read_b64_tr_b16 in two groups of 32; tools/lds_conflicts.py enumerates the costs):
//   K rows (16 consecutive rows per 16-lane read, 4 chunk columns across the lane groups): conflict-free exactly when the
//     pitch in 16-B chunks is 2 (mod 4): 6 / 10 / 10 / 18 / 22 chunks for d = 40 / 64 / 80 / 128 / 160 (an odd pitch costs 2x);
//   V rows (keys k and k + 8 of a 32-key half land in the same 32-lane group): no plain pitch is conflict-free; a skew of a
//     few chunks after every 8 rows is: (pitch, skew) = (6, 8) / (10, 8) / (10, 8) / (18, 8) / (20, 2) chunks.
constexpr int sdpa_k_pitch(int ck) { return ck + (2 - ck % 4 + 4) % 4; }
constexpr int sdpa_v_pitch(int ck) { return ck <= 6 ? 6 : ck <= 10 ? 10 : ck <= 18 ? 18 : ck <= 20 ? 20 : 22; }
constexpr int sdpa_v_skew(int ck) { return ck <= 18 ? 8 : ck <= 20 ? 2 : 8; }

// ring depth: SdpaDma<HS>::S (<= 4) for both block sizes.  Six stages for the 8-wave form (two blocks per CU leave 80 KiB each) were slower:
// 64 x 64 d40 81.8 -> 86.9 us, 96 x 96 (B 8) 1116 -> 1162 us -- the tile fetch is not latency-starved at depth 4, and the prologue zero-fills the ring
constexpr int sdpa_ring(int stage_b, int nw, int s4) { return s4; }
template <int HS>
struct SdpaDma {
  static constexpr int DQK = (HS + 31) / 32 * 32, NKS = DQK / 32, NDT = (HS + 15) / 16, CK = HS / 8;
  // HAS_PAD: the P.V tiles have spare columns (HS % 16 != 0, d = 40): column HS of the V image is preset to 1 in LDS and kept out of the
  // DMA (EXEC-masked lanes write nothing), so the row sums come out of the P.V MFMAs themselves and the ones-MFMA (4 of 32 per tile) goes
  static constexpr bool HAS_PAD = (HS % 16) != 0;
  static constexpr int KPC = sdpa_k_pitch(CK), VPC = sdpa_v_pitch(CK), VSC = sdpa_v_skew(CK);   // pitches / skew in 16-B chunks
  static constexpr int KP = KPC * 8, VP = VPC * 8, VSK = VSC * 8; // pitches / skew in halves
  static constexpr int VGC = 8 * VPC + VSC;                        // chunks per group of 8 V rows (rows + skew pad)
  static constexpr int NKI = KPC, NVI = (8 * VGC + 63) / 64;       // 1-KiB pieces of the K / V image (64 rows each)
  static constexpr int K_BYTES = NKI * 1024, STAGE_B = (NKI + NVI) * 1024;
  static constexpr int S = (144 * 1024 / STAGE_B) >= 4 ? 4 : (144 * 1024 / STAGE_B);
  static constexpr int NI = NKI + NVI, LPW = (NI + 3) / 4;        // 1-KiB pieces per tile / per wave
  static_assert(S >= 2, "ring needs two stages");
};
// the dynamic LDS of a kernel that runs the body unsplit (k_sdpa_dma, k_sdpa_dual, k_sdpa_pag): one ring
template <int HS, int NW>
constexpr int sdpa_ring_bytes() { return sdpa_ring(SdpaDma<HS>::STAGE_B, NW, SdpaDma<HS>::S) * SdpaDma<HS>::STAGE_B; }

// ---------------------------------------------------------------------------------------------------------------
// Host side.  What crosses the units: the split forms (sdpa_split.hip holds the kernels, tf_sdpa_f16's rule picks), and the unsplit part of that rule
// (sdpa_instance_unsplit in sdpa.hip, the float16 unit), which the dual and the perturbed launch ask for on their own.
// The split forms, k_sdpa_split<HS, QT, NW, KS, SR>.  Measured and NOT kept (profiles/r06_sdpa_split.txt): <40, 2, 8, 2, 3> (4 x 2 waves,
// 128 queries per block, two blocks per CU: 84-85 us against the unsplit 82 -- half the queries per fetched tile) and <80, 2, 8, 2, 3> (32-query waves:
// 128 blocks, half the CUs; 20.2 us against 17.2).
enum { SDPA_SPLIT_40_W16 = 1,    // <40, 2, 16, 2, 4>: 8 query waves x 2 slices, 256 queries per block, one block per CU (104 KiB): four waves per SIMD
       SDPA_SPLIT_80_Q16 = 2 };  // <80, 1, 8, 2, 3>: 16-query waves, 4 x 2, 64 queries per block (126 KiB): two waves per SIMD
int tfk_sdpa_split(const SdpaP& p, int form, hipStream_t st);
int tfk_sdpa_split_bf16(const SdpaP& p, int form, hipStream_t st);
int tfk_sdpa_instance_unsplit(int B, int NH, int Tq, int HS);

// the launch as every entry fills it from its pointer / size / stride arguments (nothing here is checked yet; dbg: sdpa.hip's own business)
static SdpaP sdpa_params(void* o, const void* q, const void* k, const void* v, int B, int NH, int Tq, int Tk, int HS, long long q_sb, long long q_sh, long long q_st,
                         long long k_sb, long long k_sh, long long k_st, long long v_sb, long long v_sh, long long v_st, long long o_sb, long long o_sh, long long o_st,
                         int causal) {
  SdpaP p;
  p.q = (const half_t*)q; p.k = (const half_t*)k; p.v = (const half_t*)v; p.o = (half_t*)o;
  p.B = B; p.NH = NH; p.Tq = Tq; p.Tk = Tk; p.HS = HS;
  p.q_sb = q_sb; p.q_sh = q_sh; p.q_st = q_st; p.k_sb = k_sb; p.k_sh = k_sh; p.k_st = k_st;
  p.v_sb = v_sb; p.v_sh = v_sh; p.v_st = v_st; p.o_sb = o_sb; p.o_sh = o_sh; p.o_st = o_st;
  p.scale_log2e = (1.0f / sqrtf((float)HS)) * 1.4426950408889634f;
  p.causal = causal;
  p.dbg = 0;
  return p;
}

// The argument checks, in the order every entry and query makes them; 0 or TF_E_ARG with the message set.  An entry puts its own extras (Tk2 <= 64, the
// batch range, the flag pointer) where it always had them, between these.
// dtype: null where the entry has none.  Tk2: the second key count of the dual form, or null.  least: 1 where the caller is a query (B and Tq of 0 are no launch to name)
static int sdpa_check_shape(const char* who, const int* dtype, int B, int NH, int Tq, int Tk, const int* Tk2, int HS, int least) {
  if (dtype) TF_REQUIRE(*dtype == TF_DTYPE_F16 || *dtype == TF_DTYPE_BF16, "%s: dtype=%d (0 = float16, 1 = bfloat16)", who, *dtype);
  if (Tk2) TF_REQUIRE(B >= least && NH >= 1 && Tq >= least && Tk >= 1 && *Tk2 >= 1, "%s: bad sizes B=%d NH=%d Tq=%d Tk=%d Tk2=%d", who, B, NH, Tq, Tk, *Tk2);
  else TF_REQUIRE(B >= least && NH >= 1 && Tq >= least && Tk >= 1, "%s: bad sizes B=%d NH=%d Tq=%d Tk=%d", who, B, NH, Tq, Tk);
  TF_REQUIRE(HS >= 8 && HS % 8 == 0 && HS <= 160, "%s: head size %d must be a multiple of 8 in [8, 160]", who, HS);
  return TF_OK;
}
// names: the tensors as the entry's message lists them ("k / v")
static int sdpa_check_strides(const char* who, const char* names, const long long* str, int n) {
  for (int i = 0; i < n; ++i) TF_REQUIRE(str[i] % 8 == 0, "%s: %s strides must be multiples of 8 elements (16-B rows)", who, names);
  return TF_OK;
}
// what only a launch checks: the grid, every q / k / v stride of p plus the entry's further ones, the output strides
static int sdpa_check_launch(const char* who, const char* names, const SdpaP& p, const long long* more = nullptr, int nmore = 0) {
  TF_REQUIRE((long long)((p.Tq + 63) / 64) * p.NH * p.B < (1ll << 31), "%s: too many (query block, head, batch) work items", who);
  const long long str[] = {p.q_sb, p.q_sh, p.q_st, p.k_sb, p.k_sh, p.k_st, p.v_sb, p.v_sh, p.v_st};
  if (int rc = sdpa_check_strides(who, names, str, 9)) return rc;
  if (int rc = sdpa_check_strides(who, names, more, nmore)) return rc;
  TF_REQUIRE(p.o_sb % 4 == 0 && p.o_sh % 4 == 0 && p.o_st % 4 == 0, "%s: output strides must be multiples of 4 elements", who);
  return TF_OK;
}

// K/V offsets inside a (batch, head) slice must fit 32-bit byte offsets: the buffer offsets of the DMA kernels, and k_sdpa's own
// (unsigned)(key * k_st + col) * 2u under a 32-bit num_records
static bool sdpa_addressable(int Tk, int HS, long long k_st, long long v_st) {
  return ((long long)Tk * k_st + HS) * 2 < (1ll << 31) && ((long long)Tk * v_st + HS) * 2 < (1ll << 31);
}
static int sdpa_refuse(const char* who, int Tk, int HS, long long k_st, long long v_st) {
  tf_set_error("%s: the keys / values of one (batch, head) slice span %lld / %lld bytes (Tk=%d, token strides %lld / %lld elements); every attention kernel "
               "addresses a slice with 32-bit byte offsets (< 2 GiB)", who, ((long long)Tk * k_st + HS) * 2, ((long long)Tk * v_st + HS) * 2, Tk, k_st, v_st);
  return TF_E_UNSUPPORTED;
}
// Which family a dual or a perturbed launch runs: the one sdpa_instance (sdpa.hip) names with the split forms left out, among the LDS-DMA families --
// the only ones with such instances.  0: a key set no kernel can address (the caller says which, `addressable`); < 0: the rule names the generic kernel.
static int sdpa_unsplit_dma_rule(int B, int NH, int Tq, int HS, bool addressable) {
  if (!addressable) return 0;
  const int inst = tfk_sdpa_instance_unsplit(B, NH, Tq, HS);
  return inst == TF_SDPA_INST_DMA16 || inst == TF_SDPA_INST_DMA32 || inst == TF_SDPA_INST_DMA32_W8 ? inst : -1;
}

// Launch of an attention kernel (k_sdpa, k_sdpa_dma, k_sdpa_split, k_sdpa_dual, k_sdpa_pag): its dynamic LDS is allowed once per kernel, the grid is
// one block of NW waves per QB queries of every (batch, head) of p.  arg: the kernel's argument struct (p itself, or the struct that holds it).
template <auto Kern, class Arg>
static int launch_sdpa_kernel(const Arg& arg, const SdpaP& p, int smem, int QB, int NW, hipStream_t st) {
  static bool attr_set = false;
  if (!attr_set) {
    TF_HIP(hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    attr_set = true;
  }
  hipLaunchKernelGGL(Kern, dim3((unsigned)((p.Tq + QB - 1) / QB * p.NH * p.B)), dim3(NW * 64), smem, st, arg);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

// f(std::integral_constant<int, H>) for the H among HS0, HSs... that HS equals: the head sizes a family is built for, as template arguments, so that
// `[&](auto hs) { return launch<hs, ...>(...); }` names one instance per size.  The rule a caller branched on names a family only for head sizes it has;
// anything else is refused here, not launched as another size.  (A chain, not a fold: the kernels are instantiated -- and laid out in the code object --
// in the order of the list.)
template <int HS0, int... HSs, class F>
static int sdpa_by_head_size(int HS, F&& f) {
  if (HS == HS0) return f(std::integral_constant<int, HS0>{});
  if constexpr (sizeof...(HSs) > 0) return sdpa_by_head_size<HSs...>(HS, f);
  tf_set_error("tf_sdpa: no instance of this kernel family for head size %d", HS);
  return TF_E_UNSUPPORTED;
}
