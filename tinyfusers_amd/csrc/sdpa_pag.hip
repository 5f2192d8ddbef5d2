// Perturbed-attention guidance (Ahn et al. 2024): self-attention in which a DEVICE flag turns one batch range into the identity, o = v, inside the one
// launch (tf_sdpa_pag_16; attention/attention.py:35-41 with the softmax replaced by the identity matrix for the perturbed guidance group).  k_sdpa_pag
// is k_sdpa_dma's body (sdpa_dma_body.inc, untouched) behind a block-uniform early-out, in a translation unit of its own: the code objects of sdpa.hip,
// sdpa_split.hip and sdpa_dual.hip stay what they were without it.
#include "sdpa_common.h"

struct SdpaPagP {
  SdpaP p;                 // the launch as tf_sdpa_16 would fill it (causal = 0)
  const float* flag;       // one fp32 ON THE DEVICE, read when the kernel runs: != 0 perturbs the batch entries [b0, b1)
  int b0, b1;
};

// rows 0 .. nrow - 1 of v (HS elements each, v_st apart) to o (o_st apart), by the NT threads of the block: 16-byte chunks where both sides allow them
// (o's strides are only promised in multiples of 4 elements), 2-byte elements otherwise; the bits travel through integer registers
template <int HS, int NT>
__device__ __forceinline__ void sdpa_pag_copy(half_t* odst, const half_t* vsrc, long long o_st, long long v_st, int nrow) {
  typedef unsigned pag16 __attribute__((ext_vector_type(4)));
  if (((((uintptr_t)vsrc | (uintptr_t)odst) & 15) | ((v_st | o_st) & 7)) == 0) {
    constexpr int CK = HS / 8;
    for (int i = threadIdx.x; i < nrow * CK; i += NT) {
      const int r = i / CK, c = (i - r * CK) * 8;
      *reinterpret_cast<pag16*>(odst + r * o_st + c) = *reinterpret_cast<const pag16*>(vsrc + r * v_st + c);
    }
  } else {
    for (int i = threadIdx.x; i < nrow * HS; i += NT) {
      const int r = i / HS, c = i - r * HS;
      *reinterpret_cast<unsigned short*>(odst + r * o_st + c) = *reinterpret_cast<const unsigned short*>(vsrc + r * v_st + c);
    }
  }
}

// The waves per SIMD the registers of k_sdpa_dma<HS, QT, 0, NW> allow (the compiler's report; DESIGN 4.3 has the table).  With the early-out in front
// of it the body's scheduler otherwise settles one step lower for two instances (d = 64 and 80, 16-query waves: 73 / 96 VGPRs where k_sdpa_dma has 68 /
// 76), so k_sdpa_pag asks for k_sdpa_dma's figure: the attending blocks keep its register budget.
constexpr int sdpa_pag_waves(int HS, int QT, int NW) {
  return QT == 1 ? (HS <= 64 ? 7 : HS == 80 ? 6 : 3) : NW == 8 ? (HS == 40 ? 4 : 3) : HS <= 64 ? 4 : HS == 80 ? 3 : 2;
}
// A block whose batch entry lies in [b0, b1) while *flag != 0 copies its queries' rows of v to o -- the launch's own v and o strides, so both head-merge
// forms of the caller work -- and returns: q and k of that batch entry are never read.  The batch entry is a range test on sdpa_block's remapped block
// index (no division in front of the branch); the branch depends on blockIdx, the kernel arguments and one scalar load, so it is uniform per block, and
// it sits in front of the body's first LDS write, barrier and DMA issue.  Every other block runs the body as k_sdpa_dma<HS, QT, 0, NW, BF> does, in
// the same ring (the dynamic LDS size is the launcher's, below).
template <int HS, int QT, int NW, bool BF>
__global__ void __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(sdpa_pag_waves(HS, QT, NW)))) k_sdpa_pag(const SdpaPagP pp) {
  constexpr int KS = 1, SR = 0, DBG = 0;
  const SdpaP& p = pp.p;
  {
    constexpr int QB0 = 16 * NW * QT;
    const int nqb0 = (p.Tq + QB0 - 1) / QB0, per_b = nqb0 * p.NH, nblk0 = per_b * p.B;
    const int q0 = nblk0 >> 3, r0 = nblk0 & 7, xcd0 = blockIdx.x & 7;
    // sdpa_block's remap, restated: the shift here is the unsigned blockIdx's, sdpa_block's an int's, and a helper serving both merges the two computations,
    // which takes two instructions out of every k_sdpa_pag instance (profiles/sdpa_refactor_code_identity.txt) -- the code objects are to stay what they were
    const int bid0 = (xcd0 < r0 ? xcd0 * (q0 + 1) : r0 * (q0 + 1) + (xcd0 - r0) * q0) + (blockIdx.x >> 3);
    if (bid0 >= pp.b0 * per_b && bid0 < pp.b1 * per_b && *pp.flag != 0.f) {
      const SdpaBlk blk0 = sdpa_block(p, QB0);
      const int t0 = blk0.qb * QB0;
      sdpa_pag_copy<HS, NW * 64>(p.o + blk0.b * p.o_sb + blk0.h * p.o_sh + t0 * p.o_st, p.v + blk0.b * p.v_sb + blk0.h * p.v_sh + t0 * p.v_st, p.o_st, p.v_st,
                                 min(QB0, p.Tq - t0));
      return;
    }
  }
#include "sdpa_dma_body.inc"
}

template <int HS, int QT, int NW = 4>
static int launch_sdpa_pag(const SdpaPagP& pp, hipStream_t st) {
  return launch_sdpa_kernel<k_sdpa_pag<HS, QT, NW, kBF>>(pp, pp.p, sdpa_ring_bytes<HS, NW>(), 16 * NW * QT, NW, st);      // k_sdpa_dma<HS, QT, 0, NW>'s ring
}

int tfk_sdpa_pag_bf16(const SdpaPagP& pp, int inst, hipStream_t st);
int TFK(tfk_sdpa_pag)(const SdpaPagP& pp, int inst, hipStream_t st) {
  if (inst == TF_SDPA_INST_DMA16) return sdpa_by_head_size<40, 64, 80, 128, 160>(pp.p.HS, [&](auto hs) { return launch_sdpa_pag<hs, 1>(pp, st); });
  if (inst == TF_SDPA_INST_DMA32_W8) return sdpa_by_head_size<40, 80>(pp.p.HS, [&](auto hs) { return launch_sdpa_pag<hs, 2, 8>(pp, st); });     // (the rule names it for 40 and 80 only)
  return sdpa_by_head_size<40, 64, 80, 128, 160>(pp.p.HS, [&](auto hs) { return launch_sdpa_pag<hs, 2>(pp, st); });
}

#if !TF_TU_BF
// Which family a perturbed launch runs: sdpa_unsplit_dma_rule (tf_sdpa_dual_16's rule too); the generic kernel has no perturbed instance
static int sdpa_pag_rule(int B, int NH, int Tq, int Tk, int HS, long long k_st, long long v_st) {
  return sdpa_unsplit_dma_rule(B, NH, Tq, HS, sdpa_addressable(Tk, HS, k_st, v_st));
}
static int sdpa_pag_refuse(const char* who, int rule, int Tk, int HS, long long k_st, long long v_st) {
  if (rule == 0) return sdpa_refuse(who, Tk, HS, k_st, v_st);
  tf_set_error("%s: head size %d: the perturbed form exists for the LDS-DMA families only (head sizes 40, 64, 80, 128 and 160, TF_SDPA_GENERIC unset)", who, HS);
  return TF_E_UNSUPPORTED;
}
// the checks on sizes, strides and the batch range shared by the launch and the query; 0 or a status with the message set
static int sdpa_pag_args(const char* who, int dtype, int B, int NH, int Tq, int Tk, int HS, long long k_st, long long v_st, int b0, int b1) {
  if (int rc = sdpa_check_shape(who, &dtype, B, NH, Tq, Tk, nullptr, HS, 0)) return rc;
  const long long str[] = {k_st, v_st};
  if (int rc = sdpa_check_strides(who, "k / v", str, 2)) return rc;
  TF_REQUIRE(0 <= b0 && b0 <= b1 && b1 <= B, "%s: the perturbed batch range [%d, %d) must lie in [0, B = %d] (an empty range is plain attention)", who, b0, b1, B);
  return TF_OK;
}

extern "C" int tf_sdpa_pag_instance(int dtype, int B, int NH, int Tq, int Tk, int HS, long long k_st, long long v_st, int pag_b0, int pag_b1) {
  if (int rc = sdpa_pag_args("tf_sdpa_pag_instance", dtype, B, NH, Tq, Tk, HS, k_st, v_st, pag_b0, pag_b1)) return rc;
  TF_REQUIRE(B >= 1 && Tq >= 1, "tf_sdpa_pag_instance: bad sizes B=%d Tq=%d", B, Tq);
  const int rule = sdpa_pag_rule(B, NH, Tq, Tk, HS, k_st, v_st);
  return rule > 0 ? rule : sdpa_pag_refuse("tf_sdpa_pag_instance", rule, Tk, HS, k_st, v_st);
}

extern "C" int tf_sdpa_pag_16(int dtype, void* o, const void* q, const void* k, const void* v, int B, int NH, int Tq, int Tk, int HS, long long q_sb, long long q_sh,
                              long long q_st, long long k_sb, long long k_sh, long long k_st, long long v_sb, long long v_sh, long long v_st, long long o_sb, long long o_sh,
                              long long o_st, int pag_b0, int pag_b1, const float* pag_flag_dev, tfStream_t s) {
  const char* who = "tf_sdpa_pag_16";
  TF_REQUIRE(o && q && k && v, "%s: null tensor", who);
  TF_REQUIRE(pag_flag_dev, "%s: null flag (the device address of one fp32 word)", who);
  if (int rc = sdpa_pag_args(who, dtype, B, NH, Tq, Tk, HS, k_st, v_st, pag_b0, pag_b1)) return rc;
  SdpaPagP pp;
  pp.p = sdpa_params(o, q, k, v, B, NH, Tq, Tk, HS, q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, o_sb, o_sh, o_st, 0);
  pp.flag = pag_flag_dev; pp.b0 = pag_b0; pp.b1 = pag_b1;
  if (int rc = sdpa_check_launch(who, "q / k / v", pp.p)) return rc;
  if (B == 0 || Tq == 0) return TF_OK;
  // the instance is decided (and a shape without one refused) before anything touches the device
  const int rule = sdpa_pag_rule(B, NH, Tq, Tk, HS, k_st, v_st);
  if (rule <= 0) return sdpa_pag_refuse(who, rule, Tk, HS, k_st, v_st);
  hipStream_t st = tf_hs(s);
  TfProfScope prof_(TF_PROF_FAM_SDPA, 4.0 * B * NH * (double)Tq * Tk * HS, st);      // (booked as the plain launch: what runs depends on a device word)
  return dtype == TF_DTYPE_BF16 ? tfk_sdpa_pag_bf16(pp, rule, st) : tfk_sdpa_pag(pp, rule, st);
}
#endif
