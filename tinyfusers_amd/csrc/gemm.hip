// Implicit-GEMM convolution / linear on MFMA, gfx950: HOST side -- run_gemm (resolve the configuration of a launch, then launch it) and the C-ABI
// entries -- and the small kernels around the GEMMs (e4m3 packing, GEMV, LayerNorm weight fold).  The rest of the dispatcher is in host-only headers:
// gemm_family.h (the kernel families by name, which launches each can take, launch_one), gemm_tune.h (cost model, tuning table, autotuner) and
// gemm_prof.h (event profiling); the split-K reduce kernels are gemm_reduce.hip.  The GEMM kernels live in gemm_{igemm,patch,igemm8,pp,pp3,c4,c8,ar}.h
// and are instantiated in gemm_k_*.hip, one translation unit per family so that they compile in parallel; gemm_common.h holds GemmP, the shared
// epilogue and the launcher declarations (its head comment describes the computation).
#include "gemm_prof.h"

// ---- fp8 (OCP e4m3) packing for the config-5 path ---------------------------------------------------------------------------
// activations: y8 = e4m3(x * scale), saturating (8 elements per thread, 16-byte loads / 8-byte stores)
__global__ void __launch_bounds__(256) k_quantize_fp8(unsigned char* __restrict__ y, const half_t* __restrict__ x, float scale, long long n8) {
  long long gs = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += gs) {
    h8 v = *reinterpret_cast<const h8*>(x + i * 8);
    f4 a, b;
    for (int e = 0; e < 4; ++e) { a[e] = (float)v[e] * scale; b[e] = (float)v[4 + e] * scale; }
    *reinterpret_cast<uint2*>(y + i * 8) = pack8_fp8(a, b);
  }
}
// block-scaled form (common.h: mx_quant8): rows x C fp16 -> rows x C codes + rows x C/32 E8M0 bytes behind them; a thread = 8 channels, 4 lanes = a block
__global__ void __launch_bounds__(256) k_quantize_mx8(unsigned char* __restrict__ y, const half_t* __restrict__ x, long long rows, int C) {
  const long long n8 = rows * (C >> 3), gs = (long long)gridDim.x * 256;
  const int cv8 = C >> 3;
  for (long long i0 = (long long)blockIdx.x * 256; i0 < n8; i0 += gs) {       // (block-uniform loop bound: every lane reaches the shuffles)
    const long long i = i0 + threadIdx.x;
    const bool live = i < n8;
    f4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      h8 v = *reinterpret_cast<const h8*>(x + i * 8);
      for (int e = 0; e < 4; ++e) { a[e] = (float)v[e]; b[e] = (float)v[4 + e]; }
    }
    unsigned sb;
    const uint2 code = mx_quant8(a, b, sb);
    if (live) {
      *reinterpret_cast<uint2*>(y + i * 8) = code;
      if ((i & 3) == 0) { const long long row = i / cv8; y[rows * C + row * (C >> 5) + ((i - row * cv8) >> 2)] = (unsigned char)sb; }
    }
  }
}
// weights: one wave per output row n: scale[n] = max|w[n, :]| / 448 (1 for an all-zero row), w8[n, k] = e4m3(w[n, k] / scale[n])
__global__ void __launch_bounds__(256) k_pack_weight_fp8(unsigned char* __restrict__ w8, float* __restrict__ scale, const half_t* __restrict__ w, int N, int K) {
  int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
  int n = blockIdx.x * 4 + wv;
  if (n >= N) return;
  const half_t* wr = w + (long long)n * K;
  float m = 0.f;
  for (int k = l * 8; k < K; k += 512) { h8 v = *reinterpret_cast<const h8*>(wr + k); for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf((float)v[j])); }
  m = wave_max(m);
  const float sc = m > 0.f ? __fdiv_rn(m, 448.0f) : 1.0f;
  if (l == 0) scale[n] = sc;
  for (int k = l * 8; k < K; k += 512) {
    h8 v = *reinterpret_cast<const h8*>(wr + k);
    f4 a, b;
    // a correctly rounded quotient (not w * (1 / scale)): a value on an e4m3 code boundary must round the way the definition says
    for (int e = 0; e < 4; ++e) { a[e] = __fdiv_rn((float)v[e], sc); b[e] = __fdiv_rn((float)v[4 + e], sc); }
    *reinterpret_cast<uint2*>(w8 + (long long)n * K + k) = pack8_fp8(a, b);
  }
}

// ---- weight-streaming GEMV for M <= 8 (time-embedding MLP, ResBlock emb_layers): one wave per output row; blockIdx.y: the group of 8 input
// rows a block serves (tf_gemv_rows_16 -- tf_gemv_16 launches the one group, y = 0)
template <bool BF = false>
__global__ void __launch_bounds__(256) k_gemv(half_t* __restrict__ y, const half_t* __restrict__ x, const half_t* __restrict__ w,
                                              const half_t* __restrict__ bias, int M, int N, int K, int silu_in) {
  int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
  int n = blockIdx.x * 4 + wv;
  if (n >= N) return;
  const int m0 = blockIdx.y * 8;
  x += (long long)m0 * K; y += (long long)m0 * N; M = min(M - m0, 8);
  const half_t* wr = w + (long long)n * K;
  float acc[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) acc[m] = 0.f;
  for (int k = l * 8; k < K; k += 512) {
    h8 wv8 = *reinterpret_cast<const h8*>(wr + k);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      if (m < M) {
        h8 xv = *reinterpret_cast<const h8*>(x + (long long)m * K + k);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float xf = e2f<BF>(xv[j]);
          if (silu_in) xf = silu_f(xf);
          acc[m] += xf * e2f<BF>(wv8[j]);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    if (m < M) {
      float v = wave_sum(acc[m]);
      if (l == 0) y[(long long)m * N + n] = f2e<BF>(v + (bias ? e2f<BF>(bias[n]) : 0.f));
    }
  }
}

// LayerNorm fold of a Linear weight (one wave per output row n):
//   w'[n,k] = fp16(w[n,k] * gamma[k]);  colsum[n] = sum_k float(w'[n,k]);  bias'[n] = sum_k beta[k] * w[n,k] + bias[n]
template <bool BF = false>
__global__ void __launch_bounds__(256) k_ln_fold(half_t* __restrict__ wo, half_t* __restrict__ bo, float* __restrict__ colsum, const half_t* __restrict__ w,
                                                 const half_t* __restrict__ bias, const half_t* __restrict__ gamma, const half_t* __restrict__ beta, int N, int K) {
  int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
  int n = blockIdx.x * 4 + wv;
  if (n >= N) return;
  float cs = 0.f, bs = 0.f;
  for (int k = l * 8; k < K; k += 512) {
    h8 v = *reinterpret_cast<const h8*>(w + (long long)n * K + k), g = *reinterpret_cast<const h8*>(gamma + k), b = *reinterpret_cast<const h8*>(beta + k), o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      o[j] = f2e<BF>(e2f<BF>(v[j]) * e2f<BF>(g[j]));
      cs += e2f<BF>(o[j]);
      bs += e2f<BF>(b[j]) * e2f<BF>(v[j]);
    }
    *reinterpret_cast<h8*>(wo + (long long)n * K + k) = o;
  }
  cs = wave_sum(cs); bs = wave_sum(bs);
  if (l == 0) { colsum[n] = cs; bo[n] = f2e<BF>(bs + (bias ? e2f<BF>(bias[n]) : 0.f)); }
}

// ------------------------------------------------------------------------------------------------
static int g_dbg = 0, g_force_variant = -1, g_force_order = -1;   // tf_gemm_debug

#if TF_IGEMM_STAMP
// diagnostic build (tools/igemm_stamp.py): every k_igemm launch writes its blocks' phase stamps here; tf_debug_stamps copies them out
static unsigned long long* g_stamp_buf = nullptr;
#define TF_STAMP_BLOCKS 8192
extern "C" int tf_debug_stamps(void* host_out, int blocks) {
  TF_REQUIRE(host_out && blocks >= 1 && blocks <= TF_STAMP_BLOCKS && g_stamp_buf, "tf_debug_stamps: no stamps");
  TF_HIP(hipMemcpy(host_out, g_stamp_buf, (size_t)blocks * 64, hipMemcpyDeviceToHost));
  return TF_OK;
}
extern "C" int tf_debug_loop_stamps(void* host_out) {      // TF_IGEMM_STAMP == 2: 256 K tiles x 8 u32 stamps of block 0 (behind the per-block table)
  TF_REQUIRE(host_out && g_stamp_buf, "tf_debug_loop_stamps: no stamps");
  TF_HIP(hipMemcpy(host_out, g_stamp_buf + (size_t)TF_STAMP_BLOCKS * 8, 256 * 8 * 4, hipMemcpyDeviceToHost));
  return TF_OK;
}
#endif

// The family of a configuration against what the launch really is: a family that cannot take the launch gives way to its fallback when the
// configuration came from a table row, and fails by name when it was asked for explicitly (tf_gemm_debug).  The families without a fallback (the
// k_igemm forms) pass: launch_one reports what they cannot take.  `stats_heard`: the caller listens for GroupNorm statistics.
static int settle_variant(const GemmP& p, TunedCfg* t, bool forced_tile, bool allow_split, bool stats_heard) {
  GemmP q = p;
  if (!stats_heard) q.gn_part = nullptr;                  // (statistics the caller did not ask to hear about are never requested)
  for (const Family* f = &kFamily[t->variant]; f->fallback != V_NONE; f = &kFamily[t->variant]) {
    // a family with a tile of its own runs that tile; a forced tile keeps the family only where the kernel has it
    TileCfg c = f->own_tile ? f->own_tile(p) : t->c;
    const bool refused = f->forced_tile_first && forced_tile && (t->c.bm != c.bm || t->c.bn != c.bn || t->c.splitk != c.splitk);
    if (!refused && family_admits(t->variant, q, c)) { t->c = c; break; }
    if (g_force_variant == t->variant) { tf_set_error("run_gemm: the %s kernel cannot run this launch (tile %dx%d)", f->name, t->c.bm, t->c.bn); return TF_E_UNSUPPORTED; }
    t->variant = f->fallback;
    if (f->retile_rows >= 0 && t->c.bm >= f->retile_rows) t->c = choose_tiles(p.M, p.N, p.K, p.act, allow_split);
  }
  return TF_OK;
}

// The configuration a launch runs with: the untuned default of its kind, replaced by a forced tile or by the shape's row of the tuning table (tuned
// on first use where that is allowed), clamped to what the launch and its workspace allow, and settled on a family that can take it.
static int resolve(const GemmP& p, void* workspace, size_t workspace_bytes, int force_bm, int force_bn, int force_split, hipStream_t st, bool stats_heard, TunedCfg* out) {
  TunedCfg t = {choose_tiles(p.M, p.N, p.K, p.act, true), V_RING, 0};
  bool tuned = false;
  if (p.gi_part) { t = gi_default(p); tuned = true; }    // (tuned: keep gi_default's variant unless the tuner knows better)
  if (p.fp8 && !p.mx) {                                   // untuned fp8 default: the widest tile that still gives every CU a block
    long long b128 = (long long)((p.M + 127) / 128) * ((p.N + 127) / 128);
    t.c = {p.M >= 128 ? 128 : 64, p.act == 1 || p.N >= 128 ? 128 : 64, b128 >= 128 ? 1 : t.c.splitk};
    t.variant = V_RING; tuned = true;
  }
  if (p.mx) {                                             // block-scaled e4m3: the ping-pong kernel or nothing (tf_mx8_gemm_supported tells a caller beforehand)
    t = mx_default(p);
    if (!t.c.bm) { tf_set_error("run_gemm: no block-scaled e4m3 kernel for M=%d N=%d K=%d (S=%d stride=%d ups=%d act=%d): ask tf_mx8_gemm_supported first", p.M, p.N, p.K, p.S, p.stride, p.ups, p.act); return TF_E_UNSUPPORTED; }
    tuned = true;
  }
  const TunedCfg untuned = t;
  if (force_bm) {
    t.c = {force_bm, force_bn, force_split > 0 ? force_split : 1};
    t.order = g_force_order > 0 ? 1 : 0;
    if (p.gi_part) t.variant = p.S == 3 ? V_PATCH : V_RING;
  } else if (g_autotune && !g_dbg) {
    const TuneKey key = tune_key(p);
    auto it = g_tuned.find(key);
    if (it == g_tuned.end() && p.bf16) {                    // a bfloat16 launch without a row of its own takes the fp16 row of the shape: the same kernels, the same bytes and FLOPs
      TuneKey k16 = key;
      k16[9] &= ~1024;
      it = g_tuned.find(k16);
    }
    if (g_trace_keys) g_traced[key] = it != g_tuned.end();
    if (it != g_tuned.end()) {
      t = it->second; tuned = true;
      // a table row (shipped, or loaded from a user's file) whose tile cannot carry this launch's input GroupNorm -- the key holds
      // only a gi flag, not HoWo / H / W -- falls back to the first admissible tile instead of failing the forward
      if (p.gi_part && !gi_tile_ok(p, t.c.bm, t.c.bn, t.variant)) t = gi_default(p);
      // e4m3 rows: a fixed-scale launch has k_igemm8 only, a block-scaled one the ping-pong kernel only -- a row that says otherwise (an
      // older table, a user's file) falls back to the default instead of failing the forward
      if (p.fp8) {
        const bool blk = kFamily[t.variant].pingpong;
        if (blk != (p.mx != 0) || (blk && !family_admits(t.variant, p, t.c))) t = untuned;
      }
    }
    else if (g_autotune == 2) {
      tf_set_error("run_gemm: shape M=%d N=%d K=%d C1=%d C2=%d S=%d stride=%d ups=%d act=%d flags=%d is not in the tuning table and tuning is off "
                   "(tf_gemm_autotune(2): with WORLD_SIZE > 1 every rank must run the same kernels); tune it on one GPU (tools/tune_best.sh) and ship the row",
                   key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7], key[8], key[9]);
      return TF_E_STATE;
    }
    else {
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      (void)hipStreamIsCapturing(st, &cs);
      if (cs == hipStreamCaptureStatusNone) {
        int rc = autotune(p, workspace, workspace_bytes, st, &t);
        if (rc) return rc;
        g_tuned[key] = t;
        tuned = true;
      }
    }
  }
  if (p.ln_colsum || p.out32) t.c.splitk = 1;            // row statistics need the whole K range in one block; so does the raw fp32 output
  if (t.c.splitk > 1) {
    size_t need = (size_t)t.c.splitk * p.M * p.N * sizeof(float);
    if (!workspace || workspace_bytes < need) t.c.splitk = 1;   // degrade gracefully: correctness does not depend on split-K
  }
  if (!tuned) {
    // cost-model fallback: WIDE (two blocks per CU) pays when a CU gets several tiles with a short K loop each
    long long blocks = (long long)((p.M + t.c.bm - 1) / t.c.bm) * ((p.N + t.c.bn - 1) / t.c.bn) * t.c.splitk;
    t.variant = (blocks > 256 && p.ktiles / t.c.splitk <= 24) ? V_WIDE : V_RING;
  }
  if (g_force_variant >= 0 && !(p.gi_part && p.S == 3)) t.variant = g_force_variant;
  // k_igemm_patch has no LayerNorm fold (patch_setup): asked for by name on a folded launch it says so, like the families with a fallback in
  // settle_variant -- the deep ring it quietly runs instead is for the convolution geometries it refuses, not for another epilogue
  if (g_force_variant == V_PATCH && p.ln_colsum) { tf_set_error("run_gemm: the patch kernel cannot run this launch (the LayerNorm fold; M=%d N=%d K=%d)", p.M, p.N, p.K); return TF_E_UNSUPPORTED; }
  int rc = settle_variant(p, &t, force_bm != 0, workspace != nullptr, stats_heard);
  if (rc) return rc;
  if (g_force_order >= 0) t.order = g_force_order;
  *out = t;
  return TF_OK;
}

// GroupNorm statistics of the output: they ride along only when the chosen tiling maps m-tiles onto whole images; otherwise the caller is told
// (chunks = 0) and runs the stand-alone statistics pass
static void plan_gn_stats(GemmP& p, const TunedCfg& t, int* gn_chunks) {
  if (!p.gn_part) return;
  const int eff = eff_splitk(p, t.variant, t.c.splitk);
  TileCfg sc = t.c;
  sc.bm = stats_bm(t.c.bm, t.variant);
  if (eff == 1 && !gn_tile_ok(p, sc.bm, sc.bn)) p.gn_part = nullptr;
  if (gn_chunks) *gn_chunks = p.gn_part ? gn_chunks_for(p, sc, eff) : 0;
  if (gn_chunks && p.gn_part && eff > 1 && p.on_z && tfk_splitk_reduce_applies_gn(p.HoWo, p.N, p.gn_G)) *gn_chunks = 1;   // the fused reduce leaves whole-image sums
}

static int run_gemm(GemmP p, void* workspace, size_t workspace_bytes, int force_bm, int force_bn, int force_split, hipStream_t st, int* gn_chunks = nullptr) {
#if TF_IGEMM_STAMP
  if (!g_stamp_buf) { TF_HIP(hipMalloc((void**)&g_stamp_buf, (size_t)TF_STAMP_BLOCKS * 64 + 256 * 8 * 4)); TF_HIP(hipMemset(g_stamp_buf, 0, (size_t)TF_STAMP_BLOCKS * 64 + 256 * 8 * 4)); }
  p.stamp = g_stamp_buf;
#endif
  p.ktiles = (p.K + 63) / 64;
  p.dbg = g_dbg;
  fast_div_magic((unsigned)p.HoWo, &p.dv_howo_mul, &p.dv_howo_shr);
  fast_div_magic((unsigned)p.Wo, &p.dv_wo_mul, &p.dv_wo_shr);
  TunedCfg t;
  int rc = resolve(p, workspace, workspace_bytes, force_bm, force_bn, force_split, st, gn_chunks != nullptr, &t);
  if (rc) return rc;
  ProfRec rec;
  if (g_prof && (rc = prof_begin(&rec, p, t, st))) return rc;
  plan_gn_stats(p, t, gn_chunks);
  rc = launch_one(p, t.c, t.variant, t.order, workspace, st);
  return g_prof ? prof_end(&rec, p, t, rc, st) : rc;
}

// workspace the caller must provide: enough for any split-K the tuner may pick (capped)
static size_t gemm_workspace(int M, int N, int K, int act) {
  if (act == 1 || (K + 63) / 64 < 8) return 0;
  size_t per = (size_t)M * N * sizeof(float);
  int sk = 32;
  while (sk > 1 && ((size_t)sk * per > TF_SPLITK_WS_CAP || (K + 63) / 64 / sk < 4)) sk >>= 1;
  return sk > 1 ? (size_t)sk * per : 0;
}

// test hook: force a tile configuration (0 = heuristic)
static int g_force_bm = 0, g_force_bn = 0, g_force_split = 0;

extern "C" {

int tf_gemm_debug(int flags) {
#ifdef TF_ABLATION
  g_dbg = (flags & 7) | ((flags & 4096) ? 8 : 0);         // 1 no stores, 2 no MFMA, 4 no staging, 4096 no fragment reads (k_igemm_pp): the ablation library only
#else
  TF_REQUIRE(!(flags & (7 | 4096)), "tf_gemm_debug: the ablation bits (1, 2, 4, 4096) exist only in the library built with -DTF_ABLATION (python -m tinyfusers_amd.build --ablation)");
#endif
  g_pp_np = (flags & 8192) ? 2 : 0;                       // 8192: k_igemm_pp with one phase per k-step even where the 3-slot ring allows one per K tile
  // the family every launch is asked to run on, where it is eligible; the highest bit set wins
  static const struct { int bit, variant; } force_bits[] = {{32768, V_AR}, {16384, V_C8}, {2048, V_PP3}, {1024, V_C4}, {512, V_PP}, {256, V_ALL8}, {128, V_PATCH}, {16, V_WIDE}, {8, V_RING}};
  g_force_variant = -1;
  for (const auto& fb : force_bits)
    if (flags & fb.bit) { g_force_variant = fb.variant; break; }
  g_force_order = (flags & 64) ? 1 : (flags & 32) ? 0 : -1;
  return TF_OK;
}
// element type of the split-K partial slabs: 16 = fp16 (default; half the bytes of the split-K seam, fp32 accumulation in the reducer), 32 = fp32
int tf_gemm_splitk_partials(int bits) {
  TF_REQUIRE(bits == 16 || bits == 32, "tf_gemm_splitk_partials: bits=%d (16 or 32)", bits);
  g_part16 = bits == 16;
  return TF_OK;
}
// layout of the split-K partial slabs of the launches k_splitk_reduce_gn_apply finishes: 1 = group-major (default), 0 = row-major like every other launch
int tf_gemm_splitk_slab_layout(int group_major) {
  TF_REQUIRE(group_major == 0 || group_major == 1, "tf_gemm_splitk_slab_layout: group_major=%d (0 or 1)", group_major);
  g_slab_gm = group_major;
  return TF_OK;
}
int tf_gemm_force_config(int bm, int bn, int splitk) { g_force_bm = bm; g_force_bn = bn; g_force_split = splitk; return TF_OK; }

// ---- launch descriptors: a conv / linear entry gets its GemmP from one of the two builders below (linear_problem, conv_problem) and then sets
// the fields that are its own.  The host-only predicates and the *_workspace sizes go through the same geometry (linear_shape, conv_shape).
enum Elem { EL_16, EL_E4M3, EL_MX };   // what x / x2 / w hold: 16-bit elements (GemmP::bf16 says which), e4m3 with one scale per weight row, e4m3 with block-scaled activations
static long long elem_bytes(Elem e, long long n) { return e == EL_16 ? 2 * n : n; }
static bool under_2gib(Elem e, long long bytes) { return bytes + (e == EL_MX ? bytes / 32 : 0) < (1LL << 31); }   // (a block-scaled tensor carries its scale bytes behind its codes)

// a Linear is a 1x1 conv over an M x 1 image; N = the output width (the weight has twice as many rows for GEGLU)
static void linear_shape(GemmP& p, Elem e, int M, int N, int K, int act) {
  p = {};
  p.fp8 = e != EL_16; p.mx = e == EL_MX;
  p.M = M; p.N = act == 1 ? 2 * N : N; p.K = K; p.Kc = K; p.C1 = K; p.C2 = 0; p.C = K;
  p.H = 1; p.W = M; p.Ho = 1; p.Wo = M; p.HoWo = M; p.S = 1; p.stride = 1; p.pad = 0; p.ups = 0; p.act = act;
}
// The checks every linear entry makes, under the name `fn` it makes them with, and its descriptor.  M == 0 is TF_OK with nothing to launch: the
// caller returns `if (rc || M == 0)`.  K is a multiple of 8 for 16-bit operands and of 64 for e4m3.
static int linear_problem(GemmP& p, const char* fn, Elem e, void* y, const void* x, const void* w, const void* bias, const void* residual, int M, int N, int K, int act) {
  const int kq = e == EL_16 ? 8 : 64;
  TF_REQUIRE(y && x && w, "%s: null tensor", fn);
  TF_REQUIRE(M >= 0 && N >= 1 && K >= kq && K % kq == 0, "%s: K=%d must be a positive multiple of %d", fn, K, kq);
  TF_REQUIRE(act == 0 || act == 1, "%s: act=%d", fn, act);
  TF_REQUIRE(act == 0 || (bias && N % 16 == 0), "%s: GEGLU needs a bias and N %% 16 == 0 (N=%d)", fn, N);
  if (M == 0) return TF_OK;
  linear_shape(p, e, M, N, K, act);
  p.x = (const half_t*)x; p.w = (const half_t*)w; p.y = (half_t*)y; p.bias = (const half_t*)bias; p.residual = (const half_t*)residual;
  const long long xb = elem_bytes(e, (long long)M * K), wb = elem_bytes(e, (long long)p.N * K);
  TF_REQUIRE(under_2gib(e, xb) && wb < (1LL << 31), "%s: tensors must be < 2 GiB each", fn);
  p.x_bytes = p.x2_bytes = p.x3_bytes = p.x4_bytes = (unsigned)xb; p.w_bytes = (unsigned)wb;   // (a source that is not there has the size of x)
  return TF_OK;
}

struct ConvShape { int N, H, W, C1, C2, Cout, R, S, stride, pad, upsample, C3, C4; };
// the implicit GEMM of a conv: M = output pixels, K = the R*S taps of the concat (x | x2), then the channels of the extra 1x1 sources x3 | x4.
// 0 = filled, 1 = no output pixel (or no stride), 2 = M or K beyond 32-bit indexing
static int conv_shape(GemmP& p, Elem e, const ConvShape& g) {
  p = {};
  if (g.stride < 1) return 1;
  const int ups = g.upsample ? 1 : 0;
  const int Ho = ((g.H << ups) + 2 * g.pad - g.R) / g.stride + 1, Wo = ((g.W << ups) + 2 * g.pad - g.S) / g.stride + 1;
  if (Ho <= 0 || Wo <= 0) return 1;
  if ((long long)g.N * Ho * Wo >= (1LL << 31) || (long long)g.R * g.S * (g.C1 + g.C2) >= (1LL << 31)) return 2;
  p.fp8 = e != EL_16; p.mx = e == EL_MX;
  p.M = g.N * Ho * Wo; p.N = g.Cout; p.C1 = g.C1; p.C2 = g.C2; p.C = g.C1 + g.C2; p.Kc = g.R * g.S * p.C; p.K = p.Kc + g.C3 + g.C4; p.C3 = g.C3; p.C4 = g.C4;
  p.H = g.H; p.W = g.W; p.Ho = Ho; p.Wo = Wo; p.HoWo = Ho * Wo; p.S = g.S; p.stride = g.stride; p.pad = g.pad; p.ups = ups; p.act = 0;
  return 0;
}
// The checks every conv entry makes and its descriptor; N == 0 is TF_OK with nothing to launch: the caller returns `if (rc || N == 0)`.  `fn` is
// tf_conv2d_f16 for every 16-bit entry (the messages about the extra sources say tf_conv2d_fused_f16, the entry that introduced them); channel
// counts are multiples of 8 for 16-bit operands and of 64 for e4m3.
static int conv_problem(GemmP& p, const char* fn, Elem e, const ConvShape& g, void* y, const void* x, const void* x2, const void* x3, const void* x4, const void* w,
                        const void* bias, const void* bias_nc, long long bias_nc_stride, const void* residual) {
  const int cq = e == EL_16 ? 8 : 64;
  TF_REQUIRE(g.C3 >= 0 && g.C4 >= 0 && (g.C3 == 0 || x3) && (g.C4 == 0 || (x4 && g.C3 > 0)) && g.C3 % 8 == 0 && g.C4 % 8 == 0,
             "tf_conv2d_fused_f16: extra sources C3=%d C4=%d must be multiples of 8 with their tensors given (x4 needs x3)", g.C3, g.C4);
  TF_REQUIRE(g.C3 == 0 || g.upsample == 0, "tf_conv2d_fused_f16: the extra 1x1 sources cannot be combined with upsample");
  TF_REQUIRE(y && x && w, "%s: null tensor", fn);
  TF_REQUIRE(g.C1 > 0 && g.C2 >= 0 && (g.C2 == 0 || x2), "%s: C1=%d C2=%d x2=%p", fn, g.C1, g.C2, x2);
  TF_REQUIRE(g.C1 % cq == 0 && g.C2 % cq == 0, "%s: channel counts must be multiples of %d (C1=%d C2=%d)%s", fn, cq, g.C1, g.C2, e == EL_16 ? "; use tf_im2col_nhwc_f16 for tiny C" : "");
  TF_REQUIRE(g.R >= 1 && g.S >= 1 && g.stride >= 1 && g.pad >= 0 && g.Cout >= 1 && g.N >= 0, "%s: bad geometry R=%d S=%d stride=%d pad=%d", fn, g.R, g.S, g.stride, g.pad);
  const int bad = conv_shape(p, e, g);
  TF_REQUIRE(bad != 1, "%s: empty output for H=%d W=%d", fn, g.H, g.W);
  if (g.N == 0) return TF_OK;
  TF_REQUIRE(bad != 2, "%s: problem too large for 32-bit indexing", fn);
  TF_REQUIRE(bias_nc_stride % 4 == 0 || g.Cout % 4 != 0, "%s: bias_nc_stride must be a multiple of 4", fn);
  p.x = (const half_t*)x; p.x2 = (const half_t*)x2; p.x3 = (const half_t*)x3; p.x4 = (const half_t*)x4; p.w = (const half_t*)w; p.y = (half_t*)y;
  p.bias = (const half_t*)bias; p.bias_nc = (const half_t*)bias_nc; p.residual = (const half_t*)residual; p.bias_nc_stride = bias_nc_stride;
  const long long px = (long long)g.N * g.H * g.W, xb = elem_bytes(e, px * g.C1), x2b = elem_bytes(e, px * g.C2), wb = elem_bytes(e, (long long)g.Cout * p.K);
  const long long x3b = elem_bytes(e, px * g.C3), x4b = elem_bytes(e, px * g.C4);
  TF_REQUIRE(under_2gib(e, xb) && under_2gib(e, x2b) && wb < (1LL << 31), "%s: tensors must be < 2 GiB each", fn);
  TF_REQUIRE(x3b < (1LL << 31) && x4b < (1LL << 31), "tf_conv2d_fused_f16: tensors must be < 2 GiB each");
  p.x_bytes = (unsigned)xb; p.w_bytes = (unsigned)wb;                                          // (of a block-scaled tensor: the codes; the scale bytes sit behind them)
  // a source that is not there has the size of x
  p.x2_bytes = g.C2 ? (unsigned)x2b : (unsigned)xb; p.x3_bytes = g.C3 ? (unsigned)x3b : (unsigned)xb; p.x4_bytes = g.C4 ? (unsigned)x4b : (unsigned)xb;
  return TF_OK;
}
// GroupNorm statistics of the output, where the caller gave a buffer for them: requested only for a group width the epilogue can fold (a group
// spans at most two n-tiles, one lane per group of a tile); anything else simply reports chunks = 0 and the caller runs tf_group_norm_f16 as usual
static int conv_output_stats(GemmP& p, const char* fn, int N, void* gn_partial, size_t gn_partial_bytes, int gn_groups) {
  if (!gn_partial) return TF_OK;
  TF_REQUIRE(gn_groups >= 1 && p.N % gn_groups == 0, "%s: Cout=%d not divisible by groups=%d", fn, p.N, gn_groups);
  TF_REQUIRE(gn_partial_bytes >= tf_conv2d_gn_partial_bytes(N, gn_groups), "%s: statistics buffer too small (%zu bytes)", fn, gn_partial_bytes);
  const int cpg = p.N / gn_groups;
  if (cpg >= 4 && cpg <= 64 && p.N % 8 == 0 && p.N <= 4096 && gn_groups <= 256) { p.gn_part = (float*)gn_partial; p.gn_G = gn_groups; p.gn_cpg = cpg; }
  return TF_OK;
}
static int run_forced(const GemmP& p, void* workspace, size_t workspace_bytes, tfStream_t s, int* gn_chunks = nullptr) {   // run_gemm under tf_gemm_force_config
  return run_gemm(p, workspace, workspace_bytes, g_force_bm, g_force_bn, g_force_split, tf_hs(s), gn_chunks);
}

size_t tf_conv2d_gn_partial_bytes(int N, int groups) { return (size_t)(N > 0 ? N : 0) * TF_GN_MAX_CHUNKS * (groups > 0 ? groups : 0) * 2 * sizeof(float); }

size_t tf_conv2d_fused_workspace(int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample, int C3, int C4) {
  GemmP p;
  return conv_shape(p, EL_16, {N, H, W, C1, C2, Cout, R, S, stride, pad, upsample, C3, C4}) ? 0 : gemm_workspace(p.M, p.N, p.K, 0);
}
size_t tf_conv2d_workspace(int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample) {
  return tf_conv2d_fused_workspace(N, H, W, C1, C2, Cout, R, S, stride, pad, upsample, 0, 0);
}

#define TF_REQUIRE_DTYPE(fn) TF_REQUIRE(dtype == TF_DTYPE_F16 || dtype == TF_DTYPE_BF16, fn ": dtype=%d (0 = float16, 1 = bfloat16)", dtype)
int tf_conv2d_fused_16(int dtype, void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc, long long bias_nc_stride,
                       const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample,
                       void* workspace, size_t workspace_bytes, const void* x3, const void* x4, int C3, int C4, void* gn_partial,
                       size_t gn_partial_bytes, int gn_groups, int* gn_chunks, tfStream_t s) {
  TF_REQUIRE_DTYPE("tf_conv2d_fused_16");
  TF_REQUIRE(!gn_partial || gn_chunks, "tf_conv2d_fused_f16: gn_chunks must be given with gn_partial");
  if (gn_chunks) *gn_chunks = 0;
  GemmP p;
  int rc = conv_problem(p, "tf_conv2d_f16", EL_16, {N, H, W, C1, C2, Cout, R, S, stride, pad, upsample, C3, C4}, y, x, x2, x3, x4, w, bias, bias_nc, bias_nc_stride, residual);
  if (rc || N == 0) return rc;
  p.bf16 = dtype == TF_DTYPE_BF16;
  if ((rc = conv_output_stats(p, "tf_conv2d_fused_f16", N, gn_partial, gn_partial_bytes, gn_groups))) return rc;
  return run_forced(p, workspace, workspace_bytes, s, gn_chunks);
}
int tf_conv2d_fused_f16(void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc, long long bias_nc_stride,
                        const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample,
                        void* workspace, size_t workspace_bytes, const void* x3, const void* x4, int C3, int C4, void* gn_partial,
                        size_t gn_partial_bytes, int gn_groups, int* gn_chunks, tfStream_t s) {
  return tf_conv2d_fused_16(TF_DTYPE_F16, y, x, x2, w, bias, bias_nc, bias_nc_stride, residual, N, H, W, C1, C2, Cout, R, S, stride, pad, upsample, workspace, workspace_bytes, x3, x4, C3, C4,
                            gn_partial, gn_partial_bytes, gn_groups, gn_chunks, s);
}
int tf_conv2d_f16(void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc, long long bias_nc_stride,
                  const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample,
                  void* workspace, size_t workspace_bytes, tfStream_t s) {
  return tf_conv2d_fused_16(TF_DTYPE_F16, y, x, x2, w, bias, bias_nc, bias_nc_stride, residual, N, H, W, C1, C2, Cout, R, S, stride, pad, upsample, workspace, workspace_bytes,
                            nullptr, nullptr, 0, 0, nullptr, 0, 0, nullptr, s);
}

int tf_conv2d_fused_norm_16(int dtype, void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc, long long bias_nc_stride,
                            const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample,
                            void* workspace, size_t workspace_bytes, const void* x3, const void* x4, int C3, int C4, void* gn_partial,
                            size_t gn_partial_bytes, int gn_groups, int* gn_chunks, void* z, const void* z_gamma, const void* z_beta, float z_eps,
                            int z_silu, int* z_written, tfStream_t s) {
  TF_REQUIRE_DTYPE("tf_conv2d_fused_norm_16");
  TF_REQUIRE(gn_partial && gn_chunks && z && z_written, "tf_conv2d_fused_norm_f16: gn_partial, gn_chunks, z and z_written must be given");
  TF_REQUIRE((z_gamma == nullptr) == (z_beta == nullptr), "tf_conv2d_fused_norm_f16: gamma and beta must both be given or both NULL");
  *z_written = 0; *gn_chunks = 0;
  GemmP p;
  int rc = conv_problem(p, "tf_conv2d_f16", EL_16, {N, H, W, C1, C2, Cout, R, S, stride, pad, upsample, C3, C4}, y, x, x2, x3, x4, w, bias, bias_nc, bias_nc_stride, residual);
  if (rc || N == 0) return rc;
  p.bf16 = dtype == TF_DTYPE_BF16;
  if ((rc = conv_output_stats(p, "tf_conv2d_fused_f16", N, gn_partial, gn_partial_bytes, gn_groups))) return rc;
  if (p.gn_part) {                                          // (groups the epilogue cannot fold: no statistics, no apply -- *z_written stays 0)
    p.on_z = (half_t*)z; p.on_gamma = (const half_t*)z_gamma; p.on_beta = (const half_t*)z_beta; p.on_eps = z_eps; p.on_silu = z_silu ? 1 : 0; p.on_applied = z_written;
  }
  return run_forced(p, workspace, workspace_bytes, s, gn_chunks);
}
int tf_conv2d_fused_norm_f16(void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc, long long bias_nc_stride,
                             const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample,
                             void* workspace, size_t workspace_bytes, const void* x3, const void* x4, int C3, int C4, void* gn_partial,
                             size_t gn_partial_bytes, int gn_groups, int* gn_chunks, void* z, const void* z_gamma, const void* z_beta, float z_eps,
                             int z_silu, int* z_written, tfStream_t s) {
  return tf_conv2d_fused_norm_16(TF_DTYPE_F16, y, x, x2, w, bias, bias_nc, bias_nc_stride, residual, N, H, W, C1, C2, Cout, R, S, stride, pad, upsample, workspace, workspace_bytes,
                                 x3, x4, C3, C4, gn_partial, gn_partial_bytes, gn_groups, gn_chunks, z, z_gamma, z_beta, z_eps, z_silu, z_written, s);
}

int tf_conv2d_gn_supported(int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample, int C3, int C4, int in_groups) {
  if (N < 1 || C1 < 1 || C2 < 0 || Cout < 1 || R != S || stride < 1 || in_groups < 1 || (C1 + C2) % in_groups) return 0;
  GemmP p;
  if (conv_shape(p, EL_16, {N, H, W, C1, C2, Cout, R, S, stride, pad, upsample, C3, C4})) return 0;
  static float dummy;
  p.gi_part = &dummy; p.gi_G = in_groups;
  return gi_any_ok(p) ? 1 : 0;
}

int tf_conv2d_patch_admits(int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample, int C3, int C4, int bm, int bn) {
  if (N < 1 || C1 < 1 || C2 < 0 || C3 < 0 || C4 < 0 || Cout < 1 || R != S) return 0;
  GemmP p;
  if (conv_shape(p, EL_16, {N, H, W, C1, C2, Cout, R, S, stride, pad, upsample, C3, C4})) return 0;
  return patch_admits(p, bm, bn) ? 1 : 0;
}

int tf_gemm_ring_form(int bm, int bn, int variant, int channels_on_64_grid) {
  TF_REQUIRE(((bm == 64 || bm == 128) && (bn == 64 || bn == 128 || bn == 160)) || (bm == 256 && bn == 128), "tf_gemm_ring_form: k_igemm has no %dx%d tile", bm, bn);
  TF_REQUIRE(variant == V_RING || variant == V_WIDE || variant == V_ALL8, "tf_gemm_ring_form: variant=%d is not a k_igemm form (0, 1, 3)", variant);
  return igemm_ring_form(bm, bn, variant == V_WIDE, variant == V_ALL8, !channels_on_64_grid);
}

int tf_conv2d_gn_16(int dtype, void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc, long long bias_nc_stride,
                    const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample,
                    void* workspace, size_t workspace_bytes, const void* x3, const void* x4, int C3, int C4, void* gn_partial,
                    size_t gn_partial_bytes, int gn_groups, int* gn_chunks, const void* in_gamma, const void* in_beta, const void* in_partial,
                    int in_chunks, int in_groups1, const void* in_partial2, int in_chunks2, int in_groups2, int in_groups, float in_eps, int in_silu,
                    tfStream_t s) {
  TF_REQUIRE_DTYPE("tf_conv2d_gn_16");
  TF_REQUIRE(!gn_partial || gn_chunks, "tf_conv2d_gn_f16: gn_chunks must be given with gn_partial");
  TF_REQUIRE(in_partial && in_chunks >= 1 && in_chunks <= 4096 && in_groups >= 1 && (C1 + C2) % in_groups == 0, "tf_conv2d_gn_f16: input statistics missing (chunks=%d groups=%d)", in_chunks, in_groups);
  TF_REQUIRE((in_gamma == nullptr) == (in_beta == nullptr), "tf_conv2d_gn_f16: gamma and beta must both be given or both NULL");
  int mr = 1;
  if (in_partial2) {
    // concat (x, x2) whose statistics came with its two sources: partials of G1 sub-groups of x and G2 of x2, all of one width,
    // mr adjacent sub-groups of the list [x's | x2's] form a group of the concat (tf_group_norm_apply_cat_f16's contract)
    TF_REQUIRE(C2 > 0 && in_groups1 >= 1 && in_groups2 >= 1 && C1 % in_groups1 == 0 && C2 % in_groups2 == 0 && in_chunks2 >= 1 && in_chunks2 <= 4096,
               "tf_conv2d_gn_f16: C1=%d C2=%d groups1=%d groups2=%d chunks2=%d", C1, C2, in_groups1, in_groups2, in_chunks2);
    const int sub = C1 / in_groups1, cpg = (C1 + C2) / in_groups;
    TF_REQUIRE(C2 / in_groups2 == sub && cpg % sub == 0 && cpg / sub <= 8, "tf_conv2d_gn_f16: the partials' sub-groups (%d and %d channels) do not tile the %d-channel groups", sub, C2 / in_groups2, cpg);
    mr = cpg / sub;
  }
  if (gn_chunks) *gn_chunks = 0;
  GemmP p;
  int rc = conv_problem(p, "tf_conv2d_f16", EL_16, {N, H, W, C1, C2, Cout, R, S, stride, pad, upsample, C3, C4}, y, x, x2, x3, x4, w, bias, bias_nc, bias_nc_stride, residual);
  if (rc || N == 0) return rc;
  p.bf16 = dtype == TF_DTYPE_BF16;
  if ((rc = conv_output_stats(p, "tf_conv2d_fused_f16", N, gn_partial, gn_partial_bytes, gn_groups))) return rc;
  p.gi_part = (const float*)in_partial; p.gi_gamma = (const half_t*)in_gamma; p.gi_beta = (const half_t*)in_beta;
  p.gi_chunks = in_chunks; p.gi_G = in_groups; p.gi_G1 = in_groups; p.gi_mr = mr; p.gi_eps = in_eps; p.gi_silu = in_silu ? 1 : 0;
  if (in_partial2) { p.gi_part2 = (const float*)in_partial2; p.gi_chunks2 = in_chunks2; p.gi_G1 = in_groups1; p.gi_G2 = in_groups2; }
  p.ktiles = (p.K + 63) / 64;
  if (!gi_any_ok(p)) { tf_set_error("tf_conv2d_gn_f16: this geometry cannot carry the input GroupNorm (ask tf_conv2d_gn_supported first)"); return TF_E_UNSUPPORTED; }
  return run_forced(p, workspace, workspace_bytes, s, gn_chunks);
}
int tf_conv2d_gn_f16(void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc, long long bias_nc_stride,
                     const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample,
                     void* workspace, size_t workspace_bytes, const void* x3, const void* x4, int C3, int C4, void* gn_partial,
                     size_t gn_partial_bytes, int gn_groups, int* gn_chunks, const void* in_gamma, const void* in_beta, const void* in_partial,
                     int in_chunks, int in_groups1, const void* in_partial2, int in_chunks2, int in_groups2, int in_groups, float in_eps, int in_silu,
                     tfStream_t s) {
  return tf_conv2d_gn_16(TF_DTYPE_F16, y, x, x2, w, bias, bias_nc, bias_nc_stride, residual, N, H, W, C1, C2, Cout, R, S, stride, pad, upsample, workspace, workspace_bytes, x3, x4, C3, C4,
                         gn_partial, gn_partial_bytes, gn_groups, gn_chunks, in_gamma, in_beta, in_partial, in_chunks, in_groups1, in_partial2, in_chunks2, in_groups2, in_groups, in_eps,
                         in_silu, s);
}

size_t tf_linear_workspace(int M, int N, int K, int act) { return gemm_workspace(M, act == 1 ? 2 * N : N, K, act); }

// tf_linear_16 under the name its messages carry.  heed_force = false: tf_gemm_force_config does not reach this launch (the _bf16-only entries)
static int linear_16(const char* fn, int dtype, void* y, const void* x, const void* w, const void* bias, const void* residual, int M, int N, int K, int act,
                     void* workspace, size_t workspace_bytes, bool heed_force, tfStream_t s) {
  GemmP p;
  int rc = linear_problem(p, fn, EL_16, y, x, w, bias, residual, M, N, K, act);
  if (rc || M == 0) return rc;
  p.bf16 = dtype == TF_DTYPE_BF16;
  return heed_force ? run_forced(p, workspace, workspace_bytes, s) : run_gemm(p, workspace, workspace_bytes, 0, 0, 0, tf_hs(s));
}
int tf_linear_16(int dtype, void* y, const void* x, const void* w, const void* bias, const void* residual, int M, int N, int K, int act,
                 void* workspace, size_t workspace_bytes, tfStream_t s) {
  TF_REQUIRE_DTYPE("tf_linear_16");
  return linear_16("tf_linear_f16", dtype, y, x, w, bias, residual, M, N, K, act, workspace, workspace_bytes, true, s);
}
int tf_linear_f16(void* y, const void* x, const void* w, const void* bias, const void* residual, int M, int N, int K, int act,
                  void* workspace, size_t workspace_bytes, tfStream_t s) {
  return tf_linear_16(TF_DTYPE_F16, y, x, w, bias, residual, M, N, K, act, workspace, workspace_bytes, s);
}

// scores of the unfused attention path (attention/sdpa.py:66 of the reference: cp.matmul(q, k^T) in fp32): y32[m, n] = sum_k x[m, k] w[n, k],
// fp16 operands, fp32 accumulators stored as they are
int tf_linear_f32out_f16(void* y_f32, const void* x, const void* w, int M, int N, int K, tfStream_t s) {
  GemmP p;
  int rc = linear_problem(p, "tf_linear_f32out_f16", EL_16, y_f32, x, w, nullptr, nullptr, M, N, K, 0);
  if (rc || M == 0) return rc;
  p.out32 = (float*)y_f32;
  return run_gemm(p, nullptr, 0, g_force_bm, g_force_bn, g_force_split > 1 ? 1 : g_force_split, tf_hs(s));   // no workspace: a forced split is clamped to 1
}

// ---- bfloat16 entries: the reference's op tests parametrise bfloat16 next to float16 (tests/linear.py:13, tests/layer_norm.py:13,
// tests/group_norm.py:12) -- the tagged entries with TF_DTYPE_BF16, without a workspace (so never split along K); the two linears are also out
// of tf_gemm_force_config's reach ----------------
int tf_linear_bf16(void* y, const void* x, const void* w, const void* bias, const void* residual, int M, int N, int K, tfStream_t s) {
  return linear_16("tf_linear_bf16", TF_DTYPE_BF16, y, x, w, bias, residual, M, N, K, 0, nullptr, 0, false, s);
}
// ... with the GEGLU epilogue (act = 1: w / bias packed in 16-row value | gate blocks as for tf_linear_f16; N = the output width): ff/nn.py:5-12 on bfloat16
int tf_linear_act_bf16(void* y, const void* x, const void* w, const void* bias, const void* residual, int M, int N, int K, int act, tfStream_t s) {
  return linear_16("tf_linear_act_bf16", TF_DTYPE_BF16, y, x, w, bias, residual, M, N, K, act, nullptr, 0, false, s);
}
int tf_conv2d_bf16(void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc, long long bias_nc_stride,
                   const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample, tfStream_t s) {
  return tf_conv2d_fused_16(TF_DTYPE_BF16, y, x, x2, w, bias, bias_nc, bias_nc_stride, residual, N, H, W, C1, C2, Cout, R, S, stride, pad, upsample, nullptr, 0,
                            nullptr, nullptr, 0, 0, nullptr, 0, 0, nullptr, s);
}

// ---- fp8 entries (config 5) ---------------------------------------------------------------------------------------------------
int tf_quantize_fp8_f16(void* y8, const void* x, long long n, float scale, tfStream_t s) {
  TF_REQUIRE(y8 && x && n >= 0 && n % 8 == 0, "tf_quantize_fp8_f16: n=%lld must be a multiple of 8", n);
  if (n == 0) return TF_OK;
  long long n8 = n / 8, grid = (n8 + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(k_quantize_fp8, dim3((unsigned)grid), dim3(256), 0, tf_hs(s), (unsigned char*)y8, (const half_t*)x, scale, n8);
  TF_LAUNCH_CHECK();
  return TF_OK;
}
int tf_pack_weight_fp8(void* w8, void* scale_f32, const void* w, int N, int K, tfStream_t s) {
  TF_REQUIRE(w8 && scale_f32 && w && N >= 1 && K >= 8 && K % 8 == 0, "tf_pack_weight_fp8: N=%d K=%d (K must be a multiple of 8)", N, K);
  hipLaunchKernelGGL(k_pack_weight_fp8, dim3(ceil_div(N, 4)), dim3(256), 0, tf_hs(s), (unsigned char*)w8, (float*)scale_f32, (const half_t*)w, N, K);
  TF_LAUNCH_CHECK();
  return TF_OK;
}
size_t tf_conv2d_fp8_workspace(int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample) {
  return tf_conv2d_workspace(N, H, W, C1, C2, Cout, R, S, stride, pad, upsample);
}
int tf_conv2d_fp8(void* y, const void* x8, const void* x28, const void* w8, const void* wscale, const void* bias, const void* bias_nc,
                  long long bias_nc_stride, const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad,
                  int upsample, void* workspace, size_t workspace_bytes, void* gn_partial, size_t gn_partial_bytes, int gn_groups, int* gn_chunks,
                  tfStream_t s) {
  if (gn_chunks) *gn_chunks = 0;
  TF_REQUIRE(wscale, "tf_conv2d_fp8: null tensor");
  TF_REQUIRE(R == S, "tf_conv2d_fp8: bad geometry R=%d S=%d stride=%d pad=%d", R, S, stride, pad);
  TF_REQUIRE(!gn_partial || gn_chunks, "tf_conv2d_fp8: gn_chunks must be given with gn_partial");
  GemmP p;
  int rc = conv_problem(p, "tf_conv2d_fp8", EL_E4M3, {N, H, W, C1, C2, Cout, R, S, stride, pad, upsample, 0, 0}, y, x8, x28, nullptr, nullptr, w8, bias, bias_nc, bias_nc_stride, residual);
  if (rc || N == 0) return rc;
  p.wscale = (const float*)wscale;
  if ((rc = conv_output_stats(p, "tf_conv2d_fp8", N, gn_partial, gn_partial_bytes, gn_groups))) return rc;
  return run_forced(p, workspace, workspace_bytes, s, gn_chunks);
}
int tf_linear_fp8(void* y, const void* x8, const void* w8, const void* wscale, const void* bias, const void* residual, int M, int N, int K, int act,
                  int out_fp8, void* workspace, size_t workspace_bytes, tfStream_t s) {
  TF_REQUIRE(wscale, "tf_linear_fp8: null tensor");
  TF_REQUIRE(!out_fp8 || N % 8 == 0, "tf_linear_fp8: an e4m3 output needs N %% 8 == 0 (N=%d)", N);
  GemmP p;
  int rc = linear_problem(p, "tf_linear_fp8", EL_E4M3, y, x8, w8, bias, residual, M, N, K, act);
  if (rc || M == 0) return rc;
  p.wscale = (const float*)wscale; p.out8 = out_fp8 ? 1 : 0;
  if (p.out8) workspace = nullptr, workspace_bytes = 0;   // the split-K reduce writes fp16: an e4m3 output runs unsplit
  return run_forced(p, workspace, workspace_bytes, s);
}

// ---- block-scaled e4m3 activations (round 4): one E8M0 scale per 32 consecutive channels of a pixel / token, fed to the scale operand of
// v_mfma_scale_f32_16x16x128_f8f6f4.  An "mx8" tensor is ONE buffer: rows x C codes, then rows x C/32 scale bytes (tf_mx8_bytes).
size_t tf_mx8_bytes(long long rows, int C) { return rows > 0 && C > 0 ? (size_t)rows * C + (size_t)rows * (C / 32) : 0; }
int tf_quantize_mx8_f16(void* y_mx, const void* x, long long rows, int C, tfStream_t s) {
  TF_REQUIRE(y_mx && x && rows >= 0 && C > 0 && C % 32 == 0, "tf_quantize_mx8_f16: C=%d must be a positive multiple of 32", C);
  if (rows == 0) return TF_OK;
  long long n8 = rows * (C / 8), grid = (n8 + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(k_quantize_mx8, dim3((unsigned)grid), dim3(256), 0, tf_hs(s), (unsigned char*)y_mx, (const half_t*)x, rows, C);
  TF_LAUNCH_CHECK();
  return TF_OK;
}
// does the block-scaled kernel take a GEMM of M rows (pixels / tokens) x N outputs x K?  It is the ping-pong kernel: launches that fill the chip
// with its 192- / 256-row tiles (BASELINE config 5's regime); stride-1 convolutions without up-sampling and linears; callers keep fp16 otherwise
static bool mx_shape_ok(const GemmP& p) {
  if (p.M <= 256 || p.K % 64 || p.N % 8) return false;
  TunedCfg d = mx_default(p);
  if (!d.c.bm) return false;
  static const int cand[][2] = {{192, 160}, {192, 128}, {256, 128}, {256, 160}};
  for (int ci = 0; ci < 4; ++ci)
    if (pp_ok(p, cand[ci][1], cand[ci][0]) && (long long)((p.M + cand[ci][0] - 1) / cand[ci][0]) * ((p.N + cand[ci][1] - 1) / cand[ci][1]) >= 128) return true;
  return false;
}
int tf_mx8_gemm_supported(int M, int N, int K, int act, int out_mx) {
  if (M < 1 || N < 1 || K < 64) return 0;
  GemmP p;
  linear_shape(p, EL_MX, M, N, K, act);
  p.out8 = out_mx ? 1 : 0;
  return mx_shape_ok(p) ? 1 : 0;
}
int tf_mx8_conv_supported(int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample) {
  if (N < 1 || C1 < 64 || C2 < 0 || R != S || stride != 1 || upsample || (C1 % 64) || (C2 % 64)) return 0;
  GemmP p;
  if (conv_shape(p, EL_MX, {N, H, W, C1, C2, Cout, R, S, 1, pad, 0, 0, 0})) return 0;
  p.bias_nc = (const half_t*)&p;                            // (the ResBlock convs carry a time-embedding bias: the stricter tile rule)
  return mx_shape_ok(p) ? 1 : 0;
}
int tf_conv2d_mx8(void* y, const void* x_mx, const void* x2_mx, const void* w8, const void* wscale, const void* bias, const void* bias_nc,
                  long long bias_nc_stride, const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad,
                  void* workspace, size_t workspace_bytes, void* gn_partial, size_t gn_partial_bytes, int gn_groups, int* gn_chunks, tfStream_t s) {
  if (gn_chunks) *gn_chunks = 0;
  TF_REQUIRE(wscale, "tf_conv2d_mx8: null tensor");
  TF_REQUIRE(R == S && stride == 1, "tf_conv2d_mx8: stride-1 square filters only (R=%d S=%d stride=%d pad=%d)", R, S, stride, pad);
  TF_REQUIRE(!gn_partial || gn_chunks, "tf_conv2d_mx8: gn_chunks must be given with gn_partial");
  GemmP p;
  int rc = conv_problem(p, "tf_conv2d_mx8", EL_MX, {N, H, W, C1, C2, Cout, R, S, 1, pad, 0, 0, 0}, y, x_mx, x2_mx, nullptr, nullptr, w8, bias, bias_nc, bias_nc_stride, residual);
  if (rc || N == 0) return rc;
  p.wscale = (const float*)wscale;
  if ((rc = conv_output_stats(p, "tf_conv2d_mx8", N, gn_partial, gn_partial_bytes, gn_groups))) return rc;
  return run_forced(p, workspace, workspace_bytes, s, gn_chunks);
}
int tf_linear_mx8(void* y, const void* x_mx, const void* w8, const void* wscale, const void* bias, const void* residual, int M, int N, int K, int act,
                  int out_mx, void* workspace, size_t workspace_bytes, tfStream_t s) {
  TF_REQUIRE(wscale, "tf_linear_mx8: null tensor");
  TF_REQUIRE(!out_mx || (act == 1 && N % 32 == 0 && !residual), "tf_linear_mx8: a block-scaled output is the GEGLU epilogue's (act = 1, N %% 32 == 0, no residual; N=%d)", N);
  GemmP p;
  int rc = linear_problem(p, "tf_linear_mx8", EL_MX, y, x_mx, w8, bias, residual, M, N, K, act);
  if (rc || M == 0) return rc;
  p.wscale = (const float*)wscale; p.out8 = out_mx ? 1 : 0;
  if (p.out8) workspace = nullptr, workspace_bytes = 0;   // the split-K reduce writes fp16: an e4m3 output runs unsplit
  return run_forced(p, workspace, workspace_bytes, s);
}

int tf_ln_fold_weights_16(int dtype, void* w_out, void* bias_out, void* colsum_out, const void* w, const void* bias, const void* gamma, const void* beta,
                          int N, int K, tfStream_t s) {
  TF_REQUIRE_DTYPE("tf_ln_fold_weights_16");
  TF_REQUIRE(w_out && bias_out && colsum_out && w && gamma && beta && N >= 1 && K % 8 == 0, "tf_ln_fold_weights_f16: bad arguments (K=%d)", K);
  if (dtype == TF_DTYPE_BF16) hipLaunchKernelGGL(k_ln_fold<true>, dim3(ceil_div(N, 4)), dim3(256), 0, tf_hs(s), (half_t*)w_out, (half_t*)bias_out, (float*)colsum_out, (const half_t*)w,
                                                 (const half_t*)bias, (const half_t*)gamma, (const half_t*)beta, N, K);
  else hipLaunchKernelGGL(k_ln_fold<false>, dim3(ceil_div(N, 4)), dim3(256), 0, tf_hs(s), (half_t*)w_out, (half_t*)bias_out, (float*)colsum_out, (const half_t*)w,
                          (const half_t*)bias, (const half_t*)gamma, (const half_t*)beta, N, K);
  TF_LAUNCH_CHECK();
  return TF_OK;
}
int tf_ln_fold_weights_f16(void* w_out, void* bias_out, void* colsum_out, const void* w, const void* bias, const void* gamma, const void* beta,
                           int N, int K, tfStream_t s) {
  return tf_ln_fold_weights_16(TF_DTYPE_F16, w_out, bias_out, colsum_out, w, bias, gamma, beta, N, K, s);
}

int tf_linear_ln_16(int dtype, void* y, const void* x, const void* w_folded, const void* bias_folded, const void* colsum, const void* residual, int M, int N,
                    int K, int act, float eps, tfStream_t s) {
  TF_REQUIRE_DTYPE("tf_linear_ln_16");
  TF_REQUIRE(bias_folded && colsum, "tf_linear_ln_f16: null tensor");
  TF_REQUIRE(K >= 64 && K % 64 == 0, "tf_linear_ln_f16: K=%d must be a positive multiple of 64", K);
  TF_REQUIRE((act == 1 ? N % 16 == 0 : N % 4 == 0), "tf_linear_ln_f16: N=%d must be a multiple of 4 (16 for GEGLU)", N);
  GemmP p;
  int rc = linear_problem(p, "tf_linear_ln_f16", EL_16, y, x, w_folded, bias_folded, residual, M, N, K, act);
  if (rc || M == 0) return rc;
  p.ln_colsum = (const float*)colsum; p.ln_eps = eps;
  p.bf16 = dtype == TF_DTYPE_BF16;
  return run_forced(p, nullptr, 0, s);                    // (row statistics need the whole K range in one block: never split, no workspace)
}
int tf_linear_ln_f16(void* y, const void* x, const void* w_folded, const void* bias_folded, const void* colsum, const void* residual, int M, int N,
                     int K, int act, float eps, tfStream_t s) {
  return tf_linear_ln_16(TF_DTYPE_F16, y, x, w_folded, bias_folded, colsum, residual, M, N, K, act, eps, s);
}

int tf_gemv_16(int dtype, void* y, const void* x, const void* w, const void* bias, int M, int N, int K, int silu_input, tfStream_t s) {
  TF_REQUIRE_DTYPE("tf_gemv_16");
  TF_REQUIRE(y && x && w && M >= 1 && M <= 8 && N >= 1 && K % 8 == 0, "tf_gemv_f16: needs 1 <= M <= 8 (M=%d) and K %% 8 == 0 (K=%d)", M, K);
  if (dtype == TF_DTYPE_BF16) hipLaunchKernelGGL(k_gemv<true>, dim3(ceil_div(N, 4)), dim3(256), 0, tf_hs(s), (half_t*)y, (const half_t*)x, (const half_t*)w, (const half_t*)bias, M, N, K, silu_input);
  else hipLaunchKernelGGL(k_gemv<false>, dim3(ceil_div(N, 4)), dim3(256), 0, tf_hs(s), (half_t*)y, (const half_t*)x, (const half_t*)w, (const half_t*)bias, M, N, K, silu_input);
  TF_LAUNCH_CHECK();
  return TF_OK;
}
int tf_gemv_f16(void* y, const void* x, const void* w, const void* bias, int M, int N, int K, int silu_input, tfStream_t s) {
  return tf_gemv_16(TF_DTYPE_F16, y, x, w, bias, M, N, K, silu_input, s);
}
int tf_gemv_rows_16(int dtype, void* y, const void* x, const void* w, const void* bias, int M, int N, int K, int silu_input, tfStream_t s) {
  TF_REQUIRE_DTYPE("tf_gemv_rows_16");
  TF_REQUIRE(y && x && w && M >= 1 && M <= (1 << 16) && N >= 1 && K >= 8 && K % 8 == 0, "tf_gemv_rows_16: needs 1 <= M <= 65536 (M=%d), N >= 1 (N=%d) and K a positive multiple of 8 (K=%d)", M, N, K);
  TF_REQUIRE((((uintptr_t)x | (uintptr_t)w) & 15) == 0 && ((uintptr_t)y & 1) == 0, "tf_gemv_rows_16: x and w must be 16-byte aligned");
  const dim3 grid(ceil_div(N, 4), ceil_div(M, 8));
  if (dtype == TF_DTYPE_BF16) hipLaunchKernelGGL(k_gemv<true>, grid, dim3(256), 0, tf_hs(s), (half_t*)y, (const half_t*)x, (const half_t*)w, (const half_t*)bias, M, N, K, silu_input);
  else hipLaunchKernelGGL(k_gemv<false>, grid, dim3(256), 0, tf_hs(s), (half_t*)y, (const half_t*)x, (const half_t*)w, (const half_t*)bias, M, N, K, silu_input);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

}  // extern "C"
