/*
 * tinyfusers_hip.h -- C ABI of libtinyfusers_hip.so, the MI355X (gfx950) native backend that takes the
 * place of the reference's `tinyfusers/native` ctypes layer (libcuda / libcudart / libnvrtc / libcublas
 * bindings, native/cuda/ops.py, native/cublas/ops.py, native/nvrtc/ops.py) and of the cuDNN / CuPy
 * calls the reference's per-op Python surface makes.
 *
 * Conventions (same as the reference's FFI):
 *   - every function returns int, 0 = success, otherwise a hipError_t value or a TF_E_* code; callers
 *     raise RuntimeError("<fn> failed with status N") exactly as storage/device.py:33-37 does.
 *     tf_last_error() additionally returns a thread-local human-readable string.
 *   - plain pointers and sizes only; device memory is caller-owned raw `void*`; opaque handles are
 *     created through an out-pointer and destroyed by the caller; no callbacks; nothing aborts.
 *   - all kernels are asynchronous on the given stream (NULL = the default stream, which is what the
 *     reference always uses: `stream := cuda.CUstream()`), safe to capture into a HIP graph.
 *   - activations are fp16 ("f16"), images in NHWC, tokens in (rows, C) row-major; accumulation fp32.
 *     NCHW fp32 (the reference's layout/dtype) only appears in the layout converters.
 * Each entry cites the reference interface (file:line under /root/reference) it replaces.
 */
#ifndef TINYFUSERS_HIP_H
#define TINYFUSERS_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfStream_st* tfStream_t;
typedef struct tfEvent_st* tfEvent_t;
typedef struct tfGraph_st* tfGraph_t;
typedef struct tfComm_st* tfComm_t;
typedef struct tfFunction_st* tfFunction_t;   /* a kernel compiled at run time (tf_rtc_load) */

#define TF_OK 0
#define TF_E_ARG 10001
#define TF_E_UNSUPPORTED 10002
#define TF_E_WORKSPACE 10003
#define TF_E_STATE 10004

/* cudaMemcpy kinds kept numerically identical to native/cuda/ops.py:95-96 */
#define TF_MEMCPY_H2D 1
#define TF_MEMCPY_D2H 2
#define TF_MEMCPY_D2D 3

/* ---- context / device ------------------------------------------------------------------------ */
/* cuInit + cuCtxCreate_v2 (native/cuda/ops.py:7-18; call site storage/device.py:32-37) */
int tf_init(int device);
int tf_device_count(int* count);
/* cudaDeviceGetAttribute (native/cuda/ops.py:62-66). attr: 0 = CU count, 1 = max clock kHz,
 * 2 = wavefront size, 3 = LDS bytes per workgroup, 4 = L2 bytes, 5 = total memory MiB. */
int tf_device_attr(int* value, int attr, int device);
/* gcn arch name ("gfx950:...") copied into buf */
int tf_device_arch(char* buf, int buflen, int device);

/* ---- run-time compilation: replaces nvrtcCreateProgram / nvrtcCompileProgram / nvrtcGetCUBIN (native/nvrtc/ops.py:3-45) + cuModuleLoadData /
 * cuModuleGetFunction / cuLaunchKernel (native/cuda/ops.py:3-39) as storage/device.py:31-77 and its wrappers :79-233 use them.  hiprtc compiles
 * HIP source for the current device's architecture; a failed compilation returns TF_E_ARG with the compiler's log in tf_last_error().
 * params[i] points at the i-th kernel argument (cuLaunchKernel's kernelParams). */
int tf_rtc_load(tfFunction_t* out_fn, const char* source, const char* func_name);
int tf_rtc_launch(tfFunction_t fn, unsigned gx, unsigned gy, unsigned gz, unsigned bx, unsigned by, unsigned bz, unsigned shared_bytes, tfStream_t s, void** params);
const char* tf_last_error(void);
int tf_version(void);

/* ---- memory: cudaMalloc / cudaMemcpy / cudaFree (native/cuda/ops.py:45-60; storage/tensor.py:20-46) */
int tf_malloc(void** out, size_t nbytes);
int tf_free(void* ptr);
int tf_memcpy(void* dst, const void* src, size_t nbytes, int kind);
int tf_memcpy_async(void* dst, const void* src, size_t nbytes, int kind, tfStream_t stream);
int tf_memset_async(void* dst, int value, size_t nbytes, tfStream_t stream);
/* strided device-to-device row copy (weight re-packing at install time: GEGLU block interleave, K padding) */
int tf_memcpy_2d_async(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes, size_t height,
                       tfStream_t stream);
int tf_host_alloc(void** out, size_t nbytes);   /* pinned host memory for async H2D of step parameters */
int tf_host_free(void* ptr);

/* ---- streams / events / graphs.  The reference has only the NULL stream and device-wide syncs
 * (attention/sdpa.py:70-71, variants/sd.py:40-41, ff/group_norm.py:6); timing is host-side
 * (example/sd1.py:71).  Here: explicit streams, HIP-event timing and whole-step HIP graphs. */
int tf_stream_create(tfStream_t* out);
int tf_stream_destroy(tfStream_t s);
int tf_stream_sync(tfStream_t s);
int tf_device_sync(void);
int tf_event_create(tfEvent_t* out);
int tf_event_destroy(tfEvent_t e);
int tf_event_record(tfEvent_t e, tfStream_t s);
int tf_event_sync(tfEvent_t e);
/* work launched on s after this call waits for everything recorded into e (fork / join of side branches, also while a
 * graph is being captured: the side stream joins the capture and the dependency becomes a graph edge) */
int tf_stream_wait_event(tfStream_t s, tfEvent_t e);
int tf_event_elapsed_ms(float* ms, tfEvent_t start, tfEvent_t stop);
int tf_graph_begin_capture(tfStream_t s);
int tf_graph_end_capture(tfStream_t s, tfGraph_t* out);
/* after a failed capture (an op raised between begin and end): leave capture mode and discard what was recorded, so that the
 * stream is usable again; no-op on a stream that is not capturing */
int tf_graph_abort_capture(tfStream_t s);
int tf_graph_launch(tfGraph_t g, tfStream_t s);
int tf_graph_destroy(tfGraph_t g);

/* ---- fp8 (OCP e4m3) conv / linear path, BASELINE config 5 (SD1.5 768x768 batch 32 on 8 GPUs, "fp8 MFMA conv/linear path"); the ops
 * extended are vision/conv2d.py:9-28 and ff/linear.py:112-121.  Weights: e4m3 with ONE fp32 scale per output channel, computed at pack
 * time (tf_pack_weight_fp8: scale[n] = max|w[n,:]| / 448); activations: e4m3 with scale 1, written directly by the kernels that
 * produce normalised tensors (tf_group_norm_apply_fp8, tf_layer_norm_fp8, the GEGLU epilogue of tf_linear_fp8) or by tf_quantize_fp8_f16;
 * fp32 accumulate on v_mfma_f32_16x16x32_fp8_fp8, fp16 residual stream (bias / time embedding / residual adds and the output stay
 * fp16).  Every channel count (conv) / K (linear) a multiple of 64.  x8 / x28 / w8 hold one byte per element in the layouts of the
 * fp16 entries (NHWC, KRSC, row-major). */
int tf_quantize_fp8_f16(void* y8, const void* x, long long n, float scale, tfStream_t s);
int tf_pack_weight_fp8(void* w8, void* scale_f32, const void* w, int N, int K, tfStream_t s);
size_t tf_conv2d_fp8_workspace(int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample);
int tf_conv2d_fp8(void* y, const void* x8, const void* x28, const void* w8, const void* wscale, const void* bias, const void* bias_nc,
                  long long bias_nc_stride, const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad,
                  int upsample, void* workspace, size_t workspace_bytes, void* gn_partial, size_t gn_partial_bytes, int gn_groups, int* gn_chunks,
                  tfStream_t s);
int tf_linear_fp8(void* y, const void* x8, const void* w8, const void* wscale, const void* bias, const void* residual, int M, int N, int K, int act,
                  int out_fp8, void* workspace, size_t workspace_bytes, tfStream_t s);
int tf_group_norm_apply_fp8(void* y8, const void* x, const void* x2, const void* gamma, const void* beta, const void* partial, int chunks,
                            int groups1, const void* partial2, int chunks2, int groups2, int N, int HW, int C1, int C2, int G, float eps, int silu,
                            tfStream_t s);
int tf_layer_norm_fp8(void* y8, const void* x, const void* gamma, const void* beta, int rows, int C, float eps, tfStream_t s);

/* ---- block-scaled e4m3 activations (round 4; the same reference ops: vision/conv2d.py:9-28, ff/linear.py:112-121, ff/group_norm.py:13-21,
 * ff/layer_norm.py:34-49, ff/nn.py:5-12).  An "mx8" tensor is ONE buffer: rows x C e4m3 codes (row = pixel / token, NHWC), then rows x C/32
 * E8M0 bytes: every 32 consecutive channels of a row share the power-of-two scale 2^(byte - 127) with amax / 2^e <= 448, code = e4m3(x / 2^e)
 * (round to nearest even, no saturation).  The GEMM feeds the bytes to the scale operand of v_mfma_scale_f32_16x16x128_f8f6f4; weights keep
 * tf_pack_weight_fp8's one fp32 scale per output channel.  The kernel is the 192- / 256-row ping-pong kernel: tf_mx8_gemm_supported /
 * tf_mx8_conv_supported say whether a shape fills the chip with its tiles (stride-1 convolutions without up-sampling, linears) -- a caller
 * keeps fp16 operands otherwise; an unsupported launch returns 10002.  out_mx: the GEGLU output (act = 1) as an mx8 tensor of M x N. */
size_t tf_mx8_bytes(long long rows, int C);
int tf_quantize_mx8_f16(void* y_mx, const void* x, long long rows, int C, tfStream_t s);
int tf_group_norm_apply_mx8(void* y_mx, const void* x, const void* x2, const void* gamma, const void* beta, const void* partial, int chunks,
                            int groups1, const void* partial2, int chunks2, int groups2, int N, int HW, int C1, int C2, int G, float eps, int silu,
                            tfStream_t s);
int tf_layer_norm_mx8(void* y_mx, const void* x, const void* gamma, const void* beta, int rows, int C, float eps, tfStream_t s);
int tf_mx8_gemm_supported(int M, int N, int K, int act, int out_mx);
int tf_mx8_conv_supported(int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample);
int tf_conv2d_mx8(void* y, const void* x_mx, const void* x2_mx, const void* w8, const void* wscale, const void* bias, const void* bias_nc,
                  long long bias_nc_stride, const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad,
                  void* workspace, size_t workspace_bytes, void* gn_partial, size_t gn_partial_bytes, int gn_groups, int* gn_chunks, tfStream_t s);
int tf_linear_mx8(void* y, const void* x_mx, const void* w8, const void* wscale, const void* bias, const void* residual, int M, int N, int K, int act,
                  int out_mx, void* workspace, size_t workspace_bytes, tfStream_t s);

/* ---- multi-GPU: one process per GPU, the path shards by image, and the only exchange is the one-off broadcast of
 * the packed weight arena.  The reference has no communication (device_id = 0, storage/device.py:23).  RCCL over xGMI, opened on
 * first use.  tf_comm_unique_id: rank 0 fills 128 bytes and hands them to the other ranks over any host channel; every rank then
 * calls tf_comm_init_rank on its own device (tf_init first); tf_bcast is stream-ordered and in place. */
#define TF_COMM_UNIQUE_ID_BYTES 128
int tf_comm_unique_id(void* id_out);
int tf_comm_init_rank(tfComm_t* out, const void* unique_id, int nranks, int rank);
int tf_bcast(tfComm_t comm, void* ptr, size_t nbytes, int root, tfStream_t s);
int tf_comm_destroy(tfComm_t comm);
/* per-launch profiling of the GEMM/conv kernel family with HIP events on the launch stream
 * (bench.py roofline leg): enable, run eagerly, then read back accumulated ms / flops / launches. */
int tf_prof_enable(int on);
int tf_prof_read(double* gemm_ms, double* gemm_flops, long long* gemm_launches);
/* the same accumulators with both brackets: `ms_with_reduce` spans every GEMM launch together with the split-K reduce launch that
 * finishes it (the time the conv / linear family really takes in a step), `ms_gemm_kernel_only` ends behind the k_igemm* kernel itself
 * (what tf_prof_read reports, the figure rocprofv3 lists under that kernel name) */
int tf_prof_read_full(double* ms_with_reduce, double* ms_gemm_kernel_only, double* gemm_flops, long long* gemm_launches);
float tf_prof_overhead_us(void);   /* the per-bracket event overhead tf_prof_enable(1) measured (spin-kernel pair, see csrc/gemm.hip) and subtracts */
int tf_prof_dump(const char* csv_path);   /* per-shape table: M,N,K,taps,tile,split-K,launches,ms,TFLOP/s */
/* the same event brackets around the launches of the other kernel families of the step while tf_prof_enable(1) is on (eager launches only):
 * family 1 = GroupNorm (k_gn_stats / k_gn_apply; ff/group_norm.py:3-21), 2 = the split-K reduce launches (incl. the forms that emit / apply the next
 * GroupNorm), 3 = LayerNorm (ff/layer_norm.py:8-49), 4 = SDPA (attention/sdpa.py:53-77), 5 = the image tower's input edge and exact GELU (tf_vit_patchify_u8_16, tf_gelu_erf_16; HBM bytes).  `work` = the launches' ALGORITHMIC work: HBM bytes
 * (every operand read once, every result written once) for families 1-3, FLOPs (4 B NH Tq Tk d) for family 4 -- what bench.py prices against
 * the 8 TB/s HBM roof / the MFMA peak */
int tf_prof_read_family(int family, double* ms, double* work, long long* launches);
/* element type of the split-K partial slabs a split GEMM hands to its reduce launch: 16 (default) = fp16 -- half the bytes of that seam,
 * accumulated in fp32 in split order by the reducer -- or 32 = fp32 (rounds 1-3) */
int tf_gemm_splitk_partials(int bits);
/* layout of the split-K partial slabs of the launches whose reduce also applies the GroupNorm (tf_conv2d_fused_norm_16 on k_igemm / k_igemm_patch,
 * group width a multiple of 4): 1 (default) = group-major -- the (image, group) block one reducer block owns is one contiguous run per split, read
 * 16 bytes per lane -- 0 = row-major M x N like every other split launch.  Same results bit for bit; the workspace size does not change */
int tf_gemm_splitk_slab_layout(int group_major);
/* test / tuning hook: force the GEMM tile (bm x bn in {256,128,64} x {256,160,128,64}) and split-K; 0,0,0 = heuristic */
int tf_gemm_force_config(int bm, int bn, int splitk);
/* per-shape choice of (tile, split-K, ring variant).  mode 1 (default): a shape that is not in the table is timed on its first eager
 * call and cached; mode 0: cost model only; mode 2: table only -- a shape without a row is an error naming the shape (what every rank
 * of a multi-GPU run uses, so that all ranks run the same kernels: tinyfusers_amd.native sets it when WORLD_SIZE > 1) */
int tf_gemm_autotune(int mode);
int tf_gemm_tune_save(const char* path);
int tf_gemm_tune_load(const char* path);
/* host-side view of the table (no device work).  key = {M, N, K, C1, C2, S, stride, upsample, act, flags} as tf_gemm_tune_save writes
 * a row, cfg = {bm, bn, splitk, variant, order}; tf_gemm_tune_query returns TF_E_STATE (10004) for a shape without a row */
int tf_gemm_tune_query(const int* key, int* cfg);
int tf_gemm_tune_count(int* n);
int tf_gemm_tune_entry(int index, int* key, int* cfg);
/* tf_gemm_tune_trace(1) starts remembering every shape key a launch looks up, tf_gemm_tune_trace_dump writes them (ten key fields + 1 / 0:
 * had a row), one per line -- which rows a workload needs (tools/gemm_keys.py) */
int tf_gemm_tune_trace(int on);
int tf_gemm_tune_trace_dump(const char* path);
/* test / tuning hook, kernel SELECTION only (every setting computes the same result): bits 3/4 force the deep/wide ring, 5/6 the
 * n-fastest/m-fastest block order, 7 (128) the patch variant of the 3x3 convolutions (k_igemm_patch), 8 (256) the variant whose consumer
 * waves issue part of the weight loads, each where the shape is eligible (a LayerNorm-folded linear fails under bit 7: the patch kernel has no
 * fold, and the deep ring it gives way to is for the geometries it refuses); 9 (512) the 256-row ping-pong kernel k_igemm_pp (with
 * tf_gemm_force_config(256, BN, split), BN in {128, 160, 256}: fails where it cannot take the launch), 10 (1024) the persistent short-K
 * kernel k_gemm_c4, 11 (2048) the patch form of the ping-pong kernel k_igemm_pp3 (3x3 / stride 1 convolutions on 96 / 48 / 24-pixel output rows, with
 * tf_gemm_force_config(192, BN, 1): the tile width is the instance's own; fails where it cannot take the launch), 13 (8192) the ping-pong kernel's
 * one-phase-per-k-step form on the three-slot ring, 14 (16384) the 256-row persistent short-K kernel k_gemm_c8 (with tf_gemm_force_config(256, 128, 1)), 15 (32768) the activation-resident short-K kernel k_gemm_ar (K = 256 / 320; with tf_gemm_force_config(128, 128, 1)).  The ABLATION bits -- 0 no stores,
 * 1 no MFMA, 2 no staging, 12 (4096) no fragment reads: wrong results by design -- exist only in the second library built with
 * -DTF_ABLATION (python -m tinyfusers_amd.build --ablation, loaded by the tools/ ablation scripts); the shipped library refuses them (10001) */
int tf_gemm_debug(int flags);

/* ---- layout / dtype converters (the API edge: the reference's arrays are fp32 NCHW) ----------- */
int tf_nchw_f32_to_nhwc_f16(void* dst, const void* src, int N, int C, int H, int W, tfStream_t s);
int tf_nhwc_f16_to_nchw_f32(void* dst, const void* src, int N, int C, int H, int W, tfStream_t s);
int tf_cast_f32_to_f16(void* dst, const void* src, long long n, tfStream_t s);
int tf_cast_f16_to_f32(void* dst, const void* src, long long n, tfStream_t s);
int tf_scale_cast_f32_to_f16(void* dst, const void* src, float scale, long long n, tfStream_t s);  /* 1/0.18215 * x (variants/sd.py:49) */
/* fp16 re-layouts for the VAE AttnBlock, which the reference runs on NCHW q/k/v (attention/attention.py:19-24) */
int tf_nhwc_to_nchw_f16(void* dst, const void* src, int N, int C, int H, int W, tfStream_t s);
int tf_nchw_to_nhwc_f16(void* dst, const void* src, int N, int C, int H, int W, tfStream_t s);
/* decode tail (variants/sd.py:51-53): (x+1)/2 -> clip -> *255 -> uint8; x (H,W,C) f16 -> out (H,W,C) u8 */
int tf_image_to_u8(void* out, const void* x, long long n, tfStream_t s);

/* ---- conv2d / linear: one implicit-GEMM MFMA kernel family ------------------------------------
 * tf_conv2d_f16 replaces conv_2d + Conv2d.__call__ (vision/conv2d.py:9-28, :48-58: cuDNN conv_fprop graph
 * rebuilt per call + NHWC->NCHW re-view + separate bias kernel), and folds in what surrounds it in the
 * UNet: the channel concat of vision/unet.py:72 (x2/C2), the nearest-2x upsample of unet.py:81-83
 * (upsample=1), the time-embedding broadcast add of vision/resnet.py:28 (bias_nc, one row per image) and
 * the residual add of resnet.py:30 / attention.py:75 (residual).
 *   x  : (N, H, W, C1) f16;  x2 : (N, H, W, C2) f16 or NULL (C2 = 0)
 *   w  : (Cout, R, S, C1+C2) f16 ("KRSC": the reference's (K,C,R,S) weight, vision/conv2d.py:52, with C innermost)
 *   bias : (Cout) f16 or NULL; residual : (N, Ho, Wo, Cout) f16 or NULL
 *   bias_nc : per-image bias rows f16 or NULL, image i reads bias_nc + i*bias_nc_stride (stride 0 = one row
 *             broadcast to every image, which is what resnet.py:28 does with its (1, C) embedding)
 *   y  : (N, Ho, Wo, Cout) f16, Ho = (H*(1+upsample) + 2*pad - R)/stride + 1
 *   workspace: fp32 scratch for split-K (may be NULL if tf_conv2d_workspace() returned 0).
 * Requirements: (C1+C2) % 8 == 0; R,S in {1,3} (any odd), dilation 1, groups 1 (all the UNet uses). */
int tf_conv2d_f16(void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc,
                  long long bias_nc_stride, const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R,
                  int S, int stride, int pad, int upsample, void* workspace, size_t workspace_bytes, tfStream_t s);
size_t tf_conv2d_workspace(int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample);
/* tf_conv2d_fused_f16 = tf_conv2d_f16 plus two optional fusions of what surrounds a conv in ResBlock (vision/resnet.py:6-31):
 *
 * (1) extra 1x1 sources x3 | x4 (C3 | C4 channels, same N,H,W as x; NULL / 0 = off): K continues after the R*S taps with
 *     the channels of x3 then x4 read at the output pixel itself, i.e. y += conv1x1([x3 | x4]).  w is then
 *     (Cout, R*S*(C1+C2) + C3 + C4): each row = the KRSC conv row followed by the 1x1 row; bias = the sum of both biases.
 *     This is ResBlock's ``skip_connection(x) + h`` (:24, :31) computed inside its last conv instead of a separate
 *     Conv2d(1x1) launch plus a residual read.  Not combinable with upsample.
 *     With stride > 1 the contract is: x3 | x4 are N x H x W tensors (the INPUT resolution) sampled at (ho * stride, wo * stride); a sample point
 *     beyond H or W (pad > (R - 1) / 2) reads zero.
 *
 *     R != S is admitted: the single `pad` then applies to BOTH axes (Ho = (H + 2 pad - R) / stride + 1, Wo = (W + 2 pad - S) / stride + 1), so a
 *     1 x 3 filter with pad = 1 grows the image by two rows of bias.
 *
 * (2) GroupNorm statistics of the OUTPUT (gn_partial != NULL), for the GroupNorm(32) that consumes it next
 *     (vision/resnet.py:17-18 after :11; attention/attention.py:60 after resnet.py:31): the group_norm of
 *     ff/group_norm.py:3-11 then needs no statistics pass of its own.
 *   gn_partial : f32 scratch of tf_conv2d_gn_partial_bytes(N, gn_groups) bytes, laid out (N, chunks, groups, 2)
 *                = per-chunk partial (sum, sum of squares) of the fp16 outputs, summed in a fixed order
 *   *gn_chunks : out; number of chunks written per image, to be handed to tf_group_norm_apply_f16.  0 means the
 *                statistics could not ride along for this shape (group wider than 64 channels or narrower than
 *                4, tiles that straddle images): y is complete, gn_partial is untouched, and the caller runs
 *                tf_group_norm_f16 instead. */
int tf_conv2d_fused_f16(void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc,
                        long long bias_nc_stride, const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R,
                        int S, int stride, int pad, int upsample, void* workspace, size_t workspace_bytes, const void* x3,
                        const void* x4, int C3, int C4, void* gn_partial, size_t gn_partial_bytes, int gn_groups,
                        int* gn_chunks, tfStream_t s);
/* tf_conv2d_fused_f16 that also APPLIES the GroupNorm (+ SiLU) reading its output (conv -> GroupNorm -> SiLU of vision/resnet.py:17-22,
 * :13-15 of the next block, attention/attention.py:66): when the shape runs split-K, the reduce kernel owns whole (image, group) slabs
 * (k_splitk_reduce_gn_apply), finishes the statistics and writes z = silu?(GroupNorm(y) * gamma + beta) next to y -- the
 * tf_group_norm_apply_f16 launch disappears.  *z_written = 1 when z was produced; 0 (shape ran unsplit, or groups the reduce cannot
 * hold): the caller runs tf_group_norm_apply_f16 with the statistics as before.  gn_groups must be the GroupNorm's group count. */
int tf_conv2d_fused_norm_f16(void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc, long long bias_nc_stride,
                             const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample,
                             void* workspace, size_t workspace_bytes, const void* x3, const void* x4, int C3, int C4, void* gn_partial,
                             size_t gn_partial_bytes, int gn_groups, int* gn_chunks, void* z, const void* z_gamma, const void* z_beta, float z_eps,
                             int z_silu, int* z_written, tfStream_t s);
/* tf_conv2d_fused_f16 with the GroupNorm (+ SiLU) of its INPUT applied inside the launch: GroupNorm -> SiLU -> Conv2d of
 * vision/resnet.py:13-17, :22-27 and GroupNorm -> 1x1 conv of attention/attention.py:66-68 as ONE kernel.  The statistics of x (and
 * x2) arrive as the partials their producing convs emitted (gn_partial of tf_conv2d_fused_f16: in_partial / in_chunks / in_groups1
 * for x, in_partial2 / in_chunks2 / in_groups2 for x2 or NULL; sub-group contract of tf_group_norm_apply_cat_f16); in_groups is the
 * GroupNorm's group count over C1 + C2, in_gamma / in_beta its affine (or both NULL).  The extra 1x1 sources x3 / x4 stay raw.
 * Ask tf_conv2d_gn_supported first (3x3 / stride 1 / pad 1 and 1x1 convolutions with every channel count a multiple of 64, image
 * sizes the tile grid divides); TF_E_UNSUPPORTED otherwise, and the caller runs tf_group_norm_apply_f16 + the plain conv. */
int tf_conv2d_gn_supported(int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample, int C3, int C4, int in_groups);
int tf_conv2d_gn_f16(void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc, long long bias_nc_stride,
                     const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample,
                     void* workspace, size_t workspace_bytes, const void* x3, const void* x4, int C3, int C4, void* gn_partial,
                     size_t gn_partial_bytes, int gn_groups, int* gn_chunks, const void* in_gamma, const void* in_beta, const void* in_partial,
                     int in_chunks, int in_groups1, const void* in_partial2, int in_chunks2, int in_groups2, int in_groups, float in_eps, int in_silu,
                     tfStream_t s);
size_t tf_conv2d_fused_workspace(int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample,
                                 int C3, int C4);
size_t tf_conv2d_gn_partial_bytes(int N, int groups);
/* read-only query (host code, no device work): 1 where k_igemm_patch -- the patch variant tf_gemm_debug(128) asks for -- takes the bm x bn tile of
 * this conv (vision/conv2d.py:9-28), 0 where such a launch runs the deep ring instead: the launcher's own rule, so a test can tell which ran */
int tf_conv2d_patch_admits(int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample, int C3, int C4, int bm, int bn);
/* read-only query (host code): the form of k_igemm -- 0 deep ring, 1 wide ring, 3 all-8 ring: the variant numbers of tf_prof_dump -- that the
 * bm x bn tile runs when tf_gemm_debug asked for `variant`; a form the tile does not have quietly runs the deep ring (128 x 160 and 256 x 128 have
 * no wide ring, 256 x 128 and channel counts off the 64 grid no all-8 ring).  The launcher's own rule; 10001 for a tile or variant k_igemm has not */
int tf_gemm_ring_form(int bm, int bn, int variant, int channels_on_64_grid);
/* cublasSgemm_v2 / cublasSgemmBatched (native/cublas/ops.py:22-53) as linear_cublas / gemm_batch call them
 * (ff/linear.py:58-61, :98-101): fp32, column-major, C = alpha op(A) op(B) + beta C; transa/transb 0 = N, 1 = T, 2 = C
 * (the cublasOperation_t numbers, native/cublas/ops.py:55-58).  alpha / beta are passed by value (the reference passes
 * host pointers to them).  The batched form takes DEVICE arrays of device pointers, like cuBLAS.  Test-only paths of the
 * reference (tests/linear.py:64-110): a plain fp32 FMA kernel, ascending-k accumulation. */
int tf_sgemm_f32(int transa, int transb, int m, int n, int k, float alpha, const void* A, int lda, const void* B, int ldb,
                 float beta, void* C, int ldc, tfStream_t s);
int tf_sgemm_batched_f32(int transa, int transb, int m, int n, int k, float alpha, const void* const* Aarray, int lda,
                         const void* const* Barray, int ldb, float beta, void* const* Carray, int ldc, int batch, tfStream_t s);
/* tf_linear_f16 replaces Linear.__call__ (ff/linear.py:112-121; live branch cp.dot(x, W^T)+b) and the
 * test-only cuBLAS/cuDNN paths linear_cublas / linear / gemm_batch (ff/linear.py:8-110):
 *   y(M,N) = act(x(M,K) . w(N,K)^T + bias(N)) + residual(M,N)
 * act: 0 none; 1 GEGLU (ff/nn.py:10-12): w holds 2*N rows packed by tf_pack_geglu order
 *      (16-row blocks alternating value / gate), bias likewise, y(M,N) = a * gelu_tanh(gate). */
int tf_linear_f16(void* y, const void* x, const void* w, const void* bias, const void* residual, int M, int N, int K,
                  int act, void* workspace, size_t workspace_bytes, tfStream_t s);
size_t tf_linear_workspace(int M, int N, int K, int act);
/* LayerNorm folded into the Linear that consumes it (ff/layer_norm.py:34-49 followed by ff/linear.py:112-121, the
 * norm1->to_q/k/v, norm2->to_q, norm3->GEGLU pairs of attention/attention.py:52-56):
 *   Linear(LN(x)) = rstd[m] * ( x . w'^T - mean[m] * colsum[n] ) + bias'[n],   w' = w * gamma, colsum = rowsum(w'),
 *   bias' = w . beta + bias.  tf_ln_fold_weights_f16 prepares (w', bias', colsum) once per weight set; the GEMM then runs
 *   on the RAW x and gets mean / rstd of every row from the activation fragments it streams anyway (no LayerNorm
 *   launch, no normalised tensor in HBM).  act as in tf_linear_f16 (for GEGLU fold first, then pack). */
int tf_ln_fold_weights_f16(void* w_out, void* bias_out, void* colsum_out_f32, const void* w, const void* bias, const void* gamma,
                           const void* beta, int N, int K, tfStream_t s);
int tf_linear_ln_f16(void* y, const void* x, const void* w_folded, const void* bias_folded, const void* colsum_f32, const void* residual,
                     int M, int N, int K, int act, float eps, tfStream_t s);
/* M == 1..8 weight-streaming GEMV with optional SiLU on the input (the time-embedding MLP and the 22
 * ResBlock emb_layers, vision/unet.py:53-54, vision/resnet.py:27): y(M,N) = silu?(x)(M,K) . w(N,K)^T + b */
int tf_gemv_f16(void* y, const void* x, const void* w, const void* bias, int M, int N, int K, int silu_input, tfStream_t s);

/* ---- attention: fused flash-style SDPA, replaces scaled_dot_product_attention (attention/sdpa.py:53-77:
 * cp.matmul + softmax_kernel (native/cuda/softmax.cu:24-112) + cp.matmul with the score matrix in HBM).
 * o = softmax(q k^T / sqrt(HS)) v; element strides (batch, head, token) per tensor, innermost dim HS is
 * contiguous.  Output strides select the head-merge layout: (NH*T*HS, T*HS, HS) reproduces the reference's
 * CrossAttention (attention/attention.py:38-39, no transpose back: SURVEY D11); (T*NH*HS, HS, NH*HS) is the
 * LDM-intended merge.  causal != 0 applies the CLIP causal mask (attention.py:94).  HS % 8 == 0, HS <= 160. */
int tf_sdpa_f16(void* o, const void* q, const void* k, const void* v, int B, int NH, int Tq, int Tk, int HS,
                long long q_sb, long long q_sh, long long q_st, long long k_sb, long long k_sh, long long k_st,
                long long v_sb, long long v_sh, long long v_st, long long o_sb, long long o_sh, long long o_st,
                int causal, tfStream_t s);
/* test / tuning hook: key slices inside the attention block (two slices of the key tiles per query group, merged through LDS in slice order; d = 40 / 80,
 * no causal mask).  ks = 0: per-shape choice (where the unsplit grid leaves the SIMDs short of waves), 1: never, 2: wherever a split kernel exists
 * (other launches stay unsplit).  tf_sdpa_split_ks: the number of slices (1 or 2) a tf_sdpa_f16 launch of that shape takes under the current setting. */
int tf_sdpa_force_split(int ks);
int tf_sdpa_split_ks(int B, int NH, int Tq, int Tk, int HS, int causal);
/* which kernel family a tf_sdpa_f16 / tf_sdpa_16 launch of that shape runs (the one fused launch behind attention/sdpa.py:53-77): the launcher's own
 * rule, host code, no device needed.  A function of the arguments plus tf_sdpa_force_split and the TF_SDPA_* environment switches read at load; k_st /
 * v_st are the K / V token strides in elements.  Returns a tfSdpaInstance, TF_E_ARG for arguments the launcher rejects, or TF_E_UNSUPPORTED (as the
 * launch itself does) when the keys or values of one (batch, head) slice span 2 GiB or more: every kernel addresses a slice with 32-bit byte offsets. */
typedef enum {
  TF_SDPA_INST_GENERIC = 1,   /* k_sdpa<DQK, DV>: register-staged, any head size */
  TF_SDPA_INST_DMA16 = 2,     /* k_sdpa_dma<HS, 1>: 16-query waves, 4 waves per block */
  TF_SDPA_INST_DMA32 = 3,     /* k_sdpa_dma<HS, 2>: 32-query waves, 4 waves per block */
  TF_SDPA_INST_DMA32_W8 = 4,  /* k_sdpa_dma<40 | 80, 2, 8>: 32-query waves, 8 waves per block */
  TF_SDPA_INST_SPLIT = 5      /* k_sdpa_split: two key slices inside the block */
} tfSdpaInstance;
int tf_sdpa_instance(int dtype, int B, int NH, int Tq, int Tk, int HS, long long k_st, long long v_st, int causal);
/* ---- decoupled cross-attention in ONE launch: the attention of attention/attention.py:35-41 with a second key / value set next to the text tokens (the
 * IP-Adapter's image tokens).  o = softmax(q k^T / sqrt(HS)) v + (*scale2_dev) softmax(q k2^T / sqrt(HS)) v2: two independent softmaxes, no mask;
 * scale2_dev is one fp32 ON THE DEVICE, read by the kernel, so a captured launch follows a changed scale without a re-capture, and a scale of 0 gives
 * tf_sdpa_16's values of the text set alone.  Strides and the output head-merge choices are tf_sdpa_16's (k2 / v2 carry their own).  HS in {40, 80,
 * 160}, Tk >= 1, 1 <= Tk2 <= 64 (one key tile), dtype TF_DTYPE_F16 / TF_DTYPE_BF16; anything else returns TF_E_ARG or TF_E_UNSUPPORTED with a message
 * before the device is touched, as does a key set whose (batch, head) slice spans 2 GiB or more.  The launch runs the dual instance of the family
 * tf_sdpa_instance names for the text launch with the split forms left out (TF_SDPA_INST_DMA16 / _DMA32 / _DMA32_W8); tf_sdpa_dual_instance answers with
 * that rule, host code only.  Profiled in family 4 with FLOPs 4 B NH Tq (Tk + Tk2) HS. */
int tf_sdpa_dual_16(int dtype, void* o, const void* q, const void* k, const void* v, int Tk, const void* k2, const void* v2, int Tk2, const float* scale2_dev,
                    int B, int NH, int Tq, int HS, long long q_sb, long long q_sh, long long q_st, long long k_sb, long long k_sh, long long k_st,
                    long long v_sb, long long v_sh, long long v_st, long long k2_sb, long long k2_sh, long long k2_st, long long v2_sb, long long v2_sh,
                    long long v2_st, long long o_sb, long long o_sh, long long o_st, tfStream_t s);
int tf_sdpa_dual_instance(int dtype, int B, int NH, int Tq, int Tk, int Tk2, int HS, long long k_st, long long v_st, long long k2_st, long long v2_st);
/* ---- perturbed-attention guidance in ONE launch: the self-attention of attention/attention.py:35-41 in which the batch entries [pag_b0, pag_b1) take
 * the identity in place of the softmax, o[b, h, t, :] = v[b, h, t, :] (the bits, through the launch's own v and o strides), while *pag_flag_dev -- one
 * fp32 ON THE DEVICE, read when the kernel runs -- is not zero; q and k of those entries are then not read.  Every other entry, and every entry while the
 * word is zero, gets tf_sdpa_16's result bit for bit (its unsplit LDS-DMA kernel of the same family; no causal form).  A captured launch follows the
 * word without a re-capture.  Arguments as tf_sdpa_16; an empty range is legal (plain attention).  Head sizes 40, 64, 80, 128 and 160; the launch runs
 * the family tf_sdpa_instance names with the split forms left out (TF_SDPA_INST_DMA16 / _DMA32 / _DMA32_W8), and tf_sdpa_pag_instance answers with that
 * rule, host code only.  A head size without an LDS-DMA kernel, a slice of 2 GiB or more (TF_E_UNSUPPORTED), a range outside [0, B] or a NULL flag
 * (TF_E_ARG) return with a message before the device is touched.  Profiled in family 4 as the plain launch. */
int tf_sdpa_pag_16(int dtype, void* o, const void* q, const void* k, const void* v, int B, int NH, int Tq, int Tk, int HS, long long q_sb, long long q_sh,
                   long long q_st, long long k_sb, long long k_sh, long long k_st, long long v_sb, long long v_sh, long long v_st, long long o_sb, long long o_sh,
                   long long o_st, int pag_b0, int pag_b1, const float* pag_flag_dev, tfStream_t s);
int tf_sdpa_pag_instance(int dtype, int B, int NH, int Tq, int Tk, int HS, long long k_st, long long v_st, int pag_b0, int pag_b1);
/* ---- temporal attention of a video latent (the attention of an AnimateDiff motion module; attention/sdpa.py:53-77 with the F frames of ONE pixel as
 * the tokens): for every video g < G, pixel p < P and head h < NH, o[g, f, p, h, :] = softmax_f'(q'[f] . k'[f'] / sqrt HS) v'[f'] over the F frames.
 * Element (g, f, p, h, c) of a tensor x lies at x + (g F + f) x_sf + p x_sp + h x_sh + c: a frame, a pixel and a head stride (elements) per tensor, the
 * videos F frame strides apart -- q, k, v are read where a fused q|k|v projection left them (column views of a (G F, P, 3 C) buffer: x_sf = 3 C P,
 * x_sp = 3 C, x_sh = HS) and o is written as the (G F, P, C) token matrix the output projection reads; nothing is transposed or copied.  pe_q, pe_k,
 * pe_v: optional fp32 tables of shape (F, NH HS) ON THE DEVICE, added in fp32 as the operand is loaded, q' = q + pe_q[f] (NULL: zero) -- the motion
 * module's (LN(x) + pe) W = LN(x) W + pe W with pe W precomputed.  Scores, softmax and P V are fp32 (fixed summation order, no atomics: deterministic);
 * the output is rounded once.  1 <= F <= 32 (more: TF_E_UNSUPPORTED), HS % 8 == 0 in [8, 160], NH >= 1, any G, P >= 0 (0: nothing to do); every stride
 * a multiple of 8 elements, every pointer 16-byte aligned; what is not returns TF_E_ARG with a message before the device is touched.  Profiled in
 * family 4 with 4 G P NH F^2 HS FLOPs. */
int tf_sdpa_temporal_16(int dtype, void* o, const void* q, const void* k, const void* v, const float* pe_q, const float* pe_k, const float* pe_v, int G, int F,
                        int P, int NH, int HS, long long q_sf, long long q_sp, long long q_sh, long long k_sf, long long k_sp, long long k_sh, long long v_sf,
                        long long v_sp, long long v_sh, long long o_sf, long long o_sp, long long o_sh, tfStream_t s);
/* row softmax over (N, C) fp32 -- Device.softmax (storage/device.py:129-157; softmax_func.cu:22-113) */
int tf_softmax_rows_f32(void* out, const void* inp, int N, int C, tfStream_t s);
/* softmax step of the UNFUSED attention (attention/sdpa.py:63-75 as the reference runs it: scale * matmul, + mask (:67-68: bool ->
 * -inf where false, anything else additive), softmax kernel, matmul).  Serves what tf_sdpa_f16 does not: arbitrary masks and head sizes
 * beyond 160 (AttnBlock's single head of 512, attention/attention.py:10-24).  out[r, c] = softmax_c(scale * inp[r, c] + mask[r % mask_rows, c]);
 * rows are ldc apart (ldc >= C; out's pad columns are zero-filled); mask_f32: (mask_rows, C) fp32 additive or NULL. */
int tf_softmax_mask_rows_f16(void* out, const void* inp, const void* mask_f32, long long rows, int C, int ldc, float scale, long long mask_rows,
                             tfStream_t s);
/* The same two steps with the scores kept in fp32 between them, as the reference keeps them (attention/sdpa.py:63-66: fp32 cp.matmul
 * into `preatt`, softmax kernel native/cuda/softmax.cu:24-112 on fp32): tf_linear_f32out_f16 stores the raw fp32 accumulators
 * y32(M,N) = x(M,K) . w(N,K)^T (fp16 operands, no bias / activation), tf_softmax_mask_rows_f32in_f16 reads them (rows ldi floats apart)
 * and writes fp16 probabilities (rows ldo halves apart, pad columns C..ldo-1 zero-filled).  A scaled logit of several hundred -- the
 * d = 512 single-head AttnBlock on real weights -- would lose 0.1 ... 1 in fp16 in front of the exp. */
int tf_linear_f32out_f16(void* y_f32, const void* x, const void* w, int M, int N, int K, tfStream_t s);
int tf_softmax_mask_rows_f32in_f16(void* out, int ldo, const void* inp_f32, int ldi, const void* mask_f32, long long rows, int C, float scale,
                                   long long mask_rows, tfStream_t s);

/* ---- normalisation ---------------------------------------------------------------------------
 * group_norm + GroupNorm affine (+ the SiLU that always follows it in ResBlock / UNet.out)
 * (ff/group_norm.py:3-11, :13-21; storage/tensor.py:68-70): x,y (N, HW, C) f16 NHWC, G groups, biased var.
 * x2/C2: optional second source for the channel concat (vision/unet.py:72): channels [C1, C1+C2) come from x2.
 * gamma/beta f16 (C) or NULL (plain group_norm).  workspace: tf_group_norm_workspace bytes. */
int tf_group_norm_f16(void* y, const void* x, const void* x2, const void* gamma, const void* beta, int N, int HW,
                      int C1, int C2, int G, float eps, int silu, void* workspace, size_t workspace_bytes, tfStream_t s);
size_t tf_group_norm_workspace(int N, int HW, int C, int G);
/* second half of tf_group_norm_f16 (normalise + affine [+ SiLU]) on statistics already produced by
 * tf_conv2d_fused_f16: partial (N, chunks, G, 2) f32.  Same arithmetic as tf_group_norm_f16 from the fold onwards. */
int tf_group_norm_apply_f16(void* y, const void* x, const void* gamma, const void* beta, const void* partial, int chunks,
                            int N, int HW, int C, int G, float eps, int silu, tfStream_t s);
/* GroupNorm(G) of the channel concat [x | x2] of two EQUALLY wide tensors (vision/unet.py:72 into resnet.py:8) whose
 * statistics came from tf_conv2d_fused_f16 as G-group partials of each half: a group of the concat is two adjacent
 * groups of one half, so no statistics pass over the concat is needed.  partial (N, chunks, G, 2), partial2 (N, chunks2, G, 2). */
int tf_group_norm_apply2_f16(void* y, const void* x, const void* x2, const void* gamma, const void* beta, const void* partial,
                             int chunks, const void* partial2, int chunks2, int N, int HW, int C1, int G, float eps, int silu,
                             tfStream_t s);
/* General form: the producers' partials have groups1 / groups2 sub-groups of equal width (C1/groups1 == C2/groups2) that tile the groups of
 * the concat ((C1+C2)/G = m * width, m <= 8); a group may straddle the two sources (1280 + 640 channels, 32 groups: partials with 64 and
 * 32 sub-groups of 20 channels).  tf_group_norm_apply2_f16 is the equal-split case groups1 = groups2 = G. */
int tf_group_norm_apply_cat_f16(void* y, const void* x, const void* x2, const void* gamma, const void* beta, const void* partial, int chunks,
                                int groups1, const void* partial2, int chunks2, int groups2, int N, int HW, int C1, int C2, int G, float eps,
                                int silu, tfStream_t s);
/* LayerNorm over the last dim (ff/layer_norm.py:8-32, :34-49; semantics = F.layer_norm, tests/layer_norm.py:38) */
int tf_layer_norm_f16(void* y, const void* x, const void* gamma, const void* beta, int rows, int C, float eps, tfStream_t s);
/* which kernel a tf_layer_norm_f16 / _bf16 / _fp8 / _mx8 launch of (rows, C) runs (the launches behind ff/layer_norm.py:8-49): the launcher's own
 * rule, host code, no device needed.  Returns a tfLayerNormInstance, or TF_E_ARG for sizes the launcher rejects. */
typedef enum {
  TF_LN_INST_LPR64 = 1,       /* k_layer_norm<64>: one wave per row */
  TF_LN_INST_LPR8 = 2,        /* k_layer_norm<8>: 8 rows per wave */
  TF_LN_INST_LPR16 = 3,       /* k_layer_norm<16>: 4 rows per wave */
  TF_LN_INST_LPR32 = 4,       /* k_layer_norm<32>: 2 rows per wave */
  TF_LN_INST_ANY_WAVE = 5,    /* k_layer_norm_any<true>: any row length, one wave per row */
  TF_LN_INST_ANY_BLOCK = 6    /* k_layer_norm_any<false>: any row length, one block per row */
} tfLayerNormInstance;
int tf_layer_norm_instance(int rows, int C);
/* the launch geometry of a GroupNorm of (N, HW, C) (the launches behind ff/group_norm.py:3-21), as tf_group_norm_f16 / _bf16 and the apply entries
 * compute it: *rpb pixel rows per block sweep, the statistics pass in *chunks chunks of *pix_per_chunk pixels per image, the apply pass in
 * *apply_blocks units of 4 * rpb pixels per image, *nbatch of them to a block (the launch has ceil(apply_blocks / nbatch) blocks per image).
 * Host code, no device needed; TF_E_ARG for sizes the launchers reject. */
int tf_group_norm_geometry(int N, int HW, int C, int* rpb, int* chunks, int* pix_per_chunk, int* apply_blocks, int* nbatch);

/* ---- bfloat16 forms ---------------------------------------------------------------------------
 * The reference's op tests run every case in bfloat16 as well as float16 (tests/group_norm.py:12-19 and
 * tests/layer_norm.py:13-27 with atol = rtol = 0.125; tests/linear.py:13 lists it): the same four operators with every
 * 16-bit tensor (x, x2, w, gamma, beta, bias, residual, y) holding bfloat16.  Statistics and accumulation are fp32 as
 * in the float16 forms; the GEMMs use the gfx950 bf16 MFMA (v_mfma_f32_16x16x32_bf16) on the tuned kernels of the float16 forms (round 5; these
 * entries take no workspace, so they never split K: tf_linear_16 / tf_conv2d_fused_16 below are the full forms). */
int tf_group_norm_bf16(void* y, const void* x, const void* x2, const void* gamma, const void* beta, int N, int HW,
                       int C1, int C2, int G, float eps, int silu, void* workspace, size_t workspace_bytes, tfStream_t s);
int tf_layer_norm_bf16(void* y, const void* x, const void* gamma, const void* beta, int rows, int C, float eps, tfStream_t s);
/* y(M,N) = x(M,K) . w(N,K)^T + bias(N) + residual(M,N)   (ff/linear.py:112-121) */
int tf_linear_bf16(void* y, const void* x, const void* w, const void* bias, const void* residual, int M, int N, int K, tfStream_t s);
/* tf_conv2d_bf16 (its prototype closes this block): tf_conv2d_f16's arguments without the workspace (vision/conv2d.py:9-28): NHWC x (+ concat x2), w (Cout, R, S, C1 + C2) */
/* the bfloat16 STEP (round 4: config.set_dtype("bf16"), bench.py --dtype bf16): the sampler on bfloat16 tensors throughout -- conv / linear /
 * GEGLU on the bf16 MFMA (tf_conv2d_bf16, tf_linear_act_bf16), GroupNorm / LayerNorm / SiLU in bfloat16, the time-embedding chain, CFG duplicate
 * and the CFG + DDIM update reading bfloat16 (vision/unet.py:51-97, variants/sd.py:14-46); since round 5 the step runs on the dtype-tagged fused
 * entries below (tf_*_16) and attention is native bfloat16 (tf_sdpa_16); tf_convert_* remain for callers that mix the types */
int tf_linear_act_bf16(void* y, const void* x, const void* w, const void* bias, const void* residual, int M, int N, int K, int act, tfStream_t s);
int tf_silu_bf16(void* y, const void* x, long long n, tfStream_t s);
int tf_convert_f16_to_bf16(void* y_bf16, const void* x_f16, long long n, tfStream_t s);
int tf_convert_bf16_to_f16(void* y_f16, const void* x_bf16, long long n, tfStream_t s);
int tf_timestep_embedding_bf16(void* out, const void* step_params, int dim, float max_period, tfStream_t s);
int tf_cfg_duplicate_bf16(void* x2b, const void* latent, int B, int C, int H, int W, tfStream_t s);
int tf_cfg_ddim_step_bf16(void* latent, const void* eps2, const void* params, int B, int C, int H, int W, tfStream_t s);
int tf_conv2d_bf16(void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc, long long bias_nc_stride,
                   const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample,
                   tfStream_t s);

/* ---- dtype-tagged forms of the step's fused entries (round 5): the bfloat16 step runs the SAME structure as the float16 step -- every fusion,
 * split-K, the tuned tiles -- so each of these is its _f16 namesake (same arguments, same semantics, same reference lines) with one leading tag
 * saying what every 16-bit tensor of the call holds: TF_DTYPE_F16 (= the _f16 entry) or TF_DTYPE_BF16 (v_mfma_f32_16x16x32_bf16; fp32 accumulation,
 * statistics and split-K partial slabs).  The reference's own op tests run bfloat16 next to float16 (tests/group_norm.py:12-19, tests/layer_norm.py:12-19,
 * tests/linear.py:13).  tf_sdpa_16: attention natively in bfloat16 (Q K^T and P V on the bf16 MFMA, P rounded to bfloat16): no fp16 hop, so
 * activations beyond 65504 stay finite. */
#define TF_DTYPE_F16 0
#define TF_DTYPE_BF16 1
int tf_conv2d_fused_16(int dtype, void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc, long long bias_nc_stride,
                       const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample,
                       void* workspace, size_t workspace_bytes, const void* x3, const void* x4, int C3, int C4, void* gn_partial,
                       size_t gn_partial_bytes, int gn_groups, int* gn_chunks, tfStream_t s);
int tf_conv2d_fused_norm_16(int dtype, void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc, long long bias_nc_stride,
                            const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample,
                            void* workspace, size_t workspace_bytes, const void* x3, const void* x4, int C3, int C4, void* gn_partial,
                            size_t gn_partial_bytes, int gn_groups, int* gn_chunks, void* z, const void* z_gamma, const void* z_beta, float z_eps,
                            int z_silu, int* z_written, tfStream_t s);
int tf_conv2d_gn_16(int dtype, void* y, const void* x, const void* x2, const void* w, const void* bias, const void* bias_nc, long long bias_nc_stride,
                    const void* residual, int N, int H, int W, int C1, int C2, int Cout, int R, int S, int stride, int pad, int upsample,
                    void* workspace, size_t workspace_bytes, const void* x3, const void* x4, int C3, int C4, void* gn_partial,
                    size_t gn_partial_bytes, int gn_groups, int* gn_chunks, const void* in_gamma, const void* in_beta, const void* in_partial,
                    int in_chunks, int in_groups1, const void* in_partial2, int in_chunks2, int in_groups2, int in_groups, float in_eps, int in_silu,
                    tfStream_t s);
int tf_linear_16(int dtype, void* y, const void* x, const void* w, const void* bias, const void* residual, int M, int N, int K, int act,
                 void* workspace, size_t workspace_bytes, tfStream_t s);
int tf_ln_fold_weights_16(int dtype, void* w_out, void* bias_out, void* colsum_out_f32, const void* w, const void* bias, const void* gamma, const void* beta,
                          int N, int K, tfStream_t s);
int tf_linear_ln_16(int dtype, void* y, const void* x, const void* w_folded, const void* bias_folded, const void* colsum_f32, const void* residual,
                    int M, int N, int K, int act, float eps, tfStream_t s);
int tf_gemv_16(int dtype, void* y, const void* x, const void* w, const void* bias, int M, int N, int K, int silu_input, tfStream_t s);
/* tf_gemv_16 for 1 <= M <= 65536 rows in ONE launch: the same kernel with one block row per group of 8 input rows, so every output row holds the
 * bits tf_gemv_16 gives it in a launch of its own group (a whole schedule's time-embedding rows, M = steps x images: the weight is read from HBM
 * once and from the cache by the other groups).  K a positive multiple of 8; x and w 16-byte aligned */
int tf_gemv_rows_16(int dtype, void* y, const void* x, const void* w, const void* bias, int M, int N, int K, int silu_input, tfStream_t s);
int tf_sdpa_16(int dtype, void* o, const void* q, const void* k, const void* v, int B, int NH, int Tq, int Tk, int HS,
               long long q_sb, long long q_sh, long long q_st, long long k_sb, long long k_sh, long long k_st,
               long long v_sb, long long v_sh, long long v_st, long long o_sb, long long o_sh, long long o_st, int causal, tfStream_t s);
int tf_group_norm_apply_16(int dtype, void* y, const void* x, const void* gamma, const void* beta, const void* partial, int chunks,
                           int N, int HW, int C, int G, float eps, int silu, tfStream_t s);
int tf_group_norm_apply_cat_16(int dtype, void* y, const void* x, const void* x2, const void* gamma, const void* beta, const void* partial, int chunks,
                               int groups1, const void* partial2, int chunks2, int groups2, int N, int HW, int C1, int C2, int G, float eps,
                               int silu, tfStream_t s);
int tf_add_16(int dtype, void* y, const void* a, const void* b, long long n, tfStream_t s);

/* ---- elementwise (storage/tensor.py:64-86; ff/nn.py:10-12; vision/unet.py:72, :81-83) ---------- */
int tf_silu_f16(void* y, const void* x, long long n, tfStream_t s);
int tf_sigmoid_f16(void* y, const void* x, long long n, tfStream_t s);
int tf_gelu_f16(void* y, const void* x, long long n, tfStream_t s);
int tf_quick_gelu_f16(void* y, const void* x, long long n, tfStream_t s);
/* Embedding lookup (ff/embedding.py:10-24; the CLIP text encoder's token + position embeddings, vae/encoder.py:68-73):
 * out(n_tokens, dim) f16 = table[ids[i], :] (+ pos[i % T, :] when pos != NULL).  ids: n_tokens int32 ON THE DEVICE. */
int tf_embedding_f16(void* out, const void* table, const void* ids, const void* pos, long long n_tokens, int dim, int vocab,
                     int T, tfStream_t s);
/* Debugging aid, no reference counterpart: *flag (device int) = 1 when the nbytes at x hold a non-finite f16 (is_f32 = 0) or f32
 * value.  Every element is looked at, the last one of an odd-length f16 array (nbytes % 4 == 2) included.  Stream-ordered and capturable
 * (tools/diag_graph.py instruments a whole step with it). */
int tf_debug_nonfinite(const void* x, long long nbytes, int is_f32, void* flag, tfStream_t s);
/* Debugging aid: *sum (device u64) += sum over i of word_i * ((uint32(i) * 2654435761) | 1) mod 2^64 over the nbytes / 4 WHOLE 32-bit words at x
 * (order independent).  Trailing nbytes % 4 bytes are not part of the sum: pad an odd-length fp16 array to a word before comparing checksums. */
int tf_debug_checksum(const void* x, long long nbytes, void* sum, tfStream_t s);
int tf_geglu_f16(void* y, const void* x, int rows, int C, tfStream_t s);          /* x (rows,2C) -> y (rows,C) */
int tf_add_f16(void* y, const void* a, const void* b, long long n, tfStream_t s);
int tf_add_bias_nc_f16(void* y, const void* x, const void* bias_nc, int N, int HW, int C, tfStream_t s);
int tf_upsample2x_nhwc_f16(void* y, const void* x, int N, int H, int W, int C, tfStream_t s);
int tf_concat_channels_f16(void* y, const void* a, const void* b, long long rows, int Ca, int Cb, tfStream_t s);
/* im2col for the 4-channel conv_in (K = R*S*C padded to Kpad): y (N*Ho*Wo, Kpad) */
int tf_im2col_nhwc_f16(void* y, const void* x, int N, int H, int W, int C, int R, int S, int stride, int pad, int Kpad, tfStream_t s);
/* the same for output rows [ho_begin, ho_end) of every image: y (N*(ho_end-ho_begin)*Wo, Kpad).  The 10000 x 10000 input of the
 * reference's own conv test (tests/conv2d.py:13-33) runs as row bands, each band's patch matrix below the 2 GiB a buffer descriptor spans */
int tf_im2col_rows_nhwc_f16(void* y, const void* x, int N, int H, int W, int C, int R, int S, int stride, int pad, int Kpad, int ho_begin, int ho_end,
                            tfStream_t s);
/* own-runtime kernels of the reference (native/cuda kernels via storage/device.py:79-233), fp32 */
int tf_scale_f32(void* x, float scale, long long n, tfStream_t s);                        /* scale_tensor_func.cu:5-10 */
int tf_add_bias_colmajor_f32(void* out, const void* bias, int BT, int OC, tfStream_t s);  /* add_bias_func.cu:1-9 */
int tf_transpose_f32(void* out, const void* inp, int ndim, const int* shape, const int* axes, tfStream_t s); /* transpose.cu, transpose4d.cu */

/* ---- sampler pieces (vision/unet.py:92-97; variants/sd.py:14-25, :27-46) ------------------------
 * step_params (device, fp32): [0] timestep, [1] a_t, [2] a_prev, [3] guidance -- written once per step by
 * tf_set_step_params (values travel as kernel arguments, so there is no host buffer to race with) ahead of the
 * replay of the step's HIP graph, whose kernels read them from device memory. */
int tf_set_step_params(void* step_params, float timestep, float a_t, float a_prev, float guidance, tfStream_t s);
/* the same launch also copies nbytes (a multiple of 16, both pointers 16-byte aligned) src -> dst: the time-embedding chain of
 * vision/unet.py:54-56 + the ResBlocks' Linear(SiLU(emb)) (vision/resnet.py:28) depends on the timestep alone, so a sampler computes the
 * row of a timestep once, keeps it, and hands it to the captured step through this copy instead of four launches per step */
int tf_set_step_params_copy(void* step_params, float timestep, float a_t, float a_prev, float guidance, void* dst, const void* src, long long nbytes, tfStream_t s);
int tf_timestep_embedding_f16(void* out, const void* step_params, int dim, float max_period, tfStream_t s);
/* latent (B,C,H,W) f32 NCHW  ->  unet input (2B,H,W,C) f16 NHWC = [latent ; latent]  (variants/sd.py:31; csrc/sampler.hip, the step's head) */
int tf_cfg_duplicate_f16(void* x2b_nhwc, const void* latent_nchw_f32, int B, int C, int H, int W, tfStream_t s);
/* e = e_u + g (e_c - e_u); DDIM sigma=0 update, latent updated in place (variants/sd.py:44-45, :14-25) */
int tf_cfg_ddim_step_f32(void* latent_nchw_f32, const void* unet_out_2b_nhwc_f16, const void* step_params, int B, int C,
                         int H, int W, tfStream_t s);
/* the same with the two UNet outputs in separate tensors (B,4,H,W each): the unconditional and the conditional half of the CFG pair
 * (variants/sd.py:31-45) run as two independent UNet chains on two streams / graph branches (config.cfg_parallel) */
int tf_cfg_ddim_step2_f32(void* latent, const void* eps_uncond, const void* eps_cond, const void* step_params, int B, int C, int H, int W, tfStream_t s);

/* ---- samplers beyond sigma = 0 DDIM (csrc/sampler.hip; generalises variants/sd.py:14-25 and the CFG combine of :27-46) -------------
 * csrc/sampler.hip holds the sampler side of every mode below: the generator, the parameter launch, ONE kernel for the step's opening launch
 * (tf_cfg_duplicate_*, tf_cfg_concat_*, tf_latent_stack1_*) and ONE for its closing launch (tf_cfg_sampler_step_*, tf_cfg_sampler_step_masked_*,
 * tf_cfg3_sampler_step_*, tf_sampler_step1_*); the entries differ in what their parameters mean and in which arguments they refuse.
 * Noise: Philox4x32-10, key = (seed_lo, seed_hi), counter = (q, global image index, step, tag); counter q of an image gives its NCHW
 * elements 4q .. 4q+3 (u = ((bits >> 8) + 0.5) 2^-24, Box-Muller on (u0, u1) and (u2, u3)).  Tag 0: initial latent; tag 1: the ancestral
 * noise of schedule step `step`; tag 2: the known region of an inpainting step.  Image k's noise is independent of the batch size and of the
 * rank that draws it. */
/* out (images, per_image) fp32 N(0,1): images image_offset .. image_offset + images - 1 (per_image <= 2^32) */
int tf_randn_f32(void* out, int images, long long per_image, unsigned seed_lo, unsigned seed_hi, int image_offset, int step, int tag, tfStream_t s);
/* tf_set_step_params_copy (variants/sd.py:27-46 step scalars) extended to the sampler block of 8 words: [0..3] as there, then u32 [4] the
 * schedule row, [5] [6] the seed, [7] the global index of image 0.  nbytes = 0 (dst, src may be NULL): no copy, the non-hoisted step */
int tf_set_sampler_params(void* step_params, float timestep, float a_t, float a_prev, float guidance, int row, unsigned seed_lo, unsigned seed_hi, int image_offset,
                          void* dst, const void* src, long long nbytes, tfStream_t s);
/* the DDIM update of variants/sd.py:14-25 in the one form every sampler shares: e = e_u + g (e_c - e_u), x0 = (x - sqrt(1-a_t) e) / sqrt(a_t),
 * x' = c_x x + c_0 x0 + c_1 x0_prev + c_n z (z: tag 1, step = row), x0_prev <- x0.  coeffs (rows, 4) fp32 [c_x, c_0, c_1, c_n]; the row and
 * the seed come from step_params (tf_set_sampler_params).  x0_hist (B,C,H,W) fp32 is read only when c_1 != 0.  eps2 as tf_cfg_ddim_step_f32 */
int tf_cfg_sampler_step_f32(void* latent, const void* eps2, void* x0_hist, const void* step_params, const void* coeffs, int rows, int B, int C, int H, int W, tfStream_t s);
int tf_cfg_sampler_step_bf16(void* latent, const void* eps2, void* x0_hist, const void* step_params, const void* coeffs, int rows, int B, int C, int H, int W, tfStream_t s);

/* ---- image-to-image and masked inpainting (csrc/img2img.hip): the encoder edges of vae/vae.py:12-15 (image -> means, only the means kept),
 * the inverse of the decode scale and tail of variants/sd.py:48-54; on the sampler's side the noising to a start level and the sampler
 * update of variants/sd.py:14-25 (tf_cfg_sampler_step_*) with a latent blend. */
/* uint8 (B,H,W,3) -> fp16 x / 127.5 - 1 in the same element order: the NHWC (B,3,H,W) image AutoencoderKL.encode reads; n = B*H*W*3 */
int tf_image_from_u8_f16(void* out, const void* x, long long n, tfStream_t s);
/* encoder means (B,4,H,W) fp16 NHWC -> x0 (B,4,H,W) fp32 NCHW = 0.18215 means (the decode side divides by it, variants/sd.py:49) */
int tf_means_to_latent_f32(void* x0, const void* means, int B, int H, int W, tfStream_t s);
/* out = sqrt(a) x0 + sqrt(1-a) z, z the tag-0 normal of global image image_offset + k at step 0 (tf_randn_f32's initial latent); out may
 * be x0 itself; a in (0, 1] */
int tf_noise_to_level_f32(void* out, const void* x0, int images, long long per_image, float a, unsigned seed_lo, unsigned seed_hi, int image_offset, tfStream_t s);
/* tf_cfg_sampler_step_* then x' <- m x' + (1-m) (sqrt(a_s) x0_init + sqrt(1-a_s) z2): a_s = step_params[2] (a_prev), z2 the tag-2 normal at
 * step = row; x0_init (B,C,H,W) fp32, mask (B,1,H,W) fp32, 1 = repaint (fractional values blend) */
int tf_cfg_sampler_step_masked_f32(void* latent, const void* eps2, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* x0_init,
                                   const void* mask, int B, int C, int H, int W, tfStream_t s);
int tf_cfg_sampler_step_masked_bf16(void* latent, const void* eps2, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* x0_init,
                                    const void* mask, int B, int C, int H, int W, tfStream_t s);

/* ---- the guidance-free step (variants/sd.py compile(..., cfg=False)): ONE guidance group instead of the CFG pair of
 * variants/sd.py:31 and :44 -- what a consistency model (LCM, LCM-LoRA) samples with at guidance 1, where e = e_u + 1 (e_c - e_u) = e_c and
 * the unconditional half of every launch is thrown away.  The opening and the closing launch of the captured step; the UNet between them
 * runs on B images against the context alone. */
/* latent (B,C,H,W) f32 NCHW [, cond (B,Cc,H,W) f32 NCHW] -> x (B, H, W, C+Cc) 16-bit NHWC: ONE guidance group.  cond == NULL iff Cc == 0.
 * The latent channels are rounded exactly as tf_cfg_duplicate_* / tf_cfg_concat_* round them: x is their group 0, bit for bit. */
int tf_latent_stack1_f16(void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, tfStream_t s);
int tf_latent_stack1_bf16(void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, tfStream_t s);
/* tf_cfg_sampler_step_* (variants/sd.py:14-25) without the CFG combine: e = eps (B,C,H,W NHWC 16-bit, ONE branch); then its expressions in its
 * order: x0 = (x - sqrt(1-a_t) e)/sqrt(a_t); x' = c_x x + c_0 x0 + c_1 x0_prev + c_n z (tag 1, step = row); x0_prev <- x0.
 * x0_init and mask both NULL: that is all.  Both set: then the blend of tf_cfg_sampler_step_masked_*
 * (x' <- m x' + (1-m)(sqrt(a_s) x0_init + sqrt(1-a_s) z2), tag 2, always drawn).  Exactly one of them NULL: TF_E_ARG, bad arguments.
 * x0_hist is read only when c_1 != 0, the tag-1 noise drawn only when c_n != 0; step_params[3] (guidance) is not read. */
int tf_sampler_step1_f32(void* latent, const void* eps, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* x0_init, const void* mask,
                         int B, int C, int H, int W, tfStream_t s);
int tf_sampler_step1_bf16(void* latent, const void* eps, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* x0_init, const void* mask,
                          int B, int C, int H, int W, tfStream_t s);

/* ---- perturbed-attention guidance on the sampler above (variants/sd.py compile(..., pag=True)): a third guidance group [uncond ; perturbed ; cond]
 * next to the CFG pair of variants/sd.py:31, combined by the three-branch expression at g_I = g, g_T = g + s:
 * e0 + g_T (e2 - e1) + g_I (e1 - e0) = e_u + g (e_c - e_u) + s (e_c - e_p). */
/* tf_cfg_duplicate_* (variants/sd.py:31) for THREE copies of the latent alone: latent (B,C,H,W) f32 NCHW -> x3b (3B,C,H,W) NHWC 16-bit, every group
 * rounded as tf_cfg_duplicate_* rounds it; H == 0 or W == 0 writes nothing */
int tf_latent_stack3_f16(void* x3b, const void* latent, int B, int C, int H, int W, tfStream_t s);
int tf_latent_stack3_bf16(void* x3b, const void* latent, int B, int C, int H, int W, tfStream_t s);
/* tf_cfg3_sampler_step_* then the blend of tf_cfg_sampler_step_masked_* (x' <- m x' + (1-m)(sqrt(a_s) x0_init + sqrt(1-a_s) z2), tag 2); edit_params,
 * x0_init and mask all set */
int tf_cfg3_sampler_step_masked_f32(void* latent, const void* eps3, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* edit_params,
                                    const void* x0_init, const void* mask, int B, int C, int H, int W, tfStream_t s);
int tf_cfg3_sampler_step_masked_bf16(void* latent, const void* eps3, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* edit_params,
                                     const void* x0_init, const void* mask, int B, int C, int H, int W, tfStream_t s);

/* ---- SD-2.x sampling (variants/sd.py compile(..., prediction="v", cfg_rescale=True)): the closing launch of the captured step stated ONCE, by
 * `groups` (1, 2 or 3 guidance groups in eps, combined as tf_sampler_step1_* / tf_cfg_sampler_step_* / tf_cfg3_sampler_step_* combine them) and
 * `flags` -- the update of variants/sd.py:14-25 behind the CFG combine of variants/sd.py:27-46, which know the eps parameterisation alone.
 *   bit 0  v-prediction (Salimans & Ho 2022; the 768-v checkpoints): the model output is v and x0 = sqrt(a_t) x - sqrt(1-a_t) e replaces
 *          x0 = (x - sqrt(1-a_t) e) / sqrt(a_t); nothing else changes -- the coefficient rows are in x0 form
 *   bit 1  the masked blend of tf_cfg_sampler_step_masked_*: x0_init and mask are both set iff the bit is set
 *   bit 2  CFG rescale (Lin et al. 2023; diffusers' rescale_noise_cfg): per image over its C H W elements f = std(e_t) / std(e), e_t the LAST
 *          group (the text group of a pair, of pag=True's [perturbed ; cond] and of its [uncond ; perturbed ; cond]), f = 1 where std(e) == 0;
 *          e' = phi (e f) + (1 - phi) e, and the update runs on e'.  rescale: ONE fp32 word phi on the device, read when the kernel runs, set iff
 *          the bit is set; needs groups >= 2.  phi == 0 gives the bits of the call without the bit (finite inputs)
 * edit_params is set iff groups == 3.  Anything else: TF_E_ARG, the message names the entry and the rule; nothing is launched.
 * flags 0 and 2 launch the kernel instances of the entries above and return their bits.  With bit 2 it is still ONE launch: one block per
 * image, two-pass statistics (means first, then squared deviations) summed in a fixed order -- no atomics, and image k's result depends on
 * neither B nor the other images of the launch; an image's statistics are complete before any of its elements is written. */
int tf_sampler_tail_f32(void* latent, const void* eps, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* edit_params,
                        const void* x0_init, const void* mask, const void* rescale, int B, int C, int H, int W, int groups, unsigned flags, tfStream_t s);
int tf_sampler_tail_bf16(void* latent, const void* eps, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* edit_params,
                         const void* x0_init, const void* mask, const void* rescale, int B, int C, int H, int W, int groups, unsigned flags, tfStream_t s);

/* ---- SDXL vector conditioning (csrc/adm.hip; vision/unet.py, variants/sd.py::start(pooled=)): emb = time_embed(t) + label_emb(y) with
 * y = [pooled text | Fourier(original h, w, crop top, left, target h, w)].  Everything y-dependent runs in start(), outside the captured step.
 * dtype tags the 16-bit tensors; arguments are checked before the device is touched (TF_E_ARG, nothing written); plain stores, no atomics. */
/* out (R, P + 6 D), row r = [pooled[r, :P] | emb(ids[r, 0]) | .. | emb(ids[r, 5])]; emb(t) = [cos(t f_i) | sin(t f_i)], f_i = exp(-ln(max_period) i /
 * (D / 2)), i < D / 2: tf_timestep_embedding_*'s arithmetic for the scalar t at dim = D -- the same fp32 expression, one rounding -- so the D values
 * are the bits that entry writes for the timestep t.  pooled (R, P) 16-bit: its bits are copied.  ids (R, 6) fp32 on the device.  D even, >= 2 */
int tf_adm_vector_16(int dtype, void* out, const void* pooled, const void* ids_f32, int R, int P, int D, float max_period, tfStream_t s);
/* out (S R, E): out[s R + r, :] = round16(t_emb[s, :] + y_emb[r, :]) -- fp32 add, one rounding; t_emb (S, E), y_emb (R, E).  16-byte loads and
 * stores: E a positive multiple of 8, every tensor 16-byte aligned */
int tf_adm_emb_rows_16(int dtype, void* out, const void* t_emb, const void* y_emb, int S, int R, int E, tfStream_t s);
/* out (B, W) 16-bit: out[b, :] = src[idx[b], :], src (rows, W), idx B int32 ON THE DEVICE (the EOS positions of the pooled text vector:
 * vae/open_clip_text.py).  Bits are copied.  An index outside [0, rows) gives a row of zeros.  W a positive multiple of 8; out, src 16-byte aligned */
int tf_gather_rows_16(void* out, const void* src, const void* idx_i32, int B, int W, int rows, tfStream_t s);

/* ---- LoRA adapters (csrc/lora.hip; storage/lora.py, variants/sd.py:set_adapters): the reference has no adapters -- its weights come from
 * update_state alone (storage/checkpoint.py).  Every weight is a row matrix (N, Kd) of 16-bit elements: a Linear (out, in), a conv in KRSC
 * storage (K, R S C); an adapter of it is up (N, r) and down (r, Kd). */
typedef struct { const void* up; const void* down_t; int rp; float scale; } tfLoraEntry;
/* ONE launch merges up to 8 adapters into a fresh copy of a weight:
 *   dst[n, k] = round16(base[n, k] + sum_i scale_i * sum_j up_i[n, j] * down_i[j, k]),  16-bit tensors of `dtype`.
 * table: a HOST array of n_adapters tfLoraEntry, copied into the kernel arguments by the call (nothing is uploaded).  up_i is (N, rp_i) and
 * down_t_i the TRANSPOSED down (Kd, rp_i), both contiguous along the rank, the rank zero-padded to rp_i, a multiple of 32; both 16-byte aligned.
 * The inner sum runs on the 16-bit MFMA with an fp32 accumulator per adapter (products of two 16-bit values are exact in fp32), scale_i is applied
 * to the accumulator, the base is added in fp32 and the sum is rounded once.  scale_i == 0 contributes nothing whatever the adapter holds; with
 * every scale 0 dst has base's bits.  Any N, Kd >= 1; dst and base are distinct buffers, base is only read.  No atomics: deterministic */
int tf_lora_merge_16(int dtype, void* dst, const void* base, const void* table, int n_adapters, int N, int Kd, tfStream_t s);

/* ---- CLIP ViT image tower (csrc/vit.hip; vae/clip_vision.py, the image-prompt front end of the IP-Adapter): what a ViT needs beyond the text
 * tower's kernels (vae/encoder.py:36-81, ff/nn.py:25-34).  dtype tags every 16-bit tensor (TF_DTYPE_F16 / TF_DTYPE_BF16); all three check their
 * arguments before the device is touched (TF_E_ARG, the message names the entry), store with plain vector stores and use no atomics, so a graph
 * replay is bit-identical to the eager launch; every 16-bit tensor must be 16-byte aligned. */
/* The input edge: image_u8 (B, S, S, 3) uint8 -> out (B (S/P)^2, Kpad), the patch matrix the stride-P patch-embedding conv reads as a GEMM.  Row
 * (b, py, px); column ky 3P + kx 3 + c holds fmaf((float)u8, scale3[c], shift3[c]) -- fp32, rounded once to 16 bits -- of pixel (py P + ky, px P + kx),
 * channel c, so one patch row is 3P contiguous image bytes; columns 3 P^2 .. Kpad - 1 are zero.  scale3 / shift3: three floats each ON THE HOST (they
 * travel as kernel arguments; scale = 1 / (255 std), shift = -mean / std).  S % P == 0, Kpad % 8 == 0, Kpad >= 3 P^2, P <= 64.  With the (width, 3, P, P)
 * conv weight re-packed to that column order and zero-padded to Kpad, out . W^T is the bias-free convolution of the normalised image. */
int tf_vit_patchify_u8_16(int dtype, void* out, const void* image_u8, int B, int S, int P, int Kpad, const float* scale3, const float* shift3,
                          tfStream_t stream);
/* Token assembly + pre-LayerNorm in one launch: out (B, T, D) = LayerNorm(e) gamma + beta with e[b, 0] = class_emb + pos_emb[0] and
 * e[b, 1 + p] = patch_out[b, p] + pos_emb[1 + p] (patch_out (B, T - 1, D), class_emb (D), pos_emb (T, D)); e is kept in fp32 and never stored.
 * D a multiple of 8, <= 2560 (the register form of tf_layer_norm_f16, ff/layer_norm.py:8-49); statistics two-pass in fp32.  Profiled in family 3
 * (tf_vit_patchify_u8_16 and tf_gelu_erf_16: family 5). */
int tf_vit_embed_ln_16(int dtype, void* out, const void* patch_out, const void* class_emb, const void* pos_emb, const void* gamma, const void* beta,
                       int B, int T, int D, float eps, tfStream_t stream);
/* The exact GELU (storage/tensor.py:80-82 is the tanh form, ff/nn.py:25-34 the quick form): y = 0.5 x erfc(-x / sqrt 2) in fp32 -- the form that
 * does not cancel in the negative tail -- within 1 ulp of the 16-bit type of the correctly rounded value for every finite input.  y == x allowed. */
int tf_gelu_erf_16(int dtype, void* y, const void* x, long long n, tfStream_t stream);

/* ---- FreeU (csrc/freeu.hip; Si et al. 2023 as diffusers' apply_freeu / fourier_filter state it): in front of the channel concat of
 * vision/unet.py:72 -- cat(x, saved.pop()) -- in the first two decoder stages, the skip goes through a Fourier filter and the first half of x's
 * channels is scaled, inside the captured step. */
typedef struct { void* dst; const void* src; int B; int H; int W; int C; int scale_index; } tfFreeuEntry;
/* ONE launch for up to 8 NHWC (B,H,W,C) 16-bit tensors of `dtype`: dst_i = fourier_filter(src_i, threshold 1, scale s_i), s_i =
 * scales[scale_index_i] -- fftn over (H, W), the four bins (u, v) in {0, -1}^2 times s, ifftn, real part -- in its closed form: per (image,
 * channel) plane x, y = x + (s - 1) / (H W) sum_q S_q t_q with the twiddles t = (1, cos a, sin a, cos b, sin b, cos(a + b), sin(a + b)), a = 2 pi
 * i / H, b = 2 pi j / W, and the seven fp32 sums S_q = sum_ij x t_q, combined in a fixed order (no atomics: deterministic).  table: a HOST array of
 * n_entries tfFreeuEntry, copied into the kernel arguments by the call (a captured graph node owns its copy); C a positive multiple of 8, H >= 2,
 * W >= 2, H + W <= 256, every pointer 16-byte aligned -- an error naming the entry otherwise.  scales: fp32 ON THE DEVICE, read when the kernel
 * runs.  s_i == 1 leaves dst_i = src_i bit for bit (-0, infinities and NaN payloads included).  dst_i may be src_i */
int tf_freeu_skip_16(int dtype, const void* table, int n_entries, const void* scales_f32, tfStream_t s);
/* x (rows, C) 16-bit: dst[r, c] = round16(b * src[r, c]) for c < C / 2, b = scales[scale_index] read on the device: one fp32 multiply, one
 * rounding.  The second half of the channels is copied when dst != src and not touched when dst == src.  b == 1 copies the bits.  C a positive
 * multiple of 16; 16-byte aligned pointers */
int tf_freeu_backbone_16(int dtype, void* dst, const void* src, long long rows, int C, const void* scales_f32, int scale_index, tfStream_t s);

/* ---- ControlNet (csrc/control.hip; vision/controlnet.py): a second copy of the encoder half of vision/unet.py:51-76 whose 13 outputs are
 * added to what the UNet saves for its skip concats (vision/unet.py:72) and to its middle block's output, inside the captured step. */
typedef struct { void* dst; const void* skip; const void* residual; long long n; } tfControlEntry;
/* ONE launch for up to 16 entries: dst_i[k] = round16(fmaf(scales[i], residual_i[k], skip_i[k])), k < n_i, 16-bit tensors of `dtype`.  table: a
 * HOST array of n_entries tfControlEntry, copied into the kernel arguments by the call (nothing is uploaded; a captured graph node owns its
 * copy); n_i a positive multiple of 8, every pointer 16-byte aligned.  scales: n_entries fp32 ON THE DEVICE, read when the kernel runs -- a
 * strength written between two replays takes effect without a recapture.  scales[i] == 0 leaves dst_i = skip_i bit for bit (also where
 * residual_i is not finite).  dst_i may be skip_i.  No atomics: deterministic */
int tf_control_add_16(int dtype, const void* table, int n_entries, const void* scales_f32, tfStream_t s);
/* uint8 (B,H,W,3) -> 16-bit x / 255 in the same element order: the [0, 1] NHWC (B,3,H,W) hint of the ControlNet stem (not the VAE's
 * x / 127.5 - 1 of vae/vae.py:12-15); n = B*H*W*3 */
int tf_hint_from_u8_16(int dtype, void* out, const void* x_u8, long long n, tfStream_t s);

/* ---- concat-conditioned UNets (the encoder edges: csrc/img2img.hip): the SD-1.5 inpainting checkpoint (9 input channels [latent | mask | latent of the masked
 * image]) and InstructPix2Pix (8 input channels [latent | latent of the image to edit], three guidance branches) on the sampler above: the
 * CFG duplication of variants/sd.py:31 with the conditioning channels appended, the update of variants/sd.py:14-25 behind a three-branch
 * combine, and the encoder edges of vae/vae.py:12-15 that fill the conditioning buffer. */
/* tf_cfg_duplicate_* (variants/sd.py:31) for `groups` (2 or 3) copies with cond appended: latent (B,C,H,W) f32 NCHW, cond (B,Cc,H,W) f32 NCHW
 * -> x_out (groups*B, C+Cc, H, W) NHWC 16-bit; group g, image b = [latent[b] | cond[b]], the cond channels +0 where bit g of drop_bits is set
 * (bits at or above `groups` are ignored).
 * The latent channels are rounded as tf_cfg_duplicate_* rounds them */
int tf_cfg_concat_f16(void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, int groups, unsigned drop_bits, tfStream_t s);
int tf_cfg_concat_bf16(void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, int groups, unsigned drop_bits, tfStream_t s);
/* tf_cfg_sampler_step_* (variants/sd.py:14-25) with three branches: eps3 = [e0 ; e1 ; e2] (3B,C,H,W) NHWC 16-bit,
 * e = e0 + g_T (e2 - e1) + g_I (e1 - e0), g_T = step_params[3], g_I = edit_params[0]; edit_params: a device block of 4 fp32 words
 * (tf_set_step_params writes one).  Everything behind the combine as there: x0, x', the tag-1 noise, the x0 history */
int tf_cfg3_sampler_step_f32(void* latent, const void* eps3, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* edit_params,
                             int B, int C, int H, int W, tfStream_t s);
int tf_cfg3_sampler_step_bf16(void* latent, const void* eps3, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* edit_params,
                              int B, int C, int H, int W, tfStream_t s);
/* tf_image_from_u8_f16 (vae/vae.py:12-15 input) with a uint8 mask (B,H,W): out (B,3,H,W) NHWC fp16 = x / 127.5 - 1 where the mask byte is 0
 * (bit-identical to tf_image_from_u8_f16 there), exactly 0 where it is not -- the masked image the inpainting model is conditioned on */
int tf_image_from_u8_masked_f16(void* out, const void* image_u8, const void* mask_u8, int B, int H, int W, tfStream_t s);
/* tf_means_to_latent_f32 (vae/vae.py:12-15 output) into a conditioning buffer: means (B,4,H,W) fp16 NHWC -> channels [c_off, c_off + 4) of
 * cond (B,c_total,H,W) fp32 NCHW = scale * means.  Inpainting: scale 0.18215, c_off 1, c_total 5; edit: scale 1 (the unscaled mode), 0, 4 */
int tf_means_to_cond_f32(void* cond, const void* means, int B, int H, int W, float scale, int c_off, int c_total, tfStream_t s);

#ifdef __cplusplus
}
#endif
#endif
