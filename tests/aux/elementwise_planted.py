"""Inputs, references, fp32 emulations, budgets and case tables for the elementwise, layout and step kernels of csrc/elementwise.hip (host code,
numpy only).  tests/test_elementwise_planted_host.py checks every claim made here on the CPU; tests/test_gpu_elementwise_planted.py walks the
tables on the device.

INPUTS.  patterns(dtype): all 65536 bit patterns of the storage type.  long_input(n): element i is finite pattern number hash_index(i) --
i differs from i +- 8 (the neighbouring 16-byte vector slot of a lane) and from i +- span (the same lane's next grid-stride trip: 4194304
elements for the 16-byte kernels, 524288 for the scalar ones; a plain tiling of the patterns would repeat at both).  pos_code(shape): a finite
16-bit code per coordinate tuple that differs between neighbours along every axis and between the sources of one launch (salt): a transposed
index, a stale tile edge or a wrong source is a mismatch, not a near miss.  Outputs are pre-filled with a finite sentinel and end in a guard of
GUARD elements that must come back untouched.

REFERENCES.  Bit-exact (copies, single IEEE fp32 operations, conversions): the same one or two IEEE steps on the host -- an fp32 numpy operation,
then round-to-nearest-even to the storage type; NaN compares as NaN, everything else by bits.  rne16_f64 is an independent float64 rounding the
host test holds them against where double rounding cannot occur.  Budgeted (activations, GEGLU, softmaxes, timestep embedding, DDIM update):
float64 of the rounded inputs under  tol = half_ulp(|y| + A, dtype) + A  (16-bit outputs),  tol = A  (fp32 outputs),  A = K 2^-22 scale:
    activations   scale = 1 + |y|
    GEGLU         scale = (1 + |a|) (1 + |gelu(g)|)                         y = a gelu(g)
    softmax       scale = p (1 + |scale x + mask - max|), and A has 2^-126 added: v_exp_f32 returns 0 below the fp32 normal range
    embedding     scale = 1 + |t f|
    DDIM          scale = (1 + |x| + g (|e_u| + |e_c|)) / sqrt(a_t)
K is fixed by the EMULATION of the kernel's fp32 arithmetic, never by a device: the smallest integer for which the emulation stays within A / 2 on
every case of the tables, with every v_exp_f32 / v_rcp_f32 (and fp32 division) result moved +-1 fp32 step, every expf / logf / sinf / cosf result
+-2 steps, and every product-sum evaluated both fused and unfused (the library is built with -ffp-contract=fast).  The device gets twice the
emulation's worst error and no more.  Measured  max |emulation - reference| / (A at K = 1)  (the host test prints them):
    tf_silu_f16 0.688   tf_sigmoid_f16 0.386   tf_gelu_f16 0.667   tf_quick_gelu_f16 0.667   tf_silu_bf16 0.669        -> K_ACT = 2
    tf_geglu_f16 0.288                                                                                               -> K_GEGLU = 1
    tf_softmax_rows_f32 1.192   tf_softmax_mask_rows_f16 1.251   tf_softmax_mask_rows_f32in_f16 1.645                   -> K_SOFTMAX = 4
    tf_timestep_embedding_f16 6.004   tf_timestep_embedding_bf16 6.004                                                 -> K_EMBED = 13
    tf_cfg_ddim_step_f32 / step2 0.777   tf_cfg_ddim_step_bf16 0.761                                                   -> K_DDIM = 2

SOFTMAX PLANTING.  Row r's maximum sits at column (71 r) mod C = (7 r + 64 r) mod C: lane 7 r of a wave, and the wave moves on by one per row, so
with C >= 214 rows 0 .. 3 put it into each of the four waves' column classes ((i mod 256) / 64) -- (7 r) mod C alone stays below column 64 for
the 10 rows of the tables.  It lies at least 12 above everything else after scaling and masking, and in odd rows at least 92 above: a block that loses one wave's partial sum is
off by orders of magnitude, and one that loses a wave's partial maximum overflows exp there (a smaller gap cancels in the quotient)."""
import functools
import itertools

import numpy as np

from norm_planted import _pair_tree, fma, half_ulp, round16  # noqa: F401

F32, F64, U16 = np.float32, np.float64, np.uint16
GUARD = 64
SENT16 = {"fp16": 0xF753, "bf16": 0xC6EA}      # -30000 in both storage types: finite, and no budgeted reference comes near it
SENT32 = F32(-30000.0)
SENT8 = 0xA5
VEC_SPAN, SCALAR_SPAN = 4194304, 524288        # elements one trip of the capped grid covers: 2048 blocks x 256 lanes x 8 (16-byte kernels) or x 1
K_ACT, K_GEGLU, K_SOFTMAX, K_EMBED, K_DDIM = 2, 1, 4, 13, 2
F32_TINY = 2.0 ** -126                          # v_exp_f32 returns 0 below the fp32 normal range
TF_E_ARG = 10001


# ---- storage types ------------------------------------------------------------------------------------------------------------------------------
def to_f32(bits, dtype):
    bits = np.ascontiguousarray(bits, U16)
    return bits.view(np.float16).astype(F32) if dtype == "fp16" else (bits.astype(np.uint32) << 16).view(F32)


def to_bits(x, dtype):
    """fp32 -> storage bits, round-to-nearest-even (fp16 overflows to inf from 65520 up); NaN -> a NaN."""
    x = np.ascontiguousarray(x, F32)
    with np.errstate(over="ignore"):
        if dtype == "fp16":
            return x.astype(np.float16).view(U16)
    u = x.view(np.uint32)
    r = ((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) >> 16).astype(U16)
    return np.where(np.isnan(x), U16(0x7FC0), r)


def is_nan_bits(bits, dtype):
    b = np.asarray(bits).astype(np.uint32) & 0x7FFF
    return b > (0x7C00 if dtype == "fp16" else 0x7F80)


def same_bits(got, want, dtype):
    """elementwise: NaN matches NaN, everything else by bits (signed zeros and subnormals included)."""
    return (got == want) | (is_nan_bits(got, dtype) & is_nan_bits(want, dtype))


def same_f32(got, want):
    g, w = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    return (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))


def rne16_f64(x, dtype="fp16"):
    """float64 -> storage type by one round-to-nearest-even done in float64 arithmetic (independent of numpy's casts), as float64."""
    x = np.asarray(x, F64)
    mant, emin, top = (10, -14, 65520.0) if dtype == "fp16" else (7, -126, 2.0 ** 128 * (1 - 2.0 ** -9))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e = np.maximum(np.frexp(x)[1] - 1, emin)
        q = np.ldexp(1.0, e - mant)
        r = np.rint(x / q) * q
        r = np.where(np.abs(r) >= top, np.copysign(np.inf, x), r)
    return np.where(np.isfinite(x), r, x)


def patterns(dtype=None):
    return np.arange(65536, dtype=np.uint32).astype(U16)


@functools.lru_cache(maxsize=None)
def finite_patterns(dtype):
    p = patterns()
    f = p[np.isfinite(to_f32(p, dtype))]
    f.setflags(write=False)
    return f


def hash_index(i, L, salt=0):
    i = np.asarray(i, np.int64)
    return ((i + salt) * 40503 + (i >> 16) * 12345 + (i >> 19) * 101 + salt * 7717) % L


def long_input(n, dtype, salt=0):
    f = finite_patterns(dtype)
    return f[hash_index(np.arange(n, dtype=np.int64), len(f), salt)]


def moderate_bits(h):
    """28672 distinct fp16 patterns with 2^-10 <= |v| < 16 (never zero) from an integer h: arithmetic on them stays far inside the type."""
    h = np.asarray(h, np.int64) % 28672
    rest = h % 14336
    return (((h // 14336) << 15) | ((5 + rest // 1024) << 10) | (rest % 1024)).astype(U16)


CODE_MULT = (40503, 10007, 30011, 50021)


def pos_code(shape, salt=0, kind="fin", dtype="fp16"):
    """uint16 array of `shape` (up to 4 axes): code of the coordinates.  kind "fin": any finite pattern of dtype; "mod": moderate fp16 values."""
    idx = np.full(shape, 977 * salt + 11, np.int64)
    for ax, n in enumerate(shape):
        sh = [1] * len(shape)
        sh[ax] = n
        idx = idx + (np.arange(n, dtype=np.int64) * CODE_MULT[ax]).reshape(sh)
    if kind == "mod":
        return moderate_bits(idx)
    f = finite_patterns(dtype)
    return f[idx % len(f)]


def budget16(y, A, dtype):
    return half_ulp(np.abs(y) + A, dtype) + A


def step(x, k):
    """x (fp32) moved k fp32 steps (k > 0 up, k < 0 down)."""
    x = np.asarray(x, F32)
    y = x
    for _ in range(abs(k)):
        y = np.nextafter(y, F32(np.inf if k > 0 else -np.inf))
    return np.where((x == 0) | ~np.isfinite(x), x, y)          # an exact 0 or inf (exp2 of -+inf, an overflow) is not a rounded result


# ---- Group A: 16-bit unary and binary kernels ---------------------------------------------------------------------------------------------------
A_LENGTHS = (0, 1, 7, 8, 9, 2047, VEC_SPAN + 2048 + 5)       # the last: a second trip for some lanes only, and a 5-element tail
# (entry, kind, input type, output type, leading dtype tag or None)
A_ENTRIES = [
    ("tf_silu_f16", "silu", "fp16", "fp16", None), ("tf_sigmoid_f16", "sigmoid", "fp16", "fp16", None), ("tf_gelu_f16", "gelu", "fp16", "fp16", None),
    ("tf_quick_gelu_f16", "qgelu", "fp16", "fp16", None), ("tf_silu_bf16", "silu", "bf16", "bf16", None),
    ("tf_add_f16", "add", "fp16", "fp16", None), ("tf_add_16", "add", "fp16", "fp16", 0), ("tf_add_16", "add", "bf16", "bf16", 1),
    ("tf_convert_f16_to_bf16", "cvt", "fp16", "bf16", None), ("tf_convert_bf16_to_f16", "cvt", "bf16", "fp16", None),
]
ACTS = ("silu", "sigmoid", "gelu", "qgelu")
ULP_PAIRS = ((0, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))


def a_inputs(case, dtype):
    """(a, b) bits of a Group A case: "patterns" or a length.  b (add only): a permuted by a fixed odd multiplier / a second hash."""
    if case == "patterns":
        a = patterns()
        return a, a[(np.arange(65536, dtype=np.int64) * 40503) & 0xFFFF]
    return long_input(case, dtype), long_input(case, dtype, salt=1)


def act64(op, x):
    x = np.asarray(x, F64)
    with np.errstate(over="ignore", invalid="ignore"):
        if op == "silu":
            return x / (1.0 + np.exp(-x))
        if op == "sigmoid":
            return 1.0 / (1.0 + np.exp(-x))
        if op == "qgelu":
            return x / (1.0 + np.exp(-1.702 * x))
        assert op == "gelu"                                          # 0.5 x (1 + tanh u) = x sigmoid(2 u), u = sqrt(2 / pi) (x + 0.044715 x^3)
        return x / (1.0 + np.exp(-2.0 * np.sqrt(2.0 / np.pi) * (x + 0.044715 * x * x * x)))


def sig32(v, ue=0, ur=0):
    """sigmoid_f of common.h: v_rcp_f32(1 + v_exp_f32(-v log2 e)), the two results moved ue / ur fp32 steps."""
    with np.errstate(all="ignore"):
        t = (-v) * F32(1.4426950408889634)
        e = step(np.exp2(t.astype(F64)).astype(F32), ue)
        d = F32(1.0) + e
        return step((1.0 / d.astype(F64)).astype(F32), ur)


def emulate_act(op, x, ue=0, ur=0, fused=False):
    """act<OP> of k_unary in fp32 (before the store)."""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        if op == "silu":
            return x * sig32(x, ue, ur)
        if op == "sigmoid":
            return sig32(x, ue, ur)
        if op == "qgelu":
            return x * sig32(F32(1.702) * x, ue, ur)
        q = F32(0.044715) * x
        inner = fma(q, x, F32(1.0)) if fused else (F32(1.0) + q * x)
        u = (F32(0.7978845608) * x) * inner
        return x * sig32(F32(2.0) * u, ue, ur)


def act_variants(op):
    return [(ue, ur, f) for ue, ur in ULP_PAIRS for f in ((False, True) if op == "gelu" else (False,))]


@functools.lru_cache(maxsize=None)
def act_table(op, dtype):
    """(y64, A, tol, finite) over all 65536 patterns of dtype: the float64 reference and its budget; a long input looks its elements up here."""
    with np.errstate(invalid="ignore"):                              # (signalling NaN patterns)
        x = to_f32(patterns(), dtype).astype(F64)
    fin = np.isfinite(x)
    y = np.where(fin, act64(op, np.where(fin, x, 0.0)), np.nan)
    A = K_ACT * 2.0 ** -22 * (1.0 + np.abs(y))
    tol = budget16(np.where(fin, y, 0.0), np.where(fin, A, 0.0), dtype)
    return y, A, tol, fin


def check_act(op, dtype, xbits, gotbits):
    """(largest |got - ref| / tol, largest share of A used beyond the store rounding tol - A) over the finite inputs; asserts the non-finite rules (NaN -> NaN, sigmoid(+-inf) = 1 / 0 exactly, +inf -> +inf
    for the other three; what they return for -inf is 0 x inf and is not asserted)."""
    y, A, tol, fin = act_table(op, dtype)
    x = to_f32(xbits, dtype)
    got = to_f32(gotbits, dtype)
    nan_in = np.isnan(x)
    assert np.isnan(got[nan_in]).all(), f"{op} {dtype}: NaN in must give NaN out"
    pinf, ninf = x == np.inf, x == -np.inf
    if op == "sigmoid":
        assert (got[pinf] == 1.0).all() and (got[ninf] == 0.0).all(), "sigmoid(+-inf)"
    else:
        assert (got[pinf] == np.inf).all(), f"{op}(+inf)"
    f = fin[xbits]
    err = np.abs(got[f].astype(F64) - y[xbits[f]])
    assert not np.isnan(err).any(), f"{op} {dtype}: NaN out of a finite input"
    if not f.any():
        return 0.0, 0.0
    t, a = tol[xbits[f]], A[xbits[f]]
    return float((err / t).max()), max(0.0, float(((err - (t - a)) / a).max()))


def a_exact(kind, a, b, din, dout):
    """the bit-exact reference of add / cvt: one fp32 step, then RNE to the output type."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = to_f32(a, din) + to_f32(b, din) if kind == "add" else to_f32(a, din)
    return to_bits(v, dout)


# ---- Group B: fp32 casts and the decode tail ----------------------------------------------------------------------------------------------------
B_LENGTHS = (1, 255, 257, SCALAR_SPAN + 256 + 3)
B_ENTRIES = ("tf_cast_f16_to_f32", "tf_cast_f32_to_f16", "tf_scale_cast_f32_to_f16", "tf_scale_f32", "tf_image_to_u8")
B_SCALES = (F32(1.0), F32(1.0 / 0.18215))


@functools.lru_cache(maxsize=None)
def cast_inputs():
    """fp32 inputs of the fp32 -> fp16 casts: every finite fp16 value, the midpoint to its successor and the midpoint +- one fp32 step (both
    signs); 65504, 65520 and their fp32 neighbours; 2^-25 and its successor; fp32 subnormals; +-inf and NaN."""
    p = np.arange(0x7C00, dtype=np.uint32).astype(U16)
    v = p.view(np.float16).astype(F32)
    nxt = np.append(v[1:], F32(65536.0))
    mid = (v.astype(F64) + nxt.astype(F64)) / 2
    assert (mid.astype(F32).astype(F64) == mid).all()
    mid = mid.astype(F32)
    pos = np.concatenate([v, mid, step(mid, 1), step(mid, -1)])
    extra = np.array([65504.0, 65520.0, 2.0 ** -25, 1e-45, 2.0 ** -127, 2.0 ** -126 * (1 - 2.0 ** -23), 2.0 ** -149 * 3], F32)
    extra = np.concatenate([extra, step(extra, 1), step(extra, -1)])
    x = np.concatenate([pos, -pos, extra, -extra, np.array([np.inf, -np.inf, np.nan], F32)])
    x.setflags(write=False)
    return x


def b_input(entry, case):
    """the input of a Group B case: "all" (every pattern / the whole cast set) or a length (hashed out of that set)."""
    if entry in ("tf_cast_f16_to_f32", "tf_image_to_u8"):
        full = patterns()
        if entry == "tf_image_to_u8":
            full = full[~is_nan_bits(full, "fp16")]
    else:
        full = cast_inputs()
    return full if case == "all" else full[hash_index(np.arange(case, dtype=np.int64), len(full))]


def b_reference(entry, x, scale=None):
    with np.errstate(all="ignore"):
        if entry == "tf_cast_f16_to_f32":
            return to_f32(x, "fp16")
        if entry == "tf_cast_f32_to_f16":
            return to_bits(x, "fp16")
        if entry == "tf_scale_cast_f32_to_f16":
            return to_bits(x * F32(scale), "fp16")
        if entry == "tf_scale_f32":
            return x * F32(scale)
        assert entry == "tf_image_to_u8"                              # the fp32 formula of tests/test_img2img_host.py: ((x + 1) / 2 clipped) * 255, truncated
        v = (to_f32(x, "fp16") + F32(1.0)) * F32(0.5)
        return (np.minimum(np.maximum(v, F32(0.0)), F32(1.0)) * F32(255.0)).astype(np.uint8)


# ---- Group C: re-layouts and gathers ------------------------------------------------------------------------------------------------------------
TILE_ENTRIES = ("tf_nchw_f32_to_nhwc_f16", "tf_nhwc_f16_to_nchw_f32", "tf_nhwc_to_nchw_f16", "tf_nchw_to_nhwc_f16")
TILE_CASES = [(1, 1, 1), (2, 31, 33), (3, 32, 32), (2, 33, 65), (1, 8, 1025), (2, 320, 64)]                 # (N, C, HW)
TRANSPOSE_CASES = [((11,), (0,))] + [((3, 5, 7, 2), p) for p in itertools.permutations(range(4))] + [((9, 241, 243), (2, 0, 1))]
UPSAMPLE_CASES = [(1, 1, 1, 8), (2, 3, 5, 8), (2, 5, 3, 24), (1, 16, 16, 320), (2, 32, 32, 520)]            # (N, H, W, C): the last has 532480 vectors
CONCAT_CASES = [(1, 8, 8), (5, 8, 24), (7, 24, 8), (3, 320, 640), (2049, 1280, 768)]                       # (rows, Ca, Cb)
BIAS_NC_CASES = [(1, 1, 8), (3, 5, 24), (2, 7, 320), (2, 1025, 2048)]                                      # (N, HW, C)
GEGLU_CASES = [(1, 8), (5, 24), (77, 320), (2049, 2048)]                                                   # (rows, C)
IM2COL_CASES = [(2, 9, 7, 4, 3, 3, 1, 1, 40), (1, 9, 7, 4, 3, 3, 2, 1, 64), (2, 5, 6, 3, 2, 2, 1, 0, 16), (1, 8, 8, 4, 1, 1, 1, 0, 8)]   # (N,H,W,C,R,S,stride,pad,Kpad)
EMBED_CASES = [(10, 8, 15, 5), (100, 1024, 4100, 77)]                                                      # (vocab, D, tokens, T)
COLMAJOR_CASES = [(1, 1), (7, 5), (333, 77)]                                                               # (BT, OC)


def tile_case(entry, N, C, HW):
    """(input, expected output) of a 32 x 32-tile re-layout; fp32 sides hold the codes' values (exact in both types)."""
    if entry in ("tf_nchw_f32_to_nhwc_f16", "tf_nchw_to_nhwc_f16"):
        src = pos_code((N, C, HW))
        want = np.ascontiguousarray(src.transpose(0, 2, 1))
        return (to_f32(src, "fp16"), want) if entry == "tf_nchw_f32_to_nhwc_f16" else (src, want)
    src = pos_code((N, HW, C))
    want = np.ascontiguousarray(src.transpose(0, 2, 1))
    return (src, to_f32(want, "fp16")) if entry == "tf_nhwc_f16_to_nchw_f32" else (src, want)


def im2col_out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def im2col_bands(Ho):
    return [(0, Ho), (0, 1), (Ho - 1, Ho), (Ho // 3, Ho // 3 + max(1, Ho // 3)), (2, 2)]


def im2col_ref(x, R, S, stride, pad, Kpad, h0, h1, ignore_begin=False):
    """x (N, H, W, C) uint16 -> (N, h1 - h0, Wo, Kpad), k = (r S + s) C + c, zero padded."""
    N, H, W, C = x.shape
    Ho, Wo = im2col_out_hw(H, W, R, S, stride, pad)
    y = np.zeros((N, h1 - h0, Wo, Kpad), U16)
    for j, ho in enumerate(range(h0, h1)):
        hsrc = j if ignore_begin else ho
        for wo in range(Wo):
            for r in range(R):
                for s in range(S):
                    hi, wi = hsrc * stride - pad + r, wo * stride - pad + s
                    if 0 <= hi < H and 0 <= wi < W:
                        y[:, j, wo, (r * S + s) * C:(r * S + s + 1) * C] = x[:, hi, wi, :]
    return y


def add16(a_bits, b_bits):
    """fp16 + fp16 in fp32, RNE back: the bias / position adds."""
    return to_bits(to_f32(a_bits, "fp16") + to_f32(b_bits, "fp16"), "fp16")


def geglu_inputs(rows, C):
    return pos_code((rows, 2 * C), kind="mod")


def geglu_ref(xbits, C):
    x = to_f32(xbits, "fp16").astype(F64)
    a, g = x[:, :C], x[:, C:]
    gg = act64("gelu", g)
    y = a * gg
    A = K_GEGLU * 2.0 ** -22 * (1.0 + np.abs(a)) * (1.0 + np.abs(gg))
    return y, A, budget16(y, A, "fp16")


def emulate_geglu(xbits, C, ue=0, ur=0, fused=False):
    x = to_f32(xbits, "fp16")
    return x[:, :C] * emulate_act("gelu", x[:, C:], ue, ur, fused)


# ---- Group D: row softmaxes ---------------------------------------------------------------------------------------------------------------------
D_ENTRIES = ("tf_softmax_rows_f32", "tf_softmax_mask_rows_f16", "tf_softmax_mask_rows_f32in_f16")
D_C = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
D_ROWS = (5, 10)
D_MASKS = (None, "per_row", "wrap4", "one")
MARGIN = 12.0


def d_ld(C):
    return (C, -(-C // 8) * 8, C + 13)


def peak_col(r, C):
    return (71 * np.asarray(r)) % C


def mask_rows_of(mode, rows):
    return {None: 0, "per_row": rows, "wrap4": 4, "one": 1}[mode]


def d_cases(entry):
    """(rows, C, ld out, ld in, mask mode) of an entry.  "wrap4" runs under 10 rows: the mask wraps twice and a half."""
    out = []
    for C in D_C:
        for rows in D_ROWS:
            if entry == "tf_softmax_rows_f32":
                out.append((rows, C, C, C, None))
                continue
            for ldo in sorted(set(d_ld(C))):
                for ldi in ((ldo,) if entry == "tf_softmax_mask_rows_f16" else (C, C + 3)):
                    for mode in D_MASKS:
                        if mode != "wrap4" or rows == 10:
                            out.append((rows, C, ldo, ldi, mode))
    return out


def softmax_scale(entry):
    return 1.0 if entry == "tf_softmax_rows_f32" else 0.125


def softmax_mask(nrows, C, rows_total):
    """(nrows, C) fp32: multiples of 1/2 in [-4, 0] and -inf entries, 0 at the columns that hold some row's maximum; rows differ."""
    m, c = np.arange(nrows)[:, None], np.arange(C)[None, :]
    mask = -0.5 * ((m * 30011 + c * 50021 + 5) % 9).astype(F64)
    peaks = np.zeros(C, bool)
    peaks[peak_col(np.arange(rows_total), C)] = True
    mask = np.where(peaks[None, :], 0.0, np.where((m * 7 + c * 13) % 5 == 0, -np.inf, mask))
    return mask.astype(F32)


def softmax_input(entry, rows, C):
    """x (rows, C) as fp32 (fp16 values for tf_softmax_mask_rows_f16): scaled, row r peaks at peak_col(r) with 60 (|x| = 480 at scale 1/8);
    everything else lies 12.5 to 27.5 below in even rows and 96 to 120 below in odd rows -- exp(96) overflows fp32, so a block maximum that
    misses the peak's wave gives inf / inf there (a smaller gap cancels in the quotient and would go unnoticed)."""
    scale = softmax_scale(entry)
    r, c = np.arange(rows)[:, None], np.arange(C)[None, :]
    u = ((r * 40503 + c * 10007 + 13) % 4096) / 4096.0
    z = np.where(r % 2 == 0, 60.0 - 12.5 - 15.0 * u, -36.0 - 24.0 * u)
    z = np.where(c == peak_col(r, C), 60.0, z)
    x = (z / scale).astype(F32)
    return round16(x, "fp16") if entry == "tf_softmax_mask_rows_f16" else x


def softmax_ref(entry, x, mask, by_r=False):
    """(p, A, z - max) in float64.  mask: (mask_rows, C) or None, row r reads mask[r % mask_rows] (by_r: the mutant's mask[r])."""
    rows, C = x.shape
    z = softmax_scale(entry) * x.astype(F64)
    if mask is not None:
        z = z + mask[np.arange(rows) % (rows if by_r else mask.shape[0])].astype(F64)
    d = z - z.max(axis=1, keepdims=True)
    e = np.exp(d)
    p = e / e.sum(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        A = np.where(np.isfinite(d), K_SOFTMAX * 2.0 ** -22 * p * (1.0 + np.abs(d)) + F32_TINY, 0.0)
    return p, A, d


def emulate_softmax(entry, x, mask, fused=False, ue=0, ur=0, lose_wave=None):
    """k_softmax_rows / k_softmax_mask_rows_f16 in fp32 before the store.  lose_wave: the mutant whose block maximum leaves that wave's out."""
    rows, C = x.shape
    s = F32(softmax_scale(entry))
    x = x.astype(F32)
    with np.errstate(all="ignore"):
        if entry == "tf_softmax_rows_f32":
            v = x
        else:
            m = mask[np.arange(rows) % mask.shape[0]] if mask is not None else np.zeros_like(x)
            v = fma(s, x, m) if fused else (s * x + m)
        lanes = np.full((rows, -(-C // 256) * 256), -np.inf, F32)
        lanes[:, :C] = v
        wmax = lanes.reshape(rows, -1, 4, 64).max(axis=(1, 3))                       # per wave
        if lose_wave is not None:
            wmax[:, lose_wave] = -np.inf
        mx = wmax.max(axis=1, keepdims=True)
        t = (v - mx) * F32(1.4426950408889634)                                       # __expf = v_exp_f32(x log2 e)
        e = np.exp2(t.astype(F64)).astype(F32)
        e = step(np.where(e < F32(F32_TINY), F32(0.0), e), ue)
        pad = np.zeros((rows, lanes.shape[1]), F32)
        pad[:, :C] = e
        pad = pad.reshape(rows, -1, 256)
        acc = np.zeros((rows, 256), F32)
        for k in range(pad.shape[1]):
            acc = acc + pad[:, k]
        w = _pair_tree(acc.reshape(rows, 4, 64), ascending=False)
        tot = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        inv = step((1.0 / tot.astype(F64)).astype(F32), ur)
        return e * inv[:, None]


# ---- Group E: step glue -------------------------------------------------------------------------------------------------------------------------
COPY_NBYTES = (16, 16 * 255, 16 * (64 * 256 + 3))            # the grid is capped at 64 blocks of 256 lanes: the last loops
STEP_PARAMS = (981.0, 0.0046603, 0.0064, 7.5)
EMBED_DIMS = (2, 6, 320, 1280)                               # 1280: 640 frequencies for the block's 256 lanes
EMBED_T = (0.0, 1.0, 333.25, 999.0)
MAX_PERIOD = 10000.0
DDIM_CASES = [(1, 4, 1, 1), (3, 4, 5, 7), (2, 4, 8, 8), (2, 4, 257, 256)]     # (B, C, H, W): the last has 526336 elements
GUIDANCE = 7.5
DDIM_ENTRIES = ("tf_cfg_ddim_step_f32", "tf_cfg_ddim_step2_f32", "tf_cfg_ddim_step_bf16")


def sd_alphas():
    """(a_t, a_prev) of the first, a middle and the last step of the 50-step walk 981, 961, ... 1 of the SD schedule (scaled-linear betas)."""
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=F64) ** 2
    ac = np.cumprod(1.0 - betas)
    return [(F32(ac[981]), F32(ac[961])), (F32(ac[501]), F32(ac[481])), (F32(ac[1]), F32(1.0))]


def embed_ref(dim, t, dtype):
    half = dim // 2
    a = float(F32(t)) * np.exp(-np.log(MAX_PERIOD) * np.arange(half) / half)
    y = np.concatenate([np.cos(a), np.sin(a)])
    A = K_EMBED * 2.0 ** -22 * (1.0 + np.concatenate([np.abs(a), np.abs(a)]))
    return y, A, budget16(y, A, dtype)


def emulate_embed(dim, t, kl=0, ke=0, kt=0):
    """k_timestep_embedding in fp32 before the store: logf, expf and cosf / sinf moved kl / ke / kt fp32 steps."""
    half = dim // 2
    L = step(F32(np.log(F64(F32(MAX_PERIOD)))), kl)
    arg = ((-L) * np.arange(half).astype(F32)) / F32(half)
    f = step(np.exp(arg.astype(F64)).astype(F32), ke)
    a = F32(t) * f
    return np.concatenate([step(np.cos(a.astype(F64)).astype(F32), kt), step(np.sin(a.astype(F64)).astype(F32), kt)])


EMBED_VARIANTS = ((0, 0, 0), (2, 2, 2), (-2, -2, -2), (2, -2, 2), (-2, 2, -2), (2, 2, -2), (-2, -2, 2))


def ddim_inputs(B, C, H, W, dtype):
    """latent (B, C, HW) fp32 and e_u, e_c (B, HW, C) bits of dtype: three different moderate codes over (b, hw, c)."""
    HW = H * W
    lat = np.ascontiguousarray(to_f32(pos_code((B, HW, C), salt=0, kind="mod"), "fp16").transpose(0, 2, 1))
    eu = to_bits(to_f32(pos_code((B, HW, C), salt=1, kind="mod"), "fp16"), dtype)
    ec = to_bits(to_f32(pos_code((B, HW, C), salt=2, kind="mod"), "fp16"), dtype)
    return lat, eu, ec


def ddim_ref(lat, eu, ec, a_t, a_prev, dtype, nchw_eps=False):
    """float64 update of lat (B, C, HW); eps (B, HW, C).  nchw_eps: the mutant that reads eps at the latent's own (NCHW) index."""
    B, C, HW = lat.shape
    g = GUIDANCE
    u, c = to_f32(eu, dtype).astype(F64), to_f32(ec, dtype).astype(F64)
    if nchw_eps:
        u, c = u.reshape(B, C, HW), c.reshape(B, C, HW)
    else:
        u, c = u.transpose(0, 2, 1), c.transpose(0, 2, 1)
    x = lat.astype(F64)
    at, ap = float(a_t), float(a_prev)
    e = u + g * (c - u)
    y = np.sqrt(ap) * (x - np.sqrt(1 - at) * e) / np.sqrt(at) + np.sqrt(1 - ap) * e
    A = K_DDIM * 2.0 ** -22 * (1.0 + np.abs(x) + g * (np.abs(u) + np.abs(c))) / np.sqrt(at)
    return y, A


def emulate_ddim(lat, eu, ec, a_t, a_prev, dtype, fused=0, kd=0):
    """k_cfg_ddim in fp32.  fused: 0 = no contraction, 1 / 2 = every product-sum contracted (the last line either way round); kd: the
    division's result moved kd fp32 steps."""
    u, c = to_f32(eu, dtype).transpose(0, 2, 1), to_f32(ec, dtype).transpose(0, 2, 1)
    a_t, a_prev, g = F32(a_t), F32(a_prev), F32(GUIDANCE)
    s1, r, sp, dp = np.sqrt(F32(1.0) - a_t), np.sqrt(a_t), np.sqrt(a_prev), np.sqrt(F32(1.0) - a_prev)
    d = c - u
    e = fma(g, d, u) if fused else (u + g * d)
    num = fma(-s1, e, lat) if fused else (lat - s1 * e)
    px0 = step((num.astype(F64) / F64(r)).astype(F32), kd)
    if fused == 1:
        return fma(sp, px0, dp * e)
    if fused == 2:
        return fma(dp, e, sp * px0)
    return sp * px0 + dp * e


# ---- Group F: diagnosis aids --------------------------------------------------------------------------------------------------------------------
CHECKSUM_WORDS = (1, 255, SCALAR_SPAN + 300)
NONFINITE_BIG = SCALAR_SPAN + 77                              # words: an element past one trip of the capped grid


def checksum_ref(words, start=0):
    w = np.ascontiguousarray(words, np.uint32).astype(np.uint64)
    k = ((np.arange(len(w), dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) | np.uint64(1)
    with np.errstate(over="ignore"):
        return int((np.uint64(start) + (w * k).sum(dtype=np.uint64)) & np.uint64(0xFFFFFFFFFFFFFFFF))


def nonfinite_cases():
    """(name, is_f32, element count, index planted or None): fp16 counts are elements, so an odd one ends in half a word."""
    big = 2 * NONFINITE_BIG
    out = [("fp16 first", 0, 1000, 0), ("fp16 low half", 0, 1000, 500), ("fp16 high half", 0, 1000, 501), ("fp16 last of even", 0, 1000, 999),
           ("fp16 last of odd", 0, 1001, 1000), ("fp16 single", 0, 1, 0), ("fp16 past one trip", 0, big, big - 3), ("fp16 last of odd past one trip", 0, big + 1, big),
           ("fp32 first", 1, 1000, 0), ("fp32 middle", 1, 1000, 500), ("fp32 last", 1, 1001, 1000), ("fp32 past one trip", 1, NONFINITE_BIG, NONFINITE_BIG - 2),
           ("fp16 all finite", 0, 65537, None), ("fp32 all finite", 1, 65536, None)]
    return out


def nonfinite_array(is_f32, n, at, bad):
    """bytes of the array: all-finite patterns (subnormals and +-65504 included), `bad` ("inf" / "nan") planted at element `at`."""
    if is_f32:
        a = to_f32(finite_patterns("fp16")[np.arange(n) % 63488], "fp16") * F32(3.0e33)       # finite fp32 up to 2e38, fp32 subnormals too
        a[::7] = to_f32(finite_patterns("bf16")[(np.arange(n) % 65280)], "bf16")[::7]
        assert np.isfinite(a).all()
        if at is not None:
            a[at] = np.inf if bad == "inf" else np.nan
        return a
    a = finite_patterns("fp16")[np.arange(n) % 63488].copy()
    if at is not None:
        a[at] = 0xFC00 if bad == "inf" else 0x7E01
    return a
