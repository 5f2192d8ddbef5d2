"""Planted-statistics inputs for the GroupNorm / LayerNorm kernels of csrc/norm.hip, their float64 answer, a numpy emulation of the kernels' own fp32
arithmetic, and the error budget the GPU test holds the kernels to (host code, numpy only).  tests/test_norm_planted_host.py checks every claim made
here on the CPU; tests/test_gpu_norm_planted.py walks the case tables below on the device.

INPUTS.  Seeded-normal inputs of one distribution give every (image, group) and every row the same statistics to about 1e-2: a kernel that
normalises a slice with its neighbour's statistics passes.  Here slice s (s = n (G + 3) + g for GroupNorm, s = the row for LayerNorm) holds
x = mu_s + sigma_s z, rounded to the storage type, with z standardised per slice, sigma_s = 2^((3 s + 1) mod 5 - 2) in [1/4, 4] and
mu_s = sigma_s R k_s / 16, k_s walking the 32 non-zero integers of [-16, 16] with stride 7: adjacent groups, adjacent images and any 32
consecutive rows (a wave holds at most 8) differ, and no slice has |mu| < sigma R / 16 -- so a lost tail (last pixel chunk, last channel vector)
shifts the slice's mean by (lost share) x mu.  gamma walks the 32 non-zero multiples of 1 / 8 in [-2, 2] with stride 5, beta 61 multiples of 1 / 8
in [-3.75, 3.75] with stride 11 (exact in float16 and bfloat16; rolled by 8 channels both differ at every channel).

REFERENCE.  The float64 norm of the ROUNDED inputs (biased variance, eps = float32(1e-5)), affine and SiLU in float64; a concat is normalised as
the concatenation.  The apply entries that take partials are held to the float64 norm under the statistics those partials state (partials():
float64 sums per chunk, rounded to fp32 -- what the entry is given is its contract).

BUDGET, per element, as a function of the float64 reference y:  tol = half_ulp(|y| + A) + A,
  half_ulp(v) = 2^-11 2^floor(log2 v) float16 (floor 2^-25, the subnormal spacing), 2^-8 2^floor(log2 v) bfloat16: the store rounding of the type
      (10 / 7 stored mantissa bits), taken at the largest magnitude the unrounded result can have -- it differs from the value at |y| only for
      elements within A of a power of two;
  A = K 2^-22 (1 + R) (1 + |y|) max|gamma|  [+ 2^-22 |y| behind SiLU]:  the fp32 arithmetic.  K = K_ARITH + K_STATS where the kernel computes
      its own statistics (tf_group_norm_*, tf_layer_norm_*), K = K_ARITH where the statistics arrive as fp32 partials (the apply entries).
The constants are fixed by the EMULATION, never by a device: each is the smallest integer for which the emulation's largest error is at most
A / 2 on every input of the tables (so the device gets twice the emulation's error, and no more).  Measured with emulate_* below, as
max |emulation - reference| / (A at K = 1), over all cases, variants and both storage types (tests/test_norm_planted_host.py prints them per case):
    apply entries on host partials:     0.43  (200, 2048, 33, 32) float16      -> K_ARITH = 1            (0.43 <= 1 / 2)
    GroupNorm with its own statistics:  5.86  (400, 2048, 33, 32) float16 affine -> K_ARITH + K_STATS = 12 (5.86 <= 12 / 2)
    LayerNorm (two-pass statistics):    0.28  (8195, 328) bfloat16 affine       -> far inside the same K = 12
The SiLU term: the device sigmoid is v_rcp_f32(1 + v_exp_f32(-1.4427 x)), two instructions of 1 ulp each (2^-23 relative) -- 2^-22 |y| is
added for them explicitly; emulate_silu with ulp = +-1 (both results moved one fp32 step the same way) stays within A / 2 + 2^-22 |y| on every
SiLU input (host test).

THE R LIMIT.  The statistics are single-pass: the variance is E[x^2] - mean^2 from fp32 sums, so its error grows as R^2 where the budget grows as R.
cancellation_limit() walks R = 16, 32, 64, ... at (2, 64, 289, 8) until the emulation exceeds A / 2 (or the type can no longer hold the
input: spacing at R sigma above sigma / 4).  Measured: float16 meets A / 2 up to R = 32 (0.92 of A / 2, absolute error 2.0e-4) and misses it
at R = 64 (1.53 x A / 2, 7.7e-4); bfloat16 meets it at its plantable limit R = 32 (0.28 of A / 2)."""
import functools
import math

import numpy as np

EPS = float(np.float32(1e-5))
R_MAIN = 16
K_ARITH, K_STATS = 1.0, 11.0
MANTISSA = {"fp16": 10, "bf16": 7}
SENTINEL = -30000.0          # finite in both storage types, far from every reference value (|y| < 100)
GN_MAX_CHUNKS, GN_APPLY_PPT = 64, 4
F32 = np.float32


# ---- storage types ------------------------------------------------------------------------------------------------------------------------------
def round16(x, dtype):
    """x rounded to the storage type ("fp16" / "bf16", round-to-nearest-even), as float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "fp16":
        return x.astype(np.float16).astype(np.float32)
    assert dtype == "bf16", dtype
    u = x.view(np.uint32)
    return ((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)).view(np.float32)


def half_ulp(v, dtype):
    """half the spacing of the storage type at magnitude v (float64)."""
    v = np.abs(np.asarray(v, np.float64))
    e = np.where(v > 0, np.frexp(v)[1] - 1, -1000)                  # floor(log2 v)
    if dtype == "fp16":
        return np.ldexp(1.0, np.maximum(e - 11, -25))
    return np.ldexp(1.0, np.maximum(e - 8, -140))


def budget(y, dtype, R, gmax=1.0, silu=False, stats=True):
    """(tol, A) per element of the float64 reference y (module docstring)."""
    ay = np.abs(y)
    A = (K_ARITH + (K_STATS if stats else 0.0)) * 2.0 ** -22 * (1.0 + R) * (1.0 + ay) * gmax
    if silu:
        A = A + 2.0 ** -22 * ay
    return half_ulp(ay + A, dtype) + A, A


def a_unit(y, R, gmax=1.0):
    """A at K = 1 without the SiLU term: the unit the emulation's error is quoted in."""
    return 2.0 ** -22 * (1.0 + R) * (1.0 + np.abs(y)) * gmax


# ---- launch geometry: a copy of gn_geometry / gn_batches / ln_instance of csrc/norm.hip (the GPU test checks it against the library's answers) ----
def gn_geometry(N, HW, C):
    cv = C // 8
    rpb = 1 if cv >= 256 else 256 // cv
    if rpb > HW:
        rpb = max(HW, 1)
    p = rpb * 8
    c = -(-HW // p)
    if c > GN_MAX_CHUNKS:
        c = GN_MAX_CHUNKS
        p = -(-HW // c)
        p = -(-p // rpb) * rpb
        c = -(-HW // p)
    ablocks = -(-HW // (rpb * GN_APPLY_PPT))
    nb = 1
    while nb < 8 and -(-ablocks // (2 * nb)) * N >= 768:
        nb *= 2
    return dict(rpb=rpb, chunks=c, pix_per_chunk=p, apply_blocks=ablocks, nbatch=nb, threads=cv * rpb)


LN_INSTANCES = {1: "64", 2: "8", 3: "16", 4: "32", 5: "any_wave", 6: "any_block"}       # tfLayerNormInstance
LN_LANES = {"64": 64, "8": 8, "16": 16, "32": 32, "any_wave": 64, "any_block": 256}     # lanes that share one row


def ln_instance(rows, C):
    if C % 8 or C > 64 * 8 * 5:
        return "any_wave" if C <= 4096 else "any_block"
    cv = C // 8
    if rows < 8192 or cv > 32 * 5:
        return "64"
    return "8" if cv <= 40 else "16" if cv <= 80 else "32"


# ---- the case tables ------------------------------------------------------------------------------------------------------------------------------
# GroupNorm through tf_group_norm_f16 / _bf16: (form, N, C1, C2, HW, G).  gn_form_holds says what the geometry must show for the case to be the form.
GN_CASES = [
    ("rpb_clipped", 3, 64, 0, 1, 8), ("rpb_clipped", 3, 64, 0, 3, 8),
    ("padded_block", 2, 40, 0, 70, 4),          # 5 x 51 = 255 threads; 10 channels to a group: a 16-B vector straddles two groups
    ("cpg10", 2, 320, 0, 70, 32),               # the UNet's 320 / 32
    ("two_chunks", 2, 64, 0, 289, 8),           # 256 + 33 pixels: the guards of the 4-way unrolled loop
    ("chunk_cap", 2, 2048, 0, 529, 32),         # 67 chunks of 8 pixels asked, 59 of 9 run
    ("nbatch2", 200, 2048, 0, 33, 32), ("nbatch4", 300, 2048, 0, 33, 32), ("nbatch8", 400, 2048, 0, 33, 32),   # 9 units of 4 pixels: the last block ragged
    ("concat_seam", 2, 24, 40, 70, 4),          # group 1 = channels 16 .. 31 lies on both sides of the seam at 24
    ("concat_seam", 2, 1280, 640, 16, 32),      # the UNet's 1280 | 640: group 21 = channels 1260 .. 1319
]
GN_VARIANTS = [(False, False), (True, False), (True, True)]       # (affine, SiLU): plain, GroupNorm, GroupNorm + SiLU as the UNet runs it
CANCELLATION_SHAPE = ("two_chunks", 2, 64, 0, 289, 8)


def gn_form_holds(form, geo, HW, C1, C2, G):
    C = C1 + C2
    cpg = C // G
    if form == "rpb_clipped":
        return geo["rpb"] == HW < 256 // (C // 8)
    if form == "padded_block":
        return geo["threads"] % 8 != 0 and cpg % 8 != 0
    if form == "cpg10":
        return cpg == 10
    if form == "two_chunks":
        return geo["chunks"] == 2 and HW % geo["pix_per_chunk"] != 0 and (HW % geo["pix_per_chunk"]) % (4 * geo["rpb"]) != 0
    if form == "chunk_cap":
        return -(-HW // (8 * geo["rpb"])) > GN_MAX_CHUNKS >= geo["chunks"] > 1 and geo["pix_per_chunk"] > 8 * geo["rpb"]
    if form.startswith("nbatch"):
        per_block = GN_APPLY_PPT * geo["rpb"] * geo["nbatch"]
        return geo["nbatch"] == int(form[6:]) and HW % per_block != 0 and -(-HW // per_block) > 1
    if form == "concat_seam":
        return C2 > 0 and C1 % cpg != 0
    raise KeyError(form)


# apply entries on host partials: (entry, N, C1, C2, HW, G, groups1, groups2, chunks, chunks2); entry "apply" = tf_group_norm_apply_16,
# "cat" = tf_group_norm_apply_cat_16, "apply2" = tf_group_norm_apply2_f16 (float16 only).  The fold reads 64 chunks per round: 65 and 4096 loop.
APPLY_CASES = [
    ("apply", 2, 64, 0, 70, 8, 8, 0, 1, 0), ("apply", 2, 64, 0, 70, 8, 8, 0, 8, 0), ("apply", 2, 64, 0, 70, 8, 8, 0, 65, 0), ("apply", 2, 64, 0, 70, 8, 8, 0, 4096, 0),
    ("cat", 2, 64, 32, 70, 8, 16, 8, 3, 70),        # mr = 3 sub-groups of 4 channels to a group of 12: group 5 = sub-groups 15 | 16, 17 straddles the tables
    ("cat", 2, 64, 64, 70, 4, 16, 16, 70, 3),       # mr = 8
    ("apply2", 2, 64, 64, 70, 4, 4, 4, 3, 70),      # the equal split: mr = 2
    ("apply", 200, 2048, 0, 33, 32, 32, 0, 8, 0),   # nbatch 2
]


def apply_rows():
    """APPLY_CASES x storage type (tf_group_norm_apply2_f16 is a float16 entry)."""
    return [c + (d,) for c in APPLY_CASES for d in ("fp16", "bf16") if not (c[0] == "apply2" and d == "bf16")]


# 8-bit outputs (float16 input), block-scaled and scale 1, on host partials at nbatch 2: a single source and the mr = 3 pair
GN8_CASES = [
    ("apply", 200, 2048, 0, 33, 32, 32, 0, 8, 0),
    ("cat", 384, 64, 32, 253, 8, 16, 8, 3, 70),
]
# LayerNorm through tf_layer_norm_f16 / _bf16: (form, rows, C)
LN_CASES = [
    ("64", 5, 8), ("64", 7, 2552), ("64", 3, 2560), ("64", 8195, 1288),
    ("8", 8195, 8), ("8", 8195, 320), ("16", 8195, 328), ("16", 8195, 640), ("32", 8195, 648), ("32", 8195, 1280),
    ("any_wave", 9, 10), ("any_wave", 9, 2568), ("any_wave", 9, 4095), ("any_block", 3, 4097), ("any_block", 3, 4104),
]
LN8_CASES = [("8", 8195, 320), ("16", 8195, 640), ("32", 8195, 1280)]       # tf_layer_norm_fp8 / _mx8: the forms whose lane quads differ


# ---- planted parameters -------------------------------------------------------------------------------------------------------------------------
def check_plantable(R, dtype):
    """The storage type must still resolve the slice's spread around its mean: spacing at R sigma at most sigma / 4."""
    assert R >= 1 and R == 2 ** round(math.log2(R)), f"R = {R} is not a power of two"
    assert R * 2.0 ** -MANTISSA[dtype] <= 0.25, f"cannot plant R = {R} in {dtype}: the spacing at R sigma exceeds sigma / 4"


def slice_params(s, R):
    """(mu, sigma) of slice number s (int array)."""
    s = np.asarray(s, np.int64)
    sigma = np.exp2(((3 * s + 1) % 5 - 2).astype(np.float64))
    k = (7 * s + 3) % 32 - 16
    k = np.where(k >= 0, k + 1, k)
    return sigma * (R * k / 16.0), sigma


def affine(C):
    c = np.arange(C, dtype=np.int64)
    k = (5 * c + 7) % 32 - 16
    gamma = np.where(k >= 0, k + 1, k) / 8.0
    beta = ((11 * c + 5) % 61 - 30) / 8.0
    return gamma.astype(np.float32), beta.astype(np.float32)


def _standardise(z, axes):
    z = z - z.mean(axis=axes, keepdims=True)
    sd = np.sqrt((z * z).mean(axis=axes, keepdims=True))
    return z / np.where(sd > 0, sd, 1.0)


@functools.lru_cache(maxsize=2)
def _gn_raw(N, C, HW, G, R):
    """mu_s + sigma_s z before the storage rounding (float32; both storage types round the same draw), mu and sigma (N, G)."""
    cpg = C // G
    n, g = np.meshgrid(np.arange(N), np.arange(G), indexing="ij")
    mu, sigma = slice_params(n * (G + 3) + g, R)
    pair = mu + 1j * sigma         # neighbours are distinct: adjacent groups and adjacent images (with wrap-around, as the mutants roll)
    assert (G == 1 or (pair != np.roll(pair, -1, axis=1)).all()) and (N == 1 or (pair != np.roll(pair, -1, axis=0)).all()), "neighbouring slices share their statistics"
    v = np.empty((N, HW, C), np.float32)
    rng = np.random.default_rng([23, N, C, HW, G])
    step = max(1, (1 << 22) // (HW * C))
    for n0 in range(0, N, step):
        z = rng.standard_normal((min(step, N - n0), HW, G, cpg), dtype=np.float32).astype(np.float64)
        if HW * cpg > 1:
            z = _standardise(z, (1, 3))
        v[n0:n0 + step] = (mu[n0:n0 + step, None, :, None] + sigma[n0:n0 + step, None, :, None] * z).reshape(-1, HW, C)
    return v, mu, sigma


@functools.lru_cache(maxsize=2)
def gn_input(N, C, HW, G, dtype, R=R_MAIN):
    """x (N, HW, C) float32 holding values of the storage type (NHWC, read-only), mu and sigma (N, G)."""
    check_plantable(R, dtype)
    v, mu, sigma = _gn_raw(N, C, HW, G, R)
    x = round16(v, dtype)
    for a in (x, mu, sigma):
        a.setflags(write=False)
    return x, mu, sigma


@functools.lru_cache(maxsize=3)
def ln_input(rows, C, dtype, R=R_MAIN):
    check_plantable(R, dtype)
    mu, sigma = slice_params(np.arange(rows), R)
    pair = mu + 1j * sigma
    for d in range(1, 8):                                   # rows that share a wave (at most 8) are distinct
        assert rows <= d or (pair[d:] != pair[:-d]).all(), "rows of one wave share their statistics"
    z = _standardise(np.random.default_rng([29, rows, C]).standard_normal((rows, C)), (1,))
    x = round16(mu[:, None] + sigma[:, None] * z, dtype)
    for a in (x, mu, sigma):
        a.setflags(write=False)
    return x, mu, sigma


# ---- float64 references -------------------------------------------------------------------------------------------------------------------------
def silu64(y):
    with np.errstate(over="ignore"):                          # (a mutant's output may be far out: exp overflows to inf, the quotient is -0)
        return y / (1.0 + np.exp(-y))


def gn_stats64(x, G, keep=None, count=None):
    """(mean, var) (n, G) of x (n, HW, C) in float64, biased variance.  keep: sum over the first `keep` pixels only; count: pixels the sums are
    divided by (the mutants lose a chunk or divide by a padded count)."""
    n, HW, C = x.shape
    xs = x[:, :HW if keep is None else keep].astype(np.float64).reshape(n, -1, G, C // G)
    cnt = float((HW if count is None else count) * (C // G))
    mean = xs.sum(axis=(1, 3)) / cnt
    var = np.maximum((xs * xs).sum(axis=(1, 3)) / cnt - mean * mean, 0.0) if (keep is not None or count is not None) else \
        ((xs - mean[:, None, :, None]) ** 2).sum(axis=(1, 3)) / cnt
    return mean, var


def stats_from_partials(part, HW, cpg):
    """(mean, var) (n, G) stated by partials (n, chunks, G, 2): the float64 fold k_gn_apply does."""
    S = part.astype(np.float64).sum(axis=1)
    cnt = float(HW * cpg)
    mean = S[..., 0] / cnt
    return mean, np.maximum(S[..., 1] / cnt - mean * mean, 0.0)


def gn_apply64(x, mean, var, G, gamma=None, beta=None, silu=False):
    """x (n, HW, C) normalised with the given (n, G) statistics, as y = x a + b with the per-(image, channel) coefficients in float64."""
    cpg = x.shape[2] // G
    a = np.repeat(1.0 / np.sqrt(var + EPS), cpg, axis=1)
    b = -np.repeat(mean, cpg, axis=1) * a
    if gamma is not None:
        a, b = a * gamma.astype(np.float64), b * gamma.astype(np.float64) + beta.astype(np.float64)
    y = x * a[:, None, :] + b[:, None, :]
    return silu64(y) if silu else y


def gn_ref64(x, G, gamma=None, beta=None, silu=False):
    mean, var = gn_stats64(x, G)
    return gn_apply64(x, mean, var, G, gamma, beta, silu)


def ln_stats64(x):
    x = x.astype(np.float64)
    mean = x.mean(axis=1)
    return mean, ((x - mean[:, None]) ** 2).mean(axis=1)


def ln_apply64(x, mean, var, gamma=None, beta=None):
    y = (x.astype(np.float64) - mean[:, None]) / np.sqrt(var + EPS)[:, None]
    return y * gamma.astype(np.float64) + beta.astype(np.float64) if gamma is not None else y


def ln_ref64(x, gamma=None, beta=None):
    return ln_apply64(x, *ln_stats64(x), gamma, beta)


def chunk_bounds(HW, chunks):
    """Uneven pixel boundaries of `chunks` chunks (chunks > HW: most are empty) -- the apply entries take any partition."""
    b = np.floor(HW * (np.arange(chunks + 1) / chunks) ** 1.5).astype(np.int64)
    b[-1] = HW
    return b


def partials(x, G, chunks):
    """Per-chunk (sum, sum of squares) of x (n, HW, C) per group, computed in float64 and rounded to fp32: the [N][chunks][G][2] layout of norm.hip."""
    n, HW, C = x.shape
    b = chunk_bounds(HW, chunks)
    xs = x.astype(np.float64).reshape(n, HW, G, C // G)
    out = np.zeros((n, chunks, G, 2), np.float64)
    lo, hi = b[:-1], b[1:]
    for k in np.nonzero(hi > lo)[0]:
        seg = xs[:, lo[k]:hi[k]]
        out[:, k, :, 0] = seg.sum(axis=(1, 3))
        out[:, k, :, 1] = (seg * seg).sum(axis=(1, 3))
    return out.astype(np.float32)


def cat_stats(part1, part2, HW, sub, mr, wrong_table=False):
    """(mean, var) (n, G) of the concat from the two sources' sub-group partials: group g = sub-groups [mr g, mr g + mr) of the list [x's | x2's].
    wrong_table: the mutant that looks every sub-group up in x's table."""
    s1, s2 = part1.astype(np.float64).sum(axis=1), part2.astype(np.float64).sum(axis=1)
    if wrong_table:
        s2 = s1[:, np.arange(s2.shape[1]) % s1.shape[1]]
    S = np.concatenate([s1, s2], axis=1)
    n, L, _ = S.shape
    S = S.reshape(n, L // mr, mr, 2).sum(axis=2)
    cnt = float(HW * sub * mr)
    mean = S[..., 0] / cnt
    return mean, np.maximum(S[..., 1] / cnt - mean * mean, 0.0)


# ---- emulation of the kernels' fp32 arithmetic ---------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """fp32 fused multiply-add (the build contracts a * b + c): the product of two fp32 values is exact in float64."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _pair_tree(s, ascending=True):
    """xor-shuffle tree over the last axis: o = 1, 2, 4, ... (ascending) pairs neighbours first, o = n / 2, ... 1 pairs the halves first."""
    while s.shape[-1] > 1:
        h = s.shape[-1] // 2
        s = (s[..., 0::2] + s[..., 1::2]) if ascending else (s[..., :h] + s[..., h:])
    return s[..., 0]


def emulate_gn_partials(x, G, geo):
    """k_gn_stats on x (n, HW, C) float32: each thread adds its pixels per channel (sum, and sum of squares by fma), 8 lanes walk the group's
    RPB x cpg (row-thread, channel) pairs with stride 8, then the xor tree.  -> (n, chunks, G, 2) float32."""
    n, HW, C = x.shape
    rpb, chunks, ppc = geo["rpb"], geo["chunks"], geo["pix_per_chunk"]
    cpg = C // G
    iters = ppc // rpb
    xp = np.zeros((n, chunks * ppc, C), F32)
    xp[:, :HW] = x
    xp = xp.reshape(n, chunks, iters, rpb, C)
    s = np.zeros((n, chunks, rpb, C), F32)
    ss = np.zeros((n, chunks, rpb, C), F32)
    for i in range(iters):
        f = xp[:, :, i]
        s = s + f
        ss = fma(f, f, ss)
    out = np.empty((n, chunks, G, 2), F32)
    npairs = rpb * cpg
    rounds = -(-npairs // 8)
    for j, acc in enumerate((s, ss)):
        a = np.zeros((n, chunks, G, rounds * 8), F32)
        a[..., :npairs] = acc.reshape(n, chunks, rpb, G, cpg).transpose(0, 1, 3, 2, 4).reshape(n, chunks, G, npairs)
        a = a.reshape(n, chunks, G, rounds, 8)
        S = np.zeros((n, chunks, G, 8), F32)
        for r in range(rounds):
            S = S + a[..., r, :]
        out[..., j] = _pair_tree(S)
    return out


def emulate_silu(f, ulp=0):
    """silu_f of common.h in fp32: x * rcp(1 + exp2(-x * log2 e)).  ulp = +-1 moves the exp2 and the reciprocal one fp32 step that way (the two
    instructions are accurate to 1 ulp)."""
    t = (-f * F32(1.4426950408889634)).astype(F32)
    e = np.exp2(t.astype(np.float64)).astype(F32)
    if ulp:
        e = np.nextafter(e, F32(np.inf if ulp > 0 else 0.0))
    d = (F32(1.0) + e).astype(F32)
    r = (1.0 / d.astype(np.float64)).astype(F32)
    if ulp:
        r = np.nextafter(r, F32(np.inf if ulp > 0 else 0.0))
    return (f * r).astype(F32)


def emulate_gn_apply(x, mean, var, G, gamma=None, beta=None, silu=False, ulp=0):
    """k_gn_apply behind its fp64 fold: mean and rstd rounded to fp32, a = rstd gamma, b = beta - mean a, y = x a + b (fp32, before the store)."""
    n, HW, C = x.shape
    cpg = C // G
    m32 = np.repeat(mean.astype(F32), cpg, axis=1)[:, None, :]
    r32 = np.repeat((1.0 / np.sqrt(var + float(F32(EPS)))).astype(F32), cpg, axis=1)[:, None, :]
    gm = gamma.astype(F32) if gamma is not None else F32(1.0)
    bt = beta.astype(F32) if beta is not None else F32(0.0)
    a = (r32 * gm).astype(F32)
    b = fma(-m32, a, bt)
    f = fma(x, a, b)
    return emulate_silu(f, ulp) if silu else f


def emulate_group_norm(x, G, geo, gamma=None, beta=None, silu=False, ulp=0):
    part = emulate_gn_partials(x, G, geo)
    return emulate_gn_apply(x, *stats_from_partials(part, x.shape[1], x.shape[2] // G), G, gamma, beta, silu, ulp)


def emulate_layer_norm(x, form, gamma=None, beta=None):
    """k_layer_norm<LPR> / k_layer_norm_any on x (rows, C) float32, two-pass: each lane adds its elements in order, then the shuffle tree
    (ascending offsets in k_layer_norm, descending in wave_sum; a block adds its four waves in order)."""
    rows, C = x.shape
    L = LN_LANES[form]
    e = np.arange(C)
    if C % 8 == 0:
        lane, pos = (e // 8) % L, (e // 8) // L * 8 + e % 8
    else:
        lane, pos = e % L, e // L
    P = int(pos.max()) + 1
    gather = np.full((L, P), -1, np.int64)
    gather[lane, pos] = e

    def reduce(term):
        acc = np.zeros((rows, L), F32)
        for p in range(P):
            col = gather[:, p]
            ok = col >= 0
            acc[:, ok] = term(acc[:, ok], x[:, col[ok]])
        if form == "any_block":
            w = _pair_tree(acc.reshape(rows, 4, 64), ascending=False)
            return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        return _pair_tree(acc, ascending=form not in ("any_wave",))
    mean = (reduce(lambda a, v: a + v) / F32(C)).astype(F32)

    def sq(a, v):
        d = (v - mean[:, None]).astype(F32)
        return fma(d, d, a)
    q = reduce(sq)
    arg = ((q / F32(C)).astype(F32) + F32(EPS)).astype(F32)
    rstd = (1.0 / np.sqrt(arg.astype(np.float64))).astype(F32)
    t = ((x - mean[:, None]).astype(F32) * rstd[:, None]).astype(F32)
    return fma(t, gamma.astype(F32), beta.astype(F32)) if gamma is not None else t


# ---- e4m3 outputs -------------------------------------------------------------------------------------------------------------------------------
def e4m3(x):
    """x rounded to OCP e4m3 (round to nearest even, saturating at +-448, subnormal step 2^-9), as float64."""
    a = np.minimum(np.abs(np.asarray(x, np.float64)), 448.0)
    step = np.exp2(np.floor(np.log2(np.maximum(a, 2.0 ** -6))) - 3)
    return np.copysign(np.round(a / step) * step, x)


def decode_e4m3(u8):
    """OCP e4m3 bytes -> float64 (0x7f / 0xff, the NaN codes, decode to NaN)."""
    u = np.asarray(u8, np.uint8).astype(np.int64)
    e, m = (u >> 3) & 15, u & 7
    v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * np.exp2(e - 10.0))
    v = np.where((u & 127) == 127, np.nan, v)
    return np.where(u & 128, -v, v)


def mx_quant(x):
    """Block-scaled e4m3 of x (rows, C), C % 32 == 0, dequantised (float64): one scale 2^e per 32 channels, e = ceil(log2(amax / 448)) from the
    fp32 quotient as mx_quant8 of common.h takes it (a zero block stays zero)."""
    rows, C = x.shape
    b = np.asarray(x, np.float64).reshape(rows, C // 32, 32)
    q = (np.abs(b).max(axis=-1).astype(F32) / F32(448.0)).astype(F32)
    m, ex = np.frexp(q.astype(np.float64))                    # q = m 2^ex, m in [0.5, 1)
    e = np.where(m == 0.5, ex - 1, ex).astype(np.float64)      # ceil(log2 q)
    e = np.where(q > 0, np.maximum(e, -127.0), -127.0)
    scale = np.exp2(e)[..., None]
    return (e4m3(b / scale) * scale).reshape(rows, C)


def close8(deq, want, block):
    """The acceptance rule of tests/test_gpu_mx8.py for an 8-bit output against the quantised float64 reference: (every element within one e4m3
    step of the top binade of its block -- 32 2^e with 2^e < amax / 224, + slack --, share of elements that differ at all).  block = 32 for the
    block-scaled form; for e4m3 at scale 1 (block = 0) the step is the element's own binade's."""
    if block:
        blk = np.abs(want).reshape(want.shape[0], -1, block).max(-1).repeat(block, axis=1)
        step = blk / 224.0 * 34.0 + 1e-6
    else:
        step = np.exp2(np.floor(np.log2(np.maximum(np.abs(want), 2.0 ** -6))) - 3) * (34.0 / 32.0) + 1e-6
    return bool((np.abs(deq - want) <= step).all()), float((deq != want).mean()), step


# ---- the R limit ---------------------------------------------------------------------------------------------------------------------------------
def cancellation_ratio(R, dtype):
    """max |emulation - reference| / (A / 2) of the plain GroupNorm at CANCELLATION_SHAPE with |mu| / sigma up to R."""
    _, N, C, _, HW, G = CANCELLATION_SHAPE
    x, _, _ = gn_input(N, C, HW, G, dtype, R)
    ref = gn_ref64(x, G)
    emu = emulate_group_norm(x, G, gn_geometry(N, HW, C))
    return float((np.abs(emu - ref) / (budget(ref, dtype, R)[1] / 2)).max())


def max_plantable(dtype):
    return 2 ** (MANTISSA[dtype] - 2)


@functools.lru_cache(maxsize=None)
def cancellation_limit(dtype):
    """(the largest power-of-two R >= R_MAIN the emulation still meets A / 2 at, its ratio there, the ratio one step above or None where the type
    cannot hold the next R)."""
    R = R_MAIN
    ratio = cancellation_ratio(R, dtype)
    assert ratio <= 1.0
    while 2 * R <= max_plantable(dtype):
        nxt = cancellation_ratio(2 * R, dtype)
        if nxt > 1.0:
            return R, ratio, nxt
        R, ratio = 2 * R, nxt
    return R, ratio, None


# ---- mutants of the float64 reference: what a subtly wrong kernel would compute ------------------------------------------------------------------
def image_batches(N, HW, C, budget_elems=1 << 22):
    """slices of images whose float64 work arrays stay small: the references are computed a batch at a time, never in one array."""
    step = max(1, budget_elems // (HW * C))
    return [slice(n0, min(N, n0 + step)) for n0 in range(0, N, step)]


def last_batch_pixels(HW, geo):
    """mask over the pixels of the last live batch of every k_gn_apply block (a block streams nbatch batches of 4 RPB pixels)."""
    bs = GN_APPLY_PPT * geo["rpb"]
    ppb = bs * geo["nbatch"]
    m = np.zeros(HW, bool)
    for p0 in range(0, HW, ppb):
        p1 = min(HW, p0 + ppb)
        m[p0 + (-(-(p1 - p0) // bs) - 1) * bs:p1] = True
    return m


def x2_with_stride(x2, ld):
    """x2 (n, HW, C2) read as if its rows were ld elements apart (reads past the image wrap around inside it)."""
    n, HW, C2 = x2.shape
    idx = (np.arange(HW)[:, None] * ld + np.arange(C2)[None, :]) % (HW * C2)
    return x2.reshape(n, -1)[:, idx]


def gn_mutants(x, C1, G, geo, gamma, beta, silu, stats=None, sub_tables=None):
    """name -> mutant output for x (n, HW, C) (n >= 2).  stats: (mean, var) the reference was normalised with (default: x's own); sub_tables:
    (part1, part2, sub, mr) of a concat apply on sub-group partials."""
    n, HW, C = x.shape
    mean, var = stats if stats is not None else gn_stats64(x, G)
    ap = lambda m, v, xx=x, g_=gamma, b_=beta: gn_apply64(xx, m, v, G, g_, b_, silu)
    out = {"statistics of group g + 1": ap(np.roll(mean, -1, axis=1), np.roll(var, -1, axis=1)),
           "statistics of image n + 1": ap(np.roll(mean, -1, axis=0), np.roll(var, -1, axis=0))}
    if stats is None:
        out["last statistics chunk dropped"] = ap(*gn_stats64(x, G, keep=(geo["chunks"] - 1) * geo["pix_per_chunk"], count=HW))
        padded = geo["chunks"] * geo["pix_per_chunk"]
        out["count over a padded HW"] = ap(*gn_stats64(x, G, count=padded if padded != HW else HW + geo["rpb"]))
    if gamma is not None:
        out["gamma and beta rolled by 8 channels"] = ap(mean, var, g_=np.roll(gamma, 8), b_=np.roll(beta, 8))
    if C1 < C and C - C1 != C1:                                # (equal halves have one row stride: nothing to confuse)
        xm = np.concatenate([x[..., :C1], x2_with_stride(np.ascontiguousarray(x[..., C1:]), C1)], axis=-1)
        out["x2 read with x's row stride"] = ap(mean, var, xx=xm) if stats is not None else gn_ref64(xm, G, gamma, beta, silu)
    if sub_tables is not None:
        p1, p2, sub, mr = sub_tables
        out["a sub-group taken from the wrong table"] = ap(*cat_stats(p1, p2, HW, sub, mr, wrong_table=True))
    if geo["nbatch"] > 1:
        lost = ap(mean, var).copy()
        lost[:, last_batch_pixels(HW, geo)] = SENTINEL
        out["last batch of a block not stored"] = lost
    return out


def ln_mutants(x, form, gamma, beta):
    rows, C = x.shape
    L = LN_LANES[form]
    mean, var = ln_stats64(x)
    nb = np.arange(rows) ^ 1                                   # the other row of the pair: the same wave wherever a wave holds two rows or more
    nb = np.where(nb < rows, nb, np.arange(rows) - 1)
    x64 = x.astype(np.float64)
    head = x64[:, :(C - 1) // 8 * 8]                           # without the last channel vector
    m_lost = head.sum(axis=1) / C
    v_lost = np.maximum((head * head).sum(axis=1) / C - m_lost * m_lost, 0.0)
    padded = (C // (8 * L) + 1) * 8 * L
    m_pad = x64.sum(axis=1) / padded
    out = {"statistics of the neighbouring row": ln_apply64(x, mean[nb], var[nb], gamma, beta),
           "last channel vector left out of the statistics": ln_apply64(x, m_lost, v_lost, gamma, beta),
           "mean divided by the padded width": ln_apply64(x, m_pad, ((x64 - m_pad[:, None]) ** 2).mean(axis=1), gamma, beta)}
    if gamma is not None and C > 8:                            # (a row of one vector has nothing to roll)
        out["gamma rolled by 8"] = ln_apply64(x, mean, var, np.roll(gamma, 8), beta)
    return out
