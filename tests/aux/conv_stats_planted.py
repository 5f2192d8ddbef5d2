"""Planted-statistics inputs for the GroupNorm statistics a conv produces (csrc/gemm_common.h::igemm_gn_stats, csrc/gemm_reduce.hip) and for the
GroupNorm a conv applies to its input (the GI prologue), their float64 answers, numpy emulations of the kernels' summation orders and the budgets the
GPU test holds the kernels to (host code, numpy only).  tests/test_conv_stats_planted_host.py checks every claim made here on the CPU;
tests/test_gpu_conv_stats_planted.py walks the case tables below on the device.  round16, half_ulp, budget and the slice generator are
tests/aux/norm_planted.py's.

INPUTS.  y = GEMM + bias + bias_nc + residual.
  GEMM      exact.  x holds integers of [-2, 2], w integers of [-2, 2] / 8; the second half of the input channels repeats x and negates w, so the two
            halves of K cancel, except on 8 channels whose weights carry an extra d of [-2, 2] / 8: the full sum is the small field sum_c x_c d_c
            (multiples of 1 / 8), while a split-K slab of the first half holds a partial of up to hundreds of eighths.  Every product, every fp32
            accumulation and every slab -- also an fp16 one: |partial| <= 2048 eighths -- is exact (exact_claims() checks it in numpy).  A lost or
            doubled slab moves y by a multiple of 1 / 8.
  residual  norm_planted.gn_input at R_MAIN, one slice per (image, OUTPUT group): adjacent groups and adjacent images differ in mean and sigma.
  bias      multiples of 1 / 8 in [-2, 2] per channel;  bias_nc multiples of 1 / 8 in [-1.875, 1.875] per (image, channel), a different row per
            image (rolled by one image it differs at every channel), bias_nc_stride = Cout.
  selector weights (part C): output channel o is (+-2^k, k in {0, 1}) times input channel PERM[o] at one tap (3 x 3: all nine in turn), PERM the rotation by two groups
            and one channel, which moves every channel at least two groups away: the conv output is exactly sign 2^k times the rounded normalised input.

REFERENCES.  y64 = the float64 sum of what the device was given; the device's y must satisfy |y - y64| <= half_ulp(|y64| + a) + a with
a = 3 2^-24 (|GEMM| + |bias| + |bias_nc| + |res|) (three fp32 additions).  Everything downstream of y -- tables, z, the hand-over -- is held to
float64 computed from the y READ BACK from the device: the kernels' contract is "the statistics of the 16-bit-rounded outputs".

BUDGETS, from the float64 reference and the emulations below, never from a device.
  normalised outputs (z of the fused reduce, the apply entries fed with a producer's table): z_budget() = norm_planted.budget's formula
      tol = half_ulp(|y| + A) + A, A = K 2^-22 (1 + R) (1 + |y|) max|gamma| [+ 2^-22 |y| behind SiLU], K = K_CONV[form]: 14 behind an epilogue
      table, the K_ARITH + K_STATS = 12 of norm_planted behind the two reducers.  The emulations' largest error over the case tables, as max |emulation - reference| / (A at K = 1), float16 | bfloat16
      (the host test prints them per case and fails above EMU_RATIO):
          epilogue table -> k_gn_apply's fold and apply:        6.83 | 2.69   (256 x 128 tile, 64 sequential rows per stripe; not <= 12 / 2, so K is
                                                                               raised to the smallest integer with 6.83 <= K / 2)
          k_splitk_reduce_gn table -> k_gn_apply:               1.04 | 0.21   (<= 12 / 2: K stays 12)
          k_splitk_reduce_gn_apply (its own fold and apply):    0.69 | 0.19   (K stays 12)
      A concat apply fed by an epilogue table and a reducer's table is held to the larger K of the two.
      Part C (planted x with host partials, no conv-made statistics) keeps norm_planted.budget(..., stats=True) unchanged.
  statistics tables, per slot of (N, chunks, G, 2): |S - S64| <= c 2^-24 sum |y|, |Q - Q64| <= c 2^-24 sum y^2 over the slot's rows and channels,
      c = TABLE_C[form] = twice the largest ratio the emulation of that form reaches; measured float16 | bfloat16
      (bfloat16 values carry 8 significant bits, so far more of their fp32 partial sums are exact):
          epilogue (ROWS sequential adds per column, 4 stripes, 64-lane xor tree):                          5.91 | 2.42  -> c = 11.82
          reduce_gn (rows rl, rl + RL, ... per thread, RL row lanes, wave tree):                            2.98 | 2.60  -> c = 5.96
          reduce_gn_apply (<= 8 rows per thread, fold 1 in fp32 over `parts`, fold 2 in fp64):             1.17 | 1.00  -> c = 2.34
      A slot no row or channel contributes to (piece 1 of a group that lies inside one tile) has sum |y| = 0: it must hold exactly 0.
The host test fails if an emulation exceeds TABLE_RATIO / EMU_RATIO below, the maxima these lines quote."""
import collections
import functools

import numpy as np

import norm_planted as P
from norm_planted import round16, half_ulp, budget, F32  # noqa: F401  (the GPU and host tests take them from here)

R = P.R_MAIN
GN_MAX_CHUNKS = 192           # TF_GN_MAX_CHUNKS of csrc/gemm_family.h
RGA_MAXR = 8
SENTINEL = P.SENTINEL
# measured by tests/test_conv_stats_planted_host.py (pytest -s prints them per case): the larger of the fp16 | bf16 maxima over the case tables
TABLE_RATIO = {"epilogue": 5.91, "reduce_gn": 2.98, "reduce_gn_apply": 1.17}
TABLE_C = {k: 2.0 * v for k, v in TABLE_RATIO.items()}     # twice the emulation's largest ratio: 11.82, 5.96, 2.34
EMU_RATIO = {"epilogue": 6.83, "reduce_gn": 1.04, "reduce_gn_apply": 0.69}
# K of the norm budget per producing form: K_ARITH + K_STATS = 12 of norm_planted where the emulation stays <= 12 / 2; the epilogue form's 6.83 does
# not, 14 is the smallest integer with 6.83 <= K / 2
K_CONV = {"epilogue": 14.0, "reduce_gn": P.K_ARITH + P.K_STATS, "reduce_gn_apply": P.K_ARITH + P.K_STATS}


def z_budget(y, dtype, form, gmax=1.0, silu=False):
    """(tol, A) per element of the float64 reference y of an output normalised with the statistics a producer of `form` made: norm_planted.budget's
    formula at K = K_CONV[form] (budget itself where that is its own 12)."""
    if K_CONV[form] == P.K_ARITH + P.K_STATS:
        return budget(y, dtype, R, gmax, silu, stats=True)
    A = K_CONV[form] * P.a_unit(y, R, gmax) + (2.0 ** -22 * np.abs(y) if silu else 0.0)
    return half_ulp(np.abs(y) + A, dtype) + A, A


# ---- the launch rules: copies of gemm_family.h / gemm_reduce.hip (the GPU test asserts the library's reported chunks / z_written against them) ------
VARIANT_OF_BIT = {0: 0, 8: 0, 16: 1, 128: 2, 256: 3, 512: 4, 2048: 6}     # tf_gemm_debug bit -> the variant column of tf_prof_dump (gemm_family.h)
PINGPONG_BITS = (512, 2048)   # tf_gemm_debug bits of k_igemm_pp / k_igemm_pp3: the statistics epilogue works in half-tile sub-blocks


def gn_reduce_chunks(HoWo):
    r = -(-HoWo // GN_MAX_CHUNKS)
    while HoWo % r:
        r += 1
    return HoWo // r


def gn_pieces(bn, cpg):
    return 1 if bn % cpg == 0 else 2


def eff_splitk(K, split):
    kt = -(-K // 64)
    kps = -(-kt // max(split, 1))
    return -(-kt // kps)


def slab_ranges(K, split):
    """[(k0, k1)] of the K range each split slab covers (whole 64-element K tiles)."""
    kt = -(-K // 64)
    kps = -(-kt // max(split, 1))
    return [(z * kps * 64, min(K, (z + 1) * kps * 64)) for z in range(-(-kt // kps))]


def rga_geometry(HoWo, N, G):
    """dict(gpb, CV, RPS, parts, CW) of k_splitk_reduce_gn_apply for outputs of HoWo pixels x N channels in G groups, or None (not eligible)."""
    if G < 1 or N % G or N % 4:
        return None
    cpg = N // G
    g = 1
    while g <= G and ((g * cpg) % 4 != 0 or G % g != 0):
        g += 1
    if g > G or g > 16:
        return None
    CW = g * cpg
    if CW > 256:
        return None
    cv = CW // 4
    rps = min(1024 // cv, HoWo)
    if rps * RGA_MAXR < HoWo:
        return None
    parts = 1024 // CW
    if (rps * CW + parts * CW) * 8 + g * 8 > 160 * 1024:
        return None
    return dict(gpb=g, CV=cv, RPS=rps, parts=parts, CW=CW)


def stats_requested(Cout, G):
    cpg = Cout // G
    return 4 <= cpg <= 64 and Cout % 8 == 0 and Cout <= 4096 and G <= 256


def reduce_gn_geometry(HoWo, N):
    chunks = gn_reduce_chunks(HoWo)
    Rr, nq = HoWo // chunks, N // 4
    RL = min(1024 // nq, Rr)
    return dict(chunks=chunks, R=Rr, RL=RL, threads=(RL * nq + 63) & ~63, live=RL * nq)


Conv = collections.namedtuple("Conv", "form N H W Cin Cout G ks bm bn split dbg")


def predict(c, entry="fused"):
    """(kind, chunks, z_written) the launch must report: kind in epilogue / reduce_gn / reduce_gn_apply / none."""
    HoWo, cpg = c.H * c.W, c.Cout // c.G
    if not stats_requested(c.Cout, c.G):
        return "none", 0, 0
    if eff_splitk(c.ks * c.ks * c.Cin, c.split) == 1:
        sbm = c.bm // 2 if c.dbg in PINGPONG_BITS else c.bm
        chunks = gn_pieces(c.bn, cpg) * (HoWo // sbm)
        return ("epilogue", chunks, 0) if HoWo % sbm == 0 and chunks <= GN_MAX_CHUNKS else ("none", 0, 0)
    if entry == "norm" and rga_geometry(HoWo, c.Cout, c.G):
        return "reduce_gn_apply", 1, 1
    return "reduce_gn", gn_reduce_chunks(HoWo), 0


# ---- the case tables ------------------------------------------------------------------------------------------------------------------------------
# A. epilogue statistics, split 1, tf_conv2d_fused_16.  form names what the case is for; form_holds() says what the geometry must show.
def _A(form, N, hw, Cout, G, bm, bn, dbg=8, ks=1, Cin=64):
    H, W = hw if isinstance(hw, tuple) else (hw // 8, 8)
    return Conv(form, N, H, W, Cin, Cout, G, ks, bm, bn, 1, dbg)


EPILOGUE_CASES = [
    # cpg 4: 32 groups in one tile (4 turns of the round-robin over 8 waves); on BN = 160 the only n-tile is 128 columns wide
    _A("cpg4 32 groups", 2, 64, 128, 32, 64, 160), _A("cpg4 32 groups", 3, 128, 128, 32, 128, 128), _A("cpg4 32 groups", 2, 256, 128, 32, 64, 128),
    # cpg 10 (320 / 32): two pieces on BN = 128 (last n-tile 64 columns) and BN = 64, one piece on BN = 160
    _A("two pieces narrow last", 2, 128, 320, 32, 64, 128), _A("two pieces", 3, 256, 320, 32, 128, 64), _A("one piece", 2, 64, 320, 32, 64, 160),
    _A("one piece", 5, 128, 320, 32, 128, 160), _A("two pieces narrow last", 2, 512, 320, 32, 128, 128),
    # cpg 20
    _A("two pieces", 2, 128, 640, 32, 128, 128), _A("two pieces", 2, 64, 640, 32, 64, 64), _A("one piece", 3, 256, 640, 32, 64, 160),
    # cpg 40, cpg 64
    _A("one piece", 2, 128, 1280, 32, 128, 160), _A("two pieces", 2, 64, 1280, 32, 64, 128), _A("one piece", 2, 128, 256, 4, 64, 128),
    _A("two pieces", 3, 64, 256, 4, 64, 160), _A("one piece", 2, 256, 256, 4, 128, 64),
    # a last n-tile narrower than BN: Cout = 96 on BN = 64 leaves 32 columns (cpg 12: two pieces)
    _A("two pieces narrow last", 5, 64, 96, 8, 64, 64),
    # the 256 x 128 tile; wide and all-8 rings (RING_FORM: the variant each tf_gemm_debug bit asks for; tf_gemm_ring_form says whether the tile has it)
    _A("two pieces narrow last", 2, 256, 320, 32, 256, 128), _A("two pieces narrow last", 3, 512, 320, 32, 256, 128),
    _A("two pieces narrow last", 2, 128, 320, 32, 64, 128, dbg=16), _A("one piece", 2, 128, 640, 32, 64, 160, dbg=16),      # (128 x 160 has no wide ring)
    _A("two pieces narrow last", 2, 128, 320, 32, 64, 128, dbg=256), _A("one piece", 2, 128, 640, 32, 128, 160, dbg=256),
    # k_igemm_pp (bit 512): 128- / 96-row statistics sub-blocks
    _A("two pieces narrow last", 2, 256, 320, 32, 256, 128, dbg=512), _A("one piece", 3, 512, 320, 32, 256, 160, dbg=512),
    _A("two pieces", 2, 256, 640, 32, 256, 256, dbg=512), _A("two pieces narrow last", 2, (12, 16), 320, 32, 192, 128, dbg=512),
    _A("one piece", 3, (24, 16), 640, 32, 192, 160, dbg=512),
    # k_igemm_pp3 (bit 2048): 3 x 3 on 24 x 24 images, 192-row tiles
    _A("two pieces narrow last", 2, (24, 24), 320, 32, 192, 128, dbg=2048, ks=3),
    # k_igemm_patch (bit 128): 3 x 3 on 16 x 16 images
    _A("two pieces narrow last", 2, (16, 16), 320, 32, 64, 128, dbg=128, ks=3), _A("one piece", 3, (16, 16), 640, 32, 128, 160, dbg=128, ks=3),
    # the two refusals: chunks == 0 and the table untouched
    _A("refused: tile straddles images", 2, 64, 128, 32, 128, 64), _A("refused: cpg 80", 1, 256, 2560, 32, 64, 160),
]


def form_holds(c):
    cpg = c.Cout // c.G
    kind, chunks, _ = predict(c)
    if c.form.startswith("refused"):
        return kind == "none" and (cpg == 80 or (c.H * c.W) % c.bm != 0)
    if kind != "epilogue":
        return False
    narrow = c.Cout % c.bn != 0
    if c.form == "cpg4 32 groups":
        return cpg == 4 and min(c.bn, c.Cout) // cpg == 32
    if c.form == "one piece":
        return gn_pieces(c.bn, cpg) == 1
    if c.form == "two pieces":
        return gn_pieces(c.bn, cpg) == 2
    if c.form == "two pieces narrow last":
        return gn_pieces(c.bn, cpg) == 2 and narrow
    raise KeyError(c.form)


# B. the reducers.  K tiles per requested split count, chosen so that the dispatcher runs exactly that many slabs (eff_splitk == split)
KTILES = {2: 18, 3: 18, 4: 16, 5: 20, 8: 16, 9: 18, 16: 16, 17: 17}
SPLITS = tuple(KTILES)


def _B(form, N, hw, Cout, G, split, ktiles=None):
    H, W = hw if isinstance(hw, tuple) else (hw // 8, 8)
    return Conv(form, N, H, W, 64 * (ktiles or KTILES[split]), Cout, G, 1, 64, 64, split, 8)


# k_splitk_reduce_gn through tf_conv2d_fused_16 (form: what reduce_gn_geometry must show)
REDUCE_GN_CASES = [_B("R=1", 2, 64, 128, 32, s) for s in SPLITS] + [
    _B("R multiple of RL", 2, 256, 128, 32, 2, 2),                  # R = RL = 2
    _B("R not multiple of RL", 2, (24, 24), 2048, 32, 2, 2),        # R = 3, RL = 2: 1024 threads = 16 waves against 32 groups
    # HoWo = 400 stands in for the 576 one might expect: 576 / 192 = 3 divides exactly, so gn_reduce_chunks has nothing to search there (the
    # 24 x 24 cases above and below); 400 / 192 -> 3 does not divide 400 -> R = 4, RL = 2
    _B("R multiple of RL", 2, (20, 20), 2048, 32, 3, 3),
    _B("padded wave", 3, (24, 24), 320, 32, 2, 2),                  # R = RL = 3, nq = 80: 240 live threads of 256, 4 waves against 32 groups
    _B("RL=1 N=4096", 2, 64, 4096, 64, 2, 2),
    _B("not eligible for the fused reduce", 2, (23, 71), 320, 32, 2, 2),   # (run through tf_conv2d_fused_norm_16: z_written == 0)
    _B("not eligible for the fused reduce", 2, (19, 43), 1280, 32, 2, 2),
]


def reduce_gn_form_holds(c):
    HoWo = c.H * c.W
    g = reduce_gn_geometry(HoWo, c.Cout)
    if c.form == "R=1":
        return g["R"] == 1 and eff_splitk(c.Cin, c.split) == c.split
    if c.form == "R multiple of RL":
        return g["R"] > 1 and g["R"] % g["RL"] == 0
    if c.form == "R not multiple of RL":
        return g["R"] % g["RL"] != 0 and g["threads"] == 1024
    if c.form == "padded wave":
        return g["live"] % 64 != 0 and g["threads"] == 256 and c.G == 32
    if c.form == "RL=1 N=4096":
        return g["RL"] == 1 and c.Cout == 4096 and c.Cout // c.G == 64
    if c.form == "not eligible for the fused reduce":
        return rga_geometry(HoWo, c.Cout, c.G) is None and rga_geometry(HoWo - 1, c.Cout, c.G) is not None
    raise KeyError(c.form)


# k_splitk_reduce_gn_apply through tf_conv2d_fused_norm_16: (case, affine, silu)
def _F(form, N, hw, Cout, G, split=2, ktiles=2, aff=True, silu=True):
    return _B(form, N, hw, Cout, G, split, ktiles), aff, silu


FUSED_CASES = [_F("gpb1", 2, 64, 128, 32, s, KTILES[s]) for s in SPLITS] + [      # cpg 4: RPS clipped to HoWo = 64, parts = 256 > RPS
    _F("gpb1", 3, 256, 640, 32), _F("gpb1", 1, 256, 1280, 32, silu=False), _F("gpb1", 2, 128, 256, 4, aff=False, silu=False),   # cpg 20, 40, 64
    _F("gpb2", 5, 128, 320, 32), _F("gpb2", 2, 128, 192, 32, silu=False),                                # cpg 10, 6
    _F("gpb4", 3, 128, 224, 32, aff=False),                                                              # cpg 7
    _F("ragged sweep", 2, (24, 24), 320, 32),                                                            # RPS = 204: sweeps of 204, 204, 168
    _F("largest eligible", 2, (32, 51), 320, 32), _F("largest eligible", 1, (24, 34), 1280, 32, silu=False),   # HoWo = 8 RPS: 1632 at cpg 10, 816 at cpg 40
]
# npairs = parts cpg of fold 2 is at least 1024 / 16 = 64 for every eligible geometry (gpb <= 16): "below 64" cannot be reached.


def fused_form_holds(c):
    HoWo = c.H * c.W
    g = rga_geometry(HoWo, c.Cout, c.G)
    if g is None or eff_splitk(c.Cin, c.split) != c.split:
        return False
    if c.form.startswith("gpb"):
        return g["gpb"] == int(c.form[3:])
    if c.form == "ragged sweep":
        return HoWo % g["RPS"] != 0 and HoWo > g["RPS"]
    if c.form == "largest eligible":
        return g["RPS"] * RGA_MAXR == HoWo and rga_geometry(HoWo + 1, c.Cout, c.G) is None
    raise KeyError(c.form)


# k_splitk_reduce (no statistics): (form, M rows as N x H x W, Cout, split, ktiles); every subset of {bias, bias_nc, residual} runs on the first
PLAIN_CASES = [_B("quad", 2, 64, 128, 32, s) for s in SPLITS] + [_B("second stride", 2, (32, 32), 1280, 32, 2, 2)]
LINEAR_N50 = (96, 50, 128, 2)          # M, N, K, split: the N % 4 != 0 path (tf_linear_16)
SUBSETS = [(b, n, r) for b in (0, 1) for n in (0, 1) for r in (0, 1)]

# hand-over to tf_group_norm_apply_cat_16: two producers with different chunk counts, a group of the concat on the seam: (N, HoWo, C1, C2, G, sub)
CAT_CASES = [(2, 64, 1280, 640, 32, 20), (3, 128, 64, 32, 8, 4)]

# C. the input side (tf_conv2d_gn_16, selector weights): (N, H, W, C1, C2, G, ks, bm, bn, chunks, chunks2, silu)
GI_CASES = [
    (2, 8, 8, 128, 0, 32, 1, 64, 64, 1, 0, False), (3, 16, 8, 128, 0, 32, 1, 128, 64, 4, 0, True),
    (2, 8, 8, 64, 128, 8, 1, 64, 128, 4, 1, True),             # groups of 24 channels: group 2 = channels 48 .. 71 lies on the seam at 64 (sub-groups of 8)
    (2, 16, 16, 128, 0, 32, 3, 64, 128, 4, 0, True), (2, 16, 16, 64, 128, 8, 3, 128, 128, 1, 4, False),
]
GI_SUB = 8                             # sub-group width of the two-source cases: groups1 = C1 / 8, groups2 = C2 / 8, mr = 3
GI_REFUSED = (2, 10, 10, 128, 0, 128, 3, 3, 1, 1, 0, 0, 0, 32)      # tf_conv2d_gn_supported's arguments: 3 x 3 on rows of 10 pixels (no patch tile)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------
def im2col(x, ks):
    """x (N, H, W, C) -> (N H W, ks ks C), stride 1, padding ks // 2, K order (r, s, c)."""
    N, H, W, C = x.shape
    if ks == 1:
        return x.reshape(N * H * W, C)
    p = ks // 2
    xp = np.zeros((N, H + 2 * p, W + 2 * p, C), x.dtype)
    xp[:, p:p + H, p:p + W] = x
    return np.concatenate([xp[:, r:r + H, s:s + W] for r in range(ks) for s in range(ks)], axis=-1).reshape(N * H * W, ks * ks * C)


@functools.lru_cache(maxsize=3)
def gemm_inputs(N, H, W, Cin, Cout, ks):
    """x (N, H, W, Cin), w (Cout, ks, ks, Cin) float32 (exact in float16 and bfloat16) and their exact product (N, H W, Cout) float64."""
    assert Cin % 16 == 0 and Cin >= 16
    rng = np.random.default_rng([31, N, H, W, Cin, Cout, ks])
    h = Cin // 2
    xh = rng.integers(-2, 3, (N, H, W, h))
    wh = rng.integers(-2, 3, (Cout, ks, ks, h))
    d = np.zeros_like(wh)
    d[..., :8] = rng.integers(-2, 3, (Cout, ks, ks, 8))
    x = np.concatenate([xh, xh], axis=-1).astype(F32)
    w = (np.concatenate([wh, d - wh], axis=-1) / 8.0).astype(F32)
    g = im2col(xh[..., :8].astype(np.float64), ks) @ (d[..., :8].reshape(Cout, -1).T / 8.0)      # what survives the cancellation
    for a in (x, w, g):
        a.setflags(write=False)
    return x, w, g.reshape(N, H * W, Cout)


def slab_partials(x, w, ks, split):
    """the split-K slabs (eff, M, Cout) in float64 (exact)."""
    A, B = im2col(x, ks).astype(np.float64), w.reshape(w.shape[0], -1).astype(np.float64)
    return np.stack([A[:, k0:k1] @ B[:, k0:k1].T for k0, k1 in slab_ranges(A.shape[1], split)])


def exact_claims(c):
    """The exactness the GEMM part claims, in numpy: the slabs add up to the field gemm_inputs states, every slab is at most 2048 eighths (exact
    in an fp16 slab), the fp32 product equals the float64 one.  -> the largest |slab| in eighths."""
    x, w, g = gemm_inputs(c.N, c.H, c.W, c.Cin, c.Cout, c.ks)
    parts = slab_partials(x, w, c.ks, c.split)
    M = c.N * c.H * c.W
    assert len(parts) == eff_splitk(c.ks * c.ks * c.Cin, c.split)
    assert np.array_equal(parts.sum(0), g.reshape(M, c.Cout)) and np.array_equal(parts * 8, np.round(parts * 8))
    assert np.abs(parts * 8).max() <= 2048 and np.array_equal(parts.astype(np.float16).astype(np.float64), parts)
    f32 = im2col(x, c.ks) @ w.reshape(c.Cout, -1).T
    assert f32.dtype == np.float32 and np.array_equal(f32.astype(np.float64), g.reshape(M, c.Cout))
    return float(np.abs(parts * 8).max())


def bias_of(Cout):
    return (((3 * np.arange(Cout) + 1) % 33 - 16) / 8.0).astype(F32)


def bias_nc_of(N, Cout):
    n, c = np.meshgrid(np.arange(N), np.arange(Cout), indexing="ij")
    return (((5 * c + 7 * n + 2) % 31 - 15) / 8.0).astype(F32)


def conv_problem(c, dtype, use=(1, 1, 1), res=None):
    """dict of everything the device is given (float32 arrays holding values of the storage type) and the float64 answer: x, w, bias, bias_nc,
    res (None where `use` drops it), gemm, y64, a (the fp32 part of y's bound).  res: a residual other than the case's own planted one."""
    x, w, g = gemm_inputs(c.N, c.H, c.W, c.Cin, c.Cout, c.ks)
    HoWo = c.H * c.W
    b = bias_of(c.Cout) if use[0] else None
    e = bias_nc_of(c.N, c.Cout) if use[1] else None
    if use[2] and res is None:
        res = P.gn_input(c.N, c.Cout, HoWo, c.G, dtype)[0]
    r = res if use[2] else None
    y64 = g.copy()
    mag = np.abs(g)
    if b is not None:
        y64 += b.astype(np.float64)
        mag += np.abs(b)
    if e is not None:
        y64 += e.astype(np.float64)[:, None, :]
        mag = mag + np.abs(e)[:, None, :]
    if r is not None:
        y64 += r
        mag = mag + np.abs(r)
    return dict(x=x, w=w, bias=b, bias_nc=e, res=r, gemm=g, y64=y64, a=3 * 2.0 ** -24 * mag)


def y_tol(p, dtype):
    return half_ulp(np.abs(p["y64"]) + p["a"], dtype) + p["a"]


def emulate_y(p, dtype, gemm=None, bias_nc=None):
    """the kernels' epilogue: ((GEMM + bias) + bias_nc) + residual in fp32, one storage rounding.  gemm / bias_nc: a mutant's."""
    v = (p["gemm"] if gemm is None else gemm).astype(F32)
    if p["bias"] is not None:
        v = v + p["bias"]
    e = p["bias_nc"] if bias_nc is None else bias_nc
    if e is not None:
        v = v + e[:, None, :]
    if p["res"] is not None:
        v = v + p["res"]
    return round16(v, dtype)


# ---- float64 tables -----------------------------------------------------------------------------------------------------------------------------
def _piece_of(C, G, bn):
    """(G, cpg) bool: channel lies in the SECOND n-tile its group touches."""
    cpg = C // G
    ch = np.arange(C).reshape(G, cpg)
    return (ch // bn) != (ch[:, :1] // bn)


def table64(y, G, rows, bn=None):
    """(S/Q table, sum |y| / sum y^2 table), both (N, chunks, G, 2) float64, of y (N, HoWo, C): one chunk per `rows` rows, times two pieces where bn is
    given and groups straddle n-tiles (chunk = 2 m-tile + piece, as igemm_gn_stats lays them out)."""
    N, HoWo, C = y.shape
    cpg = C // G
    yb = y.astype(np.float64).reshape(N, HoWo // rows, rows, G, cpg)
    cols = np.stack([yb.sum(2), (yb * yb).sum(2), np.abs(yb).sum(2)], axis=-1)          # (N, MT, G, cpg, 3)
    if bn is None or bn % cpg == 0:
        t = cols.sum(3)
    else:
        pm = _piece_of(C, G, bn)[None, None, :, :, None]
        t = np.stack([(cols * ~pm).sum(3), (cols * pm).sum(3)], axis=2).reshape(N, -1, G, 3)
    return t[..., :2], t[..., [2, 1]]


def table_ok(T, y, G, rows, bn, c):
    """(largest |T - T64| / (2^-24 mag) over the slots with mag > 0, all slots with mag == 0 hold exactly 0)"""
    ref, mag = table64(y, G, rows, bn)
    err = np.abs(T.astype(np.float64) - ref)
    live = mag > 0
    ratio = float((err[live] / (2.0 ** -24 * mag[live])).max())
    return ratio, bool((T[~live] == 0).all())


# ---- emulations of the three summation orders -------------------------------------------------------------------------------------------------------
def _seq(a, axis):
    """(sum, sum of squares by fma) of a float32 array along axis, added in order in fp32."""
    a = np.moveaxis(a, axis, 0)
    s = np.zeros(a.shape[1:], F32)
    q = np.zeros(a.shape[1:], F32)
    for i in range(a.shape[0]):
        s = s + a[i]
        q = P.fma(a[i], a[i], q)
    return s, q


def _seq_add(a, axis):
    a = np.moveaxis(a, axis, 0)
    s = np.zeros(a.shape[1:], F32)
    for i in range(a.shape[0]):
        s = s + a[i]
    return s


def _wave_tree(v):
    """wave_sum of common.h over the last axis (at most 64 live lanes, the rest 0): xor offsets 32, 16, ... 1."""
    pad = np.zeros(v.shape[:-1] + (64,), F32)
    pad[..., :v.shape[-1]] = v
    return P._pair_tree(pad, ascending=False)


def emulate_epilogue(y, G, sbm, bn, lost_tile=None):
    """igemm_gn_stats on y (N, HoWo, C) float32: per column ROWS = sbm / 4 sequential adds in each of 4 row stripes, the 4 stripes added in order by
    the group's wave (lane = channel of the group inside the tile), xor tree.  -> (N, chunks, G, 2) float32"""
    N, HoWo, C = y.shape
    cpg, MT, ROWS = C // G, HoWo // sbm, sbm // 4
    s, q = _seq(y.reshape(N, MT, 4, ROWS, C), 3)
    cs = np.stack([_seq_add(s, 2), _seq_add(q, 2)], axis=-1).reshape(N, MT, G, cpg, 2)       # (N, MT, G, cpg, 2)
    two = bn % cpg != 0
    out = np.zeros((N, MT, 2 if two else 1, G, 2), F32)
    pm = _piece_of(C, G, bn)
    for g in range(G):
        for piece in range(2 if two else 1):
            sel = pm[g] == bool(piece) if two else np.ones(cpg, bool)
            if sel.any():
                for j in range(2):
                    out[:, :, piece, g, j] = _wave_tree(cs[:, :, g, sel, j])
    return out.reshape(N, -1, G, 2)


def emulate_reduce_gn(y, G):
    """k_splitk_reduce_gn: thread (rl, quad) adds rows rl, rl + RL, ... of its block's R rows, the group's wave adds the RL row lanes per channel in
    order, xor tree over the channels."""
    N, HoWo, C = y.shape
    geo = reduce_gn_geometry(HoWo, C)
    chunks, Rr, RL = geo["chunks"], geo["R"], geo["RL"]
    it = -(-Rr // RL)
    yp = np.zeros((N, chunks, it * RL, C), F32)
    yp[:, :, :Rr] = y.reshape(N, chunks, Rr, C)
    s, q = _seq(yp.reshape(N, chunks, it, RL, C), 2)
    cs = np.stack([_seq_add(s, 2), _seq_add(q, 2)], axis=-1).reshape(N, chunks, G, C // G, 2)
    return np.stack([_wave_tree(cs[..., 0]), _wave_tree(cs[..., 1])], axis=-1)


def emulate_reduce_gn_apply_stats(y, G, lose_ragged=False, stale=None):
    """k_splitk_reduce_gn_apply's statistics: thread (rl, quad) adds rows rl + k RPS (k < 8), fold 1 adds the row lanes part, part + parts, ... in
    fp32, fold 2 adds the (part, channel) pairs of a group in fp64.  -> (S, Q) (N, G) float64 (the table holds them rounded to fp32).
    lose_ragged: the mutant that leaves the last, ragged sweep out of the sums; stale: the value the mutant reads from fold-1 lanes beyond RPS."""
    N, HoWo, C = y.shape
    geo = rga_geometry(HoWo, C, G)
    RPS, parts = geo["RPS"], geo["parts"]
    sweeps = -(-HoWo // RPS)
    yp = np.zeros((N, sweeps * RPS, C), F32)
    yp[:, :HoWo] = y
    if lose_ragged:
        yp[:, (sweeps - 1) * RPS:] = 0
    s, q = _seq(yp.reshape(N, sweeps, RPS, C), 1)
    it = -(-RPS // parts)
    out = []
    for a in (s, q):
        ap = np.zeros((N, it * parts, C), F32)
        ap[:, :RPS] = a
        p1 = _seq_add(ap.reshape(N, it, parts, C), 1).astype(np.float64)
        if stale is not None and RPS < parts:
            p1[:, RPS:] = stale
        out.append(p1.sum(1).reshape(N, G, C // G).sum(-1))
    return out[0], out[1]


def stats_of_sums(S, Q, cnt):
    mean = S / cnt
    return mean, np.maximum(Q / cnt - mean * mean, 0.0)


def emulate_fused(y, G, gamma=None, beta=None, silu=False):
    """(table (N, 1, G, 2) float32, z float32) of k_splitk_reduce_gn_apply on y (N, HoWo, C) float32."""
    N, HoWo, C = y.shape
    S, Q = emulate_reduce_gn_apply_stats(y, G)
    mean, var = stats_of_sums(S, Q, float(HoWo * (C // G)))
    return np.stack([S, Q], axis=-1).astype(F32)[:, None], P.emulate_gn_apply(y, mean, var, G, gamma, beta, silu)


def emulate_consumer(y, T, G, gamma=None, beta=None, silu=False):
    """tf_group_norm_apply_16 on y and a producer's table T (N, chunks, G, 2): k_gn_apply's fp64 fold, fp32 apply."""
    mean, var = P.stats_from_partials(T, y.shape[1], y.shape[2] // G)
    return P.emulate_gn_apply(y, mean, var, G, gamma, beta, silu)


# ---- selector weights (part C) ------------------------------------------------------------------------------------------------------------------
def selector(C, G, ks):
    """(w (C, ks, ks, C) float32, perm, scale, tap): output channel o = scale[o] x input channel perm[o] at tap tap[o] (the centre for a 1 x 1 conv,
    walking all nine taps for a 3 x 3 one, so that border outputs read the padding: they must be exactly 0); perm moves every channel at least
    two groups away from its own (and so never onto its own group's neighbour)."""
    cpg = C // G
    assert G >= 5
    o = np.arange(C)
    perm = (o + 2 * cpg + 1) % C
    gd = np.abs(perm // cpg - o // cpg)
    assert (np.minimum(gd, G - gd) >= 2).all() and len(set(perm.tolist())) == C
    scale = np.where(o % 2 == 0, 1.0, -1.0) * np.exp2((o // 2) % 2)      # (never below 1: halving a float16 subnormal is not exact)
    tap = o % (ks * ks)
    w = np.zeros((C, ks, ks, C), F32)
    w[o, tap // ks, tap % ks, perm] = scale
    return w, perm, scale, tap


def selector_answer(ref, tol, w, N, H, W):
    """(float64 reference, tolerance) of the selector conv's output given those of the normalised input (N, H W, C): each output element is one
    input element times +-2^k, or exactly 0 (tolerance 0) where its tap reads the padding."""
    ks, Ct = w.shape[1], w.shape[0]
    wm = w.reshape(Ct, -1).T.astype(np.float64)
    out = im2col(ref.reshape(N, H, W, Ct), ks) @ wm
    t = im2col(tol.reshape(N, H, W, Ct), ks) @ np.abs(wm)
    return out.reshape(N, H * W, Ct), t.reshape(N, H * W, Ct)


# ---- mutants --------------------------------------------------------------------------------------------------------------------------------------
def stats_mutants(y, mean, var, G, gamma, beta, silu, padded_cnt=None):
    """name -> z of a consumer that normalises y with wrong statistics (float64)."""
    ap = lambda m, v: P.gn_apply64(y, m, v, G, gamma, beta, silu)
    out = {"neighbour group's (mean, rstd)": ap(np.roll(mean, -1, axis=1), np.roll(var, -1, axis=1))}
    if y.shape[0] > 1:
        out["neighbour image's (mean, rstd)"] = ap(np.roll(mean, -1, axis=0), np.roll(var, -1, axis=0))
    if padded_cnt is not None:
        out["count replaced by the padded RPS x RGA_MAXR x cpg"] = ap(*P.gn_stats64(y, G, count=padded_cnt))
    return out


def epilogue_table_mutants(T, two_pieces, whole_group_slots):
    """name -> table of an epilogue that mishandles its slots.  T (N, chunks, G, 2); whole_group_slots: (G,) bool, the group lies inside one tile."""
    out = {}
    m = T.copy()
    m[:, -(2 if two_pieces else 1):] = 0
    out["one m-tile's chunk lost"] = m
    if two_pieces:
        m = T.copy()
        m[:, 1::2] = 0
        out["piece 1 of a straddling group lost"] = m
        m = T.copy()
        m[:, 0::2] += T[:, 1::2]
        out["piece 1 of a straddling group also added to piece 0"] = m
        if whole_group_slots.any():
            m = T.copy()
            m[:, 1::2, whole_group_slots] = SENTINEL
            out["a whole-group tile not zeroing its piece 1"] = m
    return out


def sum_partials_nb(s, slab_bits):
    """the batch width sum_partials of gemm_reduce.hip picks for s slabs of that element type."""
    if s <= 2:
        return 2
    if s <= 4:
        return 4
    return 16 if slab_bits == 16 and s > 8 else 8


def slab_mutants(p, c, dtype, slab_bits):
    """name -> y of a reducer that mishandles its slabs (float32, rounded)."""
    parts = slab_partials(p["x"], p["w"], c.ks, c.split).reshape(-1, *p["gemm"].shape)
    s = len(parts)
    out = {"one split slab lost": emulate_y(p, dtype, gemm=p["gemm"] - parts[s // 2])}
    NB = sum_partials_nb(s, slab_bits)
    clamped = -(-s // NB) * NB - s                              # loads of the last batch that re-read the last slab
    if clamped:
        out[f"the last slab added once per clamped load (NB = {NB})"] = emulate_y(p, dtype, gemm=p["gemm"] + clamped * parts[-1])
    if p["bias_nc"] is not None and c.N > 1:
        out["bias_nc rows rolled by one image"] = emulate_y(p, dtype, bias_nc=np.roll(p["bias_nc"], -1, axis=0))
    return out
