"""Conv ADDRESSING of the tap-by-tap GEMM kernels -- k_igemm in every ring form and tile, k_igemm_patch, the conv form of k_igemm_pp, k_igemm8 -- on
small-integer inputs whose answer is exact in fp32 and in the 16-bit output, so that the GPU test (tests/test_gpu_conv_geometry.py) compares with
np.array_equal instead of a tolerance.  Host code, numpy only; tests/test_conv_geometry_host.py checks every claim made here on the CPU.

INPUTS (inputs(case), seeded by the case's name; NHWC / KRSC as the C ABI takes them).  x, x2, x3, x4 and w hold integers of {-1, 0, 1}, bias of
  [-4, 4], bias_nc of [-3, 3], the residual of [-8, 8].  Every product and every fp32 partial sum is an integer far below 2^24; the result is exact in
  float16 while |y| < 2048 and in bfloat16 while |y| <= 256.  exact_cap(case, dtype) asserts that on the reference -- a condition of the table, not a
  tolerance: a sum of K products of {-1, 0, 1} values has sigma = (4 K / 9)^0.5, about 30 at K = 2048, so 256 is more than 7 sigma; bfloat16 rows keep
  K <= 2048.  A split-K slab holds a sub-sum of the same kind: exact in an fp16 slab as well.
REFERENCE (reference(case)).  The convolution by its definition in int64: zero padding written out, nearest-2x up-sampling as x[:, h >> 1, w >> 1],
  one strided slice per (r, s) tap of the concat x | x2, then the extra 1x1 segment -- x3 | x4 are N x H x W tensors sampled at (ho stride, wo stride),
  zero outside -- then bias, bias_nc[n stride_nc + o] and the residual.  gather(case) computes the same thing the way the kernels address it (one
  flat offset per (output pixel, k)); the host test holds the two against each other, and gather(case, slip) is the wrong convolution of one slip.
MUTANTS (mutants(case)): the slips of MUTANTS below that apply to the case, each a plausible mistake in stage() / the patch gather / the epilogue.
FORM (predict_form(case)): the dispatcher's rules, stated once: eff_splitk, igemm_ring_form, patch_setup's admission, pp_ok.  .row is the (bm, bn,
  splitk, variant) tf_prof_dump must show -- the split and the family ASKED for, which is what the row holds (tests/test_gpu_splitk_slabs.py pins
  that) -- .eff the split the launch really runs with (the reduce family's counters show it), .kernel the instance that runs.
CASES: the table; REFUSALS: launches that must fail by name and leave y alone."""
import collections
import functools
import zlib

import numpy as np

SENTINEL = 1234.5                      # exact in float16 (and 1232 after bfloat16 rounding: both beyond every cap below or no integer)
GUARD = 64
CAP = {"fp16": 2047, "bf16": 256}
BOTH, F16 = ("fp16", "bf16"), ("fp16",)
E_ARG, E_UNSUPPORTED = 10001, 10002
V_RING, V_WIDE, V_PATCH, V_ALL8, V_PP = 0, 1, 2, 3, 4
FAMILY_BIT = {"igemm": None, "patch": 128, "pp": 512, "igemm8": 8}
ORDER_BITS = (32, 64)
E4M3 = {-1: 0xB8, 0: 0x00, 1: 0x38}

Case = collections.namedtuple("Case", "name family dtypes N H W C1 C2 Cout R S stride pad ups C3 C4 bm bn split dbg nc res slabs rounds wscale")
Form = collections.namedtuple("Form", "row eff kernel ring patch pt_ns")

# (R, S, stride, pad, upsample) by name
GEO = {
    "3x3s1p1": (3, 3, 1, 1, 0), "3x3s2p1": (3, 3, 2, 1, 0), "3x3s2p0": (3, 3, 2, 0, 0), "3x3s1p0": (3, 3, 1, 0, 0), "3x3s1p2": (3, 3, 1, 2, 0),
    "1x1s1p0": (1, 1, 1, 0, 0), "1x1s2p0": (1, 1, 2, 0, 0), "1x1s1p1": (1, 1, 1, 1, 0), "2x2s1p0": (2, 2, 1, 0, 0), "1x3s1p1": (1, 3, 1, 1, 0),
    "3x1s1p1": (3, 1, 1, 1, 0), "3x3up": (3, 3, 1, 1, 1), "3x3ups2": (3, 3, 2, 1, 1),
}


def geo_of(c):
    return next(k for k, v in GEO.items() if v == (c.R, c.S, c.stride, c.pad, c.ups))


def out_hw(c):
    return ((c.H << c.ups) + 2 * c.pad - c.R) // c.stride + 1, ((c.W << c.ups) + 2 * c.pad - c.S) // c.stride + 1


def dims(c):
    """(Ho, Wo, M, C, Kc, K)"""
    Ho, Wo = out_hw(c)
    C = c.C1 + c.C2
    return Ho, Wo, c.N * Ho * Wo, C, c.R * c.S * C, c.R * c.S * C + c.C3 + c.C4


def nc_stride(c):
    return {"none": 0, "zero": 0, "cout": c.Cout, "padded": -(-c.Cout // 4) * 4 + 4}[c.nc]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(c):
    """dict of int64 arrays (None where the case has no such operand): x (N, H, W, C1), x2, x3, x4, w (Cout, K: the KRSC row, then the 1x1 row), bias
    (Cout), bias_nc (the flat buffer the entry is given: one row for stride 0, N rows of stride elements otherwise; padding lanes hold 7), res
    (N, Ho, Wo, Cout), wscale (Cout) float64 or None."""
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    Ho, Wo, M, C, Kc, K = dims(c)
    tri = lambda *shape: rng.integers(-1, 2, size=shape, dtype=np.int64)
    p = {"x": tri(c.N, c.H, c.W, c.C1), "x2": tri(c.N, c.H, c.W, c.C2) if c.C2 else None, "x3": tri(c.N, c.H, c.W, c.C3) if c.C3 else None,
         "x4": tri(c.N, c.H, c.W, c.C4) if c.C4 else None, "w": tri(c.Cout, K), "bias": rng.integers(-4, 5, size=(c.Cout,), dtype=np.int64)}
    st = nc_stride(c)
    if c.nc == "none":
        p["bias_nc"] = None
    elif c.nc == "zero":
        p["bias_nc"] = rng.integers(-3, 4, size=(c.Cout,), dtype=np.int64)
    else:
        rows = np.full((c.N, st), 7, np.int64)
        rows[:, :c.Cout] = rng.integers(-3, 4, size=(c.N, c.Cout), dtype=np.int64)
        p["bias_nc"] = rows.reshape(-1)
    p["res"] = rng.integers(-8, 9, size=(c.N, Ho, Wo, c.Cout), dtype=np.int64) if c.res else None
    p["wscale"] = 2.0 ** ((np.arange(c.Cout) % 5) - 2) if c.wscale == "pow2" else None   # neighbours, and rows 1 .. 4 apart, differ
    for v in p.values():
        if v is not None:
            v.setflags(write=False)
    return p


def _epilogue(c, p, y, nc_index_stride=None):
    """y (N, Ho, Wo, Cout) of the GEMM part -> + bias + bias_nc[n stride + o] + residual (wscale first, where the case has one)."""
    if p["wscale"] is not None:
        y = y * p["wscale"]
    y = y + p["bias"]
    if p["bias_nc"] is not None:
        st = nc_stride(c) if nc_index_stride is None else nc_index_stride
        idx = np.arange(c.N)[:, None] * st + np.arange(c.Cout)[None, :]
        y = y + p["bias_nc"][idx][:, None, None, :]
    if p["res"] is not None:
        y = y + p["res"]
    return y


@functools.lru_cache(maxsize=None)
def reference(c):
    """the convolution by its definition (module docstring); int64 (float64 for the one case with power-of-two weight scales)."""
    p = inputs(c)
    Ho, Wo, M, C, Kc, K = dims(c)
    xs = p["x"] if not c.C2 else np.concatenate([p["x"], p["x2"]], axis=-1)
    if c.ups:
        xs = xs[:, np.arange(2 * c.H) >> 1][:, :, np.arange(2 * c.W) >> 1]
    Hl, Wl = xs.shape[1:3]
    xp = np.zeros((c.N, Hl + 2 * c.pad, Wl + 2 * c.pad, C), np.int64)
    xp[:, c.pad:c.pad + Hl, c.pad:c.pad + Wl] = xs
    wk = p["w"][:, :Kc].reshape(c.Cout, c.R, c.S, C)
    y = np.zeros((c.N, Ho, Wo, c.Cout), np.int64)
    for r in range(c.R):
        for s in range(c.S):
            tap = xp[:, r:r + (Ho - 1) * c.stride + 1:c.stride, s:s + (Wo - 1) * c.stride + 1:c.stride]
            y += tap @ wk[:, r, s].T
    if c.C3:
        e = p["x3"] if not c.C4 else np.concatenate([p["x3"], p["x4"]], axis=-1)
        samp = np.zeros((c.N, Ho, Wo, c.C3 + c.C4), np.int64)
        hs, ws = np.arange(Ho) * c.stride, np.arange(Wo) * c.stride
        nh, nw = int((hs < c.H).sum()), int((ws < c.W).sum())
        samp[:, :nh, :nw] = e[:, hs[:nh]][:, :, ws[:nw]]
        y += samp @ p["w"][:, Kc:].T
    y = _epilogue(c, p, y)
    y.setflags(write=False)
    return y


def exact_cap(c, dtype):
    """the condition under which array_equal is the right comparison: every output within the type's exact range, and unchanged by rounding to it."""
    y = reference(c)
    assert dtype in c.dtypes, (c.name, dtype)
    assert np.abs(y).max() <= CAP[dtype], (c.name, dtype, float(np.abs(y).max()))
    assert dims(c)[5] <= 2048 or dtype == "fp16", (c.name, "bfloat16 rows keep K <= 2048")
    y32 = np.asarray(y, np.float32)
    if dtype == "fp16":
        back = y32.astype(np.float16).astype(np.float64)
    else:
        back = (y32.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)     # truncation: exact iff the low 16 bits are 0
    assert np.array_equal(back, np.asarray(y, np.float64)), (c.name, dtype)
    assert not np.any(np.asarray(y, np.float64) == SENTINEL)
    return True


# ---- the addressing engine and its slips -------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "rs_swapped": "r and s swapped",
    "tap_div_R": "tap decoded with R instead of S",
    "pad_one_axis": "pad applied to the rows only",
    "stride_one_axis": "stride applied to the rows only",
    "ups_round_up": "(hi + 1) >> 1 for the up-sampled source",
    "ups_bounds_HW": "up-sampling bounds taken from H, W instead of H << 1, W << 1",
    "row_wrap": "wi = -1 reads the previous row's last pixel instead of zero",
    "image_base_of_tile": "every row of a tile takes the image base of the tile's first row",
    "x2_pitch_C1": "x2 read with x's channel pitch",
    "seam_chunk_source": "the first 16-byte chunk behind the concat seam taken from x",
    "last_ktile_dropped": "the last, partial K tile dropped",
    "ktile_chunk_dup": "the first chunk of K tile 1 repeats the last chunk of K tile 0",
    "extra_at_ho_wo": "extra segment sampled at (ho, wo) instead of (ho stride, wo stride)",
    "x4_seam_plus8": "the x3 | x4 seam of the extra segment 8 channels late",
    "bias_nc_index_Cout": "bias_nc indexed with Cout instead of its stride",
    "col_tail_shift": "the output column tail (N % 8 != 0) shifted by one",
    "rows_beyond_S_masked": "tap validity kept for S x S taps: the filter rows r >= S of an R x S filter, R > S, read zero",
    "extra_unbounded": "extra segment read without the bounds check: a sample point beyond H or W runs on into the next row / image",
}


def _straddles(c):
    Ho, Wo, M = dims(c)[:3]
    m0 = np.arange(0, M, c.bm)
    return bool(np.any(m0 // (Ho * Wo) != (np.minimum(m0 + c.bm, M) - 1) // (Ho * Wo)))


def applies(c, slip):
    Ho, Wo, M, C, Kc, K = dims(c)
    return {
        "rs_swapped": c.R * c.S > 1, "tap_div_R": c.R != c.S, "pad_one_axis": c.pad > 0, "stride_one_axis": c.stride > 1, "ups_round_up": c.ups == 1,
        "ups_bounds_HW": c.ups == 1, "row_wrap": c.pad > 0, "image_base_of_tile": _straddles(c), "x2_pitch_C1": c.C2 > 0 and c.C1 != c.C2,
        "seam_chunk_source": c.C2 > 0, "last_ktile_dropped": K % 64 != 0 and K > 64, "ktile_chunk_dup": K > 64, "extra_at_ho_wo": c.C3 > 0 and c.stride > 1,
        "x4_seam_plus8": c.C4 > 0, "bias_nc_index_Cout": c.nc == "padded" and c.N > 1, "col_tail_shift": c.Cout % 8 >= 2,
        "rows_beyond_S_masked": c.R > c.S, "extra_unbounded": c.C3 > 0 and ((Ho - 1) * c.stride >= c.H or (Wo - 1) * c.stride >= c.W),
    }[slip]


def gather(c, slip=None):
    """the same convolution the way the kernels address it: A[m, k] = flat[base(source(k)) + pixel(m, k) pitch(k) + channel(k)] where the tap lies inside
    the (up-sampled) image, 0 elsewhere and beyond the source tensor (the buffer descriptor's range check); y = A w^T, then the epilogue.  `slip`: one of
    MUTANTS.  Returns int64 / float64 like reference()."""
    assert slip is None or slip in MUTANTS, slip
    p = inputs(c)
    Ho, Wo, M, C, Kc, K = dims(c)
    HoWo = Ho * Wo
    m = np.arange(M)
    img = m // HoWo
    rem = m - img * HoWo
    ho, wo = rem // Wo, rem % Wo
    base_img = ((m // c.bm) * c.bm) // HoWo if slip == "image_base_of_tile" else img
    sh, sw = c.stride, (1 if slip == "stride_one_axis" else c.stride)
    ph, pw = c.pad, (0 if slip == "pad_one_axis" else c.pad)
    k = np.arange(K)
    extra = k >= Kc
    kk = np.where(extra, 0, k)
    tap = kk // C
    ch = kk - tap * C
    if slip == "tap_div_R":
        r = tap // c.R
        s = tap - r * c.R
    else:
        r = tap // c.S
        s = tap - r * c.S
    if slip == "rs_swapped":
        r, s = s, r
    second = ch >= c.C1
    src = np.where(second, 1, 0)
    ld = np.where(second, c.C1 if slip == "x2_pitch_C1" else c.C2, c.C1)
    cc = np.where(second, ch - c.C1, ch)
    if slip == "seam_chunk_source" and c.C2:
        seam = second & (ch < c.C1 + 8)
        src, ld, cc = np.where(seam, 0, src), np.where(seam, c.C1, ld), np.where(seam, ch, cc)
    e = k - Kc
    second_e = e >= c.C3 + (8 if slip == "x4_seam_plus8" else 0)
    src = np.where(extra, np.where(second_e, 3, 2), src)
    ld = np.where(extra, np.where(second_e, c.C4, c.C3), ld)
    cc = np.where(extra, np.where(second_e, e - c.C3, e), cc)
    r, s = np.where(extra, ph, r), np.where(extra, pw, s)        # the output pixel itself: hi = ho stride
    hi = ho[:, None] * sh - ph + r[None, :]
    wi = wo[:, None] * sw - pw + s[None, :]
    if slip == "extra_at_ho_wo":
        hi, wi = np.where(extra[None, :], ho[:, None], hi), np.where(extra[None, :], wo[:, None], wi)
    Hl, Wl = (c.H, c.W) if slip == "ups_bounds_HW" else (c.H << c.ups, c.W << c.ups)
    ok = (hi >= 0) & (hi < Hl) & (wi >= (-1 if slip == "row_wrap" else 0)) & (wi < Wl)
    if slip == "rows_beyond_S_masked":
        ok &= (extra | (r < c.S))[None, :]
    if slip == "extra_unbounded":
        ok |= extra[None, :]
    up = (lambda v: (v + 1) >> 1) if slip == "ups_round_up" else (lambda v: v >> c.ups)
    pix = base_img[:, None] * (c.H * c.W) + up(hi) * c.W + up(wi)
    off = pix * ld[None, :] + cc[None, :]
    parts = [p["x"].reshape(-1)] + [p[n].reshape(-1) if p[n] is not None else np.zeros(0, np.int64) for n in ("x2", "x3", "x4")]
    size = np.array([a.size for a in parts])
    base = np.concatenate([[0], np.cumsum(size)[:-1]])
    flat = np.concatenate(parts)
    ok &= (off >= 0) & (off < size[src][None, :])
    A = np.where(ok, flat[np.clip(base[src][None, :] + off, 0, flat.size - 1)], 0).astype(np.float64)
    if slip == "last_ktile_dropped":
        A[:, (K // 64) * 64:] = 0
    if slip == "ktile_chunk_dup":
        A[:, 64:72] = A[:, 56:64]
    y = np.rint(A @ p["w"].astype(np.float64).T).astype(np.int64).reshape(c.N, Ho, Wo, c.Cout)      # (float64 products of small integers: exact)
    y = _epilogue(c, p, y, c.Cout if slip == "bias_nc_index_Cout" else None)
    if slip == "col_tail_shift":
        t0, good = c.Cout // 8 * 8, y
        y = good.copy()
        y[..., t0 + 1:] = good[..., t0:-1]
    return y


def mutants(c):
    """{name: wrong output} for every slip of MUTANTS that applies to the case."""
    return {name: gather(c, name) for name in MUTANTS if applies(c, name)}


# ---- the dispatcher's rules (csrc/gemm_family.h, csrc/gemm_common.h, csrc/gemm.hip) ---------------------------------------------------------------------
def eff_splitk(K, split):
    kt = -(-K // 64)
    kps = -(-kt // max(split, 1))
    return -(-kt // kps)


def split_ranges(K, split):
    kt = -(-K // 64)
    kps = -(-kt // max(split, 1))
    return [(z * kps * 64, min(K, (z + 1) * kps * 64)) for z in range(-(-kt // kps))]


def generic(c):
    return any(v % 64 for v in (c.C1, c.C2, c.C3, c.C4))


def igemm_ring_form(bm, bn, wide, all8, gen):
    if bm == 256:
        return V_RING
    if all8 and not gen:
        return V_ALL8
    return V_WIDE if wide and not (bm == 128 and bn == 160) else V_RING


def patch_setup(c):
    """pt_ns of k_igemm_patch for the case's tile, or 0 where patch_setup refuses (such a launch runs the deep ring)."""
    Ho, Wo = out_hw(c)
    if (c.R, c.S, c.stride, c.pad, c.ups) != (3, 3, 1, 1, 0) or generic(c) or c.family == "igemm8":
        return 0
    if not (c.bm in (64, 128) and c.bn in (128, 160)):
        return 0
    if c.W & (c.W - 1) or c.W < 8 or c.W > c.bm or (Ho * Wo) % c.bm:
        return 0
    ppc = ((c.bm // c.W + 2) * (c.W + 2) + 7) // 8
    if (ppc + 3) // 4 > 9:
        return 0
    stage = c.bn * 128 + (c.bm * 128 if c.C3 + c.C4 else 0)
    ns = min((163840 - 2 * ppc * 1024) // stage, 5)
    return ns if ns >= 3 else 0


def pp_ok(c):
    Ho, Wo = out_hw(c)
    if c.bn not in (128, 160, 256) or not (c.bm == 256 or (c.bm == 192 and c.bn != 256)) or generic(c):
        return False
    return not (c.nc != "none" and Ho * Wo < c.bm)


def pp_fast(c):
    """the lean addressing of k_igemm_pp: a fixed pixel shift per tap -- stride 1, no up-sampling, a square filter of at most 31 taps, and extra sources
    whose every sample point lies inside the image (Ho <= H, Wo <= W)."""
    Ho, Wo = out_hw(c)
    return c.stride == 1 and not c.ups and c.S * c.S <= 31 and c.R == c.S and not (c.C3 and (Ho > c.H or Wo > c.W))


def predict_form(c):
    Ho, Wo, M, C, Kc, K = dims(c)
    eff = eff_splitk(K, c.split)
    gen, ring, ns = generic(c), None, 0
    grid = "GENERIC" if gen else "grid64"
    bits = c.dbg & ~(ORDER_BITS[0] | ORDER_BITS[1] | 8192)
    if c.family == "igemm":
        assert bits in (8, 16, 256), c
        variant = {8: V_RING, 16: V_WIDE, 256: V_ALL8}[bits]
        assert (c.bm in (64, 128) and c.bn in (64, 128, 160)) or ((c.bm, c.bn) == (256, 128) and not gen), c
        ring = igemm_ring_form(c.bm, c.bn, variant == V_WIDE, variant == V_ALL8, gen)
        kernel = f"k_igemm<{c.bm},{c.bn},{grid},{('ring', 'wide', None, 'all8')[ring]}>"
    elif c.family == "patch":
        assert bits == 128, c
        variant, ns = V_PATCH, patch_setup(c)
        kernel = f"k_igemm_patch<{c.bm},{c.bn}>" if ns else f"k_igemm<{c.bm},{c.bn},{grid},ring>"
    elif c.family == "pp":
        assert bits == 512 and pp_ok(c), c
        can1 = 163840 // ((c.bm + c.bn) * 128) >= 3
        assert can1 or c.bm == 256, c
        np_ = 1 if can1 and not (c.dbg & 8192) else 2
        assert not (c.dbg & 8192) or (can1 and c.bm == 256), (c, "the 8192 bit belongs on a tile with both forms")
        variant, kernel = V_PP, f"k_igemm_pp<{c.bm},{c.bn},NP{np_},{'lean' if pp_fast(c) else 'gather'}>"
    else:
        assert c.family == "igemm8" and bits == 8 and not gen and not c.C3 and c.R == c.S, c
        assert (c.bm, c.bn) in ((128, 128), (64, 128), (128, 64), (256, 64), (64, 64)), c
        variant, kernel = V_RING, f"k_igemm8<{c.bm},{c.bn}>"
    return Form((c.bm, c.bn, c.split, variant), eff, kernel, ring, 1 if ns else 0, ns)


# ---- the case table ------------------------------------------------------------------------------------------------------------------------------------
def case(family, geo, shape, Cs, Cout, tile, dbg, split=1, ex=(0, 0), nc="none", res=False, slabs=16, rounds=False, wscale="ones", dtypes=None):
    R, S, stride, pad, ups = GEO[geo]
    N, H, W = shape
    C1, C2 = Cs
    dtypes = dtypes or (F16 if family == "igemm8" else BOTH)
    name = (f"{family}-{geo}-{N}x{H}x{W}-c{C1}+{C2}-o{Cout}-e{ex[0]}+{ex[1]}-{tile[0]}x{tile[1]}s{split}-d{dbg}-{nc}{'-res' if res else ''}"
            f"{'-f32slabs' if slabs == 32 else ''}{'-wscale' if wscale != 'ones' else ''}")
    return Case(name, family, dtypes, N, H, W, C1, C2, Cout, R, S, stride, pad, ups, ex[0], ex[1], tile[0], tile[1], split, dbg, nc, res, slabs, rounds, wscale)


IGEMM_TILES = ((64, 64), (64, 128), (64, 160), (128, 64), (128, 128), (128, 160))
# every geometry of the issue with the image it runs on: HoWo < 64 with N = 3 images, so that tiles hold several images, straddle one mid-row and end ragged
GEOMETRIES = (("3x3s1p1", (3, 9, 7)), ("3x3s2p1", (3, 9, 7)), ("3x3s2p1", (3, 8, 8)), ("3x3s2p0", (3, 9, 9)), ("3x3s2p0", (3, 10, 8)), ("3x3s1p0", (3, 9, 7)),
              ("3x3s1p2", (3, 6, 5)), ("1x1s1p0", (3, 9, 7)), ("1x1s2p0", (3, 9, 7)), ("1x1s1p1", (3, 7, 5)), ("2x2s1p0", (3, 9, 7)), ("1x3s1p1", (3, 9, 7)),
              ("3x1s1p1", (3, 9, 7)), ("3x3up", (3, 5, 4)), ("3x3up", (2, 4, 4)), ("3x3ups2", (3, 5, 4)))
GRID_COUNTS = ((64, 0), (128, 0), (64, 64))
GENERIC_COUNTS = ((8, 0), (24, 0), (72, 0), (40, 32), (64, 8))
COUTS = (4, 6, 72, 136, 200, 64, 128, 160)
NC_MODES = ("none", "zero", "cout", "padded")


def _igemm_cover():
    rows, i = [], 0

    def add(tile, bit, Cs):
        nonlocal i
        geo, shape = GEOMETRIES[i % len(GEOMETRIES)]
        order = (0, 32, 64)[i % 3]
        j = i
        while True:                                            # (the walk may meet a row it already made: the next output width then)
            row = case("igemm", geo, shape, Cs, COUTS[j % len(COUTS)], tile, bit | order, nc=NC_MODES[i % 4], res=i % 3 == 1)
            if row.name not in {q.name for q in rows}:
                break
            j += 1
        rows.append(row)
        i += 1
    for tile in IGEMM_TILES:                                   # every tile in every form on the 64 grid
        for bit in (8, 16, 256):
            add(tile, bit, GRID_COUNTS[i % 3])
    for rep in range(2):                                       # ring and wide on GENERIC counts, twice over: 24 rows walk the 16 geometries and the 5 counts
        for tile in IGEMM_TILES:
            for bit in (8, 16):
                add(tile, bit, GENERIC_COUNTS[(i + rep) % 5])
    for k in range(14):                                        # the rest of geometry x grid: every geometry has met a 64-grid count and a GENERIC one
        add(IGEMM_TILES[(k * 5 + 1) % 6], (8, 16, 256)[k % 3], GRID_COUNTS[k % 3])
    return rows


CASES = _igemm_cover() + [
    # the 256 x 128 tile of k_igemm (deep ring only, 64-grid counts only): five 9 x 7 images in one 256-row tile and a ragged second one
    case("igemm", "3x3s1p1", (5, 9, 7), (64, 0), 136, (256, 128), 8, nc="cout", res=True),
    case("igemm", "3x3s2p1", (5, 16, 15), (64, 64), 72, (256, 128), 8 | 64, nc="padded"),
    case("igemm", "3x3up", (5, 5, 4), (128, 0), 200, (256, 128), 16 | 32, nc="zero"),                  # (asked wide: the tile has the deep ring only)
    case("igemm", "1x1s2p0", (5, 9, 7), (64, 0), 6, (256, 128), 256, res=True),
    case("igemm", "3x1s1p1", (5, 9, 7), (64, 0), 128, (256, 128), 8, split=2, nc="cout"),
    # M edges: M < bm; one image, ragged; N = 1
    case("igemm", "3x3s1p1", (1, 9, 7), (24, 0), 72, (64, 64), 8, nc="zero"),
    case("igemm", "3x3s1p1", (1, 9, 7), (64, 0), 72, (128, 128), 256),
    case("igemm", "3x3s2p1", (1, 9, 7), (40, 32), 6, (128, 160), 8, res=True),
    case("igemm", "1x3s1p1", (2, 11, 13), (72, 0), 136, (64, 160), 16, nc="padded"),
    case("igemm", "3x1s1p1", (2, 11, 13), (64, 8), 4, (128, 64), 8 | 64, nc="padded", res=True),
    # split-K: splits 2 and 3 with ragged K tiles; cuts inside a tap on GENERIC counts (K = 648: 11 K tiles, cuts at k = 384 / 256, 512: taps of 72),
    # inside the extra segment (1x1 of 64 + 64 | 64: cuts at k = 64, 128; 1x1 of 8 + 72 | 0: the cut at k = 64 is channel 56 of x3), fp16 and fp32 slabs
    case("igemm", "3x3s1p1", (3, 9, 7), (72, 0), 72, (64, 64), 8, split=2, nc="cout", res=True),
    case("igemm", "3x3s1p1", (3, 9, 7), (72, 0), 136, (64, 128), 16 | 32, split=3, nc="zero"),
    case("igemm", "3x3s2p1", (3, 9, 7), (40, 32), 200, (128, 160), 8, split=3, slabs=32, nc="padded", res=True),
    case("igemm", "3x3s1p1", (3, 9, 7), (64, 8), 6, (128, 64), 16, split=2, nc="cout"),                # (N % 8 != 0: fp32 slabs whatever was asked)
    case("igemm", "1x1s1p0", (3, 9, 7), (64, 0), 72, (64, 64), 8, split=3, ex=(64, 64), nc="cout"),
    case("igemm", "1x1s1p0", (3, 9, 7), (64, 0), 136, (128, 128), 256, split=2, ex=(64, 64), res=True),
    case("igemm", "1x1s2p0", (3, 9, 7), (8, 0), 72, (64, 160), 8 | 64, split=2, ex=(72, 0), slabs=32),
    case("igemm", "1x1s1p0", (3, 9, 7), (72, 0), 200, (64, 128), 16, split=2, ex=(24, 8), nc="padded"),
    case("igemm", "3x3s1p1", (3, 9, 7), (64, 64), 128, (64, 160), 256 | 32, split=3, ex=(64, 64), slabs=32, res=True),
    case("igemm", "3x3up", (3, 5, 4), (128, 0), 72, (128, 160), 256, split=2, nc="zero"),
    case("igemm", "2x2s1p0", (3, 9, 7), (64, 0), 64, (128, 64), 16, split=3, rounds=True),              # 4 K tiles in 3: two per split, so two splits
    case("igemm", "3x3s1p1", (3, 9, 7), (24, 0), 4, (64, 64), 8, split=3, rounds=True, nc="padded"),    # 4 K tiles in 3: two splits
    # the extra 1x1 sources: on the 64 grid and off it, at stride 1 and stride 2, with and without the residual, every bias_nc mode
    case("igemm", "3x3s1p1", (3, 9, 7), (64, 0), 72, (64, 64), 8, ex=(64, 64), nc="padded", res=True),
    case("igemm", "3x3s2p1", (3, 9, 7), (64, 0), 136, (128, 128), 16, ex=(64, 64), nc="zero"),
    case("igemm", "3x3s2p0", (3, 10, 8), (64, 64), 128, (64, 128), 256 | 64, ex=(64, 64), res=True),
    case("igemm", "3x3s1p1", (3, 9, 7), (24, 0), 72, (64, 160), 8, ex=(24, 8), res=True),
    case("igemm", "3x3s2p1", (3, 8, 8), (72, 0), 6, (128, 64), 16, ex=(24, 8), nc="cout"),
    case("igemm", "3x3s2p1", (3, 9, 7), (40, 32), 136, (64, 64), 8 | 32, ex=(72, 0), nc="padded"),
    case("igemm", "1x1s2p0", (3, 9, 7), (64, 8), 200, (128, 160), 8, ex=(24, 8), res=True),
    case("igemm", "3x3s1p2", (3, 6, 5), (64, 0), 64, (64, 128), 8, ex=(72, 0), nc="zero"),            # Ho = H + 2: the sample points beyond H, W read zero
    case("igemm", "3x3s1p0", (3, 9, 7), (8, 0), 4, (64, 64), 16, ex=(24, 8), nc="padded", res=True),
    # k_igemm_patch (bit 128): its four tiles, W = 8 / 16 / 32 / 64 with H != W, concat, extras, split 1 / 2 / 3, pt_ns = 3 / 4 / 5
    case("patch", "3x3s1p1", (2, 24, 8), (64, 0), 136, (64, 128), 128, nc="cout", res=True),
    case("patch", "3x3s1p1", (2, 8, 16), (64, 64), 200, (128, 160), 128 | 64, nc="padded"),
    case("patch", "3x3s1p1", (2, 4, 32), (128, 0), 72, (128, 128), 128, split=2, nc="zero"),
    case("patch", "3x3s1p1", (1, 4, 64), (64, 0), 160, (64, 160), 128 | 32, split=3, slabs=32, res=True),
    case("patch", "3x3s1p1", (2, 2, 64), (64, 0), 128, (128, 128), 128, res=True),
    case("patch", "3x3s1p1", (2, 16, 8), (64, 0), 136, (128, 160), 128, ex=(64, 64), nc="cout"),                   # pt_ns = 3
    case("patch", "3x3s1p1", (2, 24, 8), (64, 64), 72, (64, 160), 128, ex=(64, 0), split=2, res=True),            # pt_ns = 4
    case("patch", "3x3s1p1", (3, 8, 16), (64, 0), 6, (64, 128), 128, ex=(64, 64), split=3, nc="padded"),
    case("patch", "3x3s1p1", (2, 8, 32), (64, 64), 64, (128, 128), 128, split=3, nc="cout", res=True),
    # ... on a stride-2 conv it is not refused: the family's table runs the deep ring (tf_conv2d_patch_admits says 0, the row still says variant 2)
    case("patch", "3x3s2p1", (2, 16, 16), (64, 0), 72, (64, 128), 128, nc="cout"),
    case("patch", "3x3s1p1", (3, 9, 7), (64, 0), 72, (64, 128), 128, res=True),                                      # W no power of two: the deep ring
    # k_igemm_pp as a conv (bit 512): five tiles, the 8192 bit on the two three-slot 256-row tiles; the lean addressing (stride 1, no up-sampling,
    # square filters) and the general gather; bias_nc only where HoWo >= bm (pp_ok)
    case("pp", "3x3s1p1", (2, 16, 16), (64, 0), 136, (256, 128), 512, nc="cout", res=True),
    case("pp", "3x3s1p1", (2, 16, 17), (64, 64), 200, (256, 160), 512 | 8192, nc="padded"),
    case("pp", "3x3s1p1", (3, 9, 7), (64, 0), 72, (256, 256), 512, res=True),
    case("pp", "3x3s2p1", (5, 16, 15), (64, 0), 136, (192, 128), 512 | 64, res=True),
    case("pp", "3x3s2p0", (5, 17, 16), (64, 64), 72, (256, 128), 512 | 8192),
    case("pp", "3x3up", (2, 8, 8), (64, 0), 200, (192, 160), 512, nc="zero"),
    case("pp", "3x3up", (3, 5, 4), (128, 0), 160, (256, 160), 512, res=True),
    case("pp", "3x3ups2", (3, 9, 8), (64, 0), 72, (256, 256), 512 | 32),
    case("pp", "1x1s1p0", (2, 16, 16), (128, 0), 136, (256, 256), 512, nc="cout"),
    case("pp", "1x1s2p0", (3, 18, 14), (64, 64), 6, (192, 128), 512, res=True),
    case("pp", "3x3s1p1", (2, 16, 12), (64, 0), 72, (192, 160), 512, ex=(64, 64), nc="padded", res=True),
    case("pp", "3x3s2p1", (3, 16, 16), (64, 0), 136, (256, 128), 512, ex=(64, 0)),
    case("pp", "3x3s1p1", (2, 16, 16), (64, 64), 128, (256, 160), 512, split=2, nc="cout", res=True),
    case("pp", "1x1s1p0", (2, 16, 13), (64, 0), 200, (192, 128), 512, split=2, ex=(64, 64), slabs=32),
    case("pp", "3x3s1p0", (3, 9, 7), (64, 0), 72, (256, 128), 512),
    case("pp", "3x3s1p2", (3, 6, 5), (128, 0), 136, (192, 160), 512, res=True),
    case("pp", "2x2s1p0", (3, 9, 7), (64, 0), 64, (256, 160), 512 | 8192),
    case("pp", "1x1s1p1", (3, 7, 5), (64, 0), 72, (192, 128), 512),
    case("pp", "1x3s1p1", (3, 9, 7), (64, 0), 136, (256, 128), 512, res=True),
    case("pp", "3x1s1p1", (3, 9, 7), (64, 0), 72, (256, 160), 512, res=True),
    case("pp", "3x1s1p1", (2, 16, 16), (64, 64), 64, (192, 128), 512, nc="zero"),
    # extras where Ho > H, Wo > W (stride 1, pad > (R - 1) / 2): the sample points beyond the image read zero -- on one- and two-phase tiles
    case("pp", "3x3s1p2", (3, 6, 5), (64, 0), 72, (256, 128), 512, ex=(64, 64), res=True),
    case("pp", "3x3s1p2", (2, 14, 14), (64, 0), 136, (256, 256), 512, ex=(64, 64), nc="cout"),
    case("pp", "1x1s1p1", (3, 7, 5), (64, 0), 72, (192, 160), 512, ex=(64, 0)),
    case("pp", "1x1s1p1", (2, 15, 15), (64, 64), 64, (256, 160), 512 | 8192, ex=(64, 0), nc="padded", res=True),
    # k_igemm8 through tf_conv2d_fp8: e4m3 codes of -1, 0, 1 written by the host; its five tiles
    case("igemm8", "3x3s1p1", (3, 9, 7), (64, 0), 136, (128, 128), 8, nc="cout", res=True),
    case("igemm8", "3x3s2p1", (3, 9, 7), (64, 0), 72, (64, 128), 8 | 64, nc="padded"),
    case("igemm8", "3x3up", (3, 5, 4), (128, 0), 200, (128, 64), 8, res=True),
    case("igemm8", "1x1s1p0", (5, 9, 7), (64, 0), 64, (256, 64), 8 | 32, nc="zero"),
    case("igemm8", "3x3s1p1", (3, 9, 7), (64, 64), 72, (64, 64), 8, res=True),
    case("igemm8", "3x3s1p1", (3, 9, 7), (64, 64), 136, (128, 128), 8, split=2, nc="cout"),
    case("igemm8", "3x3s2p0", (3, 10, 8), (64, 0), 6, (64, 64), 8, split=3, slabs=32, res=True),
    case("igemm8", "3x3s1p1", (3, 9, 7), (64, 0), 40, (64, 128), 8, wscale="pow2", nc="zero"),
    case("igemm8", "1x1s2p0", (5, 9, 7), (64, 64), 128, (256, 64), 8, res=True),
]

# rows whose bfloat16 run exact_cap excludes: none needs it at these sizes (the host test prints the count and fails if a 16-bit row is fp16-only without
# exceeding the bfloat16 cap)
FP16_ONLY = tuple(c.name for c in CASES if c.family != "igemm8" and c.dtypes == F16)


def required_instances():
    """the kernel instances the table must name (predict_form(c).kernel)."""
    need = {f"k_igemm<{bm},{bn},grid64,{f}>" for bm, bn in IGEMM_TILES for f in ("ring", "wide", "all8") if not (f == "wide" and (bm, bn) == (128, 160))}
    need |= {f"k_igemm<{bm},{bn},GENERIC,{f}>" for bm, bn in IGEMM_TILES for f in ("ring", "wide") if not (f == "wide" and (bm, bn) == (128, 160))}
    need |= {"k_igemm<256,128,grid64,ring>"}
    need |= {f"k_igemm_patch<{bm},{bn}>" for bm in (64, 128) for bn in (128, 160)}
    need |= {f"k_igemm_pp<{bm},{bn},NP1,{a}>" for bm, bn in ((256, 128), (256, 160), (192, 128), (192, 160)) for a in ("lean", "gather")}
    need |= {"k_igemm_pp<256,256,NP2,lean>", "k_igemm_pp<256,256,NP2,gather>", "k_igemm_pp<256,128,NP2,gather>", "k_igemm_pp<256,160,NP2,lean>"}
    need |= {f"k_igemm8<{bm},{bn}>" for bm, bn in ((128, 128), (64, 128), (128, 64), (256, 64), (64, 64))}
    return need


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
# (what, the case the launch is built from, overrides of the arguments, status, a piece of tf_last_error that names the entry / the family)
Refusal = collections.namedtuple("Refusal", "what case override rc says")
_R0 = case("igemm", "3x3s1p1", (2, 9, 7), (64, 0), 72, (64, 64), 8, nc="cout")
REFUSALS = [
    Refusal("C1 off the 8 grid", _R0, {"C1": 60}, E_ARG, b"tf_conv2d_f16: channel counts"),
    Refusal("C2 off the 8 grid", _R0._replace(C2=64), {"C2": 12}, E_ARG, b"tf_conv2d_f16: channel counts"),
    Refusal("empty output", _R0, {"H": 2, "pad": 0}, E_ARG, b"tf_conv2d_f16: empty output"),
    Refusal("C4 without C3", _R0._replace(C4=8), {}, E_ARG, b"tf_conv2d_fused_f16: extra sources"),
    Refusal("extras with upsample", _R0._replace(C3=64), {"ups": 1}, E_ARG, b"tf_conv2d_fused_f16: the extra 1x1 sources"),
    Refusal("bias_nc_stride off the 4 grid", _R0, {"nc_stride": 74}, E_ARG, b"tf_conv2d_f16: bias_nc_stride"),
    Refusal("ping-pong on GENERIC counts", case("pp", "3x3s1p1", (2, 16, 16), (72, 0), 72, (256, 128), 512), {}, E_UNSUPPORTED, b"ping-pong"),
    Refusal("ping-pong with bias_nc at HoWo < bm", case("pp", "3x3s1p1", (3, 9, 7), (64, 0), 72, (256, 128), 512, nc="cout"), {}, E_UNSUPPORTED, b"ping-pong"),
    Refusal("the 256 x 128 tile of k_igemm on GENERIC counts", case("igemm", "3x3s1p1", (5, 9, 7), (72, 0), 72, (256, 128), 8), {}, E_UNSUPPORTED, b"256x128"),
]
