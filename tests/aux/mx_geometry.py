"""Which E8M0 byte meets which 32 channels of which tap of which source tensor: the block-scaled e4m3 GEMMs -- k_igemm_pp<F8> in its four tiles with
half-tile slabs (H2) off and on, k_igemm_pp3<F8> on 96-, 48- and 24-pixel rows with and without the half slab -- on planted integers whose answer is
exact in fp32, in an fp16 split-K slab and in the fp16 output, so that tests/test_gpu_mx_geometry.py compares with np.array_equal.  Host code, numpy
only; tests/test_mx_geometry_host.py checks every claim made here on the CPU.

INPUTS (inputs(c), seeded with zlib.crc32 of the row's name; NHWC / KRSC as the C ABI takes them).  Activation codes and weights hold {-1, 0, 1} as
  e4m3 bytes (E4M3); every 32-channel block of every pixel draws its own scale byte from SCALE_BYTES = (126, 127, 128), i.e. 2^-1, 1, 2, and one block
  in eight is zero throughout with byte 0 (a neighbour that reads it multiplies by 2^-127).  wscale is the geometry table's pattern 2 ** ((n % 5) - 2) on
  most rows and ones on a few; bias of [-4, 4], bias_nc of [-3, 3] (strides `cout` and `padded`, padding lanes hold 7), the residual of [-8, 8].
EXACTNESS is a condition of the table (exact(c)), not a tolerance.  q = 1 (the smallest block scale) + 2 (the smallest wscale, where the row has the
  pattern): every value the epilogue could round -- the GEMM part, after wscale, after bias, after bias_nc, after the residual, and each split's partial
  sum after wscale -- must be a multiple of 2^-q of magnitude below 2^(11 - q), which fp16 holds exactly; the fp32 accumulator holds multiples of 2^-1
  far below 2^23.  The estimate behind the densities: a sum of K products x w s with P(x != 0) = P(w != 0) = d and E[s^2] = 7 / 4 has sigma =
  (7 K d^2 / 4)^0.5.  Rows with the wscale pattern need 4 |G| + 15 < 256, i.e. |G| < 60: d^2 = min(4 / 9, 36 / K) keeps sigma <= 8, seven and a half
  sigma where the largest of a row's 10^5 outputs lies near four and a half.  Rows with wscale = 1 need |G| + 15 < 1024: d = 2 / 3 gives sigma = 47 at
  K = 2880, twenty sigma.  density(c) is that rule.
REFERENCE (reference(c)): the convolution / linear by its definition in float64 on the dequantised operand code 2^(byte - 127), zero padding written
  out, one slice per tap of the concat x | x2; then wscale, bias, bias_nc[n stride + o], the residual.  gather(c) computes the same thing the way
  stage_act / stage_sc and the pp3 patch gather address it: per (output pixel, k) ONE flat code offset into the source's codes and ONE flat byte offset
  into the source's buffer (codes, then C / 32 scale bytes per pixel), out of range = 0; the host test holds the two against each other, and
  gather(c, slip) is the wrong answer of one slip.
MUTANTS: the slips, each one plausible mistake in the scale path, the K-tile bookkeeping or the epilogue; applies(c, slip) says where a row has the
  feature.  (`pad_wraps` wraps code AND scale: a padded tap's codes are zero, so its scale byte alone cannot show in any finite output.)
FORM (predict_form(c)): the dispatcher's rules for these launches, stated once -- 128-deep K tiles, eff_splitk, pp_ok, pp3_ok, the H2 choice of each
  launcher; .row is what tf_prof_dump must show, .eff the split the launch runs with, .kernel the instance.
CASES / LINEARS: the table (conv rows, tf_linear_mx8 rows); GEGLU: the block-scaled GEGLU output's shapes; REFUSALS."""
import collections
import functools
import zlib

import numpy as np

SENTINEL = 1234.5                      # exact in float16, beyond every bound of exact()
GUARD = 64
E_ARG, E_UNSUPPORTED = 10001, 10002
V_PP, V_PP3 = 4, 6
BIT = {"pp": 512, "pp3": 2048}
E4M3 = {-1: 0xB8, 0: 0x00, 1: 0x38}
SCALE_BYTES = (126, 127, 128)
TILES = ((192, 128), (192, 160), (256, 128), (256, 160))

Case = collections.namedtuple("Case", "name kind family N H W C1 C2 Cout R pad bm bn split dbg nc res bias slabs rounds wscale")
Form = collections.namedtuple("Form", "row eff kernel")

GEO = {"3x3p1": (3, 1), "3x3p0": (3, 0), "1x1p0": (1, 0), "1x1p1": (1, 1), "5x5p2": (5, 2)}


def geo_of(c):
    return next(k for k, v in GEO.items() if v == (c.R, c.pad))


def dims(c):
    """(Ho, Wo, M, C, K)"""
    Ho, Wo = c.H + 2 * c.pad - c.R + 1, c.W + 2 * c.pad - c.R + 1
    C = c.C1 + c.C2
    return Ho, Wo, c.N * Ho * Wo, C, c.R * c.R * C


def nc_stride(c):
    return {"none": 0, "cout": c.Cout, "padded": -(-c.Cout // 4) * 4 + 4}[c.nc]


def density(c):
    """P(code != 0) = P(weight != 0): the estimate of the module docstring."""
    K = dims(c)[4]
    return min(2.0 / 3.0, (36.0 / K) ** 0.5) if c.wscale == "pow2" else 2.0 / 3.0


def q_of(c):
    return 1 + (2 if c.wscale == "pow2" else 0)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------
def _blocks(rng, shape, C, d):
    """codes (shape + (C,)) of {-1, 0, 1} and scale bytes (shape + (C / 32,)); one block in eight is zero with byte 0."""
    x = rng.choice(np.array([-1, 0, 1], np.int64), size=shape + (C,), p=[d / 2, 1 - d, d / 2])
    sc = rng.choice(np.array(SCALE_BYTES, np.uint8), size=shape + (C // 32,))
    dead = rng.random(shape + (C // 32,)) < 0.125
    sc[dead] = 0
    x = np.where(np.repeat(dead, 32, axis=-1), 0, x)
    return x, sc


@functools.lru_cache(maxsize=None)
def inputs(c):
    """dict: x (N, H, W, C1) int64 of {-1, 0, 1}, xs (N, H, W, C1 / 32) uint8, x2 / x2s likewise or None, w (Cout, K) int64, wscale (Cout) float64,
    bias (Cout) or None, bias_nc (the flat buffer the entry is given, or None), res (N, Ho, Wo, Cout) or None."""
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    Ho, Wo, M, C, K = dims(c)
    d = density(c)
    p = {}
    p["x"], p["xs"] = _blocks(rng, (c.N, c.H, c.W), c.C1, d)
    p["x2"], p["x2s"] = _blocks(rng, (c.N, c.H, c.W), c.C2, d) if c.C2 else (None, None)
    p["w"] = rng.choice(np.array([-1, 0, 1], np.int64), size=(c.Cout, K), p=[d / 2, 1 - d, d / 2])
    p["wscale"] = 2.0 ** ((np.arange(c.Cout) % 5) - 2) if c.wscale == "pow2" else np.ones(c.Cout)
    p["bias"] = rng.integers(-4, 5, size=(c.Cout,), dtype=np.int64) if c.bias else None
    st = nc_stride(c)
    if c.nc == "none":
        p["bias_nc"] = None
    else:
        rows = np.full((c.N, st), 7, np.int64)
        rows[:, :c.Cout] = rng.integers(-3, 4, size=(c.N, c.Cout), dtype=np.int64)
        p["bias_nc"] = rows.reshape(-1)
    p["res"] = rng.integers(-8, 9, size=(c.N, Ho, Wo, c.Cout), dtype=np.int64) if c.res else None
    for v in p.values():
        if v is not None:
            v.setflags(write=False)
    return p


def codes_of(a):
    """integers of {-1, 0, 1} -> their e4m3 bytes."""
    out = np.zeros(a.shape, np.uint8)
    for v, code in E4M3.items():
        out[a == v] = code
    return out


def mx_buffer(x, xs):
    """the block-scaled tensor as the device holds it: the codes, then the scale bytes."""
    return np.concatenate([codes_of(x).reshape(-1), np.ascontiguousarray(xs, np.uint8).reshape(-1)])


def dequant(x, xs):
    return x.astype(np.float64) * np.repeat(np.exp2(xs.astype(np.float64) - 127.0), 32, axis=-1)


# ---- the reference -------------------------------------------------------------------------------------------------------------------------------------
def _image_of_row(c):
    Ho, Wo = dims(c)[:2]
    return np.broadcast_to(np.arange(c.N)[:, None, None], (c.N, Ho, Wo))


def _stages(c, p, g, img=None, wscale=None):
    """g (N, Ho, Wo, Cout) of the GEMM part -> the values the epilogue passes through: [g, g wscale, + bias, + bias_nc, + residual]."""
    out = [g]
    y = g * (p["wscale"] if wscale is None else wscale)
    out.append(y)
    if p["bias"] is not None:
        y = y + p["bias"]
        out.append(y)
    if p["bias_nc"] is not None:
        img = _image_of_row(c) if img is None else img
        y = y + p["bias_nc"][img[..., None] * nc_stride(c) + np.arange(c.Cout)]
        out.append(y)
    if p["res"] is not None:
        y = y + p["res"]
        out.append(y)
    return out


@functools.lru_cache(maxsize=None)
def reference(c):
    p = inputs(c)
    Ho, Wo, M, C, K = dims(c)
    xd = dequant(p["x"], p["xs"])
    if c.C2:
        xd = np.concatenate([xd, dequant(p["x2"], p["x2s"])], axis=-1)
    xp = np.zeros((c.N, c.H + 2 * c.pad, c.W + 2 * c.pad, C))
    xp[:, c.pad:c.pad + c.H, c.pad:c.pad + c.W] = xd
    wk = p["w"].reshape(c.Cout, c.R, c.R, C).astype(np.float64)
    g = np.zeros((c.N, Ho, Wo, c.Cout))
    for r in range(c.R):
        for s in range(c.R):
            g += xp[:, r:r + Ho, s:s + Wo] @ wk[:, r, s].T
    y = _stages(c, p, g)[-1]
    y.setflags(write=False)
    return y


# ---- the dispatcher's rules (csrc/gemm_family.h, gemm_k_pp8.hip, gemm_k_pp3.hip) ----------------------------------------------------------------------------
def h2(c):
    """half-tile slabs: a channel count off the 128 grid"""
    return bool(c.C1 % 128 or c.C2 % 128)


def eff_splitk(K, split):
    kt = -(-K // 128)
    kps = -(-kt // max(split, 1))
    return -(-kt // kps)


def split_ranges(K, split):
    kt = -(-K // 128)
    kps = -(-kt // max(split, 1))
    return [(z * kps * 128, min(K, (z + 1) * kps * 128)) for z in range(-(-kt // kps))]


def pp_ok(c):
    Ho, Wo = dims(c)[:2]
    if (c.bm, c.bn) not in TILES or c.C1 % 64 or c.C2 % 64 or c.R * c.R > 31:
        return False
    if (c.bm, c.bn) == (256, 160) and h2(c):
        return False
    return not (c.nc != "none" and Ho * Wo < c.bm)


def pp3_ok(c):
    Ho, Wo = dims(c)[:2]
    if (c.bm, c.bn) != (192, 128) or c.kind != "conv" or (c.R, c.pad) != (3, 1) or c.split != 1:
        return False
    if c.C1 % 64 or c.C2 % 128 or (c.C1 % 128 and (c.C2 or Wo == 24)):
        return False
    return Wo in (96, 48, 24) and (Ho * Wo) % 192 == 0


def pp3_h2(c):
    """the instance tfk_launch_pp3 picks: 96-pixel rows have the half-slab form only, 48-pixel rows both, 24-pixel rows the whole-slab form only"""
    return c.W == 96 or bool(c.C1 % 128)


def predict_form(c):
    K = dims(c)[4]
    if c.family == "pp":
        assert c.dbg == BIT["pp"] and pp_ok(c), c
        return Form((c.bm, c.bn, c.split, V_PP), eff_splitk(K, c.split), f"k_igemm_pp<F8,{c.bm},{c.bn},{'H2' if h2(c) else 'whole'}>")
    assert c.family == "pp3" and c.dbg == BIT["pp3"] and pp3_ok(c), c
    return Form((192, 128, 1, V_PP3), 1, f"k_igemm_pp3<F8,128,{c.W},{'H2' if pp3_h2(c) else 'whole'}>")


def required_instances():
    need = {f"k_igemm_pp<F8,{bm},{bn},{f}>" for bm, bn in TILES for f in ("whole", "H2") if not ((bm, bn) == (256, 160) and f == "H2")}
    return need | {"k_igemm_pp3<F8,128,96,H2>", "k_igemm_pp3<F8,128,48,H2>", "k_igemm_pp3<F8,128,48,whole>", "k_igemm_pp3<F8,128,24,whole>"}


def straddles(c):
    """a tile of the row spans two images"""
    Ho, Wo, M = dims(c)[:3]
    m0 = np.arange(0, M, c.bm)
    return bool(np.any(m0 // (Ho * Wo) != (np.minimum(m0 + c.bm, M) - 1) // (Ho * Wo)))


# ---- the addressing engine and its slips -------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "scale_block_next": "the scale byte of block b + 1",
    "scale_block_prev": "the scale byte of block b - 1",
    "scale_tap_prev": "the scale of the previous tap",
    "scale_tap_next": "the scale of the next tap",
    "scales_off": "scales not applied at all (2^0)",
    "x2_scale_pitch_C1": "the scale row pitch of C1 used for the second source",
    "x2_scales_behind_x_codes": "second-source scales read behind x's code count (nb1 for nb2)",
    "k_halves_swapped": "the scales of the two 64-channel halves of a K tile swapped",
    "last_half_tile_valid": "the last half tile of K read as valid (K = n + 1/2 tiles): tap 0 again against the next weight row's head",
    "pad_wraps": "a padded tap (wi = -1) taken from the wrapped-around pixel, code and scale, instead of zero",
    "bias_nc_first_image_of_tile": "bias_nc of image n - 1 for the second image's rows in a tile spanning two",
    "bias_nc_next_image": "bias_nc of image n + 1 for the first image's rows in a tile spanning two",
    "wscale_col_plus1": "the wscale column off by one",
    "wscale_tile_first": "wscale of the tile's first column for all of them",
    "pp3_scale_row_above": "a patch row's scale dword from the row above",
    "pp3_scale_row_below": "a patch row's scale dword from the row below",
    "pp3_half2_from_neighbour": "the half-slab form's second 2-byte scale load taken from the neighbouring patch row",
}
_EPILOGUE_SLIPS = ("bias_nc_first_image_of_tile", "bias_nc_next_image", "wscale_col_plus1", "wscale_tile_first")


def applies(c, slip):
    Ho, Wo, M, C, K = dims(c)
    two = c.nc != "none" and straddles(c)
    return {
        "scale_block_next": True, "scale_block_prev": True, "scale_tap_prev": c.R > 1, "scale_tap_next": c.R > 1, "scales_off": True,
        "x2_scale_pitch_C1": c.C2 > 0 and c.C1 != c.C2, "x2_scales_behind_x_codes": c.C2 > 0 and c.C1 != c.C2, "k_halves_swapped": True,
        "last_half_tile_valid": c.family == "pp" and K % 128 == 64, "pad_wraps": c.pad > 0, "bias_nc_first_image_of_tile": two, "bias_nc_next_image": two,
        "wscale_col_plus1": c.wscale == "pow2", "wscale_tile_first": c.wscale == "pow2", "pp3_scale_row_above": c.family == "pp3",
        "pp3_scale_row_below": c.family == "pp3", "pp3_half2_from_neighbour": c.family == "pp3" and pp3_h2(c),
    }[slip]


def _rows(c):
    Ho, Wo, M = dims(c)[:3]
    m = np.arange(M)
    img = m // (Ho * Wo)
    rem = m - img * (Ho * Wo)
    return img, rem // Wo, rem % Wo


def _source(c, ch, pitch_slip=False):
    """(second source?, channel inside it, its channel count) of concat channel ch"""
    second = ch >= c.C1
    return second, np.where(second, ch - c.C1, ch), np.where(second, c.C1 if pitch_slip else c.C2, c.C1)


@functools.lru_cache(maxsize=8)
def _codes(c, wrap):
    """(M, K) code values: x_flat[pixel(m, tap) C_src + channel] inside the image, 0 outside and beyond the codes of the source."""
    p = inputs(c)
    Ho, Wo, M, C, K = dims(c)
    img, ho, wo = _rows(c)
    k = np.arange(K)
    tap, ch = k // C, k % C
    second, cc, ld = _source(c, ch)
    hi = ho[:, None] - c.pad + (tap // c.R)[None, :]
    wi = wo[:, None] - c.pad + (tap % c.R)[None, :]
    ok = (hi >= 0) & (hi < c.H) & (wi >= (-1 if wrap else 0)) & (wi < c.W)
    off = ((img[:, None] * c.H + hi) * c.W + wi) * ld[None, :] + cc[None, :]
    flat = [p["x"].reshape(-1), p["x2"].reshape(-1) if c.C2 else np.zeros(1, np.int64)]
    out = np.zeros((M, K))
    for src in (0, 1):
        sel = ok & (second == bool(src))[None, :] & (off >= 0) & (off < flat[src].size)
        out += np.where(sel, flat[src][np.clip(off, 0, flat[src].size - 1)], 0)
    return out


def _scales(c, slip):
    """(M, K) factors 2^(byte - 127): the byte at nb_src + pixel(m, tap) C_src / 32 + channel / 32 of the source's buffer, byte 0 out of range.  (Worked
    out per 32-channel block of K -- every slip moves whole blocks -- and repeated over the block's channels.)"""
    p = inputs(c)
    Ho, Wo, M, C, K = dims(c)
    if slip == "scales_off":
        return np.ones((M, K))
    img, ho, wo = _rows(c)
    k = np.arange(0, K, 32)
    dead = np.zeros(K // 32, bool)
    if slip == "k_halves_swapped":
        if c.family == "pp":                                   # flat K tiles of 128
            k = k ^ 64
            dead = k >= K
            k = np.where(dead, 0, k)
    tap, ch = k // C, k % C
    if slip == "k_halves_swapped" and c.family == "pp3":      # 128-channel slabs of one tap
        ch = ch ^ 64
        dead = ch >= C
        ch = np.where(dead, 0, ch)
    if slip in ("scale_tap_prev", "scale_tap_next"):
        tap = np.clip(tap + (1 if slip == "scale_tap_next" else -1), 0, c.R * c.R - 1)
    second, cc, ld = _source(c, ch, slip == "x2_scale_pitch_C1")
    hi = ho[:, None] - c.pad + (tap // c.R)[None, :] + {"pp3_scale_row_above": -1, "pp3_scale_row_below": 1}.get(slip, 0)
    wi = wo[:, None] - c.pad + (tap % c.R)[None, :]
    if slip == "pp3_half2_from_neighbour":
        wi = wi + ((ch % 128) >= 64)[None, :]
    ok = (hi >= 0) & (hi < c.H) & (wi >= (-1 if slip == "pad_wraps" else 0)) & (wi < c.W) & ~dead[None, :]
    blk = cc // 32 + {"scale_block_next": 1, "scale_block_prev": -1}.get(slip, 0)
    pixels = c.N * c.H * c.W
    nb = (pixels * c.C1, pixels * (c.C1 if slip == "x2_scales_behind_x_codes" else c.C2))
    bufs = [mx_buffer(p["x"], p["xs"]), mx_buffer(p["x2"], p["x2s"]) if c.C2 else np.zeros(1, np.uint8)]
    byte = np.zeros((M, K // 32), np.uint8)
    pix = (img[:, None] * c.H + hi) * c.W + wi
    for src in (0, 1):
        off = nb[src] + pix * (ld // 32)[None, :] + blk[None, :]
        sel = ok & (second == bool(src))[None, :] & (off >= 0) & (off < bufs[src].size)
        byte |= np.where(sel, bufs[src][np.clip(off, 0, bufs[src].size - 1)], np.uint8(0))
    return np.repeat(np.exp2(byte.astype(np.float64) - 127.0), 32, axis=1)


@functools.lru_cache(maxsize=2)
def _operand0(c):
    a = _codes(c, False) * _scales(c, None)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=2)
def _gemm0(c):
    g = _operand0(c) @ inputs(c)["w"].astype(np.float64).T
    g.setflags(write=False)
    return g


def operand(c, slip=None):
    """A (M, K) float64 as the kernel assembles it: code times block scale, each from its own flat offset."""
    return _operand0(c) if slip is None else _codes(c, slip == "pad_wraps") * _scales(c, slip)


def gather(c, slip=None):
    """the row's output through the addressing engine; `slip`: one of MUTANTS."""
    assert slip is None or slip in MUTANTS, slip
    p = inputs(c)
    Ho, Wo, M, C, K = dims(c)
    w = p["w"].astype(np.float64)
    g = _gemm0(c) if slip is None or slip in _EPILOGUE_SLIPS or slip == "last_half_tile_valid" else operand(c, slip) @ w.T
    if slip == "last_half_tile_valid":
        wnext = np.concatenate([p["w"].reshape(-1), np.zeros(64, np.int64)])[(np.arange(c.Cout)[:, None] + 1) * K + np.arange(64)[None, :]]
        g = g + _operand0(c)[:, :64] @ wnext.astype(np.float64).T
    g = g.reshape(c.N, Ho, Wo, c.Cout)
    img, wscale = None, None
    if slip in ("bias_nc_first_image_of_tile", "bias_nc_next_image"):
        m = np.arange(M)
        first = (m // c.bm * c.bm) // (Ho * Wo)
        last = (np.minimum(m // c.bm * c.bm + c.bm, M) - 1) // (Ho * Wo)
        img = (first if slip == "bias_nc_first_image_of_tile" else last).reshape(c.N, Ho, Wo)
    if slip == "wscale_col_plus1":
        wscale = np.concatenate([p["wscale"][1:], [1.0]])
    if slip == "wscale_tile_first":
        wscale = p["wscale"][np.arange(c.Cout) // c.bn * c.bn]
    return _stages(c, p, g, img, wscale)[-1]


def mutants(c):
    """{name: wrong output} for every slip of MUTANTS that applies to the row."""
    return {name: gather(c, name) for name in MUTANTS if applies(c, name)}


def exact(c):
    """the condition under which array_equal is the right comparison (module docstring); asserts, returns True."""
    p = inputs(c)
    Ho, Wo, M, C, K = dims(c)
    q = q_of(c)
    live = [s[s != 0] for s in (p["xs"], p["x2s"]) if s is not None]
    assert min(int(s.min()) for s in live) == 127 - 1, (c.name, "the smallest block scale fixes q")
    assert float(p["wscale"].min()) == (0.25 if c.wscale == "pow2" else 1.0), c.name
    A, w = operand(c), p["w"].astype(np.float64)
    values = list(_stages(c, p, (A @ w.T).reshape(c.N, Ho, Wo, c.Cout)))
    assert np.array_equal(values[-1], reference(c)), c.name
    if eff_splitk(K, c.split) > 1:
        values += [(A[:, a:b] @ w[:, a:b].T) * p["wscale"] for a, b in split_ranges(K, c.split)]
    for v in values:
        assert np.array_equal(np.rint(v * 2.0 ** q), v * 2.0 ** q), (c.name, "not a multiple of 2^-q", q)
        assert np.abs(v).max() < 2.0 ** (11 - q), (c.name, "beyond 2^(11 - q)", q, float(np.abs(v).max()))
    y = reference(c)
    assert np.array_equal(y.astype(np.float16).astype(np.float64), y) and not np.any(y == SENTINEL), c.name
    return True


# ---- the case table ------------------------------------------------------------------------------------------------------------------------------------
def case(family, geo, shape, Cs, Cout, tile, split=1, nc="none", res=False, bias=True, slabs=16, rounds=False, wscale="pow2"):
    R, pad = GEO[geo]
    N, H, W = shape
    name = (f"{family}-{geo}-{N}x{H}x{W}-c{Cs[0]}+{Cs[1]}-o{Cout}-{tile[0]}x{tile[1]}s{split}-{nc}{'-res' if res else ''}{'' if bias else '-nobias'}"
            f"{'-f32slabs' if slabs == 32 else ''}{'-ones' if wscale == 'ones' else ''}")
    return Case(name, "conv", family, N, H, W, Cs[0], Cs[1], Cout, R, pad, tile[0], tile[1], split, BIT[family], nc, res, bias, slabs, rounds, wscale)


def linear(M, K, N, tile, split=1, res=True, slabs=16, rounds=False, wscale="pow2"):
    name = f"linear-{M}x{K}x{N}-{tile[0]}x{tile[1]}s{split}{'-res' if res else ''}{'-f32slabs' if slabs == 32 else ''}{'-ones' if wscale == 'ones' else ''}"
    return Case(name, "linear", "pp", 1, 1, M, K, 0, N, 1, 0, tile[0], tile[1], split, BIT["pp"], "none", res, True, slabs, rounds, wscale)


COUNTS = ((64, 0), (128, 0), (192, 0), (320, 0), (64, 64), (128, 64), (64, 128), (128, 128), (192, 64))
COUTS = (128, 136, 160, 200)
GEOS = tuple(GEO)


def _pp_cover():
    """every tile with every channel count it takes, walking the geometries, output widths, bias_nc modes, image counts and the residual; 5 x 5 filters keep
    to at most 192 channels (K = 4800) and the rows without the wscale pattern are every seventh."""
    rows, i = [], 0
    for tile in TILES:
        for Cs in COUNTS:
            if tile == (256, 160) and (Cs[0] % 128 or Cs[1] % 128):
                continue
            geo = GEOS[i % 5]
            if geo == "5x5p2" and sum(Cs) > 192:
                geo = "3x3p1"
            N = 2 + i % 2
            R, pad = GEO[geo]
            howo = (16 + 2 * pad - R + 1) ** 2
            nc = ("cout", "padded", "none")[i % 3] if howo >= tile[0] else "none"
            rows.append(case("pp", geo, (N, 16, 16), Cs, COUTS[i % 4], tile, nc=nc, res=i % 2 == 0, bias=i % 5 != 3, wscale="ones" if i % 7 == 6 else "pow2"))
            i += 1
    return rows


def _pp3_cover():
    rows, i = [], 0
    shapes = {24: ((8, 24), (16, 24)), 48: ((4, 48), (8, 48)), 96: ((2, 96), (4, 96))}        # (H, W): W x H of 24 x 8 ... 96 x 4

    def add(W, Cs):
        nonlocal i
        H, _ = shapes[W][i % 2]
        rows.append(case("pp3", "3x3p1", (2, H, W), Cs, COUTS[i % 4], (192, 128), nc=("cout", "padded", "none")[i % 3], res=i % 2 == 1, bias=i % 5 != 2,
                         wscale="ones" if i % 7 == 5 else "pow2"))
        i += 1
    for W in (24, 48, 96):
        for C1 in (128, 256, 384):
            add(W, (C1, 0))
        if W != 24:
            for C1 in (192, 320):
                add(W, (C1, 0))
        for Cs in ((128, 128), (256, 128)):
            add(W, Cs)
    # both image heights at every row length on the smallest count: a tile that is the whole image and a tile that is half of it
    for W in (24, 48, 96):
        for H, _ in shapes[W]:
            row = case("pp3", "3x3p1", (2, H, W), (128, 0), 136, (192, 128), nc="cout", res=True)
            if row.name not in {r.name for r in rows}:
                rows.append(row)
    return rows


CASES = _pp_cover() + [
    # every geometry on every tile with half-tile slabs off (128 | 128 is the count the 256 x 160 tile takes) ...
    case("pp", "3x3p0", (2, 16, 16), (128, 128), 200, (256, 160)),
    case("pp", "1x1p0", (3, 16, 16), (128, 128), 136, (256, 160), nc="padded", res=True),
    case("pp", "1x1p1", (2, 16, 16), (128, 0), 160, (256, 160), nc="cout"),
    case("pp", "5x5p2", (2, 16, 16), (128, 0), 128, (256, 160), nc="cout", res=True),
    case("pp", "5x5p2", (3, 16, 16), (64, 64), 136, (192, 160), nc="padded"),
    case("pp", "1x1p1", (3, 16, 16), (192, 64), 200, (256, 128), nc="cout", res=True),
    case("pp", "3x3p0", (3, 16, 16), (64, 128), 136, (192, 128), nc="padded", res=True),       # HoWo = 196 >= 192: bias_nc admitted, every tile spans two images
    # ... K = 4.5 tiles (64 channels, 3 x 3), the second half of the last tile beyond K, on both tile heights
    case("pp", "3x3p1", (3, 16, 16), (64, 0), 200, (192, 160), nc="cout", res=True),
    case("pp", "3x3p1", (2, 16, 16), (64, 0), 136, (256, 128), nc="padded"),
    # HoWo < bm: no bias_nc, a tile holds several images (8 x 8 images under a 192-row tile: three each)
    case("pp", "3x3p1", (5, 8, 8), (64, 64), 136, (192, 128), res=True),
    case("pp", "3x3p0", (2, 16, 16), (320, 0), 160, (256, 128), res=True, wscale="ones"),       # HoWo = 196 < 256
    # split-K: 2 with whole and ragged K tiles, fp16 and fp32 slabs, bias / bias_nc / residual through the reducer, and splits beyond the whole K tiles
    case("pp", "3x3p1", (2, 16, 16), (128, 0), 136, (256, 128), split=2, nc="cout", res=True),                       # 9 tiles: 5 + 4
    case("pp", "3x3p1", (3, 16, 16), (64, 64), 200, (192, 160), split=2, slabs=32, nc="padded", res=True),
    case("pp", "3x3p1", (2, 16, 16), (192, 64), 160, (192, 128), split=2, nc="cout"),
    case("pp", "1x1p0", (3, 16, 16), (320, 0), 128, (256, 128), split=2, res=True, slabs=32),                        # 2.5 tiles: 2 + 0.5
    case("pp", "3x3p1", (2, 16, 16), (128, 128), 160, (256, 160), split=2, nc="padded", res=True),
    case("pp", "5x5p2", (2, 16, 16), (64, 0), 136, (192, 128), split=2, nc="cout", res=True, wscale="ones"),       # 12.5 tiles: 7 + 5.5
    case("pp", "3x3p1", (3, 16, 16), (64, 0), 136, (192, 128), split=4, rounds=True, nc="cout", res=True),           # 5 K tiles in 4: two per split, so three splits
    case("pp", "1x1p0", (2, 16, 16), (192, 0), 200, (256, 128), split=3, rounds=True, slabs=32, res=True),           # 2 K tiles in 3: two splits
    case("pp", "1x1p0", (2, 16, 16), (64, 0), 128, (192, 160), split=2, rounds=True, nc="cout"),                     # half a K tile: no split at all
] + _pp3_cover()


def _linears():
    rows, i = [], 0
    Ms, Ks, Ns = (64, 300, 515), (64, 192, 640), (128, 136, 328)
    for tile in TILES:
        for split in (1, 2):
            for K in Ks:
                if tile == (256, 160) and K % 128:
                    continue
                rows.append(linear(Ms[i % 3], K, Ns[(i // 3 + i) % 3], tile, split, res=i % 4 != 3, slabs=32 if i % 5 == 4 else 16,
                                   rounds=eff_splitk(K, split) != split, wscale="ones" if i % 7 == 3 else "pow2"))
                i += 1
    return rows


LINEARS = _linears()
ALL = CASES + LINEARS

# the block-scaled GEGLU output (tf_linear_mx8 with act = 1): (M, K, out_features, tile)
Geglu = collections.namedtuple("Geglu", "name M K No bm bn")
GEGLU = [Geglu(f"geglu-{M}x{K}x{No}-{bm}x128", M, K, No, bm, 128) for M in (300, 515) for K in (128, 320) for No in (128, 160, 224) for bm in (192, 256)]


@functools.lru_cache(maxsize=None)
def geglu_inputs(g):
    """x codes / scale bytes (M, K), w (2 No, K) of {-1, 0, 1} in the order [values ; gates], wscale (2 No) of {1/2, 1} per output pair, bias (2 No): the
    gate half of [-6, 6] so that both signs and |gate| up to about 6 occur whatever the GEMM part adds."""
    rng = np.random.default_rng(zlib.crc32(g.name.encode()))
    d = (4.0 / g.K) ** 0.5                                  # the GEMM part of a gate: sigma about 2.6
    x, xs = _blocks(rng, (g.M,), g.K, d)
    w = rng.choice(np.array([-1, 0, 1], np.int64), size=(2 * g.No, g.K), p=[d / 2, 1 - d, d / 2])
    wscale = np.tile(2.0 ** -(np.arange(g.No) % 2), 2)
    bias = np.concatenate([rng.integers(-3, 4, size=g.No), rng.integers(-6, 7, size=g.No)]).astype(np.float64)
    return {"x": x, "xs": xs, "w": w, "wscale": wscale, "bias": bias}


def pack_geglu_rows(a, No):
    """[values ; gates] (2 No, ...) -> 16-row blocks v0 g0 v1 g1 ... as ff/nn.py's pack_geglu lays them out."""
    v, g = a[:No].reshape(No // 16, 16, *a.shape[1:]), a[No:].reshape(No // 16, 16, *a.shape[1:])
    return np.stack([v, g], axis=1).reshape(a.shape)


def geglu_reference(g):
    """float64: (x w_v^T wscale + b_v) gelu(x w_g^T wscale + b_g) with the tanh form of the GELU the library and the oracle use; also the gate."""
    p = geglu_inputs(g)
    y = dequant(p["x"], p["xs"]) @ p["w"].astype(np.float64).T * p["wscale"] + p["bias"]
    a, gate = y[:, :g.No], y[:, g.No:]
    return a * 0.5 * gate * (1.0 + np.tanh(0.7978845608 * gate * (1.0 + 0.044715 * gate * gate))), gate


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
# (what, the case the launch is built from, overrides of the arguments, status, a piece of tf_last_error that names the entry / the family)
Refusal = collections.namedtuple("Refusal", "what case override rc says")
_R0 = case("pp", "3x3p1", (2, 16, 16), (128, 0), 136, (192, 128), nc="cout")
_L0 = linear(300, 128, 128, (192, 128))
REFUSALS = [
    Refusal("stride 2", _R0, {"stride": 2}, E_ARG, b"tf_conv2d_mx8: stride-1 square filters only"),
    Refusal("R != S", _R0, {"S": 1}, E_ARG, b"tf_conv2d_mx8: stride-1 square filters only"),
    Refusal("256 x 160 off the 128 grid", case("pp", "3x3p1", (2, 16, 16), (192, 0), 160, (256, 160)), {}, E_UNSUPPORTED, b"ping-pong"),
    Refusal("256 x 160 with a second source off the 128 grid", case("pp", "1x1p0", (2, 16, 16), (128, 64), 160, (256, 160)), {}, E_UNSUPPORTED, b"ping-pong"),
    Refusal("bias_nc with HoWo < bm", case("pp", "3x3p0", (2, 16, 16), (128, 0), 136, (256, 128), nc="cout"), {}, E_UNSUPPORTED, b"ping-pong"),
    Refusal("pp3 on 24-pixel rows with a half slab", case("pp3", "3x3p1", (2, 8, 24), (192, 0), 136, (192, 128)), {}, E_UNSUPPORTED, b"ping-pong patch"),
    Refusal("pp3 with a half slab and a second source", case("pp3", "3x3p1", (2, 4, 48), (192, 128), 136, (192, 128)), {}, E_UNSUPPORTED, b"ping-pong patch"),
    Refusal("pp3 with a second source off the 128 grid", case("pp3", "3x3p1", (2, 4, 48), (128, 64), 136, (192, 128)), {}, E_UNSUPPORTED, b"ping-pong patch"),
    Refusal("pp3 on 32-pixel rows", case("pp3", "3x3p1", (2, 6, 32), (128, 0), 136, (192, 128)), {}, E_UNSUPPORTED, b"ping-pong patch"),
    Refusal("pp3 on a 1 x 1 filter", case("pp3", "1x1p0", (2, 4, 48), (128, 0), 136, (192, 128)), {}, E_UNSUPPORTED, b"ping-pong patch"),
    Refusal("out_mx with a residual", _L0, {"act": 1, "out_mx": 1}, E_ARG, b"tf_linear_mx8: a block-scaled output"),
    Refusal("out_mx with N % 32 != 0", _L0._replace(res=False), {"act": 1, "out_mx": 1, "Nout": 80}, E_ARG, b"tf_linear_mx8: a block-scaled output"),
]
