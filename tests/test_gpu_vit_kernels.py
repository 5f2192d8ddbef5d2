"""The three kernels of csrc/vit.hip on the device, float16 and bfloat16.

  * tf_vit_patchify_u8_16, bit for bit: every byte value at every (ky, kx, c) column, and a seeded random batch; the reference is
    round16(float32(float64(u8) * scale + shift)) -- the float64 product (8 x 24 bits) and sum are exact, so this is the kernel's single fp32
    rounding followed by the store rounding.  Pad columns are zero, the words behind the output keep their sentinel.
  * tf_gelu_erf_16 on every finite 16-bit pattern against 0.5 x erfc(-x / sqrt 2) in float64, rounded to nearest: no output further than 1 ulp of
    the output type (ordinal distance of the bit patterns); the share of inputs that differ at all is printed, not gated.
  * tf_vit_embed_ln_16 against the float64 LayerNorm of the float64 sums under the LayerNorm budget of tests/aux/norm_planted.py (tol = half_ulp +
    A, K = 12: the kernel is k_layer_norm<64>'s two-pass form; its fp32 sum of two 16-bit values adds at most 2^-24 |e| / sigma <= 2^-24 (R + |y|) per
    element, under 1 / 48 of A).  The rows are planted (every row its own mean and spread, |mean| / sigma <= R asserted on the sums), and the two
    index mistakes the kernel can make -- patch p paired with position row p, the class row taken from the patches -- are shown to miss the budget."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import norm_planted as P  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = ("fp16", "bf16")
SENT = 0x5A5A                      # a finite pattern in both types no expected value takes behind the outputs


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def tag(dtype):
    return 1 if dtype == "bf16" else 0


def bits_of(x, dtype):
    """float array (values of the storage type) -> uint16 patterns."""
    x = np.ascontiguousarray(x, np.float32)
    return x.astype(np.float16).view(np.uint16) if dtype == "fp16" else (x.view(np.uint32) >> 16).astype(np.uint16)


def value_of(bits, dtype):
    bits = np.ascontiguousarray(bits, np.uint16)
    with np.errstate(invalid="ignore"):                     # (signalling-NaN patterns among the 65 536)
        return bits.view(np.float16).astype(np.float64) if dtype == "fp16" else (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def upload_bits(tf, bits):
    a = tf.DeviceArray.empty(bits.shape, np.uint16, "row")
    return a.copy_from_numpy(np.ascontiguousarray(bits, np.uint16))


def download_bits(tf, a):
    from tinyfusers_amd.native import hip
    hip.tf_stream_sync(tf._sh())
    host = np.empty(a.shape, np.uint16)
    hip.tf_memcpy(host.ctypes.data, a.ptr, host.nbytes, 2)
    return host


def guarded(tf, n, guard=64):
    """n output words + `guard` words of sentinel behind them."""
    return upload_bits(tf, np.full((n + guard,), SENT, np.uint16))


# ---- patchify -----------------------------------------------------------------------------------------------------------------------------------
def every_byte_images():
    """(64, 28, 28, 3): patch q = 4 b + 2 py + px of 256; the byte at (ky, kx, c) of patch q is (q + 37 ky + 11 kx + 101 c) mod 256 -- over the 256
    patches every column sees every byte value once."""
    b, y, x, c = np.meshgrid(np.arange(64), np.arange(28), np.arange(28), np.arange(3), indexing="ij")
    q = 4 * b + 2 * (y // 14) + x // 14
    return ((q + 37 * (y % 14) + 11 * (x % 14) + 101 * c) % 256).astype(np.uint8)


def patch_matrix64(img, P_, kpad, scale, shift):
    """The float32 values the kernel computes, via float64: rows (b, py, px), columns (ky, kx, c), zero pad."""
    B, S = img.shape[0], img.shape[1]
    g = S // P_
    v = (img.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)
    v = v.reshape(B, g, P_, g, P_, 3).transpose(0, 1, 3, 2, 4, 5).reshape(B * g * g, 3 * P_ * P_)
    out = np.zeros((B * g * g, kpad), np.float32)
    out[:, :3 * P_ * P_] = v
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ("every_byte", "random"))
def test_patchify_is_bit_exact(tf, dtype, case):
    from tinyfusers_amd.native import hip
    from tinyfusers_amd.vae.clip_vision import norm_constants
    if case == "every_byte":
        img, kpad = every_byte_images(), 592
        cols = img.reshape(64, 2, 14, 2, 14, 3).transpose(0, 1, 3, 2, 4, 5).reshape(256, 588)
        assert all(len(set(cols[:, j])) == 256 for j in range(588))                  # every byte value in every column
    else:
        img, kpad = np.random.default_rng(11).integers(0, 256, (2, 56, 56, 3), dtype=np.uint8), 600     # (a wider pad: 12 zero columns)
    B, S = img.shape[0], img.shape[1]
    rows = B * (S // 14) ** 2
    scale, shift = norm_constants()
    want = bits_of(P.round16(patch_matrix64(img, 14, kpad, scale, shift), dtype), dtype)
    dimg = tf.DeviceArray.from_numpy(img, np.uint8, "row")
    out = guarded(tf, rows * kpad)
    hip.tf_vit_patchify_u8_16(tag(dtype), out.ptr, dimg.ptr, B, S, 14, kpad, scale.ctypes.data, shift.ctypes.data, tf._sh())
    got = download_bits(tf, out)
    assert (got[rows * kpad:] == SENT).all(), "wrote behind the output"
    got = got[:rows * kpad].reshape(rows, kpad)
    assert not got[:, 588:].any(), "pad columns must be +0"
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])


# ---- exact GELU ---------------------------------------------------------------------------------------------------------------------------------
def ordinal(bits):
    b = np.asarray(bits, np.uint16).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def nearest16(ref, dtype):
    """float64 -> the nearest value of the 16-bit type as bits (ties to even), without a double rounding through float32."""
    if dtype == "fp16":
        return np.asarray(ref, np.float64).astype(np.float16).view(np.uint16)        # (numpy rounds double -> half in one step)
    c = (np.asarray(ref, np.float64).astype(np.float32).view(np.uint32) >> 16).astype(np.int64)      # truncated candidate, then its neighbour above
    lo, hi = value_of(c.astype(np.uint16), dtype), value_of(np.minimum((c & 0x7FFF) + 1, 0x7F7F).astype(np.uint16) | (c & 0x8000).astype(np.uint16), dtype)
    dlo, dhi = np.abs(ref - lo), np.abs(ref - hi)
    up = (dhi < dlo) | ((dhi == dlo) & ((c & 1) == 1))
    return np.where(up, ((c & 0x7FFF) + 1) | (c & 0x8000), c).astype(np.uint16)


def gelu64(x):
    """0.5 x erfc(-x / sqrt 2) on double (torch.special.erfc): the form without the cancellation of 1 + erf in the negative tail."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, np.float64))
    return (0.5 * t * torch.special.erfc(-t / math.sqrt(2.0))).numpy()


@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_erf_on_every_finite_pattern(tf, dtype):
    from tinyfusers_amd.native import hip
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    x = value_of(bits, dtype)
    finite = np.isfinite(x)
    assert finite.sum() == (63488 if dtype == "fp16" else 65280)
    dx, dy = upload_bits(tf, bits), guarded(tf, 65536)
    hip.tf_gelu_erf_16(tag(dtype), dy.ptr, dx.ptr, 65536, tf._sh())
    got = download_bits(tf, dy)
    assert (got[65536:] == SENT).all()
    got = got[:65536]
    with np.errstate(over="ignore", invalid="ignore"):
        ref = gelu64(np.where(finite, x, 0.0))
    want = nearest16(ref, dtype)
    dist = np.abs(ordinal(got) - ordinal(want))[finite]
    share = float((dist != 0).mean())
    worst = int(dist.max())
    at = x[finite][int(dist.argmax())]
    print(f"\ntf_gelu_erf_16 {dtype}: {share:.5f} of the finite inputs differ from the correctly rounded value, worst {worst} ulp (at x = {at!r})")
    assert np.isfinite(value_of(got, dtype)[finite]).all()
    assert worst <= 1, (worst, at)
    # the subnormal negative tail the erfc form is for: x = -5 is a float16 subnormal result
    if dtype == "fp16":
        i = int(np.float16(-5.0).view(np.uint16))
        assert abs(ref[i]) < 2.0 ** -14 and abs(int(ordinal(got[i])) - int(ordinal(want[i]))) <= 1
    # in place == out of place
    hip.tf_gelu_erf_16(tag(dtype), dx.ptr, dx.ptr, 65536, tf._sh())
    assert np.array_equal(download_bits(tf, dx), got)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_erf_odd_length_keeps_its_guard(tf, dtype):
    from tinyfusers_amd.native import hip
    n = 8 * 261 + 3                                         # more than one block of vectors, then a 3-element tail
    x = P.round16(np.random.default_rng(5).standard_normal(n) * 3.0, dtype)
    dx, dy = upload_bits(tf, bits_of(x, dtype)), guarded(tf, n, guard=13)
    hip.tf_gelu_erf_16(tag(dtype), dy.ptr, dx.ptr, n, tf._sh())
    got = download_bits(tf, dy)
    assert (got[n:] == SENT).all(), "wrote behind an odd n"
    dist = np.abs(ordinal(got[:n]) - ordinal(nearest16(gelu64(x.astype(np.float64)), dtype)))
    assert dist.max() <= 1 and (got[:n] != SENT).all()


# ---- token assembly + pre-LayerNorm ---------------------------------------------------------------------------------------------------------------
R_PATCH, R_SUM = 8, 16


def embed_inputs(B, T, D, dtype):
    """patch rows planted at R = 8 (tests/aux/norm_planted.py), a planted class row, position rows with their own offsets and a spread of 1 / 4."""
    patch = P.ln_input(B * (T - 1), D, dtype, R_PATCH)[0].reshape(B, T - 1, D)
    rng = np.random.default_rng([31, B, T, D])
    mu_c, sg_c = P.slice_params(np.array([1009]), R_PATCH)
    cls = P.round16(mu_c[0] + sg_c[0] * rng.standard_normal(D), dtype)
    off = ((7 * np.arange(T) + 3) % 17 - 8) / 8.0                       # [-1, 1], adjacent rows differ
    pos = P.round16(off[:, None] + 0.25 * rng.standard_normal((T, D)), dtype)
    return patch, cls, pos


def assemble64(patch, cls, pos, shift=1, class_from_patches=False):
    """float64 (B T, D) sums; shift = 0 and class_from_patches are the mutants."""
    B, Tm, D = patch.shape
    e = np.empty((B, Tm + 1, D), np.float64)
    e[:, 0] = (patch[:, 0] if class_from_patches else cls).astype(np.float64) + pos[0]
    e[:, 1:] = patch.astype(np.float64) + pos[shift:shift + Tm][None]
    return e.reshape(B * (Tm + 1), D)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,D", ((1, 17, 320), (2, 257, 1280)))
def test_embed_ln_meets_the_layer_norm_budget(tf, B, T, D, dtype):
    from tinyfusers_amd.native import hip
    patch, cls, pos = embed_inputs(B, T, D, dtype)
    gm, bt = P.affine(D)
    e = assemble64(patch, cls, pos)
    mean, var = P.ln_stats64(e)
    assert (np.abs(mean) / np.sqrt(var)).max() <= R_SUM                  # the budget's R bounds |mean| / sigma of what is normalised
    ref = P.ln_apply64(e, mean, var, gm, bt)
    tol, A = P.budget(ref, dtype, R_SUM, 2.0)
    dev = [upload_bits(tf, bits_of(a, dtype)) for a in (patch, cls, pos, gm, bt)]          # (referenced until the launch has run)
    out = guarded(tf, B * T * D)
    hip.tf_vit_embed_ln_16(tag(dtype), out.ptr, *(a.ptr for a in dev), B, T, D, P.EPS, tf._sh())
    raw = download_bits(tf, out)
    assert (raw[B * T * D:] == SENT).all(), "wrote behind the output"
    got = value_of(raw[:B * T * D], dtype).reshape(B * T, D)
    assert np.isfinite(got).all() and (raw[:B * T * D] != SENT).all()
    err = np.abs(got - ref)
    worst = float((err / tol).max())
    print(f"\ntf_vit_embed_ln_16 {(B, T, D)} {dtype}: max |err| / tol = {worst:.3f}, beyond the store rounding {max(float(((err - (tol - A)) / A).max()), 0.0):.3f} of A")
    assert worst <= 1.0
    # the planted rows tell the index mistakes apart: each mutant misses the budget on the rows it touches
    for name, kw, rows in (("patch p with position row p", dict(shift=0), np.arange(B * T) % T != 0),
                           ("class row taken from the patches", dict(class_from_patches=True), np.arange(B * T) % T == 0)):
        m = assemble64(patch, cls, pos, **kw)
        mut = P.ln_ref64(m, gm, bt)
        assert ((np.abs(mut - ref) / tol)[rows].max(axis=1) > 2).all(), name


# ---- argument refusals ----------------------------------------------------------------------------------------------------------------------------
def test_argument_refusals_come_before_any_device_work(tf):
    """The refusals of tests/test_clip_vision_host.py next to a live device: placeholder pointers, TF_E_ARG naming the entry, nothing launched --
    a launch on them would fault, and the device still answers afterwards."""
    import test_clip_vision_host as H
    from tinyfusers_amd.native import hip
    H.test_kernel_entries_refuse_bad_arguments_on_the_host(None)
    hip.tf_stream_sync(tf._sh())
    x = upload_bits(tf, np.arange(16, dtype=np.uint16))
    assert np.array_equal(download_bits(tf, x), np.arange(16, dtype=np.uint16))
