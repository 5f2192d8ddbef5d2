"""tf_sdpa_pag_16 (k_sdpa_pag<HS, 1>, <HS, 2>, <40 | 80, 2, 8>, float16 and bfloat16): self-attention in which a device flag turns one batch range into
the identity, o = v.  Bit-exact throughout -- every comparison is on the 16-bit patterns.

Shapes: the dma16, dma32 and dma32_w8 rows of tests/aux/sdpa_planted.py::INSTANCE_ROWS with their head sizes, Tq = Tk at the row's own count (200 /
300: three full key tiles and a ragged one) and at 64 (one full tile; the family is then whatever the rule names for that grid, asked of
tf_sdpa_pag_instance), B = 3 where the table has 1 so that a middle range exists.  Inputs are seeded normals in the packed q | k | v layout of
self-attention (sdpa_planted.packed_self); outputs in both head merges, and in a third form whose row pitch is 4 elements longer, which takes the
kernel's 2-byte copy loop (the output strides are only promised in multiples of 4 elements; the other two take the 16-byte one).

  (a) flag 0: every batch entry equals tf_sdpa_16's output of the same shape (forced unsplit where force_split_for says its rule would split);
  (b) flag 1, the range first / middle / last / empty / whole batch: entries inside hold v's bits, entries outside the flag-0 bits;
  (c) the same with q and k of the perturbed entries filled with NaN and Inf: neither may influence anything;
  (d) every output sits between guard words, which come back untouched (as do the pad columns of the third form), and the packed input buffer
      comes back bit for bit;
  (e) the flag is read when the kernel runs: one captured launch, the word flipped between replays;
  (f) refusals return an error and write nothing (status and message: tests/test_pag_host.py)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import sdpa_planted as P  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = ("fp16", "bf16")
GUARD, FILL = 64, 0x3A55                # guard words on both sides of o, and the bit pattern every output word starts from (finite in both types)
ROWS = [(inst, 3 if b == 1 else b, nh, tq, hs) for inst, b, nh, tq, hs in P.rows(("dma16", "dma32", "dma32_w8"))]
CASES = [(inst, b, nh, t, hs) for inst, b, nh, tq, hs in ROWS for t in (tq, 64)]


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def _np_dtype(tf, dtype):
    return tf.bfloat16 if dtype == "bf16" else np.float16


def bits16(x, dtype):
    """float32 values of the storage type -> their 16-bit patterns."""
    x = np.ascontiguousarray(x, np.float32)
    return x.astype(np.float16).view(np.uint16) if dtype == "fp16" else (x.view(np.uint32) >> 16).astype(np.uint16)


def ranges(b):
    return {"first": (0, 1), "middle": (1, b - 1), "last": (b - 1, b), "empty": (1, 1), "whole": (0, b)}


@functools.lru_cache(maxsize=2)
def inputs(b, nh, t, hs, dtype):
    """The packed (B, T, 3 NH HS) bit patterns and v's (B, NH, T, HS) bit patterns, seeded normals rounded to the storage type."""
    rng = np.random.default_rng([31, b, nh, t, hs])
    q, k, v = (P.round16(rng.standard_normal((b, nh, t, hs), dtype=np.float32), dtype) for _ in range(3))
    packed, vb = bits16(P.packed_self(q, k, v), dtype), bits16(v, dtype)
    packed.setflags(write=False); vb.setflags(write=False)
    return packed, vb


class Packed:
    """The packed q | k | v buffer on the device and its q / k / v column views, with the strides a launch reads them through."""

    def __init__(self, tf, bits, nh, hs, dtype):
        b, t, c3 = bits.shape
        self.bits, self.c = bits, c3 // 3
        self.raw = tf.DeviceArray.from_numpy(bits, np.uint16, "row")
        arr = tf.DeviceArray(self.raw.ptr, (b, t, c3), _np_dtype(tf, dtype), "row", base=self.raw)
        self.q, self.k, self.v = arr, arr.view(arr.shape, "row", self.c), arr.view(arr.shape, "row", 2 * self.c)
        self.st = (t * c3, hs, c3)

    def unchanged(self):
        return np.array_equal(self.raw.numpy(), self.bits)


class Out:
    """An output in one of three forms, every word FILL, between GUARD words on each side; bits() checks the guards (and the pad columns) and returns
    the (B, NH, T, HS) bit patterns."""

    def __init__(self, tf, form, b, nh, t, hs, dtype):
        c = nh * hs
        self.form, self.dims = form, (b, nh, t, hs)
        self.shape, self.strides = {"ldm": ((b, t, c), (t * c, hs, c)), "reference": ((b, nh, t, hs), (nh * t * hs, t * hs, hs)),
                                    "ldm_pad4": ((b, t, c + 4), (t * (c + 4), hs, c + 4))}[form]
        self.n = int(np.prod(self.shape))
        self.raw = tf.DeviceArray.from_numpy(np.full(self.n + 2 * GUARD, FILL, np.uint16), np.uint16, "row")
        self.arr = tf.DeviceArray(self.raw.ptr + 2 * GUARD, self.shape, _np_dtype(tf, dtype), "row", base=self.raw)

    def all_words(self):
        return self.raw.numpy()

    def bits(self):
        b, nh, t, hs = self.dims
        w = self.all_words()
        assert (w[:GUARD] == FILL).all() and (w[GUARD + self.n:] == FILL).all(), "guard words around o overwritten"
        o = w[GUARD:GUARD + self.n].reshape(self.shape)
        if self.form == "reference":
            return o
        if self.form == "ldm_pad4":
            assert (o[..., nh * hs:] == FILL).all(), "pad columns of o overwritten"
            o = o[..., :nh * hs]
        return o.reshape(b, t, nh, hs).transpose(0, 2, 1, 3)


def pag_launch(out, pk, flag, rng_, b, nh, t, hs):
    from tinyfusers_amd.attention.sdpa import sdpa_pag_strided
    sdpa_pag_strided(out.arr, pk.q, pk.k, pk.v, flag.ptr, rng_, b, nh, t, t, hs, pk.st, pk.st, pk.st, out.strides)


def pag(tf, out, pk, flag, rng_, b, nh, t, hs):
    pag_launch(out, pk, flag, rng_, b, nh, t, hs)
    return out.bits()


def plain(tf, out, pk, inst, b, nh, t, hs):
    """tf_sdpa_16 on the family the perturbed launch runs: forced unsplit where the per-shape rule would split."""
    from tinyfusers_amd.attention.sdpa import sdpa_instance, sdpa_strided
    from tinyfusers_amd.native import lib
    assert lib.tf_sdpa_force_split(P.force_split_for(inst, t, hs)) == 0
    try:
        assert sdpa_instance(out.arr.dtype, b, nh, t, t, hs, pk.st[2], pk.st[2]) == inst
        sdpa_strided(out.arr, pk.q, pk.k, pk.v, b, nh, t, t, hs, pk.st, pk.st, pk.st, out.strides)
        return out.bits()
    finally:
        lib.tf_sdpa_force_split(0)


def poisoned(bits, c, b0, b1, dtype):
    """The packed buffer with q and k of the batch entries [b0, b1) filled with NaN, +Inf and -Inf patterns."""
    bad = np.array([0x7E00, 0x7C00, 0xFC00] if dtype == "fp16" else [0x7FC0, 0x7F80, 0xFF80], np.uint16)
    out = bits.copy()
    out[b0:b1, :, :2 * c] = bad[np.arange(out[b0:b1, :, :2 * c].size) % 3].reshape(out[b0:b1, :, :2 * c].shape)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inst,b,nh,t,hs", CASES)
def test_flag_and_range(tf, inst, b, nh, t, hs, dtype):
    from tinyfusers_amd.attention.sdpa import sdpa_pag_instance
    packed, vb = inputs(b, nh, t, hs, dtype)
    c = nh * hs
    family = sdpa_pag_instance(_np_dtype(tf, dtype), b, nh, t, t, hs, 3 * c, 3 * c)
    assert t == 64 or family == inst                     # (at the row's own token count the row's family)
    pk = Packed(tf, packed, nh, hs, dtype)
    zero, one = (tf.DeviceArray.from_numpy(np.float32([x]), np.float32, "row") for x in (0.0, 1.0))
    rs = ranges(b)
    for form in ("ldm", "reference", "ldm_pad4"):
        want0 = plain(tf, Out(tf, form, b, nh, t, hs, dtype), pk, family, b, nh, t, hs)
        for name, r in rs.items():                        # (a) flag 0: the plain launch's bits, whatever the range
            got = pag(tf, Out(tf, form, b, nh, t, hs, dtype), pk, zero, r, b, nh, t, hs)
            assert np.array_equal(got, want0), (form, name, "flag 0")
            if form != "ldm":
                break
        for i, (name, (b0, b1)) in enumerate(rs.items()):
            want = want0.copy()
            want[b0:b1] = vb[b0:b1]
            got = pag(tf, Out(tf, form, b, nh, t, hs, dtype), pk, one, (b0, b1), b, nh, t, hs)      # (b)
            assert np.array_equal(got[b0:b1], vb[b0:b1]), (form, name, "perturbed entries are not v's bits")
            assert np.array_equal(got, want), (form, name, "entries outside the range moved")
            if b1 > b0 and (form == "ldm_pad4" or (i + (form == "ldm")) % 2 == 0):                   # (c) the two 16-byte forms see every range between them
                pz = Packed(tf, poisoned(packed, c, b0, b1, dtype), nh, hs, dtype)
                got = pag(tf, Out(tf, form, b, nh, t, hs, dtype), pz, one, (b0, b1), b, nh, t, hs)
                assert np.array_equal(got, want), (form, name, "q / k of a perturbed entry influenced the output")
                assert pz.unchanged()
    assert pk.unchanged(), "the packed q | k | v buffer was written"                                  # (d)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hs", (40, 64, 160))
def test_the_flag_is_read_when_the_kernel_runs(tf, hs, dtype):
    """One captured graph holding one perturbed launch; the fp32 word behind its pointer flips between replays."""
    from tinyfusers_amd.native import hip
    inst, b, nh, t = "dma16", 3, 2, 200
    packed, vb = inputs(b, nh, t, hs, dtype)
    pk = Packed(tf, packed, nh, hs, dtype)
    want0 = plain(tf, Out(tf, "ldm", b, nh, t, hs, dtype), pk, inst, b, nh, t, hs)
    want1 = want0.copy()
    want1[1:2] = vb[1:2]
    flag, o = tf.DeviceArray.from_numpy(np.float32([0.0]), np.float32, "row"), Out(tf, "ldm", b, nh, t, hs, dtype)
    pag(tf, o, pk, flag, (1, 2), b, nh, t, hs)           # (the first launch of an instance sets its LDS attribute: not inside a capture)
    stream, g = tf.Stream(), ctypes.c_void_p()
    with tf.use_stream(stream):
        hip.tf_stream_sync(stream.handle)
        hip.tf_graph_begin_capture(stream.handle)
        try:
            pag_launch(o, pk, flag, (1, 2), b, nh, t, hs)
        finally:
            hip.tf_graph_end_capture(stream.handle, ctypes.byref(g))
        try:
            for word, want in ((1.0, want1), (0.0, want0), (-2.5, want1), (1.0, want1)):
                flag.copy_from_numpy(np.float32([word]))      # (drains the stream, then a blocking copy)
                o.raw.copy_from_numpy(np.full(o.n + 2 * GUARD, FILL, np.uint16))
                hip.tf_graph_launch(g, stream.handle)
                hip.tf_stream_sync(stream.handle)
                assert np.array_equal(o.bits(), want), word
        finally:
            hip.tf_graph_destroy(g)


def test_a_refused_launch_writes_nothing(tf):
    from tinyfusers_amd.native import lib
    b, nh, t, hs = 3, 2, 200, 40
    packed, _ = inputs(b, nh, t, hs, "fp16")
    pk = Packed(tf, packed, nh, hs, "fp16")
    flag, o = tf.DeviceArray.from_numpy(np.float32([1.0]), np.float32, "row"), Out(tf, "ldm", b, nh, t, hs, "fp16")

    def rc(b0=0, b1=1, flag_=flag.ptr, hs_=hs, o_=None, v_st=None):
        st = list(pk.st)
        vs = st[:2] + [v_st or st[2]]
        return lib.tf_sdpa_pag_16(0, o.arr.ptr if o_ is None else o_, pk.q.ptr, pk.k.ptr, pk.v.ptr, b, nh, t, t, hs_, *st, *st, *vs, *o.strides, b0, b1, flag_, None)
    assert rc(b0=-1) == 10001 and rc(b1=4) == 10001 and rc(b0=2, b1=1) == 10001 and b"batch range" in lib.tf_last_error()
    assert rc(flag_=None) == 10001 and b"null flag" in lib.tf_last_error()
    assert rc(hs_=32) == 10002 and rc(hs_=44) == 10001 and rc(v_st=44) == 10001
    assert (o.all_words() == FILL).all() and pk.unchanged()           # every word, the guards included, still holds FILL
    assert rc() == 0 and rc(b0=2, b1=2) == 0 and (o.bits() != FILL).any()
