"""tf_sdpa_dual_16, o = softmax(q k^T / sqrt d) v + s softmax(q k2^T / sqrt d) v2 in one launch (k_sdpa_dual<HS, 1>, <HS, 2>, <40 | 80, 2, 8>), in
float16 and bfloat16, at shapes chosen from the dispatch rule (tests/aux/sdpa_dual_planted.py: ROWS = sdpa_planted.INSTANCE_ROWS' dma16 / dma32 /
dma32_w8 rows at d = 40 / 80 / 160).  Each case first asserts that tf_sdpa_dual_instance names the family of its row.  77 text keys are one full tile
plus a ragged one; at 330 the ring of at most four stages wraps before the image tile lands in it.  1, 4, 16 and 64 image keys.

  (a) planted inputs against float64 for s in {0.6, 1, 2} and gamma in {0.5, 1, 1.5}, rtol = 0, atol = 2 ATOL[dtype] (1 + |s|).  Derived, not
      measured: the result lies in [-(1 + |s|), 1 + |s|], so the store rounding is <= ATOL (1 + |s|) / 2 ... ATOL (1 + |s|) (one unit in the last
      place of the storage type at 1.0 is ATOL; beyond 2.0 it doubles); each term carries the single kernel's own internal allowance, 2^-11-class
      (tests/test_gpu_sdpa_instances.py), scaled by 1 and by |s|; the 16-bit rounding of the rescaled P adds <= |s| half an ulp.  The image keys and
      values are handed over as the first Tk2 rows of a 64-row tile whose further rows repeat the targets' patterns under other values: a kernel
      that leaves the tail unmasked reads them.  Each case prints its largest error next to the bound (pytest -s);
  (b) s = 0: value-equal (np.array_equal on the floats) to tf_sdpa_16 of the text set alone at the same shape, forced to the unsplit family the
      dual launch runs, on planted and on seeded-normal inputs -- scale 0 is the adapter switched off, exactly;
  (c) seeded-normal inputs against the oracle, each term at the tolerance the single kernel is held to (ORACLE_TOL of
      tests/test_gpu_sdpa_instances.py): |err| <= atol (1 + |s|) + rtol (|o1| + |s| |o2|).  This departs from "ORACLE_TOL scaled by (1 + |s|)" in
      one respect, on purpose: the relative part is taken on the two summands, not on their sum -- each term is held to the single kernel's own
      tolerance, and where the terms cancel (s < 0 is among the cases) a bound relative to the small sum would ask more of the fused launch than the
      two separate launches meet.  The value equality of (b) and the float64 cases of (a) carry the weight.  Planted inputs cannot see a
      phantom key of score 0 (its mass is e^-24 at most); this case does;
  (d) 64 image keys, on seeded-normal inputs only (the planted image keys number 16);
  (e) the packed launches the UNet issues: q (B, Tq, C), text k | v as column views of a (B, 77, kv_n) step-level buffer, image k2 | v2 as column
      views of a (B, T, kv_n) one, both head merges on the way out;
  (f) EVERY launch of this file writes into a buffer that ends in guard words, and they come back untouched;
  (g) the scale is read from the device when the kernel runs: one captured graph, the scale changed between two replays, the two float64 answers;
  (h) refusals (Tk2 = 0, 65, an unsupported head size, null pointers, misaligned strides) leave the output untouched; their status and message are
      pinned, without a device, by tests/test_sdpa_dual_rule.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import sdpa_dual_planted as D  # noqa: E402
import sdpa_planted as P  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = ("fp16", "bf16")
ORACLE_TOL = {"fp16": dict(rtol=1e-2, atol=1e-2), "bf16": dict(rtol=2.0 ** -6, atol=2.0 ** -6)}      # tests/test_gpu_sdpa_instances.py
GUARD, FILL = 64, 0x3A55                # guard words behind o, and the bit pattern every output word starts from (finite in both types)


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def _np_dtype(tf, dtype):
    return tf.bfloat16 if dtype == "bf16" else np.float16


def dev(tf, x, dtype):
    return tf.DeviceArray.from_numpy(x, _np_dtype(tf, dtype), "row")


def scale_dev(tf, s):
    return tf.DeviceArray.from_numpy(np.float32([s]), np.float32, "row")


class Out:
    """An output of `shape` whose words all hold FILL, followed by GUARD more; get() checks the guard and returns the floats."""

    def __init__(self, tf, shape, dtype):
        self.n = int(np.prod(shape))
        self.raw = tf.DeviceArray.from_numpy(np.full(self.n + GUARD, FILL, np.uint16), np.uint16, "row")
        self.arr = tf.DeviceArray(self.raw.ptr, shape, _np_dtype(tf, dtype), "row", base=self.raw)

    def bits(self):
        return self.raw.numpy().astype(np.uint16)

    def get(self):
        out = self.arr.numpy()
        assert (self.bits()[self.n:] == FILL).all(), "guard words behind o overwritten"
        return out


def launch(tf, inst, o, q, k, v, k2, v2, sc, b, nh, tq, tk, tk2, hs, qs, ks, vs, k2s, v2s, os_):
    from tinyfusers_amd.attention.sdpa import sdpa_dual_instance, sdpa_dual_strided
    assert sdpa_dual_instance(o.dtype, b, nh, tq, tk, tk2, hs, ks[2], vs[2], k2s[2], v2s[2]) == inst
    return sdpa_dual_strided(o, q, k, v, k2, v2, sc.ptr, b, nh, tq, tk, tk2, hs, qs, ks, vs, k2s, v2s, os_)


def run(tf, inst, dtype, q, k, v, k2, v2, sc, tk2=None):
    """(B, NH, T, HS) contiguous device arrays -> (B, NH, Tq, HS) floats; k2 / v2 may hold more rows than the tk2 the kernel is told to read."""
    b, nh, tq, hs = q.shape
    tk, rows2 = k.shape[2], k2.shape[2]
    st = lambda t: (nh * t * hs, t * hs, hs)
    o = Out(tf, (b, nh, tq, hs), dtype)
    launch(tf, inst, o.arr, q, k, v, k2, v2, sc, b, nh, tq, tk, tk2 or rows2, hs, st(tq), st(tk), st(tk), st(rows2), st(rows2), st(tq))
    return o.get()


def text_only(tf, inst, dtype, q, k, v):
    """tf_sdpa_16 of the text set, on the unsplit family the dual launch of the shape runs (tests/test_gpu_sdpa_instances.py: launch)."""
    from tinyfusers_amd.attention.sdpa import sdpa_instance, sdpa_strided
    from tinyfusers_amd.native import lib
    b, nh, tq, hs = q.shape
    tk = k.shape[2]
    st = lambda t: (nh * t * hs, t * hs, hs)
    o = Out(tf, (b, nh, tq, hs), dtype)
    assert lib.tf_sdpa_force_split(1) == 0
    try:
        assert sdpa_instance(o.arr.dtype, b, nh, tq, tk, hs) == inst
        sdpa_strided(o.arr, q, k, v, b, nh, tq, tk, hs, st(tq), st(tk), st(tk), st(tq))
        return o.get()
    finally:
        lib.tf_sdpa_force_split(0)


def atol_for(dtype, s):
    return 2.0 * P.ATOL[dtype] * (1.0 + abs(s))


def close_to_float64(got, ref, dtype, s, what):
    assert np.isfinite(got).all(), "non-finite output"
    err, bound = float(np.abs(got.astype(np.float64) - ref).max()), atol_for(dtype, s)
    print(f"\nplanted dual {what} {dtype} s={s}: max |err| {err:.3e}  bound {bound:.3e}")
    assert err <= bound, (what, s, err, bound)


def normal_inputs(b, nh, tq, tk, tk2, hs, dtype):
    from tinyfusers_amd.storage.synth import synth_normal
    return [P.round16(synth_normal(29, n_, (b, nh, t, hs)), dtype) for n_, t in (("sd.q", tq), ("sd.k", tk), ("sd.v", tk), ("sd.k2", tk2), ("sd.v2", tk2))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tk2", D.IMAGE_KEY_COUNTS)
@pytest.mark.parametrize("tk", P.KEY_COUNTS)
@pytest.mark.parametrize("inst,b,nh,tq,hs", D.ROWS)
def test_planted_keys(tf, inst, b, nh, tq, hs, tk, tk2, dtype):
    o1, _ = D.text_term(b, nh, tq, tk, hs, dtype)
    k2t, v2t = D.image_tile(b, nh, tk, hs, dtype)
    d_k = d_v = None
    d_k2, d_v2 = dev(tf, k2t, dtype), dev(tf, v2t, dtype)
    scales = {s: scale_dev(tf, s) for s in D.SCALES}
    for gamma in D.GAMMAS:
        q, k, v, k2, v2, _, u = D.planted(b, nh, tq, tk, tk2, hs, dtype, gamma)
        if d_k is None:
            d_k, d_v = dev(tf, k, dtype), dev(tf, v, dtype)
        o2, _ = D.image_term(q, k2, v2, u)
        d_q = dev(tf, q, dtype)
        for s in D.SCALES:
            close_to_float64(run(tf, inst, dtype, d_q, d_k, d_v, d_k2, d_v2, scales[s], tk2), o1 + s * o2, dtype, s, f"{inst} hs={hs} tk={tk} tk2={tk2} gamma={gamma}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tk", P.KEY_COUNTS)
@pytest.mark.parametrize("inst,b,nh,tq,hs", D.ROWS)
def test_scale_zero_is_the_text_launch(tf, inst, b, nh, tq, hs, tk, dtype):
    zero = scale_dev(tf, 0.0)
    q, k, v, k2, v2, _, _ = D.planted(b, nh, tq, tk, 4, hs, dtype, 1.5)
    for what, (q, k, v, k2, v2) in (("planted", (q, k, v, k2, v2)), ("normal", normal_inputs(b, nh, tq, tk, 4, hs, dtype))):
        d = [dev(tf, a, dtype) for a in (q, k, v, k2, v2)]
        got, want = run(tf, inst, dtype, *d, zero), text_only(tf, inst, dtype, *d[:3])
        assert np.isfinite(got).all() and np.array_equal(got, want), (what, float(np.abs(got - want).max()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tk2", D.IMAGE_KEY_COUNTS + (64,))
@pytest.mark.parametrize("tk", P.KEY_COUNTS)
@pytest.mark.parametrize("inst,b,nh,tq,hs", D.ROWS)
def test_seeded_normal_inputs_match_the_oracle(tf, inst, b, nh, tq, hs, tk, tk2, dtype):
    from oracle import ops as O
    q, k, v, k2, v2 = normal_inputs(b, nh, tq, tk, tk2, hs, dtype)
    o1, o2 = O.scaled_dot_product_attention(q, k, v).numpy().astype(np.float64), O.scaled_dot_product_attention(q, k2, v2).numpy().astype(np.float64)
    d = [dev(tf, a, dtype) for a in (q, k, v, k2, v2)]
    tol = ORACLE_TOL[dtype]
    for s in (0.6, -2.0):
        got = run(tf, inst, dtype, *d, scale_dev(tf, s))
        bound = tol["atol"] * (1 + abs(s)) + tol["rtol"] * (np.abs(o1) + abs(s) * np.abs(o2))
        err = np.abs(got - (o1 + s * o2))
        assert np.isfinite(got).all() and (err <= bound).all(), (s, float(err.max()), float((err - bound).max()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inst,b,nh,tq,hs", D.ROWS)
def test_planted_keys_packed_kv_views(tf, inst, b, nh, tq, hs, dtype):
    """Cross-attention as the adapted UNet launches it: q from its own (B, Tq, C) buffer; text k | v column views of the step-level (B, 77, kv_n)
    buffer and image k2 | v2 column views of the (B, T, kv_n) one (this block's 2 C columns sit behind another block's), both head merges."""
    tk, tk2, s, gamma = 77, 4, 0.6, 1.5
    q, k, v, k2, v2, _, u = D.planted(b, nh, tq, tk, tk2, hs, dtype, gamma)
    ref = D.text_term(b, nh, tq, tk, hs, dtype)[0] + s * D.image_term(q, k2, v2, u)[0]
    c = nh * hs
    kv_n, off = 2 * c + 2 * c, 2 * c                     # [another block's k | v] [this block's k | v]
    tok = lambda a: a.transpose(0, 2, 1, 3).reshape(a.shape[0], a.shape[2], -1)
    pad = lambda t: np.full((b, t, off), 3.0, np.float32)
    kv, kv2 = dev(tf, np.concatenate([pad(tk), tok(k), tok(v)], axis=-1), dtype), dev(tf, np.concatenate([pad(tk2), tok(k2), tok(v2)], axis=-1), dtype)
    dq, sc = dev(tf, tok(q), dtype), scale_dev(tf, s)
    ks, k2s = (tk * kv_n, hs, kv_n), (tk2 * kv_n, hs, kv_n)
    for merge, os_ in (("ldm", (tq * c, hs, c)), ("reference", (nh * tq * hs, tq * hs, hs))):
        o = Out(tf, (b, tq, c) if merge == "ldm" else (b, nh, tq, hs), dtype)
        launch(tf, inst, o.arr, dq, kv.view(kv.shape, "row", off), kv.view(kv.shape, "row", off + c), kv2.view(kv2.shape, "row", off), kv2.view(kv2.shape, "row", off + c),
               sc, b, nh, tq, tk, tk2, hs, (tq * c, hs, c), ks, ks, k2s, k2s, os_)
        got = o.get()
        close_to_float64(P.unmerge(got, nh) if merge == "ldm" else got, ref, dtype, s, f"{inst} hs={hs} packed, {merge} merge")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hs", D.HEAD_SIZES)
def test_the_scale_is_read_when_the_kernel_runs(tf, hs, dtype):
    """One captured graph holding one dual launch; the fp32 scale behind its pointer changes between two replays."""
    from tinyfusers_amd.native import hip
    inst, b, nh, tq, tk, tk2, gamma = "dma16", 1, 2, 200, 77, 4, 1.5
    q, k, v, k2, v2, _, u = D.planted(b, nh, tq, tk, tk2, hs, dtype, gamma)
    o1, o2 = D.text_term(b, nh, tq, tk, hs, dtype)[0], D.image_term(q, k2, v2, u)[0]
    d = [dev(tf, a, dtype) for a in (q, k, v, k2, v2)]
    sc, st = scale_dev(tf, 1.0), lambda t: (nh * t * hs, t * hs, hs)
    o = Out(tf, (b, nh, tq, hs), dtype)
    go = lambda: launch(tf, inst, o.arr, *d, sc, b, nh, tq, tk, tk2, hs, st(tq), st(tk), st(tk), st(tk2), st(tk2), st(tq))
    go()                                                  # (the first launch of an instance sets its LDS attribute: not inside a capture)
    stream, g = tf.Stream(), ctypes.c_void_p()
    with tf.use_stream(stream):
        hip.tf_stream_sync(stream.handle)
        hip.tf_graph_begin_capture(stream.handle)
        try:
            go()
        finally:
            hip.tf_graph_end_capture(stream.handle, ctypes.byref(g))
        try:
            for s in (0.6, 2.0):
                sc.copy_from_numpy(np.float32([s]))       # (drains the stream, then a blocking copy)
                hip.tf_graph_launch(g, stream.handle)
                close_to_float64(o.get(), o1 + s * o2, dtype, s, f"captured hs={hs}")
        finally:
            hip.tf_graph_destroy(g)


def test_a_refused_launch_writes_nothing(tf):
    from tinyfusers_amd.native import lib
    b, nh, tq, tk, tk2, hs = 1, 2, 200, 77, 4, 40
    d = [dev(tf, a, "fp16") for a in normal_inputs(b, nh, tq, tk, 64, hs, "fp16")]
    sc, o = scale_dev(tf, 1.0), Out(tf, (b, nh, tq, hs), "fp16")
    st = lambda t, last=hs: (nh * t * hs, t * hs, last)

    def rc(tk2=tk2, hs_=hs, ptrs=None, k2_last=hs):
        p = ptrs or [o.arr.ptr] + [a.ptr for a in d] + [sc.ptr]
        return lib.tf_sdpa_dual_16(0, p[0], p[1], p[2], p[3], tk, p[4], p[5], tk2, p[6], b, nh, tq, hs_, *st(tq), *st(tk), *st(tk), *st(64, k2_last), *st(64), *st(tq), None)
    assert rc(tk2=0) == 10001 and rc(tk2=65) == 10002 and rc(hs_=64) == 10002 and rc(k2_last=44) == 10001
    for i in range(7):
        p = [o.arr.ptr] + [a.ptr for a in d] + [sc.ptr]
        p[i] = None
        assert rc(ptrs=p) == 10001 and b"null" in lib.tf_last_error()
    assert (o.bits() == FILL).all()                     # every word, the guard included, still holds FILL
    assert rc() == 0 and np.isfinite(o.get()).all()
