"""Every attention instance the launcher can pick (tf_sdpa_f16 / tf_sdpa_16: k_sdpa_dma<HS, 1>, <HS, 2>, <40 | 80, 2, 8>, the key-slice forms, the
generic k_sdpa<DQK, DV>), in float16 and bfloat16, at shapes chosen from the dispatch rule instead of the workload (tests/aux/sdpa_planted.py:
INSTANCE_ROWS).  Each case first asserts that tf_sdpa_instance names the instance of its row, then runs it at 77 keys (one full tile plus a
ragged one) and 330 keys (six tiles: the LDS ring of at most four stages wraps; the last tile holds ten keys):

  (a) planted-key inputs against a float64 softmax of the same rounded inputs, atol = one unit in the last place of the storage type at 1.0
      (2^-10 float16, 2^-7 bfloat16), rtol = 0.  Derived, not measured: the outputs lie in [-1, 1] and the target's probability is exactly 1.0
      before normalisation, so the store rounding is half that bound; rounding the pre-scaled Q and P to 16 bits only moves the < 1e-2 of mass
      that is off target (tests/test_sdpa_planted_host.py asserts it), by a few per cent of itself;
  (b) the suite's seeded-normal inputs against the oracle at the tolerance the instance's siblings are held to (1e-2 float16, tests/test_gpu_ops.py;
      2^-6 bfloat16, tests/test_gpu_bf16.py);
  (c) the causal mask at Tq = Tk = 330 on planted inputs (the answer is v_i; the tile clip differs per query block);
  (d) the packed launches the UNet issues (attention/attention.py:122-145): q / k / v as column views of one (B, T, 3 NH HS) buffer, and q next to
      a (B, 77, 2 NH HS) k | v buffer, both with the head merge on the way out.
Each planted case prints its largest error next to the bound (pytest -s)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import sdpa_planted as P  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = ("fp16", "bf16")
ORACLE_TOL = {"fp16": dict(rtol=1e-2, atol=1e-2), "bf16": dict(rtol=2.0 ** -6, atol=2.0 ** -6)}
ROWS = P.rows()
DMA_ROWS = P.rows(("dma16", "dma32", "dma32_w8", "split"))


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def _np_dtype(tf, dtype):
    return tf.bfloat16 if dtype == "bf16" else np.float16


def dev(tf, x, dtype):
    return tf.DeviceArray.from_numpy(x, _np_dtype(tf, dtype), "row")


def launch(tf, inst, dtype, o, q, k, v, b, nh, tq, tk, hs, qs, ks, vs, os_, causal=False, expect=None):
    """sdpa_strided under the tf_sdpa_force_split setting the row needs, after asserting that the launcher's rule names `expect` (default: the
    row's instance) for exactly this launch."""
    from tinyfusers_amd.attention.sdpa import sdpa_instance, sdpa_strided
    from tinyfusers_amd.native import lib
    assert lib.tf_sdpa_force_split(P.force_split_for(inst, tk, hs)) == 0
    try:
        assert sdpa_instance(o.dtype, b, nh, tq, tk, hs, ks[2], vs[2], causal) == (expect or inst)
        sdpa_strided(o, q, k, v, b, nh, tq, tk, hs, qs, ks, vs, os_, causal)
        return o.numpy()
    finally:
        lib.tf_sdpa_force_split(0)


def run(tf, inst, dtype, q, k, v, causal=False, expect=None):
    """(B, NH, T, HS) contiguous q / k / v -> (B, NH, Tq, HS), as scaled_dot_product_attention launches them."""
    b, nh, tq, hs = q.shape
    tk = k.shape[2]
    st = lambda t: (nh * t * hs, t * hs, hs)
    o = tf.DeviceArray.empty((b, nh, tq, hs), _np_dtype(tf, dtype), "row")
    return launch(tf, inst, dtype, o, dev(tf, q, dtype), dev(tf, k, dtype), dev(tf, v, dtype), b, nh, tq, tk, hs, st(tq), st(tk), st(tk), st(tq), causal, expect)


def close_to_float64(got, ref, dtype, what):
    assert np.isfinite(got).all(), "non-finite output"
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"\nplanted {what} {dtype}: max |err| {err:.3e}  bound {P.ATOL[dtype]:.3e}")
    np.testing.assert_allclose(got.astype(np.float64), ref, rtol=0, atol=P.ATOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tk", P.KEY_COUNTS)
@pytest.mark.parametrize("inst,b,nh,tq,hs", ROWS)
def test_planted_keys(tf, inst, b, nh, tq, hs, tk, dtype):
    q, k, v, _, ref, _ = P.planted(b, nh, tq, tk, hs, dtype)
    close_to_float64(run(tf, inst, dtype, q, k, v), ref, dtype, f"{inst} hs={hs} tk={tk}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tk", P.KEY_COUNTS)
@pytest.mark.parametrize("inst,b,nh,tq,hs", ROWS)
def test_seeded_normal_inputs_match_the_oracle(tf, inst, b, nh, tq, hs, tk, dtype):
    from oracle import ops as O
    from tinyfusers_amd.storage.synth import synth_normal
    q, k, v = (P.round16(synth_normal(29, n_, (b, nh, t, hs)), dtype) for n_, t in (("si.q", tq), ("si.k", tk), ("si.v", tk)))
    np.testing.assert_allclose(run(tf, inst, dtype, q, k, v), O.scaled_dot_product_attention(q, k, v).numpy(), **ORACLE_TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inst,b,nh,tq,hs", ROWS)
def test_planted_keys_under_the_causal_mask(tf, inst, b, nh, tq, hs, dtype):
    T = P.CAUSAL_T
    if inst == "split":          # a causal launch is never split: the rule must say so, and what it runs instead is the dma16 rows' case
        from tinyfusers_amd.attention.sdpa import sdpa_instance
        from tinyfusers_amd.native import lib
        assert lib.tf_sdpa_force_split(2) == 0
        try:
            assert sdpa_instance(_np_dtype(tf, dtype), b, nh, T, T, hs, causal=False) == "split"
            assert sdpa_instance(_np_dtype(tf, dtype), b, nh, T, T, hs, causal=True) == "dma16"
        finally:
            lib.tf_sdpa_force_split(0)
        return
    q, k, v, _, ref, _ = P.planted(P.causal_batch(inst, b), nh, T, T, hs, dtype, True)
    close_to_float64(run(tf, inst, dtype, q, k, v, causal=True), ref, dtype, f"{inst} hs={hs} causal")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inst,b,nh,t,hs", DMA_ROWS)
def test_planted_keys_packed_qkv_views(tf, inst, b, nh, t, hs, dtype):
    """Self-attention as attention/attention.py:121-123 launches it: q / k / v are column views of the (B, T, 3 C) projection, merged (B, T, C) output."""
    q, k, v, _, ref, _ = P.planted(b, nh, t, t, hs, dtype)
    c = nh * hs
    qkv = dev(tf, P.packed_self(q, k, v), dtype)
    o = tf.DeviceArray.empty((b, t, c), _np_dtype(tf, dtype), "row")
    st = (t * 3 * c, hs, 3 * c)
    got = launch(tf, inst, dtype, o, qkv, qkv.view((b, t, 3 * c), "row", c), qkv.view((b, t, 3 * c), "row", 2 * c), b, nh, t, t, hs, st, st, st, (t * c, hs, c))
    close_to_float64(P.unmerge(got, nh), ref, dtype, f"{inst} hs={hs} packed q|k|v")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inst,b,nh,tq,hs", DMA_ROWS)
def test_planted_keys_packed_kv_views(tf, inst, b, nh, tq, hs, dtype):
    """Cross-attention as attention/attention.py:129-139 launches it: q from its own (B, T, C) buffer, k / v views of one (B, 77, 2 C) buffer."""
    tk = 77
    q, k, v, _, ref, _ = P.planted(b, nh, tq, tk, hs, dtype)
    c = nh * hs
    xq, xkv = P.packed_cross(q, k, v)
    dq, kv = dev(tf, xq, dtype), dev(tf, xkv, dtype)
    o = tf.DeviceArray.empty((b, tq, c), _np_dtype(tf, dtype), "row")
    ks = (tk * 2 * c, hs, 2 * c)
    got = launch(tf, inst, dtype, o, dq, kv, kv.view(kv.shape, "row", c), b, nh, tq, tk, hs, (tq * c, hs, c), ks, ks, (tq * c, hs, c))
    close_to_float64(P.unmerge(got, nh), ref, dtype, f"{inst} hs={hs} packed k|v")
