"""tf_sdpa_temporal_16 on the GPU: F in {1, 2, 8, 16, 24, 32} frames x head sizes {8, 40, 64, 80, 160}, both storage types, with and without the
positional tables; every case walks the (pixels, heads, videos) triples of tests/aux/sdpa_temporal_planted.py::PNG (P in {1, 5, 64}: 5 is the ragged
pixel tail; NH in {1, 3, 8}: 3 leaves a head group ragged, 8 makes two; G in {1, 3}).

  (a) planted inputs against the float64 softmax of the same inputs, at the bound tests/test_gpu_sdpa_instances.py holds tf_sdpa_16 to (its
      constants, imported): atol = one unit in the last place of the storage type at 1.0, rtol = 0.  It holds for this kernel's rounding points by
      derivation: the operands are widened to fp32 exactly and the tables added in fp32 (planted q', k' are integers: exact; v' errs by <= 2^-24);
      scores, softmax and P V are fp32 sums of at most 160 + 32 terms on values <= 1 (error < 1e-4 of a unit); the ONE rounding to 16 bits is the
      store, half a unit in the last place of an output in [-1, 1] (up to 1 + 2^-7 under tables in bfloat16, where half a unit is 2^-8) -- half the
      bound.  P is never rounded to 16 bits here, unlike in tf_sdpa_16.
  (b) seeded normal inputs against float64 of the 16-bit-rounded operands at that file's ORACLE_TOL;
  (c) without tables: agreement, at ORACLE_TOL, with sdpa_strided on explicitly transposed contiguous copies ((g p), NH, F, HS);
  (d) F = 1 returns v' = v + pe_v rounded once, bit for bit;
  (e) the packed launch the motion module issues: q | k | v column views of one (G F, P, 3 C) buffer, o a (G F, P, C) matrix between guard words
      that come back untouched, the inputs unchanged; two launches agree bit for bit;
  (f) refused launches write nothing.
Each planted case prints its largest error next to the bound (pytest -s)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import sdpa_temporal_planted as TP  # noqa: E402
from test_gpu_sdpa_instances import ORACLE_TOL  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = ("fp16", "bf16")
GUARD = 64                    # elements in front of and behind every output
SENTINEL = -512.0             # (a value of both storage types no output can take)


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def _np_dtype(tf, dtype):
    return tf.bfloat16 if dtype == "bf16" else np.float16


def dev(tf, x, dtype):
    return tf.DeviceArray.from_numpy(np.ascontiguousarray(x), _np_dtype(tf, dtype), "row")


def table(tf, x):
    return None if x is None else tf.DeviceArray.from_numpy(np.ascontiguousarray(x), np.float32, "row")


def guarded(tf, n, dtype):
    """A device buffer of GUARD + n + GUARD elements full of SENTINEL and the view of its middle n."""
    full = dev(tf, np.full(n + 2 * GUARD, SENTINEL, np.float32), dtype)
    return full, full.view((n,), "row", GUARD)


def guards_untouched(full):
    x = full.numpy()
    return bool((x[:GUARD] == SENTINEL).all() and (x[-GUARD:] == SENTINEL).all())


def run(tf, dtype, q, k, v, pe=(None, None, None)):
    """(G, F, P, NH, HS) contiguous q / k / v -> o of the same shape (float32), written between guard words."""
    from tinyfusers_amd.attention.sdpa import sdpa_temporal_strided
    G, F, P, NH, HS = q.shape
    c = NH * HS
    st = (P * c, c, HS)
    full, o = guarded(tf, q.size, dtype)
    sdpa_temporal_strided(o, dev(tf, q, dtype), dev(tf, k, dtype), dev(tf, v, dtype), G, F, P, NH, HS, st, st, st, st, *(table(tf, t) for t in pe))
    out = full.numpy()
    assert (out[:GUARD] == SENTINEL).all() and (out[-GUARD:] == SENTINEL).all(), "the launch wrote outside its output"
    return out[GUARD:-GUARD].reshape(q.shape)


def seeded(G, F, P, NH, HS, dtype, pe, seed=29):
    rng = np.random.default_rng([seed, G, F, P, NH, HS])
    q, k, v = (TP.round16(rng.standard_normal((G, F, P, NH, HS)), dtype) for _ in range(3))
    tabs = tuple(rng.standard_normal((F, NH * HS)).astype(np.float32) * np.float32(0.5) for _ in range(3)) if pe else (None, None, None)
    return q, k, v, tabs


@pytest.mark.parametrize("pe", (False, True), ids=("plain", "tables"))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hs", TP.HEAD_SIZES)
@pytest.mark.parametrize("f", TP.FRAMES)
def test_planted_inputs(tf, f, hs, dtype, pe):
    worst = 0.0
    for p, nh, g in TP.PNG:
        q, k, v, pq, pk, pv, ref = TP.planted(g, f, p, nh, hs, dtype, pe)
        got = run(tf, dtype, q, k, v, (pq, pk, pv))
        assert np.isfinite(got).all(), "non-finite output"
        err = float(np.abs(got.astype(np.float64) - ref).max())
        worst = max(worst, err)
        assert err <= TP.ATOL[dtype], (p, nh, g, err, TP.ATOL[dtype])
    print(f"\nplanted temporal F={f} hs={hs} {dtype} tables={pe}: max |err| {worst:.3e}  bound {TP.ATOL[dtype]:.3e}")


@pytest.mark.parametrize("pe", (False, True), ids=("plain", "tables"))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hs", TP.HEAD_SIZES)
@pytest.mark.parametrize("f", TP.FRAMES)
def test_seeded_normal_inputs_match_float64(tf, f, hs, dtype, pe):
    for p, nh, g in ((5, 3, 3), (64, 8, 1), (1, 1, 1)):
        q, k, v, tabs = seeded(g, f, p, nh, hs, dtype, pe)
        np.testing.assert_allclose(run(tf, dtype, q, k, v, tabs), TP.ref64(q, k, v, *tabs), **ORACLE_TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hs", TP.HEAD_SIZES)
@pytest.mark.parametrize("f", TP.FRAMES)
def test_agrees_with_the_key_tile_kernel_on_transposed_copies(tf, f, hs, dtype):
    """What the kernel replaces: transpose to ((g p), NH, F, HS) contiguous, tf_sdpa_16 over the F tokens, transpose back."""
    from tinyfusers_amd.attention.sdpa import sdpa_strided
    g, p, nh = 3, 5, 3
    q, k, v, _ = seeded(g, f, p, nh, hs, dtype, False)
    got = run(tf, dtype, q, k, v)
    tr = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1, 4).reshape(g * p, nh, f, hs))
    st = (nh * f * hs, f * hs, hs)
    o = tf.DeviceArray.empty((g * p, nh, f, hs), _np_dtype(tf, dtype), "row")
    sdpa_strided(o, dev(tf, tr(q), dtype), dev(tf, tr(k), dtype), dev(tf, tr(v), dtype), g * p, nh, f, f, hs, st, st, st, st)
    back = o.numpy().reshape(g, p, nh, f, hs).transpose(0, 3, 1, 2, 4)
    np.testing.assert_allclose(got, back, **ORACLE_TOL[dtype])


@pytest.mark.parametrize("pe", (False, True), ids=("plain", "tables"))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hs", TP.HEAD_SIZES)
def test_one_frame_returns_v_rounded_once(tf, hs, dtype, pe):
    for p, nh, g in TP.PNG:
        q, k, v, tabs = seeded(g, 1, p, nh, hs, dtype, pe)
        want = v if not pe else TP.round16(v + tabs[2].reshape(1, 1, 1, nh, hs), dtype)          # (the fp32 sum, rounded to nearest even)
        got = run(tf, dtype, q, k, v, tabs)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (p, nh, g)


@pytest.mark.parametrize("pe", (False, True), ids=("plain", "tables"))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("f,hs,p,nh,g", [(16, 40, 5, 8, 2), (8, 64, 64, 2, 1), (24, 160, 5, 3, 3), (32, 8, 5, 8, 1), (2, 80, 1, 1, 3)])
def test_packed_qkv_views(tf, f, hs, p, nh, g, dtype, pe):
    """The launch of the motion module: q | k | v as column views of the (G F, P, 3 C) projection, o the (G F, P, C) token matrix."""
    from tinyfusers_amd.attention.sdpa import sdpa_temporal_strided
    q, k, v, pq, pk, pv, ref = TP.planted(g, f, p, nh, hs, dtype, pe)
    c = nh * hs
    host = TP.packed(q, k, v)
    qkv = dev(tf, host, dtype)
    tabs = [table(tf, t) for t in (pq, pk, pv)]
    si, so = (p * 3 * c, 3 * c, hs), (p * c, c, hs)
    outs = []
    for _ in range(2):
        full, o = guarded(tf, g * f * p * c, dtype)
        sdpa_temporal_strided(o, qkv, qkv.view(qkv.shape, "row", c), qkv.view(qkv.shape, "row", 2 * c), g, f, p, nh, hs, si, si, si, so, *tabs)
        assert guards_untouched(full)
        outs.append(full.numpy()[GUARD:-GUARD].reshape(g, f, p, nh, hs))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "two launches differ"
    assert np.array_equal(qkv.numpy(), host), "the launch wrote to its inputs"
    err = float(np.abs(outs[0].astype(np.float64) - ref).max())
    print(f"\nplanted temporal packed F={f} hs={hs} {dtype} tables={pe}: max |err| {err:.3e}  bound {TP.ATOL[dtype]:.3e}")
    assert err <= TP.ATOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_refused_launches_write_nothing(tf, dtype):
    from tinyfusers_amd.attention.sdpa import sdpa_temporal_strided
    g, f, p, nh, hs = 1, 8, 5, 2, 40
    c = nh * hs
    x = dev(tf, np.zeros((g * 40, p, c), np.float32), dtype)          # (room for the 33 frames the second case asks for)
    full, o = guarded(tf, g * 40 * p * c, dtype)
    st = (p * c, c, hs)
    bad = [dict(F=0), dict(F=33), dict(HS=12, NH=5), dict(HS=168, NH=1), dict(st=(p * c + 4, c, hs)), dict(st=(p * c, c, hs + 4))]
    for kw in bad:
        s = kw.get("st", st)
        with pytest.raises(RuntimeError, match="tf_sdpa_temporal_16 failed with status 1000[12]"):
            sdpa_temporal_strided(o, x, x, x, g, kw.get("F", f), p, kw.get("NH", nh), kw.get("HS", hs), s, st, st, st)
    from tinyfusers_amd.native import lib
    assert lib.tf_sdpa_temporal_16(0, None, x.ptr, x.ptr, x.ptr, None, None, None, g, f, p, nh, hs, *st, *st, *st, *st, None) == 10001
    assert (full.numpy() == SENTINEL).all()
