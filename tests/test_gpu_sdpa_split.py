"""Key slices inside the attention block (k_sdpa_split: two slices of the key tiles per query group, merged through LDS in slice order), forced
through tf_sdpa_force_split(2) at shapes small enough to reach every path of the split: slices of 2 + 2, 2 + 1, 1 + 1 and 1 + 0 tiles, a last
tile of two keys, one key, ragged and single-query blocks, strided q / k / v, and the online-softmax corners on either side of the seam.
Each output is held against the CPU oracle at the per-op tolerance (attention/sdpa.py:53-77; tests/sdpa.py:100) and against a float64 softmax
of the same fp16 inputs: the split may be no further from it than the unsplit kernel plus one fp16 rounding of the largest output,
err_split <= err_unsplit + 2^-11 max|ref| -- the merge adds two fp32 multiply-adds per element (2^-24 relative) under the fp16 store."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-2, atol=1e-2)


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def rnd(name, shape, std=1.0, seed=23):
    from tinyfusers_amd.storage.synth import synth_normal
    return synth_normal(seed, name, shape, std).astype(np.float16).astype(np.float32)


def _h(x):
    return np.asarray(x, dtype=np.float16).astype(np.float32)


def ref64(q, k, v):
    """softmax(q k^T / sqrt(d)) v in float64, head by head."""
    out = np.empty(q.shape[:-1] + (v.shape[-1],), np.float64)
    for i in np.ndindex(*q.shape[:2]):
        s = q[i].astype(np.float64) @ k[i].astype(np.float64).T / np.sqrt(q.shape[-1])
        p = np.exp(s - s.max(axis=-1, keepdims=True))
        out[i] = (p / p.sum(axis=-1, keepdims=True)) @ v[i].astype(np.float64)
    return out


def run(tf, q, k, v, ks, expect=None):
    """scaled_dot_product_attention under tf_sdpa_force_split(ks); `expect`: the number of slices the launch must take."""
    from tinyfusers_amd.attention.sdpa import scaled_dot_product_attention
    from tinyfusers_amd.native import lib
    D = lambda a: tf.DeviceArray.from_numpy(a, np.float16, "row")
    assert lib.tf_sdpa_force_split(ks) == 0
    try:
        if expect is not None:
            b, nh, tq, hs = q.shape
            assert lib.tf_sdpa_split_ks(b, nh, tq, k.shape[2], hs, 0) == expect
        return scaled_dot_product_attention(D(q), D(k), D(v)).numpy()
    finally:
        lib.tf_sdpa_force_split(0)


def check(tf, q, k, v, oracle_ref=None):
    """forced split against the oracle, against float64 next to the unsplit kernel, and against itself; returns the split output."""
    from oracle import ops as O
    split, again, unsplit = run(tf, q, k, v, 2, expect=2), run(tf, q, k, v, 2), run(tf, q, k, v, 1, expect=1)
    assert np.isfinite(split).all(), "non-finite output"
    assert np.array_equal(split, again), "two runs of the split kernel differ"
    want = O.scaled_dot_product_attention(q, k, v).numpy() if oracle_ref is None else oracle_ref
    np.testing.assert_allclose(split.astype(np.float32), want, **TOL)
    r = ref64(q, k, v)
    err_split, err_unsplit = np.abs(split - r).max(), np.abs(unsplit - r).max()
    bound = err_unsplit + 2.0 ** -11 * np.abs(r).max()
    print(f"err_split {err_split:.3e} err_unsplit {err_unsplit:.3e} bound {bound:.3e}")
    assert err_split <= bound, (err_split, err_unsplit, bound)
    return split


SHAPES = [  # tq, tk
    (128, 256),     # two tiles per slice
    (128, 192),     # slices of 2 + 1 tiles
    (128, 130),     # 2 + 1 tiles, the last tile holds 2 keys
    (128, 77),      # one tile per slice (forced: the automatic choice wants two)
    (128, 64),      # slice 1 is empty
    (128, 1),       # one key
    (200, 256),     # ragged query block
    (1, 256),       # one query
]


@pytest.mark.parametrize("hs", [40, 80])
@pytest.mark.parametrize("tq,tk", SHAPES)
def test_split_shapes(tf, tq, tk, hs):
    q, k, v = rnd("sp.q", (1, 2, tq, hs)), rnd("sp.k", (1, 2, tk, hs)), rnd("sp.v", (1, 2, tk, hs))
    check(tf, q, k, v)


def test_split_at_4096_keys(tf):
    """(1, 2, 4096, 4096, 40) of test_gpu_ops.py's SDPA_CASES: 32 tiles per slice, 16 blocks of the 16-wave form per head."""
    q, k, v = rnd("sd.q", (1, 2, 4096, 40), seed=11), rnd("sd.k", (1, 2, 4096, 40), seed=11), rnd("sd.v", (1, 2, 4096, 40), seed=11)
    check(tf, q, k, v)


@pytest.mark.parametrize("hs", [40, 80])
def test_split_strided_qkv_views(tf, hs):
    """q / k / v as views of one (b, t, 3c) buffer and the LDM head merge on the way out, as attention/attention.py:122-145 launches it."""
    from oracle import ops as O
    from tinyfusers_amd.attention.sdpa import sdpa_strided
    from tinyfusers_amd.native import lib
    b, nh, t = 1, 2, 256
    c = nh * hs
    x = rnd("sv.qkv", (b, t, 3 * c))
    heads = lambda a: np.ascontiguousarray(a.reshape(b, t, nh, hs).transpose(0, 2, 1, 3))
    q, k, v = heads(x[..., :c]), heads(x[..., c:2 * c]), heads(x[..., 2 * c:])
    outs = {}
    for ks in (2, 1):
        qkv = tf.DeviceArray.from_numpy(x, np.float16, "row")
        o = tf.DeviceArray.empty((b, t, c), np.float16, "row")
        st = (t * 3 * c, hs, 3 * c)
        assert lib.tf_sdpa_force_split(ks) == 0
        try:
            sdpa_strided(o, qkv, qkv.view((b, t, 3 * c), "row", c), qkv.view((b, t, 3 * c), "row", 2 * c), b, nh, t, t, hs, st, st, st, (t * c, hs, c))
            outs[ks] = heads(o.numpy().astype(np.float32))
        finally:
            lib.tf_sdpa_force_split(0)
    np.testing.assert_allclose(outs[2], O.scaled_dot_product_attention(q, k, v).numpy(), **TOL)
    r = ref64(q, k, v)
    assert np.abs(outs[2] - r).max() <= np.abs(outs[1] - r).max() + 2.0 ** -11 * np.abs(r).max()


@pytest.mark.parametrize("hs", [40, 80])
def test_split_spike_in_slice_1_rescales_slice_0(tf, hs):
    """One score of slice 1 (keys 128 .. 255) far above everything slice 0 saw -- more than 2^6 in the kernel's log2 units: the merge must
    scale slice 0's accumulators and row sums down to slice 1's reference maximum."""
    q, k, v = rnd("ss.q", (1, 2, 128, hs), 0.5), rnd("ss.k", (1, 2, 256, hs), 0.5), rnd("ss.v", (1, 2, 256, hs))
    k[0, 0, 200] = q[0, 0, 17] * 6.0
    k[0, 1, 130] = q[0, 1, 99] * 8.0
    q, k = _h(q), _h(k)
    s = (q[0, 0, 17] @ k[0, 0].T) / np.sqrt(hs) * np.log2(np.e)
    assert s[200] - s[:128].max() > 6.0
    check(tf, q, k, v)


@pytest.mark.parametrize("hs", [40, 80])
def test_split_first_tile_of_slice_1_far_below_zero(tf, hs):
    """Slice 1's first tile (keys 128 .. 191) hugely negative, its second far above slice 0: each slice adopts the maximum of its OWN first tile
    whatever the sign, raises it later, and the merge brings the two references together."""
    q, k, v = rnd("sf.q", (1, 2, 128, hs)), rnd("sf.k", (1, 2, 256, hs), 0.05), rnd("sf.v", (1, 2, 256, hs))
    u = np.sign(q.mean(axis=2, keepdims=True))
    k[:, :, 128:192] -= 3.0 * u * np.abs(q).mean()
    q = q + 2.0 * u
    k[:, :, 192:] += 1.5 * u
    check(tf, _h(q), _h(k), v)


@pytest.mark.parametrize("hs", [40, 80])
def test_split_slice_1_hugely_negative(tf, hs):
    """Every score of slice 1 hundreds of units below slice 0's: its merge weight 2^(m_1 - M) underflows to 0, which is the right value -- no NaN,
    and the output is slice 0's softmax."""
    q, k, v = rnd("sn.q", (1, 2, 128, hs)), rnd("sn.k", (1, 2, 256, hs), 0.05), rnd("sn.v", (1, 2, 256, hs))
    u = np.sign(q.mean(axis=2, keepdims=True))
    q = q + 2.0 * u
    k[:, :, 128:] -= 30.0 * u
    q, k = _h(q), _h(k)
    got = check(tf, q, k, v)
    np.testing.assert_allclose(got, ref64(q, k[:, :, :128], v[:, :, :128]), **TOL)


@pytest.mark.parametrize("hs", [40, 80])
def test_split_rows_sum_to_one(tf, hs):
    """V = 1: the merged row sums (row HS of O^T at d = 40, the ones-MFMA's accumulator at d = 80) divide the merged rows exactly."""
    rng = np.random.default_rng(hs)
    q, k = _h(rng.standard_normal((1, 2, 200, hs)) * 2), _h(rng.standard_normal((1, 2, 300, hs)) * 2)
    o = run(tf, q, k, np.ones((1, 2, 300, hs), np.float32), 2, expect=2)
    np.testing.assert_allclose(o, 1.0, rtol=0, atol=2e-3)


def test_automatic_choice(tf):
    """From the shape alone: the 32 x 32 self-attention of the SD-1.5 step (one 16-query wave per SIMD unsplit) takes the split kernel; cross-attention
    (77 keys: a tile per slice) and a shape whose grid already fills the chip keep the kernel they had, bit for bit."""
    from tinyfusers_amd.native import lib
    assert lib.tf_sdpa_force_split(0) == 0
    for (b, nh, tq, tk, hs), want in (((2, 8, 1024, 1024, 80), 2), ((2, 8, 4096, 77, 40), 1), ((16, 8, 512, 512, 80), 1)):
        assert lib.tf_sdpa_split_ks(b, nh, tq, tk, hs, 0) == want
        assert lib.tf_sdpa_split_ks(b, nh, tq, tk, hs, 1) == 1          # never under the causal mask
        q, k, v = rnd("au.q", (b, nh, tq, hs)), rnd("au.k", (b, nh, tk, hs)), rnd("au.v", (b, nh, tk, hs))
        auto, same = run(tf, q, k, v, 0), run(tf, q, k, v, want)
        assert np.array_equal(auto, same)
        if want == 2:
            assert not np.array_equal(auto, run(tf, q, k, v, 1))         # (another summation order: the two kernels do not agree to the bit)
