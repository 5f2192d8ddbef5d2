"""Planted-key attention inputs and their float64 answer (host code, numpy only), and the table of attention instances the tests walk.

Random q / k / v at hundreds of keys give outputs of standard deviation 0.03 - 0.05: a kernel that loses one key, or one tile, stays inside any
usable tolerance.  Here every query is a scaled copy of ONE key of its head, its target, so that the softmax puts all but < 1e-6 of its mass
(causal variant: < 5e-3) on that key and the output is that key's value row, a row of multiples of 1 / 128 in [-1, 1] that differs from every other key's: a wrong,
missing or mis-addressed key moves the output by O(1).  The matching score is 48 nats (69 in the kernels' log2 units), far beyond their
rescale threshold, so every query whose target lies behind the first key tile takes the rescale branch of the online softmax.

The expected value is the float64 softmax of the ROUNDED inputs (ref64), never v[target] itself; tests/test_sdpa_planted_host.py asserts the
conditions this rests on (target mass >= 0.99, and that each mutant of ref64 -- a dropped tile, rolled value rows, a shifted causal mask, a
neighbour's keys -- moves some output by more than 0.25) for every shape of the table."""
import functools
import math

import numpy as np

GAIN_NATS = 48.0          # score of a query against its target, in nats

# instance (attention.sdpa.SDPA_INSTANCES' name) -> B, NH, Tq, head sizes.  blocks2 = ceil(Tq / 128) NH B, blocks8 = ceil(Tq / 256) NH B:
# dma16 below 256 blocks2; dma32 at blocks2 = 256, blocks8 = 128; dma32_w8 at blocks8 = 512 (d = 40: 4096 waves, so the per-shape split rule
# steps aside); split is forced (tf_sdpa_force_split(2)); generic is every head size without a DMA kernel.
INSTANCE_ROWS = [
    ("dma16", 1, 2, 200, (40, 64, 80, 128, 160)),
    ("dma32", 8, 16, 200, (40, 64, 80, 128, 160)),
    ("dma32_w8", 16, 16, 300, (40, 80)),
    ("split", 1, 2, 200, (40, 80)),
    ("generic", 1, 2, 200, (32, 56, 72, 96, 120, 152)),
]
KEY_COUNTS = (77, 330)    # one full tile plus a ragged one; six tiles (the ring of at most four stages wraps), the last of ten keys
CAUSAL_T = 330            # three 128-query blocks (two of 256 on the eight-wave form): the causal tile clip differs per block


def causal_batch(inst, B):
    """The batch of a row's causal case.  At 330 queries the dma32 row's 128 heads make blocks8 = 256, and d = 40 / 80 would move to the eight-wave
    form: 7 x 16 = 112 heads keep blocks2 = 336 >= 256 with blocks8 = 224 < 256."""
    return 7 if inst == "dma32" else B
ATOL = {"fp16": 2.0 ** -10, "bf16": 2.0 ** -7}     # one unit in the last place of the storage type at 1.0


def force_split_for(inst, Tk, HS):
    """What tf_sdpa_force_split must hold for a row to run the instance it names: 2 for the split rows; 1 (never split) where the per-shape rule
    would split an unsplit row -- d = 80 on a grid of fewer than 256 blocks with four key tiles or more; 0 (the per-shape choice) everywhere else."""
    if inst == "split":
        return 2
    return 1 if inst == "dma16" and HS == 80 and (Tk + 63) // 64 >= 4 else 0


def rows(instances=None):
    """(instance, B, NH, Tq, HS) for every row x head size of the table."""
    return [(inst, b, nh, tq, hs) for inst, b, nh, tq, sizes in INSTANCE_ROWS if instances is None or inst in instances for hs in sizes]


def round16(x, dtype):
    """x rounded to the storage type ("fp16" / "bf16", round-to-nearest-even), as float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "fp16":
        return x.astype(np.float16).astype(np.float32)
    assert dtype == "bf16", dtype
    u = x.view(np.uint32)
    return ((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)).view(np.float32)


def targets(B, NH, Tq, Tk):
    """t[b, h, i], the key query i of head (b, h) is aimed at.  Queries 0 .. 3 of EVERY head aim at keys 0, 63, 64 and Tk - 1 (both ends of the
    first tile seam and of the key range); the others continue one walk n -> (m n + 5) mod Tk across the heads, n = (i - 4) + (Tq - 4) (b NH + h),
    m the first of 13, 17, 19, 23 coprime to Tk -- so the heads together reach every key once B NH (Tq - 4) >= Tk.  Asserted here."""
    assert Tq >= 5 and Tk >= 2
    m = next(c for c in (13, 17, 19, 23) if math.gcd(c, Tk) == 1)
    hd = np.arange(B * NH, dtype=np.int64).reshape(B, NH, 1)
    n = np.arange(Tq - 4, dtype=np.int64).reshape(1, 1, -1) + (Tq - 4) * hd
    t = np.empty((B, NH, Tq), np.int64)
    t[..., :4] = np.minimum(np.array([0, 63, 64, Tk - 1]), Tk - 1)
    t[..., 4:] = (m * n + 5) % Tk
    assert np.array_equal(np.unique(t), np.arange(Tk)), "the targets of all heads together must cover every key"
    for key in (0, min(63, Tk - 1), min(64, Tk - 1), Tk - 1):
        assert (t == key).any(axis=-1).all(), f"every head must aim at key {key}"
    return t


def values(B, NH, Tk, HS):
    """v[b, h, j, c]: multiples of 1 / 128 in [-1, 1] (exact in float16 and bfloat16); with jj = j + 17 (b NH + h), even c: ((37 jj + 11 c) mod 257
    - 128) / 128, odd c: ((41 jj + 7 c) mod 251 - 125) / 128.  Two keys of a head, and the same key of two neighbouring heads, have different rows."""
    jj = (np.arange(Tk, dtype=np.int64).reshape(1, Tk, 1) + 17 * np.arange(B * NH, dtype=np.int64).reshape(-1, 1, 1))
    c = np.arange(HS, dtype=np.int64).reshape(1, 1, HS)
    v = np.where(c % 2 == 0, (37 * jj + 11 * c) % 257 - 128, (41 * jj + 7 * c) % 251 - 125).astype(np.float32) / 128.0
    assert np.abs(v).max() <= 1.0
    return v.reshape(B, NH, Tk, HS)


def keys(B, NH, Tk, HS, dtype, seed=7):
    """Seeded normal rows scaled to unit RMS, rounded to the storage type."""
    k = np.random.default_rng([seed, B, NH, Tk, HS]).standard_normal((B, NH, Tk, HS))
    return round16(k / np.sqrt((k * k).mean(axis=-1, keepdims=True)), dtype)


CAUSAL_MASS = 0.995      # what causal_keys asks of every query (the tests' precondition is 0.99)


@functools.lru_cache(maxsize=2)
def _causal_base(T, HS, dtype, seed=11):
    """One head's keys for the causal variant, drawn one after the other: key i + 1 is the first of a stream of seeded normal unit-RMS rows with
    which query i = g (k_i + k_{i+1}) / sqrt 2 (rounded) puts >= CAUSAL_MASS on key i among the keys 0 .. i it may see (the last key also serves
    the last query, g k_i).  Independent rows do not do: the two halves of the query leave a matching score of 48 / sqrt 2 nats with a spread of
    48 / sqrt(2 HS) around it, against the best of hundreds of competitors of spread 48 / sqrt HS -- below 72 dimensions some query of 330 loses
    half its mass (measured at HS = 32, 40, 56, 64).  The condition is on the inputs, so the inputs are drawn until it holds."""
    rng = np.random.default_rng([seed, T, HS])
    g = GAIN_NATS / math.sqrt(HS)

    def draw(n):
        c = rng.standard_normal((n, HS))
        return round16(c / np.sqrt((c * c).mean(axis=-1, keepdims=True)), dtype).astype(np.float64)

    def mass_on_last(q, ks, own=None):
        """probability each query q[n] puts on the last of the keys ks (own: a further, per-query last key instead)"""
        s = q @ ks.T / math.sqrt(HS)
        if own is not None:
            s = np.concatenate([s, (q * own).sum(axis=-1, keepdims=True) / math.sqrt(HS)], axis=1)
        p = np.exp(s - s.max(axis=-1, keepdims=True))
        return p[:, -1] / p.sum(axis=-1)

    k = np.empty((T, HS))
    k[0] = draw(1)[0]
    for i in range(T - 1):
        for _ in range(400):
            c = draw(256)
            ok = mass_on_last(round16((k[i] + c) * (g / math.sqrt(2.0)), dtype).astype(np.float64), k[:i + 1]) >= CAUSAL_MASS
            if i + 1 == T - 1:
                ok &= mass_on_last(round16(c * g, dtype).astype(np.float64), k[:T - 1], own=c) >= CAUSAL_MASS
            if ok.any():
                k[i + 1] = c[np.argmax(ok)]
                break
        else:
            raise AssertionError(f"no key {i + 1} of {T} at HS = {HS} keeps query {i} on its target")
    return k.astype(np.float32)


def causal_keys(B, NH, T, HS, dtype, seed=11):
    """Head (b, h)'s keys: _causal_base's with the dimensions permuted and sign-flipped by a seeded draw of the head's own -- every inner product
    inside a head, so every probability, is the base's, and a query aimed at another head's keys finds nothing."""
    base = _causal_base(T, HS, dtype)
    k = np.empty((B * NH, T, HS), np.float32)
    for hd in range(B * NH):
        rng = np.random.default_rng([seed, hd, HS])
        k[hd] = base[:, rng.permutation(HS)] * rng.choice(np.float32([-1.0, 1.0]), HS)
    return k.reshape(B, NH, T, HS)


@functools.lru_cache(maxsize=4)
def planted(B, NH, Tq, Tk, HS, dtype, causal=False):
    """q, k, v (float32 arrays holding values of the storage type, read-only), the targets, the float64 answer and each query's mass on its target.
    causal (Tq == Tk): q_i = g (k_i + k_{i+1}) / sqrt 2 (the last query: g k_i) -- under the mask the answer is v_i, losing the diagonal costs
    O(1) and admitting key i + 1 pulls the output halfway to v_{i+1}."""
    assert HS >= 32, "too few dimensions to tell hundreds of keys apart"
    g = GAIN_NATS / math.sqrt(HS)                     # x 1 / sqrt(HS) in the kernel x |k|^2 = HS: 48 nats
    v = values(B, NH, Tk, HS)
    if causal:
        assert Tq == Tk
        k = causal_keys(B, NH, Tk, HS, dtype)
        t = np.broadcast_to(np.arange(Tq, dtype=np.int64), (B, NH, Tq))
        q = np.concatenate([(k[:, :, :-1] + k[:, :, 1:]) * (g / math.sqrt(2.0)), k[:, :, -1:] * g], axis=2)
    else:
        k = keys(B, NH, Tk, HS, dtype)
        t = targets(B, NH, Tq, Tk)
        q = np.take_along_axis(k, t[..., None], axis=2) * g
    q = round16(q, dtype)
    ref, mass = ref64(q, k, v, causal=0 if causal else None, target=t)
    for a in (q, k, v, ref, mass):
        a.setflags(write=False)
    return q, k, v, t, ref, mass


def ref64(q, k, v, causal=None, target=None):
    """softmax(q k^T / sqrt(d)) v in float64, one batch at a time.  causal = c: query i sees keys j <= i + c (0 is the causal mask, +-1 its
    shifted mutants).  With target: also the probability each query puts on its target."""
    B, NH, Tq, HS = q.shape
    Tk = k.shape[2]
    out = np.empty((B, NH, Tq, v.shape[-1]), np.float64)
    mass = np.empty((B, NH, Tq), np.float64)
    hide = None if causal is None else np.arange(Tk)[None, :] > np.arange(Tq)[:, None] + causal
    for b in range(B):
        s = np.matmul(q[b].astype(np.float64), k[b].astype(np.float64).transpose(0, 2, 1)) / math.sqrt(HS)
        if hide is not None:
            s[:, hide] = -np.inf
        p = np.exp(s - s.max(axis=-1, keepdims=True))
        p /= p.sum(axis=-1, keepdims=True)
        out[b] = np.matmul(p, v[b].astype(np.float64))
        if target is not None:
            mass[b] = np.take_along_axis(p, target[b][..., None], axis=-1)[..., 0]
    return (out, mass) if target is not None else out


def packed_self(q, k, v):
    """(B, T, 3 NH HS): q | k | v side by side, heads inside each third -- the q|k|v projection of self-attention (attention/attention.py:121-123)."""
    tok = lambda a: a.transpose(0, 2, 1, 3).reshape(a.shape[0], a.shape[2], -1)
    return np.ascontiguousarray(np.concatenate([tok(q), tok(k), tok(v)], axis=-1))


def packed_cross(q, k, v):
    """(B, Tq, NH HS) queries and the (B, Tk, 2 NH HS) k | v buffer of cross-attention (attention/attention.py:129-139)."""
    tok = lambda a: a.transpose(0, 2, 1, 3).reshape(a.shape[0], a.shape[2], -1)
    return np.ascontiguousarray(tok(q)), np.ascontiguousarray(np.concatenate([tok(k), tok(v)], axis=-1))


def unmerge(o, NH):
    """(B, T, NH HS) merged heads -> (B, NH, T, HS)."""
    b, t, c = o.shape
    return o.reshape(b, t, NH, c // NH).transpose(0, 2, 1, 3)
