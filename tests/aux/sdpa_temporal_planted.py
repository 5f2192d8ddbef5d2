"""Planted inputs for the temporal attention (tf_sdpa_temporal_16) and their float64 answer (host code, numpy only).

Tensors are (G, F, P, NH, HS): video, frame, pixel, head, channel -- the order the launch addresses them in.  Every key is ONE-HOT-LIKE: k'[f'] =
KEY_GAIN e_{d(f')}, d(f') = (f' + turn) mod HS with a rotation `turn` of every (video, pixel, head)'s own, and every query aims at one frame
t = target(g, f, p, h): q'[f] = query_gain(HS) e_{d(t)}.  The score of query f against key f' is then s = KEY_GAIN query_gain / sqrt HS (about 48
nats) where d(f') = d(t) and exactly 0 elsewhere, so the softmax weights
are known in closed form (weights()): with n frames sharing the target's dimension (n = 1 while F <= HS), each of them gets e^s / (n e^s + F - n)
and every other frame 1 / (n e^s + F - n).  The output is the mean of the value rows of those n frames up to < 1e-19: a wrong, missing or
mis-addressed frame, pixel, head or video moves it by O(1).  The value rows are multiples of 1 / 128 in [-1, 1], different for every (video, frame,
pixel, head).

With tables (pe=True) the same q', k', v' are split into what the tensors hold and what the fp32 tables add: q = q' - pe_q[f], k = k' - pe_k[f]
exactly (small integers), v = round16(v' - pe_v[f]).  The expected value is always the float64 softmax of what the kernel is given (ref64), never
the closed form itself; tests/test_sdpa_temporal_host.py ties the two together."""
import functools
import math

import numpy as np

from sdpa_planted import ATOL, round16  # noqa: F401  (the bound the key-tile kernels' planted cases are held to)

KEY_GAIN = 8.0
FRAMES = (1, 2, 8, 16, 24, 32)
HEAD_SIZES = (8, 40, 64, 80, 160)
# (P, NH, G): every pixel count (5: the ragged pixel tail), head count (3: a ragged head group, 8: two groups) and video count of the issue's sets,
# each with more than one partner
PNG = ((1, 1, 1), (5, 3, 3), (64, 8, 1), (5, 8, 1), (64, 1, 3), (1, 3, 1))


def query_gain(HS):
    """An integer (exact in both storage types, also after an integer table entry is taken off) with KEY_GAIN query_gain / sqrt HS ~ 48 nats."""
    return float(round(6.0 * math.sqrt(HS)))


def target(G, F, P, NH):
    """t[g, f, p, h]: the frame query f of (video g, pixel p, head h) aims at."""
    g, f, p, h = np.ogrid[:G, :F, :P, :NH]
    return (7 * f + 3 * p + 5 * h + 11 * g + 1) % F


def values(G, F, P, NH, HS):
    """v'[g, f, p, h, c]: multiples of 1 / 128 in [-1, 1]; with jj = f + 37 ((g P + p) NH + h), even c: ((37 jj + 11 c) mod 257 - 128) / 128, odd c:
    ((41 jj + 7 c) mod 251 - 125) / 128."""
    g, f, p, h, c = np.ogrid[:G, :F, :P, :NH, :HS]
    jj = f + 37 * ((g * P + p) * NH + h)
    v = np.where(c % 2 == 0, (37 * jj + 11 * c) % 257 - 128, (41 * jj + 7 * c) % 251 - 125).astype(np.float32) / 128.0
    assert np.abs(v).max() <= 1.0
    return np.ascontiguousarray(v)


def tables(F, NH, HS):
    """pe_q, pe_k (integers) and pe_v (multiples of 1 / 128 in [-1 / 2, 1 / 2]), fp32 of shape (F, NH HS), every row and head different.  pe_q and
    pe_k are integers in [-2, 2] except for one channel per (frame, head), which takes away 2 query_gain (2 KEY_GAIN): a launch that leaves the table
    out sees a query (a key) with a second, twice as strong direction, and its softmax lands on another frame."""
    f, c = np.ogrid[:F, :NH * HS]
    h, ch = c // HS, c % HS
    pe_q = ((3 * f + 5 * c) % 5 - 2 - 2 * query_gain(HS) * (ch == (3 * f + h) % HS)).astype(np.float32)
    pe_k = ((7 * f + 3 * c + 1) % 5 - 2 - 2 * KEY_GAIN * (ch == (5 * f + h + 1) % HS)).astype(np.float32)
    pe_v = (((11 * (f % 8) + 13 * c) % 129 - 64) / 128.0).astype(np.float32)      # (f mod 8: the frames a query of HS = 8 averages share their row)
    return pe_q, pe_k, pe_v


def with_tables(x, pe):
    """x (G, F, P, NH, HS) + pe (F, NH HS) broadcast over video and pixel, in float64."""
    G, F, P, NH, HS = x.shape
    return x.astype(np.float64) + (0.0 if pe is None else pe.astype(np.float64).reshape(1, F, 1, NH, HS))


def weights(G, F, P, NH, HS):
    """The closed form: w[g, p, h, f, f'], the softmax weight query f puts on frame f'."""
    s = KEY_GAIN * query_gain(HS) / math.sqrt(HS)
    t = target(G, F, P, NH).transpose(0, 2, 3, 1)                             # (G, P, NH, F)
    hit = (np.arange(F) % HS)[None, None, None, None, :] == (t % HS)[..., None]
    n = hit.sum(axis=-1, keepdims=True)
    # e^s / (n e^s + F - n) = 1 / (n + (F - n) e^-s)
    return np.where(hit, 1.0 / (n + (F - n) * math.exp(-s)), math.exp(-s) / (n + (F - n) * math.exp(-s)))


def ref64(q, k, v, pe_q=None, pe_k=None, pe_v=None, weights_too=False):
    """softmax_f'((q + pe_q)(k + pe_k)^T / sqrt HS)(v + pe_v) in float64 over the frames of every (video, pixel, head): (G, F, P, NH, HS)."""
    HS = q.shape[-1]
    qq, kk, vv = (with_tables(x, pe).transpose(0, 2, 3, 1, 4) for x, pe in ((q, pe_q), (k, pe_k), (v, pe_v)))      # (G, P, NH, F, HS)
    s = np.matmul(qq, kk.transpose(0, 1, 2, 4, 3)) / math.sqrt(HS)
    w = np.exp(s - s.max(axis=-1, keepdims=True))
    w /= w.sum(axis=-1, keepdims=True)
    out = np.ascontiguousarray(np.matmul(w, vv).transpose(0, 3, 1, 2, 4))
    return (out, w) if weights_too else out


@functools.lru_cache(maxsize=4)
def planted(G, F, P, NH, HS, dtype, pe=False):
    """q, k, v (float32 arrays holding values of the storage type), the three tables (None without pe) and the float64 answer, all read-only."""
    t = target(G, F, P, NH)
    c = np.arange(HS)
    g_, f_, p_, h_ = np.ogrid[:G, :F, :P, :NH]
    turn = 3 * p_ + 5 * h_ + 7 * g_                   # the dimensions of every (video, pixel, head) are rotated by an amount of its own
    q = (query_gain(HS) * (((t + turn) % HS)[..., None] == c)).astype(np.float32)
    k = (KEY_GAIN * (((f_ + turn) % HS)[..., None] == c)).astype(np.float32)
    v = values(G, F, P, NH, HS)
    tabs = (None, None, None)
    if pe:
        tabs = tables(F, NH, HS)
        sub = lambda x, tb: x - tb.reshape(1, F, 1, NH, HS)
        q, k, v = sub(q, tabs[0]), sub(k, tabs[1]), round16(sub(v, tabs[2]), dtype)
    for a in (q, k):
        assert np.array_equal(a, round16(a, dtype)), "planted q / k must be values of the storage type"
    ref = ref64(q, k, v, *tabs)
    for a in (q, k, v, ref) + tuple(x for x in tabs if x is not None):
        a.setflags(write=False)
    return (q, k, v) + tabs + (ref,)


def packed(q, k, v):
    """(G F, P, 3 C): q | k | v side by side, heads inside each third -- where the motion module's fused q|k|v projection leaves them."""
    G, F, P, NH, HS = q.shape
    return np.ascontiguousarray(np.concatenate([a.reshape(G * F, P, NH * HS) for a in (q, k, v)], axis=-1))
