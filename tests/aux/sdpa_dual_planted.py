"""Planted inputs for the decoupled (dual) attention launch, o = softmax(q k^T / sqrt d) v + s softmax(q k2^T / sqrt d) v2, and their float64 answer
(host code, numpy only).  Built on sdpa_planted: every query is aimed at ONE key of each set, so each softmax puts all but < 1e-6 of its mass on its
target and the answer is v[t] + s v2[u], rows of multiples of 1 / 128 -- a wrong, missing, mis-addressed or mis-normalised key of either set moves
the output by O(1).

  text keys    seeded normal in the first HS - 8 dimensions, zero in the last 8, scaled to |k|^2 = HS;
  image keys   the 16 signed rows of the 8 x 8 Hadamard matrix in the last 8 dimensions, zero in front, scaled to |k|^2 = HS; key u of head hd
               holds pattern (u + 5 hd) mod 16, so neighbouring heads hold different rows (Tk2 <= 16);
  queries      q = round16(g k[t] + gamma g k2[u]), g = 48 / sqrt HS: 48 nats on the text target, 48 gamma on the image target, and -- the two key
               sets live in disjoint dimensions -- nothing of one set's query half reaches the other set's scores.  t = sdpa_planted.targets, u walks
               all image keys, u = (i + hd) mod Tk2;
  gamma        0.5, 1, 1.5: the image maximum lies below, at and above the text maximum.  A kernel that lets one set's maximum rescale the other
               set's accumulator or row sum is O(1) wrong at 0.5 or at 1.5;
  values       v = sdpa_planted.values of Tk rows, v2 = the Tk2 rows that follow them in the same sequence (no row of v2 equals a row of v).

The expected value is float64 on the ROUNDED inputs.  tests/test_sdpa_dual_planted_host.py asserts what this rests on for every case of the table:
target mass >= 0.99 in both sets, and that each mutant of the answer (MUTANTS) moves some output by more than 0.25."""
import functools
import math

import numpy as np
import sdpa_planted as P

GAMMAS = (0.5, 1.0, 1.5)
SCALES = (0.6, 1.0, 2.0)
IMAGE_KEY_COUNTS = (1, 4, 16)                 # planted image keys number 16; 64 runs on seeded-normal inputs
HEAD_SIZES = (40, 80, 160)
ROWS = [r for r in P.rows(("dma16", "dma32", "dma32_w8")) if r[4] in HEAD_SIZES]      # (instance, B, NH, Tq, HS)
MUTANTS = ("joint_softmax", "image_dropped", "tail_unmasked", "neighbour_head", "scale_on_text")
HEAD_STEP = 5                                 # pattern offset between neighbouring heads (odd: sixteen heads walk all sixteen patterns)


@functools.lru_cache(maxsize=4)
def _values(B, NH, T, HS):
    """sdpa_planted.values, kept (read-only): the cases of one shape ask for the same rows again and again."""
    v = P.values(B, NH, T, HS)
    v.setflags(write=False)
    return v


def hadamard16():
    """The 16 signed rows of the 8 x 8 Sylvester Hadamard matrix: rows 0 .. 7, then their negatives."""
    h = np.array([[1.0]])
    for _ in range(3):
        h = np.block([[h, h], [h, -h]])
    return np.concatenate([h, -h], axis=0)


@functools.lru_cache(maxsize=2)
def text_keys(B, NH, Tk, HS, dtype, seed=13):
    k = np.zeros((B, NH, Tk, HS))
    r = np.random.default_rng([seed, B, NH, Tk, HS]).standard_normal((B, NH, Tk, HS - 8))
    k[..., :HS - 8] = r * np.sqrt(HS / (r * r).sum(axis=-1, keepdims=True))
    k = P.round16(k, dtype)
    k.setflags(write=False)
    return k


def image_keys(B, NH, Tk2, HS, dtype):
    """Tk2 <= 16 distinct patterns per head; image_tile() continues the sequence to the 64 rows of a key tile (pattern of row u + 16 = pattern of row u)."""
    assert 1 <= Tk2 <= 16
    return _image_rows(B, NH, Tk2, HS, dtype)


def _image_rows(B, NH, Tk2, HS, dtype):
    pat = (np.arange(Tk2).reshape(1, Tk2) + HEAD_STEP * np.arange(B * NH).reshape(-1, 1)) % 16
    k2 = np.zeros((B * NH, Tk2, HS))
    k2[..., HS - 8:] = hadamard16()[pat] * math.sqrt(HS / 8.0)
    return P.round16(k2.reshape(B, NH, Tk2, HS), dtype)


def image_targets(B, NH, Tq, Tk2):
    return ((np.arange(Tq).reshape(1, Tq) + np.arange(B * NH).reshape(-1, 1)) % Tk2).reshape(B, NH, Tq)


def _softmax(s):
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    return p / p.sum(axis=-1, keepdims=True)


def image_tile(B, NH, Tk, HS, dtype):
    """(k2, v2) of 64 rows per head: the buffers the tests hand to the kernel, which is told to read Tk2 <= 16 of them.  The rows behind Tk2 are what a
    kernel that leaves the tile's tail unmasked attends to: rows 16, 32 and 48 + u repeat the pattern of row u under other value rows."""
    return _image_rows(B, NH, 64, HS, dtype), np.ascontiguousarray(_values(B, NH, Tk + 64, HS)[:, :, Tk:])


def answers(q, k, v, k2, v2, s, t=None, u=None, mutants=False, tile=None):
    """float64 o = softmax(q k^T / sqrt d) v + s softmax(q k2^T / sqrt d) v2, one batch at a time.  With t / u: also each query's mass on its text /
    image target.  mutants: also a dict of the wrong answers named in MUTANTS (tile: image_tile's 64-row buffers, for "tail_unmasked")."""
    B, NH, Tq, HS = q.shape
    out = np.empty((B, NH, Tq, HS))
    m1, m2 = np.empty((B, NH, Tq)), np.empty((B, NH, Tq))
    mut = {n: np.empty_like(out) for n in MUTANTS} if mutants else None
    if mutants:
        k2t, v2t = tile
        k2n, v2n = np.roll(k2.reshape(B * NH, -1, HS), 1, axis=0).reshape(k2.shape), np.roll(v2.reshape(B * NH, -1, HS), 1, axis=0).reshape(v2.shape)
    f = lambda a: a.astype(np.float64)
    for b in range(B):
        qb = f(q[b])
        s1 = np.matmul(qb, f(k[b]).transpose(0, 2, 1)) / math.sqrt(HS)
        s2 = np.matmul(qb, f(k2[b]).transpose(0, 2, 1)) / math.sqrt(HS)
        p1, p2 = _softmax(s1), _softmax(s2)
        o1, o2 = np.matmul(p1, f(v[b])), np.matmul(p2, f(v2[b]))
        out[b] = o1 + s * o2
        if t is not None:
            m1[b] = np.take_along_axis(p1, t[b][..., None], axis=-1)[..., 0]
            m2[b] = np.take_along_axis(p2, u[b][..., None], axis=-1)[..., 0]
        if mutants:
            pj = _softmax(np.concatenate([s1, s2], axis=-1))
            mut["joint_softmax"][b] = np.matmul(pj[..., :s1.shape[-1]], f(v[b])) + s * np.matmul(pj[..., s1.shape[-1]:], f(v2[b]))
            mut["image_dropped"][b] = o1
            mut["tail_unmasked"][b] = o1 + s * np.matmul(_softmax(np.matmul(qb, f(k2t[b]).transpose(0, 2, 1)) / math.sqrt(HS)), f(v2t[b]))
            mut["neighbour_head"][b] = o1 + s * np.matmul(_softmax(np.matmul(qb, f(k2n[b]).transpose(0, 2, 1)) / math.sqrt(HS)), f(v2n[b]))
            mut["scale_on_text"][b] = s * o1 + o2
    return out, m1, m2, mut


@functools.lru_cache(maxsize=4)
def text_term(B, NH, Tq, Tk, HS, dtype):
    """softmax(q k^T / sqrt d) v in float64 and the mass on the text targets, computed ONCE for all gamma and Tk2 of a shape: the text keys are zero in
    the last 8 dimensions, so the text scores see only q's first HS - 8 columns, round16(g k[t]) whatever gamma and u are (the rounding is per
    element).  tests/test_sdpa_dual_planted_host.py checks the sum of the two terms against `answers` on whole inputs."""
    g = P.GAIN_NATS / math.sqrt(HS)
    k, t = text_keys(B, NH, Tk, HS, dtype), P.targets(B, NH, Tq, Tk)
    o1, m1 = P.ref64(P.round16(g * np.take_along_axis(k, t[..., None], axis=2), dtype), k, _values(B, NH, Tk + 64, HS)[:, :, :Tk], target=t)
    o1.setflags(write=False)
    m1.setflags(write=False)
    return o1, m1


def image_term(q, k2, v2, u):
    """softmax(q k2^T / sqrt d) v2 in float64 and the mass on the image targets (at most 16 keys: cheap)."""
    return P.ref64(q, k2, v2, target=u)


@functools.lru_cache(maxsize=2)
def planted(B, NH, Tq, Tk, Tk2, HS, dtype, gamma):
    """q, k, v, k2, v2 (float32 arrays holding values of the storage type, read-only), the text and image targets."""
    g = P.GAIN_NATS / math.sqrt(HS)
    k, k2 = text_keys(B, NH, Tk, HS, dtype), image_keys(B, NH, Tk2, HS, dtype)
    vv = _values(B, NH, Tk + 64, HS)                  # (row j of a head does not depend on the row count: v2 = image_tile's first Tk2 rows)
    v, v2 = np.ascontiguousarray(vv[:, :, :Tk]), np.ascontiguousarray(vv[:, :, Tk:Tk + Tk2])
    t, u = P.targets(B, NH, Tq, Tk), image_targets(B, NH, Tq, Tk2)
    q = P.round16(g * np.take_along_axis(k, t[..., None], axis=2) + gamma * g * np.take_along_axis(k2, u[..., None], axis=2), dtype)
    for a in (q, k, v, k2, v2, t, u):
        a.setflags(write=False)
    return q, k, v, k2, v2, t, u
