"""The planted-key attention inputs of tests/aux/sdpa_planted.py (host code, no GPU): for every shape tests/test_gpu_sdpa_instances.py runs, the
conditions its tolerance rests on -- in float64 every query puts >= 0.99 of its mass on its target, the values are multiples of 1 / 128 in
[-1, 1], the targets reach every key and, in every head, keys 0, 63, 64 and Tk - 1 -- and that the inputs can tell a wrong kernel from a right
one: each mutant of the float64 reference (last key tile dropped, value rows rolled by one key, one head reading its neighbour's keys, the
causal mask shifted by one either way) moves some output by more than 0.25."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import sdpa_planted as P  # noqa: E402

DTYPES = ("fp16", "bf16")
MIN_MASS, MIN_MOVE = 0.99, 0.25


def _key_counts(tq):
    return P.KEY_COUNTS + (tq,)          # the row's Tq as well: the packed self-attention launch has Tk = Tq


SHAPES = sorted({r[1:] for r in P.rows()})                                 # (the split rows have the 16-query rows' shapes)
CAUSAL_SHAPES = sorted({(P.causal_batch(inst, b), nh, hs) for inst, b, nh, _, hs in P.rows() if inst != "split"})


def _moves(ref, mutant):
    return np.abs(ref - mutant).max()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,nh,tq,hs", SHAPES)
def test_planted_inputs(b, nh, tq, hs, dtype):
    for tk in _key_counts(tq):
        q, k, v, t, ref, mass = P.planted(b, nh, tq, tk, hs, dtype)
        assert mass.min() >= MIN_MASS, (tk, mass.min())
        for a in (q, k, v):
            assert np.array_equal(a, P.round16(a, dtype))                       # what the device array will hold
        assert np.array_equal(v * 128, np.round(v * 128)) and np.abs(v).max() <= 1.0 and np.abs(ref).max() <= 1.0 + 1e-12
        assert len({row.tobytes() for row in v[0, 0]}) == tk                    # rows of distinct keys are distinct
        for key in (0, 63, 64, tk - 1):
            assert (t == key).any(axis=-1).all()
        assert np.array_equal(np.unique(t), np.arange(tk))
        # the answer is (nearly) the target's value row -- and not exactly: the float64 softmax of the rounded inputs is the reference
        assert np.abs(ref - np.take_along_axis(v, t[..., None], axis=2)).max() <= 2 * (1 - mass.min()) + 1e-12
        # mutants, on the first batch entry alone: more heads add queries, they cannot lower the largest move
        q, k, v, ref = q[:1], k[:1], v[:1], ref[:1]
        keep = (tk + 63) // 64 * 64 - 64
        moved = {"last key tile dropped": _moves(ref, P.ref64(q, k[:, :, :keep], v[:, :, :keep])),
                 "value rows rolled by one key": _moves(ref, P.ref64(q, k, np.roll(v, 1, axis=2))),
                 "a head reads its neighbour's keys": _moves(ref, P.ref64(q, np.roll(k, 1, axis=1), v)),
                 "a head reads its neighbour's values": _moves(ref, P.ref64(q, k, np.roll(v, 1, axis=1)))}
        for what, d in moved.items():
            assert d > MIN_MOVE, (tk, what, d)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,nh,hs", CAUSAL_SHAPES)
def test_planted_causal_inputs(b, nh, hs, dtype):
    T = P.CAUSAL_T
    q, k, v, t, ref, mass = P.planted(b, nh, T, T, hs, dtype, True)
    assert mass.min() >= MIN_MASS, mass.min()
    for a in (q, k):
        assert np.array_equal(a, P.round16(a, dtype))
    assert np.allclose((k.astype(np.float64) ** 2).mean(axis=-1), 1.0, atol=2.0 ** -6)      # unit RMS up to the storage rounding
    assert np.abs(ref - v).max() <= 2 * (1 - mass.min())
    q, k, v, ref = q[:1], k[:1], v[:1], ref[:1]
    keep = (T + 63) // 64 * 64 - 64
    with np.errstate(invalid="ignore"):                                          # (query 0 of the second mutant sees no key at all)
        hidden = P.ref64(q, k, v, causal=-1)
    moved = {"mask admits key i + 1": _moves(ref, P.ref64(q, k, v, causal=1)),
             "mask hides the diagonal": _moves(ref[:, :, 1:], hidden[:, :, 1:]),
             "no mask": _moves(ref, P.ref64(q, k, v)),
             "last key tile dropped": _moves(ref, P.ref64(q, k[:, :, :keep], v[:, :, :keep], causal=0)),
             "a head reads its neighbour's keys": _moves(ref, P.ref64(q, np.roll(k, 1, axis=1), v, causal=0))}
    for what, d in moved.items():
        assert d > MIN_MOVE, (what, d)


def test_generator_rejects_targets_that_miss_a_key():
    with pytest.raises(AssertionError, match="cover every key"):
        P.targets(1, 1, 100, 330)          # one head of 100 queries cannot reach 330 keys
