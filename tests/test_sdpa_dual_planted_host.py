"""The planted inputs of tests/aux/sdpa_dual_planted.py (host code, no GPU): for every case tests/test_gpu_sdpa_dual.py runs on them, the conditions
its tolerance rests on -- in float64 every query puts >= 0.99 of its mass on its text target AND on its image target, whatever gamma; the inputs are
values of the storage type; the value rows are multiples of 1 / 128 in [-1, 1] and no image row equals a text row of its head -- and that the inputs
tell a wrong kernel from a right one: each mutant of the float64 answer (one softmax over both key sets, the image term dropped, the image tile's
tail keys left unmasked, the neighbouring head's image keys and values, the scale applied to the text term) moves some output by more than 0.25."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import sdpa_dual_planted as D  # noqa: E402
import sdpa_planted as P  # noqa: E402

DTYPES = ("fp16", "bf16")
MIN_MASS, MIN_MOVE = 0.99, 0.25
SHAPES = sorted({r[1:] for r in D.ROWS})
MUTANT_SCALES = (0.6, 2.0)                 # (at s = 1 "the scale applied to the text term" is no mutant)


def test_the_table_is_the_dispatch_rows_at_the_dual_head_sizes():
    assert {r[0] for r in D.ROWS} == {"dma16", "dma32", "dma32_w8"}
    assert {r[4] for r in D.ROWS if r[0] != "dma32_w8"} == {40, 80, 160} and {r[4] for r in D.ROWS if r[0] == "dma32_w8"} == {40, 80}
    h = D.hadamard16()
    assert np.array_equal(h[:8] @ h[:8].T, 8 * np.eye(8)) and np.array_equal(h[8:], -h[:8])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,nh,tq,hs", SHAPES)
def test_planted_dual_inputs(b, nh, tq, hs, dtype):
    for tk, gamma, tk2 in itertools.product(P.KEY_COUNTS, D.GAMMAS, D.IMAGE_KEY_COUNTS):
        q, k, v, k2, v2, t, u = D.planted(b, nh, tq, tk, tk2, hs, dtype, gamma)
        for a in (q, k, v, k2, v2):
            assert np.array_equal(a, P.round16(a, dtype))                   # what the device array will hold
        assert not k[..., hs - 8:].any() and not k2[..., :hs - 8].any()       # disjoint dimensions
        assert np.allclose((k.astype(np.float64) ** 2).sum(-1), hs, rtol=2.0 ** -6) and np.allclose((k2.astype(np.float64) ** 2).sum(-1), hs, rtol=2.0 ** -6)
        assert np.array_equal(v2 * 128, np.round(v2 * 128)) and np.abs(v2).max() <= 1.0
        assert len({row.tobytes() for row in np.concatenate([v[0, 0], v2[0, 0]])}) == tk + tk2
        assert np.array_equal(np.unique(u), np.arange(tk2)) and (tk2 == 1 or (np.diff(u, axis=-1) != 0).all())
        (o1, m1), (o2, m2) = D.text_term(b, nh, tq, tk, hs, dtype), D.image_term(q, k2, v2, u)
        assert m1.min() >= MIN_MASS and m2.min() >= MIN_MASS, (tk, tk2, m1.min(), m2.min())
        want = np.take_along_axis(v, t[..., None], axis=2) + np.take_along_axis(v2, u[..., None], axis=2)
        assert np.abs(o1 + o2 - want).max() <= 2 * (1 - m1.min()) + 2 * (1 - m2.min()) + 1e-12
        # the two terms, computed apart (the text term once per shape), are the answer on the whole inputs
        whole, w1, w2, _ = D.answers(*(a[:1, :2] for a in (q, k, v, k2, v2)), 2.0, t[:1, :2], u[:1, :2])
        assert np.abs(whole - (o1[:1, :2] + 2.0 * o2[:1, :2])).max() <= 1e-12 and np.abs(w1 - m1[:1, :2]).max() <= 1e-12 and np.abs(w2 - m2[:1, :2]).max() <= 1e-12
        # mutants, on the first two heads alone: more heads add queries, they cannot lower the largest move
        k2t, v2t = D.image_tile(b, nh, tk, hs, dtype)
        assert np.array_equal(k2t[:, :, :tk2], k2) and np.array_equal(v2t[:, :, :tk2], v2)
        for s in MUTANT_SCALES:
            r1, _, _, mut = D.answers(*(a[:1, :2] for a in (q, k, v, k2, v2)), s, mutants=True, tile=(k2t[:1, :2], v2t[:1, :2]))
            assert np.abs(r1).max() <= 1 + s + 1e-9
            for what in D.MUTANTS:
                d = np.abs(r1 - mut[what]).max()
                assert d > MIN_MOVE, (tk, tk2, s, what, d)


def test_image_keys_number_sixteen():
    with pytest.raises(AssertionError):
        D.image_keys(1, 2, 17, 40, "fp16")
