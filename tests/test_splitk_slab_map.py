"""The group-major split-K slab layout on the host (tests/aux/splitk_slabs.py holds the kernels' address arithmetic): for every shape, tile and
group width of tests/test_gpu_splitk_slabs.py the stores of the GEMM epilogue are a bijection onto [0, M N) that agrees with the stated formula,
no store straddles a group or leaves its natural alignment, and the fused reducer -- 16 bytes per lane or a quad per lane -- loads every quad it
consumes from the address the epilogue wrote it to, into the thread that holds it under row-major slabs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import splitk_slabs as S  # noqa: E402

# the shapes of the GPU test on their own tiles, and on every other tile k_igemm has (a tile wider or taller than the problem included)
TILES = [(64, 64), (64, 128), (64, 160), (128, 64), (128, 128), (128, 160), (256, 128)]
CASES = [(s, s.bm, s.bn) for s in S.SHAPES] + [(s, bm, bn) for s in S.SHAPES for bm, bn in TILES if (bm, bn) != (s.bm, s.bn)]


@pytest.mark.parametrize("s,bm,bn", CASES, ids=lambda v: v.name.replace(" ", "_") if isinstance(v, S.Shape) else str(v))
def test_epilogue_stores_are_a_bijection(s, bm, bn):
    HoWo, M, N, cpg = s.H * s.W, s.N * s.H * s.W, s.Cout, s.Cout // s.G
    assert cpg % 4 == 0 and N % 8 == 0
    stores = S.epilogue_offsets(M, N, HoWo, s.G, bm, bn)
    hit = np.zeros(M * N, np.int32)
    for m, n, o, width in stores:
        assert 0 <= o and o + width <= M * N, (m, n, o)
        assert o % width == 0, ("alignment", m, n, o, width)                    # 16-byte stores of halves / two float4 on 16, 8-byte stores on 8
        assert n // cpg == (n + width - 1) // cpg, ("an item straddles a group", m, n, width)
        assert o == S.formula(m, n, N, HoWo, s.G), (m, n, o)
        assert (S.formula(m, n + np.arange(width), N, HoWo, s.G) == o + np.arange(width)).all()
        hit[o:o + width] += 1
    assert (hit == 1).all(), (int((hit == 0).sum()), int((hit > 1).sum()))
    assert {w for *_, w in stores} == ({8} if cpg % 8 == 0 else {4})


def test_the_shapes_are_the_cases_they_are_named_for():
    a, b, c, d = S.SHAPES
    assert a.H * a.W < a.bm == a.N * a.H * a.W                                   # one 128-row tile holds both images
    assert (b.Cout // b.G) % 8 == 4                                             # 4-wide items
    assert c.Cout % c.bn not in (0,) and c.Cout > c.bn                           # a last n-tile narrower than the tile
    assert [S.eff_splitk(9 * s.Cin, s.split) for s in S.SHAPES] == [4, 2, 5, 16]
    for s in S.SHAPES:
        CV, RPS = S.rga_geometry(s.H * s.W, s.Cout, s.G)
        assert (RPS * CV) % 2 == 0 and (s.H * s.W * CV) % 2 == 0                  # every one of them takes the 16-byte loads with fp16 slabs


@pytest.mark.parametrize("pairs", (False, True), ids=("quad per lane", "16 bytes per lane"))
@pytest.mark.parametrize("s", S.SHAPES + [S.Shape("eight full sweeps", 1, 24, 34, 64, 80, 2, 64, 128, 2), S.Shape("ragged last sweep", 1, 16, 24, 64, 40, 2, 64, 64, 2)],
                         ids=lambda s: s.name.replace(" ", "_"))
def test_reducer_reads_what_the_epilogue_wrote(s, pairs):
    HoWo, N, cpg = s.H * s.W, s.Cout, s.Cout // s.G
    got, loads16 = S.reducer_reads(s.N, N, HoWo, s.G, pairs)
    assert len(got) == s.N * HoWo * N // 4                                       # every quad of the output, once
    CV, RPS = S.rga_geometry(HoWo, N, s.G)
    for (m, n), (off, t) in got.items():
        assert off == S.formula(m, n, N, HoWo, s.G), (m, n, off)
        rl, v = divmod(t, CV)
        assert n % cpg == 4 * v and (m % HoWo) % RPS == rl                       # the thread that holds the quad under row-major slabs
    assert all(o % 8 == 0 for o in loads16)                                      # 8 halves = 16 bytes
    if s.name == "ragged last sweep":
        assert HoWo % RPS != 0 and HoWo > RPS
    if s.name == "eight full sweeps":
        assert RPS * S.RGA_MAXR == HoWo
