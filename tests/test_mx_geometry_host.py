"""The exact block-scaled e4m3 cases of tests/aux/mx_geometry.py (host code, no GPU), for every row tests/test_gpu_mx_geometry.py runs (the table is
imported from the aux module, so the two cannot drift apart):

  * the exactness condition holds on every row: every value the epilogue could round, and every split's partial sum, is a multiple of 2^-q below
    2^(11 - q) -- array_equal is the right comparison on the device;
  * the direct-definition reference and the addressing engine (one flat code offset and one flat scale offset per (output pixel, k)) agree on every
    row -- so a mutant is one slip away from the right answer, not a second implementation's disagreement;
  * every mutant that applies to a row changes at least one output of that row, and every mutant of the list is told from the right answer by at
    least one row (the mutant-by-row table is printed on failure);
  * predict_form is self-consistent, the refusals are what they say, and the table names every instance, count, geometry and edge it was written for.
pytest -s prints the number of rows and the instances covered."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import mx_geometry as G  # noqa: E402

ALL = G.ALL
IDS = [c.name for c in ALL]


def test_table_is_well_formed():
    assert len(set(IDS)) == len(IDS)
    for c in ALL:
        assert c.kind in ("conv", "linear") and c.family in G.BIT and c.nc in ("none", "cout", "padded") and c.slabs in (16, 32) and c.wscale in ("pow2", "ones"), c
        Ho, Wo, M, C, K = G.dims(c)
        assert c.C1 % 64 == 0 and c.C2 % 64 == 0 and c.C1 > 0 and min(Ho, Wo) >= 1 and (c.bm, c.bn) in G.TILES, c
        assert M <= 1024 and M * K <= 4e6 and M * K * c.Cout <= 800e6, (c.name, "a case is a launch of microseconds and a host reference of milliseconds")
    assert len(set(g.name for g in G.GEGLU)) == len(G.GEGLU)
    print(f"\n{len(G.CASES)} conv rows, {len(G.LINEARS)} linear rows, {len(G.GEGLU)} GEGLU shapes, {len(G.REFUSALS)} refusals")


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_exactness_and_engine(c):
    y = G.reference(c)
    Ho, Wo = G.dims(c)[:2]
    assert y.shape == (c.N, Ho, Wo, c.Cout)
    assert np.array_equal(G.gather(c), y), "the addressing engine without a slip is not the reference"
    assert G.exact(c)


def test_reference_equals_torch():
    """the float64 definition against torch's conv2d on the dequantised operand (exact: multiples of 1/2 far below 2^53)."""
    import torch
    import torch.nn.functional as F
    for c in G.CASES[::5] + G.LINEARS[::6]:
        p = G.inputs(c)
        Ho, Wo, M, C, K = G.dims(c)
        xd = G.dequant(p["x"], p["xs"])
        if c.C2:
            xd = np.concatenate([xd, G.dequant(p["x2"], p["x2s"])], axis=-1)
        w = torch.from_numpy(p["w"].reshape(c.Cout, c.R, c.R, C).astype(np.float64)).permute(0, 3, 1, 2)
        g = F.conv2d(torch.from_numpy(xd).permute(0, 3, 1, 2), w, None, stride=1, padding=c.pad).permute(0, 2, 3, 1).numpy()
        assert np.array_equal(G._stages(c, p, g)[-1], G.reference(c)), c.name


def test_every_mutant_is_killed():
    killed = collections.defaultdict(list)
    table = []
    for c in ALL:
        y = G.reference(c)
        row = {}
        for name in G.MUTANTS:
            if not G.applies(c, name):
                row[name] = "."
                continue
            wrong = G.gather(c, name)
            differs = wrong.shape == y.shape and not np.array_equal(wrong, y)
            row[name] = "K" if differs else "!"
            if differs:
                killed[name].append(c.name)
        table.append((c.name, row))
    text = "\n".join(f"{name:72s} " + " ".join(row[m] for m in G.MUTANTS) for name, row in table)
    legend = "columns: " + ", ".join(G.MUTANTS) + "  (K = told apart, ! = applies but changes nothing, . = does not apply)"
    assert not any("!" in row.values() for _, row in table), "a mutant that applies changes no output of a row\n" + legend + "\n" + text
    for name in G.MUTANTS:
        assert len(killed[name]) >= 1, (name, G.MUTANTS[name], "\n" + legend + "\n" + text)
    print("\n" + "\n".join(f"{name}: told apart by {len(rows)} rows, first {rows[0]}" for name, rows in killed.items()))


def test_predict_form_is_self_consistent():
    for c in ALL:
        f = G.predict_form(c)
        K = G.dims(c)[4]
        ranges = G.split_ranges(K, c.split)
        assert f.eff == len(ranges) <= c.split and (f.eff != c.split) == c.rounds, (c.name, f, "asks for a split the dispatcher rounds, or is marked so and does not")
        assert ranges[0][0] == 0 and ranges[-1][1] == K and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and all(a % 128 == 0 for a, _ in ranges)
        assert f.row[:3] == (c.bm, c.bn, c.split), c.name
        if c.family == "pp3":
            assert G.pp3_ok(c) and c.split == 1
        else:
            assert G.pp_ok(c)


def test_coverage():
    forms = {c.name: G.predict_form(c) for c in ALL}
    kernels = collections.Counter(f.kernel for f in forms.values())
    missing = G.required_instances() - set(kernels)
    assert not missing, sorted(missing)
    print(f"\n{len(kernels)} kernel instances named: " + ", ".join(f"{k} x{n}" for k, n in sorted(kernels.items())))
    pp = [c for c in G.CASES if c.family == "pp"]
    p3 = [c for c in G.CASES if c.family == "pp3"]
    # pp: every count on every tile that takes it, every geometry with half-tile slabs off and on, every output width, both image counts
    for tile in G.TILES:
        for Cs in G.COUNTS:
            if tile == (256, 160) and (Cs[0] % 128 or Cs[1] % 128):
                continue
            assert any((c.bm, c.bn) == tile and (c.C1, c.C2) == Cs for c in pp), (tile, Cs)
        assert {G.geo_of(c) for c in pp if (c.bm, c.bn) == tile} == set(G.GEO), tile
    for geo in G.GEO:
        assert {G.h2(c) for c in pp if G.geo_of(c) == geo} == {False, True}, geo
    assert {c.Cout for c in pp} == set(G.COUTS) and {c.N for c in pp} >= {2, 3}
    # M edges: a ragged last tile and tiles spanning two images under 192 rows, one image per tile under 256; bias_nc in such tiles; HoWo < bm without it
    assert any(c.bm == 192 and G.dims(c)[2] % 192 and G.straddles(c) and c.nc != "none" for c in pp)
    assert any(c.bm == 256 and G.dims(c)[0] * G.dims(c)[1] == 256 and c.nc != "none" for c in pp)
    assert any(G.dims(c)[0] * G.dims(c)[1] < c.bm and c.nc == "none" for c in pp)
    assert {"cout", "padded"} <= {c.nc for c in pp} and {"cout", "padded"} <= {c.nc for c in p3}
    assert any(G.dims(c)[4] == 576 for c in pp), "K = 4.5 tiles"
    # split: 2, rounded splits, both slab widths, through every epilogue operand
    sp = [c for c in ALL if c.split > 1]
    assert any(c.split == 2 and not c.rounds for c in sp) and sum(c.rounds for c in sp) >= 3 and {16, 32} <= {c.slabs for c in sp if not c.rounds}
    assert any(c.nc != "none" and c.res and c.bias for c in sp if c.kind == "conv")
    assert any(len({b - a for a, b in G.split_ranges(G.dims(c)[4], c.split)}) > 1 for c in sp)
    # pp3: every row length at both image heights, the counts of the issue, the two-source rows at every row length
    assert {(c.W, c.H) for c in p3} == {(24, 8), (24, 16), (48, 4), (48, 8), (96, 2), (96, 4)} and all(c.N == 2 for c in p3)
    for W in (24, 48, 96):
        assert {(c.C1, c.C2) for c in p3 if c.W == W} >= {(128, 0), (256, 0), (384, 0), (128, 128), (256, 128)}, W
    for W in (48, 96):
        assert {(c.C1, c.C2) for c in p3 if c.W == W} >= {(192, 0), (320, 0)}, W
    # linears: every M, K, N, every tile at both splits
    li = G.LINEARS
    assert {c.W for c in li} == {64, 300, 515} and {c.C1 for c in li} == {64, 192, 640} and {c.Cout for c in li} == {128, 136, 328}
    assert {(c.bm, c.bn, c.split) for c in li} == {(bm, bn, s) for bm, bn in G.TILES for s in (1, 2)}
    assert all(c.bias for c in li) and any(c.res for c in li)
    assert any(c.wscale == "ones" for c in ALL) and sum(c.wscale == "pow2" for c in ALL) > 0.75 * len(ALL)


def test_geglu_inputs_plant_both_signs_of_the_gate():
    for g in G.GEGLU:
        assert g.No % 32 == 0 and g.bn == 128 and g.K % 64 == 0
        y, gate = G.geglu_reference(g)
        assert y.shape == (g.M, g.No) and np.isfinite(y).all() and np.abs(y).max() < 2048
        assert (gate < -4).any() and (gate > 4).any() and (np.abs(gate) < 1).any() and np.mean(np.abs(gate) <= 6.5) > 0.8, g.name
        p = G.geglu_inputs(g)
        packed = G.pack_geglu_rows(p["w"], g.No)
        assert np.array_equal(packed[:16], p["w"][:16]) and np.array_equal(packed[16:32], p["w"][g.No:g.No + 16]) and np.array_equal(packed[32:48], p["w"][16:32])
    assert {g.No % 128 for g in G.GEGLU} == {0, 32, 96}


def test_refusals_are_what_they_say():
    whats = [r.what for r in G.REFUSALS]
    assert len(set(whats)) == len(whats) and all(r.rc in (G.E_ARG, G.E_UNSUPPORTED) for r in G.REFUSALS)
    for r in G.REFUSALS:
        if r.rc == G.E_UNSUPPORTED:
            assert not r.override and not (G.pp3_ok(r.case) if r.case.family == "pp3" else G.pp_ok(r.case)), r.what
    by = {r.what: r for r in G.REFUSALS}
    assert G.pp_ok(by["bias_nc with HoWo < bm"].case._replace(nc="none")) and G.pp_ok(by["256 x 160 off the 128 grid"].case._replace(bm=192))
    assert G.pp3_ok(by["pp3 on 24-pixel rows with a half slab"].case._replace(C1=256))
