"""The exact conv-addressing cases of tests/aux/conv_geometry.py (host code, no GPU), for every row tests/test_gpu_conv_geometry.py runs (the table is
imported from the aux module, so the two cannot drift apart):

  * exact_cap holds for every row and storage type: array_equal is the right comparison on the device;
  * the direct-definition reference equals torch's conv2d wherever torch can express the case, and the addressing engine (gather) equals the reference
    on every row -- so a mutant is one slip away from the right answer, not a second implementation's disagreement;
  * every mutant that applies to a row changes at least one output of that row, and every mutant is killed by at least three rows: the {-1, 0, 1}
    inputs at these seeds tell a wrong kernel from a right one;
  * predict_form is self-consistent: no row asks for a split the dispatcher rounds unless it is marked as doing so;
  * coverage: every kernel instance, geometry, edge and mode the table was written for is named by at least one row -- shrinking the table fails here.
pytest -s prints the number of rows, the instances covered and the rows marked fp16-only."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import conv_geometry as G  # noqa: E402

CASES = G.CASES
IDS = [c.name for c in CASES]


def test_table_is_well_formed():
    assert len(set(IDS)) == len(IDS)
    for c in CASES:
        assert c.family in G.FAMILY_BIT and set(c.dtypes) <= set(G.BOTH) and c.nc in G.NC_MODES and c.slabs in (16, 32), c
        assert G.geo_of(c) in G.GEO and min(G.out_hw(c)) >= 1, c
        assert all(v % (64 if c.family == "igemm8" else 8) == 0 for v in (c.C1, c.C2, c.C3, c.C4)) and c.C1 > 0 and (c.C3 > 0 or c.C4 == 0), c
        assert not (c.C3 and c.ups), c
        M, K = G.dims(c)[2], G.dims(c)[5]
        assert M * K * c.Cout <= 200e6 and M * K <= 2e6, (c.name, "a case is a launch of microseconds and a host reference of milliseconds")
    # the table may mark at most the rows exact_cap excludes in bfloat16 as fp16-only
    for name in G.FP16_ONLY:
        c = CASES[IDS.index(name)]
        assert np.abs(G.reference(c)).max() > G.CAP["bf16"] or G.dims(c)[5] > 2048, (name, "marked fp16-only without need")
    print(f"\n{len(CASES)} rows ({sum(len(c.dtypes) for c in CASES)} launches), {len(G.REFUSALS)} refusals; rows of the 16-bit families marked fp16-only: {len(G.FP16_ONLY)} {list(G.FP16_ONLY)}")


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_exact_cap_and_engine(c):
    for dtype in c.dtypes:
        assert G.exact_cap(c, dtype)
    y = G.reference(c)
    assert y.shape == (c.N, *G.out_hw(c), c.Cout)
    assert np.array_equal(G.gather(c), y), "the addressing engine without a slip is not the reference"


def _torch_conv(c):
    """the case through torch.nn.functional.conv2d in float64: the taps as one conv2d, the extra segment as a strided 1x1 conv2d of x3 | x4."""
    import torch
    import torch.nn.functional as F
    p = G.inputs(c)
    Ho, Wo, M, C, Kc, K = G.dims(c)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    x = t(np.concatenate([p["x"]] + ([p["x2"]] if c.C2 else []), axis=-1)).permute(0, 3, 1, 2)
    if c.ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    w = t(p["w"][:, :Kc].reshape(c.Cout, c.R, c.S, C)).permute(0, 3, 1, 2)
    y = F.conv2d(x, w, None, stride=c.stride, padding=c.pad)
    if c.C3:
        e = t(np.concatenate([p["x3"]] + ([p["x4"]] if c.C4 else []), axis=-1)).permute(0, 3, 1, 2)
        e = F.pad(e, (0, max((Wo - 1) * c.stride + 1 - c.W, 0), 0, max((Ho - 1) * c.stride + 1 - c.H, 0)))     # sample points beyond the image: zero
        y = y + F.conv2d(e, t(p["w"][:, Kc:]).reshape(c.Cout, c.C3 + c.C4, 1, 1), None, stride=c.stride)[:, :, :Ho, :Wo]
    return G._epilogue(c, p, y.permute(0, 2, 3, 1).numpy())


def test_reference_equals_torch():
    done = 0
    for c in CASES:
        y = _torch_conv(c)
        done += 1
        assert np.array_equal(y, np.asarray(G.reference(c), np.float64)), c.name
    assert done == len(CASES)
    print(f"\nreference == torch conv2d on {done} of {len(CASES)} rows")


def test_every_mutant_is_killed():
    killed = collections.defaultdict(list)
    for c in CASES:
        y = G.reference(c)
        for name, wrong in G.mutants(c).items():
            assert wrong.shape == y.shape and not np.array_equal(wrong, y), (c.name, name, "a mutant that applies changes no output of this row")
            killed[name].append(c.name)
    for name in G.MUTANTS:
        assert len(killed[name]) >= 3, (name, G.MUTANTS[name], killed[name])
    print("\n" + "\n".join(f"{name}: killed by {len(rows)} rows, first {rows[0]}" for name, rows in killed.items()))


def test_predict_form_is_self_consistent():
    for c in CASES:
        f = G.predict_form(c)
        Ho, Wo, M, C, Kc, K = G.dims(c)
        assert f.row[:3] == (c.bm, c.bn, c.split) and f.eff == len(G.split_ranges(K, c.split)) <= c.split, c.name
        assert (f.eff != c.split) == c.rounds, (c.name, "asks for a split the dispatcher rounds" if f.eff != c.split else "marked as rounding but does not")
        ranges = G.split_ranges(K, c.split)
        assert ranges[0][0] == 0 and ranges[-1][1] == K and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and all(a % 64 == 0 for a, _ in ranges)
        if c.family == "igemm":
            assert f.ring in (G.V_RING, G.V_WIDE, G.V_ALL8) and (f.ring == f.row[3] or f.ring == G.V_RING), c.name
        if c.family == "patch":
            assert (f.pt_ns >= 3) == bool(f.patch) and ("patch" in f.kernel) == bool(f.patch), c.name
        if c.family == "pp":
            assert c.nc == "none" or Ho * Wo >= c.bm, c.name
    assert sum(c.rounds for c in CASES) >= 1


def _crosses_mid_row(c):
    """a tile that starts in the middle of an output row of one image and ends in the next image."""
    Ho, Wo, M = G.dims(c)[:3]
    m0 = np.arange(0, M, c.bm)
    crosses = m0 // (Ho * Wo) != (np.minimum(m0 + c.bm, M) - 1) // (Ho * Wo)
    return bool(np.any(crosses & (m0 % (Ho * Wo) % Wo != 0)))


def test_coverage():
    forms = {c.name: G.predict_form(c) for c in CASES}
    kernels = collections.Counter(f.kernel for f in forms.values())
    missing = G.required_instances() - set(kernels)
    assert not missing, sorted(missing)
    print(f"\n{len(kernels)} kernel instances named: " + ", ".join(f"{k} x{n}" for k, n in sorted(kernels.items())))
    ig = [c for c in CASES if c.family == "igemm"]
    # every geometry on a 64-grid count and on a GENERIC count of k_igemm; the GENERIC counts and the grid counts themselves
    for geo, shape in G.GEOMETRIES:
        for gen in (False, True):
            assert any(G.geo_of(c) == geo and (c.N, c.H, c.W) == shape and G.generic(c) == gen for c in ig), (geo, shape, gen)
    for Cs in G.GRID_COUNTS + G.GENERIC_COUNTS:
        assert any((c.C1, c.C2) == Cs for c in ig), Cs
    assert all(any(c.dbg & bit for c in ig) for bit in G.ORDER_BITS)
    # M edges
    assert any(c.N == 5 and c.bm == 256 and G.dims(c)[0] * G.dims(c)[1] < 256 for c in ig)
    assert any(c.N == 3 and G.dims(c)[0] * G.dims(c)[1] < c.bm and G._straddles(c) for c in ig)
    assert any(c.N == 3 and (c.H, c.W) == (9, 7) and _crosses_mid_row(c) for c in ig), "no tile of the N = 3, 9 x 7 rows crosses an image boundary from mid-row"
    assert any(G.dims(c)[2] % c.bm != 0 and G.dims(c)[2] > c.bm for c in ig) and any(G.dims(c)[2] < c.bm for c in ig)
    # N edges and bias_nc modes
    for family in ("igemm",):
        assert {4, 6, 72, 136, 200} <= {c.Cout for c in CASES if c.family == family}
    assert all(any(c.nc == m and c.family == f for c in CASES) for m in G.NC_MODES for f in ("igemm", "patch", "pp", "igemm8"))
    assert any(c.nc == "padded" and c.Cout % 8 == 0 and G.nc_stride(c) % 8 != 0 for c in CASES)
    # split-K: 2 and 3, ragged, cuts inside the extra segment and inside a tap on GENERIC counts, both slab types, one rounding row
    sp = [c for c in CASES if c.split > 1 and not c.rounds]
    cuts = lambda c: [a for a, _ in G.split_ranges(G.dims(c)[5], c.split)][1:]
    assert {2, 3} <= {c.split for c in sp} and {16, 32} <= {c.slabs for c in sp}
    assert any(len({b - a for a, b in G.split_ranges(G.dims(c)[5], c.split)}) > 1 for c in sp)
    assert any(c.C3 and any(k > G.dims(c)[4] for k in cuts(c)) for c in sp if c.family == "igemm")
    assert any(c.C3 and G.generic(c) and any(k > G.dims(c)[4] for k in cuts(c)) for c in sp if c.family == "igemm")
    assert any(G.generic(c) and any(k < G.dims(c)[4] and k % G.dims(c)[3] for k in cuts(c)) for c in sp if c.family == "igemm")
    assert all(any(c.family == f for c in sp) for f in ("igemm", "patch", "pp", "igemm8"))
    # the extra sources: on and off the 64 grid, stride 1 and 2, with and without the residual
    ex = [c for c in CASES if c.C3]
    for gen in (False, True):
        for stride in (1, 2):
            for res in (False, True):
                assert any(G.generic(c) == gen and c.stride == stride and c.res == res for c in ex), (gen, stride, res)
    assert {(64, 64), (24, 8), (72, 0)} <= {(c.C3, c.C4) for c in ex}
    # k_igemm_patch: every ring depth patch_setup can give here, W = 8 .. 64 with H != W, and the stride-2 row it does not take
    pa = [c for c in CASES if c.family == "patch"]
    assert {3, 4, 5} <= {forms[c.name].pt_ns for c in pa} and {8, 16, 32, 64} <= {c.W for c in pa if forms[c.name].patch and c.H != c.W}
    assert any(c.stride == 2 and not forms[c.name].patch for c in pa) and {1, 2, 3} <= {c.split for c in pa if forms[c.name].patch}
    assert any(c.C2 for c in pa) and any(c.C3 for c in pa)
    # k_igemm_pp and k_igemm8: the geometries the issue lists
    pp = {G.geo_of(c) for c in CASES if c.family == "pp"}
    assert {"3x3s1p1", "3x3s2p1", "3x3up", "1x1s1p0", "1x3s1p1", "3x1s1p1"} <= pp
    assert any(c.C2 for c in CASES if c.family == "pp") and any(c.C3 for c in CASES if c.family == "pp")
    beyond = [forms[c.name].kernel for c in CASES if c.family == "pp" and c.C3 and c.stride == 1 and (G.dims(c)[0] > c.H or G.dims(c)[1] > c.W)]
    assert any("NP1" in k for k in beyond) and any("NP2" in k for k in beyond) and all("gather" in k for k in beyond), beyond
    f8 = [c for c in CASES if c.family == "igemm8"]
    assert {"3x3s1p1", "3x3s2p1", "3x3up", "1x1s1p0"} <= {G.geo_of(c) for c in f8} and any((c.C1, c.C2) == (64, 64) for c in f8)
    assert sum(c.wscale == "pow2" for c in f8) == 1
    # every 16-bit row runs in both types
    assert all(c.dtypes == G.BOTH or c.name in G.FP16_ONLY for c in CASES if c.family != "igemm8")


def test_refusals_are_what_they_say():
    whats = [r.what for r in G.REFUSALS]
    assert len(set(whats)) == len(whats) and all(r.rc in (G.E_ARG, G.E_UNSUPPORTED) for r in G.REFUSALS)
    by = {r.what: r for r in G.REFUSALS}
    assert G.generic(by["ping-pong on GENERIC counts"].case) and not G.pp_ok(by["ping-pong on GENERIC counts"].case)
    c = by["ping-pong with bias_nc at HoWo < bm"].case
    assert not G.pp_ok(c) and G.pp_ok(c._replace(nc="none"))
    c = by["bias_nc_stride off the 4 grid"]
    assert c.case.Cout % 4 == 0 and c.override["nc_stride"] % 4 != 0
    assert by["C4 without C3"].case.C3 == 0 and by["C4 without C3"].case.C4 > 0
