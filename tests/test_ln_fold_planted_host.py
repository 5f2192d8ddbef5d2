"""The planted LayerNorm-fold problems of tests/aux/ln_fold_planted.py (host code, no GPU), for every launch tests/test_gpu_ln_fold_planted.py makes
(the case tables are imported from the aux module, so the two cannot drift apart):

  * the rows equal their own storage rounding, no two rows at most 512 apart share their planted (mu, sigma), the rows keep them, and the column
    sums of the folded weights differ between neighbouring quads and between columns 16 and 64 apart;
  * the numpy emulation of the kernels' fp32 arithmetic stays within A / 2 of the float64 reference on every case (ratios printed: pytest -s), the
    constants are the smallest integers that do, and the R-limit table is what cancellation_limit() finds;
  * every mutant of the float64 reference that applies to a case exceeds tol by at least 8 times on at least one element of every row tile it
    affects (a mutant that does not apply to a case is printed in the table), and the GPU test's checker, fed a mutant as "device output", fails
    and names it;
  * every LayerNorm-folded row of the shipped tuning table has its (variant, tile, activation, tile order) among the cases.
The two chunked-walk shapes (27600 and 55200 rows) are examined on their first four, their middle and their last two row tiles."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import ln_fold_planted as L  # noqa: E402

ALL = L.CASES + L.CHUNK_CASES
WORST = {}


def _unique(cases, key):
    seen, out = set(), []
    for c in cases:
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    return out


DATA = _unique(ALL, L.data_key)                                   # one case per distinct problem (the tile and family do not change the numbers)
TILED = _unique(ALL, lambda c: L.data_key(c) + (c.bm,))           # ... and per row-tile height (what "every row tile" means)


def _tiles(c):
    """row tiles examined: all of them, or for the chunked-walk shapes the first four, the middle one and the last two."""
    bm = c.bm or 64
    nt = -(-c.M // bm)
    pick = range(nt) if nt <= 16 else sorted({0, 1, 2, 3, nt // 2, nt - 2, nt - 1})
    return bm, [slice(t * bm, min(c.M, (t + 1) * bm)) for t in pick]


def test_case_tables():
    ids = [L.case_id(c) for c in ALL]
    assert len(set(ids)) == len(ids)
    for c in ALL:
        assert c.K % 64 == 0 and L.packed_width(c) % (32 if c.act else 4) == 0, c
        if c.bm:
            assert c.M == 2 * c.bm + 37 or c.family == "ar" or c in L.CHUNK_CASES, c      # two whole row tiles and a ragged third
            assert L.predict_form(c)[3] == L.VARIANT_OF_BIT[L.family_bit(c)]
        if c.family == "ring":
            assert L.ring_form(c.bm, c.bn, L.family_bit(c)) == L.predict_form(c)[3], c
        if c.family in ("c4", "c8", "ar"):
            assert L.packed_width(c) % (64 if c.act else 8) == 0 and not (c.family == "ar" and (c.res or c.K not in (256, 320))), c
    # K tiles against ring slots on the long-K tiles: fewer, as many, more
    for bit, (bm, bn) in L.LONG_K_TILE.items():
        ks = sorted(c.K // 64 for c in L.CASES if c.family == "ring" and (c.bm, c.bn) == (bm, bn) and L.family_bit(c) == bit)
        assert ks == [1, 3, 5, 20], (bit, ks)
    # the chunked walk: chunks of 2 and 4 on 256 CUs, and one row tile less would not give them; the small short-K cases walk tile by tile
    assert [L.shortk_chunk(c) for c in L.CHUNK_CASES] == [2, 2, 4, 4]
    assert all(L.shortk_chunk(c._replace(M=c.M - c.bm)) < L.shortk_chunk(c) for c in L.CHUNK_CASES)
    assert all(L.shortk_chunk(c) == 1 for c in L.CASES if c.family in ("c4", "c8"))
    assert -(-L.packed_width(L.CHUNK_CASES[0]) // 128) % 2 == 1      # an odd number of column tiles: chunks straddle row blocks
    assert {r[0] for r in L.REFUSALS} and all(r[9] in (L.E_ARG, L.UNSUPPORTED) for r in L.REFUSALS)


@pytest.mark.parametrize("dtype", L.DTYPES)
def test_rows_are_distinct_and_keep_their_statistics(dtype):
    for M, K in sorted({(c.M, c.K) for c in ALL}):
        x, mu, sigma = L.x_input(M, K, dtype)
        assert np.array_equal(x, L.round16(x, dtype))
        assert L.rows_distinct(mu, sigma, 512), (M, K)
        live = sigma > 0
        assert (~live).sum() == len(L.const_rows(M)) and (mu[~live] != 0).all() and (x[~live] == x[~live][:, :1]).all()
        ratio = np.abs(mu[live]) / sigma[live]
        assert ratio.min() >= L.R_MAIN / 16 and ratio.max() <= L.R_MAIN * 16.75 / 16 and set(np.unique(sigma[live])) <= {0.25, 0.5, 1.0, 2.0, 4.0}
        x64 = x[live].astype(np.float64)
        assert np.allclose(x64.mean(axis=1), mu[live], rtol=0, atol=2.0 ** -L.MANTISSA[dtype] * np.abs(mu[live]).max())
        assert np.allclose(x64.std(axis=1), sigma[live], rtol=0.05 if dtype == "bf16" else 0.01)
    mu2, sigma2 = L.row_params(4000, 16)                      # the walk itself, away from the constant rows: one-to-one inside its period of 1120
    assert L.rows_distinct(mu2[4:1990], sigma2[4:1990], 1119) and not L.rows_distinct(mu2[4:1990], sigma2[4:1990], 1120)


@pytest.mark.parametrize("dtype", L.DTYPES)
def test_column_sums_differ(dtype):
    for Np, K in sorted({(L.packed_width(c), c.K) for c in ALL}):
        w, bias = L.weights(Np, K, dtype)
        wf, bf, cs = L.fold_host(w, bias, *L.affine(K), dtype)
        assert np.array_equal(w, L.round16(w, dtype)) and L.colsums_differ(cs.astype(np.float64)), (Np, K)
        assert L.colsums_differ(wf.astype(np.float64).sum(axis=1))


def _ratios(c, dtype):
    """(on float64 statistics, whole, whole at K_STAT - 1, whole at the constants, absolute error outside the constant rows), each once per run."""
    key = (L.data_key(c), dtype)
    if key not in WORST:
        pb = L.Problem(c, dtype)
        blocks = None if c not in L.CHUNK_CASES else _tiles(c)[1]
        ra, (rs, rs0, now), ab = L.emulation_ratios(pb, blocks, ((1, 1), (L.K_ACC, L.K_STAT - 1), (L.K_ACC, L.K_STAT)))
        WORST[key] = (ra, rs, rs0, now, ab)
    return WORST[key]


@pytest.mark.parametrize("dtype", L.DTYPES)
@pytest.mark.parametrize("c", DATA, ids=L.case_id)
def test_emulation_stays_within_half_the_budget(c, dtype):
    ra, rs, rs0, now, ab = _ratios(c, dtype)
    print(f"\n{L.data_key(c)} {dtype}: on float64 statistics {ra:.3f}, whole {rs:.3f} (K_STAT - 1: {rs0:.3f}) of A / 2 at K = 1; |err| <= {ab:.2e} outside the constant rows")
    assert ra <= L.K_ACC and now <= 1.0, (ra, rs, now)


def test_the_constants_are_minimal():
    """K_ACC = 1 and K_STAT = 1 hold on every case; 1 is the smallest positive K_ACC, and with K_STAT - 1 = 0 some case exceeds A / 2."""
    all_ = {(L.data_key(c), d): _ratios(c, d) for c in DATA for d in L.DTYPES}
    for i, name in enumerate(("on float64 statistics", "whole", "whole at K_STAT - 1", "whole at the constants", "absolute, outside the constant rows")):
        k = max(all_, key=lambda q: all_[q][i])
        print(f"\nlargest {name}: {all_[k][i]:.3g} at {k}")
    assert L.K_ACC == 1 and max(v[0] for v in all_.values()) <= 1.0 and max(v[3] for v in all_.values()) <= 1.0
    assert L.K_STAT == 1 and max(v[2] for v in all_.values()) > 1.0


@pytest.mark.parametrize("dtype", L.DTYPES)
def test_r_limit(dtype):
    R, ratio, nxt = L.cancellation_limit(dtype)
    print(f"\n{dtype}: meets A / 2 up to R = {R} ({ratio:.2f} of A / 2); one step above: {nxt if nxt is None else round(nxt, 2)}")
    assert R == L.R_LIMIT[dtype] and ratio <= 1.0 and (nxt is not None or 2 * R > L.max_plantable(dtype))
    for c in L.R_LIMIT_CASES:                                  # the launches the GPU test makes at that R: the emulation meets A / 2 there too
        assert L.emulation_ratios(L.Problem(c._replace(R=R), dtype))[1][1] <= 1.0, c


@pytest.mark.parametrize("dtype", L.DTYPES)
@pytest.mark.parametrize("c", TILED, ids=L.case_id)
def test_mutants_exceed_the_tolerance_in_every_row_tile(c, dtype):
    pb = L.Problem(c, dtype)
    alt = pb.alt()
    bm, tiles = _tiles(c)
    if pb.not_applicable():
        print(f"\n{L.case_id(c)} {dtype}: does not apply: {pb.not_applicable()}")
    assert set(alt) >= set(L.MUTANTS) - {"the variance without the clamp"} - ({"statistics of row m - bm (the stale chunk)"} if not c.bm else set())
    for sl in tiles:
        G = pb.gemm(sl)
        y, tol, _ = pb.block(sl, G)
        for name, ym in pb.mutants(sl, G).items():
            if alt[name]["rows"][sl].any():
                far = float(L.beyond(ym, y, tol)[alt[name]["rows"][sl]].max())
                assert far >= L.MUTANT_FACTOR, (L.case_id(c), dtype, name, sl, far)


def test_the_clamp_mutant_applies_somewhere():
    """in float64 a constant row's variance is 0 with or without the clamp: the slip shows only where the fp32 sums leave it below -eps, which depends
    on the row and the type.  float16 must have such rows at K >= 320 in every case; bfloat16 (8-bit mantissas: the fp32 sums of squares are exact up
    to K = 1280) has none, and the table says so."""
    for dtype in L.DTYPES:
        hit = [c for c in DATA if "the variance without the clamp" in L.Problem(c, dtype).alt()]
        print(f"\n{dtype}: the clamp is exercised by {len(hit)} of {len(DATA)} problems")
        if dtype == "fp16":
            assert {L.data_key(c) for c in hit} >= {L.data_key(c) for c in DATA if c.K >= 320}


DEMO = [c for c in L.CASES if L.case_id(c) in ("ring-165x100x320-a0r1-64x64-d8", "pp-421x80x320-a1r0-192x128-d512", "c8-549x168x1280-a0r1-256x128-d16384")]


@pytest.mark.parametrize("dtype", L.DTYPES)
@pytest.mark.parametrize("c", DEMO, ids=L.case_id)
def test_checker_names_a_planted_mutant(c, dtype):
    """the comparison the GPU test makes, fed wrong answers: it accepts the rounded reference and the rounded emulation, and fails every mutant by
    name (the mutant is among those "matched everywhere" of the report)."""
    pb = L.Problem(c, dtype)
    r = pb.res if pb.res is not None else 0.0
    whole = slice(0, c.M)
    y = pb.block(whole)[0]
    assert L.check_output(pb, L.round16(y, dtype))[2] is None
    emu = L.round16(L.round16(L.emulate_fold(pb, whole, L.LANES_OF_VARIANT[L.predict_form(c)[3]]), dtype) + r, dtype)
    worst, _, report = L.check_output(pb, emu)
    assert report is None and worst <= 1.0, report
    for name, ym in pb.mutants(whole).items():
        with np.errstate(all="ignore"):
            worst, _, report = L.check_output(pb, L.round16(ym, dtype))
        assert report is not None and worst >= L.MUTANT_FACTOR, (name, worst)
        assert name in report.split("mutants matched everywhere: ")[1], (name, report)


@pytest.mark.parametrize("dtype", L.DTYPES)
def test_weight_fold_emulation(dtype):
    worst = 0.0
    for N, K in L.FOLD_CASES:
        for with_bias in (True, False):
            w, bias = L.weights(N, K, dtype)
            bias = bias if with_bias else None
            gamma, beta = L.affine(K)
            wf, cs, bf, cs_tol, bf_tol, a = L.fold64(w, bias, gamma, beta, dtype)
            ecs, ebf = L.emulate_fold_weights(w, bias, gamma, beta, dtype)
            rc, rb = float((np.abs(ecs - cs) / (cs_tol / 2)).max()), float((np.abs(ebf - bf) / (a / 2)).max())
            print(f"\nk_ln_fold ({N}, {K}) {dtype} bias {with_bias}: colsum {rc:.3f}, bias' {rb:.3f} of A / 2 at K_SUM = {L.K_SUM}")
            worst = max(worst, rc, rb)
            assert (np.abs(L.round16(ebf, dtype) - bf) <= bf_tol).all()
    assert worst <= 1.0 and L.K_SUM == 1, worst                # (1: the smallest positive integer)


def test_tuning_table_forms_are_among_the_cases():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tinyfusers_amd", "gemm_tune_gfx950.txt")
    have = {L.tune_form(c) for c in ALL if c.bm}
    rows = 0
    for line in open(path):
        t = line.split()
        if len(t) != 15 or line.startswith("#"):
            continue
        t = [int(v) for v in t]
        if t[9] & 8:                                          # the LayerNorm flag of the key's flags column
            rows += 1
            assert (t[13], t[10], t[11], t[8], t[14]) in have, line
    assert rows > 0
