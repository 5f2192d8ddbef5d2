"""The planted conv inputs of tests/aux/conv_stats_planted.py (host code, no GPU), for every case tests/test_gpu_conv_stats_planted.py runs (the
case tables are imported from the aux module, so the two cannot drift apart):

  * the Python copies of gn_reduce_chunks / gn_pieces / rga_geometry give what the case tables claim -- every case is the form it is named for;
  * the exactness claims of the GEMM part hold in numpy: slabs of at most 2048 eighths that add up to the stated field, float64 equals fp32;
  * the emulated y (three fp32 additions, one storage rounding) lies within its bound of the float64 sum;
  * the numpy emulations of the three summation orders stay within TABLE_C / 2 of the float64 sums per table slot, and what a consumer computes
    from their tables within A / 2 of the float64 norm at K = K_CONV[form] -- the device gets twice the emulation's error;
  * the inputs tell a wrong kernel from a right one: every mutant moves an output or a table slot by more than 32 times its tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import norm_planted as P  # noqa: E402
import conv_stats_planted as C  # noqa: E402

DTYPES = ("fp16", "bf16")
SLABS = {"fp16": (32, 16), "bf16": (32,)}                 # element types of the split-K slabs a storage type runs with
MOVE = 32.0


def _affine(n, on):
    return P.affine(n) if on else (None, None)


def _moves(name, got, ref, tol):
    d = np.abs(np.asarray(got, np.float64) - ref)
    assert (d > MOVE * tol).any(), (name, float((d / np.maximum(tol, 1e-300)).max()))


def _table_moves(muts, T, y, G, rows, bn, c):
    ref, mag = C.table64(y, G, rows, bn)
    for name, m in muts.items():
        _moves(name, m, T.astype(np.float64), c * 2.0 ** -24 * mag)


def _z_ratio(z, y, G, gm, bt, silu, dtype, form):
    ref = P.gn_ref64(y, G, gm, bt, silu)
    tol, A = C.z_budget(ref, dtype, form, 2.0 if gm is not None else 1.0, silu)
    assert np.abs(ref).max() < 100
    return float((np.abs(z - ref) / P.a_unit(ref, C.R, 2.0 if gm is not None else 1.0)).max()), float((np.abs(z - ref) / (A / 2)).max()), ref, tol


def _y_checked(c, dtype, use=(1, 1, 1)):
    p = C.conv_problem(c, dtype, use)
    y = C.emulate_y(p, dtype)
    assert (np.abs(y - p["y64"]) <= C.y_tol(p, dtype)).all()
    return p, y


def test_rules_and_forms():
    assert C.gn_reduce_chunks(64) == 64 and C.gn_reduce_chunks(576) == 192 and C.gn_reduce_chunks(400) == 100 and C.gn_reduce_chunks(1633) == 71
    assert C.gn_pieces(128, 10) == 2 and C.gn_pieces(160, 10) == 1 and C.gn_pieces(160, 64) == 2
    assert C.rga_geometry(576, 320, 32) == dict(gpb=2, CV=5, RPS=204, parts=51, CW=20)
    assert C.rga_geometry(64, 128, 32)["RPS"] == 64 and C.rga_geometry(64, 224, 32)["gpb"] == 4
    assert C.rga_geometry(1632, 320, 32) and not C.rga_geometry(1633, 320, 32) and C.rga_geometry(816, 1280, 32) and not C.rga_geometry(817, 1280, 32)
    assert [C.eff_splitk(64 * C.KTILES[s], s) for s in C.SPLITS] == list(C.SPLITS)
    assert C.eff_splitk(64 * 18, 8) == 6 and C.eff_splitk(64 * 18, 16) == 9          # (why the split counts do not all run on 18 K tiles)
    for c in C.EPILOGUE_CASES:
        assert C.form_holds(c), c
    for c in C.REDUCE_GN_CASES:
        assert C.reduce_gn_form_holds(c) and C.predict(c)[0] == "reduce_gn", c
    for c, _, _ in C.FUSED_CASES:
        assert C.fused_form_holds(c) and C.predict(c, "norm") == ("reduce_gn_apply", 1, 1), c
    for c in C.REDUCE_GN_CASES[-2:]:
        assert C.predict(c, "norm")[0] == "reduce_gn"
    forms = {c.form for c in C.REDUCE_GN_CASES}
    assert forms >= {"R=1", "R multiple of RL", "R not multiple of RL", "padded wave", "RL=1 N=4096", "not eligible for the fused reduce"}
    assert {C.rga_geometry(c.H * c.W, c.Cout, c.G)["gpb"] for c, _, _ in C.FUSED_CASES} == {1, 2, 4}
    g = min(C.rga_geometry(c.H * c.W, c.Cout, c.G)["parts"] * (c.Cout // c.G) for c, _, _ in C.FUSED_CASES)
    assert g >= 64                                             # npairs of fold 2 never falls below 64


def _distinct(cases):
    seen, out = set(), []
    for c in cases:
        k = (c.N, c.H, c.W, c.Cin, c.Cout, c.ks, c.split)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


def test_exactness_claims():
    worst = 0.0
    for c in _distinct(C.EPILOGUE_CASES + C.REDUCE_GN_CASES + [f[0] for f in C.FUSED_CASES] + C.PLAIN_CASES):
        worst = max(worst, C.exact_claims(c))
    print(f"\nlargest split-K slab element: {worst:.0f} eighths (<= 2048)")
    assert worst >= 64                                         # the slabs are large against the field they cancel to
    w, perm, scale, tap = C.selector(128, 32, 3)
    assert set(tap.tolist()) == set(range(9))
    assert (np.count_nonzero(w.reshape(128, -1), axis=1) == 1).all() and np.array_equal(w, C.round16(w, "bf16"))


def test_planted_terms_differ():
    e = C.bias_nc_of(5, 320)
    assert (e != np.roll(e, -1, axis=0)).all() and np.array_equal(e * 8, np.round(e * 8)) and np.array_equal(C.bias_of(320) * 8, np.round(C.bias_of(320) * 8))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", C.EPILOGUE_CASES, ids=lambda c: f"{c.form}-{c.N}x{c.H}x{c.W}-{c.Cout}g{c.G}-{c.bm}x{c.bn}-{c.dbg}")
def test_epilogue(c, dtype):
    p, y = _y_checked(c, dtype)
    if c.N > 1:
        _moves("bias_nc rows rolled by one image", C.emulate_y(p, dtype, bias_nc=np.roll(p["bias_nc"], -1, axis=0)), y, C.y_tol(p, dtype))
    kind, chunks, _ = C.predict(c)
    if kind == "none":
        return
    sbm = c.bm // 2 if c.dbg in C.PINGPONG_BITS else c.bm
    T = C.emulate_epilogue(y, c.G, sbm, c.bn)
    assert T.shape == (c.N, chunks, c.G, 2)
    ratio, zeros = C.table_ok(T, y, c.G, sbm, c.bn, C.TABLE_C["epilogue"])
    gm, bt = _affine(c.Cout, True)
    unit, half, ref, tol = _z_ratio(C.emulate_consumer(y, T, c.G, gm, bt, True), y, c.G, gm, bt, True, dtype, "epilogue")
    print(f"\nepilogue {tuple(c)} {dtype}: table error / (2^-24 sum|y|) = {ratio:.3f}, consumer error / (A at K = 1) = {unit:.3f}")
    assert zeros and ratio <= C.TABLE_C["epilogue"] / 2 and ratio <= C.TABLE_RATIO["epilogue"] and half <= 1.0 and unit <= C.EMU_RATIO["epilogue"]
    two = C.gn_pieces(c.bn, c.Cout // c.G) == 2
    whole = ~C._piece_of(c.Cout, c.G, c.bn).any(axis=1)
    _table_moves(C.epilogue_table_mutants(T, two, whole), T, y, c.G, sbm, c.bn, C.TABLE_C["epilogue"])
    for name, m in C.stats_mutants(y, *P.gn_stats64(y, c.G), c.G, gm, bt, True).items():
        _moves(name, m, ref, tol)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", C.REDUCE_GN_CASES, ids=lambda c: f"{c.form}-{c.N}x{c.H}x{c.W}-{c.Cout}g{c.G}-s{c.split}")
def test_reduce_gn(c, dtype):
    p, y = _y_checked(c, dtype)
    for bits in SLABS[dtype]:
        for name, m in C.slab_mutants(p, c, dtype, bits).items():
            _moves(name, m, y, C.y_tol(p, dtype))
    geo = C.reduce_gn_geometry(c.H * c.W, c.Cout)
    T = C.emulate_reduce_gn(y, c.G)
    assert T.shape == (c.N, geo["chunks"], c.G, 2)
    ratio, zeros = C.table_ok(T, y, c.G, geo["R"], None, C.TABLE_C["reduce_gn"])
    gm, bt = _affine(c.Cout, True)
    unit, half, ref, tol = _z_ratio(C.emulate_consumer(y, T, c.G, gm, bt, True), y, c.G, gm, bt, True, dtype, "reduce_gn")
    print(f"\nreduce_gn {tuple(c)} {dtype}: table error / (2^-24 sum|y|) = {ratio:.3f}, consumer error / (A at K = 1) = {unit:.3f}")
    assert zeros and ratio <= C.TABLE_C["reduce_gn"] / 2 and ratio <= C.TABLE_RATIO["reduce_gn"] and half <= 1.0 and unit <= C.EMU_RATIO["reduce_gn"]
    _table_moves(C.epilogue_table_mutants(T, False, None), T, y, c.G, geo["R"], None, C.TABLE_C["reduce_gn"])
    for name, m in C.stats_mutants(y, *P.gn_stats64(y, c.G), c.G, gm, bt, True).items():
        _moves(name, m, ref, tol)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c,aff,silu", C.FUSED_CASES, ids=lambda v: f"{v.form}-{v.N}x{v.H}x{v.W}-{v.Cout}g{v.G}-s{v.split}" if isinstance(v, C.Conv) else str(int(v)))
def test_reduce_gn_apply(c, aff, silu, dtype):
    p, y = _y_checked(c, dtype)
    for bits in SLABS[dtype]:
        for name, m in C.slab_mutants(p, c, dtype, bits).items():
            _moves(name, m, y, C.y_tol(p, dtype))
    HoWo, cpg = c.H * c.W, c.Cout // c.G
    geo = C.rga_geometry(HoWo, c.Cout, c.G)
    gm, bt = _affine(c.Cout, aff)
    T, z = C.emulate_fused(y, c.G, gm, bt, silu)
    ratio, zeros = C.table_ok(T, y, c.G, HoWo, None, C.TABLE_C["reduce_gn_apply"])
    unit, half, ref, tol = _z_ratio(z, y, c.G, gm, bt, silu, dtype, "reduce_gn_apply")
    print(f"\nreduce_gn_apply {tuple(c)} {dtype}: table error / (2^-24 sum|y|) = {ratio:.3f}, z error / (A at K = 1) = {unit:.3f}")
    assert zeros and ratio <= C.TABLE_C["reduce_gn_apply"] / 2 and ratio <= C.TABLE_RATIO["reduce_gn_apply"] and half <= 1.0 and unit <= C.EMU_RATIO["reduce_gn_apply"]
    padded = geo["RPS"] * C.RGA_MAXR
    muts = C.stats_mutants(y, *P.gn_stats64(y, c.G), c.G, gm, bt, silu, padded_cnt=padded if padded != HoWo else None)
    cnt = float(HoWo * cpg)
    if HoWo % geo["RPS"]:
        S, Q = C.emulate_reduce_gn_apply_stats(y, c.G, lose_ragged=True)
        muts["the ragged last sweep lost from the sums"] = P.gn_apply64(y, *C.stats_of_sums(S, Q, cnt), c.G, gm, bt, silu)
    if geo["RPS"] < geo["parts"]:
        S, Q = C.emulate_reduce_gn_apply_stats(y, c.G, stale=1.0)
        muts["fold-1 lanes beyond RPS read stale"] = P.gn_apply64(y, *C.stats_of_sums(S, Q, cnt), c.G, gm, bt, silu)
    for name, m in muts.items():
        _moves(name, m, ref, tol)


@pytest.mark.parametrize("dtype", DTYPES)
def test_plain_reduce_mutants(dtype):
    for c in C.PLAIN_CASES:
        p, y = _y_checked(c, dtype)
        for bits in SLABS[dtype]:
            muts = C.slab_mutants(p, c, dtype, bits)
            s_, NB = C.eff_splitk(c.Cin, c.split), C.sum_partials_nb(C.eff_splitk(c.Cin, c.split), bits)
            assert "one split slab lost" in muts and any("clamped" in k for k in muts) == (s_ % NB != 0), (c, bits, list(muts))
            for name, m in muts.items():
                _moves(name, m, y, C.y_tol(p, dtype))
    # every batch width of sum_partials runs full and with clamped loads somewhere in the split counts
    seen = {(C.sum_partials_nb(s_, bits), s_ % C.sum_partials_nb(s_, bits) != 0) for s_ in C.SPLITS for bits in (16, 32)}
    assert seen >= {(2, False), (4, False), (4, True), (8, False), (8, True), (16, False), (16, True)}
    for use in C.SUBSETS:
        _y_checked(C.PLAIN_CASES[0], dtype, use)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H,W,C1,C2,G,ks,bm,bn,chunks,chunks2,silu", C.GI_CASES)
def test_selector_cases(N, H, W, C1, C2, G, ks, bm, bn, chunks, chunks2, silu, dtype):
    """Part C: the conv output is sign 2^k times the rounded normalised input (or exactly 0 where the tap reads the padding), so norm_planted's
    budget and its mutants carry over."""
    Ct = C1 + C2
    w, perm, scale, tap = C.selector(Ct, G, ks)
    assert C2 == 0 or (C1 % (Ct // G) != 0 and (Ct // G) % C.GI_SUB == 0)      # a group on the seam, tiled by the sub-groups
    x, _, _ = P.gn_input(N, Ct, H * W, G, dtype)
    gm, bt = _affine(Ct, True)
    if C2:
        p1, p2 = P.partials(np.ascontiguousarray(x[..., :C1]), C1 // C.GI_SUB, chunks), P.partials(np.ascontiguousarray(x[..., C1:]), C2 // C.GI_SUB, chunks2)
        st = P.cat_stats(p1, p2, H * W, C.GI_SUB, (Ct // G) // C.GI_SUB)
    else:
        st = P.stats_from_partials(P.partials(x, G, chunks), H * W, Ct // G)
    ref = P.gn_apply64(x, *st, G, gm, bt, silu)
    tol, A = C.budget(ref, dtype, C.R, 2.0, silu, stats=True)
    zn = C.round16(P.emulate_gn_apply(x, *st, G, gm, bt, silu), dtype)
    want, wtol = C.selector_answer(ref, tol, w, N, H, W)
    out = C.selector_answer(zn.astype(np.float64), tol, w, N, H, W)[0]
    assert np.array_equal(out, C.round16(out, dtype)) and (np.abs(out - want) <= wtol).all()       # exact in the storage type, inside the budget
    assert ks == 1 or ((wtol == 0) & (want == 0)).any()                                            # border outputs read the padding
    for name, m in C.stats_mutants(x, *st, G, gm, bt, silu).items():
        _moves(name, C.selector_answer(m, tol, w, N, H, W)[0], want, wtol)
