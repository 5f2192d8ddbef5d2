"""The planted-statistics norm inputs of tests/aux/norm_planted.py (host code, no GPU), for every input tests/test_gpu_norm_planted.py runs (the case
tables are imported from the aux module, so the two cannot drift apart):

  * the inputs equal their own storage rounding, neighbouring slices (adjacent groups, adjacent images, rows of one wave) have distinct planted
    statistics and the slices keep them (|mean| / std within 1 % of the planted ratio, never above R by more);
  * the numpy emulation of the kernels' fp32 arithmetic stays within A / 2 of the float64 reference (SiLU outputs: also with the exp2 and the
    reciprocal moved by one ulp either way, within A / 2 + 2^-22 |y|) -- the device is then held to A, twice the emulation's error;
  * the inputs can tell a wrong kernel from a right one: every mutant of the float64 reference (a neighbour's statistics, a lost chunk or channel
    vector, a padded count, rolled affine parameters, a wrong row stride or partial table, an unwritten batch) moves some output by more than 32 tol;
  * the 8-bit outputs: the quantised emulation meets the acceptance rule of tests/test_gpu_mx8.py against the quantised float64 reference (within
    one e4m3 step, under 3 % of the elements differ) and the mutants move a dequantised output by more than that step."""
import concurrent.futures as cf
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import norm_planted as P  # noqa: E402

DTYPES = ("fp16", "bf16")
MOVE = 32.0
R = P.R_MAIN


def _affine(C, on):
    return P.affine(C) if on else (None, None)


def _assert_moves(muts, ref, tol, what):
    for name, m in muts.items():
        assert (np.abs(m - ref) > MOVE * tol).any(), (what, name, float((np.abs(m - ref) / tol).max()))


def _worst(emu, ref, A, extra=0.0):
    return float(((np.abs(emu - ref) - extra) / (A / 2)).max())


def _check_gn_input(x, mu, sigma, G, dtype, R_):
    assert np.array_equal(x, P.round16(x, dtype))
    n, HW, C = x.shape
    if HW * (C // G) >= 64:                                   # a slice large enough to hold its planted statistics through the rounding
        m, v = P.gn_stats64(x[:4], G)
        ratio = np.abs(m) / np.sqrt(v)
        assert np.allclose(ratio, np.abs(mu[:4]) / sigma[:4], rtol=0.02) and ratio.max() <= R_ * 1.02, ratio.max()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form,N,C1,C2,HW,G", P.GN_CASES)
def test_group_norm_inputs(form, N, C1, C2, HW, G, dtype):
    C = C1 + C2
    geo = P.gn_geometry(N, HW, C)
    assert P.gn_form_holds(form, geo, HW, C1, C2, G), (form, geo)
    x, mu, sigma = P.gn_input(N, C, HW, G, dtype)
    _check_gn_input(x, mu, sigma, G, dtype, R)
    assert np.abs(mu / sigma).max() <= R and np.abs(mu / sigma).min() >= R / 16 and set(np.unique(sigma)) <= {0.25, 0.5, 1.0, 2.0, 4.0}
    def one(sl):
        worst = {}
        xb = x[sl]
        em, ev = P.stats_from_partials(P.emulate_gn_partials(xb, G, geo), HW, C // G)
        m64, v64 = P.gn_stats64(xb, G)
        for aff in (False, True):                             # GN_VARIANTS: plain, affine, affine + SiLU (which shares the affine's values)
            gm, bt = _affine(C, aff)
            ref = P.gn_apply64(xb, m64, v64, G, gm, bt, False)
            f = P.emulate_gn_apply(xb, em, ev, G, gm, bt, False)
            assert np.abs(ref).max() < 100
            runs = [(False, 0, ref, f)]
            if aff:
                rs = P.silu64(ref)
                runs += [(True, u, rs, P.emulate_silu(f, u)) for u in (0, 1, -1)]
            for silu, ulp, r_, e_ in runs:
                assert (aff, silu) in P.GN_VARIANTS
                tol, A = P.budget(r_, dtype, R, 2.0 if aff else 1.0, silu)
                worst[aff, silu, ulp] = _worst(e_, r_, A, 2.0 ** -22 * np.abs(r_) if ulp else 0.0)
                if ulp == 0 and sl.start == 0 and xb.shape[0] >= 2:
                    _assert_moves(P.gn_mutants(xb[:4], C1, G, geo, gm, bt, silu), r_[:4], tol[:4], (form, aff, silu))
        return worst
    with cf.ThreadPoolExecutor(4) as pool:                    # (numpy releases the GIL: the 400-image cases take seconds instead of ten)
        parts = list(pool.map(one, P.image_batches(N, HW, C)))
    worst = {k: max(p[k] for p in parts) for k in parts[0]}
    print(f"\ngroup norm {form} {(N, C1, C2, HW, G)} {dtype}: emulation error / (A / 2) = " + ", ".join(f"{k}: {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("entry,N,C1,C2,HW,G,g1,g2,chunks,chunks2,dtype", P.apply_rows())
def test_apply_on_host_partials(entry, N, C1, C2, HW, G, g1, g2, chunks, chunks2, dtype):
    """The apply entries on partials(): the reference is the float64 norm under the statistics the fp32 partials state, so the budget is the
    arithmetic part alone (stats = False)."""
    C = C1 + C2
    geo = P.gn_geometry(N, HW, C)
    x, _, _ = P.gn_input(N, C, HW, G, dtype)
    worst = 0.0
    for sl in P.image_batches(N, HW, C):
        xb = x[sl]
        tables = None
        if C2:
            sub = C1 // g1
            mr = (C // G) // sub
            assert C2 // g2 == sub and (C // G) % sub == 0 and mr <= 8
            p1, p2 = P.partials(np.ascontiguousarray(xb[..., :C1]), g1, chunks), P.partials(np.ascontiguousarray(xb[..., C1:]), g2, chunks2)
            tables = (p1, p2, sub, mr)
            st = P.cat_stats(p1, p2, HW, sub, mr)
        else:
            part = P.partials(xb, G, chunks)
            assert part.shape == (xb.shape[0], chunks, G, 2) and part.dtype == np.float32
            st = P.stats_from_partials(part, HW, C // G)
        true = P.gn_stats64(xb, G)                             # the partials state the slice's statistics up to their fp32 rounding
        assert np.allclose(st[0], true[0], rtol=1e-6) and np.allclose(st[1], true[1], rtol=2e-4, atol=0)
        for aff, silu in P.GN_VARIANTS:
            gm, bt = _affine(C, aff)
            ref = P.gn_apply64(xb, *st, G, gm, bt, silu)
            tol, A = P.budget(ref, dtype, R, 2.0 if aff else 1.0, silu, stats=False)
            worst = max(worst, _worst(P.emulate_gn_apply(xb, *st, G, gm, bt, silu), ref, A))
            if sl.start == 0:
                muts = P.gn_mutants(xb[:4], C1, G, geo, gm, bt, silu, stats=(st[0][:4], st[1][:4]), sub_tables=tables and (tables[0][:4], tables[1][:4], tables[2], tables[3]))
                lost = P.partials(xb[:4], G, chunks) if not C2 else None
                if lost is not None:
                    muts["last chunk of the partials dropped"] = P.gn_apply64(xb[:4], *P.stats_from_partials(lost[:, :-1] if chunks > 1 else lost * 0, HW, C // G), G, gm, bt, silu)
                _assert_moves(muts, ref[:4], tol[:4], (entry, chunks, aff, silu))
    print(f"\n{entry} {(N, C1, C2, HW, G, chunks, chunks2)} {dtype}: emulation error / (A / 2) = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form,rows,C", P.LN_CASES)
def test_layer_norm_inputs(form, rows, C, dtype):
    assert P.ln_instance(rows, C) == form
    x, mu, sigma = P.ln_input(rows, C, dtype)
    assert np.array_equal(x, P.round16(x, dtype))
    assert np.abs(mu / sigma).max() <= R and np.abs(mu / sigma).min() >= R / 16
    if C >= 64:
        m, v = P.ln_stats64(x)
        assert np.allclose(np.abs(m) / np.sqrt(v), np.abs(mu) / sigma, rtol=0.02)
    for aff in (False, True):
        gm, bt = _affine(C, aff)
        ref = P.ln_ref64(x, gm, bt)
        tol, A = P.budget(ref, dtype, R, 2.0 if aff else 1.0)
        assert np.abs(ref).max() < 100
        w = _worst(P.emulate_layer_norm(x, form, gm, bt), ref, A)
        print(f"\nlayer norm <{form}> {(rows, C)} {dtype} affine={aff}: emulation error / (A / 2) = {w:.3f}")
        assert w <= 1.0
        head = slice(0, 64)                                    # the first rows (every wave of the first block) suffice to show a mutant moves
        _assert_moves(P.ln_mutants(x[head], form, gm, bt), ref[head], tol[head], (form, rows, C, aff))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import tinyfusers_amd.native as n
    return n.lib


def test_library_rule_equals_the_copy(lib):
    """tf_layer_norm_instance / tf_group_norm_geometry (host code, no device needed: the launchers' own rule) against the aux module's copy, at
    every case of the tables and on both sides of every threshold of the rule; the header's enum carries the copy's names."""
    import ctypes
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tinyfusers_hip.h")).read()
    enum = {int(v): n for n, v in re.findall(r"TF_LN_INST_([A-Z0-9_]+) = (\d+)", hdr)}
    assert {v: n.lower().replace("lpr", "") for v, n in enum.items()} == P.LN_INSTANCES
    shapes = [(r, c) for _, r, c in P.LN_CASES] + [(r, c) for r in (1, 8191, 8192) for c in (8, 320, 328, 640, 648, 1280, 1288, 2560, 2568, 12, 4096, 4097, 100000)]
    for rows, C in shapes:
        assert P.LN_INSTANCES[lib.tf_layer_norm_instance(rows, C)] == P.ln_instance(rows, C), (rows, C)
    for form, rows, C in P.LN_CASES + P.LN8_CASES:
        assert P.LN_INSTANCES[lib.tf_layer_norm_instance(rows, C)] == form
    assert lib.tf_layer_norm_instance(4, 0) == 10001 and b"tf_layer_norm_instance" in lib.tf_last_error()
    o = [ctypes.c_int(-1) for _ in range(5)]
    refs = [ctypes.byref(v) for v in o]
    shapes = [(c[1], c[4], c[2] + c[3]) for c in P.GN_CASES + P.APPLY_CASES + P.GN8_CASES]
    shapes += [(n, hw, c) for n in (1, 2, 8) for hw in (1, 7, 64, 4096, 9216) for c in (8, 64, 320, 1920, 2048, 2056, 8192)] + [(767, 8, 2048), (768, 8, 2048)]
    for N, HW, C in shapes:
        assert lib.tf_group_norm_geometry(N, HW, C, *refs) == 0
        mine = P.gn_geometry(N, HW, C)
        got = dict(zip(("rpb", "chunks", "pix_per_chunk", "apply_blocks", "nbatch"), (v.value for v in o)))
        assert got == {k: mine[k] for k in got}, (N, HW, C, got, mine)
        assert got["chunks"] <= P.GN_MAX_CHUNKS and got["chunks"] * got["pix_per_chunk"] >= HW and got["pix_per_chunk"] % got["rpb"] == 0
    assert P.gn_geometry(8, 9216, 320)["nbatch"] == 4         # the 4-image 96 x 96 step at C = 320 (UNet batch 8)
    assert lib.tf_group_norm_geometry(2, 16, 12, *refs) == 10001 and lib.tf_group_norm_geometry(2, 16, 64, None, *refs[1:]) == 10001
    assert b"tf_group_norm_geometry" in lib.tf_last_error()


def _quantisers():
    return (("mx8", P.mx_quant, 32), ("fp8", P.e4m3, 0))


@pytest.mark.parametrize("form,rows,C", P.LN8_CASES)
def test_layer_norm_8bit_inputs(form, rows, C):
    x, _, _ = P.ln_input(rows, C, "fp16")
    gm, bt = P.affine(C)
    ref, emu = P.ln_ref64(x, gm, bt), P.emulate_layer_norm(x, form, gm, bt)
    muts = P.ln_mutants(x[:64], form, gm, bt)
    for name, quant, block in _quantisers():
        want = quant(ref)
        ok, share, step = P.close8(quant(emu.astype(np.float64)), want, block)
        print(f"\nlayer norm <{form}> {name}: share of elements the quantised emulation moves = {share:.4f}")
        assert ok and share < 0.03 / 2, share                   # (half the cap: the device gets the same margin as under the 16-bit budget)
        for what, m in muts.items():
            assert (np.abs(quant(m) - want[:64]) > step[:64]).any(), (name, what)


@pytest.mark.parametrize("entry,N,C1,C2,HW,G,g1,g2,chunks,chunks2", P.GN8_CASES)
def test_group_norm_8bit_inputs(entry, N, C1, C2, HW, G, g1, g2, chunks, chunks2):
    C = C1 + C2
    geo = P.gn_geometry(N, HW, C)
    assert geo["nbatch"] > 1
    x, _, _ = P.gn_input(N, C, HW, G, "fp16")
    gm, bt = P.affine(C)
    sl = P.image_batches(N, HW, C)[0]                          # (the share of a batch of images: every image has the same kind of slices)
    xb = x[sl]
    tables = None
    if C2:
        sub, mr = C1 // g1, (C // G) // (C1 // g1)
        p1, p2 = P.partials(np.ascontiguousarray(xb[..., :C1]), g1, chunks), P.partials(np.ascontiguousarray(xb[..., C1:]), g2, chunks2)
        tables, st = (p1[:4], p2[:4], sub, mr), P.cat_stats(p1, p2, HW, sub, mr)
    else:
        st = P.stats_from_partials(P.partials(xb, G, chunks), HW, C // G)
    ref, emu = P.gn_apply64(xb, *st, G, gm, bt, True), P.emulate_gn_apply(xb, *st, G, gm, bt, True)
    muts = P.gn_mutants(xb[:4], C1, G, geo, gm, bt, True, stats=(st[0][:4], st[1][:4]), sub_tables=tables)
    rows = lambda a: a.reshape(-1, C)
    for name, quant, block in _quantisers():
        want = quant(rows(ref))
        ok, share, step = P.close8(quant(rows(emu).astype(np.float64)), want, block)
        print(f"\ngroup norm apply {entry} {name}: share of elements the quantised emulation moves = {share:.4f}")
        assert ok and share < 0.03 / 2, share
        k = 4 * HW
        for what, m in muts.items():
            assert (np.abs(quant(rows(m)) - want[:k]) > step[:k]).any(), (name, what)


def test_numpy_quantisers_match_the_oracle():
    """e4m3 / mx_quant of the aux module (numpy only) against oracle.fp8, the definition tests/test_gpu_mx8.py holds the device quantisers to."""
    from oracle import fp8 as O8
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((64, 96)) * np.exp2(rng.integers(-12, 9, (64, 3)).repeat(32, axis=1))).astype(np.float16).astype(np.float32)
    x[0, :32] = 0.0
    x[1, 5], x[2, 7], x[3, 9] = 448.0, -896.0, 449.0
    codes = np.arange(256, dtype=np.uint8)
    assert np.array_equal(P.decode_e4m3(codes), O8.decode_e4m3(codes).astype(np.float64), equal_nan=True)
    assert np.array_equal(P.e4m3(x.astype(np.float64)), O8.quant_act(x).numpy().astype(np.float64))
    assert np.array_equal(P.mx_quant(x.astype(np.float64)), O8.quant_act_mx(x).numpy().astype(np.float64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cancellation_limit(dtype):
    """The single-pass statistics lose accuracy as R^2: the largest power-of-two R at which the emulation still meets A / 2 at (2, 64, 289, 8)
    is what the GPU test runs as its cancellation case, and what DESIGN.md states as the limit."""
    Rl, ratio, above = P.cancellation_limit(dtype)
    print(f"\ncancellation {dtype}: R = {Rl} at {ratio:.3f} of A / 2, one step above: {above}")
    assert (Rl, above is None) == {"fp16": (32, False), "bf16": (32, True)}[dtype]
    assert ratio <= 1.0 and (above is None or above > 1.0)
    _, N, C, _, HW, G = P.CANCELLATION_SHAPE
    x, mu, sigma = P.gn_input(N, C, HW, G, dtype, Rl)
    _check_gn_input(x, mu, sigma, G, dtype, Rl)
    ref = P.gn_ref64(x, G)
    _assert_moves(P.gn_mutants(x, C, G, P.gn_geometry(N, HW, C), None, None, False), ref, P.budget(ref, dtype, Rl)[0], "cancellation")


def test_generator_refuses_what_the_type_cannot_hold():
    with pytest.raises(AssertionError, match="cannot plant"):
        P.gn_input(2, 64, 289, 8, "bf16", 64)                  # spacing at 64 sigma in bfloat16: sigma / 2
    with pytest.raises(AssertionError, match="cannot plant"):
        P.ln_input(5, 8, "fp16", 512)
    with pytest.raises(AssertionError, match="power of two"):
        P.ln_input(5, 8, "fp16", 24)
