"""Which E8M0 byte meets which 32 channels of which tap of which source tensor, bit for bit: every row of tests/aux/mx_geometry.py through the C ABI
-- tf_conv2d_mx8 with x2_mx / C2, tf_linear_mx8 -- with the tile, the split and the family forced: k_igemm_pp<F8> in its four tiles with half-tile
slabs off and on, on 3x3 pad 1 / pad 0, 1x1 pad 0 / pad 1 and 5x5 pad 2, one and two sources, split 1, 2 and rounded splits with 16- and 32-bit
slabs; k_igemm_pp3<F8> on 96-, 48- and 24-pixel rows with and without the half slab, one and two sources.  tests/test_mx_geometry_host.py proves on
the CPU that the planted integers make every output exact in fp32, in an fp16 slab and in fp16, and that they tell each of seventeen slips from the
right kernel.  Per launch, in this order: the status; tf_prof_dump shows exactly one launch with the predicted (M, N, K, taps, bm, bn, splitk, variant)
-- the split ASKED for -- and the split-K reduce family no launch for an effective split of 1, one launch over exactly eff slabs otherwise; the
64-element guard behind y still holds the sentinel; no sentinel is left in y; np.array_equal(y, reference).  A mismatch reports the first wrong
output, its tile and K ranges and the mutants the device agrees with there.  Refusals: the status, tf_last_error names the entry or the family, y and
the guard untouched, nothing launched.

The block-scaled GEGLU output (tf_linear_mx8, act = 1, out_mx = 1; out_features ragged against the 128-wide tile): the epilogue computes the fp16
value once and either stores it or quantises it, so the codes and scale bytes must EQUAL oracle.fp8.quant_act_mx_codes of the out_mx = 0 launch's
y16, every byte of both regions written (two fill patterns), nothing behind rows No + rows No / 32.  The only tolerance of the file is on y16 itself
against the float64 GEGLU (the GELU is not exact): TOL of tests/test_gpu_mx8.py.

119 tests (94 rows, 24 GEGLU shapes of three launches each, the refusals: 166 launches); measured on an MI355X: 4.2 s inside pytest -- the slowest case
(the first, with the library's start) takes 0.3 s, the others 0.04 s at most."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import mx_geometry as G  # noqa: E402
from test_gpu_conv_stats_planted import forced, profiled  # noqa: E402  (the force / profile brackets, shared by import)
from test_gpu_mx8 import TOL  # noqa: E402

pytestmark = pytest.mark.gpu

S16 = np.float32(np.float16(G.SENTINEL))


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def _u8(tf, a):
    return tf.DeviceArray.from_numpy(np.ascontiguousarray(a, np.uint8).reshape(-1), np.uint8, "row")


def _f16(tf, a):
    return tf.DeviceArray.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1), np.float16, "row") if a is not None else None


def _f32(tf, a):
    return tf.DeviceArray.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1), np.float32, "row")


def _ptr(a):
    return a.ptr if a is not None else None


class Launch:
    pass


def launch(tf, c, override=None):
    """uploads the row -- block-scaled tensors as one buffer each, codes then scale bytes -- pre-fills y (+ guard) with the sentinel and runs the entry
    under the forced tile / split / family; nothing is asserted here.  `override`: arguments replaced behind the row's own (the refusals)."""
    from tinyfusers_amd.native import lib
    o = dict(override or {})
    p = G.inputs(c)
    Ho, Wo, M, C, K = G.dims(c)
    r = Launch()
    h = r.hold = dict(x=_u8(tf, G.mx_buffer(p["x"], p["xs"])), x2=_u8(tf, G.mx_buffer(p["x2"], p["x2s"])) if c.C2 else None, w=_u8(tf, G.codes_of(p["w"])),
                      wscale=_f32(tf, p["wscale"]), bias=_f16(tf, p["bias"]), bias_nc=_f16(tf, p["bias_nc"]), res=_f16(tf, p["res"]))
    n = M * c.Cout
    r.dy = tf.DeviceArray.from_numpy(np.full((n + G.GUARD,), G.SENTINEL, np.float32), np.float16, "row")
    h["ws"] = tf.DeviceArray.empty((max(c.split, 1) * M * c.Cout * 4 + 64,), np.uint8, "row")
    with forced(c.bm, c.bn, c.split, c.dbg, c.slabs), profiled() as r.prof:
        if c.kind == "linear":
            r.rc = lib.tf_linear_mx8(r.dy.ptr, h["x"].ptr, h["w"].ptr, h["wscale"].ptr, _ptr(h["bias"]), _ptr(h["res"]), M, o.get("Nout", c.Cout), K, o.get("act", 0),
                                     o.get("out_mx", 0), h["ws"].ptr, h["ws"].nbytes, tf._sh())
        else:
            r.rc = lib.tf_conv2d_mx8(r.dy.ptr, h["x"].ptr, _ptr(h["x2"]), h["w"].ptr, h["wscale"].ptr, _ptr(h["bias"]), _ptr(h["bias_nc"]), G.nc_stride(c), _ptr(h["res"]),
                                     c.N, c.H, c.W, c.C1, c.C2, c.Cout, c.R, o.get("S", c.R), o.get("stride", 1), c.pad, h["ws"].ptr, h["ws"].nbytes, None, 0, 0, None, tf._sh())
        r.err = lib.tf_last_error()
    full = r.dy.numpy()
    r.y, r.guard = full[:n].reshape(c.N, Ho, Wo, c.Cout), full[n:]
    return r


def _report(c, y, ref):
    """the first wrong output: where it is, what covers it, and which slips would explain it."""
    Ho, Wo, M, C, K = G.dims(c)
    bad = np.argwhere(y != ref)
    img, ho, wo, ch = (int(v) for v in bad[0])
    m = (img * Ho + ho) * Wo + wo
    m0, n0 = m // c.bm * c.bm, ch // c.bn * c.bn
    wrongs = G.mutants(c)
    match = [name for name, wrong in wrongs.items() if wrong[img, ho, wo, ch] == y[img, ho, wo, ch] and wrong[img, ho, wo, ch] != ref[img, ho, wo, ch]]
    whole = [name for name, wrong in wrongs.items() if np.array_equal(wrong, y)]
    return (f"{c.name}: {len(bad)} of {y.size} outputs wrong; first at (image {img}, ho {ho}, wo {wo}, channel {ch}): device {y[img, ho, wo, ch]}, reference "
            f"{ref[img, ho, wo, ch]}; tile rows [{m0}, {min(m0 + c.bm, M)}) x columns [{n0}, {min(n0 + c.bn, c.Cout)}), K ranges of the splits {G.split_ranges(K, c.split)} "
            f"(C1 | C2 = {c.C1} | {c.C2}, K = {K}); mutants matching there: {match or 'none'}; mutants matching everywhere: {whole or 'none'}; {G.predict_form(c).kernel}")


@pytest.mark.parametrize("c", G.ALL, ids=[c.name for c in G.ALL])
def test_block_scaled_gemm_is_exact(tf, c):
    form = G.predict_form(c)
    Ho, Wo, M, C, K = G.dims(c)
    r = launch(tf, c)
    assert r.rc == 0, (c.name, r.rc, r.err)                                                                       # 1. the status
    assert r.prof.rows == [(M, c.Cout, K, c.R * c.R, *form.row, 1)], (c.name, r.prof.rows, form)                  # 2. the one launch, as predicted
    if form.eff == 1:                                                                                             #    ... and the reduce family
        assert r.prof.reduce[0] == 0, (c.name, r.prof.reduce)
    else:
        slab = 2 if c.slabs == 16 and c.Cout % 8 == 0 else 4
        mn = float(M) * c.Cout
        assert r.prof.reduce == (1, mn * form.eff * slab + mn * 2.0 * (1 + (1 if c.res else 0))), (c.name, r.prof.reduce, form.eff, slab)
    assert (r.guard == S16).all(), (c.name, "the guard behind y was written", np.flatnonzero(r.guard != S16)[:8])  # 3. the guard
    assert not (r.y == S16).any(), (c.name, "outputs never written", np.argwhere(r.y == S16)[:4].tolist())         # 4. no sentinel left
    ref = np.asarray(G.reference(c), np.float64)
    assert np.array_equal(r.y, ref), _report(c, r.y.astype(np.float64), ref)                                      # 5. bit for bit


def test_refusals(tf):
    """launches the entry must refuse (TF_E_ARG) and families that must fail by name instead of running another kernel (TF_E_UNSUPPORTED): the status,
    the text, y and the guard untouched, nothing launched."""
    for ref in G.REFUSALS:
        r = launch(tf, ref.case, ref.override)
        assert r.rc == ref.rc, (ref.what, r.rc, r.err)
        assert ref.says in r.err, (ref.what, r.err)
        assert r.prof.rows == [] and r.prof.reduce[0] == 0, (ref.what, r.prof.rows)
        assert (r.y == S16).all() and (r.guard == S16).all(), (ref.what, "a refused launch wrote y")


def _geglu_launch(tf, g, h, out_mx, fill):
    """one GEGLU launch: out_mx = 0 -> (status, y16 (M, No), guard); out_mx = 1 -> (status, all bytes of the buffer + guard)."""
    from tinyfusers_amd.native import lib
    n = g.M * g.No
    if out_mx:
        total = int(lib.tf_mx8_bytes(g.M, g.No))
        assert total == n + n // 32
        dy = _u8(tf, np.full((total + G.GUARD,), fill, np.uint8))
    else:
        dy = tf.DeviceArray.from_numpy(np.full((n + G.GUARD,), G.SENTINEL, np.float32), np.float16, "row")
    with forced(g.bm, g.bn, 1, G.BIT["pp"]), profiled() as prof:
        rc = lib.tf_linear_mx8(dy.ptr, h["x"].ptr, h["w"].ptr, h["wscale"].ptr, h["bias"].ptr, None, g.M, g.No, g.K, 1, out_mx, None, 0, tf._sh())
        err = lib.tf_last_error()
    assert rc == 0, (g.name, out_mx, rc, err)
    assert prof.rows == [(g.M, 2 * g.No, g.K, 1, g.bm, g.bn, 1, G.V_PP, 1)] and prof.reduce[0] == 0, (g.name, out_mx, prof.rows, prof.reduce)
    return dy.numpy()


@pytest.mark.parametrize("g", G.GEGLU, ids=[g.name for g in G.GEGLU])
def test_geglu_block_scaled_output_is_the_quantised_fp16_output(tf, g):
    from oracle import fp8 as O8
    p = G.geglu_inputs(g)
    h = dict(x=_u8(tf, G.mx_buffer(p["x"], p["xs"])), w=_u8(tf, G.codes_of(G.pack_geglu_rows(p["w"], g.No))), wscale=_f32(tf, G.pack_geglu_rows(p["wscale"], g.No)),
             bias=_f16(tf, G.pack_geglu_rows(p["bias"], g.No)))
    n = g.M * g.No
    full = _geglu_launch(tf, g, h, 0, None)
    y16, guard = full[:n].reshape(g.M, g.No), full[n:]
    assert (guard == S16).all() and not (y16 == S16).any(), (g.name, "fp16 launch: guard written or outputs left")
    want, _ = G.geglu_reference(g)
    np.testing.assert_allclose(y16, want, **TOL)
    codes, scales = O8.quant_act_mx_codes(y16)
    for fill in (0xA5, 0x5A):
        raw = _geglu_launch(tf, g, h, 1, fill)
        got_c, got_s, guard = raw[:n].reshape(g.M, g.No), raw[n:n + n // 32].reshape(g.M, g.No // 32), raw[n + n // 32:]
        assert (guard == fill).all(), (g.name, "written behind rows No + rows No / 32", np.flatnonzero(guard != fill)[:8])
        assert np.array_equal(got_s, scales), (g.name, fill, "scale bytes", np.argwhere(got_s != scales)[:4].tolist())
        assert np.array_equal(got_c, codes), (g.name, fill, "codes", np.argwhere(got_c != codes)[:4].tolist())
