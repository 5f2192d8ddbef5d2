"""Conv addressing of k_igemm (ring / wide / all-8, GENERIC and 64-grid, every tile), k_igemm_patch, k_igemm_pp as a conv and k_igemm8, bit for bit:
every row of tests/aux/conv_geometry.py (132 rows, 255 launches with the bfloat16 twins; tests/test_conv_geometry_host.py proves on the CPU that the
{-1, 0, 1} inputs tell each of eighteen addressing slips from the right kernel) through the C ABI -- tf_conv2d_fused_16, tf_conv2d_fp8 -- with the
tile, split and family forced.  Per launch, in this order: the status; tf_prof_dump shows exactly one launch with the predicted (M, N, K, taps, bm,
bn, splitk, variant) -- the split ASKED for -- and the library's own rule (tf_gemm_ring_form, tf_conv2d_patch_admits) agrees with the aux module's
copy about the instance behind it; the split-K reduce family shows no launch for an effective split of 1 and one launch over exactly eff slabs
otherwise (the rounded split of the row that asks for more splits than whole K tiles allow); the 64-element guard behind y is untouched; no sentinel is
left in y; np.array_equal(y, reference).  A mismatch reports the first wrong output, its (image, ho, wo, channel), its tile's rows, the K range of
each split and the mutants whose output the device matches there.  Refusals (one test): the status, tf_last_error names the entry or the family, y
still holds the sentinel everywhere.

257 tests (255 launches, the refusals, the patch-on-stride-2 check); measured on an MI355X: 2.0 s inside pytest -- the slowest case (the first, with the library's start) takes 0.2 s, the others 0.05 s at most.

Among what the rows guard in k_igemm_pp: its lean addressing (a tap-validity bit per tap, built over S x S taps; the extra segment read unmasked at the
output pixel's own index) is right only for square filters and for extra sources sampled inside the image -- rows pp-3x1s1p1-*, pp-1x3s1p1-*,
pp-3x3s1p2-*-e64+64-* and pp-1x1s1p1-*-e64+0-* hold the launcher to sending R != S, and extras with Ho > H or Wo > W, to the general gather."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import conv_geometry as G  # noqa: E402
from test_gpu_conv_stats_planted import forced, profiled  # noqa: E402  (the force / profile brackets, shared by import)

pytestmark = pytest.mark.gpu

ROWS = [(c, d) for c in G.CASES for d in c.dtypes]


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def _el(tf, dtype):
    return tf.bfloat16 if dtype == "bf16" else np.float16


def _up(tf, a, dtype):
    """host integers -> a device array of the launch's 16-bit type (None stays None)."""
    return tf.DeviceArray.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1), _el(tf, dtype), "row") if a is not None else None


def _up8(tf, a):
    """host integers of {-1, 0, 1} -> the e4m3 codes themselves, written by the host."""
    if a is None:
        return None
    codes = np.zeros(a.shape, np.uint8)
    for v, code in G.E4M3.items():
        codes[a == v] = code
    return tf.DeviceArray.from_numpy(codes.reshape(-1), np.uint8, "row")


def _ptr(a):
    return a.ptr if a is not None else None


class Launch:
    pass


def launch(tf, c, dtype, override=None):
    """uploads the case, pre-fills y (+ guard) with the sentinel and runs the entry under the forced tile / split / family; nothing is asserted here.
    `override`: scalar arguments replaced behind the case's own (the refusals)."""
    from tinyfusers_amd.native import lib
    o = dict(override or {})
    p = G.inputs(c)
    Ho, Wo, M, C, Kc, K = G.dims(c)
    r = Launch()
    f8 = c.family == "igemm8"
    up = (lambda a: _up8(tf, a)) if f8 else (lambda a: _up(tf, a, dtype))
    r.hold = dict(x=up(p["x"]), x2=up(p["x2"]), x3=up(p["x3"]), x4=up(p["x4"]), w=up(p["w"]), bias=_up(tf, p["bias"], dtype), bias_nc=_up(tf, p["bias_nc"], dtype),
                  res=_up(tf, p["res"], dtype))
    h = r.hold
    if f8:
        h["wscale"] = tf.DeviceArray.from_numpy(np.asarray(p["wscale"] if p["wscale"] is not None else np.ones(c.Cout), np.float32), np.float32, "row")
    n = M * c.Cout
    r.dy = tf.DeviceArray.from_numpy(np.full((n + G.GUARD,), G.SENTINEL, np.float32), _el(tf, dtype), "row")
    eff = G.eff_splitk(K, c.split)
    h["ws"] = tf.DeviceArray.empty((max(c.split, eff) * M * c.Cout * 4 + 64,), np.uint8, "row")
    geo = (o.get("N", c.N), o.get("H", c.H), o.get("W", c.W), o.get("C1", c.C1), o.get("C2", c.C2), c.Cout, c.R, c.S, c.stride, o.get("pad", c.pad), o.get("ups", c.ups))
    front = (r.dy.ptr, h["x"].ptr, _ptr(h["x2"]), h["w"].ptr)
    mid = (_ptr(h["bias"]), _ptr(h["bias_nc"]), o.get("nc_stride", G.nc_stride(c)), _ptr(h["res"]), *geo, h["ws"].ptr, h["ws"].nbytes)
    with forced(c.bm, c.bn, c.split, c.dbg, c.slabs), profiled() as r.prof:
        if f8:
            r.rc = lib.tf_conv2d_fp8(*front, h["wscale"].ptr, *mid, None, 0, 0, None, tf._sh())
        else:
            r.rc = lib.tf_conv2d_fused_16(1 if dtype == "bf16" else 0, *front, *mid, _ptr(h["x3"]), _ptr(h["x4"]), c.C3, c.C4, None, 0, 0, None, tf._sh())
        r.err = lib.tf_last_error()
    full = r.dy.numpy()
    r.y, r.guard = full[:n].reshape(c.N, Ho, Wo, c.Cout), full[n:]
    return r


def _sentinel(dtype):
    """the sentinel as the 16-bit type holds it."""
    if dtype == "fp16":
        return np.float32(np.float16(G.SENTINEL))
    bits = np.float32(G.SENTINEL).view(np.uint32)
    return ((bits + np.uint32(0x7FFF) + ((bits >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)


def _report(c, y, ref):
    """the first wrong output: where it is, what covers it, and which slips would explain it."""
    Ho, Wo, M, C, Kc, K = G.dims(c)
    bad = np.argwhere(y != ref)
    img, ho, wo, ch = (int(v) for v in bad[0])
    m = (img * Ho + ho) * Wo + wo
    m0, n0 = m // c.bm * c.bm, ch // c.bn * c.bn
    match = [name for name, wrong in G.mutants(c).items() if wrong[img, ho, wo, ch] == y[img, ho, wo, ch] and wrong[img, ho, wo, ch] != ref[img, ho, wo, ch]]
    whole = [name for name, wrong in G.mutants(c).items() if np.array_equal(wrong, y)]
    return (f"{c.name}: {len(bad)} of {y.size} outputs wrong; first at (image {img}, ho {ho}, wo {wo}, channel {ch}): device {y[img, ho, wo, ch]}, reference "
            f"{ref[img, ho, wo, ch]}; tile rows [{m0}, {min(m0 + c.bm, M)}) x columns [{n0}, {min(n0 + c.bn, c.Cout)}), K ranges of the splits {G.split_ranges(K, c.split)} "
            f"(Kc = {Kc}, K = {K}); mutants matching there: {match or 'none'}; mutants matching everywhere: {whole or 'none'}; {G.predict_form(c).kernel}")


def _library_rule_agrees(c, form):
    """where the library exports the rule the aux module copies, the two answers must agree."""
    from tinyfusers_amd.native import lib
    if c.family == "igemm":
        assert lib.tf_gemm_ring_form(c.bm, c.bn, form.row[3], 0 if G.generic(c) else 1) == form.ring, (c.name, form)
    if c.family == "patch":
        assert lib.tf_conv2d_patch_admits(c.N, c.H, c.W, c.C1, c.C2, c.Cout, c.R, c.S, c.stride, c.pad, c.ups, c.C3, c.C4, c.bm, c.bn) == form.patch, (c.name, form)


@pytest.mark.parametrize("c,dtype", ROWS, ids=[f"{c.name}-{d}" for c, d in ROWS])
def test_conv_is_exact(tf, c, dtype):
    assert G.exact_cap(c, dtype)
    form = G.predict_form(c)
    Ho, Wo, M, C, Kc, K = G.dims(c)
    _library_rule_agrees(c, form)
    r = launch(tf, c, dtype)
    assert r.rc == 0, (c.name, r.rc, r.err)                                                                       # 1. the status
    assert r.prof.rows == [(M, c.Cout, K, c.R * c.S, *form.row, 1)], (c.name, r.prof.rows, form)                  # 2. the one launch, as predicted
    if form.eff == 1:                                                                                             # 3. the reduce family
        assert r.prof.reduce[0] == 0, (c.name, r.prof.reduce)
    else:
        slab = 2 if c.slabs == 16 and dtype == "fp16" and c.Cout % 8 == 0 else 4
        mn = float(M) * c.Cout
        assert r.prof.reduce == (1, mn * form.eff * slab + mn * 2.0 * (1 + (1 if c.res else 0))), (c.name, r.prof.reduce, form.eff, slab)
    s = _sentinel(dtype)
    assert (r.guard == s).all(), (c.name, "the guard behind y was written", np.flatnonzero(r.guard != s)[:8])      # 4. the guard
    assert not (r.y == s).any(), (c.name, "outputs never written", np.argwhere(r.y == s)[:4].tolist())             # 5. no sentinel left
    ref = np.asarray(G.reference(c), np.float64)
    assert np.array_equal(r.y, ref), _report(c, r.y.astype(np.float64), ref)                                      # 6. bit for bit


def test_refusals(tf):
    """launches the entry must refuse (TF_E_ARG) and families that must fail by name instead of running another kernel (TF_E_UNSUPPORTED): the status,
    the text, y untouched, nothing launched."""
    for ref in G.REFUSALS:
        r = launch(tf, ref.case, "fp16", ref.override)
        assert r.rc == ref.rc, (ref.what, r.rc, r.err)
        assert ref.says in r.err, (ref.what, r.err)
        assert r.prof.rows == [] and r.prof.reduce[0] == 0, (ref.what, r.prof.rows)
        s = _sentinel("fp16")
        assert (r.y == s).all() and (r.guard == s).all(), (ref.what, "a refused launch wrote y")


def test_patch_bit_on_a_stride_2_conv_runs_the_deep_ring(tf):
    """not a refusal: the patch family's table entry runs the deep ring where patch_setup says no -- y exact (above), the library's rule says 0."""
    from tinyfusers_amd.native import lib
    rows = [c for c in G.CASES if c.family == "patch" and c.stride == 2]
    assert rows
    for c in rows:
        assert G.predict_form(c).patch == 0 and "k_igemm<" in G.predict_form(c).kernel
        assert lib.tf_conv2d_patch_admits(c.N, c.H, c.W, c.C1, c.C2, c.Cout, c.R, c.S, c.stride, c.pad, c.ups, c.C3, c.C4, c.bm, c.bn) == 0
        assert lib.tf_conv2d_patch_admits(c.N, c.H, c.W, c.C1, c.C2, c.Cout, c.R, c.S, 1, c.pad, c.ups, c.C3, c.C4, c.bm, c.bn) == 1
