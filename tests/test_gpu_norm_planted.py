"""Every launch form of the norm kernels (csrc/norm.hip) on planted statistics, against float64, under a budget fixed on the CPU
(tests/aux/norm_planted.py; tests/test_norm_planted_host.py proves on the host that the inputs tell a wrong kernel from a right one and that the
emulated fp32 arithmetic stays within half the budget).  Every case

  * first asserts its form through the library's own rule -- tf_group_norm_geometry equals the aux module's copy of gn_geometry / gn_batches and
    shows what the case is named for (a clipped RPB, a padded block, the chunk cap, nbatch 2 / 4 / 8 with a ragged last block ...);
    tf_layer_norm_instance names the kernel of the row;
  * pre-fills the output with a finite sentinel no reference value comes near, so an element the kernel never wrote fails the comparison;
  * compares EVERY element with the float64 norm of the rounded inputs under tol = half_ulp + A (aux module docstring), float16 and bfloat16,
    and prints its largest error as a fraction of tol (pytest -s).  References are computed a batch of images at a time.

The apply entries (tf_group_norm_apply_16, tf_group_norm_apply_cat_16, tf_group_norm_apply2_f16) get partials made on the host (float64 sums
rounded to fp32, arbitrary chunk boundaries, 1 ... 4096 chunks: more than 64 loops the fold) and are held to the float64 norm under the statistics
those partials state -- the statistics part of A is dropped for them (stats = False: K_ARITH alone), so an error of the fold cannot hide behind
one of a producer.  The 8-bit outputs run at the forms their lane quads depend on under the acceptance rule of tests/test_gpu_mx8.py."""
import concurrent.futures as cf
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import norm_planted as P  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = ("fp16", "bf16")
R = P.R_MAIN
EPS = 1e-5
GN_ROWS = [c + (d, a, s) for c in P.GN_CASES for d in DTYPES for a, s in P.GN_VARIANTS]            # variants innermost: the input is made once
APPLY_ROWS = [c + (a, s) for c in P.apply_rows() for a, s in P.GN_VARIANTS]
LN_ROWS = [c + (d, a) for c in P.LN_CASES for d in DTYPES for a in (False, True)]
_pool = cf.ThreadPoolExecutor(8)


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def _np_dtype(tf, dtype):
    return tf.bfloat16 if dtype == "bf16" else np.float16


def dev(tf, x, dtype):
    return tf.DeviceArray.from_numpy(np.ascontiguousarray(x), _np_dtype(tf, dtype), "row")


def dev32(tf, x):
    return tf.DeviceArray.from_numpy(np.ascontiguousarray(x, np.float32), np.float32, "row")


def sentinel(tf, shape, dtype):
    return tf.DeviceArray.from_numpy(np.full(shape, P.SENTINEL, np.float32), _np_dtype(tf, dtype), "row")


def ptr(a):
    return a.ptr if a is not None else None


def affine(tf, C, on, dtype):
    if not on:
        return None, None, None, None
    gm, bt = P.affine(C)
    return gm, bt, dev(tf, gm, dtype), dev(tf, bt, dtype)


def geometry(N, HW, C):
    """tf_group_norm_geometry's answer; it must equal the aux module's copy of the rule (which the host test derives its cases from)."""
    from tinyfusers_amd.native import lib
    o = [ctypes.c_int(-1) for _ in range(5)]
    assert lib.tf_group_norm_geometry(N, HW, C, *[ctypes.byref(v) for v in o]) == 0
    geo = dict(zip(("rpb", "chunks", "pix_per_chunk", "apply_blocks", "nbatch"), (v.value for v in o)))
    mine = P.gn_geometry(N, HW, C)
    assert geo == {k: mine[k] for k in geo}, (geo, mine)
    return mine


def close_to_float64(got, ref_of, N, HW, C, what):
    """got (N, HW, C) float32 against ref_of(slice of images) -> (float64 reference, (tol, A)), a batch of images at a time; every element.
    Printed next to the largest error in units of tol: how much of A the error uses beyond the store rounding (tol - A), which alone is up to
    0.98 of tol for a correctly rounded kernel."""
    assert np.isfinite(got).all(), "non-finite output"

    def one(sl):
        ref, (tol, A) = ref_of(sl)
        assert np.abs(ref).max() < 100                           # (the sentinel is far from every reference value)
        err = np.abs(got[sl] - ref.reshape(got[sl].shape))
        return float((err / tol.reshape(err.shape)).max()), float(((err - (tol - A).reshape(err.shape)) / A.reshape(err.shape)).max())
    parts = list(_pool.map(one, P.image_batches(N, HW, C)))
    worst, of_a = max(p[0] for p in parts), max(p[1] for p in parts)
    print(f"\n{what}: max |err| / tol = {worst:.3f}, beyond the store rounding {max(of_a, 0.0):.3f} of A")
    assert worst <= 1.0, (what, worst)


@functools.lru_cache(maxsize=2)
def _stats(N, C, HW, G, dtype, R_):
    x, _, _ = P.gn_input(N, C, HW, G, dtype, R_)
    parts = list(_pool.map(lambda sl: P.gn_stats64(x[sl], G), P.image_batches(N, HW, C)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def run_group_norm(tf, N, C1, C2, HW, G, dtype, aff, silu, R_, what):
    from tinyfusers_amd.native import hip
    C = C1 + C2
    x, _, _ = P.gn_input(N, C, HW, G, dtype, R_)
    mean, var = _stats(N, C, HW, G, dtype, R_)
    gm, bt, dgm, dbt = affine(tf, C, aff, dtype)
    dx = dev(tf, x[..., :C1], dtype)
    dx2 = dev(tf, x[..., C1:], dtype) if C2 else None
    y = sentinel(tf, (N, HW, C), dtype)
    nb = hip.tf_group_norm_workspace(N, HW, C, G)
    ws = tf.DeviceArray.empty((nb,), np.uint8, "row")
    (hip.tf_group_norm_bf16 if dtype == "bf16" else hip.tf_group_norm_f16)(y.ptr, dx.ptr, ptr(dx2), ptr(dgm), ptr(dbt), N, HW, C1, C2, G, EPS, 1 if silu else 0,
                                                                         ws.ptr, nb, tf._sh())

    def ref_of(sl):
        ref = P.gn_apply64(x[sl], mean[sl], var[sl], G, gm, bt, silu)
        return ref, P.budget(ref, dtype, R_, 2.0 if aff else 1.0, silu)
    close_to_float64(y.numpy(), ref_of, N, HW, C, what)


@pytest.mark.parametrize("form,N,C1,C2,HW,G,dtype,aff,silu", GN_ROWS)
def test_group_norm(tf, form, N, C1, C2, HW, G, dtype, aff, silu):
    geo = geometry(N, HW, C1 + C2)
    assert P.gn_form_holds(form, geo, HW, C1, C2, G), (form, geo)
    run_group_norm(tf, N, C1, C2, HW, G, dtype, aff, silu, R, f"group norm {form} {(N, C1, C2, HW, G)} {dtype} affine={aff} silu={silu}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_group_norm_at_the_cancellation_limit(tf, dtype):
    """|mean| / std up to the largest power of two at which the emulated single-pass statistics still meet A / 2 (DESIGN.md states it as the
    accuracy limit of k_gn_stats): the device must meet tol there too."""
    form, N, C1, C2, HW, G = P.CANCELLATION_SHAPE
    Rl = P.cancellation_limit(dtype)[0]
    assert Rl > R
    assert P.gn_form_holds(form, geometry(N, HW, C1), HW, C1, C2, G)
    run_group_norm(tf, N, C1, C2, HW, G, dtype, False, False, Rl, f"group norm at R = {Rl} {dtype}")


def host_partials(tf, x, N, C1, C2, HW, G, g1, g2, chunks, chunks2):
    """partials() of x (or of each source of a pair) uploaded, and the (mean, var) they state."""
    C = C1 + C2
    if not C2:
        part = np.concatenate([P.partials(x[sl], G, chunks) for sl in P.image_batches(N, HW, C)])
        return (dev32(tf, part), None), P.stats_from_partials(part, HW, C // G)
    sub = C1 // g1
    mr = (C // G) // sub
    p1 = np.concatenate([P.partials(np.ascontiguousarray(x[sl][..., :C1]), g1, chunks) for sl in P.image_batches(N, HW, C)])
    p2 = np.concatenate([P.partials(np.ascontiguousarray(x[sl][..., C1:]), g2, chunks2) for sl in P.image_batches(N, HW, C)])
    return (dev32(tf, p1), dev32(tf, p2)), P.cat_stats(p1, p2, HW, sub, mr)


def assert_apply_form(entry, N, C1, C2, HW, G, g1):
    geo = geometry(N, HW, C1 + C2)
    assert geo["nbatch"] == (2 if N >= 200 else 1), geo
    if C2:
        mr = ((C1 + C2) // G) // (C1 // g1)
        assert mr == {"apply2": 2, "cat": 3 if C2 != C1 else 8}[entry]
        assert entry != "cat" or mr == 8 or g1 % mr != 0         # mr = 3: a group straddles the two tables
    return geo


@pytest.mark.parametrize("entry,N,C1,C2,HW,G,g1,g2,chunks,chunks2,dtype,aff,silu", APPLY_ROWS)
def test_apply_on_host_partials(tf, entry, N, C1, C2, HW, G, g1, g2, chunks, chunks2, dtype, aff, silu):
    from tinyfusers_amd.native import hip
    assert_apply_form(entry, N, C1, C2, HW, G, g1)
    C = C1 + C2
    x, _, _ = P.gn_input(N, C, HW, G, dtype)
    (dp1, dp2), (mean, var) = host_partials(tf, x, N, C1, C2, HW, G, g1, g2, chunks, chunks2)
    gm, bt, dgm, dbt = affine(tf, C, aff, dtype)
    dx = dev(tf, x[..., :C1], dtype)
    dx2 = dev(tf, x[..., C1:], dtype) if C2 else None
    y = sentinel(tf, (N, HW, C), dtype)
    tag = 1 if dtype == "bf16" else 0
    if entry == "apply":
        hip.tf_group_norm_apply_16(tag, y.ptr, dx.ptr, ptr(dgm), ptr(dbt), dp1.ptr, chunks, N, HW, C, G, EPS, 1 if silu else 0, tf._sh())
    elif entry == "cat":
        hip.tf_group_norm_apply_cat_16(tag, y.ptr, dx.ptr, dx2.ptr, ptr(dgm), ptr(dbt), dp1.ptr, chunks, g1, dp2.ptr, chunks2, g2, N, HW, C1, C2, G, EPS,
                                       1 if silu else 0, tf._sh())
    else:
        assert entry == "apply2" and dtype == "fp16" and g1 == g2 == G and C1 == C2
        hip.tf_group_norm_apply2_f16(y.ptr, dx.ptr, dx2.ptr, ptr(dgm), ptr(dbt), dp1.ptr, chunks, dp2.ptr, chunks2, N, HW, C1, G, EPS, 1 if silu else 0, tf._sh())

    def ref_of(sl):
        ref = P.gn_apply64(x[sl], mean[sl], var[sl], G, gm, bt, silu)
        return ref, P.budget(ref, dtype, R, 2.0 if aff else 1.0, silu, stats=False)         # the partials are exact to fp32: no statistics part
    close_to_float64(y.numpy(), ref_of, N, HW, C, f"{entry} {(N, C1, C2, HW, G)} chunks {chunks} / {chunks2} {dtype} affine={aff} silu={silu}")


@pytest.mark.parametrize("form,rows,C,dtype,aff", LN_ROWS)
def test_layer_norm(tf, form, rows, C, dtype, aff):
    from tinyfusers_amd.native import hip, lib
    assert P.LN_INSTANCES[lib.tf_layer_norm_instance(rows, C)] == form == P.ln_instance(rows, C)
    x, _, _ = P.ln_input(rows, C, dtype)
    gm, bt, dgm, dbt = affine(tf, C, aff, dtype)
    dx, y = dev(tf, x, dtype), sentinel(tf, (rows, C), dtype)
    (hip.tf_layer_norm_bf16 if dtype == "bf16" else hip.tf_layer_norm_f16)(y.ptr, dx.ptr, ptr(dgm), ptr(dbt), rows, C, EPS, tf._sh())
    got = y.numpy().reshape(rows, 1, C)

    def ref_of(sl):
        ref = P.ln_ref64(x[sl], gm, bt)
        return ref, P.budget(ref, dtype, R, 2.0 if aff else 1.0)
    close_to_float64(got, ref_of, rows, 1, C, f"layer norm <{form}> {(rows, C)} {dtype} affine={aff}")


# ---- 8-bit outputs ------------------------------------------------------------------------------------------------------------------------------
SENTINEL_BYTE = 0x7E       # e4m3 448; as a scale byte 2^-1: a block left unwritten dequantises to 224


def out8(tf, n, mx):
    return tf.DeviceArray.from_numpy(np.full((n + (n // 32 if mx else 0),), SENTINEL_BYTE, np.uint8), np.uint8, "row")


def download8(tf, a, rows, C, mx):
    """the dequantised (rows, C) float64 values of an 8-bit output buffer."""
    from tinyfusers_amd.native import hip
    hip.tf_stream_sync(tf._sh())
    host = np.empty((a.size,), np.uint8)
    hip.tf_memcpy(host.ctypes.data, a.ptr, host.size, 2)
    n = rows * C
    deq = P.decode_e4m3(host[:n]).reshape(rows, C)
    if mx:
        deq = (deq.reshape(rows, C // 32, 32) * np.exp2(host[n:].astype(np.float64) - 127.0).reshape(rows, C // 32, 1)).reshape(rows, C)
    return deq


def accept8(deq, want, mx, what):
    """tests/test_gpu_mx8.py's rule: every element within one e4m3 step of its block, under 3 % of the elements differ at all."""
    assert np.isfinite(deq).all()
    ok, share, _ = P.close8(deq, want, 32 if mx else 0)
    print(f"\n{what}: share of elements that differ from the quantised float64 reference = {share:.5f}")
    assert ok and share < 0.03, (what, share)


@pytest.mark.parametrize("mx", (True, False))
@pytest.mark.parametrize("form,rows,C", P.LN8_CASES)
def test_layer_norm_8bit(tf, form, rows, C, mx):
    from tinyfusers_amd.native import hip, lib
    assert P.LN_INSTANCES[lib.tf_layer_norm_instance(rows, C)] == form
    x, _, _ = P.ln_input(rows, C, "fp16")
    gm, bt, dgm, dbt = affine(tf, C, True, "fp16")
    dx, y = dev(tf, x, "fp16"), out8(tf, rows * C, mx)
    (hip.tf_layer_norm_mx8 if mx else hip.tf_layer_norm_fp8)(y.ptr, dx.ptr, dgm.ptr, dbt.ptr, rows, C, EPS, tf._sh())
    ref = P.ln_ref64(x, gm, bt)
    accept8(download8(tf, y, rows, C, mx), P.mx_quant(ref) if mx else P.e4m3(ref), mx, f"layer norm <{form}> {'mx8' if mx else 'fp8'}")


@pytest.mark.parametrize("mx", (True, False))
@pytest.mark.parametrize("entry,N,C1,C2,HW,G,g1,g2,chunks,chunks2", P.GN8_CASES)
def test_group_norm_apply_8bit(tf, entry, N, C1, C2, HW, G, g1, g2, chunks, chunks2, mx):
    from tinyfusers_amd.native import hip
    geo = geometry(N, HW, C1 + C2)
    assert geo["nbatch"] == 2 and (not C2 or (((C1 + C2) // G) // (C1 // g1) == 3 and g1 % 3 != 0))
    C = C1 + C2
    x, _, _ = P.gn_input(N, C, HW, G, "fp16")
    (dp1, dp2), (mean, var) = host_partials(tf, x, N, C1, C2, HW, G, g1, g2, chunks, chunks2)
    gm, bt, dgm, dbt = affine(tf, C, True, "fp16")
    dx = dev(tf, x[..., :C1], "fp16")
    dx2 = dev(tf, x[..., C1:], "fp16") if C2 else None
    y = out8(tf, N * HW * C, mx)
    (hip.tf_group_norm_apply_mx8 if mx else hip.tf_group_norm_apply_fp8)(y.ptr, dx.ptr, ptr(dx2), dgm.ptr, dbt.ptr, dp1.ptr, chunks, g1, ptr(dp2), chunks2, g2,
                                                                         N, HW, C1, C2, G, EPS, 1, tf._sh())
    quant = P.mx_quant if mx else P.e4m3
    want = np.concatenate(list(_pool.map(lambda sl: quant(P.gn_apply64(x[sl], mean[sl], var[sl], G, gm, bt, True).reshape(-1, C)), P.image_batches(N, HW, C))))
    accept8(download8(tf, y, N * HW, C, mx), want, mx, f"group norm apply {entry} {(N, C1, C2, HW, G)} {'mx8' if mx else 'fp8'}")
