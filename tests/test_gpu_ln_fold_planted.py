"""The LayerNorm fold of every GEMM family -- tf_linear_ln_16 on k_igemm (deep, wide and all-8 ring over seven tiles), k_igemm_pp (five tiles),
k_gemm_c4, k_gemm_c8 (both tile orders, the chunked walk) and k_gemm_ar, float16 and bfloat16 -- and tf_ln_fold_weights_16, through the C ABI on
planted row statistics, against float64, under budgets fixed on the CPU (tests/aux/ln_fold_planted.py; tests/test_ln_fold_planted_host.py proves on
the host that the inputs tell a slipped kernel from a right one and that the emulated fp32 arithmetic stays within half the budgets).

Every launch runs on operands the DEVICE folded (w', bias' and colsum of tf_ln_fold_weights_16, downloaded for the reference: the entry's contract is
on what it is given) and is checked in this order: the status; tf_prof_dump shows exactly one GEMM launch of the predicted (M, N, K, 1, bm, bn, 1,
variant) and tf_prof_read_family no reduce launch (the ring forms are also asked of tf_gemm_ring_form); the 64-element guard behind y still holds
the sentinel; no sentinel is left in y; y is finite; |y - reference| <= tol on every element.  A failure names the first bad (row, column), the
row's planted (mu, sigma), its tile, and the mutants of the aux module the output matches there and everywhere.  The largest error of a launch as
a fraction of tol is printed (pytest -s).  The two chunked-walk shapes are the smallest that give k_gemm_c4 / k_gemm_c8 chunks of 2 and 4 tiles
on 256 CUs and are the only launches that are not small.

Measured on an MI355X: the 249 tests of this file take 37 s of wall time, host references included -- under 0.2 s per small launch, 2 - 3 s
(M = 27600) and 6 s (M = 55200) for the chunked-walk shapes, nearly all of it the float64 reference on the host.  Every launch is within tol; the
largest share of A an error uses beyond the store rounding is 0.15 (k_igemm_pp 192 x 128, float16 at R = 256), the emulation's bound being 0.5."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import ln_fold_planted as L  # noqa: E402
from test_gpu_conv_stats_planted import forced, profiled  # noqa: E402

pytestmark = pytest.mark.gpu

_FOLDED, _PROBLEM = {}, {}


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def _np_dtype(tf, dtype):
    return tf.bfloat16 if dtype == "bf16" else np.float16


def dev(tf, x, dtype):
    return tf.DeviceArray.from_numpy(np.ascontiguousarray(x).reshape(-1), _np_dtype(tf, dtype), "row") if x is not None else None


def sentinel(tf, n, dtype):
    return tf.DeviceArray.from_numpy(np.full((n,), L.SENTINEL, np.float32), _np_dtype(tf, dtype), "row")


def sentinel_value(dtype):
    return L.round16(np.float32([L.SENTINEL]), dtype)[0]


def ptr(a):
    return a.ptr if a is not None else None


def tag(dtype):
    return 1 if dtype == "bf16" else 0


def fold_on_device(tf, w, bias, gamma, beta, dtype, guard=0):
    """tf_ln_fold_weights_16 -> device (w', bias', colsum), each followed by `guard` sentinel elements."""
    from tinyfusers_amd.native import lib
    Np, K = w.shape
    dwf, dbf = sentinel(tf, Np * K + guard, dtype), sentinel(tf, Np + guard, dtype)
    dcs = tf.DeviceArray.from_numpy(np.full((Np + guard,), L.SENTINEL, np.float32), np.float32, "row")
    hold = [dev(tf, v, dtype) for v in (w, bias, gamma, beta)]
    rc = lib.tf_ln_fold_weights_16(tag(dtype), dwf.ptr, dbf.ptr, dcs.ptr, hold[0].ptr, ptr(hold[1]), hold[2].ptr, hold[3].ptr, Np, K, tf._sh())
    assert rc == 0, (rc, lib.tf_last_error())
    return dwf, dbf, dcs


def folded(tf, Np, K, dtype):
    """the folded operands of a case's weights: device arrays for the launch, their downloads for the reference (kept per (Np, K, type))."""
    key = (Np, K, dtype)
    if key not in _FOLDED:
        if len(_FOLDED) > 12:
            _FOLDED.clear()
        w, bias = L.weights(Np, K, dtype)
        d = fold_on_device(tf, w, bias, *L.affine(K), dtype)
        _FOLDED[key] = d + (d[0].numpy().reshape(Np, K), d[1].numpy())
    return _FOLDED[key]


def problem(c, dtype, wf, bf):
    key = L.data_key(c) + (dtype,)
    if key not in _PROBLEM:
        _PROBLEM.clear()                                       # (one at a time: the chunked-walk problems are large, c4 / c8 pairs share one)
        _PROBLEM[key] = L.Problem(c, dtype, wf, bf)
    pb = _PROBLEM[key]
    pb.case, pb._alt = c, None                                 # (the stale-chunk mutant depends on the tile height)
    return pb


def run(tf, c, dtype):
    from tinyfusers_amd.native import lib
    what = f"{L.case_id(c)} {dtype} R={c.R}"
    Np = L.packed_width(c)
    dwf, dbf, dcs, wf, bf = folded(tf, Np, c.K, dtype)
    pb = problem(c, dtype, wf, bf)
    dx, dr = dev(tf, pb.x, dtype), dev(tf, pb.res, dtype)
    n = c.M * c.N
    dy = sentinel(tf, n + L.GUARD, dtype)
    form = L.predict_form(c)
    if c.family == "ring":                                     # the ring the bit asks for is the ring this tile runs
        assert lib.tf_gemm_ring_form(c.bm, c.bn, form[3], 1) == form[3] == L.ring_form(c.bm, c.bn, L.family_bit(c)), what
    with forced(c.bm, c.bn, 1 if c.bm else 0, c.dbg), profiled() as pr:
        rc = lib.tf_linear_ln_16(tag(dtype), dy.ptr, dx.ptr, dwf.ptr, dbf.ptr, dcs.ptr, ptr(dr), c.M, c.N, c.K, c.act, L.EPS, tf._sh())
    assert rc == 0, (what, rc, lib.tf_last_error())                                                    # 1. the status
    if form is not None:                                                                               # 2. the launch
        assert pr.rows == [(c.M, Np, c.K, 1) + form + (1,)], (what, pr.rows)
    else:
        assert len(pr.rows) == 1 and pr.rows[0][:4] == (c.M, Np, c.K, 1) and pr.rows[0][6] == 1 and pr.rows[0][8] == 1, (what, pr.rows)
    assert pr.reduce[0] == 0, (what, pr.reduce)
    out = dy.numpy()
    s = sentinel_value(dtype)
    assert (out[n:] == s).all(), (what, "the guard behind y was written")                                # 3. the guard
    y = out[:n].reshape(c.M, c.N)
    left = np.argwhere(y == s)
    assert len(left) == 0, (what, f"{len(left)} elements never written, the first at {tuple(left[0])}")   # 4. every element written
    worst, of_a, report = L.check_output(pb, y)
    assert np.isfinite(y).all(), (what, "non-finite output", report)                                    # 5. finite
    print(f"\n{what}: max |err| / tol = {worst:.3f}, beyond the store rounding {max(of_a, 0.0):.3f} of A" + (f" on {pr.rows[0][4:8]}" if form is None else ""))
    assert report is None, report                                                                       # 6. within tol, everywhere


@pytest.mark.parametrize("dtype", L.DTYPES)
@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_folded_linear(tf, c, dtype):
    run(tf, c, dtype)


@pytest.mark.parametrize("dtype", L.DTYPES)
@pytest.mark.parametrize("c", L.CHUNK_CASES, ids=L.case_id)
def test_chunked_walk(tf, c, dtype):
    """a block walks 2 (M = 27600) or 4 (M = 55200) consecutive tiles and keeps a row block's statistics for the following tiles of the chunk
    (stat_m0); 19 column tiles: chunks straddle row blocks.  Every row block has planted statistics of its own."""
    run(tf, c, dtype)


@pytest.mark.parametrize("dtype", L.DTYPES)
@pytest.mark.parametrize("c", L.R_LIMIT_CASES, ids=L.case_id)
def test_r_limit(tf, c, dtype):
    """|mean| / sigma at the last R the emulation meets the R_MAIN constants at (aux module docstring), once per family."""
    run(tf, c._replace(R=L.R_LIMIT[dtype]), dtype)


@pytest.mark.parametrize("dtype", L.DTYPES)
@pytest.mark.parametrize("with_bias", (True, False))
@pytest.mark.parametrize("N,K", L.FOLD_CASES)
def test_fold_weights(tf, N, K, with_bias, dtype):
    """tf_ln_fold_weights_16: w' bit for bit, colsum and bias' within their budgets of the float64 sums, nothing written beyond N."""
    w, bias = L.weights(N, K, dtype)
    bias = bias if with_bias else None
    gamma, beta = L.affine(K)
    dwf, dbf, dcs = fold_on_device(tf, w, bias, gamma, beta, dtype, L.GUARD)
    wf, cs, bf, cs_tol, bf_tol, _ = L.fold64(w, bias, gamma, beta, dtype)
    got_w, got_b, got_cs = dwf.numpy(), dbf.numpy(), dcs.numpy()
    s = sentinel_value(dtype)
    assert (got_w[N * K:] == s).all() and (got_b[N:] == s).all() and (got_cs[N:] == np.float32(L.SENTINEL)).all(), "written beyond N"
    assert np.array_equal(got_w[:N * K].view(np.uint32), wf.reshape(-1).view(np.uint32)), "w' differs from round16(w gamma)"
    assert np.isfinite(got_cs[:N]).all() and np.isfinite(got_b[:N]).all()
    rc, rb = float((np.abs(got_cs[:N] - cs) / cs_tol).max()), float((np.abs(got_b[:N] - bf) / bf_tol).max())
    print(f"\nk_ln_fold ({N}, {K}) {dtype} bias {with_bias}: colsum {rc:.3f}, bias' {rb:.3f} of tol")
    assert rc <= 1.0 and rb <= 1.0, (rc, rb)


@pytest.mark.parametrize("row", L.REFUSALS, ids=lambda r: r[0].replace(" ", "_"))
def test_refusals(tf, row):
    """the entry's argument errors, and a forced family that cannot take the fold: each fails by name, and y is untouched."""
    from tinyfusers_amd.native import lib
    what, M, N, K, act, bm, bn, dbg, with_colsum, status, word = row
    Np = 2 * N if act else N
    z = np.zeros(max(M * K, Np * K), np.float32)
    dx, dw, db = dev(tf, z[:M * K], "fp16"), dev(tf, z[:Np * K], "fp16"), dev(tf, z[:Np], "fp16")
    dcs = tf.DeviceArray.from_numpy(z[:Np], np.float32, "row")
    dy = sentinel(tf, M * N + L.GUARD, "fp16")
    with forced(bm, bn, 1 if bm else 0, dbg):
        rc = lib.tf_linear_ln_16(0, dy.ptr, dx.ptr, dw.ptr, db.ptr, dcs.ptr if with_colsum else None, None, M, N, K, act, L.EPS, tf._sh())
    err = lib.tf_last_error()
    assert rc == status and word in err, (what, rc, err)
    assert (dy.numpy() == sentinel_value("fp16")).all(), (what, "y was written")
