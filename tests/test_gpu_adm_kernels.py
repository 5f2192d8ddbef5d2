"""csrc/adm.hip on the device, bit for bit: tf_adm_vector_16 (pooled bits copied; the Fourier part the bits tf_timestep_embedding_* writes for the
same scalar, and inside that kernel's float64 budget -- tests/aux/elementwise_planted.py::embed_ref), tf_adm_emb_rows_16 (fp32 add, one rounding, against
numpy), tf_gather_rows_16 (bits moved), and tf_gemv_rows_16 (every row the bits tf_gemv_16 gives it).  Outputs sit in front of a guard."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "aux"))

import elementwise_planted as P  # noqa: E402
from test_gpu_elementwise_planted import _exact16, _hip, _lib, _within, down, out16, up  # noqa: E402

pytestmark = pytest.mark.gpu
F32, U16 = np.float32, np.uint16
DT = {"fp16": 0, "bf16": 1}
IDS = (0.0, 1.0, 1024.0, 4095.5, 512.0, 7.25)


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def _values(rng, shape, dtype):
    """fp32 values that the 16-bit type holds exactly, with signed zeros, the largest finite value and a subnormal among them."""
    x = rng.standard_normal(shape).astype(F32) * F32(3.0)
    flat = x.reshape(-1)
    flat[:4] = [0.0, -0.0, 60000.0 if dtype == "fp16" else 3.0e38, 2.0 ** -20]
    return P.to_f32(P.to_bits(x, dtype), dtype)


@pytest.mark.parametrize("dtype", ("fp16", "bf16"))
@pytest.mark.parametrize("R,Pw,D", [(1, 64, 32), (3, 1280, 256), (2, 8, 2)])
def test_adm_vector(tf, dtype, R, Pw, D):
    hip = _hip()
    rng = np.random.default_rng(R * 1000 + Pw)
    pooled = P.to_bits(_values(rng, (R, Pw), dtype), dtype)
    pooled.reshape(-1)[5 % pooled.size] = 0x7E01 if dtype == "fp16" else 0x7FC1          # a NaN payload: copied, not rounded
    ids = np.array([[IDS[(r + k) % len(IDS)] for k in range(6)] for r in range(R)], F32)
    assert {0.0, 1.0, 1024.0, 4095.5} <= set(ids.ravel().tolist())
    W = Pw + 6 * D
    y = out16(tf, R * W, dtype)
    dp, di = up(tf, pooled), up(tf, ids)                 # (held: a handle that is dropped gives its block back to the pool)
    hip.tf_adm_vector_16(DT[dtype], y.ptr, dp.ptr, di.ptr, R, Pw, D, P.MAX_PERIOD, tf._sh())
    got = y.get("tf_adm_vector_16").reshape(R, W)
    assert np.array_equal(got[:, :Pw], pooled.reshape(R, Pw)), "pooled bits"
    entry = "tf_timestep_embedding_f16" if dtype == "fp16" else "tf_timestep_embedding_bf16"
    for r in range(R):
        for k in range(6):
            t = float(ids[r, k])
            e = out16(tf, D, dtype)
            params = up(tf, np.array([t, 0.5, 0.6, 7.5], F32))
            getattr(hip, entry)(e.ptr, params.ptr, D, P.MAX_PERIOD, tf._sh())
            part = got[r, Pw + k * D:Pw + (k + 1) * D]
            assert np.array_equal(part, e.get(entry)), f"row {r} id {k} (t = {t}): not the bits of {entry}"
            ref, A, tol = P.embed_ref(D, t, dtype)
            _within(P.to_f32(part, dtype), ref, tol, A, "tf_adm_vector_16", f"tf_adm_vector_16 {(R, Pw, D)} row {r} id {k} t {t}")


def test_adm_vector_refusals(tf):
    lib = _lib()
    y = out16(tf, 64)
    a, b = up(tf, np.zeros(64, U16)), up(tf, np.zeros(6, F32))
    for args in ((0, 8, 2), (1, 8, 3), (1, 8, 0), (1, -1, 2)):
        assert lib.tf_adm_vector_16(0, y.ptr, a.ptr, b.ptr, *args, 10000.0, tf._sh()) == P.TF_E_ARG, args
    assert lib.tf_adm_vector_16(2, y.ptr, a.ptr, b.ptr, 1, 8, 2, 10000.0, tf._sh()) == P.TF_E_ARG
    assert lib.tf_adm_vector_16(0, y.ptr, a.ptr, b.ptr, 1, 8, 2, 0.0, tf._sh()) == P.TF_E_ARG
    y.untouched("tf_adm_vector_16 refused")


@pytest.mark.parametrize("dtype", ("fp16", "bf16"))
@pytest.mark.parametrize("S,R,E", [(s, r, e) for e in (8, 256) for s in (1, 3) for r in (1, 2, 5)] + [(s, r, 1280) for s in (1, 3) for r in (1, 5)])
def test_adm_emb_rows(tf, dtype, S, R, E):
    hip = _hip()
    rng = np.random.default_rng(S * 100 + R * 10 + E)
    t, y = _values(rng, (S, E), dtype), _values(rng, (R, E), dtype)
    with np.errstate(over="ignore"):                              # (the two largest finite values add up to infinity, on the device too)
        want = P.to_bits((t[:, None, :] + y[None, :, :]).astype(F32).reshape(S * R, E), dtype)     # exact operands, one fp32 add, one rounding
    out = out16(tf, S * R * E, dtype)
    dt_, dy = up(tf, P.to_bits(t, dtype)), up(tf, P.to_bits(y, dtype))
    hip.tf_adm_emb_rows_16(DT[dtype], out.ptr, dt_.ptr, dy.ptr, S, R, E, tf._sh())
    _exact16(out.get("tf_adm_emb_rows_16"), want, dtype, f"tf_adm_emb_rows_16 {(S, R, E)} {dtype}")


def test_adm_emb_rows_refusals(tf):
    lib = _lib()
    out = out16(tf, 64)
    a, b = up(tf, np.zeros(64, U16)), up(tf, np.zeros(64, U16))
    for args in ((1, 1, 12), (1, 1, 0), (0, 1, 8), (1, 0, 8)):
        assert lib.tf_adm_emb_rows_16(0, out.ptr, a.ptr, b.ptr, *args, tf._sh()) == P.TF_E_ARG, args
    assert lib.tf_adm_emb_rows_16(0, out.ptr, a.ptr + 2, b.ptr, 1, 1, 8, tf._sh()) == P.TF_E_ARG        # off the 16-byte grid
    assert lib.tf_adm_emb_rows_16(3, out.ptr, a.ptr, b.ptr, 1, 1, 8, tf._sh()) == P.TF_E_ARG
    out.untouched("tf_adm_emb_rows_16 refused")


@pytest.mark.parametrize("B,W,rows,idx", [(4, 64, 7, (3, 0, 3, 6)), (1, 8, 1, (0,)), (3, 1280, 154, (153, 0, 77)), (2, 16, 5, (-1, 5))])
def test_gather_rows(tf, B, W, rows, idx):
    hip = _hip()
    src = np.random.default_rng(B + W).integers(0, 1 << 16, (rows, W)).astype(U16)       # any bit pattern: NaNs and infinities move too
    out = out16(tf, B * W)
    dsrc, didx = up(tf, src), up(tf, np.array(idx, np.int32))
    hip.tf_gather_rows_16(out.ptr, dsrc.ptr, didx.ptr, B, W, rows, tf._sh())
    want = np.stack([src[i] if 0 <= i < rows else np.zeros(W, U16) for i in idx])        # an index outside the source: a row of zeros, nothing read
    assert np.array_equal(out.get("tf_gather_rows_16").reshape(B, W), want)
    lib = _lib()
    out = out16(tf, B * W)
    assert lib.tf_gather_rows_16(out.ptr, dsrc.ptr, didx.ptr, B, 12, rows, tf._sh()) == P.TF_E_ARG
    out.untouched("tf_gather_rows_16 refused")


@pytest.mark.parametrize("dtype", ("fp16", "bf16"))
@pytest.mark.parametrize("M,N,K", [(1, 5, 8), (8, 64, 64), (9, 6, 72), (23, 130, 256), (40, 64, 1280)])
def test_gemv_rows_is_gemv_row_for_row(tf, dtype, M, N, K):
    hip = _hip()
    rng = np.random.default_rng(M * N + K)
    x, w, b = (P.to_f32(P.to_bits(v.astype(F32), dtype), dtype) for v in (rng.standard_normal((M, K)), rng.standard_normal((N, K)) / np.sqrt(K), rng.standard_normal(N)))
    dx, dw, db = (up(tf, P.to_bits(v, dtype)) for v in (x, w, b))
    for silu in (0, 1):
        got = out16(tf, M * N, dtype)
        hip.tf_gemv_rows_16(DT[dtype], got.ptr, dx.ptr, dw.ptr, db.ptr, M, N, K, silu, tf._sh())
        want = np.empty((M, N), U16)
        for m0 in range(0, M, 8):                               # tf_gemv_16 on each group of 8 rows
            m = min(8, M - m0)
            part = out16(tf, m * N, dtype)
            hip.tf_gemv_16(DT[dtype], part.ptr, dx.ptr + m0 * K * 2, dw.ptr, db.ptr, m, N, K, silu, tf._sh())
            want[m0:m0 + m] = part.get("tf_gemv_16").reshape(m, N)
        g = got.get("tf_gemv_rows_16").reshape(M, N)
        assert np.array_equal(g, want), f"tf_gemv_rows_16 {(M, N, K)} silu {silu}: {int((g != want).sum())} elements differ"
        x64 = x.astype(np.float64)
        ref = (x64 / (1 + np.exp(-x64)) if silu else x64) @ w.astype(np.float64).T + b          # (the bits above are the check; this says they are a GEMV)
        assert np.abs(P.to_f32(g, dtype) - ref).max() <= (2.0 ** -7 if dtype == "bf16" else 2.0 ** -10) * (1 + np.abs(ref).max())
    lib = _lib()
    got = out16(tf, 64, dtype)
    for args in ((0, 4, 8), (1, 0, 8), (1, 4, 12), (1, 4, 0), ((1 << 16) + 1, 4, 8)):
        assert lib.tf_gemv_rows_16(DT[dtype], got.ptr, dx.ptr, dw.ptr, db.ptr, *args, 0, tf._sh()) == P.TF_E_ARG, args
    got.untouched("tf_gemv_rows_16 refused")
