"""Every C entry of csrc/elementwise.hip on the tables of tests/aux/elementwise_planted.py (tests/test_elementwise_planted_host.py proves on the
host that those inputs tell a wrong kernel from a right one and that the emulated fp32 arithmetic stays within half of every budget).

  * Copies, single IEEE fp32 operations and conversions are compared BIT FOR BIT (NaN as NaN): all 65536 patterns of the 16-bit kernels, position
    codes for the re-layouts and gathers.  Activations, GEGLU, the softmaxes, the timestep embedding and the DDIM update are held to float64 under
    tol = half_ulp + A (aux module docstring; K comes from the host emulation, never from a device).
  * Every grid-stride kernel has a case past one trip of its capped grid (4194304 / 524288 elements, 64 x 256 16-byte units, 256 frequencies).
  * Every output is pre-filled with a finite sentinel and ends in a guard that must come back untouched; both are checked before the values.
  * Null pointers, negative extents and widths off the vector grid must return TF_E_ARG and leave the output alone.
The last test prints the worst error / tolerance per budgeted entry (pytest -s)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import elementwise_planted as P  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64, U16 = np.float32, np.float64, np.uint16
WORST = {}


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def _hip():
    from tinyfusers_amd.native import hip
    return hip


def _lib():
    from tinyfusers_amd.native import lib
    return lib


def up(tf, host):
    """host array -> device bytes (at least 16, 256-byte aligned by the pool)."""
    host = np.ascontiguousarray(host)
    a = tf.DeviceArray.empty((max(host.nbytes, 16),), np.uint8, "row")
    if host.nbytes:
        _hip().tf_memcpy(a.ptr, host.ctypes.data, host.nbytes, tf.H2D)
    return a


def down(tf, a, n, dtype):
    _hip().tf_stream_sync(tf._sh())
    host = np.empty(n, dtype)
    if host.nbytes:
        _hip().tf_memcpy(host.ctypes.data, a.ptr, host.nbytes, tf.D2H)
    return host


class Out:
    """n elements of a sentinel plus the guard, on the device; get() checks the guard and returns the n elements."""

    def __init__(self, tf, n, dtype, sentinel):
        self.tf, self.n, self.dtype, self.sentinel = tf, int(n), np.dtype(dtype), np.array(sentinel).astype(dtype)
        self.dev = up(tf, np.full(self.n + P.GUARD, self.sentinel, dtype))
        self.ptr = self.dev.ptr

    def get(self, what=""):
        host = down(self.tf, self.dev, self.n + P.GUARD, self.dtype)
        assert (host[self.n:].view(np.uint8) == np.full(P.GUARD, self.sentinel, self.dtype).view(np.uint8)).all(), f"{what}: guard behind the output overwritten"
        return host[:self.n]

    def untouched(self, what=""):
        got = self.get(what)
        assert (got.view(np.uint8) == np.full(self.n, self.sentinel, self.dtype).view(np.uint8)).all(), f"{what}: output written"


def out16(tf, n, dtype="fp16"):
    return Out(tf, n, U16, P.SENT16[dtype])


def out32(tf, n):
    return Out(tf, n, F32, P.SENT32)


def _note(entry, ratio, of_a):
    """largest |err| / tol, and largest share of A used beyond the store rounding (tol - A; an fp32 output has none)."""
    r0, a0 = WORST.get(entry, (0.0, 0.0))
    WORST[entry] = (max(r0, float(ratio)), max(a0, float(of_a)))


def _exact16(got, want, dtype, what):
    ok = P.same_bits(got, want.reshape(got.shape), dtype)
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} differ, first at {int(np.flatnonzero(~ok.ravel())[0])}"


def _exact32(got, want, what):
    ok = P.same_f32(got, np.ascontiguousarray(want, F32).reshape(got.shape))
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} differ, first at {int(np.flatnonzero(~ok.ravel())[0])}"


def _within(got, y, tol, A, entry, what):
    got = np.asarray(got, F64).reshape(y.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err = np.abs(got - y)
    ratio = float((err / tol).max())
    ok = A > 0
    _note(entry, ratio, max(0.0, float(((err - (tol - A))[ok] / A[ok]).max())))
    assert ratio <= 1.0, (what, ratio)


# ---- Group A ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,kind,din,dout,tag", P.A_ENTRIES)
def test_group_a_16bit_unary_and_binary(tf, entry, kind, din, dout, tag):
    hip = _hip()
    fn = getattr(hip, entry)
    for case in ("patterns",) + P.A_LENGTHS:
        a, b = P.a_inputs(case, din)
        n = len(a)
        y = out16(tf, n, dout)
        da = up(tf, a)
        if kind == "add":
            db = up(tf, b)
            args = (y.ptr, da.ptr, db.ptr, n, tf._sh())
            fn(*(((tag,) + args) if tag is not None else args))
        else:
            fn(y.ptr, da.ptr, n, tf._sh())
        what = f"{entry} {din} {case}"
        got = y.get(what)
        if kind in P.ACTS:
            ratio, of_a = P.check_act(kind, din, a, got)
            _note(entry, ratio, of_a)
            assert ratio <= 1.0, (what, ratio)
        else:
            _exact16(got, P.a_exact(kind, a, b, din, dout), dout, what)


# ---- Group B ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", P.B_ENTRIES)
def test_group_b_casts_and_decode_tail(tf, entry):
    hip = _hip()
    scales = P.B_SCALES if entry in ("tf_scale_cast_f32_to_f16", "tf_scale_f32") else (None,)
    for case in ("all",) + P.B_LENGTHS:
        x = P.b_input(entry, case)
        n = len(x)
        for sc in scales:
            what = f"{entry} {case} scale {sc}"
            want = P.b_reference(entry, x, sc)
            if entry == "tf_scale_f32":                                  # in place
                buf = Out(tf, n, F32, P.SENT32)
                hip.tf_memcpy(buf.ptr, x.ctypes.data, x.nbytes, tf.H2D)
                hip.tf_scale_f32(buf.ptr, float(sc), n, tf._sh())
                _exact32(buf.get(what), want, what)
                continue
            dx = up(tf, x)
            if entry == "tf_cast_f16_to_f32":
                y = out32(tf, n)
                hip.tf_cast_f16_to_f32(y.ptr, dx.ptr, n, tf._sh())
                _exact32(y.get(what), want, what)
            elif entry == "tf_image_to_u8":
                y = Out(tf, n, np.uint8, P.SENT8)
                hip.tf_image_to_u8(y.ptr, dx.ptr, n, tf._sh())
                got = y.get(what)
                assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} differ"
            else:
                y = out16(tf, n)
                if entry == "tf_cast_f32_to_f16":
                    hip.tf_cast_f32_to_f16(y.ptr, dx.ptr, n, tf._sh())
                else:
                    hip.tf_scale_cast_f32_to_f16(y.ptr, dx.ptr, float(sc), n, tf._sh())
                _exact16(y.get(what), want, "fp16", what)


# ---- Group C ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", P.TILE_ENTRIES)
@pytest.mark.parametrize("N,C,HW", P.TILE_CASES)
def test_group_c_tile_relayouts(tf, entry, N, C, HW):
    src, want = P.tile_case(entry, N, C, HW)
    H, W = (HW // 5, 5) if HW % 5 == 0 else (1, HW)
    dsrc = up(tf, src)
    y = out32(tf, want.size) if want.dtype == F32 else out16(tf, want.size)
    getattr(_hip(), entry)(y.ptr, dsrc.ptr, N, C, H, W, tf._sh())
    what = f"{entry} {(N, C, HW)}"
    got = y.get(what)
    (_exact32(got, want, what) if want.dtype == F32 else _exact16(got, want, "fp16", what))


@pytest.mark.parametrize("shape,axes", P.TRANSPOSE_CASES)
def test_group_c_transpose_f32(tf, shape, axes):
    code = P.pos_code(shape)
    x = P.to_f32(code, "fp16").reshape(shape) * F32(1.0009765625) + np.arange(code.size, dtype=F32).reshape(shape) * F32(2.0 ** -20)   # fp32 values no 16-bit path could carry
    want = np.ascontiguousarray(x.transpose(axes))
    y = out32(tf, x.size)
    dx = up(tf, x)
    sh, ax = (ctypes.c_int * len(shape))(*shape), (ctypes.c_int * len(axes))(*axes)
    _hip().tf_transpose_f32(y.ptr, dx.ptr, len(shape), sh, ax, tf._sh())
    _exact32(y.get("tf_transpose_f32"), want, f"tf_transpose_f32 {shape} {axes}")


@pytest.mark.parametrize("N,H,W,C", P.UPSAMPLE_CASES)
def test_group_c_upsample2x(tf, N, H, W, C):
    x = P.pos_code((N, H, W, C))
    want = x[:, np.arange(2 * H) >> 1][:, :, np.arange(2 * W) >> 1]
    y, dx = out16(tf, want.size), up(tf, x)
    _hip().tf_upsample2x_nhwc_f16(y.ptr, dx.ptr, N, H, W, C, tf._sh())
    _exact16(y.get("upsample"), want, "fp16", f"tf_upsample2x_nhwc_f16 {(N, H, W, C)}")


@pytest.mark.parametrize("rows,Ca,Cb", P.CONCAT_CASES)
def test_group_c_concat_channels(tf, rows, Ca, Cb):
    a, b = P.pos_code((rows, Ca), 0), P.pos_code((rows, Cb), 1)
    want = np.concatenate([a, b], axis=1)
    y, da, db = out16(tf, want.size), up(tf, a), up(tf, b)
    _hip().tf_concat_channels_f16(y.ptr, da.ptr, db.ptr, rows, Ca, Cb, tf._sh())
    _exact16(y.get("concat"), want, "fp16", f"tf_concat_channels_f16 {(rows, Ca, Cb)}")


@pytest.mark.parametrize("N,HW,C", P.BIAS_NC_CASES)
def test_group_c_add_bias_nc(tf, N, HW, C):
    x, b = P.pos_code((N, HW, C), kind="mod"), P.pos_code((N, 1, C), 3, "mod")
    y, dx, db = out16(tf, x.size), up(tf, x), up(tf, b)
    _hip().tf_add_bias_nc_f16(y.ptr, dx.ptr, db.ptr, N, HW, C, tf._sh())
    _exact16(y.get("bias"), P.add16(x, b), "fp16", f"tf_add_bias_nc_f16 {(N, HW, C)}")


@pytest.mark.parametrize("rows,C", P.GEGLU_CASES)
def test_group_c_geglu(tf, rows, C):
    x = P.geglu_inputs(rows, C)
    ref, A, tol = P.geglu_ref(x, C)
    y, dx = out16(tf, rows * C), up(tf, x)
    _hip().tf_geglu_f16(y.ptr, dx.ptr, rows, C, tf._sh())
    _within(P.to_f32(y.get("geglu"), "fp16"), ref, tol, A, "tf_geglu_f16", f"tf_geglu_f16 {(rows, C)}")


@pytest.mark.parametrize("N,H,W,C,R,S,stride,pad,Kpad", P.IM2COL_CASES)
def test_group_c_im2col(tf, N, H, W, C, R, S, stride, pad, Kpad):
    hip = _hip()
    x = P.pos_code((N, H, W, C))
    dx = up(tf, x)
    Ho, Wo = P.im2col_out_hw(H, W, R, S, stride, pad)
    want = P.im2col_ref(x, R, S, stride, pad, Kpad, 0, Ho)
    y = out16(tf, want.size)
    hip.tf_im2col_nhwc_f16(y.ptr, dx.ptr, N, H, W, C, R, S, stride, pad, Kpad, tf._sh())
    got = y.get("im2col")
    assert (got.reshape(want.shape)[..., R * S * C:] == 0).all(), "pad columns must be exactly zero"
    _exact16(got, want, "fp16", f"tf_im2col_nhwc_f16 {(N, H, W, C, R, S, stride, pad, Kpad)}")
    for h0, h1 in P.im2col_bands(Ho):
        want = P.im2col_ref(x, R, S, stride, pad, Kpad, h0, h1)
        y = out16(tf, want.size)
        hip.tf_im2col_rows_nhwc_f16(y.ptr, dx.ptr, N, H, W, C, R, S, stride, pad, Kpad, h0, h1, tf._sh())
        got = y.get(f"im2col rows [{h0}, {h1})")
        assert (got.reshape(want.shape)[..., R * S * C:] == 0).all(), "pad columns must be exactly zero"
        _exact16(got, want, "fp16", f"tf_im2col_rows_nhwc_f16 rows [{h0}, {h1})")


@pytest.mark.parametrize("with_pos", (False, True))
@pytest.mark.parametrize("vocab,D,tokens,T", P.EMBED_CASES)
def test_group_c_embedding(tf, vocab, D, tokens, T, with_pos):
    table, pos = P.pos_code((vocab, D), 0, "mod"), P.pos_code((T, D), 1, "mod")
    ids = ((np.arange(tokens, dtype=np.int64) * 7919 + 3) % vocab).astype(np.int32)         # always inside the vocabulary
    assert tokens > T and len(np.unique(ids)) == vocab
    want = table[ids]
    if with_pos:
        want = P.add16(want, pos[np.arange(tokens) % T])
    y, dt, di, dp = out16(tf, want.size), up(tf, table), up(tf, ids), up(tf, pos)
    _hip().tf_embedding_f16(y.ptr, dt.ptr, di.ptr, dp.ptr if with_pos else None, tokens, D, vocab, T, tf._sh())
    _exact16(y.get("embedding"), want, "fp16", f"tf_embedding_f16 {(vocab, D, tokens, T)} pos={with_pos}")


@pytest.mark.parametrize("BT,OC", P.COLMAJOR_CASES)
def test_group_c_add_bias_colmajor(tf, BT, OC):
    out = P.to_f32(P.pos_code((OC, BT), 0, "mod"), "fp16") * F32(1.0009765625)
    bias = P.to_f32(P.pos_code((OC,), 5, "mod"), "fp16") * F32(0.9990234375)                # planted per column; the sums round in fp32
    want = out + bias[:, None]
    buf = out32(tf, out.size)
    _hip().tf_memcpy(buf.ptr, out.ctypes.data, out.nbytes, tf.H2D)
    db = up(tf, bias)
    _hip().tf_add_bias_colmajor_f32(buf.ptr, db.ptr, BT, OC, tf._sh())
    _exact32(buf.get("colmajor"), want, f"tf_add_bias_colmajor_f32 {(BT, OC)}")


# ---- Group D ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", P.D_C)
@pytest.mark.parametrize("entry", P.D_ENTRIES)
def test_group_d_row_softmaxes(tf, entry, C):
    hip = _hip()
    for rows, C_, ldo, ldi, mode in [c for c in P.d_cases(entry) if c[1] == C]:
        x = P.softmax_input(entry, rows, C)
        mr = P.mask_rows_of(mode, rows)
        mask = P.softmax_mask(mr, C, rows) if mr else None
        p, A, d = P.softmax_ref(entry, x, mask)
        what = f"{entry} rows {rows} C {C} ldo {ldo} ldi {ldi} mask {mode}"
        dm = up(tf, mask) if mask is not None else None
        if entry == "tf_softmax_rows_f32":
            y, dx = out32(tf, rows * C), up(tf, x)
            hip.tf_softmax_rows_f32(y.ptr, dx.ptr, rows, C, tf._sh())
            got, tol = y.get(what).astype(F64).reshape(rows, C), A
        else:
            xin = np.zeros((rows, ldi), F32)
            xin[:, :C] = x
            xin[:, C:] = 7.0                                              # the gap between rows is never read as a score
            y = out16(tf, rows * ldo)
            if entry == "tf_softmax_mask_rows_f16":
                dx = up(tf, xin.astype(np.float16))
                hip.tf_softmax_mask_rows_f16(y.ptr, dx.ptr, dm.ptr if dm else None, rows, C, ldo, 0.125, mr, tf._sh())
            else:
                dx = up(tf, xin)
                hip.tf_softmax_mask_rows_f32in_f16(y.ptr, ldo, dx.ptr, ldi, dm.ptr if dm else None, rows, C, 0.125, mr, tf._sh())
            full = y.get(what).reshape(rows, ldo)
            assert (full[:, C:] == 0).all(), f"{what}: pad columns must be exactly zero"
            got, tol = P.to_f32(full[:, :C], "fp16").astype(F64), P.budget16(p, A, "fp16")
        _within(got, p, tol, A, entry, what)
        assert (np.abs(got.sum(axis=1) - 1.0) <= tol.sum(axis=1)).all(), f"{what}: row sums"


# ---- Group E ------------------------------------------------------------------------------------------------------------------------------------
def test_group_e_set_step_params(tf):
    hip = _hip()
    want = np.array(P.STEP_PARAMS, F32)
    p = out32(tf, 4)
    hip.tf_set_step_params(p.ptr, *[float(v) for v in want], tf._sh())
    _exact32(p.get("params"), want, "tf_set_step_params")
    for nbytes in P.COPY_NBYTES:
        src = P.long_input(nbytes // 2, "fp16")
        p, dst, dsrc = out32(tf, 4), out16(tf, nbytes // 2), up(tf, src)
        hip.tf_set_step_params_copy(p.ptr, *[float(v) for v in want[::-1]], dst.ptr, dsrc.ptr, nbytes, tf._sh())
        _exact32(p.get("params"), want[::-1], f"tf_set_step_params_copy {nbytes}: params")
        _exact16(dst.get("copy"), src, "fp16", f"tf_set_step_params_copy {nbytes}: copy")


@pytest.mark.parametrize("dim", P.EMBED_DIMS)
@pytest.mark.parametrize("dtype", ("fp16", "bf16"))
def test_group_e_timestep_embedding(tf, dtype, dim):
    hip = _hip()
    entry = "tf_timestep_embedding_f16" if dtype == "fp16" else "tf_timestep_embedding_bf16"
    for t in P.EMBED_T:
        params = up(tf, np.array([t, 0.5, 0.6, 7.5], F32))
        y = out16(tf, dim, dtype)
        getattr(hip, entry)(y.ptr, params.ptr, dim, P.MAX_PERIOD, tf._sh())
        ref, A, tol = P.embed_ref(dim, t, dtype)
        _within(P.to_f32(y.get(entry), dtype), ref, tol, A, entry, f"{entry} dim {dim} t {t}")


@pytest.mark.parametrize("B,C,H,W", P.DDIM_CASES)
def test_group_e_cfg_ddim_step(tf, B, C, H, W):
    hip = _hip()
    n = B * C * H * W
    for dtype, entry in (("fp16", "tf_cfg_ddim_step_f32"), ("bf16", "tf_cfg_ddim_step_bf16")):
        lat, eu, ec = P.ddim_inputs(B, C, H, W, dtype)
        deps, du, dc = up(tf, np.concatenate([eu.ravel(), ec.ravel()])), up(tf, eu), up(tf, ec)
        for a_t, a_prev in P.sd_alphas():
            params = up(tf, np.array([981.0, a_t, a_prev, P.GUIDANCE], F32))
            ref, A = P.ddim_ref(lat, eu, ec, a_t, a_prev, dtype)
            buf = out32(tf, n)
            hip.tf_memcpy(buf.ptr, lat.ctypes.data, lat.nbytes, tf.H2D)
            getattr(hip, entry)(buf.ptr, deps.ptr, params.ptr, B, C, H, W, tf._sh())
            what = f"{entry} {(B, C, H, W)} a_t {a_t}"
            got = buf.get(what)
            _within(got, ref.ravel(), A.ravel(), A.ravel(), entry, what)
            if dtype == "fp16":                                            # the two halves in separate allocations: the same bits
                buf2 = out32(tf, n)
                hip.tf_memcpy(buf2.ptr, lat.ctypes.data, lat.nbytes, tf.H2D)
                hip.tf_cfg_ddim_step2_f32(buf2.ptr, du.ptr, dc.ptr, params.ptr, B, C, H, W, tf._sh())
                got2 = buf2.get(what)
                _within(got2, ref.ravel(), A.ravel(), A.ravel(), "tf_cfg_ddim_step2_f32", what + " (step2)")
                _exact32(got2, got, what + ": tf_cfg_ddim_step2_f32 against tf_cfg_ddim_step_f32")


# ---- Group F ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,is_f32,n,at", P.nonfinite_cases())
def test_group_f_debug_nonfinite(tf, name, is_f32, n, at):
    hip = _hip()
    for bad in (("inf", "nan") if at is not None else (None,)):
        a = P.nonfinite_array(is_f32, n, at, bad)
        da, flag = up(tf, a), up(tf, np.zeros(4, np.int32))
        hip.tf_debug_nonfinite(da.ptr, a.nbytes, is_f32, flag.ptr, tf._sh())
        assert int(down(tf, flag, 1, np.int32)[0]) == (1 if at is not None else 0), f"tf_debug_nonfinite: {name} {bad}"


@pytest.mark.parametrize("nwords", P.CHECKSUM_WORDS)
def test_group_f_debug_checksum(tf, nwords):
    hip = _hip()
    w = P.long_input(2 * nwords, "fp16").view(np.uint32)
    start = 0x0123456789ABCDEF
    dw, ds = up(tf, w), up(tf, np.array([start, 0], np.uint64))
    hip.tf_debug_checksum(dw.ptr, w.nbytes, ds.ptr, tf._sh())
    assert int(down(tf, ds, 1, np.uint64)[0]) == P.checksum_ref(w, start), "tf_debug_checksum accumulates the weighted word sum into *sum"
    if nwords > 1:
        s = w.copy()
        s[[0, nwords - 1]] = s[[nwords - 1, 0]]
        assert s[0] != w[0]
        dw, ds2 = up(tf, s), up(tf, np.array([start, 0], np.uint64))
        hip.tf_debug_checksum(dw.ptr, s.nbytes, ds2.ptr, tf._sh())
        got = int(down(tf, ds2, 1, np.uint64)[0])
        assert got == P.checksum_ref(s, start) and got != P.checksum_ref(w, start), "two words swapped: the checksum must change"
    dw, ds3 = up(tf, w), up(tf, np.array([start, 0], np.uint64))                            # whole 32-bit words only: 2 trailing bytes do not count
    hip.tf_debug_checksum(dw.ptr, w.nbytes - 2, ds3.ptr, tf._sh())
    assert int(down(tf, ds3, 1, np.uint64)[0]) == P.checksum_ref(w[:-1], start)


# ---- argument checks ------------------------------------------------------------------------------------------------------------------------------
def _bad_calls(o, i, i2, p, shape4, axes4, neg4):
    """(entry, arguments) that must return TF_E_ARG: a null pointer, a negative count, a width off the vector grid.  o: the output buffer (which
    must stay untouched), i / i2: inputs, p: step parameters."""
    N = None
    calls = []
    for e in ("tf_silu_f16", "tf_sigmoid_f16", "tf_gelu_f16", "tf_quick_gelu_f16", "tf_silu_bf16", "tf_convert_f16_to_bf16", "tf_convert_bf16_to_f16",
              "tf_cast_f32_to_f16", "tf_cast_f16_to_f32", "tf_image_to_u8"):
        calls += [(e, (N, i, 8, N)), (e, (o, N, 8, N)), (e, (o, i, -8, N))]
    calls += [("tf_add_f16", a) for a in ((N, i, i2, 8, N), (o, N, i2, 8, N), (o, i, N, 8, N), (o, i, i2, -1, N))]
    calls += [("tf_add_16", (t,) + a) for t in (0, 1) for a in ((N, i, i2, 8, N), (o, i, N, 8, N), (o, i, i2, -1, N))] + [("tf_add_16", (2, o, i, i2, 8, N))]
    calls += [("tf_scale_cast_f32_to_f16", a) for a in ((N, i, 1.0, 8, N), (o, N, 1.0, 8, N), (o, i, 1.0, -8, N))]
    calls += [("tf_scale_f32", (N, 2.0, 8, N)), ("tf_scale_f32", (o, 2.0, -8, N))]
    for e in P.TILE_ENTRIES:
        calls += [(e, (N, i, 1, 8, 2, 2, N)), (e, (o, N, 1, 8, 2, 2, N)), (e, (o, i, -1, 8, 2, 2, N)), (e, (o, i, 1, -8, 2, 2, N)), (e, (o, i, 1, 8, -2, 2, N)),
                  (e, (o, i, 1, 8, 2, -2, N)), (e, (o, i, 1, 8, -2, -2, N))]
    calls += [("tf_transpose_f32", a) for a in ((N, i, 4, shape4, axes4, N), (o, N, 4, shape4, axes4, N), (o, i, 0, shape4, axes4, N), (o, i, 5, shape4, axes4, N),
                                               (o, i, 4, neg4, axes4, N), (o, i, 4, shape4, shape4, N))]
    calls += [("tf_upsample2x_nhwc_f16", a) for a in ((N, i, 1, 2, 2, 8, N), (o, N, 1, 2, 2, 8, N), (o, i, -1, 2, 2, 8, N), (o, i, 1, -2, 2, 8, N), (o, i, 1, 2, -2, 8, N),
                                                     (o, i, 1, -2, -2, 8, N), (o, i, 1, 2, 2, 12, N), (o, i, 1, 2, 2, -8, N))]
    calls += [("tf_concat_channels_f16", a) for a in ((N, i, i2, 2, 8, 8, N), (o, N, i2, 2, 8, 8, N), (o, i, N, 2, 8, 8, N), (o, i, i2, -2, 8, 8, N), (o, i, i2, 2, 12, 8, N),
                                                     (o, i, i2, 2, 8, 4, N), (o, i, i2, 2, -8, 8, N))]
    calls += [("tf_add_bias_nc_f16", a) for a in ((N, i, i2, 1, 2, 8, N), (o, N, i2, 1, 2, 8, N), (o, i, N, 1, 2, 8, N), (o, i, i2, -1, 2, 8, N), (o, i, i2, 1, -2, 8, N),
                                                 (o, i, i2, -1, -2, 8, N), (o, i, i2, 1, 2, -8, N), (o, i, i2, 1, 2, 12, N))]
    calls += [("tf_geglu_f16", a) for a in ((N, i, 2, 8, N), (o, N, 2, 8, N), (o, i, -2, 8, N), (o, i, 2, 12, N), (o, i, 2, 0, N))]
    calls += [("tf_im2col_nhwc_f16", a) for a in ((N, i, 1, 4, 4, 4, 3, 3, 1, 1, 40, N), (o, N, 1, 4, 4, 4, 3, 3, 1, 1, 40, N), (o, i, -1, 4, 4, 4, 3, 3, 1, 1, 40, N),
                                                 (o, i, 1, 4, 4, 4, 3, 3, 1, 1, 32, N), (o, i, 1, 4, 4, 4, 3, 3, 0, 1, 40, N), (o, i, 1, 4, -4, 4, 3, 3, 1, 1, 40, N))]
    calls += [("tf_im2col_rows_nhwc_f16", a) for a in ((N, i, 1, 4, 4, 4, 3, 3, 1, 1, 40, 0, 2, N), (o, i, -1, 4, 4, 4, 3, 3, 1, 1, 40, 0, 2, N),
                                                      (o, i, 1, 4, 4, 4, 3, 3, 1, 1, 40, -1, 2, N), (o, i, 1, 4, 4, 4, 3, 3, 1, 1, 40, 3, 2, N), (o, i, 1, 4, 4, 4, 3, 3, 1, 1, 40, 0, 5, N))]
    calls += [("tf_embedding_f16", a) for a in ((N, i, i2, N, 2, 8, 4, 1, N), (o, N, i2, N, 2, 8, 4, 1, N), (o, i, N, N, 2, 8, 4, 1, N), (o, i, i2, N, -2, 8, 4, 1, N),
                                               (o, i, i2, N, 2, 12, 4, 1, N), (o, i, i2, N, 2, 8, 0, 1, N), (o, i, i2, i, 2, 8, 4, 0, N))]
    calls += [("tf_add_bias_colmajor_f32", a) for a in ((N, i, 2, 2, N), (o, N, 2, 2, N), (o, i, -2, 2, N), (o, i, 2, -2, N))]
    calls += [("tf_softmax_rows_f32", a) for a in ((N, i, 2, 8, N), (o, N, 2, 8, N), (o, i, -2, 8, N), (o, i, 2, 0, N))]
    calls += [("tf_softmax_mask_rows_f16", a) for a in ((N, i, N, 2, 8, 8, 1.0, 0, N), (o, N, N, 2, 8, 8, 1.0, 0, N), (o, i, N, -2, 8, 8, 1.0, 0, N), (o, i, N, 2, 8, 7, 1.0, 0, N),
                                                       (o, i, N, 2, 0, 8, 1.0, 0, N), (o, i, i2, 2, 8, 8, 1.0, 0, N))]
    calls += [("tf_softmax_mask_rows_f32in_f16", a) for a in ((N, 8, i, 8, N, 2, 8, 1.0, 0, N), (o, 8, N, 8, N, 2, 8, 1.0, 0, N), (o, 8, i, 8, N, -2, 8, 1.0, 0, N),
                                                             (o, 7, i, 8, N, 2, 8, 1.0, 0, N), (o, 8, i, 7, N, 2, 8, 1.0, 0, N), (o, 8, i, 8, i2, 2, 8, 1.0, 0, N))]
    calls += [("tf_set_step_params", (N, 1.0, 0.5, 0.6, 7.5, N))]
    calls += [("tf_set_step_params_copy", a) for a in ((N, 1.0, 0.5, 0.6, 7.5, o, i, 16, N), (p, 1.0, 0.5, 0.6, 7.5, N, i, 16, N), (p, 1.0, 0.5, 0.6, 7.5, o, N, 16, N),
                                                      (p, 1.0, 0.5, 0.6, 7.5, o, i, -16, N), (p, 1.0, 0.5, 0.6, 7.5, o, i, 24, N), (p, 1.0, 0.5, 0.6, 7.5, o + 8, i, 16, N))]
    for e in ("tf_timestep_embedding_f16", "tf_timestep_embedding_bf16"):
        calls += [(e, (N, p, 8, 10000.0, N)), (e, (o, N, 8, 10000.0, N)), (e, (o, p, 7, 10000.0, N)), (e, (o, p, -8, 10000.0, N)), (e, (o, p, 0, 10000.0, N))]
    for e in ("tf_cfg_ddim_step_f32", "tf_cfg_ddim_step_bf16"):
        calls += [(e, (N, i, p, 1, 4, 2, 2, N)), (e, (o, N, p, 1, 4, 2, 2, N)), (e, (o, i, N, 1, 4, 2, 2, N)), (e, (o, i, p, -1, 4, 2, 2, N)), (e, (o, i, p, 1, -4, 2, 2, N)),
                  (e, (o, i, p, 1, 4, -2, 2, N)), (e, (o, i, p, 1, 4, 2, -2, N)), (e, (o, i, p, 1, 4, -2, -2, N))]
    calls += [("tf_cfg_ddim_step2_f32", a) for a in ((N, i, i2, p, 1, 4, 2, 2, N), (o, N, i2, p, 1, 4, 2, 2, N), (o, i, N, p, 1, 4, 2, 2, N), (o, i, i2, N, 1, 4, 2, 2, N),
                                                    (o, i, i2, p, -1, 4, 2, 2, N), (o, i, i2, p, 1, 4, -2, -2, N), (o, i, i2, p, 1, 4, 2, -2, N))]
    calls += [("tf_debug_nonfinite", a) for a in ((N, 16, 0, o, N), (i, 16, 0, N, N), (i, -16, 0, o, N))]
    calls += [("tf_debug_checksum", a) for a in ((N, 16, o, N), (i, 16, N, N), (i, -16, o, N))]
    return calls


def test_bad_arguments_return_e_arg_and_leave_the_output_alone(tf):
    lib = _lib()
    o = Out(tf, 4096, U16, P.SENT16["fp16"])
    i, i2, p = up(tf, np.zeros(4096, U16)), up(tf, np.zeros(4096, U16)), up(tf, np.array([1.0, 0.5, 0.6, 7.5], F32))
    shape4, axes4, neg4 = (ctypes.c_int * 4)(2, 3, 2, 2), (ctypes.c_int * 4)(3, 2, 1, 0), (ctypes.c_int * 4)(2, -3, 2, -2)
    calls = _bad_calls(o.ptr, i.ptr, i2.ptr, p.ptr, shape4, axes4, neg4)
    named = {e for e, _ in calls}
    assert {e for e, *_ in P.A_ENTRIES} | set(P.B_ENTRIES) | set(P.TILE_ENTRIES) | set(P.D_ENTRIES) | set(P.DDIM_ENTRIES) <= named
    for entry, args in calls:
        assert getattr(lib, entry)(*args) == P.TF_E_ARG, (entry, args)
    o.untouched("after the rejected calls")
    got = down(tf, p, 4, F32)
    assert np.array_equal(got, np.array([1.0, 0.5, 0.6, 7.5], F32))


def test_report_worst_error_over_tolerance():
    """pytest -s: the largest |error| / tolerance each budgeted entry reached in the tests above, and how much of A it used beyond the store
    rounding, which alone is up to 0.98 of tol for a correctly rounded 16-bit result (DESIGN.md 4.3 records them)."""
    for entry in sorted(WORST):
        print(f"\n{entry}: worst |err| / tol = {WORST[entry][0]:.3f}, beyond the store rounding {WORST[entry][1]:.3f} of A")
        assert WORST[entry][0] <= 1.0
