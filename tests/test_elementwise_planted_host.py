"""The planted inputs, references and budgets of tests/aux/elementwise_planted.py (host code, no GPU), for every table
tests/test_gpu_elementwise_planted.py walks (the tables are imported from the aux module, so the two cannot drift apart):

  * the stated properties hold: the long-input hash differs at i +- 8 and i +- span, position codes differ between neighbours along every axis
    and between the sources of a launch, the softmax maxima keep their margin and visit every wave, no table row leaves its storage type's range;
  * every fp32 emulation stays within A / 2 of the float64 reference on every table row, under every +-ulp / contraction variant, and K is the
    smallest integer for which it does (the ratios are printed: pytest -s); the two-step bit-exact references equal one independent float64
    rounding wherever the fp32 step is exact;
  * the inputs tell a wrong kernel from a right one: each mutant below, written in numpy, breaks its group's assertion on some table row."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import elementwise_planted as P  # noqa: E402

F32, F64, U16 = np.float32, np.float64, np.uint16
RATIOS = {}


def _record(entry, ratio, K, family):
    """ratio = max |emulation - reference| / (A at K = 1): at most K / 2; the last test of this file checks that the family's K is the smallest."""
    RATIOS[entry] = (ratio, K, family)
    print(f"\n{entry}: emulation / (A at K = 1) = {ratio:.3f}  (K = {K})")
    assert ratio <= K / 2, (entry, ratio, K)


# ---- stated properties --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("fp16", "bf16"))
def test_long_input_hash_differs_at_the_vector_and_trip_strides(dtype):
    for n, span in ((P.A_LENGTHS[-1], P.VEC_SPAN), (P.B_LENGTHS[-1], P.SCALAR_SPAN)):
        for salt in (0, 1):
            a = P.long_input(n, dtype, salt)
            assert np.isfinite(P.to_f32(a, dtype)).all()
            assert (a[8:] != a[:-8]).all() and (a[span:] != a[:-span]).all() and n > span
    full = P.cast_inputs()
    i = np.arange(P.B_LENGTHS[-1])
    h = P.hash_index(i, len(full))
    assert (h[P.SCALAR_SPAN:] != h[:-P.SCALAR_SPAN]).all() and (h[1:] != h[:-1]).all()
    nw = P.CHECKSUM_WORDS[-1]
    assert nw > P.SCALAR_SPAN and P.NONFINITE_BIG > P.SCALAR_SPAN and P.COPY_NBYTES[-1] // 16 > 64 * 256 and max(P.EMBED_DIMS) // 2 > 256


def _neighbours_differ(code):
    for ax in range(code.ndim):
        if code.shape[ax] > 1:
            a, b = np.moveaxis(code, ax, 0)[1:], np.moveaxis(code, ax, 0)[:-1]
            assert (a != b).all(), (code.shape, ax)


def test_position_codes_differ_between_neighbours_and_sources():
    shapes = [(n, c, hw) for n, c, hw in P.TILE_CASES] + [s for s, _ in P.TRANSPOSE_CASES] + [c for c in P.UPSAMPLE_CASES]
    shapes += [(n, h, w, c) for n, h, w, c, *_ in P.IM2COL_CASES] + [(n, hw, c) for n, hw, c in P.BIAS_NC_CASES]
    for sh in shapes:
        for kind in ("fin", "mod"):
            code = P.pos_code(sh, kind=kind)
            _neighbours_differ(code)
            assert np.isfinite(P.to_f32(code, "fp16")).all()
    for rows, Ca, Cb in P.CONCAT_CASES:
        a, b = P.pos_code((rows, Ca), 0), P.pos_code((rows, Cb), 1)
        _neighbours_differ(a), _neighbours_differ(b)
        m = min(Ca, Cb)
        assert (a[:, :m] != b[:, :m]).all() and (a[:, -8:] != b[:, :8]).all()            # the same (row, column) and the seam
    for N, HW, C in P.BIAS_NC_CASES:
        b = P.pos_code((N, 1, C), 3, "mod")
        _neighbours_differ(b)
    for B, C, H, W in P.DDIM_CASES:
        for dtype in ("fp16", "bf16"):
            lat, eu, ec = P.ddim_inputs(B, C, H, W, dtype)
            assert (eu != ec).all() and np.abs(P.to_f32(eu, dtype)).max() <= 16 and np.abs(lat).max() < 16
            _neighbours_differ(eu), _neighbours_differ(ec)
    v = np.abs(P.to_f32(P.moderate_bits(np.arange(28672)), "fp16"))
    assert v.min() >= 2.0 ** -10 and v.max() < 16 and len(np.unique(P.moderate_bits(np.arange(28672)))) == 28672


@pytest.mark.parametrize("entry", P.D_ENTRIES)
def test_softmax_margins_and_waves(entry):
    seen = set()
    for rows, C, ldo, ldi, mode in P.d_cases(entry):
        x = P.softmax_input(entry, rows, C)
        assert np.abs(x).max() <= 480 and (entry == "tf_softmax_rows_f32" or np.abs(x).max() == 480)
        if entry == "tf_softmax_mask_rows_f16":
            assert np.array_equal(x, P.round16(x, "fp16"))
        mr = P.mask_rows_of(mode, rows)
        mask = P.softmax_mask(mr, C, rows) if mr else None
        if mode == "wrap4":
            assert rows / mr == 2.5
        if mask is not None:
            assert np.isfinite(mask).any() and (C < 8 or np.isneginf(mask).any()) and (mr == 1 or C < 4 or (mask[0] != mask[1]).any())
        p, A, d = P.softmax_ref(entry, x, mask)
        pk = P.peak_col(np.arange(rows), C)
        assert (d.argmax(axis=1) == pk).all() and np.isfinite(d.max(axis=1)).all()
        rest = np.where(np.arange(C)[None, :] == pk[:, None], -np.inf, d)
        assert C == 1 or rest.max() <= -P.MARGIN, (rows, C, mode, rest.max())
        assert np.isfinite(p).all() and (p.sum(axis=1) > 0.99).all()                      # no row has every key masked
        if C >= 214:
            assert {int(c % 256) // 64 for c in pk} == {0, 1, 2, 3}
        seen |= {int(c % 256) // 64 for c in pk}
    assert seen == {0, 1, 2, 3}


def test_tables_stay_inside_their_storage_types():
    for rows, C in P.GEGLU_CASES:
        y, A, tol = P.geglu_ref(P.geglu_inputs(rows, C), C)
        assert np.abs(y).max() < 300
    for N, HW, C in P.BIAS_NC_CASES:
        got = P.to_f32(P.add16(P.pos_code((N, HW, C), kind="mod"), P.pos_code((N, 1, C), 3, "mod")), "fp16")
        assert np.isfinite(got).all()
    for dim in P.EMBED_DIMS:
        assert dim % 2 == 0
    for a_t, a_prev in P.sd_alphas():
        assert 0 < a_t < a_prev <= 1
    assert P.sd_alphas()[-1][1] == 1.0
    for name, is_f32, n, at in P.nonfinite_cases():
        if at is None:
            a = P.nonfinite_array(is_f32, n, None, None)
            v = a if is_f32 else P.to_f32(a, "fp16")
            assert np.isfinite(v).all() and (v == 0).any() and ((np.abs(v) > 0) & (np.abs(v) < (1.2e-38 if is_f32 else 6.1e-5))).any()
            assert is_f32 or ((v == 65504).any() and (v == -65504).any())


# ---- emulations against float64 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,op,dtype", [(e, k, d) for e, k, d, _, _ in P.A_ENTRIES if k in P.ACTS])
def test_activation_emulation_within_half_the_budget(entry, op, dtype):
    y, A, tol, fin = P.act_table(op, dtype)
    x = P.to_f32(P.patterns(), dtype)[fin]
    worst = 0.0
    for ue, ur, fused in P.act_variants(op):
        emu = P.emulate_act(op, x, ue, ur, fused).astype(F64)
        worst = max(worst, float((np.abs(emu - y[fin]) / (A[fin] / P.K_ACT)).max()))
        # behind the store: the rounded emulation is inside tol
        got = P.to_f32(P.to_bits(emu.astype(F32), dtype), dtype).astype(F64)
        assert (np.abs(got - y[fin]) <= tol[fin]).all()
    _record(entry, worst, P.K_ACT, "act")


def test_geglu_emulation_within_half_the_budget():
    worst = 0.0
    for rows, C in P.GEGLU_CASES:
        xb = P.geglu_inputs(rows, C)
        y, A, tol = P.geglu_ref(xb, C)
        for ue, ur, fused in P.act_variants("gelu"):
            worst = max(worst, float((np.abs(P.emulate_geglu(xb, C, ue, ur, fused).astype(F64) - y) / (A / P.K_GEGLU)).max()))
    _record("tf_geglu_f16", worst, P.K_GEGLU, "geglu")


@pytest.mark.parametrize("entry", P.D_ENTRIES)
def test_softmax_emulation_within_half_the_budget(entry):
    worst = 0.0
    done = set()
    for rows, C, ldo, ldi, mode in P.d_cases(entry):
        if (rows, C, mode) in done:
            continue
        done.add((rows, C, mode))
        x = P.softmax_input(entry, rows, C)
        mr = P.mask_rows_of(mode, rows)
        mask = P.softmax_mask(mr, C, rows) if mr else None
        p, A, d = P.softmax_ref(entry, x, mask)
        for fused in (False, True):
            for ue, ur in P.ULP_PAIRS:
                emu = P.emulate_softmax(entry, x, mask, fused, ue, ur).astype(F64)
                ok = A > 0
                assert (emu[~ok] == 0).all()
                A1 = (A - P.F32_TINY) / P.K_SOFTMAX + P.F32_TINY
                worst = max(worst, float((np.abs(emu - p)[ok] / A1[ok]).max()))
    _record(entry, worst, P.K_SOFTMAX, "softmax")


@pytest.mark.parametrize("dtype", ("fp16", "bf16"))
def test_timestep_embedding_emulation_within_half_the_budget(dtype):
    worst = 0.0
    for dim in P.EMBED_DIMS:
        for t in P.EMBED_T:
            y, A, tol = P.embed_ref(dim, t, dtype)
            for kl, ke, kt in P.EMBED_VARIANTS:
                worst = max(worst, float((np.abs(P.emulate_embed(dim, t, kl, ke, kt).astype(F64) - y) / (A / P.K_EMBED)).max()))
    _record(f"tf_timestep_embedding_{'f16' if dtype == 'fp16' else 'bf16'}", worst, P.K_EMBED, "embed")


@pytest.mark.parametrize("dtype", ("fp16", "bf16"))
def test_ddim_emulation_within_half_the_budget(dtype):
    worst = 0.0
    for B, C, H, W in P.DDIM_CASES:
        lat, eu, ec = P.ddim_inputs(B, C, H, W, dtype)
        for a_t, a_prev in P.sd_alphas():
            y, A = P.ddim_ref(lat, eu, ec, a_t, a_prev, dtype)
            for fused in (0, 1, 2):
                for kd in (0, 1, -1):
                    worst = max(worst, float((np.abs(P.emulate_ddim(lat, eu, ec, a_t, a_prev, dtype, fused, kd).astype(F64) - y) / (A / P.K_DDIM)).max()))
    _record("tf_cfg_ddim_step_f32 / step2" if dtype == "fp16" else "tf_cfg_ddim_step_bf16", worst, P.K_DDIM, "ddim")


# ---- the two-step references against one float64 rounding ---------------------------------------------------------------------------------------
def _bits_of_f64(v, dtype):
    """bits of float64 values that are exactly representable in dtype (inf and NaN included)."""
    return P.to_bits(np.asarray(v, F64).astype(F32), dtype)


def test_exact_references_equal_one_float64_rounding_where_the_fp32_step_is_exact():
    for dtype in ("fp16", "bf16"):
        a, b = P.a_inputs("patterns", dtype)
        want = P.a_exact("add", a, b, dtype, dtype)
        with np.errstate(invalid="ignore"):
            s64 = P.to_f32(a, dtype).astype(F64) + P.to_f32(b, dtype).astype(F64)
        exact = np.isfinite(s64) & (s64.astype(F32).astype(F64) == s64)
        assert exact.mean() > 0.3
        assert P.same_bits(want[exact], _bits_of_f64(P.rne16_f64(s64[exact], dtype), dtype), dtype).all()
    p = P.patterns()
    fin = np.isfinite(P.to_f32(p, "fp16"))
    assert P.same_bits(P.a_exact("cvt", p, p, "fp16", "bf16")[fin], _bits_of_f64(P.rne16_f64(P.to_f32(p, "fp16")[fin].astype(F64), "bf16"), "bf16"), "bf16").all()
    finb = np.isfinite(P.to_f32(p, "bf16"))
    got = P.a_exact("cvt", p, p, "bf16", "fp16")
    assert P.same_bits(got[finb], _bits_of_f64(P.rne16_f64(P.to_f32(p, "bf16")[finb].astype(F64), "fp16"), "fp16"), "fp16").all()
    v = P.to_f32(p, "bf16")
    assert (P.to_f32(got, "fp16")[np.isfinite(v) & (np.abs(v) >= 65520)] == np.sign(v[np.isfinite(v) & (np.abs(v) >= 65520)]) * np.inf).all()
    sub = (p & 0x7C00) == 0                                                            # fp16 subnormals (and zeros) convert exactly to bf16
    vs, cs = P.to_f32(p[sub], "fp16").astype(F64), P.to_f32(P.a_exact("cvt", p[sub], p[sub], "fp16", "bf16"), "bf16").astype(F64)
    assert (np.abs(cs - vs) <= np.abs(vs) * 2.0 ** -8).all() and ((cs == 0) == (vs == 0)).all()      # normal numbers in bf16: rounded to 8 significant bits, never flushed
    few = (p[sub] & 0x3FF) < 256
    assert np.array_equal(cs[few], vs[few])
    x = P.cast_inputs()
    f = np.isfinite(x)
    assert P.same_bits(P.b_reference("tf_cast_f32_to_f16", x)[f], _bits_of_f64(P.rne16_f64(x[f].astype(F64)), "fp16"), "fp16").all()
    for sc in P.B_SCALES:
        prod = x[f].astype(F64) * F64(sc)
        ex = prod.astype(F32).astype(F64) == prod
        assert P.same_bits(P.b_reference("tf_scale_cast_f32_to_f16", x, sc)[f][ex], _bits_of_f64(P.rne16_f64(prod[ex]), "fp16"), "fp16").all()
    img = P.b_input("tf_image_to_u8", "all")
    v = np.clip((P.to_f32(img, "fp16").astype(F64) + 1) / 2, 0, 1) * 255                # exact in float64; the fp32 formula may round up across an integer
    ref = P.b_reference("tf_image_to_u8", img).astype(int)
    assert (np.abs(ref - np.floor(v)) <= 1).all() and (ref == np.floor(v)).mean() > 0.99 and ref.min() == 0 and ref.max() == 255


# ---- mutants: wrong kernels written in numpy ----------------------------------------------------------------------------------------------------
def _vec_kernel(x, n, drop_tail=False, repeat_first_trip=False):
    """an identity "kernel" with k_unary's walk over n elements: 2048 x 256 lanes, 8 elements a lane and trip, then the n & 7 tail."""
    y = np.full(n, P.SENT16["fp16"], U16)
    nvec = n >> 3
    y[:nvec * 8] = x[:nvec * 8]
    if repeat_first_trip:
        lanes = 2048 * 256
        v = np.arange(lanes, nvec)                                                      # the vectors of the second trip
        y[:nvec * 8].reshape(-1, 8)[v] = x[:nvec * 8].reshape(-1, 8)[v - lanes]
    if not drop_tail:
        y[nvec * 8:] = x[nvec * 8:n]
    return y


def test_mutants_of_group_a_are_caught():
    caught = {"tail": False, "trip": False}
    for n in P.A_LENGTHS:
        x, _ = P.a_inputs(n, "fp16")
        assert np.array_equal(_vec_kernel(x, n), x)
        caught["tail"] |= not np.array_equal(_vec_kernel(x, n, drop_tail=True), x)
        caught["trip"] |= not np.array_equal(_vec_kernel(x, n, repeat_first_trip=True), x)
    assert all(caught.values()), caught
    x, _ = P.a_inputs(P.A_LENGTHS[-1], "fp16")                                           # every vector of the second trip differs, not just some
    m = _vec_kernel(x, len(x), repeat_first_trip=True)
    assert (m[P.VEC_SPAN:P.VEC_SPAN + 2048] != x[P.VEC_SPAN:P.VEC_SPAN + 2048]).all()


def test_mutant_of_group_b_truncating_cast_is_caught():
    x = P.cast_inputs()
    want = P.b_reference("tf_cast_f32_to_f16", x)
    u = x.view(np.uint32)
    e = ((u >> 23) & 0xFF).astype(np.int64) - 127
    normal = np.isfinite(x) & (e >= -14) & (e <= 15)
    trunc = (((u >> 16) & 0x8000) | ((e + 15) << 10) | ((u >> 13) & 0x3FF)).astype(U16)   # the mantissa cut, never rounded
    assert (trunc[normal] != want[normal]).any() and (trunc[normal] == want[normal]).any()


def _tile_clamped(src, C, HW):
    """(N, C, HW) -> (N, HW, C) by 32 x 32 tiles that clamp the index at the edge (reads and writes) where k_transpose skips."""
    N = src.shape[0]
    Cp, Hp = -(-C // 32) * 32, -(-HW // 32) * 32
    dst = np.full((N, HW, C), P.SENT16["fp16"], U16)
    c, p = np.meshgrid(np.arange(Cp), np.arange(Hp), indexing="ij")
    val = np.where((c < C) & (p < HW), src[:, np.minimum(c, C - 1), np.minimum(p, HW - 1)], 0)
    for n in range(N):
        dst[n, np.minimum(p, HW - 1).ravel(), np.minimum(c, C - 1).ravel()] = val[n].ravel()
    return dst


def test_mutants_of_group_c_are_caught():
    caught = False
    for N, C, HW in P.TILE_CASES:
        src, want = P.tile_case("tf_nchw_to_nhwc_f16", N, C, HW)
        m = _tile_clamped(src, C, HW)
        assert (C % 32 or HW % 32) or np.array_equal(m, want)
        caught |= not np.array_equal(m, want)
    assert caught, "clamping tile"
    caught = False
    for N, H, W, C in P.UPSAMPLE_CASES:                                                  # reading (ho + 1) >> 1
        x = P.pos_code((N, H, W, C))
        ho, wo = np.arange(2 * H), np.arange(2 * W)
        want = x[:, ho >> 1][:, :, wo >> 1]
        caught |= not np.array_equal(x[:, np.minimum((ho + 1) >> 1, H - 1)][:, :, wo >> 1], want)
    assert caught, "upsample"
    for rows, Ca, Cb in P.CONCAT_CASES:                                                  # switching sources at c <= Ca: the vector at c = Ca read from a, one row on
        a, b = P.pos_code((rows, Ca), 0), P.pos_code((rows, Cb), 1)
        want = np.concatenate([a, b], axis=1)
        m = want.copy()
        m[:, Ca:Ca + 8] = np.roll(a, -1, axis=0)[:, :8]                                   # a + r Ca + Ca: the head of a's next row
        assert not np.array_equal(m, want), (rows, Ca, Cb)
    caught = False
    for N, HW, C in P.BIAS_NC_CASES:                                                     # image 0's bias for every image
        x, b = P.pos_code((N, HW, C), kind="mod"), P.pos_code((N, 1, C), 3, "mod")
        caught |= not np.array_equal(P.add16(x, b[:1]), P.add16(x, b))
    assert caught, "bias of image 0"
    caught = False
    for N, H, W, C, R, S, stride, pad, Kpad in P.IM2COL_CASES:                           # ignoring ho_begin
        x = P.pos_code((N, H, W, C))
        Ho, _ = P.im2col_out_hw(H, W, R, S, stride, pad)
        for h0, h1 in P.im2col_bands(Ho):
            assert 0 <= h0 <= h1 <= Ho
            want = P.im2col_ref(x, R, S, stride, pad, Kpad, h0, h1)
            assert (want[..., R * S * C:] == 0).all()
            caught |= not np.array_equal(P.im2col_ref(x, R, S, stride, pad, Kpad, h0, h1, ignore_begin=True), want)
    assert caught, "im2col band"


def test_mutants_of_group_d_are_caught():
    for entry in P.D_ENTRIES:
        lost = False
        for rows, C, ldo, ldi, mode in P.d_cases(entry):
            if ldo != C or ldi != C:
                continue
            x = P.softmax_input(entry, rows, C)
            mr = P.mask_rows_of(mode, rows)
            mask = P.softmax_mask(mr, C, rows) if mr else None
            p, A, d = P.softmax_ref(entry, x, mask)
            tol = A if entry == "tf_softmax_rows_f32" else P.budget16(p, A, "fp16")
            with np.errstate(all="ignore"):
                m = P.emulate_softmax(entry, x, mask, lose_wave=3).astype(F64)
            bad = ~(np.abs(m - p) <= tol)
            if C >= 214:
                assert bad.any(), (entry, rows, C, mode)
                lost = True
            if mode == "wrap4":                                                          # the mask indexed by r: rows 4 .. 9 read other rows
                wrong, _, _ = P.softmax_ref(entry, x, P.softmax_mask(rows, C, rows), by_r=True)
                assert C < 63 or (np.abs(wrong - p) > 32 * tol).any(), (entry, rows, C)
        assert lost


def test_mutant_of_group_e_ddim_reading_eps_at_the_nchw_index_is_caught():
    for dtype in ("fp16", "bf16"):
        caught = 0
        for B, C, H, W in P.DDIM_CASES:
            lat, eu, ec = P.ddim_inputs(B, C, H, W, dtype)
            for a_t, a_prev in P.sd_alphas():
                y, A = P.ddim_ref(lat, eu, ec, a_t, a_prev, dtype)
                m, _ = P.ddim_ref(lat, eu, ec, a_t, a_prev, dtype, nchw_eps=True)
                caught += bool((np.abs(m - y) > 1000 * A).any())
                swapped, _ = P.ddim_ref(lat, ec, eu, a_t, a_prev, dtype)                   # the two halves swapped
                assert (np.abs(swapped - y) > 1000 * A).any() or a_prev == 1.0 and H * W == 1
        assert caught >= 3 * (len(P.DDIM_CASES) - 1)                                     # (H W = 1: the two layouts coincide)


def test_mutant_of_group_f_scan_dropping_the_trailing_half_word_is_caught():
    def scan(a, is_f32, drop_tail):
        b = a.view(np.uint8)
        nw = len(b) // 4
        w = b[:nw * 4].view(np.uint32)
        bad = ((w & 0x7F800000) == 0x7F800000).any() if is_f32 else (((w & 0x7C00) == 0x7C00) | ((w & 0x7C000000) == 0x7C000000)).any()
        if not is_f32 and len(b) % 4 == 2 and not drop_tail:
            bad |= (int(a[-1]) & 0x7C00) == 0x7C00
        return int(bad)
    missed = []
    for name, is_f32, n, at in P.nonfinite_cases():
        for kind in ("inf", "nan"):
            a = P.nonfinite_array(is_f32, n, at, kind)
            assert scan(a, is_f32, False) == (at is not None), name
            if scan(a, is_f32, True) != (at is not None):
                missed.append(name)
    assert "fp16 last of odd" in missed and "fp16 last of even" not in missed
    w = ((np.arange(1000, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    s = w.copy()
    s[[3, 700]] = s[[700, 3]]
    assert P.checksum_ref(w) != P.checksum_ref(s) and P.checksum_ref(w, 5) == (P.checksum_ref(w) + 5) % 2 ** 64


def test_recorded_ratios_match_the_docstring():
    """the ratios printed above are the ones the aux module's docstring records (run after the emulation tests of this file)."""
    doc = P.__doc__
    worst = {}
    for entry, (ratio, K, family) in RATIOS.items():
        assert f"{entry} {ratio:.3f}" in doc, (entry, f"{ratio:.3f}")
        worst[family] = max(worst.get(family, (0.0, K)), (ratio, K))
    for family, (ratio, K) in worst.items():                                             # with the whole family run: K is the smallest integer
        if sum(f == family for _, _, f in RATIOS.values()) == {"act": 5, "geglu": 1, "softmax": 3, "embed": 2, "ddim": 2}[family]:
            assert math.ceil(2 * ratio) == K, (family, ratio, K)
