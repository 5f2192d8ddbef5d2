"""The GroupNorm statistics a conv produces -- igemm_gn_stats in the epilogue of every GEMM family, k_splitk_reduce_gn, k_splitk_reduce_gn_apply --
and the GroupNorm a conv applies to its input (the GI prologue) on planted statistics, against float64, under budgets fixed on the CPU
(tests/aux/conv_stats_planted.py; tests/test_conv_stats_planted_host.py proves on the host that the inputs tell a wrong kernel from a right one and
that the emulated summation orders stay within half the budgets).  Every case

  * first asserts the form it ran.  Every launch runs under tf_prof_enable: its row of tf_prof_dump must show the tile, the split count and the
    variant the case asked for (a split the dispatcher dropped, for a short workspace say, shows as splitk = 1), and the split-K reduce family's
    counters (tf_prof_read_family) one reduce launch over exactly `slabs x M x N` slab elements of the asked width -- or none for split 1.  The
    chunk count and z_written the launch reports must equal what the aux module's copy of the dispatcher's rule says for the form the case is
    named after.  Where a family gives way silently the launcher's own rule is asked: tf_gemm_ring_form for the wide / all-8 rings of k_igemm,
    tf_conv2d_patch_admits for k_igemm_patch; the ping-pong families and the input GroupNorm fail with TF_E_UNSUPPORTED instead of falling back;
  * pre-fills y and z with a finite sentinel and the statistics table with NaN: every slot of the reported chunks must be finite, no slot beyond
    them may have been touched;
  * holds y to its bound of the float64 sum of the exact GEMM part, bias, bias_nc and the planted residual;
  * holds the table to c 2^-24 sum |y| (sum y^2) per slot of the float64 sums of the y READ BACK, and z -- from the fused reduce, and from
    tf_group_norm_apply_16 / tf_group_norm_apply_cat_16 fed with the producer's table -- to the budget of the float64 norm of that y.
The largest error / tolerance seen per form is printed by the last test (pytest -s)."""
import contextlib
import ctypes
import os
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import norm_planted as P  # noqa: E402
import conv_stats_planted as C  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = ("fp16", "bf16")
MODES = (("fp16", 32), ("fp16", 16), ("bf16", 32))           # (storage type, bits of the split-K slabs): bfloat16 launches keep fp32 slabs
EPS = 1e-5
NAN_BITS = np.float32(np.nan).view(np.uint32)
UNSUPPORTED = 10002
WORST = {}


def _cid(c):
    return f"{c.form}-{c.N}x{c.H}x{c.W}-{c.Cin}-{c.Cout}g{c.G}-k{c.ks}-{c.bm}x{c.bn}s{c.split}-{c.dbg}".replace(" ", "_")


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def _np_dtype(tf, dtype):
    return tf.bfloat16 if dtype == "bf16" else np.float16


def dev(tf, x, dtype):
    return tf.DeviceArray.from_numpy(np.ascontiguousarray(x).reshape(-1), _np_dtype(tf, dtype), "row") if x is not None else None


def dev32(tf, x):
    return tf.DeviceArray.from_numpy(np.ascontiguousarray(x, np.float32).reshape(-1), np.float32, "row")


def sentinel(tf, n, dtype):
    return tf.DeviceArray.from_numpy(np.full((n,), C.SENTINEL, np.float32), _np_dtype(tf, dtype), "row")


def ptr(a):
    return a.ptr if a is not None else None


def tag(dtype):
    return 1 if dtype == "bf16" else 0


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


@contextlib.contextmanager
def forced(bm, bn, split, dbg, slabs=16):
    from tinyfusers_amd.native import hip, lib
    hip.tf_gemm_splitk_partials(slabs)
    lib.tf_gemm_force_config(bm, bn, split)
    hip.tf_gemm_debug(dbg)
    try:
        yield
    finally:
        lib.tf_gemm_force_config(0, 0, 0)
        lib.tf_gemm_debug(0)
        lib.tf_gemm_splitk_partials(16)


class Prof:
    pass


@contextlib.contextmanager
def profiled():
    """the launches inside, as the library's own profiling saw them: .rows = tf_prof_dump's (M, N, K, taps, bm, bn, splitk, variant, launches),
    .reduce = (launches, bytes) of the split-K reduce family."""
    from tinyfusers_amd.native import hip
    pr = Prof()
    hip.tf_prof_enable(1)
    try:
        yield pr
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "prof.csv")
            hip.tf_prof_dump(path.encode())
            pr.rows = [tuple(int(v) for v in ln.split(",")[:9]) for ln in open(path).read().splitlines()[1:]]
        ms, work, n = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_longlong(0)
        hip.tf_prof_read_family(2, ctypes.byref(ms), ctypes.byref(work), ctypes.byref(n))
        pr.reduce = (n.value, work.value)
    finally:
        hip.tf_prof_enable(0)


def assert_launch(pr, M, N, K, taps, bm, bn, split, variant, slab_bytes, residual, z, what):
    """one GEMM launch of exactly this tile, split and variant; behind split > 1 one reduce launch over C.eff_splitk slabs of slab_bytes."""
    assert pr.rows == [(M, N, K, taps, bm, bn, split, variant, 1)], (what, pr.rows)
    eff = C.eff_splitk(K, split)
    assert eff == split, (what, "the case table asks for a split count the dispatcher rounds", eff)
    if eff == 1:
        assert pr.reduce[0] == 0, (what, pr.reduce)
    else:
        mn = float(M) * N
        assert pr.reduce == (1, mn * eff * slab_bytes + mn * 2.0 * (1 + residual + z)), (what, pr.reduce, eff, slab_bytes)


def affine(tf, n, on, dtype):
    if not on:
        return None, None, None, None
    gm, bt = P.affine(n)
    return gm, bt, dev(tf, gm, dtype), dev(tf, bt, dtype)


class Run:
    pass


def launch(tf, c, dtype, entry="fused", use=(1, 1, 1), slabs=16, aff=True, silu=True, res=None, table=True):
    """One conv launch of case c through tf_conv2d_fused_16 / tf_conv2d_fused_norm_16: uploads the planted problem, pre-fills y, z and the
    table, runs under the forced tile / family / slab type and downloads everything.  The status is returned, not raised."""
    from tinyfusers_amd.native import lib
    r = Run()
    r.c, r.dtype = c, dtype
    r.p = p = C.conv_problem(c, dtype, use, res)
    HoWo = c.H * c.W
    M = c.N * HoWo
    r.hold = [dev(tf, p[k], dtype) for k in ("x", "w", "bias", "bias_nc", "res")]
    dx, dw, db, de, dr = r.hold
    r.dy = sentinel(tf, M * c.Cout, dtype)
    nslots = c.N * C.GN_MAX_CHUNKS * c.G * 2
    r.dtable = dev32(tf, np.full((nslots,), np.nan, np.float32)) if table else None
    eff = C.eff_splitk(c.ks * c.ks * c.Cin, c.split)
    ws = tf.DeviceArray.empty((eff * M * c.Cout * 4 + 64,), np.uint8, "row")
    chunks, zw = ctypes.c_int(-7), ctypes.c_int(-7)
    args = (tag(dtype), r.dy.ptr, dx.ptr, None, dw.ptr, ptr(db), ptr(de), c.Cout, ptr(dr), c.N, c.H, c.W, c.Cin, 0, c.Cout, c.ks, c.ks, 1, c.ks // 2, 0,
            ws.ptr, ws.nbytes, None, None, 0, 0, ptr(r.dtable), r.dtable.nbytes if table else 0, c.G if table else 0, ctypes.byref(chunks) if table else None)
    r.gm, r.bt, dgm, dbt = affine(tf, c.Cout, aff, dtype)
    r.dz = sentinel(tf, M * c.Cout, dtype) if entry == "norm" else None
    with forced(c.bm, c.bn, c.split, c.dbg, slabs), profiled() as r.prof:
        if entry == "norm":
            r.rc = lib.tf_conv2d_fused_norm_16(*args, r.dz.ptr, ptr(dgm), ptr(dbt), EPS, 1 if silu else 0, ctypes.byref(zw), tf._sh())
        else:
            r.rc = lib.tf_conv2d_fused_16(*args, tf._sh())
    r.err = lib.tf_last_error()
    if r.rc:
        return r
    r.chunks, r.z_written = chunks.value, zw.value
    K = c.ks * c.ks * c.Cin
    slab_bytes = 2 if slabs == 16 and dtype == "fp16" and c.Cout % 8 == 0 else 4
    assert_launch(r.prof, M, c.Cout, K, c.ks * c.ks, c.bm, c.bn, c.split, C.VARIANT_OF_BIT[c.dbg], slab_bytes, 1 if use[2] else 0,
                  1 if entry == "norm" and C.stats_requested(c.Cout, c.G) else 0, _cid(c))
    r.y = r.dy.numpy().reshape(c.N, HoWo, c.Cout)
    r.z = r.dz.numpy().reshape(c.N, HoWo, c.Cout) if r.dz is not None else None
    r.raw = r.dtable.numpy() if table else None
    return r


def check_y(r, what):
    tol = C.y_tol(r.p, r.dtype)
    assert np.isfinite(r.y).all(), what
    worst = float((np.abs(r.y - r.p["y64"]) / tol).max())
    note(("y", r.dtype), worst)
    assert worst <= 1.0, (what, worst)


def check_table(r, kind, rows, bn, what):
    """every slot of the reported chunks finite and within c 2^-24 of the float64 sums of the device's y, nothing beyond them touched."""
    c = r.c
    n = c.N * r.chunks * c.G * 2
    assert (r.raw[n:].view(np.uint32) == NAN_BITS).all(), (what, "a slot beyond the reported chunks was written")
    T = r.raw[:n].reshape(c.N, r.chunks, c.G, 2)
    assert np.isfinite(T).all(), (what, "a slot of the reported chunks was never written")
    ratio, zeros = C.table_ok(T, r.y, c.G, rows, bn, C.TABLE_C[kind])
    note((kind + " table / c", r.dtype), ratio / C.TABLE_C[kind])
    print(f"\n{what}: table error = {ratio:.3f} x 2^-24 sum|y| (c = {C.TABLE_C[kind]}, emulation {C.TABLE_RATIO[kind]})")
    assert zeros and ratio <= C.TABLE_C[kind], (what, ratio)
    return T


def check_z(z, y, G, gm, bt, silu, dtype, key, what, form):
    assert np.isfinite(z).all(), what
    ref = P.gn_ref64(y, G, gm, bt, silu)
    tol, A = C.z_budget(ref, dtype, form, 2.0 if gm is not None else 1.0, silu)
    assert np.abs(ref).max() < 100
    err = np.abs(z - ref)
    worst = float((err / tol).max())
    note((key, dtype), worst)
    print(f"\n{what}: max |err| / tol = {worst:.3f}, beyond the store rounding {max(float(((err - (tol - A)) / A).max()), 0.0):.3f} of A")
    assert worst <= 1.0, (what, worst)


def hand_over(tf, r, form, what, silu=True):
    """the table the producer left, handed to tf_group_norm_apply_16 with the y it describes."""
    from tinyfusers_amd.native import hip
    c = r.c
    HoWo = c.H * c.W
    gm, bt, dgm, dbt = affine(tf, c.Cout, True, r.dtype)
    z = sentinel(tf, c.N * HoWo * c.Cout, r.dtype)
    hip.tf_group_norm_apply_16(tag(r.dtype), z.ptr, r.dy.ptr, dgm.ptr, dbt.ptr, r.dtable.ptr, r.chunks, c.N, HoWo, c.Cout, c.G, EPS, 1 if silu else 0, tf._sh())
    check_z(z.numpy().reshape(r.y.shape), r.y, c.G, gm, bt, silu, r.dtype, form + " -> apply", what + " -> tf_group_norm_apply_16", form)


def assert_family(c):
    """what the profile row cannot show: a family that quietly gives way -- the wide / all-8 ring to the deep ring, k_igemm_patch to the deep
    ring -- is asked for by the launcher's own rule (the ping-pong families fail loudly)."""
    from tinyfusers_amd.native import lib
    if c.dbg in (8, 16, 256):                                  # the ring the bit asks for is the ring this tile runs
        assert lib.tf_gemm_ring_form(c.bm, c.bn, C.VARIANT_OF_BIT[c.dbg], 1 if c.Cin % 64 == 0 else 0) == C.VARIANT_OF_BIT[c.dbg], c
    if c.dbg == 128:
        assert lib.tf_conv2d_patch_admits(c.N, c.H, c.W, c.Cin, 0, c.Cout, c.ks, c.ks, 1, c.ks // 2, 0, 0, 0, c.bm, c.bn) == 1, c
        assert lib.tf_conv2d_patch_admits(c.N, c.H, c.W, c.Cin, 0, c.Cout, 1, 1, 1, 0, 0, 0, 0, c.bm, c.bn) == 0


# ---- A. epilogue statistics ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", C.EPILOGUE_CASES, ids=_cid)
def test_epilogue_statistics(tf, c, dtype):
    assert C.form_holds(c), c
    assert_family(c)
    kind, chunks, _ = C.predict(c)
    what = f"epilogue {_cid(c)} {dtype}"
    r = launch(tf, c, dtype)
    assert r.rc == 0, (what, r.rc, r.err)
    assert r.chunks == chunks, (what, r.chunks, chunks)
    check_y(r, what)
    if kind == "none":                                        # the two refusals: y complete, the table untouched
        assert r.chunks == 0 and (r.raw.view(np.uint32) == NAN_BITS).all(), what
        return
    sbm = c.bm // 2 if c.dbg in C.PINGPONG_BITS else c.bm
    check_table(r, "epilogue", sbm, c.bn, what)
    hand_over(tf, r, "epilogue", what)


def test_forced_family_refuses_what_it_cannot_take(tf):
    """tf_gemm_debug's ping-pong bits fail by name instead of running another kernel: that is what lets rc == 0 stand for "the family ran"."""
    c = C.Conv("refused", 2, 8, 8, 64, 320, 32, 1, 64, 128, 1, 512)      # a 64-row tile: k_igemm_pp has none
    r = launch(tf, c, "fp16")
    assert r.rc == UNSUPPORTED and b"ping-pong" in r.err, (r.rc, r.err)
    c = c._replace(bm=192, bn=128, dbg=2048)                               # 1 x 1 on 8 x 8 images: no patch form
    r = launch(tf, c, "fp16")
    assert r.rc == UNSUPPORTED and b"ping-pong patch" in r.err, (r.rc, r.err)


@pytest.mark.parametrize("entry", ("fp8", "mx8"))
def test_epilogue_statistics_e4m3(tf, entry):
    """tf_conv2d_fp8 (k_igemm8, 128 x 128 tile) and tf_conv2d_mx8 (k_igemm_pp on block-scaled activations, 256 x 128 tile: 128-row statistics
    sub-blocks).  The GEMM part is not exact in e4m3: only the table and the fill are checked, against the device's y."""
    from tinyfusers_amd.native import hip, lib
    c = C.Conv("two pieces narrow last", 2, 32, 8, 128, 320, 32, 1, 128 if entry == "fp8" else 256, 128, 1, 8 if entry == "fp8" else 512)
    p = C.conv_problem(c, "fp16")
    HoWo, M = c.H * c.W, c.N * c.H * c.W
    dx, dw, db, de, dr = (dev(tf, p[k], "fp16") for k in ("x", "w", "bias", "bias_nc", "res"))
    w8 = tf.DeviceArray.empty((c.Cout * c.Cin,), np.uint8, "row")
    wscale = tf.DeviceArray.empty((c.Cout,), np.float32, "row")
    hip.tf_pack_weight_fp8(w8.ptr, wscale.ptr, dw.ptr, c.Cout, c.Cin, tf._sh())
    if entry == "fp8":
        x8 = tf.DeviceArray.empty((M * c.Cin,), np.uint8, "row")
        hip.tf_quantize_fp8_f16(x8.ptr, dx.ptr, M * c.Cin, 1.0, tf._sh())
    else:
        x8 = tf.DeviceArray.empty((lib.tf_mx8_bytes(M, c.Cin),), np.uint8, "row")
        hip.tf_quantize_mx8_f16(x8.ptr, dx.ptr, M, c.Cin, tf._sh())
    r = Run()
    r.c, r.dtype, r.p = c, "fp16", p
    r.dy = sentinel(tf, M * c.Cout, "fp16")
    r.dtable = dev32(tf, np.full((c.N * C.GN_MAX_CHUNKS * c.G * 2,), np.nan, np.float32))
    chunks = ctypes.c_int(-7)
    head = (r.dy.ptr, x8.ptr, None, w8.ptr, wscale.ptr, db.ptr, de.ptr, c.Cout, dr.ptr, c.N, c.H, c.W, c.Cin, 0, c.Cout, 1, 1, 1, 0)
    tail = (None, 0, r.dtable.ptr, r.dtable.nbytes, c.G, ctypes.byref(chunks), tf._sh())
    with forced(c.bm, c.bn, 1, c.dbg), profiled() as prof:
        rc = lib.tf_conv2d_fp8(*head, 0, *tail) if entry == "fp8" else lib.tf_conv2d_mx8(*head, *tail)
    assert rc == 0, (rc, lib.tf_last_error())
    assert_launch(prof, M, c.Cout, c.Cin, 1, c.bm, c.bn, 1, C.VARIANT_OF_BIT[c.dbg], 0, 1, 0, entry)
    sbm = c.bm if entry == "fp8" else c.bm // 2
    r.chunks = chunks.value
    assert r.chunks == 2 * (HoWo // sbm)
    r.y, r.raw = r.dy.numpy().reshape(c.N, HoWo, c.Cout), r.dtable.numpy()
    assert np.isfinite(r.y).all()                              # (e4m3 weights: y is not held to the float64 sum here)
    check_table(r, "epilogue", sbm, c.bn, f"epilogue {entry}")
    hand_over(tf, r, "epilogue", f"epilogue {entry}")


# ---- B. the reducers ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,slabs", MODES)
@pytest.mark.parametrize("c", C.PLAIN_CASES, ids=_cid)
def test_plain_reduce(tf, c, dtype, slabs):
    subsets = C.SUBSETS if c is C.PLAIN_CASES[0] else [(1, 1, 1)]
    for use in subsets:
        r = launch(tf, c, dtype, use=use, slabs=slabs, table=False)
        assert r.rc == 0, (r.rc, r.err)
        check_y(r, f"k_splitk_reduce {_cid(c)} {dtype} slabs {slabs} terms {use}")


@pytest.mark.parametrize("dtype,slabs", MODES)
def test_plain_reduce_odd_width(tf, dtype, slabs):
    """a linear with N = 50: the N % 4 != 0 path of k_splitk_reduce (fp32 slabs whatever was asked: fp16 slabs need N % 8 == 0)."""
    from tinyfusers_amd.native import lib
    M, N, K, split = C.LINEAR_N50
    x, w, g = C.gemm_inputs(1, 1, M, K, N, 1)
    res = P.gn_input(1, N, M, 5, dtype)[0][0]
    b = C.bias_of(N)
    y64 = g[0] + b.astype(np.float64) + res
    a = 3 * 2.0 ** -24 * (np.abs(g[0]) + np.abs(b) + np.abs(res))
    dx, dw, db, dr = (dev(tf, v, dtype) for v in (x, w, b, res))
    y = sentinel(tf, M * N, dtype)
    ws = tf.DeviceArray.empty((split * M * N * 4 + 64,), np.uint8, "row")
    with forced(64, 64, split, 8, slabs), profiled() as prof:
        rc = lib.tf_linear_16(tag(dtype), y.ptr, dx.ptr, dw.ptr, db.ptr, dr.ptr, M, N, K, 0, ws.ptr, ws.nbytes, tf._sh())
    assert rc == 0, (rc, lib.tf_last_error())
    assert_launch(prof, M, N, K, 1, 64, 64, split, 0, 4, 1, 0, "linear N = 50")       # fp32 slabs whatever was asked
    got = y.numpy().reshape(M, N)
    worst = float((np.abs(got - y64) / (C.half_ulp(np.abs(y64) + a, dtype) + a)).max())
    note(("y", dtype), worst)
    assert np.isfinite(got).all() and worst <= 1.0, worst


@pytest.mark.parametrize("dtype,slabs", MODES)
@pytest.mark.parametrize("c", C.REDUCE_GN_CASES, ids=_cid)
def test_reduce_with_statistics(tf, c, dtype, slabs):
    assert C.reduce_gn_form_holds(c), c
    geo = C.reduce_gn_geometry(c.H * c.W, c.Cout)
    what = f"k_splitk_reduce_gn {_cid(c)} {dtype} slabs {slabs}"
    entry = "norm" if c.form.startswith("not eligible") else "fused"     # the first HoWo the fused reduce does not take: plain reduce + apply
    r = launch(tf, c, dtype, entry=entry, slabs=slabs)
    assert r.rc == 0, (what, r.rc, r.err)
    assert r.chunks == geo["chunks"] == C.predict(c, entry)[1] and (entry == "fused" or r.z_written == 0), (what, r.chunks, r.z_written)
    check_y(r, what)
    check_table(r, "reduce_gn", geo["R"], None, what)
    if entry == "norm":
        assert (r.z == np.float32(C.round16(np.float32(C.SENTINEL), dtype))).all(), "z_written == 0 but z was touched"
    hand_over(tf, r, "reduce_gn", what)


@pytest.mark.parametrize("dtype,slabs", MODES)
@pytest.mark.parametrize("c,aff,silu", C.FUSED_CASES, ids=lambda v: _cid(v) if isinstance(v, C.Conv) else str(int(v)))
def test_reduce_applies_group_norm(tf, c, aff, silu, dtype, slabs):
    assert C.fused_form_holds(c), c
    what = f"k_splitk_reduce_gn_apply {_cid(c)} {dtype} slabs {slabs} affine={aff} silu={silu}"
    r = launch(tf, c, dtype, entry="norm", slabs=slabs, aff=aff, silu=silu)
    assert r.rc == 0, (what, r.rc, r.err)
    assert (r.chunks, r.z_written) == (1, 1), (what, r.chunks, r.z_written)
    check_y(r, what)
    check_table(r, "reduce_gn_apply", c.H * c.W, None, what)
    check_z(r.z, r.y, c.G, r.gm, r.bt, silu, dtype, "reduce_gn_apply z", what, "reduce_gn_apply")
    hand_over(tf, r, "reduce_gn_apply", what, silu=not silu)


# ---- hand-over to the concat apply ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,HoWo,C1,C2,G,sub", C.CAT_CASES)
def test_concat_apply_on_two_producers_tables(tf, N, HoWo, C1, C2, G, sub, dtype):
    """x from an epilogue producer (one or two chunks), x2 from a split-K producer (one chunk per row): different chunk counts, groups of the
    concat made of mr = 3 sub-groups, one of them on the seam."""
    from tinyfusers_amd.native import hip
    Ct = C1 + C2
    g1, g2, mr = C1 // sub, C2 // sub, (Ct // G) // sub
    assert mr == 3 and C1 % (Ct // G) != 0
    planted = P.gn_input(N, Ct, HoWo, G, dtype)[0]
    c1 = C.Conv("x", N, HoWo // 8, 8, 64, C1, g1, 1, 64, 160 if sub == 20 else 64, 1, 8)
    c2 = C.Conv("x2", N, HoWo // 8, 8, 128, C2, g2, 1, 64, 64, 2, 8)
    r1 = launch(tf, c1, dtype, res=np.ascontiguousarray(planted[..., :C1]))
    r2 = launch(tf, c2, dtype, res=np.ascontiguousarray(planted[..., C1:]))
    assert r1.rc == 0 and r2.rc == 0, (r1.err, r2.err)
    assert r1.chunks == C.predict(c1)[1] == HoWo // 64 and r2.chunks == C.predict(c2)[1] == HoWo
    check_table(r1, "epilogue", 64, c1.bn, "concat producer x")
    check_table(r2, "reduce_gn", 1, None, "concat producer x2")
    gm, bt, dgm, dbt = affine(tf, Ct, True, dtype)
    z = sentinel(tf, N * HoWo * Ct, dtype)
    hip.tf_group_norm_apply_cat_16(tag(dtype), z.ptr, r1.dy.ptr, r2.dy.ptr, dgm.ptr, dbt.ptr, r1.dtable.ptr, r1.chunks, g1, r2.dtable.ptr, r2.chunks, g2,
                                   N, HoWo, C1, C2, G, EPS, 1, tf._sh())
    y = np.concatenate([r1.y, r2.y], axis=-1)
    check_z(z.numpy().reshape(N, HoWo, Ct), y, G, gm, bt, True, dtype, "two producers -> apply_cat", f"apply_cat {C1} | {C2} {dtype}", "epilogue")


# ---- C. the input side ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H,W,C1,C2,G,ks,bm,bn,chunks,chunks2,silu", C.GI_CASES)
def test_input_group_norm_inside_the_conv(tf, N, H, W, C1, C2, G, ks, bm, bn, chunks, chunks2, silu, dtype):
    """tf_conv2d_gn_16 with selector weights on a planted x that carries host partials: the output is sign 2^k times the rounded normalised input
    (exactly 0 where a tap reads the padding), held to norm_planted.budget."""
    from tinyfusers_amd.native import lib
    Ct, HW = C1 + C2, H * W
    assert lib.tf_conv2d_gn_supported(N, H, W, C1, C2, Ct, ks, ks, 1, ks // 2, 0, 0, 0, G) == 1
    assert lib.tf_conv2d_gn_supported(*C.GI_REFUSED) == 0
    w, perm, scale, tap = C.selector(Ct, G, ks)
    x, _, _ = P.gn_input(N, Ct, HW, G, dtype)
    gm, bt, dgm, dbt = affine(tf, Ct, True, dtype)
    if C2:
        g1, g2 = C1 // C.GI_SUB, C2 // C.GI_SUB
        p1, p2 = P.partials(np.ascontiguousarray(x[..., :C1]), g1, chunks), P.partials(np.ascontiguousarray(x[..., C1:]), g2, chunks2)
        st = P.cat_stats(p1, p2, HW, C.GI_SUB, (Ct // G) // C.GI_SUB)
        dp1, dp2 = dev32(tf, p1), dev32(tf, p2)
        stats = (dp1.ptr, chunks, g1, dp2.ptr, chunks2, g2)
    else:
        p1 = P.partials(x, G, chunks)
        st = P.stats_from_partials(p1, HW, Ct // G)
        dp1 = dev32(tf, p1)
        stats = (dp1.ptr, chunks, G, None, 0, 0)
    dx = dev(tf, x[..., :C1], dtype)
    dx2 = dev(tf, x[..., C1:], dtype) if C2 else None
    dw = dev(tf, w, dtype)
    y = sentinel(tf, N * HW * Ct, dtype)
    with forced(bm, bn, 1, 0), profiled() as prof:
        rc = lib.tf_conv2d_gn_16(tag(dtype), y.ptr, dx.ptr, ptr(dx2), dw.ptr, None, None, Ct, None, N, H, W, C1, C2, Ct, ks, ks, 1, ks // 2, 0, None, 0,
                                 None, None, 0, 0, None, 0, 0, None, dgm.ptr, dbt.ptr, *stats, G, EPS, 1 if silu else 0, tf._sh())
    assert rc == 0, (rc, lib.tf_last_error())
    # k_igemm_patch<GI> for 3 x 3, k_igemm<GI> (deep ring) for 1 x 1, on the forced tile: a tile that cannot carry the table fails by name
    assert_launch(prof, N * HW, Ct, ks * ks * Ct, ks * ks, bm, bn, 1, 2 if ks == 3 else 0, 0, 0, 0, "input side")
    assert ks == 1 or lib.tf_conv2d_patch_admits(N, H, W, C1, C2, Ct, 3, 3, 1, 1, 0, 0, 0, bm, bn) == 1
    ref = P.gn_apply64(x, *st, G, gm, bt, silu)
    tol, _ = C.budget(ref, dtype, C.R, 2.0, silu, stats=True)
    want, wtol = C.selector_answer(ref, tol, w, N, H, W)
    got = y.numpy().reshape(N, HW, Ct)
    assert np.isfinite(got).all()
    pad = wtol == 0
    assert ks == 1 or pad.any()
    assert (got[pad] == 0).all(), "a padding pixel did not come out as exactly 0"
    worst = float((np.abs(got - want)[~pad] / wtol[~pad]).max())
    note(("input side", dtype), worst)
    print(f"\ninput side {(N, H, W, C1, C2, G, ks, bm, bn, chunks, chunks2, silu)} {dtype}: max |err| / tol = {worst:.3f}")
    assert worst <= 1.0, worst


def test_zz_report():
    """(prints what the cases above measured: the largest error as a fraction of its tolerance per form, fp16 | bf16)"""
    for key in sorted({k for k, _ in WORST}):
        print(f"\n{key}: " + " | ".join(f"{WORST.get((key, d), float('nan')):.3f}" for d in DTYPES))
