"""Group-major split-K partial slabs (GemmP::slab_gm, tf_gemm_splitk_slab_layout) in front of k_splitk_reduce_gn_apply: 3 x 3 convs with GroupNorm
+ SiLU behind them through the raw entry tf_conv2d_fused_norm_16, tile / split / kernel family forced as tests/test_gpu_splitk.py forces them.
Every case runs the same launch with the switch off (row-major slabs: the parent's path) and on, and asserts

  * the launch that ran: tf_prof_dump's row shows the tile, the split count and the variant, the split-K reduce family one launch over the
    effective number of slabs of the asked width, and z_written = 1 says it was the fused reduce + GroupNorm;
  * y, z and the one-chunk statistics table of the two arms are EQUAL (the summation order of every value is the parent's);
  * the slabs themselves: the group-major workspace, un-permuted with the host copy of the address map (tests/aux/splitk_slabs.py), equals the
    row-major workspace of the other arm bit for bit;
  * the workspace behind the last slab still holds the poison it was filled with (the workspace size does not change);
  * y and z against the oracle at the tolerance of tests/test_gpu_splitk.py (rtol = atol = 1e-2).
The ping-pong kernel does not implement the layout: its case shows the switch leaves its slabs row-major and the results right.
Reference ops: vision/conv2d.py:9-58, ff/group_norm.py:3-21, vision/resnet.py:17-22."""
import contextlib
import ctypes
import functools
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import splitk_slabs as S  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 1e-5
GN_MAX_CHUNKS = 192
POISON = 0xA5
VARIANT_OF_BIT = {8: 0, 128: 2, 512: 4}
PINGPONG = S.Shape("ping-pong keeps row-major", 2, 16, 16, 64, 160, 4, 256, 160, 2)


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


@functools.lru_cache(maxsize=None)
def problem(s):
    """inputs (values of float16, held as float32; NHWC / KRSC as the entry takes them) and the oracle's y (N, HoWo, Cout); computed once per shape."""
    from oracle import ops as O
    rng = np.random.default_rng([7, s.N, s.H, s.Cin, s.Cout])
    h = lambda a: a.astype(np.float16).astype(np.float32)
    p = dict(x=h(rng.standard_normal((s.N, s.H, s.W, s.Cin))), w=h(rng.standard_normal((s.Cout, 3, 3, s.Cin)) * (9 * s.Cin) ** -0.5),
             bias=h(rng.standard_normal(s.Cout) * 0.1), bias_nc=h(rng.standard_normal((s.N, s.Cout)) * 0.5),
             res=h(rng.standard_normal((s.N, s.H * s.W, s.Cout))), gamma=h(1 + rng.standard_normal(s.Cout) * 0.1), beta=h(rng.standard_normal(s.Cout) * 0.1))
    conv = O.conv2d_bias(p["x"].transpose(0, 3, 1, 2), p["w"].transpose(0, 3, 1, 2), p["bias"], (1, 1)).numpy()
    p["conv"] = conv.transpose(0, 2, 3, 1).reshape(s.N, s.H * s.W, s.Cout)
    for v in p.values():
        v.setflags(write=False)
    return p


def z_oracle(s, p, y):
    from oracle import ops as O
    t = torch.from_numpy(np.ascontiguousarray(y.reshape(s.N, s.H, s.W, s.Cout).transpose(0, 3, 1, 2)))
    return O.silu(O.group_norm_affine(t, s.G, p["gamma"], p["beta"])).numpy().transpose(0, 2, 3, 1).reshape(y.shape)


@contextlib.contextmanager
def forced(s, bit, slabs, layout):
    from tinyfusers_amd.native import hip, lib
    hip.tf_gemm_splitk_partials(slabs)
    hip.tf_gemm_splitk_slab_layout(layout)
    lib.tf_gemm_force_config(s.bm, s.bn, s.split)
    hip.tf_gemm_debug(bit)
    hip.tf_prof_enable(1)
    try:
        yield
    finally:
        hip.tf_prof_enable(0)
        lib.tf_gemm_force_config(0, 0, 0)
        lib.tf_gemm_debug(0)
        lib.tf_gemm_splitk_partials(16)
        lib.tf_gemm_splitk_slab_layout(1)


class Run:
    pass


def launch(tf, s, bit, slabs, layout, extras):
    from tinyfusers_amd.native import hip, lib
    p = problem(s)
    HoWo, M, N, K = s.H * s.W, s.N * s.H * s.W, s.Cout, 9 * s.Cin
    eff = S.eff_splitk(K, s.split)
    f16 = lambda a: tf.DeviceArray.from_numpy(np.ascontiguousarray(a).reshape(-1), np.float16, "row")
    dx, dw, db, dgm, dbt = (f16(p[k]) for k in ("x", "w", "bias", "gamma", "beta"))
    de, dr = (f16(p["bias_nc"]), f16(p["res"])) if extras else (None, None)
    ptr = lambda a: a.ptr if a is not None else None
    dy = f16(np.full(M * N, -77.0, np.float32))
    dz = f16(np.full(M * N, -77.0, np.float32))
    dtable = tf.DeviceArray.from_numpy(np.full((s.N * GN_MAX_CHUNKS * s.G * 2,), np.nan, np.float32), np.float32, "row")
    ws_bytes = s.split * M * N * 4                             # what the entry is told: fp32 slabs of the split count ASKED for (the dispatcher drops the split otherwise), whatever the layout
    ws = tf.DeviceArray.from_numpy(np.full((ws_bytes + 4096,), POISON, np.uint8), np.uint8, "row")
    chunks, zw = ctypes.c_int(-7), ctypes.c_int(-7)
    r = Run()
    with forced(s, bit, slabs, layout):
        rc = lib.tf_conv2d_fused_norm_16(0, dy.ptr, dx.ptr, None, dw.ptr, db.ptr, ptr(de), N, ptr(dr), s.N, s.H, s.W, s.Cin, 0, N, 3, 3, 1, 1, 0,
                                         ws.ptr, ws_bytes, None, None, 0, 0, dtable.ptr, dtable.nbytes, s.G, ctypes.byref(chunks),
                                         dz.ptr, dgm.ptr, dbt.ptr, EPS, 1, ctypes.byref(zw), tf._sh())
        assert rc == 0, (rc, lib.tf_last_error())
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "prof.csv")
            hip.tf_prof_dump(path.encode())
            rows = [tuple(int(v) for v in ln.split(",")[:9]) for ln in open(path).read().splitlines()[1:]]
        ms, work, n = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_longlong(0)
        hip.tf_prof_read_family(2, ctypes.byref(ms), ctypes.byref(work), ctypes.byref(n))
    slab_bytes = 2 if slabs == 16 else 4
    what = (s.name, bit, slabs, layout, extras)
    # the launch that ran: tile, split (the row holds the count ASKED for; the reduce counters below the slabs that exist: eff), variant; ONE reduce
    # launch over eff slabs of the asked width that also wrote z; one-chunk table
    assert rows == [(M, N, K, 9, s.bm, s.bn, s.split, VARIANT_OF_BIT[bit], 1)], (what, rows)
    assert (n.value, work.value) == (1, float(M) * N * eff * slab_bytes + float(M) * N * 2.0 * (2 + (1 if extras else 0))), (what, n.value, work.value)
    assert (chunks.value, zw.value) == (1, 1), (what, chunks.value, zw.value)
    r.y, r.z = dy.numpy().reshape(s.N, HoWo, N), dz.numpy().reshape(s.N, HoWo, N)
    raw = dtable.numpy()
    r.table = raw[:s.N * s.G * 2].reshape(s.N, s.G, 2)
    assert np.isfinite(r.table).all() and np.isnan(raw[s.N * s.G * 2:]).all(), what
    wsb = ws.numpy().astype(np.uint8)
    used = eff * M * N * slab_bytes
    assert (wsb[used:] == POISON).all(), (what, "the workspace behind the last slab was written", int((wsb[used:] != POISON).sum()))
    r.slabs = wsb[:used].view(np.float16 if slabs == 16 else np.float32).reshape(eff, M * N)
    return r


def both_arms(tf, s, bit, slabs, extras=True, group_major=True):
    p = problem(s)
    HoWo, N = s.H * s.W, s.Cout
    off, on = launch(tf, s, bit, slabs, 0, extras), launch(tf, s, bit, slabs, 1, extras)
    np.testing.assert_array_equal(on.y, off.y)
    np.testing.assert_array_equal(on.z, off.z)
    np.testing.assert_array_equal(on.table, off.table)
    unpermuted = np.stack([S.to_row_major(sl, N, HoWo, s.G) for sl in on.slabs]) if group_major else on.slabs.reshape(len(on.slabs), -1, N)
    np.testing.assert_array_equal(unpermuted.view(np.uint16 if slabs == 16 else np.uint32), off.slabs.reshape(unpermuted.shape).view(np.uint16 if slabs == 16 else np.uint32))
    if group_major:
        assert not np.array_equal(on.slabs, off.slabs), "the switch changed nothing: the group-major arm did not run"
    want = p["conv"] + (p["bias_nc"][:, None, :] + p["res"] if extras else 0.0)
    np.testing.assert_allclose(on.y, want, rtol=1e-2, atol=1e-2)
    np.testing.assert_allclose(on.z, z_oracle(s, p, on.y), rtol=1e-2, atol=1e-2)
    assert np.abs(on.y).max() < 100 and not (on.y == -77.0).any() and not (on.z == -77.0).any()


@pytest.mark.parametrize("slabs", (16, 32))
@pytest.mark.parametrize("bit", (8, 128), ids=("k_igemm", "k_igemm_patch"))
@pytest.mark.parametrize("s", S.SHAPES, ids=lambda s: s.name.replace(" ", "_"))
def test_group_major_slabs_equal_row_major(tf, s, bit, slabs):
    from tinyfusers_amd.native import lib
    # bit 128 asks for k_igemm_patch; a tile it has no form for (one that spans two images) runs k_igemm's deep ring under the same variant number
    admits = lib.tf_conv2d_patch_admits(s.N, s.H, s.W, s.Cin, 0, s.Cout, 3, 3, 1, 1, 0, 0, 0, s.bm, s.bn)
    assert admits == (1 if (s.H * s.W) % s.bm == 0 else 0), (s, admits)
    both_arms(tf, s, bit, slabs)


@pytest.mark.parametrize("slabs", (16, 32))
def test_without_residual_and_time_embedding(tf, slabs):
    both_arms(tf, S.SHAPES[1], 128, slabs, extras=False)


def test_ping_pong_keeps_row_major_slabs(tf):
    both_arms(tf, PINGPONG, 512, 16, group_major=False)


def test_switch_refuses_other_values():
    from tinyfusers_amd.native import lib
    assert lib.tf_gemm_splitk_slab_layout(2) == 10001 and b"tf_gemm_splitk_slab_layout" in lib.tf_last_error()
    assert lib.tf_gemm_splitk_slab_layout(1) == 0
