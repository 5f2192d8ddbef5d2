"""GPU parity tests of the BLOCK-SCALED e4m3 path (round 4; pytest -m gpu), through the C-ABI: activations carry one E8M0 scale per 32
consecutive channels of a pixel / token (an "mx8" tensor: codes, then the scale bytes) and the GEMM hands those bytes to the scale operand of
v_mfma_scale_f32_16x16x128_f8f6f4 (k_igemm_pp<F8>).  The reference has no fp8 path (fp32 throughout, example/sd1.py:33): the ops are its
vision/conv2d.py:9-28, ff/linear.py:112-121, ff/nn.py:5-23, ff/group_norm.py:13-21, ff/layer_norm.py:34-49, attention/attention.py:35-41.

  * quantisers: codes and scale bytes equal oracle.fp8.quant_act_mx_codes BIT FOR BIT on fp16 inputs;
  * GEMMs, exact: small-integer codes with a different power-of-two scale in every block -- every product and sum is exact in fp32, so the
    device result must EQUAL the integer arithmetic (any slip in which scale meets which 32 channels -- taps, half-tile slabs, tile rows --
    shows as a wrong integer);
  * GEMMs, random data: the oracle multiplies the very operands the device holds (downloaded and decoded), atol = rtol = 1e-2;
  * model level: a transformer block and the UNet with the layer policy against the oracle (gate rel-L2 <= 0.1), and
    a 3-step sampler trajectory at config 5's shape."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-2, atol=1e-2)


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def rnd(name, shape, std=1.0, seed=31):
    from tinyfusers_amd.storage.synth import synth_normal
    return synth_normal(seed, name, shape, std).astype(np.float16).astype(np.float32)


def download_mx(a):
    """(codes uint8 (rows, C), scale bytes uint8 (rows, C/32), dequantised float32 (rows, C)) of an mx8 DeviceArray, storage order."""
    from oracle import fp8 as O8
    from tinyfusers_amd.native import hip
    hip.tf_device_sync()
    c = a.shape[1] if a.ndim == 4 else a.shape[-1]
    n = a.size
    host = np.empty((n + n // 32,), dtype=np.uint8)
    hip.tf_memcpy(host.ctypes.data, a.ptr, host.size, 2)
    codes, sc = host[:n].reshape(-1, c), host[n:].reshape(-1, c // 32)
    deq = O8.decode_e4m3(codes).reshape(-1, c // 32, 32) * np.exp2(sc.astype(np.float32) - 127.0)[:, :, None]
    return codes, sc, deq.reshape(-1, c).astype(np.float32)


def upload_mx(tf, codes, scales, shape, layout):
    """host codes (rows, C) + scale bytes (rows, C/32) -> an mx8 DeviceArray of the logical `shape`."""
    from tinyfusers_amd.ff import fp8
    from tinyfusers_amd.native import hip
    a = fp8.mx_empty(shape, layout)
    host = np.concatenate([np.ascontiguousarray(codes, np.uint8).reshape(-1), np.ascontiguousarray(scales, np.uint8).reshape(-1)])
    hip.tf_memcpy(a.ptr, host.ctypes.data, host.size, 1)
    return a


class forced:
    def __init__(self, bm, bn, sk=1, flags=512):     # 512: k_igemm_pp<F8>; 2048: k_igemm_pp3<F8> (the patch form: 3x3 convs on 48 / 24-pixel rows)
        self.cfg, self.flags = (bm, bn, sk), flags

    def __enter__(self):
        from tinyfusers_amd.native import lib
        lib.tf_gemm_force_config(*self.cfg); lib.tf_gemm_debug(self.flags)

    def __exit__(self, *a):
        from tinyfusers_amd.native import lib
        lib.tf_gemm_force_config(0, 0, 0); lib.tf_gemm_debug(0)


def test_quantize_mx_matches_the_definition_bit_for_bit(tf):
    """tf_quantize_mx8_f16 against oracle.fp8.quant_act_mx_codes: blocks of very different magnitude, all-zero blocks, block maxima that are
    exact powers of two times 448 (no round-up of the exponent) and just above, fp16 subnormals, the largest fp16 values."""
    from oracle import fp8 as O8
    from tinyfusers_amd.ff import fp8
    rows, c = 257, 320
    x = rnd("mx.q", (rows, c), 1.0)
    x *= np.exp2(np.round(rnd("mx.qs", (rows, c // 32), 4.0)).clip(-14, 6)).repeat(32, axis=1)       # a different magnitude per block
    x[3, 32:64] = 0.0
    x[4, 0:32] = 0.0; x[4, 5] = 448.0                       # amax = 448: e = 0 exactly
    x[5, 0:32] = 0.0; x[5, 7] = -896.0                      # amax = 2 * 448: e = 1 exactly
    x[6, 0:32] = 0.0; x[6, 9] = 449.0                       # just above: e = 1
    x[7, 0:32] = 6e-8; x[8, 0:32] = 65504.0; x[9, 0:32] = -65504.0
    x = x.astype(np.float16).astype(np.float32)
    got = fp8.quantize_mx(tf.DeviceArray.from_numpy(x, np.float16, "row"))
    codes, sc, deq = download_mx(got)
    wc, ws = O8.quant_act_mx_codes(x)
    np.testing.assert_array_equal(sc, ws)
    np.testing.assert_array_equal(codes, wc)
    np.testing.assert_array_equal(deq, O8.quant_act_mx(x).numpy())
    assert sc[4, 0] == 127 and sc[5, 0] == 128 and sc[6, 0] == 128 and sc[3, 1] == 0
    assert np.abs(deq - x).max() <= 0.0625 * np.abs(x).reshape(rows, -1, 32).max(-1).repeat(32, axis=1).max() and not np.isnan(deq).any()
    blk = np.abs(x).reshape(rows, -1, 32).max(-1, keepdims=True)
    err = np.abs(deq - x).reshape(rows, -1, 32)
    assert (err <= blk / 224.0 * 16.0 + 1e-30).all()        # half a step of the top binade: 16 * 2^e, and 2^e < amax / 224


@pytest.mark.parametrize("rows,c", [(300, 320), (192, 1280), (77, 64)])
def test_layer_norm_and_group_norm_write_block_scaled_tensors(tf, rows, c):
    """tf_layer_norm_mx8 / tf_group_norm_apply_mx8 (+ SiLU, single source and the concat pair) = the quantiser applied to the fp32 normalised
    values.  The device normalises in fp32 with its own rounding, so a value on a code boundary may land on the neighbouring code (and a block
    maximum on the neighbouring exponent): rare, and never more than one e4m3 step of the block."""
    from oracle import fp8 as O8, ops as O
    from tinyfusers_amd.ff import fp8
    from tinyfusers_amd.ff.group_norm import GroupNorm
    from tinyfusers_amd.ff.layer_norm import LayerNorm
    dv = lambda a, lay="row": tf.DeviceArray.from_numpy(a, np.float16, lay)
    x = rnd("mx.ln", (1, rows, c), 2.0) + 0.3
    ln = LayerNorm(c, init=False); ln.weight = dv(1 + rnd("mx.g", (c,), 0.2)); ln.bias = dv(rnd("mx.b", (c,), 0.2))

    def close(deq, want):
        want = want.reshape(deq.shape)
        blk = np.abs(want).reshape(want.shape[0], -1, 32).max(-1).repeat(32, axis=1)
        assert np.isfinite(deq).all()
        assert (np.abs(deq - want) <= blk / 224.0 * 34.0 + 1e-6).all()       # one step of the top binade, 32 * 2^e with 2^e < amax / 224 (+ slack)
        assert (deq != want).mean() < 0.03
    _, _, deq = download_mx(fp8.layer_norm_mx(dv(x), ln))
    close(deq, O8.quant_act_mx(O.layer_norm(x, ln.weight.numpy(), ln.bias.numpy())).numpy())
    if c < 128:                                            # (the conv epilogue emits statistics for groups of 4 ... 64 channels)
        return
    from tinyfusers_amd.vision.conv2d import Conv2d

    def with_stats(name, n, cc, hw, G):
        """a tensor that carries the GroupNorm partials of its producer: the output of a 1x1 conv with gn = G"""
        conv = Conv2d(64, cc, [1, 1], init=False)
        conv.weight = dv(rnd(name + ".w", (cc, 64, 1, 1), 0.2), "nhwc"); conv.bias = dv(rnd(name + ".b", (cc,), 0.3))
        y = conv(dv(rnd(name + ".x", (n, 64, hw, hw), 1.0), "nhwc"), gn=G)
        assert y.gn is not None and y.gn[2] == G
        return y, y.numpy()
    n, hw = 2, 16
    for pair in (False, True):
        da, xa = with_stats("mx.ga", n, c, hw, 32)
        srcs, ds = [xa], [da]
        if pair:
            db, xb = with_stats("mx.gb", n, c // 2, hw, 16)
            srcs.append(xb); ds.append(db)
        C = sum(s_.shape[1] for s_ in srcs)
        g = GroupNorm(32, C, init=False); g.weight = dv(1 + rnd("mx.gg", (C,), 0.2)); g.bias = dv(rnd("mx.gb2", (C,), 0.2))
        got = fp8.group_norm_mx(ds[0] if len(ds) == 1 else tuple(ds), g, True)
        assert got.shape == (n, C, hw, hw)
        _, _, deq = download_mx(got)
        ref = O.silu(O.group_norm_affine(np.concatenate(srcs, 1), 32, g.weight.numpy(), g.bias.numpy()))
        close(deq, O8.quant_act_mx(ref, 1).permute(0, 2, 3, 1).numpy())


def _int_operands(name, rows_shape, c, cout, k_per_row):
    """Small-integer e4m3 codes (values -4 ... 4) with a different power-of-two scale (2^-3 ... 2^3) in every 32-channel block, and small-integer
    weights at scale 1: every product and every partial sum is an integer multiple of 2^-3 below 2^21, i.e. exact in fp32."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    vals = rng.integers(-4, 5, size=rows_shape + (c,)).astype(np.float32)
    sc = rng.integers(124, 131, size=rows_shape + (c // 32,)).astype(np.uint8)
    w = rng.integers(-2, 3, size=(cout, k_per_row)).astype(np.float32)
    return vals, sc, w


def _e4m3_codes(v):
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


CONV_MX = [   # n, c, hw, cout, r, (bm, bn, splitk)
    (2, 128, 16, 128, 3, (256, 128, 1)),     # channel counts on the 128 grid: one scale dword per row and K tile; K = 1152 = 9 tiles
    (2, 320, 32, 320, 3, (192, 160, 1)),     # 320 channels = 2.5 tiles: the halves of a K tile lie in different taps (two 2-byte scale loads)
    (2, 320, 32, 320, 3, (256, 128, 1)),
    (2, 960, 16, 640, 3, (192, 128, 2)),     # split-K; 960 = 7.5 tiles
    (3, 64, 24, 128, 3, (256, 128, 1)),      # K = 576 = 4.5 tiles, ragged last m-tile (1728 rows)
    (2, 256, 16, 256, 1, (192, 128, 1)),     # 1x1
    (8, 320, 96, 320, 3, (192, 160, 1)),     # config 5's most frequent conv, its tile
    (2, 1280, 12, 1280, 3, (256, 160, 1)),   # 256 x 160 exists on the 128 grid only; a tile spans two images (HoWo = 144 < 256: no time embedding)
    (2, 128, 24, 128, 3, (192, 128, 1, 2048)),   # the patch form (k_igemm_pp3<F8>): one 128-channel slab -- patch and scale patch from the prologue only
    (1, 384, 48, 256, 3, (192, 128, 1, 2048)),   # three slabs: both parities of the double buffers, scale loads on tap 7
    (3, 256, 24, 200, 3, (192, 128, 1, 2048)),   # ragged channel tile, several images
    (2, 640, 48, 640, 3, (192, 128, 1, 2048)),   # config 5's level-1 conv
    (1, 320, 96, 320, 3, (192, 128, 1, 2048)),   # the half-slab form: 320 channels = 2.5 slabs (the last one half full), two 2-byte scale loads per patch row; config 5's most frequent conv
    (1, 192, 48, 136, 3, (192, 128, 1, 2048)),   # 1.5 slabs, ragged channel tile
    (1, 640, 96, 320, 3, (192, 128, 1, 2048)),   # 96-pixel rows on the 128 grid (the same instance)
    (1, 960, 48, 640, 3, (192, 128, 1, 2048)),   # 7.5 slabs
]


@pytest.mark.parametrize("n,c,hw,cout,r,force", CONV_MX)
def test_conv2d_mx8_exact_integers_and_random_operands(tf, n, c, hw, cout, r, force):
    from oracle import ops as O
    from tinyfusers_amd.ff import fp8
    pad = r // 2
    dv = lambda a, lay="row": tf.DeviceArray.from_numpy(a, np.float16, lay)
    # (a) exact: integer codes, per-block power-of-two scales, integer weights, no bias
    vals, sc, w = _int_operands(f"cmx{n}{c}{hw}{cout}{r}", (n, hw, hw), c, cout, r * r * c)
    x8 = upload_mx(tf, _e4m3_codes(vals), sc, (n, c, hw, hw), "nhwc")
    w8 = tf.DeviceArray.from_numpy(_e4m3_codes(w).view(np.uint8).reshape(cout, -1), np.uint8, "row")
    one = tf.DeviceArray.from_numpy(np.ones(cout, np.float32), np.float32, "row")
    from tinyfusers_amd.native import hip
    hip.tf_gemm_splitk_partials(32)                        # (exactness: an fp16 partial slab would round the halves of a split sum before they are added)
    try:
        with forced(*force):
            y = fp8.conv2d_mx(x8, w8, one, None, (cout, c, r, r), [pad, pad]).numpy()
    finally:
        hip.tf_gemm_splitk_partials(16)
    xdeq = (vals.reshape(n, hw, hw, c // 32, 32) * np.exp2(sc.astype(np.float32) - 127.0)[..., None]).reshape(n, hw, hw, c).transpose(0, 3, 1, 2)
    wk = w.reshape(cout, r, r, c).transpose(0, 3, 1, 2)                        # KRSC storage -> KCRS
    want = O.conv_2d(xdeq, wk, (pad, pad), (1, 1), (1, 1)).numpy()
    assert np.abs(want).max() < 60000
    np.testing.assert_array_equal(y, want.astype(np.float16).astype(np.float32))
    # (b) random operands through the producers: quantise pass, packed weights with per-channel scales, bias + time embedding + residual
    x = rnd("cmx.x", (n, c, hw, hw), 1.5) * np.exp2(np.round(rnd("cmx.s", (n, 1, hw, hw), 2.0)).clip(-6, 4))     # a different magnitude per pixel
    wt = rnd("cmx.w", (cout, c, r, r), (c * r * r) ** -0.5); b = rnd("cmx.b", (cout,), 0.1)
    e = rnd("cmx.e", (n, cout), 0.5) if hw * hw >= force[0] else None
    res = rnd("cmx.r", (n, cout, hw, hw))
    xm = fp8.quantize_mx(dv(x, "nhwc"))
    wq8, wsc = fp8.pack_weight(dv(wt, "nhwc"), {})
    with forced(*force):
        yd = fp8.conv2d_mx(xm, wq8, wsc, dv(b), wt.shape, [pad, pad], bias_nc=dv(e) if e is not None else None, residual=dv(res, "nhwc"),
                           gn=32 if cout % 128 == 0 and force[2] == 1 else 0)
    _, _, deq = download_mx(xm)
    from tests.test_gpu_fp8 import raw
    wdq = (raw(wq8).reshape(cout, r, r, c) * wsc.numpy()[:, None, None, None]).transpose(0, 3, 1, 2)
    want = O.conv2d_bias(deq.reshape(n, hw, hw, c).transpose(0, 3, 1, 2), wdq, b, (pad, pad)) + torch.from_numpy(res)
    if e is not None:
        want = want + torch.from_numpy(e)[:, :, None, None]
    got = yd.numpy()
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want.numpy(), rtol=1e-2, atol=1e-2 * max(1.0, float(np.abs(want.numpy()).max()) / 8))
    if yd.gn is not None:
        from tinyfusers_amd.ff.group_norm import GroupNorm
        g = GroupNorm(32, cout, init=False); g.weight = dv(np.ones(cout, np.float32)); g.bias = dv(np.zeros(cout, np.float32))
        np.testing.assert_allclose(g(yd, silu=True).numpy(), O.silu(O.group_norm(torch.from_numpy(got), 32, 1e-5)).numpy(), **TOL)


@pytest.mark.parametrize("m,c,force", [(2 * 1024, 640, (256, 128, 1)), (1000, 320, (192, 128, 1)), (8 * 9216, 640, None), (4608, 1280, (192, 128, 1))])
def test_feed_forward_mx8_stage_by_stage(tf, m, c, force):
    """LayerNorm -> mx8, GEGLU projection (mx8 in, mx8 out: the epilogue quantises 32-channel blocks of the gated output), second Linear +
    bias + residual: ff/nn.py:14-23 on block-scaled operands.  Every stage is checked against the oracle fed with the operands the device
    produced for the stage before."""
    from oracle import fp8 as O8, ops as O
    from tinyfusers_amd import config
    from tinyfusers_amd.ff import fp8
    from tinyfusers_amd.ff.layer_norm import LayerNorm
    from tinyfusers_amd.ff.nn import FeedForward, pack_geglu
    from tests.test_gpu_fp8 import raw
    import contextlib
    x = rnd("fmx.x", (1, m, c), 1.5) + 0.1
    ff = FeedForward(c, init=False)
    w1 = rnd("fmx.w1", (8 * c, c), c ** -0.5); b1 = rnd("fmx.b1", (8 * c,), 0.1)
    w2 = rnd("fmx.w2", (c, 4 * c), (4 * c) ** -0.5); b2 = rnd("fmx.b2", (c,), 0.1)
    dv = lambda a: tf.DeviceArray.from_numpy(a, np.float16, "row")
    ff.net[0].proj.weight, ff.net[0].proj.bias, ff.net[2].weight, ff.net[2].bias = dv(w1), dv(b1), dv(w2), dv(b2)
    ln = LayerNorm(c, init=False); ln.weight = dv(1 + rnd("fmx.g", (c,), 0.1)); ln.bias = dv(rnd("fmx.bt", (c,), 0.1))
    xd = dv(x)
    h8 = fp8.layer_norm_mx(xd, ln)
    _, _, hq = download_mx(h8)
    wp, bp = pack_geglu(ff.net[0].proj.weight, ff.net[0].proj.bias)
    w8, sc = fp8.pack_weight(wp, {})
    ctx = forced(*force) if force else contextlib.nullcontext()
    with ctx:
        hid8 = fp8.linear_mx(h8, w8, sc, bp, act=1, out_features=4 * c, out_mx=True)
        codes, hsc, hidq = download_mx(hid8)
        want_hid = O.geglu(torch.from_numpy(hq.reshape(1, m, c)), O8.quant_weight(w1)[0], b1).reshape(m, 4 * c)
        wq = O8.quant_act_mx(want_hid).numpy()
        assert np.isfinite(hidq).all()
        blk = np.abs(wq).reshape(m, -1, 32).max(-1).repeat(32, axis=1)
        assert (np.abs(hidq - wq) <= blk / 224.0 * 34.0 + 1e-3).all() and (hidq != wq).mean() < 0.05
        w28, sc2 = fp8.pack_weight(ff.net[2].weight, {})
        y = fp8.linear_mx(hid8, w28, sc2, ff.net[2].bias, residual=xd).numpy()
    want = O.linear(torch.from_numpy(hidq.reshape(1, m, 4 * c)), O8.quant_weight(w2)[0], b2) + torch.from_numpy(x)
    np.testing.assert_allclose(y, want.numpy(), **TOL)
    if force is None:                                      # the module-level call (config 5's FeedForward) is those three stages where the policy admits the shape
        config.set_dtype("fp8")
        try:
            assert fp8.linear_ok(m, 4 * c, c, 1, True) and fp8.linear_ok(m, c, 4 * c)
            np.testing.assert_array_equal(ff(xd, residual=xd, ln=ln).numpy(), y)
        finally:
            config.set_dtype("fp16")


def test_linear_mx8_exact_integers(tf):
    """Plain Linear on integer codes with per-block scales: rows = tokens, K = 640 (5 K tiles), ragged M and N."""
    from tinyfusers_amd.ff import fp8
    m, k, n = 1000, 640, 328
    vals, sc, w = _int_operands("lmx", (m,), k, n, k)
    x8 = upload_mx(tf, _e4m3_codes(vals), sc, (m, k), "row")
    w8 = tf.DeviceArray.from_numpy(_e4m3_codes(w).reshape(n, k), np.uint8, "row")
    one = tf.DeviceArray.from_numpy(np.ones(n, np.float32), np.float32, "row")
    want = (vals.reshape(m, k // 32, 32) * np.exp2(sc.astype(np.float32) - 127.0)[..., None]).reshape(m, k) @ w.T
    from tinyfusers_amd.native import hip
    for cfg in ((192, 128, 1), (256, 160, 1), (192, 160, 2)):
        hip.tf_gemm_splitk_partials(32)                    # (exactness across the split: see the conv test)
        try:
            with forced(*cfg):
                y = fp8.linear_mx(x8, w8, one, None).numpy()
        finally:
            hip.tf_gemm_splitk_partials(16)
        np.testing.assert_array_equal(y, want.astype(np.float16).astype(np.float32))


def test_unsupported_shapes_are_refused_and_the_policy_keeps_them_in_fp16(tf):
    from tinyfusers_amd import config
    from tinyfusers_amd.ff import fp8
    from tinyfusers_amd.native import lib
    assert lib.tf_mx8_gemm_supported(8 * 9216, 1920, 640, 0, 0) == 1 and lib.tf_mx8_gemm_supported(8 * 9216, 2560, 640, 1, 1) == 1
    assert lib.tf_mx8_gemm_supported(512, 3840, 1280, 0, 0) == 0              # batch 1, 16 x 16 level: 3 x 30 tiles of 192 x 128 cannot fill the chip
    assert lib.tf_mx8_conv_supported(8, 96, 96, 320, 0, 320, 3, 3, 1, 1, 0) == 1
    assert lib.tf_mx8_conv_supported(8, 96, 96, 320, 0, 320, 3, 3, 2, 1, 0) == 0 and lib.tf_mx8_conv_supported(8, 12, 12, 1280, 0, 1280, 3, 3, 1, 1, 0) == 0
    # "supported" is about filling the chip: a small launch still RUNS on the kernel (one tile) when a caller insists ...
    xs, ws_ = rnd("u.x", (64, 64)), rnd("u.w", (64, 64), 0.1)
    x8 = fp8.quantize_mx(tf.DeviceArray.from_numpy(xs, np.float16, "row"))
    w8, sc = fp8.pack_weight(tf.DeviceArray.from_numpy(ws_, np.float16, "row"), {})
    from oracle import fp8 as O8
    y = fp8.linear_mx(x8, w8, sc, None).numpy()
    np.testing.assert_allclose(y, (O8.quant_act_mx(xs) @ O8.quant_weight(ws_)[0].t()).numpy(), **TOL)
    # ... and what the kernel cannot do is refused with a status, never run on something else: a time-embedding bias on tiles that span more than
    # two images (12 x 12 pixels per image against 192-row tiles), a stride-2 convolution
    xc = fp8.quantize_mx(tf.DeviceArray.from_numpy(rnd("u.xc", (8, 128, 12, 12)), np.float16, "nhwc"))
    wc8, wcs = fp8.pack_weight(tf.DeviceArray.from_numpy(rnd("u.wc", (128, 128, 3, 3), 0.05), np.float16, "nhwc"), {})
    emb = tf.DeviceArray.from_numpy(rnd("u.e", (8, 128)), np.float16, "row")
    with pytest.raises(RuntimeError, match="tf_conv2d_mx8 failed with status 10002"):
        fp8.conv2d_mx(xc, wc8, wcs, None, (128, 128, 3, 3), [1, 1], bias_nc=emb)
    assert np.isfinite(fp8.conv2d_mx(xc, wc8, wcs, None, (128, 128, 3, 3), [1, 1]).numpy()).all()      # (without the time embedding it runs)
    from tinyfusers_amd.native import hip
    with pytest.raises(RuntimeError, match="tf_conv2d_mx8 failed with status 10001"):
        hip.tf_conv2d_mx8(xc.ptr, xc.ptr, None, wc8.ptr, wcs.ptr, None, None, 0, None, 8, 12, 12, 128, 0, 128, 3, 3, 2, 1, None, 0, None, 0, 0, None, None)
    config.set_dtype("fp8")
    try:
        assert not fp8.linear_ok(8 * 9216, 960, 320) and fp8.linear_ok(8 * 9216, 1920, 640)     # K = 320 stays fp16 (MIN_K)
    finally:
        config.set_dtype("fp16")


def test_transformer_block_fp8_policy_against_the_oracle(tf):
    """BasicTransformerBlock at the channel count of config 5's second level (9216 token rows, 640 channels: every projection of x, to_out and the FeedForward pair on
    block-scaled e4m3 operands) against the oracle's restatement of the same policy fed with the same fp16 inputs."""
    import oracle
    from oracle import fp8 as O8
    from tinyfusers_amd import config
    from tinyfusers_amd.attention.attention import BasicTransformerBlock
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_state_dict
    b, t, c, cd, nh = 2, 4608, 640, 768, 8            # (half of config 5's second level: 9216 rows still fill the chip with 192-row tiles; the oracle's fp32 score matrix stays at 1.4 GB)
    shapes = {k[len("input_blocks.4.1.transformer_blocks.0."):]: v for k, v in oracle.unet_param_shapes(oracle.SD15).items() if k.startswith("input_blocks.4.1.transformer_blocks.0.")}
    W = synth_state_dict(shapes, 3)
    blk = BasicTransformerBlock(c, cd, nh, c // nh, init=False)
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(blk, W, "")
    x = rnd("tb.x", (b, t, c), 1.0); ctx = rnd("tb.c", (b, 77, cd), 1.0)
    Wt = {"p." + k: torch.from_numpy(v.astype(np.float16).astype(np.float32)) for k, v in W.items()}
    torch.set_num_threads(16)
    ref32 = oracle.basic_transformer_block(torch.from_numpy(x), torch.from_numpy(ctx), Wt, "p", nh).numpy()
    from tinyfusers_amd.ff import fp8
    with O8.policy(attention=True):
        ref8 = oracle.basic_transformer_block(torch.from_numpy(x), torch.from_numpy(ctx), Wt, "p", nh).numpy()
    config.set_dtype("fp8")
    saved = fp8.ATTENTION
    fp8.ATTENTION = True                                   # (off by default: measured slower; the path stays covered here)
    try:
        got = blk(tf.DeviceArray.from_numpy(x, np.float16, "row"), context=tf.DeviceArray.from_numpy(ctx, np.float16, "row")).numpy()
    finally:
        fp8.ATTENTION = saved
        config.set_dtype("fp16")
    rl = lambda a, r: float(np.linalg.norm(a - r) / np.linalg.norm(r))
    assert np.isfinite(got).all()
    assert rl(ref8, ref32) > 2e-3                           # the policy quantises something at this shape
    assert rl(got, ref8) <= 0.6 * rl(ref8, ref32) + 2e-3, (rl(got, ref8), rl(ref8, ref32))    # the device follows the SAME quantised computation (independent rounding noise would read sqrt(2) x)
    assert rl(got, ref32) <= 0.05


def test_three_step_fp8_sampler_trajectory_config5(tf):
    """Config 5 is a sampler configuration: three DDIM steps (the compiled graph) at its per-GPU shape -- 4 images, 96 x 96 latents -- with the
    fp8 layer policy, against the fp32 oracle trajectory of image 0 (variants/sd.py:56-59 three times).  The latent is the sampler state: the
    UNet's fp8 error (<= 0.1 of its output, both CFG halves) enters it through the guidance combination (g = 7.5 amplifies the difference of
    the halves) and the DDIM coefficients.  Gate: rel-L2 <= 0.05 after every step (measured 0.024 after the first; the fp16 path reads 1e-3)."""
    import oracle
    from tinyfusers_amd import config
    from tests.test_gpu_fp8 import _sd_fp8
    images, S = 4, 96
    sd, W, lat, ctx, unc = _sd_fp8(tf, images, S, 91)
    lat = lat.astype(np.float32); ctx = ctx.astype(np.float16).astype(np.float32); unc = unc.astype(np.float16).astype(np.float32)
    ts, al, ap = oracle.sampler_schedule(50)
    Wt = {k: torch.from_numpy(v.astype(np.float32)) for k, v in W.items()}
    torch.set_num_threads(16)
    config.set_dtype("fp8")
    try:
        dl = sd.latent_from_numpy(lat)
        sd.compile(tf.DeviceArray.from_numpy(unc), tf.DeviceArray.from_numpy(ctx), dl, timesteps=[ts[49], ts[48], ts[47]])
        ref = torch.from_numpy(lat[0:1])
        for n, i in enumerate((49, 48, 47)):
            sd.step(ts[i], al[i], ap[i], 7.5)
            sd.synchronize()
            got = dl.numpy()[0:1]
            ref = oracle.sd_step(unc[0:1], ctx[0:1], ref, np.array([ts[i]], np.float32), al[i:i + 1], ap[i:i + 1], np.array([7.5]), Wt)
            r = float(np.linalg.norm(got - ref.numpy()) / np.linalg.norm(ref.numpy()))
            assert np.isfinite(got).all() and r <= 0.05, (n, r)
            print(f"fp8 trajectory, step {n}: latent rel-L2 {r:.4f}")
    finally:
        config.set_dtype("fp16")
