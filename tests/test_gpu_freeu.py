"""GPU checks of FreeU (csrc/freeu.hip, UNetModel.__call__(freeu=), StableDiffusion.compile(..., freeu=True), set_freeu, start(freeu=)): the
two kernels against float64 within the budget of tests/aux/freeu_ref.py over its whole case table (planted planes, guard words, aliasing,
bit-exact copies at 1, repeatability, refusals), a tiny UNet forward per parameter against the CPU restatement, tiny sampler trajectories
(graph == eager, reproducible, set_freeu without a re-capture, all ones against a freeu=False compile, bf16, under a ControlNet, cfg=False),
the argument checks, and the SD-1.5 shapes end to end."""
import contextlib
import ctypes
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))
import controlnet_oracle as C  # noqa: E402
import freeu_ref as R  # noqa: E402
from test_samplers_host import randn_ref  # noqa: E402

SEED = 0x243F6A8885A308D3
G = 7.5
FILL, GUARD = 0x7E55, 64
QUOTED = (0.9, 0.2, 1.5, 1.6)          # the values usually quoted for SD-1.5


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def _gate(got, ref, rel_l2=5e-3, max_rel=1e-2, what=""):
    """tests/test_gpu_samplers.py's gate: rel-L2 and max |d| <= max_rel max |ref|."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all()
    rl2 = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    mx = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"gate {what}: rel-L2 {rl2:.3e} (gate {rel_l2}), max|d|/max|ref| {mx:.3e} (gate {max_rel}), max|ref| {np.abs(ref).max():.2f}")
    assert rl2 <= rel_l2 and mx <= max_rel, (what, rl2, mx)


def _raw16(tf, words):
    return tf.DeviceArray.from_numpy(np.ascontiguousarray(words, dtype=np.uint16), np.uint16, "row")


def _read16(a):
    return a.numpy().astype(np.uint16)


def _nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1)).reshape(-1)


def _nchw(flat, B, C, H, W):
    return flat.reshape(B, H, W, C).transpose(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def _plane(B, C, H, W, dtype):
    return R.planted(B, C, H, W, dtype)


@functools.lru_cache(maxsize=None)
def _ref(B, C, H, W, dtype, s):
    """(float64 reference, tol) of the planted case under scale s: computed once, shared, never written."""
    x = _plane(B, C, H, W, dtype)[1]
    y = R.closed_form(x, s)
    return y, R.budget(y, x, s, dtype)[0]


def _specials(dtype):
    """-0, +inf, -inf and a NaN with a payload, as bit patterns."""
    return np.array([0x8000, 0x7F80, 0xFF80, 0x7FC5] if dtype == "bf16" else [0x8000, 0x7C00, 0xFC00, 0x7E05], np.uint16)


# ---- 1. tf_freeu_skip_16 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_freeu_skip_matches_float64_within_the_budget_over_the_case_table(tf, dtype):
    """Every (H, W) of the table in ONE launch of 8 entries, for every C and B, four times with the scale indices rotated: every (shape, s) of
    the table.  Guard words behind every dst, sources unchanged, the s = 1 entries bit-identical to their sources (-0, +-inf and a NaN payload
    planted there), dst == src the bits of out of place, a second launch the bits of the first."""
    from tinyfusers_amd.native import FreeuEntry, hip
    tag = 1 if dtype == "bf16" else 0
    d_scales = tf.DeviceArray.from_numpy(np.asarray(R.SCALES + (7.0, 7.0, 7.0, 7.0), np.float32), np.float32, "row")
    worst = 0.0
    for C in R.CASES_C:
        for B in R.CASES_B:
            for rot in range(4):
                sidx = [(k + rot) % 4 for k in range(len(R.CASES_HW))]
                srcs = []
                for (H, W), si in zip(R.CASES_HW, sidx):
                    bits = _nhwc(_plane(B, C, H, W, dtype)[0]).copy()
                    if R.SCALES[si] == 1.0:
                        bits[:4] = _specials(dtype)
                    srcs.append(bits)

                def launch(alias):
                    d_src = [_raw16(tf, np.concatenate([b, np.full(GUARD, FILL, np.uint16)])) for b in srcs]
                    d_dst = d_src if alias else [_raw16(tf, np.full(b.size + GUARD, FILL, np.uint16)) for b in srcs]
                    table = (FreeuEntry * len(srcs))()
                    for e, d, s_, (H, W), si in zip(table, d_dst, d_src, R.CASES_HW, sidx):
                        e.dst, e.src, e.B, e.H, e.W, e.C, e.scale_index = d.ptr, s_.ptr, B, H, W, C, si
                    hip.tf_freeu_skip_16(tag, ctypes.cast(table, ctypes.c_void_p), len(srcs), d_scales.ptr, None)
                    outs = [_read16(d) for d in d_dst]
                    for o, b in zip(outs, srcs):
                        assert np.all(o[b.size:] == FILL), (B, C, b.size)                 # the guard words behind each dst
                    if not alias:
                        for s_, b in zip(d_src, srcs):
                            assert np.array_equal(_read16(s_)[:b.size], b)                # out of place: the sources are read only
                    return [o[:b.size] for o, b in zip(outs, srcs)]

                out = launch(False)
                for o, b, (H, W), si in zip(out, srcs, R.CASES_HW, sidx):
                    s = R.SCALES[si]
                    if s == 1.0:
                        assert np.array_equal(o, b), (B, H, W, C)                         # the copy: the source's bits
                        continue
                    y, tol = _ref(B, C, H, W, dtype, s)
                    err = np.abs(_nchw(R.from16(o, dtype), B, C, H, W) - y)
                    worst = max(worst, float(np.max(err / tol)))
                    assert np.all(err <= tol), (dtype, B, H, W, C, s, float(np.max(err / tol)))
                if rot == 0 or (C, B) == (72, 3):
                    for a, b in zip(launch(True), out):
                        assert np.array_equal(a, b)                                       # dst aliasing src: the same bits
                    for a, b in zip(launch(False), out):
                        assert np.array_equal(a, b)                                       # a second launch: the same bits
    # one launch whose entries differ in everything: B, H, W, C and the scale index
    mixed = [((1, 2, 2, 8), 0), ((3, 16, 16, 328), 2), ((1, 5, 7, 72), 1), ((3, 6, 4, 8), 3), ((1, 12, 12, 328), 2), ((3, 3, 8, 72), 0)]
    srcs = [_nhwc(_plane(B, C, H, W, dtype)[0]) for (B, H, W, C), _ in mixed]
    d_src = [_raw16(tf, b) for b in srcs]
    d_dst = [_raw16(tf, np.full(b.size + GUARD, FILL, np.uint16)) for b in srcs]
    table = (FreeuEntry * len(mixed))()
    for e, d, s_, ((B, H, W, C), si) in zip(table, d_dst, d_src, mixed):
        e.dst, e.src, e.B, e.H, e.W, e.C, e.scale_index = d.ptr, s_.ptr, B, H, W, C, si
    hip.tf_freeu_skip_16(tag, ctypes.cast(table, ctypes.c_void_p), len(mixed), d_scales.ptr, None)
    for d, b, ((B, H, W, C), si) in zip(d_dst, srcs, mixed):
        o = _read16(d)
        assert np.all(o[b.size:] == FILL)
        if R.SCALES[si] == 1.0:
            assert np.array_equal(o[:b.size], b)
            continue
        y, tol = _ref(B, C, H, W, dtype, R.SCALES[si])
        err = np.abs(_nchw(R.from16(o[:b.size], dtype), B, C, H, W) - y)
        worst = max(worst, float(np.max(err / tol)))
        assert np.all(err <= tol), (dtype, "mixed", B, H, W, C, R.SCALES[si])
    print(f"freeu_skip {dtype}: max err / tol over the table = {worst:.3f} (bound 1)")


def test_freeu_skip_refuses_bad_entries(tf):
    from tinyfusers_amd.native import FreeuEntry, hip
    d_scales = tf.DeviceArray.from_numpy(np.ones(4, np.float32), np.float32, "row")
    buf = _raw16(tf, np.zeros(4096, np.uint16))
    table = (FreeuEntry * 2)()

    def fill(**kw):
        for e in table:
            e.dst, e.src, e.B, e.H, e.W, e.C, e.scale_index = buf.ptr, buf.ptr, 1, 4, 4, 16, 0
        for k, v in kw.items():
            setattr(table[1], k, v)
    for kw, match in ((dict(src=None), "entry 1 holds a null pointer"), (dict(C=12), "entry 1 has B=1, C=12"), (dict(H=1), "entry 1 has H=1"),
                      (dict(W=1), "W=1"), (dict(dst=buf.ptr + 8), "entry 1 is not 16-byte aligned")):
        fill(**kw)
        with pytest.raises(RuntimeError, match=match):
            hip.tf_freeu_skip_16(0, ctypes.cast(table, ctypes.c_void_p), 2, d_scales.ptr, None)
    fill()
    with pytest.raises(RuntimeError, match="n_entries"):
        hip.tf_freeu_skip_16(0, ctypes.cast(table, ctypes.c_void_p), 9, d_scales.ptr, None)
    hip.tf_freeu_skip_16(0, ctypes.cast(table, ctypes.c_void_p), 2, d_scales.ptr, None)      # (and the good table runs: scale 1 in place)
    assert not _read16(buf).any()


# ---- 2. tf_freeu_backbone_16 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_freeu_backbone_is_one_fp32_multiply_and_one_rounding_bit_for_bit(tf, dtype):
    """rows x C for C = 16 (one vector per half), 48 (an odd number of vectors per half), 1296 with a ragged last block, and 5000 x 1280 --
    800,000 vectors, more than the 2048 x 256 lanes of the largest grid, so the loop strides (in place its 400,000 do not: both ends of the
    rule); b in {1.5, 1.6, -0.37, 1}.  First half: numpy's fp32 product rounded to nearest even, bit for bit.  Second half: the source's bits."""
    from tinyfusers_amd.native import hip
    tag = 1 if dtype == "bf16" else 0
    bs = np.array([1.0, 1.0, 1.5, 1.6, -0.37, 1.0, 0.0, 0.0], np.float32)
    d_scales = tf.DeviceArray.from_numpy(bs, np.float32, "row")
    rng = np.random.default_rng(23)
    for rows, Cc in ((37, 16), (37, 48), (301, 1296), (5000, 1280)):
        x32 = (3 * rng.standard_normal((rows, Cc))).astype(np.float32)
        x32[0, :4] = [0.0, -0.0, 6e-6, 1000.0]
        bits, val = R.round16(x32, dtype)
        bits = bits.copy()
        bits[1, :4] = _specials(dtype); bits[1, Cc // 2:Cc // 2 + 4] = _specials(dtype)
        val = R.from16(bits, dtype)
        for idx in ((2, 5) if rows == 5000 else (2, 3, 4, 5)):
            b = bs[idx]

            def launch(alias):
                d_src = _raw16(tf, np.concatenate([bits.reshape(-1), np.full(GUARD, FILL, np.uint16)]))
                d_dst = d_src if alias else _raw16(tf, np.full(bits.size + GUARD, FILL, np.uint16))
                hip.tf_freeu_backbone_16(tag, d_dst.ptr, d_src.ptr, rows, Cc, d_scales.ptr, idx, None)
                o = _read16(d_dst)
                assert np.all(o[bits.size:] == FILL)
                if not alias:
                    assert np.array_equal(_read16(d_src)[:bits.size], bits.reshape(-1))
                return o[:bits.size].reshape(rows, Cc)

            out = launch(False)
            assert np.array_equal(out[:, Cc // 2:], bits[:, Cc // 2:]), (rows, Cc, b)           # the second half: copied bits
            if b == 1.0:
                assert np.array_equal(out, bits)                                                # b = 1 copies the bits, specials included
            else:
                with np.errstate(invalid="ignore", over="ignore"):
                    want = R.round16(np.float32(b) * val[:, :Cc // 2].astype(np.float32), dtype)[0]
                fin = np.isfinite(val[:, :Cc // 2])
                assert np.array_equal(out[:, :Cc // 2][fin], want[fin]), (rows, Cc, b)
                sp = R.from16(out[1, :4], dtype)
                assert np.signbit(sp[0]) == (b > 0) and sp[0] == 0 and np.isinf(sp[1]) and np.isinf(sp[2]) and np.isnan(sp[3])
            assert np.array_equal(launch(True), out)                                            # in place == out of place
    buf = _raw16(tf, np.zeros(1024, np.uint16))
    with pytest.raises(RuntimeError, match="C=24"):
        hip.tf_freeu_backbone_16(tag, buf.ptr, buf.ptr, 4, 24, d_scales.ptr, 2, None)


# ---- 3. tiny UNet forward -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny(seed=5):
    import oracle
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    W = synth_state_dict(oracle.unet_param_shapes(oracle.TINY), seed)
    Wc = synth_state_dict(C.controlnet_param_shapes(oracle.TINY), seed + 1)
    ctx = synth_normal(seed, "c", (2, 13, 64)).astype(np.float16).astype(np.float32)
    unc = synth_normal(seed, "u", (2, 13, 64)).astype(np.float16).astype(np.float32)
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (2, 128, 128, 3), dtype=np.uint8)
    img[:, 32:96, 32:96] = 255
    return W, Wc, ctx, unc, img


def _f32(W):
    return {k: torch.from_numpy(v.astype(np.float32)) for k, v in W.items()}


@functools.lru_cache(maxsize=None)
def _forward_ref(hw, freeu):
    import oracle
    from tinyfusers_amd.storage.synth import synth_normal
    W, _, ctx = _tiny()[:3]
    x = synth_normal(5, "lat", (2, 4) + hw).astype(np.float16).astype(np.float32)
    return x, R.unet_forward(x, np.array([481.0], np.float32), ctx, _f32(W), oracle.TINY, freeu=freeu).numpy()


def test_tiny_unet_forward_reads_every_freeu_parameter(tf):
    """Batch 2, 16 x 16 latent (4 x 4 and 8 x 8 stages): each parameter alone, all four, and a 24 x 16 latent (6 x 4 and 12 x 8 stages) once.
    The reference with FreeU must differ from the plain reference by >= 10 x the gate, so a step that ignores a parameter cannot pass."""
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.vision.unet import TINY, StepParams, UNetModel
    W, _, ctx = _tiny()[:3]
    unet = UNetModel(TINY); update_state(unet, W, "")
    d_ctx = tf.DeviceArray.from_numpy(ctx)
    runs = [((16, 16), p) for p in ((0.2, 1, 1, 1), (1, 0.2, 1, 1), (1, 1, 1.5, 1), (1, 1, 1, 1.6), QUOTED)] + [((24, 16), QUOTED)]
    for hw, p in runs:
        p = tuple(float(v) for v in p)
        x, plain = _forward_ref(hw, None)
        _, ref = _forward_ref(hw, p)
        moved = float(np.linalg.norm(ref - plain) / np.linalg.norm(plain))
        print(f"freeu {p} at {hw}: the reference moves by rel-L2 {moved:.3f}")
        assert moved >= 10 * 5e-3
        d_x = tf.DeviceArray.from_numpy(x, np.float16, "nhwc")
        scales = tf.DeviceArray.from_numpy(np.asarray(p, np.float32), np.float32, "row")
        got = unet(d_x, StepParams().set(481.0), d_ctx, freeu=scales).numpy()
        _gate(got, ref, what=f"tiny forward freeu={p} {hw}")
    x, plain = _forward_ref((16, 16), None)
    d_x = tf.DeviceArray.from_numpy(x, np.float16, "nhwc")
    base = unet(d_x, StepParams().set(481.0), d_ctx).numpy()
    _gate(base, plain, what="tiny forward, freeu=None")
    ones = unet(d_x, StepParams().set(481.0), d_ctx, freeu=tf.DeviceArray.from_numpy(np.ones(4, np.float32), np.float32, "row")).numpy()
    _gate(ones, plain, what="tiny forward, all ones")
    assert np.array_equal(unet(d_x, StepParams().set(481.0), d_ctx).numpy(), base)           # freeu=None: the step as it was, again
    with pytest.raises(ValueError, match="4 fp32 values"):
        unet(d_x, StepParams().set(481.0), d_ctx, freeu=tf.DeviceArray.from_numpy(np.ones(2, np.float32), np.float32, "row"))


# ---- 4. tiny sampler trajectories --------------------------------------------------------------------------------------------------------------------
def _oracle_trajectory(lat0, sch, freeu=None, img=None, cfg=True):
    """tests/test_gpu_controlnet.py's sampler loop on the restatement with FreeU: img: under a ControlNet at scale 1 (both CFG groups read the
    same hint embedding); cfg=False: the conditional group alone, e = its output."""
    import oracle
    W, Wc, ctx, unc = _tiny()[:4]
    Wf, Wcf = _f32(W), _f32(Wc)
    x, xp = lat0.astype(np.float64), np.zeros(lat0.shape)
    B, n_img = lat0.shape[0], lat0[0].size
    c2 = np.concatenate([unc[:B], ctx[:B]]) if cfg else ctx[:B]
    if img is not None:
        emb = C.hint_embedding((img.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2), Wcf)
        emb2 = torch.cat([emb, emb]) if cfg else emb
    for i, t in enumerate(sch.timesteps):
        x32 = x.astype(np.float32)
        xin, tt = (np.concatenate([x32, x32]) if cfg else x32), np.array([t], np.float32)
        r = C.controlnet_forward(xin, None, tt, c2, Wcf, oracle.TINY, hint_emb=emb2) if img is not None else None
        out = R.unet_forward(xin, tt, c2, Wf, oracle.TINY, control=r, freeu=freeu).numpy().astype(np.float64)
        e = out[:B] + G * (out[B:] - out[:B]) if cfg else out
        a_t = sch.alphas[i]
        x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
        z = np.stack([randn_ref(SEED, b, n_img, i, 1).reshape(lat0.shape[1:]) for b in range(B)])
        c_x, c_0, c_1, c_n = sch.coeffs[i]
        x, xp = c_x * x + c_0 * x0 + c_1 * xp + c_n * z, x0
    return x


def _model(tf, sch, freeu=True, cfg=True, control=False):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.controlnet import ControlNet
    from tinyfusers_amd.vision.unet import TINY
    W, Wc, ctx, unc = _tiny()[:4]
    sd = StableDiffusion(TINY); update_state(sd.model.diffusion_model, W, "")
    if control:
        net = ControlNet(TINY); update_state(net, Wc, "")
        sd.attach_control(net)
    lat = sd.latent_from_numpy(np.zeros((2, 4, 16, 16), np.float32))
    sd.compile(tf.DeviceArray.from_numpy(unc) if cfg else None, tf.DeviceArray.from_numpy(ctx), lat, sampler=sch, cfg=cfg, control=control, freeu=freeu)
    return sd, lat


def _final(sd, lat, eager=False, guidance=G, **kw):
    sd.start(seed=SEED, **kw)
    lat0 = lat.numpy().copy()
    sd.run(guidance, eager=eager); sd.synchronize()
    return lat0, lat.numpy().copy()


def _sched(n=3):
    from tinyfusers_amd.variants import samplers as S
    return S.DPMSolverPP2M().schedule(n)


def test_tiny_freeu_sampler_graph_eager_seed_restatement_and_set_freeu(tf):
    sch = _sched()
    sd, lat = _model(tf, sch)
    graph = sd._graph
    assert sd._freeu_scales.numpy().tolist() == [1.0] * 4
    lat0, a = _final(sd, lat, freeu=QUOTED)
    _, b = _final(sd, lat, eager=True)                                       # (the scalars keep their values without freeu=)
    _, c = _final(sd, lat, freeu=QUOTED)
    np.testing.assert_array_equal(a, b)                                       # graph replay == eager
    np.testing.assert_array_equal(a, c)                                       # same seed, same bits
    _gate(a, _oracle_trajectory(lat0, sch, QUOTED), what="dpmpp2m freeu")
    # set_freeu between two starts: no re-capture, and the bits of a fresh compile followed by the same set_freeu
    other = (0.6, 0.4, 1.2, 1.4)
    sd.set_freeu(*other)
    _, d = _final(sd, lat)
    assert sd._graph is graph and float(np.abs(d - a).max()) > 0.02
    fresh, flat = _model(tf, sch)
    fresh.set_freeu(*other)
    np.testing.assert_array_equal(_final(fresh, flat)[1], d)
    _gate(d, _oracle_trajectory(lat0, sch, other), what="dpmpp2m freeu, second values")
    # all ones: the un-FreeU'd model within the gate (another GroupNorm statistics path: not bit for bit), and far from the FreeU'd result
    sd.set_freeu()
    _, one = _final(sd, lat)
    plain, plat = _model(tf, sch, freeu=False)
    _, p = _final(plain, plat)
    _gate(one, p, what="all ones vs a freeu=False compile")
    _gate(one, _oracle_trajectory(lat0, sch), what="all ones vs the plain restatement")
    assert float(np.abs(a - p).max()) > 0.02


def test_tiny_freeu_sampler_in_the_bf16_step(tf):
    """Once in the bfloat16 step, over the 3-step schedule of this file's float16 trajectories.  Gate: the project's float16 trajectory gate
    (rel-L2 5e-3, max 1e-2) times 2^3, the ratio of the two types' unit roundoffs (2^-8 against 2^-11): rel-L2 4e-2, max 8e-2.  The 3e-2 / 3e-2
    the suite holds un-FreeU'd bfloat16 trajectories to is no bound for this one: b1 = 1.5 and b2 = 1.6 grow the activations every rounding acts
    on, and two runs on MI355X measured 3.08e-2 / 3.06e-2 and 2.98e-2 / 2.61e-2 (the GEMM tuner's choices for TINY's shapes differ between
    processes) -- 9 x the 3.3e-3 / 3.4e-3 of the float16 twin above, which is the precision ratio, not a defect (the kernels' own bfloat16
    arithmetic is held to its float64 budget in the first two tests)."""
    from tinyfusers_amd import config
    sch = _sched()
    config.set_dtype("bf16")
    try:
        sd, lat = _model(tf, sch)
        lat0, a = _final(sd, lat, freeu=QUOTED)
        _, b = _final(sd, lat, eager=True)
    finally:
        config.set_dtype("fp16")
    np.testing.assert_array_equal(a, b)
    _gate(a, _oracle_trajectory(lat0, sch, QUOTED), rel_l2=8 * 5e-3, max_rel=8 * 1e-2, what="bf16 freeu")


def test_tiny_freeu_under_a_controlnet_filters_after_the_residual_add(tf):
    img = _tiny()[4]
    sch = _sched()
    sd, lat = _model(tf, sch, control=True)
    lat0, a = _final(sd, lat, control_image=img, freeu=QUOTED)
    _, b = _final(sd, lat, eager=True, control_image=img)
    np.testing.assert_array_equal(a, b)
    _gate(a, _oracle_trajectory(lat0, sch, QUOTED, img), what="control + freeu")
    assert float(np.abs(a - _oracle_trajectory(lat0, sch, None, img)).max()) > 0.02


def test_tiny_freeu_without_guidance(tf):
    sch = _sched()
    sd, lat = _model(tf, sch, cfg=False)
    lat0, a = _final(sd, lat, guidance=None, freeu=QUOTED)
    _, b = _final(sd, lat, eager=True, guidance=None)
    np.testing.assert_array_equal(a, b)
    _gate(a, _oracle_trajectory(lat0, sch, QUOTED, cfg=False), what="cfg=False freeu")


# ---- 5. argument checks ----------------------------------------------------------------------------------------------------------------------------------
def test_freeu_arguments_are_checked_and_a_refusal_leaves_the_model_running(tf):
    from tinyfusers_amd import config
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    W, _, ctx, unc = _tiny()[:4]
    sch = _sched(2)
    sd, lat = _model(tf, sch)
    sd.set_freeu(*QUOTED)
    _, want = _final(sd, lat)
    d_ctx, d_unc = tf.DeviceArray.from_numpy(ctx), tf.DeviceArray.from_numpy(unc)
    new_lat = lambda shape=(2, 4, 16, 16): StableDiffusion.latent_from_numpy(np.zeros(shape, np.float32))

    def still_runs():
        assert sd._freeu_scales.numpy().tolist() == [float(np.float32(v)) for v in QUOTED]
        assert np.array_equal(_final(sd, lat)[1], want)

    with pytest.raises(ValueError, match="freeu=True needs a sampler"):
        sd.compile(d_unc, d_ctx, new_lat(), freeu=True)
    still_runs()
    with pytest.raises(ValueError, match="at least 2 x 2"):
        sd.compile(d_unc, d_ctx, new_lat((2, 4, 4, 4)), sampler=sch, freeu=True)
    still_runs()
    config.set_dtype("fp8")
    try:
        with pytest.raises(S.UnsupportedSamplerConfig, match="fp8"):
            sd.compile(d_unc, d_ctx, new_lat(), sampler=sch, freeu=True)
    finally:
        config.set_dtype("fp16")
    still_runs()
    for bad in ((1.0, 1.0, 1.0, float("nan")), (float("inf"), 1.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match="four finite floats"):
            sd.set_freeu(*bad)
        with pytest.raises(ValueError, match="four finite floats"):
            sd.start(seed=SEED, freeu=bad)
    for bad in ((1.0, 1.0, 1.0), 0.5, "abcd"):
        with pytest.raises(ValueError, match="four finite floats"):
            sd.start(seed=SEED, freeu=bad)
    with pytest.raises(ValueError, match="seed"):                          # start checks everything, then writes: the scalars stay
        sd.start(freeu=(1.0, 1.0, 1.0, 1.0))
    still_runs()
    # a model compiled without freeu refuses both ways in and runs its plain step
    plain, plat = _model(tf, sch, freeu=False)
    with pytest.raises(ValueError, match="freeu=True"):
        plain.set_freeu(*QUOTED)
    with pytest.raises(ValueError, match="freeu=True"):
        plain.start(seed=SEED, freeu=QUOTED)
    _, p = _final(plain, plat)
    assert np.isfinite(p).all() and not np.array_equal(p, want)


# ---- 6. SD-1.5 shapes ---------------------------------------------------------------------------------------------------------------------------------------
def test_sd15_two_freeu_steps(tf):
    import oracle
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.variants.samplers import DPMSolverPP2M
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import SD15
    sd = StableDiffusion(SD15)
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(sd.model.diffusion_model, synth_state_dict(oracle.unet_param_shapes(oracle.SD15), 0), "")
    ctx = tf.DeviceArray.from_numpy(synth_normal(1234, "sd.context", (1, 77, 768)))
    unc = tf.DeviceArray.from_numpy(synth_normal(1234, "sd.uncond", (1, 77, 768)))
    lat = sd.latent_from_numpy(np.zeros((1, 4, 64, 64), np.float32))
    sd.compile(unc, ctx, lat, sampler=DPMSolverPP2M().schedule(2), freeu=True)
    _, a = _final(sd, lat, freeu=QUOTED)
    _, b = _final(sd, lat, eager=True)
    _, c = _final(sd, lat)
    assert np.isfinite(a).all() and np.array_equal(a, b) and np.array_equal(a, c)
    sd.set_freeu()
    _, one = _final(sd, lat)
    assert np.isfinite(one).all() and float(np.abs(one - a).max()) > 1e-3
    sd.compile(unc, ctx, lat, sampler=DPMSolverPP2M().schedule(2))            # the plain step of the same weights
    _, p = _final(sd, lat)
    assert np.isfinite(p).all() and float(np.abs(p - a).max()) > 1e-3 and float(np.abs(p - one).max()) < float(np.abs(p - a).max())
