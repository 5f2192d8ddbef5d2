"""GPU checks of the ControlNet path (csrc/control.hip, vision/controlnet.py, UNetModel.__call__(control=), StableDiffusion.compile(...,
control=True), start(control_image= / control_hint=, control_scale=)): the two kernels against float64, a tiny ControlNet's residuals and hint
stem against the CPU restatement tests/aux/controlnet_oracle.py, tiny controlled trajectories (graph == eager, reproducible, against the
oracle, a new hint and scale without a recompile, scale 0 == the uncontrolled trajectory, bf16, with the inpainting blend), a checkpoint file,
the argument checks, and the SD-1.5 shapes end to end."""
import contextlib
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
from test_samplers_host import randn_ref  # noqa: E402

SEED = 0x243F6A8885A308D3          # a seed with both key words nonzero
G = 7.5


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


def _to16(x, dtype):
    """fp32 -> (uint16 bit patterns, the float64 values they hold) in the step's 16-bit type, round to nearest even."""
    from tinyfusers_amd.storage.tensor import bf16_bits_to_f32, f32_to_bf16_bits
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "bf16":
        bits = f32_to_bf16_bits(x)
        return bits, bf16_bits_to_f32(bits).astype(np.float64)
    h = x.astype(np.float16)
    return h.view(np.uint16), h.astype(np.float64)


def _from16(bits, dtype):
    from tinyfusers_amd.storage.tensor import bf16_bits_to_f32
    return (bf16_bits_to_f32(bits) if dtype == "bf16" else bits.view(np.float16).astype(np.float32)).astype(np.float64)


def _raw16(tf, words):
    return tf.DeviceArray.from_numpy(np.ascontiguousarray(words, dtype=np.uint16), np.uint16, "row")


def _read16(a):
    return a.numpy().astype(np.uint16)


# ---- 1. tf_control_add_16 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_control_add_matches_float64_keeps_scale_zero_exact_and_may_alias(tf, dtype):
    """Three entries, n = 8 (one vector), 8 x 257 (a second block's worth of lanes and a ragged end) and 8 x 1031 (more than one block of
    1024 vectors), scales (0, 1, -0.37).  Bound: the kernel rounds fmaf(s, r, k) (one fp32 rounding) to 16 bits -- at most one unit in the last
    place of the result, 2^-10 relative in fp16 and 2^-7 in bf16, plus 2^-24 for results in fp16's subnormal range."""
    import ctypes
    from tinyfusers_amd.native import ControlEntry, hip
    ns, scales = (8, 8 * 257, 8 * 1031), np.array([0.0, 1.0, -0.37], np.float32)
    rng = np.random.default_rng(17)
    guard, fill = 64, 0x7E55
    tag = 1 if dtype == "bf16" else 0
    skips, ress = [], []
    for n in ns:
        k, r = (3 * rng.standard_normal(n)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        k[:4] = [0.0, -0.0, 6e-6, 1000.0]
        skips.append(_to16(k, dtype)); ress.append(_to16(r, dtype))
    inf = 0x7F80 if dtype == "bf16" else 0x7C00
    ress[0][0][2], ress[0][0][5] = inf, inf | 0x8000                    # +inf and -inf under the scale-0 entry: 0 * inf would be NaN
    d_scales = tf.DeviceArray.from_numpy(scales, np.float32, "row")
    d_res = [_raw16(tf, r[0]) for r in ress]

    def launch(alias):
        d_skip = [_raw16(tf, np.concatenate([k[0], np.full(guard, fill, np.uint16)])) for k in skips]
        d_dst = d_skip if alias else [_raw16(tf, np.full(n + guard, fill, np.uint16)) for n in ns]
        table = (ControlEntry * 3)()
        for e, d, k, r, n in zip(table, d_dst, d_skip, d_res, ns):
            e.dst, e.skip, e.residual, e.n = d.ptr, k.ptr, r.ptr, n
        hip.tf_control_add_16(tag, ctypes.cast(table, ctypes.c_void_p), 3, d_scales.ptr, None)
        outs = [_read16(d) for d in d_dst]
        for o, n in zip(outs, ns):
            assert np.all(o[n:] == fill), n                               # the guard words behind each dst
        if not alias:
            for k, dk, n in zip(skips, d_skip, ns):
                assert np.array_equal(_read16(dk)[:n], k[0])              # out of place: the skips are read only
        return [o[:n] for o, n in zip(outs, ns)]

    out = launch(False)
    assert np.array_equal(out[0], skips[0][0])                            # scale 0: the skip's bits, -0 and the residual's infinities included
    rel = 2.0 ** -7 if dtype == "bf16" else 2.0 ** -10
    for i in (1, 2):
        ref = skips[i][1] + np.float64(scales[i]) * ress[i][1]
        err = np.abs(_from16(out[i], dtype) - ref)
        print(f"control_add {dtype} n={ns[i]} s={scales[i]}: max err / (rel |ref| + 2^-24) = {float(np.max(err / (rel * np.abs(ref) + 2.0 ** -24))):.3f} (bound 1)")
        assert np.all(err <= rel * np.abs(ref) + 2.0 ** -24)
    assert np.array_equal(out[1], _to16((skips[1][1] + ress[1][1]).astype(np.float32), dtype)[0])     # s = 1: the correctly rounded sum (exact in fp32)
    for a, b in zip(launch(True), out):
        assert np.array_equal(a, b)                                       # dst aliasing skip: the same bits
    table = (ControlEntry * 1)()
    with pytest.raises(RuntimeError, match="null pointer"):
        hip.tf_control_add_16(tag, ctypes.cast(table, ctypes.c_void_p), 1, d_scales.ptr, None)


# ---- 2. tf_hint_from_u8_16 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_hint_from_u8_is_x_over_255_for_all_values(tf, dtype):
    from tinyfusers_amd.native import hip
    tag = 1 if dtype == "bf16" else 0
    rel = 2.0 ** -7 if dtype == "bf16" else 2.0 ** -10
    for n, off in ((256, 0), (256 + 3 * 5 * 7 * 3, 1)):                   # the vector form; an odd count from an odd address: the scalar form
        u = np.r_[np.arange(256), np.random.default_rng(n).integers(0, 256, n - 256)].astype(np.uint8)
        d_u = tf.DeviceArray.from_numpy(np.r_[np.zeros(off, np.uint8), u], np.uint8, "row")
        out = _raw16(tf, np.full(n + 16, 0x7E55, np.uint16))
        hip.tf_hint_from_u8_16(tag, out.ptr, d_u.ptr + off, n, None)
        bits = _read16(out)
        assert np.all(bits[n:] == 0x7E55)
        got, ref = _from16(bits[:n], dtype), u.astype(np.float64) / 255.0
        assert np.all(np.abs(got - ref) <= rel * ref)
        assert got[0] == 0.0 and bits[0] == 0 and got[255] == 1.0
        assert np.array_equal(bits[:n], _to16((u.astype(np.float32) / np.float32(255.0)), dtype)[0])      # one fp32 division, one rounding


# ---- 3. - 5. tiny ControlNet ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny(seed=5):
    import oracle
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    W = synth_state_dict(oracle.unet_param_shapes(oracle.TINY), seed)
    Wc = synth_state_dict(C.controlnet_param_shapes(oracle.TINY), seed + 1)          # non-zero zero convs
    ctx = synth_normal(seed, "c", (2, 13, 64)).astype(np.float16).astype(np.float32)
    unc = synth_normal(seed, "u", (2, 13, 64)).astype(np.float16).astype(np.float32)
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (2, 128, 128, 3), dtype=np.uint8)
    img[:, 32:96, 32:96] = 255                                            # a bright square on noise
    img2 = np.ascontiguousarray(img[::-1, :, ::-1])
    x0 = synth_normal(seed, "x0", (2, 4, 16, 16))
    return W, Wc, ctx, unc, img, img2, x0


def _f32(W):
    return {k: torch.from_numpy(v.astype(np.float32)) for k, v in W.items()}


def _hint_of(img):
    return (img.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)


def _known_ref(x0_init, a_s, seed, row):
    """tests/test_gpu_img2img.py: float64 sqrt(a_s) x0_init + sqrt(1 - a_s) z2, z2 the tag-2 noise of schedule row `row`."""
    a_s = np.float64(np.float32(a_s))
    n_img = x0_init[0].size
    z2 = np.stack([randn_ref(seed, b, n_img, row, 2).reshape(x0_init.shape[1:]) for b in range(x0_init.shape[0])])
    return np.sqrt(a_s) * x0_init.astype(np.float64) + np.sqrt(1 - a_s) * z2


def _oracle_trajectory(lat0, sch, img=None, scale=1.0, x0_init=None, mask=None):
    """The sampler of tests/test_gpu_samplers.py on the CPU restatement: both CFG groups read the same hint embedding; scale: one float or one per
    residual; img None: the uncontrolled UNet."""
    import oracle
    W, Wc, ctx, unc = _tiny()[:4]
    Wf, Wcf = _f32(W), _f32(Wc)
    x, xp = lat0.astype(np.float64), np.zeros(lat0.shape)
    B, n_img = lat0.shape[0], lat0[0].size
    c2 = np.concatenate([unc[:B], ctx[:B]])
    if img is not None:
        emb = C.hint_embedding(_hint_of(img), Wcf)
        emb = emb.expand(B, -1, -1, -1) if emb.shape[0] == 1 else emb
        emb2 = torch.cat([emb, emb])
        s = np.broadcast_to(np.asarray(scale, np.float32), (len(oracle.unet._graph(oracle.TINY)[0]) + 1,))
    for i, t in enumerate(sch.timesteps):
        x32 = x.astype(np.float32)
        xin, tt = np.concatenate([x32, x32]), np.array([t], np.float32)
        if img is None:
            out = oracle.unet_forward(xin, tt, c2, Wf, oracle.TINY)
        else:
            r = C.controlnet_forward(xin, None, tt, c2, Wcf, oracle.TINY, hint_emb=emb2)
            out = C.unet_forward(xin, tt, c2, Wf, oracle.TINY, control=[float(si) * v for si, v in zip(s, r)])
        out = out.numpy().astype(np.float64)
        e = out[:B] + G * (out[B:] - out[:B])
        a_t = sch.alphas[i]
        x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
        z = np.stack([randn_ref(SEED, b, n_img, i, 1).reshape(lat0.shape[1:]) for b in range(B)])
        c_x, c_0, c_1, c_n = sch.coeffs[i]
        x, xp = c_x * x + c_0 * x0 + c_1 * xp + c_n * z, x0
        if mask is not None:
            x = mask * x + (1 - mask) * _known_ref(x0_init, sch.alphas_prev[i], SEED, i)
    return x


def _model(tf, sch, inpaint=False, net=None):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.controlnet import ControlNet
    from tinyfusers_amd.vision.unet import TINY
    W, Wc, ctx, unc = _tiny()[:4]
    sd = StableDiffusion(TINY); update_state(sd.model.diffusion_model, W, "")
    if net is None:
        net = ControlNet(TINY); update_state(net, Wc, "")
    sd.attach_control(net)
    lat = sd.latent_from_numpy(np.zeros((2, 4, 16, 16), np.float32))
    sd.compile(tf.DeviceArray.from_numpy(unc), tf.DeviceArray.from_numpy(ctx), lat, sampler=sch, inpaint=inpaint, control=True)
    return sd, lat


def _final(sd, lat, eager=False, **kw):
    sd.start(seed=SEED, **kw)
    lat0 = lat.numpy().copy()
    sd.run(G, eager=eager); sd.synchronize()
    return lat0, lat.numpy().copy()


def test_tiny_controlnet_residuals_and_hint_stem_match_the_oracle(tf):
    import oracle
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_normal
    from tinyfusers_amd.vision.controlnet import ControlNet
    from tinyfusers_amd.vision.unet import TINY
    W, Wc, ctx, unc, img = _tiny()[:5]
    net = ControlNet(TINY); update_state(net, Wc, "")
    hint = _hint_of(img).astype(np.float16).astype(np.float32)            # (the values the device reads)
    x = synth_normal(5, "lat", (2, 4, 16, 16)).astype(np.float16).astype(np.float32)
    emb = net.hint_embedding(tf.DeviceArray.from_numpy(hint, np.float16, "nhwc"))
    ref_emb = C.hint_embedding(hint, _f32(Wc)).numpy()
    assert emb.shape == (2, 64, 16, 16)
    _gate(emb.numpy(), ref_emb, what="hint_embedding")
    t = np.array([481.0], np.float32)
    res = net(tf.DeviceArray.from_numpy(x, np.float16, "nhwc"), emb, t, tf.DeviceArray.from_numpy(ctx))
    ref = C.controlnet_forward(x, hint, t, ctx, _f32(Wc), oracle.TINY)
    assert len(res) == len(ref) == len(net.input_blocks) + 1 == 10
    for i, (a, b) in enumerate(zip(res, ref)):
        assert a.shape == tuple(b.shape) and a.gn is None and a.normed is None
        _gate(a.numpy(), b.numpy(), what=f"residual {i}")
    # the same residuals from the hoisted form: one GEMV row, one K|V GEMM, handed in as `shared`
    from tinyfusers_amd.vision.unet import StepParams
    d_ctx = tf.DeviceArray.from_numpy(ctx)
    _, row, kv = net.step_shared(StepParams().set(481.0), d_ctx)
    assert row.shape == (1, sum(r.emb_layers[1].weight.shape[0] for r in net._all(type(net.middle_block[0]))))
    again = net(tf.DeviceArray.from_numpy(x, np.float16, "nhwc"), emb, None, d_ctx, shared=(None, row, kv))
    for a, b in zip(res, again):
        assert np.array_equal(a.numpy(), b.numpy())


@pytest.mark.parametrize("name", ["dpmpp2m", "euler-a"])
def test_tiny_controlled_sampler_graph_eager_seed_oracle_new_hint_and_scales(tf, name):
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    W, Wc, ctx, unc, img, img2, _ = _tiny()
    sch = S.make(name).schedule(10, strength=0.6)                # the 6 steps of the img2img / concat trajectories, here from the seed's noise
    assert len(sch.timesteps) == 6
    sd, lat = _model(tf, sch)
    graph_before = sd._graph
    lat0, a = _final(sd, lat, control_image=img)
    np.testing.assert_array_equal(lat0, StableDiffusion.randn_latent((2, 4, 16, 16), SEED).numpy())
    _, b = _final(sd, lat, eager=True, control_image=tf.DeviceArray.from_numpy(img, np.uint8, "row"))
    _, c = _final(sd, lat, control_hint=_hint_of(img))
    np.testing.assert_array_equal(a, b)                          # graph replay == eager (and a device image == a host image)
    np.testing.assert_array_equal(a, c)                          # same seed, same bits (and the float hint of the same image)
    _gate(a, _oracle_trajectory(lat0, sch, img), what=f"{name} controlled")
    if name != "dpmpp2m":
        return
    # another hint (one image for both latents) at scale 0.5, no recompile
    _, d = _final(sd, lat, control_image=img2[:1], control_scale=0.5)
    assert sd._graph is graph_before
    _gate(d, _oracle_trajectory(lat0, sch, img2[:1], 0.5), what="second hint, scale 0.5")
    moved = float(np.abs(d - a).max())
    print(f"another hint and scale move the latent by max |d| = {moved:.3f}")
    assert moved > 0.05
    # one strength per residual; the next start without control_scale is back at 1
    per = np.linspace(0.0, 1.2, 10).astype(np.float32)
    _, e = _final(sd, lat, control_image=img, control_scale=per)
    _gate(e, _oracle_trajectory(lat0, sch, img, per), what="per-residual scales")
    _, f = _final(sd, lat, control_image=img)
    np.testing.assert_array_equal(f, a)
    # scale 0: the uncontrolled trajectory (the decoder still takes the explicit-statistics GroupNorm path)
    _, z = _final(sd, lat, control_image=img, control_scale=0)
    _gate(z, _oracle_trajectory(lat0, sch), what="scale 0 vs the uncontrolled oracle")
    # set_context refreshes the ControlNet's hoisted K|V with the UNet's: equal to a fresh compile with those contexts
    sd.set_context(tf.DeviceArray.from_numpy(ctx), tf.DeviceArray.from_numpy(unc))
    _, sw = _final(sd, lat, control_image=img)
    assert float(np.abs(sw - a).max()) > 0.05
    fresh = _model_swapped(tf, sch)
    _, fr = _final(*fresh, control_image=img)
    np.testing.assert_array_equal(sw, fr)


def _model_swapped(tf, sch):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.controlnet import ControlNet
    from tinyfusers_amd.vision.unet import TINY
    W, Wc, ctx, unc = _tiny()[:4]
    sd = StableDiffusion(TINY); update_state(sd.model.diffusion_model, W, "")
    net = ControlNet(TINY); update_state(net, Wc, "")
    lat = sd.latent_from_numpy(np.zeros((2, 4, 16, 16), np.float32))
    sd.attach_control(net).compile(tf.DeviceArray.from_numpy(ctx), tf.DeviceArray.from_numpy(unc), lat, sampler=sch, control=True)
    return sd, lat


def test_tiny_controlled_sampler_in_the_bf16_step(tf):
    """The DPM++2M run in the bfloat16 step, once, at the bf16 gates tests/test_gpu_concat.py uses and over the schedule they were set for: the
    full 10 steps from noise."""
    from tinyfusers_amd import config
    from tinyfusers_amd.variants import samplers as S
    img = _tiny()[4]
    sch = S.DPMSolverPP2M().schedule(10)
    config.set_dtype("bf16")
    try:
        sd, lat = _model(tf, sch)
        lat0, a = _final(sd, lat, control_image=img)
        _, b = _final(sd, lat, eager=True, control_image=img)
    finally:
        config.set_dtype("fp16")
    np.testing.assert_array_equal(a, b)
    _gate(a, _oracle_trajectory(lat0, sch, img), rel_l2=3e-2, max_rel=3e-2, what="bf16 controlled")


def test_control_with_inpaint_keeps_the_known_half_on_its_trajectory(tf):
    """tests/test_gpu_img2img.py's half-mask check on a controlled model: after every step the kept half is sqrt(a_s) x0_init + sqrt(1 - a_s) z2
    to 2e-6 (1 + |known|); the whole latent meets the controlled oracle with the blend."""
    from tinyfusers_amd.variants import samplers as S
    img, _, x0 = _tiny()[4:]
    sch = S.DPMSolverPP2M().schedule(10, strength=0.6)
    sd, lat = _model(tf, sch, inpaint=True)
    m = np.zeros((2, 1, 16, 16), np.float32); m[..., :8] = 1.0
    sd.start(seed=SEED, init_latent=x0, mask=m, control_image=img)
    lat0 = lat.numpy().copy()
    keep = np.broadcast_to(m == 0, lat0.shape)
    for i in range(len(sch.timesteps)):
        sd.step_sampler(i, G); sd.synchronize()
        got = lat.numpy()
        known = _known_ref(x0, sch.alphas_prev[i], SEED, i)
        assert np.all(np.abs(got[keep] - known[keep]) <= 2e-6 * (1 + np.abs(known[keep]))), i
    _gate(got, _oracle_trajectory(lat0, sch, img, 1.0, x0, m), what="control + inpaint")
    _, again = _final(sd, lat, eager=True, init_latent=x0, mask=m, control_image=img)
    np.testing.assert_array_equal(got, again)


# ---- 6. checkpoint file ---------------------------------------------------------------------------------------------------------------------
def test_control_model_tensors_load_from_a_checkpoint_file(tf, tmp_path):
    import oracle
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_normal
    from tinyfusers_amd.storage.unpicker import load_checkpoint, save_safetensors
    from tinyfusers_amd.vision.controlnet import ControlNet
    from tinyfusers_amd.vision.unet import TINY
    W, Wc, ctx, unc, img = _tiny()[:5]
    path = str(tmp_path / "control_tiny.safetensors")
    save_safetensors(path, {"control_model." + k: v for k, v in Wc.items()} | {"model.diffusion_model.out.2.bias": np.zeros(4, np.float16)})

    asked = set()

    class Recording(dict):
        def __contains__(self, k):
            asked.add(k)
            return dict.__contains__(self, k)

    loaded, mem = ControlNet(TINY), ControlNet(TINY)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        update_state(loaded, Recording(load_checkpoint(path)), "control_model.")
        update_state(mem, Wc, "")
    assert "skipped" not in buf.getvalue(), buf.getvalue()
    # (update_state also probes the bias slot of the bias-free q / k / v projections, as for every model: no checkpoint holds those)
    probes = {k for k in asked if k.endswith((".to_q.bias", ".to_k.bias", ".to_v.bias"))}
    assert asked - probes == {"control_model." + k for k in C.controlnet_param_shapes(oracle.TINY)}
    x = tf.DeviceArray.from_numpy(synth_normal(5, "lat", (2, 4, 16, 16)), np.float16, "nhwc")
    hint = tf.DeviceArray.from_numpy(_hint_of(img), np.float16, "nhwc")
    d_ctx, t = tf.DeviceArray.from_numpy(ctx), np.array([481.0], np.float32)
    ra, rb = (n(x, n.hint_embedding(hint), t, d_ctx) for n in (loaded, mem))
    assert len(ra) == 10
    for a, b in zip(ra, rb):
        assert np.array_equal(a.numpy(), b.numpy()) and np.abs(a.numpy()).max() > 0


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_control_arguments_are_checked_and_a_refusal_leaves_the_model_running(tf):
    from dataclasses import replace
    from tinyfusers_amd import config
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.controlnet import ControlNet
    from tinyfusers_amd.vision.unet import TINY
    W, Wc, ctx, unc, img, img2, _ = _tiny()
    sch = S.DPMSolverPP2M().schedule(2)
    sd, lat = _model(tf, sch)
    _, want = _final(sd, lat, control_image=img)
    d_ctx, d_unc = tf.DeviceArray.from_numpy(ctx), tf.DeviceArray.from_numpy(unc)
    new_lat = lambda: StableDiffusion.latent_from_numpy(np.zeros((2, 4, 16, 16), np.float32))

    def still_runs():
        _, got = _final(sd, lat, control_image=img)
        assert np.array_equal(got, want)

    # compile(): no net attached, no sampler, concat=, the fp8 policy -- on the compiled model itself, which keeps running
    net, sd.control_model = sd.control_model, None
    with pytest.raises(ValueError, match="attach_control"):
        sd.compile(d_unc, d_ctx, new_lat(), sampler=sch, control=True)
    sd.control_model = net
    still_runs()
    with pytest.raises(ValueError, match="sampler"):
        sd.compile(d_unc, d_ctx, new_lat(), control=True)
    still_runs()
    with pytest.raises(ValueError, match="concat="):
        sd.compile(d_unc, d_ctx, new_lat(), sampler=sch, concat="inpaint", control=True)
    nine = StableDiffusion(replace(TINY, in_channels=9)).attach_control(ControlNet(replace(TINY, in_channels=9)))
    with pytest.raises(ValueError, match="concat="):
        nine.compile(d_unc, d_ctx, new_lat(), sampler=sch, concat="inpaint", control=True)
    still_runs()
    config.set_dtype("fp8")
    try:
        with pytest.raises(S.UnsupportedSamplerConfig, match="fp8"):
            sd.compile(d_unc, d_ctx, new_lat(), sampler=sch, control=True)
    finally:
        config.set_dtype("fp16")
    still_runs()
    # start(): a missing hint, wrong hint shapes and types, a wrong scale length -- all before anything is written
    emb_before, scales_before = sd._hint_emb.numpy().copy(), sd._control_scales.numpy().copy()
    for kw, match in (({}, "control_image= or control_hint="),
                      ({"control_image": img, "control_hint": _hint_of(img)}, "not both"),
                      ({"control_image": img[:, :64]}, "control_image must be"),
                      ({"control_image": img.astype(np.float32)}, "uint8"),
                      ({"control_image": np.concatenate([img, img[:1]])}, "control_image must be"),
                      ({"control_hint": _hint_of(img).transpose(0, 2, 3, 1)}, "control_hint must be"),
                      ({"control_hint": 2.0 * _hint_of(img)}, r"\[0, 1\]"),
                      ({"control_image": img, "control_scale": np.ones(13, np.float32)}, "control_scale"),      # the tiny model has 10 residuals
                      ({"control_image": img, "control_scale": np.ones((2, 5), np.float32)}, "control_scale"),
                      ({"control_image": img, "control_scale": float("nan")}, "control_scale"),
                      ({"control_image": img, "noise": np.zeros((2, 4, 16, 16), np.float32), "init_latent": np.zeros((2, 4, 16, 16), np.float32)}, "seed")):
        with pytest.raises(ValueError, match=match):
            sd.start(seed=SEED, **kw)
    assert np.array_equal(sd._hint_emb.numpy(), emb_before) and np.array_equal(sd._control_scales.numpy(), scales_before)
    still_runs()
    # a model compiled without control refuses the three arguments and runs its plain step
    plain = StableDiffusion(TINY); update_state(plain.model.diffusion_model, W, "")
    plat = new_lat()
    plain.compile(d_unc, d_ctx, plat, sampler=sch)
    for kw in ({"control_image": img}, {"control_hint": _hint_of(img)}, {"control_scale": 1.0}):
        with pytest.raises(ValueError, match="control=True"):
            plain.start(seed=SEED, **kw)
    plain.start(seed=SEED)
    plain.run(G); plain.synchronize()
    assert np.isfinite(plat.numpy()).all() and not np.array_equal(plat.numpy(), want)


# ---- 8. SD-1.5 shapes ---------------------------------------------------------------------------------------------------------------------
def test_sd15_controlled_two_steps_from_a_512_hint(tf):
    import oracle
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.variants.samplers import DPMSolverPP2M
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.controlnet import ControlNet
    from tinyfusers_amd.vision.unet import SD15
    sd, net = StableDiffusion(SD15), ControlNet(SD15)
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(sd.model.diffusion_model, synth_state_dict(oracle.unet_param_shapes(oracle.SD15), 0), "")
        update_state(net, synth_state_dict(C.controlnet_param_shapes(oracle.SD15), 1, prefix="control_model."), "control_model.")
    sd.attach_control(net)
    img = np.random.default_rng(9).integers(0, 256, (1, 512, 512, 3), dtype=np.uint8)
    ctx = tf.DeviceArray.from_numpy(synth_normal(1234, "sd.context", (1, 77, 768)))
    unc = tf.DeviceArray.from_numpy(synth_normal(1234, "sd.uncond", (1, 77, 768)))
    sch = DPMSolverPP2M().schedule(2)
    lat = sd.latent_from_numpy(np.zeros((1, 4, 64, 64), np.float32))
    sd.compile(unc, ctx, lat, sampler=sch, control=True)
    assert sd._hint_emb.shape == (2, 320, 64, 64)
    outs = [_final(sd, lat, eager=eager, control_image=img)[1] for eager in (False, True)]
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1])
    with tf.use_stream(sd._stream):
        x2 = sd._cfg_duplicate(lat)
        res = net(x2, sd._hint_emb, sd._params, sd._ctx2)
        shapes = [r.shape for r in res]
    sd.synchronize()
    c, s = [320] * 4 + [640] * 3 + [1280] * 5 + [1280], [64] * 3 + [32] * 3 + [16] * 3 + [8] * 3 + [8]
    assert shapes == [(2, ci, si, si) for ci, si in zip(c, s)]
    assert all(np.isfinite(r.numpy()).all() for r in res)
    _, off = _final(sd, lat, control_image=img, control_scale=0)
    assert np.isfinite(off).all() and float(np.abs(off - outs[0]).max()) > 0
