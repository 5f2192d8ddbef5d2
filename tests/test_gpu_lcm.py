"""GPU checks of few-step sampling: the guidance-free single-branch step (csrc/sampler.hip, StableDiffusion.compile(..., cfg=False)) and the
LCM table of variants/samplers.py -- tf_latent_stack1_* against group 0 of the CFG launches it replaces, one fused single-branch update against
float64 numpy, tiny-UNet trajectories (graph == eager, reproducible from a seed, against the CPU oracle on B images with the context alone), the
modes it composes with (inpaint, the inpainting checkpoint, ControlNet, LoRA), and the SD-1.5 size once."""
import contextlib
import io
import os
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "aux"))
import controlnet_oracle as C  # noqa: E402
import test_gpu_concat as TC  # noqa: E402
import test_gpu_controlnet as TN  # noqa: E402
import test_gpu_lora as TL  # noqa: E402
import test_gpu_samplers as TS  # noqa: E402
from test_samplers_host import randn_ref  # noqa: E402

SEED = TS.SEED                      # a seed with both key words nonzero
_gate = TS._gate                    # the project's trajectory gate: rel-L2 5e-3 and max |d| <= 1e-2 max |ref| in fp16, both 3e-2 in the bf16 step
BF16 = dict(rel_l2=3e-2, max_rel=3e-2)


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def _raw16(tf, n, fill):
    return tf.DeviceArray.from_numpy(np.full((n,), fill, np.uint16), np.uint16, "row")


def _read16(a):
    return a.numpy().astype(np.uint16)


# ---- 1. tf_latent_stack1_* ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(2, 4, 8, 12, 0), (3, 4, 5, 7, 5), (1, 4, 16, 16, 4)])
def test_latent_stack1_is_group_0_of_the_cfg_launches(tf, shape, dtype):
    """(B,C,H,W,Cc); 5x7 with 9 channels makes 18-byte pixels and odd row starts.  The output sits between two guard regions at an offset of 3
    words, so the first pixel is 2-byte aligned and no more."""
    from tinyfusers_amd.native import hip
    B, C, H, W, Cc = shape
    Ct, HW = C + Cc, H * W
    rng = np.random.default_rng(B * 1000 + Cc * 100 + H)
    lat = (3 * rng.standard_normal((B, C, H, W))).astype(np.float32)
    lat[0, 1, 1, :4] = [0.333251953125 + 2.0 ** -13, -0.0, 70000.0, 3e-6]     # an fp16 tie, -0, past the fp16 range, an fp16 subnormal
    d_lat = tf.DeviceArray.from_numpy(lat, np.float32, "row")
    bf = dtype == "bf16"
    stack1 = hip.tf_latent_stack1_bf16 if bf else hip.tf_latent_stack1_f16
    n = B * HW * Ct
    if Cc:
        cond = rng.standard_normal((B, Cc, H, W)).astype(np.float32)
        cond[0, 0, 0, :3] = [-0.0, 3e-6, -70000.0]
        d_cond = tf.DeviceArray.from_numpy(cond, np.float32, "row")
        d_ref = _raw16(tf, 2 * n, 0)
        (hip.tf_cfg_concat_bf16 if bf else hip.tf_cfg_concat_f16)(d_ref.ptr, d_lat.ptr, d_cond.ptr, B, C, Cc, H, W, 2, 0, None)
    else:
        d_cond = None
        d_ref = _raw16(tf, 2 * n, 0)
        (hip.tf_cfg_duplicate_bf16 if bf else hip.tf_cfg_duplicate_f16)(d_ref.ptr, d_lat.ptr, B, C, H, W, None)
    want = _read16(d_ref)[:n]                                        # group 0
    front, back, fill = 3, 64, 0x7E55
    buf = _raw16(tf, front + n + back, fill)
    stack1(buf.ptr + 2 * front, d_lat.ptr, d_cond.ptr if Cc else None, B, C, Cc, H, W, None)
    got = _read16(buf)
    assert np.all(got[:front] == fill) and np.all(got[front + n:] == fill)       # the guard regions are untouched
    assert np.array_equal(got[front:front + n], want)
    assert len(np.unique(want)) > 16                                 # (not a comparison of two blank buffers)
    other = tf.DeviceArray.from_numpy(np.zeros((B, max(Cc, 1), H, W), np.float32), np.float32, "row")
    with pytest.raises(RuntimeError, match="cond == NULL iff Cc == 0"):
        stack1(buf.ptr, d_lat.ptr, None, B, C, Cc + 1 if not Cc else Cc, H, W, None)        # Cc > 0 without cond
    with pytest.raises(RuntimeError, match="cond == NULL iff Cc == 0"):
        stack1(buf.ptr, d_lat.ptr, other.ptr, B, C, 0, H, W, None)                          # cond with Cc == 0
    with pytest.raises(RuntimeError, match="bad arguments"):
        stack1(None, d_lat.ptr, None, B, C, 0, H, W, None)
    assert np.array_equal(_read16(buf), got)                         # the refused calls wrote nothing


# ---- 2. one fused single-branch step --------------------------------------------------------------------------------------------------------
def _step1_ref(x, eps, hist, a_t, row, z, a_s=None, x0i=None, m=None, z2=None):
    """float64 restatement: x0 = (x - sqrt(1-a_t) e)/sqrt(a_t), x' = c_x x + c_0 x0 + c_1 x0_prev + c_n z; masked: x' <- m x' + (1-m)(sqrt(a_s)
    x0_init + sqrt(1-a_s) z2).  The scalars as the kernel holds them: fp32."""
    a_t = np.float64(np.float32(a_t))
    x0 = (x - np.sqrt(1 - a_t) * eps) / np.sqrt(a_t)
    c_x, c_0, c_1, c_n = (np.float64(np.float32(c)) for c in row)
    xn = c_x * x + c_0 * x0 + (c_1 * hist if c_1 != 0 else 0.0) + c_n * z
    if m is not None:
        a_s = np.float64(np.float32(a_s))
        xn = m * xn + (1 - m) * (np.sqrt(a_s) * x0i + np.sqrt(1 - a_s) * z2)
    return xn, x0


def _close(got, ref):
    """The project's gate for these fp32 expressions (test_one_fused_sampler_step_matches_float64)."""
    worst = float(np.max(np.abs(got - ref) / (1 + np.abs(ref))))
    assert np.all(np.abs(got - ref) <= 1e-5 * (1 + np.abs(ref))), worst


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name", ["lcm", "dpmpp2m"])
def test_one_single_branch_step_matches_float64(tf, name, masked, dtype):
    from tinyfusers_amd.native import hip
    from tinyfusers_amd.storage.tensor import bfloat16
    from tinyfusers_amd.variants import samplers as S
    bf = dtype == "bf16"
    sch = S.make(name).schedule(25)
    i, offset, g = 9, 5, 7.5
    last = len(sch.timesteps) - 1
    table = sch.coeffs.copy()
    table[i, 2] = table[i, 2] or 0.25                            # every term live: c_1 != 0 and c_n != 0
    table[i, 3] = table[i, 3] or 0.6
    assert table[0, 2] == 0.0 and sch.alphas_prev[last] == 1.0
    entry = hip.tf_sampler_step1_bf16 if bf else hip.tf_sampler_step1_f32
    two = (hip.tf_cfg_sampler_step_masked_bf16 if bf else hip.tf_cfg_sampler_step_masked_f32) if masked else \
          (hip.tf_cfg_sampler_step_bf16 if bf else hip.tf_cfg_sampler_step_f32)
    d_tab = tf.DeviceArray.from_numpy(table.astype(np.float32), np.float32, "row")
    sp = tf.DeviceArray.zeros((8,), np.float32, "row")
    for B, C, H, W in ((2, 4, 8, 12), (2, 3, 5, 7)):             # (105 elements per image: a partial last counter)
        n_img = C * H * W
        rng = np.random.default_rng(4 + C)
        x = rng.standard_normal((B, C, H, W)).astype(np.float32).astype(np.float64)
        hist = rng.standard_normal((B, C, H, W)).astype(np.float32).astype(np.float64)
        x0i = rng.standard_normal((B, C, H, W)).astype(np.float32).astype(np.float64)
        m = rng.random((B, 1, H, W)).astype(np.float32).astype(np.float64)       # fractional, with exact 0 and 1
        m[:, :, 0, :3], m[:, :, 1, :3] = 0.0, 1.0
        d_eps = tf.DeviceArray.from_numpy(rng.standard_normal((B, C, H, W)), bfloat16 if bf else np.float16, "nhwc")
        eps = d_eps.numpy().astype(np.float64)                   # the values the kernel reads
        d_x0i = tf.DeviceArray.from_numpy(x0i.astype(np.float32), np.float32, "row")
        d_m = tf.DeviceArray.from_numpy(m.astype(np.float32), np.float32, "row")
        extra = (d_x0i.ptr, d_m.ptr) if masked else (None, None)

        def run(row, x_in, hist_in, b=B, first=0):
            lat = tf.DeviceArray.from_numpy(x_in[first:first + b].astype(np.float32), np.float32, "row")
            h = tf.DeviceArray.from_numpy(hist_in[first:first + b].astype(np.float32), np.float32, "row")
            TS._set_params(hip, sp, sch.timesteps[row], sch.alphas[row], sch.alphas_prev[row], g, row, SEED, offset + first)
            entry(lat.ptr, d_eps.ptr, h.ptr, sp.ptr, d_tab.ptr, len(table), *extra, b, C, H, W, None)
            return lat.numpy().astype(np.float64), h.numpy().astype(np.float64)

        def noise(row, tag):
            return np.stack([randn_ref(SEED, offset + b, n_img, row, tag).reshape(C, H, W) for b in range(B)])

        def ref(row, hist_in):
            kw = dict(a_s=sch.alphas_prev[row], x0i=x0i, m=m, z2=noise(row, 2)) if masked else {}
            return _step1_ref(x, eps, hist_in, sch.alphas[row], table[row], noise(row, 1), **kw)

        got, got_h = run(i, x, hist)
        want, want_x0 = ref(i, hist)
        _close(got, want)
        _close(got_h, want_x0)
        # image 0 of the B = 2 launch == a B = 1 launch (the noise follows the global image index, not the batch)
        one, one_h = run(i, x, hist, b=1)
        assert np.array_equal(one[0], got[0]) and np.array_equal(one_h[0], got_h[0])
        # first step (c_1 == 0): the history is not read -- a NaN-filled one gives the zeroed one's finite result
        a, _ = run(0, x, np.full(x.shape, np.nan))
        b0, _ = run(0, x, np.zeros(x.shape))
        assert np.isfinite(a).all() and np.array_equal(a, b0)
        _close(a, ref(0, 0.0)[0])
        # against the two-branch kernel fed [e ; e] at g = 7.5 (another kernel: the gate, not the bits)
        lat2 = tf.DeviceArray.from_numpy(x.astype(np.float32), np.float32, "row")
        h2 = tf.DeviceArray.from_numpy(hist.astype(np.float32), np.float32, "row")
        d_eps2 = tf.DeviceArray.from_numpy(np.concatenate([eps, eps]), bfloat16 if bf else np.float16, "nhwc")
        TS._set_params(hip, sp, sch.timesteps[i], sch.alphas[i], sch.alphas_prev[i], g, i, SEED, offset)
        two(lat2.ptr, d_eps2.ptr, h2.ptr, sp.ptr, d_tab.ptr, len(table), *(extra if masked else ()), B, C, H, W, None)
        _close(got, lat2.numpy().astype(np.float64))
        _close(got_h, h2.numpy().astype(np.float64))
        if masked:
            # the last step (a_prev = 1): where the mask is 0 the output is x0_init, bit for bit
            end, _ = run(last, x, hist)
            keep = np.broadcast_to(m == 0, x.shape)
            assert keep.any() and np.array_equal(end[keep].astype(np.float32), x0i[keep].astype(np.float32))
            _close(end, ref(last, hist)[0])
        # exactly one of x0_init / mask: refused, nothing written
        lat = tf.DeviceArray.from_numpy(x.astype(np.float32), np.float32, "row")
        h = tf.DeviceArray.from_numpy(hist.astype(np.float32), np.float32, "row")
        for pair in ((d_x0i.ptr, None), (None, d_m.ptr)):
            with pytest.raises(RuntimeError, match="bad arguments"):
                entry(lat.ptr, d_eps.ptr, h.ptr, sp.ptr, d_tab.ptr, len(table), *pair, B, C, H, W, None)
        with pytest.raises(RuntimeError, match="bad arguments"):
            entry(lat.ptr, None, h.ptr, sp.ptr, d_tab.ptr, len(table), *extra, B, C, H, W, None)
        assert np.array_equal(lat.numpy(), x.astype(np.float32))


# ---- 3. tiny UNet trajectories --------------------------------------------------------------------------------------------------------------
def _trajectory1(eps_fn, lat0, sch, seed, x0_init=None, mask=None):
    """The float64 sampler around ONE guidance group: e = eps_fn(x as fp32, t) on B images against the context alone; then the update of
    tests/test_gpu_samplers.py::_oracle_trajectory, and with a mask the latent blend of tests/test_gpu_img2img.py."""
    x, xp = lat0.astype(np.float64), np.zeros(lat0.shape)
    B, n_img = lat0.shape[0], lat0[0].size
    for i, t in enumerate(sch.timesteps):
        e = eps_fn(x.astype(np.float32), np.array([t], np.float32)).numpy().astype(np.float64)
        a_t = sch.alphas[i]
        x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
        z = np.stack([randn_ref(seed, b, n_img, i, 1).reshape(lat0.shape[1:]) for b in range(B)])
        c_x, c_0, c_1, c_n = sch.coeffs[i]
        x, xp = c_x * x + c_0 * x0 + c_1 * xp + c_n * z, x0
        if mask is not None:
            x = mask * x + (1 - mask) * TN._known_ref(x0_init, sch.alphas_prev[i], seed, i)
    return x


def _tiny_eps(W, ctx, cfg=None, cond=None):
    import oracle
    Wf = {k: torch.from_numpy(v.astype(np.float32)) for k, v in W.items()}
    cfg = oracle.TINY if cfg is None else cfg
    return lambda x32, t: oracle.unet_forward(x32 if cond is None else np.concatenate([x32, cond], axis=1), t, ctx, Wf, cfg)


def _tiny_model(W):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY
    sd = StableDiffusion(TINY); update_state(sd.model.diffusion_model, W, "")
    lat = sd.latent_from_numpy(np.zeros((2, 4, 16, 16), np.float32))
    return sd, lat


def _three_runs(sd, lat, guidance=None, **kw):
    """graph, eager, graph again from the same seed: the initial latent and the three final latents."""
    outs = []
    for eager in (False, True, False):
        sd.start(seed=SEED, **kw)
        if not outs:
            lat0 = lat.numpy().copy()
        sd.run(guidance, eager=eager); sd.synchronize()
        outs.append(lat.numpy().copy())
    return lat0, outs


@pytest.mark.parametrize("hoist", [True, False])
def test_tiny_lcm4_single_branch_graph_eager_seed_and_oracle(tf, hoist):
    from tinyfusers_amd import config
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    W, ctx, unc = TS._tiny()
    sch = S.LCM().schedule(4)
    old = config.hoist_step_invariants
    config.hoist_step_invariants = hoist
    try:
        sd, lat = _tiny_model(W)
        sd.compile(None, tf.DeviceArray.from_numpy(ctx), lat, sampler=sch, cfg=False)
        assert sd._groups == 1 and sd._ctx2.shape[0] == 2 and (sd._kv_all is not None) == hoist
        lat0, outs = _three_runs(sd, lat)
        # a guidance scale has nowhere to go: refused before anything runs, the latent as it was
        for call in (lambda: sd.run(7.5), lambda: sd.step_sampler(0, 7.5)):
            sd.start(seed=SEED)
            with pytest.raises(ValueError, match="no guidance branch"):
                call()
            sd.synchronize()
            np.testing.assert_array_equal(lat.numpy(), lat0)
        sd.run(1.0); sd.synchronize()                                # 1.0 is the same as None
        np.testing.assert_array_equal(lat.numpy(), outs[0])
        # set_context without an unconditional context: the swapped prompts, then back
        sd.set_context(None, tf.DeviceArray.from_numpy(unc))
        sd.start(seed=SEED); sd.run(); sd.synchronize()
        swapped = lat.numpy().copy()
        sd.set_context(None, tf.DeviceArray.from_numpy(ctx))
        sd.start(seed=SEED); sd.run(); sd.synchronize()
        np.testing.assert_array_equal(lat.numpy(), outs[0])
    finally:
        config.hoist_step_invariants = old
    np.testing.assert_array_equal(lat0, StableDiffusion.randn_latent((2, 4, 16, 16), SEED).numpy())
    np.testing.assert_array_equal(outs[0], outs[1])              # graph replay == eager
    np.testing.assert_array_equal(outs[0], outs[2])              # same seed, same image
    print("LCM-4, cfg=False, fp16:", end=" ")
    _gate(outs[0], _trajectory1(_tiny_eps(W, ctx), lat0, sch, SEED))
    print("LCM-4, cfg=False, the other context:", end=" ")
    _gate(swapped, _trajectory1(_tiny_eps(W, unc), lat0, sch, SEED))
    assert float(np.abs(swapped - outs[0]).max()) > 0.05


def test_tiny_lcm4_single_branch_in_the_bf16_step(tf):
    from tinyfusers_amd import config
    from tinyfusers_amd.variants import samplers as S
    W, ctx, _ = TS._tiny()
    sch = S.LCM().schedule(4)
    config.set_dtype("bf16")
    try:
        sd, lat = _tiny_model(W)
        sd.compile(None, tf.DeviceArray.from_numpy(ctx), lat, sampler=sch, cfg=False)
        lat0, outs = _three_runs(sd, lat)
    finally:
        config.set_dtype("fp16")
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])
    print("LCM-4, cfg=False, bf16:", end=" ")
    _gate(outs[0], _trajectory1(_tiny_eps(W, ctx), lat0, sch, SEED), **BF16)


def test_tiny_lcm4_table_on_the_two_branch_kernels_at_guidance_1p5(tf):
    """cfg=True with an LCM schedule: nothing new but the table (LCM-LoRA at guidance 1-2 is a real use)."""
    from tinyfusers_amd.variants import samplers as S
    W, ctx, unc = TS._tiny()
    sch = S.LCM().schedule(4)
    sd, lat = _tiny_model(W)
    sd.compile(tf.DeviceArray.from_numpy(unc), tf.DeviceArray.from_numpy(ctx), lat, sampler=sch)
    assert sd._groups == 2
    lat0, outs = _three_runs(sd, lat, 1.5)
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])
    print("LCM-4, cfg=True, g = 1.5, fp16:", end=" ")
    _gate(outs[0], TS._oracle_trajectory(W, unc, ctx, lat0, sch, 1.5, SEED))
    with pytest.raises(TypeError, match="guidance"):
        sd.run()                                                 # a CFG model still needs its scale


def test_tiny_dpmpp2m_single_branch_reads_the_history(tf):
    from tinyfusers_amd.variants import samplers as S
    W, ctx, _ = TS._tiny()
    sch = S.DPMSolverPP2M().schedule(6)
    assert np.all(sch.coeffs[1:-1, 2] != 0)
    sd, lat = _tiny_model(W)
    sd.compile(None, tf.DeviceArray.from_numpy(ctx), lat, sampler=sch, cfg=False)
    lat0, outs = _three_runs(sd, lat)
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])
    print("DPM++2M-6, cfg=False, fp16:", end=" ")
    _gate(outs[0], _trajectory1(_tiny_eps(W, ctx), lat0, sch, SEED))


# ---- 4. the modes cfg=False composes with ---------------------------------------------------------------------------------------------------
def test_single_branch_inpaint_keeps_the_known_region_bit_for_bit(tf):
    from tinyfusers_amd.storage.synth import synth_normal
    from tinyfusers_amd.variants import samplers as S
    W, ctx, _ = TS._tiny()
    sch = S.LCM().schedule(8, strength=0.5)
    sd, lat = _tiny_model(W)
    sd.compile(None, tf.DeviceArray.from_numpy(ctx), lat, sampler=sch, inpaint=True, cfg=False)
    x0 = synth_normal(5, "x0", (2, 4, 16, 16)).astype(np.float32)
    m = np.zeros((2, 1, 16, 16), np.float32); m[..., :8] = 1.0
    lat0, outs = _three_runs(sd, lat, init_latent=x0, mask=m)
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])
    keep = np.broadcast_to(m == 0, x0.shape)
    np.testing.assert_array_equal(outs[0][keep], x0[keep])       # after the last step (a_prev = 1) the known region is x0_init
    print("LCM-8 at strength 0.5, inpaint=True, cfg=False:", end=" ")
    _gate(outs[0], _trajectory1(_tiny_eps(W, ctx), lat0, sch, SEED, x0.astype(np.float64), m.astype(np.float64)))
    sd.start(seed=SEED, init_latent=x0)                          # no mask: all ones, everything repainted
    sd.run(); sd.synchronize()
    free = lat.numpy()
    d = float(np.abs(free[~keep] - outs[0][~keep]).max())
    print(f"the mask moves the repainted region by max |d| = {d:.3f}")
    assert d > 0.01 and float(np.abs(free[keep] - x0[keep]).max()) > 0.01


def test_single_branch_on_the_tiny_inpainting_checkpoint(tf):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY
    cfg, W, ctx, _, cond = TC._tiny(9)
    sch = S.LCM().schedule(4)
    sd = StableDiffusion(replace(TINY, in_channels=9)); update_state(sd.model.diffusion_model, W, "")
    lat = sd.latent_from_numpy(np.zeros((2, 4, 16, 16), np.float32))
    sd.compile(None, tf.DeviceArray.from_numpy(ctx), lat, sampler=sch, concat="inpaint", cfg=False)
    assert sd._groups == 1
    lat0, outs = _three_runs(sd, lat, cond_latent=cond)
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])
    print("LCM-4, concat='inpaint', cfg=False:", end=" ")
    _gate(outs[0], _trajectory1(_tiny_eps(W, ctx, cfg, cond), lat0, sch, SEED))
    with pytest.raises(ValueError, match="cond_latent"):
        sd.start(seed=SEED)                                      # the conditioning is still required


def test_single_branch_controlled_step_meets_the_oracle_on_one_group(tf):
    import oracle
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.vision.controlnet import ControlNet
    W, Wc, ctx, _, img = TN._tiny()[:5]
    sch = S.LCM().schedule(4)
    sd, lat = _tiny_model(W)
    net = ControlNet(sd.model.diffusion_model.cfg); update_state(net, Wc, "")
    sd.attach_control(net).compile(None, tf.DeviceArray.from_numpy(ctx), lat, sampler=sch, control=True, cfg=False)
    assert sd._hint_emb.shape == (2, 64, 16, 16)                 # one group
    lat0, outs = _three_runs(sd, lat, control_image=img)
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])
    Wf, Wcf = TN._f32(W), TN._f32(Wc)
    emb = C.hint_embedding(TN._hint_of(img), Wcf)

    def eps(x32, t):
        return C.unet_forward(x32, t, ctx, Wf, oracle.TINY, control=C.controlnet_forward(x32, None, t, ctx, Wcf, oracle.TINY, hint_emb=emb))
    print("LCM-4, control=True, cfg=False:", end=" ")
    _gate(outs[0], _trajectory1(eps, lat0, sch, SEED))
    sd.start(seed=SEED, control_image=img, control_scale=0); sd.run(); sd.synchronize()
    assert float(np.abs(lat.numpy() - outs[0]).max()) > 0.01     # the residuals are read


def test_single_branch_survives_an_adapter_swap(tf):
    from tinyfusers_amd.variants import samplers as S
    W, _, ctx, _ = TN._tiny()[:4]
    _, A, _ = TL._adapters()
    sch = S.LCM().schedule(4)
    sd, lat = _tiny_model(W)
    sd.compile(None, tf.DeviceArray.from_numpy(ctx), lat, sampler=sch, cfg=False)
    assert sd.load_lora(A, "A") == "A"

    def final():
        sd.start(seed=SEED); sd.run(); sd.synchronize()
        return lat.numpy().copy()
    base = final()
    old = sd._graph
    sd.set_adapters(["A"])
    assert sd._graph is not old and sd._groups == 1 and sd._compile_args["cfg"] is False
    with pytest.raises(S.UnsupportedSamplerConfig, match="start"):
        sd.run()
    with_a = final()
    d = float(np.linalg.norm(with_a - base) / np.linalg.norm(base))
    print(f"adapter A moves the LCM-4 cfg=False latent by rel-L2 {d:.3f}")
    assert np.isfinite(with_a).all() and d > 1e-2
    sd.set_adapters([])
    np.testing.assert_array_equal(final(), base)                 # the base model, bit for bit
    assert sd._groups == 1                                       # ... still in the guidance-free mode
    with pytest.raises(ValueError, match="no guidance branch"):
        sd.run(7.5)


# ---- 5. SD-1.5 size, once -------------------------------------------------------------------------------------------------------------------
def test_sd15_lcm4_single_branch_is_finite_repeatable_and_graph_equals_eager(tf):
    import oracle
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.variants.samplers import LCM
    from tinyfusers_amd.variants.sd import StableDiffusion
    sd = StableDiffusion()
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(sd.model.diffusion_model, synth_state_dict(oracle.unet_param_shapes(oracle.SD15), 0), "")
    lat = sd.latent_from_numpy(np.zeros((1, 4, 64, 64), np.float32))
    ctx = tf.DeviceArray.from_numpy(synth_normal(1234, "sd.context", (1, 77, 768)))
    sch = LCM().schedule(4)
    sd.compile(None, ctx, lat, sampler=sch, cfg=False)
    assert sd._groups == 1
    sd.start(seed=SEED)
    for i in range(4):
        sd.step_sampler(i); sd.synchronize()
        assert np.isfinite(lat.numpy()).all(), i
    graph = lat.numpy().copy()
    sd.start(seed=SEED); sd.run(eager=True); sd.synchronize()
    np.testing.assert_array_equal(lat.numpy(), graph)            # graph replay == eager
    sd.start(seed=SEED); sd.run(); sd.synchronize()
    np.testing.assert_array_equal(lat.numpy(), graph)            # a second start with the same seed reproduces the image
    sd.start(seed=SEED + 1); sd.run(); sd.synchronize()
    assert not np.array_equal(lat.numpy(), graph)
