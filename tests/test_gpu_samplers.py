"""GPU checks of the samplers beyond sigma = 0 DDIM (csrc/sampler.hip, variants/samplers.py, StableDiffusion.compile(..., sampler=...)):
the device Philox normal generator against its numpy restatement, one fused sampler update against float64 numpy, fresh ancestral noise
every step, tiny-UNet trajectories (graph == eager, reproducible from a seed, against the CPU oracle) and the SD-1.5 DDIM schedule through
the new API against the reference's own 50-step trajectory."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_samplers_host import randn_ref  # noqa: E402

SEED = 0x243F6A8885A308D3          # a seed with both key words nonzero


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


def _gate(got, ref, rel_l2=5e-3, max_rel=1e-2):
    """The UNet gate's rel-L2, with the max bound of test_full_50_step_sampler_schedule_config3: max |d| <= 1e-2 max |ref| (bf16: both 3e-2).  Along a
    trajectory with CFG 7.5 the synthetic-weight latent grows to |x| ~ 25 and the fp16 rounding of the UNet input alone is ~1e-2 per element,
    so a bound relative to (1 + |ref|) of every element would be a bound on the largest absolute errors, not on the relative precision."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all()
    rl2 = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    mx = float(np.abs(got - ref).max() / np.abs(ref).max())
    worst = float(np.max(np.abs(got - ref) / (1.0 + np.abs(ref))))
    print(f"gate: rel-L2 {rl2:.3e} (gate {rel_l2}), max|d|/max|ref| {mx:.3e} (gate {max_rel}), max |d|/(1+|ref|) {worst:.3e}, max|ref| {np.abs(ref).max():.1f}")
    assert rl2 <= rel_l2 and mx <= max_rel, (rl2, mx)


def _words(seed):
    return seed & 0xFFFFFFFF, seed >> 32


# ---- 1. tf_randn_f32 --------------------------------------------------------------------------------------------------------------
def test_device_randn_matches_numpy_and_is_batch_independent(tf):
    from tinyfusers_amd.native import hip
    from tinyfusers_amd.variants.sd import StableDiffusion
    lo, hi = _words(SEED)
    for shape in ((3, 4, 16, 16), (2, 3, 5, 7)):              # (105 elements per image: a partial last counter)
        n_img = int(np.prod(shape[1:]))
        out = tf.DeviceArray.empty(shape, np.float32, "row")
        hip.tf_randn_f32(out.ptr, shape[0], n_img, lo, hi, 4, 6, 1, None)
        got = out.numpy().reshape(shape[0], -1)
        for k in range(shape[0]):
            ref = randn_ref(SEED, 4 + k, n_img, 6, 1)
            assert np.all(np.abs(got[k] - ref) <= 2e-6 * (1 + np.abs(ref))), np.max(np.abs(got[k] - ref))
    three = StableDiffusion.randn_latent((3, 4, 16, 16), SEED).numpy()
    for k in range(3):
        one = StableDiffusion.randn_latent((1, 4, 16, 16), SEED, image_offset=k).numpy()
        assert np.array_equal(one[0], three[k])
    np.testing.assert_allclose(three[0].reshape(-1), randn_ref(SEED, 0, 1024, 0, 0), rtol=0, atol=2e-5)
    assert not np.array_equal(three[0], StableDiffusion.randn_latent((1, 4, 16, 16), SEED + 1).numpy()[0])
    tag1 = tf.DeviceArray.empty((1, 4, 16, 16), np.float32, "row")
    hip.tf_randn_f32(tag1.ptr, 1, 1024, lo, hi, 0, 0, 1, None)
    assert not np.array_equal(three[0], tag1.numpy()[0])
    big = StableDiffusion.randn_latent((4, 4, 512, 512), 11).numpy().astype(np.float64)          # 2^22 samples
    m, v = float(big.mean()), float(big.var())
    print(f"2^22 device normals: mean {m:.2e}, variance {v:.5f}")
    assert abs(m) < 3e-3 and abs(v - 1.0) < 1e-2, (m, v)


# ---- 2. one fused sampler update ----------------------------------------------------------------------------------------------------
def _set_params(hip, sp, t, a_t, a_p, g, row, seed, offset):
    lo, hi = _words(seed)
    hip.tf_set_sampler_params(sp.ptr, float(t), float(a_t), float(a_p), float(g), row, lo, hi, offset, None, None, 0, None)


def _step_ref(x, eps2, hist, a_t, g, row, z):
    """float64 restatement: e = e_u + g (e_c - e_u), x0 = (x - sqrt(1-a_t) e)/sqrt(a_t), x' = c_x x + c_0 x0 + c_1 x0_prev + c_n z."""
    b = x.shape[0]
    e = eps2[:b] + g * (eps2[b:] - eps2[:b])
    a_t = np.float64(np.float32(a_t))
    x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
    c_x, c_0, c_1, c_n = (np.float64(np.float32(c)) for c in row)
    return c_x * x + c_0 * x0 + (c_1 * hist if c_1 != 0 else 0.0) + c_n * z, x0


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["ddim-eta", "euler-a", "dpmpp2m"])
def test_one_fused_sampler_step_matches_float64(tf, name, dtype):
    from tinyfusers_amd.native import hip
    from tinyfusers_amd.storage.tensor import bfloat16
    from tinyfusers_amd.variants import samplers as S
    for B, C, H, W in ((2, 4, 8, 12), (2, 3, 5, 7)):             # (105 elements per image: a partial last counter)
        n_img, g, offset = C * H * W, 7.5, 5
        sch = S.make(name).schedule(25)
        i = 9
        table = sch.coeffs.copy()
        table[i, 2] = table[i, 2] or 0.25                            # every term live: c_1 != 0 and c_n != 0
        table[i, 3] = table[i, 3] or 0.6
        rng = np.random.default_rng(4)
        x = rng.standard_normal((B, C, H, W))
        eps2 = rng.standard_normal((2 * B, C, H, W))
        hist = rng.standard_normal((B, C, H, W))
        dt = bfloat16 if dtype == "bf16" else np.float16
        d_eps = tf.DeviceArray.from_numpy(eps2, dt, "nhwc")
        eps2 = d_eps.numpy().astype(np.float64)                      # the values the kernel reads
        d_tab = tf.DeviceArray.from_numpy(table.astype(np.float32), np.float32, "row")
        sp = tf.DeviceArray.zeros((8,), np.float32, "row")
        entry = hip.tf_cfg_sampler_step_bf16 if dtype == "bf16" else hip.tf_cfg_sampler_step_f32

        def run(row, x_in, hist_in):
            lat = tf.DeviceArray.from_numpy(x_in.astype(np.float32), np.float32, "row")
            h = tf.DeviceArray.from_numpy(hist_in.astype(np.float32), np.float32, "row")
            _set_params(hip, sp, sch.timesteps[row], sch.alphas[row], sch.alphas_prev[row], g, row, SEED, offset)
            entry(lat.ptr, d_eps.ptr, h.ptr, sp.ptr, d_tab.ptr, len(table), B, C, H, W, None)
            return lat.numpy().astype(np.float64), h.numpy().astype(np.float64)

        z = np.stack([randn_ref(SEED, offset + b, n_img, i, 1).reshape(C, H, W) for b in range(B)])
        got, got_h = run(i, x, hist)
        ref, ref_x0 = _step_ref(x, eps2, hist.astype(np.float32).astype(np.float64), sch.alphas[i], g, table[i], z)
        assert np.all(np.abs(got - ref) <= 1e-5 * (1 + np.abs(ref))), float(np.max(np.abs(got - ref) / (1 + np.abs(ref))))
        assert np.all(np.abs(got_h - ref_x0) <= 1e-5 * (1 + np.abs(ref_x0)))
        # first step (c_1 == 0): the history is not read -- a NaN-filled one gives the zeroed one's finite result
        assert table[0, 2] == 0.0
        a, _ = run(0, x, np.full(x.shape, np.nan))
        b, _ = run(0, x, np.zeros(x.shape))
        assert np.isfinite(a).all() and np.array_equal(a, b)
        z0 = np.stack([randn_ref(SEED, offset + k, n_img, 0, 1).reshape(C, H, W) for k in range(B)])
        ref0, _ = _step_ref(x, eps2, 0.0, sch.alphas[0], g, table[0], z0)
        assert np.all(np.abs(a - ref0) <= 1e-5 * (1 + np.abs(ref0)))


# ---- 2b. the update's grid-stride loop: every form of the one kernel -------------------------------------------------------------------
BIG = (3, 4, 512, 512)              # 786432 Philox counters: more than the 2048 x 256 threads of the largest grid, so some threads take a second trip


@pytest.fixture(scope="module")
def big_step(tf):
    """Inputs of test_sampler_step_grid_stride_loop_equals_the_single_trip_launches, made once and only read: the host arrays and the device
    copies of x0_init and the mask.  eps holds three guidance groups of B images as the kernel reads them, (group, image, H, W, C); a form of
    G groups reads the first G."""
    B, C, H, W = BIG
    rng = np.random.default_rng(12)
    x, hist, x0i = (rng.standard_normal(BIG, dtype=np.float32) for _ in range(3))
    m = rng.random((B, 1, H, W), dtype=np.float32)
    m[:, :, 0, :4], m[:, :, 1, :4] = 0.0, 1.0
    eps = rng.standard_normal((3, B, H, W, C), dtype=np.float32)
    return dict(x=x, hist=hist, eps=eps, d_x0i=tf.DeviceArray.from_numpy(x0i, np.float32, "row"), d_m=tf.DeviceArray.from_numpy(m, np.float32, "row"))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("form", ["cfg", "cfg-masked", "cfg3", "single", "single-masked"])
def test_sampler_step_grid_stride_loop_equals_the_single_trip_launches(tf, big_step, form, dtype):
    """Image k of one B = 3 launch (threads loop) == a B = 1 launch at image offset k (262144 counters: no thread loops), latent and history,
    bit for bit, on a row with c_1 != 0 and c_n != 0.  No host reference: batch independence against the host Philox is asserted at small sizes."""
    from tinyfusers_amd.native import hip
    from tinyfusers_amd.storage.tensor import bfloat16
    from tinyfusers_amd.variants import samplers as S
    B, C, H, W = BIG
    bf = dtype == "bf16"
    suffix = "bf16" if bf else "f32"
    groups = {"cfg": 2, "cfg-masked": 2, "cfg3": 3, "single": 1, "single-masked": 1}[form]
    masked = form.endswith("masked")
    entry = getattr(hip, {"cfg": "tf_cfg_sampler_step_", "cfg-masked": "tf_cfg_sampler_step_masked_", "cfg3": "tf_cfg3_sampler_step_",
                          "single": "tf_sampler_step1_", "single-masked": "tf_sampler_step1_"}[form] + suffix)
    sch = S.make("euler-a").schedule(25)
    i, offset = 9, 5
    table = sch.coeffs.astype(np.float32)
    table[i, 2] = 0.25                                           # the history is read
    assert table[i, 3] != 0.0                                    # the noise is live
    d_tab = tf.DeviceArray.from_numpy(table, np.float32, "row")
    sp = tf.DeviceArray.zeros((8,), np.float32, "row")
    edit = tf.DeviceArray.zeros((4,), np.float32, "row")
    hip.tf_set_step_params(edit.ptr, 1.5, 0.0, 0.0, 0.0, None)
    d_x0i, d_m = big_step["d_x0i"], big_step["d_m"]

    def run(first, nb):
        lat = tf.DeviceArray.from_numpy(big_step["x"][first:first + nb], np.float32, "row")
        h = tf.DeviceArray.from_numpy(big_step["hist"][first:first + nb], np.float32, "row")
        e = tf.DeviceArray.from_numpy(big_step["eps"][:groups, first:first + nb].reshape(groups * nb, H, W, C), bfloat16 if bf else np.float16, "row")
        _set_params(hip, sp, sch.timesteps[i], sch.alphas[i], sch.alphas_prev[i], 7.5, i, SEED, offset + first)
        extra = (d_x0i.ptr + 4 * first * C * H * W, d_m.ptr + 4 * first * H * W) if masked else (None, None) if groups == 1 else (edit.ptr,) if groups == 3 else ()
        entry(lat.ptr, e.ptr, h.ptr, sp.ptr, d_tab.ptr, len(table), *extra, nb, C, H, W, None)
        return lat.numpy(), h.numpy()

    got, got_h = run(0, B)
    assert np.isfinite(got).all() and not np.array_equal(got[0], got[1])
    for k in range(B):
        one, one_h = run(k, 1)
        assert np.array_equal(one[0], got[k]) and np.array_equal(one_h[0], got_h[k]), k


# ---- 3. ancestral noise is fresh every step ---------------------------------------------------------------------------------------
def test_ancestral_noise_is_fresh_every_step(tf):
    """20 Euler-a steps on N(0, s2) data with the exact Gaussian denoiser, eps from a host loop: x' = m_i x + c_n z, so the sample
    variance follows var' = m_i^2 var + c_n^2 exactly when z is independent of x -- noise repeated across steps would not."""
    from tinyfusers_amd.native import hip
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    s2, B, C, H, W = 0.5, 1, 4, 512, 512                           # 2^20 elements
    sch = S.EulerAncestral().schedule(20)
    d_tab = tf.DeviceArray.from_numpy(sch.coeffs.astype(np.float32), np.float32, "row")
    sp = tf.DeviceArray.zeros((8,), np.float32, "row")
    hist = tf.DeviceArray.zeros((B, C, H, W), np.float32, "row")
    lat = StableDiffusion.randn_latent((B, C, H, W), 99)
    var = float(lat.numpy().astype(np.float64).var())
    for i in range(len(sch.timesteps)):
        a_t = float(np.float32(sch.alphas[i]))
        x = lat.numpy().astype(np.float64)
        sig2 = (1 - a_t) / a_t
        x0 = x / np.sqrt(a_t) * s2 / (s2 + sig2)
        eps = (x - np.sqrt(a_t) * x0) / np.sqrt(1 - a_t)
        d_eps = tf.DeviceArray.from_numpy(np.concatenate([eps, eps]), np.float16, "nhwc")
        _set_params(hip, sp, sch.timesteps[i], sch.alphas[i], sch.alphas_prev[i], 3.0, i, 1234, 0)
        hip.tf_cfg_sampler_step_f32(lat.ptr, d_eps.ptr, hist.ptr, sp.ptr, d_tab.ptr, len(sch.timesteps), B, C, H, W, None)
        c_x, c_0, _, c_n = sch.coeffs[i]
        m = c_x + c_0 / np.sqrt(a_t) * s2 / (s2 + sig2)
        var = m * m * var + c_n * c_n
        got = float(lat.numpy().astype(np.float64).var())
        assert abs(got / var - 1) < 0.015, (i, got, var)
    print(f"after 20 Euler-a steps: sample variance {got:.5f}, recursion {var:.5f}")


# ---- 4. tiny UNet trajectories --------------------------------------------------------------------------------------------------
def _tiny(seed=5):
    import oracle
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    W = synth_state_dict(oracle.unet_param_shapes(oracle.TINY), seed)
    ctx = synth_normal(seed, "c", (2, 13, 64)).astype(np.float16).astype(np.float32)
    unc = synth_normal(seed, "u", (2, 13, 64)).astype(np.float16).astype(np.float32)
    return W, ctx, unc


def _oracle_trajectory(W, unc, ctx, lat0, sch, g, seed):
    import oracle
    Wf = {k: torch.from_numpy(v.astype(np.float32)) for k, v in W.items()}
    x, xp = lat0.astype(np.float64), np.zeros(lat0.shape)
    B, n_img = lat0.shape[0], lat0[0].size
    c2 = np.concatenate([unc, ctx])
    for i, t in enumerate(sch.timesteps):
        x32 = x.astype(np.float32)
        out = oracle.unet_forward(np.concatenate([x32, x32]), np.array([t], np.float32), c2, Wf, oracle.TINY).numpy().astype(np.float64)
        e = out[:B] + g * (out[B:] - out[:B])
        a_t = sch.alphas[i]
        x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
        z = np.stack([randn_ref(seed, b, n_img, i, 1).reshape(lat0.shape[1:]) for b in range(B)])
        c_x, c_0, c_1, c_n = sch.coeffs[i]
        x, xp = c_x * x + c_0 * x0 + c_1 * xp + c_n * z, x0
    return x


@pytest.mark.parametrize("hoist", [True, False])
@pytest.mark.parametrize("name", ["dpmpp2m", "euler-a"])
def test_tiny_unet_sampler_graph_eager_seed_and_oracle(tf, name, hoist):
    from tinyfusers_amd import config
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY
    W, ctx, unc = _tiny()
    sch = S.make(name).schedule(10)
    old = config.hoist_step_invariants
    config.hoist_step_invariants = hoist
    try:
        sd = StableDiffusion(TINY); update_state(sd.model.diffusion_model, W, "")
        lat = sd.latent_from_numpy(np.zeros((2, 4, 16, 16), np.float32))
        sd.compile(tf.DeviceArray.from_numpy(unc), tf.DeviceArray.from_numpy(ctx), lat, sampler=sch)
        with pytest.raises(RuntimeError, match="compiled with a sampler"):
            sd.step(981, 0.5, 0.6, 7.5)
        outs = []
        for eager in (False, True, False):
            sd.start(seed=SEED)
            if not outs:
                lat0 = lat.numpy().copy()
            sd.run(7.5, eager=eager); sd.synchronize()
            outs.append(lat.numpy().copy())
    finally:
        config.hoist_step_invariants = old
    np.testing.assert_array_equal(lat0, StableDiffusion.randn_latent((2, 4, 16, 16), SEED).numpy())
    np.testing.assert_array_equal(outs[0], outs[1])              # graph replay == eager
    np.testing.assert_array_equal(outs[0], outs[2])              # same seed, same image
    _gate(outs[0], _oracle_trajectory(W, unc, ctx, lat0, sch, 7.5, SEED))


def test_tiny_unet_dpmpp2m_in_the_bf16_step(tf):
    from tinyfusers_amd import config
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY
    W, ctx, unc = _tiny()
    sch = S.DPMSolverPP2M().schedule(10)
    config.set_dtype("bf16")
    try:
        sd = StableDiffusion(TINY); update_state(sd.model.diffusion_model, W, "")
        lat = sd.latent_from_numpy(np.zeros((2, 4, 16, 16), np.float32))
        sd.compile(tf.DeviceArray.from_numpy(unc), tf.DeviceArray.from_numpy(ctx), lat, sampler=sch)
        outs = []
        for eager in (False, True):
            sd.start(seed=SEED)
            lat0 = lat.numpy().copy()
            sd.run(7.5, eager=eager); sd.synchronize()
            outs.append(lat.numpy().copy())
    finally:
        config.set_dtype("fp16")
    np.testing.assert_array_equal(outs[0], outs[1])
    _gate(outs[0], _oracle_trajectory(W, unc, ctx, lat0, sch, 7.5, SEED), rel_l2=3e-2, max_rel=3e-2)


def test_sampler_refuses_the_two_chain_cfg_step(tf):
    from tinyfusers_amd import config
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY
    sd = StableDiffusion(TINY)
    lat = sd.latent_from_numpy(np.zeros((1, 4, 16, 16), np.float32))
    c = tf.DeviceArray.from_numpy(np.zeros((1, 13, 64), np.float32))
    old = config.cfg_parallel
    config.cfg_parallel = True
    try:
        with pytest.raises(S.UnsupportedSamplerConfig):
            sd.compile(c, c, lat, sampler=S.DPMSolverPP2M().schedule(10))
    finally:
        config.cfg_parallel = old
    with pytest.raises(S.UnsupportedSamplerConfig):
        sd.start(seed=1)


# ---- 5. SD-1.5, DDIM(0) through the sampler API against the reference's 50-step trajectory ----------------------------------------
def test_sd15_ddim_schedule_through_the_sampler_api_meets_the_reference_trajectory(tf, golden):
    if "unet50_sd15" not in golden:
        pytest.skip("unet50_sd15.npz not generated")
    import oracle
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.variants.samplers import DDIM
    from tinyfusers_amd.variants.sd import StableDiffusion
    g = golden["unet50_sd15"]
    sd = StableDiffusion()
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(sd.model.diffusion_model, synth_state_dict(oracle.unet_param_shapes(oracle.SD15), 0), "")
    noise = synth_normal(1234, "sd.latent", (1, 4, 64, 64))
    lat = sd.latent_from_numpy(noise)
    ctx = tf.DeviceArray.from_numpy(synth_normal(1234, "sd.context", (1, 77, 768)))
    unc = tf.DeviceArray.from_numpy(synth_normal(1234, "sd.uncond", (1, 77, 768)))
    sch = DDIM().schedule(50)
    np.testing.assert_allclose(np.asarray(sch.timesteps[::-1], np.float32), g["timesteps"])
    checkpoints = sorted(int(k[len("x_after_step"):]) for k in g.files if k.startswith("x_after_step"))
    assert checkpoints[-1] == 49 and len(checkpoints) >= 6, checkpoints
    sd.compile(unc, ctx, lat, sampler=sch)
    sd.start(noise=noise)
    traj = {}
    for i in range(50):
        sd.step_sampler(i, 7.5)
        if i in checkpoints:
            sd.synchronize(); traj[i] = lat.numpy().copy()
    report = []
    for n in checkpoints:
        ref = g[f"x_after_step{n}"]
        rl2 = float(np.linalg.norm(traj[n] - ref) / np.linalg.norm(ref)); mx = float(np.abs(traj[n] - ref).max() / np.abs(ref).max())
        report.append((n + 1, round(rl2, 5), round(mx, 5)))
        assert np.isfinite(traj[n]).all() and rl2 <= 5e-3 and mx <= 1e-2, (n, rl2, mx)
    print("DDIM(0) schedule through the sampler API vs the reference (steps done, rel-L2, max|d| / max|ref|):", report)
    sd.start(noise=noise)
    sd.run(7.5); sd.synchronize()
    assert np.array_equal(lat.numpy(), traj[49])
