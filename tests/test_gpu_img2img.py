"""GPU checks of image-to-image and masked inpainting (csrc/img2img.hip and csrc/sampler.hip, StableDiffusion.encode_image / start(init_image=, init_latent=,
mask=) / compile(..., inpaint=True)): the uint8 edge and the encoder against the oracle, the noising of a clean latent against float64
numpy with the host Philox, one masked sampler update against a float64 restatement, tiny-UNet img2img and inpainting trajectories (graph ==
eager, reproducible, against the CPU oracle, the kept region exactly on its noised trajectory) and the SD-1.5 shapes end to end."""
import contextlib
import io
import os
import sys
import time

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


@pytest.fixture(scope="module")
def vae_sd(tf):
    """An SD-1.5 StableDiffusion whose first_stage_model (encoder and decoder) holds synthetic weights; the UNet stays empty."""
    from tinyfusers_amd.storage.state import param_shapes, update_state
    from tinyfusers_amd.storage.synth import synth_state_dict
    from tinyfusers_amd.variants.sd import StableDiffusion
    sd = StableDiffusion()
    W = synth_state_dict(param_shapes(sd.first_stage_model, "first_stage_model"), 0)
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(sd.first_stage_model, W, "first_stage_model")
    return sd, W


def _words(seed):
    return seed & 0xFFFFFFFF, seed >> 32


def _gate(got, ref, rel_l2=5e-3, max_rel=1e-2):
    """tests/test_gpu_samplers.py's gate: rel-L2 and max |d| <= max_rel max |ref| (the latent grows to |x| ~ 25 under CFG 7.5)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all()
    rl2 = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    mx = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"gate: rel-L2 {rl2:.3e} (gate {rel_l2}), max|d|/max|ref| {mx:.3e} (gate {max_rel}), max|ref| {np.abs(ref).max():.1f}")
    assert rl2 <= rel_l2 and mx <= max_rel, (rl2, mx)


def _level_ref(x0, a, seed, offset=0):
    """float64 sqrt(a) x0 + sqrt(1 - a) z, z the tag-0 noise of images offset, offset + 1, ... at step 0; a as the device reads it (fp32)."""
    a = np.float64(np.float32(a))
    n_img = x0[0].size
    z = np.stack([randn_ref(seed, offset + b, n_img, 0, 0).reshape(x0.shape[1:]) for b in range(x0.shape[0])])
    return np.sqrt(a) * x0.astype(np.float64) + np.sqrt(1 - a) * z


def _known_ref(x0_init, a_s, seed, row, offset=0):
    """float64 sqrt(a_s) x0_init + sqrt(1 - a_s) z2, z2 the tag-2 noise of schedule row `row`."""
    a_s = np.float64(np.float32(a_s))
    n_img = x0_init[0].size
    z2 = np.stack([randn_ref(seed, offset + b, n_img, row, 2).reshape(x0_init.shape[1:]) for b in range(x0_init.shape[0])])
    return np.sqrt(a_s) * x0_init.astype(np.float64) + np.sqrt(1 - a_s) * z2


# ---- 1. the uint8 edge ----------------------------------------------------------------------------------------------------------------
def test_image_from_u8_is_exact_and_feeds_encode_as_an_uploaded_image(tf, vae_sd):
    from tinyfusers_amd.native import hip
    sd, _ = vae_sd
    rng = np.random.default_rng(7)
    u = rng.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
    u.reshape(-1)[:256] = np.arange(256)                                  # every value
    want = np.float16(u / 127.5 - 1).transpose(0, 3, 1, 2)              # (B,3,H,W)
    d_u = tf.DeviceArray.from_numpy(u, np.uint8, "row")
    x = tf.DeviceArray.empty((2, 3, 64, 64), np.float16, "nhwc")
    hip.tf_image_from_u8_f16(x.ptr, d_u.ptr, x.size, None)
    got = x.numpy()
    assert np.array_equal(got.astype(np.float16).view(np.uint16), want.view(np.uint16))
    # the scalar path: an odd count from an unaligned source
    y = tf.DeviceArray.empty((101,), np.float16, "row")
    hip.tf_image_from_u8_f16(y.ptr, d_u.ptr + 1, 101, None)
    assert np.array_equal(y.numpy().astype(np.float16).view(np.uint16), np.float16(u.reshape(-1)[1:102] / 127.5 - 1).view(np.uint16))
    # encode of the kernel's output == encode of the same values uploaded from the host
    a = sd.first_stage_model.encode(x).numpy()
    b = sd.first_stage_model.encode(tf.DeviceArray.from_numpy(want.astype(np.float32))).numpy()
    assert np.isfinite(a).all() and np.array_equal(a, b)


# ---- 2. encode_image against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [64, 128])
def test_encode_image_matches_the_oracle_means(tf, vae_sd, size):
    import oracle
    sd, W = vae_sd
    img = np.random.default_rng(size).integers(0, 256, (1, size, size, 3), dtype=np.uint8)
    x0 = sd.encode_image(img)
    assert x0.shape == (1, 4, size // 8, size // 8) and x0.dtype == np.float32 and x0.layout == "row"
    got = x0.numpy()
    Wf = {k: v.astype(np.float16).astype(np.float32) for k, v in W.items()}
    xin = np.float16(img / 127.5 - 1).astype(np.float32).transpose(0, 3, 1, 2)
    means, _ = oracle.autoencoder_kl(xin, Wf)
    ref = 0.18215 * means.numpy().astype(np.float64)
    rl = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print(f"encode_image {size}^2: rel-L2 {rl:.2e} against 0.18215 x the oracle's means")
    assert np.isfinite(got).all() and rl < 5e-3
    # the device uint8 input gives the same latent
    assert np.array_equal(sd.encode_image(tf.DeviceArray.from_numpy(img, np.uint8, "row")).numpy(), got)


def test_encode_image_refuses_an_empty_encoder_and_bad_sizes(tf, vae_sd):
    from tinyfusers_amd.variants.sd import StableDiffusion
    with pytest.raises(RuntimeError, match="no weights"):
        StableDiffusion().encode_image(np.zeros((1, 64, 64, 3), np.uint8))
    sd, _ = vae_sd
    for bad in (np.zeros((1, 60, 64, 3), np.uint8), np.zeros((1, 64, 96, 3), np.uint8)):
        with pytest.raises(ValueError, match="multiple of"):
            sd.encode_image(bad)
    for bad in (np.zeros((1, 64, 64, 3), np.float32), np.zeros((1, 64, 64, 4), np.uint8), np.zeros((64, 64, 3), np.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            sd.encode_image(bad)


# ---- 3. noising to the start level ------------------------------------------------------------------------------------------------------
def test_noise_to_level_matches_float64_and_is_batch_independent(tf):
    from tinyfusers_amd.native import hip
    lo, hi = _words(SEED)
    for shape, a in (((3, 4, 16, 16), 0.3), ((2, 3, 5, 7), 0.8)):     # (105 elements per image: a partial last counter)
        x0 = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
        d_x0 = tf.DeviceArray.from_numpy(x0, np.float32, "row")
        n_img = int(np.prod(shape[1:]))
        out = tf.DeviceArray.empty(shape, np.float32, "row")
        hip.tf_noise_to_level_f32(out.ptr, d_x0.ptr, shape[0], n_img, a, lo, hi, 2, None)
        got = out.numpy()
        ref = _level_ref(x0, a, SEED, 2)
        assert np.all(np.abs(got - ref) <= 2e-6 * (1 + np.abs(ref))), float(np.max(np.abs(got - ref) / (1 + np.abs(ref))))
        for k in range(shape[0]):                                        # batch of B == B batch-1 calls
            one = tf.DeviceArray.empty((1,) + shape[1:], np.float32, "row")
            hip.tf_noise_to_level_f32(one.ptr, d_x0.ptr + 4 * k * n_img, 1, n_img, a, lo, hi, 2 + k, None)
            assert np.array_equal(one.numpy()[0], got[k])
        hip.tf_noise_to_level_f32(d_x0.ptr, d_x0.ptr, shape[0], n_img, a, lo, hi, 2, None)   # in place
        assert np.array_equal(d_x0.numpy(), got)
    # the noise is the text-to-image start's: a = 1e-30 ~ 0 leaves z, which randn_latent draws
    from tinyfusers_amd.variants.sd import StableDiffusion
    z = StableDiffusion.randn_latent((2, 4, 8, 8), SEED).numpy()
    out = tf.DeviceArray.empty((2, 4, 8, 8), np.float32, "row")
    hip.tf_noise_to_level_f32(out.ptr, tf.DeviceArray.zeros((2, 4, 8, 8), np.float32, "row").ptr, 2, 256, 1e-30, lo, hi, 0, None)
    assert np.array_equal(out.numpy(), z)
    with pytest.raises(RuntimeError, match="level"):
        hip.tf_noise_to_level_f32(out.ptr, out.ptr, 2, 256, 0.0, lo, hi, 0, None)


# ---- 4. one masked sampler update -------------------------------------------------------------------------------------------------------
def _set_params(hip, sp, t, a_t, a_p, g, row, seed, offset):
    lo, hi = _words(seed)
    hip.tf_set_sampler_params(sp.ptr, float(t), float(a_t), float(a_p), float(g), row, lo, hi, offset, None, None, 0, None)


def _masked_ref(x, eps2, hist, a_t, a_s, g, row, z, known, m):
    """float64: e = e_u + g (e_c - e_u), x0 = (x - sqrt(1-a_t) e)/sqrt(a_t), x' = c_x x + c_0 x0 + c_1 x0_prev + c_n z, x' <- m x' + (1-m) known."""
    b = x.shape[0]
    e = eps2[:b] + g * (eps2[b:] - eps2[:b])
    a_t = np.float64(np.float32(a_t))
    x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
    c_x, c_0, c_1, c_n = (np.float64(np.float32(c)) for c in row)
    xn = c_x * x + c_0 * x0 + (c_1 * hist if c_1 != 0 else 0.0) + c_n * z
    return m * xn + (1 - m) * known, x0


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["ddim-eta", "euler-a", "dpmpp2m"])
def test_one_masked_sampler_step_matches_float64(tf, name, dtype):
    from tinyfusers_amd.native import hip
    from tinyfusers_amd.storage.tensor import bfloat16
    from tinyfusers_amd.variants import samplers as S
    for B, C, H, W in ((2, 4, 8, 12), (2, 3, 5, 7)):             # (105 elements per image: a partial last counter)
        n_img, g, offset = C * H * W, 7.5, 5
        sch = S.make(name).schedule(25, strength=0.8)
        i = 9
        table = sch.coeffs.copy()
        table[i, 2] = table[i, 2] or 0.25                            # every term live: c_1 != 0 and c_n != 0
        table[i, 3] = table[i, 3] or 0.6
        rng = np.random.default_rng(4)
        x, hist, x0i = (rng.standard_normal((B, C, H, W)).astype(np.float32) for _ in range(3))
        eps2 = rng.standard_normal((2 * B, C, H, W))
        m = rng.random((B, 1, H, W)).astype(np.float32)               # fractional, with exact 0 and 1 pixels
        m[:, :, 0, :4], m[:, :, 1, :4] = 0.0, 1.0
        dt = bfloat16 if dtype == "bf16" else np.float16
        d_eps = tf.DeviceArray.from_numpy(eps2, dt, "nhwc")
        eps2 = d_eps.numpy().astype(np.float64)                      # the values the kernel reads
        d_tab = tf.DeviceArray.from_numpy(table.astype(np.float32), np.float32, "row")
        sp = tf.DeviceArray.zeros((8,), np.float32, "row")
        masked = hip.tf_cfg_sampler_step_masked_bf16 if dtype == "bf16" else hip.tf_cfg_sampler_step_masked_f32
        plain = hip.tf_cfg_sampler_step_bf16 if dtype == "bf16" else hip.tf_cfg_sampler_step_f32

        def run(row, lo_img, hi_img, mask, off=offset, with_mask=True):
            sl = slice(lo_img, hi_img)
            lat = tf.DeviceArray.from_numpy(x[sl], np.float32, "row")
            h = tf.DeviceArray.from_numpy(hist[sl], np.float32, "row")
            xi = tf.DeviceArray.from_numpy(x0i[sl], np.float32, "row")
            dm = tf.DeviceArray.from_numpy(mask[sl], np.float32, "row")
            e2 = d_eps if (lo_img, hi_img) == (0, B) else tf.DeviceArray.from_numpy(np.concatenate([eps2[sl], eps2[B + lo_img:B + hi_img]]), dt, "nhwc")
            _set_params(hip, sp, sch.timesteps[row], sch.alphas[row], sch.alphas_prev[row], g, row, SEED, off)
            nb = hi_img - lo_img
            if with_mask:
                masked(lat.ptr, e2.ptr, h.ptr, sp.ptr, d_tab.ptr, len(table), xi.ptr, dm.ptr, nb, C, H, W, None)
            else:
                plain(lat.ptr, e2.ptr, h.ptr, sp.ptr, d_tab.ptr, len(table), nb, C, H, W, None)
            return lat.numpy(), h.numpy()

        z = np.stack([randn_ref(SEED, offset + b, n_img, i, 1).reshape(C, H, W) for b in range(B)])
        known = _known_ref(x0i, sch.alphas_prev[i], SEED, i, offset)
        got, got_h = run(i, 0, B, m)
        ref, ref_x0 = _masked_ref(x, eps2, hist, sch.alphas[i], sch.alphas_prev[i], g, table[i], z, known, m)
        assert np.all(np.abs(got - ref) <= 1e-5 * (1 + np.abs(ref))), float(np.max(np.abs(got - ref) / (1 + np.abs(ref))))
        assert np.all(np.abs(got_h - ref_x0) <= 1e-5 * (1 + np.abs(ref_x0)))
        keep = np.broadcast_to(m == 0, got.shape)                     # the kept pixels: sqrt(a_s) x0_init + sqrt(1 - a_s) z2, z2 = tag 2 at the row
        assert keep.sum() > 0 and np.all(np.abs(got[keep] - known[keep]) <= 2e-6 * (1 + np.abs(known[keep])))
        # batch independence: image 1 alone, as global image offset + 1
        one, _ = run(i, 1, 2, m, off=offset + 1)
        assert np.array_equal(one[0], got[1])
        # mask 1 everywhere: the unmasked update, bit for bit
        ones = np.ones_like(m)
        a, ah = run(i, 0, B, ones)
        b, bh = run(i, 0, B, ones, with_mask=False)
        assert np.array_equal(a, b) and np.array_equal(ah, bh)
        # the last row (a_s = 1) with mask 0: x0_init exactly
        last = len(table) - 1
        assert sch.alphas_prev[last] == 1.0
        fin, _ = run(last, 0, B, np.zeros_like(m))
        assert np.array_equal(fin, x0i)


# ---- 5. / 6. tiny-UNet img2img and inpainting --------------------------------------------------------------------------------------------
def _tiny(seed=5):
    import oracle
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    W = synth_state_dict(oracle.unet_param_shapes(oracle.TINY), seed)
    ctx = synth_normal(seed, "c", (2, 13, 64)).astype(np.float16).astype(np.float32)
    unc = synth_normal(seed, "u", (2, 13, 64)).astype(np.float16).astype(np.float32)
    x0 = synth_normal(seed, "x0", (2, 4, 16, 16))
    return W, ctx, unc, x0


def _oracle_trajectory(W, unc, ctx, lat0, sch, g, seed, x0_init=None, mask=None):
    """The sampler of tests/test_gpu_samplers.py on the CPU oracle's UNet, from lat0; with a mask, each step ends in the blend."""
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
        if mask is not None:
            x = mask * x + (1 - mask) * _known_ref(x0_init, sch.alphas_prev[i], seed, i)
    return x


def _model(tf, W, unc, ctx, sch, inpaint=False):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY
    sd = StableDiffusion(TINY); update_state(sd.model.diffusion_model, W, "")
    lat = sd.latent_from_numpy(np.zeros((2, 4, 16, 16), np.float32))
    sd.compile(tf.DeviceArray.from_numpy(unc), tf.DeviceArray.from_numpy(ctx), lat, sampler=sch, inpaint=inpaint)
    return sd, lat


def _img2img_runs(tf, name):
    from tinyfusers_amd.variants import samplers as S
    W, ctx, unc, x0 = _tiny()
    sch = S.make(name).schedule(10, strength=0.6)
    assert len(sch.timesteps) == 6
    sd, lat = _model(tf, W, unc, ctx, sch)
    outs = []
    for k, eager in enumerate((False, True, False)):
        sd.start(seed=SEED, init_latent=x0 if k != 1 else tf.DeviceArray.from_numpy(x0, np.float32, "row"))
        if not outs:
            lat0 = lat.numpy().copy()
        sd.run(7.5, eager=eager); sd.synchronize()
        outs.append(lat.numpy().copy())
    return W, ctx, unc, x0, sch, lat0, outs


@pytest.mark.parametrize("name", ["dpmpp2m", "euler-a"])
def test_tiny_unet_img2img_graph_eager_seed_and_oracle(tf, name):
    W, ctx, unc, x0, sch, lat0, outs = _img2img_runs(tf, name)
    ref0 = _level_ref(x0, sch.alphas[0], SEED)
    assert np.all(np.abs(lat0 - ref0) <= 2e-6 * (1 + np.abs(ref0)))
    np.testing.assert_array_equal(outs[0], outs[1])              # graph replay == eager
    np.testing.assert_array_equal(outs[0], outs[2])              # same seed, same image
    _gate(outs[0], _oracle_trajectory(W, unc, ctx, lat0, sch, 7.5, SEED))


def test_tiny_unet_inpainting_all_zero_all_one_and_half_masks(tf):
    from tinyfusers_amd.variants import samplers as S
    W, ctx, unc, x0 = _tiny()
    sch = S.DPMSolverPP2M().schedule(10, strength=0.6)
    sd, lat = _model(tf, W, unc, ctx, sch, inpaint=True)
    with pytest.raises(ValueError, match="init"):
        sd.start(seed=SEED)
    # mask all 0: nothing is repainted, the last step lands on x0_init exactly
    sd.start(seed=SEED, init_latent=x0, mask=np.zeros((2, 1, 16, 16), np.float32))
    sd.run(7.5); sd.synchronize()
    assert np.array_equal(lat.numpy(), x0)
    # mask all 1 (and no mask: all ones): the unmasked img2img run, bit for bit
    _, _, _, _, _, _, plain = _img2img_runs(tf, "dpmpp2m")
    for mask in (np.ones((2, 128, 128), np.uint8), None):
        sd.start(seed=SEED, init_latent=x0, mask=mask)
        sd.run(7.5); sd.synchronize()
        got = lat.numpy()
        print(f"mask all 1 vs unmasked: max |d| = {np.abs(got - plain[0]).max():.3e}")
        assert np.array_equal(got, plain[0])
    # half mask: after every step the kept half is exactly on its noised trajectory; the whole latent meets the oracle
    m = np.zeros((2, 1, 16, 16), np.float32); m[..., :8] = 1.0
    _half_mask_run(tf, sd, lat, W, unc, ctx, x0, sch, m, gates=(5e-3, 1e-2))


def _half_mask_run(tf, sd, lat, W, unc, ctx, x0, sch, m, gates, eager=False):
    sd.start(seed=SEED, init_latent=x0, mask=m)
    lat0 = lat.numpy().copy()
    keep = np.broadcast_to(m == 0, lat0.shape)
    for i in range(len(sch.timesteps)):
        sd.step_sampler(i, 7.5, eager=eager); sd.synchronize()
        got = lat.numpy()
        known = _known_ref(x0, sch.alphas_prev[i], SEED, i)
        assert np.all(np.abs(got[keep] - known[keep]) <= 2e-6 * (1 + np.abs(known[keep]))), i
    _gate(got, _oracle_trajectory(W, unc, ctx, lat0, sch, 7.5, SEED, x0, m), *gates)
    return got


def test_tiny_unet_inpainting_in_the_bf16_step(tf):
    """The half-mask checks in the bfloat16 step, at the bf16 gates of test_tiny_unet_dpmpp2m_in_the_bf16_step.  Over the full schedule
    (strength 1): those gates bound max |d| by max |ref| of a trajectory from noise (|x| ~ 25); from strength 0.6 the latent stays near
    |x| ~ 11 while the bf16 UNet's absolute error is the same (measured there: rel-L2 2.4e-2, max |d| 0.40 = 3.5e-2 max |ref|)."""
    from tinyfusers_amd import config
    from tinyfusers_amd.variants import samplers as S
    W, ctx, unc, x0 = _tiny()
    sch = S.DPMSolverPP2M().schedule(10, strength=1.0)
    m = np.zeros((2, 1, 16, 16), np.float32); m[..., :8] = 1.0
    config.set_dtype("bf16")
    try:
        sd, lat = _model(tf, W, unc, ctx, sch, inpaint=True)
        a = _half_mask_run(tf, sd, lat, W, unc, ctx, x0, sch, m, gates=(3e-2, 3e-2))
        b = _half_mask_run(tf, sd, lat, W, unc, ctx, x0, sch, m, gates=(3e-2, 3e-2), eager=True)
        sd.start(seed=SEED, init_latent=x0, mask=np.zeros_like(m))
        sd.run(7.5); sd.synchronize()
        zero = lat.numpy()
    finally:
        config.set_dtype("fp16")
    assert np.array_equal(a, b)
    assert np.array_equal(zero, x0)


def test_inpaint_and_mask_arguments_are_checked(tf):
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY
    W, ctx, unc, x0 = _tiny()
    sd = StableDiffusion(TINY)
    lat = sd.latent_from_numpy(np.zeros((2, 4, 16, 16), np.float32))
    c = tf.DeviceArray.from_numpy(ctx)
    with pytest.raises(ValueError, match="inpaint"):
        sd.compile(c, c, lat, inpaint=True)
    sch = S.DPMSolverPP2M().schedule(10, strength=0.6)
    sd, lat = _model(tf, W, unc, ctx, sch)
    with pytest.raises(ValueError, match="inpaint=True"):
        sd.start(seed=SEED, init_latent=x0, mask=np.ones((2, 1, 16, 16), np.float32))
    with pytest.raises(ValueError, match="not both"):
        sd.start(seed=SEED, init_latent=x0, init_image=np.zeros((2, 128, 128, 3), np.uint8))
    with pytest.raises(ValueError, match="seed"):
        sd.start(init_latent=x0)
    with pytest.raises(ValueError, match="shape"):
        sd.start(seed=SEED, init_latent=x0[:1])
    sd, lat = _model(tf, W, unc, ctx, sch, inpaint=True)
    with pytest.raises(ValueError, match="latent size"):
        sd.start(seed=SEED, init_latent=x0, mask=np.ones((2, 64, 64), np.uint8))


def test_a_refused_start_changes_nothing_of_the_run_in_progress(tf):
    """start() checks every argument before it writes: refused in the middle of a schedule it leaves seed, cursor, latent and the inpainting
    buffers alone, and run() finishes the schedule as if the refused calls had not been made."""
    from tinyfusers_amd.variants import samplers as S
    W, ctx, unc, x0 = _tiny()
    sch = S.DPMSolverPP2M().schedule(4)
    m = np.zeros((2, 1, 16, 16), np.float32); m[..., :8] = 1.0
    sd, lat = _model(tf, W, unc, ctx, sch, inpaint=True)
    sd.start(seed=3, init_latent=x0, mask=m)
    sd.run(7.5); sd.synchronize()
    want = lat.numpy().copy()
    sd.start(seed=3, init_latent=x0, mask=m)
    sd.step_sampler(0, 7.5)
    for bad in (dict(init_latent=x0[:1]),                                                       # a wrong shape
                dict(init_latent=tf.DeviceArray.from_numpy(x0, np.float16, "row")),              # a device array that is not fp32
                dict(init_latent=x0, mask=np.ones((2, 64, 64), np.uint8)),                       # a mask of another latent size
                dict(init_image=np.zeros((2, 64, 64, 3), np.uint8))):                            # an image that encodes to (2,4,8,8)
        with pytest.raises(ValueError):
            sd.start(seed=SEED, **bad)
    sd.run(7.5); sd.synchronize()                                 # continues from step 1, with seed 3
    assert np.array_equal(lat.numpy(), want)


# ---- 7. SD-1.5 shapes ------------------------------------------------------------------------------------------------------------------
def test_sd15_img2img_and_inpainting_at_512(tf):
    import oracle
    from tinyfusers_amd.storage.state import param_shapes, update_state
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.variants.samplers import DPMSolverPP2M
    from tinyfusers_amd.variants.sd import StableDiffusion
    sd = StableDiffusion()
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(sd.model.diffusion_model, synth_state_dict(oracle.unet_param_shapes(oracle.SD15), 0), "")
        update_state(sd.first_stage_model, synth_state_dict(param_shapes(sd.first_stage_model, "first_stage_model"), 0), "first_stage_model")
    img = np.random.default_rng(9).integers(0, 256, (1, 512, 512, 3), dtype=np.uint8)
    ctx = tf.DeviceArray.from_numpy(synth_normal(1234, "sd.context", (1, 77, 768)))
    unc = tf.DeviceArray.from_numpy(synth_normal(1234, "sd.uncond", (1, 77, 768)))
    sch = DPMSolverPP2M().schedule(20, strength=0.5)
    assert len(sch.timesteps) == 10
    lat = sd.latent_from_numpy(np.zeros((1, 4, 64, 64), np.float32))
    sd.compile(unc, ctx, lat, sampler=sch, inpaint=True)
    for _ in range(2):
        hip_sync = tf.hip.tf_stream_sync
        t0 = time.perf_counter()
        x0 = sd.encode_image(img)
        hip_sync(None)
        enc_ms = 1e3 * (time.perf_counter() - t0)
    print(f"encode_image 512^2 -> {x0.shape}: {enc_ms:.1f} ms (second call)")
    sd.start(seed=SEED, init_image=img)                           # no mask: all ones, the img2img run
    sd.run(7.5); sd.synchronize()
    assert np.isfinite(lat.numpy()).all()
    sd.start(seed=SEED, init_image=img, mask=np.zeros((1, 512, 512), bool))
    sd.run(7.5); sd.synchronize()
    final, x0_init = lat.numpy(), sd._x0_init.numpy()
    assert np.isfinite(final).all() and np.array_equal(final, x0_init)
    with tf.use_stream(sd._stream):
        a = sd.decode(lat)
        b = sd.decode(sd._x0_init)
    assert a.shape == (512, 512, 3) and np.array_equal(a, b)
