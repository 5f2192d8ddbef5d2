"""Host checks of image-to-image and inpainting (no GPU): the ``strength`` schedules of Sampler.schedule (a suffix of the full walk with its
coefficient table rebuilt on the truncated walk), StableDiffusion.latent_mask, the uint8 -> fp16 formula of tf_image_from_u8_f16, and the
header block of csrc/img2img.hip (test_abi checks that the library exports what the header declares), and what a model that was never compiled
answers."""
import math
import os
import re

import numpy as np
import pytest

from tinyfusers_amd.variants import samplers as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLERS = [S.DDIM(), S.DDIM(1.0), S.EulerAncestral(), S.DPMSolverPP2M()]


def _same(a, b):
    assert a.sampler is b.sampler and a.timesteps == b.timesteps
    for f in ("alphas", "alphas_prev", "coeffs"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), f


# ---- 1. strength schedules ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", SAMPLERS, ids=repr)
def test_strength_one_is_todays_schedule(sampler):
    for steps in range(1, 51):
        _same(sampler.schedule(steps, strength=1.0), sampler.schedule(steps))
    ts = [961, 700, 400, 121, 3]
    _same(sampler.schedule(timesteps=ts, strength=1), sampler.schedule(timesteps=ts))
    assert S.Schedule._fields == ("sampler", "timesteps", "alphas", "alphas_prev", "coeffs")


@pytest.mark.parametrize("sampler", SAMPLERS, ids=repr)
@pytest.mark.parametrize("strength", [0.01, 0.3, 0.5, 0.6, 0.75, 0.999])
def test_strength_keeps_the_tail_of_the_walk_and_rebuilds_its_table(sampler, strength):
    for steps in (1, 2, 7, 20, 50):
        full, sch = sampler.schedule(steps), sampler.schedule(steps, strength=strength)
        n = len(full.timesteps)
        k = max(1, math.floor(n * strength))
        assert len(sch.timesteps) == k and sch.timesteps == full.timesteps[n - k:]
        assert np.array_equal(sch.alphas, full.alphas[n - k:]) and np.array_equal(sch.alphas_prev, full.alphas_prev[n - k:])
        assert sch.alphas_prev[-1] == 1.0
        walk = np.concatenate([sch.alphas, [1.0]])
        assert np.array_equal(sch.coeffs, sampler.coefficients(walk))
        assert sch.sampler is sampler


def test_dpmpp2m_first_kept_step_is_first_order():
    sampler = S.DPMSolverPP2M()
    for steps in (10, 20, 50):
        full = sampler.schedule(steps)
        for strength in (0.3, 0.5, 0.6, 0.9):
            sch = sampler.schedule(steps, strength=strength)
            k = len(sch.timesteps)
            assert sch.coeffs[0, 2] == 0.0
            assert full.coeffs[len(full.timesteps) - k, 2] != 0.0          # (the same step of the full walk is second order)
            np.testing.assert_array_equal(sch.coeffs[1:], full.coeffs[len(full.timesteps) - k + 1:])


def test_the_start_level_of_strength_is_alphas0():
    sch = S.DPMSolverPP2M().schedule(20, strength=0.5)
    ac = S.get_alphas_cumprod()
    assert sch.timesteps[0] == S.default_timesteps(20)[10] and sch.alphas[0] == np.float64(ac[sch.timesteps[0]])


@pytest.mark.parametrize("bad", [0, 0.0, -0.5, 1.0000001, 2, float("nan"), float("inf"), -float("inf")])
def test_invalid_strength_raises(bad):
    with pytest.raises(ValueError, match="strength"):
        S.DDIM().schedule(20, strength=bad)


# ---- 2. latent_mask -----------------------------------------------------------------------------------------------------------------
def _mask_ref(rep):
    b, h, w = rep.shape
    out = np.zeros((b, 1, h // 8, w // 8), np.float32)
    for k in range(b):
        for i in range(h // 8):
            for j in range(w // 8):
                out[k, 0, i, j] = float(rep[k, 8 * i:8 * i + 8, 8 * j:8 * j + 8].any())
    return out


def test_latent_mask_is_the_8x8_maximum_of_the_thresholded_mask():
    from tinyfusers_amd.variants.sd import StableDiffusion as SD
    rng = np.random.default_rng(3)
    f = rng.random((2, 32, 48)) ** 40                                # mostly below 0.5: some 8x8 blocks hold no pixel >= 0.5
    rep = f >= 0.5
    want = _mask_ref(rep)
    assert 0 < want.mean() < 1
    for m in (f, f.astype(np.float32), rep, rep.astype(np.uint8), rep.astype(np.uint8) * 255):
        got = SD.latent_mask(m)
        assert got.dtype == np.float32 and got.shape == (2, 1, 4, 6)
        np.testing.assert_array_equal(got, want)
    one = np.zeros((1, 16, 16), np.float32); one[0, 9, 3] = 0.5          # a single pixel at the threshold repaints its latent pixel
    np.testing.assert_array_equal(SD.latent_mask(one)[0, 0], [[0, 0], [1, 0]])
    one[0, 9, 3] = 0.49
    assert SD.latent_mask(one).sum() == 0


def test_latent_mask_passes_a_latent_size_float_mask_through():
    from tinyfusers_amd.variants.sd import StableDiffusion as SD
    m = np.random.default_rng(0).random((3, 1, 5, 7))
    got = SD.latent_mask(m)
    assert got.dtype == np.float32 and got.shape == m.shape and np.array_equal(got, m.astype(np.float32))


@pytest.mark.parametrize("bad,exc", [
    (np.zeros((1, 12, 16), np.float32), ValueError),                  # H not a multiple of 8
    (np.zeros((16, 16), np.float32), ValueError),                     # no batch axis
    (np.zeros((1, 2, 4, 4), np.float32), ValueError),                 # a latent-size mask has one channel
    (np.zeros((1, 1, 4, 4), np.uint8), ValueError),                   # ... and is float
    (np.full((1, 16, 16), 1.5, np.float32), ValueError),              # out of [0, 1]
    (np.full((1, 16, 16), -0.1), ValueError),
    (np.full((1, 1, 2, 2), np.nan, np.float32), ValueError),
    (np.zeros((1, 16, 16), np.int32), TypeError),
])
def test_latent_mask_refuses_bad_shapes_ranges_and_types(bad, exc):
    from tinyfusers_amd.variants.sd import StableDiffusion as SD
    with pytest.raises(exc):
        SD.latent_mask(bad)


def test_encoder_size_rule():
    from tinyfusers_amd import config
    from tinyfusers_amd.variants.sd import StableDiffusion as SD
    assert config.head_merge == "reference_exact"
    for h, w in ((512, 512), (64, 64), (128, 64), (96, 1280)):
        assert SD.encoder_size_error(h, w) is None
    for h, w in ((500, 512), (512, 500), (0, 64), (64, 96), (64, 1344)):
        assert SD.encoder_size_error(h, w)


# ---- 3. the u8 -> fp16 map ------------------------------------------------------------------------------------------------------------
def test_u8_to_fp16_formula_is_exact_and_tf_image_to_u8_inverts_it():
    """tf_image_from_u8_f16 computes fp16((float)(2u - 255) / 255.0f): for every u it is the fp16 of u / 127.5 - 1, and the decode tail
    (tf_image_to_u8, variants/sd.py:51-53: ((x + 1) / 2) * 255, truncated) gives back u up to the fp16 rounding."""
    u = np.arange(256)
    dev = ((2 * u - 255).astype(np.float32) / np.float32(255)).astype(np.float16)
    want = np.float16(u / 127.5 - 1)
    assert np.array_equal(dev.view(np.uint16), want.view(np.uint16))
    back = (np.clip((dev.astype(np.float32) + np.float32(1)) * np.float32(0.5), 0, 1) * np.float32(255)).astype(np.uint8)
    assert np.abs(back.astype(int) - u).max() <= 1


# ---- 4. header -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_img2img_entries_with_their_citations():
    hdr = open(os.path.join(ROOT, "include", "tinyfusers_hip.h")).read()
    i = hdr.index("csrc/img2img.hip")
    block = hdr[hdr.rindex("/*", 0, i):]
    head = block[:block.index("*/")]
    for cite in ("vae/vae.py:12-15", "variants/sd.py:48-54", "variants/sd.py:14-25"):
        assert cite in head, cite
    names = set(re.findall(r"\b(tf_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", block, flags=re.S)))
    assert {"tf_image_from_u8_f16", "tf_means_to_latent_f32", "tf_noise_to_level_f32", "tf_cfg_sampler_step_masked_f32",
            "tf_cfg_sampler_step_masked_bf16"} <= names


# ---- 5. a model that was never compiled -----------------------------------------------------------------------------------------------
def test_a_model_that_was_never_compiled_names_compile_in_every_refusal():
    from tinyfusers_amd.variants.samplers import UnsupportedSamplerConfig
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY
    sd = StableDiffusion(TINY)
    x = np.zeros((1, 4, 8, 8), np.float32)
    for exc, call in ((RuntimeError, lambda: sd.step(981.0, 0.5, 0.6, 7.5)), (RuntimeError, lambda: sd.set_latent(x)),
                      (RuntimeError, lambda: sd.set_context(x, x)), (RuntimeError, sd.synchronize),
                      (UnsupportedSamplerConfig, lambda: sd.start(seed=1)), (UnsupportedSamplerConfig, lambda: sd.run(7.5)),
                      (UnsupportedSamplerConfig, lambda: sd.step_sampler(0, 7.5))):
        with pytest.raises(exc, match="compile"):
            call()
