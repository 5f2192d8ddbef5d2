"""Host-side checks of the concat-conditioned checkpoints (no GPU): StableDiffusion.concat_mask / concat_mask_u8 (the nearest-neighbour mask
rule of the SD-1.5 inpainting UNet, against latent_mask's block maximum), the SD15_INPAINT / SD15_EDIT configurations and the module trees they
build, the compile() refusals that are decided before any device work, and the header block of the concat-conditioned entries (test_abi checks that the
library exports what the header declares)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. concat_mask ---------------------------------------------------------------------------------------------------------------------
def test_concat_mask_is_the_nearest_pixel_not_the_block_maximum():
    from tinyfusers_amd.variants.sd import StableDiffusion as SD
    m = np.zeros((2, 16, 24), np.uint8)
    m[0, 3, 5] = 1              # block (0, 0): set, but not at its [8i, 8j] corner
    m[0, 8, 16] = 7             # block (1, 2): its corner pixel (any nonzero uint8 repaints)
    m[1, 15, 23] = 1            # block (1, 2) of image 1: the far corner
    got = SD.concat_mask(m)
    assert got.shape == (2, 1, 2, 3) and got.dtype == np.float32
    want = np.zeros((2, 1, 2, 3), np.float32); want[0, 0, 1, 2] = 1.0
    assert np.array_equal(got, want)
    blend = SD.latent_mask(m)
    assert blend[0, 0, 0, 0] == 1.0 and got[0, 0, 0, 0] == 0.0           # where the blend's 8x8 maximum repaints, the nearest rule does not
    assert blend[1, 0, 1, 2] == 1.0 and got[1, 0, 1, 2] == 0.0
    assert np.array_equal(got, m[:, None, ::8, ::8] != 0)


def test_concat_mask_dtypes_and_the_uint8_image_mask():
    from tinyfusers_amd.variants.sd import StableDiffusion as SD
    rng = np.random.default_rng(3)
    f = rng.random((2, 16, 16)).astype(np.float32)
    f[0, 0, 0], f[0, 0, 8], f[0, 8, 0] = 0.5, 0.49999, 1.0              # binarised at image resolution: >= 0.5 repaints
    rep = f >= 0.5
    for m in (f, f.astype(np.float64), rep, rep.astype(np.uint8) * 255):
        u8 = SD.concat_mask_u8(m)
        assert u8.dtype == np.uint8 and u8.shape == (2, 16, 16) and u8.flags["C_CONTIGUOUS"] and np.array_equal(u8, rep.astype(np.uint8))
        lm = SD.concat_mask(m)
        assert lm.dtype == np.float32 and np.array_equal(lm, rep[:, None, ::8, ::8].astype(np.float32))
    assert SD.concat_mask(f)[0, 0].tolist() == [[1.0, 0.0], [1.0, float(rep[0, 8, 8])]]


@pytest.mark.parametrize("bad,exc", [
    (np.zeros((1, 12, 16), np.float32), ValueError),                  # H not a multiple of 8
    (np.zeros((16, 16), np.float32), ValueError),                     # no batch axis
    (np.zeros((1, 1, 2, 2), np.float32), ValueError),                 # a latent-size array is not a mask at image resolution
    (np.zeros((0, 16, 16), np.uint8), ValueError),
    (np.full((1, 16, 16), 1.5, np.float32), ValueError),              # out of [0, 1]
    (np.full((1, 16, 16), np.nan, np.float32), ValueError),
    (np.zeros((1, 16, 16), np.int32), TypeError),
])
def test_concat_mask_refuses_bad_shapes_ranges_and_types(bad, exc):
    from tinyfusers_amd.variants.sd import StableDiffusion as SD
    with pytest.raises(exc):
        SD.concat_mask(bad)
    with pytest.raises(exc):
        SD.concat_mask_u8(bad)


# ---- 2. configurations and module trees ---------------------------------------------------------------------------------------------------
def test_the_concat_configs_differ_from_sd15_in_the_input_channels_only():
    from dataclasses import replace
    from tinyfusers_amd.vision.unet import SD15, SD15_EDIT, SD15_INPAINT
    assert (SD15.in_channels, SD15_INPAINT.in_channels, SD15_EDIT.in_channels) == (4, 9, 8)
    assert replace(SD15_INPAINT, in_channels=4) == SD15 and replace(SD15_EDIT, in_channels=4) == SD15
    assert SD15_INPAINT.out_channels == SD15_EDIT.out_channels == 4


@pytest.mark.parametrize("name,cin", [("SD15_INPAINT", 9), ("SD15_EDIT", 8)])
def test_a_concat_model_has_the_wide_conv_in_the_vae_and_the_text_encoder(name, cin):
    import oracle
    from dataclasses import replace
    from tinyfusers_amd.storage.state import param_shapes
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision import unet
    sd = StableDiffusion(getattr(unet, name))
    shapes = param_shapes(sd)
    assert tuple(shapes["model.diffusion_model.input_blocks.0.0.weight"]) == (320, cin, 3, 3)
    assert tuple(shapes["model.diffusion_model.out.2.weight"]) == (4, 320, 3, 3)
    assert tuple(shapes["first_stage_model.encoder.conv_in.weight"]) == (128, 3, 3, 3)
    assert tuple(shapes["first_stage_model.quant_conv.weight"]) == (8, 8, 1, 1)
    assert "first_stage_model.decoder.conv_out.weight" in shapes
    assert any(k.startswith("cond_stage_model.transformer.text_model.") for k in shapes)
    # the UNet's names and shapes are the oracle's for the same configuration
    want = oracle.unet_param_shapes(replace(oracle.SD15, in_channels=cin))
    got = {k[len("model.diffusion_model."):]: tuple(v) for k, v in shapes.items() if k.startswith("model.diffusion_model.")}
    assert got == {k: tuple(v) for k, v in want.items()}


# ---- 3. refusals decided before any device work --------------------------------------------------------------------------------------------
def test_compile_refuses_mismatched_concat_arguments_before_touching_a_device():
    from tinyfusers_amd.variants.samplers import DPMSolverPP2M
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import SD15_EDIT, SD15_INPAINT, TINY
    from dataclasses import replace
    sch = DPMSolverPP2M().schedule(4)
    plain, inp, edit = StableDiffusion(TINY), StableDiffusion(replace(TINY, in_channels=9)), StableDiffusion(SD15_EDIT)
    assert StableDiffusion(SD15_INPAINT).model.diffusion_model.cfg.in_channels == 9
    with pytest.raises(ValueError, match="concat="):
        plain.compile(None, None, None, sampler=sch, concat="outpaint")
    with pytest.raises(ValueError, match="sampler"):
        inp.compile(None, None, None, concat="inpaint")
    with pytest.raises(ValueError, match="in_channels=9"):
        plain.compile(None, None, None, sampler=sch, concat="inpaint")
    with pytest.raises(ValueError, match="in_channels=8"):
        inp.compile(None, None, None, sampler=sch, concat="edit")
    with pytest.raises(ValueError, match="in_channels=9"):
        edit.compile(None, None, None, sampler=sch, concat="inpaint")
    with pytest.raises(ValueError, match="concat-conditioned"):
        inp.compile(None, None, None, sampler=sch)
    with pytest.raises(ValueError, match="concat-conditioned"):
        edit.compile(None, None, None)
    with pytest.raises(ValueError, match="inpaint=True"):
        inp.compile(None, None, None, sampler=sch, concat="inpaint", inpaint=True)


# ---- 4. header ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_concat_entries_with_their_citations():
    hdr = open(os.path.join(ROOT, "include", "tinyfusers_hip.h")).read()
    i = hdr.index("---- concat-conditioned UNets")
    block = hdr[hdr.rindex("/*", 0, i):]
    head = block[:block.index("*/")]
    for cite in ("variants/sd.py:31", "variants/sd.py:14-25", "vae/vae.py:12-15"):
        assert cite in head, cite
    names = set(re.findall(r"\b(tf_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", block, flags=re.S)))
    assert names == {"tf_cfg_concat_f16", "tf_cfg_concat_bf16", "tf_cfg3_sampler_step_f32", "tf_cfg3_sampler_step_bf16", "tf_image_from_u8_masked_f16",
                     "tf_means_to_cond_f32"}
