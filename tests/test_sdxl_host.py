"""Host checks of the SDXL path: the UNet plan (transformer depth per level, label_emb) and its parameter total, the unchanged plans of the earlier
configurations name for name (tests/golden/unet_param_names.json, recorded with the parent commit's code), the compile / start refusals, the vector
conditioning of tests/aux/sdxl_ref.py against its closed form, and the pooled index rule."""
import json
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "aux"))

import sdxl_ref as X  # noqa: E402


@pytest.fixture(scope="module")
def built():
    import __graft_entry__
    __graft_entry__.build()


def test_sdxl_plan_and_parameter_total(built):
    from tinyfusers_amd.attention.attention import SpatialTransformer
    from tinyfusers_amd.storage.state import param_shapes
    from tinyfusers_amd.vision.resnet import ResBlock
    from tinyfusers_amd.vision.unet import SDXL, TINY_XL, UNetModel, depth_at, head_sizes, heads_at, pag_layers
    unet = UNetModel(SDXL)
    ps = param_shapes(unet)
    assert sum(int(np.prod(s)) for s in ps.values()) == 2_567_463_684
    assert ps["label_emb.0.0.weight"] == (1280, 2816) and ps["label_emb.0.2.weight"] == (1280, 1280) and ps["label_emb.0.2.bias"] == (1280,)
    assert ps["input_blocks.4.1.transformer_blocks.1.attn2.to_k.weight"] == (640, 2048)
    assert ps["middle_block.1.transformer_blocks.9.ff.net.2.weight"] == (1280, 5120)
    assert ps["output_blocks.8.0.skip_connection.weight"] == (320, 640, 1, 1)
    assert not any(k.startswith("input_blocks.1.1.") for k in ps) and "input_blocks.4.1.transformer_blocks.2.norm1.weight" not in ps
    assert "middle_block.1.transformer_blocks.10.norm1.weight" not in ps and "input_blocks.9.0.in_layers.0.weight" not in ps       # three levels: 9 input blocks
    assert ps == X.unet_shapes(SDXL)                                   # the reference's own statement of the plan, name for name
    assert param_shapes(UNetModel(TINY_XL)) == X.unet_shapes(TINY_XL)
    sts = unet._all(SpatialTransformer)
    depths = [len(st.transformer_blocks) for st in sts]
    assert depths == [2, 2, 10, 10, 10, 10, 10, 10, 2, 2, 2] and sum(depths) == 70
    assert [st.transformer_blocks[-1].attn2.num_heads for st in sts] == [10, 10, 20, 20, 20, 20, 20, 20, 10, 10, 10]
    assert sum(2 * blk.attn2.to_k.out_features for st in sts for blk in st.transformer_blocks) == 166_400       # kv_n of the one K|V GEMM
    assert sum(r.emb_layers[1].out_features for r in unet._all(ResBlock)) == 13_760                              # ResBlock-projection columns
    assert [depth_at(SDXL, lev) for lev in (0, 1, 2, "mid")] == [0, 2, 10, 10] and head_sizes(SDXL) == [64] and heads_at(SDXL, 640) == (10, 64)
    assert pag_layers(SDXL) == ["input_blocks.4", "input_blocks.5", "input_blocks.7", "input_blocks.8", "middle_block"] + [f"output_blocks.{i}" for i in range(6)]
    from dataclasses import replace
    for bad in (replace(SDXL, transformer_depth=(0, 2)), replace(SDXL, transformer_depth=(0, 2, 0)), replace(SDXL, transformer_depth=(0, -1, 2))):
        with pytest.raises(ValueError, match="transformer_depth"):
            UNetModel(bad)


def test_earlier_plans_are_the_parents_name_for_name(built):
    from tinyfusers_amd.storage.state import param_shapes
    from tinyfusers_amd.vision import unet as U
    with open(os.path.join(HERE, "golden", "unet_param_names.json")) as f:
        golden = json.load(f)
    assert sorted(golden) == ["SD15", "SD21", "TINY", "TINY_V2"]
    for name, want in golden.items():
        got = param_shapes(U.UNetModel(getattr(U, name)))
        assert list(got) == list(want), name                            # the same names in the same order ...
        assert {k: list(v) for k, v in got.items()} == want, name       # ... with the same shapes
        assert getattr(U.UNetModel(getattr(U, name)), "label_emb") is None
    assert [U.depth_at(U.SD15, lev) for lev in (0, 1, 2, 3, "mid")] == [1, 1, 1, 0, 1]


def test_sdxl_model_tree_names(built):
    from tinyfusers_amd.storage.state import param_shapes
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import SD15, SD21, SDXL
    sd = StableDiffusion(SDXL)
    ps = param_shapes(sd)
    e0, e1 = "conditioner.embedders.0.transformer.text_model.", "conditioner.embedders.1.model."
    assert ps[e0 + "embeddings.token_embedding.weight"] == (49408, 768) and ps[e0 + "encoder.layers.11.mlp.fc2.weight"] == (768, 3072)
    assert ps[e1 + "text_projection"] == (1280, 1280) and ps[e1 + "positional_embedding"] == (77, 1280) and ps[e1 + "ln_final.weight"] == (1280,)
    assert ps[e1 + "transformer.resblocks.31.attn.in_proj_weight"] == (3840, 1280) and ps[e1 + "transformer.resblocks.31.mlp.c_fc.weight"] == (5120, 1280)
    assert e1 + "transformer.resblocks.32.ln_1.weight" not in ps
    assert ps["first_stage_model.decoder.conv_in.weight"] == (512, 4, 3, 3) and ps["model.diffusion_model.label_emb.0.0.weight"] == (1280, 2816)
    assert sd.latent_scale == 0.13025 and StableDiffusion(SD15).latent_scale == 0.18215 and StableDiffusion(SD21).latent_scale == 0.18215
    assert not any(k.startswith("conditioner.") for k in param_shapes(StableDiffusion(SD15)))
    with pytest.raises(RuntimeError, match="no conditioner"):
        StableDiffusion(SD15).encode_prompt(np.zeros((1, 77), np.int64), np.zeros((1, 77), np.int64))


def _config(cfg_parallel=False, dtype="fp16"):
    return types.SimpleNamespace(cfg_parallel=cfg_parallel, dtype=dtype, parallel_branches=False, is_bf16=lambda: dtype == "bf16")


def test_compile_and_start_refusals(built):
    from tinyfusers_amd.variants import inputs as I
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY, TINY_XL, freeu_stages, pag_layers
    sch = S.DPMSolverPP2M().schedule(4)
    lat = types.SimpleNamespace(shape=(2, 4, 16, 16))
    ok = lambda **k: I.check_compile(k.pop("cin", 4), k.pop("net", False), k.pop("config", _config()), lat, k.pop("sampler", sch), k.pop("inpaint", False),
                                     k.pop("concat", None), k.pop("control", False), k.pop("cfg", True), adm=True, **k)
    # what SDXL runs
    ok(); ok(cfg=False); ok(inpaint=True); ok(prediction="v"); ok(cfg_rescale=True); ok(prediction="v", cfg_rescale=True, inpaint=True); ok(config=_config(dtype="bf16"))
    for name in ("DDIM", "DPMSolverPP2M", "EulerAncestral", "DPMSolverPP2SAncestral", "LCM"):
        if hasattr(S, name):
            ok(sampler=getattr(S, name)().schedule(4))
    # what it refuses, each by name
    U = S.UnsupportedSamplerConfig
    with pytest.raises(U, match="SDXL model needs a sampler schedule"):
        ok(sampler=None)
    with pytest.raises(U, match=r"control=True \(an SDXL ControlNet\) on an SDXL model is not supported"):
        ok(control=True, net=True)
    with pytest.raises(U, match=r"ip_adapter=True \(an SDXL IP-Adapter\) on an SDXL model is not supported"):
        ok(ip_adapter=True, has_ip_adapter=True, head_sizes=(64,))
    for concat, cin in (("inpaint", 9), ("edit", 8)):
        with pytest.raises(U, match=f"concat='{concat}' on an SDXL model is not supported"):
            ok(concat=concat, cin=cin)
    with pytest.raises(U, match="pag=True on an SDXL model is not supported"):
        ok(pag=True, pag_table=pag_layers(TINY_XL))
    with pytest.raises(U, match="freeu=True on an SDXL model is not supported"):
        ok(freeu=True, freeu_plan=freeu_stages(TINY_XL))
    with pytest.raises(U, match="SDXL model runs in the fp16 and the bf16 step, not under the fp8 policy"):
        ok(config=_config(dtype="fp8"))
    with pytest.raises(U, match=r"SDXL model has no two-chain CFG form \(TF_CFG_PARALLEL\)"):
        ok(config=_config(cfg_parallel=True))
    # start: no stream, no buffers -- a write would fail loudly, so these are refused before anything is written
    sd = StableDiffusion(TINY_XL)
    sd._sched, sd._adm = sch, True                          # as compile leaves them
    with pytest.raises(U, match="pooled="):
        sd.start(seed=1)
    with pytest.raises(U, match="pooled="):
        sd.start(seed=1, original_size=(512, 512))
    plain = StableDiffusion(TINY)
    plain._sched = sch
    for kw in (dict(pooled=np.zeros((2, 64), np.float32)), dict(uncond_pooled=np.zeros((2, 64), np.float32)), dict(original_size=(128, 128)),
               dict(crop_top_left=(0, 0)), dict(target_size=(128, 128)), dict(uncond_size_ids=np.zeros((1, 6)))):
        with pytest.raises(U, match=f"{next(iter(kw))}= needs a vector-conditioned UNet"):
            plain.start(seed=1, **kw)
    with pytest.raises(U, match="load_lora: LoRA adapters on an SDXL model are not supported"):
        StableDiffusion(TINY_XL).load_lora({})
    # the argument checks of start(pooled=, ...)
    assert I.adm_pooled(np.ones((1, 64)), 2, 64, "pooled").shape == (2, 64)
    for bad in (np.ones((2, 63)), np.ones((3, 64)), np.ones((64,)), np.full((2, 64), np.nan)):
        with pytest.raises(ValueError, match="pooled"):
            I.adm_pooled(bad, 2, 64, "pooled")
    ids = I.adm_size_ids(None, None, None, 2, 128, 96)
    assert ids.dtype == np.float32 and np.array_equal(ids, [[128, 96, 0, 0, 128, 96]] * 2)
    ids = I.adm_size_ids([(512, 256), (300, 200)], (8, 16), None, 2, 128, 128)
    assert np.array_equal(ids, [[512, 256, 8, 16, 128, 128], [300, 200, 8, 16, 128, 128]])
    for bad in (dict(original_size=(1, 2, 3)), dict(crop_top_left=[(0, 0)] * 3), dict(target_size=(-1, 5)), dict(original_size=(np.inf, 5))):
        with pytest.raises(ValueError):
            I.adm_size_ids(bad.get("original_size"), bad.get("crop_top_left"), bad.get("target_size"), 2, 128, 128)


def test_reference_vector_against_the_closed_form():
    # one id checked by hand: t = 1024 at dim 8 -> frequencies 10000^(-i/4) = 1, 0.1, 0.01, 0.001; angles 1024, 102.4, 10.24, 1.024
    e = X.fourier(1024.0, 8)
    ang = np.array([1024.0, 102.4, 10.24, 1.024])
    assert e.shape == (8,) and np.allclose(e, np.concatenate((np.cos(ang), np.sin(ang))), rtol=0, atol=1e-12)
    assert abs(e[3] - 0.5199533) < 1e-6 and abs(e[7] - 0.8541947) < 1e-6              # cos(1.024), sin(1.024) from a table
    assert np.array_equal(X.fourier(0.0, 32), np.concatenate((np.ones(16), np.zeros(16))))
    pooled = np.arange(10, dtype=np.float64).reshape(2, 5)
    ids = np.array([[1024, 512, 0, 0, 1024, 1024], [768, 4095.5, 8, 16, 512, 1]], np.float64)
    y = X.adm_vector(pooled, ids, 8)
    assert y.shape == (2, 5 + 6 * 8) and np.array_equal(y[:, :5], pooled)
    for r in range(2):
        for k in range(6):
            assert np.array_equal(y[r, 5 + 8 * k:5 + 8 * (k + 1)], X.fourier(ids[r, k], 8))
    assert np.allclose(y[0, 5:13], e, rtol=0, atol=0)                                   # the first id of image 0 is the hand-checked one
    from tinyfusers_amd.vision.unet import SDXL, TINY_XL
    assert SDXL.adm_in_channels == 1280 + 6 * SDXL.adm_time_dim == 2816 and TINY_XL.adm_in_channels == 64 + 6 * TINY_XL.adm_time_dim == 256


def test_pooled_index_rule(built):
    from tinyfusers_amd.vae.open_clip_text import pooled_rows
    ids = np.array([[49406, 320, 1125, 49407, 0, 0, 0],           # end of text in front of the padding
                    [49406, 49407, 0, 0, 0, 0, 0],                # the empty prompt
                    [49406, 5, 6, 7, 8, 9, 49407],                # end of text in the last place
                    [49406, 9, 49407, 49407, 49407, 49407, 49407]])       # padded WITH the end-of-text id: the first one counts
    assert np.array_equal(X.pooled_index(ids), [3, 1, 6, 2])
    rows = pooled_rows(ids)
    assert rows.dtype == np.int32 and np.array_equal(rows, np.arange(4) * 7 + np.array([3, 1, 6, 2]))
    for bad in (ids[0], ids.astype(np.float32)):
        with pytest.raises(ValueError, match="integer token ids"):
            pooled_rows(bad)
