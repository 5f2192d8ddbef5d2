"""The CLIP vision tower's host side (no GPU): the reader on a ``.safetensors`` and a nested ``.bin`` the test writes, the configuration derived
from the shapes, every refusal (text keys, token count, unknown head count, missing / surplus / mis-shaped key), the packed patch weight against
the conv weight, the attention instance the launcher picks for the tower's shape, and start()'s argument checks for ``ip_image=``."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "aux"))

import clip_vision_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def built():
    import __graft_entry__
    __graft_entry__.build()


def test_param_shapes_and_config_agree_with_the_restatement(built):
    from tinyfusers_amd.vae import clip_vision as V
    assert V.VIT_H == V.ClipVisionConfig() and V.VIT_H.tokens == 257 and V.VIT_H.kpad == 592
    assert V.param_shapes(V.VIT_H) == R.vision_param_shapes(R.VIT_H)
    tiny = V.ClipVisionConfig(**R.TINY)
    assert V.param_shapes(tiny) == R.vision_param_shapes(R.TINY) and tiny.tokens == 17
    assert (V.CLIP_MEAN, V.CLIP_STD) == (R.CLIP_MEAN, R.CLIP_STD)
    scale, shift = V.norm_constants()
    assert scale.dtype == shift.dtype == np.float32
    np.testing.assert_allclose(scale.astype(np.float64) * 255.0 * np.float64(R.CLIP_STD), 1.0, rtol=1e-7)
    np.testing.assert_allclose(shift.astype(np.float64) * np.float64(R.CLIP_STD), -np.float64(R.CLIP_MEAN), rtol=1e-7)
    # the attribute tree spells the file's names: what update_state walks is param_shapes minus the class embedding (installed by load)
    from tinyfusers_amd.storage.state import _slots
    names = {n for n, *_ in _slots(V.ClipVision(tiny))}
    assert names - {"visual_projection.bias"} == set(R.vision_param_shapes(R.TINY)) - {"vision_model.embeddings.class_embedding"}


def test_reader_round_trips_and_derives_the_configuration(built, tmp_path):
    from tinyfusers_amd.storage.unpicker import save_safetensors
    from tinyfusers_amd.vae import clip_vision as V
    W = R.make_weights(R.TINY)
    flat, nested = str(tmp_path / "vit.safetensors"), str(tmp_path / "vit.bin")
    save_safetensors(flat, W)
    with_ids = {k: torch.from_numpy(v.copy()) for k, v in W.items()}
    with_ids["vision_model.embeddings.position_ids"] = torch.arange(17)[None]
    torch.save({"state_dict": with_ids}, nested)
    for src in (flat, nested, W, {"state_dict": with_ids}):
        got = V.load_state(src)
        assert set(got) == set(W)                                # (position_ids is dropped)
        for k in W:
            assert got[k].dtype == np.float16 and np.array_equal(got[k], W[k]), k
        cfg = V.config_from_state(got, heads=4)
        assert cfg == V.ClipVisionConfig(**R.TINY)
        V.check_state(got, cfg)
    with pytest.raises(TypeError):
        V.load_state(3)
    bf = V.load_state({k: torch.from_numpy(v.copy()).to(torch.bfloat16) for k, v in W.items()})      # a bfloat16 .bin: through float32, exactly
    k = "visual_projection.weight"
    assert bf[k].dtype == np.float32 and np.array_equal(bf[k], torch.from_numpy(W[k].copy()).to(torch.bfloat16).float().numpy())
    H = {k: np.zeros(s, np.float16) for k, s in R.vision_param_shapes(dict(R.VIT_H, layers=1)).items()}
    assert V.config_from_state(H) == V.ClipVisionConfig(layers=1)                    # width 1280: heads = 16 without being told


def test_every_refusal_names_its_reason(built):
    from tinyfusers_amd.vae import clip_vision as V
    W = R.make_weights(R.TINY)
    cfg = V.ClipVisionConfig(**R.TINY)
    with pytest.raises(ValueError, match=r"text tower \(text_model\.embeddings"):
        V.load_state(dict(W, **{"text_model.embeddings.token_embedding.weight": np.zeros((8, 8), np.float16)}))
    with pytest.raises(ValueError, match="head count is not in the file"):
        V.config_from_state(W)
    with pytest.raises(ValueError, match="heads=3 does not divide"):
        V.config_from_state(W, heads=3)
    bad = dict(W); bad["vision_model.embeddings.position_embedding.weight"] = np.zeros((18, 320), np.float16)
    with pytest.raises(ValueError, match=r"position_embedding\.weight has shape \(18, 320\).*token count"):
        V.config_from_state(bad, heads=4)
    bad = dict(W); del bad["vision_model.encoder.layers.1.self_attn.k_proj.bias"]
    with pytest.raises(ValueError, match=r"lacks vision_model\.encoder\.layers\.1\.self_attn\.k_proj\.bias"):
        V.check_state(bad, cfg)
    bad = dict(W); del bad["visual_projection.weight"]
    with pytest.raises(ValueError, match=r"lacks visual_projection\.weight"):
        V.config_from_state(bad, heads=4)
    bad = dict(W); bad["vision_model.encoder.layers.0.mlp.fc2.weight"] = np.zeros((320, 640), np.float16)
    with pytest.raises(ValueError, match=r"mlp\.fc2\.weight has shape \(320, 640\).*\(320, 1280\)"):
        V.check_state(bad, cfg)
    bad = dict(W); bad["vision_model.encoder.layers.2.layer_norm1.weight"] = np.zeros(320, np.float16)
    with pytest.raises(ValueError, match=r"no place for.*layers\.2\.layer_norm1"):
        V.check_state(bad, cfg)
    bad = dict(W); bad["vision_model.embeddings.patch_embedding.weight"] = np.zeros((320, 4, 14, 14), np.float16)
    with pytest.raises(ValueError, match=r"patch_embedding\.weight has shape \(320, 4, 14, 14\)"):
        V.config_from_state(bad, heads=4)
    with pytest.raises(ValueError, match="unsupported configuration"):
        V.ClipVision(V.ClipVisionConfig(image=60))


def test_packed_patch_weight_is_the_conv_weight_under_ky_kx_c(built):
    from tinyfusers_amd.vae.clip_vision import pack_patch_weight
    rng = np.random.default_rng(0)
    w = rng.standard_normal((5, 3, 14, 14)).astype(np.float16)
    p = pack_patch_weight(w, 592)
    assert p.shape == (5, 592) and p.dtype == np.float32 and not p[:, 588:].any()
    for ky, kx, c in ((0, 0, 0), (0, 0, 2), (0, 13, 1), (1, 0, 0), (13, 13, 2), (7, 3, 1)):
        assert np.array_equal(p[:, ky * 42 + kx * 3 + c], w[:, c, ky, kx].astype(np.float32)), (ky, kx, c)
    assert np.array_equal(np.sort(p[:, :588], axis=1), np.sort(w.reshape(5, -1).astype(np.float32), axis=1))     # a permutation: nothing lost
    # the contract is the product: patches (same column order) . packed^T == the strided convolution of the restatement
    img = rng.integers(0, 256, (2, 28, 28, 3), dtype=np.uint8)
    x = R.normalise(img).numpy()                                                       # (N, 3, S, S) float64
    patches = x.reshape(2, 3, 2, 14, 2, 14).transpose(0, 2, 4, 3, 5, 1).reshape(8, 588)   # rows (b, py, px), columns (ky, kx, c)
    want = R.patch_embed(img, {"vision_model.embeddings.patch_embedding.weight": w}, dict(patch=14)).numpy().reshape(8, 5)
    np.testing.assert_allclose(patches @ p[:, :588].astype(np.float64).T, want, rtol=0, atol=1e-9)
    with pytest.raises(AssertionError):
        pack_patch_weight(w, 584)


def test_the_towers_attention_runs_the_in_block_split_form(built):
    from tinyfusers_amd.native import lib
    split = 5                                                    # TF_SDPA_INST_SPLIT
    for dtype in (0, 1):
        for b in (1, 2):
            assert lib.tf_sdpa_instance(dtype, b, 16, 257, 257, 80, 3 * 1280, 3 * 1280, 0) == split, (dtype, b)


def test_kernel_entries_refuse_bad_arguments_on_the_host(built):
    """Before the device is touched: TF_E_ARG with a message naming the entry (placeholder pointers are never dereferenced)."""
    from tinyfusers_amd.native import lib
    P, E = ctypes.c_void_p(4096), 10001
    f3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    nan3 = (ctypes.c_float * 3)(1.0, float("nan"), 1.0)

    def refused(rc, who):
        assert rc == E and lib.tf_last_error().decode().startswith(who), (rc, lib.tf_last_error())
    q = lib.tf_vit_patchify_u8_16
    for args in ((2, P, P, 1, 28, 14, 592, f3, f3), (0, None, P, 1, 28, 14, 592, f3, f3), (0, P, None, 1, 28, 14, 592, f3, f3), (0, P, P, 1, 30, 14, 592, f3, f3),
                 (0, P, P, 1, 28, 14, 588, f3, f3), (0, P, P, 1, 28, 14, 584, f3, f3), (0, P, P, -1, 28, 14, 592, f3, f3), (0, P, P, 1, 28, 0, 592, f3, f3),
                 (0, P, P, 1, 28, 14, 592, None, f3), (0, P, P, 1, 28, 14, 592, f3, nan3), (0, ctypes.c_void_p(4104), P, 1, 28, 14, 592, f3, f3)):
        refused(q(*args, None), "tf_vit_patchify_u8_16")
    q = lib.tf_vit_embed_ln_16
    for args in ((3, P, P, P, P, P, P, 1, 17, 320, 1e-5), (0, None, P, P, P, P, P, 1, 17, 320, 1e-5), (0, P, None, P, P, P, P, 1, 17, 320, 1e-5),
                 (0, P, P, P, P, None, P, 1, 17, 320, 1e-5), (0, P, P, P, P, P, P, 1, 0, 320, 1e-5), (0, P, P, P, P, P, P, 1, 17, 324, 1e-5),
                 (0, P, P, P, P, P, P, 1, 17, 2568, 1e-5), (0, P, P, P, P, P, P, 1, 17, 320, 0.0), (0, P, P, P, ctypes.c_void_p(4098), P, P, 1, 17, 320, 1e-5)):
        refused(q(*args, None), "tf_vit_embed_ln_16")
    q = lib.tf_gelu_erf_16
    for args in ((5, P, P, 8), (0, None, P, 8), (0, P, None, 8), (0, P, P, -1), (1, P, ctypes.c_void_p(4098), 8)):
        refused(q(*args, None), "tf_gelu_erf_16")
    assert q(0, P, P, 0, None) == 0 and lib.tf_vit_patchify_u8_16(0, P, P, 0, 28, 14, 592, f3, f3, None) == 0      # nothing to do: no launch


def test_start_checks_ip_image_before_anything_is_written(built):
    from tinyfusers_amd.variants.samplers import UnsupportedSamplerConfig
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vae.clip_vision import ClipVision, ClipVisionConfig
    tower = types.SimpleNamespace(cfg=ClipVisionConfig(**R.TINY), dtype=np.dtype(np.float16))
    adapter = types.SimpleNamespace(embed_dim=32, paths=[(1, "a"), (3, "b")])

    def check(tower_=tower, adapter_=adapter, **kw):
        me = types.SimpleNamespace(_ip=True, _ip_model_compiled=adapter_, _latent=types.SimpleNamespace(shape=(2, 4, 16, 16)), _clip_vision=tower_,
                                   _check_tower_fits=StableDiffusion._check_tower_fits)
        return StableDiffusion._check_ip(me, kw.get("ip_image_embeds"), kw.get("ip_image"), kw.get("ip_scale"))
    img = np.zeros((2, 56, 56, 3), np.uint8)
    got, scales = check(ip_image=img)
    assert got.dtype == np.uint8 and got.shape == img.shape and scales.shape == (4,)
    assert check(ip_image=img[:1])[0].shape == (1, 56, 56, 3)                       # one image for every latent
    with pytest.raises(ValueError, match="not both"):
        check(ip_image=img, ip_image_embeds=np.zeros((2, 32), np.float32))
    for bad in (img.astype(np.float32), img[:, :28], np.zeros((3, 56, 56, 3), np.uint8), img[..., :2], img[0]):
        with pytest.raises(ValueError, match=r"ip_image must be uint8 \(2, 56, 56, 3\)"):
            check(ip_image=bad)
    with pytest.raises(UnsupportedSamplerConfig, match="CLIP vision tower"):
        check(tower_=None, ip_image=img)
    with pytest.raises(ValueError, match="projects to 32 values.*reads 1024"):
        check(adapter_=types.SimpleNamespace(embed_dim=1024, paths=[]), ip_image=img)
    with pytest.raises(ValueError, match="pass ip_image_embeds= or ip_image="):
        check()
    # attach_clip_vision: the type and, with an adapter attached, the widths (the message names both numbers)
    sd = types.SimpleNamespace(_ip_model=types.SimpleNamespace(embed_dim=1024), _clip_vision=None, _check_tower_fits=StableDiffusion._check_tower_fits)
    with pytest.raises(TypeError, match="ClipVision"):
        StableDiffusion.attach_clip_vision(sd, object())
    with pytest.raises(ValueError, match="32 values.*1024"):
        StableDiffusion.attach_clip_vision(sd, ClipVision(ClipVisionConfig(**R.TINY)))
    sd._ip_model = None
    assert StableDiffusion.attach_clip_vision(sd, ClipVision(ClipVisionConfig(**R.TINY))) is sd and sd._clip_vision is not None
