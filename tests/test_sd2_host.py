"""Host checks of the SD-2.x path: the head plan of UNetConfig.d_head, the checkpoint names of the OpenCLIP text tower, the compile / start
refusals of prediction= and cfg_rescale=, the tokenizer's pad id, and the float64 tail restatement of tests/aux/sd2_ref.py against closed forms."""
import json
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "aux"))

import sd2_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def built():
    import __graft_entry__
    __graft_entry__.build()


def test_head_plan(built):
    from dataclasses import replace
    from tinyfusers_amd.attention.attention import SpatialTransformer
    from tinyfusers_amd.storage.state import param_shapes
    from tinyfusers_amd.vision.controlnet import ControlNet
    from tinyfusers_amd.vision.unet import SD15, SD21, SD21_INPAINT, TINY, TINY_V2, UNetModel, head_sizes, heads_at

    def plan(cfg):
        u = UNetModel(cfg)
        return [(a.num_heads, a.head_size) for st in u._all(SpatialTransformer) for a in (st.transformer_blocks[0].attn1, st.transformer_blocks[0].attn2)]
    want21 = [(5, 64)] * 4 + [(10, 64)] * 4 + [(20, 64)] * 4 + [(20, 64)] * 2 + [(20, 64)] * 6 + [(10, 64)] * 6 + [(5, 64)] * 6
    assert plan(SD21) == want21 and plan(SD21_INPAINT) == want21
    assert plan(TINY_V2) == [(1, 64)] * 4 + [(2, 64)] * 4 + [(2, 64)] * 2 + [(2, 64)] * 6 + [(1, 64)] * 6
    assert plan(SD15) == [(8, 40)] * 4 + [(8, 80)] * 4 + [(8, 160)] * 4 + [(8, 160)] * 2 + [(8, 160)] * 6 + [(8, 80)] * 6 + [(8, 40)] * 6
    assert set(plan(TINY)) == {(2, 32), (2, 64)}
    assert SD21.in_channels == 4 and SD21_INPAINT.in_channels == 9 and SD21.context_dim == 1024 and SD15.d_head is None and TINY.d_head is None
    assert head_sizes(SD21) == [64] and head_sizes(SD15) == [40, 80, 160] and heads_at(SD21, 1280) == (20, 64) and heads_at(SD15, 1280) == (8, 160)
    ps = param_shapes(UNetModel(SD21))
    assert ps["input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight"] == (320, 1024)
    assert ps["middle_block.1.transformer_blocks.0.attn2.to_v.weight"] == (1280, 1024) and ps["input_blocks.1.1.proj_in.weight"] == (320, 320, 1, 1)
    assert set(ps) == set(param_shapes(UNetModel(replace(SD15, context_dim=1024))))          # the same tensors: only the head split differs
    cn = ControlNet(cfg=SD21)                                                                 # follows from encoder_plan
    assert {(a.num_heads, a.head_size) for st in cn._all(SpatialTransformer) for a in (st.transformer_blocks[0].attn1,)} == {(5, 64), (10, 64), (20, 64)}
    for bad in (replace(SD21, d_head=48), replace(TINY_V2, d_head=128), replace(SD21, d_head=0)):
        with pytest.raises(ValueError, match="d_head"):
            UNetModel(bad)


def test_open_clip_names_and_the_in_proj_split(built):
    from tinyfusers_amd.storage.state import param_shapes
    from tinyfusers_amd.vae import open_clip_text as O
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import SD15, SD21, SD21_INPAINT
    for cfg in (SD21, SD21_INPAINT):
        sd = StableDiffusion(cfg)
        ps = param_shapes(sd)
        pre = "cond_stage_model.model."
        assert ps[pre + "token_embedding.weight"] == (49408, 1024) and ps[pre + "positional_embedding"] == (77, 1024)
        assert ps[pre + "ln_final.weight"] == ps[pre + "ln_final.bias"] == (1024,)
        for n in range(23):                                                                    # the penultimate layer's output: 23 of the 24 resblocks have a slot
            b = f"{pre}transformer.resblocks.{n}."
            assert ps[b + "attn.in_proj_weight"] == (3072, 1024) and ps[b + "attn.in_proj_bias"] == (3072,)
            assert ps[b + "attn.out_proj.weight"] == (1024, 1024) and ps[b + "attn.out_proj.bias"] == (1024,)
            assert ps[b + "mlp.c_fc.weight"] == (4096, 1024) and ps[b + "mlp.c_fc.bias"] == (4096,)
            assert ps[b + "mlp.c_proj.weight"] == (1024, 4096) and ps[b + "mlp.c_proj.bias"] == (1024,)
            for ln in ("ln_1", "ln_2"):
                assert ps[b + ln + ".weight"] == ps[b + ln + ".bias"] == (1024,)
        text = [k for k in ps if k.startswith("cond_stage_model.")]
        assert len(text) == 4 + 23 * 12 and not any("resblocks.23." in k or "text_projection" in k or "q_proj" in k for k in text)
        assert any(k.startswith("first_stage_model.decoder.") for k in ps) and any(k.startswith("first_stage_model.encoder.") for k in ps)
    assert not any(k.startswith("cond_stage_model.model.") for k in param_shapes(StableDiffusion(SD15)))
    # the fused in_proj is q | k | v by rows: the reference's renamer on a tiny configuration, against the synthetic state's own rows
    cfg = O.OpenClipTextConfig(width=128, layers=3, heads=2, mlp=512)
    assert set(O.param_shapes(cfg)) == {k[len("cond_stage_model.model."):] for k in param_shapes(types.SimpleNamespace(cond_stage_model=O.OpenClipText(cfg)))}
    st = O.synthetic_state(cfg, 3)
    assert "transformer.resblocks.2.attn.in_proj_weight" in st and "transformer.resblocks.2.attn.in_proj_weight" not in O.param_shapes(cfg)
    hf = R.ldm_to_hf(st, 2)
    w, b = st["transformer.resblocks.1.attn.in_proj_weight"], st["transformer.resblocks.1.attn.in_proj_bias"]
    for k, name in enumerate(("q_proj", "k_proj", "v_proj")):
        assert np.array_equal(hf[f"encoder.layers.1.self_attn.{name}.weight"], w[128 * k:128 * (k + 1)]) and hf[f"encoder.layers.1.self_attn.{name}.weight"].shape == (128, 128)
        assert np.array_equal(hf[f"encoder.layers.1.self_attn.{name}.bias"], b[128 * k:128 * (k + 1)])
    assert O.config_from_state(st, heads=2) == cfg and O.config_from_state(O.load_state({"cond_stage_model.model." + k: v for k, v in st.items()}), 2) == cfg
    with pytest.raises(ValueError, match="lacks"):
        O.config_from_state({k: v for k, v in st.items() if k != "positional_embedding"})


def _config(cfg_parallel=False, dtype="fp16"):
    return types.SimpleNamespace(cfg_parallel=cfg_parallel, dtype=dtype, parallel_branches=False, is_bf16=lambda: dtype == "bf16")


def test_compile_refusals_and_the_phi_range(built):
    from tinyfusers_amd.variants import inputs as I
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import SD15, SD21, TINY_V2, head_sizes, pag_layers
    sch = S.DPMSolverPP2M().schedule(4)
    lat = types.SimpleNamespace(shape=(2, 4, 16, 16))
    ok = lambda **k: I.check_compile(k.pop("cin", 4), k.pop("net", False), k.pop("config", _config()), lat, k.pop("sampler", sch), k.pop("inpaint", False),
                                     k.pop("concat", None), k.pop("control", False), k.pop("cfg", True), **k)
    # what combines
    ok(prediction="v"); ok(prediction="v", cfg=False); ok(prediction="v", inpaint=True); ok(prediction="v", concat="inpaint", cin=9); ok(prediction="v", concat="edit", cin=8)
    ok(prediction="v", control=True, net=True); ok(prediction="v", pag=True, pag_table=pag_layers(TINY_V2)); ok(prediction="v", config=_config(dtype="bf16"))
    ok(cfg_rescale=True); ok(cfg_rescale=True, prediction="v"); ok(cfg_rescale=True, cfg=False, pag=True, pag_table=pag_layers(TINY_V2)); ok(cfg_rescale=True, inpaint=True)
    ok(cfg_rescale=True, pag=True, pag_table=pag_layers(SD21))
    # what is refused, each with its reason
    with pytest.raises(ValueError, match="prediction= takes 'eps' or 'v'"):
        ok(prediction="x0")
    for kw, word in ((dict(prediction="v"), "prediction='v'"), (dict(cfg_rescale=True), "cfg_rescale=True")):
        with pytest.raises(ValueError, match=word + " needs a sampler schedule"):
            ok(sampler=None, **kw)
        with pytest.raises(S.UnsupportedSamplerConfig, match="TF_CFG_PARALLEL"):
            ok(config=_config(cfg_parallel=True), **kw)
    with pytest.raises(ValueError, match="cfg_rescale=True and concat='edit'"):
        ok(cfg_rescale=True, concat="edit", cin=8)
    with pytest.raises(ValueError, match="cfg_rescale=True needs a guidance pair or triple"):
        ok(cfg_rescale=True, cfg=False)
    with pytest.raises(S.UnsupportedSamplerConfig, match="head size 64.*40, 80, 160"):
        ok(ip_adapter=True, has_ip_adapter=True, head_sizes=head_sizes(SD21))
    ok(ip_adapter=True, has_ip_adapter=True, head_sizes=head_sizes(SD15))
    # phi: checked before anything is written -- on this machine nothing CAN be written, so a check that came late would raise something else
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "much", None):
        with pytest.raises(ValueError, match=r"phi is a float in \[0, 1\]"):
            I.cfg_rescale_phi(bad)
    assert I.cfg_rescale_phi(0) == 0.0 and I.cfg_rescale_phi(1) == 1.0 and I.cfg_rescale_phi(np.float32(0.5)) == 0.5
    sd = StableDiffusion(TINY_V2)
    sd._sched, sd._rescale = sch, True                     # as compile(..., cfg_rescale=True) leaves them; no stream, no buffers: a write would fail loudly
    for call in (lambda: sd.set_cfg_rescale(1.5), lambda: sd.start(seed=1, cfg_rescale=-0.5), lambda: sd.start(seed=1, cfg_rescale=float("nan"))):
        with pytest.raises(ValueError, match=r"phi is a float in \[0, 1\]"):
            call()
    sd._rescale = False
    for call in (lambda: sd.set_cfg_rescale(0.5), lambda: sd.start(seed=1, cfg_rescale=0.5)):
        with pytest.raises(ValueError, match="compiled with cfg_rescale=True"):
            call()
    assert StableDiffusion(TINY_V2)._rescale_phi is None and StableDiffusion(TINY_V2)._vpred is False       # declared in _reset_state
    with pytest.raises(S.UnsupportedSamplerConfig):
        StableDiffusion(TINY_V2).set_cfg_rescale(0.5)                                                        # never compiled


def test_tokenizer_pad_id(built):
    from tinyfusers_amd.tokenizer.clip import ClipTokenizer
    G = os.path.join(HERE, "golden")
    tok = ClipTokenizer(os.path.join(G, "clip_bpe_toy.txt.gz"))
    g = json.load(open(os.path.join(G, "clip_tokens.json")))
    for text, want in zip(g["texts"], g["ids"]):
        assert tok.encode(text) == tok.encode(text, pad_id=None) == want
        n = want.index(49407)                                 # the first end-of-text token
        got = tok.encode(text, pad_id=0)
        assert len(got) == 77 and got[:n + 1] == want[:n + 1] and got[n + 1:] == [0] * (76 - n), text
    full = tok.encode(" ".join(["cat"] * 200), pad_id=0)
    assert len(full) == 77 and full[-1] == 49407 and 0 not in full
    assert tok.encode("", pad_id=0) == [49406, 49407] + [0] * 75


def test_float64_tail_against_closed_forms():
    rng = np.random.default_rng(11)
    B, C, H, W = 2, 4, 6, 5
    x, h = rng.standard_normal((2, B, C, H, W))
    a_t, a_s, row = 0.37, 0.52, (0.3, 0.6, 0.25, 0.0)
    # v-prediction with phi irrelevant: x0 = sqrt(a) x - sqrt(1 - a) v; with v = sqrt(a) eps - sqrt(1 - a) x0* and x = sqrt(a) x0* + sqrt(1 - a) eps it is x0*
    x0s, eps = rng.standard_normal((2, B, C, H, W))
    a = np.float64(np.float32(a_t))
    xt, v = np.sqrt(a) * x0s + np.sqrt(1 - a) * eps, np.sqrt(a) * eps - np.sqrt(1 - a) * x0s
    r = R.tail(xt, [v], h, a_t, a_s, 1.0, row, vpred=True)
    assert np.allclose(r["x0"], x0s, rtol=0, atol=1e-14) and np.all(r["f"] == 1)
    assert np.allclose(r["latent"], row[0] * xt + row[1] * x0s + np.float64(np.float32(row[2])) * h - (np.float64(np.float32(row[0])) - row[0]) * xt, rtol=0, atol=1e-6)
    re = R.tail(xt, [eps], h, a_t, a_s, 1.0, row)
    assert np.allclose(re["x0"], x0s, rtol=0, atol=1e-13)                                       # the eps form lands on the same x0
    pair = R.tail(xt, [v, v], h, a_t, a_s, 7.5, row, vpred=True, phi=0.7)                       # e_u == e_c: e = e_t, f = 1 whatever phi
    assert np.allclose(pair["f"], 1.0, rtol=1e-14) and np.allclose(pair["x0"], x0s, rtol=0, atol=1e-13)
    # the planted rescale case: e_u = 0, e_t = +-1 in equal numbers, g = 2, phi = 1: e = 2 e_t, f = 1/2, e' = e_t exactly
    et = np.ones((B, C * H * W)); et[:, ::2] = -1.0
    et = et.reshape(B, C, H, W)
    p = R.tail(x, [np.zeros_like(et), et], h, a_t, a_s, 2.0, row, phi=1.0)
    assert np.array_equal(p["f"].reshape(-1), [0.5, 0.5]) and np.array_equal(p["e"], et)
    one = R.tail(x, [et], h, a_t, a_s, 1.0, row)
    assert np.array_equal(p["latent"], one["latent"]) and np.array_equal(p["x0"], one["x0"])
    half = R.tail(x, [np.zeros_like(et), et], h, a_t, a_s, 2.0, row, phi=0.5)
    assert np.array_equal(half["e"], 1.5 * et)                                                  # phi (e f) + (1 - phi) e = 0.5 e_t + 0.5 (2 e_t)
    zero = R.tail(x, [np.zeros_like(et), et], h, a_t, a_s, 2.0, row, phi=0.0)
    plain = R.tail(x, [np.zeros_like(et), et], h, a_t, a_s, 2.0, row)
    assert np.array_equal(zero["latent"], plain["latent"])
    # three groups: the text group is the last one
    e0, e1 = rng.standard_normal((2, B, C, H, W))
    t3 = R.tail(x, [e0, e1, et], h, a_t, a_s, 10.5, row, g_i=7.5, phi=1.0)
    e = e0 + 10.5 * (et - e1) + 7.5 * (e1 - e0)
    assert np.allclose(t3["f"].reshape(-1), et.reshape(B, -1).std(1) / e.reshape(B, -1).std(1), rtol=1e-13)
    assert np.allclose(t3["e"].reshape(B, -1).std(1), 1.0, rtol=1e-13)                          # phi = 1: the rescaled output has the text group's deviation
    # std(e) == 0 -> f = 1, nothing non-finite
    c = R.tail(x, [np.full_like(et, 0.25), np.full_like(et, -0.5)], h, a_t, a_s, 7.5, row, phi=0.7)
    assert np.all(c["f"] == 1) and np.isfinite(c["latent"]).all() and np.all(c["e"] == 0.25 + 7.5 * (-0.75))
    # the masked blend: mask 1 keeps the update, mask 0 the noised known region
    m = np.zeros((B, 1, H, W)); m[0] = 1.0
    x0i, z2 = rng.standard_normal((2, B, C, H, W))
    mk = R.tail(x, [e0, et], h, a_t, a_s, 7.5, row, phi=0.7, vpred=True, x0_init=x0i, mask=m, z2=z2)
    un = R.tail(x, [e0, et], h, a_t, a_s, 7.5, row, phi=0.7, vpred=True)
    a2 = np.float64(np.float32(a_s))
    assert np.array_equal(mk["latent"][0], un["latent"][0]) and np.array_equal(mk["latent"][1], (np.sqrt(a2) * x0i + np.sqrt(1 - a2) * z2)[1])
