"""Host checks of the AnimateDiff motion modules (vision/motion.py): the loader (both spellings, the sinusoid, mid_block, every refusal names its
tensor), the slot plan against the committed name list, properties of the float64 restatement (tests/aux/motion_ref.py) itself, and the
sensitivity conditions that make the GPU gates of tests/test_gpu_motion.py mean something: on the inputs those tests use the restatement moves by
>= 10 x the gate when the positional tables are zeroed, the two attentions' weights are swapped, the head count is the UNet's where it must be 8, or
the GroupNorm eps is 1e-5 where it must be 1e-6.  No device."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))
import motion_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motion_slots.json")
T = R.T


def _gate_units(a, ref):
    """The largest |a - ref| in units of the module gate atol + rtol |ref|."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(a - ref) / (R.ATOL + R.RTOL * np.abs(ref))))


@functools.lru_cache(maxsize=None)
def _case(C, F, V, h, w, max_len):
    W, x = R.module_weights(C, max_len), R.module_input(C, F, V, h, w)
    return W, x, R.motion_module_forward(x, W, F).numpy()


def _tiny_file(**kw):
    from tinyfusers_amd.storage.synth import synth_motion_state_dict
    from tinyfusers_amd.vision.unet import TINY
    return synth_motion_state_dict(TINY, 3, **kw)


# ---- the slot plan ----------------------------------------------------------------------------------------------------------------------------------
def test_slot_plan_matches_the_committed_name_list():
    from tinyfusers_amd.vision.motion import motion_slots
    from tinyfusers_amd.vision.unet import SD15, TINY
    gold = json.load(open(GOLDEN))
    for name, cfg, mid in (("SD15", SD15, False), ("SD15_mid", SD15, True), ("TINY", TINY, False), ("TINY_mid", TINY, True)):
        got = [[p, s] for p, s, _ in motion_slots(cfg, mid)]
        assert got == gold[name], name
    sd = motion_slots(SD15)
    assert sum(p.startswith("down_blocks.") for p, _, _ in sd) == 8 and sum(p.startswith("up_blocks.") for p, _, _ in sd) == 12 and len(motion_slots(SD15, True)) == 21
    assert [c for _, _, c in sd] == [320, 320, 640, 640, 1280, 1280, 1280, 1280] + [1280] * 3 + [1280] * 3 + [640] * 3 + [320] * 3
    ty = motion_slots(TINY, True)
    assert len(ty) == 6 + 1 + 9 and [c for _, _, c in ty] == [64, 64, 128, 128, 128, 128, 128] + [128] * 3 + [128] * 3 + [64] * 3
    import oracle
    assert [list(r) for r in R.slot_names(oracle.SD15)] == gold["SD15"]          # (the restatement's own plan: the same list)


def test_unet_walk_places_the_modules_at_their_slots():
    from tinyfusers_amd.attention.attention import SpatialTransformer
    from tinyfusers_amd.vision.motion import MotionAdapter, MotionModule
    from tinyfusers_amd.vision.resnet import ResBlock
    from tinyfusers_amd.vision.unet import TINY, UNetModel, Upsample
    unet, ad = UNetModel(TINY), MotionAdapter(TINY, 24, mid=True)
    inp, mid, out = unet._with_motion(ad)
    kinds = lambda b: [type(m).__name__ for m in b]
    assert kinds(inp[0]) == ["Conv2d"] and kinds(inp[1]) == ["ResBlock", "SpatialTransformer", "MotionModule"] and kinds(inp[3]) == ["Downsample"]
    assert kinds(inp[7]) == ["ResBlock", "MotionModule"] and kinds(mid) == ["ResBlock", "SpatialTransformer", "MotionModule", "ResBlock"]
    assert kinds(out[2]) == ["ResBlock", "MotionModule", "Upsample"] and kinds(out[5]) == ["ResBlock", "SpatialTransformer", "MotionModule", "Upsample"]
    assert kinds(out[8]) == ["ResBlock", "SpatialTransformer", "MotionModule"]
    assert sum(isinstance(m, MotionModule) for b in inp + [mid] + out for m in b) == 16
    assert [len(b) for b in unet.input_blocks] == [1, 2, 2, 1, 2, 2, 1, 1, 1] and len(unet.middle_block) == 3       # the model's own lists are untouched
    assert inp[1][2] is ad.modules["input_blocks.1"] and out[8][2] is ad.modules["output_blocks.8"] and inp[1][2].channels == 64 and out[0][1].channels == 128
    assert not any(isinstance(m, (SpatialTransformer, ResBlock, Upsample)) for m in ad.module_list())
    from dataclasses import replace
    with pytest.raises(ValueError, match="was built for"):
        UNetModel(replace(TINY, context_dim=32))._with_motion(ad)


# ---- the loader (host part: parse_motion_state checks everything before anything is uploaded) ---------------------------------------------------------
def test_both_spellings_parse_to_the_same_modules_and_mid_block_follows_the_file():
    from tinyfusers_amd.vision.motion import parse_motion_state
    from tinyfusers_amd.vision.unet import TINY
    for mid in (False, True):
        W = _tiny_file(max_len=24, mid=mid)
        assert all(".temporal_transformer." in k for k in W) and any(k.endswith("attention_blocks.1.pos_encoder.pe") for k in W)
        a = parse_motion_state(TINY, W)
        b = parse_motion_state(TINY, R.to_diffusers(W))
        assert any(".attn2.pos_embed.pe" in k for k in R.to_diffusers(W)) and not any("temporal_transformer" in k for k in R.to_diffusers(W))
        assert a[0] == b[0] == 24 and a[1] is b[1] is mid and ("mid_block.motion_modules.0" in a[2]) is mid and len(a[2]) == 15 + mid
        assert a[2].keys() == b[2].keys()
        for p in a[2]:
            assert a[2][p].keys() == b[2][p].keys() and len(a[2][p]) == 28
            for k in a[2][p]:
                assert np.array_equal(a[2][p][k], b[2][p][k]), (p, k)
        mods = R.split_modules(W)
        for p in mods:
            for k, v in mods[p].items():
                assert np.array_equal(a[2][p][k], v), (p, k)


def test_a_file_without_pe_gets_the_sinusoid():
    from tinyfusers_amd.vision.motion import MAX_FRAMES, parse_motion_state, sinusoid_pe
    from tinyfusers_amd.vision.unet import TINY
    max_len, mid, mods = parse_motion_state(TINY, _tiny_file(pe=False))
    assert max_len == MAX_FRAMES == 32 and not mid
    for p, m in mods.items():
        c = m["norm.weight"].shape[0]
        pos = np.arange(32, dtype=np.float64)[:, None]
        div = np.exp(-np.log(1e4) * np.arange(0, c, 2) / c)
        for i in (0, 1):
            pe = m[f"{T}attention_blocks.{i}.pos_encoder.pe"]
            assert pe.shape == (1, 32, c)
            np.testing.assert_allclose(pe[0, :, 0::2], np.sin(pos * div), atol=1e-6)
            np.testing.assert_allclose(pe[0, :, 1::2], np.cos(pos * div), atol=1e-6)
    assert sinusoid_pe(24, 64)[0, 0, :4].tolist() == [0.0, 1.0, 0.0, 1.0]


def test_every_refusal_names_what_is_wrong():
    from tinyfusers_amd.vision.motion import MotionAdapter, parse_motion_state
    from tinyfusers_amd.vision.unet import SD15, TINY
    W = _tiny_file(max_len=24)
    key = f"up_blocks.1.motion_modules.2.temporal_transformer.{T}attention_blocks.1.to_k.weight"
    bad = dict(W); del bad[key]
    with pytest.raises(ValueError, match=r"lacks up_blocks\.1\.motion_modules\.2\.temporal_transformer\.transformer_blocks\.0\.attention_blocks\.1\.to_k\.weight"):
        parse_motion_state(TINY, bad)
    bad = dict(W); bad[key] = np.zeros((128, 64), np.float16)
    with pytest.raises(ValueError, match=r"attention_blocks\.1\.to_k\.weight has shape \(128, 64\), this UNet needs \(128, 128\)"):
        parse_motion_state(TINY, bad)
    bad = dict(W); bad["down_blocks.0.motion_modules.0.temporal_transformer.transformer_blocks.0.attention_blocks.0.to_q.bias"] = np.zeros(64, np.float16)
    with pytest.raises(ValueError, match=r"no place for.*attention_blocks\.0\.to_q\.bias"):
        parse_motion_state(TINY, bad)
    bad = dict(W); bad["model.diffusion_model.out.2.weight"] = np.zeros(4, np.float16)
    with pytest.raises(ValueError, match=r"name no motion module.*model\.diffusion_model\.out\.2\.weight"):
        parse_motion_state(TINY, bad)
    bad = dict(W); bad[f"down_blocks.0.motion_modules.0.temporal_transformer.{T}attention_blocks.1.pos_encoder.pe"] = np.zeros((1, 16, 64), np.float16)
    with pytest.raises(ValueError, match=r"attention_blocks\.1\.pos_encoder\.pe has shape \(1, 16, 64\), this UNet needs \(1, 24, 64\)"):
        parse_motion_state(TINY, bad)
    bad = {k: v for k, v in W.items() if not k.startswith("down_blocks.2.motion_modules.1.")}
    with pytest.raises(ValueError, match=r"lacks the module down_blocks\.2\.motion_modules\.1"):
        parse_motion_state(TINY, bad)
    # a slot plan that does not match the configuration: a module for a block that does not exist, a wrong channel count
    with pytest.raises(ValueError, match=r"module at down_blocks\.3\.motion_modules\.0, this UNet configuration has no such block"):
        from tinyfusers_amd.storage.synth import synth_motion_state_dict
        parse_motion_state(TINY, synth_motion_state_dict(SD15, 3, max_len=24))
    from dataclasses import replace
    with pytest.raises(ValueError, match=r"down_blocks\.1\.motion_modules\.0 has 128 channels \(norm\.weight\), the UNet's block has 192"):
        parse_motion_state(replace(TINY, channel_mult=(1, 3, 2)), W)
    with pytest.raises(ValueError, match="holds no motion module"):
        parse_motion_state(TINY, {})
    with pytest.raises(TypeError, match="file name or a dict"):
        MotionAdapter.load(TINY, 3)


# ---- the restatement's own properties ---------------------------------------------------------------------------------------------------------------
def _zero_pe(W):
    W = dict(W)
    for i in (0, 1):
        W[f"{T}attention_blocks.{i}.pos_encoder.pe"] = np.zeros_like(W[f"{T}attention_blocks.{i}.pos_encoder.pe"])
    return W


def _swap_attentions(W):
    out = dict(W)
    for k in W:
        if ".attention_blocks.0." in k:
            k1 = k.replace(".attention_blocks.0.", ".attention_blocks.1.")
            out[k], out[k1] = W[k1], W[k]
    return out


def test_restatement_without_pe_commutes_with_a_frame_permutation():
    C, F, V, h, w, ml = 64, 5, 2, 3, 2, 32
    W, x = _zero_pe(R.module_weights(C, ml)), R.module_input(C, F, V, h, w)
    y = R.motion_module_forward(x, W, F).numpy()
    perm = np.array([3, 0, 4, 1, 2])
    idx = np.concatenate([v * F + perm for v in range(V)])
    yp = R.motion_module_forward(x[idx], W, F).numpy()
    np.testing.assert_allclose(yp, y[idx], rtol=0, atol=1e-12)
    Wpe = R.module_weights(C, ml)                                  # ... and with the tables it does not
    assert np.abs(R.motion_module_forward(x[idx], Wpe, F).numpy() - R.motion_module_forward(x, Wpe, F).numpy()[idx]).max() > 0.1


def test_restatement_keeps_the_videos_apart():
    C, F, V, h, w, ml = R.MODULE_CASES[0]
    W, x, y = _case(*R.MODULE_CASES[0])
    for v in range(V):
        x2 = x.copy()
        x2[v * F:(v + 1) * F] += 1.0
        y2 = R.motion_module_forward(x2, W, F).numpy()
        other = slice((1 - v) * F, (2 - v) * F)
        assert np.array_equal(y2[other], y[other])                   # the other video: the same float64 values
        assert np.abs(y2[v * F:(v + 1) * F] - y[v * F:(v + 1) * F]).max() > 0.1


def test_restatement_at_one_frame_is_the_value_projection():
    """F = 1: the softmax over one frame is 1, each attention is to_out(to_v(LN(x) + pe[0]))."""
    C, ml = 64, 32
    W = R.module_weights(C, ml)
    x = R.module_input(C, 1, 3, 2, 2)
    W64 = {k: R.t64(v) for k, v in W.items()}
    t = R._group_norm(R.t64(x), 32, W64["norm.weight"], W64["norm.bias"], 1e-6).reshape(3, C, 4).permute(0, 2, 1) @ W64["proj_in.weight"].t() + W64["proj_in.bias"]
    for i in (0, 1):
        p = f"{T}attention_blocks.{i}."
        y = R._layer_norm(t, W64[f"{T}norms.{i}.weight"], W64[f"{T}norms.{i}.bias"]) + W64[p + "pos_encoder.pe"][0, 0]
        t = t + (y @ W64[p + "to_v.weight"].t()) @ W64[p + "to_out.0.weight"].t() + W64[p + "to_out.0.bias"]
    y = R._layer_norm(t, W64[T + "ff_norm.weight"], W64[T + "ff_norm.bias"]) @ W64[T + "ff.net.0.proj.weight"].t() + W64[T + "ff.net.0.proj.bias"]
    a, g = torch.chunk(y, 2, dim=-1)
    from oracle import ops
    t = t + (a * ops.gelu(g.float()).double()) @ W64[T + "ff.net.2.weight"].t() + W64[T + "ff.net.2.bias"]
    want = R.t64(x) + (t @ W64["proj_out.weight"].t() + W64["proj_out.bias"]).permute(0, 2, 1).reshape(3, C, 2, 2)
    np.testing.assert_allclose(R.motion_module_forward(x, W, 1).numpy(), want.numpy(), rtol=0, atol=2e-6)     # (2e-6: the float32 GELU of the oracle)


def test_restatement_scale_and_zero_proj_out():
    W, x, y = _case(*R.MODULE_CASES[0])
    F = R.MODULE_CASES[0][1]
    assert np.array_equal(R.motion_module_forward(x, W, F, scale=0.0).numpy(), x.astype(np.float64))
    np.testing.assert_allclose(R.motion_module_forward(x, W, F, scale=0.5).numpy(), x + 0.5 * (y - x), rtol=0, atol=1e-12)
    W0 = dict(W); W0["proj_out.weight"] = np.zeros_like(W["proj_out.weight"]); W0["proj_out.bias"] = np.zeros_like(W["proj_out.bias"])
    assert np.array_equal(R.motion_module_forward(x, W0, F).numpy(), x.astype(np.float64))


# ---- sensitivity: what the GPU gates can see ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.MODULE_CASES)
def test_module_gate_sees_pe_attention_order_and_head_count(case):
    C, F = case[0], case[1]
    W, x, ref = _case(*case)
    for what, alt in (("pe zeroed", R.motion_module_forward(x, _zero_pe(W), F)), ("attention blocks swapped", R.motion_module_forward(x, _swap_attentions(W), F)),
                      ("2 heads where it must be 8", R.motion_module_forward(x, W, F, heads=2))):
        u = _gate_units(alt.numpy(), ref)
        print(f"C={C} F={F} {what}: the restatement moves by {u:.1f} x the gate")
        assert u >= 10, (case, what, u)


def test_module_gate_sees_the_groupnorm_eps():
    C, F, V, h, w, ml = R.EPS_CASE
    W, x = R.module_weights(C, ml), R.eps_case_input()
    var = x.reshape(V * F, 32, -1).var(axis=-1)
    assert 0.5e-5 < float(np.median(var)) < 2e-5                      # per-group variance near 1e-5
    ref = R.motion_module_forward(x, W, F).numpy()
    u = _gate_units(R.motion_module_forward(x, W, F, gn_eps=1e-5).numpy(), ref)
    print(f"eps case: the restatement moves by {u:.1f} x the gate")
    assert u >= 10, u
    # (on the ordinary inputs the two eps are indistinguishable: that is why the case has an input scale of its own)
    W0, x0, ref0 = _case(*R.MODULE_CASES[0])
    assert _gate_units(R.motion_module_forward(x0, W0, R.MODULE_CASES[0][1], gn_eps=1e-5).numpy(), ref0) < 0.1


@functools.lru_cache(maxsize=None)
def tiny_forward_refs():
    """(x, ctx, plain, with motion) of the TINY eager-forward test: V = 2, F = 3, a 16 x 16 latent; shared with tests/test_gpu_motion.py."""
    import oracle
    from tinyfusers_amd.storage.synth import synth_motion_state_dict, synth_normal, synth_state_dict
    from tinyfusers_amd.vision.unet import TINY
    W = synth_state_dict(oracle.unet_param_shapes(oracle.TINY), 5)
    Wm = synth_motion_state_dict(TINY, 3, max_len=24, mid=True)
    x = synth_normal(5, "motion.lat", (6, 4, 16, 16)).astype(np.float16).astype(np.float32)
    ctx = np.repeat(synth_normal(5, "motion.c", (2, 13, 64)).astype(np.float16).astype(np.float32), 3, axis=0)
    Wf = {k: torch.from_numpy(v.astype(np.float32)) for k, v in W.items()}
    mods = {p: {k: v.astype(np.float32) for k, v in m.items()} for p, m in R.split_modules(Wm).items()}
    t = np.array([481.0], np.float32)
    plain = R.unet_forward_motion(x, t, ctx, Wf, oracle.TINY).numpy()
    moved = R.unet_forward_motion(x, t, ctx, Wf, oracle.TINY, motion=(mods, 3, 1.0)).numpy()
    return x, ctx, plain, moved, W, Wm


def test_unet_gate_sees_the_motion_modules():
    import oracle
    x, ctx, plain, moved, W, _ = tiny_forward_refs()
    Wf = {k: torch.from_numpy(v.astype(np.float32)) for k, v in W.items()}
    assert np.array_equal(plain, oracle.unet_forward(x, np.array([481.0], np.float32), ctx, Wf, oracle.TINY).numpy())      # motion=None: the oracle's walk
    rl2 = float(np.linalg.norm(moved - plain) / np.linalg.norm(plain))
    mx = float(np.abs(moved - plain).max() / np.abs(plain).max())
    print(f"TINY forward: the restatement with motion differs from the plain one by rel-L2 {rl2:.3f}, max {mx:.3f}")
    assert rl2 >= 10 * 5e-3 and mx >= 10 * 1e-2
