"""Host checks of the LoRA adapter path (storage/lora.py, StableDiffusion.load_lora / set_adapters): the generated target table, parsing of
kohya and PEFT files in both checkpoint formats, the operand layout the merge kernel reads, every refusal, and set_adapters' argument checks
and scale arithmetic against a stub that records merge calls.  No GPU: nothing here uploads or launches."""
import contextlib
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))
import lora_ref as R  # noqa: E402

from tinyfusers_amd.storage import lora as L  # noqa: E402
from tinyfusers_amd.storage.state import param_shapes  # noqa: E402

TE = "cond_stage_model.transformer.text_model."
UN = "model.diffusion_model."
SPOT = {
    "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q": UN + "input_blocks.1.1.transformer_blocks.0.attn1.to_q",
    "lora_unet_down_blocks_2_attentions_1_transformer_blocks_0_ff_net_0_proj": UN + "input_blocks.8.1.transformer_blocks.0.ff.net.0.proj",
    "lora_unet_mid_block_attentions_0_proj_in": UN + "middle_block.1.proj_in",
    "lora_unet_up_blocks_1_attentions_0_transformer_blocks_0_attn2_to_out_0": UN + "output_blocks.3.1.transformer_blocks.0.attn2.to_out.0",
    "lora_unet_up_blocks_3_attentions_2_proj_out": UN + "output_blocks.11.1.proj_out",
    "lora_unet_down_blocks_1_resnets_0_conv1": UN + "input_blocks.4.0.in_layers.2",
    "lora_unet_down_blocks_1_resnets_0_conv_shortcut": UN + "input_blocks.4.0.skip_connection",
    "lora_unet_down_blocks_0_downsamplers_0_conv": UN + "input_blocks.3.0.op",
    "lora_unet_up_blocks_0_upsamplers_0_conv": UN + "output_blocks.2.1.conv",
    "lora_unet_up_blocks_1_upsamplers_0_conv": UN + "output_blocks.5.2.conv",
    "lora_unet_up_blocks_2_resnets_1_time_emb_proj": UN + "output_blocks.7.0.emb_layers.1",
    "lora_te_text_model_encoder_layers_11_mlp_fc2": TE + "encoder.layers.11.mlp.fc2",
    "lora_unet_conv_in": UN + "input_blocks.0.0",
    "lora_unet_conv_out": UN + "out.2",
}
ATTN = ("_proj_in", "_proj_out", "_to_q", "_to_k", "_to_v", "_to_out_0", "_ff_net_0_proj", "_ff_net_2")


def _sd(cfg):
    from tinyfusers_amd.variants.sd import StableDiffusion
    return StableDiffusion(cfg)


@pytest.fixture(scope="module")
def sd15():
    from tinyfusers_amd.vision.unet import SD15
    return _sd(SD15)


@pytest.fixture(scope="module")
def tiny():
    from tinyfusers_amd.vision.unet import TINY
    return _sd(TINY)


# ---- the name table -------------------------------------------------------------------------------------------------------------------------------
def test_target_table_of_sd15(sd15):
    from tinyfusers_amd.ff.linear import Linear
    from tinyfusers_amd.vision.conv2d import Conv2d
    paths, targets, shapes = L.lora_target_paths(sd15), L.lora_targets(sd15), param_shapes(sd15)
    unet = [k for k in paths if k.startswith("lora_unet_")]
    te = [k for k in paths if k.startswith("lora_te_")]
    assert len([k for k in unet if "_attentions_" in k and k.endswith(ATTN)]) == 192
    assert len(te) == 72 and len(unet) + len(te) == len(paths)
    for k, p in SPOT.items():
        assert paths[k] == p, k
    for k, p in paths.items():
        assert len(shapes[p + ".weight"]) in (2, 4), k
        assert isinstance(targets[k], (Linear, Conv2d)) and L.weight_shape(targets[k]) == tuple(shapes[p + ".weight"])
        assert targets[k] is L._resolve(sd15, p)
    assert len(set(paths.values())) == len(paths)
    # conv_shortcut exactly where the ResBlock's skip is a conv: 3 in the encoder (320->640, 640->1280), all 12 of the decoder
    short = [k for k in paths if k.endswith("_conv_shortcut")]
    for k in short:
        assert isinstance(targets[k], Conv2d) and tuple(targets[k]._shape[2:]) == (1, 1)
    res = [k[:-len("_conv1")] for k in paths if k.endswith("_conv1")]
    assert len(res) == 22
    for r in res:
        block = L._resolve(sd15, paths[r + "_conv1"].rsplit(".in_layers.2", 1)[0])
        assert (r + "_conv_shortcut" in paths) == isinstance(block.skip_connection, Conv2d), r
    assert "lora_unet_down_blocks_0_resnets_0_conv_shortcut" not in paths and "lora_unet_mid_block_resnets_0_conv_shortcut" not in paths
    assert "lora_unet_down_blocks_3_downsamplers_0_conv" not in paths and "lora_unet_up_blocks_3_upsamplers_0_conv" not in paths
    assert "lora_unet_down_blocks_3_attentions_0_proj_in" not in paths


def test_target_table_of_tiny_follows_its_module_tree(tiny):
    from tinyfusers_amd.attention.attention import SpatialTransformer
    from tinyfusers_amd.vision.resnet import ResBlock
    paths, shapes = L.lora_target_paths(tiny), param_shapes(tiny)
    assert not any(k.startswith("lora_te_") for k in paths)              # TINY has no text encoder
    for k, p in paths.items():
        assert len(shapes[p + ".weight"]) in (2, 4), k
    unet = tiny.model.diffusion_model
    blocks = [bb for b in unet.input_blocks for bb in b] + list(unet.middle_block) + [bb for b in unet.output_blocks for bb in b]
    n_res, n_st = sum(isinstance(b, ResBlock) for b in blocks), sum(isinstance(b, SpatialTransformer) for b in blocks)
    assert len([k for k in paths if k.endswith("_conv1")]) == n_res
    assert len([k for k in paths if k.endswith("_proj_in")]) == n_st
    # every Linear / Conv2d weight below the blocks is reached exactly once (the time-embedding MLP is not a target)
    mat = {k[:-len(".weight")] for k, s in shapes.items() if k.endswith(".weight") and len(s) in (2, 4) and ".time_embed." not in k}
    assert set(paths.values()) == mat
    assert paths["lora_unet_up_blocks_1_upsamplers_0_conv"] == UN + "output_blocks.5.2.conv"      # attention at level 1: the third element
    assert paths["lora_unet_up_blocks_0_upsamplers_0_conv"] == UN + "output_blocks.2.1.conv"      # none at level 2: the second


# ---- parsing ----------------------------------------------------------------------------------------------------------------------------------------
PEFT = {
    "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q": "unet.down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q",
    "lora_unet_mid_block_attentions_0_transformer_blocks_0_ff_net_0_proj": "unet.mid_block.attentions.0.transformer_blocks.0.ff.net.0.proj",
    "lora_unet_up_blocks_1_attentions_0_proj_out": "unet.up_blocks.1.attentions.0.proj_out",
    "lora_unet_down_blocks_1_resnets_0_conv1": "unet.down_blocks.1.resnets.0.conv1",
    "lora_te_text_model_encoder_layers_3_self_attn_q_proj": "text_encoder.text_model.encoder.layers.3.self_attn.q_proj",
}


def _kohya(sd15, rank=4, alpha=True):
    targets = L.lora_targets(sd15)
    rng = np.random.default_rng(3)
    out = {}
    for k in PEFT:
        shape = L.weight_shape(targets[k])
        up = (rank, 1, 1) if len(shape) == 4 else (rank,)
        out[k + ".lora_up.weight"] = rng.standard_normal((shape[0],) + up).astype(np.float16)
        out[k + ".lora_down.weight"] = rng.standard_normal((rank,) + shape[1:]).astype(np.float16)
        if alpha:
            out[k + ".alpha"] = np.asarray(np.float32(rank / 2))
    return out


def _as_peft(kohya):
    out = {}
    for key, v in kohya.items():
        mod, what = key.split(".", 1)
        out[PEFT[mod] + {"lora_up.weight": ".lora_B.weight", "lora_down.weight": ".lora_A.weight", "alpha": ".alpha"}[what]] = v
    return out


def _load(sd, src, **kw):
    mods, other = L.parse_lora(src)
    shapes = {k: L.weight_shape(m) for k, m in L.lora_targets(sd).items()}
    return L.check_lora(mods, other, shapes, has_text_encoder=sd.cond_stage_model is not None, **kw)


def test_kohya_and_peft_files_in_both_formats_parse_alike(sd15, tmp_path):
    from tinyfusers_amd.storage.unpicker import save_safetensors
    kohya = _kohya(sd15)
    peft = _as_peft(kohya)
    want = _load(sd15, kohya)
    assert set(want) == set(PEFT)
    srcs = []
    for name, d in (("k", kohya), ("p", peft)):
        st, pt = str(tmp_path / f"{name}.safetensors"), str(tmp_path / f"{name}.pt")
        save_safetensors(st, d)
        torch.save({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in d.items()}, pt)        # fp32 on disk: exact for fp16 values
        srcs += [st, pt, d]
    for src in srcs:
        got = _load(sd15, src)
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(got[k].up, want[k].up) and np.array_equal(got[k].down_t, want[k].down_t), (src, k)
            assert got[k].alpha == want[k].alpha == 2.0 and got[k].rank == want[k].rank == 4
            assert got[k].up.dtype == np.float16 and got[k].down_t.dtype == np.float16
    assert all(w.alpha == 4.0 and w.rank == 4 for w in _load(sd15, _kohya(sd15, alpha=False)).values())     # no alpha: the rank


def test_operand_layout_transposes_pads_and_flattens_conv_rows_as_the_device_stores_them(sd15, monkeypatch):
    import tinyfusers_amd.storage.tensor as T
    kohya = _kohya(sd15, rank=5)
    got = _load(sd15, kohya)
    lin, conv = "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q", "lora_unet_down_blocks_1_resnets_0_conv1"
    for k in (lin, conv):
        up, down = kohya[k + ".lora_up.weight"], kohya[k + ".lora_down.weight"]
        w = got[k]
        n, kd = up.shape[0], int(np.prod(down.shape[1:]))
        assert w.up.shape == (n, 32) and w.down_t.shape == (kd, 32) and w.up.flags.c_contiguous and w.down_t.flags.c_contiguous
        assert np.array_equal(w.up[:, :5], up.reshape(n, 5)) and not w.up[:, 5:].any() and not w.down_t[:, 5:].any()
        assert np.array_equal(w.down_t[:, :5].T, R.stored(down))
    assert L.pad_rank(1) == 32 and L.pad_rank(32) == 32 and L.pad_rank(33) == 64 and L.pad_rank(256) == 256
    # the device storage rule itself: what asarray hands to the upload for a 4-D array (the NHWC transposition of storage/tensor.py)
    down = kohya[conv + ".lora_down.weight"]
    sent = {}
    monkeypatch.setattr(T._pool, "alloc", lambda nbytes: (0x1000, int(nbytes)))
    monkeypatch.setattr(T.hip, "tf_memcpy", lambda dst, src, n, kind: sent.update(b=ctypes.string_at(src, n)), raising=False)
    a = T.asarray(down, np.float16)
    a._fin.detach()                                                      # (no device block behind it)
    assert a.layout == "nhwc"
    stored = np.frombuffer(sent["b"], np.float16).reshape(5, -1)
    assert np.array_equal(got[conv].down_t[:, :5].T, stored)
    assert stored.shape[1] == 9 * 320 and np.array_equal(stored[:, :320], down[:, :, 0, 0])      # (r, s) = (0, 0) first, channels innermost


def test_bf16_cast_rounds_to_nearest_even(sd15):
    k = "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q"
    d = {k + ".lora_up.weight": np.full((320, 1), 1.0 + 2.0 ** -8, np.float32), k + ".lora_down.weight": np.full((1, 320), 1.0 + 3 * 2.0 ** -8, np.float32)}
    w = _load(sd15, d, bf16=True)[k]
    assert w.up.dtype == np.float32 and w.up[0, 0] == 1.0 and w.down_t[0, 0] == np.float32(1.0 + 2.0 ** -6)      # ties to even, both ways
    w = _load(sd15, d)[k]
    assert w.up[0, 0] == np.float16(1.0 + 2.0 ** -8)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_the_key(sd15, tiny):
    k = "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q"
    c = "lora_unet_down_blocks_1_resnets_0_conv1"
    up, down = k + ".lora_up.weight", k + ".lora_down.weight"
    base = {up: np.ones((320, 4), np.float16), down: np.ones((4, 320), np.float16)}

    def bad(match, **change):
        d = dict(base)
        d.update(change)
        with pytest.raises(ValueError, match=match):
            _load(sd15, {kk: v for kk, v in d.items() if v is not None})
    bad(r"lora_up\.weight: 319 output rows", **{up: np.ones((319, 4), np.float16)})
    bad(r"lora_down\.weight: input side \(321,\)", **{down: np.ones((4, 321), np.float16)})
    bad(r"lora_up\.weight: shape \(320, 5\) does not match the rank 4", **{up: np.ones((320, 5), np.float16)})
    bad(r"lora_down\.weight: rank 257", **{up: np.ones((320, 257), np.float16), down: np.ones((257, 320), np.float16)})
    bad(r"lora_up\.weight: a value is not finite", **{up: np.full((320, 4), np.nan, np.float16)})
    bad(r"lora_down\.weight: a value is not finite", **{down: np.full((4, 320), np.inf, np.float32)})
    bad(r"lora_down\.weight: a value is not finite after the cast", **{down: np.full((4, 320), 1e6, np.float32)})
    bad(r"alpha: alpha must be one finite number", **{k + ".alpha": np.float32(np.inf)})
    bad(r"has no lora_up tensor", **{up: None})
    with pytest.raises(ValueError, match=r"conv1\.lora_up\.weight: the lora_up of a conv must be 1x1"):
        _load(sd15, {c + ".lora_up.weight": np.ones((640, 4, 3, 3), np.float16), c + ".lora_down.weight": np.ones((4, 320, 3, 3), np.float16)})
    with pytest.raises(ValueError, match=r"conv1\.lora_down\.weight: input side \(320, 1, 1\)"):
        _load(sd15, {c + ".lora_up.weight": np.ones((640, 4, 1, 1), np.float16), c + ".lora_down.weight": np.ones((4, 320, 1, 1), np.float16)})
    for key, why in ((k + ".hada_w1_a", "LoHa"), (k + ".lokr_w1", "LoKr"), (k + ".dora_scale", "DoRA"), (c + ".lora_mid.weight", "Tucker"),
                     ("unet.down_blocks.0.attentions.0.transformer_blocks.0.attn1.processor.to_q_lora.down.weight", "attention-processor")):
        with pytest.raises(ValueError, match=why) as e:
            L.parse_lora(dict(base, **{key: np.ones((4, 4), np.float16)}))
        assert key in str(e.value)
    # keys that match no target: the first five are listed; strict=False prints them
    stray = {f"lora_unet_nowhere_{i}.lora_down.weight": np.ones((4, 8), np.float16) for i in range(7)}
    with pytest.raises(ValueError, match=r"7 key\(s\) match no target") as e:
        _load(sd15, dict(base, **stray))
    assert str(e.value).count("lora_unet_nowhere_") == 5
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        got = _load(sd15, dict(base, **stray, **{"some.other.key": np.ones(3)}), strict=False)
    assert set(got) == {k}
    assert sorted(buf.getvalue().split("\n")[:-1]) == sorted([f"skipped: {s}" for s in stray] + ["skipped: some.other.key"])
    # a model without a text encoder refuses lora_te_* keys unless strict=False
    te = "lora_te_text_model_encoder_layers_0_mlp_fc1"
    d = {te + ".lora_up.weight": np.ones((3072, 4), np.float16), te + ".lora_down.weight": np.ones((4, 768), np.float16)}
    assert set(_load(sd15, d)) == {te}
    with pytest.raises(ValueError, match="no text encoder"):
        tiny.load_lora(d, "te")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert _load(tiny, d, strict=False) == {}
    assert buf.getvalue().count("skipped: " + te) == 2
    assert tiny._lora is None                                              # (the refused load left nothing behind)


# ---- set_adapters: arguments and scales -----------------------------------------------------------------------------------------------------------------
class _M:
    def __init__(self, tag):
        self.weight = tag


class _W:
    def __init__(self, alpha, rank):
        self.alpha, self.rank = alpha, rank


def test_plan_scales_and_argument_checks():
    u1, u2, t1 = "lora_unet_a", "lora_unet_b", "lora_te_c"
    loaded = {"A": {u1: _W(8.0, 4), t1: _W(1.0, 16)}, "B": {u1: _W(0.3, 8), u2: _W(3.0, 3)}}
    plan, active = L.plan_adapters(loaded, ["A", "B"], [0.7, -0.4])
    assert active == {"A": (0.7, 0.7), "B": (-0.4, -0.4)} and list(active) == ["A", "B"]
    assert [n for n, _ in plan[u1]] == ["A", "B"] and [n for n, _ in plan[u2]] == ["B"] and [n for n, _ in plan[t1]] == ["A"]
    assert plan[u1][0][1] == np.float32(0.7 * 8.0 / 4) and plan[u1][1][1] == np.float32(np.float64(-0.4) * 0.3 / 8)
    assert plan[u2][0][1] == np.float32(np.float64(-0.4) * 3.0 / 3) and plan[t1][0][1] == np.float32(0.7 / 16)
    assert all(isinstance(s, np.float32) for e in plan.values() for _, s in e)
    # float64 first, one rounding: not the fp32 product of fp32 factors
    w, a, r = 0.1, 0.7, 3
    p, _ = L.plan_adapters({"A": {u1: _W(a, r)}}, ["A"], w)
    assert p[u1][0][1] == np.float32(np.float64(w) * a / r)
    # the text encoder's weight: default the UNet's, else its own; a zero weight drops the adapter from that side
    plan, active = L.plan_adapters(loaded, ["A", "B"], 1.0, text_encoder_weights=[0.0, 2.0])
    assert t1 not in plan and active == {"A": (1.0, 0.0), "B": (1.0, 2.0)}
    plan, _ = L.plan_adapters(loaded, ["A", "B"], [1.0, 0.0])
    assert [n for n, _ in plan[u1]] == ["A"] and u2 not in plan and plan[t1][0][1] == np.float32(1 / 16)
    assert L.plan_adapters(loaded, [], 1.0) == ({}, {})
    for names, kw, match in ((["A", "C"], {}, "unknown adapter 'C'"), (["A", "A"], {}, "named twice"), (["A"], {"weights": np.nan}, "not finite"),
                             (["A"], {"weights": [1.0, 2.0]}, "one float or one per name"), (["A", "B"], {"text_encoder_weights": [np.inf, 1]}, "not finite"),
                             (["A"], {"weights": 1e39}, "not finite in fp32")):
        with pytest.raises(ValueError, match=match):
            L.plan_adapters(loaded, names, **kw)
    nine = {f"L{i}": {u1: _W(1.0, 4)} for i in range(9)}
    assert len(L.plan_adapters(nine, list(nine)[:8])[0][u1]) == 8
    with pytest.raises(ValueError, match="9 adapters on lora_unet_a"):
        L.plan_adapters(nine, list(nine))
    assert len(L.plan_adapters(nine, list(nine), [1] * 8 + [0])[0][u1]) == 8          # (a zero weight does not count)


def test_registry_merges_from_the_base_and_hands_the_base_object_back():
    u1, u2 = "lora_unet_a", "lora_unet_b"
    targets = {u1: _M("base1"), u2: _M("base2")}
    base1, base2 = targets[u1].weight, targets[u2].weight
    reg = L.LoraRegistry()
    reg.loaded = {"A": {u1: _W(4.0, 4)}, "B": {u1: _W(8.0, 4), u2: _W(4.0, 4)}}
    calls = []

    def merge(base, entries):
        calls.append((base, [(lw, float(s)) for lw, s in entries]))
        return f"merged{len(calls)}"

    def set_(names, *a, **kw):
        plan, active = L.plan_adapters(reg.loaded, names, *a, **kw)
        return reg.apply(plan, targets, merge)
    changed, retired = set_(["A"])
    assert changed and retired == [] and calls == [(base1, [(reg.loaded["A"][u1], 1.0)])]
    assert targets[u1].weight == "merged1" and targets[u2].weight is base2
    assert set_(["A"]) == (False, []) and len(calls) == 1                        # nothing changed: no launch
    changed, retired = set_(["A", "B"], [0.5, 2.0])
    assert changed and retired == ["merged1"]
    assert calls[1] == (base1, [(reg.loaded["A"][u1], 0.5), (reg.loaded["B"][u1], 4.0)])      # from the BASE, never from a merged weight
    assert calls[2] == (base2, [(reg.loaded["B"][u2], 2.0)])
    # update_state in between: the installed weight is the new base
    targets[u2].weight = "fresh2"
    changed, retired = set_(["A", "B"], [0.5, 2.0])
    assert changed and calls[3][0] == "fresh2" and len(calls) == 4 and retired == []
    changed, retired = set_([])
    assert changed and sorted(retired) == ["merged2", "merged4"]
    assert targets[u1].weight is base1 and targets[u2].weight == "fresh2" and reg.base == {} and reg.merged == {}
    assert set_([]) == (False, [])


def test_set_adapters_and_unload_check_names_before_touching_anything(tiny):
    from tinyfusers_amd.vision.unet import TINY
    sd = _sd(TINY)
    assert sd.adapters() == {}
    with pytest.raises(ValueError, match="unknown adapter 'x'"):
        sd.set_adapters(["x"])
    with pytest.raises(TypeError):
        sd.set_adapters("x")
    with pytest.raises(ValueError, match="unknown adapter"):
        sd.unload_lora("x")
    sd._lora = L.LoraRegistry()                                          # (as load_lora leaves it, without the upload)
    sd._lora.loaded, sd._lora.active = {"A": {}, "B": {}}, {"A": (1.0, 1.0)}
    with pytest.raises(ValueError, match="'A' is active"):
        sd.unload_lora("A")
    with pytest.raises(ValueError, match="loaded already"):
        sd.load_lora({}, "B")
    sd.unload_lora("B")
    assert sorted(sd._lora.loaded) == ["A"] and sd.adapters() == {"A": (1.0, 1.0)}
