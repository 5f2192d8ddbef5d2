"""The IP-Adapter's host side (no GPU): the file reader on both published layouts written by the test, the index <-> module table against the
explicit list of SD-1.5's sixteen cross-attentions (adapter order is down, up, MID; the module walk is input, middle, output), shape checks that
name the key, the refusal of the plus / FaceID families, the argument checks of compile() / start(), and the CPU restatement's own sanity (scale 0
is oracle.unet_forward; the image term moves the output)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "aux"))

import ip_adapter_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def built():
    import __graft_entry__
    __graft_entry__.build()


def _state(cfg, tokens=4, embed_dim=32, seed=3):
    rng = np.random.default_rng(seed)
    return {k: (rng.standard_normal(s) * 0.1).astype(np.float16) for k, s in R.adapter_param_shapes(cfg, tokens, embed_dim).items()}


def _nested(state):
    return {"image_proj": {k[len("image_proj."):]: torch.from_numpy(v.copy()) for k, v in state.items() if k.startswith("image_proj.")},
            "ip_adapter": {k[len("ip_adapter."):]: torch.from_numpy(v.copy()) for k, v in state.items() if k.startswith("ip_adapter.")}}


def test_index_table_is_down_up_mid(built):
    import oracle
    from tinyfusers_amd.storage.ip_adapter import adapter_paths
    from tinyfusers_amd.vision.unet import SD15, UNetModel
    unet = UNetModel(SD15)
    table = [(n, p) for n, p, _ in adapter_paths(unet)]
    assert table == R.SD15_PATHS == R.paths(oracle.SD15) and len(table) == 16
    assert [n for n, _ in table] == list(range(1, 32, 2)) and table[-1] == (31, "middle_block.1")
    # the module walk the step-level K|V GEMM uses is another order: the table must not follow it
    from tinyfusers_amd.attention.attention import SpatialTransformer
    walk = unet._all(SpatialTransformer)
    assert [id(st) for _, _, st in adapter_paths(unet)] != [id(s) for s in walk] and {id(st) for _, _, st in adapter_paths(unet)} == {id(s) for s in walk}
    for (n, p, st) in adapter_paths(unet):                     # each path names the module it is paired with
        part, i, j = p.split(".") if p.count(".") == 2 else (p.split(".")[0], None, p.split(".")[1])
        assert (getattr(unet, part)[int(i)][int(j)] if i is not None else unet.middle_block[int(j)]) is st


def test_reader_round_trips_both_layouts(built, tmp_path):
    import oracle
    from tinyfusers_amd.storage.ip_adapter import IPAdapter, load_ip_adapter
    from tinyfusers_amd.storage.unpicker import save_safetensors
    from tinyfusers_amd.vision.unet import SD15, UNetModel
    state = _state(oracle.SD15, tokens=4, embed_dim=32)
    flat, nested = str(tmp_path / "ip.safetensors"), str(tmp_path / "ip.bin")
    save_safetensors(flat, state)
    torch.save(_nested(state), nested)
    unet = UNetModel(SD15)
    for src in (flat, nested, state, _nested(state)):
        got = load_ip_adapter(src)
        assert set(got) == set(state)
        for k in state:
            assert got[k].dtype == np.float16 and np.array_equal(got[k], state[k]), k
        assert IPAdapter.token_count(unet, got) == (4, 32)
        IPAdapter(unet, 4, 32).check(got)
    with pytest.raises(TypeError):
        load_ip_adapter(3)


def test_shape_checks_name_the_key(built):
    import oracle
    from tinyfusers_amd.storage.ip_adapter import IPAdapter, UnsupportedAdapter
    from tinyfusers_amd.vision.unet import SD15, TINY, UNetModel
    unet, state = UNetModel(SD15), _state(oracle.SD15)
    ad = IPAdapter(unet, 4, 32)
    assert ad.expected_shapes() == R.adapter_param_shapes(oracle.SD15, 4, 32)
    bad = dict(state); bad["ip_adapter.13.to_v_ip.weight"] = np.zeros((640, 768), np.float16)
    with pytest.raises(ValueError, match=r"ip_adapter\.13\.to_v_ip\.weight has shape \(640, 768\).*\(1280, 768\)"):
        ad.check(bad)
    bad = dict(state); del bad["ip_adapter.31.to_k_ip.weight"]
    with pytest.raises(ValueError, match=r"lacks ip_adapter\.31\.to_k_ip\.weight"):
        ad.check(bad)
    bad = dict(state); bad["ip_adapter.33.to_k_ip.weight"] = bad["ip_adapter.31.to_k_ip.weight"]
    with pytest.raises(ValueError, match=r"no place for.*ip_adapter\.33"):
        ad.check(bad)
    with pytest.raises(ValueError, match="image_proj.proj.weight"):            # an SD-1.5 adapter on a UNet of another context width
        IPAdapter.token_count(UNetModel(TINY), {"image_proj.proj.weight": np.zeros((4 * 768 + 8, 32), np.float16)})
    with pytest.raises(ValueError, match="image_proj.norm.weight"):
        IPAdapter(UNetModel(TINY), 48, 32).check(state)                         # (3072 = 48 x 64: the token count reads, the norm does not fit)
    with pytest.raises(UnsupportedAdapter, match="1 .. 64"):
        IPAdapter(unet, 65, 32)


def test_other_adapter_families_are_refused_by_name(built):
    import oracle
    from tinyfusers_amd.storage.ip_adapter import UnsupportedAdapter, load_ip_adapter
    state = _state(oracle.SD15)
    plus = dict(state); plus["image_proj.latents"] = np.zeros((1, 16, 768), np.float16)
    with pytest.raises(UnsupportedAdapter, match="plus family is unsupported"):
        load_ip_adapter(plus)
    nested = _nested(state); nested["image_proj"]["latents"] = torch.zeros(1, 16, 768)
    with pytest.raises(UnsupportedAdapter, match="plus"):
        load_ip_adapter(nested)
    face = dict(state); face["ip_adapter.1.to_k_lora.down.weight"] = np.zeros((128, 320), np.float16)
    with pytest.raises(UnsupportedAdapter, match="FaceID family is unsupported"):
        load_ip_adapter(face)
    face = {k: v for k, v in state.items() if not k.startswith("image_proj.proj.")}; face["image_proj.proj.0.weight"] = np.zeros((8, 8), np.float16)
    with pytest.raises(UnsupportedAdapter, match="FaceID"):
        load_ip_adapter(face)
    with pytest.raises(UnsupportedAdapter, match="not an ip-adapter_sd15 file"):
        load_ip_adapter({"model.diffusion_model.out.2.bias": np.zeros(4, np.float16)})


def test_compile_and_start_argument_checks(built):
    import types
    from tinyfusers_amd.variants import inputs
    from tinyfusers_amd.variants import samplers as S
    sch = S.DPMSolverPP2M().schedule(4)
    cfg = lambda **k: types.SimpleNamespace(cfg_parallel=k.get("par", False), dtype=k.get("dtype", "f16"), parallel_branches=False, is_bf16=lambda: k.get("dtype") == "bf16")
    lat = types.SimpleNamespace(shape=(2, 4, 16, 16))
    ok = lambda **k: inputs.check_compile(k.pop("cin", 4), k.pop("net", False), k.pop("config", cfg()), lat, k.pop("sampler", sch), k.pop("inpaint", False),
                                          k.pop("concat", None), k.pop("control", False), k.pop("cfg", True), ip_adapter=True, has_ip_adapter=k.pop("has", True))
    ok(); ok(cfg=False); ok(inpaint=True); ok(concat="inpaint", cin=9); ok(control=True, net=True); ok(config=cfg(dtype="bf16"))
    with pytest.raises(ValueError, match="attach_ip_adapter"):
        ok(has=False)
    with pytest.raises(ValueError, match="needs a sampler"):
        ok(sampler=None)
    with pytest.raises(ValueError, match="concat='edit'"):
        ok(concat="edit", cin=8)
    with pytest.raises(S.UnsupportedSamplerConfig, match="TF_CFG_PARALLEL"):
        ok(config=cfg(par=True))
    with pytest.raises(S.UnsupportedSamplerConfig, match="fp8"):
        ok(config=cfg(dtype="fp8"))
    # start(ip_scale=, ip_image_embeds=)
    assert np.array_equal(inputs.ip_scales(None, 16), np.ones(16, np.float32)) and inputs.ip_scales(0.5, 11).shape == (12,)
    assert np.array_equal(inputs.ip_scales(0.5, 11), np.float32([0.5] * 11 + [1.0]))
    assert np.array_equal(inputs.ip_scales(np.arange(16), 16), np.arange(16, dtype=np.float32))
    for bad in (np.ones(15), np.ones((2, 8)), float("nan")):
        with pytest.raises(ValueError, match="ip_scale"):
            inputs.ip_scales(bad, 16)
    e = inputs.ip_embeds(np.ones((1, 32)), 2, 32)
    assert e.shape == (2, 32) and e.dtype == np.float32 and e.flags.c_contiguous
    for bad in (np.ones((3, 32)), np.ones((2, 31)), np.ones(32), np.full((2, 32), np.inf)):
        with pytest.raises(ValueError, match="ip_image_embeds"):
            inputs.ip_embeds(bad, 2, 32)


def test_the_restatement_at_scale_zero_is_the_oracle_unet():
    import oracle
    cfg = oracle.TINY
    rng = np.random.default_rng(1)
    from tinyfusers_amd.storage.synth import synth_state_dict
    W = {k: torch.from_numpy(v.astype(np.float32)) for k, v in synth_state_dict(oracle.unet_param_shapes(cfg), 5).items()}
    A = {k: v.astype(np.float32) * 5 for k, v in _state(cfg, 4, 32).items()}
    x, ctx = rng.standard_normal((2, 4, 8, 8)).astype(np.float32), rng.standard_normal((2, 13, cfg.context_dim)).astype(np.float32)
    tok = R.image_tokens(rng.standard_normal((2, 32)).astype(np.float32), A, cfg.context_dim)
    assert tuple(tok.shape) == (2, 4, cfg.context_dim) and tuple(R.context_kv(tok, A, cfg).shape)[:2] == (2, 4)
    assert abs(float(tok.mean(-1).abs().max())) < 0.5                      # (LayerNorm over each token, then the affine)
    t = np.array([481.0], np.float32)
    plain = oracle.unet_forward(x, t, ctx, W, cfg).numpy()
    assert np.array_equal(R.unet_forward(x, t, ctx, W, A, tok, 0.0, cfg).numpy(), plain)
    moved = R.unet_forward(x, t, ctx, W, A, tok, 1.0, cfg).numpy()
    assert np.abs(moved - plain).max() > 1e-3 * np.abs(plain).max()
    per = np.zeros(len(R.paths(cfg)), np.float32); per[-1] = 1.0           # the middle block alone
    mid = R.unet_forward(x, t, ctx, W, A, tok, per, cfg).numpy()
    assert not np.array_equal(mid, plain) and not np.array_equal(mid, moved)
