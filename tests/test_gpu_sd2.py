"""The SD-2.x path on the device: the UNet with a head count per level (UNetConfig.d_head, TINY_V2: 1 / 2 / 2 heads of 64), 2-D proj_in / proj_out
tensors, sampling with prediction="v" and cfg_rescale=True inside the captured step (tf_sampler_tail_*), one SD21-size step, and the OpenCLIP text
tower (vae/open_clip_text.py) -- against tests/aux/sd2_ref.py: the oracle's forward per step with the float64 tail around it, and
transformers.CLIPTextModel in float64.  Gates: tests/test_gpu_samplers.py::_gate (rel-L2 5e-3, max 1e-2 relative; bf16 3e-2 both), and for the text
tower the gate tests/test_gpu_model.py holds the SD-1.5 text encoder to (``_text_gate``).

The guidance of the trajectories.  The gate was set on eps-prediction trajectories at guidance 7.5.  Read as v, the output of these untrained
weights drives x0 = sqrt(a) x - sqrt(1 - a) v about three times harder than it drives (x - sqrt(1 - a) e) / sqrt(a): rounding nothing but the
step's input and output to fp16 in the float64 reference moves the 4-step DPM++2M result by 5.6e-4 (rel-L2) for eps at guidance 7.5, by 1.48e-3
for v at 7.5 and by 6.3e-4 for v at 3.0 (8.1e-4 / 4.6e-4 with rescale 0.7) -- figures of the reference alone.  The runs here use guidance 3.0, where
the v problem is as well conditioned as the eps problem the gate was set for.  At 7.5 the fp16 v run measured rel-L2 6.7e-3 against the gate's
5e-3 (the bf16 v + rescale run 3.8e-2 against 3e-2) with every single step inside its float64 budget (tests/test_gpu_sampler_tail.py) and the UNet
forward at 1.5e-3."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "aux"))

import sd2_ref as R  # noqa: E402
from test_gpu_samplers import SEED, _gate  # noqa: E402
from test_samplers_host import randn_ref  # noqa: E402

pytestmark = pytest.mark.gpu
G = 3.0                                 # (module docstring)
SHAPE = (2, 4, 16, 16)


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


@pytest.fixture(scope="module")
def data():
    """(UNet weights by LDM name, context, unconditional context) of TINY_V2: computed once, never written."""
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.vision.unet import TINY_V2
    W = synth_state_dict(R.unet_shapes(TINY_V2), 5)
    ctx = synth_normal(5, "c", (2, 13, 128)).astype(np.float16).astype(np.float32)
    unc = synth_normal(5, "u", (2, 13, 128)).astype(np.float16).astype(np.float32)
    return W, ctx, unc


def _sched(n=4):
    from tinyfusers_amd.variants import samplers as S
    return S.DPMSolverPP2M().schedule(n)


def _model(tf, data, sch, **modes):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY_V2
    W, ctx, unc = data
    sd = StableDiffusion(TINY_V2)
    update_state(sd.model.diffusion_model, W, "")
    lat = sd.latent_from_numpy(np.zeros(SHAPE, np.float32))
    sd.compile(tf.DeviceArray.from_numpy(unc), tf.DeviceArray.from_numpy(ctx), lat, sampler=sch, **modes)
    return sd, lat


def _final(sd, lat, eager=False, guidance=G, **start):
    sd.start(seed=SEED, **start)
    lat0 = lat.numpy().copy()
    sd.run(guidance, eager=eager); sd.synchronize()
    return lat0, lat.numpy().copy()


def _f32(W):
    import torch
    return {k: torch.from_numpy(v.astype(np.float32)) for k, v in W.items()}


def _noise(tag):
    n = int(np.prod(SHAPE[1:]))
    return lambda i: np.stack([randn_ref(SEED, b, n, i, tag).reshape(SHAPE[1:]) for b in range(SHAPE[0])])


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_one_unet_forward_with_a_head_count_per_level(tf, data, dtype):
    from tinyfusers_amd import config
    from tinyfusers_amd.attention.attention import SpatialTransformer
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_normal
    from tinyfusers_amd.storage.tensor import bfloat16
    from tinyfusers_amd.vision.unet import TINY_V2, UNetModel
    W, ctx, _ = data
    x = synth_normal(7, "x", SHAPE).astype(np.float16).astype(np.float32)
    ref = R.unet_forward(x, np.array([481.0], np.float32), ctx, _f32(W), TINY_V2).numpy()
    config.set_dtype(dtype)
    try:
        dt = bfloat16 if dtype == "bf16" else np.float16
        unet = UNetModel(TINY_V2)
        update_state(unet, W, "")
        assert [st.transformer_blocks[0].attn1.num_heads for st in unet._all(SpatialTransformer)] == [1, 1, 2, 2, 2, 2, 2, 2, 1, 1, 1]
        got = unet(tf.DeviceArray.from_numpy(x, dt, "nhwc"), 481.0, tf.DeviceArray.from_numpy(ctx, dt)).numpy()
    finally:
        config.set_dtype("fp16")
    tol = 3e-2 if dtype == "bf16" else None
    _gate(got, ref, *((tol, tol) if tol else ()))


def test_two_dimensional_proj_tensors_install_the_four_dimensional_bits(tf, data):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_normal
    from tinyfusers_amd.vision.unet import TINY_V2, UNetModel
    W, ctx, _ = data
    lin = {k: (v.reshape(v.shape[:2]) if k.endswith((".proj_in.weight", ".proj_out.weight")) else v) for k, v in W.items()}
    assert sum(v.ndim == 2 and W[k].ndim == 4 for k, v in lin.items()) == 22           # 11 SpatialTransformers
    a, b = UNetModel(TINY_V2), UNetModel(TINY_V2)
    update_state(a, W, ""); update_state(b, lin, "")
    for sa, sb in zip(a._all(type(a.middle_block[1])), b._all(type(b.middle_block[1]))):
        for m in ("proj_in", "proj_out"):
            wa, wb = getattr(sa, m).weight, getattr(sb, m).weight
            assert wa.shape == wb.shape and wa.layout == wb.layout and np.array_equal(wa.numpy(), wb.numpy())
    x = tf.DeviceArray.from_numpy(synth_normal(7, "x", SHAPE).astype(np.float16), np.float16, "nhwc")
    c = tf.DeviceArray.from_numpy(ctx, np.float16)
    assert np.array_equal(a(x, 481.0, c).numpy(), b(x, 481.0, c).numpy())
    bad = dict(W); bad["middle_block.1.proj_in.weight"] = W["middle_block.1.proj_in.weight"].reshape(-1)       # any other rank: as before, no reshape
    c3 = UNetModel(TINY_V2); update_state(c3, bad, "")
    assert c3.middle_block[1].proj_in.weight.shape != a.middle_block[1].proj_in.weight.shape


def test_v_prediction_and_cfg_rescale_sampling(tf, data):
    W, ctx, unc = data
    sch = _sched()
    Wf = _f32(W)
    # prediction="v"
    sd, lat = _model(tf, data, sch, prediction="v")
    outs = [_final(sd, lat, eager=e) for e in (False, True, False)]
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][1], outs[2][1])          # graph == eager == graph again
    lat0 = outs[0][0]
    from tinyfusers_amd.vision.unet import TINY_V2
    ref_v = R.trajectory(Wf, TINY_V2, [unc, ctx], lat0, sch, G, vpred=True)
    _gate(outs[0][1], ref_v)
    v_plain = outs[0][1]
    # prediction="v", cfg_rescale=True: phi = 0.7 after compile
    sd, lat = _model(tf, data, sch, prediction="v", cfg_rescale=True)
    assert abs(float(sd._rescale_phi.numpy()[0]) - 0.7) < 1e-7 and sd._compile_args["cfg_rescale"] is True and sd._compile_args["prediction"] == "v"
    outs = [_final(sd, lat, eager=e) for e in (False, True, False)]
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][1], outs[2][1])
    ref_r = R.trajectory(Wf, TINY_V2, [unc, ctx], lat0, sch, G, vpred=True, phi=np.float64(np.float32(0.7)))
    _gate(outs[0][1], ref_r)
    d = np.linalg.norm(outs[0][1] - v_plain) / np.linalg.norm(v_plain)
    print(f"phi 0.7 against phi 0: rel-L2 {d:.3e}")
    assert d > 5e-3 and np.abs(outs[0][1] - v_plain).max() > 1e-2 * np.abs(v_plain).max()            # more than the gate: the word is read
    sd.set_cfg_rescale(0.0)
    assert np.array_equal(_final(sd, lat)[1], v_plain)                                                 # phi = 0: the cfg_rescale=False compile, bit for bit
    assert np.array_equal(_final(sd, lat, cfg_rescale=0.7)[1], outs[0][1])                            # start(cfg_rescale=) writes the same word, no re-capture
    before = lat.numpy().copy()
    with pytest.raises(ValueError, match="phi"):
        sd.start(seed=1, cfg_rescale=1.5)
    assert np.array_equal(lat.numpy(), before)                                                         # refused before anything was written


def test_the_rescaled_step_has_the_plain_steps_entries(tf, data):
    sys.path.insert(0, os.path.dirname(HERE))
    from tools.sampler_bench import step_entries
    sch = _sched()
    counts = {}
    for key, modes in (("plain", {}), ("v", dict(prediction="v")), ("rescale", dict(prediction="v", cfg_rescale=True))):
        sd, _ = _model(tf, data, sch, **modes)
        counts[key] = step_entries(tf, sd)
    total = {k: sum(v.values()) for k, v in counts.items()}
    assert total["plain"] == total["v"] == total["rescale"], total
    assert counts["plain"].get("tf_cfg_sampler_step_f32") == 1 and "tf_sampler_tail_f32" not in counts["plain"]      # the defaults call what they called
    for key in ("v", "rescale"):
        assert counts[key].get("tf_sampler_tail_f32") == 1 and "tf_cfg_sampler_step_f32" not in counts[key]


def test_v_prediction_composes_and_the_text_group_is_the_last_group(tf, data):
    from tinyfusers_amd import config
    from tinyfusers_amd.vision.unet import TINY_V2
    W, ctx, unc = data
    sch, Wf = _sched(), _f32(W)
    phi = np.float64(np.float32(0.7))
    # inpaint=True: the masked blend behind the v update
    from tinyfusers_amd.variants import samplers as S
    sch_i = S.DPMSolverPP2M().schedule(4, strength=0.7)
    rng = np.random.default_rng(3)
    x0 = rng.standard_normal(SHAPE).astype(np.float32)
    mask = (rng.random((2, 1, 16, 16)) < 0.5).astype(np.float32)
    sd, lat = _model(tf, data, sch_i, prediction="v", inpaint=True)
    lat0, got = _final(sd, lat, init_latent=x0, mask=mask)
    _gate(got, R.trajectory(Wf, TINY_V2, [unc, ctx], lat0, sch_i, G, vpred=True, x0_init=x0.astype(np.float64), mask=mask.astype(np.float64), noise2=_noise(2)))
    # cfg=False: one group
    sd, lat = _model(tf, data, sch, prediction="v", cfg=False)
    lat0, got = _final(sd, lat, guidance=None)
    _gate(got, R.trajectory(Wf, TINY_V2, [ctx], lat0, sch, 1.0, vpred=True))
    # pag=True, cfg_rescale=True: [uncond ; perturbed ; cond], the text group is group 2 (scale 3 on the middle block after compile)
    sd, lat = _model(tf, data, sch, prediction="v", pag=True, cfg_rescale=True)
    lat0, got = _final(sd, lat)
    ref = R.trajectory(Wf, TINY_V2, [unc, ctx, ctx], lat0, sch, np.float64(np.float32(G + 3.0)), vpred=True, phi=phi, g_i=G, perturb=[(), ("middle_block",), ()])
    _gate(got, ref)
    wrong = R.trajectory(Wf, TINY_V2, [unc, ctx, ctx], lat0, sch, np.float64(np.float32(G + 3.0)), vpred=True, phi=None, g_i=G, perturb=[(), ("middle_block",), ()])
    assert np.linalg.norm(got - wrong) > 5e-3 * np.linalg.norm(wrong)
    # ... and without CFG [perturbed ; cond]: the pair tail at guidance 1 + s
    sd, lat = _model(tf, data, sch, prediction="v", pag=True, cfg=False, cfg_rescale=True)
    lat0, got = _final(sd, lat, guidance=None)
    _gate(got, R.trajectory(Wf, TINY_V2, [ctx, ctx], lat0, sch, np.float64(np.float32(1.0 + 3.0)), vpred=True, phi=phi, perturb=[("middle_block",), ()]))
    # the bf16 step
    config.set_dtype("bf16")
    try:
        sd, lat = _model(tf, data, sch, prediction="v", cfg_rescale=True)
        lat0, got = _final(sd, lat)
        assert np.array_equal(got, _final(sd, lat, eager=True)[1])
    finally:
        config.set_dtype("fp16")
    _gate(got, R.trajectory(Wf, TINY_V2, [unc, ctx], lat0, sch, G, vpred=True, phi=phi), rel_l2=3e-2, max_rel=3e-2)


def test_sd21_size_one_captured_step(tf):
    from tinyfusers_amd.attention.sdpa import sdpa_instance
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import SD21
    sd = StableDiffusion(SD21)
    update_state(sd.model.diffusion_model, synth_state_dict(R.unet_shapes(SD21), 5), "")
    ctx = tf.DeviceArray.from_numpy(synth_normal(5, "c", (1, 77, 1024)).astype(np.float16))
    unc = tf.DeviceArray.from_numpy(synth_normal(5, "u", (1, 77, 1024)).astype(np.float16))
    lat = sd.latent_from_numpy(np.zeros((1, 4, 64, 64), np.float32))
    sd.compile(unc, ctx, lat, sampler=_sched(2), prediction="v", cfg_rescale=True)
    outs = []
    for eager in (False, True):
        sd.start(seed=SEED)
        sd.step_sampler(0, G, eager=eager); sd.synchronize()
        outs.append(lat.numpy().copy())
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1])
    kv_n = sd.model.diffusion_model._prepare()["kv_n"]
    for ch, side in ((320, 64), (640, 32), (1280, 16), (1280, 8)):
        nh, t = ch // 64, side * side
        assert sdpa_instance(np.float16, 2, nh, t, t, 64, 3 * ch, 3 * ch) != "generic", (ch, side)       # self-attention: q | k | v rows of 3 ch
        assert sdpa_instance(np.float16, 2, nh, t, 77, 64, kv_n, kv_n) != "generic", (ch, side)           # cross-attention: the hoisted K|V
        assert sdpa_instance(np.float16, 2, nh, t, t, 64, 3 * ch, 3 * ch).startswith("dma") and sdpa_instance(np.float16, 2, nh, t, 77, 64, kv_n, kv_n).startswith("dma")


# ---- the OpenCLIP text tower ---------------------------------------------------------------------------------------------------------------
def _text_gate(got, ref, bf16=False):
    """The gate tests/test_gpu_model.py holds the SD-1.5 text encoder to -- the UNet's: rel-L2 <= 5e-3, max |d| <= 1e-2 (1 + |ref|) -- and in the
    bfloat16 step the project's bf16 form of that gate, 3e-2 for both (tests/test_gpu_samplers.py, tests/test_gpu_bf16.py)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    rl2 = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    worst = float(np.max(np.abs(got - ref) / (1 + np.abs(ref))))
    print(f"text tower{' bf16' if bf16 else ''}: rel-L2 {rl2:.3e}, max |d| / (1 + |ref|) {worst:.3e}")
    assert np.isfinite(got).all() and rl2 <= (3e-2 if bf16 else 5e-3) and worst <= (3e-2 if bf16 else 1e-2), (rl2, worst)


def _ids(cfg, b, t, seed=0):
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, cfg.vocab - 2, (b, t))
    ids[:, 0] = cfg.vocab - 2
    for k in range(b):
        ids[k, t - 2 - 3 * k:] = 0                       # SD-2.x pads with id 0 ...
        ids[k, t - 3 - 3 * k] = cfg.vocab - 1            # ... behind the end-of-text token
    return ids


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_open_clip_text_tower_tiny(tf, dtype):
    from tinyfusers_amd import config
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.vae import open_clip_text as O
    cfg = O.OpenClipTextConfig(width=128, layers=3, heads=2, mlp=512, vocab=1000)
    st = O.synthetic_state(cfg, 1)
    config.set_dtype(dtype)
    try:
        tower = O.OpenClipText.load(st, heads=2)
        assert tower.cfg == cfg
        for t in (77, 13):
            ids = _ids(cfg, 2, t)
            got = tower(ids)
            assert got.shape == (2, t, 128)
            _text_gate(got.numpy(), R.text_tower(st, cfg, ids), dtype == "bf16")
        ids = _ids(cfg, 2, 13)
        base = tower(ids).numpy()
        # the last resblock, text_projection, logit_scale, attn_mask: read past without a word, never run
        poisoned = {"cond_stage_model.model." + k: (np.full_like(v, np.nan) if k.startswith("transformer.resblocks.2.") else v) for k, v in st.items()}
        poisoned.update({"cond_stage_model.model.text_projection": np.full((128, 64), np.nan, np.float32), "cond_stage_model.model.logit_scale": np.float32(np.nan),
                         "cond_stage_model.model.attn_mask": np.full((77, 77), np.nan, np.float32)})
        holder = type("M", (), {})()
        holder.cond_stage_model = O.OpenClipText(cfg)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            update_state(holder, poisoned, "")                                   # LDM naming through update_state ...
        assert "skipped" not in out.getvalue(), out.getvalue()
        assert np.array_equal(holder.cond_stage_model(ids).numpy(), base)        # ... equals OpenClipText.load bit for bit, NaNs and all
        assert np.array_equal(O.OpenClipText.load(poisoned, heads=2)(ids).numpy(), base)
    finally:
        config.set_dtype("fp16")


def test_open_clip_text_tower_full_width_layers(tf):
    from tinyfusers_amd.vae import open_clip_text as O
    cfg = O.OpenClipTextConfig(width=1024, layers=3, heads=16, mlp=4096, vocab=1000)      # two layers run: the real GEMM and attention shapes
    st = O.synthetic_state(cfg, 2)
    tower = O.OpenClipText.load(st)
    assert tower.cfg == cfg
    ids = _ids(cfg, 2, 77)
    _text_gate(tower(ids).numpy(), R.text_tower(st, cfg, ids))
