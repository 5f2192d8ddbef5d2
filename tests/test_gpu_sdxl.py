"""The SDXL path on the device, on TINY_XL (transformer depth 0 / 1 / 2, heads of 64, y = 64 pooled + 6 x 32 Fourier values), latent 16 x 16, B = 2:
the UNet with one time-embedding row per image, sampling through start(pooled=, ...) with the schedule's rows built in start, the two text towers with
the pooled vector, the launch count of the step, and the earlier configurations' results bit for bit against the parent commit's library -- against
tests/aux/sdxl_ref.py.  Gates: tests/test_gpu_samplers.py::_gate (rel-L2 5e-3, max 1e-2 relative; bf16 3e-2 both) and, for the towers,
tests/test_gpu_sd2.py::_text_gate.  Guidance 7.5, the scale the gate was set at (eps-prediction)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "aux"))

import sdxl_ref as X  # noqa: E402
from test_gpu_samplers import SEED, _gate  # noqa: E402
from test_gpu_sd2 import _ids, _text_gate  # noqa: E402

pytestmark = pytest.mark.gpu
G = 7.5
SHAPE = (2, 4, 16, 16)
# per image: original (h, w), crop (top, left), target (h, w) -- the two images differ in every id
SIZES = dict(original_size=[(128, 128), (512, 384)], crop_top_left=[(0, 0), (16, 48)], target_size=[(128, 128), (256, 192)])
IDS = np.array([[128, 128, 0, 0, 128, 128], [512, 384, 16, 48, 256, 192]], np.float64)
UNC_IDS = np.array([[128, 128, 0, 0, 128, 128], [64, 96, 8, 0, 128, 160]], np.float64)


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


@pytest.fixture(scope="module")
def data():
    """(UNet weights by LDM name, context, unconditional context, pooled, unconditional pooled, another pooled) of TINY_XL: computed once, never written."""
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.vision.unet import TINY_XL
    W = synth_state_dict(X.unet_shapes(TINY_XL), 5)
    f16 = lambda name, shape: synth_normal(5, name, shape).astype(np.float16).astype(np.float32)
    return dict(W=W, ctx=f16("c", (2, 13, 128)), unc=f16("u", (2, 13, 128)), pooled=f16("p", (2, 64)), unc_pooled=f16("q", (2, 64)), pooled2=f16("r", (2, 64)))


def _f32(W):
    import torch
    return {k: torch.from_numpy(v.astype(np.float32)) for k, v in W.items()}


def _sched(n=4):
    from tinyfusers_amd.variants import samplers as S
    return S.DPMSolverPP2M().schedule(n)


def _model(tf, data, sch, **modes):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY_XL
    sd = StableDiffusion(TINY_XL)
    update_state(sd.model.diffusion_model, data["W"], "")
    lat = sd.latent_from_numpy(np.zeros(SHAPE, np.float32))
    sd.compile(tf.DeviceArray.from_numpy(data["unc"]), tf.DeviceArray.from_numpy(data["ctx"]), lat, sampler=sch, **modes)
    return sd, lat


def _final(sd, lat, eager=False, guidance=G, **start):
    sd.start(seed=SEED, **start)
    lat0 = lat.numpy().copy()
    sd.run(guidance, eager=eager); sd.synchronize()
    return lat0, lat.numpy().copy()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_unet_forward_with_a_row_per_image(tf, data, dtype):
    from tinyfusers_amd import config
    from tinyfusers_amd.attention.attention import SpatialTransformer
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_normal
    from tinyfusers_amd.storage.tensor import bfloat16
    from tinyfusers_amd.vision.unet import TINY_XL, UNetModel
    W, ctx = data["W"], data["ctx"]
    x = synth_normal(7, "x", SHAPE).astype(np.float16).astype(np.float32)
    y = X.adm_vector(np.stack([data["unc_pooled"][0], data["pooled"][1]]), IDS, TINY_XL.adm_time_dim)       # the two images: other pooled vectors, other ids
    t = np.array([481.0], np.float32)
    ref = X.unet_forward(x, t, ctx, y, _f32(W), TINY_XL).numpy()
    wrong = X.unet_forward(x, t, ctx, np.stack([y[0], y[0]]), _f32(W), TINY_XL).numpy()                      # image 1 reading image 0's row
    config.set_dtype(dtype)
    try:
        dt = bfloat16 if dtype == "bf16" else np.float16
        unet = UNetModel(TINY_XL)
        update_state(unet, W, "")
        assert [len(st.transformer_blocks) for st in unet._all(SpatialTransformer)] == [1, 1, 2, 2, 2, 2, 2, 2, 1, 1, 1]
        assert [st.transformer_blocks[0].attn1.num_heads for st in unet._all(SpatialTransformer)] == [2] * 11
        bt = unet._prepare()
        assert bt["kv_n"] == 17 * 2 * 128 and len(bt["kv_off"]) == 17 and sorted(bt["kv_off"].values()) == [256 * i for i in range(17)]       # one slice per block
        y_emb = unet.label_embedding(tf.DeviceArray.from_numpy(y, dt))
        got = unet(tf.DeviceArray.from_numpy(x, dt, "nhwc"), 481.0, tf.DeviceArray.from_numpy(ctx, dt), y_emb=y_emb).numpy()
        with pytest.raises(ValueError, match="y_emb"):
            unet(tf.DeviceArray.from_numpy(x, dt, "nhwc"), 481.0, tf.DeviceArray.from_numpy(ctx, dt))
    finally:
        config.set_dtype("fp16")
    tol = 3e-2 if dtype == "bf16" else 5e-3
    _gate(got, ref, tol, 3e-2 if dtype == "bf16" else 1e-2)
    d = float(np.linalg.norm(got[1] - wrong[1]) / np.linalg.norm(wrong[1]))
    print(f"image 1 against the output with image 0's row: rel-L2 {d:.3e}")
    assert d > 4 * tol, d                                                        # far outside the gate: a stride-0 read of the rows fails here
    with pytest.raises(AssertionError):
        _gate(got, wrong, tol, 3e-2 if dtype == "bf16" else 1e-2)


def test_sampling_with_cfg_and_without(tf, data):
    from tinyfusers_amd.vision.unet import TINY_XL
    sch, Wf, D = _sched(), _f32(data["W"]), TINY_XL.adm_time_dim
    y_c, y_u = X.adm_vector(data["pooled"], IDS, D), X.adm_vector(data["unc_pooled"], UNC_IDS, D)
    start = dict(pooled=data["pooled"], uncond_pooled=data["unc_pooled"], uncond_size_ids=UNC_IDS, **SIZES)
    sd, lat = _model(tf, data, sch)
    outs = [_final(sd, lat, eager=e, **start) for e in (False, True, False)]
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][1], outs[2][1])          # graph == eager == graph again
    _gate(outs[0][1], X.trajectory(Wf, TINY_XL, [data["unc"], data["ctx"]], [y_u, y_c], outs[0][0], sch, G))
    # the defaults: zeros for the unconditional pooled vector, the conditional ids for the unconditional group, the latent's size x 8
    lat0, got = _final(sd, lat, pooled=data["pooled"])
    ids = np.array([[128, 128, 0, 0, 128, 128]] * 2, np.float64)
    _gate(got, X.trajectory(Wf, TINY_XL, [data["unc"], data["ctx"]], [X.adm_vector(np.zeros((2, 64)), ids, D), X.adm_vector(data["pooled"], ids, D)], lat0, sch, G))
    assert not np.array_equal(got, outs[0][1])
    # cfg=False: one group, the conditional rows alone
    sd, lat = _model(tf, data, sch, cfg=False)
    one = [_final(sd, lat, eager=e, guidance=None, pooled=data["pooled"], **SIZES) for e in (False, True)]
    assert np.array_equal(one[0][1], one[1][1])
    _gate(one[0][1], X.trajectory(Wf, TINY_XL, [data["ctx"]], [y_c], one[0][0], sch, 1.0))


def test_sdxl_composes_with_v_rescale_inpaint_and_bf16(tf, data):
    """The modes the SDXL step shares with the other families, through the tail that exists: prediction="v" + cfg_rescale=True + inpaint=True in one
    fp16 run, and the bf16 step.  Guidance 3.0 for v, as tests/test_gpu_sd2.py argues."""
    from tinyfusers_amd import config
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.vision.unet import TINY_XL
    from test_samplers_host import randn_ref
    Wf, D, g = _f32(data["W"]), TINY_XL.adm_time_dim, 3.0
    y_c, y_u = X.adm_vector(data["pooled"], IDS, D), X.adm_vector(data["unc_pooled"], IDS, D)
    start = dict(pooled=data["pooled"], uncond_pooled=data["unc_pooled"], **SIZES)
    sch_i = S.DPMSolverPP2M().schedule(4, strength=0.7)
    rng = np.random.default_rng(3)
    x0 = rng.standard_normal(SHAPE).astype(np.float32)
    mask = (rng.random((2, 1, 16, 16)) < 0.5).astype(np.float32)
    n = int(np.prod(SHAPE[1:]))
    noise2 = lambda i: np.stack([randn_ref(SEED, b, n, i, 2).reshape(SHAPE[1:]) for b in range(SHAPE[0])])
    sd, lat = _model(tf, data, sch_i, prediction="v", cfg_rescale=True, inpaint=True)
    outs = [_final(sd, lat, eager=e, guidance=g, init_latent=x0, mask=mask, **start) for e in (False, True)]
    assert np.array_equal(outs[0][1], outs[1][1])
    _gate(outs[0][1], X.trajectory(Wf, TINY_XL, [data["unc"], data["ctx"]], [y_u, y_c], outs[0][0], sch_i, g, vpred=True, phi=np.float64(np.float32(0.7)),
                                   x0_init=x0.astype(np.float64), mask=mask.astype(np.float64), noise2=noise2))
    sch = _sched()
    config.set_dtype("bf16")
    try:
        sd, lat = _model(tf, data, sch)
        lat0, got = _final(sd, lat, **start)
        assert np.array_equal(got, _final(sd, lat, eager=True, **start)[1])
    finally:
        config.set_dtype("fp16")
    _gate(got, X.trajectory(Wf, TINY_XL, [data["unc"], data["ctx"]], [y_u, y_c], lat0, sch, G), rel_l2=3e-2, max_rel=3e-2)
    # an ancestral sampler: the device noise of every step next to the rows of every step
    sd, lat = _model(tf, data, S.EulerAncestral().schedule(4))
    a, b = (_final(sd, lat, eager=e, **start)[1] for e in (False, True))
    assert np.isfinite(a).all() and np.array_equal(a, b)


def test_a_second_start_invalidates_the_rows(tf, data):
    sch = _sched()
    sd, lat = _model(tf, data, sch)
    first = _final(sd, lat, pooled=data["pooled"], uncond_pooled=data["unc_pooled"], **SIZES)[1]
    rows_before = sd._adm_table.numpy().copy()
    second = _final(sd, lat, pooled=data["pooled2"], uncond_pooled=data["unc_pooled"], **SIZES)[1]
    d = float(np.linalg.norm(second - first) / np.linalg.norm(first))
    print(f"another pooled vector: rel-L2 {d:.3e}")
    assert d > 5e-3 and not np.array_equal(sd._adm_table.numpy(), rows_before)
    fresh_sd, fresh_lat = _model(tf, data, sch)
    fresh = _final(fresh_sd, fresh_lat, pooled=data["pooled2"], uncond_pooled=data["unc_pooled"], **SIZES)[1]
    assert np.array_equal(second, fresh)                                          # nothing of the first start's table survived
    assert np.array_equal(_final(sd, lat, pooled=data["pooled"], uncond_pooled=data["unc_pooled"], **SIZES)[1], first)       # ... and back again
    # the table in one pass holds the bits of the row-by-row computation
    unet = sd.model.diffusion_model
    with tf.use_stream(sd._stream):
        rows = [unet.time_embedding_all(float(t), sd._y_emb)[1].numpy() for t in sch.timesteps]
    sd.synchronize()
    assert np.array_equal(sd._adm_table.numpy(), np.concatenate(rows))
    before = lat.numpy().copy()
    from tinyfusers_amd.variants.samplers import UnsupportedSamplerConfig
    with pytest.raises(UnsupportedSamplerConfig, match="pooled="):
        sd.start(seed=1)
    with pytest.raises(ValueError, match="pooled must be float"):
        sd.start(seed=1, pooled=np.zeros((2, 63), np.float32))
    assert np.array_equal(lat.numpy(), before)                                    # refused before anything was written


def test_the_step_has_the_plans_launches_and_none_for_the_conditioning(tf, data):
    sys.path.insert(0, os.path.dirname(HERE))
    from dataclasses import replace
    from tools.sampler_bench import step_entries
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY_XL
    sch = _sched()
    sd, lat = _model(tf, data, sch)
    sd.start(seed=SEED, pooled=data["pooled"])
    xl = step_entries(tf, sd)
    plain_cfg = replace(TINY_XL, adm_in_channels=None)                            # the same plan without label_emb: one (1, N) row, the stride-0 read
    plain = StableDiffusion(plain_cfg)
    update_state(plain.model.diffusion_model, {k: v for k, v in data["W"].items() if not k.startswith("label_emb.")}, "")
    plat = plain.latent_from_numpy(np.zeros(SHAPE, np.float32))
    plain.compile(tf.DeviceArray.from_numpy(data["unc"]), tf.DeviceArray.from_numpy(data["ctx"]), plat, sampler=sch)
    plain.start(seed=SEED)
    assert xl == step_entries(tf, plain), (xl, step_entries(tf, plain))           # entry for entry: everything y-dependent lives in start()
    blocks = 2 * 1 + 2 * 2 + 2 + 3 * 2 + 3 * 1                                    # TINY_XL's plan: 17 transformer blocks
    assert sum(v for k, v in xl.items() if k.startswith("tf_sdpa")) == 2 * blocks  # one self- and one cross-attention launch per block
    assert not any(k.startswith(("tf_adm", "tf_gemv", "tf_timestep", "tf_gather")) for k in xl), xl
    assert sd._emb_cur.shape == (4, sd.model.diffusion_model._prepare()["emb_w"].shape[0])       # G B rows travel in the parameter launch


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_both_towers_and_the_pooled_vector(tf, dtype):
    from tinyfusers_amd import config
    from tinyfusers_amd.storage.state import param_shapes, update_state
    from tinyfusers_amd.storage.synth import synth_normal
    from tinyfusers_amd.vae import open_clip_text as O
    from tinyfusers_amd.vae.encoder import CLIPTextTransformer
    cfg = O.OpenClipTextConfig(width=64, layers=3, heads=1, mlp=256, vocab=1000)
    st = O.synthetic_state(cfg, 1, pooled=True)
    ids = _ids(cfg, 2, 13)
    ids[1, 4] = cfg.vocab - 1; ids[1, 5:] = 0                                    # the end-of-text token in the middle of the row
    shape_l = dict(width=64, layers=3, heads=1, mlp=256, vocab=1000, positions=77)
    rng = np.random.default_rng(2)
    sl = {k: ((1.0 + 0.05 * rng.standard_normal(s)) if "layer_norm" in k and k.endswith("weight") else 0.05 * rng.standard_normal(s) if k.endswith("bias") or "embedding" in k
              else rng.standard_normal(s) * 0.7 / np.sqrt(s[-1])).astype(np.float16).astype(np.float32) for k, s in param_shapes(CLIPTextTransformer(init=False, **shape_l)).items()}
    ref_g, ref_pooled = X.big_g(st, cfg, ids)
    ref_l = X.clip_l_hidden(sl, ids, 64, 3, 1, 256, 1000)
    config.set_dtype(dtype)
    try:
        tower = O.OpenClipText(cfg, tap="penultimate_raw", pooled=True)
        update_state(tower.model, st, "")
        ctx, pooled = tower(ids)
        assert ctx.shape == (2, 13, 64) and pooled.shape == (2, 64)
        _text_gate(ctx.numpy(), ref_g, dtype == "bf16")
        _text_gate(pooled.numpy(), ref_pooled, dtype == "bf16")
        plain = O.OpenClipText(cfg)                                              # the SD-2.x tower on the same tensors: ln_final of what the raw tap returns
        update_state(plain.model, {k: v for k, v in st.items() if k in O.param_shapes(cfg)}, "")
        assert not np.array_equal(plain(ids).numpy(), ctx.numpy())
        clip_l = CLIPTextTransformer(init=False, tap=2, **shape_l)
        update_state(clip_l, sl, "")
        got_l = clip_l(ids)
        assert got_l.shape == (2, 13, 64)
        _text_gate(got_l.numpy(), ref_l, dtype == "bf16")
    finally:
        config.set_dtype("fp16")


@pytest.mark.parametrize("name", ["TINY", "TINY_V2"])
def test_earlier_configurations_compute_the_parents_bits(tf, name):
    """tests/golden/sdxl_parent_trajectories.npz: the 2-step DPM++2M result of ``X.parent_recipe`` run on the parent commit's library (on an MI355X,
    GEMM tiles from the cost model alone so that no run-time tuning enters).  The plan readers, the per-block K|V offsets and the stride rule of the
    time-embedding row must leave every launch of these configurations as it was."""
    golden = np.load(os.path.join(HERE, "golden", "sdxl_parent_trajectories.npz"))
    got = X.parent_recipe(name)
    assert np.array_equal(got, golden[name]), float(np.abs(got - golden[name]).max())
