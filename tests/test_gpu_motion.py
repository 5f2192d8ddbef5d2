"""GPU checks of the AnimateDiff motion modules (vision/motion.py, UNetModel.__call__(motion=), StableDiffusion.compile(..., motion=True, frames=F),
set_motion_scale, start(motion_scale=)): one module against the float64 restatement of tests/aux/motion_ref.py at the bound tests/test_gpu_model.py
holds SpatialTransformer to (rtol 1e-2, atol 1.5e-2; bfloat16: x 8), its bit-for-bit properties, the loader on the device, a tiny UNet forward and
tiny sampler trajectories against the restatement at the trajectory gate (rel-L2 5e-3, max 1e-2), the refusals, and the SD-1.5 shapes end to end.
tests/test_motion_host.py shows on the CPU that every gate here would see a dropped positional table, swapped attentions, the UNet's head count or
GroupNorm's default eps."""
import contextlib
import ctypes
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))
import motion_ref as R  # noqa: E402
from test_motion_host import tiny_forward_refs  # noqa: E402
from test_samplers_host import randn_ref  # noqa: E402

SEED = 0x13198A2E03707344
G = 7.5
V, F = 2, 3
T = R.T


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T_
    T_.ensure_init(0)
    return T_


def _gate(got, ref, rel_l2=5e-3, max_rel=1e-2, what=""):
    """tests/test_gpu_freeu.py's gate: rel-L2 and max |d| <= max_rel max |ref|."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all()
    rl2 = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    mx = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"gate {what}: rel-L2 {rl2:.3e} (gate {rel_l2}), max|d|/max|ref| {mx:.3e} (gate {max_rel}), max|ref| {np.abs(ref).max():.2f}")
    assert rl2 <= rel_l2 and mx <= max_rel, (what, rl2, mx)


def _bound(got, ref, dtype, what):
    k = 8.0 if dtype == "bf16" else 1.0
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    u = np.abs(got - ref) / (k * (R.ATOL + R.RTOL * np.abs(ref)))
    print(f"module {what} {dtype}: max |err| {np.abs(got - ref).max():.3e}, {u.max():.3f} of the bound")
    assert np.isfinite(got).all() and u.max() <= 1.0, (what, dtype, float(u.max()))


@contextlib.contextmanager
def _dtype(dtype):
    from tinyfusers_amd import config
    config.set_dtype("bf16" if dtype == "bf16" else "fp16")
    try:
        yield
    finally:
        config.set_dtype("fp16")


def _np_dtype(tf, dtype):
    return tf.bfloat16 if dtype == "bf16" else np.float16


def _module(tf, C, max_len, W):
    """A MotionModule filled (in the current config dtype) from names below temporal_transformer."""
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.vision.motion import MotionModule
    m = MotionModule(C, max_len, init=False)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        update_state(m, W, "")
    assert "skipped" not in out.getvalue(), out.getvalue()
    return m


@functools.lru_cache(maxsize=None)
def _module_ref(case, dtype, eps_case=False, scale=1.0):
    """(weights, x, float64 restatement) on the 16-bit-rounded weights and input: computed once, shared, never written."""
    C, Fr, Vv, h, w, ml = case
    W = {k: R.round16(v, dtype) for k, v in R.module_weights(C, ml).items()}
    x = R.round16(R.eps_case_input() if eps_case else R.module_input(C, Fr, Vv, h, w), dtype)
    return W, x, R.motion_module_forward(x, W, Fr, scale=scale).numpy()


# ---- 1. one module against the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("case", R.MODULE_CASES + (R.EPS_CASE + ("eps",),), ids=lambda c: "C{}-F{}-V{}-{}x{}{}".format(*c[:5], "-eps" if len(c) == 7 else ""))
def test_module_matches_the_float64_restatement(tf, case, dtype):
    eps_case, case = len(case) == 7, tuple(case[:6])
    C, Fr, Vv, h, w, ml = case
    W, x, ref = _module_ref(case, dtype, eps_case)
    with _dtype(dtype):
        m = _module(tf, C, ml, W)
        got = m(tf.DeviceArray.from_numpy(x, _np_dtype(tf, dtype), "nhwc"), Fr).numpy()
    _bound(got, ref, dtype, f"C={C} F={Fr} V={Vv} {h}x{w}" + (" eps" if eps_case else ""))


def test_loader_installs_both_spellings_as_the_same_modules(tf):
    from tinyfusers_amd.storage.synth import synth_motion_state_dict
    from tinyfusers_amd.vision.motion import MotionAdapter
    from tinyfusers_amd.vision.unet import TINY
    Wm = synth_motion_state_dict(TINY, 3, max_len=24, mid=True)
    a, b = MotionAdapter.load(TINY, Wm), MotionAdapter.load(TINY, R.to_diffusers(Wm))
    assert a.max_len == b.max_len == 24 and a.mid and list(a.modules) == list(b.modules) and len(a.modules) == 16
    from tinyfusers_amd.storage.state import _slots
    for slot in a.modules:
        sa, sb = list(_slots(a.modules[slot])), list(_slots(b.modules[slot]))
        assert [n for n, *_ in sa] == [n for n, *_ in sb] and len([1 for _, _, _, cur, _ in sa if cur is not None]) == 28
        for (n, _, _, ca, _), (_, _, _, cb, _) in zip(sa, sb):
            if ca is not None:
                assert np.array_equal(ca.numpy(), cb.numpy()), (slot, n)
    mods = R.split_modules(Wm)
    got = a.modules["middle_block"].transformer_blocks[0].attention_blocks[1].pos_encoder.pe.numpy()
    assert np.array_equal(got, mods["mid_block.motion_modules.0"][f"{T}attention_blocks.1.pos_encoder.pe"].astype(np.float32))
    assert MotionAdapter.load(TINY, synth_motion_state_dict(TINY, 3, pe=False)).max_len == 32


# ---- 2. properties on the device ---------------------------------------------------------------------------------------------------------------------
def test_module_properties_bit_for_bit(tf):
    case = R.MODULE_CASES[0]
    C, Fr, Vv, h, w, ml = case
    W, x, ref = _module_ref(case, "fp16")
    dev = lambda a: tf.DeviceArray.from_numpy(a, np.float16, "nhwc")
    m = _module(tf, C, ml, W)
    y = m(dev(x), Fr).numpy()
    assert np.array_equal(m(dev(x), Fr).numpy(), y)                             # two runs agree
    for v in range(Vv):                                                          # the videos stay apart
        x2 = x.copy()
        x2[v * Fr:(v + 1) * Fr] = R.round16(x2[v * Fr:(v + 1) * Fr] + 1.0, "fp16")
        y2 = m(dev(x2), Fr).numpy()
        other = slice((1 - v) * Fr, (2 - v) * Fr)
        assert np.array_equal(y2[other], y[other]) and np.abs(y2[v * Fr:(v + 1) * Fr] - y[v * Fr:(v + 1) * Fr]).max() > 0.1
    m.set_scale(0.0)
    assert np.array_equal(m(dev(x), Fr).numpy(), x)                              # scale 0: x_in
    m.set_scale(0.5)
    _bound(m(dev(x), Fr).numpy(), _module_ref(case, "fp16", False, 0.5)[2], "fp16", "scale 0.5")
    m.set_scale(1.0)
    assert np.array_equal(m(dev(x), Fr).numpy(), y)                              # ... and back
    with pytest.raises(ValueError, match="finite float"):
        m.set_scale(float("nan"))
    W0 = dict(W); W0["proj_out.weight"] = np.zeros_like(W["proj_out.weight"]); W0["proj_out.bias"] = np.zeros_like(W["proj_out.bias"])
    assert np.array_equal(_module(tf, C, ml, W0)(dev(x), Fr).numpy(), x)         # proj_out = 0: x_in
    with pytest.raises(ValueError, match="videos of 4 frames"):
        m(dev(x), 4)
    with pytest.raises(ValueError, match="33 frames"):
        _module(tf, C, ml, W)(dev(np.zeros((33, C, 1, 1), np.float32)), 33)


# ---- 3. tiny UNet forward ----------------------------------------------------------------------------------------------------------------------------
def _tiny_unet(tf):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.vision.motion import MotionAdapter
    from tinyfusers_amd.vision.unet import TINY, UNetModel
    x, ctx, plain, moved, W, Wm = tiny_forward_refs()
    unet = UNetModel(TINY); update_state(unet, W, "")
    return unet, MotionAdapter.load(TINY, Wm)


def test_tiny_unet_forward_with_motion_modules(tf):
    from tinyfusers_amd.vision.unet import StepParams
    x, ctx, plain, moved, _, _ = tiny_forward_refs()
    unet, ad = _tiny_unet(tf)
    d_x, d_ctx = tf.DeviceArray.from_numpy(x, np.float16, "nhwc"), tf.DeviceArray.from_numpy(ctx)
    base = unet(d_x, StepParams().set(481.0), d_ctx).numpy()
    got = unet(d_x, StepParams().set(481.0), d_ctx, motion=(ad, F)).numpy()
    _gate(got, moved, what="tiny forward, motion")
    _gate(base, plain, what="tiny forward, motion=None")
    assert np.array_equal(unet(d_x, StepParams().set(481.0), d_ctx).numpy(), base)              # motion=None: the walk as it was, again
    with pytest.raises(ValueError, match="videos of 4 frames"):
        unet(d_x, StepParams().set(481.0), d_ctx, motion=(ad, 4))


# ---- 4. tiny sampler trajectories ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny():
    from tinyfusers_amd.storage.synth import synth_normal
    _, _, _, _, W, Wm = tiny_forward_refs()
    ctx = synth_normal(5, "motion.c", (V, 13, 64)).astype(np.float16).astype(np.float32)
    unc = synth_normal(5, "motion.u", (V, 13, 64)).astype(np.float16).astype(np.float32)
    return W, Wm, ctx, unc


def _f32(W):
    return {k: torch.from_numpy(v.astype(np.float32)) for k, v in W.items()}


def _oracle_trajectory(lat0, sch, cfg=True, scale=1.0, motion=True):
    """tests/test_gpu_freeu.py's sampler loop on the restatement with the motion modules; one prompt per video, broadcast to its frames."""
    import oracle
    W, Wm, ctx, unc = _tiny()
    Wf = _f32(W)
    mods = {p: {k: v.astype(np.float32) for k, v in m.items()} for p, m in R.split_modules(Wm).items()}
    x, xp = lat0.astype(np.float64), np.zeros(lat0.shape)
    B, n_img = lat0.shape[0], lat0[0].size
    cf, uf = np.repeat(ctx, F, axis=0), np.repeat(unc, F, axis=0)
    c2 = np.concatenate([uf, cf]) if cfg else cf
    for i, t in enumerate(sch.timesteps):
        x32 = x.astype(np.float32)
        xin = np.concatenate([x32, x32]) if cfg else x32
        out = R.unet_forward_motion(xin, np.array([t], np.float32), c2, Wf, oracle.TINY, motion=(mods, F, scale) if motion else None).numpy().astype(np.float64)
        e = out[:B] + G * (out[B:] - out[:B]) if cfg else out
        a_t = sch.alphas[i]
        x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
        z = np.stack([randn_ref(SEED, b, n_img, i, 1).reshape(lat0.shape[1:]) for b in range(B)])
        c_x, c_0, c_1, c_n = sch.coeffs[i]
        x, xp = c_x * x + c_0 * x0 + c_1 * xp + c_n * z, x0
    return x


def _model(tf, sch, motion=True, cfg=True, per_frame=False, attach=True, **kw):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.motion import MotionAdapter
    from tinyfusers_amd.vision.unet import TINY
    W, Wm, ctx, unc = _tiny()
    sd = StableDiffusion(TINY); update_state(sd.model.diffusion_model, W, "")
    if attach:
        sd.attach_motion(MotionAdapter.load(TINY, Wm))
    rows = (lambda a: np.repeat(a, F, axis=0)) if (per_frame or not motion) else (lambda a: a)
    lat = sd.latent_from_numpy(np.zeros((V * F, 4, 16, 16), np.float32))
    sd.compile(tf.DeviceArray.from_numpy(rows(unc)) if cfg else None, tf.DeviceArray.from_numpy(rows(ctx)), lat, sampler=sch, cfg=cfg,
               **(dict(motion=True, frames=F) if motion else {}), **kw)
    return sd, lat


def _final(sd, lat, eager=False, guidance=G, **kw):
    sd.start(seed=SEED, **kw)
    lat0 = lat.numpy().copy()
    sd.run(guidance, eager=eager); sd.synchronize()
    return lat0, lat.numpy().copy()


def _sched(n=3):
    from tinyfusers_amd.variants import samplers as S
    return S.DPMSolverPP2M().schedule(n)


@pytest.mark.parametrize("cfg,per_frame", [(True, False), (False, False), (True, True)], ids=["cfg-per-video", "nocfg-per-video", "cfg-per-frame"])
def test_tiny_motion_sampler_graph_eager_seed_and_restatement(tf, cfg, per_frame):
    sch = _sched()
    sd, lat = _model(tf, sch, cfg=cfg, per_frame=per_frame)
    g = G if cfg else None
    lat0, a = _final(sd, lat, guidance=g)
    _, b = _final(sd, lat, eager=True, guidance=g)
    _, c = _final(sd, lat, guidance=g)
    np.testing.assert_array_equal(a, b)                                       # graph replay == eager
    np.testing.assert_array_equal(a, c)                                       # same seed, same bits
    _gate(a, _oracle_trajectory(lat0, sch, cfg), what=f"dpmpp2m motion cfg={cfg} per_frame={per_frame}")
    assert (sd._ctx_vid is None) == per_frame and sd._kv_all.shape[0] == (2 if cfg else 1) * V * F


def test_set_motion_scale_keeps_the_graph_and_scale_zero_is_the_image_step(tf):
    """Scale 0 is within the gate of a motion=False compile on the same frames, not bit for bit: every module returns x_in's bits, but the GroupNorm
    statistics take another path -- the module's last launch emits those of ITS output for the consumer (from fp32 sums of the rounded x_in plus an
    exact zero), where the image step's consumer reads the statistics the ResBlock / SpatialTransformer in front emitted from its fp32 accumulators
    in front of the rounding -- and the block in front of a module emits plain 32-group statistics where it emitted concat sub-groups."""
    sch = _sched()
    sd, lat = _model(tf, sch)
    graph = sd._graph
    lat0, a = _final(sd, lat)
    sd.set_motion_scale(0.5)
    _, h = _final(sd, lat)
    assert sd._graph is graph and float(np.abs(h - a).max()) > 0.02
    fresh, flat = _model(tf, sch)
    fresh.set_motion_scale(0.5)
    np.testing.assert_array_equal(_final(fresh, flat)[1], h)                  # the bits of a fresh compile with that scale
    _gate(h, _oracle_trajectory(lat0, sch, scale=0.5), what="motion scale 0.5")
    _, z = _final(sd, lat, motion_scale=0.0)                                  # start(motion_scale=) writes what set_motion_scale writes
    assert sd._graph is graph
    plain, plat = _model(tf, sch, motion=False)
    _, p = _final(plain, plat)
    _gate(z, p, what="scale 0 vs a motion=False compile")
    _gate(z, _oracle_trajectory(lat0, sch, motion=False), what="scale 0 vs the plain restatement")
    assert float(np.abs(a - p).max()) > 0.02
    _, back = _final(sd, lat, motion_scale=[1.0] * 16)                        # one value per module
    np.testing.assert_array_equal(back, a)
    for bad in (float("nan"), [1.0, 2.0], "abc"):
        with pytest.raises(ValueError, match="one finite float or 16"):
            sd.set_motion_scale(bad)
        with pytest.raises(ValueError, match="one finite float or 16"):
            sd.start(seed=SEED, motion_scale=bad)
    np.testing.assert_array_equal(_final(sd, lat)[1], a)                      # the refusals wrote nothing
    with pytest.raises(ValueError, match="motion=True"):
        plain.set_motion_scale(0.5)
    with pytest.raises(ValueError, match="motion=True"):
        plain.start(seed=SEED, motion_scale=0.5)


def test_tiny_motion_sampler_in_the_bf16_step(tf):
    """Once in the bfloat16 step at 8 x the float16 gate (the ratio of the two types' unit roundoffs), as tests/test_gpu_freeu.py's bf16 step."""
    sch = _sched()
    with _dtype("bf16"):
        sd, lat = _model(tf, sch)
        lat0, a = _final(sd, lat)
        _, b = _final(sd, lat, eager=True)
        sd.set_motion_scale(0.5)
        _, h = _final(sd, lat)
    np.testing.assert_array_equal(a, b)
    _gate(a, _oracle_trajectory(lat0, sch), rel_l2=8 * 5e-3, max_rel=8 * 1e-2, what="bf16 motion")
    _gate(h, _oracle_trajectory(lat0, sch, scale=0.5), rel_l2=8 * 5e-3, max_rel=8 * 1e-2, what="bf16 motion, scale 0.5")


def test_motion_combines_with_v_prediction_rescale_and_img2img(tf):
    from tinyfusers_amd.variants import samplers as S
    sch = S.DPMSolverPP2M().schedule(3, strength=0.6)
    sd, lat = _model(tf, sch, prediction="v", cfg_rescale=True)
    init = np.random.default_rng(3).standard_normal((V * F, 4, 16, 16)).astype(np.float32)
    _, a = _final(sd, lat, init_latent=init)
    _, b = _final(sd, lat, eager=True, init_latent=init)
    assert np.isfinite(a).all() and np.array_equal(a, b)


# ---- 5. an attached adapter and motion=False ---------------------------------------------------------------------------------------------------------------
def _entries(sd, guidance=G):
    """The library's own count of one eager step: (GEMM-family launches, [GroupNorm, split-K reduce, LayerNorm, attention] launches)."""
    from tinyfusers_amd.native import hip, lib
    sd.start(seed=SEED); sd.synchronize()
    hip.tf_prof_enable(1)
    try:
        sd.step_sampler(0, guidance, eager=True); sd.synchronize()
        ms, fl, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        assert lib.tf_prof_read(ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(n)) == 0
        fam = []
        for f in (1, 2, 3, 4):
            w, k = ctypes.c_double(), ctypes.c_longlong()
            assert lib.tf_prof_read_family(f, ctypes.byref(ms), ctypes.byref(w), ctypes.byref(k)) == 0
            fam.append(k.value)
        return n.value, fam
    finally:
        hip.tf_prof_enable(0)


def test_an_attached_adapter_without_motion_is_the_image_step(tf):
    sch = _sched()
    never, nlat = _model(tf, sch, motion=False, attach=False)
    has, hlat = _model(tf, sch, motion=False, attach=True)
    np.testing.assert_array_equal(_final(never, nlat)[1], _final(has, hlat)[1])
    a, b = _entries(never), _entries(has)
    assert a == b and a[0] > 0, (a, b)
    video, _ = _model(tf, sch)
    c = _entries(video)
    print(f"TINY entries per step: image {a}, video {c}")
    assert c[0] == a[0] + 7 * 16 and c[1][3] == a[1][3] + 2 * 16 and c[1][2] == a[1][2], (a, c)
    has.detach_motion()
    with pytest.raises(ValueError, match="attach_motion"):
        has.compile(None, has._ctx, hlat, sampler=sch, motion=True, frames=F)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_raises_by_name_and_leaves_the_model_running(tf):
    from tinyfusers_amd import config
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_motion_state_dict
    from tinyfusers_amd.variants.samplers import UnsupportedSamplerConfig
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.controlnet import ControlNet
    from tinyfusers_amd.vision.motion import MotionAdapter
    from tinyfusers_amd.vision.unet import SD15, TINY, TINY_XL
    W, Wm, ctx, unc = _tiny()
    sch = _sched(2)
    sd, lat = _model(tf, sch)
    _, want = _final(sd, lat)
    d_ctx, d_unc = tf.DeviceArray.from_numpy(ctx), tf.DeviceArray.from_numpy(unc)
    new_lat = lambda n=V * F: StableDiffusion.latent_from_numpy(np.zeros((n, 4, 16, 16), np.float32))
    sd.attach_control(ControlNet(TINY))

    def refused(exc, match, **kw):
        args = dict(sampler=sch, motion=True, frames=F)
        args.update(kw)
        with pytest.raises(exc, match=match):
            sd.compile(d_unc, d_ctx, args.pop("latent", new_lat()), **args)
        assert np.array_equal(_final(sd, lat)[1], want)                       # ... and the model still runs its compiled step

    for kw, name in ((dict(control=True), "control=True"), (dict(ip_adapter=True), "ip_adapter=True"), (dict(pag=True), "pag=True"), (dict(freeu=True), "freeu=True"),
                     (dict(inpaint=True), "inpaint=True")):
        refused(UnsupportedSamplerConfig, f"motion=True and {name}", **kw)
    refused(UnsupportedSamplerConfig, "motion=True and concat='inpaint'", concat="inpaint")
    refused(ValueError, "motion=True needs a sampler", sampler=None)
    for bad in (None, 0, 25, 33, 2.0, True):
        refused(ValueError, "1 <= F <= 24", frames=bad)
    refused(ValueError, "no multiple of frames=4", frames=4)
    refused(ValueError, "one context row per frame", latent=new_lat(4 * F))
    with pytest.raises(ValueError, match="belongs to motion=True"):
        sd.compile(d_unc, d_ctx, new_lat(), sampler=sch, frames=F)
    assert np.array_equal(_final(sd, lat)[1], want)
    config.set_dtype("fp8")
    try:
        with pytest.raises(UnsupportedSamplerConfig, match="fp8 policy"):
            sd.compile(d_unc, d_ctx, new_lat(), sampler=sch, motion=True, frames=F)
    finally:
        config.set_dtype("fp16")
    assert np.array_equal(_final(sd, lat)[1], want)
    config.cfg_parallel = True
    try:
        with pytest.raises(UnsupportedSamplerConfig, match="TF_CFG_PARALLEL"):
            sd.compile(d_unc, d_ctx, new_lat(), sampler=sch, motion=True, frames=F)
    finally:
        config.cfg_parallel = False
    assert np.array_equal(_final(sd, lat)[1], want)
    with pytest.raises(TypeError, match="takes a MotionAdapter"):
        sd.attach_motion(object())
    with pytest.raises(ValueError, match="was built for"):
        sd.attach_motion(MotionAdapter(SD15))
    xl = StableDiffusion(TINY_XL)
    xl._motion_model = sd._motion_model                                       # (attach_motion refuses it by the configuration; compile by the model family)
    with pytest.raises(UnsupportedSamplerConfig, match="SDXL"):
        xl.compile(d_unc, d_ctx, new_lat(), sampler=sch, motion=True, frames=F)
    # a LoRA file with motion-module targets fails strict as any unknown target does
    key = "lora_unet_down_blocks_0_motion_modules_0_temporal_transformer_transformer_blocks_0_attention_blocks_0_to_q"
    lora = {key + ".lora_down.weight": np.zeros((4, 64), np.float16), key + ".lora_up.weight": np.zeros((64, 4), np.float16), key + ".alpha": np.float32(4.0)}
    with pytest.raises(ValueError, match="match no target of this model.*motion_modules"):
        sd.load_lora(lora, "motion-lora")
    assert np.array_equal(_final(sd, lat)[1], want)


def test_motion_with_a_lora_on_the_unet_recaptures_with_motion_remembered(tf):
    import lora_ref as LR
    from tinyfusers_amd.storage import lora as L
    from tinyfusers_amd.vision.unet import TINY, UNetModel
    W = _tiny()[0]
    sch = _sched(2)
    sd, lat = _model(tf, sch)
    _, base = _final(sd, lat)
    paths = L.unet_target_paths(UNetModel(TINY))
    sd.load_lora(LR.make_adapter({k: W[p + ".weight"] for k, p in paths.items()}, 4, 11), "A")
    graph = sd._graph
    sd.set_adapters(["A"])
    assert sd._graph is not graph and sd._motion and sd._compile_args["motion"] is True and sd._compile_args["frames"] == F
    _, a = _final(sd, lat)
    _, b = _final(sd, lat, eager=True)
    np.testing.assert_array_equal(a, b)
    assert float(np.abs(a - base).max()) > 1e-3
    sd.set_adapters([])
    np.testing.assert_array_equal(_final(sd, lat)[1], base)


# ---- 7. SD-1.5 shapes ------------------------------------------------------------------------------------------------------------------------------------------
def test_sd15_two_video_steps_of_16_frames(tf):
    """V = 1, F = 16 on a 16 x 16 latent: the d = 40 / 80 / 160 module shapes at F = 16.  The plan of DESIGN 4.3: per module 7 GEMM-family launches
    (proj_in with the GroupNorm inside, 2 x (q|k|v, to_out), GEGLU, ff.net[2] folded into proj_out) and 2 temporal attention launches -- 9 entries --
    and no LayerNorm launch; the module's GroupNorm costs a launch of its own only where its statistics could not ride (at most one per module)."""
    import oracle
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_motion_state_dict, synth_normal, synth_state_dict
    from tinyfusers_amd.variants.samplers import DPMSolverPP2M
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.motion import MotionAdapter
    from tinyfusers_amd.vision.unet import SD15
    sd = StableDiffusion(SD15)
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(sd.model.diffusion_model, synth_state_dict(oracle.unet_param_shapes(oracle.SD15), 0), "")
    sd.attach_motion(MotionAdapter.load(SD15, synth_motion_state_dict(SD15, 1, max_len=24)))
    ctx = tf.DeviceArray.from_numpy(synth_normal(1234, "sd.context", (1, 77, 768)))
    unc = tf.DeviceArray.from_numpy(synth_normal(1234, "sd.uncond", (1, 77, 768)))
    lat = sd.latent_from_numpy(np.zeros((16, 4, 16, 16), np.float32))
    sch = DPMSolverPP2M().schedule(2)
    sd.compile(unc, ctx, lat, sampler=sch, motion=True, frames=16)
    assert sorted({m.channels // 8 for m in sd._motion_compiled.module_list()}) == [40, 80, 160] and len(sd._motion_compiled.modules) == 20
    _, a = _final(sd, lat)
    _, b = _final(sd, lat, eager=True)
    _, c = _final(sd, lat)
    assert np.isfinite(a).all() and np.array_equal(a, b) and np.array_equal(a, c)
    video = _entries(sd)
    sd.set_motion_scale(0.0)
    _, z = _final(sd, lat)
    rows = lambda a: tf.DeviceArray.from_numpy(np.repeat(a.numpy(), 16, axis=0))    # (the image step reads one context row per image: no broadcast there)
    sd.compile(rows(unc), rows(ctx), lat, sampler=sch)                        # the image step of the same weights on the same 16 frames
    _, p = _final(sd, lat)
    image = _entries(sd)
    print(f"SD15 entries per step: image {image}, video {video}")
    assert np.isfinite(p).all() and float(np.abs(p - a).max()) > 1e-3 and float(np.abs(p - z).max()) < float(np.abs(p - a).max())
    assert video[0] == image[0] + 7 * 20 and video[1][3] == image[1][3] + 2 * 20 and video[1][2] == image[1][2], (image, video)
    assert image[1][0] <= video[1][0] <= image[1][0] + 20, (image, video)
