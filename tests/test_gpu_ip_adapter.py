"""GPU checks of the IP-Adapter path (storage/ip_adapter.py, UNetModel.__call__(ip=), StableDiffusion.compile(..., ip_adapter=True),
start(ip_image_embeds=, ip_scale=), set_ip_scale) against the CPU restatement tests/aux/ip_adapter_ref.py.

The UNet is a small one of the TINY topology whose heads are 40 and 80 wide (model_channels 160, 4 heads, context 64, eleven cross-attentions):
the dual attention launch is built for the SD UNets' head sizes (40 / 80 / 160) and refuses the 32 / 64 of vision/unet.py::TINY.  Gates are the
project's stated ones: a UNet forward at rel-L2 <= 5e-3 and max |d| <= 1e-2 (1 + |ref|); trajectories at tests/test_gpu_controlnet.py::_gate."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "aux"))
import controlnet_oracle as C  # noqa: E402
import ip_adapter_ref as R  # noqa: E402
from test_gpu_controlnet import G, SEED, _f32, _gate  # noqa: E402
from test_samplers_host import randn_ref  # noqa: E402

SHAPE = dict(model_channels=160, channel_mult=(1, 2, 2), attention_levels=(0, 1), n_heads=4, context_dim=64)
E, T, B = 32, 4, 2


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T_
    T_.ensure_init(0)
    return T_


def _cfgs():
    import oracle
    from tinyfusers_amd.vision.unet import UNetConfig
    return UNetConfig(**SHAPE), oracle.UNetConfig(**SHAPE)


@functools.lru_cache(maxsize=None)
def _data(seed=5):
    import oracle
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    _, ocfg = _cfgs()
    W = synth_state_dict(oracle.unet_param_shapes(ocfg), seed)
    rng = np.random.default_rng(seed)
    A = {}
    for k, s in R.adapter_param_shapes(ocfg, T, E).items():
        a = rng.standard_normal(s) * (0.2 if k.startswith("ip_adapter.") else 0.1)
        A[k] = (a + 1.0 if k == "image_proj.norm.weight" else a).astype(np.float16)
    f16 = lambda a: a.astype(np.float16).astype(np.float32)
    ctx, unc = f16(synth_normal(seed, "c", (B, 13, 64))), f16(synth_normal(seed, "u", (B, 13, 64)))
    emb, emb2 = f16(synth_normal(seed, "e", (B, E))), f16(synth_normal(seed, "e2", (B, E)))
    return W, A, ctx, unc, emb, emb2


def _tokens_ref(emb):
    _, ocfg = _cfgs()
    return R.image_tokens(emb, _f32(_data()[1]), ocfg.context_dim)


def _oracle_trajectory(lat0, sch, emb=None, scale=1.0, cfg=True):
    """tests/test_gpu_controlnet.py's sampler loop on the restatement: the unconditional group reads tokens(0), the conditional group tokens(emb);
    emb None: the un-adapted UNet; cfg=False: the conditional group alone, e = its output."""
    import oracle
    _, ocfg = _cfgs()
    W, A, ctx, unc = _data()[:4]
    Wf, Af = _f32(W), _f32(A)
    x, xp = lat0.astype(np.float64), np.zeros(lat0.shape)
    n_img = lat0[0].size
    c2 = np.concatenate([unc, ctx]) if cfg else ctx
    if emb is not None:
        tok = torch.cat([_tokens_ref(np.zeros_like(emb)), _tokens_ref(emb)]) if cfg else _tokens_ref(emb)
    for i, t in enumerate(sch.timesteps):
        x32 = x.astype(np.float32)
        xin, tt = (np.concatenate([x32, x32]) if cfg else x32), np.array([t], np.float32)
        out = oracle.unet_forward(xin, tt, c2, Wf, ocfg) if emb is None else R.unet_forward(xin, tt, c2, Wf, Af, tok, scale, ocfg)
        out = out.numpy().astype(np.float64)
        e = out[:B] + G * (out[B:] - out[:B]) if cfg else out
        a_t = sch.alphas[i]
        x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
        z = np.stack([randn_ref(SEED, b, n_img, i, 1).reshape(lat0.shape[1:]) for b in range(B)])
        c_x, c_0, c_1, c_n = sch.coeffs[i]
        x, xp = c_x * x + c_0 * x0 + c_1 * xp + c_n * z, x0
    return x


def _adapter(unet, src=None):
    from tinyfusers_amd.storage.ip_adapter import IPAdapter
    return IPAdapter.load(unet, _data()[1] if src is None else src)


def _model(tf, sch, ip=True, src=None, cfg=True, **modes):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants.sd import StableDiffusion
    W, _, ctx, unc = _data()[:4]
    sd = StableDiffusion(_cfgs()[0]); update_state(sd.model.diffusion_model, W, "")
    if ip:
        sd.attach_ip_adapter(_adapter(sd.model.diffusion_model, src))
    if modes.get("control"):
        from tinyfusers_amd.storage.synth import synth_state_dict
        from tinyfusers_amd.vision.controlnet import ControlNet
        net = ControlNet(_cfgs()[0]); update_state(net, synth_state_dict(C.controlnet_param_shapes(_cfgs()[1]), 6), "")
        sd.attach_control(net)
    lat = sd.latent_from_numpy(np.zeros((B, 4, 16, 16), np.float32))
    sd.compile(tf.DeviceArray.from_numpy(unc) if cfg else None, tf.DeviceArray.from_numpy(ctx), lat, sampler=sch, cfg=cfg, ip_adapter=ip, **modes)
    return sd, lat


def _final(sd, lat, eager=False, guidance=G, **kw):
    sd.start(seed=SEED, **kw)
    lat0 = lat.numpy().copy()
    sd.run(guidance, eager=eager); sd.synchronize()
    return lat0, lat.numpy().copy()


def _sched(name="dpmpp2m", n=3):
    from tinyfusers_amd.variants import samplers as S
    return (S.LCM() if name == "lcm" else S.make(name)).schedule(n)


def test_tokens_context_kv_and_one_adapted_forward_match_the_restatement(tf):
    import oracle
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_normal
    from tinyfusers_amd.vision.unet import StepParams, UNetModel
    cfg, ocfg = _cfgs()
    W, A, ctx, unc, emb, _ = _data()
    unet = UNetModel(cfg); update_state(unet, W, "")
    ad = _adapter(unet)
    assert ad.num_tokens == T and ad.embed_dim == E and len(ad.paths) == 11 == len(R.paths(ocfg)) and ad.paths == R.paths(ocfg)
    tok = ad.tokens(tf.DeviceArray.from_numpy(emb, np.float16, "row"))
    ref_tok = _tokens_ref(emb)
    assert tok.shape == (B, T, 64)
    _gate(tok.numpy(), ref_tok.numpy(), what="image tokens")
    kv = ad.context_kv(tok)
    ref_kv = R.context_kv(tok.numpy(), _f32(A), ocfg)                       # (from the device's own 16-bit tokens)
    assert kv.shape == tuple(ref_kv.shape) == (B, T, ad.kv_layout()[1]) and ad.kv_layout()[1] == 2 * (5 * 160 + 6 * 320)
    _gate(kv.numpy(), ref_kv.numpy(), what="K_ip | V_ip")
    x = synth_normal(5, "lat", (B, 4, 16, 16)).astype(np.float16).astype(np.float32)
    t = np.array([481.0], np.float32)
    per = np.linspace(0.4, 1.5, 11).astype(np.float32)
    scales = tf.DeviceArray.from_numpy(np.concatenate([per, [1.0]]).astype(np.float32), np.float32, "row")
    d_x, d_ctx = tf.DeviceArray.from_numpy(x, np.float16, "nhwc"), tf.DeviceArray.from_numpy(ctx)
    got = unet(d_x, StepParams().set(481.0), d_ctx, ip=(ad, kv, scales)).numpy()
    ref = R.unet_forward(x, t, ctx, _f32(W), _f32(A), ref_tok, per, ocfg).numpy()
    rl2 = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    worst = float((np.abs(got - ref) / (1 + np.abs(ref))).max())
    print(f"\nadapted UNet forward: rel-L2 {rl2:.3e} (gate 5e-3), max |d|/(1+|ref|) {worst:.3e} (gate 1e-2)")
    assert np.isfinite(got).all() and rl2 <= 5e-3 and worst <= 1e-2
    plain = unet(d_x, StepParams().set(481.0), d_ctx).numpy()
    assert float(np.abs(got - plain).max()) > 0.02                          # (the adapter is no rounding error)
    zero = tf.DeviceArray.from_numpy(np.zeros(12, np.float32), np.float32, "row")
    assert np.array_equal(unet(d_x, StepParams().set(481.0), d_ctx, ip=(ad, kv, zero)).numpy(), plain)
    with pytest.raises(ValueError, match="do not fit"):
        unet(d_x, StepParams().set(481.0), d_ctx, ip=(ad, kv.view((1, T, kv.shape[2]), "row"), scales))


def test_adapted_sampler_graph_eager_seed_restatement_new_prompt_and_scales(tf):
    W, A, ctx, unc, emb, emb2 = _data()
    sch = _sched()
    sd, lat = _model(tf, sch)
    graph = sd._graph
    lat0, a = _final(sd, lat, ip_image_embeds=emb)
    _, b = _final(sd, lat, eager=True, ip_image_embeds=emb)
    _, c = _final(sd, lat, ip_image_embeds=emb)
    np.testing.assert_array_equal(a, b)                                     # graph replay == eager
    np.testing.assert_array_equal(a, c)                                     # same seed, same bits
    _gate(a, _oracle_trajectory(lat0, sch, emb), what="dpmpp2m adapted")
    # another image prompt (one row for both latents) at scale 0.5: no re-capture
    _, d = _final(sd, lat, ip_image_embeds=emb2[:1], ip_scale=0.5)
    assert sd._graph is graph
    _gate(d, _oracle_trajectory(lat0, sch, np.repeat(emb2[:1], B, 0), 0.5), what="second prompt, scale 0.5")
    assert float(np.abs(d - a).max()) > 0.02
    # set_ip_scale between start and run: the same values as start(ip_scale=)
    sd.start(seed=SEED, ip_image_embeds=emb2[:1]); sd.set_ip_scale(0.5); sd.run(G); sd.synchronize()
    assert sd._graph is graph
    np.testing.assert_array_equal(lat.numpy(), d)
    # one strength per cross-attention, one block at 0; the next start without ip_scale is back at 1
    per = np.linspace(0.3, 1.3, 11).astype(np.float32); per[4] = 0.0
    _, e = _final(sd, lat, ip_image_embeds=emb, ip_scale=per)
    _gate(e, _oracle_trajectory(lat0, sch, emb, per), what="per-block scales")
    _, f = _final(sd, lat, ip_image_embeds=emb)
    np.testing.assert_array_equal(f, a)
    # scale 0: the un-adapted model's trajectory, value for value
    _, z = _final(sd, lat, ip_image_embeds=emb, ip_scale=0)
    plain, plat = _model(tf, sch, ip=False)
    _, p = _final(plain, plat)
    np.testing.assert_array_equal(z, p)
    assert float(np.abs(a - p).max()) > 0.02


def test_adapted_lcm_step_without_guidance(tf):
    emb = _data()[4]
    sch = _sched("lcm")
    sd, lat = _model(tf, sch, cfg=False)
    lat0, a = _final(sd, lat, guidance=None, ip_image_embeds=emb)
    _, b = _final(sd, lat, eager=True, guidance=None, ip_image_embeds=emb)
    np.testing.assert_array_equal(a, b)
    _gate(a, _oracle_trajectory(lat0, sch, emb, cfg=False), what="lcm cfg=False adapted")
    _, z = _final(sd, lat, guidance=None, ip_image_embeds=emb, ip_scale=0.0)
    plain, plat = _model(tf, sch, ip=False, cfg=False)
    np.testing.assert_array_equal(z, _final(plain, plat, guidance=None)[1])


def test_an_adapter_file_drives_the_same_bits(tf, tmp_path):
    from tinyfusers_amd.storage.unpicker import save_safetensors
    A, emb = _data()[1], _data()[4]
    flat, nested = str(tmp_path / "ip.safetensors"), str(tmp_path / "ip.bin")
    save_safetensors(flat, A)
    torch.save({"image_proj": {k[11:]: torch.from_numpy(v.copy()) for k, v in A.items() if k.startswith("image_proj.")},
                "ip_adapter": {k[11:]: torch.from_numpy(v.copy()) for k, v in A.items() if k.startswith("ip_adapter.")}}, nested)
    sch = _sched()
    want = _final(*_model(tf, sch), ip_image_embeds=emb)[1]
    for src in (flat, nested):
        np.testing.assert_array_equal(_final(*_model(tf, sch, src=src), ip_image_embeds=emb)[1], want)


def test_composition_with_inpaint_control_and_a_lora(tf):
    """Each composed mode: graph == eager bit for bit, the adapter moves the result, and at scale 0 the composed trajectory is the un-adapted
    composed model's, value for value."""
    import lora_ref as LR
    from tinyfusers_amd.storage import lora as L
    from tinyfusers_amd.storage.synth import synth_normal
    from tinyfusers_amd.vision.unet import UNetModel
    W, A, ctx, unc, emb, _ = _data()
    sch = _sched()
    x0 = synth_normal(5, "x0", (B, 4, 16, 16))
    mask = np.zeros((B, 1, 16, 16), np.float32); mask[:, :, :, 8:] = 1.0
    img = np.random.default_rng(5).integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)
    for modes, kw in ((dict(inpaint=True), dict(init_latent=x0, mask=mask)), (dict(control=True), dict(control_image=img))):
        sd, lat = _model(tf, sch, **modes)
        _, a = _final(sd, lat, ip_image_embeds=emb, **kw)
        _, b = _final(sd, lat, eager=True, ip_image_embeds=emb, **kw)
        np.testing.assert_array_equal(a, b)
        _, z = _final(sd, lat, ip_image_embeds=emb, ip_scale=0.0, **kw)
        plain, plat = _model(tf, sch, ip=False, **modes)
        _, p = _final(plain, plat, **kw)
        np.testing.assert_array_equal(z, p)
        assert np.isfinite(a).all() and float(np.abs(a - p).max()) > 0.02, modes
    # LoRA: set_adapters on the compiled adapted model re-captures with ip_adapter=True still in force
    sd, lat = _model(tf, sch)
    _, base = _final(sd, lat, ip_image_embeds=emb)
    paths = L.unet_target_paths(UNetModel(_cfgs()[0]))
    lora = LR.make_adapter({k: W[p + ".weight"] for k, p in paths.items()}, 4, 11)
    sd.load_lora(lora, "A")
    graph = sd._graph
    sd.set_adapters(["A"])
    assert sd._graph is not graph and sd._ip and sd._compile_args["ip_adapter"] is True
    _, a = _final(sd, lat, ip_image_embeds=emb)
    _, b = _final(sd, lat, eager=True, ip_image_embeds=emb)
    np.testing.assert_array_equal(a, b)
    _, z = _final(sd, lat, ip_image_embeds=emb, ip_scale=0.0)
    assert float(np.abs(a - base).max()) > 1e-3 and float(np.abs(a - z).max()) > 0.02      # the LoRA moved it; the adapter is still acting
    sd.set_adapters([])
    np.testing.assert_array_equal(_final(sd, lat, ip_image_embeds=emb)[1], base)


def test_an_adapted_step_books_the_plain_step_s_attention_launches(tf):
    from tinyfusers_amd.native import hip, lib
    emb, sch, counts = _data()[4], _sched(), []
    for ip in (False, True):
        sd, lat = _model(tf, sch, ip=ip)
        sd.start(seed=SEED, **(dict(ip_image_embeds=emb) if ip else {}))
        sd.synchronize()
        hip.tf_prof_enable(1)
        try:
            sd.step_sampler(0, G, eager=True); sd.synchronize()
            ms, work, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
            assert lib.tf_prof_read_family(4, ctypes.byref(ms), ctypes.byref(work), ctypes.byref(n)) == 0
            counts.append((n.value, work.value))
        finally:
            hip.tf_prof_enable(0)
    assert counts[0][0] == counts[1][0] == 22 and counts[1][1] > counts[0][1], counts      # 11 self- + 11 cross-attentions either way; more FLOPs


def test_start_and_compile_refusals_leave_the_model_running(tf):
    from tinyfusers_amd.storage.ip_adapter import IPAdapter
    from tinyfusers_amd.variants.samplers import UnsupportedSamplerConfig
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY, UNetModel
    emb, sch = _data()[4], _sched()
    sd, lat = _model(tf, sch)
    _, a = _final(sd, lat, ip_image_embeds=emb)
    before = lat.numpy().copy()
    for kw, exc, match in ((dict(), ValueError, "pass ip_image_embeds="), (dict(ip_image_embeds=emb[:, :8]), ValueError, "ip_image_embeds must be"),
                           (dict(ip_image_embeds=emb, ip_scale=np.ones(3)), ValueError, "ip_scale"),
                           (dict(ip_image=np.zeros((B, 224, 224, 3), np.uint8)), UnsupportedSamplerConfig, "CLIP vision tower"),
                           (dict(ip_image_embeds=emb, control_image=np.zeros((B, 128, 128, 3), np.uint8)), ValueError, "control=True")):
        with pytest.raises(exc, match=match):
            sd.start(seed=SEED + 1, **kw)
    np.testing.assert_array_equal(lat.numpy(), before)                      # nothing was written
    np.testing.assert_array_equal(_final(sd, lat, ip_image_embeds=emb)[1], a)
    plain, _ = _model(tf, sch, ip=False)
    with pytest.raises(ValueError, match="ip_adapter=True"):
        plain.start(seed=SEED, ip_image_embeds=emb)
    with pytest.raises(ValueError, match="ip_adapter=True"):
        plain.set_ip_scale(0.5)
    with pytest.raises(ValueError, match="attach_ip_adapter"):
        plain.compile(None, None, lat, sampler=sch, ip_adapter=True)
    with pytest.raises(TypeError, match="IPAdapter"):
        plain.attach_ip_adapter(object())
    with pytest.raises(ValueError, match="another UNet"):
        plain.attach_ip_adapter(IPAdapter(UNetModel(TINY), T, E))
    sd.detach_ip_adapter()
    assert sd._ip_model is None
    np.testing.assert_array_equal(_final(sd, lat, ip_image_embeds=emb)[1], a)      # the compiled step keeps the adapter it captured


def test_sd15_size_one_captured_step(tf):
    import oracle
    from tinyfusers_amd.storage.ip_adapter import IPAdapter
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import SD15
    sd = StableDiffusion(SD15)
    update_state(sd.model.diffusion_model, synth_state_dict(oracle.unet_param_shapes(oracle.SD15), 5), "")
    rng = np.random.default_rng(2)
    A = {k: (rng.standard_normal(s) * (0.03 if "ip_adapter" in k or "proj" in k else 0.1) + (1.0 if k == "image_proj.norm.weight" else 0.0)).astype(np.float16)
         for k, s in R.adapter_param_shapes(oracle.SD15, 4, 1024).items()}
    ad = IPAdapter.load(sd.model.diffusion_model, A)
    assert [(n, p) for n, p in ad.paths] == R.SD15_PATHS
    sd.attach_ip_adapter(ad)
    ctx = tf.DeviceArray.from_numpy(synth_normal(5, "c", (1, 77, 768)).astype(np.float16))
    unc = tf.DeviceArray.from_numpy(synth_normal(5, "u", (1, 77, 768)).astype(np.float16))
    lat = sd.latent_from_numpy(np.zeros((1, 4, 64, 64), np.float32))
    sd.compile(unc, ctx, lat, sampler=_sched(n=2), ip_adapter=True)
    emb = synth_normal(5, "e", (1, 1024))
    outs = []
    for s in (1.0, 1.0, 0.0):
        sd.start(seed=SEED, ip_image_embeds=emb, ip_scale=s)
        sd.step_sampler(0, G); sd.synchronize()
        outs.append(lat.numpy().copy())
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])
