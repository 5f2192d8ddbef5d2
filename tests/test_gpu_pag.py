"""GPU checks of perturbed-attention guidance through the model (UNetModel.__call__(pag=), StableDiffusion.compile(..., pag=True), set_pag,
start(pag=)) against the CPU restatement tests/aux/pag_ref.py, on tests/test_gpu_ip_adapter.py's small UNet (heads 40 and 80 wide; weights,
contexts and seed: tests/test_pag_host.py::data, where the restatement's perturbed branch is shown to differ from the conditional one by 10 x
these gates).  Gates are the project's stated ones: a UNet forward at rel-L2 <= 5e-3 and max |d| <= 1e-2 (1 + |ref|); trajectories at
tests/test_gpu_controlnet.py::_gate (rel-L2 5e-3, max 1e-2)."""
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
import pag_ref as PR  # noqa: E402
import test_pag_host as H  # noqa: E402
from test_gpu_controlnet import G, SEED, _f32, _gate  # noqa: E402
from test_pag_host import B, TRAJ_BLOCKS, TRAJ_LAYERS  # noqa: E402
from test_samplers_host import randn_ref  # noqa: E402


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T_
    T_.ensure_init(0)
    return T_


def _sched(name="dpmpp2m", n=3):
    from tinyfusers_amd.variants import samplers as S
    return (S.LCM() if name == "lcm" else S.make(name)).schedule(n)


@functools.lru_cache(maxsize=None)
def _ref_trajectory(name, blocks, s, a=0.0, cfg=True, pag=True):
    """tests/test_gpu_controlnet.py's sampler loop on the restatement from the seed's own initial latent: e_u and e_c from oracle.unet_forward's
    restatement, e_p with ``blocks`` perturbed, the float64 combine.  pag=False: the CFG (or guidance-free) trajectory.  -> (lat0, final latent)."""
    sch = _sched(name)
    W, ctx, unc, _ = H.data()
    Wf, ocfg = _f32(W), H.cfgs()[1]
    n_img = 4 * 16 * 16
    lat0 = np.stack([randn_ref(SEED, b, n_img, 0, 0).reshape(4, 16, 16) for b in range(B)]).astype(np.float32)
    x, xp = lat0.astype(np.float64), np.zeros(lat0.shape)
    for i, t in enumerate(sch.timesteps):
        x32, tt = x.astype(np.float32), np.array([t], np.float32)
        e_c = PR.unet_forward(x32, tt, ctx, Wf, (), ocfg).numpy().astype(np.float64)
        e_u = PR.unet_forward(x32, tt, unc, Wf, (), ocfg).numpy().astype(np.float64) if cfg else None
        if pag:
            e = PR.combine(e_u, PR.unet_forward(x32, tt, ctx, Wf, blocks, ocfg).numpy(), e_c, G, PR.scale_at(s, a, t))
        else:
            e = e_u + G * (e_c - e_u) if cfg else e_c
        a_t = sch.alphas[i]
        x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
        z = np.stack([randn_ref(SEED, b, n_img, i, 1).reshape(lat0.shape[1:]) for b in range(B)])
        c_x, c_0, c_1, c_n = sch.coeffs[i]
        x, xp = c_x * x + c_0 * x0 + c_1 * xp + c_n * z, x0
    return lat0, x


def _model(tf, sch, cfg=True, pag=True, ip=False, **modes):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants.sd import StableDiffusion
    W, ctx, unc, _ = H.data()
    sd = StableDiffusion(H.cfgs()[0]); update_state(sd.model.diffusion_model, W, "")
    if ip:
        import test_gpu_ip_adapter as IP
        sd.attach_ip_adapter(IP._adapter(sd.model.diffusion_model))
    if modes.get("control"):
        from tinyfusers_amd.storage.synth import synth_state_dict
        from tinyfusers_amd.vision.controlnet import ControlNet
        net = ControlNet(H.cfgs()[0]); update_state(net, synth_state_dict(C.controlnet_param_shapes(H.cfgs()[1]), 6), "")
        sd.attach_control(net)
    lat = sd.latent_from_numpy(np.zeros((B, 4, 16, 16), np.float32))
    sd.compile(tf.DeviceArray.from_numpy(unc) if cfg else None, tf.DeviceArray.from_numpy(ctx), lat, sampler=sch, cfg=cfg, pag=pag, ip_adapter=ip, **modes)
    return sd, lat


def _final(sd, lat, eager=False, guidance=G, **kw):
    sd.start(seed=SEED, **kw)
    lat0 = lat.numpy().copy()
    sd.run(guidance, eager=eager); sd.synchronize()
    return lat0, lat.numpy().copy()


def test_one_pag_forward_matches_the_restatement_and_no_layer_is_the_conditional_branch(tf):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.vision.unet import PAG_WORDS, StepParams, UNetModel, pag_layers
    from tinyfusers_amd.variants import inputs
    cfg, ocfg = H.cfgs()
    W, ctx, unc, x = H.data()
    unet = UNetModel(cfg); update_state(unet, W, "")
    table = pag_layers(cfg)
    d_x = tf.DeviceArray.from_numpy(np.concatenate([x, x, x]), np.float16, "nhwc")
    d_ctx = tf.DeviceArray.from_numpy(np.concatenate([unc, ctx, ctx]))
    e_u, e_c = H.ref_forward((), H.T0, True), H.ref_forward(())
    plain = unet(d_x, StepParams().set(H.T0), d_ctx).numpy()
    for layers, blocks in (("mid", ("middle_block",)), ("all", tuple(table))):
        flags = tf.DeviceArray.from_numpy(inputs.pag_layer_words(layers, table), np.float32, "row")
        got = unet(d_x, StepParams().set(H.T0), d_ctx, pag=(flags, (B, 2 * B))).numpy()
        for name, g, ref in (("e_u", got[:B], e_u), ("e_p", got[B:2 * B], H.ref_forward(blocks)), ("e_c", got[2 * B:], e_c)):
            rl2 = float(np.linalg.norm(g - ref) / np.linalg.norm(ref))
            worst = float((np.abs(g - ref) / (1 + np.abs(ref))).max())
            print(f"\nPAG forward, layers {layers}, {name}: rel-L2 {rl2:.3e} (gate 5e-3), max |d|/(1+|ref|) {worst:.3e} (gate 1e-2)")
            assert np.isfinite(g).all() and rl2 <= 5e-3 and worst <= 1e-2, (layers, name, rl2, worst)
        assert np.array_equal(got[:B], plain[:B]) and np.array_equal(got[2 * B:], plain[2 * B:])      # the other groups: the plain launch's bits
        assert float(np.abs(got[B:2 * B] - got[2 * B:]).max()) > 0.02                                   # (the perturbation is no rounding error)
    # no layer selected: e_p == e_c bit for bit, and the whole call is the plain one
    none = tf.DeviceArray.from_numpy(np.zeros(PAG_WORDS, np.float32), np.float32, "row")
    got = unet(d_x, StepParams().set(H.T0), d_ctx, pag=(none, (B, 2 * B))).numpy()
    assert np.array_equal(got[B:2 * B], got[2 * B:]) and np.array_equal(got, plain)
    with pytest.raises(ValueError, match="do not fit"):
        unet(d_x, StepParams().set(H.T0), d_ctx, pag=(none, (2 * B, 4 * B)))
    with pytest.raises(ValueError, match="self-attention"):
        st = unet.middle_block[1].transformer_blocks[0]
        st.attn2(tf.DeviceArray.from_numpy(np.zeros((1, 4, st.attn2.num_heads * st.attn2.head_size), np.float16)), context=d_ctx, pag=(none.ptr, (0, 1)))


def test_pag_sampler_graph_eager_restatement_and_changes_without_a_recapture(tf):
    sch = _sched()
    sd, lat = _model(tf, sch)
    graph = sd._graph
    lat0, a = _final(sd, lat, pag=(3.0, TRAJ_LAYERS))
    _, b = _final(sd, lat, eager=True, pag=(3.0, TRAJ_LAYERS))
    _, c = _final(sd, lat)                                                   # (the values stay until the next set_pag / start(pag=))
    np.testing.assert_array_equal(a, b)                                      # graph replay == eager
    np.testing.assert_array_equal(a, c)
    ref0, ref = _ref_trajectory("dpmpp2m", TRAJ_BLOCKS, 3.0)
    np.testing.assert_allclose(lat0, ref0, rtol=0, atol=2e-5)
    _gate(a, ref, what="dpmpp2m pag 3.0 on mid + output_blocks.3")
    # other layers, another scale and an adaptive scale that clips the last step's s_t to 0: no re-capture, the restatement's trajectory
    adaptive = 2.5 / (1000.0 - sch.timesteps[1])                             # s_t: > 0 at step 0, 0 from step 1 on
    assert PR.scale_at(2.5, adaptive, sch.timesteps[0]) > 0.5 and PR.scale_at(2.5, adaptive, sch.timesteps[2]) == 0.0
    _, d = _final(sd, lat, pag=(2.5, ["mid", 3, "output_blocks.8"], adaptive))
    assert sd._graph is graph
    _gate(d, _ref_trajectory("dpmpp2m", ("middle_block", "input_blocks.5", "output_blocks.8"), 2.5, adaptive)[1], what="pag 2.5, three layers, adaptive")
    assert float(np.abs(d - a).max()) > 0.02
    # set_pag between start and run: the same bits as start(pag=)
    sd.start(seed=SEED); sd.set_pag(3.0, TRAJ_LAYERS); sd.run(G); sd.synchronize()
    assert sd._graph is graph
    np.testing.assert_array_equal(lat.numpy(), a)
    # no layer selected: e_p == e_c bit for bit, so the scale drops out of e = e_u + g (e_c - e_u) + s (e_c - e_p) exactly
    _, n3 = _final(sd, lat, pag=(3.0, []))
    _, n9 = _final(sd, lat, pag=(9.0, []))
    np.testing.assert_array_equal(n3, n9)
    # scale 0: the pag=False trajectory within the gate (the three-group tail rounds differently)
    _, z = _final(sd, lat, pag=(0.0, TRAJ_LAYERS))
    plain, plat = _model(tf, sch, pag=False)
    _, p = _final(plain, plat)
    _gate(z, p, what="scale 0 against pag=False")
    _gate(n3, p, what="no layer against pag=False")
    _gate(p, _ref_trajectory("dpmpp2m", (), 0.0, pag=False)[1], what="pag=False against the restatement")
    assert float(np.abs(a - p).max()) > 0.02


def test_pag_without_cfg_on_the_lcm_step(tf):
    sch = _sched("lcm")
    sd, lat = _model(tf, sch, cfg=False)
    assert sd._groups == 2
    _, a = _final(sd, lat, guidance=None, pag=(3.0, TRAJ_LAYERS))
    _, b = _final(sd, lat, eager=True, guidance=None, pag=(3.0, TRAJ_LAYERS))
    np.testing.assert_array_equal(a, b)
    _gate(a, _ref_trajectory("lcm", TRAJ_BLOCKS, 3.0, cfg=False)[1], what="lcm cfg=False pag 3.0")
    _, z = _final(sd, lat, guidance=None, pag=(0.0, TRAJ_LAYERS))
    plain, plat = _model(tf, sch, cfg=False, pag=False)
    _, p = _final(plain, plat, guidance=None)
    _gate(z, p, what="lcm cfg=False scale 0 against pag=False")
    assert float(np.abs(a - p).max()) > 0.02
    with pytest.raises(ValueError, match="cfg=False"):
        sd.run(7.5)


def test_composition_with_inpaint_control_a_lora_and_an_ip_adapter(tf):
    """Each composed mode: graph == eager bit for bit, PAG moves the result, and at scale 0 the composed trajectory is the composed pag=False
    model's within the gate."""
    import lora_ref as LR
    import test_gpu_ip_adapter as IP
    from tinyfusers_amd.storage import lora as L
    from tinyfusers_amd.storage.synth import synth_normal
    from tinyfusers_amd.vision.unet import UNetModel
    W = H.data()[0]
    sch = _sched()
    x0 = synth_normal(5, "x0", (B, 4, 16, 16))
    mask = np.zeros((B, 1, 16, 16), np.float32); mask[:, :, :, 8:] = 1.0
    img = np.random.default_rng(5).integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)
    emb = IP._data()[4]
    for modes, kw in ((dict(inpaint=True), dict(init_latent=x0, mask=mask)), (dict(control=True), dict(control_image=img)), (dict(ip=True), dict(ip_image_embeds=emb)),
                      (dict(inpaint=True, cfg=False), dict(init_latent=x0, mask=mask))):
        g = None if modes.get("cfg") is False else G
        sd, lat = _model(tf, sch, **modes)
        _, a = _final(sd, lat, guidance=g, pag=(3.0, TRAJ_LAYERS), **kw)
        _, b = _final(sd, lat, eager=True, guidance=g, pag=(3.0, TRAJ_LAYERS), **kw)
        np.testing.assert_array_equal(a, b)
        _, z = _final(sd, lat, guidance=g, pag=(0.0, TRAJ_LAYERS), **kw)
        plain, plat = _model(tf, sch, pag=False, **modes)
        _, p = _final(plain, plat, guidance=g, **kw)
        _gate(z, p, what=f"{modes}: scale 0 against pag=False")
        assert np.isfinite(a).all() and float(np.abs(a - p).max()) > 0.02, modes
    # LoRA: set_adapters on the compiled PAG model re-captures with pag=True still in force (scale and layers back at compile's 3.0 / "mid")
    sd, lat = _model(tf, sch)
    _, base = _final(sd, lat, pag=(3.0, TRAJ_LAYERS))
    paths = L.unet_target_paths(UNetModel(H.cfgs()[0]))
    lora = LR.make_adapter({k: W[p + ".weight"] for k, p in paths.items()}, 4, 11)
    sd.load_lora(lora, "A")
    graph = sd._graph
    sd.set_adapters(["A"])
    assert sd._graph is not graph and sd._pag and sd._compile_args["pag"] is True and sd._groups == 3
    _, a = _final(sd, lat, pag=(3.0, TRAJ_LAYERS))
    _, b = _final(sd, lat, eager=True, pag=(3.0, TRAJ_LAYERS))
    np.testing.assert_array_equal(a, b)
    _, z = _final(sd, lat, pag=(0.0, TRAJ_LAYERS))
    assert float(np.abs(a - base).max()) > 1e-3 and float(np.abs(a - z).max()) > 0.02       # the LoRA moved it; PAG is still acting
    sd.set_adapters([])
    np.testing.assert_array_equal(_final(sd, lat, pag=(3.0, TRAJ_LAYERS))[1], base)


def test_a_pag_step_books_the_plain_step_s_attention_launches(tf):
    from tinyfusers_amd.native import hip, lib
    sch, counts = _sched(), []
    for pag in (False, True):
        sd, lat = _model(tf, sch, pag=pag)
        sd.start(seed=SEED, **(dict(pag=(3.0, "all")) if pag else {}))
        sd.synchronize()
        hip.tf_prof_enable(1)
        try:
            sd.step_sampler(0, G, eager=True); sd.synchronize()
            ms, work, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
            assert lib.tf_prof_read_family(4, ctypes.byref(ms), ctypes.byref(work), ctypes.byref(n)) == 0
            counts.append((n.value, work.value))
        finally:
            hip.tf_prof_enable(0)
    assert counts[0][0] == counts[1][0] == 22, counts                       # 11 self- + 11 cross-attentions either way
    assert abs(counts[1][1] / counts[0][1] - 1.5) < 1e-9, counts            # three guidance groups instead of two


def test_start_and_compile_refusals_leave_the_model_running(tf):
    from tinyfusers_amd.variants.samplers import UnsupportedSamplerConfig
    sch = _sched()
    sd, lat = _model(tf, sch)
    _, a = _final(sd, lat, pag=(3.0, TRAJ_LAYERS))
    before = lat.numpy().copy()
    flags = sd._pag_flags.numpy().copy()
    for kw, match in ((dict(pag=(3.0, "middle")), "names no SpatialTransformer"), (dict(pag=(3.0, 11)), "names no SpatialTransformer"),
                      (dict(pag=(3.0, ["mid", "input_blocks.3"])), "names no SpatialTransformer"), (dict(pag=(-1.0, "mid")), "finite floats >= 0"),
                      (dict(pag=(3.0, "mid", float("nan"))), "finite floats >= 0"), (dict(pag=3.0), r"\(scale, layers\)"), (dict(pag=(3.0,)), r"\(scale, layers\)")):
        with pytest.raises(ValueError, match=match):
            sd.start(seed=SEED + 1, **kw)
    with pytest.raises(ValueError, match="names no SpatialTransformer"):
        sd.set_pag(3.0, "everything")
    np.testing.assert_array_equal(lat.numpy(), before)                      # nothing was written
    np.testing.assert_array_equal(sd._pag_flags.numpy(), flags)
    np.testing.assert_array_equal(_final(sd, lat)[1], a)
    plain, plat = _model(tf, sch, pag=False)
    with pytest.raises(ValueError, match="pag=True"):
        plain.start(seed=SEED, pag=(3.0, "mid"))
    with pytest.raises(ValueError, match="pag=True"):
        plain.set_pag(3.0)
    with pytest.raises(ValueError, match="warmup >= 1"):
        plain.compile(None, None, plat, sampler=sch, pag=True, warmup=0)
    with pytest.raises(ValueError, match="fourth"):
        plain.compile(None, None, plat, sampler=sch, pag=True, concat="edit")
    np.testing.assert_array_equal(_final(sd, lat)[1], a)


def test_sd15_size_one_captured_step(tf):
    import oracle
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import SD15
    sd = StableDiffusion(SD15)
    update_state(sd.model.diffusion_model, synth_state_dict(oracle.unet_param_shapes(oracle.SD15), 5), "")
    ctx = tf.DeviceArray.from_numpy(synth_normal(5, "c", (1, 77, 768)).astype(np.float16))
    unc = tf.DeviceArray.from_numpy(synth_normal(5, "u", (1, 77, 768)).astype(np.float16))
    lat = sd.latent_from_numpy(np.zeros((1, 4, 64, 64), np.float32))
    sd.compile(unc, ctx, lat, sampler=_sched(n=2), pag=True)
    assert sd._groups == 3 and sd._pag_flags.numpy().tolist() == [0.0] * 6 + [1.0] + [0.0] * 9      # after compile: the middle block
    outs = []
    for pag in ((3.0, "all"), (3.0, "all"), (0.0, "all")):
        sd.start(seed=SEED, pag=pag)
        sd.step_sampler(0, G); sd.synchronize()
        outs.append(lat.numpy().copy())
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])
