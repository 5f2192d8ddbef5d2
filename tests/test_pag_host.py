"""Host checks of perturbed-attention guidance (no GPU): the two identities that map its combine onto the tails that exist, the layer-name mapper,
compile's refusals, the launcher's instance rule (tf_sdpa_pag_instance), and the precondition of tests/test_gpu_pag.py -- on the CPU restatement
(tests/aux/pag_ref.py), at that file's weights and seed, the perturbed branch differs from the conditional one by at least 10 x the gate the GPU
results are held to, so a model that ignored ``pag=`` could not pass there."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "aux"))

import pag_ref as PR  # noqa: E402
import sdpa_planted as P  # noqa: E402

F16, BF16 = 0, 1
E_ARG, E_UNSUPPORTED = 10001, 10002
REL_L2_GATE = 5e-3                 # tests/test_gpu_controlnet.py::_gate
# tests/test_gpu_ip_adapter.py's small UNet: heads 40 and 80 wide (the perturbed launch is built for the LDS-DMA head sizes)
SHAPE = dict(model_channels=160, channel_mult=(1, 2, 2), attention_levels=(0, 1), n_heads=4, context_dim=64)
B, PAG_SEED, G_CFG, T0 = 2, 5, 7.5, 481.0
# what the trajectory tests perturb: the middle block alone moves a step's latent by rel-L2 0.03 at s = 3 (seeds 1 .. 12: 0.030 - 0.036, the weight
# seed hardly matters), short of 10 x the gate; with the first decoder transformer next to it the step moves by 0.117 (asserted below)
TRAJ_LAYERS = ["mid", "output_blocks.3"]
TRAJ_BLOCKS = ("middle_block", "output_blocks.3")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    import tinyfusers_amd.native as n
    return n


def cfgs():
    import oracle
    from tinyfusers_amd.vision.unet import UNetConfig
    return UNetConfig(**SHAPE), oracle.UNetConfig(**SHAPE)


@functools.lru_cache(maxsize=None)
def data(seed=PAG_SEED):
    """(UNet weights, context, unconditional context, a latent), all values of the 16-bit storage type: what the GPU model tests run on."""
    import oracle
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    W = synth_state_dict(oracle.unet_param_shapes(cfgs()[1]), seed)
    f16 = lambda a: a.astype(np.float16).astype(np.float32)
    return W, f16(synth_normal(seed, "c", (B, 13, 64))), f16(synth_normal(seed, "u", (B, 13, 64))), f16(synth_normal(seed, "lat", (B, 4, 16, 16)))


@functools.lru_cache(maxsize=None)
def ref_forward(perturb, t=T0, uncond=False):
    """The restatement's UNet output at data()'s latent (float64), for a tuple of perturbed blocks; computed once per argument set."""
    import torch
    W, ctx, unc, x = data()
    Wf = {k: torch.from_numpy(v.astype(np.float32)) for k, v in W.items()}
    out = PR.unet_forward(x, np.array([t], np.float32), unc if uncond else ctx, Wf, perturb, cfgs()[1]).numpy().astype(np.float64)
    out.setflags(write=False)
    return out


def test_both_identities_hold_against_the_float64_combine(native):
    from tinyfusers_amd.variants import inputs
    three = lambda e0, e1, e2, g_t, g_i: e0 + g_t * (e2 - e1) + g_i * (e1 - e0)        # k_sampler_step<T, 3, .>'s expression (csrc/sampler.hip)
    pair = lambda e0, e1, g: e0 + g * (e1 - e0)                                         # k_sampler_step<T, 2, .>'s
    rng = np.random.default_rng(11)
    clipped = 0
    for _ in range(200):
        e_u, e_p, e_c = rng.standard_normal((3, 64))
        g, s, a, t = rng.uniform(1.0, 12.0), rng.uniform(0.0, 6.0), rng.choice([0.0, rng.uniform(0.0, 0.02)]), float(rng.integers(1, 1000))
        s_t = inputs.pag_scale_at(s, a, t)
        assert s_t == PR.scale_at(s, a, t) == max(0.0, s - a * (1000.0 - t)) and s_t >= 0.0
        clipped += s_t == 0.0 and s > 0.0
        g_t, g_i = inputs.pag_guidance_words(g, s_t, cfg=True)
        np.testing.assert_allclose(three(e_u, e_p, e_c, g_t, g_i), PR.combine(e_u, e_p, e_c, g, s_t), rtol=0, atol=1e-12)
        w, none = inputs.pag_guidance_words(1.0, s_t, cfg=False)
        assert none is None
        np.testing.assert_allclose(pair(e_p, e_c, w), PR.combine(None, e_p, e_c, None, s_t), rtol=0, atol=1e-12)
    assert clipped >= 10                                                                # the adaptive term clipped s_t to 0 often enough
    assert inputs.pag_scale_at(3.0, 0.01, 600.0) == 0.0 and inputs.pag_scale_at(3.0, 0.0, 1.0) == 3.0
    assert inputs.pag_guidance_words(7.5, 0.0) == (7.5, 7.5) and inputs.pag_guidance_words(1.0, 0.0, cfg=False) == (1.0, None)
    for bad in ((-1.0, 0.0), (float("nan"), 0.0), (3.0, -0.1), (3.0, float("inf")), ("x", 0.0), (None, 0.0)):
        with pytest.raises(ValueError, match="finite floats >= 0"):
            inputs.pag_values(*bad)
    assert inputs.pag_values(3, 0) == (3.0, 0.0)


def test_layer_names_map_to_the_flag_words(native):
    import oracle
    from tinyfusers_amd.variants import inputs
    from tinyfusers_amd.vision.unet import PAG_WORDS, SD15, TINY, UNetConfig, pag_layers
    table = pag_layers(SD15)
    assert table == PR.SD15_LAYERS == PR.layers(oracle.SD15) and len(table) == 16 == PAG_WORDS == inputs.PAG_WORDS
    assert pag_layers(UNetConfig(**SHAPE)) == PR.layers(cfgs()[1]) and len(pag_layers(UNetConfig(**SHAPE))) == 11
    assert pag_layers(TINY) == PR.layers(oracle.UNetConfig(model_channels=64, channel_mult=(1, 2, 2), attention_levels=(0, 1), n_heads=2, context_dim=64))
    on = lambda layers, tb=table: np.flatnonzero(inputs.pag_layer_words(layers, tb)).tolist()
    assert on("mid") == [6] and on("down") == [0, 1, 2, 3, 4, 5] and on("up") == list(range(7, 16)) and on("all") == list(range(16)) and on([]) == []
    assert on(6) == [6] and on([0, 15]) == [0, 15] and on(np.int64(3)) == [3]
    assert on("input_blocks.4") == [2] and on("middle_block") == [6] and on("output_blocks.7") == [11] and on("output_blocks.11") == [15]
    assert on("input_blocks.1") == [0] and on("input_blocks.1.1") == [0] and on("middle_block.1") == [6] and on("output_blocks.11.1") == [15]
    assert on(["down", "middle_block", 15, "output_blocks.3"]) == [0, 1, 2, 3, 4, 5, 6, 7, 15]
    words = inputs.pag_layer_words("mid", table)
    assert words.dtype == np.float32 and words.shape == (16,) and words.nbytes == 64 and set(words.tolist()) == {0.0, 1.0}
    small = pag_layers(UNetConfig(**SHAPE))
    assert on("mid", small) == [4] and on("up", small) == [5, 6, 7, 8, 9, 10] and on("all", small) == list(range(11))
    # an unknown name, a block or an index without a transformer: refused before anything is returned
    for bad in ("middle", "input_blocks.3", "input_blocks.0", "output_blocks.0", "output_blocks.12", "input_blocks", 16, -1, True, 1.5, None, ["mid", "nope"],
                "input_blocks.4.0"):
        with pytest.raises(ValueError, match="names no SpatialTransformer"):
            inputs.pag_layer_words(bad, table)
    with pytest.raises(ValueError, match="names no SpatialTransformer"):
        inputs.pag_layer_words(11, small)


def test_compile_refuses_the_four_combinations(native):
    from types import SimpleNamespace
    from tinyfusers_amd import config
    from tinyfusers_amd.variants import inputs
    from tinyfusers_amd.variants.samplers import DPMSolverPP2M, UnsupportedSamplerConfig
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import SD15, TINY, pag_layers
    sch, lat = DPMSolverPP2M().schedule(4), SimpleNamespace(shape=(1, 4, 16, 16))
    check = lambda cin=4, sampler=sch, concat=None, **kw: inputs.check_compile(cin, False, config, lat, sampler, False, concat, False, pag=True,
                                                                                pag_table=pag_layers(SD15), **kw)
    with pytest.raises(ValueError, match="pag=True needs a sampler schedule"):
        check(sampler=None)
    with pytest.raises(ValueError, match="pag=True and concat='edit'.*fourth"):
        check(cin=8, concat="edit")
    old = config.cfg_parallel
    config.cfg_parallel = True
    try:
        with pytest.raises(UnsupportedSamplerConfig, match="TF_CFG_PARALLEL"):
            check()
    finally:
        config.cfg_parallel = old
    config.set_dtype("fp8")
    try:
        with pytest.raises(UnsupportedSamplerConfig, match="pag=True.*fp8"):
            check()
    finally:
        config.set_dtype("fp16")
    with pytest.raises(ValueError, match="17 SpatialTransformers"):
        inputs.check_compile(4, False, config, lat, sch, False, None, False, pag=True, pag_table=["x"] * 17)
    # what combines: cfg=False, inpaint=True, concat="inpaint", freeu
    check(); check(cfg=False); check(cin=9, concat="inpaint")
    inputs.check_compile(4, False, config, lat, sch, True, None, False, pag=True, pag_table=pag_layers(SD15))
    # through the model: refused before any device work (an uncompiled model says so afterwards, too)
    sd = StableDiffusion(TINY)
    with pytest.raises(ValueError, match="pag=True needs a sampler schedule"):
        sd.compile(None, None, None, pag=True)
    with pytest.raises(UnsupportedSamplerConfig, match="compile"):
        sd.set_pag(3.0, "mid")


def test_the_instance_rule_is_the_dual_launch_s(native):
    """tf_sdpa_pag_instance: sdpa_instance_unsplit's answer -- tf_sdpa_dual_instance's family for the same (B, NH, Tq, HS) at the head sizes both
    have, tf_sdpa_instance's under tf_sdpa_force_split(1) at 64 and 128 -- whatever tf_sdpa_force_split holds: a shape the plain launch would split
    runs the unsplit family (the split forms are left out), a head size without an LDS-DMA kernel (the generic kernel) and a bad range are refused."""
    from tinyfusers_amd.attention.sdpa import SDPA_INSTANCES as names, sdpa_pag_instance
    lib = native.lib
    pag = lambda dtype, b, nh, tq, tk, hs, b0=0, b1=0, st=None: lib.tf_sdpa_pag_instance(dtype, b, nh, tq, tk, hs, *(st or (hs, hs)), b0, b1)
    shapes = [(b, nh, tq, hs) for inst, b, nh, tq, hs in P.rows(("dma16", "dma32", "dma32_w8"))]
    shapes += [(2, 8, 4096, 40), (2, 8, 1024, 80), (2, 8, 256, 160), (2, 8, 64, 160), (1, 8, 4096, 40), (3, 8, 4096, 40), (3, 8, 1024, 80), (3, 8, 256, 160), (3, 4, 256, 40),
               (3, 4, 64, 80), (1, 127, 200, 160), (1, 128, 200, 160), (3, 2, 64, 64), (3, 2, 300, 128)]
    try:
        for ks in (0, 1, 2):
            for b, nh, tq, hs in shapes:
                for tk in (tq, 77, 330):
                    assert lib.tf_sdpa_force_split(1) == 0
                    want = lib.tf_sdpa_instance(F16, b, nh, tq, tk, hs, hs, hs, 0)
                    assert lib.tf_sdpa_force_split(ks) == 0
                    assert names[want] in ("dma16", "dma32", "dma32_w8")
                    for dtype in (F16, BF16):
                        assert pag(dtype, b, nh, tq, tk, hs, 0, b) == want, (ks, b, nh, tq, tk, hs)
                        assert pag(dtype, b, nh, tq, tk, hs, st=(3 * nh * hs, 3 * nh * hs)) == want                       # the packed q|k|v buffer
                        if hs in (40, 80, 160):
                            assert lib.tf_sdpa_dual_instance(dtype, b, nh, tq, tk, 4, hs, hs, hs, hs, hs) == want
    finally:
        lib.tf_sdpa_force_split(0)
    assert sdpa_pag_instance(np.float16, 1, 2, 200, 200, 80) == "dma16" and sdpa_pag_instance(np.float16, 16, 16, 300, 300, 40, batch_range=(3, 9)) == "dma32_w8"
    for inst, b, nh, tq, hs in P.rows(("dma16", "dma32", "dma32_w8")):
        assert sdpa_pag_instance(np.float16, b, nh, tq, tq, hs) == inst
    msg = lambda: lib.tf_last_error()
    for hs in (32, 56, 72, 96, 120, 152):                                   # the generic kernel's head sizes
        assert pag(F16, 1, 2, 200, 200, hs) == E_UNSUPPORTED and b"tf_sdpa_pag_instance" in msg() and b"head size %d" % hs in msg()
    for b0, b1 in ((-1, 1), (2, 1), (0, 4), (4, 4), (3, 5)):                # outside [0, B = 3], or reversed
        assert pag(F16, 3, 2, 200, 200, 40, b0, b1) == E_ARG and b"batch range" in msg(), (b0, b1)
    for b0, b1 in ((0, 0), (3, 3), (0, 3), (1, 2)):                         # empty ranges are legal
        assert pag(F16, 3, 2, 200, 200, 40, b0, b1) == 2
    assert pag(F16, 1, 2, 200, 200, 44) == E_ARG and pag(2, 1, 2, 200, 200, 40) == E_ARG and pag(F16, 1, 2, 200, 200, 40, st=(44, 40)) == E_ARG
    assert pag(F16, 1, 2, 200, 1 << 20, 40, st=(1024, 40)) == E_UNSUPPORTED and b"32-bit" in msg()
    with pytest.raises(RuntimeError, match="head size 32"):
        sdpa_pag_instance(np.float16, 1, 2, 200, 200, 32)
    # the launch refuses what the query refuses, before it reads a pointer (placeholders): a null flag, a bad range, a generic head size
    import ctypes
    ph = ctypes.c_void_p(4096)
    launch = lambda hs=40, b0=0, b1=1, flag=ph, o=ph: lib.tf_sdpa_pag_16(F16, o, ph, ph, ph, 3, 2, 200, 200, hs, *([2 * 200 * hs, 200 * hs, hs] * 4), b0, b1, flag, None)
    assert launch(flag=None) == E_ARG and b"null flag" in msg()
    assert launch(o=None) == E_ARG and b"null tensor" in msg()
    assert launch(b0=2, b1=4) == E_ARG and b"batch range" in msg()
    assert launch(hs=32) == E_UNSUPPORTED and b"head size 32" in msg()


def test_the_perturbed_branch_is_no_rounding_error_on_the_reference(native):
    """The precondition of tests/test_gpu_pag.py, on the CPU restatement at its weights and seed: ||e_c - e_p|| / ||e_c|| >= 10 x the rel-L2 gate for
    the mid-only and for the all-layers selection, and one DPM++2M step at s = 3 on TRAJ_LAYERS moves the latent by >= 10 x the gate against s = 0."""
    from tinyfusers_amd.variants import samplers as S
    table = tuple(PR.layers(cfgs()[1]))
    e_c = ref_forward(())
    for sel in (("middle_block",), table):
        e_p = ref_forward(sel)
        rel = float(np.linalg.norm(e_c - e_p) / np.linalg.norm(e_c))
        print(f"\n||e_c - e_p|| / ||e_c|| with {len(sel)} perturbed transformer(s): {rel:.4f} (needs >= {10 * REL_L2_GATE})")
        assert rel >= 10 * REL_L2_GATE, (sel, rel)
    sch = S.make("dpmpp2m").schedule(3)
    x = data()[3].astype(np.float64)
    t, a_t = float(sch.timesteps[0]), float(sch.alphas[0])
    e_u, e_c, e_p = ref_forward((), t, True), ref_forward((), t), ref_forward(TRAJ_BLOCKS, t)
    nxt = []
    for s in (0.0, 3.0):
        e = PR.combine(e_u, e_p, e_c, G_CFG, PR.scale_at(s, 0.0, t))
        x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
        c_x, c_0, _, _ = sch.coeffs[0]
        nxt.append(c_x * x + c_0 * x0)
    moved = float(np.linalg.norm(nxt[1] - nxt[0]) / np.linalg.norm(nxt[0]))
    print(f"one step at s = 3 against s = 0 ({TRAJ_LAYERS}): the latent moves by rel-L2 {moved:.4f} (needs >= {10 * REL_L2_GATE})")
    assert moved >= 10 * REL_L2_GATE, moved
