"""Host-side checks of the ControlNet (no GPU): the CPU restatement tests/aux/controlnet_oracle.py against oracle.unet_forward, the names and
shapes a control_*_sd15_* checkpoint holds against the module tree vision/controlnet.py builds, the block plan shared with the UNet, the
compile() refusals decided before any device work, and the header / ctypes declarations of csrc/control.hip (test_abi checks that the library
exports what the header declares)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "aux"))
import controlnet_oracle as C  # noqa: E402


def _tiny_inputs():
    import oracle
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    W = {k: v.astype(np.float32) for k, v in synth_state_dict(oracle.unet_param_shapes(oracle.TINY), 5).items()}
    Wc = {k: v.astype(np.float32) for k, v in synth_state_dict(C.controlnet_param_shapes(oracle.TINY), 6).items()}
    x = synth_normal(5, "x", (2, 4, 8, 8))
    ctx = synth_normal(5, "c", (2, 5, 64))
    hint = np.random.default_rng(3).random((2, 3, 64, 64)).astype(np.float32)
    return W, Wc, x, ctx, hint


def test_zero_residuals_leave_the_restated_unet_forward_exact():
    import oracle
    W, Wc, x, ctx, hint = _tiny_inputs()
    t = np.array([481.0], np.float32)
    plain = oracle.unet_forward(x, t, ctx, W, oracle.TINY).numpy()
    assert np.array_equal(C.unet_forward(x, t, ctx, W, oracle.TINY).numpy(), plain)
    r = C.controlnet_forward(x, hint, t, ctx, Wc, oracle.TINY)
    assert len(r) == 10 and all(np.abs(v.numpy()).max() > 0 for v in r)
    zeros = [np.zeros(tuple(v.shape), np.float32) for v in r]
    assert np.array_equal(C.unet_forward(x, t, ctx, W, oracle.TINY, control=zeros).numpy(), plain)
    moved = C.unet_forward(x, t, ctx, W, oracle.TINY, control=r).numpy()
    assert np.abs(moved - plain).max() > 1e-3                       # ... and non-zero ones are read
    # zero-initialised zero convs (a freshly made ControlNet) give all-zero residuals: the controlled model starts as the plain one
    Wz = {k: (np.zeros_like(v) if k.startswith(("zero_convs.", "middle_block_out.")) else v) for k, v in Wc.items()}
    assert all(not v.numpy().any() for v in C.controlnet_forward(x, hint, t, ctx, Wz, oracle.TINY))
    # a single hint is broadcast over the batch (fp32 rounding only: the convolution of one image may sum in another order than of two)
    one = C.controlnet_forward(x, hint[:1], t, ctx, Wc, oracle.TINY)
    two = C.controlnet_forward(x, np.concatenate([hint[:1], hint[:1]]), t, ctx, Wc, oracle.TINY)
    assert all(np.allclose(a.numpy(), b.numpy(), rtol=1e-4, atol=1e-5) for a, b in zip(one, two))


def test_controlnet_param_shapes_are_the_checkpoint_names_and_the_module_tree():
    import oracle
    from tinyfusers_amd.storage.state import param_shapes
    from tinyfusers_amd.vision.controlnet import ControlNet
    from tinyfusers_amd.vision.unet import SD15, TINY
    P = C.controlnet_param_shapes(oracle.SD15)
    stem = [(3, 16), (16, 16), (16, 32), (32, 32), (32, 96), (96, 96), (96, 256), (256, 320)]
    for i, (ci, co) in enumerate(stem):
        assert P[f"input_hint_block.{2 * i}.weight"] == (co, ci, 3, 3) and P[f"input_hint_block.{2 * i}.bias"] == (co,)
    assert sorted(k for k in P if k.startswith("input_hint_block.")) == sorted(f"input_hint_block.{2 * i}.{l}" for i in range(8) for l in ("weight", "bias"))
    zc = [320, 320, 320, 320, 640, 640, 640, 1280, 1280, 1280, 1280, 1280]
    for i, c in enumerate(zc):
        assert P[f"zero_convs.{i}.0.weight"] == (c, c, 1, 1) and P[f"zero_convs.{i}.0.bias"] == (c,)
    assert len([k for k in P if k.startswith("zero_convs.")]) == 24
    assert P["middle_block_out.0.weight"] == (1280, 1280, 1, 1) and P["middle_block_out.0.bias"] == (1280,)
    U = oracle.unet_param_shapes(oracle.SD15)
    trunk = ("time_embed.", "input_blocks.", "middle_block.")
    assert {k: v for k, v in P.items() if k.startswith(trunk)} == {k: v for k, v in U.items() if k.startswith(trunk)}
    assert not any(k.startswith(("output_blocks.", "out.")) for k in P)
    # the module tree asks for exactly these names, with or without the trailing dot of the checkpoint's prefix
    for cfg, ocfg, n_zero in ((SD15, oracle.SD15, 12), (TINY, oracle.TINY, 9)):
        net = ControlNet(cfg)
        assert len(net.zero_convs) == n_zero == len(net.input_blocks)
        want = {k: tuple(v) for k, v in C.controlnet_param_shapes(ocfg).items()}
        assert {k: tuple(v) for k, v in param_shapes(net).items()} == want
        assert {k: tuple(v) for k, v in param_shapes(net, "control_model.").items()} == {"control_model." + k: v for k, v in want.items()}
        assert param_shapes(net, "control_model.") == param_shapes(net, "control_model")
    # a concat-conditioned UNet's ControlNet still reads the 4 latent channels
    from dataclasses import replace
    assert C.controlnet_param_shapes(replace(oracle.SD15, in_channels=9))["input_blocks.0.0.weight"] == (320, 4, 3, 3)
    assert param_shapes(ControlNet(replace(SD15, in_channels=9)))["input_blocks.0.0.weight"] == (320, 4, 3, 3)


def test_the_encoder_plan_exists_once_and_both_models_walk_it():
    import inspect
    from tinyfusers_amd.storage.state import param_shapes
    from tinyfusers_amd.vision import controlnet, unet
    assert issubclass(unet.UNetModel, unet.StepModel) and issubclass(controlnet.ControlNet, unet.StepModel)
    for cls in (unet.UNetModel, controlnet.ControlNet):
        assert "encoder_plan(" in inspect.getsource(cls.__init__) and "self._encode(" in inspect.getsource(cls.__call__)
        for name in ("_prepare", "time_embedding_all", "context_kv", "weights_key", "_encode", "_runner"):
            assert getattr(cls, name) is getattr(unet.StepModel, name), (cls, name)
    import oracle
    for cfg, ocfg in ((unet.SD15, oracle.SD15), (unet.TINY, oracle.TINY), (unet.SD15_INPAINT, None)):
        got = {k: tuple(v) for k, v in param_shapes(unet.UNetModel(cfg)).items()}
        if ocfg is not None:
            assert got == {k: tuple(v) for k, v in oracle.unet_param_shapes(ocfg).items()}            # the UNet's tree is what it was
    net = controlnet.ControlNet(unet.SD15)
    assert len(net._all(unet.ResBlock)) == 10 and len(net._all(unet.SpatialTransformer)) == 7     # 8 in the input blocks + 2 in the middle; 6 + 1
    assert len(unet.UNetModel(unet.SD15)._all(unet.ResBlock)) == 22 and len(unet.UNetModel(unet.SD15)._all(unet.SpatialTransformer)) == 16


def test_compile_refuses_control_before_touching_a_device():
    from dataclasses import replace
    from tinyfusers_amd import config
    from tinyfusers_amd.variants.samplers import DPMSolverPP2M, UnsupportedSamplerConfig
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.controlnet import ControlNet
    from tinyfusers_amd.vision.unet import SD15, TINY
    sch = DPMSolverPP2M().schedule(4)
    sd = StableDiffusion(TINY)
    assert sd.control_model is None
    with pytest.raises(ValueError, match="attach_control"):
        sd.compile(None, None, None, sampler=sch, control=True)
    with pytest.raises(TypeError, match="ControlNet"):
        sd.attach_control(object())
    with pytest.raises(ValueError, match="built for"):
        sd.attach_control(ControlNet(SD15))
    assert sd.control_model is None
    assert sd.attach_control(ControlNet(TINY)) is sd and sd.control_model is not None
    with pytest.raises(ValueError, match="sampler"):
        sd.compile(None, None, None, control=True)
    nine = StableDiffusion(replace(TINY, in_channels=9)).attach_control(ControlNet(replace(TINY, in_channels=9)))
    with pytest.raises(ValueError, match="concat="):
        nine.compile(None, None, None, sampler=sch, concat="inpaint", control=True)
    old = config.cfg_parallel
    config.cfg_parallel = True
    try:
        with pytest.raises(UnsupportedSamplerConfig, match="TF_CFG_PARALLEL"):
            sd.compile(None, None, None, sampler=sch, control=True)
    finally:
        config.cfg_parallel = old
    config.set_dtype("fp8")
    try:
        with pytest.raises(UnsupportedSamplerConfig, match="fp8"):
            sd.compile(None, None, None, sampler=sch, control=True)
    finally:
        config.set_dtype("fp16")


def test_header_and_ctypes_declare_the_control_entries():
    import ctypes
    import tinyfusers_amd.native as native
    hdr = open(os.path.join(ROOT, "include", "tinyfusers_hip.h")).read()
    i = hdr.index("csrc/control.hip")
    block = hdr[hdr.rindex("/*", 0, i):hdr.index("---- concat-conditioned UNets")]
    assert "vision/unet.py:72" in block[:block.index("*/")]
    names = set(re.findall(r"\b(tf_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", block, flags=re.S)))
    assert names == {"tf_control_add_16", "tf_hint_from_u8_16"}
    assert names <= set(native.declared_symbols())
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert native.lib.tf_control_add_16.argtypes == [i32, vp, i32, vp, vp] and native.lib.tf_control_add_16.restype is i32
    assert native.lib.tf_hint_from_u8_16.argtypes == [i32, vp, vp, i64, vp]
    # the host table row is the header's struct: three pointers and a 64-bit count
    m = re.search(r"typedef struct \{([^}]*)\} tfControlEntry;", hdr)
    assert [f.split()[-1] for f in m.group(1).split(";") if f.strip()] == [n for n, _ in native.ControlEntry._fields_] == ["dst", "skip", "residual", "n"]
    assert ctypes.sizeof(native.ControlEntry) == 32
    # argument validation happens before any device work
    row = (native.ControlEntry * 1)()
    assert native.lib.tf_control_add_16(0, ctypes.cast(row, vp), 17, vp(64), None) == 10001 and b"n_entries" in native.lib.tf_last_error()
    assert native.lib.tf_control_add_16(2, ctypes.cast(row, vp), 1, vp(64), None) == 10001 and b"dtype" in native.lib.tf_last_error()
    assert native.lib.tf_control_add_16(0, ctypes.cast(row, vp), 1, vp(64), None) == 10001 and b"null pointer" in native.lib.tf_last_error()
    row[0].dst, row[0].skip, row[0].residual, row[0].n = 64, 64, 128, 12
    assert native.lib.tf_control_add_16(0, ctypes.cast(row, vp), 1, vp(64), None) == 10001 and b"multiple of 8" in native.lib.tf_last_error()
    row[0].n, row[0].residual = 16, 130
    assert native.lib.tf_control_add_16(1, ctypes.cast(row, vp), 1, vp(64), None) == 10001 and b"16-byte aligned" in native.lib.tf_last_error()
    assert native.lib.tf_hint_from_u8_16(0, None, vp(64), 8, None) == 10001 and b"bad arguments" in native.lib.tf_last_error()
