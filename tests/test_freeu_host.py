"""Host-side checks of FreeU (no GPU): the closed form of the Fourier filter against the torch.fft restatement on every case of the table, the
numpy emulation of the kernel's fp32 arithmetic inside half of the budget's fp32 term (which fixes its constant), the planted planes against
mutants, the stage -> block map for SD15 and TINY, the restated UNet forward with freeu=None against the oracle, the refusals compile() and
set_freeu() decide before any device work, and the header / ctypes declarations of csrc/freeu.hip with the launchers' host-side refusals."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "aux"))
import freeu_ref as R  # noqa: E402


# ---- 1. the closed form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", R.CASES_HW)
def test_closed_form_is_the_fft_restatement(hw):
    """float64 against float64: what is left is the rounding of two different summation orders, a few units of 2^-53 of the plane's largest
    sum (|x| reaches 20 here, the DC bin H W times that) -- 1e-13 is 50 of them at 16 x 16; the issue's 9e-16 was seen on unit-size noise."""
    H, W = hw
    worst = 0.0
    for C in R.CASES_C:
        for B in R.CASES_B:
            x = R.planted(B, C, H, W, "fp16")[1]
            for s in R.SCALES:
                d = float(np.abs(R.closed_form(x, s) - R.fourier_filter(x, s).numpy()).max())
                worst = max(worst, d)
    print(f"closed form vs FFT {hw}: max |d| = {worst:.2e}")
    assert worst <= 1e-13
    with pytest.raises(ValueError, match="H >= 2"):
        R.closed_form(np.zeros((1, 8, 1, 4)), 0.5)


def test_filter_passes_frequency_two_and_nyquist_and_scales_the_box():
    """What the four bins are.  A real harmonic cos(2 pi (u i / H + v j / W) + p) holds the bins (u, v) and (-u, -v) in equal parts, and the box
    is {0, -1}^2 -- not symmetric: the plane comes back times (m(u, v) + m(-u, -v)) / 2, m = s inside the box and 1 outside."""
    H, W, s = 12, 16, 0.25
    i, j = np.arange(H)[:, None] / H, np.arange(W)[None, :] / W
    m = lambda u, v: s if (u % H in (0, H - 1) and v % W in (0, W - 1)) else 1.0
    for (u, v), want in (((0, 0), s), ((1, 0), (1 + s) / 2), ((0, 1), (1 + s) / 2), ((1, 1), (1 + s) / 2), ((-1, -1), (1 + s) / 2), ((1, -1), 1.0),
                         ((2, 0), 1.0), ((0, 2), 1.0), ((6, 8), 1.0), ((1, 2), 1.0), ((2, 2), 1.0)):
        assert (m(u, v) + m(-u, -v)) / 2 == want
        x = np.cos(2 * np.pi * (u * i + v * j) + 0.3)[None, None]
        assert np.allclose(R.closed_form(x, s), want * x, atol=1e-12), (u, v)
        assert np.allclose(R.fourier_filter(x, s).numpy(), want * x, atol=1e-12), (u, v)


# ---- 2. the emulation fixes the budget's constant ----------------------------------------------------------------------------------------------
def test_emulation_stays_within_half_of_the_fp32_term_and_fixes_its_constant():
    worst, rows = 0.0, []
    for dtype in ("fp16", "bf16"):
        for (B, H, W, C) in R.cases():
            bits, x = R.planted(B, C, H, W, dtype)
            for s in R.SCALES:
                y = R.closed_form(x, s)
                e, ebits = R.emulate(x.astype(np.float32), s, dtype)
                err = np.abs(e.astype(np.float64) - y)
                tol, A = R.budget(y, x, s, dtype)
                assert np.all(err <= A / 2), (dtype, B, H, W, C, s)
                assert np.all(np.abs(R.from16(ebits, dtype) - y) <= tol), (dtype, B, H, W, C, s)
                if s == 1.0:
                    assert np.array_equal(ebits, bits)
                k = R.k_needed(err, y, x, s)
                rows.append((k, dtype, B, H, W, C, s))
                worst = max(worst, k)
    for k, *case in sorted(rows, reverse=True)[:12]:
        print(f"K needed {k:.2f} at {case}")
    for s in R.SCALES:
        print(f"s = {s}: K needed {max(r[0] for r in rows if r[6] == s):.2f}")
    assert worst <= R.K_FREEU and math.ceil(worst) == R.K_FREEU, worst          # the smallest integer


def test_planted_planes_tell_mutants_from_the_filter():
    for (B, H, W, C) in R.cases():
        x = R.planted(B, C, H, W, "fp16")[1]
        assert np.abs(x).max() < 40 and np.abs(x).mean() > 1
        for s in (0.2, 0.9, -0.5):
            y = R.closed_form(x, s)
            tol, _ = R.budget(y, x, s, "fp16")
            for name, m in R.mutants(x, s).items():
                if name == "sine terms dropped" and (H, W) == (2, 2):
                    continue                                                                      # (all sines are zero there)
                assert float(np.max(np.abs(m - y) / tol)) > 100, (name, B, H, W, C, s)


# ---- 3. the stage map ----------------------------------------------------------------------------------------------------------------------------
def test_stage_map_follows_diffusers_up_blocks_for_sd15_and_tiny():
    import oracle
    from dataclasses import replace
    from tinyfusers_amd.vision.unet import SD15, TINY, UNetModel, freeu_stages
    sd15 = freeu_stages(SD15)
    assert sd15 == R.stage_map(oracle.SD15)
    assert [(st, blk) for st, blk, *_ in sd15] == [(0, 0), (0, 1), (0, 2), (1, 3), (1, 4), (1, 5)]
    assert [(ch, sk) for _, _, ch, sk, _ in sd15] == [(1280, 1280)] * 5 + [(1280, 640)]
    assert [64 // d for *_, d in sd15] == [8, 8, 8, 16, 16, 16]                      # a 64 x 64 latent
    tiny = freeu_stages(TINY)
    assert tiny == R.stage_map(oracle.TINY)
    assert [(ch, sk) for _, _, ch, sk, _ in tiny] == [(128, 128)] * 5 + [(128, 64)] and [16 // d for *_, d in tiny] == [4, 4, 4, 8, 8, 8]
    # the map names the module tree's own blocks: the first ResBlock of block i reads backbone + skip channels
    for cfg, plan in ((SD15, sd15), (TINY, tiny)):
        net = UNetModel(cfg)
        for _, blk, ch, sk, _ in plan:
            assert net.output_blocks[blk][0].in_layers[0].num_channels == ch + sk
    with pytest.raises(ValueError, match="two decoder stages"):
        freeu_stages(replace(TINY, channel_mult=(1,), attention_levels=(0,)))


# ---- 4. the restated UNet ---------------------------------------------------------------------------------------------------------------------------
def test_restated_unet_forward_without_freeu_is_the_oracle_and_reads_all_four_parameters():
    import oracle
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    W = {k: v.astype(np.float32) for k, v in synth_state_dict(oracle.unet_param_shapes(oracle.TINY), 5).items()}
    x, ctx, t = synth_normal(5, "x", (2, 4, 16, 16)), synth_normal(5, "c", (2, 5, 64)), np.array([481.0], np.float32)
    plain = oracle.unet_forward(x, t, ctx, W, oracle.TINY).numpy()
    assert float(np.abs(R.unet_forward(x, t, ctx, W, oracle.TINY).numpy() - plain).max()) == 0.0
    ones = R.unet_forward(x, t, ctx, W, oracle.TINY, freeu=(1.0, 1.0, 1.0, 1.0)).numpy()
    assert np.allclose(ones, plain, rtol=1e-4, atol=1e-5)                               # (the FFT round trip's rounding only)
    for k, v in enumerate((0.2, 0.2, 1.5, 1.6)):
        p = [1.0] * 4; p[k] = v
        moved = R.unet_forward(x, t, ctx, W, oracle.TINY, freeu=tuple(p)).numpy()
        rl2 = float(np.linalg.norm(moved - plain) / np.linalg.norm(plain))
        print(f"freeu parameter {k} = {v}: rel-L2 against the plain output {rl2:.3f}")
        assert rl2 >= 10 * 5e-3


# ---- 5. refusals decided before any device work -------------------------------------------------------------------------------------------------
def test_compile_and_set_freeu_refuse_before_touching_a_device():
    from types import SimpleNamespace
    from tinyfusers_amd import config
    from tinyfusers_amd.variants import inputs
    from tinyfusers_amd.variants.samplers import DPMSolverPP2M, UnsupportedSamplerConfig
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import SD15, TINY, freeu_stages
    sch = DPMSolverPP2M().schedule(4)
    sd = StableDiffusion(TINY)
    with pytest.raises(ValueError, match="freeu=True needs a sampler"):
        sd.compile(None, None, None, freeu=True)
    old = config.cfg_parallel
    config.cfg_parallel = True
    try:
        with pytest.raises(UnsupportedSamplerConfig, match="TF_CFG_PARALLEL"):
            sd.compile(None, None, None, sampler=sch, freeu=True)
    finally:
        config.cfg_parallel = old
    config.set_dtype("fp8")
    try:
        with pytest.raises(UnsupportedSamplerConfig, match="fp8"):
            sd.compile(None, None, None, sampler=sch, freeu=True)
    finally:
        config.set_dtype("fp16")
    # the kernels' rules on the stage tensors: a 4 x 4 latent leaves stage 1 of TINY a 1 x 1 plane; a width whose half is no whole vector
    lat = SimpleNamespace(shape=(1, 4, 4, 4))
    with pytest.raises(ValueError, match="output block 0 .stage 1.*1 x 1"):
        inputs.check_compile(4, False, config, lat, sch, False, None, False, freeu=True, freeu_plan=freeu_stages(TINY))
    with pytest.raises(ValueError, match="multiples of 16"):
        inputs.check_compile(4, False, config, SimpleNamespace(shape=(1, 4, 16, 16)), sch, False, None, False, freeu=True,
                             freeu_plan=[(0, 0, 24, 24, 4)])
    inputs.check_compile(4, False, config, SimpleNamespace(shape=(2, 4, 64, 64)), sch, False, None, False, freeu=True, freeu_plan=freeu_stages(SD15))
    inputs.check_compile(4, False, config, SimpleNamespace(shape=(2, 4, 16, 16)), sch, False, None, False, cfg=False, freeu=True, freeu_plan=freeu_stages(TINY))
    # the four scalars
    assert inputs.freeu_scales((0.9, 0.2, 1.5, 1.6)).tolist() == [np.float32(v) for v in (0.9, 0.2, 1.5, 1.6)]
    for bad in ((1.0, 1.0, 1.0), (1.0, 1.0, 1.0, float("nan")), (1.0, 1.0, float("inf"), 1.0), "abcd", None, (1.0, 1.0, 1.0, 1.0, 1.0), ((1.0, 1.0), (1.0, 1.0)),
                (1.0, "x", 1.0, 1.0)):
        with pytest.raises(ValueError, match="four finite floats"):
            inputs.freeu_scales(bad)
    # a model that was never compiled, and the names of the keywords
    with pytest.raises(UnsupportedSamplerConfig, match="compile"):
        sd.set_freeu(0.9, 0.2, 1.5, 1.6)
    import inspect
    assert list(inspect.signature(StableDiffusion.set_freeu).parameters)[1:] == ["s1", "s2", "b1", "b2"]
    assert "freeu" in inspect.signature(StableDiffusion.start).parameters and "freeu" in inspect.signature(StableDiffusion.compile).parameters


# ---- 6. header ------------------------------------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_declare_the_freeu_entries_and_the_launchers_refuse_on_the_host():
    import ctypes
    import tinyfusers_amd.native as native
    hdr = open(os.path.join(ROOT, "include", "tinyfusers_hip.h")).read()
    i = hdr.index("csrc/freeu.hip")
    block = hdr[hdr.rindex("/*", 0, i):hdr.index("/* ---- ControlNet")]
    assert "vision/unet.py:72" in block[:block.index("*/")]
    names = set(re.findall(r"\b(tf_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", block, flags=re.S)))
    assert names == {"tf_freeu_skip_16", "tf_freeu_backbone_16"} and names <= set(native.declared_symbols())
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert native.lib.tf_freeu_skip_16.argtypes == [i32, vp, i32, vp, vp] and native.lib.tf_freeu_skip_16.restype is i32
    assert native.lib.tf_freeu_backbone_16.argtypes == [i32, vp, vp, i64, i32, vp, i32, vp]
    m = re.search(r"typedef struct \{([^}]*)\} tfFreeuEntry;", hdr)
    assert [f.split()[-1] for f in m.group(1).split(";") if f.strip()] == [n for n, _ in native.FreeuEntry._fields_] == ["dst", "src", "B", "H", "W", "C", "scale_index"]
    assert ctypes.sizeof(native.FreeuEntry) == 40
    assert "freeu.hip" in __import__("tinyfusers_amd.build", fromlist=["SOURCES"]).SOURCES
    # argument validation happens before any device work, and names the entry
    skip, err = native.lib.tf_freeu_skip_16, native.lib.tf_last_error
    row = (native.FreeuEntry * 2)()

    def fill(e, **kw):
        e.dst, e.src, e.B, e.H, e.W, e.C, e.scale_index = 64, 128, 1, 4, 4, 8, 0
        for k, v in kw.items():
            setattr(e, k, v)
    fill(row[0]); fill(row[1])
    assert skip(0, ctypes.cast(row, vp), 9, vp(64), None) == 10001 and b"n_entries" in err()
    assert skip(2, ctypes.cast(row, vp), 2, vp(64), None) == 10001 and b"dtype" in err()
    fill(row[1], src=None)
    assert skip(0, ctypes.cast(row, vp), 2, vp(64), None) == 10001 and b"entry 1 holds a null pointer" in err()
    fill(row[1], C=12)
    assert skip(1, ctypes.cast(row, vp), 2, vp(64), None) == 10001 and b"entry 1" in err() and b"multiple of 8" in err()
    fill(row[1], H=1)
    assert skip(0, ctypes.cast(row, vp), 2, vp(64), None) == 10001 and b"entry 1 has H=1" in err()
    fill(row[0], W=1)
    assert skip(0, ctypes.cast(row, vp), 2, vp(64), None) == 10001 and b"entry 0 has H=4, W=1" in err()
    fill(row[0]); fill(row[1], dst=72)
    assert skip(0, ctypes.cast(row, vp), 2, vp(64), None) == 10001 and b"entry 1 is not 16-byte aligned" in err()
    fill(row[1], H=200, W=100)
    assert skip(0, ctypes.cast(row, vp), 2, vp(64), None) == 10001 and b"H + W" in err()
    bb = native.lib.tf_freeu_backbone_16
    assert bb(0, vp(64), vp(64), 4, 24, vp(64), 2, None) == 10001 and b"C=24" in err()
    assert bb(0, None, vp(64), 4, 32, vp(64), 2, None) == 10001 and b"bad arguments" in err()
    assert bb(3, vp(64), vp(64), 4, 32, vp(64), 2, None) == 10001 and b"dtype" in err()
    assert bb(0, vp(64), vp(72), 4, 32, vp(64), 2, None) == 10001 and b"16-byte aligned" in err()
