"""GPU checks of the concat-conditioned checkpoints (csrc/sampler.hip and csrc/img2img.hip, StableDiffusion.compile(..., concat="inpaint" | "edit"),
start(cond_image= / cond_mask= / cond_latent=, image_guidance=)): the four kernels bit for bit against their host constructions and their
img2img / sampler namesakes, one three-branch update against a float64 restatement, tiny-UNet trajectories of a 9-channel and an 8-channel
model (graph == eager, reproducible, against the CPU oracle fed the concatenated input), the conditioning path through the VAE encoder, the
argument checks, and the SD-1.5 shapes end to end."""
import contextlib
import io
import os
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_samplers_host import randn_ref  # noqa: E402

SEED = 0x243F6A8885A308D3          # a seed with both key words nonzero
G_T, G_I = 7.5, 1.5


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


@pytest.fixture(scope="module")
def vae_sd(tf):
    """An SD-1.5 StableDiffusion whose first_stage_model (encoder and decoder) holds synthetic weights; the UNet stays empty."""
    from tinyfusers_amd.storage.state import param_shapes, update_state
    from tinyfusers_amd.storage.synth import synth_state_dict
    from tinyfusers_amd.variants.sd import StableDiffusion
    sd = StableDiffusion()
    W = synth_state_dict(param_shapes(sd.first_stage_model, "first_stage_model"), 0)
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(sd.first_stage_model, W, "first_stage_model")
    return sd, W


def _words(seed):
    return seed & 0xFFFFFFFF, seed >> 32


def _gate(got, ref, rel_l2=5e-3, max_rel=1e-2):
    """tests/test_gpu_samplers.py's gate: rel-L2 and max |d| <= max_rel max |ref| (the latent grows to |x| ~ 25 under CFG 7.5)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all()
    rl2 = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    mx = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"gate: rel-L2 {rl2:.3e} (gate {rel_l2}), max|d|/max|ref| {mx:.3e} (gate {max_rel}), max|ref| {np.abs(ref).max():.1f}")
    assert rl2 <= rel_l2 and mx <= max_rel, (rl2, mx)


def _bits16(x, dtype):
    """fp32 -> the 16-bit patterns of the step's type, round-to-nearest-even on the host."""
    from tinyfusers_amd.storage.tensor import f32_to_bf16_bits
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(over="ignore"):
        return f32_to_bf16_bits(x) if dtype == "bf16" else x.astype(np.float16).view(np.uint16)


def _raw16(tf, n, fill):
    """A device buffer of n uint16 words, every word `fill`."""
    return tf.DeviceArray.from_numpy(np.full((n,), fill, np.uint16), np.uint16, "row")


def _read16(a):
    return a.numpy().astype(np.uint16)


# ---- 1. tf_cfg_concat_* -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(1, 4, 5, 5, 7), (2, 4, 5, 8, 12), (3, 4, 4, 5, 7), (2, 4, 4, 16, 16)])
def test_cfg_concat_matches_the_host_construction_and_cfg_duplicate(tf, shape, dtype):
    """(B,C,Cc,H,W); 5x7 makes every row and image start odd, 9 channels make 18-byte pixels.  The output sits between two guard regions at an
    offset of 3 words, so the first pixel is 2-byte aligned and no more."""
    from tinyfusers_amd.native import hip
    B, C, Cc, H, W = shape
    Ct, HW = C + Cc, H * W
    rng = np.random.default_rng(B * 1000 + Cc * 100 + H)
    lat = (3 * rng.standard_normal((B, C, H, W))).astype(np.float32)
    cond = rng.standard_normal((B, Cc, H, W)).astype(np.float32)
    cond[0, 0, 0, :4] = [-0.0, 3e-6, 70000.0, -1.0]                  # -0 (kept where the group keeps cond), an fp16 subnormal, past the fp16 range
    lat[0, 1, 1, :2] = [0.333251953125 + 2.0 ** -13, -0.0]          # a tie in fp16's 11 bits: round to even
    d_lat = tf.DeviceArray.from_numpy(lat, np.float32, "row")
    d_cond = tf.DeviceArray.from_numpy(cond, np.float32, "row")
    concat = hip.tf_cfg_concat_bf16 if dtype == "bf16" else hip.tf_cfg_concat_f16
    dup = hip.tf_cfg_duplicate_bf16 if dtype == "bf16" else hip.tf_cfg_duplicate_f16
    d_dup = _raw16(tf, 2 * B * HW * C, 0)
    dup(d_dup.ptr, d_lat.ptr, B, C, H, W, None)
    dup_bits = _read16(d_dup).reshape(2, B, HW, C)
    assert np.array_equal(dup_bits[0], dup_bits[1])
    front, back, fill = 3, 64, 0x7E55
    for groups in (2, 3):
        for drop in (0, 1, 0b101):
            n = groups * B * HW * Ct
            buf = _raw16(tf, front + n + back, fill)
            concat(buf.ptr + 2 * front, d_lat.ptr, d_cond.ptr, B, C, Cc, H, W, groups, drop, None)
            got = _read16(buf)
            assert np.all(got[:front] == fill) and np.all(got[front + n:] == fill), (groups, drop)      # the guard regions are untouched
            got = got[front:front + n].reshape(groups, B, HW, Ct)
            for g in range(groups):
                dropped = bool((drop >> g) & 1)
                full = np.concatenate([lat, np.zeros_like(cond) if dropped else cond], axis=1)           # (B, Ct, H, W)
                want = _bits16(full.transpose(0, 2, 3, 1), dtype).reshape(B, HW, Ct)
                assert np.array_equal(got[g], want), (groups, drop, g)
                assert np.array_equal(got[g][..., :C], dup_bits[0]), (groups, drop, g)                    # tf_cfg_duplicate_*'s rounding
                if dropped:
                    assert np.all(got[g][..., C:] == 0), (groups, drop, g)                                # +0: no sign bit
    with pytest.raises(RuntimeError, match="groups"):
        concat(buf.ptr, d_lat.ptr, d_cond.ptr, B, C, Cc, H, W, 4, 0, None)
    with pytest.raises(RuntimeError, match="bad arguments"):
        concat(buf.ptr, d_lat.ptr, None, B, C, Cc, H, W, 2, 0, None)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_latent_stack_grid_stride_loop_matches_the_host_construction(tf, dtype):
    """(3, 4, 256, 256) with 5 conditioning channels: 786432 elements per group for tf_cfg_duplicate_*, 1769472 for tf_cfg_concat_* -- both past the
    2048 x 256 threads of the largest grid, so threads take a second (and a fourth) trip.  Two groups against the host cast of the test above."""
    from tinyfusers_amd.native import hip
    B, C, Cc, H, W = 3, 4, 5, 256, 256
    rng = np.random.default_rng(31)
    lat = 3 * rng.standard_normal((B, C, H, W), dtype=np.float32)
    cond = rng.standard_normal((B, Cc, H, W), dtype=np.float32)
    d_lat = tf.DeviceArray.from_numpy(lat, np.float32, "row")
    d_cond = tf.DeviceArray.from_numpy(cond, np.float32, "row")
    n = B * H * W * C
    d_dup = _raw16(tf, 2 * n, 0x7E55)
    (hip.tf_cfg_duplicate_bf16 if dtype == "bf16" else hip.tf_cfg_duplicate_f16)(d_dup.ptr, d_lat.ptr, B, C, H, W, None)
    want = _bits16(lat.transpose(0, 2, 3, 1), dtype).reshape(-1)
    got = _read16(d_dup).reshape(2, n)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
    n = B * H * W * (C + Cc)
    d_cat = _raw16(tf, 2 * n, 0x7E55)
    (hip.tf_cfg_concat_bf16 if dtype == "bf16" else hip.tf_cfg_concat_f16)(d_cat.ptr, d_lat.ptr, d_cond.ptr, B, C, Cc, H, W, 2, 0b01, None)
    got = _read16(d_cat).reshape(2, n)
    for g, kept in enumerate((np.zeros_like(cond), cond)):          # group 0 drops the conditioning
        want = _bits16(np.concatenate([lat, kept], axis=1).transpose(0, 2, 3, 1), dtype).reshape(-1)
        assert np.array_equal(got[g], want), g


# ---- 2. tf_image_from_u8_masked_f16 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(3, 5), (16, 24)])
def test_image_from_u8_masked_keeps_unmasked_pixels_and_zeroes_the_rest(tf, hw):
    from tinyfusers_amd.native import hip
    H, W = hw
    B = 2
    rng = np.random.default_rng(H)
    u = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    u.reshape(-1)[:90] = np.r_[np.arange(45), np.arange(211, 256)]
    m = (rng.random((B, H, W)) < 0.4).astype(np.uint8) * rng.integers(1, 256, (B, H, W)).astype(np.uint8)     # any nonzero byte masks
    m[0, 0, 0], m[0, 0, 1] = 0, 255
    d_u, d_m = tf.DeviceArray.from_numpy(u, np.uint8, "row"), tf.DeviceArray.from_numpy(m, np.uint8, "row")
    n = u.size
    plain, masked = _raw16(tf, n, 0x7E55), _raw16(tf, n + 16, 0x7E55)
    hip.tf_image_from_u8_f16(plain.ptr, d_u.ptr, n, None)
    hip.tf_image_from_u8_masked_f16(masked.ptr, d_u.ptr, d_m.ptr, B, H, W, None)
    p, g = _read16(plain).reshape(B, H, W, 3), _read16(masked)
    assert np.all(g[n:] == 0x7E55)
    g = g[:n].reshape(B, H, W, 3)
    keep = m == 0
    assert keep.any() and (~keep).any()
    assert np.array_equal(g[keep], p[keep])                          # bit-equal to tf_image_from_u8_f16
    assert np.array_equal(p, np.float16(u / 127.5 - 1).view(np.uint16))
    assert np.all(g[~keep] == 0)                                     # exactly +0


# ---- 3. tf_means_to_cond_f32 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(3, 5), (8, 8)])
def test_means_to_cond_is_the_fp32_product_in_its_channels(tf, hw):
    from tinyfusers_amd.native import hip
    H, W = hw
    B = 2
    rng = np.random.default_rng(W)
    means = (4 * rng.standard_normal((B, 4, H, W))).astype(np.float16)
    d_means = tf.DeviceArray.from_numpy(means, np.float16, "nhwc")
    m32 = means.astype(np.float32)
    for scale, off, total in ((0.18215, 1, 5), (1.0, 0, 4)):
        before = rng.standard_normal((B, total, H, W)).astype(np.float32)
        d_cond = tf.DeviceArray.from_numpy(before, np.float32, "row")
        hip.tf_means_to_cond_f32(d_cond.ptr, d_means.ptr, B, H, W, scale, off, total, None)
        got = d_cond.numpy()
        want = before.copy()
        want[:, off:off + 4] = np.float32(scale) * m32              # one fp32 multiply: exact
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (scale, off, total)
        if off:
            assert np.array_equal(got[:, 0], before[:, 0])           # the mask channel is not this kernel's
    a, b = (tf.DeviceArray.zeros((B, 4, H, W), np.float32, "row") for _ in range(2))
    hip.tf_means_to_cond_f32(a.ptr, d_means.ptr, B, H, W, 0.18215, 0, 4, None)
    hip.tf_means_to_latent_f32(b.ptr, d_means.ptr, B, H, W, None)
    assert np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32))
    with pytest.raises(RuntimeError, match="channels"):
        hip.tf_means_to_cond_f32(a.ptr, d_means.ptr, B, H, W, 1.0, 1, 4, None)


# ---- 4. one three-branch update ---------------------------------------------------------------------------------------------------------
def _set_params(hip, sp, t, a_t, a_p, g, row, seed, offset):
    lo, hi = _words(seed)
    hip.tf_set_sampler_params(sp.ptr, float(t), float(a_t), float(a_p), float(g), row, lo, hi, offset, None, None, 0, None)


def _cfg3_ref(x, eps3, hist, a_t, g_t, g_i, row, z):
    """float64: e = e0 + g_T (e2 - e1) + g_I (e1 - e0), x0 = (x - sqrt(1-a_t) e)/sqrt(a_t), x' = c_x x + c_0 x0 + c_1 x0_prev + c_n z."""
    b = x.shape[0]
    e0, e1, e2 = eps3[:b], eps3[b:2 * b], eps3[2 * b:]
    g_t, g_i = np.float64(np.float32(g_t)), np.float64(np.float32(g_i))
    e = e0 + g_t * (e2 - e1) + g_i * (e1 - e0)
    a_t = np.float64(np.float32(a_t))
    x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
    c_x, c_0, c_1, c_n = (np.float64(np.float32(c)) for c in row)
    return c_x * x + c_0 * x0 + (c_1 * hist if c_1 != 0 else 0.0) + c_n * z, x0


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["ddim-eta", "euler-a", "dpmpp2m"])
def test_one_three_branch_sampler_step_matches_float64(tf, name, dtype):
    """The form of test_one_masked_sampler_step_matches_float64, at its gate 1e-5 (1 + |ref|): the three-way combine adds one fp32 multiply-add of
    the same magnitude to arithmetic that gate already covers."""
    from tinyfusers_amd.native import hip
    from tinyfusers_amd.storage.tensor import bfloat16
    from tinyfusers_amd.variants import samplers as S
    for B, C, H, W in ((2, 4, 8, 12), (2, 3, 5, 7)):             # (105 elements per image: a partial last counter)
        n_img, offset = C * H * W, 5
        sch = S.make(name).schedule(25, strength=0.8)
        i = 9
        table = sch.coeffs.copy()
        table[i, 2] = table[i, 2] or 0.25                            # every term live: c_1 != 0 and c_n != 0
        table[i, 3] = table[i, 3] or 0.6
        rng = np.random.default_rng(4)
        x, hist = (rng.standard_normal((B, C, H, W)).astype(np.float32) for _ in range(2))
        dt = bfloat16 if dtype == "bf16" else np.float16
        d_eps = tf.DeviceArray.from_numpy(rng.standard_normal((3 * B, C, H, W)), dt, "nhwc")
        eps3 = d_eps.numpy().astype(np.float64)                      # the values the kernel reads
        d_tab = tf.DeviceArray.from_numpy(table.astype(np.float32), np.float32, "row")
        sp = tf.DeviceArray.zeros((8,), np.float32, "row")
        edit = tf.DeviceArray.zeros((4,), np.float32, "row")
        three = hip.tf_cfg3_sampler_step_bf16 if dtype == "bf16" else hip.tf_cfg3_sampler_step_f32
        two = hip.tf_cfg_sampler_step_bf16 if dtype == "bf16" else hip.tf_cfg_sampler_step_f32

        def run(eps, lo_img, hi_img, g_i, off=offset, branches=3):
            sl = slice(lo_img, hi_img)
            nb = hi_img - lo_img
            lat = tf.DeviceArray.from_numpy(x[sl], np.float32, "row")
            h = tf.DeviceArray.from_numpy(hist[sl], np.float32, "row")
            e = tf.DeviceArray.from_numpy(np.concatenate([eps[k * B + lo_img:k * B + hi_img] for k in range(eps.shape[0] // B)]), dt, "nhwc")
            _set_params(hip, sp, sch.timesteps[i], sch.alphas[i], sch.alphas_prev[i], G_T, i, SEED, off)
            if branches == 3:
                hip.tf_set_step_params(edit.ptr, float(g_i), 0.0, 0.0, 0.0, None)
                three(lat.ptr, e.ptr, h.ptr, sp.ptr, d_tab.ptr, len(table), edit.ptr, nb, C, H, W, None)
            else:
                two(lat.ptr, e.ptr, h.ptr, sp.ptr, d_tab.ptr, len(table), nb, C, H, W, None)
            return lat.numpy(), h.numpy()

        z = np.stack([randn_ref(SEED, offset + b, n_img, i, 1).reshape(C, H, W) for b in range(B)])
        got, got_h = run(eps3, 0, B, G_I)
        ref, ref_x0 = _cfg3_ref(x, eps3, hist, sch.alphas[i], G_T, G_I, table[i], z)
        print(f"three-branch {name} {dtype}: max |d| / (1 + |ref|) latent {float(np.max(np.abs(got - ref) / (1 + np.abs(ref)))):.2e}, "
              f"x0 {float(np.max(np.abs(got_h - ref_x0) / (1 + np.abs(ref_x0)))):.2e} (gate 1e-5)")
        assert np.all(np.abs(got - ref) <= 1e-5 * (1 + np.abs(ref))), float(np.max(np.abs(got - ref) / (1 + np.abs(ref))))
        assert np.all(np.abs(got_h - ref_x0) <= 1e-5 * (1 + np.abs(ref_x0)))
        # batch independence: image 1 alone, as global image offset + 1
        one, one_h = run(eps3, 1, 2, G_I, off=offset + 1)
        assert np.array_equal(one[0], got[1]) and np.array_equal(one_h[0], got_h[1])
        # g_I = 1 with e1 := e0 is the two-branch update on [e0 ; e2] (to the gate: FMA contraction may differ between the two kernels)
        same = np.concatenate([eps3[:B], eps3[:B], eps3[2 * B:]])
        a, ah = run(same, 0, B, 1.0)
        b, bh = run(np.concatenate([eps3[:B], eps3[2 * B:]]), 0, B, None, branches=2)
        assert np.all(np.abs(a - b) <= 1e-5 * (1 + np.abs(b))) and np.all(np.abs(ah - bh) <= 1e-5 * (1 + np.abs(bh)))
        with pytest.raises(RuntimeError, match="bad arguments"):
            three(sp.ptr, d_eps.ptr, sp.ptr, sp.ptr, d_tab.ptr, len(table), None, B, C, H, W, None)


# ---- 5. - 7. tiny concat-conditioned UNets -----------------------------------------------------------------------------------------------
def _tiny(cin, seed=5):
    import oracle
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    cfg = replace(oracle.TINY, in_channels=cin)
    W = synth_state_dict(oracle.unet_param_shapes(cfg), seed)
    ctx = synth_normal(seed, "c", (2, 13, 64)).astype(np.float16).astype(np.float32)
    unc = synth_normal(seed, "u", (2, 13, 64)).astype(np.float16).astype(np.float32)
    cc = cin - 4
    cond = synth_normal(seed, "cond", (2, cc, 16, 16)).astype(np.float16).astype(np.float32)     # (16-bit values: the step reads them rounded)
    if cin == 9:
        cond[:, 0] = 0.0
        cond[:, 0, :, :8] = 1.0                                   # a half mask in channel 0
    return cfg, W, ctx, unc, cond


def _oracle_trajectory(cfg, W, unc, ctx, lat0, cond, sch, seed, g_t=G_T, g_i=None):
    """The sampler of tests/test_gpu_samplers.py on the CPU oracle's UNet fed concatenate([x, cond]): two groups [x|c, unc ; x|c, ctx], or with
    g_i three groups [x|0, unc ; x|c, unc ; x|c, ctx] and e = e0 + g_T (e2 - e1) + g_I (e1 - e0)."""
    import oracle
    Wf = {k: torch.from_numpy(v.astype(np.float32)) for k, v in W.items()}
    x, xp = lat0.astype(np.float64), np.zeros(lat0.shape)
    B, n_img = lat0.shape[0], lat0[0].size
    cstack = np.concatenate([unc, ctx] if g_i is None else [unc, unc, ctx])
    for i, t in enumerate(sch.timesteps):
        x32 = x.astype(np.float32)
        xc = np.concatenate([x32, cond], axis=1)
        xin = np.concatenate([xc, xc] if g_i is None else [np.concatenate([x32, np.zeros_like(cond)], axis=1), xc, xc])
        out = oracle.unet_forward(xin, np.array([t], np.float32), cstack, Wf, cfg).numpy().astype(np.float64)
        if g_i is None:
            e = out[:B] + g_t * (out[B:] - out[:B])
        else:
            e = out[:B] + g_t * (out[2 * B:] - out[B:2 * B]) + g_i * (out[B:2 * B] - out[:B])
        a_t = sch.alphas[i]
        x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
        z = np.stack([randn_ref(seed, b, n_img, i, 1).reshape(lat0.shape[1:]) for b in range(B)])
        c_x, c_0, c_1, c_n = sch.coeffs[i]
        x, xp = c_x * x + c_0 * x0 + c_1 * xp + c_n * z, x0
    return x


def _model(tf, cin, W, unc, ctx, sch, concat, hw=(16, 16), batch=2):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY
    sd = StableDiffusion(replace(TINY, in_channels=cin)); update_state(sd.model.diffusion_model, W, "")
    lat = sd.latent_from_numpy(np.zeros((batch, 4) + hw, np.float32))
    sd.compile(tf.DeviceArray.from_numpy(unc[:batch]), tf.DeviceArray.from_numpy(ctx[:batch]), lat, sampler=sch, concat=concat)
    return sd, lat


def _runs(tf, sd, lat, cond, **kw):
    """graph, eager (the conditioning as a device array), graph again: the three final latents, and the initial latent."""
    outs = []
    for k, eager in enumerate((False, True, False)):
        sd.start(seed=SEED, cond_latent=cond if k != 1 else tf.DeviceArray.from_numpy(cond, np.float32, "row"), **kw)
        if not outs:
            lat0 = lat.numpy().copy()
        sd.run(G_T, eager=eager); sd.synchronize()
        outs.append(lat.numpy().copy())
    return lat0, outs


@pytest.mark.parametrize("name", ["dpmpp2m", "euler-a"])
def test_tiny_inpainting_checkpoint_graph_eager_seed_and_oracle(tf, name):
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    cfg, W, ctx, unc, cond = _tiny(9)
    sch = S.make(name).schedule(10, strength=0.6)                # the 6 steps of the img2img trajectories, here from the seed's noise
    assert len(sch.timesteps) == 6
    sd, lat = _model(tf, 9, W, unc, ctx, sch, "inpaint")
    lat0, outs = _runs(tf, sd, lat, cond)
    np.testing.assert_array_equal(lat0, StableDiffusion.randn_latent((2, 4, 16, 16), SEED).numpy())
    np.testing.assert_array_equal(outs[0], outs[1])              # graph replay == eager
    np.testing.assert_array_equal(outs[0], outs[2])              # same seed, same image
    _gate(outs[0], _oracle_trajectory(cfg, W, unc, ctx, lat0, cond, sch, SEED))
    other = cond.copy()
    other[:, 0] = 1.0 - other[:, 0]
    other[:, 1:] = other[:, 1:][:, ::-1]
    sd.start(seed=SEED, cond_latent=other)
    sd.run(G_T); sd.synchronize()
    d = float(np.abs(lat.numpy() - outs[0]).max())
    print(f"another cond_latent moves the latent by max |d| = {d:.3f}")
    assert d > 0.1                                               # the conditioning is read (identical runs agree bit for bit)


def test_tiny_inpainting_checkpoint_in_the_bf16_step(tf):
    """The DPM++2M run above in the bfloat16 step, once, at the bf16 gates of test_tiny_unet_inpainting_in_the_bf16_step and over the schedule
    those gates were set for: the full 10 steps from noise (they bound max |d| by max |ref| of a trajectory that grows to |x| ~ 25)."""
    from tinyfusers_amd import config
    from tinyfusers_amd.variants import samplers as S
    cfg, W, ctx, unc, cond = _tiny(9)
    sch = S.DPMSolverPP2M().schedule(10)
    config.set_dtype("bf16")
    try:
        sd, lat = _model(tf, 9, W, unc, ctx, sch, "inpaint")
        lat0, outs = _runs(tf, sd, lat, cond)
    finally:
        config.set_dtype("fp16")
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])
    _gate(outs[0], _oracle_trajectory(cfg, W, unc, ctx, lat0, cond, sch, SEED), rel_l2=3e-2, max_rel=3e-2)


@pytest.mark.parametrize("name", ["dpmpp2m", "euler-a"])
def test_tiny_edit_checkpoint_three_groups_graph_eager_and_oracle(tf, name):
    """The gate is the project's for this network and step count, derived: the combine weights the three UNet outputs by (1 - g_I, g_I - g_T, g_T)
    = (-0.5, -6, 7.5), norm 9.6; the two-way step weights its two by (-6.5, 7.5), norm 9.9 -- rounding error is amplified no more than there."""
    from tinyfusers_amd.variants import samplers as S
    cfg, W, ctx, unc, cond = _tiny(8)
    sch = S.make(name).schedule(10, strength=0.6)
    assert len(sch.timesteps) == 6
    sd, lat = _model(tf, 8, W, unc, ctx, sch, "edit")
    lat0, outs = _runs(tf, sd, lat, cond)                         # g_I: compile's default, 1.5
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])
    _gate(outs[0], _oracle_trajectory(cfg, W, unc, ctx, lat0, cond, sch, SEED, g_i=G_I))
    if name != "dpmpp2m":
        return
    # image_guidance= is read, stream-ordered, and kept until the next value
    sd.start(seed=SEED, cond_latent=cond, image_guidance=1.0)
    sd.run(G_T); sd.synchronize()
    g1 = lat.numpy().copy()
    assert float(np.abs(g1 - outs[0]).max()) > 0.05
    _gate(g1, _oracle_trajectory(cfg, W, unc, ctx, lat0, cond, sch, SEED, g_i=1.0))
    sd.start(seed=SEED, cond_latent=cond)
    sd.run(G_T); sd.synchronize()
    np.testing.assert_array_equal(lat.numpy(), g1)
    # set_context on the compiled three-group model == a fresh compile with those contexts
    unc2, ctx2 = ctx[::-1].copy(), (0.5 * unc).astype(np.float16).astype(np.float32)
    sd.set_context(tf.DeviceArray.from_numpy(unc2), tf.DeviceArray.from_numpy(ctx2))
    sd.start(seed=SEED, cond_latent=cond, image_guidance=G_I)
    sd.run(G_T); sd.synchronize()
    swapped = lat.numpy().copy()
    fresh, flat = _model(tf, 8, W, unc2, ctx2, sch, "edit")
    fresh.start(seed=SEED, cond_latent=cond)
    fresh.run(G_T); fresh.synchronize()
    np.testing.assert_array_equal(swapped, flat.numpy())
    assert float(np.abs(swapped - outs[0]).max()) > 0.05


# ---- 8. the conditioning path through the VAE encoder -------------------------------------------------------------------------------------
@pytest.mark.parametrize("concat", ["inpaint", "edit"])
def test_start_from_cond_image_fills_the_conditioning_buffer(tf, vae_sd, concat):
    import oracle
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    cin = 9 if concat == "inpaint" else 8
    cfg, W, ctx, unc, _ = _tiny(cin)
    vae, Wv = vae_sd
    sd, lat = _model(tf, cin, W, unc, ctx, S.DPMSolverPP2M().schedule(2), concat, batch=1)
    with pytest.raises(RuntimeError, match="first_stage_model"):
        sd.start(seed=SEED, cond_image=np.zeros((1, 128, 128, 3), np.uint8), cond_mask=np.zeros((1, 128, 128), bool) if cin == 9 else None)
    sd.first_stage_model = vae.first_stage_model                  # the synthetic VAE (a tiny UNet configuration builds none of its own)
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (1, 128, 128, 3), dtype=np.uint8)
    mask = np.zeros((1, 128, 128), np.float32)
    mask[0, 8:72, 3:67] = 1.0                                      # edges off the 8-pixel grid: the nearest rule and the block maximum differ
    kw = {"cond_mask": mask} if cin == 9 else {}
    sd.start(seed=SEED, cond_image=img, **kw)
    sd.synchronize()
    got = sd._cond.numpy()
    Wf = {k: v.astype(np.float16).astype(np.float32) for k, v in Wv.items()}
    xin = np.float16(img / 127.5 - 1).astype(np.float32).transpose(0, 3, 1, 2)
    if cin == 9:
        xin = xin * (1.0 - mask[:, None])
        want_mask = StableDiffusion.concat_mask(mask)
        assert not np.array_equal(want_mask, StableDiffusion.latent_mask(mask))
        assert got.shape == (1, 5, 16, 16) and np.array_equal(got[:, :1], want_mask)           # the mask channel is exact
        means, scale = got[:, 1:], 0.18215
    else:
        assert got.shape == (1, 4, 16, 16)
        means, scale = got, 1.0
    ref = scale * oracle.autoencoder_kl(xin, Wf)[0].numpy().astype(np.float64)
    rl = float(np.linalg.norm(means - ref) / np.linalg.norm(ref))
    print(f"start(cond_image=) {concat}: rel-L2 {rl:.2e} against {scale} x the oracle's means")
    assert np.isfinite(got).all() and rl < 5e-3
    # a device image gives the same buffer; the sampler then runs from it
    sd.start(seed=SEED, cond_image=tf.DeviceArray.from_numpy(img, np.uint8, "row"), **kw)
    sd.synchronize()
    assert np.array_equal(sd._cond.numpy(), got)
    sd.run(G_T); sd.synchronize()
    assert np.isfinite(lat.numpy()).all()


# ---- 9. argument checks -------------------------------------------------------------------------------------------------------------------
def test_concat_arguments_are_checked_and_a_refusal_leaves_the_model_running(tf, vae_sd):
    from tinyfusers_amd import config
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY
    sch = S.DPMSolverPP2M().schedule(2)
    cfg9, W9, ctx, unc, cond9 = _tiny(9)
    d_ctx, d_unc = tf.DeviceArray.from_numpy(ctx), tf.DeviceArray.from_numpy(unc)
    new_lat = lambda: StableDiffusion.latent_from_numpy(np.zeros((2, 4, 16, 16), np.float32))
    nine, eight, four = (StableDiffusion(replace(TINY, in_channels=c)) for c in (9, 8, 4))
    with pytest.raises(ValueError, match="sampler"):
        nine.compile(d_unc, d_ctx, new_lat(), concat="inpaint")
    with pytest.raises(ValueError, match="in_channels=8"):
        nine.compile(d_unc, d_ctx, new_lat(), sampler=sch, concat="edit")
    with pytest.raises(ValueError, match="in_channels=9"):
        eight.compile(d_unc, d_ctx, new_lat(), sampler=sch, concat="inpaint")
    with pytest.raises(ValueError, match="in_channels=9"):
        four.compile(d_unc, d_ctx, new_lat(), sampler=sch, concat="inpaint")
    with pytest.raises(ValueError, match="concat-conditioned"):
        nine.compile(d_unc, d_ctx, new_lat(), sampler=sch)
    with pytest.raises(ValueError, match="concat-conditioned"):
        eight.compile(d_unc, d_ctx, new_lat())
    with pytest.raises(ValueError, match="inpaint=True"):
        nine.compile(d_unc, d_ctx, new_lat(), sampler=sch, concat="inpaint", inpaint=True)
    old = config.cfg_parallel
    config.cfg_parallel = True
    try:
        with pytest.raises(S.UnsupportedSamplerConfig):
            nine.compile(d_unc, d_ctx, new_lat(), sampler=sch, concat="inpaint")
    finally:
        config.cfg_parallel = old
    # start() on a compiled inpainting model
    sd, lat = _model(tf, 9, W9, unc, ctx, sch, "inpaint")
    sd.first_stage_model = vae_sd[0].first_stage_model
    sd.start(seed=SEED, cond_latent=cond9)
    sd.run(G_T); sd.synchronize()
    want, cond_before = lat.numpy().copy(), sd._cond.numpy().copy()
    img, m = np.zeros((2, 128, 128, 3), np.uint8), np.zeros((2, 128, 128), bool)
    for kw, match in (({}, "conditioning"),                                               # no conditioning at all
                      ({"cond_image": img}, "cond_mask"),                                  # an inpainting image without its mask
                      ({"cond_mask": m}, "cond_image"),                                    # a mask without an image
                      ({"cond_mask": m, "cond_latent": cond9}, "cond_image"),
                      ({"cond_image": img, "cond_mask": m, "cond_latent": cond9}, "not both"),
                      ({"cond_latent": cond9, "image_guidance": 1.5}, "concat='edit'"),
                      ({"cond_latent": cond9[:, :4]}, "shape"),
                      ({"cond_latent": tf.DeviceArray.from_numpy(cond9[:1], np.float32, "row")}, "device cond_latent"),
                      ({"cond_image": img[:, :64], "cond_mask": m[:, :64]}, "cond_image must be"),
                      ({"cond_image": img.astype(np.float32), "cond_mask": m}, "uint8"),
                      ({"cond_image": img, "cond_mask": m[:, :64]}, "cond_mask is"),
                      ({"cond_latent": cond9, "init_latent": cond9[:, :4], "noise": cond9[:, :4]}, "seed")):     # a latent-side refusal
        with pytest.raises(ValueError, match=match):
            sd.start(seed=SEED, **kw)
    with pytest.raises(TypeError):
        sd.start(seed=SEED, cond_image=img, cond_mask=np.zeros((2, 128, 128), np.int32))
    assert np.array_equal(sd._cond.numpy(), cond_before)          # every refusal came before anything was written
    sd.start(seed=SEED, cond_latent=cond9)                        # ... and the model still runs a normal step
    sd.run(G_T); sd.synchronize()
    assert np.array_equal(lat.numpy(), want)
    # img2img on the inpainting checkpoint: the conditioning arguments are orthogonal to the init ones
    sd.start(seed=SEED, init_latent=cond9[:, 1:], cond_latent=cond9)
    sd.run(G_T); sd.synchronize()
    assert np.isfinite(lat.numpy()).all() and not np.array_equal(lat.numpy(), want)
    # an edit model refuses a mask; a model without concat refuses all four arguments
    cfg8, W8, _, _, cond8 = _tiny(8)
    ed, _ = _model(tf, 8, W8, unc, ctx, sch, "edit")
    with pytest.raises(ValueError, match="cond_mask"):
        ed.start(seed=SEED, cond_image=img, cond_mask=m)
    with pytest.raises(ValueError, match="image_guidance"):
        ed.start(seed=SEED, cond_latent=cond8, image_guidance=float("nan"))
    import oracle
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_state_dict
    update_state(four.model.diffusion_model, synth_state_dict(oracle.unet_param_shapes(oracle.TINY), 5), "")
    lat4 = new_lat()
    four.compile(d_unc, d_ctx, lat4, sampler=sch)
    for kw in ({"cond_latent": cond8}, {"cond_image": img}, {"cond_mask": m}, {"image_guidance": 1.5}):
        with pytest.raises(ValueError, match="concat="):
            four.start(seed=SEED, **kw)
    four.start(seed=SEED)
    four.run(G_T); four.synchronize()
    assert np.isfinite(lat4.numpy()).all()


# ---- 10. SD-1.5 shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("concat", ["inpaint", "edit"])
def test_sd15_concat_checkpoint_two_steps_from_an_image_at_512(tf, vae_sd, concat):
    import oracle
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.variants.samplers import DPMSolverPP2M
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import SD15_EDIT, SD15_INPAINT
    cfg = SD15_INPAINT if concat == "inpaint" else SD15_EDIT
    sd = StableDiffusion(cfg)
    assert sd.first_stage_model is not None and sd.cond_stage_model is not None
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(sd.model.diffusion_model, synth_state_dict(oracle.unet_param_shapes(replace(oracle.SD15, in_channels=cfg.in_channels)), 0), "")
        update_state(sd.first_stage_model, vae_sd[1], "first_stage_model")
    img = np.random.default_rng(9).integers(0, 256, (1, 512, 512, 3), dtype=np.uint8)
    kw = {}
    if concat == "inpaint":
        kw["cond_mask"] = np.zeros((1, 512, 512), bool)
        kw["cond_mask"][0, 100:300, 200:450] = True
    ctx = tf.DeviceArray.from_numpy(synth_normal(1234, "sd.context", (1, 77, 768)))
    unc = tf.DeviceArray.from_numpy(synth_normal(1234, "sd.uncond", (1, 77, 768)))
    sch = DPMSolverPP2M().schedule(2)
    assert len(sch.timesteps) == 2
    lat = sd.latent_from_numpy(np.zeros((1, 4, 64, 64), np.float32))
    sd.compile(unc, ctx, lat, sampler=sch, concat=concat)
    outs = []
    for eager in (False, True):
        sd.start(seed=SEED, cond_image=img, **kw)
        sd.run(G_T, eager=eager); sd.synchronize()
        outs.append(lat.numpy().copy())
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1])
    cond = sd._cond.numpy()
    assert np.isfinite(cond).all() and np.abs(cond[:, -4:]).max() > 0
    if concat == "inpaint":
        assert np.array_equal(cond[:, :1], StableDiffusion.concat_mask(kw["cond_mask"]))
    with tf.use_stream(sd._stream):
        image = sd.decode(lat)
    assert image.shape == (512, 512, 3) and image.dtype == np.uint8
