"""GPU checks of the LoRA adapter path (csrc/lora.hip, storage/lora.py, StableDiffusion.load_lora / set_adapters / adapters / unload_lora): the
merge kernel against float64 (tests/aux/lora_ref.py) on ragged, multi-adapter and multi-K-step shapes; tiny-UNet trajectories with adapters over
every target (merge then compile, compile then merge = a re-captured step, two adapters, weights alone, removal, bf16, with a ControlNet)
against the CPU oracle fed the float64-merged weights; the SD-1.5 text encoder; and the SD-1.5 shapes once, from a file."""
import contextlib
import ctypes
import functools
import io
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "aux"))
import controlnet_oracle as C  # noqa: E402
import lora_ref as R  # noqa: E402
from test_gpu_controlnet import G, SEED, _f32, _from16, _gate, _hint_of, _raw16, _read16, _tiny, _to16  # noqa: E402
from test_samplers_host import randn_ref  # noqa: E402


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


# ---- 1. tf_lora_merge_16 ------------------------------------------------------------------------------------------------------------------------
SHAPES = (
    (4, 36, (4,), (0.7,)),                                  # both dimensions ragged and below one tile: conv_out, and the 4-channel conv_in's Kd
    (72, 40, (4,), (0.7,)),                                 # ragged edge tiles
    (64, 576, (8, 16), (0.7, -0.4)),                        # two adapters of different rank, a 3x3 conv row
    (320, 768, (128,), (0.7,)),                             # several K steps of the MFMA
    (136, 264, (4,) * 8, (0.7, -0.4, 0.3, -0.2, 0.5, -0.6, 0.1, -0.9)),      # the 8-adapter limit
    (5, 37, (4,), (0.7,)),                                  # Kd % 4 != 0: the element-wise loads and stores
)
GUARD, FILL = 64, 0x7E55


def _operands(rng, n, kd, ranks, dtype):
    """base 3 N(0,1) with planted values, up / down N(0,1), all rounded to the element type: (bits, float64 values) each; up (N, Rp) and down_t
    (Kd, Rp) zero-padded along the rank."""
    b = (3 * rng.standard_normal(n * kd)).astype(np.float32)
    b[:4] = [0.0, -0.0, 6e-6, 1000.0]
    base = _to16(b.reshape(n, kd), dtype)
    ads = []
    for r in ranks:
        rp = (r + 31) // 32 * 32
        up, dn = np.zeros((n, rp), np.float32), np.zeros((kd, rp), np.float32)
        up[:, :r], dn[:, :r] = rng.standard_normal((n, r)), rng.standard_normal((kd, r))
        ads.append((_to16(up, dtype), _to16(dn, dtype), rp))
    return base, ads


def _merge(tf, dtype, base_bits, ads, scales):
    """One launch -> (dst bits, base bits read back); checks the guard words behind dst."""
    from tinyfusers_amd.native import LoraEntry, hip
    n, kd = base_bits.shape
    d_base = _raw16(tf, base_bits.reshape(-1))
    d_dst = _raw16(tf, np.full(n * kd + GUARD, FILL, np.uint16))
    keep = [(_raw16(tf, u[0].reshape(-1)), _raw16(tf, d[0].reshape(-1))) for u, d, _ in ads]
    table = (LoraEntry * len(ads))()
    for e, (du, dd), (_, _, rp), s in zip(table, keep, ads, scales):
        e.up, e.down_t, e.rp, e.scale = du.ptr, dd.ptr, rp, float(s)
    hip.tf_lora_merge_16(1 if dtype == "bf16" else 0, d_dst.ptr, d_base.ptr, ctypes.cast(table, ctypes.c_void_p), len(ads), n, kd, None)
    out = _read16(d_dst)
    assert np.all(out[n * kd:] == FILL), (n, kd)
    assert np.array_equal(_read16(d_base), base_bits.reshape(-1))           # base is read only
    return out[:n * kd].reshape(n, kd)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_lora_merge_matches_float64_on_ragged_multi_adapter_and_multi_k_shapes(tf, dtype):
    """|got - ref| <= rel |ref| + n 2^-24 S + 2^-24 (lora_ref.merge_bound): rel one unit in the last place of the 16-bit type, n = sum Rp_i +
    2 adapters + 1 the length of the fp32 chain, S = |base| + sum |s_i| sum |up| |down| in float64."""
    rng = np.random.default_rng(23)
    for n, kd, ranks, scales in SHAPES:
        base, ads = _operands(rng, n, kd, ranks, dtype)
        s32 = [np.float32(s) for s in scales]
        got = _merge(tf, dtype, base[0], ads, s32)
        ref, mag = base[1].copy(), np.abs(base[1])
        for (u, d, _), s in zip(ads, s32):
            ref += np.float64(s) * (u[1] @ d[1].T)
            mag += abs(np.float64(s)) * (np.abs(u[1]) @ np.abs(d[1]).T)
        bound = R.merge_bound(ref, mag, ranks, dtype)
        err = np.abs(_from16(got, dtype) - ref)
        print(f"lora_merge {dtype} N={n} Kd={kd} ranks={list(ranks)}: worst err / bound = {float(np.max(err / bound)):.3f} (bound 1)")
        assert np.all(err <= bound), (n, kd, ranks)
        assert np.array_equal(_merge(tf, dtype, base[0], ads, s32), got)    # two launches: the same bits
        zero = _merge(tf, dtype, base[0], ads, [0.0] * len(ads))
        assert np.array_equal(zero, base[0])                                # every scale 0: base's bits, -0 and the subnormal included
        assert zero.reshape(-1)[1] == 0x8000


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_lora_merge_scale_zero_contributes_nothing_whatever_the_adapter_holds(tf, dtype):
    rng = np.random.default_rng(29)
    n, kd = 72, 40
    base, ads = _operands(rng, n, kd, (4, 8), dtype)
    inf = 0x7F80 if dtype == "bf16" else 0x7C00
    ads[1][0][0][3, 1], ads[1][1][0][5, 2] = inf, inf | 0x8000              # infinities in the adapter at scale 0: 0 * inf would be NaN
    alone = _merge(tf, dtype, base[0], ads[:1], [0.7])
    assert np.array_equal(_merge(tf, dtype, base[0], ads, [0.7, 0.0]), alone)
    assert np.array_equal(_merge(tf, dtype, base[0], ads[::-1], [0.0, 0.7]), alone)


def test_lora_merge_checks_its_arguments(tf):
    from tinyfusers_amd.native import LoraEntry, hip
    buf = _raw16(tf, np.zeros(4096, np.uint16))
    other = _raw16(tf, np.zeros(4096, np.uint16))
    table = (LoraEntry * 9)()
    for e in table:
        e.up, e.down_t, e.rp, e.scale = buf.ptr, buf.ptr, 32, 1.0
    tp = ctypes.cast(table, ctypes.c_void_p)
    for args, match in (((0, None, buf.ptr, tp, 1, 8, 8), "null pointer"), ((0, other.ptr, None, tp, 1, 8, 8), "null pointer"),
                        ((0, other.ptr, buf.ptr, None, 1, 8, 8), "null pointer"), ((0, other.ptr, buf.ptr, tp, 0, 8, 8), "n_adapters=0"),
                        ((0, other.ptr, buf.ptr, tp, 9, 8, 8), "n_adapters=9"), ((0, buf.ptr, buf.ptr, tp, 1, 8, 8), "distinct"),
                        ((2, other.ptr, buf.ptr, tp, 1, 8, 8), "dtype=2"), ((0, other.ptr, buf.ptr, tp, 1, 0, 8), "N=0")):
        with pytest.raises(RuntimeError, match=match):
            hip.tf_lora_merge_16(*args, None)
    table[0].rp = 16
    with pytest.raises(RuntimeError, match="Rp=16"):
        hip.tf_lora_merge_16(0, other.ptr, buf.ptr, tp, 1, 8, 8, None)
    table[0].rp, table[0].up = 32, None
    with pytest.raises(RuntimeError, match="adapter 0 holds a null pointer"):
        hip.tf_lora_merge_16(0, other.ptr, buf.ptr, tp, 1, 8, 8, None)
    assert not _read16(other).any()                                         # nothing ran


# ---- 2. tiny UNet: trajectories -------------------------------------------------------------------------------------------------------------------
WEIGHTS_AB = [0.7, -0.4]


@functools.lru_cache(maxsize=None)
def _adapters():
    """Adapter A (rank 4) and B (rank 8, another seed) in kohya names over EVERY target of the tiny UNet -- so behind every derived cache: the fused
    + LayerNorm-folded q|k|v and to_q, the hoisted K|V GEMM, to_out, the GEGLU pack, the FF2 x proj_out product, proj_in, 3x3 convs, the 1x1-skip
    fold, the hoisted time rows, down- and upsamplers, and the ragged conv_in / conv_out -- each at ||s up down||_F = 0.05 ||W||_F."""
    from tinyfusers_amd.storage import lora as L
    from tinyfusers_amd.vision.unet import TINY, UNetModel
    W = _tiny()[0]
    paths = L.unet_target_paths(UNetModel(TINY))
    weights = {k: W[p + ".weight"] for k, p in paths.items()}
    return paths, R.make_adapter(weights, 4, 11), R.make_adapter(weights, 8, 12)


def _sched():
    from tinyfusers_amd.variants import samplers as S
    sch = S.make("dpmpp2m").schedule(10, strength=0.6)
    assert len(sch.timesteps) == 6
    return sch


def _trajectory(W, lat0, sch, Wc=None, img=None):
    """tests/test_gpu_samplers.py's sampler on the CPU oracle with the UNet weights W; Wc, img: the controlled step of tests/aux/controlnet_oracle.py."""
    import oracle
    ctx, unc = _tiny()[2:4]
    Wf = _f32(W)
    x, xp = lat0.astype(np.float64), np.zeros(lat0.shape)
    B, n_img = lat0.shape[0], lat0[0].size
    c2 = np.concatenate([unc[:B], ctx[:B]])
    if img is not None:
        Wcf = _f32(Wc)
        emb = C.hint_embedding(_hint_of(img), Wcf)
        emb2 = torch.cat([emb, emb])
    for i, t in enumerate(sch.timesteps):
        x32 = x.astype(np.float32)
        xin, tt = np.concatenate([x32, x32]), np.array([t], np.float32)
        if img is None:
            out = oracle.unet_forward(xin, tt, c2, Wf, oracle.TINY)
        else:
            out = C.unet_forward(xin, tt, c2, Wf, oracle.TINY, control=C.controlnet_forward(xin, None, tt, c2, Wcf, oracle.TINY, hint_emb=emb2))
        out = out.numpy().astype(np.float64)
        e = out[:B] + G * (out[B:] - out[:B])
        x0 = (x - np.sqrt(1 - sch.alphas[i]) * e) / np.sqrt(sch.alphas[i])
        z = np.stack([randn_ref(SEED, b, n_img, i, 1).reshape(lat0.shape[1:]) for b in range(B)])
        c_x, c_0, c_1, c_n = sch.coeffs[i]
        x, xp = c_x * x + c_0 * x0 + c_1 * xp + c_n * z, x0
    return x


@functools.lru_cache(maxsize=None)
def _lat0():
    from tinyfusers_amd.variants.sd import StableDiffusion
    return StableDiffusion.randn_latent((2, 4, 16, 16), SEED).numpy()


@functools.lru_cache(maxsize=None)
def _oracle_final(which):
    """The oracle's final latent of the 6-step DPM++2M run: 'base', 'A' (A at 1) or 'AB' (A, B at 0.7, -0.4), from weights merged in float64 and
    rounded to fp16.  Computed once per session and shared."""
    paths, A, B = _adapters()
    W = _tiny()[0]
    ads = {"base": [], "A": [(1.0, A)], "AB": [(WEIGHTS_AB[0], A), (WEIGHTS_AB[1], B)]}[which]
    return _trajectory(R.merged_state(W, paths, ads), _lat0(), _sched())


def _model(tf, compile_now=True, load=True):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY
    W, _, ctx, unc = _tiny()[:4]
    _, A, B = _adapters()
    sd = StableDiffusion(TINY); update_state(sd.model.diffusion_model, W, "")
    lat = sd.latent_from_numpy(np.zeros((2, 4, 16, 16), np.float32))
    args = (tf.DeviceArray.from_numpy(unc), tf.DeviceArray.from_numpy(ctx), lat)
    if compile_now:
        sd.compile(*args, sampler=_sched())
    if load:
        assert sd.load_lora(A, "A") == "A" and sd.load_lora(B, "B") == "B"
    return sd, lat, args


def _final(sd, lat, eager=False, **kw):
    sd.start(seed=SEED, **kw)
    sd.run(G, eager=eager); sd.synchronize()
    return lat.numpy().copy()


@functools.lru_cache(maxsize=None)
def _merged_then_compiled(tf):
    """set_adapters(["A"]) on an uncompiled model, then compile: (model, latent, the final latent of the graph run)."""
    sd, lat, args = _model(tf, compile_now=False)
    before = {k: m.weight for k, m in _targets(sd).items()}
    assert sd._graph is None
    sd.set_adapters(["A"])                                  # a model that was never compiled only swaps handles
    assert sd._graph is None and sd.adapters() == {"A": (1.0, 1.0)}
    assert all(m.weight is not before[k] and m.weight.shape == before[k].shape and m.weight.layout == before[k].layout for k, m in _targets(sd).items())
    sd.compile(*args, sampler=_sched())
    return sd, lat, _final(sd, lat)


def _targets(sd):
    from tinyfusers_amd.storage import lora as L
    return L.lora_targets(sd)


def test_the_adapters_move_the_oracle_trajectory_by_ten_times_the_gate():
    base, a, ab = (_oracle_final(k) for k in ("base", "A", "AB"))
    for name, x in (("A", a), ("A, B", ab)):
        d = float(np.linalg.norm(x - base) / np.linalg.norm(base))
        print(f"oracle: adapters {name} move the final latent by rel-L2 {d:.3f} (needed: >= 5e-2); max |x| = {np.abs(x).max():.2f}")
        assert np.isfinite(x).all() and d >= 5e-2


def test_merge_then_compile_matches_the_oracle_graph_equals_eager_and_repeats(tf):
    sd, lat, a = _merged_then_compiled(tf)
    np.testing.assert_array_equal(_lat0(), sd.randn_latent((2, 4, 16, 16), SEED).numpy())
    _gate(a, _oracle_final("A"), what="adapter A merged, then compiled")
    np.testing.assert_array_equal(a, _final(sd, lat, eager=True))          # graph == eager
    np.testing.assert_array_equal(a, _final(sd, lat))                      # two runs
    with pytest.raises(ValueError, match="'A' is active"):
        sd.unload_lora("A")
    sd.unload_lora("B")
    with pytest.raises(ValueError, match="unknown adapter 'B'"):
        sd.set_adapters(["A", "B"])
    np.testing.assert_array_equal(a, _final(sd, lat))                      # (the refused call changed nothing)


def test_compile_then_set_adapters_recaptures_and_two_adapters_meet_the_oracle_and_the_float64_merge(tf):
    from tinyfusers_amd.variants.samplers import UnsupportedSamplerConfig
    _, _, a = _merged_then_compiled(tf)
    paths, A, B = _adapters()
    W = _tiny()[0]
    sd, lat, _ = _model(tf)
    plain = _final(sd, lat)
    _gate(plain, _oracle_final("base"), what="no adapter")
    old = sd._graph
    sd.set_adapters(["A"])
    assert sd._graph is not old and sd._graph                             # a new, live graph
    for call in (lambda: sd.run(G), lambda: sd.step_sampler(0, G)):
        with pytest.raises(UnsupportedSamplerConfig, match="start"):
            call()
    np.testing.assert_array_equal(_final(sd, lat), a)                      # bit-equal to the model compiled after the merge
    old = sd._graph
    sd.set_adapters(["A"])                                                 # nothing changed: no merge, no capture
    assert sd._graph is old
    sd.run(G)                                                              # (and the start's state is still there: an empty rest of the schedule)
    sd.set_adapters(["A", "B"], weights=WEIGHTS_AB)
    assert sd.adapters() == {"A": (0.7, 0.7), "B": (-0.4, -0.4)}
    _gate(_final(sd, lat), _oracle_final("AB"), what="A at 0.7, B at -0.4")
    worst = 0.0
    for k, m in _targets(sd).items():
        w16 = W[paths[k] + ".weight"].astype(np.float64)
        entries = [(R.scale(wt, float(ad[k + ".alpha"]), ad[k + ".lora_down.weight"].shape[0]), ad[k + ".lora_up.weight"].astype(np.float64),
                    ad[k + ".lora_down.weight"].astype(np.float64)) for wt, ad in zip(WEIGHTS_AB, (A, B))]
        ref, mag = R.merge_ref(w16, entries)
        err = np.abs(R.stored(m.weight.numpy()).astype(np.float64) - ref)
        bound = R.merge_bound(ref, mag, (4, 8), "fp16")
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), k
    print(f"merged weights of {len(paths)} modules vs float64: worst err / bound = {worst:.3f} (bound 1)")


def test_a_refused_start_after_a_recapture_does_not_count_as_a_start(tf):
    from tinyfusers_amd.variants.samplers import UnsupportedSamplerConfig
    sd, lat, _ = _model(tf)
    sd.start(seed=SEED)
    sd.set_adapters(["A"])                                                 # re-captured: the start's state is gone
    with pytest.raises(ValueError, match="shape"):
        sd.start(seed=SEED, init_latent=np.zeros((1, 4, 16, 16), np.float32))
    with pytest.raises(UnsupportedSamplerConfig, match="start"):
        sd.run(G)


def test_weights_alone_and_removal_are_exact(tf):
    _, _, a = _merged_then_compiled(tf)
    sd, lat, _ = _model(tf)
    base = {k: m.weight for k, m in _targets(sd).items()}
    plain = _final(sd, lat)
    sd.set_adapters(["A", "B"], weights=WEIGHTS_AB)
    assert all(m.weight is not base[k] for k, m in _targets(sd).items())
    sd.set_adapters(["A", "B"], weights=[1.0, 0.0])                        # the weights alone, no reload
    np.testing.assert_array_equal(_final(sd, lat), a)
    sd.set_adapters([])
    assert sd.adapters() == {}
    assert all(m.weight is base[k] for k, m in _targets(sd).items())       # the original handle objects
    np.testing.assert_array_equal(_final(sd, lat), plain)                  # == a model that never saw an adapter
    # update_state in between: the installed weight is the new base
    from tinyfusers_amd.storage.state import update_state
    k = "lora_unet_mid_block_attentions_0_proj_in"
    p = _adapters()[0][k]
    sd.set_adapters(["A"])
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(sd.model.diffusion_model, {p + ".weight": 2 * _tiny()[0][p + ".weight"]}, "")
    new_base = _targets(sd)[k].weight
    sd.set_adapters([])
    assert _targets(sd)[k].weight is new_base and all(m.weight is base[kk] for kk, m in _targets(sd).items() if kk != k)


def test_adapter_in_the_bf16_step(tf):
    """One DPM++2M run in the bfloat16 step, 10 steps from noise, at the bf16 gates the sampler tests use (3e-2); the oracle reads the bf16 values
    the device holds, the adapter's included (an fp16 adapter file is rounded to bf16 when it is loaded)."""
    from tinyfusers_amd import config
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import TINY
    W, _, ctx, unc = _tiny()[:4]
    paths, A, _ = _adapters()
    sch = S.DPMSolverPP2M().schedule(10)
    config.set_dtype("bf16")
    try:
        sd = StableDiffusion(TINY); update_state(sd.model.diffusion_model, W, "")
        sd.load_lora(A, "A")
        lat = sd.latent_from_numpy(np.zeros((2, 4, 16, 16), np.float32))
        sd.compile(tf.DeviceArray.from_numpy(unc), tf.DeviceArray.from_numpy(ctx), lat, sampler=sch)
        sd.set_adapters(["A"])
        a, b = _final(sd, lat), _final(sd, lat, eager=True)
    finally:
        config.set_dtype("fp16")
    np.testing.assert_array_equal(a, b)
    W16 = {k: R.to16(v, "bf16").astype(np.float32) for k, v in W.items()}
    _gate(a, _trajectory(R.merged_state(W16, paths, [(1.0, A)], "bf16"), _lat0(), sch), rel_l2=3e-2, max_rel=3e-2, what="bf16, adapter A")


def test_adapter_on_the_unet_of_a_controlled_model(tf):
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.controlnet import ControlNet
    from tinyfusers_amd.vision.unet import TINY
    W, Wc, ctx, unc, img = _tiny()[:5]
    paths, A, _ = _adapters()
    sd = StableDiffusion(TINY); update_state(sd.model.diffusion_model, W, "")
    net = ControlNet(TINY); update_state(net, Wc, "")
    sd.attach_control(net)
    lat = sd.latent_from_numpy(np.zeros((2, 4, 16, 16), np.float32))
    sd.compile(tf.DeviceArray.from_numpy(unc), tf.DeviceArray.from_numpy(ctx), lat, sampler=_sched(), control=True)
    sd.load_lora(A, "A")
    sd.set_adapters(["A"])
    got = _final(sd, lat, control_image=img)
    _gate(got, _trajectory(R.merged_state(W, paths, [(1.0, A)]), _lat0(), _sched(), Wc, img), what="controlled, adapter A on the UNet")
    np.testing.assert_array_equal(got, _final(sd, lat, eager=True, control_image=img))


# ---- 3. text encoder -----------------------------------------------------------------------------------------------------------------------------
def test_text_encoder_adapter_against_the_oracle_and_its_own_weight(tf):
    import oracle
    from test_gpu_model import unet_gate
    from tinyfusers_amd.storage import lora as L
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_state_dict
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import SD15
    pre = "cond_stage_model.transformer.text_model."
    W = synth_state_dict(oracle.clip_param_shapes(), 7)
    sd = StableDiffusion(SD15)
    text = sd.cond_stage_model.transformer.text_model
    update_state(text, W, pre.rstrip("."))
    paths = {k: pre + p for k, p in L.text_target_paths(text).items()}
    assert len(paths) == 72
    ad = R.make_adapter({k: W[p + ".weight"] for k, p in paths.items()}, 4, 13)
    # one UNet module gets a weight and an adapter too: text_encoder_weights=0 must leave the text encoder alone while the UNet's handle is swapped
    uk = "lora_unet_mid_block_attentions_0_proj_in"
    um = L.lora_targets(sd)[uk]
    um.weight = tf.asarray((np.random.default_rng(1).standard_normal((1280, 1280, 1, 1)) / 36).astype(np.float16))
    both = dict(ad, **R.make_adapter({uk: um.weight.numpy()}, 4, 14))
    ids = np.asarray(json.load(open(os.path.join(HERE, "golden", "clip_tokens.json")))["ids"][:2])
    assert ids.shape == (2, 77)
    te_base = {k: m.weight for k, m in L.lora_targets(sd).items() if k.startswith("lora_te_")}
    u_base = um.weight
    plain = text(ids).numpy()
    sd.load_lora(both, "te")
    sd.set_adapters(["te"], weights=1.0, text_encoder_weights=0)
    assert um.weight is not u_base and all(L.lora_targets(sd)[k].weight is w for k, w in te_base.items())
    assert sd.adapters() == {"te": (1.0, 0.0)}
    np.testing.assert_array_equal(text(ids).numpy(), plain)
    sd.set_adapters(["te"])
    assert all(L.lora_targets(sd)[k].weight is not w for k, w in te_base.items())
    got = text(ids).numpy()
    Wf = {k: v.astype(np.float32) for k, v in W.items()}
    ref_base = oracle.clip_text_transformer(ids, Wf).numpy()
    ref = oracle.clip_text_transformer(ids, R.merged_state(W, paths, [(1.0, ad)])).numpy()
    moved = float(np.linalg.norm(ref - ref_base) / np.linalg.norm(ref_base))
    print(f"text encoder: the adapter moves the oracle's output by rel-L2 {moved:.3f} (needed: >= 10 x 5e-3)")
    assert moved >= 10 * 5e-3
    print("CLIP text transformer with the adapter vs oracle: rel-L2 %.3e worst %.3e" % unet_gate(got, ref))
    sd.set_adapters([])
    assert um.weight is u_base and all(L.lora_targets(sd)[k].weight is w for k, w in te_base.items())
    np.testing.assert_array_equal(text(ids).numpy(), plain)


# ---- 4. SD-1.5 shapes, once ------------------------------------------------------------------------------------------------------------------------
def test_sd15_rank16_file_over_all_attention_and_text_targets_plus_locon_convs(tf, tmp_path):
    import oracle
    from tinyfusers_amd.storage import lora as L
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.storage.unpicker import save_safetensors
    from tinyfusers_amd.variants.samplers import DPMSolverPP2M
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import SD15
    pre = "cond_stage_model.transformer.text_model."
    W = synth_state_dict(oracle.unet_param_shapes(oracle.SD15), 0, prefix="model.diffusion_model.")
    W.update(synth_state_dict(oracle.clip_param_shapes(), 7))
    sd = StableDiffusion(SD15)
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(sd.model.diffusion_model, W, "model.diffusion_model.")
        update_state(sd.cond_stage_model.transformer.text_model, W, pre.rstrip("."))
    paths = L.lora_target_paths(sd)
    attn = ("_proj_in", "_proj_out", "_to_q", "_to_k", "_to_v", "_to_out_0", "_ff_net_0_proj", "_ff_net_2")
    convs = ["lora_unet_down_blocks_0_resnets_0_conv1", "lora_unet_down_blocks_1_resnets_0_conv_shortcut", "lora_unet_down_blocks_2_downsamplers_0_conv",
             "lora_unet_mid_block_resnets_0_conv2"]          # one LoCon conv per level; the last a 1280-channel 3x3
    names = [k for k in paths if k.startswith("lora_te_") or ("_attentions_" in k and k.endswith(attn))]
    assert len(names) == 264
    names += convs
    path = str(tmp_path / "rank16.safetensors")
    ad = R.make_adapter({k: W[paths[k] + ".weight"] for k in names}, 16, 15, exact=False)
    save_safetensors(path, ad)
    assert sd.load_lora(path) == "rank16"
    base = {k: L.lora_targets(sd)[k].weight for k in names}
    hip_sync = lambda: tf.hip.tf_stream_sync(tf._sh())
    hip_sync()
    t0 = time.perf_counter()
    sd.set_adapters(["rank16"])
    hip_sync()
    print(f"SD-1.5: set_adapters merged {len(names)} modules (rank 16) in {1e3 * (time.perf_counter() - t0):.1f} ms (uncompiled model; no target)")
    sample = ["lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_ff_net_0_proj", "lora_unet_mid_block_resnets_0_conv2",
              "lora_unet_down_blocks_0_resnets_0_conv1", "lora_unet_down_blocks_1_resnets_0_conv_shortcut", "lora_unet_up_blocks_1_attentions_2_transformer_blocks_0_attn2_to_k",
              "lora_unet_mid_block_attentions_0_proj_out", "lora_te_text_model_encoder_layers_5_mlp_fc1", "lora_unet_up_blocks_3_attentions_0_transformer_blocks_0_attn1_to_out_0"]
    assert L.weight_shape(L.lora_targets(sd)[sample[0]]) == (2560, 320) and L.weight_shape(L.lora_targets(sd)[sample[1]]) == (1280, 1280, 3, 3)
    for k in sample:
        m = L.lora_targets(sd)[k]
        s = R.scale(1.0, float(ad[k + ".alpha"]), 16)
        ref, mag = R.merge_ref(W[paths[k] + ".weight"].astype(np.float64), [(s, ad[k + ".lora_up.weight"].astype(np.float64), ad[k + ".lora_down.weight"].astype(np.float64))])
        err, bound = np.abs(R.stored(m.weight.numpy()).astype(np.float64) - ref), R.merge_bound(ref, mag, (16,), "fp16")
        print(f"SD-1.5 {k} {ref.shape}: worst err / bound = {float(np.max(err / bound)):.3f} (bound 1)")
        assert np.all(err <= bound), k
    ctx = tf.DeviceArray.from_numpy(synth_normal(1234, "sd.context", (1, 77, 768)))
    unc = tf.DeviceArray.from_numpy(synth_normal(1234, "sd.uncond", (1, 77, 768)))
    lat = sd.latent_from_numpy(np.zeros((1, 4, 64, 64), np.float32))
    sd.compile(unc, ctx, lat, sampler=DPMSolverPP2M().schedule(2))
    out = _final(sd, lat)
    assert np.isfinite(out).all()
    sd.set_adapters([])
    assert all(L.lora_targets(sd)[k].weight is base[k] for k in names)
