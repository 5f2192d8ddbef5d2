#!/usr/bin/env python3
"""Samplers on one box, one process (report, not a gate): the SD-1.5 compiled step with DPM-Solver++(2M) (the fused sampler update,
tf_cfg_sampler_step_f32) against the DDIM step (tf_cfg_ddim_step_f32), 100 graph replays each, alternated over several rounds; and the
config-3 end-to-end img/s (CLIP x2 -> steps -> VAE decode, batch 1) at 20 DPM++2M steps against 50 DDIM steps.

    python tools/sampler_bench.py [--replays 100] [--rounds 5] [--images 3] [--dpm-steps 20] [--inpaint] [--concat inpaint|edit] [--control] [--lora] [--lcm] [--ip-adapter] [--freeu] [--pag]
    python tools/sampler_bench.py --motion [--replays 80]      # a run of its own: the AnimateDiff video step against the image step at batch 16
--inpaint adds the masked DPM++2M step (tf_cfg_sampler_step_masked_f32, a model compiled with inpaint=True on the same shape, half the
latent repainted) to the alternation, and the VAE encoder's time for a 512^2 image (StableDiffusion.encode_image).
--concat adds the DPM++2M step of a concat-conditioned UNet (SD15_INPAINT: 9 input channels, two CFG groups; SD15_EDIT: 8 input channels, three
groups, so UNet batch 3 instead of 2) to the alternation -- the same weights but for conv_in -- and the time of start(cond_image=...) for a 512^2
image (upload, VAE encoder, conditioning buffer).
--control adds the controlled DPM++2M step (compile(..., control=True): the same UNet weights plus a synthetic SD-1.5 ControlNet) to the
alternation, the time of start(control_image=...) for a 512^2 hint (upload, x / 255, the hint stem), and k_control_add's achieved GB/s on the
13 skip shapes of the step next to tf_add_16 on the same byte count.
--ip-adapter adds, interleaved with the plain DPM++2M step in the same rounds: the adapted step (compile(..., ip_adapter=True): the same UNet weights
plus a synthetic ip-adapter_sd15, every cross-attention the fused tf_sdpa_dual_16 launch) and an adapted step that composes what the fused launch
replaces -- two tf_sdpa_16 launches plus tf_add_16 per cross-attention, built only inside this tool (the image term at scale 1) -- and the time of
start(ip_image_embeds=) (tokens + the hoisted K_ip | V_ip GEMM) and start(ip_image=) through the CLIP ViT-H image tower (clip_vision_bench: the tower
captured and eager at batch 1 and 2, its weight-streaming floor, the exact-GELU passes' share, the GEMM shapes it had to autotune); written to
profiles/sampler_bench_ip_adapter.json as well.
--lora adds, for a synthetic adapter of rank 16 and of rank 128 over the 192 UNet attention / FF / proj targets plus the 72 text-encoder targets:
lora_merge_ms (one set_adapters on an uncompiled model, every launch, wall clock incl. the final sync), lora_merge_gb_s (base read + dst write
over the launches' device time) next to add_16_gb_s, lora_recapture_ms (set_adapters on a compiled model minus the merge), lora_step_over_plain
(the adapted DPM++2M step against the plain one) and host_merge_ms (the same merge in numpy float32 plus the upload).  No target is set for any.
--lcm adds the guidance-free step (compile(..., cfg=False): one guidance group, UNet batch 1 instead of 2) to the alternation: the DPM++2M step with
cfg=False (dpmpp2m_nocfg_step_ms) next to the cfg=True one of the same rounds, the LCM step in both modes (lcm_step_ms, lcm_nocfg_step_ms), the
ratios with the rounds' own spread next to them, and the end-to-end img/s of 4 LCM steps with cfg=False (e2e_lcm4_nocfg: one CLIP pass, the
sampler, the VAE decode) against the DPM++2M run.
--freeu adds the FreeU step (compile(..., freeu=True): the same UNet weights) to the alternation at the values usually quoted for SD-1.5 (0.9, 0.2,
1.5, 1.6) and at all ones, next to the plain step of the same rounds with the rounds' spread; the library entries one eager step of each calls
(step_entries, and which entries differ); and microseconds per launch of tf_freeu_skip_16 on the step's six skip shapes and of
tf_freeu_backbone_16 on its two backbone shapes; written to profiles/sampler_bench_freeu.json as well.
--pag adds the perturbed-attention-guidance step (compile(..., pag=True): the same UNet weights, three guidance groups [uncond ; perturbed ; cond], so
UNet batch 3 instead of 2) to the alternation at scale 3 on the middle block and on every transformer, next to the plain CFG step of the same rounds
with the rounds' spread, and the library entries one eager step of each calls (the launch count per step); written to
profiles/sampler_bench_pag.json as well.
--sd2 is a run of its own (nothing above is timed): the SD21 step (heads of 64, 1024-wide context) against the SD15 step at 64x64 in the same
rounds, the SD21 step at 96x96 for 1 and 4 images, the v-prediction step with and without CFG rescale at both sizes and batches, tf_sampler_tail_*
alone with bit 2 against without, and the OpenCLIP text tower for two prompts; written to profiles/sampler_bench_sd2.json.
Prints one JSON line."""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def control_add_bench(T, hip, model, timed, args):
    """k_control_add (one launch over the 13 skip shapes of the SD-1.5 step at CFG batch 2) against tf_add_16 (one launch over one tensor of the
    same byte count): achieved GB/s of each, two reads and one write of every element, medians of --rounds rounds of --replays launches."""
    from tinyfusers_amd.native import ControlEntry
    shapes = [(2, c, s, s) for c, s in zip([320] * 4 + [640] * 3 + [1280] * 6, [64] * 3 + [32] * 3 + [16] * 3 + [8] * 4)]
    with T.use_stream(model._stream):
        skips, ress, dsts = ([T.DeviceArray.zeros(sh, np.float16, "nhwc") for sh in shapes] for _ in range(3))
        total = sum(k.size for k in skips)
        a, b, y = (T.DeviceArray.zeros((total,), np.float16, "row") for _ in range(3))
        scales = T.DeviceArray.from_numpy(np.full((16,), 0.75, np.float32), np.float32, "row")
    table = (ControlEntry * len(shapes))()
    for e, d, k, r in zip(table, dsts, skips, ress):
        e.dst, e.skip, e.residual, e.n = d.ptr, k.ptr, r.ptr, k.size
    tp = ctypes.cast(table, ctypes.c_void_p)

    def ctl(n):
        for _ in range(n):
            hip.tf_control_add_16(0, tp, len(shapes), scales.ptr, model._stream.handle)

    def add(n):
        for _ in range(n):
            hip.tf_add_16(0, y.ptr, a.ptr, b.ptr, total, model._stream.handle)

    ctl(10); add(10)
    ms = {"ctl": [], "add": []}
    for _ in range(args.rounds):
        ms["ctl"].append(timed(model, ctl, args.replays))
        ms["add"].append(timed(model, add, args.replays))
    nbytes = 3 * 2 * total
    c, d = float(np.median(ms["ctl"])), float(np.median(ms["add"]))
    return {"control_add_bytes": nbytes, "control_add_us": round(1e3 * c, 2), "control_add_gb_s": round(nbytes / c / 1e6, 1),
            "add_16_us": round(1e3 * d, 2), "add_16_gb_s": round(nbytes / d / 1e6, 1)}


def step_entries(T, model):
    """{entry: calls} of one eager step of a compiled model: every library entry it calls that is not a copy, an allocation, a host-side query or
    stream / event / graph plumbing.  (An entry is one kernel launch except where it says otherwise: a split-K GEMM adds its reduce, a GroupNorm that computes its
    own statistics is a statistics and an apply kernel.)"""
    from tinyfusers_amd.native import declared_symbols, hip as H
    counts, saved = {}, {}
    for name in declared_symbols():
        fn = getattr(H, name)
        saved[name] = fn

        def rec(*a, _fn=fn, _name=name):
            counts[_name] = counts.get(_name, 0) + 1
            return _fn(*a)
        setattr(H, name, rec)
    try:
        with T.use_stream(model._stream):
            model._eager_step(model._params)
        model.synchronize()
    finally:
        for name, fn in saved.items():
            setattr(H, name, fn)
    plumbing = ("tf_mem", "tf_malloc", "tf_stream", "tf_event", "tf_graph", "tf_last_error", "tf_pool", "tf_prof", "tf_gemm_tune", "tf_gemm_autotune")
    queries = ("_workspace", "_partial_bytes", "_admits")                 # host-side questions: no launch
    return {k: v for k, v in counts.items() if k != "tf_free" and not k.startswith(plumbing) and not k.endswith(queries)}


def freeu_kernel_bench(T, hip, model, timed, args):
    """tf_freeu_skip_16 on the six SD-1.5 skip shapes of a CFG step (one launch, 4.3 MB in and out) and tf_freeu_backbone_16 in place on the two
    backbone shapes: microseconds per launch, medians of --rounds rounds of --replays launches on the model's stream."""
    import ctypes
    from tinyfusers_amd.native import FreeuEntry
    shapes = [(2, 8, 8, 1280)] * 3 + [(2, 16, 16, 1280)] * 2 + [(2, 16, 16, 640)]
    with T.use_stream(model._stream):
        src = [T.DeviceArray.from_numpy(np.random.default_rng(i).standard_normal((b, c, h, w)).astype(np.float32), np.float16, "nhwc") for i, (b, h, w, c) in enumerate(shapes)]
        dst = [T.DeviceArray.empty(a.shape, a.dtype, "nhwc") for a in src]
        scales = T.DeviceArray.from_numpy(np.asarray([0.9, 0.2, 1.5, 1.6], np.float32), np.float32, "row")
    table = (FreeuEntry * 6)()
    for i, (e, d, a, (b, h, w, c)) in enumerate(zip(table, dst, src, shapes)):
        e.dst, e.src, e.B, e.H, e.W, e.C, e.scale_index = d.ptr, a.ptr, b, h, w, c, i // 3

    def skip(n):
        for _ in range(n):
            hip.tf_freeu_skip_16(0, ctypes.cast(table, ctypes.c_void_p), 6, scales.ptr, model._stream.handle)

    def backbone(a, idx):
        def run(n):
            for _ in range(n):
                hip.tf_freeu_backbone_16(0, a.ptr, a.ptr, a.shape[0] * a.shape[2] * a.shape[3], a.shape[1], scales.ptr, idx, model._stream.handle)
        return run
    out = {}
    for key, fn in (("freeu_skip_6_us", skip), ("freeu_backbone_8x8_us", backbone(dst[0], 2)), ("freeu_backbone_16x16_us", backbone(dst[3], 3))):
        fn(20)
        out[key] = round(1e3 * float(np.median([timed(model, fn, args.replays) for _ in range(args.rounds)])), 3)
    return out


def synthetic_lora(targets, rank, seed):
    """A kohya-format adapter over ``targets`` ({kohya name: module}): up, down ~ N(0, 1) in fp16, alpha such that alpha / rank = 0.05 / sqrt(Kd rank)
    (about 5 % of a synthetic weight's norm: the sampler stays finite)."""
    from tinyfusers_amd.storage.lora import weight_shape
    rng = np.random.default_rng(seed)
    out = {}
    for k, m in targets.items():
        shape = weight_shape(m)
        kd = int(np.prod(shape[1:]))
        out[k + ".lora_up.weight"] = rng.standard_normal((shape[0], rank) + ((1, 1) if len(shape) == 4 else ()), dtype=np.float32).astype(np.float16)
        out[k + ".lora_down.weight"] = rng.standard_normal((rank,) + shape[1:], dtype=np.float32).astype(np.float16)
        out[k + ".alpha"] = np.asarray(0.05 * rank / np.sqrt(kd * rank), np.float32)
    return out


def lora_bench(T, hip, timed, args, state, donor, unc, ctx, noise, sched, plain_m, plain_replays, lat0):
    """The figures of --lora (see the module docstring) for rank 16 and rank 128.  donor: the model whose text encoder holds weights."""
    from tinyfusers_amd.storage import lora as L
    from tinyfusers_amd.storage.state import update_state
    from tinyfusers_amd.variants.sd import StableDiffusion
    attn = ("_proj_in", "_proj_out", "_to_q", "_to_k", "_to_v", "_to_out_0", "_ff_net_0_proj", "_ff_net_2")

    def model():
        m = StableDiffusion()
        update_state(m.model.diffusion_model, state, "")
        m.cond_stage_model = donor.cond_stage_model
        return m
    eager_m, graph_m = model(), model()
    targets = {k: t for k, t in L.lora_targets(eager_m).items() if k.startswith("lora_te_") or ("_attentions_" in k and k.endswith(attn))}
    assert len(targets) == 264, len(targets)
    elems = sum(t.weight.size for t in targets.values())
    lat = graph_m.latent_from_numpy(noise)
    graph_m.compile(unc, ctx, lat, sampler=sched)

    def adapted_replays(n):
        k = len(sched.timesteps)
        for s in range(n):
            i = s % k
            if i == 0:
                hip.tf_memcpy_async(lat.ptr, lat0.ptr, lat.nbytes, 3, graph_m._stream.handle)
            graph_m.step_sampler(i, 7.5)

    n_add = min(elems, 1 << 26)
    a, b, y = (T.DeviceArray.zeros((n_add,), np.float16, "row") for _ in range(3))
    hip.tf_stream_sync(None)

    def add(n):
        for _ in range(n):
            hip.tf_add_16(0, y.ptr, a.ptr, b.ptr, n_add, plain_m._stream.handle)
    add(10)
    add_ms = float(np.median([timed(plain_m, add, args.replays) for _ in range(args.rounds)]))
    out = {"lora_targets": len(targets), "lora_weight_elems": elems, "add_16_gb_s": round(3 * 2 * n_add / add_ms / 1e6, 1)}
    ev0, ev1, ms, host = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_float(), {}
    hip.tf_event_create(ctypes.byref(ev0)); hip.tf_event_create(ctypes.byref(ev1))
    for rank in (16, 128):
        ad = synthetic_lora(targets, rank, rank)
        name = f"r{rank}"
        eager_m.load_lora(ad, name); graph_m.load_lora(ad, name)
        wall, dev = [], []
        for r in range(args.rounds + 1):
            hip.tf_stream_sync(None)
            t0 = time.perf_counter()
            hip.tf_event_record(ev0, None)
            eager_m.set_adapters([name])
            hip.tf_event_record(ev1, None)
            hip.tf_stream_sync(None)
            wall.append(1e3 * (time.perf_counter() - t0))
            hip.tf_event_elapsed_ms(ctypes.byref(ms), ev0, ev1)
            dev.append(ms.value)
            eager_m.set_adapters([])
        merge_ms, dev_ms = float(np.median(wall[1:])), float(np.median(dev[1:]))
        recap = []
        for r in range(3):
            t0 = time.perf_counter()
            graph_m.set_adapters([name])
            graph_m.synchronize()
            recap.append(1e3 * (time.perf_counter() - t0))
            if r < 2:
                graph_m.set_adapters([])
        graph_m.start(seed=1234)
        adapted_replays(20); plain_replays(20)
        step = {"plain": [], "lora": []}
        for _ in range(args.rounds):
            step["plain"].append(timed(plain_m, plain_replays, args.replays))
            step["lora"].append(timed(graph_m, adapted_replays, args.replays))
        assert np.isfinite(lat.numpy()).all()
        graph_m.set_adapters([])
        # the same merge on the host: numpy float32, one rounding to fp16, one upload per module
        if not host:
            host.update({k: t.weight.numpy().reshape(t.weight.shape[0], -1) for k, t in targets.items()})      # (Linear and 1x1 conv weights: (N, Kd) as stored)
        keep = []
        t0 = time.perf_counter()
        for k in targets:
            w = host[k]
            up = ad[k + ".lora_up.weight"].reshape(w.shape[0], rank).astype(np.float32)
            dn = ad[k + ".lora_down.weight"].reshape(rank, -1).astype(np.float32)
            s = np.float32(float(ad[k + ".alpha"]) / rank)
            keep.append(T.DeviceArray.from_numpy((w + s * (up @ dn)).astype(np.float16), np.float16, "row"))
        hip.tf_stream_sync(None)
        host_ms = 1e3 * (time.perf_counter() - t0)
        del keep
        eager_m.unload_lora(name); graph_m.unload_lora(name)
        p, l = float(np.median(step["plain"])), float(np.median(step["lora"]))
        out[f"rank{rank}"] = {"lora_merge_ms": round(merge_ms, 3), "lora_merge_device_ms": round(dev_ms, 3), "lora_merge_gb_s": round(2 * 2 * elems / dev_ms / 1e6, 1),
                              "lora_recapture_ms": round(float(np.median(recap)) - merge_ms, 2), "lora_step_ms": round(l, 4), "plain_step_ms": round(p, 4),
                              "lora_step_over_plain": round(l / p, 4), "host_merge_ms": round(host_ms, 1)}
    hip.tf_event_destroy(ev0); hip.tf_event_destroy(ev1)
    return out


def clip_vision_bench(T, hip, model, ip_emb, args):
    """--ip-adapter: the CLIP ViT-H image tower (vae/clip_vision.py, synthetic weights) in front of the adapted model.  Interleaved rounds, medians and
    the spread between rounds: the tower at batch 1 and 2, captured (graph replay) and eager, wall time from the call to the drained stream (the
    150 KB image upload included); start(ip_image=) against start(ip_image_embeds=) on the batch-1 model; the 32 exact-GELU passes of one tower on
    their own (stream events); the tower against its weight-streaming floor (every fp16 weight once at the 8 TB/s HBM peak); the GEMM shapes of
    the tower that had no row in the tuning table (autotuned on the first eager call)."""
    import tempfile
    from tinyfusers_amd.native import lib
    from tinyfusers_amd.vae.clip_vision import VIT_H, ClipVision, param_shapes, synthetic_state
    with contextlib.redirect_stdout(io.StringIO()):
        tower = ClipVision.load(synthetic_state(VIT_H, 11))
    weight_bytes = 2 * sum(int(np.prod(s)) for s in param_shapes(VIT_H).values())
    rng = np.random.default_rng(5)
    imgs = {b: rng.integers(0, 256, (b, 224, 224, 3), dtype=np.uint8) for b in (1, 2)}
    def table_keys():
        """The shape keys that have a row in the library's tuning table right now (tf_gemm_tune_count / tf_gemm_tune_entry: its own host-side view)."""
        n, key, cfg_ = ctypes.c_int(0), (ctypes.c_int * 10)(), (ctypes.c_int * 5)()
        hip.tf_gemm_tune_count(ctypes.byref(n))
        keys = set()
        for i in range(n.value):
            hip.tf_gemm_tune_entry(i, key, cfg_)
            keys.add(tuple(key))
        return keys
    before = table_keys()                                                  # (the shipped table plus what this process has tuned so far)
    with tempfile.TemporaryDirectory() as d:                               # which GEMM shapes the first eager calls had to tune
        lib.tf_gemm_tune_trace(1)
        for b in (1, 2):
            tower(imgs[b])                                                 # eager, then captured
        lib.tf_gemm_tune_trace_dump(os.path.join(d, "keys.txt").encode())
        lib.tf_gemm_tune_trace(0)
        rows = sorted({tuple(int(v) for v in line.split())[:10] for line in open(os.path.join(d, "keys.txt"))})
    # (the trace's own "had a row" flag is that of a key's LAST lookup, behind the tuning: the table as it stood before the first call decides)
    untuned = [list(r[:3]) for r in rows if r not in before]

    def wall(fn):
        t0 = time.perf_counter()
        out = fn()
        tower._stream.synchronize()
        del out
        return 1e3 * (time.perf_counter() - t0)
    model.attach_clip_vision(tower)
    t = {k: [] for k in ("captured_b1", "eager_b1", "captured_b2", "eager_b2", "start_ip_image", "start_ip_image_embeds")}
    for r in range(args.rounds + 1):
        for b in (1, 2):
            t[f"captured_b{b}"].append(wall(lambda: tower(imgs[b])))
            t[f"eager_b{b}"].append(wall(lambda: tower.eager(imgs[b])))
        for key, kw in (("start_ip_image", dict(ip_image=imgs[1])), ("start_ip_image_embeds", dict(ip_image_embeds=ip_emb))):
            t0 = time.perf_counter()
            model.start(seed=1234, **kw)
            model.synchronize()
            t[key].append(1e3 * (time.perf_counter() - t0))
    med = {k: float(np.median(v[1:])) for k, v in t.items()}
    spread = {k: round(max(v[1:]) - min(v[1:]), 3) for k, v in t.items()}
    # the GELU pass alone: 32 in-place launches on a (257 B, 5120) buffer, per batch size
    gelu = {}
    ev0, ev1, ms = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_float()
    hip.tf_event_create(ctypes.byref(ev0)); hip.tf_event_create(ctypes.byref(ev1))
    with T.use_stream(tower._stream):
        for b in (1, 2):
            x = T.DeviceArray.from_numpy(rng.standard_normal((257 * b, VIT_H.mlp)).astype(np.float32), np.float16, "row")
            per = []
            for r in range(args.rounds + 1):
                hip.tf_event_record(ev0, tower._stream.handle)
                for _ in range(VIT_H.layers):
                    hip.tf_gelu_erf_16(0, x.ptr, x.ptr, x.size, T._sh())
                hip.tf_event_record(ev1, tower._stream.handle)
                tower._stream.synchronize()
                hip.tf_event_elapsed_ms(ctypes.byref(ms), ev0, ev1)
                per.append(ms.value)
            gelu[b] = float(np.median(per[1:]))
    hip.tf_event_destroy(ev0); hip.tf_event_destroy(ev1)
    # the same from the library's own brackets: family 5 (tf_vit_patchify_u8_16 + the 32 tf_gelu_erf_16) over one instrumented eager tower at batch 1
    fam = {}
    hip.tf_prof_enable(1)
    try:
        tower.eager(imgs[1])
        tower._stream.synchronize()
        fms, fwork, fn = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        hip.tf_prof_read_family(5, ctypes.byref(fms), ctypes.byref(fwork), ctypes.byref(fn))
        fam = {"launches": fn.value, "ms": round(fms.value, 4), "bytes": int(fwork.value)}
    finally:
        hip.tf_prof_enable(0)
    floor_ms = weight_bytes / 8e12 * 1e3
    tower.release_graphs()
    return {"clip_vision": {"config": "ViT-H/14 (synthetic weights)", "weight_bytes": weight_bytes, "weight_floor_ms_at_8TBps": round(floor_ms, 4),
                            "tower_ms": {k: round(med[k], 3) for k in ("captured_b1", "eager_b1", "captured_b2", "eager_b2")},
                            "tower_over_floor": {k: round(med[k] / floor_ms, 2) for k in ("captured_b1", "captured_b2")},
                            "gelu_32_passes_ms": {f"b{b}": round(gelu[b], 4) for b in gelu},
                            "gelu_share_of_captured_tower": {f"b{b}": round(gelu[b] / med[f"captured_b{b}"], 4) for b in gelu},
                            "prof_family_5_patchify_and_gelu_b1": fam,
                            "round_spread_ms": spread, "gemm_shapes_autotuned_MNK": untuned, "gemm_shapes_total": len(rows)},
            "start_ip_image_ms": round(med["start_ip_image"], 3), "start_ip_image_embeds_interleaved_ms": round(med["start_ip_image_embeds"], 3)}


def sd2_bench(args):
    """--sd2: medians of --rounds rounds of --replays graph replays (or launches), every comparison's sides alternating inside the same rounds,
    the spread between the rounds stated.  Synthetic weights."""
    import tinyfusers_amd.storage.tensor as T
    from tinyfusers_amd.native import hip
    from tinyfusers_amd.storage.state import param_shapes, update_state
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.vae import open_clip_text as O
    from tinyfusers_amd.variants.samplers import DPMSolverPP2M
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import SD15, SD21

    T.ensure_init(0)
    sched = DPMSolverPP2M().schedule(args.dpm_steps)
    states = {}

    def model(cfg, side, images, **modes):
        if cfg not in states:
            states[cfg] = synth_state_dict(param_shapes(StableDiffusion(cfg).model.diffusion_model), 0)
        m = StableDiffusion(cfg)
        update_state(m.model.diffusion_model, states[cfg], "")
        ctx = T.DeviceArray.from_numpy(synth_normal(5, "c", (images, 77, cfg.context_dim)).astype(np.float16))
        unc = T.DeviceArray.from_numpy(synth_normal(5, "u", (images, 77, cfg.context_dim)).astype(np.float16))
        lat = m.latent_from_numpy(np.zeros((images, 4, side, side), np.float32))
        m.compile(unc, ctx, lat, sampler=sched, **modes)
        m.start(seed=1234)
        return m, lat

    def timed(stream, fn, n):
        ev0, ev1, ms = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_float()
        hip.tf_event_create(ctypes.byref(ev0)); hip.tf_event_create(ctypes.byref(ev1))
        stream.synchronize()
        hip.tf_event_record(ev0, stream.handle)
        fn(n)
        hip.tf_event_record(ev1, stream.handle)
        stream.synchronize()
        hip.tf_event_elapsed_ms(ctypes.byref(ms), ev0, ev1)
        hip.tf_event_destroy(ev0); hip.tf_event_destroy(ev1)
        return ms.value / n

    def replays(m, lat):
        m.synchronize()
        lat0 = T.DeviceArray.from_numpy(lat.numpy(), np.float32, "row")      # the start latent, put back at the head of every pass over the schedule

        def run(n):
            for s in range(n):
                i = s % len(sched.timesteps)
                if i == 0:
                    hip.tf_memcpy_async(lat.ptr, lat0.ptr, lat.nbytes, 3, m._stream.handle)
                m.step_sampler(i, 7.5)
        return run

    def alternate(arms):
        """arms: {key: (stream, fn(n))} -> {key: (median ms, spread ms)} of --rounds rounds, the arms alternating inside every round."""
        for st, fn in arms.values():
            timed(st, fn, 20)
        ms = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, (st, fn) in arms.items():
                ms[k].append(timed(st, fn, args.replays))
        return {k: (round(float(np.median(v)), 4), round(max(v) - min(v), 4)) for k, v in ms.items()}

    out = {"protocol": f"median of {args.rounds} rounds of {args.replays} replays, (median ms, max - min over the rounds); DPM++2M, CFG pair, synthetic weights"}
    # 1. SD21 against SD15 at 64 x 64, one image (UNet batch 2); the v step and the rescaled v step in the same rounds
    for side, images in ((64, 1), (96, 1), (96, 4)):
        arms = {}
        for key, cfg, modes in (("sd15", SD15, {}), ("sd21", SD21, {}), ("sd21_v", SD21, dict(prediction="v")), ("sd21_v_rescale", SD21, dict(prediction="v", cfg_rescale=True))):
            if key == "sd15" and side != 64:
                continue
            m, lat = model(cfg, side, images, **modes)
            arms[key] = (m._stream, replays(m, lat), m, lat)
        res = alternate({k: v[:2] for k, v in arms.items()})
        for k, (_, _, m, lat) in arms.items():
            m.synchronize()
            assert np.isfinite(lat.numpy()).all(), k
        out[f"step_ms_{side}x{side}_images{images}"] = res
        if side == 64:
            ent = {k: step_entries(T, v[2]) for k, v in arms.items()}
            out["step_entries"] = {k: sum(v.values()) for k, v in ent.items()}
        del arms
    # 2. the tail alone: tf_sampler_tail_f32 with bit 2 against without (flags 1: v), the CFG pair
    st = T.Stream()
    with T.use_stream(st):
        for side in (64, 96):
            for images in (1, 4):
                lat, hist = (T.DeviceArray.zeros((images, 4, side, side), np.float32, "row") for _ in range(2))
                eps = T.DeviceArray.from_numpy(synth_normal(3, "eps", (2 * images, 4, side, side)), np.float16, "nhwc")
                tab = T.DeviceArray.from_numpy(np.asarray(sched.coeffs, np.float32), np.float32, "row")
                sp, phi = T.DeviceArray.zeros((8,), np.float32, "row"), T.DeviceArray.from_numpy(np.float32([0.7, 0, 0, 0]), np.float32, "row")
                hip.tf_set_sampler_params(sp.ptr, 500.0, 0.3, 0.4, 7.5, 3, 1, 2, 0, None, None, 0, T._sh())

                def launches(flags):
                    def run(n):
                        for _ in range(n):
                            hip.tf_sampler_tail_f32(lat.ptr, eps.ptr, hist.ptr, sp.ptr, tab.ptr, len(sched.timesteps), None, None, None, phi.ptr if flags & 4 else None,
                                                    images, 4, side, side, 2, flags, T._sh())
                    return run
                res = alternate({"v": (st, launches(1)), "v_rescale": (st, launches(5))})
                out[f"tail_us_{side}x{side}_images{images}"] = {k: (round(1e3 * a, 2), round(1e3 * b, 2)) for k, (a, b) in res.items()}
    # 3. the OpenCLIP tower for two prompts (eager launches, as example/sd1.py runs it)
    tower = O.OpenClipText.load(O.synthetic_state(O.VIT_H_TEXT, 0))
    ids = np.zeros((2, 77), np.int64); ids[:, 0] = 49406; ids[0, 1:10] = np.random.default_rng(0).integers(1, 49406, 9); ids[0, 10] = 49407; ids[1, 1] = 49407
    keep = []

    def towers(n):
        for _ in range(n):
            keep.append(tower(ids)); del keep[:-2]
    with T.use_stream(st):
        towers(3)
        a, b = alternate({"open_clip_two_prompts": (st, towers)})["open_clip_two_prompts"]
    out["open_clip_text_two_prompts_ms"] = (a, b)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sampler_bench_sd2.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def sdxl_bench(args):
    """--sdxl: the SDXL base step (synthetic weights) -- 128 x 128 latent, CFG pair, --dpm-steps DPM++2M steps; medians of --rounds rounds of --replays
    replays with the spread between the rounds.  start() with the schedule's rows built in one pass (time_embedding_table: the batched ResBlock
    projection once at M = S R) against S passes at M = R, alternating in the same rounds; both text towers for the prompt pair; the library entries of
    one step; the GEMM shapes that had no row in the tuning table.  Writes profiles/sampler_bench_sdxl.json."""
    import tinyfusers_amd.storage.tensor as T
    from tinyfusers_amd.native import hip
    from tinyfusers_amd.storage.state import param_shapes, update_state
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.vae.open_clip_text import synthetic_state
    from tinyfusers_amd.variants.samplers import DPMSolverPP2M
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.unet import SDXL

    T.ensure_init(0)

    def table_keys():
        n, key, cfg_ = ctypes.c_int(0), (ctypes.c_int * 10)(), (ctypes.c_int * 5)()
        hip.tf_gemm_tune_count(ctypes.byref(n))
        keys = set()
        for i in range(n.value):
            hip.tf_gemm_tune_entry(i, key, cfg_)
            keys.add(tuple(key))
        return keys
    shipped = table_keys()
    sched = DPMSolverPP2M().schedule(args.dpm_steps)
    side, images = args.sdxl_side, 1
    m = StableDiffusion(SDXL)
    big_g = "conditioner.embedders.1.model."
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(m.model.diffusion_model, synth_state_dict(param_shapes(m.model.diffusion_model), 0), "")
        update_state(m.conditioner, synth_state_dict({k: v for k, v in param_shapes(m.conditioner, "conditioner").items() if not k.startswith(big_g)}, 0), "conditioner")
        update_state(m.conditioner, synthetic_state(m.conditioner.embedders[1].cfg, 0, big_g, pooled=True), "conditioner")
    rng = np.random.default_rng(0)
    prompt = np.full((1, 77), 49407, dtype=np.int64); prompt[0, 0] = 49406; prompt[0, 1:10] = rng.integers(0, 49406, 9)
    empty = np.full((1, 77), 49407, dtype=np.int64); empty[0, 0] = 49406
    pg, eg = prompt.copy(), empty.copy()
    pg[0, 11:] = 0; eg[0, 2:] = 0
    out = {"protocol": f"median of {args.rounds} rounds of {args.replays} replays, (median ms, max - min over the rounds); SDXL base, {side} x {side} latent, "
                       f"CFG pair, {args.dpm_steps}-step DPM++2M, synthetic weights"}
    # 1. both towers, the prompt pair (eager launches, wall time from the call to the drained stream)
    m.encode_prompt(prompt, pg); m.encode_prompt(empty, eg)
    hip.tf_stream_sync(None)
    tw = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        ctx, pooled = m.encode_prompt(prompt, pg)
        unc, unc_pooled = m.encode_prompt(empty, eg)
        hip.tf_stream_sync(None)
        tw.append(1e3 * (time.perf_counter() - t0))
    out["both_towers_two_prompts_ms"] = (round(float(np.median(tw)), 3), round(max(tw) - min(tw), 3))
    pooled_h, unc_pooled_h = pooled.numpy(), unc_pooled.numpy()
    # 2. the step
    lat = m.latent_from_numpy(np.zeros((images, 4, side, side), np.float32))
    m.compile(unc, ctx, lat, sampler=sched)
    kw = dict(pooled=pooled_h, uncond_pooled=unc_pooled_h, original_size=(8 * side, 8 * side), target_size=(8 * side, 8 * side))
    m.start(seed=1234, **kw)
    m.synchronize()
    lat0 = T.DeviceArray.from_numpy(lat.numpy(), np.float32, "row")
    ev0, ev1, ms = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_float()
    hip.tf_event_create(ctypes.byref(ev0)); hip.tf_event_create(ctypes.byref(ev1))

    def replays(n):
        m.synchronize()
        hip.tf_event_record(ev0, m._stream.handle)
        for s_ in range(n):
            i = s_ % len(sched.timesteps)
            if i == 0:
                hip.tf_memcpy_async(lat.ptr, lat0.ptr, lat.nbytes, 3, m._stream.handle)
            m.step_sampler(i, 7.5)
        hip.tf_event_record(ev1, m._stream.handle)
        m.synchronize()
        hip.tf_event_elapsed_ms(ctypes.byref(ms), ev0, ev1)
        return ms.value / n
    replays(len(sched.timesteps))
    per = [replays(args.replays) for _ in range(args.rounds)]
    assert np.isfinite(lat.numpy()).all()
    out["step_ms"] = (round(float(np.median(per)), 4), round(max(per) - min(per), 4))
    ent = step_entries(T, m)
    out["step_entries"] = sum(ent.values())
    out["step_entries_by_name"] = dict(sorted(ent.items()))
    # 3. start(): the rows in one pass against one pass per timestep, alternating
    unet = m.model.diffusion_model

    def start_wall(per_timestep):
        if per_timestep:
            def rows_one_by_one():
                ts = [float(t) for t in sched.timesteps]
                keep = [unet.time_embedding_all(t, m._y_emb)[1] for t in ts]                  # S passes of the projection at M = R
                m._adm_table, m._emb_key = keep, m._weights_key()
                m._emb_rows = dict(zip(ts, keep))
            m._build_adm_table = rows_one_by_one
        t0 = time.perf_counter()
        m.start(seed=1234, **kw)
        m.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        if per_timestep:
            del m._build_adm_table                       # (the instance attribute: the method is back)
        return dt
    start_wall(False); start_wall(True)
    st = {"single_pass": [], "per_timestep": []}
    for _ in range(args.rounds):
        st["single_pass"].append(start_wall(False)); st["per_timestep"].append(start_wall(True))
    out["start_ms"] = {k: (round(float(np.median(v)), 3), round(max(v) - min(v), 3)) for k, v in st.items()}
    with T.use_stream(m._stream):
        tb = []
        for _ in range(args.rounds + 1):
            m.synchronize()
            t0 = time.perf_counter()
            keep = unet.time_embedding_table(sched.timesteps, m._y_emb)
            m.synchronize()
            t1 = time.perf_counter()
            keep = [unet.time_embedding_all(float(t), m._y_emb)[1] for t in sched.timesteps]
            m.synchronize()
            tb.append((1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)))
    out["rows_alone_ms"] = {"single_pass": round(float(np.median([a for a, _ in tb[1:]])), 3), "per_timestep": round(float(np.median([b for _, b in tb[1:]])), 3)}
    m.start(seed=1234, **kw); m.synchronize()
    bt = unet._prepare()
    out["plan"] = {"transformer_blocks": len(bt["kv_off"]), "kv_n": bt["kv_n"], "resblock_projection_columns": int(bt["emb_w"].shape[0]),
                   "rows_per_step": int(m._emb_cur.shape[0]), "table_rows": int(m._adm_table.shape[0])}
    out["gemm_shapes_autotuned_MNK"] = sorted({tuple(k[:3]) for k in table_keys() - shipped})
    hip.tf_event_destroy(ev0); hip.tf_event_destroy(ev1)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sampler_bench_sdxl.json")
    if not args.sdxl_no_write:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


def motion_bench(args):
    """--motion: the AnimateDiff video step (synthetic weights) -- SD-1.5, one 16-frame video on a 64 x 64 latent, CFG pair, --dpm-steps DPM++2M steps --
    against the plain image step at batch 16, alternating in the same rounds: medians of --rounds rounds of --replays replays with the spread between
    the rounds, the library entries of both steps, the GEMM shapes that had no row in the tuning table.  The share of the step spent in
    tf_sdpa_temporal_16 comes from a kernel trace in a run of its own: ``--motion-trace`` replays the video step alone (under rocprofv3 --kernel-trace
    --stats), ``--kernel-stats CSV`` reads that run's kernel_stats.csv into the result.  Writes profiles/sampler_bench_motion.json."""
    import csv
    import tinyfusers_amd.storage.tensor as T
    from tinyfusers_amd.native import hip
    from tinyfusers_amd.storage.state import param_shapes, update_state
    from tinyfusers_amd.storage.synth import synth_motion_state_dict, synth_normal, synth_state_dict
    from tinyfusers_amd.variants.samplers import DPMSolverPP2M, linear_alphas_cumprod
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.motion import MotionAdapter
    from tinyfusers_amd.vision.unet import SD15

    T.ensure_init(0)

    def table_keys():
        n, key, cfg_ = ctypes.c_int(0), (ctypes.c_int * 10)(), (ctypes.c_int * 5)()
        hip.tf_gemm_tune_count(ctypes.byref(n))
        keys = set()
        for i in range(n.value):
            hip.tf_gemm_tune_entry(i, key, cfg_)
            keys.add(tuple(key))
        return keys
    shipped = table_keys()
    frames, side = 16, args.motion_side
    sched = DPMSolverPP2M().schedule(args.dpm_steps, alphas_cumprod=linear_alphas_cumprod())
    ctx = T.DeviceArray.from_numpy(synth_normal(1234, "sd.context", (1, 77, 768)))
    unc = T.DeviceArray.from_numpy(synth_normal(1234, "sd.uncond", (1, 77, 768)))
    rep = lambda a: T.DeviceArray.from_numpy(np.repeat(a.numpy(), frames, axis=0))
    arms = {}
    for name in ("video",) if args.motion_trace else ("video", "image"):
        m = StableDiffusion(SD15)
        with contextlib.redirect_stdout(io.StringIO()):
            update_state(m.model.diffusion_model, synth_state_dict(param_shapes(m.model.diffusion_model), 0), "")
        lat = m.latent_from_numpy(np.zeros((frames, 4, side, side), np.float32))
        if name == "video":
            m.attach_motion(MotionAdapter.load(SD15, synth_motion_state_dict(SD15, 1, max_len=24)))
            m.compile(unc, ctx, lat, sampler=sched, motion=True, frames=frames)          # one prompt for the video
        else:
            m.compile(rep(unc), rep(ctx), lat, sampler=sched)                            # the same 16 latents as 16 images
        m.start(seed=1234); m.synchronize()
        arms[name] = (m, lat, T.DeviceArray.from_numpy(lat.numpy(), np.float32, "row"))
    ev0, ev1, ms = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_float()
    hip.tf_event_create(ctypes.byref(ev0)); hip.tf_event_create(ctypes.byref(ev1))

    def replays(name, n):
        m, lat, lat0 = arms[name]
        m.synchronize()
        hip.tf_event_record(ev0, m._stream.handle)
        for s_ in range(n):
            i = s_ % len(sched.timesteps)
            if i == 0:
                hip.tf_memcpy_async(lat.ptr, lat0.ptr, lat.nbytes, 3, m._stream.handle)
            m.step_sampler(i, 7.5)
        hip.tf_event_record(ev1, m._stream.handle)
        m.synchronize()
        hip.tf_event_elapsed_ms(ctypes.byref(ms), ev0, ev1)
        return ms.value / n
    if args.motion_trace:
        replays("video", 2 * len(sched.timesteps))
        assert np.isfinite(arms["video"][1].numpy()).all()
        return print(json.dumps({"traced_replays": 2 * len(sched.timesteps)}))
    per = {k: [] for k in arms}
    for k in arms:
        replays(k, len(sched.timesteps))
    for _ in range(args.rounds):
        for k in arms:
            per[k].append(replays(k, args.replays))
    for k in arms:
        assert np.isfinite(arms[k][1].numpy()).all()
    out = {"protocol": f"median of {args.rounds} rounds of {args.replays} replays, alternating video / image in the same run, (median ms, max - min over the rounds); "
                       f"SD-1.5, {side} x {side} latent, one {frames}-frame video (one prompt) against {frames} images, CFG pair, {args.dpm_steps}-step DPM++2M on the "
                       "linear-beta table, synthetic weights"}
    med = {k: float(np.median(v)) for k, v in per.items()}
    out["video_step_ms"] = (round(med["video"], 4), round(max(per["video"]) - min(per["video"]), 4))
    out["image_step_ms"] = (round(med["image"], 4), round(max(per["image"]) - min(per["image"]), 4))
    out["video_over_image"] = round(med["video"] / med["image"], 4)
    for k in arms:
        ent = step_entries(T, arms[k][0])
        out[f"{k}_step_entries"] = sum(ent.values())
        out[f"{k}_step_entries_by_name"] = dict(sorted(ent.items()))
    out["motion_modules"] = len(arms["video"][0]._motion_compiled.modules)
    share = "not measured"
    if args.kernel_stats:
        rows = list(csv.DictReader(open(args.kernel_stats)))
        total = sum(float(r["TotalDurationNs"]) for r in rows)
        temporal = sum(float(r["TotalDurationNs"]) for r in rows if "sdpa_temporal" in r["Name"])
        share = {"share_of_kernel_time": round(temporal / total, 4), "calls": sum(int(r["Calls"]) for r in rows if "sdpa_temporal" in r["Name"]),
                 "source": "rocprofv3 --kernel-trace --stats over --motion-trace's replays of the video step alone"}
    out["sdpa_temporal_16_share"] = share
    out["gemm_shapes_autotuned_MNK"] = sorted({tuple(k[:3]) for k in table_keys() - shipped})
    hip.tf_event_destroy(ev0); hip.tf_event_destroy(ev1)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sampler_bench_motion.json")
    if not args.motion_no_write:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--images", type=int, default=3)
    ap.add_argument("--dpm-steps", type=int, default=20)
    ap.add_argument("--inpaint", action="store_true", help="also time the masked step against the unmasked one, and the VAE encoder")
    ap.add_argument("--concat", choices=["inpaint", "edit"], default=None, help="also time the step of the 9-channel inpainting / 8-channel edit UNet against the plain one")
    ap.add_argument("--control", action="store_true", help="also time the ControlNet-conditioned step against the plain one, start(control_image=), and k_control_add")
    ap.add_argument("--lora", action="store_true", help="also time the LoRA merge (tf_lora_merge_16), the re-capture and the adapted step, for rank 16 and rank 128")
    ap.add_argument("--ip-adapter", action="store_true", help="also time the IP-Adapter step (fused dual attention) against the plain one and against a composed two-launch form")
    ap.add_argument("--freeu", action="store_true", help="also time the FreeU step (compile(..., freeu=True)) at the quoted values and at all ones against the plain one, and count the entries of both steps")
    ap.add_argument("--pag", action="store_true", help="also time the perturbed-attention-guidance step (compile(..., pag=True), three guidance groups) against the plain CFG one, and count the entries of both steps")
    ap.add_argument("--lcm", action="store_true", help="also time the guidance-free step (cfg=False) against the CFG step for DPM++2M and LCM, and LCM-4 cfg=False end to end")
    ap.add_argument("--sd2", action="store_true", help="a run of its own: the SD-2.x step (SD21, v-prediction, CFG rescale), the rescaled tail alone and the OpenCLIP text tower; writes profiles/sampler_bench_sd2.json")
    ap.add_argument("--sdxl", action="store_true", help="a run of its own: the SDXL base step, start() with the time-embedding rows in one pass against one pass per timestep, both text towers; writes profiles/sampler_bench_sdxl.json")
    ap.add_argument("--sdxl-side", type=int, default=128, help="with --sdxl: the latent's side (default 128: a 1024 x 1024 image)")
    ap.add_argument("--sdxl-no-write", action="store_true", help="with --sdxl: print the result only")
    ap.add_argument("--motion", action="store_true", help="a run of its own: the AnimateDiff video step (one 16-frame video) against the image step at batch 16; writes profiles/sampler_bench_motion.json")
    ap.add_argument("--motion-side", type=int, default=64, help="with --motion: the latent's side (default 64: 512 x 512 frames)")
    ap.add_argument("--motion-trace", action="store_true", help="with --motion: replay the video step alone and write nothing (the run to put under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--kernel-stats", default="", help="with --motion: the kernel_stats.csv of the --motion-trace run, for the share of tf_sdpa_temporal_16")
    ap.add_argument("--motion-no-write", action="store_true", help="with --motion: print the result only")
    args = ap.parse_args()
    if args.motion:
        return motion_bench(args)
    if args.sd2:
        return sd2_bench(args)
    if args.sdxl:
        return sdxl_bench(args)

    import torch  # noqa: F401  (the weight arena is a torch allocation)
    import tinyfusers_amd.storage.tensor as T
    from bench import build_weight_arena
    from tinyfusers_amd.native import hip
    from tinyfusers_amd.storage.state import param_shapes, update_state
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.variants.samplers import DDIM, DPMSolverPP2M
    from tinyfusers_amd.variants.sd import StableDiffusion

    T.ensure_init(0)
    ddim_m, dpm_m = StableDiffusion(), StableDiffusion()
    arena, _, _, _, state = build_weight_arena(ddim_m.model.diffusion_model, 0, 1, 0)
    update_state(dpm_m.model.diffusion_model, state, "")
    with contextlib.redirect_stdout(io.StringIO()):
        for name, sub in (("first_stage_model", ddim_m.first_stage_model), ("cond_stage_model", ddim_m.cond_stage_model)):
            update_state(sub, synth_state_dict(param_shapes(sub, name), 0), name)
    rng = np.random.default_rng(0)
    prompt = np.full((1, 77), 49407, dtype=np.int64); prompt[0, 0] = 49406; prompt[0, 1:10] = rng.integers(0, 49406, 9)
    empty = np.full((1, 77), 49407, dtype=np.int64); empty[0, 0] = 49406
    text_model = ddim_m.cond_stage_model.transformer.text_model
    text_model(prompt)
    ctx, unc = text_model(prompt), text_model(empty)
    hip.tf_stream_sync(None)

    noise = synth_normal(1234, "sd.latent", (1, 4, 64, 64))
    ddim_sched, dpm_sched = DDIM().schedule(50), DPMSolverPP2M().schedule(args.dpm_steps)
    lat_a, lat_b = ddim_m.latent_from_numpy(noise), dpm_m.latent_from_numpy(noise)
    ddim_m.compile(unc, ctx, lat_a, timesteps=ddim_sched.timesteps)                 # the DDIM step() path, exactly as bench.py captures it
    dpm_m.compile(unc, ctx, lat_b, sampler=dpm_sched)
    if args.inpaint:
        inp_m = StableDiffusion()
        update_state(inp_m.model.diffusion_model, state, "")
        lat_c = inp_m.latent_from_numpy(noise)
        inp_m.compile(unc, ctx, lat_c, sampler=dpm_sched, inpaint=True)
        half = np.zeros((1, 1, 64, 64), np.float32); half[..., :32] = 1.0
        inp_m.start(seed=1234, init_latent=0.5 * noise, mask=half)
    if args.concat:
        from tinyfusers_amd.storage.synth import synth_tensor
        from tinyfusers_amd.vision.unet import SD15_EDIT, SD15_INPAINT
        cfg = SD15_INPAINT if args.concat == "inpaint" else SD15_EDIT
        cat_m = StableDiffusion(cfg)
        conv_in = "input_blocks.0.0.weight"
        update_state(cat_m.model.diffusion_model, dict(state, **{conv_in: synth_tensor(0, conv_in, (320, cfg.in_channels, 3, 3))}), "")
        cat_m.first_stage_model = ddim_m.first_stage_model                 # (the model whose first_stage_model holds weights)
        lat_d = cat_m.latent_from_numpy(noise)
        cat_m.compile(unc, ctx, lat_d, sampler=dpm_sched, concat=args.concat)
        cond = 0.5 * synth_normal(1234, "sd.cond", (1, cfg.in_channels - 4, 64, 64))
        if args.concat == "inpaint":
            cond[:, 0] = 0.0; cond[:, 0, :, :32] = 1.0
        cat_m.start(seed=1234, cond_latent=cond)
    if args.control:
        from tinyfusers_amd.vision.controlnet import ControlNet
        ctl_m, net = StableDiffusion(), ControlNet()
        update_state(ctl_m.model.diffusion_model, state, "")
        with contextlib.redirect_stdout(io.StringIO()):
            update_state(net, synth_state_dict(param_shapes(net), 1), "")
        lat_e = ctl_m.latent_from_numpy(noise)
        ctl_m.attach_control(net).compile(unc, ctx, lat_e, sampler=dpm_sched, control=True)
        hint_img = np.random.default_rng(1).integers(0, 256, (1, 512, 512, 3), dtype=np.uint8)
        ctl_m.start(seed=1234, control_image=hint_img)
    ipa = {}                                                               # --ip-adapter: key -> (model, latent)
    if args.ip_adapter:
        import tinyfusers_amd.attention.attention as attn_mod
        from tinyfusers_amd.attention.sdpa import sdpa_strided
        from tinyfusers_amd.storage.ip_adapter import IPAdapter
        from tinyfusers_amd.storage.tensor import dtag

        def composed(o, q, k, v, k2, v2, scale_ptr, b, nh, tq, tk, tk2, hs, qs, ks, vs, k2s, v2s, os_):
            """what sdpa_dual_strided replaces: two plain attention launches and an add (scale 1; the tool's own arm, never in the library)"""
            o2 = T.DeviceArray.empty(o.shape, o.dtype, "row")
            sdpa_strided(o, q, k, v, b, nh, tq, tk, hs, qs, ks, vs, os_)
            sdpa_strided(o2, q, k2, v2, b, nh, tq, tk2, hs, qs, k2s, v2s, os_)
            hip.tf_add_16(dtag(o.dtype), o.ptr, o.ptr, o2.ptr, o.size, T._sh())
            o._base = (o._base, o2)                                        # (referenced while the launches are queued / captured)
            return o
        ip_emb = synth_normal(7, "ip.embeds", (1, 1024))
        fused_fn = attn_mod.sdpa_dual_strided
        for key, fn in (("dpmpp2m_ip_fused", fused_fn), ("dpmpp2m_ip_composed", composed)):
            m = StableDiffusion()
            update_state(m.model.diffusion_model, state, "")
            ad = IPAdapter(m.model.diffusion_model, 4, 1024)
            with contextlib.redirect_stdout(io.StringIO()):
                update_state(ad, {k_: (synth_normal(3, k_, s_, 0.03) + (1.0 if k_ == "image_proj.norm.weight" else 0.0)).astype(np.float16)
                                  for k_, s_ in ad.expected_shapes().items()}, "")
            lat_i = m.latent_from_numpy(noise)
            attn_mod.sdpa_dual_strided = fn
            try:
                m.attach_ip_adapter(ad).compile(unc, ctx, lat_i, sampler=dpm_sched, ip_adapter=True)
            finally:
                attn_mod.sdpa_dual_strided = fused_fn
            m.start(seed=1234, ip_image_embeds=ip_emb)
            ipa[key] = (m, lat_i)
    few = {}                                                               # --lcm: key -> (model, latent, schedule, guidance)
    if args.lcm:
        from tinyfusers_amd.variants.samplers import LCM
        lcm_sched = LCM().schedule(4)
        for key, sched, cfg_on in (("dpmpp2m_nocfg", dpm_sched, False), ("lcm", lcm_sched, True), ("lcm_nocfg", lcm_sched, False)):
            m = StableDiffusion()
            update_state(m.model.diffusion_model, state, "")
            lat_f = m.latent_from_numpy(noise)
            m.compile(unc if cfg_on else None, ctx, lat_f, sampler=sched, cfg=cfg_on)
            m.start(seed=1234)
            few[key] = (m, lat_f, sched, 7.5 if cfg_on else None)
    if args.freeu:
        for key, vals in (("dpmpp2m_freeu", (0.9, 0.2, 1.5, 1.6)), ("dpmpp2m_freeu_ones", (1.0, 1.0, 1.0, 1.0))):
            m = StableDiffusion()
            update_state(m.model.diffusion_model, state, "")
            lat_f = m.latent_from_numpy(noise)
            m.compile(unc, ctx, lat_f, sampler=dpm_sched, freeu=True)
            m.start(seed=1234, freeu=vals)
            few[key] = (m, lat_f, dpm_sched, 7.5)
    if args.pag:
        for key, layers in (("dpmpp2m_pag", "mid"), ("dpmpp2m_pag_all", "all")):
            m = StableDiffusion()
            update_state(m.model.diffusion_model, state, "")
            lat_f = m.latent_from_numpy(noise)
            m.compile(unc, ctx, lat_f, sampler=dpm_sched, pag=True)
            m.start(seed=1234, pag=(3.0, layers))
            few[key] = (m, lat_f, dpm_sched, 7.5)
    lat0 = T.DeviceArray.from_numpy(noise, np.float32, "row")
    ts, al, ap_ = ddim_sched.timesteps, ddim_sched.alphas, ddim_sched.alphas_prev

    def ddim_replays(n):
        for s in range(n):
            i = s % 50
            if i == 0:
                hip.tf_memcpy_async(lat_a.ptr, lat0.ptr, lat_a.nbytes, 3, ddim_m._stream.handle)   # a fresh trajectory every 50 steps
            ddim_m.step(ts[i], al[i], ap_[i], 7.5)

    def dpm_replays(n):
        k = len(dpm_sched.timesteps)
        for s in range(n):
            i = s % k
            if i == 0:
                hip.tf_memcpy_async(lat_b.ptr, lat0.ptr, lat_b.nbytes, 3, dpm_m._stream.handle)
            dpm_m.step_sampler(i, 7.5)

    def inp_replays(n):
        k = len(dpm_sched.timesteps)
        for s in range(n):
            i = s % k
            if i == 0:
                hip.tf_memcpy_async(lat_c.ptr, lat0.ptr, lat_c.nbytes, 3, inp_m._stream.handle)
            inp_m.step_sampler(i, 7.5)

    def cat_replays(n):
        k = len(dpm_sched.timesteps)
        for s in range(n):
            i = s % k
            if i == 0:
                hip.tf_memcpy_async(lat_d.ptr, lat0.ptr, lat_d.nbytes, 3, cat_m._stream.handle)
            cat_m.step_sampler(i, 7.5)

    def ctl_replays(n):
        k = len(dpm_sched.timesteps)
        for s in range(n):
            i = s % k
            if i == 0:
                hip.tf_memcpy_async(lat_e.ptr, lat0.ptr, lat_e.nbytes, 3, ctl_m._stream.handle)
            ctl_m.step_sampler(i, 7.5)

    def ipa_replays(key):
        m, lat_i = ipa[key]
        k = len(dpm_sched.timesteps)

        def replays(n):
            for s in range(n):
                i = s % k
                if i == 0:
                    hip.tf_memcpy_async(lat_i.ptr, lat0.ptr, lat_i.nbytes, 3, m._stream.handle)
                m.step_sampler(i, 7.5)
        return replays

    def few_replays(key):
        m, lat_f, sched, g = few[key]
        k = len(sched.timesteps)

        def replays(n):
            for s in range(n):
                i = s % k
                if i == 0:
                    hip.tf_memcpy_async(lat_f.ptr, lat0.ptr, lat_f.nbytes, 3, m._stream.handle)
                m.step_sampler(i, g)
        return replays

    def timed(model, fn, n):
        ev0, ev1, ms = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_float()
        hip.tf_event_create(ctypes.byref(ev0)); hip.tf_event_create(ctypes.byref(ev1))
        model.synchronize()
        hip.tf_event_record(ev0, model._stream.handle)
        fn(n)
        hip.tf_event_record(ev1, model._stream.handle)
        model.synchronize()
        hip.tf_event_elapsed_ms(ctypes.byref(ms), ev0, ev1)
        hip.tf_event_destroy(ev0); hip.tf_event_destroy(ev1)
        return ms.value / n

    ddim_replays(20); dpm_replays(20)
    step_ms = {"ddim": [], "dpmpp2m": []}
    if args.inpaint:
        inp_replays(20)
        step_ms["dpmpp2m_masked"] = []
    cat_key = f"dpmpp2m_concat_{args.concat}"
    if args.concat:
        cat_replays(20)
        step_ms[cat_key] = []
    if args.control:
        ctl_replays(20)
        step_ms["dpmpp2m_control"] = []
    ipa_fn = {k: ipa_replays(k) for k in ipa}
    for k in ipa:
        ipa_fn[k](20)
        step_ms[k] = []
    few_fn = {k: few_replays(k) for k in few}
    for k in few:
        few_fn[k](20)
        step_ms[k] = []
    for _ in range(args.rounds):
        step_ms["ddim"].append(timed(ddim_m, ddim_replays, args.replays))
        step_ms["dpmpp2m"].append(timed(dpm_m, dpm_replays, args.replays))
        if args.inpaint:
            step_ms["dpmpp2m_masked"].append(timed(inp_m, inp_replays, args.replays))
        if args.concat:
            step_ms[cat_key].append(timed(cat_m, cat_replays, args.replays))
        if args.control:
            step_ms["dpmpp2m_control"].append(timed(ctl_m, ctl_replays, args.replays))
        for k in ipa:
            step_ms[k].append(timed(ipa[k][0], ipa_fn[k], args.replays))
        for k in few:
            step_ms[k].append(timed(few[k][0], few_fn[k], args.replays))
    med = {k: float(np.median(v)) for k, v in step_ms.items()}
    extra = {}
    if args.inpaint:
        img = np.random.default_rng(0).integers(0, 256, (1, 512, 512, 3), dtype=np.uint8)
        enc = []
        with T.use_stream(ddim_m._stream):                                 # (the model whose first_stage_model holds weights)
            for r in range(args.rounds + 1):
                t0 = time.perf_counter()
                ddim_m.encode_image(img)
                ddim_m.synchronize()
                enc.append(time.perf_counter() - t0)                     # (includes the 0.75 MB host -> device upload of the image)
        extra = {"dpmpp2m_masked_step_ms": round(med["dpmpp2m_masked"], 4), "masked_over_unmasked": round(med["dpmpp2m_masked"] / med["dpmpp2m"], 4),
                 "encode_512_ms": round(1e3 * float(np.median(enc[1:])), 3)}
    if args.concat:
        img = np.random.default_rng(0).integers(0, 256, (1, 512, 512, 3), dtype=np.uint8)
        kw = {"cond_mask": np.arange(512)[None, None, :].repeat(512, 1) < 256} if args.concat == "inpaint" else {}
        cnd = []
        for r in range(args.rounds + 1):
            t0 = time.perf_counter()
            cat_m.start(seed=1234, cond_image=img, **kw)
            cat_m.synchronize()
            cnd.append(time.perf_counter() - t0)                         # (includes the 0.75 MB host -> device upload of the image)
        extra.update({f"{cat_key}_step_ms": round(med[cat_key], 4), "concat_over_plain": round(med[cat_key] / med["dpmpp2m"], 4),
                      "start_cond_image_512_ms": round(1e3 * float(np.median(cnd[1:])), 3)})

    if args.control:
        st = []
        for r in range(args.rounds + 1):
            t0 = time.perf_counter()
            ctl_m.start(seed=1234, control_image=hint_img)
            ctl_m.synchronize()
            st.append(time.perf_counter() - t0)                          # (includes the 0.75 MB host -> device upload of the hint)
        extra.update({"dpmpp2m_control_step_ms": round(med["dpmpp2m_control"], 4), "control_over_plain": round(med["dpmpp2m_control"] / med["dpmpp2m"], 4),
                      "start_control_image_512_ms": round(1e3 * float(np.median(st[1:])), 3), **control_add_bench(T, hip, ctl_m, timed, args)})

    if args.ip_adapter:
        fm = ipa["dpmpp2m_ip_fused"][0]
        st = []
        for r in range(args.rounds + 1):
            t0 = time.perf_counter()
            fm.start(seed=1234, ip_image_embeds=ip_emb)
            fm.synchronize()
            st.append(time.perf_counter() - t0)
        for k in ipa:
            assert np.isfinite(ipa[k][1].numpy()).all(), k
        spread_ms = lambda k: round(max(step_ms[k]) - min(step_ms[k]), 4)
        extra.update({"dpmpp2m_ip_fused_step_ms": round(med["dpmpp2m_ip_fused"], 4), "dpmpp2m_ip_composed_step_ms": round(med["dpmpp2m_ip_composed"], 4),
                      "ip_fused_over_plain": round(med["dpmpp2m_ip_fused"] / med["dpmpp2m"], 4), "ip_composed_over_plain": round(med["dpmpp2m_ip_composed"] / med["dpmpp2m"], 4),
                      "start_ip_image_embeds_ms": round(1e3 * float(np.median(st[1:])), 3),
                      "ip_round_spread_ms": {k: spread_ms(k) for k in ("dpmpp2m", "dpmpp2m_ip_fused", "dpmpp2m_ip_composed")},
                      **clip_vision_bench(T, hip, fm, ip_emb, args)})

    if args.lora:
        extra.update(lora_bench(T, hip, timed, args, state, ddim_m, unc, ctx, noise, dpm_sched, dpm_m, dpm_replays, lat0))

    if args.lcm:
        spread = lambda k: (max(step_ms[k]) - min(step_ms[k])) / med[k]    # a run's own spread between rounds, relative to its median
        for k in few:
            assert np.isfinite(few[k][1].numpy()).all(), k
        extra.update({"dpmpp2m_nocfg_step_ms": round(med["dpmpp2m_nocfg"], 4), "lcm_step_ms": round(med["lcm"], 4), "lcm_nocfg_step_ms": round(med["lcm_nocfg"], 4),
                      "dpmpp2m_nocfg_over_cfg": round(med["dpmpp2m_nocfg"] / med["dpmpp2m"], 4), "lcm_nocfg_over_cfg": round(med["lcm_nocfg"] / med["lcm"], 4),
                      "lcm_over_dpmpp2m": round(med["lcm"] / med["dpmpp2m"], 4),
                      "round_spread": {k: round(spread(k), 4) for k in ("dpmpp2m", "dpmpp2m_nocfg", "lcm", "lcm_nocfg")}})

    if args.freeu:
        spread_ms = lambda k: round(max(step_ms[k]) - min(step_ms[k]), 4)
        for k in ("dpmpp2m_freeu", "dpmpp2m_freeu_ones"):
            assert np.isfinite(few[k][1].numpy()).all(), k
        entries = {k: step_entries(T, m) for k, m in (("dpmpp2m", dpm_m), ("dpmpp2m_freeu", few["dpmpp2m_freeu"][0]))}
        extra.update({"dpmpp2m_freeu_step_ms": round(med["dpmpp2m_freeu"], 4), "dpmpp2m_freeu_ones_step_ms": round(med["dpmpp2m_freeu_ones"], 4),
                      "freeu_over_plain": round(med["dpmpp2m_freeu"] / med["dpmpp2m"], 4), "freeu_ones_over_plain": round(med["dpmpp2m_freeu_ones"] / med["dpmpp2m"], 4),
                      "freeu_round_spread_ms": {k: spread_ms(k) for k in ("dpmpp2m", "dpmpp2m_freeu", "dpmpp2m_freeu_ones")},
                      "step_entries": {k: sum(v.values()) for k, v in entries.items()},
                      "step_entries_freeu_minus_plain": {k: entries["dpmpp2m_freeu"].get(k, 0) - entries["dpmpp2m"].get(k, 0)
                                                         for k in sorted(set(entries["dpmpp2m"]) | set(entries["dpmpp2m_freeu"]))
                                                         if entries["dpmpp2m_freeu"].get(k, 0) != entries["dpmpp2m"].get(k, 0)},
                      **freeu_kernel_bench(T, hip, few["dpmpp2m_freeu"][0], timed, args)})

    if args.pag:
        spread_ms = lambda k: round(max(step_ms[k]) - min(step_ms[k]), 4)
        for k in ("dpmpp2m_pag", "dpmpp2m_pag_all"):
            assert np.isfinite(few[k][1].numpy()).all(), k
        entries = {k: step_entries(T, m) for k, m in (("dpmpp2m", dpm_m), ("dpmpp2m_pag", few["dpmpp2m_pag"][0]))}
        extra.update({"dpmpp2m_pag_step_ms": round(med["dpmpp2m_pag"], 4), "dpmpp2m_pag_all_step_ms": round(med["dpmpp2m_pag_all"], 4),
                      "pag_over_plain": round(med["dpmpp2m_pag"] / med["dpmpp2m"], 4), "pag_all_over_plain": round(med["dpmpp2m_pag_all"] / med["dpmpp2m"], 4),
                      "pag_round_spread_ms": {k: spread_ms(k) for k in ("dpmpp2m", "dpmpp2m_pag", "dpmpp2m_pag_all")},
                      "pag_step_entries": {k: sum(v.values()) for k, v in entries.items()},
                      "step_entries_pag_minus_plain": {k: entries["dpmpp2m_pag"].get(k, 0) - entries["dpmpp2m"].get(k, 0)
                                                       for k in sorted(set(entries["dpmpp2m"]) | set(entries["dpmpp2m_pag"]))
                                                       if entries["dpmpp2m_pag"].get(k, 0) != entries["dpmpp2m"].get(k, 0)}})

    def e2e(model, steps, sample, uncond=True):
        recs = []
        for n in range(args.images + 1):
            t0 = time.perf_counter()
            c, u = text_model(prompt), text_model(empty) if uncond else None      # (a cfg=False model encodes the prompt alone)
            hip.tf_stream_sync(None)
            t1 = time.perf_counter()
            model.set_context(u, c)
            sample(n)
            model.synchronize()
            t2 = time.perf_counter()
            with T.use_stream(model._stream):
                img = ddim_m.decode(model._latent)
            t3 = time.perf_counter()
            assert img.shape == (512, 512, 3)
            recs.append((t1 - t0, t2 - t1, t3 - t2))
        c, s, d = (float(np.median([r[i] for r in recs[1:]])) for i in range(3))
        return {"img_per_s": round(1.0 / (c + s + d), 3), "steps": steps, "clip_ms": round(c * 1e3, 2), "sampler_ms": round(s * 1e3, 2), "decode_ms": round(d * 1e3, 2)}

    def ddim_sample(n):
        ddim_m.set_latent(synth_normal(1234 + n, "sd.latent", (1, 4, 64, 64)))
        for i in range(50):
            ddim_m.step(ts[i], al[i], ap_[i], 7.5)

    def dpm_sample(n):
        dpm_m.start(seed=1234, image_offset=n)
        dpm_m.run(7.5)

    out = {"metric": "sd15_sampler_step_ms", "ddim_step_ms": round(med["ddim"], 4), "dpmpp2m_step_ms": round(med["dpmpp2m"], 4),
           "dpmpp2m_over_ddim": round(med["dpmpp2m"] / med["ddim"], 4), **extra, "replays": args.replays, "rounds": args.rounds,
           "step_ms_per_round": {k: [round(x, 4) for x in v] for k, v in step_ms.items()},
           "e2e_ddim50": e2e(ddim_m, 50, ddim_sample), "e2e_dpmpp2m": e2e(dpm_m, len(dpm_sched.timesteps), dpm_sample)}
    out["e2e_speedup"] = round(out["e2e_dpmpp2m"]["img_per_s"] / out["e2e_ddim50"]["img_per_s"], 3)
    if args.lcm:
        lcm1_m = few["lcm_nocfg"][0]

        def lcm_sample(n):
            lcm1_m.start(seed=1234, image_offset=n)
            lcm1_m.run()
        out["e2e_lcm4_nocfg"] = e2e(lcm1_m, 4, lcm_sample, uncond=False)
        out["e2e_lcm4_nocfg_over_dpmpp2m"] = round(out["e2e_lcm4_nocfg"]["img_per_s"] / out["e2e_dpmpp2m"]["img_per_s"], 3)
    print(json.dumps(out))
    if args.ip_adapter:
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sampler_bench_ip_adapter.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if args.freeu:
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sampler_bench_freeu.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if args.pag:
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sampler_bench_pag.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    del arena


if __name__ == "__main__":
    main()
