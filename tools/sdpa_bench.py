#!/usr/bin/env python3
"""Graph-timed SDPA shapes of the SD-1.5 step (self + cross attention at every level) through tf_sdpa_f16.
usage: tools/sdpa_bench.py [d40] [--ks 0|1|2]    (--ks: tf_sdpa_force_split -- 0 per-shape choice, 1 unsplit, 2 key slices wherever a split kernel exists)
       tools/sdpa_bench.py --dual               (the cross-attentions as plain / dual (tf_sdpa_dual_16) / two launches + add, interleaved rounds)"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinyfusers_amd.storage.tensor as T
from tinyfusers_amd.native import hip, lib
from tools.gemm_bench import time_call, st

SHAPES = [("self 64^2 d40", 2, 8, 4096, 4096, 40), ("self 32^2 d80", 2, 8, 1024, 1024, 80), ("self 16^2 d160", 2, 8, 256, 256, 160),
          ("self 8^2 d160", 2, 8, 64, 64, 160), ("cross 64^2 d40", 2, 8, 4096, 77, 40), ("cross 32^2 d80", 2, 8, 1024, 77, 80),
          ("cross 16^2 d160", 2, 8, 256, 77, 160), ("vae 64^2 d512", 1, 1, 4096, 4096, 512),
          ("c5 self 96^2 d40", 8, 8, 9216, 9216, 40), ("c5 cross 96^2 d40", 8, 8, 9216, 77, 40), ("c5 self 48^2 d80", 8, 8, 2304, 2304, 80)]


def dual(rounds=3, tk2=4):
    """--dual: the SD-1.5 cross-attentions (CFG batch 2 and batch 1) three ways, interleaved over `rounds` rounds in one process: the plain launch
    (tf_sdpa_16, text keys alone), the dual launch (tf_sdpa_dual_16, + `tk2` image keys) and what the dual launch replaces -- two tf_sdpa_16 launches and
    tf_add_16 (the image term at scale 1).  One line per shape: the median of each arm and its spread (max - min) between rounds, in us."""
    rng = np.random.default_rng(0)
    one = T.DeviceArray.from_numpy(np.float32([1.0]), np.float32, "row")
    for name, b, nh, tq, tk, hs in [s for s in SHAPES if s[0].startswith("cross")] + [("cross 64^2 d40 B1", 1, 8, 4096, 77, 40), ("cross 32^2 d80 B1", 1, 8, 1024, 77, 80)]:
        c = nh * hs
        arr = lambda t: T.DeviceArray.from_numpy(rng.standard_normal((b, t, c)).astype(np.float16), layout="row")
        q, k, v, k2, v2 = arr(tq), arr(tk), arr(tk), arr(tk2), arr(tk2)
        o, o2 = T.DeviceArray.empty((b, tq, c), np.float16, "row"), T.DeviceArray.empty((b, tq, c), np.float16, "row")
        s3 = lambda t: (t * c, hs, c)

        def plain():
            hip.tf_sdpa_16(0, o.ptr, q.ptr, k.ptr, v.ptr, b, nh, tq, tk, hs, *s3(tq), *s3(tk), *s3(tk), *s3(tq), 0, st.handle)

        def fused():
            hip.tf_sdpa_dual_16(0, o.ptr, q.ptr, k.ptr, v.ptr, tk, k2.ptr, v2.ptr, tk2, one.ptr, b, nh, tq, hs, *s3(tq), *s3(tk), *s3(tk), *s3(tk2), *s3(tk2), *s3(tq), st.handle)

        def composed():
            plain()
            hip.tf_sdpa_16(0, o2.ptr, q.ptr, k2.ptr, v2.ptr, b, nh, tq, tk2, hs, *s3(tq), *s3(tk2), *s3(tk2), *s3(tq), 0, st.handle)
            hip.tf_add_16(0, o.ptr, o.ptr, o2.ptr, o.size, st.handle)
        us = {f.__name__: [] for f in (plain, fused, composed)}
        for _ in range(rounds):
            for f in (plain, fused, composed):
                us[f.__name__].append(time_call(f))
        print(f"{name:18s} B={b} Tq={tq:5d} Tk={tk}+{tk2} d={hs:3d}  " + "  ".join(f"{n} {np.median(t):7.2f} us (spread {max(t) - min(t):.2f})" for n, t in us.items()), flush=True)


TEMPORAL_SHAPES = [("motion 64^2 C320", 4096, 8, 40), ("motion 32^2 C640", 1024, 8, 80), ("motion 16^2 C1280", 256, 8, 160), ("motion 8^2 C1280", 64, 8, 160)]


def temporal(rounds=5, g=2, f=16, out=None):
    """--temporal [--json FILE]: tf_sdpa_temporal_16 at the four shapes an AnimateDiff motion module has in an SD-1.5 UNet (64 x 64 latent, F = 16
    frames, CFG pair: G = 2), launched as the module would: q | k | v column views of the (G F, P, 3 C) projection, with the three tables, o a
    (G F, P, C) matrix.  Against (1) its HBM floor, q, k, v, o once at 8 TB/s, and (2) the composed arm: transpose the projection to (G, P, F, 3 C)
    (tf_transpose_f32 on pairs of elements), tf_sdpa_16 over the F tokens of the G P batches, transpose o back -- without tables, which that arm
    cannot add.  Arms alternate over `rounds` rounds in one process; one line per shape: the median of each arm and its spread (max - min), in us."""
    import ctypes
    import json
    rng = np.random.default_rng(0)
    rows = []
    for name, p, nh, hs in TEMPORAL_SHAPES:
        c = nh * hs
        qkv = T.DeviceArray.from_numpy(rng.standard_normal((g * f, p, 3 * c)).astype(np.float16), layout="row")
        pe = [T.DeviceArray.from_numpy(rng.standard_normal((f, c)).astype(np.float32), np.float32, "row") for _ in range(3)]
        o = T.DeviceArray.empty((g * f, p, c), np.float16, "row")
        qkv_t, o_t = T.DeviceArray.empty((g, p, f, 3 * c), np.float16, "row"), T.DeviceArray.empty((g, p, f, c), np.float16, "row")
        si, so = (p * 3 * c, 3 * c, hs), (p * c, c, hs)
        i4 = lambda *v: (ctypes.c_int * 4)(*v)
        sh_in, sh_out, swap = i4(g, f, p, 3 * c // 2), i4(g, p, f, c // 2), i4(0, 2, 1, 3)

        def fused():
            hip.tf_sdpa_temporal_16(0, o.ptr, qkv.ptr, qkv.ptr + 2 * c, qkv.ptr + 4 * c, pe[0].ptr, pe[1].ptr, pe[2].ptr, g, f, p, nh, hs, *si, *si, *si, *so, st.handle)

        def composed():
            hip.tf_transpose_f32(qkv_t.ptr, qkv.ptr, 4, sh_in, swap, st.handle)
            s3 = (f * 3 * c, hs, 3 * c)
            hip.tf_sdpa_16(0, o_t.ptr, qkv_t.ptr, qkv_t.ptr + 2 * c, qkv_t.ptr + 4 * c, g * p, nh, f, f, hs, *s3, *s3, *s3, f * c, hs, c, 0, st.handle)
            hip.tf_transpose_f32(o.ptr, o_t.ptr, 4, sh_out, swap, st.handle)
        us = {"fused": [], "composed": []}
        for _ in range(rounds):
            for fn in (fused, composed):
                us[fn.__name__].append(time_call(fn))
        floor = 4.0 * g * f * p * c * 2 / 8e12 * 1e6
        fl = 4.0 * g * p * nh * f * f * hs
        med = {n: float(np.median(t)) for n, t in us.items()}
        rows.append({"shape": name, "G": g, "F": f, "P": p, "NH": nh, "HS": hs, "hbm_floor_us": floor, "flops": fl, "rounds_us": us, "median_us": med,
                     "spread_us": {n: max(t) - min(t) for n, t in us.items()}})
        print(f"{name:18s} G={g} F={f} P={p:5d} NH={nh} d={hs:3d}  floor {floor:6.2f} us  " +
              "  ".join(f"{n} {med[n]:7.2f} us (spread {max(t) - min(t):.2f})" for n, t in us.items()) +
              f"  fused {fl / med['fused'] / 1e6:5.1f} TFLOP/s, {floor / med['fused'] * 100:4.1f}% of the floor's rate", flush=True)
    if out:
        with open(out, "w") as fh:
            json.dump({"tool": "tools/sdpa_bench.py --temporal", "rounds": rounds, "shapes": rows}, fh, indent=1)
            fh.write("\n")


def main():
    if "--dual" in sys.argv:
        return dual()
    if "--temporal" in sys.argv:
        return temporal(out=sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None)
    rng = np.random.default_rng(0)
    ks = int(sys.argv[sys.argv.index("--ks") + 1]) if "--ks" in sys.argv else 0
    split = hasattr(lib, "tf_sdpa_force_split")          # (an earlier library under TF_LIB_PATH has no key slices)
    if split:
        hip.tf_sdpa_force_split(ks)
    for name, b, nh, tq, tk, hs in SHAPES:
        if hs > 160 or (len(sys.argv) > 1 and sys.argv[1] == "d40" and hs != 40):
            continue
        c = nh * hs
        q = T.DeviceArray.from_numpy(rng.standard_normal((b, tq, c)).astype(np.float16), layout="row")
        k = T.DeviceArray.from_numpy(rng.standard_normal((b, tk, c)).astype(np.float16), layout="row")
        v = T.DeviceArray.from_numpy(rng.standard_normal((b, tk, c)).astype(np.float16), layout="row")
        o = T.DeviceArray.empty((b, tq, c), np.float16, "row")

        def fn():
            hip.tf_sdpa_f16(o.ptr, q.ptr, k.ptr, v.ptr, b, nh, tq, tk, hs, tq * c, hs, c, tk * c, hs, c, tk * c, hs, c, tq * c, hs, c, 0, st.handle)
        us = time_call(fn)
        fl = 4.0 * b * nh * tq * tk * hs
        print(f"{name:18s} B={b} NH={nh} Tq={tq:5d} Tk={tk:5d} d={hs:3d} slices={lib.tf_sdpa_split_ks(b, nh, tq, tk, hs, 0) if split else 1}  {us:8.1f} us  {fl / us / 1e6:7.1f} TFLOP/s", flush=True)


if __name__ == "__main__":
    main()
