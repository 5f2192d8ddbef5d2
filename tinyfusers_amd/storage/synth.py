"""Deterministic synthetic weights / inputs for the SD-1.x UNet path (no checkpoint exists offline).

Build-owned (the reference ships no generator: its default init -- U(-sqrt3,sqrt3) conv weights,
all-ones Linear, vision/conv2d.py:52, ff/linear.py:114 -- overflows fp16 within a few layers).
Every tensor is drawn from its own Philox stream keyed by (seed, crc32(name)), so any subset can be
regenerated independently and both the HIP path and the CPU oracle see bit-identical values.
Values are rounded to fp16 once here; the oracle uses those fp16 values widened to fp32.
"""
import zlib

import numpy as np

__all__ = ["synth_tensor", "synth_state_dict", "synth_normal", "synth_motion_state_dict"]


def _rng(seed, name):
    return np.random.Generator(np.random.Philox(key=[int(seed) & 0xFFFFFFFFFFFFFFFF, zlib.crc32(name.encode())]))


def synth_normal(seed, name, shape, std=1.0, dtype=np.float32):
    """N(0, std^2) tensor from the (seed, name) stream."""
    x = _rng(seed, name).standard_normal(size=shape, dtype=np.float32)
    if std != 1.0:
        x *= np.float32(std)
    return x.astype(dtype, copy=False)


def synth_tensor(seed, name, shape):
    """One UNet parameter by LDM name: conv/linear weight ~ N(0, 1/fan_in); their bias ~ N(0, 0.02^2);
    norm gamma ~ 1 + 0.1 N, beta ~ 0.1 N.  Returned as fp16."""
    shape = tuple(shape)
    is_norm = len(shape) == 1 and (".norm" in name or name.endswith("in_layers.0.weight") or name.endswith("in_layers.0.bias")
                                   or name.endswith("out_layers.0.weight") or name.endswith("out_layers.0.bias")
                                   or name.startswith("out.0.") or "layer_norm" in name)
    x = _rng(seed, name).standard_normal(size=shape, dtype=np.float32)
    if name.endswith(".weight") and len(shape) >= 2:
        fan_in = int(np.prod(shape[1:]))
        x *= np.float32(1.0 / np.sqrt(fan_in))
    elif is_norm and name.endswith(".weight"):
        x = np.float32(1.0) + np.float32(0.1) * x
    elif is_norm:
        x *= np.float32(0.1)
    else:
        x *= np.float32(0.02)
    return x.astype(np.float16)


def synth_state_dict(shapes, seed=0, prefix=""):
    """name -> fp16 array for every entry of ``shapes`` (name -> shape)."""
    return {prefix + k: synth_tensor(seed, k, s) for k, s in shapes.items()}


def synth_motion_state_dict(cfg, seed=0, max_len=32, mid=False, pe=True):
    """A synthetic AnimateDiff motion-module file for the UNet configuration ``cfg`` (vision/motion.py: names in the AnimateDiff repository's
    spelling), name -> fp16 array: projection weights ~ N(0, 1 / fan_in), their bias ~ N(0, 0.02^2), every norm's gamma ~ 1 + 0.1 N and beta ~ 0.1 N,
    the positional tables the sinusoid + 0.1 N (``pe=False``: a file without them).  ``proj_out`` is NOT zero: the published files' zero-initialised
    proj_out has been trained away from zero, and a zero one would hide the whole module from a test."""
    from ..vision.motion import module_shapes, motion_slots, sinusoid_pe
    out = {}
    for prefix, _, c in motion_slots(cfg, mid):
        for rel, shape in module_shapes(c, max_len, pe).items():
            name = f"{prefix}.temporal_transformer.{rel}"
            x = _rng(seed, name).standard_normal(size=shape, dtype=np.float32)
            if rel.endswith(".pe"):
                x = sinusoid_pe(max_len, c) + np.float32(0.1) * x
            elif len(shape) == 2:
                x *= np.float32(1.0 / np.sqrt(shape[1]))
            elif rel.startswith("norm.") or ".norms." in rel or ".ff_norm." in rel:
                x = (np.float32(1.0) + np.float32(0.1) * x) if rel.endswith(".weight") else np.float32(0.1) * x
            else:
                x *= np.float32(0.02)
            out[name] = x.astype(np.float16)
    return out
