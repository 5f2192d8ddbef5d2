"""CrossAttention(..., ip=(KVSlice, scale_ptr)): the decoupled cross-attention of an image-prompt adapter as ONE attention launch (sdpa_dual_strided)
in place of sdpa_strided, nothing else in the block changed.  Text K|V and image K|V are column slices of wider step-level buffers (other columns hold
large values: a mis-addressed slice shows), 200 queries (a ragged last query tile), 8 heads of 40 and 4 heads of 80, float16 and bfloat16.

  * scale 0 equals the block without ip= value for value (np.array_equal): the adapter switched off is the plain block, exactly;
  * scales 0.6 and -1.5 against a float64 restatement of the block on the device's own q (the 16-bit q the projection wrote is recomputed on the host
    from the same rounded inputs), at the project's stated gate for a block of the UNet (rel-L2 <= 5e-3 float16, 3e-2 bfloat16);
  * the scale is a device word: the same call follows a new value written behind the pointer;
  * one launch: with the profiler on, the adapted block books as many attention launches as the plain one;
  * ip= on self-attention, or a K|V whose batch or width does not fit, raises before any launch."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import sdpa_planted as P  # noqa: E402

pytestmark = pytest.mark.gpu

GATE = {"fp16": 5e-3, "bf16": 3e-2}
B, T, TK, TK2 = 2, 200, 77, 4


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T_
    T_.ensure_init(0)
    return T_


def _np_dtype(tf, dtype):
    return tf.bfloat16 if dtype == "bf16" else np.float16


class Case:
    def __init__(self, tf, nh, hs, dtype):
        from tinyfusers_amd.attention.attention import CrossAttention
        from tinyfusers_amd.storage.synth import synth_normal
        from tinyfusers_amd.vision.unet import KVSlice
        self.tf, self.dtype, self.nh, self.hs, c = tf, dtype, nh, hs, nh * hs
        dev = lambda a: tf.DeviceArray.from_numpy(a, _np_dtype(tf, dtype), "row")
        r = lambda name, shape, std=1.0: P.round16(synth_normal(41, f"ca.{name}.{nh}.{hs}", shape, std), dtype)
        self.x, self.wq, self.wo, self.bo = r("x", (B, T, c)), r("wq", (c, c), c ** -0.5), r("wo", (c, c), c ** -0.5), r("bo", (c,), 0.1)
        self.kv, self.kv2 = r("kv", (B, TK, 2 * c)), r("kv2", (B, TK2, 2 * c))
        # the slices inside wider buffers: [64 columns of 100.0 | k | v] and [2 c columns of 100.0 | k2 | v2 | c columns of 100.0]
        wide = lambda a, front, back: np.concatenate([np.full(a.shape[:2] + (front,), 100.0, np.float32), a, np.full(a.shape[:2] + (back,), 100.0, np.float32)], axis=-1)
        self.d_kv, self.d_kv2 = dev(wide(self.kv, 64, 0)), dev(wide(self.kv2, 2 * c, c))
        self.text, self.image = KVSlice(self.d_kv, 64, c, 2 * c + 64), KVSlice(self.d_kv2, 2 * c, c, 5 * c)
        self.attn = CrossAttention(c, 768, nh, hs, init=False)
        self.attn.to_q.weight, self.attn.to_out[0].weight, self.attn.to_out[0].bias = dev(self.wq), dev(self.wo), dev(self.bo)
        self.d_x = dev(self.x)
        self.scale = tf.DeviceArray.from_numpy(np.float32([0.0]), np.float32, "row")

    def run(self, s=None):
        if s is None:
            return self.attn(self.d_x, kv=self.text).numpy()
        self.scale.copy_from_numpy(np.float32([s]))
        return self.attn(self.d_x, kv=self.text, ip=(self.image, self.scale.ptr)).numpy()

    def ref(self, s):
        from tinyfusers_amd import config
        nh, hs, c = self.nh, self.hs, self.nh * self.hs
        f = lambda a: a.astype(np.float64)
        heads = lambda a: f(a).reshape(a.shape[0], a.shape[1], nh, hs).transpose(0, 2, 1, 3)
        q = heads(P.round16(f(self.x) @ f(self.wq).T, self.dtype))

        def attend(kv):
            p = np.exp((lambda sc: sc - sc.max(-1, keepdims=True))(q @ heads(kv[..., :c]).transpose(0, 1, 3, 2) / math.sqrt(hs)))
            return (p / p.sum(-1, keepdims=True)) @ heads(kv[..., c:])
        o = attend(self.kv) + s * attend(self.kv2)                          # (b, nh, t, hs)
        o = o.reshape(B, T, c) if config.head_merge == "reference_exact" else o.transpose(0, 2, 1, 3).reshape(B, T, c)
        return f(P.round16(o, self.dtype)) @ f(self.wo).T + f(self.bo)


@pytest.fixture(scope="module", params=[(8, 40, "fp16"), (8, 40, "bf16"), (4, 80, "fp16"), (4, 80, "bf16")], ids=lambda p: f"{p[0]}x{p[1]}-{p[2]}")
def case(tf, request):
    return Case(tf, *request.param)


def test_scale_zero_is_the_plain_block(case):
    plain, off = case.run(), case.run(0.0)
    assert np.isfinite(plain).all() and np.array_equal(plain, off)


def test_against_the_float64_block(case):
    plain = case.run()
    for s in (0.6, -1.5):
        got, ref = case.run(s).astype(np.float64), case.ref(s)
        rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        print(f"\ncross-attention ip {case.nh}x{case.hs} {case.dtype} s={s}: rel-L2 {rel:.3e}  gate {GATE[case.dtype]:.1e}")
        assert np.isfinite(got).all() and rel <= GATE[case.dtype], (s, rel)
        assert np.linalg.norm(got - plain) / np.linalg.norm(ref) > 0.05         # (the image term is no rounding error: it moves the block's output)
    rel0 = np.linalg.norm(plain - case.ref(0.0)) / np.linalg.norm(case.ref(0.0))
    assert rel0 <= GATE[case.dtype], rel0                                         # the restatement itself, on the plain block


def test_one_attention_launch(case):
    from tinyfusers_amd.native import hip, lib
    counts = []
    for s in (None, 0.6):
        case.run(s)                                                               # (warm: tuned, packed)
        hip.tf_prof_enable(1)
        try:
            case.run(s)
            ms, work, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
            assert lib.tf_prof_read_family(4, ctypes.byref(ms), ctypes.byref(work), ctypes.byref(n)) == 0
            counts.append((n.value, work.value))
        finally:
            hip.tf_prof_enable(0)
    fl = 4.0 * B * case.nh * T * case.hs
    assert counts[0] == (1, fl * TK) and counts[1] == (1, fl * (TK + TK2)), counts


def test_refusals(case, tf):
    from tinyfusers_amd.vision.unet import KVSlice
    ip = (case.image, case.scale.ptr)
    with pytest.raises(ValueError, match="self-attention"):
        case.attn(case.d_x, ip=ip)
    c = case.nh * case.hs
    one = tf.DeviceArray.zeros((1, TK2, 5 * c), _np_dtype(tf, case.dtype), "row")
    with pytest.raises(ValueError, match="does not fit"):
        case.attn(case.d_x, kv=case.text, ip=(KVSlice(one, 2 * c, c, 5 * c), case.scale.ptr))
    with pytest.raises(ValueError, match="does not fit"):
        case.attn(case.d_x, kv=case.text, ip=(KVSlice(case.d_kv2, 4 * c, c, 5 * c), case.scale.ptr))
