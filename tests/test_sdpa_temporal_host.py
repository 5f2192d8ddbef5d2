"""The temporal attention without a GPU: the planted inputs of tests/aux/sdpa_temporal_planted.py (what tests/test_gpu_sdpa_temporal.py's tolerance
rests on) and the pinned status and message of every launch tf_sdpa_temporal_16 refuses before it touches the device.

Planted inputs: q, k and the tables' sums are values of the storage type; the float64 softmax weights ARE the closed form (to 1e-12); the answer lies
in [-1, 1] (up to the storage rounding of v under tables) and is the mean of the value rows of the target's frames; each mutant of the float64
reference -- value rows rolled by one frame, the last frame dropped, a pixel / a head / a video reading its neighbour's queries, the tables left
out -- moves some output by more than 0.25."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aux"))

import sdpa_temporal_planted as TP  # noqa: E402

DTYPES = ("fp16", "bf16")
MIN_MOVE = 0.25
TF_E_ARG, TF_E_UNSUPPORTED = 10001, 10002


@pytest.mark.parametrize("pe", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hs", TP.HEAD_SIZES)
@pytest.mark.parametrize("f", TP.FRAMES)
def test_planted_inputs(f, hs, dtype, pe):
    g, p, nh = 3, 5, 3
    q, k, v, pq, pk, pv, ref = TP.planted(g, f, p, nh, hs, dtype, pe)
    for a in (q, k, v):
        assert a.shape == (g, f, p, nh, hs) and np.array_equal(a, TP.round16(a, dtype))            # what the device array will hold
    out, w = TP.ref64(q, k, v, pq, pk, pv, weights_too=True)
    assert np.array_equal(out, ref)
    closed = TP.weights(g, f, p, nh, hs)
    assert np.abs(w - closed).max() <= 1e-12                                                       # the softmax weights are known in closed form
    vv = TP.with_tables(v, pv)
    assert np.abs(vv).max() <= 1.0 + 2.0 ** -7 and np.abs(ref).max() <= 1.0 + 2.0 ** -7
    if not pe:
        assert np.array_equal(v * 128, np.round(v * 128)) and np.abs(ref).max() <= 1.0
    # the answer is the mean of the value rows of the frames that share the target's dimension (one frame while F <= HS)
    t = TP.target(g, f, p, nh).transpose(0, 2, 3, 1)
    hit = ((np.arange(f)[None, None, None, None, :] - t[..., None]) % hs == 0).astype(np.float64)
    mean = np.matmul(hit / hit.sum(-1, keepdims=True), vv.transpose(0, 2, 3, 1, 4)).transpose(0, 3, 1, 2, 4)
    assert np.abs(ref - mean).max() <= 1e-12
    if f <= hs:
        assert hit.sum(-1).max() == 1
    if f == 1:
        assert np.array_equal(ref, vv)                                                             # one frame: the answer is v' itself
        return
    moved = {"value rows rolled by one frame": TP.ref64(q, k, np.roll(v, 1, axis=1), pq, pk, pv),
             "a pixel reads its neighbour's queries": TP.ref64(np.roll(q, 1, axis=2), k, v, pq, pk, pv),
             "a head reads its neighbour's queries": TP.ref64(np.roll(q, 1, axis=3), k, v, pq, pk, pv),
             "a video reads its neighbour's queries": TP.ref64(np.roll(q, 1, axis=0), k, v, pq, pk, pv),
             "a head reads its neighbour's values": TP.ref64(q, k, np.roll(v, 1, axis=3), pq, pk, pv)}
    if f > 2:
        drop = TP.ref64(q[:, :-1], k[:, :-1], v[:, :-1], *(None if x is None else x[:-1] for x in (pq, pk, pv)))
        moved["the last frame dropped"] = np.concatenate([drop, ref[:, -1:]], axis=1)
    if pe:
        moved["the query table left out"] = TP.ref64(q, k, v, None, pk, pv)
        moved["the key table left out"] = TP.ref64(q, k, v, pq, None, pv)
        moved["the value table left out"] = TP.ref64(q, k, v, pq, pk, None)
    for what, m in moved.items():
        assert np.abs(ref - m).max() > MIN_MOVE, (what, np.abs(ref - m).max())


def test_value_rows_are_distinct():
    v = TP.values(3, 32, 5, 3, 8)
    assert len({row.tobytes() for row in v.reshape(-1, 8)}) == 3 * 32 * 5 * 3


def test_packed_layout():
    q, k, v = (np.full((2, 3, 5, 2, 8), x, np.float32) for x in (1.0, 2.0, 3.0))
    x = TP.packed(q, k, v)
    assert x.shape == (6, 5, 48) and (x[..., :16] == 1).all() and (x[..., 16:32] == 2).all() and (x[..., 32:] == 3).all()


# ---- refusals: status and message, before the device is touched (no GPU is needed, and none is used: the pointers are placeholders) ----------------
@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    import tinyfusers_amd.native as n
    return n


def _call(native, dtype=0, o=4096, q=4096, k=4096, v=4096, pe=(None, None, None), G=1, F=16, P=4, NH=2, HS=40, strides=None):
    c = NH * HS
    st = list(strides) if strides is not None else [3 * c * P, 3 * c, HS] * 3 + [c * P, c, HS]
    ptr = lambda a: None if a is None else ctypes.c_void_p(a)
    rc = native.lib.tf_sdpa_temporal_16(dtype, ptr(o), ptr(q), ptr(k), ptr(v), *(ptr(t) for t in pe), G, F, P, NH, HS, *st, None)
    return rc, native.lib.tf_last_error().decode()


REFUSALS = [
    ("F = 0", dict(F=0), TF_E_ARG, "tf_sdpa_temporal_16: bad sizes G=1 F=0 P=4 NH=2"),
    ("F = 33", dict(F=33), TF_E_UNSUPPORTED, "tf_sdpa_temporal_16: 33 frames: one launch attends over at most 32 (no sliding window)"),
    ("HS = 12", dict(HS=12), TF_E_ARG, "tf_sdpa_temporal_16: head size 12 must be a multiple of 8 in [8, 160]"),
    ("HS = 168", dict(HS=168), TF_E_ARG, "tf_sdpa_temporal_16: head size 168 must be a multiple of 8 in [8, 160]"),
    ("HS = 0", dict(HS=0), TF_E_ARG, "tf_sdpa_temporal_16: head size 0 must be a multiple of 8 in [8, 160]"),
    ("NH = 0", dict(NH=0), TF_E_ARG, "tf_sdpa_temporal_16: bad sizes G=1 F=16 P=4 NH=0"),
    ("G < 0", dict(G=-1), TF_E_ARG, "tf_sdpa_temporal_16: bad sizes G=-1 F=16 P=4 NH=2"),
    ("null o", dict(o=None), TF_E_ARG, "tf_sdpa_temporal_16: null tensor"),
    ("null q", dict(q=None), TF_E_ARG, "tf_sdpa_temporal_16: null tensor"),
    ("null k", dict(k=None), TF_E_ARG, "tf_sdpa_temporal_16: null tensor"),
    ("null v", dict(v=None), TF_E_ARG, "tf_sdpa_temporal_16: null tensor"),
    ("misaligned q", dict(q=4096 + 8), TF_E_ARG, "tf_sdpa_temporal_16: tensors and tables must be 16-byte aligned"),
    ("misaligned table", dict(pe=(4096, 4096 + 4, None)), TF_E_ARG, "tf_sdpa_temporal_16: tensors and tables must be 16-byte aligned"),
    ("dtype", dict(dtype=2), TF_E_ARG, "tf_sdpa_temporal_16: dtype=2 (0 = float16, 1 = bfloat16)"),
    ("too many work items", dict(G=1 << 16, P=1 << 16), TF_E_ARG, "tf_sdpa_temporal_16: too many (video, pixel, head group) work items"),
]


@pytest.mark.parametrize("what,kw,status,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(native, what, kw, status, message):
    assert _call(native, **kw) == (status, message)


@pytest.mark.parametrize("which", range(12))
def test_every_stride_must_be_a_multiple_of_8(native, which):
    st = [480, 240, 40] * 3 + [160, 80, 40]
    st[which] += 4
    assert _call(native, strides=st) == (TF_E_ARG, "tf_sdpa_temporal_16: q / k / v / o strides must be multiples of 8 elements (16-B rows)")


def test_nothing_to_do_is_no_error(native):
    """No video or no pixel: the launch returns TF_OK before the device is touched (as tf_sdpa_16 does for an empty batch)."""
    assert _call(native, G=0)[0] == 0 and _call(native, P=0)[0] == 0
