"""Which kernel family a dual attention launch runs (tf_sdpa_dual_instance: the rule tf_sdpa_dual_16 branches on, host code, no device needed), and
what the launch refuses before it touches a device: pins the table tests/test_gpu_sdpa_dual.py walks (tests/aux/sdpa_dual_planted.py: ROWS), that
the rule is tf_sdpa_instance's with the split forms left out, and the status and message of every refusal."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "aux"))

import sdpa_dual_planted as D  # noqa: E402
import sdpa_planted as P  # noqa: E402

F16, BF16 = 0, 1
E_ARG, E_UNSUPPORTED = 10001, 10002


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import tinyfusers_amd.native as n
    return n.lib


@pytest.fixture(scope="module")
def names():
    from tinyfusers_amd.attention.sdpa import SDPA_INSTANCES
    return SDPA_INSTANCES


def dual(lib, names, dtype, b, nh, tq, tk, tk2, hs, st=None):
    rc = lib.tf_sdpa_dual_instance(dtype, b, nh, tq, tk, tk2, hs, *(st or [hs] * 4))
    return names.get(rc, rc)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_instance_table(lib, names, dtype):
    for row, b, nh, tq, hs in D.ROWS:
        c = nh * hs
        for tk in P.KEY_COUNTS:
            for tk2 in D.IMAGE_KEY_COUNTS + (64,):
                assert dual(lib, names, dtype, b, nh, tq, tk, tk2, hs) == row, (row, hs, tk, tk2)
                assert dual(lib, names, dtype, b, nh, tq, tk, tk2, hs, [2 * c, 2 * c, 4 * c, 4 * c]) == row     # the step's k | v buffers


def test_the_rule_is_the_text_launch_s_without_the_split_forms(lib, names):
    """Whatever tf_sdpa_force_split holds: where the text launch alone would split, the dual launch runs the unsplit family of the same shape."""
    try:
        for ks in (0, 1, 2):
            assert lib.tf_sdpa_force_split(ks) == 0
            for b, nh, tq, tk, hs in [(2, 8, 4096, 77, 40), (2, 8, 1024, 77, 80), (2, 8, 256, 77, 160), (2, 8, 64, 77, 160), (1, 8, 4096, 77, 40),
                                      (1, 2, 200, 330, 80), (2, 8, 4096, 4096, 40), (16, 16, 300, 330, 40), (1, 127, 200, 77, 160), (1, 128, 200, 77, 160)]:
                assert lib.tf_sdpa_force_split(1) == 0
                want = names[lib.tf_sdpa_instance(F16, b, nh, tq, tk, hs, hs, hs, 0)]
                assert lib.tf_sdpa_force_split(ks) == 0
                for dtype in (F16, BF16):
                    assert dual(lib, names, dtype, b, nh, tq, tk, 4, hs) == want, (ks, b, nh, tq, tk, hs)
    finally:
        lib.tf_sdpa_force_split(0)


def _launch(lib, dtype=F16, ptrs=None, tk=77, tk2=4, hs=40, b=1, nh=2, tq=200, k_st=None, k2_st=None, v2_st=None, q_st=None, o_st=None):
    p = ptrs or [ctypes.c_void_p(4096)] * 7                   # o q k v k2 v2 scale: placeholders, a refused launch reads none of them
    s = lambda t, st: (nh * t * hs, t * hs, st or hs)
    return lib.tf_sdpa_dual_16(dtype, p[0], p[1], p[2], p[3], tk, p[4], p[5], tk2, p[6], b, nh, tq, hs, *s(tq, q_st), *s(tk, k_st), *s(tk, None), *s(tk2, k2_st),
                               *s(tk2, v2_st), *s(tq, o_st), None)


def test_refusals(lib, names):
    msg = lambda: lib.tf_last_error()
    assert _launch(lib, tk2=0) == E_ARG and b"tf_sdpa_dual_16" in msg() and b"Tk2=0" in msg()
    assert _launch(lib, tk2=65) == E_UNSUPPORTED and b"Tk2=65" in msg() and b"64" in msg()
    assert _launch(lib, tk=0) == E_ARG and b"Tk=0" in msg()
    for hs in (64, 128, 32, 72):                                    # head sizes tf_sdpa_16 runs, without a dual form
        assert _launch(lib, hs=hs) == E_UNSUPPORTED and b"head size %d" % hs in msg()
    assert _launch(lib, hs=44) == E_ARG and _launch(lib, hs=168) == E_ARG and b"multiple of 8" in msg()
    assert _launch(lib, dtype=2) == E_ARG and b"dtype=2" in msg()
    for i in range(7):                                              # a null o / q / k / v / k2 / v2 / scale
        p = [ctypes.c_void_p(4096)] * 7
        p[i] = None
        assert _launch(lib, ptrs=p) == E_ARG and b"null" in msg(), i
    for kw in ("k_st", "k2_st", "v2_st", "q_st"):
        assert _launch(lib, **{kw: 44}) == E_ARG and b"multiples of 8" in msg(), kw
    assert _launch(lib, o_st=42) == E_ARG and b"multiples of 4" in msg()
    # the 2 GiB slice rule, for either key set
    big = 1 << 25                                                   # 64 keys x 2^25 elements x 2 bytes = 4 GiB
    assert _launch(lib, tk2=64, k2_st=big) == E_UNSUPPORTED and b"32-bit" in msg() and b"Tk=64" in msg()
    assert _launch(lib, tk2=64, v2_st=big) == E_UNSUPPORTED and b"32-bit" in msg()
    assert _launch(lib, tk=1 << 20, k_st=1024) == E_UNSUPPORTED and b"32-bit" in msg()
    assert _launch(lib, b=0) == 0 and _launch(lib, tq=0) == 0       # nothing to do is no error (tf_sdpa_16's convention)
    # the query refuses what the launch refuses
    q = lambda **k: lib.tf_sdpa_dual_instance(k.get("dtype", F16), 1, 2, 200, k.get("tk", 77), k.get("tk2", 4), k.get("hs", 40), *k.get("st", [k.get("hs", 40)] * 4))
    assert q(tk2=0) == E_ARG and b"tf_sdpa_dual_instance" in msg()
    assert q(tk2=65) == E_UNSUPPORTED and q(hs=64) == E_UNSUPPORTED and q(hs=44) == E_ARG and q(dtype=3) == E_ARG
    assert q(st=[40, 40, 44, 40]) == E_ARG and q(tk2=64, st=[40, 40, big, 40]) == E_UNSUPPORTED and b"32-bit" in msg()
