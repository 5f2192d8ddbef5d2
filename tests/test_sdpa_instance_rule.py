"""Which kernel family an attention launch runs (tf_sdpa_instance: the rule tf_sdpa_f16 / tf_sdpa_16 branch on, host code, no device needed).
Pins the instance table tests/test_gpu_sdpa_instances.py walks (tests/aux/sdpa_planted.py: INSTANCE_ROWS), the thresholds between the instances,
the shapes the workload itself launches, and the refusal of a launch whose keys or values no kernel can address with 32-bit byte offsets."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "aux"))

import sdpa_planted as P  # noqa: E402

F16, BF16 = 0, 1


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


def test_python_names_mirror_the_header(names):
    hdr = open(os.path.join(ROOT, "include", "tinyfusers_hip.h")).read()
    enum = dict((n.lower(), int(v)) for n, v in re.findall(r"TF_SDPA_INST_([A-Z0-9_]+) = (\d+)", hdr))
    assert enum == {n: v for v, n in names.items()} and len(enum) == 5 and 0 not in names


def inst(lib, names, dtype, b, nh, tq, tk, hs, causal=0, k_st=None, v_st=None):
    rc = lib.tf_sdpa_instance(dtype, b, nh, tq, tk, hs, hs if k_st is None else k_st, hs if v_st is None else v_st, causal)
    return names.get(rc, rc)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_instance_table(lib, names, dtype):
    """Every row of the table, at both key counts, the packed self-attention key count and under the causal mask, names the instance it runs --
    under the tf_sdpa_force_split setting the GPU tests launch it with."""
    try:
        for row, b, nh, tq, hs in P.rows():
            c = nh * hs
            for tk, k_st in [(tk, hs) for tk in P.KEY_COUNTS] + [(77, 2 * c), (tq, 3 * c)]:     # contiguous; the k | v and q | k | v buffers
                ks = P.force_split_for(row, tk, hs)
                assert lib.tf_sdpa_force_split(ks) == 0
                assert inst(lib, names, dtype, b, nh, tq, tk, hs, 0, k_st, k_st) == row, (row, b, nh, tq, tk, hs, k_st)
                if ks == 1:          # the only rows the per-shape rule would move: it takes them to the split kernel
                    assert lib.tf_sdpa_force_split(0) == 0
                    assert inst(lib, names, dtype, b, nh, tq, tk, hs, 0, k_st, k_st) == "split"
            T = P.CAUSAL_T
            assert lib.tf_sdpa_force_split(P.force_split_for(row, T, hs)) == 0
            # never split under the causal mask: the split rows run what their unsplit twins run
            assert inst(lib, names, dtype, P.causal_batch(row, b), nh, T, T, hs, 1) == ("dma16" if row == "split" else row), (row, hs)
    finally:
        lib.tf_sdpa_force_split(0)


def test_thresholds(lib, names):
    """blocks2 = ceil(Tq / 128) NH B: 16-query waves below 256; blocks8 = ceil(Tq / 256) NH B: eight-wave blocks from 256 on, d = 40 / 80 only."""
    assert lib.tf_sdpa_force_split(0) == 0
    for hs in (40, 64, 80, 128, 160):
        assert inst(lib, names, F16, 1, 127, 200, 77, hs) == "dma16" and inst(lib, names, F16, 1, 128, 200, 77, hs) == "dma32"     # blocks2 254, 256
        assert inst(lib, names, F16, 1, 255, 128, 77, hs) == "dma16" and inst(lib, names, F16, 1, 255, 129, 77, hs) == "dma32"     # blocks2 255, 510
    for hs in (40, 80):
        assert inst(lib, names, F16, 1, 255, 256, 77, hs) == "dma32" and inst(lib, names, F16, 1, 256, 256, 77, hs) == "dma32_w8"
        assert inst(lib, names, F16, 1, 128, 257, 77, hs) == "dma32_w8"
    for hs in (64, 128, 160):
        assert inst(lib, names, F16, 16, 16, 300, 77, hs) == "dma32"                        # no eight-wave form
    for hs in range(8, 161, 8):
        want = "generic" if hs not in (40, 64, 80, 128, 160) else "dma16"
        assert inst(lib, names, F16, 1, 2, 200, 77, hs) == want and inst(lib, names, BF16, 1, 2, 200, 77, hs) == want
    # d = 40 on the eight-wave grid: split only while 8 waves per block leave the CUs short (blocks8 x 8 < 4096 waves)
    assert inst(lib, names, F16, 2, 8, 4096, 4096, 40) == "split" and inst(lib, names, F16, 4, 8, 4096, 4096, 40) == "dma32_w8"


def test_workload_shapes(lib, names):
    """The SD-1.5 step's own launches (CFG batch 2, 64 x 64 latent; config 5's 24 x 24 level; four images at 96 x 96)."""
    assert lib.tf_sdpa_force_split(0) == 0
    c = lambda hs: 8 * hs
    for (b, nh, tq, tk, hs), want in [((2, 8, 4096, 4096, 40), "split"), ((2, 8, 1024, 1024, 80), "split"), ((2, 8, 256, 256, 160), "dma16"),
                                      ((2, 8, 64, 64, 160), "dma16"), ((2, 8, 4096, 77, 40), "dma32_w8"), ((2, 8, 1024, 77, 80), "dma16"),
                                      ((8, 8, 576, 576, 160), "dma32"), ((8, 8, 9216, 9216, 40), "dma32_w8"), ((8, 8, 2304, 2304, 80), "dma32_w8"),
                                      ((1, 12, 77, 77, 64), "dma16")]:
        k_st = 3 * c(hs) if tq == tk else 2 * c(hs)
        for dtype in (F16, BF16):
            assert inst(lib, names, dtype, b, nh, tq, tk, hs, 0, k_st, k_st) == want, (b, nh, tq, tk, hs)
    assert inst(lib, names, F16, 1, 12, 77, 77, 64, 1) == "dma16"                            # CLIP's causal attention


def test_the_query_agrees_with_tf_sdpa_split_ks(lib, names):
    try:
        for ks in (0, 1, 2):
            assert lib.tf_sdpa_force_split(ks) == 0
            for b, nh, tq, tk, hs in [(2, 8, 4096, 4096, 40), (2, 8, 1024, 1024, 80), (1, 2, 200, 330, 80), (1, 2, 200, 77, 40), (16, 16, 300, 330, 40),
                                      (1, 2, 200, 330, 160), (1, 2, 200, 330, 72)]:
                for causal in (0, 1):
                    split = inst(lib, names, F16, b, nh, tq, tk, hs, causal) == "split"
                    assert split == (lib.tf_sdpa_split_ks(b, nh, tq, tk, hs, causal) == 2), (ks, b, nh, tq, tk, hs, causal)
    finally:
        lib.tf_sdpa_force_split(0)


def test_a_slice_beyond_32_bit_offsets_is_refused(lib, names):
    """Keys or values of one (batch, head) slice spanning 2 GiB or more: every kernel -- the generic one too -- computes 32-bit byte offsets inside
    the slice, so the launch is refused (TF_E_UNSUPPORTED) before anything touches a device: placeholder pointers, no launch."""
    P4 = [ctypes.c_void_p(4096)] * 4
    tk, hs = 1 << 20, 64
    big = 1024                                          # (tk x 1024 + 64) x 2 bytes = 2 GiB + 128
    ok = 1016                                           # (tk x 1016 + 64) x 2 bytes < 2 GiB
    assert inst(lib, names, F16, 1, 1, 8, tk, hs, 0, ok, ok) == "dma16"
    for dtype in (F16, BF16):
        for k_st, v_st in ((big, hs), (hs, big), (big, big), (1 << 40, hs)):
            assert lib.tf_sdpa_instance(dtype, 1, 1, 8, tk, hs, k_st, v_st, 0) == 10002
            assert b"tf_sdpa_instance" in lib.tf_last_error() and b"32-bit" in lib.tf_last_error()
            assert lib.tf_sdpa_16(dtype, *P4, 1, 1, 8, tk, hs, hs, hs, hs, k_st, k_st, k_st, v_st, v_st, v_st, hs, hs, hs, 0, None) == 10002
            assert b"tf_sdpa_f16" in lib.tf_last_error() and b"32-bit" in lib.tf_last_error()
    assert lib.tf_sdpa_f16(*P4, 1, 1, 8, tk, 72, *([72] * 3), *([big] * 3), *([72] * 3), *([72] * 3), 0, None) == 10002      # a generic head size
    assert lib.tf_sdpa_instance(F16, 1, 1, 8, tk, 72, big, 72, 0) == 10002
    # arguments the launcher rejects are rejected here
    assert lib.tf_sdpa_instance(2, 1, 1, 8, 8, 64, 64, 64, 0) == 10001 and lib.tf_sdpa_instance(F16, 1, 1, 8, 8, 12, 16, 16, 0) == 10001
    assert lib.tf_sdpa_instance(F16, 1, 1, 8, 8, 64, 60, 64, 0) == 10001 and b"tf_sdpa_instance" in lib.tf_last_error()
