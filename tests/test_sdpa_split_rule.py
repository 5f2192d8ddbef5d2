"""Which attention launches take the key-slice kernel (tf_sdpa_split_ks: the launcher's own rule, host code, no device needed): only shapes whose
unsplit grid leaves the SIMDs short of waves, with two tiles of 64 keys for each slice, without the causal mask, at the head sizes that have a
split kernel; tf_sdpa_force_split overrides the first two conditions only."""
import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import tinyfusers_amd.native as n
    return n.lib


SD15_STEP = [  # b, nh, tq, tk, hs -> slices (the SD-1.5 step at CFG batch 2, 64 x 64 latent)
    ((2, 8, 4096, 4096, 40), 2), ((2, 8, 1024, 1024, 80), 2), ((2, 8, 256, 256, 160), 1), ((2, 8, 64, 64, 160), 1),
    ((2, 8, 4096, 77, 40), 1), ((2, 8, 1024, 77, 80), 1), ((2, 8, 256, 77, 160), 1),
]
FILLED = [  # grids that give every SIMD four waves already, or that the split form would not add waves to
    ((8, 8, 9216, 9216, 40), 1), ((8, 8, 2304, 2304, 80), 1), ((16, 8, 512, 512, 80), 1), ((4, 8, 4096, 4096, 40), 1), ((1, 2, 4096, 4096, 40), 1),
    ((2, 8, 1024, 1024, 64), 1), ((2, 8, 4096, 191, 40), 1), ((2, 8, 4096, 193, 40), 2),
]


def test_automatic_rule(lib):
    assert lib.tf_sdpa_force_split(0) == 0
    for (b, nh, tq, tk, hs), want in SD15_STEP + FILLED:
        assert lib.tf_sdpa_split_ks(b, nh, tq, tk, hs, 0) == want, (b, nh, tq, tk, hs)
        assert lib.tf_sdpa_split_ks(b, nh, tq, tk, hs, 1) == 1, (b, nh, tq, tk, hs)


def test_forced(lib):
    try:
        assert lib.tf_sdpa_force_split(2) == 0
        assert lib.tf_sdpa_split_ks(1, 2, 128, 64, 40, 0) == 2 and lib.tf_sdpa_split_ks(16, 8, 512, 512, 80, 0) == 2
        assert lib.tf_sdpa_split_ks(1, 2, 128, 256, 160, 0) == 1 and lib.tf_sdpa_split_ks(1, 2, 128, 256, 40, 1) == 1    # no split kernel: unsplit
        assert lib.tf_sdpa_force_split(1) == 0
        assert lib.tf_sdpa_split_ks(2, 8, 1024, 1024, 80, 0) == 1
        assert lib.tf_sdpa_force_split(3) == 10001 and b"tf_sdpa_force_split" in lib.tf_last_error()
        assert lib.tf_sdpa_split_ks(2, 8, 1024, 1024, 80, 0) == 1                                                           # (a rejected value changes nothing)
    finally:
        lib.tf_sdpa_force_split(0)
    assert lib.tf_sdpa_split_ks(2, 8, 1024, 1024, 80, 0) == 2
