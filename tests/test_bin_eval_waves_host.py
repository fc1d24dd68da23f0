"""obe_sweep_bins_eval_waves(): how many wavefronts share a group of 64 settings in bin_eval_kernel, as a function of
the settings of the call (csrc/obe_sweep_bins.h: plan_bin_eval_waves; DESIGN.md, "Several wavefronts per group of
settings").  Host only, no GPU."""
import numpy as np
import pytest

BUILT = {1: 4, 3: 4, 6: 2, 8: 1}        # W -> groups of 64 settings per workgroup
CUS, WAVES_PER_CU = 256, 12             # MI355X; three wavefronts of the kernel per SIMD


@pytest.fixture(scope="module")
def waves():
    from optbayesexpt_amd import _lib
    return _lib.load().cdll.obe_sweep_bins_eval_waves


def test_the_values_design_md_states(waves):
    assert waves(65536) == 3            # c3
    assert waves(4096) == 8             # c2
    assert waves(65536 // 8) == 8       # a one-of-eight slice of c3
    # the last size of every instance and the first of the next
    assert [waves(n) for n in (16384, 16385, 32768, 32769, 65536, 65537)] == [8, 6, 6, 3, 3, 1]


def test_monotone_never_above_the_largest_instance_and_one_beyond_the_chip(waves):
    sizes = np.unique(np.concatenate([np.arange(1, 700), np.arange(1, 1400) * 64, np.arange(1, 1400) * 64 + 1,
                                      [2 ** 20, 2 ** 31, 2 ** 40]]))
    got = [waves(int(n)) for n in sizes]
    assert set(got) == set(BUILT) and got[0] == max(BUILT)
    assert all(a >= b for a, b in zip(got, got[1:]))
    assert all(w == 1 for n, w in zip(sizes, got) if n > 65536)
    assert waves(0) == waves(-5) == max(BUILT)              # (as one setting)


def test_every_workgroup_of_a_launch_is_resident_at_once(waves):
    """W > 1: workgroups of G groups x W wavefronts, a multiple of four, 12 // (G W) of them per CU: one round, and
    never more wavefronts than the chip holds at the kernel's occupancy."""
    for n in list(range(1, 66000, 61)) + [16384, 32768, 65536]:
        w = waves(n)
        g = BUILT[w]
        assert (g * w) % 4 == 0
        workgroups = -(-(-(-n // 64)) // g)
        if w > 1:
            assert workgroups <= CUS * (WAVES_PER_CU // (g * w)) and workgroups * g * w <= CUS * WAVES_PER_CU, (n, w)
