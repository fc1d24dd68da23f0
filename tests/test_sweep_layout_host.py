"""The host-side sizes and plans of the utility sweep (csrc/obe_sweep.hip: sweep_ws_bytes_bound, plan_sweep;
csrc/obe_sweep_cells.h: CellLayout, plan_cell_chunks; csrc/obe_sweep_bins.h: BinLayout, BinKeepLayout,
plan_bin_eval_waves) against tests/golden/sweep_layout_parent.json, recorded with tools/record_sweep_layout.py from the
build of commit 03e02b5, "Rebuild the bin grouping in four launches; fold finalize into bin_eval", before the sweep's
forms got a file and a host object each.  Every answer is an integer and is compared exactly.  Host only, no GPU.

The table crosses every branch of the functions: clouds of 1, 255 and 256 draws (one chunk, the one-workgroup sweep),
1 031, 131 072 / 131 073 (the bin units' cap), 1 048 576, 2^30 and 2^30 + 1 (the bin form's limit); 1 to 65 536 settings
(1, 2, 4 and 8 per lane; 1, 3, 6 and 8 wavefronts per group of bin_eval_kernel); 1, 2 and 5 channels (more than 4: at
most 2 settings per lane); 1, 3, 10 and 16 parameters (the packed width)."""
import itertools
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_layout_parent.json")
PARTICLES = (1, 255, 256, 1031, 131072, 131073, 1048576, 2 ** 30, 2 ** 30 + 1)
SETTINGS = (1, 193, 511, 512, 1024, 2048, 4096, 65536)
CHANNELS = (1, 2, 5)
DIMS = (1, 3, 10, 16)
DRAWS = (-1, 0, 30, 256, 257) + PARTICLES            # (none given, the one-workgroup sweep and its two limits)
WAVES_AT = (-5, 0) + SETTINGS + (16384, 16385, 32768, 32769, 65537, 2 ** 40)
# (x_min, x_max, d): a grid of 30 line widths, one of 3 000 (more cells than the cap), one point, and what is refused
GRIDS = ((1.5, 4.5, 0.1), (1.5, 4.5, 0.001), (3.0, 3.0, 0.1), (2.0, 10.5, 0.125), (4.5, 1.5, 0.1), (1.5, 4.5, 0.0),
         (1.5, 4.5, -0.1), (1.5, float("inf"), 0.1), (1.5, 4.5, float("nan")), (-1e308, 1e308, 1e-300))


def answers(cdll):
    """{function: [answer for every row of its table]}, the tables in the order of itertools.product."""
    plan_rows = list(itertools.product(GRIDS, SETTINGS + (0,), PARTICLES + (0,)))
    return {
        "obe_workspace_bytes": [int(cdll.obe_workspace_bytes(p, s, c, d))
                                for p, s, c, d in itertools.product(PARTICLES + (0,), SETTINGS + (0,), CHANNELS, DIMS)],
        "obe_sweep_bins_keep_bytes": [int(cdll.obe_sweep_bins_keep_bytes(n)) for n in DRAWS],
        "obe_sweep_settings_per_lane": [int(cdll.obe_sweep_settings_per_lane(s)) for s in (0,) + SETTINGS],
        "obe_sweep_settings_per_lane_for": [int(cdll.obe_sweep_settings_per_lane_for(s, n))
                                            for s, n in itertools.product((0,) + SETTINGS, DRAWS)],
        "obe_sweep_cells_plan": [int(cdll.obe_sweep_cells_plan(*g, s, n)) for g, s, n in plan_rows],
        "obe_sweep_bins_plan": [int(cdll.obe_sweep_bins_plan(*g, s, n)) for g, s, n in plan_rows],
        "obe_sweep_bins_eval_waves": [int(cdll.obe_sweep_bins_eval_waves(s)) for s in WAVES_AT],
    }


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)["host"]


@pytest.fixture(scope="module")
def got():
    from optbayesexpt_amd import _lib
    return answers(_lib.load().cdll)


FUNCTIONS = ("obe_workspace_bytes", "obe_sweep_bins_keep_bytes", "obe_sweep_settings_per_lane",
             "obe_sweep_settings_per_lane_for", "obe_sweep_cells_plan", "obe_sweep_bins_plan", "obe_sweep_bins_eval_waves")


@pytest.mark.parametrize("name", FUNCTIONS)
def test_the_library_answers_as_the_parent_did(got, recorded, name):
    assert sorted(got) == sorted(FUNCTIONS) == sorted(recorded)
    want = recorded[name]
    assert len(got[name]) == len(want) and len(want) > 0
    differ = [i for i, (a, b) in enumerate(zip(got[name], want)) if a != b]
    assert not differ, (name, len(differ), differ[:8])


def test_the_table_reaches_every_branch(recorded):
    """What the fixture says of itself: every form of every answer occurs."""
    assert set(recorded["obe_sweep_settings_per_lane"]) == {1, 2, 4, 8}
    assert set(recorded["obe_sweep_settings_per_lane_for"]) == {1, 2, 4, 8}
    assert set(recorded["obe_sweep_cells_plan"]) == {0, 1, 3} == set(recorded["obe_sweep_bins_plan"])
    assert set(recorded["obe_sweep_bins_eval_waves"]) == {1, 3, 6, 8}
    # (4 bytes per draw, rounded up to 16: sizes never fall, and 255 / 256 draws are the one pair within a rounding)
    keep = dict(zip(DRAWS, recorded["obe_sweep_bins_keep_bytes"]))
    assert keep[-1] == keep[0] == keep[1] and keep[255] == keep[256] < keep[257]
    assert len(set(keep.values())) == len(set(max(n, 1) for n in DRAWS)) - 1
    ws = recorded["obe_workspace_bytes"]
    assert len(ws) == 10 * 9 * 3 * 4 and min(ws) > 0 and len(set(ws)) > len(ws) // 2
