"""Whole cycles with the keep buffer in its records form (``tuning_parameters['sweep_bins_keep'] = True``, the default),
with the grouping alone (``'grouping'``) and without a buffer (False): the 16 seeded cycles of test_gpu_kept_bins.py
(4 200 settings x 40 000 particles, a set_pdf at cycle 9) choose the same settings with the same utilities, resample
in the same cycles and end with the same particles and weights, bit for bit; and with a drift per update every sweep
rebuilds."""
import numpy as np
import pytest

from test_gpu_kept_bins import N_CYCLES, SET_PDF_AT, final_state, new_experiment, one_cycle, replacement_cloud, run, \
    same_records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def obe(hip):
    import optbayesexpt_amd
    return optbayesexpt_amd


@pytest.fixture(scope="module")
def runs(obe):
    return {keep: run(obe, keep) for keep in (True, "grouping", False)}


def test_the_three_forms_give_the_same_cycles(runs):
    records, state = runs[False]
    assert not any(r[1] for r in records)
    resampled = [r[3] for r in records]
    assert any(resampled) and not all(resampled), resampled
    for keep in (True, "grouping"):
        got, got_state = runs[keep]
        same_records(got, records)
        assert np.array_equal(got_state[0], state[0]) and np.array_equal(got_state[1], state[1]), keep


def test_the_two_buffers_are_reused_in_the_same_cycles(runs):
    kept = [r[1] for r in runs[True][0]]
    assert kept == [r[1] for r in runs["grouping"][0]]
    resampled = [r[3] for r in runs[True][0]]
    for k, reused in enumerate(kept):
        fresh_cloud = k == 0 or resampled[k - 1] or k == SET_PDF_AT
        assert reused is (not fresh_cloud), (k, kept, resampled)


def test_the_buffer_sizes_follow_the_tuning_value(obe):
    sizes = {}
    for keep in (True, "grouping"):
        o = new_experiment(obe, keep)
        o.opt_setting()
        sizes[keep] = o._bins_keep[1].numel() * 4
        cdll = o._mlib.cdll
    assert sizes[True] == cdll.obe_sweep_bins_keep_records_bytes(40000)
    assert sizes["grouping"] == cdll.obe_sweep_bins_keep_bytes(40000)
    o = new_experiment(obe, False)
    o.opt_setting()
    assert "_bins_keep" not in o.__dict__


def drift_run(obe, keep):
    o = new_experiment(obe, keep)
    o.set_parameter_drift(np.array([1e-4, 0.5, 2.0]), per_update=True)
    records = []
    for k in range(N_CYCLES):
        if k == SET_PDF_AT:
            o.set_pdf(replacement_cloud())
        records.append(one_cycle(o, k))
    o._drop_speculative_sweep()
    return records, final_state(o)


def test_with_a_drift_per_update_every_sweep_rebuilds(obe):
    records, state = drift_run(obe, True)
    plain, plain_state = drift_run(obe, False)
    assert not any(r[1] for r in records), [r[1] for r in records]
    same_records(records, plain)
    assert np.array_equal(state[0], plain_state[0]) and np.array_equal(state[1], plain_state[1])
