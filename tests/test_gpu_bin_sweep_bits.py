"""The bin sweep (OBE_SWEEP_BINS) pinned to recorded bits: yvar of four seeded calls against
tests/golden/bin_sweep_parent_bits.npz, np.array_equal.

The fixture was recorded on one MI355X with tools/record_bin_sweep_bits.py (which imports cases() and sweep() from
this file) from the build of commit 48a9df2, "Add device-side quantiles of the next reading: reading_quantile()":
the last commit in which bin_eval_kernel walked every bin with one wavefront per 64 settings and bin_moments_kernel
reduced its 86 sums by 86 butterflies.  Later schedules of the two kernels (several wavefronts per group of settings,
loads ahead of the arithmetic, one transposed reduction) add the same numbers in the same order, so they give these
bits; a change that does not is a change of the association, not of the schedule.  The file holds the four yvar arrays
and nothing else; the inputs are made here from seeds.

The shapes: 7 draws (every item a few lanes of one trip), 4 099 draws (items of several trips with a ragged last
one), 150 001 draws (bins of four items: the fold), and a cloud with one bin of exactly 1 024 draws (one full item),
one of 1 025 (two items, the second of one draw) and two bins whose only item is under 64 draws."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bin_sweep_parent_bits.npz")
D = 0.1
ITEM_LAYOUT_COUNTS = (1024, 1025, 30, 63)        # draws in bins 0, 1, 2, 3 of the "items" case


def _prior(n, seed):
    g = np.random.default_rng(seed)
    return np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])


def _weights(n, seed):
    w = np.random.default_rng(seed).exponential(1.0, n)
    return w / w.sum()


def _item_layout():
    """x0 such that x0 / d fills bins 0..3 (width 2 / OBE_CELL_RHO_INV in x / d, the origin at the smallest x0) with
    ITEM_LAYOUT_COUNTS draws, well inside each bin, in a shuffled order."""
    from optbayesexpt_amd import _lib
    g = np.random.default_rng(4242)
    width = D * 2.0 / _lib.OBE_CELL_RHO_INV
    x0 = [np.array([3.0])]                                   # the origin: the first draw of bin 0
    for b, count in enumerate(ITEM_LAYOUT_COUNTS):
        x0.append(3.0 + width * (b + g.uniform(0.05, 0.95, count - (b == 0))))
    x0 = g.permutation(np.concatenate(x0))
    # (the kernels' own bin: (tau0 - origin) * (1 / width), truncated)
    bins = ((x0 / D - (x0 / D).min()) * (_lib.OBE_CELL_RHO_INV / 2.0)).astype(int)
    assert tuple(np.bincount(bins)) == ITEM_LAYOUT_COUNTS
    n = x0.size
    return np.array([x0, g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])


def cases():
    """name -> (settings, cloud, weights)"""
    out = {}
    for ns, n in ((257, 7), (63, 4099), (4099, 150001)):
        out[f"ns{ns}_n{n}"] = (np.linspace(1.5, 4.5, ns), _prior(n, 1000 + n), _weights(n, 2000 + n))
    cloud = _item_layout()
    out["items_1024_1025"] = (np.linspace(1.5, 4.5, 257), cloud, _weights(cloud.shape[1], 4243))
    return out


def sweep(obe, x, cloud, w):
    o = obe.OptBayesExpt(obe.models.lorentzian(1), (np.asarray(x, dtype=np.float64),), cloud.copy(), (D,),
                         utility_method="variance_full", auto_resample=False, default_noise_std=500.0)
    o.tuning_parameters["sweep_bins"] = "always"
    o.tuning_parameters["sweep_cells"] = "auto"
    o.tuning_parameters["sweep_shift"] = "never"
    o.particle_weights = w
    yvar = np.array(o.yvar_from_parameter_draws()[0], dtype=np.float64)
    assert o.last_sweep["bins"] is True and not o.last_sweep["shifted"], o.last_sweep
    return yvar


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("name", ["ns257_n7", "ns63_n4099", "ns4099_n150001", "items_1024_1025"])
def test_yvar_has_the_recorded_bits(hip, recorded, name):
    import optbayesexpt_amd
    x, cloud, w = cases()[name]
    got = sweep(optbayesexpt_amd, x, cloud, w)
    want = recorded[name]
    assert got.shape == want.shape and np.all(np.isfinite(got))
    differ = np.flatnonzero(got != want)
    assert np.array_equal(got, want), (name, differ.size, differ[:5], got[differ[:5]], want[differ[:5]])
