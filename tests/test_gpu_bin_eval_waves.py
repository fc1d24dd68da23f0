"""bin_eval_kernel with several wavefronts per group of 64 settings (include/obe_hip.h: obe_sweep_bins_eval_waves): the
utility of a setting must not depend on how many wavefronts shared its bins.  A grid long enough for the
one-wavefront instance is swept whole through the C entry point, then in slices short enough for every other
instance, at offsets that are no multiple of 64: yvar of a slice is, bit for bit, that of the same settings in the
whole sweep.  Clouds of 513 draws at the layouts where the split over the wavefronts can go wrong, and the two calls
that answer NaN (a poisoned cloud, a refused reuse) at the largest instance."""
import numpy as np
import pytest

from test_gpu_bin_sweep import D, c_sweep, make, weights
from test_gpu_kept_bins import c_keep, keep_buffer, refused

pytestmark = pytest.mark.gpu

NS = 65599                      # from 65 537 settings on: one wavefront per group
# (offset, n_local, wavefronts per group): the largest instance, and the two between it and one
SLICES = [(7, 1, 8), (1031, 63, 8), (4099, 64, 8), (33333, 65, 8), (60001, 257, 8), (12345, 20000, 6), (3, 32769, 3),
          (1001, 60001, 3)]
N = 513


@pytest.fixture(scope="module")
def obe(hip):
    import optbayesexpt_amd
    return optbayesexpt_amd


def _layouts():
    from optbayesexpt_amd import _lib
    g = np.random.default_rng(9001)
    width = 2.0 / _lib.OBE_CELL_RHO_INV                 # of a bin, in x / d

    def cloud(x0):
        return np.array([x0, g.uniform(-2000, -400, x0.size), g.normal(50000, 1000, x0.size)])

    def spanning(first, last, d):                        # x0 / d from `first` to `last`, both ends present
        return d * np.concatenate([[first, last], g.uniform(first, last, N - 2)])
    cap = _lib.OBE_BIN_MAX
    # name -> (cloud, d, bins of the plan)
    return {
        "the prior of c3: tiles of 16, 16 and 9": (cloud(spanning(20.0, 40.0, D)), D, 41),
        "every draw in one bin": (cloud(3.0 + 0.02 * g.uniform(-1, 1, N)), D, 1),
        "17 bins: one in the second tile": (cloud(spanning(30.0, 30.0 + 16.5 * width, D)), D, 17),
        "two clusters, empty bins between": (cloud(np.concatenate([g.uniform(1.6, 1.7, 300), g.uniform(4.1, 4.3, 213)])),
                                             D, None),
        "the cap of OBE_BIN_MAX bins": (cloud(spanning(20.0, 20.0 + width * (cap - 1), 0.125)), 0.125, cap),
    }


LAYOUTS = None


@pytest.mark.parametrize("layout", ["the prior of c3: tiles of 16, 16 and 9", "every draw in one bin",
                                    "17 bins: one in the second tile", "two clusters, empty bins between",
                                    "the cap of OBE_BIN_MAX bins"])
def test_a_slice_has_the_bits_of_the_whole_sweep(obe, layout):
    from optbayesexpt_amd import _lib
    global LAYOUTS
    if LAYOUTS is None:
        LAYOUTS = _layouts()
    cloud, d, nbins = LAYOUTS[layout]
    assert cloud.shape[1] == N
    tau = cloud[0] / d
    counted = int(np.floor((tau.max() - tau.min()) * (_lib.OBE_CELL_RHO_INV / 2.0))) + 1
    if nbins is None:           # the clusters: occupied bins at both ends, more empty than occupied ones between
        occupied = np.unique(np.floor((tau - tau.min()) * (_lib.OBE_CELL_RHO_INV / 2.0)).astype(int))
        assert counted > 48 and occupied.size < counted // 4 and occupied[1] < 16 and occupied[-1] >= 48
    else:
        assert counted == nbins
    waves = _lib.load().cdll.obe_sweep_bins_eval_waves
    o = make(obe, np.linspace(1.5, 4.5, NS), cloud, weights(N, 9002), d=d)
    assert waves(NS) == 1
    rc, whole, kappa, _ = c_sweep(o, _lib.OBE_SWEEP_BINS, 0, NS)
    assert rc == 0 and np.isfinite(kappa) and np.all(np.isfinite(whole))
    for lo, n_local, w in SLICES:
        assert waves(n_local) == w, (n_local, w)
        rc, part, kappa, _ = c_sweep(o, _lib.OBE_SWEEP_BINS, lo, n_local)
        assert rc == 0 and np.isfinite(kappa)
        assert np.array_equal(part, whole[lo:lo + n_local]), (layout, lo, n_local, w)


def test_a_poisoned_cloud_answers_nan_at_the_largest_instance(obe):
    from optbayesexpt_amd import _lib
    g = np.random.default_rng(9003)
    x0 = np.concatenate([g.uniform(2, 4, N - 1), [3.0 + 1.01 * _lib.OBE_BIN_MAX * 2.0 / _lib.OBE_CELL_RHO_INV * D]])
    cloud = np.array([x0, g.uniform(-2000, -400, N), g.normal(50000, 1000, N)])
    o = make(obe, np.linspace(1.5, 4.5, 257), cloud, weights(N, 9004))
    assert _lib.load().cdll.obe_sweep_bins_eval_waves(257) == 8
    rc, got, kappa, _ = c_sweep(o, _lib.OBE_SWEEP_BINS, 0, 257)
    assert rc == 0 and np.isnan(kappa) and np.all(np.isnan(got))


def test_a_refused_reuse_answers_nan_at_the_largest_instance(obe):
    from optbayesexpt_amd import _lib
    g = np.random.default_rng(9005)
    cloud = np.array([g.uniform(2, 4, N), g.uniform(-2000, -400, N), g.normal(50000, 1000, N)])
    o = make(obe, np.linspace(1.5, 4.5, 257), cloud, weights(N, 9006))
    assert _lib.load().cdll.obe_sweep_bins_eval_waves(257) == 8
    keep = keep_buffer(o)                                 # never filled: the reuse is refused
    assert refused(c_keep(o, _lib.OBE_SWEEP_BINS | _lib.OBE_SWEEP_BINS_KEPT, keep))
    # ... and the same buffer, filled by a rebuild, is then reused at the same instance with the rebuild's bits
    first = c_keep(o, _lib.OBE_SWEEP_BINS, keep)
    again = c_keep(o, _lib.OBE_SWEEP_BINS | _lib.OBE_SWEEP_BINS_KEPT, keep)
    assert np.all(np.isfinite(first[0])) and np.array_equal(first[0], again[0])
