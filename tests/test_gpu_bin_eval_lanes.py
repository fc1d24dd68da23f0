"""bin_eval_kernel with a bin's row held in registers across the lanes (csrc/obe_models.h: LorentzBins::LaneRow) and
the occupied bins named by two 64-bit ballots: yvar of seeded calls through the C entry points against
tests/golden/bin_eval_lanes_parent_bits.npz, np.array_equal.

The fixture was recorded on one MI355X with tools/record_bin_eval_lanes_bits.py (which imports the cases from this
file) from the build of commit cf4c4b9, "Test the resample gather and nudge bit for bit at every cloud width": the
last commit in which the rows came through an LDS tile of 16 bins.  The file holds yvar arrays and nothing else; of a
sweep of more than 257 settings it holds the values at kept_of(n) (every 61st setting and the last 193), which is
what is compared.

What is new and what the cases ask of it:
  * plans of 1, 2, 16, 17, 63, 64, 65, 127 and 128 bins, every bin occupied: the 16-bin pieces of the old tile leave
    no trace, and bin 63 | bin 64 is the boundary between the two masks;
  * a plan of 128 bins whose bins 15, 16, 63, 64 and 126 hold no draw and whose other bins all do (the plan ends at
    the largest draw, so its last bin is never empty: 126 is the last bin that can be);
  * a plan of 17 bins one of which holds only zero-weight draws: its row is all zeros and is added, not skipped;
  * each of them at 1, 15, 17, 63, 65 and 257 settings (eight wavefronts per group of 64 settings), two of them also at
    16 385, 32 769 and 65 537 (six, three, one): the last wavefront has lanes without a setting at every position of
    a 16-lane row;
  * a prior of 4 099 draws.  What the recorder counts on the CPU for its 257 settings (--coefficients, the NumPy
    restatement of tests/test_bin_expansion_host.py): a coefficient that takes its neighbour's value, as a row fed from
    the wrong lane would, changes a recorded value for 79 of the 86 coefficients (silent: orders 23-26 of M1 and 24-26
    of M2, whose terms are below the last place of the sums); one ulp on a coefficient shows for 2 of 86 in one bin and
    for 5 of 86 in every bin: yvar does not see the last place of a single coefficient, so it is the neighbour count
    that says what these bits pin;
  * a rebuild into a keep buffer and a reuse of it, at eight wavefronts per group and at one."""
import os

import numpy as np
import pytest

from test_gpu_bin_sweep import c_sweep, make, prior_cloud, weights
from test_gpu_kept_bins import c_keep, keep_buffer

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bin_eval_lanes_parent_bits.npz")
D8 = 0.125                       # x0 / d and every bin edge are exact
N = 389                          # draws of a layout cloud
GRID = 65537                     # settings of every object: one wavefront per group when swept whole
SMALL = (1, 15, 17, 63, 65, 257)
LARGE = ((16385, 6), (32769, 3), (65537, 1))
PLANS = (1, 2, 16, 17, 63, 64, 65, 127, 128)
EMPTY = (15, 16, 63, 64, 126)
WITH_LARGE = ("plan of 65 bins", "bins 15, 16, 63, 64, 126 empty")
PLACEMENT_N = 4099


def kept_of(n):
    """The settings of a sweep of n whose values the fixture holds."""
    return np.arange(n) if n <= 257 else np.unique(np.concatenate([np.arange(0, n, 61), np.arange(n - 193, n)]))


def offset_of(n):
    """Where the slice of n settings starts in the grid (no multiple of 64 unless it has to be 0)."""
    return 0 if n == GRID else min((GRID - n) // 2 | 1, GRID - n)


def _layout(g, nbins, empty=()):
    """(cloud, bins of its draws): N draws whose x0 / d fill exactly the bins 0..nbins-1 but `empty`, the origin in
    bin 0 and the largest draw in the last bin."""
    from optbayesexpt_amd import _lib
    width = 2.0 / _lib.OBE_CELL_RHO_INV
    live = np.array([b for b in range(nbins) if b not in empty])
    bins = np.concatenate([live, g.choice(live, N - live.size)])
    at = bins + g.uniform(0.05, 0.95, N)
    at[0] = 0.0                                            # the origin
    if nbins > 1:
        at[live.size - 1] = nbins - 1 + 0.5                # the last bin, whatever else falls into it
    x0 = D8 * (20.0 + width * at)
    counted = int(np.floor((x0.max() / D8 - x0.min() / D8) / width)) + 1
    assert counted == nbins, (counted, nbins)
    got = np.floor((x0 / D8 - 20.0) / width).astype(int)
    assert set(got) == set(live)
    return np.array([x0, g.uniform(-2000, -400, N), g.normal(50000, 1000, N)]), got


def clouds():
    """name -> (cloud, weights, d)"""
    g = np.random.default_rng(8801)
    out = {}
    for nbins in PLANS:
        name = f"plan of {nbins} bin" + ("s" if nbins > 1 else "")
        out[name] = (_layout(g, nbins)[0], weights(N, 8802 + nbins), D8)
    out["bins 15, 16, 63, 64, 126 empty"] = (_layout(g, 128, EMPTY)[0], weights(N, 8803), D8)
    cloud, bins = _layout(g, 17)
    w = weights(N, 8804)
    w[bins == 5] = 0.0
    assert np.any(bins == 5)
    out["bin 5 of 17 holds only zero-weight draws"] = (cloud, w / w.sum(), D8)
    return out


def grid(d):
    return np.linspace(2.0, 10.5, GRID) if d == D8 else np.linspace(1.5, 4.5, GRID)


def slices_of(name):
    return SMALL + (tuple(n for n, _ in LARGE) if name in WITH_LARGE else ())


def key(name, n):
    return f"{name} | {n}"


def sweep_cloud(obe, name, cloud, w, d):
    """{key: yvar at kept_of(n)} of every slice of one cloud."""
    from optbayesexpt_amd import _lib
    waves = _lib.load().cdll.obe_sweep_bins_eval_waves
    o = make(obe, grid(d), cloud, w, d=d)
    out = {}
    for n in slices_of(name):
        assert waves(n) == dict(LARGE).get(n, 8), (n, waves(n))
        rc, yvar, kappa, _ = c_sweep(o, _lib.OBE_SWEEP_BINS, offset_of(n), n)
        assert rc == 0 and np.isfinite(kappa) and np.all(np.isfinite(yvar)), (name, n)
        out[key(name, n)] = yvar[kept_of(n)]
    return out


def placement_case():
    return prior_cloud(PLACEMENT_N, 8805), weights(PLACEMENT_N, 8806), 0.1


def sweep_placement(obe):
    from optbayesexpt_amd import _lib
    cloud, w, d = placement_case()
    o = make(obe, grid(d), cloud, w, d=d)
    out = {}
    for n in (257, 65537):
        rc, yvar, kappa, _ = c_sweep(o, _lib.OBE_SWEEP_BINS, offset_of(n), n)
        assert rc == 0 and np.isfinite(kappa) and np.all(np.isfinite(yvar)), n
        out[key("prior of 4099 draws", n)] = yvar[kept_of(n)]
    return out


KEEP_SETTINGS = (257, 65537)      # eight wavefronts per group, one


def sweep_keep(obe, ns):
    """(yvar of a rebuild into a keep buffer, yvar of a reuse of it) at kept_of(ns), all ns settings of the object."""
    from optbayesexpt_amd import _lib
    cloud, w, d = placement_case()
    o = make(obe, np.linspace(1.5, 4.5, ns), cloud[:, :513], w[:513] / w[:513].sum(), d=d)
    keep = keep_buffer(o)
    first = c_keep(o, _lib.OBE_SWEEP_BINS, keep)
    again = c_keep(o, _lib.OBE_SWEEP_BINS | _lib.OBE_SWEEP_BINS_KEPT, keep)
    assert np.isfinite(first[1]) and np.isfinite(again[1])
    return first[0][kept_of(ns)], again[0][kept_of(ns)]


def record(obe):
    """Everything the fixture holds (tools/record_bin_eval_lanes_bits.py)."""
    out = {}
    for name, (cloud, w, d) in clouds().items():
        out.update(sweep_cloud(obe, name, cloud, w, d))
    out.update(sweep_placement(obe))
    for ns in KEEP_SETTINGS:
        first, again = sweep_keep(obe, ns)
        assert np.array_equal(first, again), ns
        out[key("keep buffer", ns)] = first
    return out


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def obe(hip):
    import optbayesexpt_amd
    return optbayesexpt_amd


def same_bits(got, want, what):
    assert got.shape == want.shape, what
    differ = np.flatnonzero(got != want)
    assert np.array_equal(got, want), (what, differ.size, differ[:5], got[differ[:5]], want[differ[:5]])


CLOUDS = None


@pytest.mark.parametrize("name", [f"plan of {n} bin" + ("s" if n > 1 else "") for n in PLANS]
                         + ["bins 15, 16, 63, 64, 126 empty", "bin 5 of 17 holds only zero-weight draws"])
def test_every_instance_has_the_recorded_bits(obe, recorded, name):
    global CLOUDS
    if CLOUDS is None:
        CLOUDS = clouds()
    cloud, w, d = CLOUDS[name]
    got = sweep_cloud(obe, name, cloud, w, d)
    assert len(got) == len(slices_of(name))
    for k, v in got.items():
        same_bits(v, recorded[k], k)


def test_every_coefficient_is_fed_from_its_own_lane(obe, recorded):
    for k, v in sweep_placement(obe).items():
        same_bits(v, recorded[k], k)


@pytest.mark.parametrize("ns", KEEP_SETTINGS)
def test_rebuild_and_reuse_have_the_recorded_bits(obe, recorded, ns):
    first, again = sweep_keep(obe, ns)
    same_bits(first, recorded[key("keep buffer", ns)], f"rebuild, {ns} settings")
    same_bits(again, recorded[key("keep buffer", ns)], f"reuse, {ns} settings")
