"""The counting pass of a rebuild (csrc/obe_sweep_bins.h: bin_group_kernel<false>) ranks the 64 draws of a trip by
matching lanes: one ballot per bit of the bin index, whatever the number of distinct bins among them.  Here the sorted
position of every draw that a rebuild leaves in the keep buffer is compared with NumPy:

    dest = the inverse permutation of np.argsort(bin, kind="stable"),  bin = floor((x0 / d - min) * 2)

with d = 1/8 and x0 a multiple of 1/16, so that the division, the subtraction and the floor are exact and the host's
bin is the device's.  binstart (the first sorted position of every bin) and the plan's bin count are compared too.
The clouds are built to hit the match: one bin in all 64 lanes, 64 distinct bins, all OBE_BIN_MAX bins with b and
b + 64 in the same trip, two bins 64 apart in turn, last trips of 1 and 63 live lanes (whose dead lanes must not join
any bin), and a unit boundary inside a run of equal bins.  Without a keep buffer no position is left to read: that call
must give the five results of the call with one, bit for bit.  (tests/test_gpu_bin_rebuild.py stays the check against
the parent's bytes.)"""
import numpy as np
import pytest

from test_gpu_bin_sweep import make, weights
from test_gpu_bin_rebuild import D8, N_SETTINGS, keep_buffer, keep_bytes, sweep_call

pytestmark = pytest.mark.gpu

HEAD_INTS = 16                   # plan (origin, nbins, poison), mark, draws, d, mismatch, pad
BIN_MAX = 128


def _cases():
    g = np.random.default_rng(4201)
    out = {}
    out["64 draws in one bin"] = np.zeros(64, dtype=np.int64)
    out["64 draws in 64 bins"] = g.permutation(64)
    # trip 0: bins 0-31 and 64-95, trip 1: bins 32-63 and 96-127, each shuffled
    lo = np.arange(32)
    out["128 bins, b and b + 64 in one trip"] = np.concatenate([g.permutation(np.concatenate([lo, lo + 64])),
                                                                 g.permutation(np.concatenate([lo + 32, lo + 96]))])
    out["two bins 64 apart in turn"] = 64 * (np.arange(200) % 2)
    for n in (1, 63, 65, 4097):
        b = g.integers(0, BIN_MAX, n)
        out[f"{n} draws"] = b - b.min()
    # 131 073 draws: units of 128 draws, runs of 1000 equal bins
    out["a unit boundary inside a run"] = (np.arange(131073) // 1000) % BIN_MAX
    return out


CASES = None
NAMES = ["64 draws in one bin", "64 draws in 64 bins", "128 bins, b and b + 64 in one trip", "two bins 64 apart in turn",
         "1 draws", "63 draws", "65 draws", "4097 draws", "a unit boundary inside a run"]


@pytest.fixture(scope="module")
def obe(hip):
    import optbayesexpt_amd
    return optbayesexpt_amd


@pytest.mark.parametrize("name", NAMES)
def test_dest_is_the_stable_sort_by_bin(obe, name):
    global CASES
    if CASES is None:
        CASES = _cases()
        assert list(CASES) == NAMES
    bins = np.asarray(CASES[name], dtype=np.int64)
    n = bins.size
    g = np.random.default_rng(4202 + n)
    x0 = D8 * (20.0 + 0.5 * bins)
    # the host's bin, as the docstring states it
    tau0 = x0 / D8
    host_bin = np.floor((tau0 - tau0.min()) * 2.0).astype(np.int64)
    assert np.array_equal(host_bin, bins) and bins.min() == 0 and bins.max() < BIN_MAX
    cloud = np.array([x0, g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    o = make(obe, np.linspace(2.0, 10.5, N_SETTINGS), cloud, weights(n, 4203 + n), d=D8)
    keep = keep_buffer(o, n)
    with_buffer = sweep_call(o, N_SETTINGS, keep=keep)
    ints = keep_bytes(keep).view(np.int32)
    assert not np.isnan(with_buffer["kappa"]), name              # (not poisoned; one draw has no variance: inf)
    assert ints[2] == bins.max() + 1, (name, ints[2])
    counts = np.bincount(bins, minlength=BIN_MAX)
    binstart = ints[HEAD_INTS:HEAD_INTS + BIN_MAX + 1]
    assert np.array_equal(binstart, np.concatenate([[0], np.cumsum(counts)])), name
    order = np.argsort(bins, kind="stable")
    want = np.empty(n, dtype=np.int64)
    want[order] = np.arange(n)
    dest_at = (HEAD_INTS + 2 * (BIN_MAX + 2) + 3) & ~3
    dest = ints[dest_at:dest_at + n]
    differ = np.flatnonzero(dest != want)
    assert np.array_equal(dest, want), (name, differ.size, differ[:8], dest[differ[:8]], want[differ[:8]])
    without = sweep_call(o, N_SETTINGS)
    for k, v in with_buffer.items():
        assert np.array_equal(v, without[k]), (name, k)
