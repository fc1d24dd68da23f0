"""bin_eval_kernel finishing its own settings (csrc/obe_sweep_bins.h: bin_eval_kernel; csrc/obe_sweep_common.h: BinFinish) - variance, utility, and the first maximum
and worst kappa of every group of 64 settings, which used to be a launch of sweep_finalize over one chunk of moments -
against the bits of that launch: tests/golden/bin_chain_parent_bits.npz (see test_gpu_bin_rebuild.py for how and from
which commit it was recorded).

One cloud of 4 096 draws; slices of a grid of 65 537 settings at the counts that select every instance of the kernel
and every edge of a group: 1, 63, 64, 65; 16 384 and 16 385 (eight wavefronts per group, then six); 32 769 (three);
65 537 (one).  Noise as one value, as a row per setting (noise_ld > 0) and from the moments block (noise_ld < 0); cost
as one value and as an array.  Of a sweep of more than 257 settings the fixture holds the values at kept_of(n) (every
257th setting and the last 129); the best value, its index and kappa are of all of them.

Without the fixture: obe_utility_argmax on the sweep's own yvar uses the same utility_of and the same first-maximum
rule, so it gives the sweep's utility, best value and index bit for bit at every setting (noise_ld >= 0).  A cloud of
amplitude 0 has the same moments at every setting: a flat utility, index 0.  A poisoned cloud: NaN, kappa = NaN."""
import numpy as np
import pytest

from test_gpu_bin_sweep import make, prior_cloud, weights
from test_gpu_bin_rebuild import GOLDEN, same_bits, sweep_call

pytestmark = pytest.mark.gpu

GRID = 65537
N_DRAWS = 4096
COUNTS = ((1, 8), (63, 8), (64, 8), (65, 8), (16384, 8), (16385, 6), (32769, 3), (65537, 1))     # settings, wavefronts
NOISE = ("scalar", "rows", "moments")
COST = ("scalar", "array")


def kept_of(n):
    return np.arange(n) if n <= 257 else np.unique(np.concatenate([np.arange(0, n, 257), np.arange(n - 129, n)]))


def offset_of(n):
    """Where the slice of n settings starts in the grid (no multiple of 64 unless it has to be 0)."""
    return 0 if n == GRID else min((GRID - n) // 2 | 1, GRID - n)


def the_object(obe, cloud=None):
    cloud = prior_cloud(N_DRAWS, 9401) if cloud is None else cloud
    return make(obe, np.linspace(1.5, 4.5, GRID), cloud, weights(N_DRAWS, 9402))


def noise_of(kind, n):
    if kind == "scalar":
        return ("scalar", 250000.0)
    if kind == "rows":
        return ("rows", np.random.default_rng(9403 + n).uniform(1e5, 4e5, n))
    return ("moments", 2)            # the second moment of b over the sum of the weights


def cost_of(kind, n):
    return None if kind == "scalar" else np.random.default_rng(9404 + n).uniform(0.5, 2.0, n)


def sweep(o, n, noise, cost):
    from optbayesexpt_amd import _lib
    assert _lib.load().cdll.obe_sweep_bins_eval_waves(n) == dict(COUNTS)[n]
    got = sweep_call(o, n, s_begin=offset_of(n), noise=noise_of(noise, n), cost=cost_of(cost, n))
    assert np.isfinite(got["kappa"]) and np.all(np.isfinite(got["yvar"])) and np.all(np.isfinite(got["utility"]))
    return got


def kept(got, n):
    return {k: (v[kept_of(n)] if v.ndim else v) for k, v in got.items()}


def record(obe):
    """Everything the fixture holds of this file (tools/record_bin_chain_bits.py)."""
    o = the_object(obe)
    out = {}
    for n, _ in COUNTS:
        for noise in NOISE:
            for cost in COST:
                got = kept(sweep(o, n, noise, cost), n)
                if (noise, cost) != ("scalar", "scalar"):
                    del got["yvar"], got["kappa"]                 # (they do not depend on the noise or the cost)
                out.update({f"finalize {n} {noise} {cost} | {k}": v for k, v in got.items()})
    return out


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def obe(hip):
    import optbayesexpt_amd
    return optbayesexpt_amd


@pytest.fixture(scope="module")
def swept(obe):
    return the_object(obe)


def utility_argmax(o, yvar, noise, cost):
    """obe_utility_argmax on a yvar of one channel: (utility, best, idx)."""
    import torch
    from optbayesexpt_amd import _lib
    from optbayesexpt_amd.particlepdf import _ptr
    n = yvar.size
    dev = o._device
    f64 = dict(dtype=torch.float64, device=dev)
    yv = torch.from_numpy(yvar.reshape(1, n).copy()).to(dev)
    if noise[0] == "scalar":
        noise_t, noise_ld = torch.full((1,), noise[1], **f64), 0
    else:
        noise_t, noise_ld = torch.from_numpy(np.ascontiguousarray(noise[1])).to(dev), n
    cost_t = None if cost is None else torch.from_numpy(np.ascontiguousarray(cost)).to(dev)
    util = torch.zeros(n, **f64)
    out = _lib.pinned_array(2)
    best, idx = out[0:1], out.view(np.int64)[1:2]
    rc = o._mlib.cdll.obe_utility_argmax(_ptr(yv), 1, n, _ptr(noise_t), noise_ld, None if cost_t is None else _ptr(cost_t),
                                         1.0, _ptr(util), _lib.host_ptr(best), _lib.host_ptr(idx), _ptr(o._ws), o._ws_bytes,
                                         o._stream())
    torch.cuda.synchronize()
    assert rc == 0, o._mlib.last_error()
    return util.cpu().numpy(), float(best[0]), int(idx[0])


@pytest.mark.parametrize("n", [n for n, _ in COUNTS])
def test_every_instance_finishes_with_the_recorded_bits(swept, recorded, n):
    for noise in NOISE:
        for cost in COST:
            got = sweep(swept, n, noise, cost)
            want_yvar = recorded[f"finalize {n} scalar scalar | yvar"]
            assert np.array_equal(got["yvar"][kept_of(n)], want_yvar), (n, noise, cost)
            assert np.array_equal(got["kappa"], recorded[f"finalize {n} scalar scalar | kappa"]), (n, noise, cost)
            part = kept(got, n)
            if (noise, cost) != ("scalar", "scalar"):
                del part["yvar"], part["kappa"]
            same_bits(part, recorded, f"finalize {n} {noise} {cost}")
            if noise == "moments":
                continue
            utility, best, idx = utility_argmax(swept, got["yvar"], noise_of(noise, n), cost_of(cost, n))
            assert np.array_equal(utility, got["utility"]), (n, noise, cost)
            assert best == float(got["best"]) and idx == int(got["idx"]), (n, noise, cost)
            assert idx == int(np.argmax(got["utility"])) and best == got["utility"][idx]


@pytest.mark.parametrize("n", [65, 16385, 65537])
def test_a_flat_utility_returns_index_0(obe, n):
    cloud = prior_cloud(N_DRAWS, 9405)
    cloud[1] = 0.0                                           # amplitude 0: y = b at every setting
    got = sweep_call(the_object(obe, cloud), n, s_begin=offset_of(n))
    assert np.all(got["utility"] == got["utility"][0]) and got["utility"][0] > 0.0
    assert int(got["idx"]) == 0 and float(got["best"]) == got["utility"][0]


@pytest.mark.parametrize("n", [65, 16385, 65537])
def test_a_poisoned_cloud_returns_nan(obe, n):
    from optbayesexpt_amd import _lib
    cloud = prior_cloud(N_DRAWS, 9406)
    cloud[0, 7] = 3.0 + 1.01 * _lib.OBE_BIN_MAX * 2.0 / _lib.OBE_CELL_RHO_INV * 0.1       # a span beyond the cap
    got = sweep_call(the_object(obe, cloud), n, s_begin=offset_of(n))
    assert np.all(np.isnan(got["yvar"])) and np.isnan(got["kappa"])
