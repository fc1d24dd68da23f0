"""The bins' grouping of a cloud kept from sweep to sweep (include/obe_hip.h: obe_sweep_utility_keep,
OBE_SWEEP_BINS_KEPT): a sweep that reuses the kept grouping writes the same packed records to the same sorted
positions as a sweep that rebuilds it, so every comparison here is bit for bit.  The object's bookkeeping (when it
may reuse), the exact continuation of whole cycles with and without the keep, across copies and restores, and the
checked refusals of the C entry point."""
import copy

import numpy as np
import pytest

from oracle import models as omodels
from test_gpu_bin_sweep import D, _layouts, make, prior_cloud, weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def obe(hip):
    import optbayesexpt_amd
    return optbayesexpt_amd


def sweep_bits(o):
    """One full sweep and one opt_setting() of the object as it stands: (yvar, utility, best index, kept, kept)."""
    yvar = np.array(o.yvar_from_parameter_draws()[0])
    first = o.last_sweep["kept"]
    assert o.last_sweep["bins"] and not o.last_sweep["shifted"], o.last_sweep
    utility = o._utility_dev.cpu().numpy().copy()
    o.opt_setting()
    assert o.last_sweep["bins"], o.last_sweep
    return yvar, utility, o.last_setting_index, first, o.last_sweep["kept"]


def check_reuse_equals_rebuild(obe, x, cloud, w1, w2, d, what):
    o = make(obe, x, cloud, w1, d=d)
    o.yvar_from_parameter_draws()
    assert o.last_sweep["bins"] and o.last_sweep["kept"] is False, (what, o.last_sweep)
    o.particle_weights = w2                                   # only the weights change: the grouping stands
    yvar, utility, best, kept_a, kept_b = sweep_bits(o)
    assert kept_a is True and kept_b is True, what
    fresh = make(obe, x, cloud, w2, d=d)
    ref_yvar, ref_utility, ref_best, fresh_a, fresh_b = sweep_bits(fresh)
    assert fresh_a is False and fresh_b is True, what          # (its second sweep reuses what its first one made)
    assert np.all(np.isfinite(ref_yvar)), what
    assert np.array_equal(yvar, ref_yvar), what
    assert np.array_equal(utility, ref_utility), what
    assert best == ref_best, what


@pytest.mark.parametrize("ns,n", [(63, 2), (257, 7), (4099, 513), (63, 4099), (4099, 4099)])
def test_reuse_gives_the_bits_of_a_rebuild(obe, ns, n):
    x = np.linspace(1.5, 4.5, ns)
    check_reuse_equals_rebuild(obe, x, prior_cloud(n, 300 + n), weights(n, 400 + n), weights(n, 500 + n), D,
                               f"{ns} settings x {n} particles")


LAYOUTS = None


@pytest.mark.parametrize("layout", ["every particle in one bin", "every particle in a bin of its own",
                                    "two clusters, empty bins between", "x0 on bin edges", "exactly OBE_BIN_MAX bins",
                                    "zero-weight particles at the extremes"])
def test_reuse_gives_the_bits_of_a_rebuild_at_every_layout(obe, layout):
    global LAYOUTS
    if LAYOUTS is None:
        LAYOUTS = _layouts()
    cloud, w2, d, fits = LAYOUTS[layout]
    assert fits
    n = cloud.shape[1]
    if w2 is None:
        w2 = weights(n, 601)
    x = np.linspace(1.5, 4.5, 257) if d == D else np.linspace(2.0, 10.5, 257)
    check_reuse_equals_rebuild(obe, x, cloud, weights(n, 602), w2, d, layout)


# ---------------------------------------------------------------------------------------------- whole cycles
TRUE = (3.0, -1000.0, 50000.0)


def new_experiment(obe, keep):
    g = np.random.default_rng(31)
    n, ns = 40000, 4200
    x = np.linspace(1.5, 4.5, ns)
    prior = np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    o = obe.OptBayesExpt(obe.models.lorentzian(1), (x,), prior, (D,), scale=False, utility_method="variance_full",
                         default_noise_std=100.0, auto_resample=True)
    o.tuning_parameters["sweep_bins"] = "always"
    o.tuning_parameters["sweep_shift"] = "never"
    o.tuning_parameters["sweep_bins_keep"] = keep
    o.tuning_parameters["speculative_sweep"] = True
    o.rng = np.random.default_rng(32)
    return o


def one_cycle(o, k):
    """Cycle k of the seeded experiment: (chosen index, kept, utility, resampled, a sweep was enqueued ahead)."""
    xs = o.opt_setting()
    assert o.last_sweep["bins"], (k, o.last_sweep)
    rec = (o.last_setting_index, o.last_sweep["kept"], o._utility_dev.cpu().numpy().copy())
    y = float(omodels.lorentzian(xs, TRUE, (D,))) + 100.0 * np.random.default_rng(1000 + k).standard_normal()
    o.pdf_update((xs, y, 100.0))
    return rec + (bool(o.just_resampled), o._sweeps.ticket is not None)


def final_state(o):
    return np.array(o.particles), np.array(o.particle_weights)


def same_records(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert ra[0] == rb[0] and ra[3] == rb[3]
        assert np.array_equal(ra[2], rb[2])


N_CYCLES, SET_PDF_AT, FORK_AT = 16, 9, 5


def replacement_cloud():
    g = np.random.default_rng(41)
    n = 40000
    return np.array([g.normal(3.0, 0.05, n), g.normal(-1000.0, 100.0, n), g.normal(50000, 300, n)])


def run(obe, keep, first=0, o=None, forks=None):
    o = new_experiment(obe, keep) if o is None else o
    records = []
    for k in range(first, N_CYCLES):
        if k == SET_PDF_AT:
            o.set_pdf(replacement_cloud())
        if forks is not None and k == FORK_AT:
            forks.append(o)
        records.append(one_cycle(o, k))
    o._drop_speculative_sweep()
    return records, final_state(o)


class Forks(list):
    """At the start of cycle FORK_AT (a sweep enqueued ahead may be in flight): a deep copy of the object, and a
    restore of its saved state (what ``save`` / ``load`` and ``pickle`` do: _state.py)."""

    def append(self, o):
        import pickle
        list.append(self, copy.deepcopy(o))
        list.append(self, pickle.loads(pickle.dumps(o)))


@pytest.fixture(scope="module")
def kept_run(obe):
    forks = Forks()
    records, state = run(obe, True, forks=forks)
    return records, state, forks


def test_cycles_reuse_until_the_particles_change(kept_run):
    records, _, _ = kept_run
    resampled = [r[3] for r in records]
    assert any(resampled) and not all(resampled), resampled
    assert any(r[4] for r in records)                         # sweeps were enqueued ahead by pdf_update()
    for k, r in enumerate(records):
        fresh_cloud = k == 0 or resampled[k - 1] or k == SET_PDF_AT
        assert r[1] is (not fresh_cloud), (k, [x[1] for x in records], resampled)


def test_cycles_are_those_of_an_object_without_the_keep(obe, kept_run):
    records, state, _ = kept_run
    plain, plain_state = run(obe, False)
    assert not any(r[1] for r in plain)
    same_records(records, plain)
    assert np.array_equal(state[0], plain_state[0]) and np.array_equal(state[1], plain_state[1])


@pytest.mark.parametrize("which", [0, 1], ids=["deepcopy", "restore"])
def test_a_copy_rebuilds_once_and_continues_with_the_same_bits(obe, kept_run, which):
    records, state, forks = kept_run
    o = forks[which]
    assert "_bins_keep" not in o.__dict__ and not o._bins_kept()
    tail, tail_state = run(obe, True, first=FORK_AT, o=o)
    assert tail[0][1] is False                                # the copy's first sweep rebuilds ...
    assert [r[1] for r in tail[1:]] == [r[1] for r in records[FORK_AT + 1:]]      # ... and then it goes as the original
    same_records(tail, records[FORK_AT:])
    assert np.array_equal(tail_state[0], state[0]) and np.array_equal(tail_state[1], state[1])


# ---------------------------------------------------------------------------------------------- the C entry point
def keep_buffer(o, n_draws=None):
    import torch
    nbytes = int(o._mlib.cdll.obe_sweep_bins_keep_bytes(o.n_particles if n_draws is None else n_draws))
    assert nbytes % 16 == 0 and nbytes >= 4 * (o.n_particles if n_draws is None else n_draws)
    return torch.zeros(nbytes // 4, dtype=torch.int32, device=o._device)


def c_keep(o, flags, keep, keep_bytes=None):
    """obe_sweep_utility_keep over all settings with the object's own cloud: (yvar, kappa, best index)."""
    import torch
    from optbayesexpt_amd import _lib
    from optbayesexpt_amd.particlepdf import _ptr, _P
    p, w = o._pw_tensors()
    mom = o._moments_on_device()
    ns = o._n_settings
    noise = torch.full((1,), 250000.0, dtype=torch.float64, device=w.device)
    yvar = torch.zeros((1, ns), dtype=torch.float64, device=w.device)
    util = torch.zeros(ns, dtype=torch.float64, device=w.device)
    out = _lib.pinned_array(4)
    best, idx, kappa = out[0:1], out.view(np.int64)[1:2], out[2:3]
    hp = _lib.host_ptr
    if keep_bytes is None:
        keep_bytes = 0 if keep is None else keep.numel() * 4
    rc = o._mlib.cdll.obe_sweep_utility_keep(o._model_struct, _P(o._settings_dev.data_ptr()), ns, ns, _ptr(p), p.shape[1],
                                             o.n_particles, _ptr(w), None, 0, _ptr(mom), flags, _ptr(noise), 0, None, 1.0,
                                             _ptr(yvar), _ptr(util), hp(best), hp(idx), hp(kappa), _ptr(o._ws),
                                             o._ws_bytes, o._stream(), None if keep is None else _ptr(keep), keep_bytes)
    torch.cuda.synchronize()
    assert rc == 0, o._mlib.last_error()
    return yvar.cpu().numpy()[0], float(kappa[0]), int(idx[0])


def refused(result):
    yvar, kappa, _ = result
    return np.isnan(kappa) and bool(np.all(np.isnan(yvar)))


def same_result(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and bool(np.all(np.isfinite(a[0])))


X = np.linspace(1.5, 4.5, 257)


def bins_flags():
    from optbayesexpt_amd import _lib
    return _lib.OBE_SWEEP_BINS, _lib.OBE_SWEEP_BINS | _lib.OBE_SWEEP_BINS_KEPT


def test_abi_a_buffer_that_was_never_filled_is_refused(obe):
    _, kept = bins_flags()
    o = make(obe, X, prior_cloud(4099, 21), weights(4099, 22))
    keep = keep_buffer(o)
    assert refused(c_keep(o, kept, keep))
    assert not bool(keep.any())                               # ... and nothing was written into it


def moved_cloud(cloud, within):
    """`cloud` with one particle (neither the leftmost nor the rightmost) moved to the middle of its own bin
    (`within`) or of the bin three further on."""
    tau = cloud[0] / D
    origin = tau.min()
    j = int(np.argsort(tau)[tau.size // 3])
    b = int(np.floor((tau[j] - origin) * 2.0))
    target = b if within else b + 3
    moved = cloud.copy()
    moved[0, j] = (origin + (target + 0.5) * 0.5) * D
    new = moved[0] / D
    assert moved[0, j] != cloud[0, j] and new.min() == origin and new.max() == tau.max()
    assert int(np.floor((new[j] - origin) * 2.0)) == target
    return moved


@pytest.mark.parametrize("within", [False, True], ids=["to another bin", "within its bin"])
def test_abi_a_moved_particle(obe, within):
    build, kept = bins_flags()
    cloud, w = prior_cloud(4099, 23), weights(4099, 24)
    a = make(obe, X, cloud, w)
    b = make(obe, X, moved_cloud(cloud, within), w)
    keep = keep_buffer(a)
    made = c_keep(a, build, keep)
    assert same_result(c_keep(a, kept, keep), made)           # (the cloud it was made for)
    reused = c_keep(b, kept, keep)
    if not within:
        assert refused(reused)
        return
    rebuilt = c_keep(b, build, keep_buffer(b))
    assert same_result(reused, rebuilt)
    assert not np.array_equal(rebuilt[0], made[0])


def test_abi_a_buffer_made_for_another_number_of_draws_is_refused(obe):
    build, kept = bins_flags()
    small = make(obe, X, prior_cloud(513, 25), weights(513, 26))
    large = make(obe, X, prior_cloud(4099, 27), weights(4099, 28))
    keep = keep_buffer(large)                                 # room for 4099 draws: the head refuses, not the size
    assert np.isfinite(c_keep(small, build, keep)[1])
    assert same_result(c_keep(small, kept, keep), c_keep(small, build, keep_buffer(small)))
    assert refused(c_keep(large, kept, keep))


def test_abi_a_buffer_that_is_too_small_is_ignored(obe):
    from test_gpu_bin_sweep import c_sweep
    build, kept = bins_flags()
    o = make(obe, X, prior_cloud(4099, 29), weights(4099, 30))
    keep = keep_buffer(o)
    got = c_keep(o, kept, keep, keep_bytes=keep.numel() * 4 - 16)
    rc, yvar, kappa, idx = c_sweep(o, build, 0, X.size)
    assert rc == 0 and same_result(got, (yvar, kappa, idx))
    assert not bool(keep.any())                               # nothing was rebuilt into it either


def test_abi_a_poisoned_cloud_stays_poisoned(obe):
    build, kept = bins_flags()
    cloud, _, d, fits = _layouts()["one bin more than OBE_BIN_MAX"]
    assert not fits
    o = make(obe, np.linspace(2.0, 10.5, 257), cloud, weights(cloud.shape[1], 33), d=d)
    keep = keep_buffer(o)
    assert refused(c_keep(o, build, keep))
    assert refused(c_keep(o, kept, keep))
