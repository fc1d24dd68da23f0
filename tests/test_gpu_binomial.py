"""Yes/no outcomes on the device (OptBayesExptBinomial; csrc/obe_binomial.hip) against tests/_binomial_oracle.py.

Inputs (tests/_binomial_oracle.py; checked without a device in tests/test_binomial_host.py): the one-channel cloud
(the one-peak Lorentzian as a probability curve, p in [0.10, 0.90], largest information 0.053 .. 0.074 nats), the same
cloud converged (sigma(x0) = 0.002: 3e-5 .. 5e-5 nats), and a two-channel Ramsey pair through a formula's plugin
(p in [0.019, 0.966], largest information 0.15 nats), all with non-uniform weights.  The oracle is fed the NumPy form
of the same curves: its p and the device's differ by a few ulp, which moves the information by ~1e-15.  These figures
are the oracle's for the weights used here, uniform draws under a bell over the first parameter: the bell narrows the
weighted cloud, so there is less to learn than from the same cloud under even weights.  The two floors the tolerance
leans on (below) hold, and the converged cloud's information still stands four orders above the tolerance.

Tolerances.  Likelihood: |dL| <= 1e-10 L; every particle of these inputs has oracle log L >= -600 (asserted), so
nothing is left out.  Information: |dU cost| <= 1e-9 C nats — each sum is of at most N non-negative terms in a fixed
order, relative error <= N eps = 2.9e-11 at 2^17 + 3, plus a few ulp of log; both entropy terms are <= C log 2 and
|dH / dPbar_o| = |log Pbar_o + 1| <= 5.6 while Pbar_o >= 0.01, asserted from the oracle alone before the device is
asked, together with a largest information >= 1e-5 (a cloud of ONE particle has information 0 by identity and is
compared with 0 at the same bound).  nu_bar: 1e-10 relative (N positive terms in a fixed order lose at most N eps).
Run to run, slice against whole grid, one output against both: the same bits."""
import copy
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _binomial_oracle as oracle

pytestmark = pytest.mark.gpu
GRID, TIMES = oracle.GRID, oracle.TIMES
INFO_TOL = 1e-9                  # nats per channel
SLICES = ((0, 64), (64, 130), (37, 101), (129, 130))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ the objects
def _lorentz_object(cloud, w=None, grid=GRID, **kw):
    import optbayesexpt_amd as obe
    kw.setdefault("scale", False)
    o = obe.OptBayesExptBinomial(obe.models.lorentzian(1), (grid,), cloud, (oracle.WIDTH,), **kw)
    if w is not None:
        o.particle_weights = w
    return o


def _ramsey_model(extra=()):
    import optbayesexpt_amd as obe
    return obe.models.from_expression(oracle.RAMSEY + tuple(extra), settings=("t",), parameters=("f", "T2"))


def _ramsey_object(cloud, w=None, extra=(), grid=TIMES, **kw):
    import optbayesexpt_amd as obe
    kw.setdefault("scale", False)
    o = obe.OptBayesExptBinomial(_ramsey_model(extra), (grid,), cloud, (), **kw)
    if w is not None:
        o.particle_weights = w
    return o


def _case(kind, n, probabilities=True):
    """(cloud, weights, P (n_settings, C, n)) of the inputs named in the module docstring."""
    seed, make, probs = {"wide": (300, oracle.lorentz_cloud, oracle.lorentz_probabilities),
                         "converged": (400, oracle.converged_cloud, oracle.lorentz_probabilities),
                         "ramsey": (500, oracle.ramsey_cloud, oracle.ramsey_probabilities)}[kind]
    g = np.random.default_rng(seed + n)
    cloud = make(g, n)
    return cloud, oracle.weights(g, cloud), probs(cloud) if probabilities else None


def _lean_on(P, w, floor=True):
    """What the information tolerance leans on, from the oracle alone; returns the oracle's (information, nu_bar)."""
    want = oracle.information(P, w)
    assert oracle.outcome_marginals(P, w).min() >= 0.01
    if floor:
        assert want.max() >= 1e-5
    return want, oracle.noise_variance(P, w)


def _entry(o, begin, end, info=True, nu=True, cost=None, cost_scalar=1.0, shots=1.0):
    """One call of obe_binomial_information on the settings [begin, end) of the object's grid, outputs pre-filled."""
    import torch
    from optbayesexpt_amd.particlepdf import _P, _ptr
    p, w = o._pw_tensors()
    n, n_p, dev = end - begin, p.shape[1], o._device
    d_info = torch.full((n,), -7.0, dtype=torch.float64, device=dev) if info else None
    d_nu = torch.full((o.n_channels, n), -7.0, dtype=torch.float64, device=dev) if nu else None
    d_cost = None if cost is None else torch.from_numpy(np.ascontiguousarray(cost, dtype=np.float64)).to(dev)
    nbytes = int(o._mlib.cdll.obe_binomial_workspace_bytes(n_p, n, o.n_channels))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    o._mlib.call("obe_binomial_information", o._model_struct, _P(o._settings_dev.data_ptr() + 8 * begin),
                 o._n_settings, n, _ptr(p), n_p, n_p, _ptr(w), float(shots), None if d_cost is None else _ptr(d_cost),
                 float(cost_scalar), None if d_info is None else _ptr(d_info), None if d_nu is None else _ptr(d_nu),
                 _ptr(ws), nbytes, o._stream())
    return (None if d_info is None else d_info.cpu().numpy()), (None if d_nu is None else d_nu.cpu().numpy())


def _close(what, got_info, got_nu, want_info, want_nu, n_c):
    assert got_info.shape == want_info.shape and got_nu.shape == want_nu.shape, what
    err = np.abs(got_info - want_info)
    assert np.all(err <= INFO_TOL * n_c), f"{what}: information off by {err.max():.3g} nats at {int(np.argmax(err))}"
    assert_allclose(got_nu, want_nu, rtol=1e-10, atol=0.0, err_msg=what)


# ------------------------------------------------------------------------------------------------ 1. likelihood
def _check_likelihood(what, o, setting, successes, shots, n_lik=None, choke=None):
    """Both forms of the kernel for one record against the oracle fed the product's own model values."""
    y = np.asarray(o.eval_over_all_parameters(setting)).reshape(o.n_channels, -1)
    n_lik = o.n_channels if n_lik is None else n_lik
    k, n = np.atleast_1d(successes).astype(float), np.atleast_1d(shots).astype(float)
    ll = oracle.log_likelihood(y, k, n, n_lik)
    assert ll.min() >= -600.0, (what, ll.min())                        # the oracle alone: nothing is left out
    want = oracle.likelihood(y, k, n, n_lik, choke)
    o.choke = choke
    record = (setting, k[:n_lik] if o.n_channels > 1 else k[0], n[:n_lik] if o.n_channels > 1 else n[0])
    from_model = o._likelihood_device(None, record).cpu().numpy()
    from_y = o._likelihood_device(y, record).cpu().numpy()
    assert from_model.shape == (y.shape[1],) and from_model.dtype == np.float64
    assert_array_equal(_bits(from_model), _bits(from_y), err_msg=f"{what}: model form vs d_y form")
    assert_array_equal(_bits(o.likelihood(y, record)), _bits(from_y), err_msg=f"{what}: likelihood()")
    err = np.abs(from_model - want)
    worst = int(np.argmax(err / want))
    assert np.all(err <= 1e-10 * want), f"{what}: particle {worst}: {from_model[worst]!r} vs {want[worst]!r}"
    return from_model


@pytest.mark.parametrize("n", [1, 65, 257, 4097, (1 << 17) + 3])
def test_likelihood_one_channel(hip, n):
    cloud, _, _ = _case("wide", n, probabilities=False)
    o = _lorentz_object(cloud)
    for x in (2.0, 3.0, 3.37):
        for shots in (1, 7, 64):
            for k in sorted({0, shots // 3, shots}):
                _check_likelihood(f"n={n} x={x} {k}/{shots}", o, (x,), k, shots)
    o.shots = 7                                                        # a record without n takes the object's shots
    y = np.asarray(o.eval_over_all_parameters((3.0,))).reshape(1, -1)
    assert_array_equal(_bits(o._likelihood_device(None, ((3.0,), 2)).cpu().numpy()),
                       _bits(o._likelihood_device(y, ((3.0,), 2, 7)).cpu().numpy()))


def test_likelihood_two_channels_and_choke(hip):
    cloud, _, _ = _case("ramsey", 4097)
    o = _ramsey_object(cloud)
    assert o._mlib is not o._lib                                       # the plugin serves the model's entry points
    for t in (0.05, 1.0, 3.0):
        for k, n in (((0, 64), (64, 64)), ((1, 0), (1, 1)), ((3, 5), (7, 7)), ((20, 64), (64, 64)), ((2, 0), (7, 1))):
            for n_lik in (1, 2):
                _check_likelihood(f"t={t} {k}/{n} n_lik={n_lik}", o, (t,), k, n, n_lik=n_lik)
    plain = _check_likelihood("choke: none", o, (1.0,), (3, 5), (7, 7))
    choked = _check_likelihood("choke 0.5", o, (1.0,), (3, 5), (7, 7), choke=0.5)
    assert_allclose(choked, np.sqrt(plain), rtol=1e-14)
    # a one-value record of a two-channel model enters with its first channel alone
    o.choke = None
    y = np.asarray(o.eval_over_all_parameters((1.0,)))
    assert_array_equal(_bits(o._likelihood_device(y, ((1.0,), 3, 7)).cpu().numpy()),
                       _bits(_check_likelihood("one value", o, (1.0,), (3, 0), (7, 1), n_lik=1)))


def test_likelihood_of_crafted_probabilities(hip):
    """Through the form that takes given model values: certain outcomes are exactly 1, impossible ones and particles
    whose p is no probability are exactly 0."""
    y = np.array([[0.0, 1.0, 0.5, -1e-9, 1.0 + 1e-9, np.nan, 0.25]])
    o = _lorentz_object(oracle.lorentz_cloud(np.random.default_rng(1), 7))
    none = o._likelihood_device(y, ((3.0,), 0, 3)).cpu().numpy()
    every = o._likelihood_device(y, ((3.0,), 3, 3)).cpu().numpy()
    some = o._likelihood_device(y, ((3.0,), 1, 3)).cpu().numpy()
    assert_array_equal(none[[0, 1, 3, 4, 5]], [1.0, 0.0, 0.0, 0.0, 0.0])
    assert_array_equal(every[[0, 1, 3, 4, 5]], [0.0, 1.0, 0.0, 0.0, 0.0])
    assert_array_equal(some[[0, 1, 3, 4, 5]], [0.0] * 5)
    assert_allclose(none[[2, 6]], [0.125, 0.75 ** 3], rtol=1e-15)
    assert_allclose(every[[2, 6]], [0.125, 0.25 ** 3], rtol=1e-15)
    assert_allclose(some[[2, 6]], [0.125, 0.25 * 0.75 ** 2], rtol=1e-15)
    for k in (0, 1, 3):
        assert_allclose(o.likelihood(y, ((3.0,), k, 3)), oracle.likelihood(y, [k], [3], 1), rtol=1e-15)


# ------------------------------------------------------------------------------------------------ 2. information
def _check_information(what, o, P, w, n_c, floor=True):
    want_info, want_nu = _lean_on(P, w, floor)
    n_s = P.shape[0]
    info, nu = _entry(o, 0, n_s)
    _close(what, info, nu, want_info, want_nu, n_c)
    again = _entry(o, 0, n_s)
    assert_array_equal(_bits(again[0]), _bits(info), err_msg=f"{what}: run to run")
    assert_array_equal(_bits(again[1]), _bits(nu), err_msg=f"{what}: run to run")
    for k in [k for k in oracle.N_SETTINGS if k <= n_s]:
        got = _entry(o, 0, k)
        _close(f"{what} n_settings={k}", got[0], got[1], want_info[:k], want_nu[:, :k], n_c)
    # a slice of the grid, as a settings shard asks for it: the whole grid's columns, bit for bit
    for b, e in [(b, min(e, n_s)) for b, e in SLICES if b < n_s]:
        got = _entry(o, b, e)
        assert_array_equal(_bits(got[0]), _bits(info[b:e]), err_msg=f"{what}: slice {b}:{e}")
        assert_array_equal(_bits(got[1]), _bits(nu[:, b:e]), err_msg=f"{what}: slice {b}:{e}")
    # either output alone
    only_info, none = _entry(o, 0, n_s, nu=False)
    assert none is None
    assert_array_equal(_bits(only_info), _bits(info), err_msg=f"{what}: d_noise_var = NULL")
    none, only_nu = _entry(o, 0, n_s, info=False)
    assert none is None
    assert_array_equal(_bits(only_nu), _bits(nu), err_msg=f"{what}: d_information = NULL")
    # the cost divides the information, the shots the variance: IEEE divisions of the same numerators
    cost = 0.5 + np.arange(n_s) % 7
    by_array, nu4 = _entry(o, 0, n_s, cost=cost, cost_scalar=99.0, shots=4.0)
    assert_array_equal(_bits(by_array), _bits(info / cost), err_msg=f"{what}: d_cost")
    assert_array_equal(_bits(nu4), _bits(nu / 4.0), err_msg=f"{what}: shots")
    by_scalar, _ = _entry(o, 0, n_s, cost_scalar=3.0)
    assert_array_equal(_bits(by_scalar), _bits(info / 3.0), err_msg=f"{what}: cost")
    return info, nu


@pytest.mark.parametrize("n", oracle.N_PARTICLES)
def test_information_one_channel(hip, n):
    """One chunk (300 x 130), a chunk boundary, a ragged last chunk, many chunks (2^17 + 3 x 1); both sides of the
    wave of 64 settings; the wide cloud and the converged one."""
    for kind in ("wide", "converged"):
        cloud, w, P = _case(kind, n)
        o = _lorentz_object(cloud, w)
        _check_information(f"{kind} n={n}", o, P, w, 1, floor=n > 1)
        assert_array_equal(_bits(o.yvar_noise_model()), _bits(_entry(o, 0, GRID.size)[1]))


@pytest.mark.parametrize("n", [300, 4097])
def test_information_two_channels(hip, n):
    cloud, w, P = _case("ramsey", n)
    o = _ramsey_object(cloud, w)
    info, _ = _check_information(f"ramsey n={n}", o, P, w, 2)
    assert info.max() > 0.1


def test_information_three_channels(hip):
    """The widest model the class takes: 8 outcome sums per lane."""
    extra, grid = ("0.3 + 0.4*exp(-t/T2)",), np.linspace(0.4, 2.6, 23)
    cloud, w, _ = _case("ramsey", 257)
    two = oracle.ramsey_probabilities(cloud, grid)
    P = np.concatenate([two, (0.3 + 0.4 * np.exp(-grid.reshape(-1, 1) / cloud[1]))[:, None, :]], axis=1)
    assert P.shape == (23, 3, 257)
    o = _ramsey_object(cloud, w, extra=extra, grid=grid)
    want_info, want_nu = _lean_on(P, w)
    info, nu = _entry(o, 0, 23)
    _close("three channels", info, nu, want_info, want_nu, 3)
    assert_array_equal(_bits(_entry(o, 5, 20)[0]), _bits(info[5:20]))
    assert_array_equal(_bits(o.utility()), _bits(info))


# ------------------------------------------------------------------------------------------------ 3. exclusion
def test_particles_without_weight_do_not_count_whatever_they_are(hip):
    n = 4097
    cloud, w, _ = _case("wide", n)
    g = np.random.default_rng(9)
    idx = g.permutation(n)[:n // 10]
    kinds = np.arange(idx.size) % 3
    w = w.copy()
    w[idx[kinds == 0]] = 0.0
    w[idx[kinds == 1]] = np.nan
    w[idx[kinds == 2]] = -w[idx[kinds == 2]] - 1e-9
    broken = cloud.copy()
    broken[:, idx] = np.nan
    want_info, want_nu = _lean_on(oracle.lorentz_probabilities(cloud), w)
    first = _entry(_lorentz_object(broken, w), 0, GRID.size)
    second = _entry(_lorentz_object(cloud, w), 0, GRID.size)           # the same particles with valid parameters
    assert_array_equal(_bits(first[0]), _bits(second[0]))
    assert_array_equal(_bits(first[1]), _bits(second[1]))
    _close("dirty weights", first[0], first[1], want_info, want_nu, 1)


def test_a_particle_whose_p_is_no_probability_drops_out(hip):
    n = 300
    cloud, w, _ = _case("wide", n)
    out = [3, 64, 299]
    # everywhere: b = 1.5 puts p above 1 at every setting — the oracle on the cloud without these particles
    bad = cloud.copy()
    bad[2, out] = 1.5
    keep = np.setdiff1d(np.arange(n), out)
    want_info, want_nu = _lean_on(oracle.lorentz_probabilities(cloud[:, keep]), w[keep])
    info, nu = _entry(_lorentz_object(bad, w), 0, GRID.size)
    _close("p > 1 everywhere", info, nu, want_info, want_nu, 1)
    # at some settings only: a = 5 leaves p <= 1 far from the line — there the particle still counts
    bad = cloud.copy()
    bad[1, out] = 5.0
    P = oracle.lorentz_probabilities(bad)
    counted = oracle.contributing(P, w)[:, out]
    assert counted.any() and not counted.all()
    want_info, want_nu = _lean_on(P, w)
    info, nu = _entry(_lorentz_object(bad, w), 0, GRID.size)
    _close("p > 1 near the line", info, nu, want_info, want_nu, 1)
    # below 0 and NaN
    bad = cloud.copy()
    bad[2, out[0]], bad[1, out[1]], bad[0, out[2]] = -0.9, np.nan, np.nan
    want_info, want_nu = _lean_on(oracle.lorentz_probabilities(cloud[:, keep]), w[keep])
    info, nu = _entry(_lorentz_object(bad, w), 0, GRID.size)
    _close("p < 0 or NaN", info, nu, want_info, want_nu, 1)


def test_a_cloud_without_any_contributing_particle_gives_nan(hip):
    cloud, w, _ = _case("wide", 300)
    for weights in (np.zeros(300), np.full(300, np.nan), -np.ones(300)):
        info, nu = _entry(_lorentz_object(cloud, weights), 0, GRID.size)
        assert np.all(np.isnan(info)) and np.all(np.isnan(nu))
    bad = cloud.copy()
    bad[2] = 1.5
    o = _lorentz_object(bad, w)
    info, nu = _entry(o, 0, GRID.size)
    assert np.all(np.isnan(info)) and np.all(np.isnan(nu))
    assert np.all(np.isnan(o.utility())) and np.all(np.isnan(o.yvar_noise_model()))


# ------------------------------------------------------------------------------------------------ 4. the class
def test_utility_and_the_choice(hip):
    cloud, w, P = _case("wide", 4097)
    o = _lorentz_object(cloud, w)
    assert o.utility_method == "mutual_information" and o._noise_token() is None
    want, _ = _lean_on(P, w)
    info, _ = _entry(o, 0, GRID.size)
    u = o.utility()
    assert u.shape == (GRID.size,)
    assert_array_equal(_bits(u), _bits(info))
    assert_array_equal(_bits(o.utility_information()), _bits(info))
    x = o.opt_setting()
    assert x == (GRID[o.last_setting_index],)
    assert want[o.last_setting_index] >= want.max() - INFO_TOL          # (the surface has near-ties: no index compared)
    o.rng = np.random.default_rng(3)
    good = o.good_setting()
    assert len(good) == 1 and good[0] in GRID and good == (GRID[o.last_setting_index],)
    # a cost_estimate() override divides the information
    cost = 1.0 + np.arange(GRID.size) % 5
    o.cost_estimate = lambda: cost
    assert_array_equal(_bits(o.utility()), _bits(info / cost))
    assert_array_equal(_bits(o.utility()), _bits(_entry(o, 0, GRID.size, cost=cost)[0]))
    o.cost_estimate = lambda: 2.0
    assert_array_equal(_bits(o.utility()), _bits(info / 2.0))
    o.opt_setting()
    assert (want / 2.0)[o.last_setting_index] >= want.max() / 2.0 - INFO_TOL


def test_shots_divide_the_noise_variance_and_leave_the_information(hip):
    cloud, w, P = _case("wide", 300)
    o = _lorentz_object(cloud, w)
    info, nu = o.utility(), o.yvar_noise_model()
    assert nu.shape == (1, GRID.size)
    assert_allclose(nu, oracle.noise_variance(P, w), rtol=1e-10, atol=0.0)
    o.shots = 4
    assert_array_equal(_bits(o.yvar_noise_model()), _bits(nu / 4.0))
    assert_array_equal(_bits(o.utility()), _bits(info))
    t, ld = o._noise_var_device()
    assert ld == t.shape[1] == GRID.size
    assert_array_equal(_bits(t.cpu().numpy()), _bits(nu / 4.0))
    for bad in (0, 2.5, [1, 2], np.nan):
        o.shots = bad                                                  # checked where it is used
        with pytest.raises(ValueError):
            o.yvar_noise_model()
        with pytest.raises(ValueError):
            o.pdf_update(((3.0,), 0))
    # shots per channel
    cloud, w, P = _case("ramsey", 300)
    o = _ramsey_object(cloud, w, shots=[1, 5])
    assert_allclose(o.yvar_noise_model(), oracle.noise_variance(P, w, [1.0, 5.0]), rtol=1e-10, atol=0.0)


def test_variance_utilities_use_the_binomial_noise_variance(hip):
    """utility_method="variance_approx": the Gaussian approximation, with nu_bar for the noise — the utility of a plain
    OptBayesExpt whose yvar_noise_model() returns that same array."""
    import optbayesexpt_amd as obe
    cloud, w, P = _case("wide", 4097)
    o = _lorentz_object(cloud, w, utility_method="variance_approx", n_draws=40, shots=8)
    assert o.utility_method == "variance_approx"
    nubar = o.yvar_noise_model()
    assert_allclose(nubar, oracle.noise_variance(P, w, 8.0), rtol=1e-10, atol=0.0)
    plain = obe.OptBayesExpt(obe.models.lorentzian(1), (GRID,), cloud, (oracle.WIDTH,), scale=False,
                             utility_method="variance_approx", n_draws=40)
    plain.particle_weights = w
    plain.yvar_noise_model = lambda: nubar
    o.rng, plain.rng = np.random.default_rng(5), np.random.default_rng(5)
    u = o.utility()
    assert u.shape == (GRID.size,) and np.all(np.isfinite(u)) and np.ptp(u) > 0
    assert_allclose(u, plain.utility(), rtol=1e-10, atol=0.0)
    o.rng, plain.rng = np.random.default_rng(6), np.random.default_rng(6)
    assert o.opt_setting() == plain.opt_setting()
    # the information is there whatever the method
    assert_array_equal(_bits(o.utility_information()), _bits(_entry(o, 0, GRID.size)[0]))


def test_update_multiplies_the_weights_by_the_likelihood(hip):
    cloud, w, _ = _case("wide", 4097)
    o = _lorentz_object(cloud, w, auto_resample=False)
    y = np.asarray(o.eval_over_all_parameters((3.1,))).reshape(1, -1)
    for record, k, n in ((((3.1,), 1), 1, 1), (((3.1,), 3, 7), 3, 7), (((3.1,), 0, 64), 0, 64)):
        o.particle_weights = w
        o.pdf_update(record)
        want = oracle.normalised(w * oracle.likelihood(y, [k], [n], 1))
        assert_allclose(o.particle_weights, want, rtol=1e-10, atol=0.0)
    o.particle_weights = w
    o.pdf_update(((3.1,), 3, 7), y)                                    # ... and from given model values
    assert_allclose(o.particle_weights, oracle.normalised(w * oracle.likelihood(y, [3], [7], 1)), rtol=1e-10, atol=0.0)

    class Mine(type(o)):
        def likelihood(self, y_model, record):                         # a user's likelihood is honoured
            return np.full(self.n_particles, 0.5) * (np.arange(self.n_particles) % 2)

    mine = Mine(o.model_function, (GRID,), cloud, (oracle.WIDTH,), scale=False, auto_resample=False)
    mine.pdf_update(((3.1,), 1))
    assert np.all(mine.particle_weights[::2] == 0.0) and np.all(mine.particle_weights[1::2] > 0.0)


# ------------------------------------------------------------------------------------------------ 5. a run
TRUTH = (3.1, 0.45, 0.2)
RUN_SEED, RUN_CYCLES = 41, 150


def _outcome(draw, x):
    p = TRUTH[2] + TRUTH[1] / (((x[0] - TRUTH[0]) / oracle.WIDTH) ** 2 + 1.0)
    return int(draw.random() < p)


def test_single_shot_run_finds_the_line(hip):
    """150 cycles opt_setting() -> one shot -> pdf_update((x, k)) at 2000 particles and 130 settings.  Seed and cycle
    count from the same loop on the oracle (information() for the design, likelihood() for the update, a Liu-West
    resample below N_eff = N / 2) on the CPU: seed 41 gave sigma(x0) 0.229 -> 0.0215 after 150 cycles (0.0126 after
    300) with x0 0.39 sigma from the truth; seeds 42 and 43 gave 0.0198 and 0.0302, within 0.7 sigma."""
    g = np.random.default_rng(RUN_SEED)
    cloud = oracle.lorentz_cloud(g, 2000)
    o = _lorentz_object(cloud)
    o.rng = np.random.default_rng(RUN_SEED + 2)
    draw = np.random.default_rng(RUN_SEED + 1)
    prior_std = o.std()[0]
    chosen = set()
    for _ in range(RUN_CYCLES):
        x = o.opt_setting()
        chosen.add(x[0])
        o.pdf_update((x, _outcome(draw, x)))
    mean, std = o.mean(), o.std()
    assert np.all(np.isfinite(mean)) and np.all(std > 0) and len(chosen) > 1
    assert np.all(np.abs(mean - np.array(TRUTH)) < 3.0 * std), (mean, std)
    assert std[0] < prior_std / 3.0, (std[0], prior_std)


# ------------------------------------------------------------------------------------------------ 6. state
def test_save_load_copy_and_pickle_continue_alike(hip, tmp_path):
    import optbayesexpt_amd as obe
    g = np.random.default_rng(31)
    o = _lorentz_object(oracle.lorentz_cloud(g, 2000), shots=3)
    o.rng = np.random.default_rng(32)
    draw = np.random.default_rng(33)
    for _ in range(12):
        x = o.opt_setting()
        o.pdf_update((x, _outcome(draw, x) + _outcome(draw, x) + _outcome(draw, x)))
    path = os.path.join(tmp_path, "binomial.state")
    obe.save(o, path)
    twins = [obe.load(path), copy.deepcopy(o), pickle.loads(pickle.dumps(o))]
    outcomes = [int(draw.integers(0, 4)) for _ in range(3)]
    trail = []
    for k in outcomes:
        x = o.opt_setting()
        o.pdf_update((x, k))
        trail.append((x, o.particle_weights.copy(), o.particles.copy()))
    for t in twins:
        assert type(t) is obe.OptBayesExptBinomial
        assert t.utility_method == "mutual_information" and np.all(np.asarray(t.shots) == 3)
        assert getattr(t.utility, "__func__", None) is obe.OptBayesExptBinomial.utility_information
        for k, (x, weights, particles) in zip(outcomes, trail):
            assert t.opt_setting() == x
            t.pdf_update((x, k))
            assert_array_equal(_bits(t.particle_weights), _bits(weights))
            assert_array_equal(_bits(t.particles), _bits(particles))
        assert_array_equal(_bits(t.yvar_noise_model()), _bits(o.yvar_noise_model()))
    # a variance method travels too, and a saved file of another class loads as before
    v = _lorentz_object(oracle.lorentz_cloud(g, 64), utility_method="variance_full", shots=[2])
    obe.save(v, path)
    back = obe.load(path)
    assert type(back) is obe.OptBayesExptBinomial and back.utility_method == "variance_full"
    assert np.all(np.asarray(back.shots) == 2)
    plain = obe.OptBayesExpt(obe.models.lorentzian(1), (GRID,), oracle.lorentz_cloud(g, 64), (oracle.WIDTH,))
    obe.save(plain, path)
    assert type(obe.load(path)) is obe.OptBayesExpt


def _averaged(base):
    """A user's subclass of another class that keeps a public ``shots`` of its own (readings averaged per update)."""
    return type(f"Averaged{base.__name__}", (base,), {"__module__": __name__, "__qualname__": f"Averaged{base.__name__}"})


def test_shots_of_another_class_is_the_users_and_travels(hip, tmp_path):
    """``shots`` is the library's attribute on an OptBayesExptBinomial only: on the other classes it goes through save /
    load, pickle and deepcopy with the user's other attributes."""
    import optbayesexpt_amd as obe
    g = np.random.default_rng(41)
    model, cloud = obe.models.lorentzian(1), oracle.lorentz_cloud(g, 64)
    made = []
    for base, kw in ((obe.OptBayesExpt, {}), (obe.OptBayesExptSignalNoise, dict(noise_gain=0.01))):
        cls = _averaged(base)
        globals()[cls.__name__] = cls                                  # (where pickle and load look a class up)
        made.append(cls(model, (GRID,), cloud, (oracle.WIDTH,), **kw))
    made.append(obe.ParticlePDF(cloud))
    path = os.path.join(tmp_path, "averaged.state")
    for o in made:
        o.shots, o.my_note = 1000, "kept"
        obe.save(o, path)
        for t in (obe.load(path), copy.deepcopy(o), pickle.loads(pickle.dumps(o))):
            assert type(t) is type(o) and t.shots == 1000 and t.my_note == "kept", type(o).__name__


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_and_construction_checks(hip):
    import optbayesexpt_amd as obe
    cloud, w, _ = _case("wide", 300)
    o = _lorentz_object(cloud, w)
    x, y = np.array([3.0, 3.1]), np.array([1.0, 0.0])
    for call in (lambda: o.predictive_logpdf((x,), y, 0.5), lambda: o.predictive_cdf((x,), y, 0.5),
                 lambda: o.predictive_pvalue((x,), y, 0.5), lambda: o.reading_quantile(0.5, (x,), 0.5),
                 lambda: o.reading_interval(0.9, (x,), 0.5), lambda: o.records_loglik((x,), y, 0.5),
                 lambda: o.pdf_update_batch((x,), y, 0.5), lambda: o.predictive_logpdf((x,), y),
                 lambda: o.reading_quantile(0.5)):
        with pytest.raises(NotImplementedError, match="counts"):
            call()
    for call in (lambda: o.expected_variance_reduction(sigma=0.5), lambda: o.opt_setting_batch(2, sigma=0.5)):
        with pytest.raises(ValueError, match="counts"):
            call()
    # what has no reading in it works unchanged, and so do the designs that take the object's own noise
    mean, std = o.predict((x,))
    lo, hi = o.predictive_interval(0.9, (x,))
    assert mean.shape == std.shape == lo.shape == hi.shape == (1, 2) and np.all(lo <= hi)
    assert o.mean().shape == (3,) and o.covariance().shape == (3, 3)
    assert o.expected_variance_reduction().shape == (3, GRID.size)
    assert len(o.opt_setting_batch(3)[0]) == 3
    # bad counts: the weights stay as they were
    before = o.particle_weights.copy()
    for record in (((3.0,), 0.5), ((3.0,), 2), ((3.0,), -1), ((3.0,), 1, 0), ((3.0,), 3, 2), ((3.0,), 1, 1.5),
                   ((3.0,), np.nan), ((3.0,), 1, np.inf)):
        with pytest.raises(ValueError):
            o.pdf_update(record)
    assert_array_equal(_bits(o.particle_weights), _bits(before))
    # construction
    model = obe.models.lorentzian(1)
    with pytest.raises(ValueError, match="DeviceModel"):
        obe.OptBayesExptBinomial(lambda s, p, c: p[0], (GRID,), cloud, (oracle.WIDTH,))
    for shots in (0, -2, 1.5, [1, 2], np.nan):
        with pytest.raises(ValueError, match="shots"):
            obe.OptBayesExptBinomial(model, (GRID,), cloud, (oracle.WIDTH,), shots=shots)
    with pytest.raises(SyntaxError):
        obe.OptBayesExptBinomial(model, (GRID,), cloud, (oracle.WIDTH,), utility_method="nonsense")
    four = obe.models.DeviceModel.__new__(obe.models.DeviceModel)      # (a model of four channels, never built)
    four.n_channels = 4
    with pytest.raises(ValueError, match="OBE_BINOMIAL_MAX_CHANNELS"):
        obe.OptBayesExptBinomial(four, (GRID,), np.full((2, 8), 0.5), ())


# ------------------------------------------------------------------------------------------------ 8. the example
def test_binary_outcomes_example(hip):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    done = subprocess.run([sys.executable, os.path.join(root, "examples", "binary_outcomes.py"), "60", "2000"],
                          capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr[-2000:]
    assert "60 single shots" in done.stdout and "x0 =" in done.stdout
