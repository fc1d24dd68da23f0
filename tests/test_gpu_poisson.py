"""Counted events on the device (OptBayesExptPoisson; csrc/obe_poisson.hip) against tests/_poisson_oracle.py.

Inputs (tests/_poisson_oracle.py; checked without a device in tests/test_poisson_host.py): the one-peak Lorentzian as a
count rate between 2 and 12 per unit exposure, wide (largest information 0.26 nats at exposure 1) and converged
(sigma(x0) = 0.002: 2e-4 nats), and a two-channel formula (a decay and its complement) through its plugin for the
likelihood and variance paths, all with the binomial tests' non-uniform weights.  The oracle is fed the NumPy form of the
same curves: its rates and the device's differ by a few ulp, which moves every figure below by ~1e-15 relative.

Tolerances.
Likelihood: |dL| <= 1e-10 L.  Records have k <= 1000 and exposure x rate <= ~1e3, so every term of the exponent is
<= 7e3 and a few ulp of log move it by ~1e-12; the oracle's log L >= -600 is asserted first, so no particle is left out.
Information: |dU cost| <= 1e-9 nats.  Each sum has at most N non-negative terms in a fixed order: relative error
<= N eps = 2.9e-11 at 2^17 + 3; a relative error d in the Pbar moves -sum Pbar log Pbar by at most d (H + 1) with
H <= log 65, and hbar <= H carries the same d: 2.7e-10 in all.  The oracle's largest information >= 1e-5 is asserted
before the device is asked; a one-particle cloud is compared with 0 at the same bound.
d_tail: 1e-10 absolute.  d_pmf: the rows Pbar_k, k < cap, 1e-10 relative where the oracle's value is >= 1e-280 and
<= 1e-280 elsewhere.  The last row of d_pmf is taubar, the very number d_tail holds (asserted bit for bit), and is held
to d_tail's bound: tau_i = 1 - sum_k p_k,i is a difference of numbers near 1, known to cap eps = 1.4e-14 absolute in the
oracle as in the kernel (the oracle in float64 and in extended precision differ by that much), so where taubar is 1e-9
no relative 1e-10 can be asked of either; where the oracle's taubar >= 1e-3 that absolute error IS below 1e-10 relative,
and there the relative bound is asserted as well.
nu_bar: 1e-10 relative (N positive terms in a fixed order lose at most N eps).
Run to run, slice against whole grid, any subset of the outputs against all of them: the same bits.

At 2^17 + 3 particles the oracle is asked for eight columns of the grid (both sides of every tile edge), the device for
all 130; every other size is compared column for column."""
import copy
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _poisson_oracle as oracle

pytestmark = pytest.mark.gpu
GRID, TIMES = oracle.GRID, oracle.TIMES
INFO_TOL = 1e-9                  # nats
TAIL_TOL = 1e-10                 # absolute
SLICES = oracle.SLICES
BIG = (1 << 17) + 3
BIG_COLUMNS = np.array([0, 37, 63, 64, 65, 127, 128, 129])
OUTPUTS = ("info", "tail", "pmf", "nu")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ the objects
def _lorentz_object(cloud, w=None, grid=GRID, **kw):
    import optbayesexpt_amd as obe
    kw.setdefault("scale", False)
    o = obe.OptBayesExptPoisson(obe.models.lorentzian(1), (grid,), cloud, (oracle.WIDTH,), **kw)
    if w is not None:
        o.particle_weights = w
    return o


def _decay_object(cloud, w=None, grid=TIMES, **kw):
    import optbayesexpt_amd as obe
    kw.setdefault("scale", False)
    kw.setdefault("utility_method", "variance_approx")
    model = obe.models.from_expression(oracle.DECAYS, settings=("t",), parameters=("a", "b", "T1"))
    o = obe.OptBayesExptPoisson(model, (grid,), cloud, (), **kw)
    if w is not None:
        o.particle_weights = w
    return o


_CASES = {}


def _case(kind, n):
    """(cloud, weights, R (n_settings, n)) of the inputs named in the module docstring; made once per session."""
    if (kind, n) not in _CASES:
        seed, make = {"wide": (300, oracle.lorentz_cloud), "converged": (400, oracle.converged_cloud)}[kind]
        g = np.random.default_rng(seed + n)
        cloud = make(g, n)
        _CASES[kind, n] = (cloud, oracle.weights(g, cloud), oracle.lorentz_rates(cloud))
    return _CASES[kind, n]


_WANT = {}


def _want(kind, n, exposure, cap):
    """The oracle's (information, distribution (n_cols, cap + 1), nu_bar (1, n_cols), columns) for a case; computed once
    and shared."""
    key = (kind, n, exposure, cap)
    if key not in _WANT:
        _, w, R = _case(kind, n)
        cols = BIG_COLUMNS if n >= BIG else np.arange(GRID.size)
        info, pmf = oracle.design(R[cols], w, exposure, cap)
        _WANT[key] = (info, pmf, oracle.noise_variance(R[cols], w, exposure), cols)
    return _WANT[key]


def _entry(o, begin, end, cap=32, exposure=1.0, outputs=OUTPUTS, cost=None, cost_scalar=1.0):
    """One call of obe_poisson_information on the settings [begin, end) of the object's grid, outputs pre-filled;
    a dict of the outputs asked for (pmf transposed to (n, cap + 1), as count_distribution() gives it)."""
    import torch
    from optbayesexpt_amd.particlepdf import _P, _ptr
    p, w = o._pw_tensors()
    n, n_p, dev = end - begin, p.shape[1], o._device
    shapes = {"info": (n,), "tail": (n,), "pmf": (cap + 1, n), "nu": (o.n_channels, n)}
    out = {k: torch.full(shapes[k], -7.0, dtype=torch.float64, device=dev) for k in outputs}
    d_cost = None if cost is None else torch.from_numpy(np.ascontiguousarray(cost, dtype=np.float64)).to(dev)
    nbytes = int(o._mlib.cdll.obe_poisson_workspace_bytes(n_p, n, o.n_channels, cap))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    o._mlib.call("obe_poisson_information", o._model_struct, _P(o._settings_dev.data_ptr() + 8 * begin),
                 o._n_settings, n, _ptr(p), n_p, n_p, _ptr(w), float(exposure), cap,
                 None if d_cost is None else _ptr(d_cost), float(cost_scalar),
                 *[_ptr(out[k]) if k in out else None for k in OUTPUTS], _ptr(ws), nbytes, o._stream())
    got = {k: v.cpu().numpy() for k, v in out.items()}
    if "pmf" in got:
        got["pmf"] = np.ascontiguousarray(got["pmf"].T)
    return got


def _close(what, got, want_info, want_pmf, want_nu, cost=1.0):
    """The tolerances of the module docstring, for whichever outputs ``got`` holds."""
    cap = want_pmf.shape[1] - 1
    if "info" in got:
        err = np.abs(got["info"] * cost - want_info)
        assert got["info"].shape == want_info.shape, what
        assert np.all(err <= INFO_TOL), f"{what}: information off by {err.max():.3g} nats at {int(np.argmax(err))}"
    if "tail" in got:
        err = np.abs(got["tail"] - want_pmf[:, cap])
        assert np.all(err <= TAIL_TOL), f"{what}: tail off by {err.max():.3g}"
        sure = want_pmf[:, cap] >= 1e-3
        assert_allclose(got["tail"][sure], want_pmf[sure, cap], rtol=1e-10, atol=0.0, err_msg=what)
    if "pmf" in got:
        assert got["pmf"].shape == want_pmf.shape, what
        rows, ref = got["pmf"][:, :cap], want_pmf[:, :cap]
        big = ref >= 1e-280
        assert np.all(np.abs(rows[big] - ref[big]) <= 1e-10 * ref[big]), \
            f"{what}: distribution off by {np.max(np.abs(rows[big] - ref[big]) / ref[big]):.3g} relative"
        assert np.all(rows[~big] <= 1e-280), what
        assert np.all(np.abs(got["pmf"][:, cap] - want_pmf[:, cap]) <= TAIL_TOL), what
        if "tail" in got:
            assert_array_equal(_bits(got["pmf"][:, cap]), _bits(got["tail"]), err_msg=f"{what}: pmf's last row is tail")
    if "nu" in got:
        assert_allclose(got["nu"], want_nu, rtol=1e-10, atol=0.0, err_msg=what)


def _same(what, a, b, columns=slice(None)):
    for k in a:
        full = b[k][..., columns] if k in ("nu",) else b[k][columns]
        assert_array_equal(_bits(a[k]), _bits(full), err_msg=f"{what}: {k}")


# ------------------------------------------------------------------------------------------------ 1. likelihood
def _check_likelihood(what, o, setting, counts, exposure, n_lik=None, choke=None):
    """Both forms of the kernel for one record against the oracle fed the product's own model values."""
    y = np.asarray(o.eval_over_all_parameters(setting)).reshape(o.n_channels, -1)
    n_lik = o.n_channels if n_lik is None else n_lik
    k, t = np.atleast_1d(counts).astype(float), np.atleast_1d(exposure).astype(float)
    ll = oracle.log_likelihood(y, k, t, n_lik)
    assert ll.min() >= -600.0, (what, ll.min())                        # the oracle alone: nothing is left out
    want = oracle.likelihood(y, k, t, n_lik, choke)
    o.choke = choke
    one = o.n_channels == 1
    record = (setting, k[0] if one else k[:n_lik], t[0] if one or t.size == 1 else t[:n_lik])
    from_model = o._likelihood_device(None, record).cpu().numpy()
    from_y = o._likelihood_device(y, record).cpu().numpy()
    assert from_model.shape == (y.shape[1],) and from_model.dtype == np.float64
    assert_array_equal(_bits(from_model), _bits(from_y), err_msg=f"{what}: model form vs d_y form")
    assert_array_equal(_bits(o.likelihood(y, record)), _bits(from_y), err_msg=f"{what}: likelihood()")
    err = np.abs(from_model - want)
    worst = int(np.argmax(err / want))
    assert np.all(err <= 1e-10 * want), f"{what}: particle {worst}: {from_model[worst]!r} vs {want[worst]!r}"
    return from_model


@pytest.mark.parametrize("n", [1, 65, 257, 4097, BIG])
def test_likelihood_one_channel(hip, n):
    cloud, _, _ = _case("wide", n)
    o = _lorentz_object(cloud)
    for x in (2.0, 3.0, 3.37):
        for k, t in ((0, 1.0), (3, 1.0), (12, 1.0), (5, 0.5), (40, 4.0)):
            _check_likelihood(f"n={n} x={x} k={k} t={t}", o, (x,), k, t)
    _check_likelihood(f"n={n} a thousand counts", o, (2.0,), 1000, 300.0)          # (rates 2 .. 4 there)
    o.exposure = 0.5                                                   # a record without t takes the object's exposure
    y = np.asarray(o.eval_over_all_parameters((3.0,))).reshape(1, -1)
    assert_array_equal(_bits(o._likelihood_device(None, ((3.0,), 2)).cpu().numpy()),
                       _bits(o._likelihood_device(y, ((3.0,), 2, 0.5)).cpu().numpy()))


def test_likelihood_two_channels_and_choke(hip):
    g = np.random.default_rng(504)
    cloud = oracle.decay_cloud(g, 4097)
    o = _decay_object(cloud)
    assert o._mlib is not o._lib                                       # the plugin serves the model's entry points
    for t in (0.05, 1.0, 3.0):
        for k, e in (((0, 9), (1.0, 1.0)), ((7, 0), (1.0, 1.0)), ((3, 5), 2.0), ((20, 64), (4.0, 9.5)), ((2, 0), (0.25, 7.0))):
            for n_lik in (1, 2):
                _check_likelihood(f"t={t} {k}/{e} n_lik={n_lik}", o, (t,), k, e, n_lik=n_lik)
    plain = _check_likelihood("choke: none", o, (1.0,), (3, 5), (1.0, 2.0))
    choked = _check_likelihood("choke 0.5", o, (1.0,), (3, 5), (1.0, 2.0), choke=0.5)
    assert_allclose(choked, np.sqrt(plain), rtol=1e-14)
    # a one-value record of a two-channel model enters with its first channel alone
    o.choke = None
    y = np.asarray(o.eval_over_all_parameters((1.0,)))
    assert_array_equal(_bits(o._likelihood_device(y, ((1.0,), 3, 2.0)).cpu().numpy()),
                       _bits(_check_likelihood("one value", o, (1.0,), (3, 0), (2.0, 1.0), n_lik=1)))


def test_likelihood_of_crafted_rates(hip):
    """Through the form that takes given model values: every special case of the header, exactly."""
    y = np.array([[0.0, -1.0, np.nan, np.inf, 1e-300, 700.0, 800.0, 2.0]])
    o = _lorentz_object(oracle.lorentz_cloud(np.random.default_rng(1), 8))
    none = o._likelihood_device(y, ((3.0,), 0)).cpu().numpy()
    some = o._likelihood_device(y, ((3.0,), 3)).cpu().numpy()
    assert_array_equal(none[:4], [1.0, 0.0, 0.0, 0.0])                  # lambda = 0, k = 0: the factor 1
    assert_array_equal(some[:4], [0.0, 0.0, 0.0, 0.0])                  # lambda = 0, k > 0: L = 0
    assert none[4] == 1.0 and none[6] == 0.0 and some[4] == 0.0 and some[6] == 0.0
    for k, t in ((0, 1.0), (3, 1.0), (0, 0.5), (700, 1.0), (3, 2.0)):
        got = o.likelihood(y, ((3.0,), k, t))
        want = oracle.likelihood(y, [k], [t], 1)
        assert_array_equal(got[:4], want[:4])
        assert_allclose(got[4:], want[4:], rtol=1e-10, atol=0.0)
    assert_allclose(o.likelihood(y, ((3.0,), 700, 1.0))[5], 0.015, rtol=0.02)      # k = lambda = 700: no overflow
    # an exposure that takes a finite rate to infinity
    big = np.array([[1e300, 2.0] * 4])
    got = o.likelihood(big, ((3.0,), 0, 1e10))
    assert_array_equal(got, [0.0] * 8)                                 # (not a rate; exp(-2e10))
    assert_array_equal(oracle.likelihood(big, [0], [1e10], 1), [0.0] * 8)


# ------------------------------------------------------------------------------------------------ 2. information
@pytest.mark.parametrize("n", oracle.N_PARTICLES)
def test_information_at_every_cloud_size(hip, n):
    """A lone particle, both sides of the wave, a chunk edge (257) and many chunks; cap 32 at exposure 1 with every
    settings count, slice and subset of outputs; the other caps on the whole grid."""
    cloud, w, _ = _case("wide", n)
    o = _lorentz_object(cloud, w)
    want_info, want_pmf, want_nu, cols = _want("wide", n, 1.0, 32)
    if n > 1:
        assert want_info.max() >= 1e-5                                  # the oracle alone, before the device is asked
    n_s = GRID.size
    whole = _entry(o, 0, n_s)
    _close(f"n={n}", {k: v[..., cols] if k == "nu" else v[cols] for k, v in whole.items()}, want_info, want_pmf, want_nu)
    if n == 1:
        assert np.all(whole["info"] <= INFO_TOL)                        # one particle: nothing to learn
    _same(f"n={n}: run to run", _entry(o, 0, n_s), whole)
    if n < BIG:
        for k in [k for k in oracle.N_SETTINGS if k < n_s]:
            _close(f"n={n} n_settings={k}", _entry(o, 0, k), want_info[:k], want_pmf[:k], want_nu[:, :k])
    # a slice of the grid, as a settings shard asks for it: the whole grid's columns, bit for bit
    for b, e in SLICES:
        _same(f"n={n}: slice {b}:{e}", _entry(o, b, e), whole, slice(b, e))
    # any subset of the outputs
    for subset in (("info",), ("tail",), ("pmf",), ("nu",), ("info", "nu"), ("tail", "pmf"), ("info", "tail", "pmf")):
        got = _entry(o, 0, n_s, outputs=subset)
        assert sorted(got) == sorted(subset)
        _same(f"n={n}: outputs {subset}", got, whole)
    # the cost divides the information, the exposure the variance: IEEE divisions of the same numerators
    cost = 0.5 + np.arange(n_s) % 7
    by_array = _entry(o, 0, n_s, cost=cost, cost_scalar=99.0, outputs=("info", "tail"))
    assert_array_equal(_bits(by_array["info"]), _bits(whole["info"] / cost))
    assert_array_equal(_bits(by_array["tail"]), _bits(whole["tail"]))
    assert_array_equal(_bits(_entry(o, 0, n_s, cost_scalar=3.0, outputs=("info",))["info"]), _bits(whole["info"] / 3.0))
    assert_array_equal(_bits(o.yvar_noise_model()), _bits(whole["nu"]))
    assert_array_equal(_bits(o.count_distribution()), _bits(whole["pmf"]))
    for cap in (16, 64):
        want_info, want_pmf, want_nu, cols = _want("wide", n, 1.0, cap)
        got = _entry(o, 0, n_s, cap=cap)
        _close(f"n={n} cap={cap}", {k: v[..., cols] if k == "nu" else v[cols] for k, v in got.items()}, want_info,
               want_pmf, want_nu)
        assert_array_equal(_bits(got["nu"]), _bits(whole["nu"]))        # (the variance knows no cap)
        _same(f"n={n} cap={cap}: slice", _entry(o, 37, 101, cap=cap), got, slice(37, 101))


@pytest.mark.parametrize("n", [257, 4097])
def test_information_of_a_converged_cloud(hip, n):
    cloud, w, _ = _case("converged", n)
    o = _lorentz_object(cloud, w)
    want_info, want_pmf, want_nu, _ = _want("converged", n, 1.0, 32)
    assert 1e-5 <= want_info.max() <= 1e-3
    got = _entry(o, 0, GRID.size)
    _close(f"converged n={n}", got, want_info, want_pmf, want_nu)
    assert abs(got["info"].max() - want_info.max()) <= INFO_TOL


@pytest.mark.parametrize("exposure,cap", [(1.0, 16), (4.0, 16), (4.0, 64), (0.05, 32), (4.0, 32)])
def test_exposures_and_caps(hip, exposure, cap):
    """The censoring at work: the tail mass from 1e-17 to 0.7, the information with it."""
    cloud, w, R = _case("wide", 4097)
    o = _lorentz_object(cloud, w)
    want_info, want_pmf, want_nu, _ = _want("wide", 4097, exposure, cap)
    assert want_info.max() >= 1e-5
    got = _entry(o, 0, GRID.size, cap=cap, exposure=exposure)
    _close(f"exposure={exposure} cap={cap}", got, want_info, want_pmf, want_nu)
    if (exposure, cap) == (4.0, 16):
        assert got["tail"].max() > 0.5                                  # censoring bites ...
        full = _entry(o, 0, GRID.size, cap=64, exposure=4.0, outputs=("info",))["info"]
        assert np.all(got["info"] < full) and got["info"].max() < 0.8 * full.max()      # ... data processing
    if (exposure, cap) == (0.05, 32):
        assert got["tail"].max() <= 1e-15 and got["info"].max() < 0.03
    # the class: exposure and count_cap are attributes, last_information follows the pass
    o.exposure, o.count_cap = exposure, cap
    assert_array_equal(_bits(o.utility()), _bits(got["info"]))
    assert o.last_information == {"cap": cap, "tail_max": float(got["tail"].max())}
    assert_array_equal(_bits(o.yvar_noise_model()), _bits(got["nu"]))
    assert_array_equal(_bits(o.count_distribution()), _bits(got["pmf"]))


def test_noise_variance_of_two_channels(hip):
    """d_noise_var alone works for every channel count; the outcome sums of a two-channel model are refused."""
    g = np.random.default_rng(500 + 300)
    cloud = oracle.decay_cloud(g, 300)
    w = oracle.weights(g, cloud)
    R = oracle.decay_rates(cloud)
    o = _decay_object(cloud, w, exposure=[1.0, 5.0])
    assert_allclose(o.yvar_noise_model(), oracle.noise_variance(R, w, [1.0, 5.0]), rtol=1e-10, atol=0.0)
    for cap in (16, 32, 64):
        got = _entry(o, 0, TIMES.size, cap=cap, exposure=2.0, outputs=("nu",))
        assert_allclose(got["nu"], oracle.noise_variance(R, w, 2.0), rtol=1e-10, atol=0.0)
    _same("slice", _entry(o, 7, 65, exposure=2.0, outputs=("nu",)), got, slice(7, 65))
    before = o.particle_weights.copy()
    for outputs in (("info",), ("tail", "nu"), ("pmf",)):
        with pytest.raises(RuntimeError, match="one channel"):
            _entry(o, 0, TIMES.size, outputs=outputs)
    for call in (o.utility_information, o.count_distribution):
        with pytest.raises(ValueError, match="one channel"):
            call()
    assert_array_equal(_bits(o.particle_weights), _bits(before))
    u = o.utility()                                                    # variance_approx on nu_bar
    assert u.shape == (TIMES.size,) and np.all(np.isfinite(u))


# ------------------------------------------------------------------------------------------------ 3. exclusion
def test_particles_without_weight_do_not_count_whatever_they_are(hip):
    n = 4097
    cloud, w, R = _case("wide", n)
    g = np.random.default_rng(9)
    idx = g.permutation(n)[:n // 10]
    kinds = np.arange(idx.size) % 3
    w = w.copy()
    w[idx[kinds == 0]] = 0.0
    w[idx[kinds == 1]] = np.nan
    w[idx[kinds == 2]] = -w[idx[kinds == 2]] - 1e-9
    broken = cloud.copy()
    broken[:, idx] = np.nan
    first = _entry(_lorentz_object(broken, w), 0, GRID.size)
    second = _entry(_lorentz_object(cloud, w), 0, GRID.size)           # the same particles with valid parameters
    _same("dirty weights", first, second)
    info, pmf = oracle.design(R, w)
    _close("dirty weights", first, info, pmf, oracle.noise_variance(R, w))


def test_a_particle_whose_rate_is_no_rate_drops_out(hip):
    n = 300
    g = np.random.default_rng(300 + n)
    cloud = oracle.lorentz_cloud(g, n)
    w = oracle.weights(g, cloud)
    out = [3, 64, 299]
    keep = np.setdiff1d(np.arange(n), out)

    def check(what, bad, R_want, w_want):
        info, pmf = oracle.design(R_want, w_want)
        assert info.max() >= 1e-5
        _close(what, _entry(_lorentz_object(bad, w), 0, GRID.size), info, pmf, oracle.noise_variance(R_want, w_want))

    # everywhere: b = -20 puts the rate below 0 at every setting — the oracle on the cloud without these particles
    bad = cloud.copy()
    bad[2, out] = -20.0
    check("r < 0 everywhere", bad, oracle.lorentz_rates(cloud[:, keep]), w[keep])
    # at some settings only: a = -9 leaves r >= 0 far from the line — there the particle still counts
    bad = cloud.copy()
    bad[1, out] = -9.0
    R = oracle.lorentz_rates(bad)
    counted = oracle.contributing(R, w)[:, out]
    assert counted.any() and not counted.all()
    check("r < 0 near the line", bad, R, w)
    # NaN and infinite
    bad = cloud.copy()
    bad[2, out[0]], bad[1, out[1]], bad[0, out[2]] = np.inf, np.nan, np.nan
    check("inf or NaN", bad, oracle.lorentz_rates(cloud[:, keep]), w[keep])


def test_a_cloud_without_any_contributing_particle_gives_nan(hip):
    cloud, w, _ = _case("wide", 257)
    for weights in (np.zeros(257), np.full(257, np.nan), -np.ones(257)):
        got = _entry(_lorentz_object(cloud, weights), 0, GRID.size)
        assert all(np.all(np.isnan(v)) for v in got.values())
    bad = cloud.copy()
    bad[2] = -20.0
    o = _lorentz_object(bad, w)
    got = _entry(o, 0, GRID.size)
    assert all(np.all(np.isnan(v)) for v in got.values())
    assert np.all(np.isnan(o.utility())) and np.all(np.isnan(o.yvar_noise_model()))
    assert np.all(np.isnan(o.count_distribution())) and o.last_information == {"cap": 32, "tail_max": 0.0}


# ------------------------------------------------------------------------------------------------ 4. the class
def test_utility_and_the_choice(hip):
    cloud, w, R = _case("wide", 4097)
    o = _lorentz_object(cloud, w)
    assert o.utility_method == "mutual_information" and o._noise_token() is None and o.last_information is None
    want, _, _, _ = _want("wide", 4097, 1.0, 32)
    got = _entry(o, 0, GRID.size)
    u = o.utility()
    assert u.shape == (GRID.size,)
    assert_array_equal(_bits(u), _bits(got["info"]))
    assert_array_equal(_bits(o.utility_information()), _bits(got["info"]))
    assert o.last_information["cap"] == 32 and 0.0 < o.last_information["tail_max"] < 1e-8
    x = o.opt_setting()
    assert x == (GRID[o.last_setting_index],)
    assert o.last_setting_index == int(np.argmax(want)) or want[o.last_setting_index] >= want.max() - INFO_TOL
    o.rng = np.random.default_rng(3)
    good = o.good_setting()
    assert len(good) == 1 and good[0] in GRID and good == (GRID[o.last_setting_index],)
    # the exposure changes the information as the oracle says; reassigning count_cap changes last_information
    o.exposure = 4.0
    o.count_cap = 64
    assert np.all(np.abs(o.utility() - _want("wide", 4097, 4.0, 64)[0]) <= INFO_TOL)
    assert o.last_information["cap"] == 64
    o.opt_setting()
    assert o.last_setting_index == int(np.argmax(_want("wide", 4097, 4.0, 64)[0]))
    o.count_cap = 16
    o.utility()
    assert o.last_information["cap"] == 16 and o.last_information["tail_max"] > 0.5
    o.exposure, o.count_cap = 1.0, 32
    # a cost_estimate() override divides the information
    cost = 1.0 + np.arange(GRID.size) % 5
    o.cost_estimate = lambda: cost
    assert_array_equal(_bits(o.utility()), _bits(got["info"] / cost))
    o.cost_estimate = lambda: 2.0
    assert_array_equal(_bits(o.utility()), _bits(got["info"] / 2.0))
    # the predicted histogram at given settings: the design grid's rows
    xs = GRID[[5, 64, 129]]
    assert_array_equal(_bits(o.count_distribution((xs,))), _bits(got["pmf"][[5, 64, 129]]))
    for bad in (0, 48, None, 16.5):
        o.count_cap = bad                                              # checked where it is used
        with pytest.raises(ValueError, match="count_cap"):
            o.utility()
    o.count_cap = 32
    for bad in (0, -1.0, [1, 2], np.nan, np.inf):
        o.exposure = bad
        with pytest.raises(ValueError, match="exposure"):
            o.yvar_noise_model()
        with pytest.raises(ValueError):
            o.pdf_update(((3.0,), 0))


def test_variance_utilities_use_the_poisson_noise_variance(hip):
    """utility_method="variance_approx": the Gaussian approximation, with nu_bar for the noise — the utility of a plain
    OptBayesExpt whose yvar_noise_model() returns that same array."""
    import optbayesexpt_amd as obe
    cloud, w, R = _case("wide", 4097)
    o = _lorentz_object(cloud, w, utility_method="variance_approx", n_draws=40, exposure=8.0)
    assert o.utility_method == "variance_approx"
    nubar = o.yvar_noise_model()
    assert nubar.shape == (1, GRID.size)
    assert_allclose(nubar, oracle.noise_variance(R, w, 8.0), rtol=1e-10, atol=0.0)
    o.exposure = 2.0                                                   # the exposure divides nu_bar
    assert_allclose(o.yvar_noise_model(), oracle.noise_variance(R, w, 2.0), rtol=1e-10, atol=0.0)
    t, ld = o._noise_var_device()
    assert ld == t.shape[1] == GRID.size
    o.exposure = 8.0
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
    assert_array_equal(_bits(o.utility_information()), _bits(_entry(o, 0, GRID.size, exposure=8.0)["info"]))


def test_update_multiplies_the_weights_by_the_likelihood(hip):
    cloud, w, _ = _case("wide", 4097)
    o = _lorentz_object(cloud, w, auto_resample=False, exposure=2.0)
    y = np.asarray(o.eval_over_all_parameters((3.1,))).reshape(1, -1)
    for record, k, t in ((((3.1,), 4), 4, 2.0), (((3.1,), 0), 0, 2.0), (((3.1,), 3, 0.5), 3, 0.5),
                         (((3.1,), 30, 4.0), 30, 4.0)):                # ((x, k, t)) overrides exposure
        o.particle_weights = w
        o.pdf_update(record)
        want = oracle.normalised(w * oracle.likelihood(y, [k], [t], 1))
        assert_allclose(o.particle_weights, want, rtol=1e-10, atol=0.0)
    o.particle_weights = w
    o.pdf_update(((3.1,), 3, 0.5), y)                                  # ... and from given model values
    assert_allclose(o.particle_weights, oracle.normalised(w * oracle.likelihood(y, [3], [0.5], 1)), rtol=1e-10, atol=0.0)

    class Mine(type(o)):
        def likelihood(self, y_model, record):                         # a user's likelihood is honoured
            return np.full(self.n_particles, 0.5) * (np.arange(self.n_particles) % 2)

    mine = Mine(o.model_function, (GRID,), cloud, (oracle.WIDTH,), scale=False, auto_resample=False)
    mine.pdf_update(((3.1,), 1))
    assert np.all(mine.particle_weights[::2] == 0.0) and np.all(mine.particle_weights[1::2] > 0.0)


def test_a_function_model_runs_through_its_plugin(hip):
    import _fn_models
    import optbayesexpt_amd as obe
    cloud, w, _ = _case("wide", 257)
    model = obe.models.from_function(_fn_models.lorentzian)
    o = obe.OptBayesExptPoisson(model, (GRID,), cloud, (oracle.WIDTH,), scale=False)
    o.particle_weights = w
    assert o._mlib is not o._lib
    want_info, want_pmf, want_nu, _ = _want("wide", 257, 1.0, 32)
    _close("from_function", _entry(o, 0, GRID.size), want_info, want_pmf, want_nu)
    assert np.all(np.abs(o.utility() - want_info) <= INFO_TOL)
    _check_likelihood("from_function", o, (3.0,), 7, 1.0)


# ------------------------------------------------------------------------------------------------ 5. a run
TRUTH = (3.1, 5.0, 3.0)
RUN_SEED, RUN_CYCLES = 41, 200


def _count(draw, x, exposure=1.0):
    r = TRUTH[2] + TRUTH[1] / (((x[0] - TRUTH[0]) / oracle.WIDTH) ** 2 + 1.0)
    return int(draw.poisson(exposure * r))


def test_counting_run_finds_the_line(hip):
    """200 cycles opt_setting() -> one count -> pdf_update((x, k)) at 2000 particles and 130 settings.  Seed and cycle
    count from the same loop on the oracle (design() for the choice, likelihood() for the update, a Liu-West resample
    below N_eff = N / 2) on the CPU: seed 41 ended 1.3 posterior standard deviations from the truth with sigma(x0)
    0.229 -> 0.0082; seeds 42 and 43 ended 0.5 and 0.01 standard deviations away (0.0065 and 0.0079)."""
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
        o.pdf_update((x, _count(draw, x)))
    mean, std = o.mean(), o.std()
    assert np.all(np.isfinite(mean)) and np.all(std > 0) and len(chosen) > 1
    assert abs(mean[0] - TRUTH[0]) < 5.0 * std[0], (mean, std)
    assert std[0] < prior_std, (std[0], prior_std)
    assert o.last_information["cap"] == 32 and o.last_information["tail_max"] < 1e-6


# ------------------------------------------------------------------------------------------------ 6. state
def test_save_load_copy_and_pickle_continue_alike(hip, tmp_path):
    import optbayesexpt_amd as obe
    g = np.random.default_rng(31)
    o = _lorentz_object(oracle.lorentz_cloud(g, 2000), exposure=3.0, count_cap=64)
    o.rng = np.random.default_rng(32)
    draw = np.random.default_rng(33)
    for _ in range(12):
        x = o.opt_setting()
        o.pdf_update((x, _count(draw, x, 3.0)))
    path = os.path.join(tmp_path, "poisson.state")
    obe.save(o, path)
    twins = [obe.load(path), copy.deepcopy(o), pickle.loads(pickle.dumps(o))]
    outcomes = [int(draw.integers(0, 30)) for _ in range(3)]
    trail = []
    for k in outcomes:
        x = o.opt_setting()
        o.pdf_update((x, k))
        trail.append((x, o.particle_weights.copy(), o.particles.copy()))
    for t in twins:
        assert type(t) is obe.OptBayesExptPoisson
        assert t.utility_method == "mutual_information" and np.all(np.asarray(t.exposure) == 3.0) and t.count_cap == 64
        assert getattr(t.utility, "__func__", None) is obe.OptBayesExptPoisson.utility_information
        for k, (x, weights, particles) in zip(outcomes, trail):
            assert t.opt_setting() == x
            t.pdf_update((x, k))
            assert_array_equal(_bits(t.particle_weights), _bits(weights))
            assert_array_equal(_bits(t.particles), _bits(particles))
        assert_array_equal(_bits(t.yvar_noise_model()), _bits(o.yvar_noise_model()))
        assert_array_equal(_bits(t.count_distribution()), _bits(o.count_distribution()))
    # a variance method travels too, and a saved file of another class loads as before
    v = _lorentz_object(oracle.lorentz_cloud(g, 64), utility_method="variance_full", exposure=[0.25], count_cap=16)
    obe.save(v, path)
    back = obe.load(path)
    assert type(back) is obe.OptBayesExptPoisson and back.utility_method == "variance_full"
    assert np.all(np.asarray(back.exposure) == 0.25) and back.count_cap == 16
    plain = obe.OptBayesExpt(obe.models.lorentzian(1), (GRID,), oracle.lorentz_cloud(g, 64), (oracle.WIDTH,))
    obe.save(plain, path)
    assert type(obe.load(path)) is obe.OptBayesExpt


def _timed(base):
    """A user's subclass of another class that keeps a public ``exposure`` and ``count_cap`` of its own."""
    return type(f"Timed{base.__name__}", (base,), {"__module__": __name__, "__qualname__": f"Timed{base.__name__}"})


def test_exposure_of_another_class_is_the_users_and_travels(hip, tmp_path):
    """``exposure`` and ``count_cap`` are the library's attributes on an OptBayesExptPoisson only: on the other classes
    they go through save / load, pickle and deepcopy with the user's other attributes."""
    import optbayesexpt_amd as obe
    g = np.random.default_rng(41)
    model, cloud = obe.models.lorentzian(1), oracle.lorentz_cloud(g, 64)
    made = []
    for base, kw in ((obe.OptBayesExpt, {}), (obe.OptBayesExptBinomial, {})):
        cls = _timed(base)
        globals()[cls.__name__] = cls                                  # (where pickle and load look a class up)
        made.append(cls(model, (GRID,), cloud * np.array([[1.0], [0.05], [0.05]]), (oracle.WIDTH,), **kw))
    made.append(obe.ParticlePDF(cloud))
    path = os.path.join(tmp_path, "timed.state")
    for o in made:
        o.exposure, o.count_cap, o.my_note = 0.125, 7, "kept"
        obe.save(o, path)
        for t in (obe.load(path), copy.deepcopy(o), pickle.loads(pickle.dumps(o))):
            assert type(t) is type(o) and t.exposure == 0.125 and t.count_cap == 7 and t.my_note == "kept", \
                type(o).__name__


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_and_construction_checks(hip):
    import optbayesexpt_amd as obe
    cloud, w, _ = _case("wide", 257)
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
    # bad records: the weights stay as they were
    before = o.particle_weights.copy()
    for record in (((3.0,), 0.5), ((3.0,), -1), ((3.0,), np.nan), ((3.0,), np.inf), ((3.0,), 1, 0), ((3.0,), 1, -2.0),
                   ((3.0,), 1, np.inf), ((3.0,), 1, np.nan), ((3.0,), "a")):
        with pytest.raises(ValueError):
            o.pdf_update(record)
    assert_array_equal(_bits(o.particle_weights), _bits(before))
    # construction
    model = obe.models.lorentzian(1)
    with pytest.raises(ValueError, match="DeviceModel"):
        obe.OptBayesExptPoisson(lambda s, p, c: p[0], (GRID,), cloud, (oracle.WIDTH,))
    for exposure in (0, -2, [1, 2], np.nan, np.inf):
        with pytest.raises(ValueError, match="exposure"):
            obe.OptBayesExptPoisson(model, (GRID,), cloud, (oracle.WIDTH,), exposure=exposure)
    for cap in (0, 8, 48, 128, 32.5):
        with pytest.raises(ValueError, match="count_cap"):
            obe.OptBayesExptPoisson(model, (GRID,), cloud, (oracle.WIDTH,), count_cap=cap)
    with pytest.raises(SyntaxError):
        obe.OptBayesExptPoisson(model, (GRID,), cloud, (oracle.WIDTH,), utility_method="nonsense")
    with pytest.raises(ValueError, match="variance_approx"):
        obe.OptBayesExptPoisson(obe.models.coil(), (GRID,), cloud, ())


# ------------------------------------------------------------------------------------------------ 8. the example
def test_photon_counts_example(hip):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    done = subprocess.run([sys.executable, os.path.join(root, "examples", "photon_counts.py"), "40", "2000"],
                          capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr[-2000:]
    assert "40 readings" in done.stdout and "x0 =" in done.stdout and "last_information = {'cap': 32" in done.stdout
    assert ">=32" in done.stdout
