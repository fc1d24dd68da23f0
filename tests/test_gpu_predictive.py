"""Device-side posterior predictive summaries (OptBayesExpt.predict / predictive_quantile / predictive_interval;
csrc/obe_predict.hip) against oracles on the rows y = eval_over_all_parameters((x_s,)) of the product itself.

Quantiles are compared for EQUALITY: with tests/_posterior_oracle.py's fixed-point definition for any weights, with
NumPy's inverted_cdf for weights of the form integer / 2^m.  The mean is held to 1e-10 A, A = sum w |y| / sum w, and
the variance to 1e-10 var + 1e-20 A^2, against long double two-pass moments (tests/_predictive_oracle.py).

Measured on an MI355X: see the figures printed by test_worst_errors_are_reported and DESIGN.md section 6."""
import importlib.util
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _fn_models
import _posterior_oracle as post
import _predictive_oracle as oracle
import _state_cases as cases
from optbayesexpt_amd import _posterior

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = (1 << 20) + 3
QS = (0.0, 0.025, 0.5, 0.975, 1.0)
Q17 = tuple(np.linspace(0.0, 1.0, 17) ** 2)
WORST = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ the objects
def _model(name):
    import optbayesexpt_amd as obe
    m = obe.models
    if name == "lorentz1":
        return m.lorentzian(1), (0.1,)
    if name == "lorentz7":
        return m.lorentzian(7), (0.1,)
    if name == "coil":
        return m.coil(), ()
    if name == "rabi":
        return m.rabi(), (1.0e5, 0.3, 2.0)
    if name == "first":
        return m.first_parameter(), ()
    if name == "expression":          # a pole at x = 0: +-inf there, NaN at x = NaN
        return m.from_expression("b + a / x", settings=("x",), parameters=("a", "b")), ()
    if name == "function":
        return m.from_function(_fn_models.lorentzian), (0.1,)
    raise KeyError(name)


def _prior(name, g, n):
    if name in ("lorentz1", "function"):
        return np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    if name == "lorentz7":
        return np.vstack([g.uniform(2, 4, (7, n)), g.uniform(400, 2000, (1, n)), g.normal(500, 1000, (1, n)),
                          g.exponential(500, (1, n))])
    if name == "coil":                 # L, R, C: the imaginary part changes sign across the resonance
        return np.array([g.normal(1e-3, 1e-4, n), g.normal(10.0, 1.0, n), g.normal(1e-6, 1e-7, n)])
    if name == "rabi":
        return np.array([g.uniform(0.5, 2.0, n), g.uniform(-3.0, 3.0, n)])
    if name == "first":
        return np.full((1, n), 3.25)
    if name == "expression":
        return np.array([g.normal(0.0, 2.0, n), g.normal(5.0, 1.0, n)])
    raise KeyError(name)


def _points(name, g, n_x):
    """(n_setdims, n_x) setting points that exercise the model (not a design grid: unsorted, with repeats)."""
    if name == "coil":
        x = g.uniform(1.0e4, 6.0e4, n_x)               # resonance near 3.2e4 rad/s
        return x[None, :]
    if name == "rabi":
        return np.array([g.uniform(0.0, 3.0, n_x), g.uniform(-4.0, 4.0, n_x)])
    if name == "expression":
        return g.uniform(-3.0, 3.0, n_x)[None, :]
    x = g.uniform(1.5, 4.5, n_x)
    if n_x > 2:
        x[1] = x[0]
    return x[None, :]


def _design(name):
    if name == "rabi":
        return (np.linspace(0.0, 3.0, 5), np.linspace(-4.0, 4.0, 7))
    if name == "coil":
        return (np.linspace(1.0e4, 6.0e4, 33),)
    return (np.linspace(1.5, 4.5, 33),)


def _object(name, cloud, weights=None, **kw):
    import optbayesexpt_amd as obe
    model, cons = _model(name)
    o = obe.OptBayesExpt(model, _design(name), cloud, cons, scale=False, **kw)
    if weights is not None:
        o.particle_weights = weights
    return o


def _rows(o, x):
    """y (n_x, C, N_p): the product's own model values, one setting at a time."""
    return np.stack([np.asarray(o.eval_over_all_parameters(tuple(float(v) for v in x[:, s]))).reshape(o.n_channels, -1)
                     for s in range(x.shape[1])])


# ------------------------------------------------------------------------------------------------- the checks
def _check_quantiles(what, o, x, y, w, qs, dyadic):
    got = o.predictive_quantile(qs, x)
    n_x, n_c = y.shape[0], y.shape[1]
    assert got.shape == (len(qs), n_c, n_x) and got.dtype == np.float64
    want = np.empty_like(got)
    for s in range(n_x):
        for c in range(n_c):
            want[:, c, s] = post.quantile_fixed_point(y[s, c], w, qs)
            ys, ws = oracle.kept(y[s, c], w)
            if dyadic and np.all(np.isfinite(ys)):
                assert_array_equal(want[:, c, s], post.quantile_numpy(ys, ws, qs), err_msg=f"{what}: oracle vs NumPy")
    assert_array_equal(got, want, err_msg=what)
    return got


def _check_moments(what, o, x, y, w):
    mean, std = o.predict(x)
    n_x, n_c = y.shape[0], y.shape[1]
    assert mean.shape == std.shape == (n_c, n_x) and mean.dtype == std.dtype == np.float64
    for s in range(n_x):
        for c in range(n_c):
            m, v, a = oracle.moments(y[s, c], w)
            if not np.isfinite(m):
                assert_array_equal(mean[c, s], m, err_msg=f"{what}: mean of setting {s}")
                assert np.isnan(std[c, s]), (what, s, std[c, s])
                continue
            e_mean, e_var = abs(mean[c, s] - m), abs(std[c, s] ** 2 - v)
            tol_mean, tol_var = oracle.mean_tolerance(a), oracle.var_tolerance(v, a)
            for kind, err, tol in (("mean", e_mean, tol_mean), ("var", e_var, tol_var)):
                ratio = err / tol if tol > 0 else (0.0 if err == 0 else np.inf)
                if ratio >= WORST.get(kind, (0.0, ""))[0]:
                    WORST[kind] = ratio, what
                assert err <= tol, f"{what}: {kind} of setting {s}, channel {c}: error {err:.3g} > {tol:.3g}"
    return mean, std


def _general_weights(g, cloud):
    w = g.random(cloud.shape[1]) * np.exp(-0.5 * ((cloud[0] - np.median(cloud[0])) / (np.std(cloud[0]) + 1e-300)) ** 2)
    return w / w.sum()


def _dyadic_weights(g, n):
    w = g.integers(0, 1000, size=n).astype(np.float64) / 2.0 ** 30
    if not w.any():
        w[0] = 2.0 ** -30
    return w


# ------------------------------------------------------------- 1. shapes: clouds x settings, every summary
@pytest.mark.parametrize("n_x", [1, 2, 65, 1000])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_shapes_lorentzian(hip, n, n_x):
    g = np.random.default_rng([n, n_x])
    cloud = _prior("lorentz1", g, n)
    x = _points("lorentz1", g, n_x)
    for dyadic in (True, False):
        w = _dyadic_weights(g, n) if dyadic else _general_weights(g, cloud)
        o = _object("lorentz1", cloud, w)
        y = _rows(o, x)
        what = f"lorentz1 {n} x {n_x} {'dyadic' if dyadic else 'general'}"
        _check_quantiles(what, o, x, y, w, QS, dyadic)
        _check_moments(what, o, x, y, w)
        if n_x == 65:
            _check_quantiles(what + " 17 q", o, x, y, w, Q17, dyadic)          # served in two groups
        lo, hi = o.predictive_interval(0.95, x)
        both = o.predictive_quantile(_posterior.interval_quantiles(0.95), x)
        assert_array_equal(_bits(lo), _bits(both[0]))
        assert_array_equal(_bits(hi), _bits(both[1]))
        assert_array_equal(_bits(o.predictive_quantile(0.5, x)), _bits(o.predictive_quantile((0.5,), x)[0]))


@pytest.mark.parametrize("n_x", [1, 2, 65])
def test_shapes_at_a_million_particles(hip, n_x):
    g = np.random.default_rng([BIG, n_x])
    cloud = _prior("lorentz1", g, BIG)
    x = _points("lorentz1", g, n_x)
    w = _general_weights(g, cloud) if n_x == 2 else _dyadic_weights(g, BIG)
    o = _object("lorentz1", cloud, w)
    y = _rows(o, x)
    _check_quantiles(f"lorentz1 BIG x {n_x}", o, x, y, w, QS, n_x != 2)
    _check_moments(f"lorentz1 BIG x {n_x}", o, x, y, w)


def test_quantiles_of_256_settings_at_a_million_particles(hip):
    g = np.random.default_rng(256)
    n = 1 << 20
    cloud = _prior("lorentz1", g, n)
    cloud[0] = 3.0 + 0.01 * g.normal(size=n)                # a converged centre: most lanes share a digit
    w = _general_weights(g, cloud)
    o = _object("lorentz1", cloud, w)
    x = np.linspace(2.9, 3.1, 256)[None, :]
    y = _rows(o, x)
    _check_quantiles("lorentz1 2^20 x 256", o, x, y, w, (0.025, 0.5, 0.975), False)


@pytest.mark.parametrize("name", ["lorentz7", "coil", "rabi", "expression", "function"])
def test_models(hip, name):
    for n, n_x in ((5000, 65), (65, 1000), (64, 2)):
        g = np.random.default_rng([sum(map(ord, name)), n])
        cloud = _prior(name, g, n)
        x = _points(name, g, n_x)
        for dyadic in (True, False):
            w = _dyadic_weights(g, n) if dyadic else _general_weights(g, cloud)
            o = _object(name, cloud, w)
            assert (o._mlib is not o._lib) == (name in ("expression", "function"))       # plugins serve their own model
            y = _rows(o, x)
            what = f"{name} {n} x {n_x} {'dyadic' if dyadic else 'general'}"
            _check_quantiles(what, o, x, y, w, QS, dyadic)
            _check_moments(what, o, x, y, w)
            if name == "coil":
                assert y.shape[1] == 2 and np.any(y[:, 1] > 0) and np.any(y[:, 1] < 0)      # a sign change


# ------------------------------------------------------------------------------------------ 2. cloud contents
def test_ties_zero_weights_and_nan_weights(hip):
    g = np.random.default_rng(31)
    n = 5000
    cloud = _prior("lorentz1", g, n)
    cloud[:, ::5] = cloud[:, 1::5]                          # every fifth particle repeats its neighbour: ties in y
    x = _points("lorentz1", g, 9)
    w = _dyadic_weights(g, n)
    o = _object("lorentz1", cloud, w)
    y0 = _rows(o, x[:, :1])[0, 0]
    order = np.argsort(y0)
    w[order[:3]] = 0.0                                      # zero weights at both ends of setting 0's sorted y
    w[order[-3:]] = 0.0
    w[order[5]] = np.nan                                    # NaN weights count as zero
    w[order[-7]] = np.nan
    w[order[100]] = -0.25                                   # and so do negative ones
    o.particle_weights = w
    y = _rows(o, x)
    _check_quantiles("ties", o, x, y, w, QS, True)
    _check_moments("ties", o, x, y, w)


def test_constant_output(hip):
    """first_parameter with equal particles: every quantile is that value, the variance exactly zero."""
    g = np.random.default_rng(32)
    for n in (1, 64, 5000):
        cloud = _prior("first", g, n)
        w = _general_weights(g, g.normal(size=(1, n)))
        o = _object("first", cloud, w)
        x = _points("first", g, 3)
        mean, std = o.predict(x)
        assert_array_equal(o.predictive_quantile(QS, x), np.full((len(QS), 1, 3), 3.25))
        assert np.all(np.abs(mean - 3.25) <= 1e-10 * 3.25)
        assert np.all(std ** 2 <= 1e-20 * 3.25 ** 2)
        _check_moments("constant", o, x, _rows(o, x), w)


def test_settings_that_make_the_model_nan_or_inf(hip):
    g = np.random.default_rng(33)
    n = 5000
    # NaN setting: every y is NaN
    cloud = _prior("lorentz1", g, n)
    w = _general_weights(g, cloud)
    o = _object("lorentz1", cloud, w)
    x = np.array([[2.5, np.nan, 3.5, np.inf]])
    y = _rows(o, x)
    assert np.all(np.isnan(y[1])) and np.all(np.isfinite(y[3]))
    got = _check_quantiles("nan setting", o, x, y, w, QS, False)
    assert np.all(np.isnan(got[:, 0, 1])) and np.all(np.isfinite(got[:, 0, [0, 2, 3]]))
    mean, std = _check_moments("nan setting", o, x, y, w)
    assert np.isnan(mean[0, 1]) and np.isnan(std[0, 1]) and np.all(np.isfinite(mean[0, [0, 2, 3]]))
    # a pole: +inf and -inf by the sign of a, NaN where a == 0 (0 / 0)
    cloud = _prior("expression", g, n)
    cloud[0, :5] = 0.0
    w = _dyadic_weights(g, n)
    o = _object("expression", cloud, w)
    x = np.array([[0.0, 1.0, -0.0, 2.0]])
    y = _rows(o, x)
    assert np.any(np.isposinf(y[0])) and np.any(np.isneginf(y[0])) and np.any(np.isnan(y[0]))
    got = _check_quantiles("pole", o, x, y, w, QS, True)
    assert got[0, 0, 0] == -np.inf and (np.isnan(got[-1, 0, 0]) or got[-1, 0, 0] == np.inf)
    _check_moments("pole", o, x, y, w)
    # only positive amplitudes carry weight: the mean is +inf, no NaN among the weighted y
    w2 = np.where(cloud[0] > 0, w, 0.0)
    o.particle_weights = w2
    mean, std = _check_moments("pole, positive side", o, x, y, w2)
    assert mean[0, 0] == np.inf and np.isfinite(mean[0, 1])
    _check_quantiles("pole, positive side", o, x, y, w2, QS, True)


# ----------------------------------------------------------------------------------------- 3. variance cases
def test_variance_of_a_converged_cloud(hip):
    """theta_i = theta0 (1 + 1e-6 z_i): sd / A ~ 1e-6, so a sum about a centre that is off by eps A would be wrong by
    ~1e-4 of the variance; the floor 1e-20 A^2 is 1e-8 of it."""
    g = np.random.default_rng(41)
    for name, theta0 in (("lorentz1", np.array([3.0, -1000.0, 50000.0])),
                         ("lorentz7", np.array([2.2, 2.5, 2.8, 3.1, 3.4, 3.7, 3.9, 1000.0, 500.0, 500.0]))):
        for n in (5000, 1 << 18):
            cloud = theta0[:, None] * (1.0 + 1e-6 * g.normal(size=(theta0.size, n)))
            w = _general_weights(g, g.normal(size=(1, n)))
            o = _object(name, cloud, w)
            x = _points(name, g, 65)
            y = _rows(o, x)
            for s in range(0, 65, 16):
                m, v, a = oracle.moments(y[s, 0], w)
                assert 1e-8 < np.sqrt(v) / a < 1e-4
            _check_moments(f"converged {name} {n}", o, x, y, w)
            _check_quantiles(f"converged {name} {n}", o, x[:, :9], y[:9], w, QS, False)


def test_variance_with_a_single_weight(hip):
    g = np.random.default_rng(42)
    n = 5000
    cloud = _prior("lorentz1", g, n)
    w = np.zeros(n)
    w[1234] = 0.5
    o = _object("lorentz1", cloud, w)
    x = _points("lorentz1", g, 65)
    y = _rows(o, x)
    mean, std = _check_moments("single weight", o, x, y, w)
    assert_array_equal(mean[0], y[:, 0, 1234])
    assert np.all(std == 0.0)
    assert_array_equal(o.predictive_quantile(QS, x), np.broadcast_to(y[:, 0, 1234], (len(QS), 1, 65)))


def test_variance_of_a_prior_width_cloud(hip):
    g = np.random.default_rng(43)
    for name in ("lorentz1", "coil", "rabi"):
        n = 1 << 16
        cloud = _prior(name, g, n)
        w = np.full(n, 1.0 / n)
        o = _object(name, cloud, w)
        x = _points(name, g, 65)
        _check_moments(f"prior {name}", o, x, _rows(o, x), w)


# --------------------------------------------------------------------------------------------- 4. K1 cross-check
def test_variance_agrees_with_the_full_sweep(hip):
    """A variance_full object: predict()[1]**2 on its grid and yvar_from_parameter_draws() (K1) both within 1e-10
    relative of the oracle."""
    o = cases.build("strict4096")
    cases.run(o, "strict4096", 0, 6)
    w = np.array(o.particle_weights)
    x = np.asarray(o.allsettings)
    y = _rows(o, x)
    mean, std = o.predict()
    yvar = np.asarray(o.yvar_from_parameter_draws())
    for s in range(x.shape[1]):
        m, v, a = oracle.moments(y[s, 0], w)
        assert abs(std[0, s] ** 2 - v) <= 1e-10 * v, (s, std[0, s] ** 2, v)
        assert abs(yvar[0, s] - v) <= 1e-10 * v, (s, yvar[0, s], v)
        assert abs(mean[0, s] - m) <= oracle.mean_tolerance(a)


def test_c2_size_against_the_host_sweep(hip):
    """4 096 settings x 262 144 particles after three real updates: predict()[1]**2 against oracle/csweep.c's plain-C
    full sweep on the host cores (as tests/test_gpu_scale.py uses it), 1e-10 relative."""
    import time
    import bench
    from oracle import csweep
    csweep.build()
    settings, prior, cons, true, sigma = bench.make_workload("c2")
    o = bench.build_obe("c2", None, settings, prior.copy(), cons)
    o.rng = np.random.default_rng(5)
    o.tuning_parameters["auto_resample"] = False
    sim = np.random.default_rng(9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for _ in range(3):
            xs = o.opt_setting()
            o.pdf_update((xs, float(o.model_function(xs, true, cons)) + sigma * sim.standard_normal(), sigma))
    w = np.array(o.particle_weights)
    ref = np.asarray(csweep.lorentz_yvar(np.ascontiguousarray(settings[0]), np.array(o.particles), w, cons[0], 1)).reshape(-1)
    t0 = time.perf_counter()
    mean, std = o.predict()
    print(f"predict() at c2 size: {1e3 * (time.perf_counter() - t0):.1f} ms wall")
    err = np.abs(std[0] ** 2 - ref) / ref
    WORST["c2 variance vs csweep (relative)"] = float(err.max()), "c2"
    assert np.all(err <= 1e-10), float(err.max())
    yvar = np.asarray(o.yvar_from_parameter_draws())
    assert np.all(np.abs(yvar[0] - ref) <= 1e-10 * ref)
    # the mean of a sample of settings against the long double oracle
    for s in range(0, 4096, 512):
        m, v, a = oracle.moments(_rows(o, np.asarray(o.allsettings)[:, s:s + 1])[0, 0], w)
        assert abs(mean[0, s] - m) <= oracle.mean_tolerance(a)


# ------------------------------------------------------------------------------------- 5. reference posteriors
@pytest.mark.parametrize("name,cycles", [("lorentz3_demo", 30), ("multilorentz7_noise", 20)])
def test_reference_posteriors(hip, name, cycles):
    import _replay
    import optbayesexpt_amd as obe
    fx = _replay.load_traj(name)
    model = {"lorentzian": obe.models.lorentzian(1), "multi_lorentzian_7": obe.models.lorentzian(7)}[fx["meta"]["model"]]
    o = _replay.construct(fx, obe.OptBayesExpt, obe.OptBayesExptNoiseParameter, model)
    meta = fx["meta"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for cyc in range(cycles):
            x = o.opt_setting() if meta["selection"] == "opt" else o.good_setting(meta["pickiness"])
            yv = float(fx["y_meas"][cyc][0])
            o.pdf_update((x, yv, meta["sigma_meas"]) if meta["cls"] == "base" else (x, yv))
    w = np.array(o.particle_weights)
    x = np.asarray(o.allsettings)
    y = _rows(o, x)
    # settings=None is the design grid
    mean, std = _check_moments(name, o, None, y, w)
    got = _check_quantiles(name, o, None, y, w, QS, False)
    lo, hi = o.predictive_interval(0.95)
    assert_array_equal(_bits(lo), _bits(got[1]))
    assert_array_equal(_bits(hi), _bits(got[3]))
    assert np.all(lo <= got[2]) and np.all(got[2] <= hi)


# ------------------------------------------------------------------------------------------- 6. determinism
def test_results_are_bit_identical_from_run_to_run_and_under_permutation(hip):
    g = np.random.default_rng(61)
    n = 1 << 18
    for name in ("lorentz1", "coil"):
        cloud = _prior(name, g, n)
        x = _points(name, g, 65)
        for spread in (0.002, 5.0):
            w = np.exp(-0.5 * ((cloud[0] - np.median(cloud[0])) / (spread * np.std(cloud[0]))) ** 2) * g.random(n)
            w /= w.sum()
            perm = g.permutation(n)
            a, b = _object(name, cloud, w), _object(name, cloud[:, perm], w[perm])
            q1, m1, s1 = a.predictive_quantile(QS, x), *a.predict(x)
            q2, m2, s2 = a.predictive_quantile(QS, x), *a.predict(x)
            assert_array_equal(_bits(q1), _bits(q2))
            assert_array_equal(_bits(m1), _bits(m2))
            assert_array_equal(_bits(s1), _bits(s2))
            assert_array_equal(_bits(b.predictive_quantile(QS, x)), _bits(q1), err_msg="permuted cloud")
            lo, hi = b.predictive_interval(0.9, x)
            lo1, hi1 = a.predictive_interval(0.9, x)
            assert_array_equal(_bits(lo), _bits(lo1))
            assert_array_equal(_bits(hi), _bits(hi1))


# --------------------------------------------------------------------------------------- 7. no side effects
def _summaries(o):
    x = (np.linspace(2.0, 4.0, 7),)
    return o.predict(), o.predict(x), o.predictive_quantile((0.1, 0.9)), o.predictive_quantile(0.5, x), \
        o.predictive_interval(0.95), o.predictive_interval(0.5, x)


def _flags(o):
    return (o._particles.version, o._weights.version, o._particles._host_valid, o._weights._host_valid,
            o._particles._dev_valid, o._weights._dev_valid, o._mom_host_key, o._mom_dev_key, o._cdf_key, o._sumsq_key,
            json.dumps(o.rng.bit_generator.state, sort_keys=True, default=str))


def _run(case, n, watch):
    o = cases.build(case)
    picks, resampled = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for cyc in range(n):
            x = o.opt_setting()
            picks.append(int(o.last_setting_index))
            if watch:
                before = _flags(o), o.sweep_state()
                _summaries(o)
                assert (_flags(o), o.sweep_state()) == before, f"cycle {cyc}, after opt_setting"
            o.pdf_update(cases.measure(o, case, cyc, x))
            resampled.append(bool(o.just_resampled))
            if watch:
                assert not o._weights._host_valid         # behind a device-side update the host copies stay stale
                before = _flags(o), o.sweep_state()
                _summaries(o)
                assert (_flags(o), o.sweep_state()) == before, f"cycle {cyc}, after pdf_update"
                assert not o._weights._host_valid
    return o, cases.outcome(o, picks, resampled)


@pytest.mark.parametrize("case", ["lorentz_full", "noise7", "expression", "function"])
def test_a_trajectory_is_unchanged_by_predictions_between_its_cycles(hip, case):
    """30 seeded cycles with the three methods called after every opt_setting() and every pdf_update() (lorentz_full:
    with a speculative variance_full sweep in flight; noise7: a noise-parameter object; expression, function: plugin
    models) against the same run without them: settings, resample flags, weights, cloud and generator state."""
    from optbayesexpt_amd import _state
    watched, got = _run(case, 30, True)
    plain, want = _run(case, 30, False)
    assert got["picks"] == want["picks"] and got["resampled"] == want["resampled"]
    assert any(want["resampled"])
    assert_array_equal(_bits(got["weights"]), _bits(want["weights"]))
    assert_array_equal(_bits(got["particles"]), _bits(want["particles"]))
    np.testing.assert_equal(got["rng"], want["rng"])
    assert set(_state.snapshot(watched)) == set(_state.snapshot(plain))          # nothing added to snapshots


# ------------------------------------------------------------------------------------------------ 8. breadth
@pytest.mark.parametrize("case", ["noise7", "sweeper"])
def test_experiment_objects_answer_for_their_cloud(hip, case):
    o = cases.build(case)
    cases.run(o, case, 0, 12)
    w = np.array(o.particle_weights)
    if case == "noise7":
        assert np.any(w == 0.0)                                     # the constraint zeroed some weights
    x = np.asarray(o.allsettings)[:, ::3]
    y = _rows(o, x)
    _check_moments(case, o, x, y, w)
    _check_quantiles(case, o, x, y, w, QS, False)


def test_host_edits_are_uploaded_first(hip):
    g = np.random.default_rng(81)
    n = 5000
    cloud = _prior("lorentz1", g, n)
    w = _dyadic_weights(g, n)
    o = _object("lorentz1", cloud, w)
    x = _points("lorentz1", g, 5)
    o.predict(x)
    o.particle_weights[cloud[0] > 3.0] = 0                           # in place, by host code
    w2 = np.where(cloud[0] > 3.0, 0.0, w)
    y = _rows(o, x)
    _check_quantiles("edited weights", o, x, y, w2, QS, True)
    _check_moments("edited weights", o, x, y, w2)
    o.particles[2] += 100.0                                          # the background row
    y2 = _rows(o, x)
    assert np.all(y2 != y)
    _check_quantiles("edited particles", o, x, y2, w2, QS, True)
    _check_moments("edited particles", o, x, y2, w2)
    o.particle_weights = w[:-1]
    with pytest.raises(ValueError, match="different lengths"):
        o.predict(x)


def test_settings_none_is_the_design_grid(hip):
    g = np.random.default_rng(82)
    cloud = _prior("rabi", g, 5000)
    o = _object("rabi", cloud, _general_weights(g, cloud))
    grid = np.asarray(o.allsettings)
    assert grid.shape == (2, 35)
    for call in (lambda s: o.predict(s), lambda s: (o.predictive_quantile(QS, s),), lambda s: o.predictive_interval(0.8, s)):
        for other in (grid, (grid[0], grid[1])):
            for a, b in zip(call(None), call(other)):
                assert a.shape[-2:] == (1, 35)
                assert_array_equal(_bits(a), _bits(b))
    one = o.predict((grid[0, 3], grid[1, 3]))                        # scalars: one point
    assert one[0].shape == (1, 1)
    assert_array_equal(_bits(one[0][:, 0]), _bits(o.predict()[0][:, 3]))
    half = o.predict((0.5, grid[1]))                                  # a scalar broadcast against points
    assert half[0].shape == (1, 35)


def test_requests_larger_than_one_call_are_tiled(hip, monkeypatch):
    from optbayesexpt_amd import _predictive
    g = np.random.default_rng(83)
    cloud = _prior("coil", g, 640)
    o = _object("coil", cloud, _general_weights(g, cloud))
    x = _points("coil", g, 1000)
    want_q, want_m = o.predictive_quantile(Q17, x), o.predict(x)
    monkeypatch.setattr(_predictive, "SETTINGS_PER_CALL", 333)
    assert_array_equal(_bits(o.predictive_quantile(Q17, x)), _bits(want_q))
    got_m = o.predict(x)
    assert_array_equal(_bits(got_m[0]), _bits(want_m[0]))
    assert_array_equal(_bits(got_m[1]), _bits(want_m[1]))


# --------------------------------------------------------------------------- 9. example and delivery audit
def test_predictive_band_example(hip):
    spec = importlib.util.spec_from_file_location("predictive_band", os.path.join(ROOT, "examples", "predictive_band.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        true_curve, history = mod.main(n_measure=60, n_samples=20000, every=20, seed=3, quiet=True)
    assert [h[0] for h in history] == [20, 40, 60]
    i, x, mean, std, lo, hi = history[-1]
    assert mean.shape == std.shape == lo.shape == hi.shape == x.shape == true_curve.shape
    assert np.all(lo <= hi) and np.all(std >= 0)
    assert np.mean(history[-1][3]) < np.mean(history[0][3])          # the band narrows
    assert np.all(np.abs(mean - true_curve) <= 10 * std + 5 * (hi - lo))


def test_worst_errors_are_reported(hip):
    """(runs last of the comparisons: the worst error / tolerance ratios seen by this file's moment checks)"""
    for kind, (ratio, what) in sorted(WORST.items()):
        print(f"worst {kind}: {ratio:.3g} ({what})")
    assert WORST


def test_this_file_under_the_delivery_audit(hip, tmp_path):
    """Once more in a child process with OBE_CHECK_DELIVERY=1 (the pattern of tests/test_gpu_posterior.py): no armed
    host word is read, no landing zone is released with armed words."""
    assert "OBE_PREDICTIVE_AUDIT_CHILD" not in os.environ, "the audited child must not start a child of its own"
    report = tmp_path / "audit.jsonl"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"), OBE_CHECK_DELIVERY="1",
               OBE_AUDIT_REPORT=str(report), OBE_PREDICTIVE_AUDIT_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider", "-k", "not test_this_file_under_the_delivery_audit"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "DeliveryError" not in r.stdout + r.stderr and " passed" in r.stdout and "skipped" not in r.stdout
    assert "1 deselected" in r.stdout
    rows = [json.loads(line) for line in report.read_text().splitlines()]
    assert rows and not any(row["pending_violations"] for row in rows), rows
    assert sum(row["reads"] for row in rows) > 100
