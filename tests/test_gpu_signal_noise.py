"""Signal-dependent measurement noise on the device (OptBayesExptSignalNoise; csrc/obe_signal_noise.hip) against
tests/_signal_noise_oracle.py, fed the product's own model values y = eval_over_all_parameters((x,)): the comparison
is about these two kernels and the class, not about the model.

Tolerances.  Likelihood: |dL| <= 1e-10 L on the particles whose oracle log L >= -600 (the exponent's absolute error is
a few eps |arg| with |arg| <= 600), L <= 1e-250 on the others; the compared particles are at least 90 % of the cloud in
every case, asserted from the oracle alone before the device is asked.  nu_bar: 1e-10 relative (N positive terms in a
fixed order lose at most N eps: 1.2e-10 at 2^20, less below).  Run to run: the same bits."""
import copy
import os
import pickle
import warnings

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _replay
import _signal_noise_oracle as oracle

pytestmark = pytest.mark.gpu
BIG = (1 << 20) + 3
LIK_SETTINGS = (2.0, 3.0, 3.37)
LIK_COEF = ((0.0, 1.0, 0.0), (4e4, 0.5, 1e-5), (9e4, 0.0, 0.0), (0.0, 0.0, 4e-5))      # (a, b, c) of nu
GRID = np.linspace(2.0, 4.0, 130)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _public(abc):
    """(noise_floor, noise_gain, noise_relative) keywords from (a, b, c) rows, one per channel."""
    abc = np.atleast_2d(np.asarray(abc, dtype=np.float64))
    return dict(noise_floor=np.sqrt(abc[:, 0]), noise_gain=abc[:, 1].copy(), noise_relative=np.sqrt(abc[:, 2]))


# ------------------------------------------------------------------------------------------------ the objects
def _model(name):
    import optbayesexpt_amd as obe
    m = obe.models
    if name in ("dip", "peak"):
        return m.lorentzian(1), (0.1,)
    if name == "coil":
        return m.coil(), ()
    if name == "rabi":
        return m.rabi(), (1.0e5, 0.3, 2.0)
    if name == "expression":
        return m.from_expression("b + a / (x * x + 1)", settings=("x",), parameters=("a", "b")), ()
    if name == "first":
        return m.first_parameter(), ()
    raise KeyError(name)


def _prior(name, g, n):
    if name == "dip":
        return np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 300, n)])
    if name == "peak":
        return np.array([g.normal(3, 0.05, n), g.uniform(400, 2000, n), g.normal(50, 5, n)])
    if name == "coil":
        return np.array([g.normal(1e-3, 1e-4, n), g.normal(10.0, 1.0, n), g.normal(1e-6, 1e-7, n)])
    if name == "rabi":
        return np.array([g.uniform(0.5, 2.0, n), g.uniform(-3.0, 3.0, n)])
    if name == "expression":
        return np.array([g.normal(0.0, 2.0, n), g.normal(5.0, 1.0, n)])
    raise KeyError(name)


def _design(name):
    if name == "rabi":
        return (np.linspace(0.0, 3.0, 5), np.linspace(-4.0, 4.0, 7))
    if name == "coil":
        return (np.linspace(1.0e4, 6.0e4, 33),)
    if name == "expression":
        return (np.linspace(-3.0, 3.0, 33),)
    return (np.linspace(2.0, 4.0, 201),)


def _weights(g, cloud):
    w = g.random(cloud.shape[1]) * np.exp(-0.5 * ((cloud[0] - np.median(cloud[0])) / (np.std(cloud[0]) + 1e-300)) ** 2)
    return w / w.sum()


def _object(name, cloud, abc, design=None, weights=None, **kw):
    import optbayesexpt_amd as obe
    model, cons = _model(name)
    kw.setdefault("scale", False)
    o = obe.OptBayesExptSignalNoise(model, _design(name) if design is None else design, cloud, cons, **_public(abc), **kw)
    if weights is not None:
        o.particle_weights = weights
    return o


def _rows(o, settings=None):
    """Y (n_settings, C, N_p): the product's own model values, one setting of the design grid at a time."""
    pts = o.allsettings if settings is None else np.atleast_2d(settings)
    return np.stack([np.asarray(o.eval_over_all_parameters(tuple(float(v) for v in pts[:, s]))).reshape(o.n_channels, -1)
                     for s in range(pts.shape[1])])


def _scaled_coef(Y):
    """Coefficient sets (a, b, c) per channel on the scale of the model values' own spread s (the median over the
    settings): a floor of s alone, then a floor of s / 2 with counting noise, with relative noise, and with both, each
    of which reaches s at the median signal.  (Every set keeps a floor: an output that crosses zero — the coil's
    reactance at resonance — would otherwise have particles of vanishing nu, whose log-likelihood no double holds.)"""
    n_c = Y.shape[1]
    s = np.array([np.median(np.std(Y[:, c], axis=1)) + 1e-300 for c in range(n_c)])
    mag = np.array([np.median(np.abs(Y[:, c])) + 1e-300 for c in range(n_c)])
    zero, floor = np.zeros(n_c), s * s / 4
    return [np.stack(k, axis=1) for k in ((s * s, zero, zero), (floor, 0.75 * s * s / mag, zero),
                                          (floor, zero, 0.75 * (s / mag) ** 2),
                                          (floor, 0.5 * s * s / mag, 0.25 * (s / mag) ** 2))]


# ------------------------------------------------------------------------------------------------ 1. likelihood
def _check_likelihood(what, o, setting, y, abc, g, n_lik=None, choke=None):
    """Both forms of the kernel for one record against the oracle fed y (C, N_p)."""
    n_c, n = y.shape
    n_lik = n_c if n_lik is None else n_lik
    abc = np.atleast_2d(abc)
    pick = int(g.integers(0, n))
    ym = y[:, pick] + np.sqrt(oracle.nu(y[:, pick], abc)) * g.normal(0.0, 1.0, n_c)
    ll = oracle.log_likelihood(y, ym, abc, n_lik)
    compared = ll >= -600.0
    assert np.count_nonzero(compared) >= 0.9 * n, (what, np.count_nonzero(compared), n)      # the oracle alone
    want = oracle.likelihood(y, ym, abc, n_lik, choke)
    for k, v in _public(abc).items():
        setattr(o, k, v)
    o.choke = choke
    record = (setting, ym[:n_lik] if n_c > 1 else float(ym[0]), 123.0)            # (a record's sigma is ignored)
    from_model = o._likelihood_device(None, record).cpu().numpy()
    from_y = o._likelihood_device(y, record).cpu().numpy()
    assert from_model.shape == (n,) and from_model.dtype == np.float64
    assert_array_equal(_bits(from_model), _bits(from_y), err_msg=f"{what}: model form vs d_y form")
    assert_array_equal(_bits(o.likelihood(y, record[:2])), _bits(from_y), err_msg=f"{what}: likelihood()")
    err = np.abs(from_model - want)
    worst = int(np.argmax(np.where(compared, err / np.maximum(want, 1e-300), 0.0)))
    assert np.all(err[compared] <= 1e-10 * want[compared]), \
        f"{what}: particle {worst}: {from_model[worst]!r} vs {want[worst]!r}"
    assert np.all(from_model[~compared] <= 1e-250), what
    return from_model


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099, 70001])
def test_likelihood_dip_cloud(hip, n):
    g = np.random.default_rng(100 + n)
    cloud = _prior("dip", g, n)
    o = _object("dip", cloud, LIK_COEF[0])
    for x in LIK_SETTINGS:
        y = _rows(o, [[x]])[0]
        for abc in LIK_COEF:
            _check_likelihood(f"dip n={n} x={x} coef={abc}", o, (x,), y, abc, g)


def test_likelihood_choke(hip):
    g = np.random.default_rng(7)
    o = _object("dip", _prior("dip", g, 4099), LIK_COEF[1])
    y = _rows(o, [[3.37]])[0]
    plain = _check_likelihood("choke: none", o, (3.37,), y, LIK_COEF[1], np.random.default_rng(8))
    choked = _check_likelihood("choke 0.5", o, (3.37,), y, LIK_COEF[1], np.random.default_rng(8), choke=0.5)
    assert_allclose(choked, np.sqrt(plain), rtol=1e-14)


@pytest.mark.parametrize("name", ["coil", "rabi", "expression"])
def test_likelihood_other_models(hip, name):
    """Two channels with n_lik_channels 1 and 2 (coil), two setting dimensions (rabi), a formula's plugin."""
    g = np.random.default_rng(sum(map(ord, name)))
    cloud = _prior(name, g, 4099)
    o = _object(name, cloud, np.ones((1, 3)) if name != "coil" else np.ones((2, 3)))
    pts = o.allsettings[:, [1, o.allsettings.shape[1] // 2, -2]]
    Y = _rows(o, pts)
    for abc in _scaled_coef(Y):
        for k in range(pts.shape[1]):
            for n_lik in range(1, o.n_channels + 1):
                _check_likelihood(f"{name} point {k} n_lik={n_lik}", o, tuple(pts[:, k]), Y[k], abc, g, n_lik=n_lik)


@pytest.mark.parametrize("name", ["first", "expression"])
def test_particle_with_zero_noise_variance_gets_zero_likelihood(hip, name):
    """a = 0 and y = 0 exactly: nu = 0, L == 0 — and the update zeroes that particle's weight."""
    g = np.random.default_rng(3)
    if name == "first":
        cloud = g.uniform(10.0, 20.0, (1, 300))
        cloud[0, [0, 77, 299]] = 0.0
        design, setting = (np.linspace(0.0, 1.0, 5),), (0.5,)
    else:
        cloud = np.array([g.uniform(10.0, 20.0, 300), g.uniform(1.0, 2.0, 300)])
        cloud[:, [0, 77, 299]] = 0.0
        design, setting = None, (1.5,)
    for abc in ((0.0, 1.0, 0.0), (0.0, 0.0, 0.01), (0.0, 1.0, 0.01)):
        o = _object(name, cloud, abc, design=design, auto_resample=False)
        y = _rows(o, [[setting[0]]])[0]
        assert np.all(y[0, [0, 77, 299]] == 0.0) and np.count_nonzero(y) == 297
        lik = o._likelihood_device(None, (setting, 15.0)).cpu().numpy()
        assert_array_equal(lik[[0, 77, 299]], [0.0, 0.0, 0.0])
        assert np.all(lik[y[0] != 0] > 0)
        assert_array_equal(_bits(lik), _bits(o._likelihood_device(y, (setting, 15.0)).cpu().numpy()))
        assert_allclose(lik, oracle.likelihood(y, [15.0], [abc], 1), rtol=1e-10)
        o.pdf_update((setting, 15.0))
        w = o.particle_weights
        assert_array_equal(w[[0, 77, 299]], [0.0, 0.0, 0.0])
        assert abs(w.sum() - 1.0) < 1e-12


# ------------------------------------------------------------------------------------------------ 2. nu_bar
def _fresh(o, begin, end):
    """nu_bar of the settings [begin, end) by a call of its own (the object's cache emptied first)."""
    o._nu_bar = {}
    return o._noise_variance(begin, end).cpu().numpy()


def _dirty_weights(g, cloud):
    """Weights of which some are zero, NaN or negative; the particles of zero weight carry NaN or inf parameters."""
    n = cloud.shape[1]
    w = _weights(g, cloud)
    cloud = cloud.copy()
    idx = g.permutation(n)[:max(3, n // 5)]
    kinds = np.arange(idx.size) % 3
    w[idx[kinds == 0]] = 0.0
    w[idx[kinds == 1]] = np.nan
    w[idx[kinds == 2]] = -w[idx[kinds == 2]] - 1e-9
    cloud[0, idx[::2]] = np.nan
    cloud[1, idx[1::2]] = np.inf
    return w, cloud


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099, 70001])
def test_noise_variance_dip_cloud(hip, n):
    """One chunk, a chunk boundary, a ragged last chunk, many chunks; both sides of the wave of 64 settings; clean and
    dirty weights; the slice form."""
    g = np.random.default_rng(200 + n)
    clean = _prior("dip", g, n)
    variants = [("clean", _weights(g, clean), clean)]
    if n > 1:
        variants.append(("dirty",) + _dirty_weights(g, clean))
    for kind, w, cloud in variants:
        o = _object("dip", cloud, LIK_COEF[1], design=(GRID,), weights=w)
        Y = _rows(o)                    # (NaN or inf where the parameters are: the oracle drops what has no weight)
        for abc in (LIK_COEF[1], LIK_COEF[0], LIK_COEF[3]):
            for k, v in _public(abc).items():
                setattr(o, k, v)
            want = oracle.noise_variance(Y, w, [abc])
            whole = _fresh(o, 0, GRID.size)
            assert whole.shape == (1, GRID.size) and np.all(np.isfinite(want))
            assert_allclose(whole, want, rtol=1e-10, atol=0.0, err_msg=f"{kind} n={n} coef={abc}")
            assert_array_equal(_bits(_fresh(o, 0, GRID.size)), _bits(whole), err_msg="run to run")
            for n_s in (1, 63, 64, 65):
                got = _fresh(o, 0, n_s)
                assert got.shape == (1, n_s)
                assert_allclose(got, want[:, :n_s], rtol=1e-10, atol=0.0, err_msg=f"{kind} n={n} n_settings={n_s}")
            # a slice of the grid, as a settings shard asks for it: the whole grid's columns, bit for bit
            for b, e in ((0, 64), (64, 130), (37, 101), (129, 130)):
                assert_array_equal(_bits(_fresh(o, b, e)), _bits(whole[:, b:e]), err_msg=f"slice {b}:{e}")
        assert_array_equal(_bits(o.yvar_noise_model()), _bits(_fresh(o, 0, GRID.size)))


def test_noise_variance_large_cloud(hip):
    """2^20 + 3 particles, 65 settings: the chunk count is capped by the grid, the last chunk is ragged."""
    g = np.random.default_rng(11)
    cloud = _prior("dip", g, BIG)
    w = _weights(g, cloud)
    x = np.linspace(2.0, 4.0, 65)
    o = _object("dip", cloud, LIK_COEF[1], design=(x,), weights=w)
    got = _fresh(o, 0, 65)
    for s in range(65):
        y = np.asarray(o.eval_over_all_parameters((float(x[s]),))).reshape(1, 1, -1)
        assert_allclose(got[:, s:s + 1], oracle.noise_variance(y, w, [LIK_COEF[1]]), rtol=1e-10, atol=0.0, err_msg=str(s))
    assert_array_equal(_bits(_fresh(o, 0, 65)), _bits(got))


def test_noise_variance_of_all_zero_weights_is_nan(hip):
    g = np.random.default_rng(12)
    cloud = _prior("dip", g, 300)
    for w in (np.zeros(300), np.full(300, np.nan), -np.ones(300)):
        o = _object("dip", cloud, LIK_COEF[1], design=(GRID,), weights=w)
        assert np.all(np.isnan(_fresh(o, 0, GRID.size)))
        o.noise_gain, o.noise_relative = np.zeros(1), np.zeros(1)            # the floor alone: still no cloud to average over
        assert np.all(np.isnan(_fresh(o, 0, GRID.size)))


@pytest.mark.parametrize("name", ["coil", "rabi", "expression"])
def test_noise_variance_other_models(hip, name):
    g = np.random.default_rng(sum(map(ord, name)) + 1)
    cloud = _prior(name, g, 4099)
    w = _weights(g, cloud)
    o = _object(name, cloud, np.ones((2 if name == "coil" else 1, 3)), weights=w)
    Y = _rows(o)
    n_s = Y.shape[0]
    for abc in _scaled_coef(Y):
        for k, v in _public(abc).items():
            setattr(o, k, v)
        want = oracle.noise_variance(Y, w, abc)
        got = _fresh(o, 0, n_s)
        assert got.shape == (o.n_channels, n_s)
        assert_allclose(got, want, rtol=1e-10, atol=0.0, err_msg=name)
        assert_array_equal(_bits(_fresh(o, 3, n_s - 2)), _bits(got[:, 3:n_s - 2]))
        assert_array_equal(_bits(o.yvar_noise_model()), _bits(got))


# ------------------------------------------------------------------------------------------------ 3. the class
class _Counting:
    """The object's model library with its calls counted by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def call(self, name, *args):
        self.calls[name] = self.calls.get(name, 0) + 1
        return self._lib.call(name, *args)

    def __getattr__(self, name):
        return getattr(self._lib, name)


def _class_case(name, n=4099, seed=0, abc=None, **kw):
    g = np.random.default_rng(seed)
    cloud = _prior(name, g, n)
    w = _weights(g, cloud)
    abc = {"dip": LIK_COEF[1], "peak": (25.0, 1.0, 0.0)}[name] if abc is None else abc
    return _object(name, cloud, abc, weights=w, **kw), cloud, w, np.atleast_2d(abc)


@pytest.mark.parametrize("name", ["dip", "peak"])
def test_update_multiplies_the_weights_by_the_likelihood(hip, name):
    o, cloud, w, abc = _class_case(name, auto_resample=False)
    x = 3.1
    y = _rows(o, [[x]])[0]
    ym = float(y[0, 17] + 0.7 * np.sqrt(oracle.nu(y[0, 17], abc)[0]))
    want = oracle.normalised(w * oracle.likelihood(y, [ym], abc, 1))
    for record in (((x,), ym), ((x,), ym, 9.9e9)):                     # a 2-tuple; a sigma that is ignored
        o.particle_weights = w
        o.pdf_update(record)
        _replay.close_weights(o.particle_weights, want, 1e-10, f"{name}: weights after pdf_update{len(record)}")
    o.particle_weights = w
    o.pdf_update(((x,), ym), y)                                        # ... and from given model values
    _replay.close_weights(o.particle_weights, want, 1e-10, f"{name}: weights after pdf_update(record, y)")
    o.particle_weights = w
    o.choke = 0.5
    o.pdf_update(((x,), ym))
    _replay.close_weights(o.particle_weights, oracle.normalised(w * oracle.likelihood(y, [ym], abc, 1, 0.5)), 1e-10,
                          f"{name}: choked weights")


@pytest.mark.parametrize("name", ["dip", "peak"])
def test_variance_full_utility_and_choice(hip, name):
    o, cloud, w, abc = _class_case(name, utility_method="variance_full")
    Y = _rows(o)
    nubar = oracle.noise_variance(Y, w, abc)
    yvar = o.yvar_from_parameter_draws()
    assert_allclose(yvar, oracle.weighted_variance(Y, w), rtol=1e-9)
    want = oracle.utility(yvar, nubar)
    top = np.sort(want)
    assert top[-1] - top[-2] > 1e-8 * top[-1]                          # the oracle alone: the choice is decided
    assert_allclose(o.yvar_noise_model(), nubar, rtol=1e-10, atol=0.0)
    t, ld = o._noise_var_device()
    assert ld == t.shape[1] == Y.shape[0]
    assert_array_equal(_bits(t.cpu().numpy()), _bits(o.yvar_noise_model()))
    assert_allclose(o.utility(), want, rtol=1e-9, atol=0.0)
    chosen = o.opt_setting()
    assert chosen == (o.allsettings[0, int(np.argmax(want))],)
    assert o.last_setting_index == int(np.argmax(want))


def test_counting_noise_moves_the_choice_on_the_peak_cloud(hip):
    """The brightest setting is the noisiest one: with nu = 25 + |y| the design leaves the setting a flat sigma = 5
    chooses on the same cloud."""
    import optbayesexpt_amd as obe
    o, cloud, w, _ = _class_case("peak", utility_method="variance_full")
    model, cons = _model("peak")
    flat = obe.OptBayesExpt(model, _design("peak"), cloud, cons, scale=False, utility_method="variance_full",
                            default_noise_std=5.0)
    flat.particle_weights = w
    assert o.opt_setting() != flat.opt_setting()


@pytest.mark.parametrize("method", ["variance_approx", "max_min", "pseudo_utility", "parameter_variance"])
def test_other_utilities_use_the_same_noise_variance(hip, method):
    """Each utility equals, bit for bit, that of a plain OptBayesExpt whose yvar_noise_model() is replaced by a
    function that returns this object's nu_bar (the per-setting override every utility already honours)."""
    import optbayesexpt_amd as obe
    o, cloud, w, abc = _class_case("peak", utility_method=method, n_draws=40)
    nubar = o.yvar_noise_model()
    assert_allclose(nubar, oracle.noise_variance(_rows(o), w, abc), rtol=1e-10, atol=0.0)
    model, cons = _model("peak")
    plain = obe.OptBayesExpt(model, _design("peak"), cloud, cons, scale=False, utility_method=method, n_draws=40)
    plain.particle_weights = w
    plain.yvar_noise_model = lambda: nubar
    o.rng, plain.rng = np.random.default_rng(5), np.random.default_rng(5)
    u = o.utility()
    assert u.shape == (o.allsettings.shape[1],) and np.all(np.isfinite(u)) and np.ptp(u) > 0
    assert_array_equal(_bits(u), _bits(plain.utility()))
    if method == "parameter_variance":
        gain = o.expected_variance_reduction()
        assert_array_equal(_bits(gain), _bits(plain.expected_variance_reduction()))
        picks = o.opt_setting_batch(3)
        assert_array_equal(picks[0], plain.opt_setting_batch(3)[0])


def test_noise_variance_is_cached_until_the_cloud_changes(hip):
    o, cloud, w, abc = _class_case("peak", utility_method="variance_full", auto_resample=False)
    o._mlib = counting = _Counting(o._mlib)
    first = o.opt_setting()
    assert counting.calls.get("obe_signal_noise_variance") == 1
    before = o.yvar_noise_model()
    assert o.opt_setting() == first and o.utility().shape == (o.allsettings.shape[1],)
    assert counting.calls["obe_signal_noise_variance"] == 1           # nothing new on an unchanged cloud
    o.pdf_update((first, 900.0))
    assert counting.calls["obe_signal_noise_likelihood"] == 1
    o.opt_setting()
    assert counting.calls["obe_signal_noise_variance"] == 2           # the weights changed
    after = o.yvar_noise_model()
    assert counting.calls["obe_signal_noise_variance"] == 2
    assert np.any(after != before)
    assert_allclose(after, oracle.noise_variance(_rows(o), o.particle_weights, abc), rtol=1e-10, atol=0.0)
    o.noise_gain = np.array([0.5])                                     # the coefficients changed
    o.opt_setting()
    assert counting.calls["obe_signal_noise_variance"] == 3
    assert o._noise_token() is None and o.sweep_state() is not None


def test_closed_loop_with_counting_noise(hip):
    """30 cycles design -> simulated counting measurement -> update on the peak cloud."""
    g = np.random.default_rng(21)
    o = _object("peak", _prior("peak", g, 20000), (25.0, 1.0, 0.0), utility_method="variance_full")
    o.rng = np.random.default_rng(22)
    true = np.array([3.02, 1200.0, 50.0])
    abc = np.array([[25.0, 1.0, 0.0]])
    chosen = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for _ in range(30):
            x = o.opt_setting()
            y = true[2] + true[1] / (((x[0] - true[0]) / 0.1) ** 2 + 1.0)
            o.pdf_update((x, y + np.sqrt(oracle.nu(np.array([y]), abc)[0]) * g.normal()))
            chosen.append(x[0])
    mean, std = o.mean(), o.std()
    assert np.all(np.isfinite(mean)) and std[0] > 0 and len(set(chosen)) > 1
    assert abs(mean[0] - true[0]) < 3.0 * std[0], (mean, std)
    assert std[0] < 0.05 / 3                                           # the prior's spread of x0 has shrunk


def test_methods_that_take_a_record_sigma_are_refused(hip):
    o, _, _, _ = _class_case("peak", n=300)
    x, y = np.array([3.0, 3.1]), np.array([900.0, 500.0])
    for call in (lambda: o.predictive_logpdf((x,), y, 5.0), lambda: o.predictive_cdf((x,), y, 5.0),
                 lambda: o.predictive_pvalue((x,), y, 5.0), lambda: o.reading_quantile(0.5, (x,), 5.0),
                 lambda: o.reading_interval(0.9, (x,), 5.0), lambda: o.records_loglik((x,), y, 5.0),
                 lambda: o.pdf_update_batch((x,), y, 5.0), lambda: o.predictive_logpdf((x,), y),
                 lambda: o.reading_quantile(0.5)):
        with pytest.raises(NotImplementedError, match="depends on the signal"):
            call()
    # what has no noise in it works unchanged
    mean, std = o.predict((x,))
    lo, hi = o.predictive_interval(0.9, (x,))
    assert mean.shape == std.shape == lo.shape == hi.shape == (1, 2) and np.all(lo <= hi)
    assert o.mean().shape == (3,) and o.covariance().shape == (3, 3)


def test_construction_checks(hip):
    import optbayesexpt_amd as obe
    model, cons = _model("coil")
    g = np.random.default_rng(1)
    cloud = _prior("coil", g, 64)
    o = obe.OptBayesExptSignalNoise(model, _design("coil"), cloud, cons, noise_floor=[1.0, 0.0], noise_gain=0.5)
    assert_array_equal(o.noise_floor, [1.0, 0.0])
    assert_array_equal(o.noise_gain, [0.5, 0.5])
    assert_array_equal(o.noise_relative, [0.0, 0.0])
    for bad in (dict(noise_gain=0.0), dict(noise_gain=-1.0), dict(noise_floor=[1.0, 2.0, 3.0]),
                dict(noise_relative=np.nan), dict(noise_floor=[1.0, 0.0], noise_gain=[1.0, 0.0])):
        with pytest.raises(ValueError):
            obe.OptBayesExptSignalNoise(model, _design("coil"), cloud, cons, **bad)
    o.noise_gain = np.array([0.0, 0.0])                               # channel 1 is left without noise
    with pytest.raises(ValueError):
        o.yvar_noise_model()
    with pytest.raises(ValueError):
        o.pdf_update(((2.0e4,), np.array([1.0, 1.0])))


def test_save_load_copy_and_pickle_continue_alike(hip, tmp_path):
    import optbayesexpt_amd as obe
    g = np.random.default_rng(31)
    o = _object("peak", _prior("peak", g, 4099), (25.0, 0.5, 1e-4), utility_method="variance_full")
    o.rng = np.random.default_rng(32)
    readings = iter(900.0 + 40.0 * g.normal(size=8))
    for _ in range(3):
        o.pdf_update((o.opt_setting(), next(readings)))
    path = os.path.join(tmp_path, "signal_noise.state")
    obe.save(o, path)
    twins = [obe.load(path), copy.deepcopy(o), pickle.loads(pickle.dumps(o))]
    reading = next(readings)
    x = o.opt_setting()
    o.pdf_update((x, reading))
    for t in twins:
        assert type(t) is obe.OptBayesExptSignalNoise
        for k in ("noise_floor", "noise_gain", "noise_relative"):
            assert_array_equal(getattr(t, k), getattr(o, k))
        assert t.opt_setting() == x
        t.pdf_update((x, reading))
        assert_array_equal(_bits(t.particle_weights), _bits(o.particle_weights))
        assert_array_equal(_bits(t.particles), _bits(o.particles))
        assert_array_equal(_bits(t.yvar_noise_model()), _bits(o.yvar_noise_model()))
    # a saved file of another class loads as before
    model, cons = _model("peak")
    plain = obe.OptBayesExpt(model, _design("peak"), _prior("peak", g, 64), cons)
    obe.save(plain, path)
    assert type(obe.load(path)) is obe.OptBayesExpt


def test_counting_noise_example(hip):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("counting_noise", os.path.join(root, "examples", "counting_noise.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        true, result = mod.main(n_measure=25, n_samples=10000, seed=3, quiet=True)
    for name in ("signal noise", "flat noise"):
        mean, std, chosen = result[name]
        assert np.all(np.isfinite(mean)) and np.all(std > 0) and chosen.shape == (25,)
    mean, std, _ = result["signal noise"]
    assert np.all(np.abs(mean - np.array(true)) < 5 * std + 1e-9), (true, mean, std)


def test_formula_model_runs_through_its_plugin(hip):
    o, cloud, w, _ = _class_case("expression", abc=(0.25, 0.5, 0.01), utility_method="variance_full", auto_resample=False)
    assert o._mlib is not o._lib                                       # the plugin serves the model's entry points
    abc = np.array([[0.25, 0.5, 0.01]])
    Y = _rows(o)
    nubar = oracle.noise_variance(Y, w, abc)
    assert_allclose(o.yvar_noise_model(), nubar, rtol=1e-10, atol=0.0)
    want = oracle.utility(o.yvar_from_parameter_draws(), nubar)
    assert_allclose(o.utility(), want, rtol=1e-9, atol=0.0)
    x = o.opt_setting()
    assert x == (o.allsettings[0, int(np.argmax(want))],)
    y = Y[o.last_setting_index]
    o.pdf_update((x, 5.5))
    _replay.close_weights(o.particle_weights, oracle.normalised(w * oracle.likelihood(y, [5.5], abc, 1)), 1e-10,
                          "expression: weights after pdf_update")
