"""Signal-dependent measurement noise, the parts that need no GPU: the coefficient checks of
optbayesexpt_amd/obe_signalnoise.py, the NumPy oracle (tests/_signal_noise_oracle.py) against closed forms and
against the reference Gaussian, the coefficient fields of a snapshot, and the C ABI's declarations."""
import pickle
import types

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _signal_noise_oracle as oracle
from oracle import obe_oracle
from optbayesexpt_amd import _lib, _state, build, obe_signalnoise
from optbayesexpt_amd.obe_signalnoise import check_coefficients

NEW_ENTRY_POINTS = ("obe_signal_noise_likelihood", "obe_signal_noise_workspace_bytes", "obe_signal_noise_variance")


# ------------------------------------------------------------------------------------------- coefficient checks
def test_coefficients_broadcast_and_square():
    assert_array_equal(check_coefficients(3.0, 1.0, 0.5, 1), [[9.0, 1.0, 0.25]])
    assert_array_equal(check_coefficients(0.0, 1.0, 0.0, 2), [[0.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    got = check_coefficients([1.0, 2.0], 0.5, [0.0, 0.1], 2)
    assert got.shape == (2, 3) and got.dtype == np.float64 and got.flags.c_contiguous
    assert_array_equal(got, [[1.0, 0.5, 0.0], [4.0, 0.5, 0.1 * 0.1]])
    assert_array_equal(got, oracle.coefficients([1.0, 2.0], 0.5, [0.0, 0.1], 2))
    assert_array_equal(check_coefficients(np.float64(2.0), np.array([1.0]), 0, 1), [[4.0, 1.0, 0.0]])


@pytest.mark.parametrize("args", [
    ([1.0, 2.0, 3.0], 1.0, 0.0),          # three values for two channels
    (1.0, [1.0], 0.0),                    # one value in a sequence for two channels
    (np.ones((2, 1)), 1.0, 0.0),          # two-dimensional
    (-1.0, 1.0, 0.0),                     # negative
    (0.0, [1.0, -0.5], 0.0),
    (0.0, 1.0, -1e-3),
    (np.nan, 1.0, 0.0),                   # NaN
    (0.0, [1.0, np.nan], 0.0),
    (0.0, np.inf, 0.0),                   # not finite
    (0.0, 0.0, 0.0),                      # all zero in every channel
    ([1.0, 0.0], [0.0, 0.0], [0.0, 0.0]),     # all zero in channel 1 only
    ("a", 1.0, 0.0),
])
def test_coefficients_refused(args):
    with pytest.raises(ValueError):
        check_coefficients(*args, 2)


def test_each_term_alone_is_enough():
    for k in range(3):
        args = [0.0, 0.0, 0.0]
        args[k] = 0.5
        assert np.count_nonzero(check_coefficients(*args, 3)) == 3


# ------------------------------------------------------------------------------------- the oracle, closed forms
def test_nu_closed_forms():
    coef = np.array([[4.0, 0.5, 0.01], [0.0, 1.0, 0.0]])
    y = np.array([[-10.0, 0.0, 10.0], [-9.0, 0.0, 16.0]])
    assert_array_equal(oracle.nu(y, coef), [[4.0 + 5.0 + 1.0, 4.0, 10.0], [9.0, 0.0, 16.0]])
    # per setting as well: (C, n_settings, N)
    assert oracle.nu(np.zeros((2, 5, 7)), coef).shape == (2, 5, 7)


def test_likelihood_of_one_particle_and_of_a_constant_model():
    coef = np.array([[0.0, 1.0, 0.0]])                    # Poisson: nu = |y|
    got = oracle.likelihood(np.array([[100.0]]), [110.0], coef, 1)
    assert_allclose(got, [np.exp(-100.0 / 200.0) / 10.0], rtol=1e-15)
    # a constant model: every particle the same likelihood, and the normalised weights unchanged
    y = np.full((1, 9), 64.0)
    lik = oracle.likelihood(y, [60.0], coef, 1)
    assert_array_equal(lik, np.full(9, np.exp(-16.0 / 128.0) / 8.0))
    w = np.arange(1.0, 10.0) / 45.0
    assert_allclose(oracle.normalised(w * lik), w, rtol=4e-16)
    # two channels multiply; n_lik = 1 takes the first alone
    coef2 = np.array([[0.0, 1.0, 0.0], [9.0, 0.0, 0.0]])
    y2 = np.array([[100.0, 400.0], [1.0, 2.0]])
    first = oracle.likelihood(y2, [100.0, 1.0], coef2, 1)
    assert_allclose(first, [1.0 / 10.0, np.exp(-300.0 ** 2 / 800.0) / 20.0], rtol=1e-15)
    both = oracle.likelihood(y2, [100.0, 1.0], coef2, 2)
    # (one exp of the summed exponent against a product of exps: the sum's rounding, eps / 2 of 112.6, is relative here)
    assert_allclose(both, first * [1.0 / 3.0, np.exp(-1.0 / 18.0) / 3.0], rtol=1e-13)
    # the choke is an exponent; log_likelihood is the log of the un-choked value
    assert_allclose(oracle.likelihood(y2, [100.0, 1.0], coef2, 2, choke=0.5), np.sqrt(both), rtol=4e-16)
    assert_allclose(oracle.log_likelihood(y2, [100.0, 1.0], coef2, 2), np.log(both), rtol=1e-14)


def test_likelihood_is_zero_where_nu_is_not_positive_and_finite():
    coef = np.array([[0.0, 1.0, 0.0]])
    y = np.array([[0.0, 25.0, np.inf, np.nan]])
    lik = oracle.likelihood(y, [1.0], coef, 1)
    assert_array_equal(lik[[0, 2, 3]], [0.0, 0.0, 0.0])
    assert lik[1] > 0
    assert_array_equal(oracle.log_likelihood(y, [1.0], coef, 1)[[0, 2, 3]], [-np.inf] * 3)


@pytest.mark.parametrize("floor", [0.5, 4.0, 256.0])
def test_floor_alone_is_the_reference_gaussian(floor):
    """b = c = 0: exp(-(y - ym)^2 / (2 floor^2)) / floor, the reference's _gauss_noise_likelihood with sigma = floor.
    With a power of two for the floor every scaling is exact, so both orders of operations round alike: 1e-15."""
    g = np.random.default_rng(5)
    y = g.normal(1000.0, 3.0 * floor, (2, 500))
    ym = np.array([1000.0 + floor, 1000.0 - 2.0 * floor])
    coef = oracle.coefficients(floor, 0.0, 0.0, 2)
    per_channel = [obe_oracle.gauss_likelihood(y[c], ym[c], floor) for c in range(2)]
    for c in range(2):
        got = oracle.likelihood(y[c:c + 1], ym[c:c + 1], coef[c:c + 1], 1)
        assert np.all(per_channel[c] > 0)
        assert_allclose(got, per_channel[c], rtol=1e-15, atol=0.0)
    # two channels: one exp of the summed exponent against the product of two exps.  The sum of the exponents is
    # rounded once (eps / 2 of |arg|, which the exp turns into a relative error), the two exps and the product of
    # the reference add three roundings: (|arg| + 4) eps
    arg = np.sum([((y[c] - ym[c]) / floor) ** 2 / 2 for c in range(2)], axis=0)
    got, want = oracle.likelihood(y, ym, coef, 2), per_channel[0] * per_channel[1]
    assert np.all(np.abs(got - want) <= (arg + 4.0) * 2.3e-16 * want)


def test_noise_variance_closed_forms():
    coef = np.array([[4.0, 0.5, 0.25]])
    # constant y: nu_bar = nu(y) whatever the weights
    Y = np.full((3, 1, 11), -6.0)
    w = np.random.default_rng(1).random(11)
    assert_allclose(oracle.noise_variance(Y, w, coef), np.full((1, 3), 4.0 + 3.0 + 9.0), rtol=4e-16)
    # one particle
    assert_array_equal(oracle.noise_variance(np.array([[[2.0]], [[-4.0]]]), [0.3], coef), [[6.0, 10.0]])
    # zero, NaN and negative weights count as zero, whatever the y of such a particle
    Y = np.array([[[1.0, np.nan, np.inf, 3.0, -7.0]]])
    w = np.array([1.0, 0.0, np.nan, 3.0, -2.0])
    assert_allclose(oracle.noise_variance(Y, w, coef), [[4.0 + 0.5 * (1.0 + 9.0) / 4.0 + 0.25 * (1.0 + 27.0) / 4.0]],
                    rtol=4e-16)
    # W == 0
    assert np.all(np.isnan(oracle.noise_variance(Y, np.zeros(5), coef)))
    # b = c = 0: the floor's variance at every setting
    assert_array_equal(oracle.noise_variance(np.ones((4, 1, 3)), np.ones(3), np.array([[9.0, 0.0, 0.0]])), np.full((1, 4), 9.0))


def test_utility_divides_by_the_settings_own_noise():
    yvar = np.array([[4.0, 9.0], [1.0, 1.0]])
    nubar = np.array([[2.0, 9.0], [1.0, 0.5]])
    assert_array_equal(oracle.utility(yvar, nubar, 2.0), [(2.0 + 1.0) / 2.0, (1.0 + 2.0) / 2.0])
    assert_array_equal(oracle.utility(yvar, nubar), obe_oracle.utility_from_yvar(yvar, nubar, 1.0))
    y = np.array([[[1.0, 3.0, 5.0]]])
    assert_allclose(oracle.weighted_variance(y, [1.0, 2.0, 1.0]), [[2.0]], rtol=4e-16)


# ----------------------------------------------------------------------------------------------------- the state
def test_state_fields_round_trip():
    obj = types.SimpleNamespace(noise_floor=np.array([3.0, 0.0]), noise_gain=np.array([1.0, 0.25]),
                                noise_relative=np.array([0.0, 0.01]))
    fields = obe_signalnoise.state_fields(obj)
    assert sorted(fields) == ["noise_floor", "noise_gain", "noise_relative"]
    obj.noise_gain[0] = 7.0                                # (copies: later edits of the object leave the snapshot)
    back = obe_signalnoise.kwargs_from_state(pickle.loads(pickle.dumps({"signal_noise": fields}))["signal_noise"])
    assert_array_equal(back["noise_floor"], [3.0, 0.0])
    assert_array_equal(back["noise_gain"], [1.0, 0.25])
    assert_array_equal(back["noise_relative"], [0.0, 0.01])
    assert_array_equal(check_coefficients(**back, n_channels=2), [[9.0, 1.0, 0.0], [0.0, 0.25, 1e-4]])
    # the names are the library's own attributes, not a user's: they do not travel twice
    assert set(fields) <= _state.LIBRARY_ATTRIBUTES
    from optbayesexpt_amd import OptBayesExptSignalNoise
    assert _state.library_class(type("Mine", (OptBayesExptSignalNoise,), {})) is OptBayesExptSignalNoise


def test_class_is_exported_and_needs_a_device_model():
    import optbayesexpt_amd as obe
    assert obe.OptBayesExptSignalNoise is obe_signalnoise.OptBayesExptSignalNoise
    assert issubclass(obe.OptBayesExptSignalNoise, obe.OptBayesExpt)
    with pytest.raises(ValueError, match="DeviceModel"):
        obe.OptBayesExptSignalNoise(lambda s, p, c: p[0] * s[0], (np.linspace(0, 1, 5),), np.ones((1, 8)), ())


# --------------------------------------------------------------------------------------------------- the C ABI
def test_new_entry_points_are_declared_and_served_by_plugins():
    declared = _lib.declared_symbols()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.MODEL_ENTRY_POINTS, name
        assert name in declared and name in _lib.PROTOTYPES, name
    assert set(_lib.MODEL_ENTRY_POINTS) <= set(declared)
    assert "obe_signal_noise.hip" in build.PLUGIN_SOURCES
    assert _lib.OBE_ABI_VERSION == 3
    # no host result parameters: nothing for the delivery audit to rule
    for name in NEW_ENTRY_POINTS:
        assert not [p for _, p in _lib.PROTOTYPES[name][1] if p.startswith("h_") and "out" in p]
    names = [p for _, p in _lib.PROTOTYPES["obe_signal_noise_variance"][1]]
    assert names == ["m", "d_settings", "ld_s", "n_settings", "d_particles", "ld_p", "n_particles", "d_weights",
                     "h_noise_coef", "d_noise_var", "d_ws", "ws_bytes", "stream"]


def test_bad_arguments_are_refused_before_any_launch():
    """Bad pointers, bad sizes or a bad coefficient: status -1 with a message, on a machine without a GPU too."""
    from optbayesexpt_amd import models
    lib = _lib.load()
    m = models.lorentzian(1).struct(3, (0.1,))
    dev = 1 << 20                        # (never dereferenced: every call below is refused on its arguments)
    good = np.array([0.0, 1.0, 0.0])
    ym = np.zeros(8)
    hp = _lib.host_ptr
    ws = lib.cdll.obe_signal_noise_workspace_bytes(1000, 65, 1)
    assert ws >= 8 * 3 * 64 * 2 and ws == lib.cdll.obe_signal_noise_workspace_bytes(1, 65, 1)
    assert lib.cdll.obe_signal_noise_workspace_bytes(1000, 130, 1) >= ws
    assert lib.cdll.obe_signal_noise_workspace_bytes(1000, 65, 2) > ws

    def variance(coef=good, settings=dev, ld_s=65, n_s=65, n_p=1000, ld_p=1000, ws_bytes=ws, out=dev):
        return lib.cdll.obe_signal_noise_variance(m, settings, ld_s, n_s, dev, ld_p, n_p, dev,
                                                  None if coef is None else hp(coef), out, dev, ws_bytes, None)
    for kw, word in ((dict(settings=None), "null"), (dict(out=None), "null"), (dict(n_s=0), "n_settings"),
                     (dict(ld_s=64), "n_settings"), (dict(n_p=0), "cloud"), (dict(ld_p=999), "cloud"),
                     (dict(ws_bytes=ws - 8), "workspace"), (dict(coef=None), "h_noise_coef"),
                     (dict(coef=np.array([0.0, -1.0, 0.0])), "coefficient"),
                     (dict(coef=np.array([np.nan, 1.0, 0.0])), "coefficient"),
                     (dict(coef=np.array([0.0, np.inf, 0.0])), "coefficient"),
                     (dict(coef=np.zeros(3)), "all zero")):
        assert variance(**kw) == -1, kw
        assert word in lib.last_error(), (kw, lib.last_error())

    def likelihood(coef=good, d_y=None, ld_y=0, particles=dev, ld_p=1000, n_p=1000, n_lik=1, out=dev, y_meas=ym):
        return lib.cdll.obe_signal_noise_likelihood(m, d_y, ld_y, particles, ld_p, n_p, None,
                                                    None if y_meas is None else hp(y_meas),
                                                    None if coef is None else hp(coef), n_lik, float("nan"), out, None)
    for kw in (dict(out=None), dict(y_meas=None), dict(n_p=0), dict(particles=None), dict(ld_p=999),
               dict(d_y=dev, ld_y=999), dict(n_lik=2), dict(n_lik=-1), dict(coef=None), dict(coef=np.zeros(3)),
               dict(coef=np.array([1.0, 1.0, -1.0]))):
        assert likelihood(**kw) == -1, kw
        assert "obe_signal_noise_likelihood" in lib.last_error() or "n_lik" in lib.last_error(), lib.last_error()
