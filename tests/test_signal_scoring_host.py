"""nu(y)-aware scoring and reading bands of OptBayesExptSignalNoise without a device: every argument check of
optbayesexpt_amd/_signal.py runs before the device is touched, the five Gaussian-named methods point at the new ones,
and the C ABI declares and binds the three entry points."""
import inspect

import numpy as np
import pytest

from optbayesexpt_amd import _lib, _signal, build, obe_signalnoise

SIG = obe_signalnoise.OptBayesExptSignalNoise
NEW_METHODS = ("signal_logpdf", "signal_cdf", "signal_pvalue", "signal_quantile", "signal_interval")
NEW_ENTRY_POINTS = ("obe_signal_noise_logpdf", "obe_signal_noise_tails", "obe_signal_noise_reading_quantiles")


def _host_object(n_channels=1, n_setdims=1):
    """An object of the class as far as the host-side checks read it; past them the call stops at the missing device
    model (TypeError), which the tests below take for 'every host check passed'."""
    o = object.__new__(SIG)
    o.n_channels = n_channels
    o.allsettings = np.zeros((n_setdims, 5))
    o.noise_floor, o.noise_gain, o.noise_relative = np.ones(n_channels), np.ones(n_channels), np.zeros(n_channels)
    o._device_model = None
    return o


def _passes_the_host_checks(call):
    with pytest.raises(TypeError, match="on the device"):
        call()


# ------------------------------------------------------------------------------------------------ the public surface
def test_the_methods_take_no_sigma():
    o = _host_object()
    for name in NEW_METHODS:
        par = inspect.signature(getattr(SIG, name)).parameters
        assert "sigma" not in par, name
    assert list(inspect.signature(SIG.signal_logpdf).parameters) == ["self", "settings", "y_meas"]
    assert list(inspect.signature(SIG.signal_cdf).parameters) == ["self", "settings", "y_meas", "upper"]
    assert list(inspect.signature(SIG.signal_pvalue).parameters) == ["self", "settings", "y_meas"]
    assert list(inspect.signature(SIG.signal_quantile).parameters) == ["self", "q", "settings", "max_passes", "full_output"]
    assert list(inspect.signature(SIG.signal_interval).parameters) == ["self", "level", "settings", "max_passes",
                                                                      "full_output"]
    assert inspect.signature(SIG.signal_quantile).parameters["max_passes"].default == 48
    assert inspect.signature(SIG.signal_interval).parameters["level"].default == 0.95
    for call in (lambda: o.signal_logpdf((1.0,), 2.0, sigma=1.0), lambda: o.signal_cdf((1.0,), 2.0, sigma=1.0),
                 lambda: o.signal_pvalue((1.0,), 2.0, sigma=1.0), lambda: o.signal_quantile(0.5, sigma=1.0),
                 lambda: o.signal_interval(0.9, sigma=1.0)):
        with pytest.raises(TypeError, match="sigma"):
            call()


def test_the_gaussian_named_methods_point_at_the_new_ones():
    o = _host_object()
    assert "depends on the signal" in SIG._REFUSAL and "yet" not in SIG._REFUSAL
    for name in NEW_METHODS:
        assert name + "()" in SIG._REFUSAL, name
    x, y = (np.array([3.0, 3.1]),), np.array([900.0, 500.0])
    for name, call in (("predictive_logpdf", lambda: o.predictive_logpdf(x, y, 5.0)),
                       ("predictive_logpdf", lambda: o.predictive_logpdf(x, y)),
                       ("predictive_cdf", lambda: o.predictive_cdf(x, y, 5.0)),
                       ("predictive_pvalue", lambda: o.predictive_pvalue(x, y)),
                       ("reading_quantile", lambda: o.reading_quantile(0.5, x, 5.0)),
                       ("reading_quantile", lambda: o.reading_quantile(0.5)),
                       ("reading_interval", lambda: o.reading_interval(0.9, x, 5.0))):
        with pytest.raises(NotImplementedError, match="depends on the signal") as err:
            call()
        assert str(err.value).startswith(name + "()") and "signal_interval()" in str(err.value)
    assert obe_signalnoise.OWN_ATTRIBUTES == frozenset()


# ------------------------------------------------------------------------------------------------ argument checks
def test_levels_lie_in_the_open_interval():
    o = _host_object()
    for bad in (0.0, 1.0, -0.1, 1.5, np.nan, (0.5, 1.0), (), [[0.5]], "half"):
        with pytest.raises(ValueError):
            o.signal_quantile(bad)
    for bad in (0.0, 1.0, -0.5, 2.0, np.nan, "most"):
        with pytest.raises(ValueError, match="level"):
            o.signal_interval(bad)
    for good in (0.5, (1e-300, 0.5, 1.0 - 1e-16), np.linspace(0.01, 0.99, 40)):
        _passes_the_host_checks(lambda: o.signal_quantile(good))
    _passes_the_host_checks(lambda: o.signal_interval(0.5))


def test_the_pass_budget_is_1_to_64():
    o = _host_object()
    for bad in (0, 65, -1, 3.0, True, "48", None):
        with pytest.raises(ValueError, match="max_passes"):
            o.signal_quantile(0.5, max_passes=bad)
        with pytest.raises(ValueError, match="max_passes"):
            o.signal_interval(0.9, None, bad)
    for good in (1, 64, np.int64(7)):
        _passes_the_host_checks(lambda: o.signal_quantile(0.5, max_passes=good))


def test_records_broadcast_to_one_number_of_records():
    one, two = _host_object(1), _host_object(2, n_setdims=2)
    _passes_the_host_checks(lambda: one.signal_logpdf((1.0,), 2.0))
    _passes_the_host_checks(lambda: one.signal_cdf((np.arange(4.0),), [1.0, 2.0, 3.0, 4.0]))
    _passes_the_host_checks(lambda: one.signal_pvalue((np.arange(4.0),), 2.0))
    _passes_the_host_checks(lambda: two.signal_logpdf((1.0, 2.0), [3.0, 4.0]))
    _passes_the_host_checks(lambda: two.signal_cdf((np.arange(3.0), 2.0), np.ones((2, 3)), upper=True))
    with pytest.raises(ValueError, match="broadcast"):
        one.signal_logpdf((np.arange(4.0),), [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="channels"):
        two.signal_cdf((1.0, 2.0), 3.0)
    with pytest.raises(ValueError, match="channels"):
        two.signal_pvalue((1.0, 2.0), [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="channels"):
        two.signal_logpdf((np.arange(3.0), 2.0), np.ones((3, 3)))
    with pytest.raises(ValueError, match="setting"):
        two.signal_logpdf((1.0,), [3.0, 4.0])
    with pytest.raises(ValueError, match="setting"):
        one.signal_quantile(0.5, (1.0, 2.0))
    with pytest.raises(ValueError, match="y_meas"):
        one.signal_logpdf((1.0,), None)
    with pytest.raises(ValueError):
        one.signal_logpdf((1.0,), np.ones((1, 0)))
    with pytest.raises(ValueError):
        one.signal_interval(0.9, (np.ones((2, 2)),))


def test_bad_coefficients_are_refused_when_the_call_starts():
    """The attributes may be reassigned between calls; what they hold is checked before anything else is read."""
    calls = (lambda o: o.signal_logpdf((1.0,), 2.0), lambda o: o.signal_cdf((1.0,), 2.0),
             lambda o: o.signal_pvalue((1.0,), 2.0), lambda o: o.signal_quantile(0.5), lambda o: o.signal_interval(0.9),
             lambda o: o.signal_logpdf("not a setting", None))           # (the coefficients come first)
    for field, bad in (("noise_gain", np.array([-1.0])), ("noise_floor", np.array([np.nan])),
                       ("noise_relative", np.array([np.inf])), ("noise_gain", np.ones(3)), ("noise_floor", "loud")):
        for call in calls:
            o = _host_object()
            setattr(o, field, bad)
            with pytest.raises(ValueError, match=field):
                call(o)
    o = _host_object(2, n_setdims=1)
    o.noise_floor, o.noise_gain = np.array([1.0, 0.0]), np.array([1.0, 0.0])      # channel 1 is left without noise
    with pytest.raises(ValueError, match="no noise at all"):
        o.signal_interval(0.9)
    o.noise_gain = np.array([1.0, 2.0])
    _passes_the_host_checks(lambda: o.signal_interval(0.9))


def test_the_module_reads_the_siblings_limits():
    from optbayesexpt_amd import _reading, _scoring
    assert _signal._scoring is _scoring and _signal._reading is _reading
    assert _scoring.RECORDS_PER_CALL == _reading.SETTINGS_PER_CALL == 1 << 16 and _reading.MAX_Q_PER_CALL == 16


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_bound_and_served_by_a_plugin():
    declared = _lib.declared_symbols()
    for name in NEW_ENTRY_POINTS:
        assert name in declared and name in _lib.PROTOTYPES and name in _lib.MODEL_ENTRY_POINTS
        assert _lib.PROTOTYPES[name][0] is _lib.c_int
    assert "obe_signal_noise.hip" in build.PLUGIN_SOURCES
    assert _lib._H["OBE_ABI_VERSION"] == 3                      # (additive)

    def swapped(sibling):
        """The sibling's parameters with h_noise_coef in place of its d_sigma, ld_sigma, h_noise_rows triple."""
        names = [p for _, p in _lib.PROTOTYPES[sibling][1]]
        at = names.index("d_sigma")
        assert names[at:at + 3] == ["d_sigma", "ld_sigma", "h_noise_rows"]
        return names[:at] + ["h_noise_coef"] + names[at + 3:]

    for name, sibling in zip(NEW_ENTRY_POINTS, ("obe_predictive_logpdf", "obe_predictive_tails",
                                                "obe_predictive_reading_quantiles")):
        params = _lib.PROTOTYPES[name][1]
        assert [p for _, p in params] == swapped(sibling), name
        types = dict((p, t) for t, p in params)
        theirs = dict((p, t) for t, p in _lib.PROTOTYPES[sibling][1])
        assert all(types[p] is theirs[p] for p in types if p != "h_noise_coef")
        assert types["h_noise_coef"] is _lib.c_void_p


def test_bad_arguments_are_refused_before_any_launch():
    """Bad pointers, bad sizes, bad levels or a bad coefficient: status -1 with the entry point's name in the message,
    on a machine without a GPU too."""
    from optbayesexpt_amd import models
    lib = _lib.load()
    m = models.lorentzian(1).struct(3, (0.1,))
    dev = 1 << 20                        # (never dereferenced: every call below is refused on its arguments)
    good = np.array([0.0, 1.0, 0.0])
    hp = _lib.host_ptr
    ws = lib.cdll.obe_predictive_score_workspace_bytes(1000, 65, 1)
    ws_q = lib.cdll.obe_predictive_reading_workspace_bytes(1000, 65, 1, 2)
    q, z = np.array([0.025, 0.975]), np.array([-1.96, 1.96])

    def logpdf(coef=good, settings=dev, ld_s=65, n_r=65, y=dev, ld_y=65, n_p=1000, ld_p=1000, out=dev, ws_bytes=ws):
        return lib.cdll.obe_signal_noise_logpdf(m, settings, ld_s, n_r, y, ld_y, None if coef is None else hp(coef), dev,
                                                ld_p, n_p, dev, out, dev, ws_bytes, None)

    def tails(coef=good, settings=dev, ld_s=65, n_r=65, y=dev, ld_y=65, n_p=1000, ld_p=1000, out=dev, ws_bytes=ws):
        return lib.cdll.obe_signal_noise_tails(m, settings, ld_s, n_r, y, ld_y, None if coef is None else hp(coef), dev,
                                               ld_p, n_p, dev, dev, out, dev, ws_bytes, None)

    def quantiles(coef=good, settings=dev, ld_s=65, n_r=65, n_p=1000, ld_p=1000, out=dev, ws_bytes=ws_q, q=q, z=z, n_q=2,
                  max_passes=48):
        return lib.cdll.obe_signal_noise_reading_quantiles(m, settings, ld_s, n_r, None if coef is None else hp(coef), dev,
                                                           ld_p, n_p, dev, hp(q), hp(z), n_q, max_passes, out, dev, dev,
                                                           ws_bytes, None)
    shared = ((dict(settings=None), "null"), (dict(out=None), "null"), (dict(n_r=0), "n_settings"),
              (dict(ld_s=64), "n_settings"), (dict(n_p=0), "cloud"), (dict(ld_p=999), "cloud"),
              (dict(ws_bytes=ws - 8), "workspace"), (dict(coef=None), "h_noise_coef"),
              (dict(coef=np.array([0.0, -1.0, 0.0])), "coefficient"), (dict(coef=np.array([np.nan, 1.0, 0.0])), "coefficient"),
              (dict(coef=np.array([0.0, np.inf, 0.0])), "coefficient"), (dict(coef=np.zeros(3)), "all zero"))
    records = ((dict(y=None), "null"), (dict(ld_y=64), "y_meas"))
    levels = ((dict(n_q=0), "levels"), (dict(n_q=17), "levels"), (dict(max_passes=0), "max_passes"),
              (dict(max_passes=65), "max_passes"), (dict(q=np.array([0.0, 0.5])), "q outside"),
              (dict(q=np.array([0.5, 1.0])), "q outside"), (dict(z=np.array([np.inf, 0.0])), "h_z"))
    for call, name, cases in ((logpdf, NEW_ENTRY_POINTS[0], shared + records), (tails, NEW_ENTRY_POINTS[1], shared + records),
                              (quantiles, NEW_ENTRY_POINTS[2], shared + levels)):
        for kw, word in cases:
            assert call(**kw) == -1, (name, kw)
            assert name in lib.last_error() and word in lib.last_error(), (name, kw, lib.last_error())
