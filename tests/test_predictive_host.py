"""Posterior predictive summaries, the part that needs no device: the moment oracle the GPU tests compare with is
pinned against NumPy, the argument checks raise before any library call, the three entry points are declared,
exported and bound, and they refuse bad arguments with status -1 and a message without touching a device."""
import types

import numpy as np
import pytest

import _predictive_oracle as oracle
from optbayesexpt_amd import _lib, _predictive, models


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


NAMES = ("obe_predictive_workspace_bytes", "obe_predictive_moments", "obe_predictive_quantiles")


# -------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("n", [1, 7, 64, 1000])
def test_moment_oracle_is_numpys_average_and_two_pass_variance_on_dyadic_data(n):
    """Integers y in [-16, 16] and weights k / 1024 that sum to a power of two: every product, sum and quotient of the
    two-pass form is exact in float64, so fsum, long double and NumPy must agree to the bit."""
    g = np.random.default_rng(n)
    y = g.integers(-16, 17, size=n).astype(np.float64)
    k = g.integers(0, 8, size=n)
    k[0] += 1
    k[0] += (1 << int(np.ceil(np.log2(k.sum())))) - k.sum()          # sum k = 2^m
    w = k / 1024.0
    mean = np.average(y, weights=w)
    var = np.average((y - mean) ** 2, weights=w)
    a = np.average(np.abs(y), weights=w)
    assert oracle.moments_fsum(y, w) == (mean, var, a)
    assert oracle.moments(y, w) == (mean, var, a)
    # NaN and negative weights count as zero, and what such a particle's y is does not matter
    y2 = np.concatenate([y, [np.nan, np.inf, 5.0]])
    w2 = np.concatenate([w, [0.0, np.nan, -1.0]])
    assert oracle.moments(y2, w2) == (mean, var, a) == oracle.moments_fsum(y2, w2)


def test_moment_oracle_with_general_weights_and_its_tolerances():
    g = np.random.default_rng(5)
    y = 5e4 + 30.0 * g.normal(size=20000)
    w = g.random(y.size)
    mean, var, a = oracle.moments(y, w)
    f_mean, f_var, f_a = oracle.moments_fsum(y, w)
    assert abs(mean - f_mean) <= 4e-16 * a and abs(var - f_var) <= 1e-13 * var and abs(a - f_a) <= 4e-16 * a
    assert abs(mean - np.average(y, weights=w)) <= oracle.mean_tolerance(a)
    assert oracle.var_tolerance(var, a) < 1e-9 * var                 # the floor is far below a real variance ...
    one_pass = np.average(y * y, weights=w) - np.average(y, weights=w) ** 2
    assert oracle.var_tolerance(0.0, a) < 1e-4 * 2.2e-16 * a * a     # ... and below a badly centred sum's error
    assert abs(one_pass - var) < 1e-6 * var
    # a weighted NaN or inf reaches the result
    y[3] = np.inf
    assert oracle.moments(y, w)[0] == np.inf and np.isnan(oracle.moments(y, w)[1])


# -------------------------------------------------------------------------------------------- argument checks
def test_settings_check():
    P = _predictive
    np.testing.assert_array_equal(P.check_settings((2.5,), 1), [[2.5]])
    np.testing.assert_array_equal(P.check_settings(([1, 2, 3],), 1), [[1.0, 2.0, 3.0]])
    np.testing.assert_array_equal(P.check_settings((0.5, [1, 2, 3]), 2), [[0.5, 0.5, 0.5], [1, 2, 3]])      # points
    np.testing.assert_array_equal(P.check_settings(np.arange(8.0).reshape(2, 4), 2), np.arange(8.0).reshape(2, 4))
    got = P.check_settings(np.arange(8.0).reshape(2, 4)[:, ::2], 2)
    assert got.flags.c_contiguous and got.dtype == np.float64 and got.shape == (2, 2)
    for bad, n in (((1.0, 2.0), 1), ((1.0,), 2), ((), 1), (([],), 1), (([1, 2], [1, 2, 3]), 2), ((np.zeros((2, 2)),), 1),
                   (np.zeros((2, 0)), 2), (3.0, 1), (None, 1), (("a",), 1), (np.zeros((3, 4)), 2)):
        with pytest.raises(ValueError):
            P.check_settings(bad, n)


def test_methods_check_their_arguments_before_any_library_call():
    """The three methods exist on OptBayesExpt (the noise-parameter and sweeper classes inherit them) and refuse bad
    arguments before they touch the cloud or the library: driven here on objects that have no device state at all."""
    from optbayesexpt_amd import OptBayesExpt, OptBayesExptNoiseParameter, OptBayesExptSweeper
    for cls in (OptBayesExptNoiseParameter, OptBayesExptSweeper):
        for name in ("predict", "predictive_quantile", "predictive_interval"):
            assert getattr(cls, name) is getattr(OptBayesExpt, name)
    fake = types.SimpleNamespace(_device_model=object(), allsettings=np.zeros((2, 5)))
    calls = [lambda: OptBayesExpt.predict(fake, settings=(1.0,)),
             lambda: OptBayesExpt.predict(fake, settings=([], [])),
             lambda: OptBayesExpt.predict(fake, settings=(np.zeros((2, 2)), 1.0)),
             lambda: OptBayesExpt.predictive_quantile(fake, 0.5, settings=(1.0, 2.0, 3.0)),
             lambda: OptBayesExpt.predictive_quantile(fake, 1.5),
             lambda: OptBayesExpt.predictive_quantile(fake, []),
             lambda: OptBayesExpt.predictive_interval(fake, level=2.0),
             lambda: OptBayesExpt.predictive_interval(fake, level="wide"),
             lambda: OptBayesExpt.predictive_interval(fake, 0.9, settings=np.zeros((2, 0)))]
    for k, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
    # a host-callable model (a plain Python model_function) is refused by name, whatever the other arguments
    host = types.SimpleNamespace(_device_model=None)
    for call in (lambda: OptBayesExpt.predict(host), lambda: OptBayesExpt.predictive_quantile(host, 0.5),
                 lambda: OptBayesExpt.predictive_interval(host, 0.9, settings=(1.0,))):
        with pytest.raises(TypeError, match="from_function.*from_expression"):
            call()


# ------------------------------------------------------------------------------------------ the entry points
def test_symbols_are_declared_exported_and_bound(lib):
    for name in NAMES:
        assert name in _lib.declared_symbols() and name in _lib.PROTOTYPES and name in _lib.MODEL_ENTRY_POINTS
        fn = getattr(lib.cdll, name)
        restype, params = _lib.PROTOTYPES[name]
        assert fn.restype is restype and len(fn.argtypes) == len(params)
    assert _lib.PROTOTYPES[NAMES[0]][0] is _lib.c_int64
    assert [p for _, p in _lib.PROTOTYPES[NAMES[1]][1]] == [
        "m", "d_settings", "ld_s", "n_settings", "d_particles", "ld_p", "n_particles", "d_weights", "d_mean", "d_var",
        "d_ws", "ws_bytes", "stream"]
    assert [p for _, p in _lib.PROTOTYPES[NAMES[2]][1]] == [
        "m", "d_settings", "ld_s", "n_settings", "d_particles", "ld_p", "n_particles", "d_weights", "h_q", "n_q",
        "d_quantiles", "d_ws", "ws_bytes", "stream"]
    from optbayesexpt_amd import build
    assert "obe_predict.hip" in build.PLUGIN_SOURCES
    assert lib.cdll.obe_abi_version() == 3


def test_workspace_size_is_positive_and_does_not_shrink(lib):
    size = lib.cdll.obe_predictive_workspace_bytes
    assert size(1, 1, 1, 0) > 0
    g = np.random.default_rng(8)
    for _ in range(3000):
        n, s = int(g.integers(1, 1 << 22)), int(g.integers(1, 1 << 18))
        c, q = int(g.integers(1, 9)), int(g.integers(0, 17))
        base = size(n, s, c, q)
        assert base > 0
        assert size(n + int(g.integers(1, 1 << 20)), s, c, q) >= base
        assert size(n, s + int(g.integers(1, 1 << 16)), c, q) >= base
        assert size(n, s, c + 1, q) >= base
        assert size(n, s, c, min(q + 1, 16)) >= base
    # the quantiles keep the model values of up to 64 (setting, channel) rows, and 2 KiB per (row, q)
    assert size(1 << 20, 100, 2, 3) >= 64 * (1 << 20) * 8 + 64 * 3 * 256 * 8
    assert size(1 << 20, 1 << 16, 2, 3) == size(1 << 20, 100, 2, 3)          # whatever the number of settings


def test_entry_points_refuse_bad_arguments_without_a_device(lib):
    dev = 1 << 20                    # (never dereferenced: every call below is refused by its argument checks)
    c = lib.cdll
    m = models.lorentzian(1).struct(3, (0.1,))
    n, s, big = 1000, 10, 1 << 30
    q = np.array([0.025, 0.975])
    Q = _lib.host_ptr(q)

    def refused(rc, word):
        assert rc == -1 and word in lib.last_error(), (rc, lib.last_error())

    def mom(**kw):
        a = dict(m=m, d_settings=dev, ld_s=s, n_settings=s, d_particles=dev, ld_p=n, n_particles=n, d_weights=dev,
                 d_mean=dev, d_var=dev, d_ws=dev, ws_bytes=big, stream=None)
        a.update(kw)
        return c.obe_predictive_moments(*a.values())

    def qua(**kw):
        a = dict(m=m, d_settings=dev, ld_s=s, n_settings=s, d_particles=dev, ld_p=n, n_particles=n, d_weights=dev,
                 h_q=Q, n_q=2, d_quantiles=dev, d_ws=dev, ws_bytes=big, stream=None)
        a.update(kw)
        return c.obe_predictive_quantiles(*a.values())

    for name in ("m", "d_settings", "d_particles", "d_weights", "d_mean", "d_var", "d_ws"):
        refused(mom(**{name: None}), "null pointer")
    for name in ("m", "d_settings", "d_particles", "d_weights", "h_q", "d_quantiles", "d_ws"):
        refused(qua(**{name: None}), "null pointer")
    for call in (mom, qua):
        refused(call(n_settings=0), "n_settings < 1")
        refused(call(n_settings=-5), "n_settings < 1")
        refused(call(ld_s=s - 1), "n_settings")
        refused(call(n_particles=0), "cloud size")
        refused(call(ld_p=n - 1), "cloud size")
    refused(qua(n_q=0), "quantiles per call")
    refused(qua(n_q=17, h_q=_lib.host_ptr(np.full(17, 0.5))), "quantiles per call")
    for bad in (-0.1, 1.5, float("nan")):
        refused(qua(h_q=_lib.host_ptr(np.array([0.5, bad]))), "outside [0, 1]")
    refused(mom(ws_bytes=c.obe_predictive_workspace_bytes(n, s, 1, 0) - 1), "workspace too small")
    refused(qua(ws_bytes=c.obe_predictive_workspace_bytes(n, s, 1, 2) - 1), "workspace too small")
    # the model is validated as everywhere
    bad = models.lorentzian(1).struct(3, (0.1,))
    bad.aux = 9
    refused(mom(m=bad), "aux")
    # two channels need twice the histograms
    coil = models.coil().struct(3, ())
    refused(mom(m=coil, ws_bytes=c.obe_predictive_workspace_bytes(n, s, 1, 0)), "workspace too small")
    refused(qua(m=coil, ws_bytes=c.obe_predictive_workspace_bytes(n, 1, 1, 2)), "workspace too small")
    with pytest.raises(_lib.ObeHipError) as e:
        lib.call("obe_predictive_quantiles", m, dev, s, s, dev, n, n, dev, Q, 2, dev, dev, 0, None)
    assert e.value.refused_before_launch
