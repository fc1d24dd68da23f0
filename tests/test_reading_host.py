"""Quantiles of the next reading, the part that needs no device: the oracle the GPU tests compare with is pinned against
SciPy and against mpmath at 50 digits, the argument checks raise before any library call, the two entry points are
declared, exported and bound, and they refuse bad arguments with status -1 and a message without touching a device."""
import math
import statistics
import types

import numpy as np
import pytest
from scipy import optimize, stats

import _reading_oracle as oracle
from optbayesexpt_amd import _lib, _reading, models

NAMES = ("obe_predictive_reading_workspace_bytes", "obe_predictive_reading_quantiles")
ARGS = ["m", "d_settings", "ld_s", "n_settings", "d_sigma", "ld_sigma", "h_noise_rows", "d_particles", "ld_p",
        "n_particles", "d_weights", "h_q", "h_z", "n_q", "max_passes", "d_quantiles", "d_passes", "d_ws", "ws_bytes",
        "stream"]
LEVELS = (1e-12, 1e-6, 0.025, 0.4999, 0.5, float(np.nextafter(0.5, 1.0)), 0.5001, 0.975, 1.0 - 1e-6, 1.0 - 1e-12)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# -------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("q", LEVELS)
def test_oracle_one_particle_is_scipys_ppf(q):
    for f, s in ((3.0, 0.5), (-50000.0, 30.0), (1e-300, 3e-300), (4e300, 1e299)):
        r = oracle.Reading([[f]], [0.7], [s])
        z = stats.norm.ppf(q) if q <= 0.5 else -stats.norm.ppf(1.0 - q)         # (ppf(q) itself rounds q's distance to 1)
        want = f + s * z
        assert abs(r.quantile(0, q) - want) <= 1e-13 * max(abs(want), s), (f, s, q, r.quantile(0, q), want)


def _mixture(g, n, per_particle):
    y = g.normal(5.0, 2.0, (1, n))
    w = g.random(n) + 1e-3
    sigma = g.uniform(0.5, 3.0, (1, n)) if per_particle else np.array([1.3])
    return y, w, sigma


@pytest.mark.parametrize("per_particle", [False, True])
@pytest.mark.parametrize("n", [1, 7, 1000])
def test_oracle_is_brentq_on_scipys_cdf_mixture(n, per_particle):
    g = np.random.default_rng([n, per_particle])
    y, w, sigma = _mixture(g, n, per_particle)
    s = np.broadcast_to(sigma.reshape(1, -1), y.shape)[0]
    r = oracle.Reading(y, w, sigma)
    for q in (1e-6, 0.025, 0.3, 0.5, 0.7, 0.975, 1.0 - 1e-6):
        lo, hi = r.bracket(0, q)
        if q <= 0.5:
            def g_(v):
                return np.sum(w * stats.norm.cdf((v - y[0]) / s)) - q * w.sum()
        else:
            def g_(v):
                return np.sum(w * stats.norm.sf((v - y[0]) / s)) - (1.0 - q) * w.sum()
        want = optimize.brentq(g_, lo - 1e-6, hi + 1e-6, xtol=1e-300, rtol=4 * oracle.EPS)
        got = r.quantile(0, q)
        assert lo <= got <= hi
        assert abs(got - want) <= 1e-12 * max(abs(want), 1.0), (n, per_particle, q, got, want)
        assert r.residual(0, q, got) <= r.tolerance(0, q, got)


MP_CASES = {
    "sigma 1": lambda g: (g.normal(0.0, 2.0, (1, 30)), g.random(30), np.ones(1)),
    "sigma 1e-150": lambda g: (1e-150 * g.normal(0.0, 2.0, (1, 30)), g.random(30), np.full(1, 1e-150)),
    "sigma 1e150": lambda g: (1e150 * g.normal(0.0, 2.0, (1, 30)), g.random(30), np.full(1, 1e150)),
    "sigma rows 1e-150 .. 1e150": lambda g: (g.normal(0.0, 1.0, (1, 31)) * 10.0 ** np.linspace(-150, 150, 31),
                                             g.random(31), 10.0 ** np.linspace(-150, 150, 31)[None, :]),
}


@pytest.mark.parametrize("q", [1e-12, 0.3, 1.0 - 1e-12])
@pytest.mark.parametrize("case", sorted(MP_CASES))
def test_oracle_against_mpmath_at_50_digits(case, q):
    """The oracle's root in mpmath's tail: |A(v) - target| is within what the last bit of v is worth, 4 eps |v| D(v)
    (brentq's rtol), plus 1e-13 of the target for the double-precision sum the root was found in."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    y, w, sigma = MP_CASES[case](np.random.default_rng(sorted(MP_CASES).index(case)))
    s = np.broadcast_to(np.asarray(sigma).reshape(1, -1), y.shape)[0]
    r = oracle.Reading(y, w, sigma)
    v = r.quantile(0, q)
    assert np.isfinite(v)
    upper = q > 0.5
    tail, dens = mp.mpf(0), mp.mpf(0)
    for i in range(y.shape[1]):
        z = (mp.mpf(v) - mp.mpf(float(y[0, i]))) / mp.mpf(float(s[i]))
        a = (z if upper else -z) / mp.sqrt(2)
        # (mpmath's erfc overflows on an argument of 1e300: beyond +-1e4 it is 0 or 2 to far more than 50 digits)
        tail += mp.mpf(float(w[i])) * (mp.erfc(a) if abs(a) < 1e4 else (0 if a > 0 else 2)) / 2
        if abs(z) < 1e4:
            dens += mp.mpf(float(w[i])) * mp.exp(-z * z / 2) / (mp.mpf(float(s[i])) * mp.sqrt(2 * mp.pi))
    target = (mp.mpf(1) - mp.mpf(q) if upper else mp.mpf(q)) * mp.fsum(mp.mpf(float(x)) for x in w)
    err = abs(tail - target)
    assert err <= mp.mpf(1e-13) * target + 4 * oracle.EPS * abs(mp.mpf(v)) * dens, (case, q, float(err / target))
    # and the oracle's own tail, target and density at that point
    assert abs(mp.mpf(r.tail(0, v, upper)) - tail) <= mp.mpf(1e-13) * tail
    assert abs(mp.mpf(r.target(0, q)[0]) - target) <= mp.mpf(1e-15) * target
    assert abs(mp.mpf(r.density(0, v)) - dens) <= mp.mpf(1e-12) * dens


def test_oracle_rules():
    g = np.random.default_rng(5)
    y, w, sigma = g.normal(5.0, 2.0, (2, 40)), g.random(40), g.uniform(0.5, 2.0, (2, 40))
    base = oracle.Reading(y, w, sigma)
    want = [[base.quantile(c, q) for q in (0.1, 0.9)] for c in range(2)]
    # zero, NaN and negative weights; a noise row <= 0 or NaN in either channel; a NaN or infinite y in the channel itself
    y2 = np.concatenate([y, [[1.0, np.nan, np.inf, 2.0, 3.0, 4.0, np.nan, -np.inf], [1.0] * 8]], axis=1)
    s2 = np.concatenate([sigma, [[1.0, 1.0, 1.0, 0.0, 1.0, np.nan, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0, -1.0, 1.0, 1.0, 1.0]]],
                        axis=1)
    w2 = np.concatenate([w, [0.0, np.nan, -2.0, 0.5, 0.5, 0.5, 0.5, 0.5]])
    more = oracle.Reading(y2, w2, s2)
    assert [more.quantile(0, q) for q in (0.1, 0.9)] == want[0]
    # channel 1 of the last two particles is finite with good rows: they contribute THERE
    assert more.total(0) == base.total(0) and abs(more.total(1) - (base.total(1) + 1.0)) < 1e-12
    assert more.quantile(1, 0.1) != want[1][0]
    # nobody contributes: NaN
    assert math.isnan(oracle.Reading(y, 0 * w, sigma).quantile(0, 0.5))
    assert math.isnan(oracle.Reading(y, w, -sigma).quantile(1, 0.5))
    assert math.isnan(oracle.Reading(np.full((1, 3), np.inf), np.ones(3), np.ones(1)).quantile(0, 0.5))
    # the target is taken in the tail where it is small
    assert base.target(0, 0.25) == (0.25 * base.total(0), False) and base.target(0, 0.75) == (0.25 * base.total(0), True)
    assert base.target(0, 0.5)[1] is False and base.target(0, float(np.nextafter(0.5, 1.0)))[1] is True


# -------------------------------------------------------------------------------------------- argument checks
def test_level_forms():
    R = _reading
    for value, size, scalar in ((0.5, 1, True), ([0.1, 0.9], 2, False), ([0.3], 1, False), (np.linspace(0.01, 0.99, 40), 40, False),
                                (5e-324, 1, True), (float(np.nextafter(1.0, 0.0)), 1, True)):
        qs, one = R.check_levels(value)
        assert qs.shape == (size,) and qs.dtype == np.float64 and one is scalar
    for bad in (0.0, 1.0, -0.1, 1.5, np.nan, [0.5, 0.0], [0.5, 1.0], [0.5, np.nan], np.full((2, 2), 0.5), [], "half", None):
        with pytest.raises(ValueError):
            R.check_levels(bad)
    z = R.normal_quantiles(np.array(LEVELS))
    nd = statistics.NormalDist()
    assert z[4] == 0.0 and z[0] == nd.inv_cdf(1e-12) and z[-1] == -nd.inv_cdf(1.0 - (1.0 - 1e-12))
    assert np.all(np.diff(z) >= 0) and abs(z[0] + z[-1]) < 1e-3 and np.all(np.isfinite(z))
    for ok in (1, 48, 64, np.int32(7)):
        assert R.check_max_passes(ok) == int(ok)
    for bad in (0, 65, -1, 2.0, True, None, "3"):
        with pytest.raises(ValueError):
            R.check_max_passes(bad)


def test_requests_broadcast_sigma_over_the_settings():
    R = _reading
    x, s = R.check_request((np.arange(4.0),), 0.5, 1, 1, None, 9)
    assert x.shape == (1, 4) and s.shape == (1, 4) and s.flags.c_contiguous and np.all(s == 0.5)
    x, s = R.check_request(None, [0.5, 2.0], 1, 2, None, 9)                       # the design grid
    assert x is None and s.shape == (2, 9) and np.all(s[1] == 2.0)
    x, s = R.check_request((np.arange(4.0),), np.arange(1.0, 5.0), 1, 1, None, 9)  # one channel: (n_x,)
    np.testing.assert_array_equal(s, [[1.0, 2.0, 3.0, 4.0]])
    x, s = R.check_request((np.arange(3.0), 1.0), np.ones((2, 3)), 2, 2, None, 9)
    assert x.shape == (2, 3) and s.shape == (2, 3)
    x, s = R.check_request((1.0,), None, 1, 2, np.array([3, 4], dtype=np.int32), 9)
    assert x.shape == (1, 1) and s is None
    bad = [((3.0,), None, 1, 1, None, 9),                                         # sigma is required on the base class
           ((3.0,), 0.1, 1, 1, np.zeros(1, dtype=np.int32), 9),                   # and refused by the noise-parameter class
           ((np.arange(4.0),), np.ones((1, 3)), 1, 1, None, 9),                   # lengths that do not broadcast
           (None, np.ones((1, 4)), 1, 1, None, 9),
           ((np.arange(4.0),), np.ones(3), 1, 1, None, 9),
           ((3.0, 1.0), 0.1, 1, 1, None, 9), ((3.0,), 0.0, 1, 1, None, 9), ((3.0,), -0.1, 1, 1, None, 9),
           ((3.0,), np.nan, 1, 1, None, 9), ((3.0,), np.inf, 1, 1, None, 9), ((3.0,), [0.1, 0.2, 0.3], 1, 2, None, 9),
           ((np.arange(3.0), np.arange(4.0)), 0.1, 2, 1, None, 9)]
    for args in bad:
        with pytest.raises(ValueError):
            R.check_request(*args)


def test_methods_check_their_arguments_before_any_library_call():
    """The two methods exist on OptBayesExpt (the noise-parameter and sweeper classes inherit them) and refuse bad
    arguments before they touch the cloud or the library: driven here on objects that have no device state at all."""
    from optbayesexpt_amd import OptBayesExpt, OptBayesExptNoiseParameter, OptBayesExptSweeper
    for cls in (OptBayesExptNoiseParameter, OptBayesExptSweeper):
        for name in ("reading_quantile", "reading_interval"):
            assert getattr(cls, name) is getattr(OptBayesExpt, name)
    base = types.SimpleNamespace(_device_model=object(), allsettings=np.zeros((1, 5)), n_channels=2)
    noise = types.SimpleNamespace(_device_model=object(), allsettings=np.zeros((1, 5)), n_channels=2,
                                  _noise_rows=np.array([3, 4], dtype=np.int32))
    quantile, interval = OptBayesExpt.reading_quantile, OptBayesExpt.reading_interval
    for obj, args, kw in ((base, (0.0,), dict(sigma=0.5)), (base, (1.0,), dict(sigma=0.5)), (base, (np.nan,), dict(sigma=0.5)),
                          (base, (np.full((2, 2), 0.5),), dict(sigma=0.5)), (base, ([0.5, 1.5],), dict(sigma=0.5)),
                          (base, (0.5,), {}),                                    # no sigma on the base class
                          (base, (0.5, (3.0,)), dict(sigma=None)),
                          (noise, (0.5,), dict(sigma=0.5)),                      # a sigma on the noise-parameter class
                          (noise, (0.5, (3.0,), [0.5, 0.5]), {}),
                          (base, (0.5,), dict(sigma=0.0)), (base, (0.5,), dict(sigma=[0.5, -1.0])),
                          (base, (0.5,), dict(sigma=[0.5, np.nan])),
                          (base, (0.5,), dict(sigma=np.ones((2, 4)))),          # the grid has five points
                          (base, (0.5, (np.arange(3.0),)), dict(sigma=np.ones((2, 4)))),
                          (base, (0.5, (3.0, 4.0)), dict(sigma=0.5)),           # two settings for a model of one
                          (base, (0.5,), dict(sigma=0.5, max_passes=0)), (base, (0.5,), dict(sigma=0.5, max_passes=65))):
        with pytest.raises(ValueError):
            quantile(obj, *args, **kw)
    for obj, args, kw in ((base, (0.0,), dict(sigma=0.5)), (base, (1.0,), dict(sigma=0.5)), (base, (np.nan,), dict(sigma=0.5)),
                          (base, ("wide",), dict(sigma=0.5)), (base, (0.9,), {}), (noise, (0.9,), dict(sigma=0.5)),
                          (base, (0.9, (np.arange(3.0),)), dict(sigma=np.ones((2, 4))))):
        with pytest.raises(ValueError):
            interval(obj, *args, **kw)
    # a host-callable model (a plain Python model_function) is refused by name, as predict() refuses it
    host = types.SimpleNamespace(_device_model=None)
    for call in (quantile, interval):
        with pytest.raises(TypeError, match="from_function.*from_expression"):
            call(host, 0.5, (3.0,), 0.5)


# ------------------------------------------------------------------------------------------ the entry points
def test_symbols_are_declared_exported_and_bound(lib):
    for name in NAMES:
        assert name in _lib.declared_symbols() and name in _lib.PROTOTYPES and name in _lib.MODEL_ENTRY_POINTS
        fn = getattr(lib.cdll, name)
        restype, params = _lib.PROTOTYPES[name]
        assert fn.restype is restype and len(fn.argtypes) == len(params)
    assert _lib.PROTOTYPES[NAMES[0]][0] is _lib.c_int64
    assert [p for _, p in _lib.PROTOTYPES[NAMES[0]][1]] == ["n_particles", "n_settings", "n_channels", "n_q"]
    assert _lib.PROTOTYPES[NAMES[1]][0] is _lib.c_int
    assert [p for _, p in _lib.PROTOTYPES[NAMES[1]][1]] == ARGS
    from optbayesexpt_amd import build
    assert "obe_predict.hip" in build.PLUGIN_SOURCES
    assert lib.cdll.obe_abi_version() == 3


def test_workspace_size_is_positive_and_does_not_shrink(lib):
    size = lib.cdll.obe_predictive_reading_workspace_bytes
    assert size(1, 1, 1, 1) > 0
    g = np.random.default_rng(8)
    for _ in range(3000):
        n, s, c, k = int(g.integers(1, 1 << 22)), int(g.integers(1, 1 << 18)), int(g.integers(1, 9)), int(g.integers(1, 17))
        base = size(n, s, c, k)
        assert base > 0
        assert size(n + int(g.integers(1, 1 << 20)), s, c, k) >= base
        assert size(n, s + int(g.integers(1, 1 << 16)), c, k) >= base
        assert size(n, s, c + 1, k) >= base
        assert size(n, s, c, k + 1) >= base
    assert size(1 << 24, 1024, 1, 2) < 1 << 24                 # per chunk, not per particle: 10 MiB for a drawn band


def test_entry_point_refuses_bad_arguments_without_a_device(lib):
    dev = 1 << 20                    # (never dereferenced: every call below is refused by its argument checks)
    c = lib.cdll
    m = models.lorentzian(1).struct(4, (0.1,))
    n, r, big = 1000, 10, 1 << 30
    rows = np.array([3, 0, 0, 0, 0, 0, 0, 0], dtype=np.int32)
    q = np.array([0.025, 0.975])
    z = _reading.normal_quantiles(q)

    def refused(rc, word):
        assert rc == -1 and word in lib.last_error(), (rc, lib.last_error())

    def call(**kw):
        a = dict(m=m, d_settings=dev, ld_s=r, n_settings=r, d_sigma=dev, ld_sigma=r, h_noise_rows=None, d_particles=dev,
                 ld_p=n, n_particles=n, d_weights=dev, h_q=_lib.host_ptr(q), h_z=_lib.host_ptr(z), n_q=2, max_passes=48,
                 d_quantiles=dev, d_passes=dev, d_ws=dev, ws_bytes=big, stream=None)
        assert list(a) == ARGS
        a.update(kw)
        return c.obe_predictive_reading_quantiles(*a.values())

    for name in ("m", "d_settings", "d_particles", "d_weights", "h_q", "h_z", "d_quantiles", "d_passes", "d_ws"):
        refused(call(**{name: None}), "null pointer")
    refused(call(d_sigma=None), "exactly one of d_sigma and h_noise_rows")                   # neither
    refused(call(h_noise_rows=_lib.host_ptr(rows)), "exactly one of d_sigma and h_noise_rows")          # both
    refused(call(n_settings=0), "n_settings < 1")
    refused(call(ld_s=r - 1), "shorter")
    refused(call(ld_sigma=r - 1), "shorter than n_records")
    refused(call(n_particles=0), "cloud size")
    refused(call(ld_p=n - 1), "cloud size")
    for bad in (-1, 4, 1 << 20):
        refused(call(d_sigma=None, h_noise_rows=_lib.host_ptr(np.array([bad] * 8, dtype=np.int32))),
                "noise row index out of range")
    for bad in (0, -1, 17):
        refused(call(n_q=bad), "1..16 levels")
    for bad in (0.0, 1.0, -0.5, 1.5, np.nan):
        refused(call(h_q=_lib.host_ptr(np.array([0.5, bad]))), "q outside (0, 1)")
    for bad in (np.nan, np.inf, -np.inf):
        refused(call(h_z=_lib.host_ptr(np.array([bad, 0.0]))), "h_z is not finite")
    for bad in (0, -3, 65):
        refused(call(max_passes=bad), "max_passes outside 1..64")
    refused(call(ws_bytes=c.obe_predictive_reading_workspace_bytes(n, r, 1, 2) - 1), "workspace too small")
    broken = models.lorentzian(1).struct(3, (0.1,))
    broken.aux = 9
    refused(call(m=broken), "aux")
    # two channels, or more levels, need more room
    coil = models.coil().struct(3, ())
    refused(call(m=coil, ws_bytes=c.obe_predictive_reading_workspace_bytes(n, r, 1, 2)), "workspace too small")
    refused(call(ws_bytes=c.obe_predictive_reading_workspace_bytes(n, r, 1, 1)), "workspace too small")
    with pytest.raises(_lib.ObeHipError) as e:
        lib.call("obe_predictive_reading_quantiles", m, dev, r, r, dev, r, None, dev, n, n, dev, _lib.host_ptr(q),
                 _lib.host_ptr(z), 2, 48, dev, dev, dev, 0, None)
    assert e.value.refused_before_launch
