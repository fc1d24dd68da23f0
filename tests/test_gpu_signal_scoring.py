"""nu(y)-aware scoring and reading bands of OptBayesExptSignalNoise (signal_logpdf / signal_cdf / signal_pvalue /
signal_quantile / signal_interval; csrc/obe_signal_noise.hip, K21) against the oracles of their Gaussian siblings,
tests/_scoring_oracle.py and tests/_reading_oracle.py, fed a sigma row per particle: sigma = sqrt(nu(y)) with
y = eval_over_all_parameters((x,)) of the product itself and nu from tests/_signal_noise_oracle.py, and NaN in EVERY
channel of a particle whose nu is not > 0 or not finite in ANY channel (the contribution rule of include/obe_hip.h).

Tolerances are the siblings': |d log p| <= logpdf_tolerance; each tail 1e-10 relative where the oracle has it > 0 and
exactly the oracle's 0 or NaN elsewhere ("plain" records have both oracle tails > 1e-280, asserted from the oracle alone
before the device is asked); |A(v) - target| <= Reading.tolerance(c, q, v) for a quantile v.  Run to run: the same bits.
The worst error / tolerance ratios seen are printed by test_worst_errors_are_reported."""
import copy
import importlib.util
import math
import os
import pickle
import warnings

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _expr_models
import _fn_models
import _own_records_models
import _reading_oracle as reading
import _scoring_oracle as scoring
import _signal_noise_oracle as sn
from optbayesexpt_amd import _reading, _scoring

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = (1 << 17) + 3
WORST = {"passes": (0, "")}
HALF_UP = float(np.nextafter(0.5, 1.0))
EDGES = (1e-12, 0.5, HALF_UP, 1.0 - 1e-12)
FIVE = (1e-12, 0.3, 0.5, HALF_UP, 1.0 - 1e-12)
BAND = (0.025, 0.975)
LD = np.longdouble


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
    if name == "expression":
        return m.from_expression("b + a / (x * x + 1)", settings=("x",), parameters=("a", "b")), ()
    if name == "function":
        return m.from_function(_fn_models.lorentzian), (0.1,)
    if name == "row":                                        # the output is the parameter row itself
        return _own_records_models.expression_models()["row"], ()
    if name == "wide":                                       # five channels; at x = 0 channel c is the row p[4 c]
        return _expr_models.expression_models()["wide"], ()
    raise KeyError(name)


def _prior(name, g, n):
    if name in ("lorentz1", "function"):
        return np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    if name == "lorentz7":
        return np.vstack([g.uniform(2, 4, (7, n)), g.uniform(400, 2000, (1, n)), g.normal(500, 1000, (1, n)),
                          g.exponential(500, (1, n))])
    if name == "coil":
        return np.array([g.normal(1e-3, 1e-4, n), g.normal(10.0, 1.0, n), g.normal(1e-6, 1e-7, n)])
    if name == "rabi":
        return np.array([g.uniform(0.5, 2.0, n), g.uniform(-3.0, 3.0, n)])
    if name == "expression":
        return np.array([g.normal(0.0, 2.0, n), g.normal(5.0, 1.0, n)])
    raise KeyError(name)


def _points(name, g, n_x):
    if name == "coil":
        return g.uniform(1.0e4, 6.0e4, n_x)[None, :]
    if name == "rabi":
        return np.array([g.uniform(0.0, 3.0, n_x), g.uniform(-4.0, 4.0, n_x)])
    if name == "expression":
        return g.uniform(-3.0, 3.0, n_x)[None, :]
    if name in ("row", "wide"):
        return np.zeros((1, n_x))
    return g.uniform(1.5, 4.5, n_x)[None, :]


def _design(name):
    if name == "rabi":
        return (np.linspace(0.0, 3.0, 5), np.linspace(-4.0, 4.0, 7))
    if name == "coil":
        return (np.linspace(1.0e4, 6.0e4, 33),)
    if name in ("row", "wide"):
        return (np.linspace(0.0, 1.0, 3),)
    return (np.linspace(1.5, 4.5, 33),)


def _object(name, cloud, noise, weights=None, **kw):
    """``noise``: (noise_floor, noise_gain, noise_relative), scalars or one value per channel."""
    import optbayesexpt_amd as obe
    model, cons = _model(name)
    kw.setdefault("scale", False)
    o = obe.OptBayesExptSignalNoise(model, _design(name), cloud, cons, noise_floor=noise[0], noise_gain=noise[1],
                                    noise_relative=noise[2], **kw)
    if weights is not None:
        o.particle_weights = weights
    return o


def _rows(o, x):
    """y (n_x, C, N_p): the product's own model values, one setting at a time."""
    return np.stack([np.asarray(o.eval_over_all_parameters(tuple(float(v) for v in x[:, r]))).reshape(o.n_channels, -1)
                     for r in range(x.shape[1])])


def _weights(g, cloud):
    w = g.random(cloud.shape[1]) * np.exp(-0.5 * ((cloud[0] - np.median(cloud[0])) / (np.std(cloud[0]) + 1e-300)) ** 2)
    return w / w.sum()


def _sigma_rows(y, coef):
    """sigma (n_x, C, N_p) = sqrt(nu(y)), NaN in every channel of a particle whose nu is not > 0 or not finite in any."""
    out = np.empty_like(y)
    for r in range(y.shape[0]):
        nu = sn.nu(y[r], coef)
        with np.errstate(invalid="ignore"):
            bad = ~np.all((nu > 0.0) & np.isfinite(nu), axis=0)
            out[r] = np.sqrt(nu)
        out[r][:, bad] = np.nan
    return out


def _noise_sets(y):
    """Coefficient sets (floor, gain, relative) per channel on the scale s of the model values' own spread: a floor of
    s alone, then a floor of s / 2 with counting noise, with relative noise and with both (test_gpu_signal_noise's)."""
    n_c = y.shape[1]
    s = np.array([np.median(np.std(y[:, c], axis=1)) for c in range(n_c)]) + 1e-3 * np.median(np.abs(y[:, :, 0]), axis=0) \
        + 1e-300
    mag = np.array([np.median(np.abs(y[:, c])) + 1e-300 for c in range(n_c)])
    zero = np.zeros(n_c)
    return {"floor": (s, zero, zero), "floor+gain": (s / 2, 0.75 * s * s / mag, zero),
            "floor+relative": (s / 2, zero, np.sqrt(0.75) * s / mag), "all three": (s / 2, 0.5 * s * s / mag, 0.5 * s / mag)}


def _readings(g, y, w, sig):
    """Readings (C, n_r) within a few of its own sigma of a weighted, contributing particle's model value."""
    n_r, n_c, _ = y.shape
    ym = np.empty((n_c, n_r))
    for r in range(n_r):
        with np.errstate(invalid="ignore"):
            heavy = np.nonzero((w > 0) & np.all(sig[r] > 0, axis=0))[0]
        i = heavy[g.integers(0, heavy.size)]
        ym[:, r] = y[r, :, i] + sig[r, :, i] * g.normal(0.0, 1.5, n_c)
    return ym


# ------------------------------------------------------------------------------------------------- the checks
def _note(kind, err, tol, what):
    ratio = err / tol if tol > 0 else (0.0 if err == 0 else np.inf)
    if ratio >= WORST.get(kind, (0.0, ""))[0]:
        WORST[kind] = ratio, what


def _check_scores(what, o, x, ym, y, w, plain_tails=True, records=None, sig=None):
    """The three scoring methods for the records (x, ym) against the scoring oracle fed y (n_r, C, N_p) and sigma rows
    (``sig``; None: sqrt(nu(y)) of the object's coefficients)."""
    n_r, n_c = y.shape[0], y.shape[1]
    sig = _sigma_rows(y, o._coefficients()) if sig is None else sig
    want = []
    for r in (range(n_r) if records is None else records):
        lo, hi = scoring.tails(y[r], w, ym[:, r], sig[r])
        if plain_tails:
            assert np.all(lo > 1e-280) and np.all(hi > 1e-280), (what, r, lo, hi)       # the choice of records: CPU only
        want.append((r, scoring.logpdf(y[r], w, ym[:, r], sig[r]), lo, hi))
    logp = o.signal_logpdf(x, ym)
    lower = o.signal_cdf(x, ym)
    upper = o.signal_cdf(x, ym, upper=True)
    p = o.signal_pvalue(x, ym)
    assert logp.shape == (x.shape[1],) and lower.shape == upper.shape == p.shape == (n_c, x.shape[1])
    assert logp.dtype == lower.dtype == upper.dtype == p.dtype == np.float64
    assert_array_equal(_bits(p), _bits(np.minimum(2.0 * np.minimum(lower, upper), 1.0)), err_msg=f"{what}: p-value")
    assert_array_equal(_bits(o.signal_logpdf(x, ym)), _bits(logp), err_msg=f"{what}: run to run")
    assert_array_equal(_bits(o.signal_cdf(x, ym)), _bits(lower), err_msg=f"{what}: run to run")
    assert_array_equal(_bits(o.signal_cdf(x, ym, upper=True)), _bits(upper), err_msg=f"{what}: run to run")
    for r, lp, lo, hi in want:
        if np.isfinite(lp):
            err, tol = abs(logp[r] - lp), scoring.logpdf_tolerance(lp)
            _note("log p", err, tol, what)
            assert err <= tol, f"{what}: log p of record {r}: {logp[r]!r} vs {lp!r}, error {err:.3g} > {tol:.3g}"
        else:
            assert_array_equal(logp[r], lp, err_msg=f"{what}: log p of record {r}")
        for kind, got, ref in (("lower", lower[:, r], lo), ("upper", upper[:, r], hi)):
            for c in range(n_c):
                if ref[c] > 0:
                    err, tol = abs(got[c] - ref[c]), 1e-10 * ref[c]
                    _note("tail", err, tol, what)
                    assert err <= tol, f"{what}: {kind} tail of record {r}, channel {c}: {got[c]!r} vs {ref[c]!r}"
                else:
                    assert_array_equal(got[c], ref[c], err_msg=f"{what}: {kind} tail of record {r}, channel {c}")
    return logp, lower, upper


def _check_quantiles(what, o, x, qs, y, w, settings=None, sig=None, **kw):
    """signal_quantile for the levels ``qs`` at the points ``x`` against the reading oracle fed y (n_x, C, N_p) and sigma
    rows.  Returns (quantiles, passes)."""
    qs = np.atleast_1d(np.asarray(qs, dtype=np.float64))
    sig = _sigma_rows(y, o._coefficients()) if sig is None else sig
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                                     # (an open row would warn)
        out, info = o.signal_quantile(qs, x, full_output=True, **kw)
        again = o.signal_quantile(qs, x, **kw)
    n_c = y.shape[1]
    assert out.shape == (qs.size, n_c, x.shape[1]) and out.dtype == np.float64
    assert info["passes"].shape == out.shape and info["passes"].dtype == np.int32
    assert info["unconverged"] == 0 and np.all(info["passes"] >= 1), (what, info["unconverged"], info["passes"].min())
    assert_array_equal(_bits(again), _bits(out), err_msg=f"{what}: run to run")
    for r in (range(x.shape[1]) if settings is None else settings):
        mix = reading.Reading(y[r], w, sig[r])
        for c in range(n_c):
            for j, q in enumerate(qs):
                v = float(out[j, c, r])
                assert np.isfinite(v), (what, r, c, q)
                res, tol = mix.residual(c, float(q), v), mix.tolerance(c, float(q), v)
                _note("quantile", res, tol, what)
                assert res <= tol, f"{what}: setting {r}, channel {c}, q {q!r}: {v!r}, residual {res:.3g} > {tol:.3g}"
    top = int(info["passes"].max())
    if top >= WORST["passes"][0]:
        WORST["passes"] = top, what
    return out, info["passes"]


def _check_all(what, o, x, y, w, g, qs=BAND, **kw):
    sig = _sigma_rows(y, o._coefficients())
    _check_scores(what, o, x, _readings(g, y, w, sig), y, w, sig=sig, **kw)
    return _check_quantiles(what, o, x, qs, y, w, sig=sig)


def _case(name, seed, n, n_x, noise="all three"):
    g = np.random.default_rng(seed)
    cloud = _prior(name, g, n)
    w = _weights(g, cloud) if n > 1 else np.ones(1)
    x = _points(name, g, n_x)
    o = _object(name, cloud, (1.0, 0.0, 0.0), w)
    y = _rows(o, x)
    for field, value in zip(("noise_floor", "noise_gain", "noise_relative"), _noise_sets(y)[noise]):
        setattr(o, field, value)
    return g, o, x, y, w


# ------------------------------------------------------------------------- 1. shapes: settings x particles x levels
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, (1 << 14) + 3])
def test_shapes_lorentzian(hip, n):
    """Both sides of the wave of 64 records or settings and of the chunk of 256 particles; one particle; 65 chunks."""
    for n_x in (1, 63, 64, 65, 130):
        g, o, x, y, w = _case("lorentz1", [n, n_x], n, n_x)
        _check_all(f"lorentz1 {n_x} x {n}", o, x, y, w, g)


def test_seventy_settings_at_131075_particles(hip):
    """70 settings x 2^17 + 3 particles: seven different settings against the oracles, each repeated in ten lanes of
    two waves, which must all hold the same bits."""
    g, o, x7, y7, w = _case("lorentz1", 70, BIG, 7)
    sig7 = _sigma_rows(y7, o._coefficients())
    ym7 = _readings(g, y7, w, sig7)
    x, ym = np.tile(x7, 10), np.tile(ym7, 10)
    logp, lower, upper = _check_scores("lorentz1 70 x BIG", o, x, ym, y7, w, records=range(7), sig=sig7)
    assert_array_equal(_bits(logp), _bits(np.tile(logp[:7], 10)))
    assert_array_equal(_bits(lower), _bits(np.tile(lower[:, :7], 10)))
    assert_array_equal(_bits(upper), _bits(np.tile(upper[:, :7], 10)))
    out, passes = _check_quantiles("lorentz1 70 x BIG", o, x, BAND, y7, w, settings=range(7), sig=sig7)
    assert_array_equal(_bits(out), _bits(np.tile(out[:, :, :7], 10)))
    assert_array_equal(passes, np.tile(passes[:, :, :7], 10))


@pytest.mark.parametrize("n_q", [1, 2, 5, 16, 17])
def test_level_counts(hip, n_q):
    """One level, two, five (a group of eight is not full), sixteen (two groups of a call) and seventeen (two calls),
    the far tails, the median and the float just above it among them; every level's result is the bits of a call of its
    own."""
    g, o, x, y, w = _case("lorentz1", n_q, 300, 3)
    qs = {1: (HALF_UP,), 2: (1e-12, 1.0 - 1e-12), 5: FIVE}.get(n_q)
    if qs is None:
        qs = tuple(np.sort(np.concatenate([EDGES, np.linspace(0.02, 0.97, n_q - 4)])))
    assert len(set(qs)) == n_q
    out, passes = _check_quantiles(f"{n_q} levels", o, x, qs, y, w)
    for j, q in enumerate(qs):
        alone, info = o.signal_quantile(q, x, full_output=True)
        assert alone.shape == (1, 3)                                         # a scalar q: no level axis
        assert_array_equal(_bits(alone), _bits(out[j]), err_msg=f"level {q!r} of {n_q}")
        assert_array_equal(info["passes"], passes[j])
    apart = [j for j, q in enumerate(qs) if q != HALF_UP or 0.5 not in qs]
    if len(apart) > 1:
        assert np.all(np.diff(out[apart], axis=0) > 0.0)


# ------------------------------------------------------------------------------- 2. models and coefficient sets
@pytest.mark.parametrize("name", ["lorentz7", "coil", "rabi", "expression", "function"])
def test_models(hip, name):
    """Every set keeps a floor here: an output that crosses zero (the coil's reactance at resonance) would otherwise have
    particles of vanishing nu."""
    for (n, n_x), noise in zip(((5000, 65), (300, 3)), ("all three", "floor+gain")):
        g, o, x, y, w = _case(name, [sum(map(ord, name)), n], n, n_x, noise)
        assert (o._mlib is not o._lib) == (name in ("expression", "function"))          # plugins serve their own model
        assert y.shape[1] == (2 if name == "coil" else 1) and x.shape[0] == (2 if name == "rabi" else 1)
        _check_all(f"{name} {n_x} x {n} {noise}", o, x, y, w, g, FIVE if n == 300 else BAND)


@pytest.mark.parametrize("noise", ["gain", "relative", "all three", "floor+relative"])
def test_coefficient_sets_lorentzian(hip, noise):
    """Gain only and relative only on the Lorentzian dip, whose values stay near 50 000 (nu never vanishes)."""
    g, o, x, y, w = _case("lorentz1", [7, len(noise)], 3000, 9)
    if noise == "gain":
        o.noise_floor, o.noise_gain, o.noise_relative = np.zeros(1), np.array([4.0]), np.zeros(1)
    elif noise == "relative":
        o.noise_floor, o.noise_gain, o.noise_relative = np.zeros(1), np.zeros(1), np.array([0.01])
    else:
        o.noise_floor, o.noise_gain, o.noise_relative = _noise_sets(y)[noise]
    _check_all(f"lorentz1 {noise} only", o, x, y, w, g, FIVE)


def test_coefficients_per_channel(hip):
    """A different mix in each channel of the coil: a floor alone in one, all three in the other."""
    g, o, x, y, w = _case("coil", 12, 2000, 11)
    sets = _noise_sets(y)
    for field, k in zip(("noise_floor", "noise_gain", "noise_relative"), range(3)):
        setattr(o, field, np.array([sets["floor"][k][0], sets["all three"][k][1]]))
    coef = o._coefficients()
    assert coef[0, 1] == 0.0 and coef[0, 2] == 0.0 and np.all(coef[1] > 0.0)
    _check_all("coil, per-channel coefficients", o, x, y, w, g, FIVE)


def test_a_floor_alone_agrees_with_the_base_class(hip):
    """noise_floor alone: the base class's answers at sigma = noise_floor.  "Agree to the same tolerances" is meant
    through the shared oracle: both classes are held to the Gaussian oracle at that sigma with the siblings' tolerances,
    so density and tails of the two differ by at most twice the tolerance (asserted directly below), and the quantiles
    of both satisfy the same residual bound |A(v) - target| <= Reading.tolerance — a bound on the tail at v, not on v,
    which is why the two classes' quantiles are not subtracted from one another."""
    import optbayesexpt_amd as obe
    g = np.random.default_rng(13)
    cloud = _prior("coil", g, 3000)
    w = _weights(g, cloud)
    x = _points("coil", g, 9)
    model, cons = _model("coil")
    base = obe.OptBayesExpt(model, _design("coil"), cloud, cons, scale=False)
    base.particle_weights = w
    y = _rows(base, x)
    floor = _noise_sets(y)["floor"][0]
    o = _object("coil", cloud, (floor, 0.0, 0.0), w)
    sig = np.broadcast_to(floor[None, :, None], y.shape)                     # the base class's sigma, not sqrt(floor^2)
    ym = _readings(g, y, w, sig)
    logp, lower, upper = _check_scores("floor alone", o, x, ym, y, w, sig=sig)
    out, _ = _check_quantiles("floor alone", o, x, FIVE, y, w, sig=sig)
    sigma = np.broadcast_to(floor[:, None], (2, 9))
    for r in range(9):
        tol = 2.0 * scoring.logpdf_tolerance(logp[r])
        assert abs(base.predictive_logpdf(x, ym, sigma)[r] - logp[r]) <= tol
    assert np.all(np.abs(base.predictive_cdf(x, ym, sigma) - lower) <= 2e-10 * lower)
    assert np.all(np.abs(base.predictive_cdf(x, ym, sigma, upper=True) - upper) <= 2e-10 * upper)
    ref = base.reading_quantile(FIVE, x, sigma)
    for r in range(9):
        mix = reading.Reading(y[r], w, floor)
        for c in range(2):
            for j, q in enumerate(FIVE):
                assert mix.residual(c, q, ref[j, c, r]) <= mix.tolerance(c, q, ref[j, c, r])


# ----------------------------------------------------------------------------------- 3. crafted values (row model)
CHUNKED = 1000                                               # 4 chunks of 256: particles 0 | 511 | 768 | 999
PLACES = {"first": 0, "last of a middle chunk": 511, "first of the last chunk": 768, "last": CHUNKED - 1}


def _row_case(seed, noise, n=CHUNKED):
    g = np.random.default_rng(seed)
    cloud = g.uniform(50.0, 150.0, (1, n))
    w = g.random(n) + 0.1
    return g, cloud, w / w.sum(), noise


def _row_check(what, cloud, w, noise, g, n_x=3):
    o = _object("row", cloud, noise, w)
    x = _points("row", g, n_x)
    y = _rows(o, x)
    assert_array_equal(_bits(y[0, 0]), _bits(cloud[0]))                      # the model value IS the parameter row
    sig = _sigma_rows(y, o._coefficients())
    ym = _readings(g, y, w, sig)
    got = _check_scores(what, o, x, ym, y, w, plain_tails=False, sig=sig)
    return got, _check_quantiles(what, o, x, BAND, y, w, sig=sig), (o, x, ym)


@pytest.mark.parametrize("place", list(PLACES))
def test_values_and_weights_that_do_not_contribute(hip, place):
    """NaN, +inf, -inf, a value whose square overflows, a value of vanishing nu, and a zero, NaN or negative weight — one
    at a time at the given place of the cloud, with a weight that would move every answer if it were counted."""
    at = PLACES[place]
    gain, mixed = (0.0, 1.0, 0.0), (3.0, 1.0, 0.05)
    for k, (value, weight, noise) in enumerate(((np.nan, 0.3, mixed), (np.inf, 0.3, mixed), (-np.inf, 0.3, mixed),
                                                (1e200, 0.3, mixed), (1e200, 0.3, gain), (0.0, 0.3, gain),
                                                (100.0, 0.0, mixed), (1e6, np.nan, mixed), (1e6, -1.0, mixed))):
        g, cloud, w, _ = _row_case([at, k], noise)
        cloud[0, at], w[at] = value, weight
        (logp, lower, upper), (out, _), (o, x, ym) = _row_check(f"{value!r} / w {weight!r} {place}", cloud, w, noise, g)
        assert np.all(np.isfinite(logp)) and np.all(np.isfinite(out))
        # left out of the tails and the band, but (a weight > 0) counted in the normaliser of the density and the tails
        keep = np.ones(cloud.shape[1], dtype=bool)
        keep[at] = False
        if at == cloud.shape[1] - 1:                         # (the same chunks without it: the band's very bits)
            assert_array_equal(_bits(_object("row", cloud[:, keep], noise, w[keep]).signal_quantile(BAND, x)), _bits(out))
        share = math.fsum(w[keep]) / math.fsum(scoring.clean(w))
        assert np.all(np.abs(lower + upper - share) <= 1e-9)                 # (a continuous mixture: the tails sum to it)


def test_a_vanishing_nu_in_one_channel_leaves_the_particle_out_of_all(hip):
    """Five channels (the `wide` cubic at x = 0: channel c is the row p[4 c]); channel 2 has counting noise alone, so a
    model value of 0 there has nu = 0; a NaN in channel 4.  Either removes the particle from EVERY channel."""
    g = np.random.default_rng(40)
    n = 600
    cloud = np.zeros((20, n))
    cloud[::4] = g.uniform(50.0, 150.0, (5, n))
    w = g.random(n) + 0.1
    cloud[8, [0, 255, 256, 599]] = 0.0
    cloud[16, [1, 300]] = np.nan
    cloud[0, [0, 1]] = 1e4                                   # (their channel-0 values would move channel 0's band)
    w[[0, 1, 255]] = 20.0
    w /= w.sum()
    noise = (np.array([3.0, 2.0, 0.0, 1.0, 5.0]), np.array([0.0, 1.0, 1.0, 0.0, 0.5]), np.array([0.0, 0.0, 0.0, 0.1, 0.02]))
    o = _object("wide", cloud, noise, w)
    x = _points("wide", g, 2)
    y = _rows(o, x)
    assert_array_equal(_bits(y[0]), _bits(cloud[::4]))
    sig = _sigma_rows(y, o._coefficients())
    assert np.all(np.isnan(sig[0][:, [0, 1, 255, 256, 300, 599]])) and np.isfinite(sig[0][:, 2:255]).all()
    ym = _readings(g, y, w, sig)
    _check_scores("wide, nu = 0 in one channel", o, x, ym, y, w, sig=sig)
    out, _ = _check_quantiles("wide, nu = 0 in one channel", o, x, FIVE, y, w, sig=sig)
    assert np.all(out[:, 0] < 1e3)                           # the particles at 1e4 in channel 0 are gone from its band


def test_nobody_contributing_and_no_weight_at_all(hip):
    g, cloud, w, noise = _row_case(41, (3.0, 1.0, 0.05), n=300)
    x, ym = np.zeros((1, 4)), np.full(4, 100.0)
    bad = cloud.copy()
    bad[0, :100], bad[0, 100:200], bad[0, 200:] = np.nan, np.inf, -1e200
    o = _object("row", bad, noise, w)
    assert_array_equal(o.signal_logpdf(x, ym), np.full(4, -np.inf))
    for tail in (o.signal_cdf(x, ym), o.signal_cdf(x, ym, upper=True), o.signal_pvalue(x, ym)):
        assert_array_equal(tail, np.zeros((1, 4)))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        out, info = o.signal_quantile(BAND, x, full_output=True)
    assert np.all(np.isnan(out)) and not info["passes"].any() and info["unconverged"] == 0
    for dead in (np.zeros(300), np.full(300, np.nan), -np.ones(300)):
        o = _object("row", cloud, noise, dead)
        assert np.all(np.isnan(o.signal_logpdf(x, ym))) and np.all(np.isnan(o.signal_cdf(x, ym)))
        assert np.all(np.isnan(o.signal_pvalue(x, ym))) and np.all(np.isnan(o.signal_cdf(x, ym, upper=True)))
        out, info = o.signal_quantile(BAND, x, full_output=True)
        assert np.all(np.isnan(out)) and not info["passes"].any()


# ------------------------------------------------------------------------------------------------ 4. width spread
def test_widths_over_five_decades(hip):
    """Relative noise on values from 1e-2 to 1e3: the components' widths differ by five decades across the cloud."""
    g = np.random.default_rng(50)
    n = 2000
    cloud = 10.0 ** g.uniform(-2.0, 3.0, (1, n))
    w = g.random(n) + 0.1
    w /= w.sum()
    (_, _, _), (out, passes), _ = _row_check("five decades of width", cloud, w, (0.0, 0.0, 0.1), g)
    sig = np.sqrt(sn.nu(cloud, np.array([[0.0, 0.0, 0.1 * 0.1]])))
    assert sig.max() / sig.min() > 5e4
    o = _object("row", cloud, (0.0, 0.0, 0.1), w)
    _check_quantiles("five decades of width, far levels", o, np.zeros((1, 1)), FIVE, cloud[None], w)


def test_two_modes_a_hundred_widths_apart(hip):
    g = np.random.default_rng(51)
    n = 1000
    cloud = np.where(g.random((1, n)) < 0.5, 100.0, 1100.0) + g.normal(0.0, 0.5, (1, n))      # widths 10 and about 10
    w = np.full(n, 1.0 / n)
    noise = (10.0, 0.0, 0.0)
    (_, _, _), (out, _), (o, x, _) = _row_check("two modes", cloud, w, noise, g)
    out, _ = _check_quantiles("two modes, levels between them", o, x, (0.3, 0.45, 0.5, HALF_UP, 0.55, 0.7), cloud[None].repeat(3, 0), w)
    assert np.all((out < 140.0) | (out > 1060.0))


def test_one_particle_is_f_plus_z_sqrt_nu(hip):
    """One particle: f + z sqrt(nu(f)) to rounding, at the bound of test_gpu_reading's one-particle case."""
    noise = (3.0, 1.0, 0.05)
    qs = np.array(FIVE + BAND)
    z = _reading.normal_quantiles(qs)
    # (the tolerance in y, to first order: the residual over the density, 1e-10 sigma min(q, 1 - q) / phi(z) — 1.26e-10
    # sigma at the median, less in the tails — and the 8 eps |y| of the last bits, twice for f + sigma z)
    mills = np.minimum(qs, 1.0 - qs) / (np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi))
    for f in (0.0, 7.5, -120.0, 1e5):
        cloud, w = np.array([[f]]), np.array([0.37])
        o = _object("row", cloud, noise, w)
        x = np.zeros((1, 1))
        y = _rows(o, x)
        assert_array_equal(_bits(y[0, 0]), _bits(cloud[0]))
        sg = float(_sigma_rows(y, o._coefficients())[0, 0, 0])
        out, _ = _check_quantiles(f"one particle at {f!r}", o, x, qs, y, w)
        want = f + z * sg
        assert np.all(np.abs(out[:, 0, 0] - want) <= 1.01e-10 * mills * sg + 16 * reading.EPS * np.abs(want)), (f, out[:, 0, 0] - want)
        ym = np.array([[f + 0.7 * sg]])
        _check_scores(f"one particle at {f!r}", o, x, ym, y, w)


def test_a_converged_cloud_is_the_mean_plus_z_sqrt_nu(hip):
    """The model values agree to 1e-7 of themselves (sd / sigma of the order of 1e-6, as in test_gpu_reading's converged
    cloud), so the widths sqrt(nu(f_i)) agree to 1e-7 too and their first-order effect cancels about the weighted mean:
    the band is mean + z sqrt(nu(mean)) within that test's 1e-9 sigma."""
    g = np.random.default_rng(53)
    n = 3000
    cloud = 400.0 * (1.0 + 1e-7 * g.normal(size=(1, n)))
    w = _weights(g, g.normal(size=(1, n)))
    noise = (2.0, 1.0, 0.01)
    o = _object("row", cloud, noise, w)
    x = np.zeros((1, 3))
    y = _rows(o, x)
    mean, _ = o.predict(x)
    sg = float(np.sqrt(sn.nu(mean[:, :1], o._coefficients())[0, 0]))
    ratio = np.std(y[:, 0, :], axis=1) / sg
    assert np.all((ratio > 1e-7) & (ratio < 1e-5)), ratio
    qs = np.array(FIVE + BAND)
    out, _ = _check_quantiles("converged cloud", o, x, qs, y, w)
    _check_scores("converged cloud", o, x, _readings(g, y, w, _sigma_rows(y, o._coefficients())), y, w)
    z = _reading.normal_quantiles(qs)
    assert np.all(np.abs(out[:, 0, :] - (mean[0][None, :] + z[:, None] * sg)) <= 1e-9 * sg)


# --------------------------------------------------------------------------------------------------- 5. identities
def test_interval_is_the_two_quantiles_and_tiles_do_not_matter(hip, monkeypatch):
    g, o, x, y, w = _case("coil", 81, 2000, 23)
    lo, hi = o.signal_interval(0.9, x)
    both = o.signal_quantile(((1.0 - 0.9) / 2.0, (1.0 + 0.9) / 2.0), x)
    assert lo.shape == hi.shape == (2, 23)
    assert_array_equal(_bits(lo), _bits(both[0]))
    assert_array_equal(_bits(hi), _bits(both[1]))
    assert np.all(lo < hi)
    lo3, hi3, info = o.signal_interval(0.9, x, full_output=True)
    assert_array_equal(_bits(lo3), _bits(lo))
    assert_array_equal(_bits(hi3), _bits(hi))
    assert info["unconverged"] == 0 and info["passes"].shape == (2, 2, 23)
    sig = _sigma_rows(y, o._coefficients())
    ym = _readings(g, y, w, sig)
    want = o.signal_quantile(FIVE, x, full_output=True)
    scores = o.signal_logpdf(x, ym), o.signal_cdf(x, ym), o.signal_cdf(x, ym, upper=True), o.signal_pvalue(x, ym)
    monkeypatch.setattr(_reading, "SETTINGS_PER_CALL", 7)
    monkeypatch.setattr(_reading, "MAX_Q_PER_CALL", 2)
    monkeypatch.setattr(_scoring, "RECORDS_PER_CALL", 5)
    got = o.signal_quantile(FIVE, x, full_output=True)
    assert_array_equal(_bits(got[0]), _bits(want[0]))
    assert_array_equal(got[1]["passes"], want[1]["passes"])
    for a, b in zip(scores, (o.signal_logpdf(x, ym), o.signal_cdf(x, ym), o.signal_cdf(x, ym, upper=True),
                             o.signal_pvalue(x, ym))):
        assert_array_equal(_bits(a), _bits(b))


def test_the_design_grid_is_the_default(hip):
    g, o, _, _, w = _case("coil", 82, 700, 3)
    grid = np.asarray(o.allsettings, dtype=np.float64)
    whole = o.signal_quantile(BAND)
    assert whole.shape == (2, 2, grid.shape[1])
    assert_array_equal(_bits(whole), _bits(o.signal_quantile(BAND, grid)))
    _check_quantiles("design grid", o, grid, BAND, _rows(o, grid), w)
    lo, hi = o.signal_interval()
    assert lo.shape == hi.shape == (2, grid.shape[1]) and np.all(lo < hi)


def test_round_trip_through_the_tails(hip):
    """signal_cdf(x, signal_quantile(q, x)) is q: within 1e-10 min(q, 1 - q) plus what the last bits of the quantile are
    worth, 8 eps |v| D / T — in the tail the level was solved in, and (one rounding of a value near 1 more) in the
    other one.  A cloud without left-out particles: the tails' normaliser is the quantiles' T."""
    g, o, x, y, w = _case("coil", 83, 3000, 9)
    sig = _sigma_rows(y, o._coefficients())
    assert np.all(np.isfinite(sig))
    qs = np.array((1e-12, 1e-6, 0.025, 0.4999, 0.5, HALF_UP, 0.5001, 0.975, 1.0 - 1e-6, 1.0 - 1e-12))
    out, _ = _check_quantiles("round trip", o, x, qs, y, w, sig=sig)
    for j, q in enumerate(qs):
        lower = o.signal_cdf(x, out[j])
        upper = o.signal_cdf(x, out[j], upper=True)
        for r in range(x.shape[1]):
            mix = reading.Reading(y[r], w, sig[r])
            for c in range(2):
                v = out[j, c, r]
                tol = 1e-10 * min(q, 1.0 - q) + 8.0 * reading.EPS * abs(v) * mix.density(c, v) / mix.total(c)
                if q <= 0.5:
                    assert abs(lower[c, r] - q) <= tol, (q, r, c, lower[c, r])
                    assert abs(upper[c, r] - (1.0 - q)) <= tol + 2 * reading.EPS
                else:
                    assert abs(upper[c, r] - (1.0 - q)) <= tol, (q, r, c, upper[c, r])
                    assert abs(lower[c, r] - q) <= tol + 2 * reading.EPS


def test_logpdf_of_one_record_is_the_evidence_of_records_loglik(hip):
    """log(sum w exp(records_loglik) / sum w), formed here in long double, for one record at a time."""
    g, o, x, y, w = _case("coil", 84, 3000, 4)
    ym = _readings(g, y, w, _sigma_rows(y, o._coefficients()))
    for r in range(4):
        setting = (float(x[0, r]),)
        got = o.signal_logpdf(setting, ym[:, r])
        assert isinstance(got, float)
        l = np.asarray(o.records_loglik((x[:, r:r + 1][0],), ym[:, r:r + 1]), dtype=np.float64).astype(LD)
        assert np.all(np.isfinite(l))
        top = l.max()
        want = float(top + np.log(np.sum(np.sort(w.astype(LD) * np.exp(l - top)))) - np.log(LD(math.fsum(w))))
        assert abs(got - want) <= scoring.logpdf_tolerance(want), (r, got, want)
        assert_array_equal(_bits(got), _bits(o.signal_logpdf(x[:, r:r + 1], ym[:, r:r + 1])[0]))


# ------------------------------------------------------------------------------------- 6. no side effects, state
def _peak_object(seed, n=4099):
    g = np.random.default_rng(seed)
    cloud = np.array([g.normal(3, 0.05, n), g.uniform(400, 2000, n), g.normal(50, 5, n)])
    o = _object("lorentz1", cloud, (5.0, 1.0, 0.01), utility_method="variance_full")
    o.rng = np.random.default_rng(seed + 1)
    return g, o


def _run(watch, cycles=12):
    g, o = _peak_object(60)
    picks, resampled, inside = [], [], 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for _ in range(cycles):
            x = o.opt_setting()
            f = 50.0 + 1200.0 / (((x[0] - 3.02) / 0.1) ** 2 + 1.0)
            yv = f + math.sqrt(25.0 + f + 1e-4 * f * f) * g.normal()
            picks.append(int(o.last_setting_index))
            if watch:
                before = o.sweep_state()
                lo, hi, info = o.signal_interval(0.95, x, full_output=True)
                assert info["unconverged"] == 0 and lo.shape == (1, 1) and lo[0, 0] < hi[0, 0]
                assert np.isfinite(o.signal_logpdf(x, yv)) and 0.0 <= o.signal_pvalue(x, yv)[0, 0] <= 1.0
                assert o.sweep_state() == before
                inside += lo[0, 0] <= yv <= hi[0, 0]
            o.pdf_update((x, yv))
            resampled.append(bool(o.just_resampled))
    return o, picks, resampled, inside


def test_a_trajectory_is_unchanged_by_the_new_calls(hip):
    from optbayesexpt_amd import _state
    watched, picks, resampled, inside = _run(True)
    plain, want_picks, want_resampled, _ = _run(False)
    assert picks == want_picks and resampled == want_resampled and any(resampled)
    assert_array_equal(_bits(watched.particle_weights), _bits(plain.particle_weights))
    assert_array_equal(_bits(watched.particles), _bits(plain.particles))
    np.testing.assert_equal(watched.rng.bit_generator.state, plain.rng.bit_generator.state)
    assert set(_state.snapshot(watched)) == set(_state.snapshot(plain))          # nothing added to snapshots
    assert set(vars(watched)) == set(vars(plain))                                # ... nor to the object
    assert inside >= 9                                                           # honest readings fall inside


def test_restored_copied_and_pickled_objects(hip, tmp_path):
    import optbayesexpt_amd as obe
    g, o = _peak_object(61)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for _ in range(3):
            o.pdf_update((o.opt_setting(), 900.0 + 40.0 * g.normal()))
    x, ym = (np.linspace(2.0, 4.0, 9),), 60.0 + 30.0 * g.random(9)
    want = o.signal_quantile((0.025, 0.5, 0.975), x, full_output=True)
    assert want[1]["unconverged"] == 0
    scores = o.signal_logpdf(x, ym), o.signal_cdf(x, ym), o.signal_pvalue(x, ym)
    path = str(tmp_path / "signal.state")
    obe.save(o, path)
    for other in (obe.load(path), copy.deepcopy(o), pickle.loads(pickle.dumps(o))):
        got = other.signal_quantile((0.025, 0.5, 0.975), x, full_output=True)
        assert_array_equal(_bits(got[0]), _bits(want[0]))
        assert_array_equal(got[1]["passes"], want[1]["passes"])
        for a, b in zip(scores, (other.signal_logpdf(x, ym), other.signal_cdf(x, ym), other.signal_pvalue(x, ym))):
            assert_array_equal(_bits(a), _bits(b))


def test_reassigned_coefficients_are_used_by_the_next_call(hip):
    g, o, x, y, w = _case("lorentz1", 62, 2000, 5)
    first, _ = _check_all("before the reassignment", o, x, y, w, g)
    o.noise_gain = np.array([8.0 * float(o.noise_gain[0])])
    second, _ = _check_all("after the reassignment", o, x, y, w, g)              # (the oracle reads the new coefficients)
    assert np.all(second[0] < first[0]) and np.all(second[1] > first[1])          # more noise: a wider band
    o.noise_gain = np.array([-1.0])
    for call in (lambda: o.signal_logpdf(x, np.full(5, 49000.0)), lambda: o.signal_pvalue(x, np.full(5, 49000.0)),
                 lambda: o.signal_quantile(0.5, x), lambda: o.signal_interval(0.9)):
        with pytest.raises(ValueError, match="noise_gain"):
            call()


def test_host_edits_are_uploaded_first(hip):
    g, o, x, y, w = _case("lorentz1", 63, 3000, 5)
    cloud = np.asarray(o.particles)
    o.particle_weights[cloud[0] > 3.0] = 0                           # in place, by host code
    _check_all("edited weights", o, x, y, np.where(cloud[0] > 3.0, 0.0, w), g)
    o.particle_weights = w[:-1]
    with pytest.raises(ValueError, match="different lengths"):
        o.signal_quantile(0.5, x)


# ------------------------------------------------------------------------------------------------------ 7. budget
def test_a_budget_of_one_pass_warns_and_the_default_does_not(hip):
    g = np.random.default_rng(91)
    cloud = _prior("lorentz1", g, 5000)
    w = _weights(g, cloud)
    o = _object("lorentz1", cloud, (30.0, 0.0, 0.0), w)              # far below the prior's spread of model values
    x = _points("lorentz1", g, 70)
    y = _rows(o, x)
    sig = _sigma_rows(y, o._coefficients())
    with pytest.warns(RuntimeWarning, match=r"signal_quantile: \d+ of 140 results were still open after 1 passes"):
        out, info = o.signal_quantile(BAND, x, max_passes=1, full_output=True)
    assert info["unconverged"] > 0 and info["unconverged"] == np.count_nonzero(info["passes"] == -1)
    assert np.all((info["passes"] == -1) | (info["passes"] == 1))
    assert np.all(np.isfinite(out))
    for r in range(70):
        mix = reading.Reading(y[r], w, sig[r])
        for j, q in enumerate(BAND):
            lo, hi = mix.bracket(0, q)
            assert np.nextafter(lo, -np.inf) <= out[j, 0, r] <= np.nextafter(hi, np.inf)
    _, passes = _check_quantiles("prior-width cloud, default budget", o, x, BAND, y, w, sig=sig)      # (warnings are errors)
    assert passes.max() > 1


# ------------------------------------------------------------------------------------------------ 8. the example
def test_counting_band_example(hip):
    spec = importlib.util.spec_from_file_location("counting_band", os.path.join(ROOT, "examples", "counting_band.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        points, (lo, hi), (flat_lo, flat_hi), inside = mod.main(n_measure=25, n_samples=10000, n_check=400, seed=3, quiet=True)
    assert lo.shape == hi.shape == flat_lo.shape == flat_hi.shape == points.shape and np.all(lo < hi)
    # the flat floor's band is too narrow on the peak, where the counting noise is largest
    top = int(np.argmax(hi - lo))
    assert hi[top] - lo[top] > 1.5 * (flat_hi[top] - flat_lo[top])
    # 95 % +- 5 binomial standard deviations of 400 readings: a condition on the example's seed, not a measurement
    assert 0.90 <= inside["signal noise"] <= 0.99, inside
    assert inside["flat noise"] < inside["signal noise"]


def test_worst_errors_are_reported(hip):
    """(runs last of the comparisons: the worst error / tolerance ratios and the worst pass count of this file)"""
    for kind in ("log p", "tail", "quantile"):
        print(f"worst {kind}: {WORST[kind][0]:.3g} of its tolerance ({WORST[kind][1]})")
    print(f"worst pass count: {WORST['passes'][0]} ({WORST['passes'][1]})")
    assert all(WORST[kind][1] for kind in ("log p", "tail", "quantile")) and WORST["passes"][0] >= 1
