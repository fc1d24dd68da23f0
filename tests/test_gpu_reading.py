"""Device-side quantiles of the next reading (OptBayesExpt.reading_quantile / reading_interval; csrc/obe_predict.hip, K15)
against tests/_reading_oracle.py on the rows y = eval_over_all_parameters((x_s,)) of the product itself.

Acceptance per result v (level q, channel c): |A(v) - target| <= 1e-10 target + 8 eps max(|v|, 2^-1022) D(v), A the tail
the level solves in, D the density mass, both the oracle's (_reading_oracle.Reading.tolerance: derived from the stopping
rule, the fixed-order sums and the 4-ulp bracket, not measured).  ``unconverged == 0`` is asserted in every comparison.
Run to run: the same bits.  The worst residual / tolerance ratio and the worst pass count seen are printed by
test_worst_errors_are_reported."""
import copy
import importlib.util
import os
import warnings

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _fn_models
import _reading_oracle as oracle
import _state_cases as cases
from optbayesexpt_amd import _reading

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = (1 << 17) + 3
WORST = {"ratio": (0.0, ""), "passes": (0, "")}
HALF_UP = float(np.nextafter(0.5, 1.0))
EDGES = (1e-12, 0.5, HALF_UP, 1.0 - 1e-12)
FIVE = (1e-12, 0.3, 0.5, HALF_UP, 1.0 - 1e-12)


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
    return g.uniform(1.5, 4.5, n_x)[None, :]


def _design(name):
    if name == "rabi":
        return (np.linspace(0.0, 3.0, 5), np.linspace(-4.0, 4.0, 7))
    if name == "coil":
        return (np.linspace(1.0e4, 6.0e4, 33),)
    return (np.linspace(1.5, 4.5, 33),)


def _object(name, cloud, weights=None, noise_rows=None):
    import optbayesexpt_amd as obe
    model, cons = _model(name)
    if noise_rows is None:
        o = obe.OptBayesExpt(model, _design(name), cloud, cons, scale=False)
    else:
        o = obe.OptBayesExptNoiseParameter(model, _design(name), cloud, cons, noise_parameter_index=noise_rows, scale=False)
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


def _sigma(g, y, w):
    """A known sigma (C, n_x) that differs per setting and channel, of the size of the model values' own spread."""
    n_x, n_c, _ = y.shape
    good = np.where(np.isfinite(y), y, np.nan)
    spread = np.array([[np.nanstd(good[r, c]) for r in range(n_x)] for c in range(n_c)])
    level = np.array([[abs(np.nanmedian(good[r, c])) for r in range(n_x)] for c in range(n_c)])
    return (spread + 1e-3 * level + 1e-12) * g.uniform(0.25, 2.0, (n_c, n_x))


def _noise_cloud(name, g, n, rows, x):
    """The prior of ``name`` with noise rows ``rows`` (one per channel) of the size of the model values' own spread."""
    cloud = _prior(name, g, n)
    y = _rows(_object(name, cloud), x[:, :3])
    scale = [np.median([np.std(y[r, c]) + 1e-3 * abs(y[r, c, 0]) + 1e-12 for r in range(y.shape[0])])
             for c in range(y.shape[1])]
    extra = np.ones((max(rows) + 1 - cloud.shape[0], n))
    for c, row in enumerate(rows):
        extra[row - cloud.shape[0]] = scale[c] * g.uniform(0.5, 2.0, n)
    return np.vstack([cloud, extra])


# ------------------------------------------------------------------------------------------------- the checks
def _check(what, o, x, qs, sigma, y, w, sig_rows=None, settings=None, **kw):
    """reading_quantile for the levels ``qs`` at the points ``x`` against the oracle fed y (n_x, C, N_p); ``settings``:
    the ones to compare (all).  Returns (quantiles, passes)."""
    qs = np.atleast_1d(np.asarray(qs, dtype=np.float64))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                                     # (an open row would warn)
        out, info = o.reading_quantile(qs, x, sigma, full_output=True, **kw)
        again = o.reading_quantile(qs, x, sigma, **kw)
    n_c = y.shape[1]
    assert out.shape == (qs.size, n_c, x.shape[1]) and out.dtype == np.float64
    assert info["passes"].shape == out.shape and info["passes"].dtype == np.int32
    assert info["unconverged"] == 0 and np.all(info["passes"] >= 1), (what, info["unconverged"], info["passes"].min())
    assert_array_equal(_bits(again), _bits(out), err_msg=f"{what}: run to run")
    for r in (range(x.shape[1]) if settings is None else settings):
        mix = oracle.Reading(y[r], w, sigma[:, r] if sig_rows is None else sig_rows)
        for c in range(n_c):
            for j, q in enumerate(qs):
                v = float(out[j, c, r])
                assert np.isfinite(v), (what, r, c, q)
                res, tol = mix.residual(c, float(q), v), mix.tolerance(c, float(q), v)
                if res / tol >= WORST["ratio"][0]:
                    WORST["ratio"] = res / tol, what
                if res > 0.5 * tol:
                    print(f"{what}: setting {r} channel {c} q {q!r}: residual {res:.3g}, tolerance {tol:.3g}, "
                          f"passes {info['passes'][j, c, r]}")
                assert res <= tol, f"{what}: setting {r}, channel {c}, q {q!r}: {v!r}, residual {res:.3g} > {tol:.3g}"
    top = int(info["passes"].max())
    if top >= WORST["passes"][0]:
        WORST["passes"] = top, what
    return out, info["passes"]


# ------------------------------------------------------------------------- 1. shapes: settings x particles x levels
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_shapes_lorentzian(hip, n):
    """Both sides of the wave of 64 settings and of the chunk of 256 particles; one particle; 20 chunks."""
    for n_x in (1, 63, 64, 65, 130):
        g = np.random.default_rng([n, n_x])
        cloud = _prior("lorentz1", g, n)
        w = _weights(g, cloud) if n > 1 else np.ones(1)
        o = _object("lorentz1", cloud, w)
        x = _points("lorentz1", g, n_x)
        y = _rows(o, x)
        sigma = _sigma(g, y, w)
        _check(f"lorentz1 {n_x} x {n}", o, x, (0.025, 0.975), sigma, y, w)


def test_seventy_settings_at_131075_particles(hip):
    """70 settings x 2^17 + 3 particles (513 chunks): seven different settings against the oracle, each repeated in ten
    lanes of two waves, which must all hold the same bits."""
    g = np.random.default_rng(70)
    cloud = _prior("lorentz1", g, BIG)
    cloud[0] = 3.0 + 0.05 * g.normal(size=BIG)
    w = _weights(g, cloud)
    o = _object("lorentz1", cloud, w)
    x7 = np.linspace(2.6, 3.4, 7)[None, :]
    y7 = _rows(o, x7)
    sigma7 = _sigma(g, y7, w)
    x, sigma = np.tile(x7, 10), np.tile(sigma7, 10)
    out, passes = _check("lorentz1 70 x BIG", o, x, (0.025, 0.975), sigma, y7, w, settings=range(7))
    assert_array_equal(_bits(out), _bits(np.tile(out[:, :, :7], 10)))
    assert_array_equal(passes, np.tile(passes[:, :, :7], 10))


@pytest.mark.parametrize("n_q", [1, 2, 5, 16, 17])
def test_level_counts(hip, n_q):
    """One level, two, five (a group of eight is not full), sixteen (two groups of a call) and seventeen (two calls),
    the far tails, the median and the float just above it among them; every level's result is the bits of a call of its
    own."""
    g = np.random.default_rng(n_q)
    cloud = _prior("lorentz1", g, 300)
    w = _weights(g, cloud)
    o = _object("lorentz1", cloud, w)
    x = _points("lorentz1", g, 3)
    y = _rows(o, x)
    sigma = _sigma(g, y, w)
    qs = {1: (HALF_UP,), 2: (1e-12, 1.0 - 1e-12), 5: FIVE}.get(n_q)
    if qs is None:
        qs = tuple(np.sort(np.concatenate([EDGES, np.linspace(0.02, 0.97, n_q - 4)])))
    assert len(set(qs)) == n_q
    out, passes = _check(f"{n_q} levels", o, x, qs, sigma, y, w)
    for j, q in enumerate(qs):
        alone, info = o.reading_quantile(q, x, sigma, full_output=True)
        assert alone.shape == (1, 3)                                         # a scalar q: no level axis
        assert_array_equal(_bits(alone), _bits(out[j]), err_msg=f"level {q!r} of {n_q}")
        assert_array_equal(info["passes"], passes[j])
    # strictly increasing in q — among levels the result can tell apart: the median and the float just above it differ
    # by 1e-16 sigma in y, far below one ulp of y, and are solved in different tails, each to its tolerance
    apart = [j for j, q in enumerate(qs) if q != HALF_UP or 0.5 not in qs]
    if len(apart) > 1:
        assert np.all(np.diff(out[apart], axis=0) > 0.0)


@pytest.mark.parametrize("name", ["lorentz7", "coil", "rabi", "expression", "function"])
def test_models(hip, name):
    for n, n_x in ((5000, 65), (300, 3)):
        g = np.random.default_rng([sum(map(ord, name)), n])
        cloud = _prior(name, g, n)
        w = _weights(g, cloud)
        o = _object(name, cloud, w)
        assert (o._mlib is not o._lib) == (name in ("expression", "function"))          # plugins serve their own model
        x = _points(name, g, n_x)
        y = _rows(o, x)
        sigma = _sigma(g, y, w)
        assert y.shape[1] == (2 if name == "coil" else 1) and x.shape[0] == (2 if name == "rabi" else 1)
        if name == "coil":
            assert np.all(sigma[0] != sigma[1])                              # a different sigma per channel
        _check(f"{name} {n_x} x {n}", o, x, FIVE if n == 300 else (0.025, 0.975), sigma, y, w)


@pytest.mark.parametrize("name,rows", [("lorentz1", (3,)), ("coil", (3, 4)), ("coil", (4, 4))])
def test_noise_parameter_class(hip, name, rows):
    for n, n_x in ((5000, 65), (257, 2)):
        g = np.random.default_rng([sum(map(ord, name)), n, len(set(rows))])
        x = _points(name, g, n_x)
        cloud = _noise_cloud(name, g, n, rows, x)
        w = _weights(g, cloud)
        o = _object(name, cloud, w, noise_rows=rows if len(rows) > 1 else rows[0])
        y = _rows(o, x)
        _check(f"noise {name} {rows} {n_x} x {n}", o, x, FIVE if n == 257 else (0.025, 0.975), None, y, w, cloud[list(rows)])
        with pytest.raises(ValueError, match="noise parameter"):
            o.reading_quantile(0.5, x, 1.0)


def test_a_tile_whose_lanes_close_at_different_passes(hip):
    """One wave: settings on the flank of a sharp peak (the model values spread over many sigma) and far from it (they
    agree to a fraction of sigma).  The lanes close at different passes, the tile stays open for the slowest."""
    g = np.random.default_rng(61)
    n = 2000
    cloud = np.array([3.0 + 0.02 * g.normal(size=n), g.uniform(-2000, -400, n), 50000.0 + g.normal(size=n)])
    w = _weights(g, cloud)
    o = _object("lorentz1", cloud, w)
    x = np.concatenate([np.linspace(2.9, 3.1, 32), np.linspace(1.5, 1.8, 16), np.linspace(4.2, 4.5, 16)])[None, :]
    y = _rows(o, x)
    sigma = np.full((1, 64), 5.0)
    spread = np.std(y[:, 0, :], axis=1)
    assert spread[:32].min() > 50.0 and spread[32:].max() < 5.0
    out, passes = _check("mixed tile", o, x, (0.025, 0.5, 0.975), sigma, y, w)
    assert passes.min() < passes.max(), passes
    assert passes[:, :, 32:].max() < passes[:, :, :32].max()


# ---------------------------------------------------------------------------------------------- 2. special clouds
def test_a_converged_cloud_is_the_mean_plus_z_sigma(hip):
    g = np.random.default_rng(62)
    n = 3000
    cloud = np.array([3.0, -1000.0, 50000.0])[:, None] * (1.0 + 1e-10 * g.normal(size=(3, n)))
    w = _weights(g, g.normal(size=(1, n)))
    o = _object("lorentz1", cloud, w)
    x = np.array([[2.5, 3.0, 3.05, 4.0]])
    y = _rows(o, x)
    sg = 5.0
    ratio = np.std(y[:, 0, :], axis=1) / sg
    assert np.all((ratio > 1e-7) & (ratio < 1e-5)), ratio                   # sd / sigma of the order of 1e-6
    qs = np.array(FIVE + (0.025, 0.975))
    out, _ = _check("converged cloud", o, x, qs, np.full((1, 4), sg), y, w)
    mean, _ = o.predict(x)
    z = _reading.normal_quantiles(qs)
    assert np.all(np.abs(out[:, 0, :] - (mean[0][None, :] + z[:, None] * sg)) <= 1e-9 * sg)


def test_one_particle_is_f_plus_sigma_z(hip):
    g = np.random.default_rng(63)
    for name in ("lorentz1", "coil"):
        cloud = _prior(name, g, 1)
        o = _object(name, cloud, np.array([0.37]))
        x = _points(name, g, 5)
        y = _rows(o, x)
        sigma = _sigma(g, y, np.ones(1))                                     # (no spread: a thousandth of the value)
        qs = np.array(FIVE)
        out, _ = _check(f"one particle {name}", o, x, qs, sigma, y, np.array([0.37]))
        z = _reading.normal_quantiles(qs)
        want = y[:, :, 0].T[None, :, :] + z[:, None, None] * sigma[None, :, :]
        # (the tolerance in y, to first order: the residual over the density, 1e-10 sigma min(q, 1 - q) / phi(z) —
        # 1.26e-10 sigma at the median, less in the tails — and the 8 eps |y| of the last bits, twice for f + sigma z)
        mills = np.minimum(qs, 1.0 - qs) / (np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi))
        assert np.all(np.abs(out - want) <= 1.01e-10 * mills[:, None, None] * sigma[None] + 16 * oracle.EPS * np.abs(want))


def test_two_modes_a_hundred_sigma_apart(hip):
    """Half of the weight at 0, half at 100 sigma (a = 0: the model value is b): the levels just below and just above the
    median lie in different modes, four sigma from their centres."""
    n = 1000
    for jitter in (0.0, 0.1):
        g = np.random.default_rng(64)
        b = np.repeat([0.0, 100.0], n // 2) + jitter * g.normal(size=n)
        cloud = np.array([g.uniform(2, 4, n), np.zeros(n), b])
        w = np.ones(n) / n
        o = _object("lorentz1", cloud, w)
        x = np.array([[2.0, 3.0]])
        y = _rows(o, x)
        assert_array_equal(y[0, 0], b)
        out, _ = _check(f"two modes, jitter {jitter}", o, x, (0.4999, 0.5001), np.ones((1, 2)), y, w)
        assert np.all(out[0] < 5.0) and np.all(out[1] > 95.0), out


def test_sigma_rows_over_five_decades(hip):
    g = np.random.default_rng(65)
    n = 2000
    cloud = np.array([g.uniform(2, 4, n), np.zeros(n), g.normal(0.0, 1.0, n), 10.0 ** g.uniform(-3.0, 2.0, n)])
    w = g.random(n)
    w /= w.sum()
    o = _object("lorentz1", cloud, w, noise_rows=3)
    x = np.array([[2.0, 3.3]])
    y = _rows(o, x)
    assert cloud[3].max() / cloud[3].min() > 1e4
    _check("sigma rows 1e-3 .. 1e2", o, x, FIVE + (0.025, 0.975), None, y, w, cloud[[3]])


@pytest.mark.parametrize("scale", [1e-300, 1e300])
def test_scales(hip, scale):
    g = np.random.default_rng(66)
    n = 1000
    cloud = _prior("lorentz1", g, n)
    cloud[1:] *= scale                                                       # the model is linear in (a, b)
    w = _weights(g, cloud)
    o = _object("lorentz1", cloud, w)
    x = _points("lorentz1", g, 4)
    y = _rows(o, x)
    assert np.all(np.isfinite(y)) and abs(np.log10(np.abs(y).max() / scale) - 4.7) < 0.5
    _check(f"scale {scale:g}", o, x, FIVE, np.full((1, 4), 300.0 * scale), y, w)


# ------------------------------------------------------------------------------------------------- 3. exclusions
def test_particles_that_do_not_contribute_base_class(hip):
    """Zero, NaN and negative weights, and weighted particles with a NaN or +-inf model value: bit-equal to the cloud
    in which they have no weight (the same places, so the same chunks), and both as the oracle has them."""
    g = np.random.default_rng(71)
    n = 600                                                  # three chunks
    cloud = _prior("lorentz1", g, n)
    w = _weights(g, cloud)
    w[[0, 1, 255, 256, 599]] = [0.0, np.nan, -0.25, 0.0, np.nan]
    cloud[0, 0], cloud[1, 1], cloud[1, 255], cloud[0, 256] = np.nan, np.inf, -np.inf, np.nan      # no weight anyway
    cloud[0, 10], cloud[1, 300], cloud[1, 301] = np.nan, np.inf, -np.inf                          # weighted: left out
    o = _object("lorentz1", cloud, w)
    x = _points("lorentz1", g, 5)
    y = _rows(o, x)
    assert np.all(np.isnan(y[:, 0, 10])) and np.all(y[:, 0, 300] == np.inf) and np.all(y[:, 0, 301] == -np.inf)
    good = np.isfinite(y).all(axis=(0, 1))
    assert good.sum() == n - 7                               # (0, 1, 255 and 256 without a weight; 10, 300 and 301 with one)
    sigma = _sigma(g, y, w)
    out, passes = _check("non-finite", o, x, FIVE, sigma, y, w)
    with np.errstate(invalid="ignore"):
        w2 = np.where(good & (w > 0), w, 0.0)
    o2 = _object("lorentz1", np.where(good, cloud, 3.0), w2)
    out2, info2 = o2.reading_quantile(FIVE, x, sigma, full_output=True)
    assert_array_equal(_bits(out2), _bits(out))
    assert_array_equal(info2["passes"], passes)


def test_particles_that_do_not_contribute_noise_class(hip):
    g = np.random.default_rng(72)
    n = 600
    cloud = np.vstack([_prior("coil", g, n), np.ones((2, n))])
    x = _points("coil", g, 5)
    y0 = _rows(_object("coil", cloud[:3]), x)
    for c in range(2):
        cloud[3 + c] = np.median(np.std(y0[:, c, :], axis=1)) * g.uniform(0.5, 2.0, n)
    clean = cloud.copy()
    w = _weights(g, cloud)
    cloud[3, [5, 256, 257]] = [0.0, -1.0, np.nan]
    cloud[4, [6, 599]] = [np.nan, -0.0]
    cloud[3, 7], w[7] = -3.0, 0.0
    cloud[0, 8] = np.nan                                     # a NaN model value with good rows
    o = _object("coil", cloud, w, noise_rows=(3, 4))
    y = _rows(o, x)
    assert np.all(np.isnan(y[:, :, 8]))
    out, passes = _check("bad noise rows", o, x, FIVE, None, y, w, cloud[[3, 4]])
    w2 = w.copy()
    w2[[5, 256, 257, 6, 599, 7, 8]] = 0.0
    o2 = _object("coil", clean, w2, noise_rows=(3, 4))
    out2, info2 = o2.reading_quantile(FIVE, x, full_output=True)
    assert_array_equal(_bits(out2), _bits(out))
    assert_array_equal(info2["passes"], passes)


def test_nobody_contributing_gives_nan_and_zero_passes(hip):
    g = np.random.default_rng(73)
    cloud = _prior("lorentz1", g, 300)
    x = _points("lorentz1", g, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        for w in (np.zeros(300), np.full(300, np.nan), -np.ones(300)):
            out, info = _object("lorentz1", cloud, w).reading_quantile((0.1, 0.9), x, 500.0, full_output=True)
            assert out.shape == (2, 1, 3) and np.all(np.isnan(out)) and not info["passes"].any() and info["unconverged"] == 0
        bad = np.vstack([cloud, -np.ones((1, 300))])         # every noise row negative
        out, info = _object("lorentz1", bad, np.ones(300), noise_rows=3).reading_quantile(0.5, x, full_output=True)
        assert np.all(np.isnan(out)) and not info["passes"].any()
        nan_cloud = cloud.copy()
        nan_cloud[0] = np.nan                                # every model value NaN
        lo, hi, info = _object("lorentz1", nan_cloud, np.ones(300)).reading_interval(0.9, x, 500.0, full_output=True)
        assert np.all(np.isnan(lo)) and np.all(np.isnan(hi)) and not info["passes"].any()


# -------------------------------------------------------------------------------------------------- 4. properties
def _coil_case(seed, n=5000, n_x=130):
    g = np.random.default_rng(seed)
    cloud = _prior("coil", g, n)
    w = _weights(g, cloud)
    o = _object("coil", cloud, w)
    x = _points("coil", g, n_x)
    return g, o, x, w


def test_interval_is_the_two_quantiles_and_tiles_do_not_matter(hip, monkeypatch):
    g, o, x, w = _coil_case(81, n_x=23)
    y = _rows(o, x)
    sigma = _sigma(g, y, w)
    lo, hi = o.reading_interval(0.9, x, sigma)
    both = o.reading_quantile(((1.0 - 0.9) / 2.0, (1.0 + 0.9) / 2.0), x, sigma)
    assert lo.shape == hi.shape == (2, 23)
    assert_array_equal(_bits(lo), _bits(both[0]))
    assert_array_equal(_bits(hi), _bits(both[1]))
    assert np.all(lo < hi)
    lo3, hi3, info = o.reading_interval(0.9, x, sigma, full_output=True)
    assert_array_equal(_bits(lo3), _bits(lo))
    assert_array_equal(_bits(hi3), _bits(hi))
    assert info["unconverged"] == 0 and info["passes"].shape == (2, 2, 23)
    want = o.reading_quantile(FIVE, x, sigma, full_output=True)
    monkeypatch.setattr(_reading, "SETTINGS_PER_CALL", 7)
    got = o.reading_quantile(FIVE, x, sigma, full_output=True)
    assert_array_equal(_bits(got[0]), _bits(want[0]))
    assert_array_equal(got[1]["passes"], want[1]["passes"])
    # sigma forms: a scalar, one value per channel
    one = o.reading_quantile(0.3, x, 7.0)
    assert_array_equal(_bits(one), _bits(o.reading_quantile(0.3, x, [7.0, 7.0])))
    assert_array_equal(_bits(one), _bits(o.reading_quantile(0.3, x, np.full((2, 23), 7.0))))


def test_the_design_grid_is_the_default(hip):
    g, o, _, w = _coil_case(82, n=700)
    grid = np.asarray(o.allsettings, dtype=np.float64)
    y = _rows(o, grid)
    sigma = _sigma(g, y, w)
    whole = o.reading_quantile((0.025, 0.975), None, sigma)
    assert whole.shape == (2, 2, grid.shape[1])
    assert_array_equal(_bits(whole), _bits(o.reading_quantile((0.025, 0.975), grid, sigma)))
    _check("design grid", o, grid, (0.025, 0.975), sigma, y, w)


def test_round_trip_through_the_tails(hip):
    """predictive_cdf(x, reading_quantile(q, x, sigma), sigma) is q: within 1e-10 min(q, 1 - q) plus what the last bits
    of the quantile are worth, 8 eps |v| D / T — in the tail the level was solved in, and (one rounding of a value near
    1 more) in the other one."""
    g, o, x, w = _coil_case(83, n=3000, n_x=9)
    y = _rows(o, x)
    sigma = _sigma(g, y, w)
    qs = np.array((1e-12, 1e-6, 0.025, 0.4999, 0.5, HALF_UP, 0.5001, 0.975, 1.0 - 1e-6, 1.0 - 1e-12))
    out, _ = _check("round trip", o, x, qs, sigma, y, w)
    for j, q in enumerate(qs):
        lower = o.predictive_cdf(x, out[j], sigma)
        upper = o.predictive_cdf(x, out[j], sigma, upper=True)
        for r in range(x.shape[1]):
            mix = oracle.Reading(y[r], w, sigma[:, r])
            for c in range(2):
                v = out[j, c, r]
                ulp = 8.0 * oracle.EPS * abs(v) * mix.density(c, v) / mix.total(c)
                tol = 1e-10 * min(q, 1.0 - q) + ulp
                if q <= 0.5:
                    assert abs(lower[c, r] - q) <= tol, (q, r, c, lower[c, r])
                    assert abs(upper[c, r] - (1.0 - q)) <= tol + 2 * oracle.EPS
                else:
                    assert abs(upper[c, r] - (1.0 - q)) <= tol, (q, r, c, upper[c, r])
                    assert abs(lower[c, r] - q) <= tol + 2 * oracle.EPS


def test_host_edits_are_uploaded_first(hip):
    g = np.random.default_rng(84)
    cloud = _prior("lorentz1", g, 3000)
    w = _weights(g, cloud)
    o = _object("lorentz1", cloud, w)
    x = _points("lorentz1", g, 5)
    y = _rows(o, x)
    sigma = _sigma(g, y, w)
    _check("before the edits", o, x, (0.1, 0.9), sigma, y, w)
    o.particle_weights[cloud[0] > 3.0] = 0                           # in place, by host code
    _check("edited weights", o, x, (0.1, 0.9), sigma, y, np.where(cloud[0] > 3.0, 0.0, w))
    o.particle_weights = w[:-1]
    with pytest.raises(ValueError, match="different lengths"):
        o.reading_quantile(0.5, x, sigma)


# ------------------------------------------------------------------------------------------------------ 5. budget
def test_a_budget_of_one_pass_warns_and_the_default_does_not(hip):
    g = np.random.default_rng(91)
    cloud = _prior("lorentz1", g, 5000)
    w = _weights(g, cloud)
    o = _object("lorentz1", cloud, w)
    x = _points("lorentz1", g, 70)
    y = _rows(o, x)
    sigma = np.full((1, 70), 30.0)                                   # far below the prior's spread of model values
    qs = (0.025, 0.975)
    with pytest.warns(RuntimeWarning, match=r"\d+ of 140 results were still open after 1 passes"):
        out, info = o.reading_quantile(qs, x, sigma, max_passes=1, full_output=True)
    assert info["unconverged"] > 0 and info["unconverged"] == np.count_nonzero(info["passes"] == -1)
    assert np.all((info["passes"] == -1) | (info["passes"] == 1))
    assert np.all(np.isfinite(out))
    for r in range(70):
        mix = oracle.Reading(y[r], w, sigma[:, r])
        for j, q in enumerate(qs):
            lo, hi = mix.bracket(0, q)
            assert np.nextafter(lo, -np.inf) <= out[j, 0, r] <= np.nextafter(hi, np.inf)
    _, passes = _check("prior-width cloud, default budget", o, x, qs, sigma, y, w)          # (warnings are errors there)
    assert passes.max() > 1


# ------------------------------------------------------------------------------------- 6. no side effects, state
def _run(case, n, watch):
    o = cases.build(case)
    picks, resampled, bands = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for cyc in range(n):
            x = o.opt_setting()
            picks.append(int(o.last_setting_index))
            if watch:
                before = o.sweep_state()
                sigma = None if case == "noise7" else cases.SIGMA
                lo, hi, info = o.reading_interval(0.95, x, sigma, full_output=True)
                assert info["unconverged"] == 0 and lo.shape == (1, 1) and lo[0, 0] < hi[0, 0]
                assert o.sweep_state() == before, f"cycle {cyc}"
                bands.append((lo[0, 0], hi[0, 0]))
            record = cases.measure(o, case, cyc, x)
            o.pdf_update(record)
            resampled.append(bool(o.just_resampled))
            if watch:
                bands[-1] += (record[1],)
    return o, cases.outcome(o, picks, resampled), bands


@pytest.mark.parametrize("case", ["lorentz_full", "noise7"])
def test_a_trajectory_is_unchanged_by_asking_for_the_band(hip, case):
    """30 seeded cycles with reading_interval() called before every pdf_update() (lorentz_full: with a speculative
    variance_full sweep enqueued ahead; noise7: a noise-parameter object) against the same run without it: settings,
    resample flags, weights, cloud and generator state."""
    from optbayesexpt_amd import _state
    watched, got, bands = _run(case, 30, True)
    plain, want, _ = _run(case, 30, False)
    assert got["picks"] == want["picks"] and got["resampled"] == want["resampled"]
    assert any(want["resampled"])
    assert_array_equal(_bits(got["weights"]), _bits(want["weights"]))
    assert_array_equal(_bits(got["particles"]), _bits(want["particles"]))
    np.testing.assert_equal(got["rng"], want["rng"])
    assert set(_state.snapshot(watched)) == set(_state.snapshot(plain))          # nothing added to snapshots
    assert set(vars(watched)) == set(vars(plain))                                # ... nor to the object
    assert sum(lo <= yv <= hi for lo, hi, yv in bands) >= 24                     # honest readings fall inside


def test_restored_and_copied_objects(hip, tmp_path):
    import optbayesexpt_amd as obe
    for case, sigma in (("strict4096", cases.SIGMA), ("noise7", None)):
        o = cases.build(case)
        cases.run(o, case, 0, 5)
        x = (np.linspace(2.0, 4.0, 9),)
        want = o.reading_quantile((0.025, 0.5, 0.975), x, sigma, full_output=True)
        assert want[1]["unconverged"] == 0
        path = str(tmp_path / (case + ".state"))
        obe.save(o, path)
        for other in (obe.load(path), copy.deepcopy(o)):
            got = other.reading_quantile((0.025, 0.5, 0.975), x, sigma, full_output=True)
            assert_array_equal(_bits(got[0]), _bits(want[0]))
            assert_array_equal(got[1]["passes"], want[1]["passes"])


# ------------------------------------------------------------------------------------------------ 7. the example
def test_reading_band_example(hip):
    spec = importlib.util.spec_from_file_location("reading_band", os.path.join(ROOT, "examples", "reading_band.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        true_pars, fraction, n_readings, (curve_lo, curve_hi, read_lo, read_hi) = mod.main(
            n_measure=40, n_samples=20000, n_check=400, seed=3, quiet=True)
    assert n_readings == 440
    # 95 % +- 5 binomial standard deviations of 400 readings: a condition on the example's seed, not a measurement
    assert 0.90 <= fraction <= 0.99, fraction
    assert read_lo.shape == read_hi.shape == curve_lo.shape == (1, 200)
    assert np.all(read_lo < curve_lo) and np.all(curve_hi < read_hi)            # the noise widens the band everywhere
    assert np.all(read_hi - read_lo > 2 * 1.9 * 500.0)


def test_worst_errors_are_reported(hip):
    """(runs last of the comparisons: the worst residual / tolerance ratio and the worst pass count of this file)"""
    print(f"worst residual: {WORST['ratio'][0]:.3g} of its tolerance ({WORST['ratio'][1]})")
    print(f"worst pass count: {WORST['passes'][0]} ({WORST['passes'][1]})")
    assert WORST["ratio"][1] and WORST["passes"][0] >= 1
