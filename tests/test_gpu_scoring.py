"""Device-side scoring of measurements (OptBayesExpt.predictive_logpdf / predictive_cdf / predictive_pvalue;
csrc/obe_predict.hip, K11) against tests/_scoring_oracle.py on the rows y = eval_over_all_parameters((x_r,)) of the
product itself, against the reference's likelihood arithmetic (the oracle classes, the sum t of obe_bayes_update_model)
and on golden-trajectory posteriors.

Tolerances: |d log p| <= 1e-10 max(1, |log p|) (the absolute error of a log-term is a few eps |l|, contributing terms
lie within 745 of the largest, fixed-order positive sums add N eps at worst); each tail 1e-10 relative on records whose
two oracle tails both exceed 1e-280 (asserted from the oracle alone before the device is asked).  Run to run: the same
bits.  The worst error / tolerance ratios seen are printed by test_worst_errors_are_reported."""
import importlib.util
import json
import os
import subprocess
import sys
import types
import warnings

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _fn_models
import _scoring_oracle as oracle
import _state_cases as cases
from optbayesexpt_amd import _lib, _scoring

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = (1 << 20) + 3
WORST = {}
# the launch geometry of csrc/obe_predict.hip: 64 records per wave, chunks of at least 256 particles in whole waves,
# at most 8192 waves per launch
WAVE, MIN_CHUNK, WAVES = 64, 256, 8192


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _chunk_len(n, n_r):
    tiles = (n_r + WAVE - 1) // WAVE
    chunks = max(1, min((n + MIN_CHUNK - 1) // MIN_CHUNK, max(1, WAVES // tiles)))
    return ((n + chunks - 1) // chunks + WAVE - 1) // WAVE * WAVE


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


def _points(name, g, n_r):
    if name == "coil":
        return g.uniform(1.0e4, 6.0e4, n_r)[None, :]
    if name == "rabi":
        return np.array([g.uniform(0.0, 3.0, n_r), g.uniform(-4.0, 4.0, n_r)])
    if name == "expression":
        return g.uniform(-3.0, 3.0, n_r)[None, :]
    return g.uniform(1.5, 4.5, n_r)[None, :]


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
    """y (n_r, C, N_p): the product's own model values, one record's setting at a time."""
    return np.stack([np.asarray(o.eval_over_all_parameters(tuple(float(v) for v in x[:, r]))).reshape(o.n_channels, -1)
                     for r in range(x.shape[1])])


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


def _weights(g, cloud):
    w = g.random(cloud.shape[1]) * np.exp(-0.5 * ((cloud[0] - np.median(cloud[0])) / (np.std(cloud[0]) + 1e-300)) ** 2)
    return w / w.sum()


def _readings(g, y, w, sig_rows=None):
    """Known sigma (C, n_r) that differs per record and channel (None with noise rows), and readings (C, n_r) within a
    few sigma of a weighted particle's model value: some weighted particle has |z| of order 1."""
    n_r, n_c, n = y.shape
    heavy = np.nonzero(w > 0)[0] if sig_rows is None else np.nonzero((w > 0) & np.all(sig_rows > 0, axis=0))[0]
    pick = heavy[g.integers(0, heavy.size, n_r)]
    if sig_rows is None:
        spread = np.array([[np.std(y[r, c]) for r in range(n_r)] for c in range(n_c)])
        sigma = (spread + 1e-3 * np.abs(y[:, :, 0].T) + 1e-12) * g.uniform(0.25, 2.0, (n_c, n_r))
        at = sigma
    else:
        sigma, at = None, sig_rows[:, pick]
    ym = np.array([[y[r, c, pick[r]] for r in range(n_r)] for c in range(n_c)]) + at * g.normal(0.0, 1.5, (n_c, n_r))
    return ym, sigma


# ------------------------------------------------------------------------------------------------- the checks
def _note(kind, err, tol, what):
    ratio = err / tol if tol > 0 else (0.0 if err == 0 else np.inf)
    if ratio >= WORST.get(kind, (0.0, ""))[0]:
        WORST[kind] = ratio, what


def _check(what, o, x, ym, sigma, y, w, sig_rows=None, plain_tails=True, records=None):
    """The three methods for the records (x, ym, sigma) against the oracle fed y (n_r, C, N_p); ``records``: the ones
    to compare (all).  ``plain_tails``: every compared tail must exceed 1e-280 and is held to 1e-10 relative; else a
    tail the oracle has as 0 or NaN must be that exactly, any other within 1e-10 relative."""
    n_r, n_c = y.shape[0], y.shape[1]
    want = []
    for r in (range(n_r) if records is None else records):
        sg = sigma[:, r] if sig_rows is None else sig_rows
        lo, hi = oracle.tails(y[r], w, ym[:, r], sg)
        if plain_tails:
            assert np.all(lo > 1e-280) and np.all(hi > 1e-280), (what, r, lo, hi)       # the choice of records: CPU only
        want.append((r, oracle.logpdf(y[r], w, ym[:, r], sg), lo, hi))
    logp = o.predictive_logpdf(x, ym, sigma)
    lower = o.predictive_cdf(x, ym, sigma)
    upper = o.predictive_cdf(x, ym, sigma, upper=True)
    p = o.predictive_pvalue(x, ym, sigma)
    assert logp.shape == (x.shape[1],) and lower.shape == upper.shape == p.shape == (n_c, x.shape[1])
    assert logp.dtype == lower.dtype == upper.dtype == p.dtype == np.float64
    assert_array_equal(_bits(p), _bits(np.minimum(2.0 * np.minimum(lower, upper), 1.0)), err_msg=f"{what}: p-value")
    assert_array_equal(_bits(o.predictive_logpdf(x, ym, sigma)), _bits(logp), err_msg=f"{what}: run to run")
    assert_array_equal(_bits(o.predictive_cdf(x, ym, sigma)), _bits(lower), err_msg=f"{what}: run to run")
    assert_array_equal(_bits(o.predictive_cdf(x, ym, sigma, upper=True)), _bits(upper), err_msg=f"{what}: run to run")
    for r, lp, lo, hi in want:
        if np.isfinite(lp):
            err, tol = abs(logp[r] - lp), oracle.logpdf_tolerance(lp)
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


# ------------------------------------------------------------------------- 1. shapes: records x particles
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, (1 << 14) + 3])
def test_shapes_lorentzian(hip, n):
    """Both sides of the wave of 64 records and of the chunk of 256 particles; one particle; more than one chunk."""
    for n_r in (1, 63, 64, 65, 130):
        g = np.random.default_rng([n, n_r])
        cloud = _prior("lorentz1", g, n)
        w = _weights(g, cloud)
        o = _object("lorentz1", cloud, w)
        x = _points("lorentz1", g, n_r)
        y = _rows(o, x)
        ym, sigma = _readings(g, y, w)
        _check(f"lorentz1 {n_r} x {n}", o, x, ym, sigma, y, w)


def test_a_thousand_records_at_a_million_particles(hip):
    """1 000 records x 2^20 + 3 particles: eight different records against the oracle, each repeated in 125 lanes of 16
    waves, which must all hold the same bits."""
    g = np.random.default_rng(1000)
    cloud = _prior("lorentz1", g, BIG)
    cloud[0] = 3.0 + 0.05 * g.normal(size=BIG)
    w = _weights(g, cloud)
    o = _object("lorentz1", cloud, w)
    x8 = np.linspace(2.6, 3.4, 8)[None, :]
    y8 = _rows(o, x8)
    ym8, sigma8 = _readings(g, y8, w)
    x, ym, sigma = (np.tile(a, 125) for a in (x8, ym8, sigma8))
    assert x.shape == (1, 1000) and 400 < -(-BIG // _chunk_len(BIG, 1000)) <= 512       # chunks
    logp, lower, upper = _check("lorentz1 1000 x BIG", o, x, ym, sigma, y8, w, records=range(8))
    for got in (logp[None, :], lower, upper):
        assert_array_equal(_bits(got), _bits(np.tile(got[:, :8], 125)))


@pytest.mark.parametrize("name", ["lorentz7", "coil", "rabi", "expression", "function"])
def test_models(hip, name):
    for n, n_r in ((5000, 65), (300, 3)):
        g = np.random.default_rng([sum(map(ord, name)), n])
        cloud = _prior(name, g, n)
        w = _weights(g, cloud)
        o = _object(name, cloud, w)
        assert (o._mlib is not o._lib) == (name in ("expression", "function"))          # plugins serve their own model
        x = _points(name, g, n_r)
        y = _rows(o, x)
        ym, sigma = _readings(g, y, w)
        assert y.shape[1] == (2 if name == "coil" else 1) and x.shape[0] == (2 if name == "rabi" else 1)
        _check(f"{name} {n_r} x {n}", o, x, ym, sigma, y, w)


@pytest.mark.parametrize("name,rows", [("lorentz1", (3,)), ("coil", (3, 4)), ("coil", (4, 4))])
def test_noise_parameter_class(hip, name, rows):
    for n, n_r in ((5000, 65), (257, 2)):
        g = np.random.default_rng([sum(map(ord, name)), n, len(set(rows))])
        x = _points(name, g, n_r)
        cloud = _noise_cloud(name, g, n, rows, x)
        w = _weights(g, cloud)
        o = _object(name, cloud, w, noise_rows=rows if len(rows) > 1 else rows[0])
        y = _rows(o, x)
        sig_rows = cloud[list(rows)]
        ym, _ = _readings(g, y, w, sig_rows)
        _check(f"noise {name} {rows} {n_r} x {n}", o, x, ym, None, y, w, sig_rows)
        with pytest.raises(ValueError, match="noise parameter"):
            o.predictive_logpdf(x, ym, 1.0)


# ----------------------------------------------------------------------- 2. the rescale branch, on purpose
def _spanning_case(g, n):
    """A Lorentzian cloud and two records with a small sigma: the log-terms of record 0 span more than 10^4."""
    cloud = _prior("lorentz1", g, n)
    w = g.random(n) + 0.1
    w /= w.sum()
    x = np.array([[3.0, 2.7]])
    sigma = np.array([[10.0, 25.0]])
    return cloud, w, x, sigma


def _terms(cloud, w, x, ym, sigma):
    o = _object("lorentz1", cloud, w)
    y = _rows(o, x)
    return o, y, np.asarray(oracle.log_terms(y[0], ym[:, 0], sigma[:, 0]), dtype=np.float64)


@pytest.mark.parametrize("order", ["ascending", "descending", "alternating"])
def test_clouds_sorted_by_likelihood(hip, order):
    g = np.random.default_rng(21)
    n = (1 << 14) + 3
    cloud, w, x, sigma = _spanning_case(g, n)
    ym = np.array([[49500.0, 49200.0]])
    _, _, l = _terms(cloud, w, x, ym, sigma)
    assert l.max() - l.min() > 1e4
    rank = np.argsort(l)
    if order == "descending":
        rank = rank[::-1]
    elif order == "alternating":          # worst, best, second worst, second best, ...
        both = np.empty(n, dtype=np.int64)
        both[0::2], both[1::2] = rank[:(n + 1) // 2], rank[::-1][:n // 2]
        rank = both
    cloud, w = cloud[:, rank], w[rank]
    o, y, l = _terms(cloud, w, x, ym, sigma)
    if order == "ascending":
        assert np.all(np.diff(l) >= 0)    # every particle raises the running maximum: a rescale each time
    _check(f"sorted {order}", o, x, ym, sigma, y, w, plain_tails=False)


@pytest.mark.parametrize("where", ["first", "last", "first of the last chunk", "last of a middle chunk"])
def test_the_best_particle_at_a_chunk_boundary(hip, where):
    g = np.random.default_rng(22)
    n = (1 << 14) + 3
    chunk = _chunk_len(n, 2)
    assert chunk == 256 and n % chunk == 3
    at = {"first": 0, "last": n - 1, "first of the last chunk": n - 3, "last of a middle chunk": 31 * chunk + chunk - 1}[where]
    cloud, w, x, sigma = _spanning_case(g, n)
    ym = np.array([[49500.0, 49200.0]])
    _, _, l = _terms(cloud, w, x, ym, sigma)
    best = int(np.argmax(l))
    cloud[:, [at, best]] = cloud[:, [best, at]]
    w[[at, best]] = w[[best, at]]
    o, y, l = _terms(cloud, w, x, ym, sigma)
    assert int(np.argmax(l)) == at and np.sort(l)[-1] - np.sort(l)[-2] > 0
    _check(f"best particle {where}", o, x, ym, sigma, y, w, plain_tails=False)


# ------------------------------------------------------------------- 3. exclusions and non-finite values
def test_weights_that_do_not_count_and_model_values_that_are_not_finite(hip):
    g = np.random.default_rng(31)
    n = 600                                                  # three chunks
    cloud = _prior("lorentz1", g, n)
    w = _weights(g, cloud)
    w[[0, 1, 255, 256, 599]] = [0.0, np.nan, -0.25, 0.0, np.nan]
    cloud[0, 0], cloud[1, 1], cloud[1, 255], cloud[0, 256] = np.nan, np.inf, -np.inf, np.nan      # ignored: no weight
    cloud[0, 10], cloud[1, 300], cloud[1, 301] = np.nan, np.inf, -np.inf                          # weighted: excluded
    o = _object("lorentz1", cloud, w)
    x = _points("lorentz1", g, 5)
    y = _rows(o, x)
    assert np.all(np.isnan(y[:, 0, 10])) and np.all(y[:, 0, 300] == np.inf) and np.all(y[:, 0, 301] == -np.inf)
    good = np.isfinite(y).all(axis=(0, 1))
    ym, sigma = _readings(g, np.where(good, y, 50000.0), np.where(good, w, 0.0))
    logp, lower, upper = _check("non-finite", o, x, ym, sigma, y, w)
    assert np.all(np.isfinite(logp))
    # the same cloud without those particles' weights: the same density terms, another sum w
    w2 = np.where(good, w, 0.0)
    o2 = _object("lorentz1", np.where(good, cloud, 3.0), w2)
    shift = np.log(np.sum(oracle.clean(w2)) / np.sum(oracle.clean(w)))
    assert np.all(np.abs(o2.predictive_logpdf(x, ym, sigma) + shift - logp) <= 1e-10 * np.maximum(1.0, np.abs(logp)))


def test_noise_rows_that_are_not_positive(hip):
    g = np.random.default_rng(32)
    n = 600
    cloud = np.vstack([_prior("coil", g, n), g.uniform(0.5, 2.0, (2, n))])
    w = _weights(g, cloud)
    cloud[3, [5, 256, 257]] = [0.0, -1.0, np.nan]
    cloud[4, [6, 599]] = [np.nan, -0.0]
    cloud[3, 7], w[7] = -3.0, 0.0
    o = _object("coil", cloud, w, noise_rows=(3, 4))
    x = _points("coil", g, 5)
    y = _rows(o, x)
    sig_rows = cloud[[3, 4]]
    ym, _ = _readings(g, y, w, sig_rows)
    _check("bad noise rows", o, x, ym, None, y, w, sig_rows)
    # every particle excluded: log p = -inf, tails 0
    cloud[3] = -np.abs(cloud[3])
    o = _object("coil", cloud, w, noise_rows=(3, 4))
    logp, lower, upper = _check("all excluded", o, x, ym, None, y, w, cloud[[3, 4]], plain_tails=False)
    assert np.all(logp == -np.inf) and not lower.any() and not upper.any()
    assert_array_equal(o.predictive_pvalue(x, ym), np.zeros((2, 5)))


def test_no_weight_at_all_gives_nan(hip):
    g = np.random.default_rng(33)
    cloud = _prior("lorentz1", g, 300)
    x = _points("lorentz1", g, 3)
    for w in (np.zeros(300), np.full(300, np.nan), -np.ones(300)):
        o = _object("lorentz1", cloud, w)
        assert np.all(np.isnan(o.predictive_logpdf(x, np.full(3, 49000.0), 500.0)))
        assert np.all(np.isnan(o.predictive_cdf(x, np.full(3, 49000.0), 500.0)))
        assert np.all(np.isnan(o.predictive_pvalue(x, np.full(3, 49000.0), 500.0)))


def test_a_reading_forty_sigma_out(hip):
    """|z| of about 40 for every particle: the far tail is exactly 0.0, the near one 1 within 1e-10."""
    g = np.random.default_rng(34)
    n = 5000
    cloud = np.array([3.0, -1000.0, 50000.0])[:, None] * (1.0 + 1e-6 * g.normal(size=(3, n)))
    w = _weights(g, g.normal(size=(1, n)))
    o = _object("lorentz1", cloud, w)
    x = np.array([[3.0, 4.0, 3.0, 4.0]])
    y = _rows(o, x)
    sigma = np.full((1, 4), 10.0)
    ym = y[:, 0, 0][None, :] + np.array([[400.0, 400.0, -400.0, -400.0]])
    z = (y[:, 0, :] - ym[0][:, None]) / 10.0
    assert np.all(np.abs(np.abs(z) - 40.0) < 0.5)
    logp, lower, upper = _check("forty sigma", o, x, ym, sigma, y, w, plain_tails=False)
    assert_array_equal(upper[0, :2], [0.0, 0.0])             # readings above every particle's curve: P(Y >= y) = 0
    assert_array_equal(lower[0, 2:], [0.0, 0.0])
    assert np.all(np.abs(lower[0, :2] - 1.0) <= 1e-10) and np.all(np.abs(upper[0, 2:] - 1.0) <= 1e-10)
    assert np.all(np.isfinite(logp)) and np.all(logp < -790.0)
    assert_array_equal(o.predictive_pvalue(x, ym, sigma), np.zeros((1, 4)))


# ------------------------------------------------------------------- 4. tied to the reference's arithmetic
@pytest.mark.parametrize("name,rows", [("lorentz1", None), ("coil", None), ("lorentz1", (3,)), ("coil", (3, 4))])
def test_one_particle_is_the_reference_likelihood(hip, name, rows):
    """exp(log p) (2 pi)^(C/2) of a cloud of one particle against the oracle classes' likelihood() (oracle/obe_oracle.py:
    the reference's obe_base.py:451-461 and obe_noiseparam.py:109-120, operation by operation)."""
    from oracle import obe_oracle
    g = np.random.default_rng([sum(map(ord, name)), 41])
    x = _points(name, g, 9)
    cloud = _noise_cloud(name, g, 1, rows, x) if rows else _prior(name, g, 1)
    o = _object(name, cloud, np.ones(1), noise_rows=None if rows is None else (rows if len(rows) > 1 else rows[0]))
    n_c = o.n_channels
    y = _rows(o, x)
    sig = cloud[list(rows)] if rows else None
    ym, sigma = _readings(g, y, np.ones(1), sig)
    logp = o.predictive_logpdf(x, ym, sigma)
    for r in range(9):
        if rows:
            fake = types.SimpleNamespace(parameters=cloud, noise_parameter_index=np.array(rows), choke=None)
            want = obe_oracle.OracleOptBayesExptNoiseParameter.likelihood(fake, y[r], (None, ym[:, r]))
        else:
            fake = types.SimpleNamespace(choke=None)
            want = obe_oracle.OracleOptBayesExpt.likelihood(fake, y[r], (None, ym[:, r], sigma[:, r]))
        want = float(np.asarray(want).reshape(-1)[0])
        got = np.exp(logp[r]) * (2.0 * np.pi) ** (n_c / 2.0)
        assert want > 1e-300 and abs(got - want) <= 1e-10 * want, (name, rows, r, got, want)
        _note("one particle vs likelihood()", abs(got - want), 1e-10 * want, f"{name} {rows}")


@pytest.mark.parametrize("name,rows", [("lorentz1", None), ("coil", None), ("lorentz1", (3,)), ("coil", (3, 4))])
def test_density_is_the_updates_sum_t(hip, name, rows):
    """Normalised weights: log p + (C / 2) log 2 pi against log(sum t) of obe_bayes_update_model (h_out[0]) on a copy of
    the same weights, record by record; no choke.  Readings within 5 sigma of the cloud's mean curve."""
    import torch
    g = np.random.default_rng([sum(map(ord, name)), 42])
    n = 20000
    x = _points(name, g, 6)
    cloud = _noise_cloud(name, g, n, rows, x) if rows else _prior(name, g, n)
    w = _weights(g, cloud)
    o = _object(name, cloud, w, noise_rows=None if rows is None else (rows if len(rows) > 1 else rows[0]))
    n_c = o.n_channels
    mean, spread = o.predict(x)
    if rows:
        sigma, s_mean = None, np.sqrt(np.sum(w * cloud[list(rows)] ** 2, axis=1))[:, None]
    else:                                  # of the size of the cloud's own spread: the mean curve is within reach
        sigma = s_mean = (spread + 1e-3 * np.abs(mean) + 1e-12) * g.uniform(0.5, 2.0, mean.shape)
    ym = mean + s_mean * g.uniform(-3.0, 3.0, mean.shape)
    logp = o.predictive_logpdf(x, ym, sigma)
    par, wd = o._parameters.tensor(), o._weights.tensor()
    ws = torch.empty(o._ws_bytes // 8 + 1, dtype=torch.float64, device=o._device)
    h_out = np.zeros(16)
    for r in range(6):
        w_copy = wd.clone()
        st = np.zeros(_lib.OBE_MAX_SETDIMS)
        st[:x.shape[0]] = x[:, r]
        yy, ss = np.zeros(_lib.OBE_MAX_CHANNELS), np.ones(_lib.OBE_MAX_CHANNELS)
        yy[:n_c] = ym[:, r]
        if sigma is not None:
            ss[:n_c] = sigma[:, r]
        o._mlib.call("obe_bayes_update_model", o._model_struct, par.data_ptr(), par.shape[1], n, w_copy.data_ptr(),
                     _lib.host_ptr(st), _lib.host_ptr(yy), None if rows else _lib.host_ptr(ss),
                     _lib.host_ptr(o._noise_rows) if rows else None, n_c, float("nan"), ws.data_ptr(), o._ws_bytes,
                     _lib.host_ptr(h_out), o._stream())
        torch.cuda.synchronize()
        want = float(np.log(h_out[0]))
        got = logp[r] + 0.5 * n_c * np.log(2.0 * np.pi)
        assert h_out[0] > 1e-200, h_out[0]                               # far from underflow
        tol = oracle.logpdf_tolerance(want)
        _note("log p vs the update's sum t", abs(got - want), tol, f"{name} {rows}")
        assert abs(got - want) <= tol, (name, rows, r, got, want)
    assert_array_equal(_bits(np.array(o.particle_weights)), _bits(w))    # the object's own weights were not touched


@pytest.mark.parametrize("name,cycles", [("lorentz3_opt", 25), ("coil_2ch_noise", 20)])
def test_golden_trajectory_posteriors(hip, name, cycles):
    """The posterior after ``cycles`` cycles of a golden trajectory scores every recorded reading of that trajectory."""
    import _replay
    import optbayesexpt_amd as obe
    fx = _replay.load_traj(name)
    meta = fx["meta"]
    model = {"lorentzian": obe.models.lorentzian(1), "coil": obe.models.coil()}[meta["model"]]
    o = _replay.construct(fx, obe.OptBayesExpt, obe.OptBayesExptNoiseParameter, model)
    noise = meta["cls"] != "base"
    log_evidence = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for cyc in range(cycles):
            xs = o.opt_setting()
            yv = fx["y_meas"][cyc]
            yv = float(yv[0]) if yv.size == 1 else yv
            record = (xs, yv) if noise else (xs, yv, meta["sigma_meas"])
            one = o.predictive_logpdf(*record)
            assert isinstance(one, float) and np.isfinite(one)
            log_evidence += one
            o.pdf_update(record)
    print(f"{name}: log evidence of {cycles} readings {log_evidence:.6f}")
    w = np.array(o.particle_weights)
    cloud = np.array(o.particles)
    x = np.asarray(fx["setval_0"])[fx["chosen_index"]][None, :]
    ym = np.ascontiguousarray(fx["y_meas"].T)
    y = _rows(o, x)
    if noise:
        rows = [int(r) for r in o._noise_rows[:o.n_channels]]
        _check(name, o, x, ym, None, y, w, cloud[rows], plain_tails=False)
    else:
        _check(name, o, x, ym, meta["sigma_meas"] * np.ones_like(ym), y, w, plain_tails=False)
        assert_array_equal(_bits(o.predictive_logpdf(x, ym, meta["sigma_meas"])),
                           _bits(o.predictive_logpdf(x, ym, np.full_like(ym, meta["sigma_meas"]))))


# --------------------------------------------------------------------------------------- 5. no side effects
def _score_all(o, record):
    return o.predictive_logpdf(*record), o.predictive_cdf(*record), o.predictive_cdf(*record, upper=True), \
        o.predictive_pvalue(*record)


def _flags(o):
    return (o._particles.version, o._weights.version, o._particles._host_valid, o._weights._host_valid,
            o._particles._dev_valid, o._weights._dev_valid, o._mom_host_key, o._mom_dev_key, o._cdf_key, o._sumsq_key,
            json.dumps(o.rng.bit_generator.state, sort_keys=True, default=str))


def _run(case, n, watch):
    o = cases.build(case)
    picks, resampled, scores = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for cyc in range(n):
            x = o.opt_setting()
            picks.append(int(o.last_setting_index))
            record = cases.measure(o, case, cyc, x)
            if watch:
                before = _flags(o), o.sweep_state()
                scores.append(_score_all(o, record))
                assert (_flags(o), o.sweep_state()) == before, f"cycle {cyc}"
            o.pdf_update(record)
            resampled.append(bool(o.just_resampled))
    return o, cases.outcome(o, picks, resampled), scores


@pytest.mark.parametrize("case", ["lorentz_full", "noise7"])
def test_a_trajectory_is_unchanged_by_scoring_its_readings(hip, case):
    """30 seeded cycles with the three methods called on the record before every pdf_update() (lorentz_full: with a
    speculative variance_full sweep enqueued ahead; noise7: a noise-parameter object) against the same run without
    them: settings, resample flags, weights, cloud and generator state."""
    from optbayesexpt_amd import _state
    watched, got, scores = _run(case, 30, True)
    plain, want, _ = _run(case, 30, False)
    assert got["picks"] == want["picks"] and got["resampled"] == want["resampled"]
    assert any(want["resampled"])
    assert_array_equal(_bits(got["weights"]), _bits(want["weights"]))
    assert_array_equal(_bits(got["particles"]), _bits(want["particles"]))
    np.testing.assert_equal(got["rng"], want["rng"])
    assert set(_state.snapshot(watched)) == set(_state.snapshot(plain))          # nothing added to snapshots
    assert all(isinstance(s[0], float) and np.isfinite(s[0]) and s[1].shape == (1, 1) for s in scores)
    assert sum(s[3][0, 0] > 1e-3 for s in scores) >= 25                         # honest readings are plausible


def test_host_edits_are_uploaded_first(hip):
    g = np.random.default_rng(51)
    n = 3000
    cloud = _prior("lorentz1", g, n)
    w = _weights(g, cloud)
    o = _object("lorentz1", cloud, w)
    x = _points("lorentz1", g, 5)
    y = _rows(o, x)
    ym, sigma = _readings(g, y, w)
    _check("before the edits", o, x, ym, sigma, y, w)
    o.particle_weights[cloud[0] > 3.0] = 0                           # in place, by host code
    w2 = np.where(cloud[0] > 3.0, 0.0, w)
    _check("edited weights", o, x, ym, sigma, y, w2, plain_tails=False)
    o.particles[2] += 100.0                                          # the background row
    y2 = _rows(o, x)
    assert np.all(y2 != y)
    _check("edited particles", o, x, ym, sigma, y2, w2, plain_tails=False)
    o.particle_weights = w[:-1]
    with pytest.raises(ValueError, match="different lengths"):
        o.predictive_logpdf(x, ym, sigma)


def test_argument_forms_on_a_live_object(hip):
    g = np.random.default_rng(52)
    cloud = _prior("coil", g, 2000)
    o = _object("coil", cloud, _weights(g, cloud))
    x = _points("coil", g, 4)
    y = _rows(o, x)
    ym, sigma = _readings(g, y, np.array(o.particle_weights))
    whole = o.predictive_logpdf(x, ym, sigma)
    one = o.predictive_logpdf((x[0, 2],), ym[:, 2], sigma[:, 2])                 # a record as pdf_update takes it
    assert isinstance(one, float) and _bits(one) == _bits(whole[2])
    assert_array_equal(_bits(o.predictive_logpdf((x[0],), ym, sigma)), _bits(whole))          # a tuple of points
    same = o.predictive_logpdf((x[0, 1],), np.tile(ym[:, 1:2], 3), sigma[:, 1])               # broadcast to 3 records
    assert_array_equal(_bits(same), _bits(np.full(3, whole[1])))
    tails = o.predictive_cdf((x[0, 1],), ym[:, 1], sigma[:, 1]), o.predictive_cdf((x[0, 1],), ym[:, 1], sigma[:, 1], True)
    assert tails[0].shape == (2, 1) and np.all(np.abs(tails[0] + tails[1] - 1.0) < 1e-12)
    with pytest.raises(ValueError):
        o.predictive_logpdf(x, ym)                                               # sigma is required on the base class
    with pytest.raises(ValueError):
        o.predictive_logpdf(x, ym[0], sigma)                                     # one channel of two


def test_requests_larger_than_one_call_are_tiled(hip, monkeypatch):
    g = np.random.default_rng(53)
    cloud = _prior("coil", g, 640)
    o = _object("coil", cloud, _weights(g, cloud))
    x = _points("coil", g, 200)
    y = _rows(o, x)
    ym, sigma = _readings(g, y, np.array(o.particle_weights))
    want = _score_all(o, (x, ym, sigma))
    monkeypatch.setattr(_scoring, "RECORDS_PER_CALL", 37)
    for a, b in zip(_score_all(o, (x, ym, sigma)), want):
        assert_array_equal(_bits(a), _bits(b))


# --------------------------------------------------------------------------- 6. example and delivery audit
def test_outlier_check_example(hip):
    spec = importlib.util.spec_from_file_location("outlier_check", os.path.join(ROOT, "examples", "outlier_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        true_pars, mean, std, history, log_evidence = mod.main(n_measure=40, n_samples=20000, seed=3, quiet=True)
    assert [h[0] for h in history] == list(range(40))
    glitches = [h for h in history if h[1]]
    honest = [h for h in history if not h[1]]
    assert len(glitches) == 4 and all(h[2] < 1e-6 and not h[3] for h in glitches), glitches
    assert all(h[2] > 1e-3 and h[3] for h in honest), [h for h in honest if h[2] <= 1e-3]
    assert np.isfinite(log_evidence) and log_evidence < 0
    assert abs(mean[0] - true_pars[0]) < 5 * std[0] + 0.01                      # the glitches did not reach the fit


def test_worst_errors_are_reported(hip):
    """(runs last of the comparisons: the worst error / tolerance ratios seen by this file's checks)"""
    for kind, (ratio, what) in sorted(WORST.items()):
        print(f"worst {kind}: {ratio:.3g} of its tolerance ({what})")
    assert WORST


def test_this_file_under_the_delivery_audit(hip, tmp_path):
    """Once more in a child process with OBE_CHECK_DELIVERY=1 (the pattern of tests/test_gpu_predictive.py): no armed
    host word is read, no landing zone is released with armed words."""
    assert "OBE_SCORING_AUDIT_CHILD" not in os.environ, "the audited child must not start a child of its own"
    report = tmp_path / "audit.jsonl"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"), OBE_CHECK_DELIVERY="1",
               OBE_AUDIT_REPORT=str(report), OBE_SCORING_AUDIT_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider", "-k", "not test_this_file_under_the_delivery_audit"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "DeliveryError" not in r.stdout + r.stderr and " passed" in r.stdout and "skipped" not in r.stdout
    assert "1 deselected" in r.stdout
    rows = [json.loads(line) for line in report.read_text().splitlines()]
    assert rows and not any(row["pending_violations"] for row in rows), rows
    assert sum(row["reads"] for row in rows) > 100
