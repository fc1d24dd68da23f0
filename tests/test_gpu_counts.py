"""Count-aware scoring and reading bands on the device (CountReadings.count_*; csrc/obe_counts.hip, K20) against
tests/_counts_oracle.py.

Inputs (tests/_counts_oracle.py; checked without a device in tests/test_counts_host.py): the one-peak Lorentzian as a
success probability in [0.1, 0.9] and as a count rate in [2, 12] (lambda in [16, 96] at exposure 8), wide and converged
clouds, the two-channel formulae RAMSEY and DECAYS through their plugins, all with the binomial tests' non-uniform
weights; a high-rate case (lambda 750 .. 1000, where e^-lambda underflows) and crafted probabilities 0 and 1.  The oracle
is fed the NumPy form of the same curves: its values and the device's differ by a few ulp, ~1e-15 relative in a row.

Tolerances (tests/test_gpu_poisson.py's): the rows Pbar_c(k) 1e-10 relative — at most 4097 non-negative terms in a
fixed order lose N eps = 4.5e-13, the block's start value exp(k0 log lambda - lambda - log k0!) carries a few ulp of an
exponent <= 9e3, 3e-12, and the recurrence (1 + 3 eps) per outcome over at most 63 outcomes —; binomial tails and
exp(count_logpmf) 1e-10 relative (sums of non-negative terms); the Poisson mass above the window and the upper tails
that include it 1e-10 absolute, a difference of numbers near 1, and 1e-10 relative as well where the oracle's value is
>= 1e-3; quantiles exactly the oracle's whole numbers (test_counts_host.py asserts that every cdf value keeps 1e-9 from
every level)."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _counts_oracle as oracle
from _counts_oracle import BINOMIAL, POISSON

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-10, 1e-10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = oracle.LEVELS


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ the objects
def _models():
    import _counts_models
    return _counts_models.expression_models()


def _object(law, kind, n, side, grid=None):
    """The class of ``law`` on the input ``oracle.case(law, kind, n)`` with its weights."""
    import optbayesexpt_amd as obe
    cloud, w, _ = oracle.case(law, kind, n)
    if kind == "two":
        model, grid, consts = _models()["ramsey" if law == BINOMIAL else "decays"], oracle.TIMES, ()
    else:
        model, grid, consts = obe.models.lorentzian(1), oracle.GRID if grid is None else grid, (0.1,)
    if law == BINOMIAL:
        o = obe.OptBayesExptBinomial(model, (grid,), cloud, consts, shots=side, scale=False)
    else:
        o = obe.OptBayesExptPoisson(model, (grid,), cloud, consts, exposure=side, scale=False,
                                    utility_method="variance_approx")
    o.particle_weights = w
    return o


def _row_object(law, values, weights, side):
    """A one-channel object whose model value IS the particle's parameter (tests/_own_records_models.py)."""
    import optbayesexpt_amd as obe
    import _own_records_models
    model = _own_records_models.expression_models()["row"]
    cloud = np.asarray(values, dtype=np.float64).reshape(1, -1)
    if law == BINOMIAL:
        o = obe.OptBayesExptBinomial(model, (np.array([0.0, 1.0]),), cloud, (), shots=side, scale=False)
    else:
        o = obe.OptBayesExptPoisson(model, (np.array([0.0, 1.0]),), cloud, (), exposure=side, scale=False)
    o.particle_weights = np.asarray(weights, dtype=np.float64)
    return o


def _close_table(what, law, got, want, shots=None, tiny_rows=False):
    """The module docstring's tolerances for a table (n_points, C, count_max + 2).  Every row of the oracle is >= 1e-200
    and compared relatively (binomial: up to the shots), unless the case is one of ``tiny_rows`` (the high-rate case),
    whose rows below 1e-200 are held to that bound absolutely."""
    assert got.shape == want.shape, what
    rows, ref = got[:, :, :-1], want[:, :, :-1]
    big = ref >= 1e-200
    if not tiny_rows:
        upto = rows.shape[2] if shots is None else min(rows.shape[2], int(shots) + 1)
        assert np.all(big[:, :, :upto]), f"{what}: the oracle has a row of {ref[:, :, :upto].min():.3g}, below 1e-200"
    err = np.abs(rows[big] - ref[big]) / ref[big]
    print(f"{what}: rows off by {err.max() if err.size else 0:.3g} relative, smallest compared {ref[big].min():.3g}")
    assert np.all(err <= RTOL), f"{what}: a row off by {err.max():.3g} relative"
    assert np.all(np.abs(rows[~big]) <= 1e-200), what
    if law == BINOMIAL and shots is not None:                       # (beyond the shots: exactly nothing)
        assert np.all(rows[:, :, int(shots) + 1:] == 0.0), what
    above, ref = got[:, :, -1], want[:, :, -1]
    err = np.abs(above - ref)
    print(f"{what}: mass above off by {err.max():.3g} absolute")
    assert np.all(err <= ATOL), f"{what}: the mass above off by {err.max():.3g}"
    sure = ref >= 1e-3
    assert_allclose(above[sure], ref[sure], rtol=RTOL, atol=0.0, err_msg=what)
    assert np.all(np.abs(rows.sum(axis=2) + above - 1.0)[above > 0] <= ATOL), what


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("n", oracle.N_PARTICLES)
def test_poisson_pmf_at_every_cloud_size(n):
    o = _object(POISSON, "wide", n, oracle.EXPOSURE)
    got = o.count_pmf(count_max=65)
    _close_table(f"poisson, {n} particles", POISSON, got, oracle.case_table(POISSON, "wide", n, oracle.EXPOSURE, 65))


@pytest.mark.parametrize("n_points", oracle.N_POINTS)
def test_poisson_pmf_at_every_point_count(n_points):
    o = _object(POISSON, "wide", 257, oracle.EXPOSURE)
    got = o.count_pmf((oracle.GRID[:n_points],), count_max=191)
    want = oracle.case_table(POISSON, "wide", 257, oracle.EXPOSURE, 191)[:n_points]
    _close_table(f"poisson, {n_points} points", POISSON, got, want)


@pytest.mark.parametrize("kind", ("wide", "converged"))
@pytest.mark.parametrize("count_max", oracle.COUNT_MAXES)
def test_poisson_pmf_at_every_count_max(count_max, kind):
    o = _object(POISSON, kind, 257, oracle.EXPOSURE)
    got = o.count_pmf((oracle.GRID[:65],), count_max=count_max)
    want = oracle.case_table(POISSON, kind, 257, oracle.EXPOSURE, count_max, 65)
    _close_table(f"poisson {kind}, count_max {count_max}", POISSON, got, want)


def test_poisson_default_count_max_and_exposure_keyword():
    o = _object(POISSON, "wide", 65, 1.0)
    got = o.count_pmf((oracle.GRID[:3],), exposure=oracle.DEFAULT_EXPOSURE)
    assert got.shape == (3, 1, 258)
    _close_table("poisson default", POISSON, got, oracle.case_table(POISSON, "wide", 65, oracle.DEFAULT_EXPOSURE, 256, 3))


@pytest.mark.parametrize("shots", oracle.SHOTS)
def test_binomial_pmf_at_every_shot_count(shots):
    o = _object(BINOMIAL, "wide", 257, shots)
    got = o.count_pmf()                                             # (count_max: the shots; nothing above)
    assert got.shape == (130, 1, shots + 2) and np.all(got[:, :, -1] == 0.0)
    _close_table(f"binomial, {shots} shots", BINOMIAL, got, oracle.case_table(BINOMIAL, "wide", 257, shots, shots), shots)


@pytest.mark.parametrize("n", oracle.N_PARTICLES)
def test_binomial_pmf_at_every_cloud_size(n):
    o = _object(BINOMIAL, "wide", n, 100)
    _close_table(f"binomial, {n} particles", BINOMIAL, o.count_pmf(),
                 oracle.case_table(BINOMIAL, "wide", n, 100, 100), 100)


@pytest.mark.parametrize("kind", ("wide", "converged"))
@pytest.mark.parametrize("count_max", oracle.COUNT_MAXES)
def test_binomial_pmf_at_every_count_max(count_max, kind):
    o = _object(BINOMIAL, kind, 257, 100)
    got = o.count_pmf((oracle.GRID[:65],), count_max=count_max)
    want = oracle.case_table(BINOMIAL, kind, 257, 100, count_max, 65)
    _close_table(f"binomial {kind}, count_max {count_max}", BINOMIAL, got, want, 100)
    if count_max >= 100:
        assert np.all(got[:, :, -1] == 0.0)


@pytest.mark.parametrize("law,side", ((BINOMIAL, (31, 33)), (POISSON, (4.0, 8.0))))
def test_two_channel_plugin_model(law, side):
    """RAMSEY / DECAYS through their plugin libraries, another side datum per channel: table, tails, joint evidence."""
    o = _object(law, "two", 257, side)
    _, w, V = oracle.case(law, "two", 257)
    count_max = 65
    want = oracle.case_table(law, "two", 257, side, count_max)
    _close_table(f"{law}, two channels", law, o.count_pmf(count_max=count_max), want,
                 tiny_rows=law == BINOMIAL)                         # (shots 31 and 33: exact zeros beyond them)
    g = np.random.default_rng(5)
    k = g.integers(0, 30, size=(2, oracle.TIMES.size)).astype(float)
    lo, up = o.count_cdf((oracle.TIMES,), k), o.count_cdf((oracle.TIMES,), k, upper=True)
    big = int(max(k.max(), max(side) if law == BINOMIAL else 0))
    want_lo, want_up = oracle.tails(oracle.table(law, V, w, np.array(side, dtype=float), big), k)
    assert_allclose(lo, want_lo, rtol=RTOL, atol=0.0)
    if law == BINOMIAL:
        assert_allclose(up, want_up, rtol=RTOL, atol=0.0)
    else:
        assert np.all(np.abs(up - want_up) <= ATOL)
        assert_allclose(up[want_up >= 1e-3], want_up[want_up >= 1e-3], rtol=RTOL, atol=0.0)
    got = o.count_logpmf((oracle.TIMES,), k)
    want = oracle.joint_logpmf(law, V, w, k, np.array(side, dtype=float))
    assert got.shape == want.shape and np.all(np.isfinite(want))
    assert_allclose(np.exp(got - want), 1.0, rtol=RTOL, atol=0.0)


# ------------------------------------------------------------------------------------------------ tails, p-values
@pytest.mark.parametrize("law", (BINOMIAL, POISSON))
def test_tails_pvalue_and_their_invariant(law):
    """Records with a side datum of their own each; then, with one side datum, lower + upper - Pbar(k) = 1."""
    from optbayesexpt_amd._scoring import pvalue_from_tails
    n_r = 130
    o = _object(law, "wide", 257, 100 if law == BINOMIAL else oracle.EXPOSURE)
    _, w, V = oracle.case(law, "wide", 257)
    g = np.random.default_rng(17)
    if law == BINOMIAL:
        side = g.choice(np.array(oracle.SHOTS, dtype=float), size=(1, n_r))
        k = np.floor(g.random((1, n_r)) * (side + 1))
        kw = {"shots": side}
    else:
        side = g.choice(np.array([1.0, 4.0, 8.0]), size=(1, n_r))
        k = g.poisson(6.0 * side).astype(float)
        kw = {"exposure": side}
    lo, up = o.count_cdf((oracle.GRID,), k, **kw), o.count_cdf((oracle.GRID,), k, upper=True, **kw)
    big = int(max(k.max(), side.max() if law == BINOMIAL else 0))
    want_lo, want_up = oracle.tails(oracle.table(law, V, w, side, big), k)
    assert lo.shape == up.shape == (1, n_r)
    assert_allclose(lo, want_lo, rtol=RTOL, atol=0.0)
    if law == BINOMIAL:
        assert_allclose(up, want_up, rtol=RTOL, atol=0.0)
    else:
        assert np.all(np.abs(up - want_up) <= ATOL)
        assert_allclose(up[want_up >= 1e-3], want_up[want_up >= 1e-3], rtol=RTOL, atol=0.0)
    assert_array_equal(o.count_pvalue((oracle.GRID,), k, **kw), pvalue_from_tails(lo, up))
    # the invariant, on the device's own numbers
    one = float(side[0, 0])
    kw = {"shots" if law == BINOMIAL else "exposure": one}
    k = np.minimum(k, one) if law == BINOMIAL else k
    big = int(max(k.max(), one if law == BINOMIAL else 0))
    lo, up = o.count_cdf((oracle.GRID,), k, **kw), o.count_cdf((oracle.GRID,), k, upper=True, **kw)
    pmf = o.count_pmf(count_max=big, **kw)
    at_k = pmf[np.arange(n_r), 0, k[0].astype(int)]
    assert np.all(np.abs(lo[0] + up[0] - at_k - 1.0) <= ATOL)


# ------------------------------------------------------------------------------------------------ the joint evidence
@pytest.mark.parametrize("law", (BINOMIAL, POISSON))
def test_logpmf_against_oracle_and_likelihood(law):
    side = 33 if law == BINOMIAL else oracle.EXPOSURE
    o = _object(law, "wide", 4097, side)
    _, w, V = oracle.case(law, "wide", 4097)
    g = np.random.default_rng(23)
    k = (g.integers(0, 34, size=(1, 130)) if law == BINOMIAL else g.poisson(50.0, size=(1, 130))).astype(float)
    got = o.count_logpmf((oracle.GRID,), k)
    want = oracle.joint_logpmf(law, V, w, k, side)
    assert got.shape == (130,) and np.all(want > -600)
    assert_allclose(np.exp(got - want), 1.0, rtol=RTOL, atol=0.0)
    # one record, as pdf_update takes it: a float, and log(sum w L / sum w) of likelihood()
    import math
    x, kk = float(oracle.GRID[64]), float(k[0, 64])
    single = o.count_logpmf((x,), kk)
    assert isinstance(single, float) and single == got[64]
    lik = o.likelihood(o.eval_over_all_parameters((x,)), ((x,), kk))
    const = math.lgamma(side + 1) - math.lgamma(kk + 1) - math.lgamma(side - kk + 1) if law == BINOMIAL else 0.0
    assert_allclose(math.exp(single), math.exp(const) * np.sum(w * lik) / np.sum(w), rtol=RTOL)


# ------------------------------------------------------------------------------------------------ quantiles
@pytest.mark.parametrize("law,kind", ((BINOMIAL, "wide"), (BINOMIAL, "two"), (POISSON, "wide"), (POISSON, "two")))
def test_quantiles_are_the_oracles_whole_numbers(law, kind):
    side, count_max = oracle.QUANTILE_CASES[law, kind]
    o = _object(law, kind, 257, side)
    want = oracle.quantiles(oracle.case_table(law, kind, 257, side, count_max), LEVELS)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got, info = o.count_quantile(LEVELS, count_max=count_max, full_output=True)
        lo, hi = o.count_interval(0.95, count_max=count_max)
        median = o.count_quantile(0.5, count_max=count_max)
    assert info == {"beyond": 0} and got.shape == want.shape and not np.any(np.isnan(want))
    assert_array_equal(got, want)
    assert_array_equal(lo, got[0])
    assert_array_equal(hi, got[2])
    assert_array_equal(median, got[1])
    # cdf(quantile) >= q > cdf(quantile - 1), on the device's own table
    cum = np.cumsum(o.count_pmf(count_max=count_max)[:, :, :-1], axis=2)
    for j, q in enumerate(LEVELS):
        k = got[j].T.astype(int)                                   # (n_x, C)
        at = np.take_along_axis(cum, k[:, :, None], axis=2)[:, :, 0]
        before = np.where(k > 0, np.take_along_axis(cum, np.maximum(k - 1, 0)[:, :, None], axis=2)[:, :, 0], 0.0)
        assert np.all(at >= q) and np.all(before < q)


def test_quantile_beyond_count_max_is_nan_with_one_warning():
    o = _object(POISSON, "wide", 257, oracle.EXPOSURE)
    want = oracle.quantiles(oracle.case_table(POISSON, "wide", 257, oracle.EXPOSURE, 31), LEVELS)
    assert np.any(np.isnan(want)) and not np.all(np.isnan(want))
    with pytest.warns(RuntimeWarning, match="beyond count_max = 31") as caught:
        got, info = o.count_quantile(LEVELS, count_max=31, full_output=True)
    assert len(caught) == 1 and info == {"beyond": int(np.isnan(want).sum())}
    assert_array_equal(got, want)                                   # (NaN at the same places)


def test_nobody_contributes_gives_nan():
    """No particle's value is a probability: NaN everywhere, and no warning (nothing lies beyond count_max)."""
    o = _row_object(BINOMIAL, [1.5, -0.2, 2.0], [0.2, 0.3, 0.5], 5)
    assert np.all(np.isnan(o.count_pmf()))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        q, info = o.count_quantile(0.5, full_output=True)
    assert np.all(np.isnan(q)) and info == {"beyond": 0}
    assert np.all(np.isnan(o.count_cdf((0.5,), 2.0))) and np.isnan(o.count_logpmf((0.5,), 2.0))
    # ... and a particle of weight 0 contributes nothing whatever its value is
    o = _row_object(BINOMIAL, [0.25, 7.0], [1.0, 0.0], 5)
    want = oracle.table(BINOMIAL, np.full((2, 1, 1), 0.25), [1.0], 5, 5)
    _close_table("weight 0", BINOMIAL, o.count_pmf(), want, 5)


@pytest.mark.parametrize("shots", (1, 33, 100))
def test_binomial_point_masses_at_p_0_and_p_1(shots):
    values, weights = [0.0, 1.0, 0.3, 0.0, 1.0, 0.75], [0.1, 0.2, 0.25, 0.05, 0.15, 0.25]
    o = _row_object(BINOMIAL, values, weights, shots)
    got = o.count_pmf()
    assert np.all(np.isfinite(got))
    V = np.broadcast_to(np.array(values), (2, 1, 6))
    _close_table(f"point masses, {shots} shots", BINOMIAL, got, oracle.table(BINOMIAL, V, weights, shots, shots), shots)
    only = _row_object(BINOMIAL, [0.0, 1.0], [0.25, 0.75], shots).count_pmf()
    want = np.zeros(shots + 2)
    want[0], want[shots] = 0.25, 0.75
    assert_array_equal(only[0, 0], want)
    k = np.array([[0.0, float(shots)]])
    lp = _row_object(BINOMIAL, [0.0, 1.0], [0.25, 0.75], shots).count_logpmf((np.array([0.0, 1.0]),), k)
    assert_allclose(np.exp(lp), [0.25, 0.75], rtol=RTOL)


@pytest.mark.parametrize("shots", (31, 63, 100, 127))
def test_binomial_probabilities_next_to_0_and_1(shots):
    """(1 - p)^n or p^n underflows, or nearly, at one end of a block while the mass sits at the other: every particle's
    block is run from its large end.  Each particle alone, then all of them mixed; rows >= 1e-200 at 1e-10."""
    values, weights = oracle.EDGE_PROBABILITIES, oracle.EDGE_WEIGHTS
    for vals, wts in [([v], [1.0]) for v in values] + [(values, weights)]:
        got = _row_object(BINOMIAL, vals, wts, shots).count_pmf()
        want = oracle.edge_table(vals, wts, shots)
        what = f"p in {vals}, {shots} shots"
        _close_table(what, BINOMIAL, got, want, shots, tiny_rows=True)
        assert np.all(np.abs(got[:, :, :-1].sum(axis=2) - 1.0) <= ATOL), what
        k = np.array([[0.0, float(shots)]])
        o = _row_object(BINOMIAL, vals, wts, shots)
        up = o.count_cdf((np.array([0.0, 1.0]),), k, upper=True)
        want_lo, want_up = oracle.tails(want, k)
        sure = want_up >= 1e-200
        assert_allclose(up[sure], want_up[sure], rtol=RTOL, atol=0.0, err_msg=what)
        lo = o.count_cdf((np.array([0.0, 1.0]),), k)
        sure = want_lo >= 1e-200
        assert_allclose(lo[sure], want_lo[sure], rtol=RTOL, atol=0.0, err_msg=what)


def test_poisson_point_mass_at_rate_0():
    got = _row_object(POISSON, [0.0, 0.0], [0.5, 0.5], 3.0).count_pmf(count_max=70)
    want = np.zeros(72)
    want[0] = 1.0
    assert_array_equal(got[0, 0], want)


def test_high_rate_where_exp_minus_lambda_underflows():
    import optbayesexpt_amd as obe
    cloud, w, V = oracle.high_rate_case()
    assert np.exp(-oracle.HIGH_EXPOSURE * V.min()) == 0.0
    o = obe.OptBayesExptPoisson(obe.models.lorentzian(1), (oracle.HIGH_POINTS,), cloud, (0.1,),
                                exposure=oracle.HIGH_EXPOSURE, scale=False)
    o.particle_weights = w
    want = oracle.table(POISSON, V, w, oracle.HIGH_EXPOSURE, oracle.HIGH_COUNT_MAX)
    got = o.count_pmf(count_max=oracle.HIGH_COUNT_MAX)
    assert np.max(want[:, :, :-1]) > 1e-3
    _close_table("high rate", POISSON, got, want, tiny_rows=True)
    k = np.array([[700.0, 880.0, 1100.0]])
    lo, up = o.count_cdf((oracle.HIGH_POINTS,), k), o.count_cdf((oracle.HIGH_POINTS,), k, upper=True)
    want_lo, want_up = oracle.tails(oracle.table(POISSON, V, w, oracle.HIGH_EXPOSURE, 1100), k)
    big = want_lo >= 1e-200
    assert_allclose(lo[big], want_lo[big], rtol=RTOL, atol=0.0)
    assert np.all(np.abs(up - want_up) <= ATOL)
    assert np.any(want_up >= 1e-3)
    assert_allclose(up[want_up >= 1e-3], want_up[want_up >= 1e-3], rtol=RTOL, atol=0.0)


# ------------------------------------------------------------------------------------------------ tiles, bits
@pytest.mark.parametrize("law", (BINOMIAL, POISSON))
def test_tiled_requests_give_the_bits_of_one_call(law, monkeypatch):
    from optbayesexpt_amd import _counts
    side = (31, 33) if law == BINOMIAL else (4.0, 8.0)
    o = _object(law, "two", 257, side)
    g = np.random.default_rng(3)
    k = g.integers(0, 30, size=(2, oracle.TIMES.size)).astype(float)

    def everything():
        return (o.count_pmf(count_max=40), o.count_quantile(LEVELS, count_max=127), o.count_cdf((oracle.TIMES,), k),
                o.count_cdf((oracle.TIMES,), k, upper=True), o.count_logpmf((oracle.TIMES,), k))
    whole = everything()
    again = everything()
    monkeypatch.setattr(_counts, "TABLE_BYTES_PER_CALL", 8 * 2 * 35 * 7)          # 7 points per call at count_max 33
    monkeypatch.setattr(_counts, "RECORDS_PER_CALL", 7)
    assert _counts.points_per_call(2, 33) == 7
    tiled = everything()
    for a, b, c in zip(whole, again, tiled):
        assert_array_equal(_bits(a), _bits(b))                      # run to run
        assert_array_equal(_bits(a), _bits(c))                      # however the points are cut


@pytest.mark.parametrize("cap", (16, 32, 64))
def test_count_pmf_agrees_with_count_distribution(cap):
    o = _object(POISSON, "wide", 4097, 2.0)
    o.count_cap = cap
    old = o.count_distribution()
    new = o.count_pmf(count_max=cap - 1)[:, 0, :]
    assert old.shape == new.shape
    assert_allclose(new[:, :cap], old[:, :cap], rtol=RTOL, atol=0.0)
    assert np.all(np.abs(new[:, cap] - old[:, cap]) <= ATOL)
    # ... and more than asked: the same arithmetic in the same order, so the rows k < cap are the same bits
    assert_array_equal(_bits(new[:, :cap]), _bits(old[:, :cap]))


# ------------------------------------------------------------------------------------------------ refusals
def test_c_level_refusals_come_before_any_launch():
    import torch
    from optbayesexpt_amd._devcall import ptr
    from optbayesexpt_amd import _counts, _lib
    o = _object(POISSON, "wide", 65, 1.0)
    lib, m, dev = o._mlib, o._model_struct, o._device
    p, w = o._pw_tensors()
    n, n_p = 4, p.shape[1]
    x = torch.full((2, n), 3.0, dtype=torch.float64, device=dev)    # [settings; exposure]
    lf = _counts._logfact(dev)
    pmf = torch.full((1, 10, n), -7.0, dtype=torch.float64, device=dev)
    out = torch.full((3, 1, n), -7.0, dtype=torch.float64, device=dev)
    nbytes = int(lib.cdll.obe_count_workspace_bytes(n_p, n, 1, 8))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    levels = np.array([0.5, 1.0])

    def table(law=_lib.OBE_COUNT_POISSON, count_max=8, ws_bytes=nbytes, n_points=n, d_pmf=ptr(pmf), ld_side=n):
        return lib.cdll.obe_count_table(m, law, ptr(x), n, n_points, ptr(x[1:]), ld_side, ptr(lf), ptr(p), n_p, n_p,
                                        ptr(w), count_max, d_pmf, ptr(ws), ws_bytes, o._stream())

    def logpmf(law=_lib.OBE_COUNT_POISSON, ws_bytes=nbytes, d_out=ptr(out)):
        return lib.cdll.obe_count_logpmf(m, law, ptr(x), n, n, ptr(x), n, ptr(x[1:]), n, ptr(x), ptr(p), n_p, n_p,
                                         ptr(w), d_out, ptr(ws), ws_bytes, o._stream())
    tails, quantiles = lib.cdll.obe_count_tails, lib.cdll.obe_count_quantiles
    h_levels = _lib.host_ptr(levels)
    refused = [
        (lambda: table(law=2), "obe_count_table: law"), (lambda: table(count_max=-1), "count_max outside"),
        (lambda: table(count_max=_lib.OBE_COUNT_MAX_OUTCOMES + 1), "count_max outside"),
        (lambda: table(ws_bytes=nbytes - 8), "obe_count_table: workspace too small"),
        (lambda: table(n_points=0), "n_settings < 1"), (lambda: table(d_pmf=None), "obe_count_table: null pointer"),
        (lambda: table(ld_side=n - 1), "d_side"),
        (lambda: logpmf(law=-1), "obe_count_logpmf: law"), (lambda: logpmf(ws_bytes=8), "workspace too small"),
        (lambda: logpmf(d_out=None), "obe_count_logpmf: null pointer"),
        (lambda: tails(ptr(pmf), 1, 8, n, ptr(x), n, None, None, o._stream()), "d_lower"),
        (lambda: tails(ptr(pmf), 0, 8, n, ptr(x), n, ptr(out), None, o._stream()), "n_channels"),
        (lambda: tails(ptr(pmf), 1, 8, n, ptr(x), n - 1, ptr(out), None, o._stream()), "d_counts"),
        (lambda: quantiles(ptr(pmf), 1, 8, n, h_levels, 2, ptr(out), o._stream()), "a level outside"),
        (lambda: quantiles(ptr(pmf), 1, 8, n, h_levels, 17, ptr(out), o._stream()), "n_levels"),
        (lambda: quantiles(ptr(pmf), 1, 4097, n, h_levels, 1, ptr(out), o._stream()), "count_max outside"),
    ]
    for call, words in refused:
        assert call() == -1 and words in lib.last_error(), (words, lib.last_error())
    torch.cuda.synchronize()
    assert torch.all(pmf == -7.0) and torch.all(out == -7.0)        # nothing was launched
    assert table() == 0 and logpmf() == 0                           # ... and the same calls, well-formed, run
    torch.cuda.synchronize()
    assert not torch.any(pmf == -7.0)


@pytest.mark.parametrize("law", (BINOMIAL, POISSON))
def test_host_refuses_beyond_the_outcome_bound_before_any_device_call(law, monkeypatch):
    from optbayesexpt_amd import _counts
    o = _object(law, "wide", 63, 5 if law == BINOMIAL else 1.0)

    def no_call(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_counts, "model_call", no_call)
    with pytest.raises(ValueError, match="OBE_COUNT_MAX_OUTCOMES"):
        o.count_pmf(count_max=4097)
    with pytest.raises(ValueError, match="OBE_COUNT_MAX_OUTCOMES"):
        o.count_cdf((3.0,), 4097.0, **({"shots": 5000} if law == BINOMIAL else {}))
    if law == BINOMIAL:
        with pytest.raises(ValueError, match="OBE_COUNT_MAX_OUTCOMES"):
            o.count_quantile(0.5, shots=4097)


@pytest.mark.parametrize("law", (BINOMIAL, POISSON))
def test_gaussian_named_methods_still_refuse(law):
    o = _object(law, "wide", 63, 5 if law == BINOMIAL else 1.0)
    calls = (lambda: o.predictive_logpdf((3.0,), 1.0), lambda: o.predictive_cdf((3.0,), 1.0),
             lambda: o.predictive_pvalue((3.0,), 1.0), lambda: o.reading_quantile(0.5),
             lambda: o.reading_interval(0.9))
    for call in calls:
        with pytest.raises(NotImplementedError, match="counts") as err:
            call()
        assert "count_cdf()" in str(err.value) and "batch assimilation" not in str(err.value)


# ------------------------------------------------------------------------------------------------ the example
def test_example_prints_a_band_that_holds_its_share_of_the_counts():
    """examples/recorded_counts_check.py: a 95 % band of whole numbers holds at least 95 % of the next counts in
    expectation; of its 60 simulated counts at least 51 (57 expected, 3.5 standard deviations of 1.7 below) lie inside,
    and the p-values it prints are probabilities."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "recorded_counts_check.py")],
                         capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    line = [t for t in run.stdout.splitlines() if t.startswith("inside the 95 % band:")]
    assert len(line) == 1, run.stdout
    inside, total = (int(t) for t in line[0].split(":")[1].split("of"))
    assert total == 60 and 51 <= inside <= 60, line[0]
    smallest = [t for t in run.stdout.splitlines() if t.startswith("smallest p-value:")]
    assert len(smallest) == 1 and 0.0 < float(smallest[0].split(":")[1].split()[0]) <= 1.0
