"""Count-aware scoring without a device: the oracle of the GPU tests (tests/_counts_oracle.py) against scipy.stats, every
argument check of optbayesexpt_amd/_counts.py, and the conditions tests/test_gpu_counts.py relies on, asserted on the
oracle alone so that no case is ever left out there."""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal
from scipy import stats

import _counts_oracle as oracle
from _counts_oracle import BINOMIAL, POISSON
from optbayesexpt_amd import _counts, _lib, obe_binomial, obe_poisson

BIN, POIS = obe_binomial.OptBayesExptBinomial._COUNT_LAW, obe_poisson.OptBayesExptPoisson._COUNT_LAW


# ------------------------------------------------------------------------------------------------ oracle vs scipy
@pytest.mark.parametrize("dtype", (np.float64, np.longdouble))
def test_oracle_pmf_is_scipys(dtype):
    p = np.array([0.0, 1e-9, 0.1, 0.5, 0.9, 1.0])
    for n in (1, 2, 33, 100):
        for k in range(n + 2):
            assert_allclose(np.asarray(oracle.pmf(BINOMIAL, k, n, p, dtype), dtype=np.float64),
                            stats.binom.pmf(k, n, p), rtol=2e-12, atol=0.0)
    lam = np.array([0.0, 1e-3, 1.0, 16.0, 96.0, 800.0, 1000.0])
    for k in (0, 1, 31, 64, 191, 800, 1200):
        assert_allclose(np.asarray(oracle.pmf(POISSON, k, 4.0, lam / 4.0, dtype), dtype=np.float64),
                        stats.poisson.pmf(k, lam), rtol=2e-11, atol=0.0)


def test_oracle_tables_and_tails_are_scipys_on_the_inputs():
    """pmf, cdf and sf of the mixture on the oracle's own inputs (a cloud of 63 particles)."""
    for law, side, count_max in ((BINOMIAL, 33, 33), (POISSON, oracle.EXPOSURE, 191)):
        _, w, V = oracle.case(law, "wide", 63)
        tab = oracle.table(law, V[:5], w, side, count_max)
        k = np.arange(count_max + 1)
        dist = (lambda v: stats.binom(side, v)) if law == BINOMIAL else (lambda v: stats.poisson(side * v))
        for s in range(5):
            d = dist(V[s, 0][:, None])
            assert_allclose(tab[s, 0, :-1], w @ d.pmf(k) / w.sum(), rtol=1e-11)
            assert_allclose(tab[s, 0, -1], w @ d.sf(count_max)[:, 0] / w.sum(), rtol=1e-9, atol=1e-14)
            ks = np.array([[3.0, 10.0, 20.0]])
            lo, up = oracle.tails(tab[s:s + 1].repeat(3, axis=0), ks)
            assert_allclose(lo[0], w @ d.cdf(ks[0]) / w.sum(), rtol=1e-11)
            assert_allclose(up[0], w @ d.sf(ks[0] - 1) / w.sum(), rtol=1e-9)


def test_oracle_quantiles_and_joint_evidence():
    tab = np.array([[[0.1, 0.2, 0.3, 0.4, 0.0]]])
    assert_array_equal(oracle.quantiles(tab, (0.05, 0.1, 0.3000001, 0.99))[:, 0, 0], [0, 0, 2, 3])
    assert np.isnan(oracle.quantiles(np.array([[[0.1, 0.2, 0.7]]]), (0.5,))[0, 0, 0])
    # one particle: the joint evidence is the product of the channels' pmfs
    V = np.array([[[0.3], [0.6]]])
    got = oracle.joint_logpmf(BINOMIAL, V, [1.0], np.array([[2.0], [5.0]]), (4, 7))
    assert_allclose(got, np.log(stats.binom.pmf(2, 4, 0.3) * stats.binom.pmf(5, 7, 0.6)), rtol=1e-13)


# ------------------------------------------------------------------------------------------------ argument checks
def test_constants_come_from_the_header():
    assert _counts.MAX_OUTCOMES == _lib.OBE_COUNT_MAX_OUTCOMES == 4096
    assert (_lib.OBE_COUNT_BINOMIAL, _lib.OBE_COUNT_POISSON) == (BIN.code, POIS.code) == (0, 1)
    lf = _counts.log_factorials()
    assert lf.shape == (4098,) and lf[0] == lf[1] == 0.0
    import math
    sums = [math.fsum(math.log(j) for j in range(1, k + 1)) for k in (2, 10, 4097)]          # log k!, term by term
    assert_allclose(lf[[2, 10, 4097]], sums, rtol=1e-14)
    for name in ("obe_count_workspace_bytes", "obe_count_table", "obe_count_tails", "obe_count_quantiles",
                 "obe_count_logpmf"):
        assert name in _lib.MODEL_ENTRY_POINTS and name in _lib.PROTOTYPES


def test_check_count_max():
    assert _counts.check_count_max(None, 256) == 256 and _counts.check_count_max(np.int64(0), 5) == 0
    assert _counts.check_count_max(4096, 1) == 4096
    for bad in (-1, 4097, 3.0, True, "7", None):
        with pytest.raises(ValueError, match="count_max"):
            _counts.check_count_max(bad, None if bad is None else 5)
    with pytest.raises(ValueError, match="OBE_COUNT_MAX_OUTCOMES"):
        _counts.check_count_max(None, 5000)                         # (a default from shots beyond the bound)


def test_points_per_call_bounds_the_table():
    assert _counts.TABLE_BYTES_PER_CALL == 1 << 28
    for n_c, count_max in ((1, 0), (1, 63), (3, 256), (8, 4096)):
        n = _counts.points_per_call(n_c, count_max)
        assert n >= 1 and 8 * n_c * (count_max + 2) * n <= _counts.TABLE_BYTES_PER_CALL < 8 * n_c * (count_max + 2) * (n + 1)


def test_check_scored_records_shapes_and_broadcasting():
    x, k, b, const, single = _counts.check_scored_records(BIN, (1.0,), 3, None, 10, 1, 1)
    assert (x.shape, k.shape, b.shape, const.shape, single) == ((1, 1), (1, 1), (1, 1), (1, 1), True)
    assert b[0, 0] == 10 and and_close(const[0, 0], np.log(120.0))
    x, k, b, const, single = _counts.check_scored_records(BIN, (np.arange(4.0),), [0, 1, 2, 3], [3, 4, 5, 6], 10, 1, 1)
    assert (x.shape, k.shape, b.shape, single) == ((1, 4), (1, 4), (1, 4), False)
    assert_array_equal(b, [[3, 4, 5, 6]])
    # two channels: one record as (C,), side as a scalar, (C,) and (C, n_r)
    x, k, b, _, single = _counts.check_scored_records(POIS, (2.0,), [3, 4], None, [1.0, 2.0], 1, 2)
    assert single and and_equal(b, [[1.0], [2.0]])
    x, k, b, _, single = _counts.check_scored_records(POIS, (np.arange(3.0),), np.ones((2, 3)), 0.5, 1.0, 1, 2)
    assert not single and b.shape == (2, 3) and np.all(b == 0.5)
    _, _, b, _, _ = _counts.check_scored_records(POIS, (np.arange(3.0),), np.ones((2, 3)), np.arange(1.0, 7).reshape(2, 3),
                                                 1.0, 1, 2)
    assert_array_equal(b, np.arange(1.0, 7).reshape(2, 3))
    bad = [
        ((np.arange(3.0),), np.ones((2, 4)), None),                 # records do not broadcast
        ((np.arange(3.0),), np.ones((2, 3)), np.ones((2, 4))),      # nor does the side datum
        ((np.arange(3.0),), np.ones((3, 3)), None),                 # rows are not the channels
        ((np.arange(3.0),), np.ones((2, 3)), [1.0, 2.0, 3.0]),      # (C,) of another length
        ((np.arange(3.0), np.arange(3.0)), np.ones((2, 3)), None),  # settings of another model
        ((1.0,), None, None),
    ]
    for settings, counts, side in bad:
        with pytest.raises(ValueError):
            _counts.check_scored_records(POIS, settings, counts, side, 1.0, 1, 2)


def and_close(a, b):
    assert_allclose(a, b, rtol=1e-14)
    return True


def and_equal(a, b):
    assert_array_equal(a, b)
    return True


def test_check_scored_records_values_and_bound():
    for counts, shots in ((1.5, 4), (-1, 4), (5, 4), (1, 0), (1, 2.5), (np.nan, 4)):
        with pytest.raises(ValueError):
            _counts.check_scored_records(BIN, (1.0,), counts, shots, 10, 1, 1)
    for counts, exposure in ((1.5, 1.0), (-1, 1.0), (1, 0.0), (1, np.inf), (np.inf, 1.0)):
        with pytest.raises(ValueError):
            _counts.check_scored_records(POIS, (1.0,), counts, exposure, 1.0, 1, 1)
    _counts.check_scored_records(BIN, (1.0,), 4096, 4096, 10, 1, 1)
    _counts.check_scored_records(POIS, (1.0,), 4096, 1e9, 1.0, 1, 1)
    with pytest.raises(ValueError, match="OBE_COUNT_MAX_OUTCOMES"):
        _counts.check_scored_records(BIN, (1.0,), 5, 4097, 10, 1, 1)
    with pytest.raises(ValueError, match="OBE_COUNT_MAX_OUTCOMES"):
        _counts.check_scored_records(POIS, (1.0,), 4097, None, 1.0, 1, 1)


def test_check_grid_request_and_the_side_keyword():
    x, b = _counts.check_grid_request(BIN, None, None, 7, 1, 2)
    assert x is None and and_equal(b, [7, 7])
    x, b = _counts.check_grid_request(POIS, (np.arange(3.0),), [1.0, 2.0], 5.0, 1, 2)
    assert x.shape == (1, 3) and and_equal(b, [1.0, 2.0])
    for law, side in ((BIN, 0), (BIN, 2.5), (BIN, [1, 2, 3]), (BIN, np.ones((2, 3))), (POIS, 0.0), (POIS, -1.0),
                      (POIS, [1.0, 2.0, 3.0]), (POIS, np.inf)):
        with pytest.raises(ValueError):
            _counts.check_grid_request(law, None, side, 1, 1, 2)
    with pytest.raises(ValueError, match="OBE_COUNT_MAX_OUTCOMES"):
        _counts.check_grid_request(BIN, None, 4097, 1, 1, 1)
    _counts.check_grid_request(POIS, None, 1e6, 1, 1, 1)              # (an exposure is no count)
    with pytest.raises(ValueError):
        _counts.check_grid_request(POIS, (np.arange(3.0), np.arange(3.0)), None, 1.0, 1, 1)
    assert BIN.default_max(np.array([3.0, 9.0])) == 9 and POIS.default_max(np.array([3.0])) == 256
    assert (BIN.name, POIS.name) == ("shots", "exposure")


def test_levels():
    from optbayesexpt_amd._reading import check_levels
    assert _counts.check_levels is check_levels
    for bad in (0.0, 1.0, -0.1, np.nan, [], [[0.5]], "x"):
        with pytest.raises(ValueError):
            _counts.check_levels(bad)
    assert _counts.check_level(0.9) == 0.9
    for bad in (0.0, 1.0, "x", None):
        with pytest.raises(ValueError):
            _counts.check_level(bad)


def test_the_classes_point_at_the_count_methods():
    for cls in (obe_binomial.OptBayesExptBinomial, obe_poisson.OptBayesExptPoisson):
        assert "counts" in cls._REFUSAL and "count_cdf()" in cls._REFUSAL and "not built" not in cls._REFUSAL
        for name in ("count_logpmf", "count_cdf", "count_pvalue", "count_pmf", "count_quantile", "count_interval"):
            assert name + "()" in cls.__doc__, name
            assert callable(getattr(cls, name))
    import inspect
    assert "shots" in inspect.signature(obe_binomial.OptBayesExptBinomial.count_cdf).parameters
    assert "exposure" in inspect.signature(obe_poisson.OptBayesExptPoisson.count_quantile).parameters


# ------------------------------------------------------------------------------------------------ what the GPU tests rely on
def _gpu_tables():
    """Every (law, table) tests/test_gpu_counts.py compares row by row."""
    for n in oracle.N_PARTICLES:
        yield POISSON, oracle.case_table(POISSON, "wide", n, oracle.EXPOSURE, 65)
        yield BINOMIAL, oracle.case_table(BINOMIAL, "wide", n, 100, 100)
    yield POISSON, oracle.case_table(POISSON, "wide", 257, oracle.EXPOSURE, 191)
    for kind in ("wide", "converged"):
        yield POISSON, oracle.case_table(POISSON, kind, 257, oracle.EXPOSURE, 191, 65)
        yield BINOMIAL, oracle.case_table(BINOMIAL, kind, 257, 100, 100, 65)
    for shots in oracle.SHOTS:
        yield BINOMIAL, oracle.case_table(BINOMIAL, "wide", 257, shots, shots)
    yield POISSON, oracle.case_table(POISSON, "wide", 65, oracle.DEFAULT_EXPOSURE, 256, 3)
    yield POISSON, oracle.case_table(POISSON, "two", 257, (4.0, 8.0), 65)
    yield BINOMIAL, oracle.case_table(BINOMIAL, "two", 257, (31, 33), 65)[:, :, :32]          # (up to the fewer shots)
    yield BINOMIAL, oracle.case_table(BINOMIAL, "two", 257, (31, 33), 65)[:, 1:, :34]


def test_condition_a_every_compared_row_is_far_above_underflow():
    """(a): every mixture value the GPU tests compare relatively is >= 1e-200 (shots 100 and lambda in [16, 96] with
    k <= 191: the smallest are 4e-51 and 5e-20), so no compared row is left out by the tests' 1e-200 rule."""
    for law, tab in _gpu_tables():
        rows = tab[:, :, :-1]
        if law == BINOMIAL and tab.shape[2] > 102:                  # (count_max 191 at 100 shots: zeros beyond them)
            rows = rows[:, :, :101]
        assert np.all(rows >= 1e-200), (law, rows.min())
    # the edge probabilities: what is compared relatively there is what the oracle has above 1e-200, and in extended
    # precision the same rows to 1e-12: the float64 oracle is a reference at p = 1 - 1e-12 too
    for shots in (31, 63, 100, 127):
        t64 = oracle.edge_table(oracle.EDGE_PROBABILITIES, oracle.EDGE_WEIGHTS, shots)
        tld = oracle.edge_table(oracle.EDGE_PROBABILITIES, oracle.EDGE_WEIGHTS, shots, np.longdouble)
        assert np.all(t64[:, :, :-1] >= 1e-200)
        assert_allclose(t64.astype(np.float64), tld.astype(np.float64), rtol=1e-12, atol=0.0)
    cloud, w, V = oracle.high_rate_case()
    lam = oracle.HIGH_EXPOSURE * V
    assert lam.min() > 745.2 and lam.max() < 1001.0 and np.exp(-lam.min()) == 0.0


@pytest.mark.parametrize("law,kind", sorted(oracle.QUANTILE_CASES))
def test_condition_b_no_level_sits_on_a_step_of_the_cdf(law, kind):
    """(b): the extended-precision cdf keeps at least 1e-9 from every level at every k, point and channel."""
    side, count_max = oracle.QUANTILE_CASES[law, kind]
    tab = oracle.case_table(law, kind, 257, side, count_max, None, np.longdouble)
    assert oracle.level_margin(tab, oracle.LEVELS) >= 1e-9
    q64 = oracle.quantiles(oracle.case_table(law, kind, 257, side, count_max), oracle.LEVELS)
    assert_array_equal(oracle.quantiles(tab, oracle.LEVELS), q64)
    assert not np.any(np.isnan(q64))
    # ... and count_max 31 is too small for some, not all, of the Poisson levels (the NaN-and-warning test)
    if (law, kind) == (POISSON, "wide"):
        short = oracle.quantiles(oracle.case_table(POISSON, "wide", 257, oracle.EXPOSURE, 31), oracle.LEVELS)
        assert 0 < np.isnan(short).sum() < short.size


@pytest.mark.parametrize("law,side", ((BINOMIAL, (31, 33)), (POISSON, (4.0, 8.0))))
def test_condition_c_the_joint_evidence_is_not_the_product_of_marginals(law, side):
    """(c): on the two-channel inputs the joint log-pmf and the sum of the channels' marginal logs differ by more than
    1e-3 at every record the GPU test scores: an implementation that multiplies marginals fails there."""
    _, w, V = oracle.case(law, "two", 257)
    k = np.random.default_rng(5).integers(0, 30, size=(2, oracle.TIMES.size)).astype(float)
    joint = oracle.joint_logpmf(law, V, w, k, np.array(side, dtype=float))
    product = oracle.marginal_logpmf_sum(law, V, w, k, np.array(side, dtype=float))
    assert np.all(np.isfinite(joint)) and np.all(np.isfinite(product))
    assert np.max(np.abs(joint - product)) > 1e-3
    assert np.median(np.abs(joint - product)) > 1e-3
