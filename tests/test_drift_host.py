"""Parameter drift on the CPU: the argument forms and refusals of optbayesexpt_amd/_drift.py, and tests/_drift_oracle.py
— against a hand-worked case and integer arithmetic, and the inputs of tests/test_gpu_drift.py against the neighbours
of the contract (a chain that rounds its products, one summed in the other order, one started from the old value, a
reflection contracted into one fma): each must move enough outputs for a bit-for-bit comparison to see it."""
import math

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _drift_oracle as do
from optbayesexpt_amd import _drift

N = 293                      # the cloud of the GPU file's general cases


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------- argument forms
def test_every_form_reduces_to_one_rows_factor_pair():
    rows, L = _drift.normalize(0.5, None, 3)                              # scalar: every row
    assert rows.dtype == np.int32 and rows.tolist() == [0, 1, 2]
    assert_array_equal(L, np.diag([0.5, 0.5, 0.5]))
    rows, L = _drift.normalize(0.5, [2, 0], 3)                            # scalar on chosen rows, sorted
    assert rows.tolist() == [0, 2] and np.array_equal(L, np.diag([0.5, 0.5]))
    rows, L = _drift.normalize([0.1, 0.2, 0.3], None, 3)                  # vector: one entry per row
    assert rows.tolist() == [0, 1, 2] and np.array_equal(L, np.diag([0.1, 0.2, 0.3]))
    rows, L = _drift.normalize({2: 0.3, 0: 0.1}, None, 4)                 # mapping
    assert rows.tolist() == [0, 2] and np.array_equal(L, np.diag([0.1, 0.3]))
    rows, L = _drift.normalize({-1: 0.3}, None, 4)                        # NumPy negative indexing
    assert rows.tolist() == [3] and np.array_equal(L, [[0.3]])
    Q = np.array([[4.0, 1.0], [1.0, 2.0]])
    rows, L = _drift.normalize(Q, [1, 3], 4)                              # covariance: its lower Cholesky factor
    assert rows.tolist() == [1, 3]
    assert_array_equal(_bits(L), _bits(np.linalg.cholesky(Q)))
    assert L.flags.c_contiguous and L.dtype == np.float64
    assert _drift.normalize(None, None, 3) is None


def test_rows_of_zero_rate_do_not_drift():
    rows, L = _drift.normalize([0.1, 0.0, 0.3], None, 3)
    assert rows.tolist() == [0, 2] and np.array_equal(L, np.diag([0.1, 0.3]))
    rows, L = _drift.normalize({0: 0.0, 1: 0.2}, None, 3)
    assert rows.tolist() == [1] and np.array_equal(L, [[0.2]])
    Q = np.zeros((3, 3))
    Q[0, 0], Q[2, 2], Q[0, 2], Q[2, 0] = 4.0, 2.0, 1.0, 1.0
    rows, L = _drift.normalize(Q, None, 3)                                # a zero row and column of a covariance
    assert rows.tolist() == [0, 2]
    assert_array_equal(_bits(L), _bits(np.linalg.cholesky(np.array([[4.0, 1.0], [1.0, 2.0]]))))
    rows, L = _drift.normalize(0.0, None, 3)                              # nothing drifts
    assert rows.size == 0 and L.shape == (0, 0)


def test_unsorted_rows_are_sorted_together_with_their_rates():
    rows, L = _drift.normalize([0.3, 0.1, 0.2], [2, 0, 1], 3)
    assert rows.tolist() == [0, 1, 2] and np.array_equal(L, np.diag([0.1, 0.2, 0.3]))
    Q = np.array([[4.0, 1.0, 0.5], [1.0, 2.0, 0.25], [0.5, 0.25, 1.0]])
    rows, L = _drift.normalize(Q, [5, 1, 3], 6)
    order = [1, 2, 0]                                                     # rows 1, 3, 5
    assert rows.tolist() == [1, 3, 5]
    assert_array_equal(_bits(L), _bits(np.linalg.cholesky(Q[np.ix_(order, order)])))


def test_refusals():
    with pytest.raises(ValueError, match="rates"):
        _drift.normalize(-0.1, None, 3)                                   # a negative standard deviation
    with pytest.raises(ValueError, match="rates"):
        _drift.normalize([0.1, -0.2, 0.1], None, 3)
    with pytest.raises(ValueError, match="rates"):
        _drift.normalize({1: float("nan")}, None, 3)
    with pytest.raises(ValueError, match="rates"):                        # not positive semi-definite
        _drift.normalize(np.array([[1.0, 2.0], [2.0, 1.0]]), [0, 1], 3)
    with pytest.raises(ValueError, match="rates"):                        # not symmetric
        _drift.normalize(np.array([[1.0, 0.5], [0.0, 1.0]]), [0, 1], 3)
    with pytest.raises(ValueError, match="rates"):                        # the wrong size
        _drift.normalize(np.eye(2), None, 3)
    with pytest.raises(ValueError, match="rates"):
        _drift.normalize([0.1, 0.2], None, 3)
    with pytest.raises(IndexError):                                       # a row out of range
        _drift.normalize(0.1, [3], 3)
    with pytest.raises(IndexError):
        _drift.normalize({-4: 0.1}, None, 3)
    with pytest.raises(IndexError):
        _drift.normalize(0.1, [0.5], 3)
    with pytest.raises(ValueError, match="twice"):                        # a row named twice
        _drift.normalize(0.1, [1, 1], 3)
    with pytest.raises(ValueError, match="twice"):
        _drift.normalize(0.1, [1, -2], 3)
    with pytest.raises(ValueError, match="rows"):                         # a mapping names its rows itself
        _drift.normalize({0: 0.1}, [0], 3)
    with pytest.raises(ValueError, match="OBE_FAST_DIMS"):                # K > 16
        _drift.normalize(0.1, None, 17)
    rows, _ = _drift.normalize(0.1, list(range(16)), 40)                  # 16 rows of a wide cloud: fine
    assert rows.size == 16
    rows, _ = _drift.normalize([0.1] * 16 + [0.0], None, 17)              # ... and 17 rows of which 16 drift
    assert rows.size == 16
    with pytest.raises(ValueError, match="at_bounds"):
        _drift.settings(0.1, None, 3, at_bounds="fold")
    for bad in (-1.0, -1e-300, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="dt"):
            _drift.check_dt(bad)
    assert _drift.check_dt(0) == 0.0 and _drift.check_dt(2) == 2.0


def test_the_factor_is_the_cholesky_factor_times_root_dt():
    Q = np.array([[4.0, 1.0], [1.0, 2.0]])
    L = _drift.normalize(Q, None, 2)[1]
    G = _drift.factor(L, 0.3)
    assert_array_equal(_bits(G), _bits(L * math.sqrt(0.3)))
    assert G.flags.c_contiguous and G[0, 1] == 0.0
    assert_array_equal(_drift.factor(L, 1.0), L)


def test_settings_and_their_copy():
    s = _drift.settings({2: 0.3, 0: 0.1}, None, 4, per_update=1, at_bounds="reflect")
    assert s["rows"].tolist() == [0, 2] and s["per_update"] is True and s["at_bounds"] == "reflect"
    c = _drift.copy(s)
    assert c["rows"] == (0, 2) and c["cholesky"] is not s["cholesky"]
    c["cholesky"][0, 0] = 9.0
    assert s["cholesky"][0, 0] == 0.1
    assert _drift.settings(None, None, 4) is None and _drift.copy(None) is None


def test_reflection_bounds_only_where_a_drifted_row_is_bounded():
    s = _drift.settings({0: 0.1, 2: 0.3}, None, 4, at_bounds="reflect")
    lower, upper = np.array([-np.inf, 0.0, 0.0, -np.inf]), np.array([np.inf, 1.0, np.inf, np.inf])
    flags = np.zeros(4, dtype=bool)
    lo, hi = _drift.reflection_bounds(s, (lower, upper, flags, flags))
    assert_array_equal(lo, [-np.inf, 0.0])
    assert_array_equal(hi, [np.inf, np.inf])
    only_row_1 = (np.array([-np.inf, 0.0, -np.inf, -np.inf]), np.full(4, np.inf), flags, flags)
    assert _drift.reflection_bounds(s, only_row_1) is None                # no bound on a drifted row: the mask's call
    assert _drift.reflection_bounds(s, None) is None
    masked = _drift.settings({0: 0.1, 2: 0.3}, None, 4, at_bounds="mask")
    assert _drift.reflection_bounds(masked, (lower, upper, flags, flags)) is None


# ---------------------------------------------------------------------------------------------- the oracle
def test_the_oracle_is_a_hand_worked_example():
    """D = 3, rows 0 and 2, two particles, exact binary fractions: every step written out."""
    x = np.array([[1.0, 2.0], [7.0, 7.5], [10.0, 20.0]])
    z = np.array([[0.5, -1.0], [2.0, 0.25]])
    G = np.array([[2.0, 0.0], [-1.0, 0.5]])
    # p = 0: s0 = 0.5*2 = 1, s1 = -0.5 - 0.5 = -1;  p = 1: s0 = 4, s1 = -2 + 0.125
    want = np.array([[2.0, 6.0], [7.0, 7.5], [9.0, 18.125]])
    assert_array_equal(_bits(do.drift_exact(x, [0, 2], z, G)), _bits(want))
    # reflected at [1.5, 5] on row 0 and [9.5, +inf) on row 2: 6 -> 5 - 1 = 4, 9 -> 9.5 + 0.5 = 10
    reflected = np.array([[2.0, 4.0], [7.0, 7.5], [10.0, 18.125]])
    assert_array_equal(_bits(do.drift_exact(x, [0, 2], z, G, [1.5, 9.5], [5.0, np.inf])), _bits(reflected))


def test_reflection_takes_one_step_and_leaves_nan_alone():
    v = np.array([[-0.25, 1.25, -3.0, 0.0, 1.0, np.nan, 0.5]])
    got = do.reflect_two_roundings(v, [0.0], [1.0])
    # past lo, past hi, past both by more than the interval (still outside: no folding), exactly on a bound, NaN, inside
    assert_array_equal(_bits(got), _bits(np.array([[0.25, 0.75, 3.0, 0.0, 1.0, np.nan, 0.5]])))
    assert_array_equal(do.reflect_two_roundings(v, [-np.inf], [np.inf])[:, :5], v[:, :5])


@pytest.mark.parametrize("k,d", [(1, 1), (2, 2), (3, 6), (16, 16), (2, 40)])
def test_on_exact_data_the_oracle_is_integer_arithmetic(k, d):
    x, rows, z, G = do.integer_case(k, 97, d)
    want = do.drift_integers(x, rows, z, G)
    assert_array_equal(_bits(do.drift_exact(x, rows, z, G)), _bits(want))
    for wrong in do.WRONG_CHAINS.values():                                # exact data: every order, the same bits
        assert_array_equal(_bits(wrong(x, rows, z, G)), _bits(want))
    plain = x.copy()
    plain[rows] += (z @ G.T).T                                            # plain NumPy, written out
    assert_array_equal(want, plain)
    untouched = np.setdiff1d(np.arange(d), rows)
    assert_array_equal(_bits(want[untouched]), _bits(x[untouched]))


def test_spread_rows_are_ascending_and_not_adjacent():
    for k in (1, 2, 3, 8, 16):
        assert do.spread_rows(k, k).tolist() == list(range(k))
        rows = do.spread_rows(k, k + 3)
        assert rows.size == k and np.all(np.diff(rows) > 0) and rows[-1] == k + 2
        if k > 1:
            assert np.any(np.diff(rows) > 1)
    assert do.spread_rows(2, 40).tolist() == [0, 39]


@pytest.mark.parametrize("k", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("extra", [0, 3])
def test_the_gpu_inputs_tell_the_contract_from_its_neighbours(k, extra):
    """Each wrong chain moves at least one of the K x 293 drifted values (of these draws: 5 / 5 / 94 at K = D = 2,
    1 / 4 / 85 at K = 2, D = 5, 176 / 252 / 2424 at K = D = 16).  At K = 1 a one-term chain from zero is the rounded
    product whichever way it is written: only the chain started from x differs there.  With a lower-triangular G the
    first drifted row has one term at any K, and a row of scale 1 .. D absorbs most last-bit changes of a sum of scale
    0.1: the counts are small at small K."""
    x, rows, z, G = do.general_case(k, N, k + extra)
    assert np.all(np.triu(G, 1) == 0.0) and np.all(G[np.tril_indices(k)] != 0.0)
    want = do.drift_exact(x, rows, z, G)
    untouched = np.setdiff1d(np.arange(k + extra), rows)
    assert_array_equal(_bits(want[untouched]), _bits(x[untouched]))
    for name, wrong in do.WRONG_CHAINS.items():
        if k == 1 and name != "started from x":
            continue
        differ = int(np.count_nonzero(_bits(wrong(x, rows, z, G)) != _bits(want)))
        print(f"K = {k}, D = {k + extra}: {name}: {differ} of {k * N} drifted values differ")
        assert differ >= 1, name


@pytest.mark.parametrize("k", [1, 2, 3, 8, 16])
def test_the_gpu_inputs_tell_the_reflection_from_a_contracted_one(k):
    """fma(2, lo, -v) against lo + (lo - v) rounded twice on the GPU file's reflecting case: nearly every value is
    reflected, and at least a tenth of those differ (of these draws: about half)."""
    x, rows, z, G = do.general_case(k, N, k + 3)
    moved = do.drift_exact(x, rows, z, G)[rows]
    lo, hi = do.reflection_interval(k)
    below, above = moved < lo[:, None], moved > hi[:, None]
    assert np.count_nonzero(below) >= 0.3 * moved.size and np.count_nonzero(above) >= 0.3 * moved.size
    once = do.reflect_two_roundings(moved, lo, hi)
    still_outside = int(np.count_nonzero((once < lo[:, None]) | (once > hi[:, None])))
    assert still_outside >= 0.5 * moved.size                              # one reflection, no folding
    differ = int(np.count_nonzero(_bits(do.reflect_contracted(moved, lo, hi)) != _bits(once)))
    outside = int(np.count_nonzero(below | above))
    print(f"K = {k}: contracted reflection: {differ} of {outside} reflected values differ")
    assert differ >= 5 and differ >= 0.1 * outside
    assert_array_equal(_bits(do.drift_exact(x, rows, z, G, lo, hi)[rows]), _bits(once))
