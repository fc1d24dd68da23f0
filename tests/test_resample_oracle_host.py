"""tests/_resample_oracle.py on the CPU: its fma against the rational definition, the oracle against a hand-worked case
and against integer arithmetic, and the inputs of tests/test_gpu_resample_exact.py against the neighbours of the
contract — a chain that rounds its products, one summed in the other order, one started from the old value, a
contracted scale step: each must move enough outputs of those inputs for a bit-for-bit comparison to see it."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _resample_oracle as ro

N = 293                      # the cloud of the GPU file's general cases


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_the_c_library_fma_is_the_rational_one_on_the_table():
    f = ro._libm_fma()
    assert f is not None, "no fma in the C maths library: the oracle would fall back to the (slow) rational form"
    assert len(ro.FMA_TABLE) >= 400
    differs_from_two_roundings = 0
    for x, y, c in ro.FMA_TABLE:
        want = ro.fma_exact(x, y, c)
        assert _bits(f(x, y, c)) == _bits(want), (x, y, c)
        differs_from_two_roundings += _bits(x * y + c) != _bits(want)
    assert ro.fast_fma_checked() is not None
    # the table can tell: a multiply-then-add gives other bits on most of the crafted rows
    assert differs_from_two_roundings >= 75


def test_fma_exact_rounds_once():
    x = 1.0 + 2.0 ** -30
    assert x * x == 1.0 + 2.0 ** -29                                    # the 2^-60 term is lost ...
    assert ro.fma_exact(x, x, -(x * x)) == 2.0 ** -60                   # ... unless the product is kept exact
    assert ro.fma_exact(x, x, 2.0 ** -53) == 1.0 + 2.0 ** -29 + 2.0 ** -52     # above the tie: up
    assert x * x + 2.0 ** -53 == 1.0 + 2.0 ** -29                       # two roundings: the tie goes to even
    assert ro.fma_exact(3.0, 5.0, 7.0) == 22.0
    assert ro.fma_exact(0.1, 10.0, -1.0) == 2.0 ** -54                  # 0.1 = (1 + 2^-54 ...)/10 exactly above a tenth


def test_the_oracle_is_a_hand_worked_example():
    """D = 2, two particles, exact binary fractions: every step written out."""
    old = np.array([[1.0, 2.0], [10.0, 20.0]])
    idx = np.array([1, 0])
    z = np.array([[0.5, -1.0], [2.0, 0.25]])
    F = np.array([[2.0, 4.0], [-1.0, 0.5]])
    mean = np.array([3.0, -8.0])
    # p = 0 (source 1): s0 = 0.5*2 - 1*4 = -3, s1 = -0.5 - 0.5 = -1;  p = 1 (source 0): s0 = 4 + 1 = 5, s1 = -2 + 0.125
    want = np.array([[2.0 - 3.0, 1.0 + 5.0], [20.0 - 1.0, 10.0 - 1.875]])
    assert_array_equal(_bits(ro.nudge_exact(old, idx, z, F, mean, 0.5, 0)), _bits(want))
    scaled = np.array([[-0.5 + 1.5, 3.0 + 1.5], [9.5 - 4.0, 4.0625 - 4.0]])
    assert_array_equal(_bits(ro.nudge_exact(old, idx, z, F, mean, 0.5, 1)), _bits(scaled))
    # a = 0.75: 1 - a = 0.25
    assert_array_equal(ro.nudge_exact(old, idx, z, F, mean, 0.75, 1), want * 0.75 + (mean * 0.25)[:, None])
    # indices outside the cloud read its ends
    assert_array_equal(ro.nudge_exact(old, np.array([5, -3]), z, F, mean, 0.5, 0),
                       ro.nudge_exact(old, np.array([1, 0]), z, F, mean, 0.5, 0))
    assert_array_equal(ro.clamp([-1, 2, 2 ** 62, -2 ** 62, 7], 2), [0, 1, 1, 0, 1])


def test_one_rounding_where_two_differ():
    """D = 1: the only chain step is fma(z, F, 0) = the rounded product; D = 2 with a product whose tail matters."""
    x = 1.0 + 2.0 ** -30
    old, idx, mean = np.zeros((2, 1)), np.array([0]), np.zeros(2)
    z = np.array([[x, 1.0]])
    F = np.array([[-(x * x), x], [x, -(x * x)]])
    got = ro.nudge_exact(old, idx, z, F, mean, 0.5, 0)
    # row 0: fma(1, x, fma(x, -x*x, 0)) ; row 1: fma(1, -x*x, fma(x, x, 0)) = x*x - x*x = 0 (the first step rounds)
    assert got[1, 0] == 0.0
    assert got[0, 0] == ro.fma_exact(1.0, x, x * -(x * x))
    rev = ro.nudge_reversed_j(old, idx, z, F, mean, 0.5, 0)
    assert rev[1, 0] == 2.0 ** -60                                      # the other order keeps the tail
    assert ro.nudge_mul_then_add(old, idx, z, F, mean, 0.5, 0)[1, 0] == 0.0


@pytest.mark.parametrize("d", [1, 2, 5, 16, 17])
@pytest.mark.parametrize("scale", [0, 1])
def test_on_exact_data_the_oracle_is_integer_arithmetic(d, scale):
    old, idx, z, F, mean = ro.integer_case(d, 97)
    idx[:3] = (-1, 97, 2 ** 62)                                         # the clamp, both sides
    want = ro.nudge_integers(old, idx, z, F, mean, scale)
    assert_array_equal(_bits(ro.nudge_exact(old, idx, z, F, mean, 0.5, scale)), _bits(want))
    for wrong in ro.WRONG_CHAINS.values():                              # exact data: every order, the same bits
        assert_array_equal(_bits(wrong(old, idx, z, F, mean, 0.5, scale)), _bits(want))
    # plain NumPy, written out
    v = old[:, np.clip(idx, 0, 96)] + (z @ F.T).T
    assert_array_equal(want, v * 0.5 + (mean * 0.5)[:, None] if scale else v)


@pytest.fixture(scope="module")
def unscaled():
    """The oracle before its scale step on the GPU file's inputs, once per width."""
    return {d: ro.unscaled_exact(*ro.general_case(d, N)[:4]) for d in range(1, 17)}


@pytest.mark.parametrize("d", range(1, 17))
def test_the_gpu_inputs_tell_the_contract_from_its_neighbours(unscaled, d):
    """Each wrong chain moves at least 5 outputs, and from D = 4 on at least 1 % of them (measured with draws of this
    kind: 25 / 32 / 181 of 586 at D = 2, 94 / 100 / 520 of 1172 at D = 4, 470 / 642 / 3123 of 4688 at D = 16).  At
    D = 1 a one-term chain from zero is the rounded product whichever way it is written: only the chain started from
    the old value differs there."""
    old, idx, z, F, mean = ro.general_case(d, N)
    want = unscaled[d]
    for name, wrong in ro.WRONG_CHAINS.items():
        if d == 1 and name != "started from old":
            continue
        differ = int(np.count_nonzero(_bits(wrong(old, idx, z, F, mean, ro.A_PARAM, 0)) != _bits(want)))
        print(f"D = {d}: {name}: {differ} of {want.size} outputs differ")
        assert differ >= 5, name
        if d >= 4:
            assert differ >= 0.01 * want.size, name
    # ... and the scale step keeps them apart (a, the mean: the GPU file's)
    scaled = ro.scale_two_roundings(want, mean, ro.A_PARAM)
    assert_array_equal(_bits(scaled), _bits(ro.nudge_exact(old, idx, z, F, mean, ro.A_PARAM, 1)))


@pytest.mark.parametrize("d", range(1, 17))
def test_the_gpu_inputs_tell_the_scale_step_from_a_contracted_one(unscaled, d):
    """fma(v, a, mean*(1 - a)) against v*a + mean*(1 - a) rounded three times: at least 1 % of the outputs differ
    (measured 1186 of 5000 on v ~ N(0, 3), mean 1.7, a = 0.98)."""
    mean = ro.general_case(d, N)[4]
    v = unscaled[d]
    differ = int(np.count_nonzero(_bits(ro.scale_contracted(v, mean, ro.A_PARAM))
                                  != _bits(ro.scale_two_roundings(v, mean, ro.A_PARAM))))
    print(f"D = {d}: contracted scale step: {differ} of {v.size} outputs differ")
    assert differ >= 0.01 * v.size


def test_violators_open_and_closed_ends():
    new = np.array([[0.0, -0.0, 1.0, 2.0, 3.0], [5.0, 5.0, 5.0, 5.0, 9.0]])
    assert_array_equal(ro.violators(new, [0], [1.0], [2.0], [0]), [True, True, False, False, True])
    assert_array_equal(ro.violators(new, [0], [1.0], [2.0], [3]), [True, True, True, True, True])
    assert_array_equal(ro.violators(new, [0], [1.0], [2.0], [1]), [True, True, True, False, True])
    assert_array_equal(ro.violators(new, [0], [0.0], [np.inf], [1]), [True, True, False, False, False])
    assert_array_equal(ro.violators(new, [0], [0.0], [np.inf], [0]), [False, False, False, False, False])
    # two entries for one row intersect; an entry on another row adds its own violators
    assert_array_equal(ro.violators(new, [0, 0, 1], [0.0, 1.0, -np.inf], [3.0, np.inf, 9.0], [0, 0, 2]),
                       [True, True, False, False, True])
