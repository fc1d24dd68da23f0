"""The two references of tests/_moments_oracle.py, pinned on the CPU: exact_block against rational arithmetic, the
oracle package and np.cov; longdouble_block against rational arithmetic; and the SENSITIVITY of the comparison that
tests/test_gpu_moments_exact.py makes — on that file's own general inputs every mutant of the reference (a dropped
particle at the places a kernel loses one, the tiled path's plausible mistakes, the two terms of the scale) moves at
least one value of the block beyond block_bounds.  Condition: each mutation that applies to a case's shape is caught
on EVERY listed case; the inputs (weights over 300 decades with the critical particles at the top of the range, sum w
= 0.8125, rows of distinct scale and distinct mean) are chosen so that the reference alone satisfies it."""
import decimal
import math
from fractions import Fraction

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _moments_oracle as mo
import oracle

SMALL_N = (1, 2, 3, 64, 257, 293)


def _fl(v):
    """A rational number rounded once to float64 (Fraction.__float__ rounds correctly)."""
    return float(v)


def _fraction_block(x, w, exact_sums=False):
    """The block by fractions.Fraction: the sums exactly (required to BE float64 values when exact_sums), then the
    documented operations, each a single correctly rounded step."""
    d, n = x.shape
    fx = [[Fraction(float(v)) for v in row] for row in x]
    fw = [Fraction(float(v)) for v in w]
    w_sum, w2 = sum(fw), sum(v * v for v in fw)
    m1 = [sum(a * b for a, b in zip(row, fw)) for row in fx]
    m2 = [sum(a * a * b for a, b in zip(row, fw)) for row in fx]
    mean = [v / w_sum for v in m1]
    dev = [[a - mu for a in row] for row, mu in zip(fx, mean)]
    s = [[None] * d for _ in range(d)]
    for i in range(d):
        dw = [a * c for a, c in zip(dev[i], fw)]
        for j in range(i, d):
            s[i][j] = s[j][i] = sum(a * b for a, b in zip(dw, dev[j]))
    if not exact_sums:
        return w_sum, w2, mean, m1, m2, s
    for v in [w_sum, w2] + m1 + m2 + [v for row in s for v in row]:
        assert Fraction(_fl(v)) == v, "a sum of an exact cloud is a float64 value"
    out = np.empty(mo.block_len(d))
    sec = mo.sections(d)
    out[0], out[1] = _fl(w_sum), _fl(w2)
    out[sec["mean"]] = [_fl(v) for v in mean]
    out[sec["m1"]], out[sec["m2"]] = [_fl(v) for v in m1], [_fl(v) for v in m2]
    sq = [Fraction(_fl(v * v)) for v in m1]
    var = [_fl(b - a) for a, b in zip(sq, m2)]            # (negative where sum w > 1 and the centre is far out: NaN)
    out[sec["std"]] = [math.sqrt(v) if v >= 0 else np.nan for v in var]
    fact = Fraction(_fl(w_sum - Fraction(_fl(w2 / w_sum))))
    if fact == 0:
        out[sec["cov"]] = np.nan                       # 0 * inf
        assert all(v == 0 for row in s for v in row)
    else:
        scale = Fraction(_fl(1 / fact))
        out[sec["cov"]] = [_fl(v * scale) for row in s for v in row]
    return out


def _same_bits(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert_array_equal(np.isnan(a), np.isnan(b), err_msg=what + ": NaN pattern")
    ok = ~np.isnan(a)
    assert_array_equal(a.view(np.int64)[ok], b.view(np.int64)[ok], err_msg=what)


@pytest.mark.parametrize("d", list(range(1, 17)) + [17, 33])
def test_exact_block_is_rational_arithmetic(d):
    g = np.random.default_rng(100 + d)
    for n in SMALL_N if d in (1, 5) else (293,):
        for shift in (0, 2, -3) if d in (1, 5) else ((0, 2, -3)[d % 3],):
            x, q, k = mo.exact_cloud(g, d, n, shift)
            _same_bits(mo.exact_block(x, q, k, shift), _fraction_block(x, mo.exact_weights(q, k, shift), True),
                       f"d={d} n={n} shift={shift}")
    # zero weights in between, and a one-hot weight (fact == 0)
    x, q, k = mo.exact_cloud(g, d, 64, 0)
    x, q = mo.with_zero_weights(g, x, q, 10, 7)
    _same_bits(mo.exact_block(x, q, k), _fraction_block(x, mo.exact_weights(q, k), True), f"d={d} zero weights")
    x, q, k = mo.exact_cloud(g, d, 1, 0)
    x, q = mo.with_zero_weights(g, x, q, 0, 5)
    hot = mo.exact_block(x, q, k)
    _same_bits(hot, _fraction_block(x, mo.exact_weights(q, k), True), f"d={d} one-hot")
    assert np.all(np.isnan(hot[mo.sections(d)["cov"]])) and np.all(hot[mo.sections(d)["std"]] == 0.0)


@pytest.mark.parametrize("d,n,shift", [(1, 293, 0), (3, 65537, 2), (16, 5000, -3), (17, 293, 0), (40, 5000, 2),
                                       (8, 2 ** 21 + 293, 0)])
def test_exact_block_is_the_oracle_package_and_numpy(d, n, shift):
    g = np.random.default_rng(200 + d)
    x, q, k = mo.exact_cloud(g, d, n, shift)
    assert q.max() <= mo.Q_MAX and int(q.sum()) == 1 << k
    w = mo.exact_weights(q, k, shift)
    blk, sec = mo.exact_block(x, q, k, shift), mo.sections(d)
    assert blk[0] == 2.0 ** shift
    assert_array_equal(blk[sec["mean"]], oracle.weighted_mean(x, w))          # (NumPy's sums are exact here as well)
    with np.errstate(invalid="ignore"):                    # (sum w = 4: m2 - m1^2 may be negative, NaN on both sides)
        assert_array_equal(blk[sec["std"]], oracle.weighted_std(x, w))
    cov = blk[sec["cov"]].reshape(d, d)
    assert_array_equal(cov, cov.T)
    assert_allclose(cov, oracle.weighted_covariance(x, w), rtol=1e-14)
    assert_allclose(cov, np.cov(x, aweights=w).reshape(d, d), rtol=1e-14)


def test_exact_cloud_refuses_what_would_not_be_exact():
    g = np.random.default_rng(3)
    x, q, k = mo.exact_cloud(g, 3, 293)
    big = q.copy()
    big[0], big[1] = big[0] + big[1], 0                    # still sums to 2^k, but may pass 2^10
    big[0] += mo.Q_MAX
    with pytest.raises(AssertionError):
        mo.exact_sums(x, big, k)
    with pytest.raises(AssertionError):
        mo.exact_sums(x + 0.5, q, k)
    shifted = x.copy()
    shifted[0, 0] += 1.0                                   # the mean is no integer any more
    with pytest.raises(AssertionError):
        mo.exact_sums(shifted, q, k)


def _sqrt_fraction(v):
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        return (decimal.Decimal(v.numerator) / decimal.Decimal(v.denominator)).sqrt()


@pytest.mark.parametrize("d,n", [(1, 293), (3, 5), (5, 293), (16, 64), (17, 64), (33, 24)])
def test_longdouble_block_is_rational_arithmetic(d, n):
    """... to 1 / 256 of block_bounds: the reference's own error is no part of what the GPU comparison measures."""
    x, w = mo.general_cloud(np.random.default_rng(300 + d), d, n)
    ref, bound, sec = mo.longdouble_block(x, w), mo.block_bounds(x, w, n), mo.sections(d)
    w_sum, w2, mean, m1, m2, s = _fraction_block(x, w)
    exact = [w_sum, w2] + mean + m1 + m2
    for at, want in enumerate(exact):
        err = abs(Fraction(*ref[at].as_integer_ratio()) - want)
        assert err <= Fraction(float(bound[at])) / 256, (d, n, at)
    for i in range(d):
        std = _sqrt_fraction(m2[i] - m1[i] * m1[i])
        at = sec["std"].start + i
        num, den = ref[at].as_integer_ratio()
        with decimal.localcontext() as ctx:
            ctx.prec = 60
            assert abs(decimal.Decimal(num) / decimal.Decimal(den) - std) <= decimal.Decimal(float(bound[at])) / 256, (d, n, i)
    fact = w_sum - w2 / w_sum
    for i in range(d):
        for j in range(d):
            at = sec["cov"].start + i * d + j
            err = abs(Fraction(*ref[at].as_integer_ratio()) - s[i][j] / fact)
            assert err <= Fraction(float(bound[at])) / 256, (d, n, i, j)


def test_block_bounds_are_of_the_order_of_the_arithmetic():
    """A bound is useful only if it is small: on every general case each is below 1e-9 of the scale of its value's
    own terms (the tolerance of the existing moment tests is 1e-10 ... 1e-12 of the value plus a share of the
    largest), and NumPy's float64 moments, an independent implementation of the same arithmetic, stay within it."""
    for d, n in [(1, 293), (16, 293), (7, 65537), (17, 5000), (40, 5000)]:
        x, w = mo.general_case(d, n)
        ref, bound, sec = mo.longdouble_block(x, w), mo.block_bounds(x, w, n), mo.sections(d)
        sd = np.sqrt(np.diag(ref[sec["cov"]].reshape(d, d).astype(np.float64)))
        assert np.all(bound[sec["mean"]] <= 1e-9 * np.maximum(np.abs(ref[sec["mean"]]), sd))
        assert np.all(bound[sec["cov"]].reshape(d, d) <= 1e-9 * np.outer(sd, sd))
        assert np.all(bound[:2] <= 1e-13 * np.abs(ref[:2]))
        m1, m2 = (x * w).sum(axis=1), (x * x * w).sum(axis=1)
        got = np.concatenate([[w.sum(), (w * w).sum()], m1 / w.sum(), m1, m2, np.sqrt(m2 - m1 * m1),
                              oracle.weighted_covariance(x, w).reshape(-1)])
        worst = mo.worst_fraction(got, ref, bound, d)
        assert max(worst.values()) < 1.0, (d, n, worst)


@pytest.mark.parametrize("d,n", mo.GENERAL_CASES)
def test_every_mutant_is_caught_on_the_gpu_files_inputs(d, n):
    x, w = mo.general_case(d, n)
    ref, bound = mo.longdouble_block(x, w), mo.block_bounds(x, w, n)
    assert np.all(np.isfinite(bound)) and np.all(bound > 0)
    found = mo.mutants(x, w)
    expected = {"the last particle dropped", "W = 1 used for sum w", "the W2 / W term left out"}
    if n > 256:
        expected |= {"particle 256 dropped", "the last workgroup's first particle dropped"}
    if n > 65536:
        expected |= {"particle 65 536 dropped"}
    if d > 16:
        expected |= {"a tile pair's i and j swapped", "a mean taken from the previous tile"}
        if d % 8:
            expected |= {"row d - 1 read in place of a short tile's zero padding"}
    assert set(found) == expected
    for name, block in found.items():
        worst = mo.worst_fraction(block, ref, bound, d)
        assert max(worst.values()) > 1.0, f"d={d} n={n}: '{name}' would pass the GPU comparison ({worst})"
