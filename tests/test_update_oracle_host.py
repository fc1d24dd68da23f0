"""The references of tests/_update_oracle.py, pinned on the CPU: the exact update clouds against fractions.Fraction
(and every realisation of them — likelihood, supplied y, model — against the documented arithmetic in float64), the
long double likelihood against mpmath at 50 digits, the special values against NumPy, resample_due against its
statement; and the SENSITIVITY of the comparisons that tests/test_gpu_update_exact.py makes: on that file's own inputs
every mutant of the reference (a particle dropped or applied twice, sigma[0] for every channel, 1/s left out after
channel 0, the choke per channel, n_lik_channels ignored, a noise row off by one, nan_to_num missing on t, a float32
exponent) is rejected by the comparison used there — equality of bits, or likelihood_bound — on EVERY case it applies
to.  (The choke per channel is the same number as the choke on the product wherever both exist; it differs where the
product of two negative factors is positive, which is what particles 5 and 6 of the noise-row cases are for.)"""
from fractions import Fraction

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _update_oracle as uo

SMALL_N = (1, 2, 3, 63, 64, 65, 255, 256, 257)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _float64_likelihood(y, y_meas, sig, n_lik):
    """likelihood_of in float64, operation by operation (np.exp(-0.0) == 1 and np.exp(-2048) == 0 exactly)."""
    a, s = uo.exp_arguments(y, y_meas, sig, n_lik)
    lk = np.ones(a.shape[1])
    with np.errstate(all="ignore"):
        for c in range(n_lik):
            lk = lk * (np.exp(-a[c]) / s[c])
    return lk


# ------------------------------------------------------------------------------------------------ (a) exact clouds
@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("n", SMALL_N)
def test_exact_cloud_is_rational_arithmetic(n, fixed):
    cloud = uo.exact_update_cloud(np.random.default_rng(50 + n), n, uo.J_MAX if fixed else None)
    w, lik = cloud.prior(), cloud.lik()
    for shift in (0, 5):
        t = [Fraction(float(a)) * Fraction(float(b)) * 2 ** shift for a, b in zip(w, lik)]
        total = sum(t)
        w1 = [v / total for v in t]
        w2 = sum(v * v for v in w1)
        for v in t + w1 + [total, w2]:
            assert Fraction(float(v)) == v, "every value of an exact cloud is a float64 value"
        got_w, got_t, got_w2 = cloud.posterior(shift)
        _same_bits(got_w, [float(v) for v in w1], f"n={n}: weights")
        assert float(total) == got_t and float(w2) == got_w2
    if fixed:
        assert np.all(cloud.j == uo.J_MAX)


@pytest.mark.parametrize("n", uo.EXACT_SMALL + uo.EXACT_GRID)
def test_exact_cases_of_the_gpu_file_notice_any_single_particle(n):
    """Dropping or applying twice ANY single live particle changes the bits of sum t (and the last particle, live or
    dead, is covered by the weights themselves: its own weight is compared)."""
    for fixed in (False, True):
        cloud = uo.exact_case(n, fixed)
        _, total, _ = cloud.posterior()
        t = cloud.prior() * cloud.lik()
        live = ~cloud.dead
        assert np.all(t[live] > 0) and np.all(t[~live] == 0)
        assert np.all(total - t[live] != total) and np.all(total + t[live] != total)
        assert float(np.sum(t)) == total                       # (np.sum's own order: exact as every other)


@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_every_realisation_of_an_exact_cloud_is_the_same_update(n):
    """The y problems (rows and fixed sigma, 1 ... 8 channels, n_lik < channels) and the model problems, evaluated by
    the documented arithmetic in float64, give the cloud's likelihood times 2^shift — to the bit."""
    g = np.random.default_rng(70 + n)
    for fixed in (False, True):
        cloud = uo.exact_case(n, fixed)
        for c, n_lik in ((1, 1), (2, 2), (3, 2), (8, 8), (8, 5)):
            p = uo.exact_y_problem(g, cloud, c, n_lik, rows=not fixed)
            sig = p["particles"][p["noise_rows"]] if not fixed else p["sigma"]
            assert np.all(np.isnan(p["y"][n_lik:]))
            _same_bits(_float64_likelihood(p["y"], p["y_meas"], sig, n_lik), np.ldexp(cloud.lik(), p["shift"]),
                       f"n={n} fixed={fixed} channels={c}/{n_lik}")
        for model, d, row in (("line_ab", 2, None), ("line_ab", 3, 2), ("line_ab", 16, 9), ("first_param", 2, 1)):
            if (row is None) != fixed:
                continue
            p = uo.exact_model_problem(g, cloud, model, d, row)
            x = p["particles"]
            y = x[0] + x[1] * p["setting"] if model == "line_ab" else x[0]
            sig = x[p["noise_rows"]] if row is not None else np.array([p["sigma"]])
            _same_bits(_float64_likelihood(y[None], [p["y_meas"]], sig, 1), np.ldexp(cloud.lik(), p["shift"]),
                       f"n={n} {model} d={d}")
            assert np.all(x == np.round(x)) or row is not None


# --------------------------------------------------------------------------------------------- (b) general doubles
def test_general_cases_cover_what_the_issue_lists():
    cases = uo.GENERAL_CASES
    assert {c[0] for c in cases} == {1, 2, 8, 9, 16, 17}
    assert {c[3] for c in cases} == {None, 0.6, 1.7} and {c[2] for c in cases} == {False, True}
    for c in (2, 8, 9, 16, 17):
        assert {k[1] == c for k in cases if k[0] == c} == {True, False}
    assert any(k[1] > 8 and k[1] < k[0] for k in cases)
    p = uo.general_case((17, 17, True, None))
    assert len(set(p["noise_rows"].tolist())) == 17 and p["y"].shape == (17, uo.GENERAL_N)
    a, _ = uo.exp_arguments(p["y"], p["y_meas"], p["sig"], 17)
    z = np.sqrt(2 * a.sum(axis=0))
    assert z.min() == 0.0 and 39.9 < z.max() < 40.1
    assert np.abs(p["y_meas"]).max() > 1e4


@pytest.mark.parametrize("case", [uo.EXP_CASE, uo.POW_CASES[0], uo.POW_CASES[1]] + uo.GENERAL_CASES[::5])
def test_likelihood_ld_against_mpmath(case):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    p = uo.general_case(case)
    n_lik, choke = p["n_lik"], p["choke"]
    ref = uo.likelihood_ld(p["y"], p["y_meas"], p["sig"], n_lik, choke)
    bound = uo.likelihood_bound(p["y"], p["y_meas"], p["sig"], n_lik, choke)
    a, s = uo.exp_arguments(p["y"], p["y_meas"], p["sig"], n_lik)
    cols = sorted(set(range(12)) | set(uo.SPECIAL_COLUMNS) | set(range(20, uo.GENERAL_N, 37)))
    for i in cols:
        lik = mp.mpf(1)
        for c in range(n_lik):
            lik *= mp.exp(-mp.mpf(float(a[c, i]))) / mp.mpf(float(s[c, i]))
        if choke is not None:
            if lik < 0:
                assert np.isnan(ref[i]) and np.isnan(bound[i])
                continue
            lik = lik ** mp.mpf(choke)
        got = mp.mpf(int(np.frexp(ref[i])[0] * 2.0 ** 64)) * mp.mpf(2) ** (int(np.frexp(ref[i])[1]) - 64)
        own = (3 * n_lik + 2) * uo.U_REF * (1 if choke is None else max(1.0, choke))
        assert abs(got - lik) <= own * abs(lik), (case, i, got, lik)
        assert bound[i] > 0 and (lik == 0 or bound[i] >= 2 ** -53 * float(abs(got)))


@pytest.mark.parametrize("case", [uo.EXP_CASE, *uo.POW_CASES] + uo.GENERAL_CASES)
def test_the_documented_arithmetic_in_float64_is_within_the_bound(case):
    """A right kernel passes: likelihood_of evaluated with NumPy's float64 exp and power (both good to one ulp)."""
    p = uo.general_case(case)
    n_lik, choke = p["n_lik"], p["choke"]
    lk = _float64_likelihood(p["y"], p["y_meas"], p["sig"], n_lik)
    with np.errstate(all="ignore"):
        lk = lk if choke is None else np.power(lk, choke)
    frac = uo.fraction_of_bound(lk, uo.likelihood_ld(p["y"], p["y_meas"], p["sig"], n_lik, choke),
                                uo.likelihood_bound(p["y"], p["y_meas"], p["sig"], n_lik, choke))
    assert frac.max() <= 1.0, (case, int(frac.argmax()), frac.max())
    if isinstance(case, tuple) and case[0] != "pow" and case[2] and case[1] >= 2 and choke is not None:
        assert np.isnan(lk[7]) and not np.isnan(lk[5]) and not np.isnan(lk[6])


@pytest.mark.parametrize("case", uo.GENERAL_CASES)
def test_every_likelihood_mutant_leaves_the_bound(case):
    p = uo.general_case(case)
    n_lik, choke = p["n_lik"], p["choke"]
    ref = uo.likelihood_ld(p["y"], p["y_meas"], p["sig"], n_lik, choke)
    bound = uo.likelihood_bound(p["y"], p["y_meas"], p["sig"], n_lik, choke)
    mutants = uo.likelihood_mutants(case)
    want = {"a float32 exponent"}
    if n_lik >= 2:
        want |= {"sigma[0] used for every channel", "1/s omitted after channel 0"}
        if choke is not None and case[2]:
            want.add("the choke applied per channel")
    if n_lik < case[0]:
        want.add("n_lik_channels ignored")
    if case[2]:
        want.add("a noise row off by one")
    assert set(mutants) == want
    for name, lik in mutants.items():
        assert uo.fraction_of_bound(lik, ref, bound).max() > 1.0, f"{case}: {name} passes the comparison"


@pytest.mark.parametrize("case", [k for k in uo.GENERAL_CASES if k[0] <= 8])
def test_a_dropped_or_repeated_particle_leaves_the_bound_on_sum_t(case):
    """The posterior cases of the GPU file (supplied y, up to 8 channels): sum t without the last particle, or with
    one of the SPECIAL_COLUMNS twice, is beyond sum_t_bound."""
    p = uo.general_case(case)
    ref = uo.likelihood_ld(p["y"], p["y_meas"], p["sig"], p["n_lik"], p["choke"])
    bound = uo.likelihood_bound(p["y"], p["y_meas"], p["sig"], p["n_lik"], p["choke"])
    w1, total = uo.posterior_ld(p["w"], ref)
    b = uo.sum_t_bound(p["w"], ref, bound)
    t = uo.nan_to_num_ld(p["w"].astype(uo.LD) * ref)
    assert 0 < b < 1e-12 * float(total)
    for col in uo.SPECIAL_COLUMNS:
        assert float(t[col]) > b, (case, col)                  # dropped or applied twice: beyond the bound
    assert abs(float(w1.sum()) - 1.0) < 1e-15


# ----------------------------------------------------------------------------------------------- (c) special values
def test_special_values_against_numpy():
    cases = uo.special_cases()
    assert set(cases) == {"one NaN weight", "w = inf with L = 0", "one t = DBL_MAX among tiny others",
                          "two infinities", "every likelihood zero", "a negative weight"}
    for name, (w, j, dead, needs) in cases.items():
        lik = uo.special_lik(j, dead)
        w1, total, w2 = uo.posterior_np(w, lik)
        assert len(w) == uo.SPECIAL_N <= 256
        # order independent: any permutation of the cloud gives the same bits
        g = np.random.default_rng(3)
        for _ in range(5):
            perm = g.permutation(len(w))
            p1, ptotal, pw2 = uo.posterior_np(w[perm], lik[perm])
            _same_bits(p1, w1[perm], name)
            assert _bits([ptotal, pw2]).tolist() == _bits([total, w2]).tolist(), name
        assert np.all(np.isfinite(w1))
        mutant = uo.posterior_without_nan_to_num_on_t(w, lik)
        differs = not np.array_equal(_bits(mutant[0]), _bits(w1)) or _bits([mutant[1]])[0] != _bits([total])[0]
        assert differs == needs, f"{name}: nan_to_num missing on t"
    w1, total, w2 = uo.posterior_np(*[(c[0], uo.special_lik(c[1], c[2])) for c in [cases["every likelihood zero"]]][0])
    assert not w1.any() and total == 0.0 and w2 == 0.0
    w1, total, w2 = uo.posterior_np(*[(c[0], uo.special_lik(c[1], c[2])) for c in [cases["two infinities"]]][0])
    assert not w1.any() and total == np.inf and w2 == 0.0
    c = cases["one t = DBL_MAX among tiny others"]
    w1, total, w2 = uo.posterior_np(c[0], uo.special_lik(c[1], c[2]))
    assert total == uo.DBL_MAX and w2 == 1.0 and np.count_nonzero(w1 == 1.0) == 1
    c = cases["a negative weight"]
    w1, total, w2 = uo.posterior_np(c[0], uo.special_lik(c[1], c[2]))
    assert np.count_nonzero(w1 < 0) == 1 and total > 0


# ------------------------------------------------------------------------------------------------ (d) resample test
def test_resample_due_is_the_statement_of_the_header():
    n = 1000
    assert uo.resample_due(1.0 / 99.0, n, 0.0) and not uo.resample_due(1.0 / 101.0, n, 0.0)
    assert not uo.resample_due(1.0 / 100.0, n, 0.0) or 1.0 / (1.0 / 100.0) < 0.1 * n
    assert uo.resample_due(1.0 / 500.0, n, 0.51) and not uo.resample_due(1.0 / 500.0, n, 0.49)
    assert not uo.resample_due(0.0, n, 0.5)                     # n_eff = inf
    assert not uo.resample_due(np.nan, n, 0.5)                  # every comparison with NaN is false
    assert uo.resample_due(np.inf, n, 0.0)                      # n_eff = 0
    for s in np.random.default_rng(8).uniform(1e-4, 1e-1, 200):
        n_eff = 1.0 / s
        assert uo.resample_due(s, n, 0.3) == (n_eff < 0.1 * n or n_eff / n < 0.3)
