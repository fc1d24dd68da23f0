"""Pins the oracle (oracle/obe_oracle.py) against (1) golden vectors produced by the
real reference (tests/golden/make_golden.py) and (2) the literal expectations of the
reference's own unit tests for this path.  CPU only."""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _replay
import oracle
from oracle import models

ORACLE_MODELS = {
    "lorentzian": models.lorentzian,
    "multi_lorentzian_7": models.multi_lorentzian(7),
    "line_mb": models.line_mb,
    "rabi": models.rabi,
    "coil": models.coil,
}

# The oracle uses the same NumPy primitives as the reference, so it is held to a
# much tighter tolerance than the 1e-10 the HIP path is allowed.
ORACLE_RTOL = 1e-13


@pytest.mark.parametrize("name", _replay.TRAJECTORIES)
def test_trajectory_matches_reference(name):
    fx = _replay.load_traj(name)
    obe = _replay.construct(fx, oracle.OracleOptBayesExpt,
                            oracle.OracleOptBayesExptNoiseParameter,
                            ORACLE_MODELS[fx["meta"]["model"]])
    stats = _replay.replay(fx, obe, ORACLE_RTOL,
                           get_draw_idx=lambda o: o.last_draw_indices,
                           get_utility=lambda o: o.last_utility)
    assert stats["cycles"] == fx["meta"]["n_cycles"]
    assert stats["resamples"] == int(np.sum(fx["resampled"])) >= 5


@pytest.mark.parametrize("name", _replay.UTILITY_TRAJECTORIES)
def test_yspace_utility_trajectory_matches_reference(name):
    """max_min, pseudo_utility (van Es / Ebrahimi windows), full_kld_utility."""
    fx = _replay.load_traj(name)
    obe = _replay.construct(fx, oracle.OracleOptBayesExpt, oracle.OracleOptBayesExptNoiseParameter,
                            ORACLE_MODELS[fx["meta"]["model"]])
    obe.noise_rng = _replay.noise_rng(fx)
    stats = _replay.replay(fx, obe, ORACLE_RTOL,
                           get_draw_idx=lambda o: o.last_draw_indices,
                           get_utility=lambda o: np.asarray(o.last_utility).reshape(-1))
    assert stats["resamples"] == int(np.sum(fx["resampled"])) >= 5


@pytest.mark.parametrize("name", _replay.SWEEPER_TRAJECTORIES)
def test_sweeper_trajectory_matches_reference(name):
    """(start, stop) sweep selection and per-point updates of the reference's
    demos/sweeper/obe_sweeper.py, optimal and good selection."""
    fx = _replay.load_traj(name)
    ctor = dict(fx["meta"]["ctor"])
    obe = oracle.OracleOptBayesExptSweeper(models.lorentzian, (fx["setval_0"],), fx["prior"].copy(),
                                           tuple(fx["cons"]), **ctor)
    stats = _replay.replay_sweeper(fx, obe, ORACLE_RTOL, lambda g: setattr(obe, "sweep_rng", g),
                                   get_draw_idx=lambda o: o.last_draw_indices,
                                   get_utility=lambda o: o.last_utility)
    assert stats["points"] == len(fx["y_concat"]) > 100 and int(np.sum(fx["n_resamples"])) >= 10


def test_reference_conditioning_10_parameters(monkeypatch):
    """Why the HIP tolerance on the 10-parameter trajectory is 1e-6 and not 1e-10: the
    reference algorithm, run on the CPU with its weighted covariance summed in reverse
    particle order (an equally valid float64 evaluation), no longer reproduces its own
    golden utilities to 1e-10 once a resample has happened."""
    from oracle import obe_oracle
    fx = _replay.load_traj("multilorentz7_noise")
    straight = obe_oracle.weighted_covariance
    monkeypatch.setattr(obe_oracle, "weighted_covariance",
                        lambda p, w: straight(np.asarray(p)[:, ::-1].copy(), np.asarray(w)[::-1].copy()))
    obe = _replay.construct(fx, oracle.OracleOptBayesExpt, oracle.OracleOptBayesExptNoiseParameter,
                            ORACLE_MODELS["multi_lorentzian_7"])
    worst = 0.0
    import warnings
    for cyc in range(fx["meta"]["n_cycles"]):
        x = obe.opt_setting()
        assert obe.last_setting_index == fx["chosen_index"][cyc]
        worst = max(worst, np.abs(obe.last_utility / fx["utility"][cyc] - 1).max())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            obe.pdf_update((x, float(fx["y_meas"][cyc][0])))
    assert 2e-8 < worst < _replay.HIP_RTOL["multilorentz7_noise"]


def test_unit_cases():
    u = _replay.load("unit_cases.npz")
    for d in (1, 3, 10):
        x, w = u[f"mom{d}_x"], u[f"mom{d}_w"]
        assert_allclose(oracle.weighted_mean(x, w), u[f"mom{d}_mean"], rtol=1e-14)
        cov = oracle.weighted_covariance(x, w)
        assert cov.shape == (d, d)
        assert_allclose(cov, u[f"mom{d}_cov"], rtol=1e-13, atol=1e-13 * np.abs(u[f"mom{d}_cov"]).max())
        assert_allclose(oracle.weighted_std(x, w), u[f"mom{d}_std"], rtol=1e-13)
    for tag, scale in (("s0", False), ("s1", True)):
        pdf = oracle.OracleParticlePDF(u[f"rs_{tag}_x"].copy(), scale=scale)
        pdf.particle_weights = u[f"rs_{tag}_w"].copy()
        pdf.rng = np.random.default_rng(4242)
        draws = pdf.randdraw(30)
        assert_array_equal(pdf.last_draw_indices, u[f"rs_{tag}_draw_idx"])
        assert_array_equal(draws, u[f"rs_{tag}_draws"])
        pdf.resample()
        assert_array_equal(pdf.last_draw_indices, u[f"rs_{tag}_resample_idx"])
        assert_allclose(pdf.particles, u[f"rs_{tag}_particles"], rtol=1e-14)
        assert_array_equal(pdf.particle_weights, u[f"rs_{tag}_weights"])
    with np.errstate(all="ignore"):
        assert_array_equal(oracle.normalized_product(u["bu_w"], u["bu_lik"]), u["bu_out"])
        assert_array_equal(oracle.normalized_product(u["bu_w"], np.zeros_like(u["bu_w"])),
                           u["bu_zero_out"])
    assert not np.any(u["bu_zero_out"])
    assert np.isinf(oracle.effective_particles(u["bu_zero_out"]))


def test_full_sweep_matches_reference_limit():
    """weighted-variance sweep == reference with every particle drawn,
    at uniform weights."""
    f = _replay.load("full_sweep_uniform.npz")
    cases = [("lor", models.lorentzian, (f["fs_lor_x"],), (0.1,)),
             ("ml7", models.multi_lorentzian(7), (f["fs_lor_x"],), (0.1,)),
             ("coil", models.coil, (f["fs_coil_w"],), ()),
             ("rabi", models.rabi, (f["fs_rabi_s0"], f["fs_rabi_s1"]), (100000.0, 0.01, 2.0))]
    for tag, fn, sv, cons in cases:
        prior = f[f"fs_{tag}_prior"]
        n = prior.shape[1]
        yvar = oracle.yvar_full_sweep(fn, oracle.flatten_settings(sv), prior,
                                      np.full(n, 1.0 / n), cons, chunk=300)
        ref = f[f"fs_{tag}_yvar"]
        assert yvar.shape == ref.shape
        assert_allclose(yvar, ref, rtol=1e-11, atol=1e-13 * ref.max(), err_msg=tag)


def test_weighted_full_sweep_matches_the_reference_with_integer_multiplicities():
    """VERDICT r3 #3 / SURVEY 8(c): the weighted full sweep pinned to the REAL reference, exactly.  The
    fixture drove the reference with randdraw() returning particle i duplicated k_i times (k in 0..7), so
    its np.var over the sum(k) draws (obe_base.py:463-489) is the weighted variance with w = k / sum(k)."""
    f = _replay.load("full_sweep_integer_weights.npz")
    cases = [("lor", models.lorentzian, (f["iw_x48"],), (0.1,), 500.0 ** 2, None),
             ("lornarrow", models.lorentzian, (f["iw_x48"],), (0.1,), 500.0 ** 2, None),
             ("ml7", models.multi_lorentzian(7), (f["iw_x48"],), (0.1,), None, (9,)),
             ("coil", models.coil, (f["iw_coil_w"],), (), None, (3, 3)),
             ("rabi", models.rabi, (f["iw_rabi_s0"], f["iw_rabi_s1"]), (100000.0, 0.01, 2.0), 300.0 ** 2, None)]
    for tag, fn, sv, cons, noise_var, noise_rows in cases:
        prior, k = f[f"iw_{tag}_prior"], f[f"iw_{tag}_k"]
        assert k.min() == 0 and k.max() == 7
        w = k / k.sum()
        yvar = oracle.yvar_full_sweep(fn, oracle.flatten_settings(sv), prior, w, cons, chunk=300)
        ref = f[f"iw_{tag}_yvar"]
        assert yvar.shape == ref.shape
        assert_allclose(yvar, ref, rtol=ORACLE_RTOL * 10, atol=1e-13 * ref.max(), err_msg=tag)
        if noise_rows is not None:       # obe_noiseparam.py:122-136
            noise_var = np.array([np.average(prior[r] ** 2, weights=w) for r in noise_rows]).reshape(-1, 1)
        util = oracle.utility_from_yvar(yvar, noise_var, 1.0)
        assert_allclose(util, f[f"iw_{tag}_utility"], rtol=ORACLE_RTOL * 10, err_msg=tag)


def test_state_reset_replay_of_the_10_parameter_model():
    """every cycle of the 7-peak noise-parameter model from the reference's own
    state, at the oracle's tolerance (the free-running trajectory above stays as the drift test)."""
    fx = _replay.load("state_multilorentz7_noise.npz")
    obe = oracle.OracleOptBayesExptNoiseParameter(models.multi_lorentzian(7), (fx["setval_0"],), fx["prior"].copy(),
                                                  tuple(fx["cons"]), scale=False, noise_parameter_index=9)
    stats = _replay.replay_state_reset(fx, obe, ORACLE_RTOL, lambda o: o.last_draw_indices, lambda o: o.last_utility,
                                       lambda o: o.last_draw_indices)
    assert stats["resamples"] == int(np.sum(fx["resampled"])) >= 5
    assert int(np.max(fx["n_constrained"])) > 0          # the constraint mask is exercised


# ---- the reference's own unit-test expectations, restated against the oracle ----

def _toy_pdf():
    return oracle.OracleParticlePDF((np.array([0, 1, 2, 3]), np.array([1, 3, 2, 4])))


def test_reference_particlepdf_literals():
    """reference tests/test_particlepdf.py:17-152."""
    pdf = _toy_pdf()
    assert (pdf.n_dims, pdf.n_particles) == (2, 4)
    assert_array_equal(pdf.particle_weights, [.25, .25, .25, .25])
    assert pdf.just_resampled is False
    assert_array_equal(pdf.mean(), (1.5, 2.5))
    assert_allclose(pdf.covariance(), [[5 / 3, 4 / 3], [4 / 3, 5 / 3]])
    assert_array_equal(pdf.std(), np.sqrt(np.array([1, 1]) * 5.0 / 4.0))
    samples = np.arange(15).reshape((3, 5))
    pdf.set_pdf(samples)
    assert (pdf.n_dims, pdf.n_particles) == (3, 5)
    assert_array_equal(pdf.particle_weights, np.ones(5) / 5.0)
    pdf.set_pdf(samples, weights=np.array([1, 2, 3, 4, 5]))
    assert_array_equal(pdf.particle_weights, np.array([1, 2, 3, 4, 5]) / 15)
    with pytest.raises(ValueError):
        pdf.set_pdf(samples, weights=np.ones(4))
    pdf = _toy_pdf()
    pdf.tuning_parameters["auto_resample"] = False
    lik = np.array([.5, 1.5, 1.5, .5])
    pdf.bayesian_update(lik)
    assert_array_equal(pdf.particle_weights, lik / np.sum(lik))
    pdf = _toy_pdf()
    pdf.particle_weights = np.array([0, .5, .5, 0])
    pdf.resample()
    assert pdf.particles.shape == (2, 4)
    assert_array_equal(pdf.particle_weights, [.25, .25, .25, .25])
    pdf = _toy_pdf()
    pdf.particle_weights = np.array([.1, .4, .4, .1])
    pdf.resample_test()
    assert pdf.just_resampled is False
    pdf.particle_weights = np.array([0, .75, .25, 0])
    pdf.resample_test()
    assert pdf.just_resampled is True


def test_reference_optbayesexpt_literals():
    """reference tests/test_optbayesexpt.py:21-69."""
    pars = (np.array([0, 1, 2, 3]), np.array([1, 3, 2, 4]))
    obe = oracle.OracleOptBayesExpt(models.line_ab, (np.array([0, 1, 2]),), pars, ())
    assert_array_equal(obe.allsettings, (np.array([0, 1, 2]),))
    assert_array_equal(obe.parameters, pars)
    assert_array_equal(obe.eval_over_all_parameters((1,)), [[1, 4, 4, 7]])
    assert_array_equal(obe.eval_over_all_settings([1, 3]), [[1, 4, 7]])
    ymodel = np.array(((1, 4, 4, 7),))
    assert_array_equal(obe.likelihood(ymodel, ((1,), (5.0,), 1.0)),
                       np.exp(-(ymodel - 5.0) ** 2 / 2)[0])
    lkl = np.exp(-(np.array((1, 4, 4, 7)) - 5.0) ** 2 / 2)
    obe.pdf_update(((1,), 5.0, 1.0))
    assert_array_equal(obe.particle_weights, lkl / np.sum(lkl))


def test_reference_infer():
    """reference tests/test_zinference.py:89-108 (analytic posterior, 1e-15) and the
    reference's own output for it (fixture)."""
    u = _replay.load("unit_cases.npz")
    xs = u["infer_x"]
    n = len(xs)
    obe = oracle.OracleOptBayesExpt(models.first_parameter, (0,), (xs, np.ones(n)), (0,))
    obe.tuning_parameters["resample_threshold"] = 0
    obe.pdf_update(((), 1.0, 1.0))
    known = np.exp(-(1.0 - xs) ** 2 / 2) / np.sqrt(2 * np.pi)
    known /= np.sum(known)
    assert_allclose(obe.particle_weights, known, atol=1e-15, rtol=1e-15)
    assert_array_equal(obe.particle_weights, u["infer_w"])


def test_likelihood_two_channel_choke():
    u = _replay.load("unit_cases.npz")
    n = u["lk_ym"].shape[1]
    obe = oracle.OracleOptBayesExpt(models.coil, (np.logspace(4, 6, 5),),
                                    np.ones((4, n)), (), choke=0.6, n_channels=2)
    got = obe.likelihood(u["lk_ym"], ((1.0,), (0.3, -0.2), (1.5, 0.7)))
    assert_allclose(got, u["lk_out"], rtol=1e-15)


def test_c_restatement_agrees_with_numpy_oracle_and_reference():
    """oracle/csweep.c (plain C, OpenMP) against the NumPy oracle and, at uniform weights,
    against the real reference's full-sweep golden vector."""
    from oracle import csweep
    f = _replay.load("full_sweep_uniform.npz")
    g = np.random.default_rng(8)
    for tag, k, fn in (("lor", 1, models.lorentzian), ("ml7", 7, models.multi_lorentzian(7))):
        prior, x = f[f"fs_{tag}_prior"], f["fs_lor_x"]
        n = prior.shape[1]
        uni = np.full(n, 1.0 / n)
        assert_allclose(csweep.lorentz_yvar(x, prior, uni, 0.1, k), f[f"fs_{tag}_yvar"][0], rtol=1e-11)
        w = g.exponential(1.0, n)
        w /= w.sum()
        ref = oracle.yvar_full_sweep(fn, oracle.flatten_settings((x,)), prior, w, (0.1,))[0]
        assert_allclose(csweep.lorentz_yvar(x, prior, w, 0.1, k), ref, rtol=1e-11)
    prior = f["fs_lor_prior"]
    w = g.exponential(1.0, prior.shape[1])
    w /= w.sum()
    lik = oracle.gauss_likelihood(models.lorentzian((3.1,), prior, (0.1,)), 49200.0, 400.0)
    got, s2 = csweep.lorentz_update(3.1, 49200.0, 400.0, prior, w, 0.1)
    want = oracle.normalized_product(w, lik)
    assert_allclose(got, want, rtol=1e-12)
    assert_allclose(s2, np.sum(want * want), rtol=1e-12)
    assert csweep.threads() >= 1


def test_numpy_pairwise_sum_restatement_is_np_sum_bit_for_bit():
    """oracle.numpy_pairwise_sum (the order the device's strict_sums mode reproduces) against np.sum ITSELF — the
    reference's particlepdf.py:138, 243 call exactly that —: every length 0..5000 plus a few long ones, values of
    mixed magnitude and sign so that any other association shows in the last bits."""
    g = np.random.default_rng(2024)
    lengths = list(range(0, 1300)) + list(range(1300, 5001, 7)) + [8191, 8192, 8193, 16384, 16391, 65536 + 5, 70001]
    diff = 0
    for n in lengths:
        a = g.normal(size=n) * 10.0 ** g.integers(-8, 8, size=n)
        got, want = oracle.numpy_pairwise_sum(a), np.sum(a)
        assert got.tobytes() == np.float64(want).tobytes(), (n, got, want)
        diff += np.float64(np.sum(a[::-1])).tobytes() != np.float64(want).tobytes()
    assert diff > len(lengths) // 2          # (the inputs do tell summation orders apart)
    # the reference's own literal (tests/test_optbayesexpt.py:58-69): lkl / np.sum(lkl)
    lkl = np.exp(-(np.array((1, 4, 4, 7)) - 5.0) ** 2 / 2)
    assert oracle.numpy_pairwise_sum(0.25 * lkl).tobytes() == np.float64(np.sum(0.25 * lkl)).tobytes()


# ---- the y-space reductions: oracle.spacing_entropy and its one-line companions ----

ENTROPY_SIZES = list(range(5, 65)) + [99, 100, 101, 999, 1000, 1001, 1024, 2047, 2048, 5000]


def _entropy_columns(g, n):
    """Three columns of n samples: a wide and a narrow normal on an offset, and a heavy-tailed one."""
    return np.stack([g.normal(3.0, 10.0, n), g.normal(-812.5, 1e-4, n), g.standard_cauchy(n) * 1e3], axis=1)


def test_spacing_entropy_matches_scipy_at_every_estimator_and_switch():
    """oracle.spacing_entropy against scipy.stats.differential_entropy(axis=0) — the function the reference calls
    (obe_base.py:7-10) — for every sample size 5 ... 64 (van Es up to 10, Ebrahimi from 11, windows m = 2 ... 8) and
    around the switches and limits further up (99 ... 101, 999 | 1000 | 1001 Ebrahimi -> Vasicek, 1024, 2047, 2048,
    5000): three columns each plus one with ties (-inf on both sides) and one with a NaN (NaN on both sides).
    scipy is the LESS accurate side (float64 logs, np.mean): it is held to the tolerance that _replay states for a
    float64 evaluation against the oracle."""
    diffent = pytest.importorskip("scipy.stats").differential_entropy
    g = np.random.default_rng(1507)
    worst = 0.0
    for n in ENTROPY_SIZES:
        cols = _entropy_columns(g, n)
        tied = g.integers(0, 3, n).astype(np.float64)                  # {0, 1, 2}, and one window is all one value
        tied[:2 * int(np.floor(np.sqrt(n) + 0.5)) + 1] = 1.0
        holed = g.normal(size=n)
        holed[g.integers(n)] = np.nan
        y = np.concatenate([cols, tied[:, None], holed[:, None]], axis=1)
        h, scale = oracle.spacing_entropy(y, axis=0, with_log_scale=True)
        with np.errstate(all="ignore"):
            ref = diffent(y, axis=0)
        assert h.shape == ref.shape == (5,)
        assert np.all(np.isfinite(ref[:3])) and ref[3] == -np.inf and np.isnan(ref[4]), (n, ref)
        worst = max(worst, _replay.assert_entropy(ref, h, _replay.entropy_tolerance(n, h, scale), f"n = {n}"))
        # along another axis, and a (n, C, N_s)-shaped y-space
        assert_array_equal(oracle.spacing_entropy(y.T.copy(), axis=1), h)
        assert_array_equal(oracle.spacing_entropy(y.reshape(n, 5, 1), axis=0), h.reshape(5, 1))
    print(f"scipy against the oracle: worst error / tolerance {worst:.3f}")
    for n in (1, 2, 3, 4):                                              # scipy < 1.12 raises the same for these
        with pytest.raises(ValueError, match="Window length"):
            oracle.spacing_entropy(np.arange(float(n)))


def test_spacing_entropy_estimators_differ_where_they_switch():
    """The pins above can tell the estimators apart: at n = 10 | 11 and 1000 | 1001 evaluating the neighbouring
    estimator's formula instead moves H by far more than the tolerance."""
    diffent = pytest.importorskip("scipy.stats").differential_entropy
    g = np.random.default_rng(3)
    for n, other in ((10, "ebrahimi"), (11, "van es"), (1000, "vasicek"), (1001, "ebrahimi")):
        y = g.normal(size=(n, 4))
        h, scale = oracle.spacing_entropy(y, with_log_scale=True)
        assert np.all(np.abs(diffent(y, axis=0, method=other) - h) > 1e6 * _replay.entropy_tolerance(n, h, scale))


@pytest.mark.parametrize("n", [9, 30, 1001])
def test_spacing_entropy_matches_a_50_digit_evaluation(n):
    """One column per estimator (van Es n = 9, Ebrahimi n = 30, Vasicek n = 1001) against the same formula evaluated
    with mpmath at 50 digits from the sorted float64 samples.  What separates the two is the float64 rounding of the
    logarithms' ARGUMENTS — at most three roundings each (the spacing, the factor, their product or quotient), i.e.
    a relative error <= 2 eps of the argument = an absolute error <= 2 eps of each log term and of their mean — and
    the final rounding of H to float64: |H - H_50| <= eps (2 + |H|); x2 margin."""
    mp = pytest.importorskip("mpmath")
    g = np.random.default_rng(n)
    col = g.normal(40.0, 0.37, n)
    with mp.workdps(50):
        x = [mp.mpf(float(v)) for v in np.sort(col)]
        m = int(np.floor(np.sqrt(n) + 0.5))
        if n <= 10:
            h = sum(mp.log(mp.mpf(n + 1) / m * (x[i + m] - x[i])) for i in range(n - m)) / (n - m)
            h += sum(mp.mpf(1) / k for k in range(m, n + 1)) + mp.log(m) - mp.log(n + 1)
        else:
            h = mp.mpf(0)
            for i in range(1, n + 1):
                d = x[min(i - 1 + m, n - 1)] - x[max(i - 1 - m, 0)]
                if n <= 1000:
                    ci = 1 + mp.mpf(i - 1) / m if i <= m else 1 + mp.mpf(n - i) / m if i >= n - m + 1 else mp.mpf(2)
                    h += mp.log(n * d / (ci * m))
                else:
                    h += mp.log(mp.mpf(n) / (2 * m) * d)
            h /= n
        got = oracle.spacing_entropy(col)
        err = float(abs(mp.mpf(float(got)) - h))
    assert err <= 2 * _replay.EPS * (2 + abs(float(h))), (n, float(got), float(h), err)


def test_yspace_one_liners():
    """yspace_maxmin, yspace_variance, entropy_variance, kld_utility: the reference's expressions
    (obe_base.py:487, 516-517, 531-534, 720) on a (N_d, C, N_s) array."""
    g = np.random.default_rng(12)
    y = g.normal(5.0, 2.0, (7, 2, 9))
    assert_array_equal(oracle.yspace_maxmin(y), (y.max(axis=0) - y.min(axis=0)) ** 2)
    assert_array_equal(oracle.yspace_maxmin(y[:1]), np.zeros((2, 9)))
    assert_array_equal(oracle.yspace_variance(y), np.var(y, axis=0))
    assert_allclose(oracle.yspace_variance(y), np.mean((y - y.mean(axis=0)) ** 2, axis=0), rtol=1e-14)
    h = g.normal(size=(2, 9))
    assert_array_equal(oracle.entropy_variance(h), np.exp(2 * h) / (2 * np.pi * np.e))
    assert oracle.entropy_variance(-np.inf) == 0.0
    assert_allclose(oracle.entropy_variance(0.5 * np.log(2 * np.pi * np.e * 4.0)), 4.0, rtol=1e-15)   # N(., 2^2)
    hn = np.array([0.3, -1.1])
    assert_array_equal(oracle.kld_utility(h, hn), np.exp(h - hn[:, None]) - 1.0)
    assert_array_equal(oracle.kld_utility(np.full((2, 1), -np.inf), hn), [[-1.0], [-1.0]])
