"""Assimilating a recorded data set, the part that needs no device: the argument checks and refusals raise before any
library call, the stage search is checked against an ESS function in closed form, the oracle the GPU tests compare
with (tests/_batch_oracle.py) is pinned against the oracle classes' own sequential updates, and the whole tempered
algorithm is run on the conjugate (linear-Gaussian) case against the closed-form posterior."""
import math
import types
import warnings

import numpy as np
import pytest

import _batch_oracle as bo
import oracle
from _replay import close_weights
from optbayesexpt_amd import _batch, _lib
from oracle import models as omodels

NAMES = ("obe_records_loglik_workspace_bytes", "obe_records_loglik", "obe_tempered_sums", "obe_tempered_likelihood")


# ------------------------------------------------------------------------------------- argument checks, refusals
def test_entry_points_are_declared_and_the_audit_knows_the_sync_one():
    from optbayesexpt_amd import _audit
    assert set(NAMES) <= set(_lib.PROTOTYPES)
    assert {"obe_records_loglik_workspace_bytes", "obe_records_loglik"} <= set(_lib.MODEL_ENTRY_POINTS)
    assert not {"obe_tempered_sums", "obe_tempered_likelihood"} & set(_lib.MODEL_ENTRY_POINTS)
    names = [n for _, n in _lib.PROTOTYPES["obe_tempered_sums"][1]]
    rule, *reads = _audit._BATCH_RULES["obe_tempered_sums"]
    assert set(reads) <= set(names)
    # the rule delivers 2 + 2 n_trials words of h_sums and arms nothing
    zone = np.zeros(64)
    a = _audit._Audit()
    a.zone_created(zone.ctypes.data, zone.nbytes, None)
    a.zones[zone.ctypes.data].armed[:] = True
    args = [None] * len(names)
    args[names.index("n_trials")], args[names.index("h_sums")] = 3, zone.ctypes.data + 8 * 4
    a.after_call("obe_tempered_sums", tuple(args))
    assert np.flatnonzero(~a.zones[zone.ctypes.data].armed).tolist() == list(range(4, 12))
    assert _batch.TRIALS_PER_PASS == 16 and _batch.TEMPERED_WS_BYTES >= 8 * (2 + 256) * 34


def test_batch_arguments_are_checked_on_the_host():
    assert _batch.check_batch_arguments(True, 64, None) == (True, 64)
    assert _batch.check_batch_arguments(np.bool_(False), np.int64(1), print) == (False, 1)
    for bad in (1, "yes", None):
        with pytest.raises(TypeError):
            _batch.check_batch_arguments(bad, 64, None)
    for bad in (1.5, "3", None, True):
        with pytest.raises(TypeError):
            _batch.check_batch_arguments(True, bad, None)
    with pytest.raises(ValueError):
        _batch.check_batch_arguments(True, 0, None)
    with pytest.raises(TypeError):
        _batch.check_batch_arguments(True, 4, "not callable")
    assert _batch.check_choke(None) == 1.0 and _batch.check_choke(0.5) == 0.5
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _batch.check_choke(bad)


def test_host_models_and_likelihood_hooks_are_refused_by_name():
    host = types.SimpleNamespace(_device_model=None, _likelihood_overridden=lambda: False)
    with pytest.raises(TypeError, match="from_function.*from_expression"):
        _batch.refuse_host_model(host)
    with pytest.raises(TypeError, match="from_function.*from_expression"):
        _batch.records_loglik(host, (1.0,), 2.0, 1.0)
    with pytest.raises(TypeError, match="from_function.*from_expression"):
        _batch.pdf_update_batch(host, (1.0,), 2.0, 1.0)
    hooked = types.SimpleNamespace(_device_model=object(), _likelihood_overridden=lambda: True)
    with pytest.raises(TypeError, match="likelihood"):
        _batch.refuse_host_model(hooked)


def test_records_are_checked_as_the_scoring_methods_check_them():
    from optbayesexpt_amd._scoring import check_records
    x, y, s, _ = check_records((np.arange(5.0),), np.arange(5.0), 2.0, 1, 1, None)
    assert x.shape == y.shape == s.shape == (1, 5)
    with pytest.raises(ValueError, match="sigma is required"):
        check_records((np.arange(5.0),), np.arange(5.0), None, 1, 1, None)
    with pytest.raises(ValueError, match="call without sigma"):         # OptBayesExptNoiseParameter refuses a sigma
        check_records((np.arange(5.0),), np.arange(5.0), 1.0, 1, 1, np.array([2], dtype=np.int32))
    fake = types.SimpleNamespace(_device_model=object(), _likelihood_overridden=lambda: False, choke=None,
                                 _noise_rows=np.array([2], dtype=np.int32), n_channels=1, allsettings=np.zeros((1, 3)))
    with pytest.raises(ValueError, match="call without sigma"):
        _batch.pdf_update_batch(fake, (np.arange(5.0),), np.arange(5.0), sigma=1.0)
    with pytest.raises(ValueError, match="call without sigma"):
        _batch.records_loglik(fake, (np.arange(5.0),), np.arange(5.0), sigma=1.0)


# -------------------------------------------------------------------------------------------- the stage search
def _counted(f):
    calls = []

    def fractions(deltas):
        calls.append(len(deltas))
        return [f(d) for d in deltas]
    return fractions, calls


@pytest.mark.parametrize("c", [3.0, 1e3, 7.7e7, 1e9])
@pytest.mark.parametrize("delta_max", [1.0, 0.37, 2.0 ** -20])
def test_stage_search_keeps_a_passing_delta_whose_next_grid_point_fails(c, delta_max):
    """N_eff / N = 1 / (1 + (c delta)^2) in closed form: the delta kept passes, the next grid point fails, eight passes
    of at most 16 trials each."""
    f = lambda d: 1.0 / (1.0 + (c * d) ** 2)          # noqa: E731
    thr = 0.5
    fractions, calls = _counted(f)
    k, passed = _batch.search_stage(fractions, delta_max, thr)
    if c * delta_max <= 1.0:
        assert (k, passed) == (1 << 32, True) and calls == [16]
        return
    assert passed and 1 <= k < 1 << 32
    assert f(_batch.trial_delta(delta_max, k)) >= thr > f(_batch.trial_delta(delta_max, k + 1))
    assert abs(_batch.trial_delta(delta_max, k) - 1.0 / c) <= delta_max * 2.0 ** -32 * (1 + 1e-9)
    assert len(calls) == 8 and max(calls) <= 16
    # the oracle's plain binary bisection finds the same grid point
    assert bo.search_stage(f, delta_max, thr) == (k, True)
    assert bo.trial_delta(delta_max, k) == _batch.trial_delta(delta_max, k)


def test_stage_search_takes_the_smallest_step_when_nothing_passes():
    fractions, calls = _counted(lambda d: 0.1)
    assert _batch.search_stage(fractions, 1.0, 0.5) == (1, False)
    assert len(calls) == 8
    assert bo.search_stage(lambda d: 0.1, 1.0, 0.5) == (1, False)


def test_stages_end_at_beta_exactly_one():
    """The host loop of pdf_update_batch on a closed-form ESS that allows a step of ~0.13 per stage: beta rises
    strictly and the last stage, the whole remainder, leaves it at exactly 1.0."""
    f = lambda d: 1.0 / (1.0 + (7.7 * d) ** 2)        # noqa: E731
    beta, betas = 0.0, []
    while True:
        k, passed = _batch.search_stage(lambda ds: [f(d) for d in ds], 1.0 - beta, 0.5)
        assert passed
        if k == 1 << 32:
            beta = 1.0
            betas.append(beta)
            break
        beta += _batch.trial_delta(1.0 - beta, k)
        betas.append(beta)
    assert betas[-1] == 1.0 and len(betas) == 8 and np.all(np.diff([0.0] + betas) > 0.0)
    assert _batch.ess_fraction(3.0, 4.5, 2) == 1.0 and _batch.ess_fraction(0.0, 0.0, 5) == 0.0


# -------------------------------------------------------------------------------------------- the oracle, pinned
def _lorentz_case(n_p, n_r, seed, sigma=300.0):
    g = np.random.default_rng(seed)
    prior = np.array([g.uniform(2, 4, n_p), g.uniform(-2000, -400, n_p), g.normal(50000, 1000, n_p)])
    x = g.uniform(1.5, 4.5, n_r)
    y = np.array([float(omodels.lorentzian((xi,), (3.0, -1000.0, 50000.0), (0.1,))) for xi in x]) + g.normal(0, sigma, n_r)
    return prior, x, y


def _rows(model, x, particles, cons):
    return np.array([np.atleast_2d(model((np.asarray(xi),) if np.ndim(xi) == 0 else tuple(xi), particles, cons)) for xi in x])


@pytest.mark.parametrize("n_r", [1, 3, 8])
def test_oracle_loglik_is_the_product_of_gauss_likelihoods(n_r):
    prior, x, y = _lorentz_case(200, n_r, [1, n_r], sigma=800.0)
    sig = np.random.default_rng(5).uniform(600.0, 1500.0, n_r)
    rows = _rows(omodels.lorentzian, x, prior, (0.1,))
    l, cond = bo.loglik(rows, y[None, :], sig[None, :])
    prod = np.ones(200)
    for r in range(n_r):
        prod = prod * oracle.gauss_likelihood(rows[r, 0], y[r], sig[r])
    want = prod * (2 * np.pi) ** (-n_r / 2)
    got = np.exp(l).astype(np.float64)
    assert np.all(want > 1e-250)
    assert np.max(np.abs(got - want) / want) <= 1e-13
    assert np.all(cond >= np.abs(l).astype(np.float64) * (1 - 1e-12))


def test_oracle_marks_what_contributes_nothing():
    rows = np.random.default_rng(2).normal(0, 1, (4, 2, 6))
    rows[1, 0, 2], rows[3, 1, 4] = np.nan, -np.inf
    sig = np.full((2, 6), 1.5)
    sig[0, 0], sig[1, 1] = 0.0, np.nan
    l, _ = bo.loglik(rows, np.zeros((2, 4)), sig, per_particle=True)
    assert np.isnan(l.astype(np.float64)).tolist() == [True, True, True, False, True, False]
    known = np.full((2, 4), 1.5)
    known[1, 2] = -1.0
    assert np.all(np.isnan(bo.loglik(rows, np.zeros((2, 4)), known)[0].astype(np.float64)))
    # the tempered sums skip them, and particles of zero, NaN or negative weight
    w = np.array([0.2, 0.1, 0.3, 0.1, np.nan, -1.0])
    top, sw, ((s1, s2),) = bo.tempered_sums(l, w, [0.5])
    assert float(top) == float(l[3]) and abs(float(sw) - 0.7) < 1e-15
    assert abs(float(s1) - 0.1) < 1e-15 and abs(float(s2) - 0.01) < 1e-15


@pytest.mark.parametrize("choke", [None, 0.5])
def test_oracle_one_stage_is_the_sequential_updates(choke):
    """One stage against R sequential OracleOptBayesExpt.pdf_update() calls with auto_resample=False: the weights,
    and the log evidence against the chain sum_r log sum_i w_i L_ri - R (C / 2) log 2 pi."""
    n_p, n_r, sig = 500, 12, 900.0
    prior, x, y = _lorentz_case(n_p, n_r, 11, sigma=sig)
    sv = (np.linspace(1.5, 4.5, 50),)
    seq = oracle.OracleOptBayesExpt(omodels.lorentzian, sv, prior.copy(), (0.1,), auto_resample=False, choke=choke)
    chain = 0.0
    for r in range(n_r):
        rec = ((x[r],), y[r], sig)
        lik = seq.likelihood(seq.eval_over_all_parameters(rec[0]), rec)
        chain += math.log(np.sum(np.nan_to_num(seq.particle_weights * lik)))
        seq.pdf_update(rec)
    assert np.min(seq.particle_weights) > 1e-280
    rows = _rows(omodels.lorentzian, x, prior, (0.1,))
    l, _ = bo.loglik(rows, y[None, :], np.full((1, n_r), sig))
    w0 = np.full(n_p, 1.0 / n_p)
    kappa = 1.0 if choke is None else choke
    close_weights(bo.stage_weights(l, w0, kappa), seq.particle_weights, 1e-12, "one stage")
    if choke is None:
        want = chain - n_r * 0.5 * math.log(2 * math.pi)
        assert abs(bo.stage_log_evidence(l, w0, 1.0) - want) <= 1e-12 * abs(want)


# ------------------------------------------------------------------------- the conjugate case (linear, Gaussian)
def test_oracle_tempered_update_reaches_the_conjugate_posterior():
    prior, x, y, sigma, mean, cov = bo.conjugate_case()
    sd = np.sqrt(np.diag(cov))
    obe = oracle.OracleOptBayesExpt(omodels.line_ab, (np.linspace(-1, 3, 11),), prior.copy(), ())
    obe.rng = np.random.default_rng(77)
    one = bo.ess_fraction(bo.loglik(_rows(omodels.line_ab, x, prior, ()), y[None, :], np.full((1, len(x)), sigma))[0],
                          obe.particle_weights, 1.0)
    assert one * obe.n_particles < 50.0                       # (one stage would leave a handful of particles)
    betas = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        report = bo.tempered_update(obe, lambda o: _rows(omodels.line_ab, x, o.particles, ()), y[None, :],
                                    np.full((1, len(x)), sigma), on_stage=lambda info: betas.append(info["beta"]))
    assert len(report["stages"]) >= 3 and betas[-1] == 1.0 and np.all(np.diff(betas) > 0)
    thr = obe.tuning_parameters["resample_threshold"]
    assert all(f >= thr * obe.n_particles * (1 - 1e-9) for f in report["n_eff"][:-1])
    # half of the margins the GPU test holds the product to: 0.2 sd on the mean, 20 % on each std
    assert np.all(np.abs(obe.mean() - mean) <= 0.1 * sd), (obe.mean(), mean, sd)
    assert np.all(np.abs(obe.std() / sd - 1.0) <= 0.1), (obe.std(), sd)
    # the evidence of the whole data set, against the closed form of the linear-Gaussian model
    a = np.stack([np.ones(len(x)), x], axis=1)
    s = sigma ** 2 * np.eye(len(x)) + a @ np.diag([4.0, 2.25]) @ a.T
    r = y - a @ np.array([1.0, -2.0])
    exact = -0.5 * (r @ np.linalg.solve(s, r) + np.linalg.slogdet(s)[1] + len(x) * math.log(2 * math.pi))
    assert abs(report["log_evidence"] - exact) <= 0.5, (report["log_evidence"], exact)
