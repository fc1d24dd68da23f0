"""Host oracle of the own-noise classes' batch assimilation (obe_signal_noise_records_loglik,
obe_binomial_records_loglik, obe_poisson_records_loglik; records_loglik() / pdf_update_batch() of
OptBayesExptSignalNoise, OptBayesExptBinomial and OptBayesExptPoisson), from rows of model values.

``f`` (R, C, N_p): the model at each record's setting for every particle; the records' data (C, R).  Every function
returns ``(l (N_p,) long double, B (N_p,) float64)``: the full log density of the records per particle, constants
included, and the conditioning sum B_i of the absolute values of its terms (as ``_batch_oracle.loglik`` has it).  The
rules of include/obe_hip.h: NaN where a model value is one the class does not take, at any record and channel; -inf
where a record is impossible for the particle.  Everything is long double but ``lgamma``, which is ``math.lgamma``.
The tempered algorithm is ``_batch_oracle``'s, restated over a function that gives l for the present cloud.
"""
import math
import warnings

import numpy as np

import _batch_oracle as bo

LD = np.longdouble
HALF_LOG_2PI = np.log(LD(2.0) * LD(np.pi)) / 2


def _rows(a, n_c, n_r):
    """(R, C, 1) long double of a record table given as (C, R), a scalar or (C,)."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim < 2:
        a = np.broadcast_to(a.reshape(-1, 1), (n_c, n_r))
    return a.reshape(n_c, n_r).T[:, :, None].astype(LD)


def _lgamma1(a):
    return np.vectorize(lambda v: math.lgamma(v + 1.0), otypes=[np.float64])(np.asarray(a, dtype=np.float64)).astype(LD)


def _finish(terms, cond, constant, dead):
    with np.errstate(all="ignore"):
        l = terms.sum(axis=(0, 1)) + constant
        b = cond.sum(axis=(0, 1)) + abs(constant)
    l = np.where(dead, LD(np.nan), l)
    return l, np.where(dead | ~np.isfinite(b), 1.0, b).astype(np.float64)


def signal_noise(f, y_meas, coef):
    """l_i = sum_r sum_c [-(f - y)^2 / (2 nu) - log(nu) / 2] - R C log(2 pi) / 2, nu = a_c + b_c |f| + c_c f^2 with
    ``coef`` (C, 3); NaN where a nu is not > 0 or not finite."""
    f = np.asarray(f, dtype=np.float64)
    n_r, n_c, _ = f.shape
    coef = np.asarray(coef, dtype=np.float64).astype(LD)
    a, b, c = (coef[:, k].reshape(1, n_c, 1) for k in range(3))
    y = _rows(y_meas, n_c, n_r)
    with np.errstate(all="ignore"):
        fl = f.astype(LD)
        nu = a + b * np.abs(fl) + c * (fl * fl)
        dead = ~np.all((nu > 0) & np.isfinite(nu), axis=(0, 1))
        quad, logs = (fl - y) ** 2 / (2 * nu), np.log(nu) / 2
        return _finish(-(quad + logs), np.abs(quad) + np.abs(logs), -n_r * n_c * HALF_LOG_2PI, dead)


def binomial(p, successes, shots):
    """l_i = sum_r sum_c [k log p + (n - k) log1p(-p) + log C(n, k)], a term whose count is 0 skipped; NaN where a p is
    NaN or outside [0, 1]; -inf where p = 0 meets k > 0 or p = 1 meets n - k > 0."""
    p = np.asarray(p, dtype=np.float64)
    n_r, n_c, _ = p.shape
    k, n = _rows(successes, n_c, n_r), _rows(shots, n_c, n_r)
    constant = (_lgamma1(n) - _lgamma1(k) - _lgamma1(n - k)).sum()
    with np.errstate(all="ignore"):
        dead = ~np.all((p >= 0) & (p <= 1), axis=(0, 1))
        pl = p.astype(LD)
        t1 = np.where(k > 0, k * np.log(pl), LD(0.0))
        t2 = np.where(n - k > 0, (n - k) * np.log1p(-pl), LD(0.0))
        return _finish(t1 + t2, np.abs(t1) + np.abs(t2), constant, dead)


def poisson(r, counts, exposure):
    """l_i = sum_r sum_c [k log lambda - lambda - log k!], lambda = t r, a channel with k = 0 contributing -lambda
    alone; NaN where an r is not a rate (NaN, negative, +inf, t r overflows); -inf where lambda = 0 meets k > 0."""
    r = np.asarray(r, dtype=np.float64)
    n_r, n_c, _ = r.shape
    k, t = _rows(counts, n_c, n_r), _rows(exposure, n_c, n_r)
    constant = -_lgamma1(k).sum()
    with np.errstate(all="ignore"):
        dead = ~np.all((r >= 0) & (r * t.astype(np.float64) < np.inf), axis=(0, 1))
        lam = t * r.astype(LD)
        t1 = np.where(k > 0, k * np.log(lam), LD(0.0))
        return _finish(t1 - lam, np.abs(t1) + np.abs(lam), constant, dead)


# ------------------------------------------------------------------------------------------------ the tempered update
def tempered_update(obe, loglik_of, max_stages=64):
    """``_batch_oracle.tempered_update`` over ``loglik_of(obe)``, l (N_p,) of the present cloud of an
    ``oracle.OracleOptBayesExpt`` (no choke): the stage search, the stage's weights and evidence, the resample and the
    constraints between stages, the resample test at the end.  Returns the report dict of pdf_update_batch."""
    thr = obe.tuning_parameters["resample_threshold"]
    report = dict(stages=[], n_eff=[], resamples=0, log_evidence=0.0, beta=[])
    beta = 0.0
    while True:
        l = loglik_of(obe)
        w = np.asarray(obe.particle_weights, dtype=np.float64)
        delta_max = 1.0 - beta
        if len(report["stages"]) + 1 >= max_stages:
            k = 1 << bo.SEARCH_BITS
        else:
            k, _ = bo.search_stage(lambda d: bo.ess_fraction(l, w, d), delta_max, thr)
        last = k == 1 << bo.SEARCH_BITS
        delta = delta_max if last else bo.trial_delta(delta_max, k)
        report["log_evidence"] += bo.stage_log_evidence(l, w, delta)
        obe.particle_weights = bo.stage_weights(l, w, delta)
        report["stages"].append(delta)
        report["n_eff"].append(float(1.0 / np.sum(obe.particle_weights ** 2)))
        beta = 1.0 if last else beta + delta
        report["beta"].append(beta)
        if last:
            break
        obe.resample()
        obe.just_resampled = True
        report["resamples"] += 1
        obe.parameters = obe.particles
        obe.enforce_parameter_constraints()
    if obe.tuning_parameters["auto_resample"]:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            obe.resample_test()
        report["resamples"] += int(obe.just_resampled)
    obe.parameters = obe.particles
    if obe.just_resampled:
        obe.enforce_parameter_constraints()
    return report


# ------------------------------------------------------------------------------------------------ the conjugate cases
N_CONJUGATE, R_CONJUGATE = 20000, 200
RESAMPLING_SEED = 77            # the generator both the restatement and the device run resample from
#: What the restatement reaches at these seeds (tests/test_own_records_host.py measures and asserts it; rounded up in
#: the last digit kept): |mean - exact| / sd, |std / sd - 1| and |log_evidence - exact|.  The device run
#: (tests/test_gpu_own_records.py) is held to twice these.
#: measured: 0.00790, 0.00658, 0.02294 (3 stages)
POISSON_REACHED = dict(mean=0.0080, std=0.0066, evidence=0.023)
#: measured: 0.00795, 0.00716, 0.01156 (3 stages)
BINOMIAL_REACHED = dict(mean=0.0080, std=0.0072, evidence=0.012)


def poisson_conjugate_case():
    """A constant rate under a Gamma prior: ``(prior (1, N), x (R,), k (R,), t (R,), post_mean, post_sd,
    log_evidence)``.  rate ~ Gamma(shape 6, rate 1.5); k_r ~ Poisson(t_r 3.2), t_r ~ U(0.5, 2).  The posterior is
    Gamma(6 + K, 1.5 + T); the evidence prod_r [t^k / k!] 1.5^6 / Gamma(6) Gamma(6 + K) / (1.5 + T)^(6 + K).  Shared
    with the GPU test: same seeds, same data."""
    g = np.random.default_rng(20260301)
    shape, rate = 6.0, 1.5
    prior = g.gamma(shape, 1.0 / rate, (1, N_CONJUGATE))
    x = np.linspace(0.0, 1.0, R_CONJUGATE)                     # (the model ignores the setting)
    t = g.uniform(0.5, 2.0, R_CONJUGATE)
    k = g.poisson(3.2 * t).astype(np.float64)
    K, T = k.sum(), t.sum()
    evidence = (math.fsum(k * np.log(t)) - math.fsum(math.lgamma(v + 1.0) for v in k) + shape * math.log(rate)
                - math.lgamma(shape) + math.lgamma(shape + K) - (shape + K) * math.log(rate + T))
    return prior, x, k, t, (shape + K) / (rate + T), math.sqrt(shape + K) / (rate + T), evidence


def binomial_conjugate_case():
    """A constant probability under a Beta prior: ``(prior (1, N), x (R,), k (R,), n (R,), post_mean, post_sd,
    log_evidence)``.  p ~ Beta(8, 12); k_r ~ Binomial(n_r, 0.43), n_r in 1..20.  The posterior is Beta(8 + K, 12 + F);
    the evidence prod_r C(n, k) B(8 + K, 12 + F) / B(8, 12).  Shared with the GPU test: same seeds, same data."""
    g = np.random.default_rng(20260302)
    a0, b0 = 8.0, 12.0
    prior = g.beta(a0, b0, (1, N_CONJUGATE))
    x = np.linspace(0.0, 1.0, R_CONJUGATE)
    n = g.integers(1, 21, R_CONJUGATE).astype(np.float64)
    k = g.binomial(n.astype(np.int64), 0.43).astype(np.float64)
    K, F = k.sum(), (n - k).sum()

    def log_beta(a, b):
        return math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)
    a1, b1 = a0 + K, b0 + F
    log_choose = math.fsum(math.lgamma(nn + 1.0) - math.lgamma(kk + 1.0) - math.lgamma(nn - kk + 1.0)
                           for kk, nn in zip(k, n))
    evidence = log_choose + log_beta(a1, b1) - log_beta(a0, b0)
    sd = math.sqrt(a1 * b1 / ((a1 + b1) ** 2 * (a1 + b1 + 1.0)))
    return prior, x, k, n, a1 / (a1 + b1), sd, evidence
