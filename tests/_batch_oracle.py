"""Host oracle of the batch update (obe_records_loglik, obe_tempered_sums, pdf_update_batch), from rows of model values.

``y`` (R, C, N_p): the model at each record's setting for every particle; ``y_meas`` (C, R); ``sigma`` (C, R) for a
known noise or (C, N_p) for a row per particle (``per_particle=True``).  z = (y - y_meas) / sigma.  The rules of
include/obe_hip.h: l_i is NaN where the particle contributes nothing — a noise row that is not > 0, a model output
that is not finite, and for every particle a record sigma that is not > 0 —; the tempered sums count NaN and negative
weights as zero and skip a particle whose l is not finite.  Everything is long double; sums are sorted first.
"""
import warnings

import numpy as np

LD = np.longdouble
LOG_2PI = np.log(LD(2.0) * LD(np.pi))
SEARCH_BITS = 32


def loglik(y, y_meas, sigma, per_particle=False):
    """``(l (N_p,) long double, B (N_p,) float64)``: l_i = sum_r sum_c [-z^2 / 2 - log sigma] - R (C / 2) log 2 pi and
    the conditioning sum B_i of the absolute values of those terms."""
    y = np.asarray(y, dtype=np.float64)
    n_r, n_c, n_p = y.shape
    ym = np.asarray(y_meas, dtype=np.float64).reshape(n_c, n_r)
    sg = np.asarray(sigma, dtype=np.float64)
    sg = sg.reshape(n_c, n_p)[None, :, :] if per_particle else sg.reshape(n_c, n_r).T[:, :, None]
    sg = np.broadcast_to(sg, y.shape)
    with np.errstate(all="ignore"):
        z = (y.astype(LD) - ym.T.astype(LD)[:, :, None]) / sg.astype(LD)
        quad, logs = (z * z) / 2, np.log(sg.astype(LD))
        const = n_r * n_c * LOG_2PI / 2
        l = -(quad + logs).sum(axis=(0, 1)) - const
        cond = (np.abs(quad) + np.abs(logs)).sum(axis=(0, 1)) + const
        dead = ~np.all(np.isfinite(y), axis=(0, 1)) | ~np.all(sg > 0.0, axis=(0, 1))
    l = np.where(dead, LD(np.nan), l)
    return l, np.where(dead, 1.0, cond).astype(np.float64)


def loglik_tolerance(cond):
    """|d l_i| <= 1e-10 max(1, B_i)."""
    return 1e-10 * np.maximum(1.0, cond)


def clean(w):
    w = np.asarray(w, dtype=np.float64)
    return np.where(w > 0.0, w, 0.0)


def _sum(a):
    return np.sort(np.asarray(a, dtype=LD)).sum() if len(a) else LD(0.0)


def tempered_sums(l, w, exponents):
    """``(m, sum w, [(S1, S2), ...])`` in long double."""
    l, w = np.asarray(l, dtype=LD), clean(w)
    live = w > 0.0
    use = live & np.isfinite(l)
    top = l[use].max() if use.any() else LD(-np.inf)
    out = []
    for a in exponents:
        with np.errstate(under="ignore"):
            t = w[use].astype(LD) * np.exp(LD(a) * (l[use] - top))
        out.append((_sum(t), _sum(t * t)))
    return top, _sum(w[live]), out


def ess_fraction(l, w, a):
    """N_eff / N of the weights w exp(a l) / sum, long double."""
    (s1, s2), = tempered_sums(l, w, [a])[2]
    return float(s1 * s1 / s2) / len(w) if s2 > 0 else 0.0


def stage_weights(l, w, a):
    """normalised w exp(a (l - m)), 0 where l is not finite (float64)."""
    l, w = np.asarray(l, dtype=LD), np.asarray(w, dtype=np.float64)
    top, _, ((s1, _),) = tempered_sums(l, w, [a])
    with np.errstate(all="ignore"):
        t = np.where(np.isfinite(l), clean(w).astype(LD) * np.exp(LD(a) * (l - top)), LD(0.0))
    return (t / s1).astype(np.float64)


def stage_log_evidence(l, w, delta):
    top, sw, ((s1, _),) = tempered_sums(l, w, [delta])
    return float(np.log(s1 / sw) + LD(delta) * top)


def trial_delta(delta_max, k):
    return delta_max * (k / float(1 << SEARCH_BITS))


def search_stage(ess_of, delta_max, threshold):
    """The largest k in 1 .. 2^32 with ess_of(delta_max k 2^-32) >= threshold by plain binary bisection (one trial per
    step: the device takes the same 32 halvings 16 trials at a time), or (2^32, True) if the whole remainder
    passes, or (1, False) if nothing does."""
    top = 1 << SEARCH_BITS
    if ess_of(delta_max) >= threshold:
        return top, True
    lo, hi = 0, top                                # lo passes (or is 0), hi fails
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ess_of(trial_delta(delta_max, mid)) >= threshold:
            lo = mid
        else:
            hi = mid
    return (lo, True) if lo > 0 else (1, False)


def tempered_update(obe, rows_of, y_meas, sigma, per_particle=False, max_stages=64, on_stage=None):
    """The whole tempered algorithm over an ``oracle.OracleOptBayesExpt``: ``rows_of(obe)`` returns y (R, C, N_p) of
    its present cloud (``sigma`` a callable of obe when per_particle).  Returns the report dict of pdf_update_batch."""
    kappa = 1.0 if obe.choke is None else float(obe.choke)
    thr = obe.tuning_parameters["resample_threshold"]
    report = dict(stages=[], n_eff=[], resamples=0, log_evidence=None if obe.choke is not None else 0.0, beta=[])
    beta = 0.0
    while True:
        sg = sigma(obe) if callable(sigma) else sigma
        l, _ = loglik(rows_of(obe), y_meas, sg, per_particle)
        w = np.asarray(obe.particle_weights, dtype=np.float64)
        delta_max = 1.0 - beta
        if len(report["stages"]) + 1 >= max_stages:
            k = 1 << SEARCH_BITS
            if ess_fraction(l, w, kappa * delta_max) < thr:
                warnings.warn("max_stages", RuntimeWarning)
        else:
            k, _ = search_stage(lambda d: ess_fraction(l, w, kappa * d), delta_max, thr)
        last = k == 1 << SEARCH_BITS
        delta = delta_max if last else trial_delta(delta_max, k)
        if report["log_evidence"] is not None:
            report["log_evidence"] += stage_log_evidence(l, w, delta)
        obe.particle_weights = stage_weights(l, w, kappa * delta)
        report["stages"].append(delta)
        report["n_eff"].append(float(1.0 / np.sum(obe.particle_weights ** 2)))
        beta = 1.0 if last else beta + delta
        report["beta"].append(beta)
        if on_stage is not None:
            on_stage(dict(stage=len(report["stages"]) - 1, delta=delta, beta=beta, n_eff=report["n_eff"][-1]))
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


def conjugate_case():
    """``(prior (2, N), x, y, sigma, post_mean, post_cov)``: y = a + b x + noise, a Gaussian prior on (a, b); the
    closed-form posterior.  Shared with the GPU test: same seeds, same data."""
    g = np.random.default_rng(20250101)
    n_p, n_r, sigma = 20000, 200, 0.5
    m0, s0 = np.array([1.0, -2.0]), np.array([2.0, 1.5])
    prior = m0[:, None] + s0[:, None] * g.standard_normal((2, n_p))
    x = g.uniform(-1.0, 3.0, n_r)
    y = 1.7 - 2.6 * x + sigma * g.standard_normal(n_r)
    a = np.stack([np.ones(n_r), x], axis=1)
    prec = np.diag(1.0 / s0 ** 2) + a.T @ a / sigma ** 2
    cov = np.linalg.inv(prec)
    mean = cov @ (m0 / s0 ** 2 + a.T @ y / sigma ** 2)
    return prior, x, y, sigma, mean, cov
