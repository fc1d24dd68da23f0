"""Plain NumPy oracle of the counted-event statistics (OptBayesExptPoisson; csrc/obe_poisson.hip), written from the
formulae of include/obe_hip.h, and the inputs the GPU tests run on (built and checked without a device).

Deliberately NOT the kernel's recurrence: every ``p_k = exp(k log lambda - lambda - lgamma(k + 1))`` is formed directly,
with ``math.lgamma``.  Rates come from the caller: ``r`` is ``(C, N_p)`` for one setting, ``R`` is ``(n_settings, N_p)``
for the one-channel design and ``(n_settings, C, N_p)`` for the noise variance.  ``dtype=np.longdouble`` evaluates the
same formulae in extended precision (the inputs stay the float64 values).
"""
import math

import numpy as np

# ------------------------------------------------------------------------------------------------ the statistics


def clean_weights(w):
    """NaN and negative weights count as zero."""
    w = np.asarray(w, dtype=np.float64)
    return np.where(w > 0, w, 0.0)


def is_rate(r, exposure=1.0):
    """Finite and >= 0, and so is exposure x rate (NaN fails)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (r >= 0) & (r * exposure < np.inf)


def xlogx(p):
    """p log p with 0 log 0 = 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p > 0, p * np.log(np.where(p > 0, p, 1)), 0 * p)


def log_pmf(k, lam):
    """``k log lambda - lambda - log k!`` elementwise over ``lam``; with k = 0 it is ``-lambda`` alone, no log."""
    lam = np.asarray(lam)
    if k == 0:
        return -lam
    with np.errstate(divide="ignore", invalid="ignore"):
        return k * np.log(lam) - lam - lam.dtype.type(math.lgamma(k + 1.0))


def log_likelihood(r, counts, exposure, n_lik):
    """(N_p,) ``sum_{c < n_lik} [k_c log lambda_c - lambda_c - log k_c!]``, ``lambda_c = t_c r_c``; -inf for a particle
    with any r_c, of all C channels, that is NaN, negative or +inf.  ``exposure``: one value, or one per channel."""
    r = np.asarray(r, dtype=np.float64)
    k = np.asarray(counts, dtype=np.float64).reshape(-1)
    t_in = np.asarray(exposure, dtype=np.float64).reshape(-1)
    t = np.ones(r.shape[0])
    t[:n_lik] = t_in[0] if t_in.size == 1 else t_in[:n_lik]
    ok = np.ones(r.shape[1], dtype=bool)
    ll = np.zeros(r.shape[1])
    for c in range(r.shape[0]):
        ok &= is_rate(r[c], t[c])
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(n_lik):
            ll = ll + log_pmf(k[c], t[c] * r[c])
    return np.where(ok, ll, -np.inf)


def likelihood(r, counts, exposure, n_lik, choke=None):
    """(N_p,) exp of ``log_likelihood``, then ``** choke``."""
    with np.errstate(invalid="ignore"):
        lik = np.exp(log_likelihood(r, counts, exposure, n_lik))
    return lik if choke is None else np.power(lik, choke)


def contributing(R, w, exposure=1.0):
    """(n_settings, N_p) bool: the weight is > 0 and every r_c at that setting is a rate.  ``R`` (n_s, N_p) or
    (n_s, C, N_p)."""
    R = np.asarray(R, dtype=np.float64)
    ok = is_rate(R, exposure)
    if R.ndim == 3:
        ok = np.all(ok, axis=1)
    return (clean_weights(w) > 0)[None, :] & ok


def _particle_terms(lam, cap):
    """``(p (cap, n), tau (n,), h (n,))`` of the censored reading for the means ``lam``: every p_k formed directly."""
    with np.errstate(divide="ignore", invalid="ignore"):
        logp = np.array([log_pmf(k, lam) for k in range(cap)])
    p = np.exp(logp)                                          # (lambda = 0: exp(-inf) = 0 for k > 0, 1 for k = 0)
    tau = np.maximum(1 - np.sum(p, axis=0), 0)
    # log lambda reads as 0 at lambda = 0, where p_k log p_k is 0 times a finite number
    logp[1:, lam == 0] = -np.array([math.lgamma(k + 1.0) for k in range(1, cap)]).reshape(-1, 1)
    h = -np.sum(p * logp, axis=0) - xlogx(tau)
    return p, tau, h


def design(R, w, exposure=1.0, cap=32, cost=1.0, dtype=np.float64):
    """``(information (n_settings,), distribution (n_settings, cap + 1))`` of the one-channel rates ``R``
    (n_settings, N_p):
        Pbar_k = sum w_i Pois(k; t r_i) / W for k < cap, taubar = sum w_i tau_i / W (the last column),
        U = max(-sum_k Pbar_k log Pbar_k - taubar log taubar - sum_i w_i h_i / W, 0) / cost,
    the mutual information, in nats, between the parameters and the next reading's count censored at ``cap``; NaN where
    W == 0."""
    R = np.asarray(R, dtype=np.float64)
    w = clean_weights(w)
    keep = contributing(R, w, exposure)
    pbar = np.full((R.shape[0], cap + 1), np.nan, dtype=dtype)
    info = np.full(R.shape[0], np.nan, dtype=dtype)
    for s in range(R.shape[0]):
        lam, ww = (exposure * R[s][keep[s]]).astype(dtype), w[keep[s]].astype(dtype)
        W = np.sum(ww)
        if not W > 0:
            continue
        p, tau, h = _particle_terms(lam, cap)
        pbar[s, :cap] = np.sum(ww * p, axis=1) / W
        pbar[s, cap] = np.sum(ww * tau) / W
        info[s] = max(-np.sum(xlogx(pbar[s])) - np.sum(ww * h) / W, 0)
    return info / np.asarray(cost, dtype=dtype), pbar


def information(R, w, exposure=1.0, cap=32, cost=1.0, dtype=np.float64):
    """(n_settings,): ``design()``'s information."""
    return design(R, w, exposure, cap, cost, dtype)[0]


def count_distribution(R, w, exposure=1.0, cap=32, dtype=np.float64):
    """(n_settings, cap + 1): ``design()``'s distribution."""
    return design(R, w, exposure, cap, 1.0, dtype)[1]


def noise_variance(R, w, exposure=1.0, dtype=np.float64):
    """(C, n_settings) ``sum w r_c / W / exposure_c``: the variance of the reading k / t; NaN where W == 0.  ``R``
    (n_s, C, N_p), or (n_s, N_p) for one channel."""
    R = np.asarray(R, dtype=np.float64)
    if R.ndim == 2:
        R = R[:, None, :]
    w = clean_weights(w)
    n_s, n_c, _ = R.shape
    t = np.broadcast_to(np.asarray(exposure, dtype=np.float64), (n_c,))
    keep = (clean_weights(w) > 0)[None, :] & np.all(is_rate(R, t[None, :, None]), axis=1)
    out = np.full((n_c, n_s), np.nan, dtype=dtype)
    for s in range(n_s):
        r, ww = R[s][:, keep[s]].astype(dtype), w[keep[s]].astype(dtype)
        W = np.sum(ww)
        if W > 0:
            out[:, s] = np.sum(ww * r, axis=1) / W / t
    return out


def normalised(t):
    """particlepdf.py:136-139: nan_to_num(t) / sum, nan_to_num again."""
    t = np.nan_to_num(np.asarray(t, dtype=np.float64))
    return np.nan_to_num(t / np.sum(t))


# ------------------------------------------------------------------------------------------------ the inputs
GRID = np.linspace(2.0, 4.0, 130)                 # one-channel and converged clouds
WIDTH = 0.1                                       # the Lorentzian's constant d
TIMES = np.linspace(0.05, 3.0, 65)                # two-channel cloud
DECAYS = ("b + a*exp(-t/T1)", "b + a*(1 - exp(-t/T1))")          # two counted channels: a decay and its complement
N_PARTICLES = (1, 63, 64, 65, 257, 4097, (1 << 17) + 3)
N_SETTINGS = (1, 63, 64, 65, 130)
SLICES = ((0, 64), (64, 130), (37, 101), (129, 130))
CAPS = (16, 32, 64)


def lorentz_cloud(g, n):
    """(3, n): x0 ~ U(2.6, 3.4), a ~ U(3, 8), b ~ U(2, 4): r = b + a / (1 + ((x - x0) / d)^2) in [2, 12]."""
    return np.array([g.uniform(2.6, 3.4, n), g.uniform(3.0, 8.0, n), g.uniform(2.0, 4.0, n)])


def converged_cloud(g, n):
    """(3, n): sigma(x0) = 0.002 about 3.0, a ~ N(5, 0.02), b ~ N(3, 0.02)."""
    return np.array([g.normal(3.0, 0.002, n), g.normal(5.0, 0.02, n), g.normal(3.0, 0.02, n)])


def decay_cloud(g, n):
    """(3, n): a ~ U(3, 8), b ~ U(0.5, 2), T1 ~ U(0.5, 2)."""
    return np.array([g.uniform(3.0, 8.0, n), g.uniform(0.5, 2.0, n), g.uniform(0.5, 2.0, n)])


def weights(g, cloud):
    """Non-uniform weights that sum to 1: uniform draws under a bell over the first parameter (the binomial tests')."""
    x = cloud[0]
    w = g.random(x.size) * np.exp(-0.5 * ((x - np.median(x)) / (np.std(x) + 1e-300)) ** 2)
    return w / w.sum()


def lorentz_rates(cloud, x=GRID):
    """(n_settings, N_p): the one-peak Lorentzian as a rate (optbayesexpt_amd.models.lorentzian(1))."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 1)
    return cloud[2] + cloud[1] / (((x - cloud[0]) / WIDTH) ** 2 + 1)


def decay_rates(cloud, t=TIMES):
    """(n_settings, 2, N_p): DECAYS, as models.from_expression takes them."""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1)
    a, b, t1 = cloud
    e = np.exp(-t / t1)
    return np.stack([b + a * e, b + a * (1 - e)], axis=1)
