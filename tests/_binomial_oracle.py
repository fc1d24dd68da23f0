"""Plain NumPy oracle of the yes/no-outcome statistics (OptBayesExptBinomial; csrc/obe_binomial.hip), written from the
formulae of include/obe_hip.h, and the inputs the GPU tests run on (built and checked without a device).

Probabilities come from the caller: ``p`` is ``(C, N_p)`` for one setting, ``P`` is ``(n_settings, C, N_p)``.
``dtype=np.longdouble`` evaluates the same formulae in extended precision (the inputs stay the float64 values).
"""
import numpy as np

# ------------------------------------------------------------------------------------------------ the statistics


def clean_weights(w):
    """NaN and negative weights count as zero."""
    w = np.asarray(w, dtype=np.float64)
    return np.where(w > 0, w, 0.0)


def is_probability(p):
    """NaN fails."""
    with np.errstate(invalid="ignore"):
        return (p >= 0) & (p <= 1)


def xlogx(p):
    """p log p with 0 log 0 = 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p > 0, p * np.log(np.where(p > 0, p, 1)), 0 * p)


def h2(p):
    """-p log p - (1 - p) log1p(-p), 0 log 0 = 0."""
    q = 1 - p
    with np.errstate(divide="ignore", invalid="ignore"):
        return -xlogx(p) - np.where(q > 0, q * np.log1p(np.where(q > 0, -p, 0)), 0 * p)


def log_likelihood(p, successes, shots, n_lik):
    """(N_p,) ``sum_{c < n_lik} [k_c log p_c + (n_c - k_c) log1p(-p_c)]``, a term whose count is 0 skipped; -inf for a
    particle with any p_c, of all C channels, that is NaN or outside [0, 1]."""
    p = np.asarray(p, dtype=np.float64)
    k = np.asarray(successes, dtype=np.float64).reshape(-1)
    n = np.asarray(shots, dtype=np.float64).reshape(-1)
    ok = np.all(is_probability(p), axis=0)
    ll = np.zeros(p.shape[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(n_lik):
            if k[c] > 0:
                ll = ll + k[c] * np.log(p[c])
            if n[c] - k[c] > 0:
                ll = ll + (n[c] - k[c]) * np.log1p(-p[c])
    return np.where(ok, ll, -np.inf)


def likelihood(p, successes, shots, n_lik, choke=None):
    """(N_p,) exp of ``log_likelihood``, then ``** choke``."""
    lik = np.exp(log_likelihood(p, successes, shots, n_lik))
    return lik if choke is None else np.power(lik, choke)


def contributing(P, w):
    """(n_settings, N_p) bool: the weight is > 0 and every p_c at that setting is in [0, 1]."""
    return (clean_weights(w) > 0)[None, :] & np.all(is_probability(np.asarray(P, dtype=np.float64)), axis=1)


def outcome_marginals(P, w, dtype=np.float64):
    """(n_settings, 2^C): ``Pbar_o = sum_i w_i prod_c (bit c of o ? p_c,i : 1 - p_c,i) / W``; NaN where W == 0."""
    P = np.asarray(P, dtype=np.float64)
    w = clean_weights(w)
    keep = contributing(P, w)
    n_s, n_c, _ = P.shape
    out = np.full((n_s, 1 << n_c), np.nan, dtype=dtype)
    for s in range(n_s):
        p, ww = P[s][:, keep[s]].astype(dtype), w[keep[s]].astype(dtype)
        W = np.sum(ww)
        if not W > 0:
            continue
        for o in range(1 << n_c):
            prod = np.ones(p.shape[1], dtype=dtype)
            for c in range(n_c):
                prod = prod * (p[c] if (o >> c) & 1 else 1 - p[c])
            out[s, o] = np.sum(ww * prod) / W
    return out


def information(P, w, cost=1.0, dtype=np.float64):
    """(n_settings,) ``max(-sum_o Pbar_o log Pbar_o - hbar, 0) / cost``, ``hbar = sum_i w_i sum_c h2(p_c,i) / W``: the
    mutual information, in nats, between the parameters and the joint outcome of one shot in every channel; NaN where
    W == 0."""
    P = np.asarray(P, dtype=np.float64)
    w = clean_weights(w)
    keep = contributing(P, w)
    pbar = outcome_marginals(P, w, dtype)
    out = np.full(P.shape[0], np.nan, dtype=dtype)
    for s in range(P.shape[0]):
        p, ww = P[s][:, keep[s]].astype(dtype), w[keep[s]].astype(dtype)
        W = np.sum(ww)
        if not W > 0:
            continue
        hbar = np.sum(ww * np.sum(h2(p), axis=0)) / W
        out[s] = max(-np.sum(xlogx(pbar[s])) - hbar, 0)
    return out / np.asarray(cost, dtype=dtype)


def channel_information(P, w, dtype=np.float64):
    """(C, n_settings): the information of each channel's outcome alone."""
    P = np.asarray(P, dtype=np.float64)
    return np.array([information(P[:, c:c + 1], w, dtype=dtype) for c in range(P.shape[1])])


def noise_variance(P, w, shots=1.0, dtype=np.float64):
    """(C, n_settings) ``sum w p_c (1 - p_c) / W / shots_c``: the variance of the fraction k / n; NaN where W == 0."""
    P = np.asarray(P, dtype=np.float64)
    w = clean_weights(w)
    keep = contributing(P, w)
    n_s, n_c, _ = P.shape
    shots = np.broadcast_to(np.asarray(shots, dtype=np.float64), (n_c,))
    out = np.full((n_c, n_s), np.nan, dtype=dtype)
    for s in range(n_s):
        p, ww = P[s][:, keep[s]].astype(dtype), w[keep[s]].astype(dtype)
        W = np.sum(ww)
        if W > 0:
            out[:, s] = np.sum(ww * p * (1 - p), axis=1) / W / shots
    return out


def normalised(t):
    """particlepdf.py:136-139: nan_to_num(t) / sum, nan_to_num again."""
    t = np.nan_to_num(np.asarray(t, dtype=np.float64))
    return np.nan_to_num(t / np.sum(t))


# ------------------------------------------------------------------------------------------------ the inputs
GRID = np.linspace(2.0, 4.0, 130)                 # one-channel and converged clouds
WIDTH = 0.1                                       # the Lorentzian's constant d
TIMES = np.linspace(0.05, 3.0, 65)                # two-channel cloud
RAMSEY = ("0.5*(1 - exp(-t/T2)*cos(2*pi*f*t))", "0.5*(1 - exp(-t/T2)*sin(2*pi*f*t))")
N_PARTICLES = (1, 63, 64, 65, 255, 256, 257, 300, 4097, (1 << 17) + 3)
N_SETTINGS = (1, 63, 64, 65, 130)


def lorentz_cloud(g, n):
    """(3, n): x0 ~ U(2.6, 3.4), a ~ U(0.3, 0.6), b ~ U(0.1, 0.3): p = b + a / (1 + ((x - x0) / d)^2) in [0.1, 0.9]."""
    return np.array([g.uniform(2.6, 3.4, n), g.uniform(0.3, 0.6, n), g.uniform(0.1, 0.3, n)])


def converged_cloud(g, n):
    """(3, n): sigma(x0) = 0.002 about 3.0, a and b as narrow."""
    return np.array([g.normal(3.0, 0.002, n), g.normal(0.45, 0.002, n), g.normal(0.2, 0.002, n)])


def ramsey_cloud(g, n):
    """(2, n): f ~ U(0.8, 1.2), T2 ~ U(2, 6)."""
    return np.array([g.uniform(0.8, 1.2, n), g.uniform(2.0, 6.0, n)])


def weights(g, cloud):
    """Non-uniform weights that sum to 1: uniform draws under a bell over the first parameter."""
    x = cloud[0]
    w = g.random(x.size) * np.exp(-0.5 * ((x - np.median(x)) / (np.std(x) + 1e-300)) ** 2)
    return w / w.sum()


def lorentz_probabilities(cloud, x=GRID):
    """(n_settings, 1, N_p): the one-peak Lorentzian as a probability curve (optbayesexpt_amd.models.lorentzian(1))."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 1)
    return (cloud[2] + cloud[1] / (((x - cloud[0]) / WIDTH) ** 2 + 1))[:, None, :]


def ramsey_probabilities(cloud, t=TIMES):
    """(n_settings, 2, N_p): the two quadratures of a Ramsey fringe (RAMSEY, as models.from_expression takes it)."""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1)
    f, t2 = cloud
    env = np.exp(-t / t2)
    return np.stack([0.5 * (1 - env * np.cos(2 * np.pi * f * t)), 0.5 * (1 - env * np.sin(2 * np.pi * f * t))], axis=1)
