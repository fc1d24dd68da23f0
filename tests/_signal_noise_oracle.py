"""Plain NumPy oracle of the signal-dependent noise model (OptBayesExptSignalNoise; csrc/obe_signal_noise.hip).

``coef`` is ``(C, 3)``: per channel ``{a, b, c}`` of ``nu_c(y) = a_c + b_c |y| + c_c y^2`` (a = noise_floor^2,
b = noise_gain, c = noise_relative^2).  Model values come from the caller: ``y`` is ``(C, N_p)`` for one setting,
``Y`` is ``(n_settings, C, N_p)``.
"""
import numpy as np


def coefficients(noise_floor, noise_gain, noise_relative, n_channels):
    """(C, 3) from the three public arguments (scalars or (C,))."""
    f, g, r = (np.broadcast_to(np.asarray(v, dtype=np.float64), (n_channels,))
               for v in (noise_floor, noise_gain, noise_relative))
    return np.stack([f * f, g, r * r], axis=1)


def nu(y, coef):
    """Noise variance of readings whose noise-free values are ``y`` (C, ...)."""
    y = np.asarray(y, dtype=np.float64)
    coef = np.asarray(coef, dtype=np.float64)
    shape = (coef.shape[0],) + (1,) * (y.ndim - 1)
    a, b, c = (coef[:, k].reshape(shape) for k in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        return a + b * np.abs(y) + c * (y * y)


def log_likelihood(y, y_meas, coef, n_lik):
    """(N_p,) log of the un-choked likelihood; -inf where a nu is not > 0 or not finite."""
    y = np.asarray(y, dtype=np.float64)[:n_lik]
    v = nu(y, np.asarray(coef)[:n_lik])
    ym = np.asarray(y_meas, dtype=np.float64).reshape(-1)[:n_lik, None]
    ok = np.all((v > 0) & np.isfinite(v), axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ll = np.sum(-(y - ym) ** 2 / (2.0 * v) - 0.5 * np.log(v), axis=0)
    return np.where(ok, ll, -np.inf)


def likelihood(y, y_meas, coef, n_lik, choke=None):
    """(N_p,) ``prod_{c < n_lik} exp(-(y_c - y_meas_c)^2 / (2 nu_c)) / sqrt(nu_c)``, then ``** choke``; 0 where a nu is
    not > 0 or not finite (obe_base.py:418-461 with sigma^2 = nu)."""
    y = np.asarray(y, dtype=np.float64)[:n_lik]
    v = nu(y, np.asarray(coef)[:n_lik])
    ym = np.asarray(y_meas, dtype=np.float64).reshape(-1)[:n_lik, None]
    ok = np.all((v > 0) & np.isfinite(v), axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        lik = np.exp(-np.sum((y - ym) ** 2 / (2.0 * v), axis=0)) / np.prod(np.sqrt(v), axis=0)
    lik = np.where(ok, lik, 0.0)
    if choke is not None:
        lik = np.power(lik, choke)
    return lik


def clean_weights(w):
    """NaN and negative weights count as zero."""
    w = np.asarray(w, dtype=np.float64)
    return np.where(w > 0, w, 0.0)


def noise_variance(Y, w, coef):
    """(C, n_settings) ``a + b sum w |y| / W + c sum w y^2 / W`` over the cloud; a particle of zero weight contributes
    nothing whatever its y is; W == 0 gives NaN."""
    Y = np.asarray(Y, dtype=np.float64)
    coef = np.asarray(coef, dtype=np.float64)
    w = clean_weights(w)
    keep = w > 0
    Yk, wk = Y[:, :, keep], w[keep]
    W = np.sum(wk)
    with np.errstate(divide="ignore", invalid="ignore"):
        s1 = np.sum(np.abs(Yk) * wk, axis=2) / W          # (n_settings, C)
        s2 = np.sum(Yk * Yk * wk, axis=2) / W
        return (coef[:, 0] + coef[:, 1] * s1 + coef[:, 2] * s2).T


def weighted_variance(Y, w):
    """(C, n_settings) ``sum w (y - mean)^2 / W``: the variance_full numerator."""
    Y = np.asarray(Y, dtype=np.float64)
    w = clean_weights(w)
    keep = w > 0
    Yk, wk = Y[:, :, keep], w[keep]
    W = np.sum(wk)
    mean = np.sum(Yk * wk, axis=2, keepdims=True) / W
    return (np.sum((Yk - mean) ** 2 * wk, axis=2) / W).T


def utility(yvar, nubar, cost=1.0):
    """(n_settings,) ``[sum_c yvar_c / nubar_c] / cost`` (obe_base.py:650-655 with a per-setting noise variance)."""
    return np.sum(np.asarray(yvar) / np.asarray(nubar), axis=0) / cost


def normalised(t):
    """particlepdf.py:136-139: nan_to_num(t) / sum, nan_to_num again."""
    t = np.nan_to_num(np.asarray(t, dtype=np.float64))
    return np.nan_to_num(t / np.sum(t))
