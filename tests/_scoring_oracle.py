"""Host oracle of the scoring entry points (obe_predictive_logpdf / obe_predictive_tails), from rows of model values.

``y`` (C, N_p): the model at the record's setting for every particle; ``w`` (N_p,); ``y_meas`` (C,); ``sigma`` (C,)
for a known noise or (C, N_p) for a row per particle.  z = (y - y_meas) / sigma.  The rules of include/obe_hip.h:
NaN and negative weights count as zero; a particle enters only with a weight > 0 and every sigma of it > 0;
the density skips a particle whose log-term is -inf or NaN, a tail skips a NaN z; sum w == 0 gives NaN.
The density is a log-sum-exp in long double, the tails are math.fsum sums of erfc terms.
"""
import math

import numpy as np
from scipy import special

LD = np.longdouble
LOG_2PI = np.log(LD(2.0) * LD(np.pi))


def clean(w):
    w = np.asarray(w, dtype=np.float64)
    return np.where(w > 0.0, w, 0.0)


def _rows(y, sigma):
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    sigma = np.asarray(sigma, dtype=np.float64)
    if sigma.ndim < 2:
        sigma = sigma.reshape(-1, 1)
    return y, np.broadcast_to(sigma, y.shape)


def _valid(w, sigma):
    with np.errstate(invalid="ignore"):
        return (w > 0.0) & np.all(sigma > 0.0, axis=0)


def log_terms(y, y_meas, sigma):
    """l_i = sum_c [-z_c^2 / 2 - log sigma_c] in long double (NaN / -inf where the device skips)."""
    y, sigma = _rows(y, sigma)
    ym = np.asarray(y_meas, dtype=np.float64).reshape(-1, 1)
    with np.errstate(all="ignore"):
        z = (y.astype(LD) - ym.astype(LD)) / sigma.astype(LD)
        return np.sum(-(z * z) / 2 - np.log(sigma.astype(LD)), axis=0)


def logpdf(y, w, y_meas, sigma):
    y, sigma = _rows(y, sigma)
    w = clean(w)
    sw = math.fsum(w)
    if not sw > 0.0:
        return float("nan")
    l = log_terms(y, y_meas, sigma)
    keep = _valid(w, sigma) & np.isfinite(l)
    if not keep.any():
        return float("-inf")
    l, wk = l[keep], w[keep].astype(LD)
    top = l.max()
    with np.errstate(under="ignore"):
        terms = np.sort(wk * np.exp(l - top))
    return float(top + np.log(terms.sum()) - np.log(LD(sw)) - y.shape[0] * LOG_2PI / 2)


def tails(y, w, y_meas, sigma):
    """(lower (C,), upper (C,)): P(Y_c <= y_meas_c) and P(Y_c >= y_meas_c)."""
    y, sigma = _rows(y, sigma)
    ym = np.asarray(y_meas, dtype=np.float64).reshape(-1, 1)
    w = clean(w)
    sw = math.fsum(w)
    n_c = y.shape[0]
    if not sw > 0.0:
        return np.full(n_c, np.nan), np.full(n_c, np.nan)
    ok = _valid(w, sigma)
    lower, upper = np.zeros(n_c), np.zeros(n_c)
    with np.errstate(all="ignore"):
        z = ((y.astype(LD) - ym.astype(LD)) / sigma.astype(LD) / np.sqrt(LD(2.0))).astype(np.float64)
    for c in range(n_c):
        keep = ok & ~np.isnan(z[c])
        zc, wc = z[c][keep], w[keep]
        lower[c] = math.fsum(wc * (0.5 * special.erfc(zc))) / sw
        upper[c] = math.fsum(wc * (0.5 * special.erfc(-zc))) / sw
    return lower, upper


def logpdf_tolerance(want):
    """|d log p| <= 1e-10 max(1, |log p|): the exponent-scale rule of tests/_replay.py: close_weights."""
    return 1e-10 * max(1.0, abs(want))
