"""Host oracle of obe_predictive_reading_quantiles (quantiles of the next reading), from rows of model values.

``y`` (C, N_p): the model at the setting for every particle; ``w`` (N_p,); ``sigma`` (C,) for a known noise or (C, N_p)
for a row per particle.  The rules of include/obe_hip.h:

* a particle CONTRIBUTES to channel c iff its weight is > 0 (NaN and negative weights count as zero), every sigma of it
  is > 0 (all channels: the scoring rule) and y[c] is finite (+-inf too is left out: a reading cannot be infinite);
* T_c = sum w over the contributing particles; T_c == 0 gives NaN;
* L_c(v) = sum w Phi((v - y_c) / sigma_c), U_c(v) = sum w Phi((y_c - v) / sigma_c), each a sum of positive terms;
* the result for the level q is the v with L_c(v) = q T_c for q <= 1/2, with U_c(v) = (1 - q) T_c for q > 1/2 — the
  TARGET, in the tail where it is small (1 - q is exact in double there).

The tails are math.fsum sums of erfc terms with z formed in long double; the root comes from scipy.optimize.brentq on the
guaranteed bracket [min (y + z- sigma), max (y + z+ sigma)], z-+ = Phi^-1(q) -+ 1e-9 (1 + |Phi^-1(q)|): at its lower end
every term of L is <= q (every term of U >= 1 - q), at its upper end the other way round.
"""
import math

import numpy as np
from scipy import optimize, special

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
TINY = 2.0 ** -1022
SQRT2 = np.sqrt(LD(2.0))
INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)


def clean(w):
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(w > 0.0, w, 0.0)


def normal_quantile(q):
    """Phi^-1(q), from the tail q is small in."""
    return float(special.ndtri(q)) if q <= 0.5 else -float(special.ndtri(1.0 - q))


class Reading:
    """The mixture of one setting: rows ``y`` (C, N_p), weights, sigma (C,) or (C, N_p)."""

    def __init__(self, y, w, sigma):
        self.y = np.atleast_2d(np.asarray(y, dtype=np.float64))
        sigma = np.asarray(sigma, dtype=np.float64)
        if sigma.ndim < 2:
            sigma = sigma.reshape(-1, 1)
        self.sigma = np.broadcast_to(sigma, self.y.shape)
        self.w = clean(w)
        with np.errstate(invalid="ignore"):
            self.valid = (self.w > 0.0) & np.all(self.sigma > 0.0, axis=0)

        self._kept = {}

    def _rows(self, c):
        if c not in self._kept:
            keep = self.valid & np.isfinite(self.y[c])
            self._kept[c] = self.y[c][keep], self.w[keep], self.sigma[c][keep], math.fsum(self.w[keep])
        return self._kept[c][:3]

    def total(self, c):
        self._rows(c)
        return self._kept[c][3]

    def target(self, c, q):
        """(target, upper): q T_c in the lower tail, or (1 - q) T_c in the upper one."""
        upper = q > 0.5
        return (1.0 - q if upper else q) * self.total(c), upper

    def tail(self, c, v, upper):
        """L_c(v), or U_c(v)."""
        f, w, s = self._rows(c)
        with np.errstate(all="ignore"):
            z = ((LD(v) - f.astype(LD)) / s.astype(LD) / SQRT2).astype(np.float64)
        return math.fsum(w * (0.5 * special.erfc(z if upper else -z)))

    def density(self, c, v):
        """D_c(v) = sum w phi(z) / sigma."""
        f, w, s = self._rows(c)
        with np.errstate(all="ignore"):
            z = ((LD(v) - f.astype(LD)) / s.astype(LD)).astype(np.float64)
            return math.fsum(w * np.exp(-0.5 * z * z) / s) * INV_SQRT_2PI

    def residual(self, c, q, v):
        target, upper = self.target(c, q)
        return abs(self.tail(c, v, upper) - target)

    def bracket(self, c, q):
        f, _, s = self._rows(c)
        z = normal_quantile(q)
        hair = 1e-9 * (1.0 + abs(z))
        return float(np.min(f + (z - hair) * s)), float(np.max(f + (z + hair) * s))

    def quantile(self, c, q):
        target, upper = self.target(c, q)
        if not target > 0.0:
            return float("nan")
        lo, hi = self.bracket(c, q)
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)      # (the ends themselves are rounded sums)

        def g(v):
            return self.tail(c, v, upper) - target
        g_lo, g_hi = g(lo), g(hi)
        if g_lo == 0.0:
            return lo
        if g_hi == 0.0:
            return hi
        assert (g_lo < 0.0) != (g_hi < 0.0), (lo, hi, g_lo, g_hi)
        return float(optimize.brentq(g, lo, hi, xtol=5e-324, rtol=4.0 * EPS, maxiter=5000))

    def tolerance(self, c, q, v):
        """What |A(v) - target| may be for a device result v: 1e-10 target + 8 eps max(|v|, 2^-1022) D(v).  Derived, not
        measured: the stopping rule is 2^-36 = 1.5e-11 of the target, the fixed-order sums add at most (chunk length +
        chunks) eps < 1e-12, and a bracket closed at 4 ulp moves A by at most 4 ulp D."""
        return 1e-10 * self.target(c, q)[0] + 8.0 * EPS * max(abs(v), TINY) * self.density(c, v)
