"""Plain NumPy oracle of count-aware scoring and reading bands (CountReadings.count_*; csrc/obe_counts.hip, K20), written
from the formulae of include/obe_hip.h, and the inputs the GPU tests run on (built and checked without a device).

Deliberately NOT the kernel's block recurrence: every ``P(k)`` is formed directly from ``math.lgamma``,
``exp(log C(n, k) + k log p + (n - k) log1p(-p))`` and ``exp(k log lambda - lambda - log k!)``, with the point masses at
p = 0, p = 1 and lambda = 0 by definition.  The model values come from the curves and clouds of _binomial_oracle.py and
_poisson_oracle.py: ``V`` is ``(n_points, C, N_p)``.  ``side`` (shots, exposure) is ``(C,)`` or ``(C, n_points)``.
``dtype=np.longdouble`` evaluates the same formulae in extended precision (the inputs and the lgamma constants stay
float64 values).
"""
import math

import numpy as np

import _binomial_oracle as bino
import _poisson_oracle as pois

BINOMIAL, POISSON = "binomial", "poisson"


# ------------------------------------------------------------------------------------------------ the statistics
def pmf(law, k, side, v, dtype=np.float64):
    """``P(k)`` of one channel elementwise over the model values ``v`` (p or r), ``side`` the shots n or exposure t."""
    v = np.asarray(v, dtype=dtype)
    if law == BINOMIAL:
        n = int(side)
        if k > n:
            return np.zeros_like(v)
        lc = math.lgamma(n + 1.0) - math.lgamma(k + 1.0) - math.lgamma(n - k + 1.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = k * np.log(np.where(v > 0, v, 1)) if k > 0 else 0 * v
            b = (n - k) * np.log1p(-np.where(v < 1, v, 0)) if n - k > 0 else 0 * v
            out = np.exp(dtype(lc) + a + b)
        if k > 0:
            out = np.where(v == 0, 0, out)
        if n - k > 0:
            out = np.where(v == 1, 0, out)
        return out
    lam = dtype(side) * v
    if k == 0:
        return np.exp(-lam)
    with np.errstate(divide="ignore"):
        out = np.exp(k * np.log(np.where(lam > 0, lam, 1)) - lam - dtype(math.lgamma(k + 1.0)))
    return np.where(lam == 0, 0, out)


def contributing(law, V, w, side):
    """(n_points, N_p) bool: the weight is > 0 and every channel's value at the point is one the law takes."""
    V = np.asarray(V, dtype=np.float64)
    side = _side(side, V)
    clean = np.where(np.asarray(w, dtype=np.float64) > 0, w, 0.0) > 0
    if law == BINOMIAL:
        ok = np.all(bino.is_probability(V), axis=1)
    else:
        ok = np.all(pois.is_rate(V, side.T[:, :, None]), axis=1)
    return clean[None, :] & ok


def _side(side, V):
    """(C, n_points)."""
    side = np.asarray(side, dtype=np.float64)
    if side.ndim == 0:
        side = np.full(V.shape[1], float(side))
    return np.ascontiguousarray(np.broadcast_to(side.reshape(V.shape[1], -1), (V.shape[1], V.shape[0])))


def table(law, V, w, side, count_max, dtype=np.float64):
    """(n_points, C, count_max + 2): ``Pbar_c(k) = sum_i w_i P_c,i(k) / W`` for k = 0 .. count_max, then the mass above:
    ``sum_i w_i max(1 - sum_k P_c,i(k), 0) / W``, exactly 0 for shots <= count_max.  NaN where W == 0."""
    V = np.asarray(V, dtype=np.float64)
    w = np.where(np.asarray(w, dtype=np.float64) > 0, w, 0.0)
    side = _side(side, V)
    keep = contributing(law, V, w, side)
    n_pts, n_c, _ = V.shape
    out = np.full((n_pts, n_c, count_max + 2), np.nan, dtype=dtype)
    for s in range(n_pts):
        ww = w[keep[s]].astype(dtype)
        W = np.sum(ww)
        if not W > 0:
            continue
        for c in range(n_c):
            v = V[s, c][keep[s]]
            total = np.zeros(v.shape, dtype=dtype)
            for k in range(count_max + 1):
                p = pmf(law, k, side[c, s], v, dtype)
                out[s, c, k] = np.sum(ww * p) / W
                total = total + p
            if law == BINOMIAL and side[c, s] <= count_max:
                out[s, c, count_max + 1] = 0
            else:
                out[s, c, count_max + 1] = np.sum(ww * np.maximum(1 - total, 0)) / W
    return out


def tails(tab, k):
    """``(lower, upper)`` (C, n_points) from a table (n_points, C, count_max + 2) and the counts k (C, n_points):
    ``sum_{j <= k} Pbar(j)`` and ``sum_{j >= k} Pbar(j)`` + the mass above; both include k."""
    n_pts, n_c, _ = tab.shape
    lo, up = np.empty((n_c, n_pts), dtype=tab.dtype), np.empty((n_c, n_pts), dtype=tab.dtype)
    for s in range(n_pts):
        for c in range(n_c):
            kk = int(k[c, s])
            lo[c, s] = np.sum(tab[s, c, :kk + 1])
            up[c, s] = np.sum(tab[s, c, kk:][::-1])
    return lo, up


def cdf(tab):
    """(n_points, C, count_max + 1): the running sums of a table's rows."""
    return np.cumsum(tab[:, :, :-1], axis=2)


def quantiles(tab, qs):
    """(n_q, C, n_points) float64: the smallest k with cdf(k) >= q, NaN where count_max is too small (or W == 0)."""
    cum = cdf(tab)
    n_pts, n_c, n_k = cum.shape
    out = np.full((len(qs), n_c, n_pts), np.nan)
    for j, q in enumerate(qs):
        reached = cum >= q
        first = np.argmax(reached, axis=2)
        out[j] = np.where(np.any(reached, axis=2), first, np.nan).T
    return out


def level_margin(tab, qs):
    """The smallest ``|cdf(k) - q|`` over every point, channel, k and level: condition (b) of the quantile tests."""
    cum = cdf(tab)
    return min(float(np.nanmin(np.abs(cum - type(cum.flat[0])(q)))) for q in qs)


def joint_logpmf(law, V, w, k, side, dtype=np.float64):
    """(n_points,): ``log(sum_i w_i prod_c P_c,i(k_c) / W)`` of the records k (C, n_points) — the joint evidence;
    -inf where impossible for everybody, NaN where W == 0."""
    V = np.asarray(V, dtype=np.float64)
    w = np.where(np.asarray(w, dtype=np.float64) > 0, w, 0.0)
    side = _side(side, V)
    keep = contributing(law, V, w, side)
    out = np.full(V.shape[0], np.nan, dtype=dtype)
    for s in range(V.shape[0]):
        ww = w[keep[s]].astype(dtype)
        W = np.sum(ww)
        if not W > 0:
            continue
        prod = np.ones(ww.shape, dtype=dtype)
        for c in range(V.shape[1]):
            prod = prod * pmf(law, int(k[c, s]), side[c, s], V[s, c][keep[s]], dtype)
        with np.errstate(divide="ignore"):
            out[s] = np.log(np.sum(ww * prod) / W)
    return out


def marginal_logpmf_sum(law, V, w, k, side, dtype=np.float64):
    """(n_points,): ``sum_c log Pbar_c(k_c)``, what an implementation that multiplies the channels' mixtures gives."""
    V = np.asarray(V, dtype=np.float64)
    side = _side(side, V)
    out = np.zeros(V.shape[0], dtype=dtype)
    for c in range(V.shape[1]):
        out = out + joint_logpmf(law, V[:, c:c + 1], w, k[c:c + 1], side[c:c + 1], dtype)
    return out


# ------------------------------------------------------------------------------------------------ the inputs
N_PARTICLES = (1, 63, 64, 65, 257, 4097)
N_POINTS = (1, 63, 64, 65, 130)
COUNT_MAXES = (0, 1, 31, 32, 33, 63, 64, 65, 191)
SHOTS = (1, 2, 31, 32, 33, 100)
EXPOSURE = 8.0                    # Lorentzian rates 2 .. 12: lambda in [16, 96]
DEFAULT_EXPOSURE = 16.0           # ... in [32, 192]: every row up to the default count_max 256 stays above 1e-200
# probabilities next to 0 and 1 (and one in the middle), each alone and mixed
EDGE_PROBABILITIES = [1.0 - 1e-6, 1.0 - 1e-12, 1e-6, 1e-12, 0.99999, 0.3]
EDGE_WEIGHTS = [0.3, 0.2, 0.1, 0.1, 0.2, 0.1]
LEVELS = (0.025, 0.5, 0.975)
# (side, count_max) of the quantile tests, by (law, kind of input); 257 particles each
QUANTILE_CASES = {(BINOMIAL, "wide"): (100, 100), (BINOMIAL, "two"): ((31, 33), 33),
                  (POISSON, "wide"): (EXPOSURE, 191), (POISSON, "two"): ((4.0, 8.0), 127)}
GRID, TIMES = pois.GRID, pois.TIMES

_CASES = {}


def case(law, kind, n):
    """``(cloud, weights, V (n_points, C, n))`` of an input: ``kind`` in wide / converged (the one-peak Lorentzian over
    GRID, one channel) or two (DECAYS for Poisson, RAMSEY for binomial over TIMES, two channels); made once."""
    key = (law, kind, n)
    if key not in _CASES:
        o = bino if law == BINOMIAL else pois
        seed = {"wide": 500, "converged": 600, "two": 700}[kind] + n + (0 if law == BINOMIAL else 50000)
        g = np.random.default_rng(seed)
        if kind == "two":
            cloud = (o.ramsey_cloud if law == BINOMIAL else o.decay_cloud)(g, n)
            V = o.ramsey_probabilities(cloud) if law == BINOMIAL else o.decay_rates(cloud)
        else:
            cloud = (o.lorentz_cloud if kind == "wide" else o.converged_cloud)(g, n)
            V = o.lorentz_probabilities(cloud) if law == BINOMIAL else o.lorentz_rates(cloud)[:, None, :]
        _CASES[key] = (cloud, o.weights(g, cloud), np.ascontiguousarray(V))
    return _CASES[key]


_TABLES = {}


def case_table(law, kind, n, side, count_max, points=None, dtype=np.float64):
    """``table()`` of a case at its first ``points`` points; computed once and shared (read-only)."""
    key = (law, kind, n, tuple(np.atleast_1d(side).tolist()), count_max, points, dtype)
    if key not in _TABLES:
        _, w, V = case(law, kind, n)
        t = table(law, V[:points], w, side, count_max, dtype)
        t.setflags(write=False)
        _TABLES[key] = t
    return _TABLES[key]


# the high-rate case: exposure x rate in about 800 .. 1000, where e^-lambda underflows
HIGH_EXPOSURE, HIGH_COUNT_MAX, HIGH_POINTS = 100.0, 1200, np.array([2.99, 3.0, 3.01])


def high_rate_case():
    """(cloud (3, 257), weights, V (3, 1, 257)): the Lorentzian with b in [3, 4] and a in [5, 6] at three points on the
    peak (x0 within 0.02 of 3): rates 7.5 .. 10 per unit exposure, lambda 750 .. 1000 at exposure 100."""
    if "high" not in _CASES:
        g = np.random.default_rng(811)
        cloud = np.array([g.uniform(2.98, 3.02, 257), g.uniform(5.0, 6.0, 257), g.uniform(3.0, 4.0, 257)])
        V = pois.lorentz_rates(cloud, HIGH_POINTS)[:, None, :]
        _CASES["high"] = (cloud, pois.weights(g, cloud), np.ascontiguousarray(V))
    return _CASES["high"]


def edge_table(values, weights, shots, dtype=np.float64):
    """``table()`` of particles whose probability IS ``values``, at two points, count_max = shots."""
    V = np.broadcast_to(np.asarray(values, dtype=np.float64), (2, 1, len(values)))
    return table(BINOMIAL, V, weights, shots, shots, dtype)
