"""NumPy / math.fsum oracles for the posterior summaries (tests/test_posterior_host.py pins them against NumPy;
tests/test_gpu_posterior.py compares the device results with them)."""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)


def clean_weights(w):
    """NaN weights count as zero (the rule of bayesian_update's nan_to_num)."""
    w = np.array(w, dtype=np.float64)
    w[np.isnan(w)] = 0.0
    return w


def bin_index(x, edges):
    """Bin of every x by the edges alone: edges[k] <= x < edges[k + 1], x == edges[-1] in the last bin, -1 for
    values outside the range and NaN."""
    x = np.asarray(x, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    k = np.searchsorted(edges, x, side="right") - 1
    k[x == edges[-1]] = len(edges) - 2
    with np.errstate(invalid="ignore"):
        inside = (x >= edges[0]) & (x <= edges[-1])
    k[~inside] = -1
    return k


def histogram_fsum(x, w, edges):
    """(exactly rounded mass per bin, particles per bin) — math.fsum of the weights of each bin."""
    k = bin_index(x, edges)
    w = clean_weights(w)
    n_bins = len(edges) - 1
    order = np.argsort(k, kind="stable")
    ks, ws = k[order], w[order]
    starts = np.searchsorted(ks, np.arange(n_bins), side="left")
    stops = np.searchsorted(ks, np.arange(n_bins), side="right")
    mass = np.array([math.fsum(ws[a:b]) for a, b in zip(starts, stops)])
    return mass, (stops - starts).astype(np.int64)


def histogram2d_index(x, y, xedges, yedges):
    kx, ky = bin_index(x, xedges), bin_index(y, yedges)
    flat = kx * (len(yedges) - 1) + ky
    flat[(kx < 0) | (ky < 0)] = -1
    return flat


def mass_bound(mass_exact, n_bin, sum_w):
    """|fixed-point mass - exact| per bin: one rounding of each product, rint off by at most 1/2, one rounding of the
    final conversion."""
    return 4 * EPS * mass_exact + n_bin * 2.0 ** -62 * sum_w


def scale_exponent(sum_w):
    """k of Q = rint(w 2^k): 62 - e for the smallest e with sum_w <= 2^e (1 + 2^-20)."""
    if not (sum_w > 0 and np.isfinite(sum_w)):
        return 62
    m, ex = math.frexp(sum_w)
    return 62 - (ex - 1 if m <= 0.5 * (1 + 2.0 ** -20) else ex)


def integer_weights(w):
    """(Q as Python-exact uint64 array, k)."""
    w = clean_weights(w)
    w[w < 0] = 0.0
    k = scale_exponent(float(np.sum(w)))
    return np.rint(np.ldexp(w, k)).astype(np.uint64), k


def quantile_fixed_point(x, w, q):
    """The definition the kernels implement: the smallest particle value (np.sort order) whose cumulative integer
    weight reaches max(1, ceil(q sum Q))."""
    x = np.asarray(x, dtype=np.float64)
    Q, _ = integer_weights(w)
    order = np.argsort(x, kind="stable")
    cum = np.cumsum(Q[order])
    total = int(cum[-1])
    out = []
    for qq in np.atleast_1d(q):
        want = min(max(1, int(math.ceil(float(qq) * float(total)))), max(total, 1))
        i = int(np.searchsorted(cum, np.uint64(want), side="left"))
        out.append(x[order][min(i, len(x) - 1)])
    return np.array(out)


def quantile_numpy(x, w, q):
    return np.quantile(np.asarray(x, dtype=np.float64), q, weights=clean_weights(w), method="inverted_cdf")


def cdf_bracket(x, w, value):
    """(F(value-), F(value)): exactly rounded weight strictly below, and at or below, ``value``."""
    x = np.asarray(x, dtype=np.float64)
    w = clean_weights(w)
    return math.fsum(w[x < value]), math.fsum(w[x <= value])


def dyadic_cloud(g, n_dims, n, bits=30, top=1000):
    """A cloud whose weights are integers / 2^bits: every weighted sum is exact in any order."""
    x = g.normal(size=(n_dims, n)) * (10.0 ** g.integers(-2, 3, size=(n_dims, 1)))
    w = g.integers(0, top, size=n).astype(np.float64) / 2.0 ** bits
    if not w.any():
        w[0] = 1.0 / 2.0 ** bits
    return x, w
