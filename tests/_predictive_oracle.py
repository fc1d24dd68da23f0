"""Oracles for the posterior predictive summaries (tests/test_predictive_host.py pins them against NumPy;
tests/test_gpu_predictive.py compares the device results with them).  The rows y come from the product's own
eval_over_all_parameters; on them the moments are formed in extended precision (math.fsum of exact products where the
data allow it, long double otherwise) and the quantiles by tests/_posterior_oracle.py."""
import math

import numpy as np

import _posterior_oracle as post


def kept(y, w):
    """(y, w) of the particles that count: NaN and negative weights are zero, a particle of zero weight is left out
    whatever its y."""
    w = post.clean_weights(w)
    w[w < 0] = 0.0
    keep = w > 0
    return np.asarray(y, dtype=np.float64)[keep], w[keep]


def moments_fsum(y, w):
    """(mean, var, A): math.fsum of the double products — exact when the products are (dyadic data)."""
    y, w = kept(y, w)
    sw = math.fsum(w)
    mean = math.fsum(w * y) / sw
    var = math.fsum(w * (y - mean) ** 2) / sw
    return mean, var, math.fsum(w * np.abs(y)) / sw


def moments(y, w):
    """(mean, var, A) in long double, two passes: mean = sum w y / sum w, var = sum w (y - mean)^2 / sum w about that
    mean, A = sum w |y| / sum w.  Returned as float64 (NaN / inf where the data make them)."""
    y, w = kept(y, w)
    y, w = y.astype(np.longdouble), w.astype(np.longdouble)
    with np.errstate(invalid="ignore", over="ignore"):
        sw = w.sum()
        mean = (w * y).sum() / sw
        var = (w * (y - mean) ** 2).sum() / sw
        a = (w * np.abs(y)).sum() / sw
    return float(mean), float(var), float(a)


def mean_tolerance(a):
    """|err| <= 1e-10 A: the project's 1e-10 on the conditioning of a weighted mean (a channel may cross zero)."""
    return 1e-10 * a


def var_tolerance(var, a):
    """|err| <= 1e-10 var + 1e-20 A^2: the project's bar with a floor for exactly degenerate clouds (a badly centred
    sum errs by ~1e-16 A^2, far above the floor)."""
    return 1e-10 * var + 1e-20 * a * a
