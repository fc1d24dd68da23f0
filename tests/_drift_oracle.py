"""One step of the parameter drift (include/obe_hip.h: obe_drift_particles) in exact arithmetic, on the CPU only.

The contract is the chain of operations itself, each of them one correctly rounded double operation, per drifted row
k and particle p:

    s = 0.0;  s = fma(z[p, j], G[k, j], s)  for j = 0 .. K-1        (all K terms, one rounding per step)
    v = x[rows[k], p] + s
    with bounds:  if v < lo[k]: v = lo[k] + (lo[k] - v)   elif v > hi[k]: v = hi[k] - (v - hi[k])     (two roundings)

— the nudge of a resample without its gather, so ``fma`` and the chain are tests/_resample_oracle.py's own.  Rows that
are not drifted are returned as they came.

The neighbouring chains a kernel could compute instead (``drift_mul_then_add``, ``drift_reversed_j``,
``drift_from_x``) and the reflection contracted into one fma (``reflect_contracted``) are here for
tests/test_drift_host.py, which shows that the inputs of tests/test_gpu_drift.py (``general_case``) tell the contract
from each of them.
"""
import numpy as np

import _resample_oracle as ro


def reflect_two_roundings(v, lo, hi):
    """One reflection at the bound crossed, the difference and the sum (or second difference) rounded separately;
    NaN (every comparison false) is left alone.  ``lo`` / ``hi``: (K,), one interval per row of ``v`` (K, n)."""
    lo, hi = (np.asarray(b, dtype=np.float64)[:, None] for b in (lo, hi))
    with np.errstate(invalid="ignore"):
        below, above = v < lo, v > hi
        over_lo = lo - v
        over_hi = v - hi
        return np.where(below, lo + over_lo, np.where(above, hi - over_hi, v))


def reflect_contracted(v, lo, hi):
    """The wrong form 2*lo - v (2*hi - v) as ONE fma: the difference lo - v is not rounded."""
    f = ro.fast_fma_checked() or ro.fma_exact
    out = np.array(v, dtype=np.float64)
    for k, row in enumerate(out.tolist()):
        l, h = float(lo[k]), float(hi[k])
        out[k] = [f(2.0, l, -x) if x < l else (f(2.0, h, -x) if x > h else x) for x in row]
    return out


def _apply(x, rows, moved, lo, hi):
    if lo is not None:
        moved = reflect_two_roundings(moved, lo, hi)
    out = np.array(x, dtype=np.float64)
    out[np.asarray(rows, dtype=np.int64)] = moved
    return out


def _inputs(x, rows, z, G):
    x, z, G = (np.asarray(a, dtype=np.float64) for a in (x, z, G))
    return x, np.asarray(rows, dtype=np.int64), z, G


def drift_exact(x, rows, z, G, lo=None, hi=None):
    """The (D, n) array obe_drift_particles leaves, from ``x`` (D, n), ``rows`` (K,), ``z`` (n, K), ``G`` (K, K) and,
    for a reflecting step, ``lo`` / ``hi`` (K,)."""
    x, rows, z, G = _inputs(x, rows, z, G)
    return _apply(x, rows, x[rows] + ro._chain(z, G), lo, hi)


# ---- the neighbours of the contract: each differs from it in the last bit or two on general doubles
def drift_mul_then_add(x, rows, z, G, lo=None, hi=None):
    """s = s + z*G: the product rounded before the addition."""
    x, rows, z, G = _inputs(x, rows, z, G)
    return _apply(x, rows, x[rows] + ro._chain(z, G, fused=False), lo, hi)


def drift_reversed_j(x, rows, z, G, lo=None, hi=None):
    """The FMA chain from zero, j = K-1 .. 0."""
    x, rows, z, G = _inputs(x, rows, z, G)
    return _apply(x, rows, x[rows] + ro._chain(z, G, order=range(z.shape[1] - 1, -1, -1)), lo, hi)


def drift_from_x(x, rows, z, G, lo=None, hi=None):
    """The FMA chain started from x[rows[k], p] instead of zero (no addition of its own)."""
    x, rows, z, G = _inputs(x, rows, z, G)
    return _apply(x, rows, ro._chain(z, G, start=np.ascontiguousarray(x[rows])), lo, hi)


WRONG_CHAINS = {"mul-then-add": drift_mul_then_add, "reversed j": drift_reversed_j, "started from x": drift_from_x}


def drift_integers(x, rows, z, G):
    """The same array for INTEGER inputs (|x| <= 2^20, |z|, |G| <= 8) in NumPy integer arithmetic: every operation of
    the contract is exact on such data, so every evaluation order gives these bits."""
    x, z, G = (np.asarray(a) for a in (x, z, G))
    for a in (x, z, G):
        assert np.array_equal(a, np.rint(a))
    out = x.astype(np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    out[rows] = out[rows] + G.astype(np.int64) @ z.astype(np.int64).T
    return out.astype(np.float64)


# ---- the inputs of the GPU file
def spread_rows(k, d):
    """K ascending rows of a D-row cloud: all of them for D = K, else non-adjacent where there is room."""
    if d == k:
        return np.arange(k, dtype=np.int32)
    if k == 1:
        return np.array([d - 1], dtype=np.int32)
    rows = np.unique(np.round(np.linspace(0, d - 1, k)).astype(np.int32))
    assert rows.size == k
    return rows


def general_case(k, n, d=None, seed=None):
    """General doubles: rows of ``x`` of scale 1 .. D, a full lower-triangular G ~ N(0, 0.1), z ~ N(0, 1).
    (x (D, n), rows (K,) int32, z (n, K), G (K, K)), C-contiguous."""
    d = k if d is None else d
    g = np.random.default_rng(33000 + 1000 * d + 100 * k + n % 9973 if seed is None else seed)
    x = g.normal(0.0, 1.0, (d, n)) * np.arange(1, d + 1)[:, None]
    z = g.standard_normal((n, k))
    G = np.tril(g.normal(0.0, 0.1, (k, k)))
    return tuple(np.ascontiguousarray(a) for a in (x, spread_rows(k, d), z, G))


def reflection_interval(k):
    """(lo, hi) per drifted row for the reflecting cases: an interval far narrower than the rows' spread and no simple
    multiple of anything, so that nearly every value is reflected, most of them from further away than the interval is
    wide (they stay outside: one reflection, no folding), and ``lo - v`` is rarely exact — what tells the two
    roundings of the contract from one."""
    return np.full(k, 0.0123456789), np.full(k, 0.0423456789)


def integer_case(k, n, d=None, seed=None):
    """Data on which every operation is exact: integers, G full."""
    d = k if d is None else d
    g = np.random.default_rng(34000 + 1000 * d + 100 * k + n % 9973 if seed is None else seed)
    x = g.integers(-2 ** 20, 2 ** 20 + 1, (d, n)).astype(np.float64)
    z = g.integers(-8, 9, (n, k)).astype(np.float64)
    G = g.integers(-8, 9, (k, k)).astype(np.float64)
    return x, spread_rows(k, d), z, G
