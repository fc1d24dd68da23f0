"""Declarative parameter bounds: what ``OptBayesExpt.set_parameter_bounds()`` accepts, as arrays.

The reference keeps a posterior physical through one hook, ``enforce_parameter_constraints()`` (obe_base.py:401-416),
which its callers fill with a NumPy loop over the cloud: ``sigma <= 0`` (obe_noiseparam.py:57-79), any parameter
``< 0`` (demos/lockin/lockin_of_coil.py:115-133).  Here the same constraint is data — a box per parameter row — and
the device applies it (csrc/obe_common.h: outside_bounds).  This module is the host side of that: pure NumPy, no
library call, so that every refusal comes before anything reaches the device.
"""
import numpy as np

from ._lib import OBE_MAX_DIMS


def _pair(value, what, row):
    if value is None:
        return None, None
    try:
        lo, hi = value
    except (TypeError, ValueError):
        raise ValueError(f"{what} of row {row}: expected a (lower, upper) pair or None, got {value!r}") from None
    return lo, hi


def _flags(inclusive, n_dims):
    """(lower_open, upper_open) bool arrays from ``inclusive``: a bool, or per row (mapping or sequence) a bool or
    a ``(bool_lower, bool_upper)`` pair."""
    lower_open, upper_open = np.zeros(n_dims, dtype=bool), np.zeros(n_dims, dtype=bool)
    if isinstance(inclusive, (bool, np.bool_)):
        lower_open[:] = upper_open[:] = not inclusive
        return lower_open, upper_open
    items = inclusive.items() if hasattr(inclusive, "items") else enumerate(inclusive)
    if not hasattr(inclusive, "items") and len(inclusive) != n_dims:
        raise ValueError(f"inclusive: expected one entry per parameter row ({n_dims}), got {len(inclusive)}")
    for row, inc in items:
        r = _row(row, n_dims)
        if inc is None:
            continue
        lo_inc, hi_inc = (inc, inc) if isinstance(inc, (bool, np.bool_)) else inc
        lower_open[r], upper_open[r] = not lo_inc, not hi_inc
    return lower_open, upper_open


def _row(row, n_dims):
    r = int(row)
    if r != row or not -n_dims <= r < n_dims:
        raise IndexError(f"parameter row {row!r} out of range for {n_dims} parameters")
    return r % n_dims            # NumPy negative indexing


def normalize(bounds, n_dims, inclusive=True):
    """``(lower, upper, lower_open, upper_open)``, arrays of ``n_dims``, or None for no bounds.  ``bounds``: None, a
    mapping row -> ``(lower, upper)``, or a sequence of ``n_dims`` such pairs (or None); an end that is None or
    infinite is absent (lower = -inf, upper = +inf, never exclusive).  A value violates an inclusive end by
    ``v < lower`` / ``v > upper``, an exclusive (``*_open``) one by ``v <= lower`` / ``v >= upper``."""
    if bounds is None:
        return None
    lower, upper = np.full(n_dims, -np.inf), np.full(n_dims, np.inf)
    if hasattr(bounds, "items"):
        items = list(bounds.items())
    else:
        items = list(enumerate(bounds))
        if len(items) != n_dims:
            raise ValueError(f"bounds: expected one entry per parameter row ({n_dims}), got {len(items)}")
    seen = set()
    for row, value in items:
        r = _row(row, n_dims)
        if r in seen:
            raise ValueError(f"bounds: parameter row {r} is named twice")
        seen.add(r)
        lo, hi = _pair(value, "bounds", row)
        lower[r] = -np.inf if lo is None else float(lo)
        upper[r] = np.inf if hi is None else float(hi)
    lower_open, upper_open = _flags(inclusive, n_dims)
    return check(lower, upper, lower_open, upper_open)


def check(lower, upper, lower_open, upper_open):
    """The refusals of a set of bounds (ValueError), and absent ends made canonical."""
    if np.any(np.isnan(lower)) or np.any(np.isnan(upper)):
        raise ValueError("bounds: a bound is NaN")
    if np.any(lower > upper):
        raise ValueError(f"bounds: lower > upper on row(s) {np.flatnonzero(lower > upper).tolist()}")
    lower_open = lower_open & (lower > -np.inf)
    upper_open = upper_open & (upper < np.inf)
    empty = (lower == upper) & (lower_open | upper_open)
    if np.any(empty):
        raise ValueError(f"bounds: lower == upper with an exclusive end on row(s) {np.flatnonzero(empty).tolist()}")
    if np.count_nonzero((lower > -np.inf) | (upper < np.inf)) > OBE_MAX_DIMS:
        raise ValueError(f"bounds: more than {OBE_MAX_DIMS} bounded rows (OBE_MAX_DIMS)")
    return lower, upper, lower_open, upper_open


def intersect_positive(bounds, rows):
    """``bounds`` intersected with ``(0, +inf)``, lower end exclusive, on ``rows``: the noise-parameter class's own
    ``sigma > 0`` (obe_noiseparam.py:57-79) next to the user's bounds."""
    lower, upper, lower_open, upper_open = (a.copy() for a in bounds)
    for r in rows:
        if lower[r] <= 0.0:
            lower[r], lower_open[r] = 0.0, True
    return check(lower, upper, lower_open, upper_open)


def pack(bounds):
    """What the library takes: ``(rows int32, lower, upper, open int32)`` of the bounded rows only (open: bit 0 =
    lower end exclusive, bit 1 = upper end), or None if no row is bounded."""
    if bounds is None:
        return None
    lower, upper, lower_open, upper_open = bounds
    rows = np.flatnonzero((lower > -np.inf) | (upper < np.inf)).astype(np.int32)
    if rows.size == 0:
        return None
    return (rows, np.ascontiguousarray(lower[rows]), np.ascontiguousarray(upper[rows]),
            (lower_open[rows].astype(np.int32) | (upper_open[rows].astype(np.int32) << 1)).astype(np.int32))
