"""Parameter drift: what ``ParticlePDF.set_parameter_drift()`` accepts, as one ``(rows, L)`` pair.

The reference's parameters are constants of nature: its cloud moves only in the nudge of a resample
(particlepdf.py:296-305).  Here chosen parameter rows may do a Gaussian random walk between measurements,
``theta_rows += sqrt(dt) L z`` with ``L L^T = Q`` the drift covariance per unit time, and the device applies the step
(csrc/obe_drift.hip).  This module is the host side of that — the argument forms, the refusals and the factor the
library is handed —: pure NumPy, no library call, so that every refusal comes before anything reaches the device.
"""
import math

import numpy as np

from ._lib import OBE_FAST_DIMS

AT_BOUNDS = ("mask", "reflect")


def _row(row, n_dims):
    r = int(row)
    if r != row or not -n_dims <= r < n_dims:
        raise IndexError(f"rates: parameter row {row!r} out of range for {n_dims} parameters")
    return r % n_dims            # NumPy negative indexing


def _rows(rows, n_dims):
    out = [_row(r, n_dims) for r in np.atleast_1d(np.asarray(rows, dtype=object)).tolist()]
    if len(set(out)) != len(out):
        raise ValueError(f"rows: a parameter row is named twice in {out}")
    return out


def _stds(values):
    std = np.asarray(values, dtype=np.float64)
    if not np.all(np.isfinite(std)) or np.any(std < 0.0):
        raise ValueError("rates: a standard deviation must be finite and >= 0")
    return std


def normalize(rates, rows, n_dims):
    """``(rows, L)``: the drifted rows, int32 ascending, and the (K, K) lower-triangular factor of the drift
    covariance per unit time; None for ``rates=None`` (no drift).  ``rates``: a scalar or a (K,) vector of standard
    deviations per sqrt(time) (``rows``: which rows, default all of them, a vector then has one entry per row), a
    mapping row -> standard deviation (``rows`` must be None), or a (K, K) covariance of ``rows`` (default all rows;
    L = ``np.linalg.cholesky``).  A row whose standard deviation is 0 — in a matrix: whose row and column are 0 — is
    not among the K.  Rows given out of order are sorted together with their rates."""
    if rates is None:
        if rows is not None:
            raise ValueError("rows: given without rates")
        return None
    if hasattr(rates, "items"):
        if rows is not None:
            raise ValueError("rows: a mapping of rates names its rows itself")
        items = list(rates.items())
        rows, rates = [r for r, _ in items], [v for _, v in items]
        if not rows:
            return np.zeros(0, dtype=np.int32), np.zeros((0, 0))
    r = list(range(n_dims)) if rows is None else _rows(rows, n_dims)
    q = np.asarray(rates, dtype=np.float64)
    if q.ndim == 0:
        cov_l = np.diag(np.full(len(r), float(_stds(q))))
    elif q.ndim == 1:
        if q.shape[0] != len(r):
            raise ValueError(f"rates: {q.shape[0]} standard deviations for {len(r)} rows")
        cov_l = np.diag(_stds(q))
    elif q.ndim == 2 and q.shape[0] == q.shape[1]:
        if q.shape[0] != len(r):
            raise ValueError(f"rates: a {q.shape[0]} x {q.shape[0]} covariance for {len(r)} rows")
        if not np.all(np.isfinite(q)):
            raise ValueError("rates: the covariance must be finite")
        if not np.array_equal(q, q.T):
            raise ValueError("rates: the covariance is not symmetric")
        cov_l = None
    else:
        raise ValueError(f"rates: expected a scalar, a vector, a square matrix or a mapping, got shape {q.shape}")
    order = np.argsort(np.asarray(r, dtype=np.int64), kind="stable")
    r = np.asarray(r, dtype=np.int64)[order]
    if cov_l is not None:                                  # diagonal: the standard deviations themselves
        std = np.diag(cov_l)[order]
        keep = std > 0.0
        L = np.diag(std[keep])
    else:
        q = q[np.ix_(order, order)]
        keep = np.any(q != 0.0, axis=1)
        q = q[np.ix_(keep, keep)]
        try:
            L = np.linalg.cholesky(q) if q.size else np.zeros((0, 0))
        except np.linalg.LinAlgError:
            raise ValueError("rates: the covariance is not positive definite") from None
    r = r[keep]
    if r.size > OBE_FAST_DIMS:
        raise ValueError(f"rates: more than {OBE_FAST_DIMS} drifting rows (OBE_FAST_DIMS)")
    return r.astype(np.int32), np.ascontiguousarray(L, dtype=np.float64)


def check_at_bounds(at_bounds):
    if at_bounds not in AT_BOUNDS:
        raise ValueError(f"at_bounds: expected one of {AT_BOUNDS}, got {at_bounds!r}")
    return at_bounds


def check_dt(dt):
    dt = float(dt)
    if not (dt >= 0.0 and math.isfinite(dt)):
        raise ValueError(f"dt: expected a finite time step >= 0, got {dt!r}")
    return dt


def factor(L, dt):
    """G = L sqrt(dt), C-contiguous: what obe_drift_particles takes as h_factor."""
    return np.ascontiguousarray(L * math.sqrt(dt))


def settings(rates, rows, n_dims, per_update=False, at_bounds="mask"):
    """The drift of an object as a plain dict (what snapshots carry), or None."""
    at_bounds = check_at_bounds(at_bounds)
    normal = normalize(rates, rows, n_dims)
    if normal is None:
        return None
    return dict(rows=normal[0], cholesky=normal[1], per_update=bool(per_update), at_bounds=at_bounds)


def copy(drift):
    """A plain dict copy (rows as a tuple of ints), or None."""
    if drift is None:
        return None
    return dict(rows=tuple(int(r) for r in drift["rows"]), cholesky=drift["cholesky"].copy(),
                per_update=drift["per_update"], at_bounds=drift["at_bounds"])


def reflection_bounds(drift, bounds):
    """``(lower, upper)`` of the drifted rows for ``at_bounds='reflect'`` from the object's effective bounds
    (``_bounds.normalize``'s arrays, one interval per parameter row), or None: the mask's call, no reflection —
    ``at_bounds='mask'``, or no bound on any drifted row."""
    if drift["at_bounds"] != "reflect" or bounds is None:
        return None
    rows = drift["rows"]
    lower, upper = np.ascontiguousarray(bounds[0][rows]), np.ascontiguousarray(bounds[1][rows])
    if not (np.any(lower > -np.inf) or np.any(upper < np.inf)):
        return None
    return lower, upper
