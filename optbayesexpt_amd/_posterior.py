"""Posterior summaries computed where the cloud lives: marginal and joint histograms, quantiles, credible intervals.

The reference's users read these from the whole cloud (the weighted scatter plots of demos/pipulse/pipulse.py:159 and
demos/find_peak/seqLor_pdfevolve.py:156-163, the histograms of docs/manual_demos.rst); here ``particles`` and
``particle_weights`` are device arrays whose host mirrors cost a copy of the whole cloud, so the summaries are HIP
kernels (csrc/obe_posterior.hip) and only the few result values travel.  The argument checks are plain functions of
this module (no device needed); ``ParticlePDF`` has the methods.
"""
import numpy as np
import torch

from . import _lib
from ._devcall import P as _P, ptr as _ptr, workspace

MAX_Q_PER_CALL = 16          # obe_weighted_quantiles: values of q one call serves (more are served in groups)
MAX_BINS = 1 << 24           # bins one call fills, all rows together


# ---------------------------------------------------------------------------------------- argument checks (host)
def _as_int(value, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{what} must be an integer, got {value!r}")
    return int(value)


def check_bins(bins):
    """The number of equal-width bins of a marginal: an integer >= 1."""
    bins = _as_int(bins, "bins")
    if bins < 1:
        raise ValueError("`bins` must be positive, when an integer")
    if bins > MAX_BINS:
        raise ValueError(f"at most {MAX_BINS} bins per call are supported on the device, got {bins}")
    return bins


def check_bins2(bins):
    """(bins_x, bins_y) of a joint histogram from an integer or a pair of integers."""
    if isinstance(bins, (int, np.integer)) and not isinstance(bins, (bool, np.bool_)):
        bx = by = check_bins(bins)
    else:
        try:
            bx, by = bins
        except (TypeError, ValueError):
            raise ValueError(f"bins must be an integer or a pair of integers, got {bins!r}") from None
        bx, by = check_bins(bx), check_bins(by)
    if bx * by > MAX_BINS:
        raise ValueError(f"at most {MAX_BINS} bins per call are supported on the device, got {bx} x {by}")
    return bx, by


def check_q(q):
    """(float64 vector of q, whether q was a scalar); every q in [0, 1]."""
    try:
        arr = np.asarray(q, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"q must be a number or a sequence of numbers in [0, 1], got {q!r}") from None
    if arr.ndim > 1 or arr.size == 0:
        raise ValueError("q must be a scalar or a non-empty one-dimensional sequence")
    if not np.all((arr >= 0.0) & (arr <= 1.0)):          # (NaN fails both comparisons)
        raise ValueError("Quantiles must be in the range [0, 1]")
    return np.ascontiguousarray(arr.reshape(-1)), arr.ndim == 0


def check_level(level):
    """The probability content of a credible interval, in [0, 1]."""
    try:
        level = float(level)
    except (TypeError, ValueError):
        raise ValueError(f"level must be a number in [0, 1], got {level!r}") from None
    if not 0.0 <= level <= 1.0:
        raise ValueError(f"level must be in [0, 1], got {level!r}")
    return level


def check_dims(dims, n_dims):
    """int32 vector of parameter rows: ``None`` = every row, an integer = that row, else a sequence of rows."""
    if dims is None:
        return np.arange(n_dims, dtype=np.int32)
    try:
        seq = [dims] if np.ndim(dims) == 0 else list(dims)
    except TypeError:
        raise ValueError(f"dims must be None, a row index or a sequence of row indices, got {dims!r}") from None
    if not seq:
        raise ValueError("dims must name at least one parameter row")
    rows = [_as_int(d, "a dimension") for d in seq]
    for d in rows:
        if not 0 <= d < n_dims:
            raise ValueError(f"dimension {d} is out of range for a cloud of {n_dims} parameter rows")
    return np.asarray(rows, dtype=np.int32)


def _check_pair(pair):
    try:
        lo, hi = pair
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"range must be (min, max), got {pair!r}") from None
    if lo > hi:
        raise ValueError("max must be larger than min in range parameter.")
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"supplied range of [{lo}, {hi}] is not finite")
    return lo, hi


def check_range(range_, n_rows):
    """``None``, or one (min, max) per row: a single pair serves every row, else a sequence of ``n_rows`` pairs."""
    if range_ is None:
        return None
    try:
        items = list(range_)
    except TypeError:
        raise ValueError(f"range must be (min, max) or one (min, max) per row, got {range_!r}") from None
    if len(items) == 2 and all(np.ndim(x) == 0 for x in items):
        return [_check_pair(items)] * n_rows
    if len(items) != n_rows:
        raise ValueError(f"range must be (min, max) or one (min, max) for each of the {n_rows} rows")
    return [_check_pair(x) for x in items]


def bin_edges(lo, hi, bins):
    """``np.histogram_bin_edges(row, bins, (lo, hi))`` — NumPy's own edges for that range, a constant row's
    (x - 0.5, x + 0.5) included; the data do not enter once the range is known."""
    return np.histogram_bin_edges(np.empty(0), bins, (lo, hi))


def interval_quantiles(level):
    """The two q of the equal-tailed interval of probability content ``level``."""
    level = check_level(level)
    return (1.0 - level) / 2.0, 1.0 - (1.0 - level) / 2.0


# ------------------------------------------------------------------------------------------------- device calls
def _workspace(pdf, n_rows, n_bins, n_q):
    return workspace(pdf._lib, pdf._device, "obe_posterior_workspace_bytes", pdf.n_particles, n_rows, n_bins, n_q)


def _auto_ranges(pdf, p, rows):
    out = torch.empty(2 * len(rows), dtype=torch.float64, device=pdf._device)
    ws, ws_bytes = _workspace(pdf, len(rows), 0, 0)
    pdf._lib.call("obe_minmax_rows", _ptr(p), p.shape[1], pdf.n_dims, pdf.n_particles, _lib.host_ptr(rows), len(rows),
                  _ptr(out), _ptr(ws), ws_bytes, pdf._stream())
    mm = out.cpu().numpy().reshape(len(rows), 2)
    for lo, hi in mm:
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError(f"autodetected range of [{lo}, {hi}] is not finite")
    return [(float(lo), float(hi)) for lo, hi in mm]


def marginal_histogram(pdf, dims=None, bins=64, range=None, density=False):
    rows = check_dims(dims, pdf.n_dims)
    bins = check_bins(bins)
    ranges = check_range(range, len(rows))
    if len(rows) * bins > MAX_BINS:
        raise ValueError(f"at most {MAX_BINS} bins per call are supported on the device, got {len(rows)} x {bins}")
    p, w = pdf._pw_tensors()
    if ranges is None:
        ranges = _auto_ranges(pdf, p, rows)
    edges = np.stack([bin_edges(lo, hi, bins) for lo, hi in ranges])
    d_edges = torch.from_numpy(edges).to(pdf._device)
    d_mass = torch.empty((len(rows), bins), dtype=torch.float64, device=pdf._device)
    ws, ws_bytes = _workspace(pdf, len(rows), bins, 0)
    pdf._lib.call("obe_weighted_histogram", _ptr(p), p.shape[1], pdf.n_dims, pdf.n_particles, _ptr(w),
                  _lib.host_ptr(rows), len(rows), _ptr(d_edges), bins, _ptr(d_mass), _ptr(ws), ws_bytes, pdf._stream())
    mass = d_mass.cpu().numpy()
    if density:           # np.histogram: n / db / n.sum()
        mass = np.stack([m / np.diff(e) / m.sum() for m, e in zip(mass, edges)])
    return mass, edges


def joint_histogram(pdf, dim_x, dim_y, bins=64, range=None, density=False):
    rows = check_dims([dim_x, dim_y], pdf.n_dims)
    bx, by = check_bins2(bins)
    ranges = check_range(range, 2)
    if range is not None and np.ndim(list(range)[0]) == 0:
        raise ValueError("range of a joint histogram must be ((xmin, xmax), (ymin, ymax))")
    p, w = pdf._pw_tensors()
    if ranges is None:
        ranges = _auto_ranges(pdf, p, rows)
    xedges, yedges = bin_edges(*ranges[0], bx), bin_edges(*ranges[1], by)
    d_edges = torch.from_numpy(np.concatenate([xedges, yedges])).to(pdf._device)
    d_mass = torch.empty((bx, by), dtype=torch.float64, device=pdf._device)
    ws, ws_bytes = _workspace(pdf, 1, bx * by, 0)
    pdf._lib.call("obe_weighted_histogram2d", _ptr(p), p.shape[1], pdf.n_dims, pdf.n_particles, _ptr(w), int(rows[0]),
                  int(rows[1]), _ptr(d_edges), bx, _P(d_edges.data_ptr() + 8 * (bx + 1)), by, _ptr(d_mass), _ptr(ws),
                  ws_bytes, pdf._stream())
    mass = d_mass.cpu().numpy()
    if density:           # np.histogramdd: divided by the bin widths axis by axis, then by the total
        s = mass.sum()
        mass = mass / np.diff(xedges).reshape(bx, 1)
        mass = mass / np.diff(yedges).reshape(1, by)
        mass /= s
    return mass, xedges, yedges


def quantile(pdf, q, dims=None):
    qs, scalar = check_q(q)
    rows = check_dims(dims, pdf.n_dims)
    p, w = pdf._pw_tensors()
    out = np.empty((len(rows), qs.size))
    for start in np.arange(0, qs.size, MAX_Q_PER_CALL):
        part = np.ascontiguousarray(qs[start:start + MAX_Q_PER_CALL])
        d_out = torch.empty((len(rows), part.size), dtype=torch.float64, device=pdf._device)
        ws, ws_bytes = _workspace(pdf, len(rows), 0, part.size)
        pdf._lib.call("obe_weighted_quantiles", _ptr(p), p.shape[1], pdf.n_dims, pdf.n_particles, _ptr(w),
                      _lib.host_ptr(rows), len(rows), _lib.host_ptr(part), part.size, _ptr(d_out), _ptr(ws), ws_bytes,
                      pdf._stream())
        out[:, start:start + part.size] = d_out.cpu().numpy()
    return out[:, 0] if scalar else out
