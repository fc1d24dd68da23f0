"""Where will the next reading fall?  Quantiles of the posterior predictive of a MEASUREMENT, noise included.

``predictive_interval()`` is a credible band of the model curve alone, so measured points do not fall inside it;
``predictive_cdf()`` scores a reading that has been taken.  This is its inverse: for a setting, a channel and a level q
the y with ``P(Y_c <= y) = q`` under ``sum_i w_i N(y; f_c(x; theta_i), sigma_c,i) / sum_i w_i`` — the band to draw
against data, an outlier threshold fixed before the reading is taken, the range to set on an instrument.  Inverting a
mixture of N_p Gaussians takes settings x particles evaluations per step; the bracket, the safeguarded Newton steps
and their bookkeeping are HIP kernels (csrc/obe_predict.hip, K15), a fixed budget of passes is enqueued and only the
``(n_q, C, n_x)`` results travel.  The argument checks are plain functions of this module (no device needed), the
calls are tiled over the settings and the levels; ``OptBayesExpt`` has the methods.  The band is per channel, not
joint, and nothing is kept on the object.
"""
import statistics
import warnings

import numpy as np
import torch

from . import _lib
from ._devcall import cloud, column_tiles, model_call, ptr as _ptr
from ._predictive import _device_model, check_settings
from ._scoring import _noise_rows, check_sigma

MAX_Q_PER_CALL = 16                            # obe_predictive_reading_quantiles: levels one call serves
SETTINGS_PER_CALL = 1 << 16                    # settings one library call is given
MAX_PASSES = 64                                # ... and the largest pass budget it takes
_NORMAL = statistics.NormalDist()


# ---------------------------------------------------------------------------------------- argument checks (host)
def check_levels(q):
    """(float64 vector of q, whether q was a scalar); every q in the OPEN interval (0, 1)."""
    try:
        arr = np.asarray(q, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"q must be a number or a sequence of numbers in (0, 1), got {q!r}") from None
    if arr.ndim > 1 or arr.size == 0:
        raise ValueError("q must be a scalar or a non-empty one-dimensional sequence")
    if not np.all((arr > 0.0) & (arr < 1.0)):            # (NaN fails both comparisons)
        raise ValueError("the levels of a reading's quantiles must lie in the open interval (0, 1)")
    return np.ascontiguousarray(arr.reshape(-1)), arr.ndim == 0


def normal_quantiles(qs):
    """The standard normal quantile of every level, from the tail the level is small in (1 - q is exact for
    q > 1/2)."""
    return np.array([_NORMAL.inv_cdf(q) if q <= 0.5 else -_NORMAL.inv_cdf(1.0 - q) for q in map(float, qs)])


def check_max_passes(max_passes):
    if isinstance(max_passes, bool) or not isinstance(max_passes, (int, np.integer)) or not 1 <= max_passes <= MAX_PASSES:
        raise ValueError(f"max_passes must be an integer in 1..{MAX_PASSES}, got {max_passes!r}")
    return int(max_passes)


def check_request(settings, sigma, n_setdims, n_channels, noise_rows, n_grid):
    """``(x (n_setdims, n_x) or None for the design grid, sigma (C, n_x) or None)``.  ``noise_rows``: the object takes
    sigma from its cloud (None: it does not); ``n_grid``: the points of the design grid."""
    if noise_rows is None and sigma is None:
        raise ValueError("sigma is required: the measurement noise of the reading(s), a scalar, (C,) or (C, n_x)")
    if noise_rows is not None and sigma is not None:
        raise ValueError("this object takes sigma from its noise parameter(s): call without sigma")
    x = None if settings is None else check_settings(settings, n_setdims)
    n_x = n_grid if x is None else x.shape[1]
    if sigma is None:
        return x, None
    s = check_sigma(sigma, n_channels)
    if s.shape[1] not in (1, n_x):
        raise ValueError(f"sigma has {s.shape[1]} columns for {n_x} setting points")
    return x, np.array(np.broadcast_to(s, (n_channels, n_x)), order="C")          # (a copy: writable, contiguous)


# ------------------------------------------------------------------------------------------------- device calls
def reading_quantile(obe, q, settings=None, sigma=None, max_passes=48, full_output=False):
    _device_model(obe)
    qs, scalar = check_levels(q)
    max_passes = check_max_passes(max_passes)
    rows = _noise_rows(obe)
    n_c = obe.n_channels
    x, s = check_request(settings, sigma, obe.allsettings.shape[0], n_c, rows, obe.allsettings.shape[1])
    zs = normal_quantiles(qs)
    dev = obe._device
    x = obe._settings_dev if x is None else torch.from_numpy(x).to(dev)      # (the whole design grid, sharded or not)
    p, w = cloud(obe)
    n_s, n_x, n_p = x.shape[0], x.shape[1], p.shape[1]
    if s is not None:
        if s.shape[1] != n_x:
            raise ValueError(f"sigma has {s.shape[1]} columns for {n_x} setting points")
        x = torch.cat([x, torch.from_numpy(s).to(dev)])
    out = np.empty((qs.size, n_c, n_x))
    passes = np.empty((qs.size, n_c, n_x), dtype=np.int32)
    for q0 in range(0, qs.size, MAX_Q_PER_CALL):
        part_q = np.ascontiguousarray(qs[q0:q0 + MAX_Q_PER_CALL])
        part_z = np.ascontiguousarray(zs[q0:q0 + MAX_Q_PER_CALL])
        for start, part in column_tiles(x, SETTINGS_PER_CALL):
            n = part.shape[1]
            d_out = torch.empty((part_q.size, n_c, n), dtype=torch.float64, device=dev)
            d_passes = torch.empty((part_q.size, n_c, n), dtype=torch.int32, device=dev)
            model_call(obe, "obe_predictive_reading_quantiles", "obe_predictive_reading_workspace_bytes",
                       (n_p, n, n_c, part_q.size), _ptr(part), n, n, None if s is None else _ptr(part[n_s:]), n,
                       None if rows is None else _lib.host_ptr(rows), _ptr(p), n_p, n_p, _ptr(w),
                       _lib.host_ptr(part_q), _lib.host_ptr(part_z), part_q.size, max_passes, _ptr(d_out),
                       _ptr(d_passes))
            out[q0:q0 + part_q.size, :, start:start + n] = d_out.cpu().numpy()
            passes[q0:q0 + part_q.size, :, start:start + n] = d_passes.cpu().numpy()
    unconverged = int(np.count_nonzero(passes < 0))
    if unconverged:
        warnings.warn(f"reading_quantile: {unconverged} of {passes.size} results were still open after {max_passes} "
                      "passes and are the midpoints of their brackets", RuntimeWarning, stacklevel=3)
    if scalar:
        out, passes = out[0], passes[0]
    return (out, {"passes": passes, "unconverged": unconverged}) if full_output else out


def reading_interval(obe, level=0.95, settings=None, sigma=None, max_passes=48, full_output=False):
    try:
        level = float(level)
    except (TypeError, ValueError):
        raise ValueError(f"level must be a number in (0, 1), got {level!r}") from None
    if not 0.0 < level < 1.0:
        raise ValueError(f"level must lie in the open interval (0, 1), got {level!r}")
    got = reading_quantile(obe, ((1.0 - level) / 2.0, (1.0 + level) / 2.0), settings, sigma, max_passes, full_output)
    if full_output:
        return got[0][0], got[0][1], got[1]
    return got[0], got[1]
