"""Scoring a reading, and the band of the next one, when the noise depends on the signal (OptBayesExptSignalNoise).

The predictive of a reading is still a mixture of N_p Gaussians; component i of channel c has the mean
``f_c(x; theta_i)`` and the variance ``nu_c(f_c(x; theta_i))``: every particle brings its own width, from the model
value itself.  ``_scoring.py`` and ``_reading.py`` with the object's three coefficients in sigma's place: their shapes,
their tiling (65 536 records or settings and 16 levels per library call), their checks and their unconverged-rows
warning; the kernels are csrc/obe_signal_noise.hip's (K21).  A particle contributes by the likelihood's rule: a weight
> 0 and every channel's nu > 0 and finite.  The argument checks need no device; nothing is kept on the object.
"""
import warnings

import numpy as np
import torch

from . import _lib, _reading, _scoring         # (the per-call limits are read from the two modules at every call)
from ._devcall import cloud, column_tiles, model_call, ptr as _ptr
from ._predictive import _device_model, check_settings
from ._reading import check_levels, check_max_passes, normal_quantiles
from ._scoring import check_records, pvalue_from_tails


# ------------------------------------------------------------------------------------------------- device calls
def _score(obe, entry, out_rows, n_out, settings, y_meas):
    """The ``n_out`` device results of ``entry`` (each (out_rows, n_r)) for the checked records, and ``single``."""
    coef = obe._coefficients()                               # (the attributes as they stand when the call starts)
    n_c = obe.n_channels
    x, y, _, single = check_records(settings, y_meas, None, obe.allsettings.shape[0], n_c, True)
    _device_model(obe)
    p, w = cloud(obe)
    n_r, n_p, n_s = x.shape[1], p.shape[1], x.shape[0]
    dev = obe._device
    stacked = torch.from_numpy(np.vstack([x, y])).to(dev)
    outs = [torch.empty((out_rows, n_r), dtype=torch.float64, device=dev) for _ in range(n_out)]
    for start, part in column_tiles(stacked, _scoring.RECORDS_PER_CALL):
        n = part.shape[1]
        d_out = [torch.empty((out_rows, n), dtype=torch.float64, device=dev) for _ in range(n_out)]
        model_call(obe, entry, "obe_predictive_score_workspace_bytes", (n_p, n, n_c),
                   _ptr(part), n, n, _ptr(part[n_s:]), n, _lib.host_ptr(coef), _ptr(p), n_p, n_p, _ptr(w),
                   *[_ptr(t) for t in d_out])
        for whole, piece in zip(outs, d_out):
            whole[:, start:start + n] = piece
    return [t.cpu().numpy() for t in outs], single


def signal_logpdf(obe, settings, y_meas):
    (logp,), single = _score(obe, "obe_signal_noise_logpdf", 1, 1, settings, y_meas)
    return float(logp[0, 0]) if single else logp[0]


def signal_tails(obe, settings, y_meas):
    """``(lower, upper)``, each ``(C, n_r)``."""
    (lower, upper), _ = _score(obe, "obe_signal_noise_tails", obe.n_channels, 2, settings, y_meas)
    return lower, upper


def signal_cdf(obe, settings, y_meas, upper=False):
    return signal_tails(obe, settings, y_meas)[1 if upper else 0]


def signal_pvalue(obe, settings, y_meas):
    return pvalue_from_tails(*signal_tails(obe, settings, y_meas))


def signal_quantile(obe, q, settings=None, max_passes=48, full_output=False):
    coef = obe._coefficients()                               # (the attributes as they stand when the call starts)
    qs, scalar = check_levels(q)
    max_passes = check_max_passes(max_passes)
    n_c = obe.n_channels
    x = None if settings is None else check_settings(settings, obe.allsettings.shape[0])
    _device_model(obe)
    zs = normal_quantiles(qs)
    dev = obe._device
    x = obe._settings_dev if x is None else torch.from_numpy(x).to(dev)      # (the whole design grid, sharded or not)
    p, w = cloud(obe)
    n_x, n_p = x.shape[1], p.shape[1]
    out = np.empty((qs.size, n_c, n_x))
    passes = np.empty((qs.size, n_c, n_x), dtype=np.int32)
    for q0 in range(0, qs.size, _reading.MAX_Q_PER_CALL):
        part_q = np.ascontiguousarray(qs[q0:q0 + _reading.MAX_Q_PER_CALL])
        part_z = np.ascontiguousarray(zs[q0:q0 + _reading.MAX_Q_PER_CALL])
        for start, part in column_tiles(x, _reading.SETTINGS_PER_CALL):
            n = part.shape[1]
            d_out = torch.empty((part_q.size, n_c, n), dtype=torch.float64, device=dev)
            d_passes = torch.empty((part_q.size, n_c, n), dtype=torch.int32, device=dev)
            model_call(obe, "obe_signal_noise_reading_quantiles", "obe_predictive_reading_workspace_bytes",
                       (n_p, n, n_c, part_q.size), _ptr(part), n, n, _lib.host_ptr(coef), _ptr(p), n_p, n_p,
                       _ptr(w), _lib.host_ptr(part_q), _lib.host_ptr(part_z), part_q.size, max_passes, _ptr(d_out),
                       _ptr(d_passes))
            out[q0:q0 + part_q.size, :, start:start + n] = d_out.cpu().numpy()
            passes[q0:q0 + part_q.size, :, start:start + n] = d_passes.cpu().numpy()
    unconverged = int(np.count_nonzero(passes < 0))
    if unconverged:
        warnings.warn(f"signal_quantile: {unconverged} of {passes.size} results were still open after {max_passes} "
                      "passes and are the midpoints of their brackets", RuntimeWarning, stacklevel=3)
    if scalar:
        out, passes = out[0], passes[0]
    return (out, {"passes": passes, "unconverged": unconverged}) if full_output else out


def signal_interval(obe, level=0.95, settings=None, max_passes=48, full_output=False):
    try:
        level = float(level)
    except (TypeError, ValueError):
        raise ValueError(f"level must be a number in (0, 1), got {level!r}") from None
    if not 0.0 < level < 1.0:
        raise ValueError(f"level must lie in the open interval (0, 1), got {level!r}")
    got = signal_quantile(obe, ((1.0 - level) / 2.0, (1.0 + level) / 2.0), settings, max_passes, full_output)
    if full_output:
        return got[0][0], got[0][1], got[1]
    return got[0], got[1]
