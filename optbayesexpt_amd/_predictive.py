"""Posterior predictive summaries computed where the cloud lives: the model curve's mean, spread and credible band.

The reference's demos draw the model at the mean parameters (demos/line_plus_noise/line_plus_noise.py:138,181): a
plug-in estimate without a band.  The weighted mean, standard deviation and quantiles of ``model(x; theta_i)`` over
the whole cloud take settings x particles evaluations; they are HIP kernels (csrc/obe_predict.hip) and only the
``(C, n_x)`` results travel.  The argument checks are plain functions of this module (no device needed), the calls
are tiled over the settings (the library tiles the quantiles once more, 64 rows of model values at a time), so that no
workspace grows with the request; ``OptBayesExpt`` has the methods.
"""
import numpy as np
import torch

from . import _lib, _posterior
from ._devcall import cloud, column_tiles, model_call, ptr as _ptr

MAX_Q_PER_CALL = _posterior.MAX_Q_PER_CALL     # obe_predictive_quantiles: values of q one call serves
SETTINGS_PER_CALL = 1 << 16                    # settings one library call is given (its results: C x n_q x 512 KiB)
_WORKSPACE = "obe_predictive_workspace_bytes"


# ---------------------------------------------------------------------------------------- argument checks (host)
def check_settings(settings, n_setdims):
    """``(n_setdims, n_x)`` float64 points from a tuple of ``n_setdims`` scalars or 1-D arrays (broadcast to one
    length: points, not meshgrid axes) or an ``(n_setdims, n_x)`` array."""
    try:
        rows = list(settings)
    except TypeError:
        raise ValueError(f"settings must be a tuple of {n_setdims} scalars or 1-D arrays, or an "
                         f"({n_setdims}, n_x) array, got {settings!r}") from None
    if len(rows) != n_setdims:
        raise ValueError(f"the model takes {n_setdims} setting(s), got {len(rows)}")
    try:
        rows = [np.asarray(r, dtype=np.float64) for r in rows]
    except (TypeError, ValueError):
        raise ValueError("settings must be numbers") from None
    if any(r.ndim > 1 for r in rows):
        raise ValueError("each setting must be a scalar or a one-dimensional array of points")
    try:
        rows = np.broadcast_arrays(*[r.reshape(-1) for r in rows])
    except ValueError:
        raise ValueError("the settings do not broadcast to one number of points") from None
    out = np.ascontiguousarray(np.stack(rows), dtype=np.float64)
    if out.shape[1] == 0:
        raise ValueError("settings must hold at least one point")
    return out


def _device_model(obe):
    if obe._device_model is None:
        raise TypeError("the posterior predictive summaries evaluate the model on the device: pass a device model "
                        "(models.from_function / models.from_expression turn a formula into one), not a plain "
                        "Python model_function")


# ------------------------------------------------------------------------------------------------- device calls
def _inputs(obe, settings):
    """(device settings (n_setdims, n_x), particles, weights); host edits of the cloud are uploaded here."""
    if settings is None:
        x = obe._settings_dev          # the whole design grid, on a sharded object too
    else:
        x = torch.from_numpy(check_settings(settings, obe.allsettings.shape[0])).to(obe._device)
    return (x,) + cloud(obe)


def moments(obe, x, p, w):
    """Device ``(mean, var)`` of the model output over the cloud, each ``(C, n_x)``, for device settings ``x``."""
    n_x, n_p, n_c, dev = x.shape[1], p.shape[1], obe.n_channels, obe._device
    mean = torch.empty((n_c, n_x), dtype=torch.float64, device=dev)
    var = torch.empty_like(mean)
    for start, part in column_tiles(x, SETTINGS_PER_CALL):
        n = part.shape[1]
        d_mean = torch.empty((n_c, n), dtype=torch.float64, device=dev)
        d_var = torch.empty_like(d_mean)
        model_call(obe, "obe_predictive_moments", _WORKSPACE, (n_p, n, n_c, 0),
                   _ptr(part), n, n, _ptr(p), n_p, n_p, _ptr(w), _ptr(d_mean), _ptr(d_var))
        mean[:, start:start + n] = d_mean
        var[:, start:start + n] = d_var
    return mean, var


def predict(obe, settings=None):
    _device_model(obe)
    mean, var = moments(obe, *_inputs(obe, settings))
    return mean.cpu().numpy(), torch.sqrt(torch.clamp(var, min=0.0)).cpu().numpy()


def predictive_quantile(obe, q, settings=None):
    qs, scalar = _posterior.check_q(q)
    _device_model(obe)
    x, p, w = _inputs(obe, settings)
    n_x, n_p, n_c = x.shape[1], p.shape[1], obe.n_channels
    out = np.empty((qs.size, n_c, n_x))
    for q0 in range(0, qs.size, MAX_Q_PER_CALL):
        part_q = np.ascontiguousarray(qs[q0:q0 + MAX_Q_PER_CALL])
        for start, part in column_tiles(x, SETTINGS_PER_CALL):
            n = part.shape[1]
            d_out = torch.empty((part_q.size, n_c, n), dtype=torch.float64, device=obe._device)
            model_call(obe, "obe_predictive_quantiles", _WORKSPACE, (n_p, n, n_c, part_q.size),
                       _ptr(part), n, n, _ptr(p), n_p, n_p, _ptr(w), _lib.host_ptr(part_q), part_q.size, _ptr(d_out))
            out[q0:q0 + part_q.size, :, start:start + n] = d_out.cpu().numpy()
    return out[0] if scalar else out


def predictive_interval(obe, level=0.95, settings=None):
    lo, hi = predictive_quantile(obe, _posterior.interval_quantiles(level), settings)
    return lo, hi
