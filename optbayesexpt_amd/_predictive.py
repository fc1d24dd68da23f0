"""Posterior predictive summaries computed where the cloud lives: the model curve's mean, spread and credible band.

The reference's demos draw the model at the mean parameters (demos/line_plus_noise/line_plus_noise.py:138,181): a
plug-in estimate without a band.  The weighted mean, standard deviation and quantiles of ``model(x; theta_i)`` over
the whole cloud take settings x particles evaluations; they are HIP kernels (csrc/obe_predict.hip) and only the
``(C, n_x)`` results travel.  The argument checks are plain functions of this module (no device needed), the calls
are tiled over the settings (the library tiles the quantiles once more, 64 rows of model values at a time), so that no
workspace grows with the request; ``OptBayesExpt`` has the methods.
"""
import ctypes

import numpy as np

from . import _posterior

MAX_Q_PER_CALL = _posterior.MAX_Q_PER_CALL     # obe_predictive_quantiles: values of q one call serves
SETTINGS_PER_CALL = 1 << 16                    # settings one library call is given (its results: C x n_q x 512 KiB)
_P = ctypes.c_void_p


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
def _ptr(t):
    return _P(t.data_ptr())


def _inputs(obe, settings):
    """(device settings (n_setdims, n_x), particles, weights); host edits of the cloud are uploaded here."""
    import torch
    if settings is None:
        x = obe._settings_dev          # the whole design grid, on a sharded object too
    else:
        x = torch.from_numpy(check_settings(settings, obe.allsettings.shape[0])).to(obe._device)
    p, w = obe._parameters.tensor(), obe._weights.tensor()
    if p.shape[1] != w.shape[0]:
        raise ValueError("particles and particle_weights have different lengths")
    return x, p, w


def _workspace(obe, n_particles, n_settings, n_q):
    """A workspace of the call's own: the object's workspace keeps the record of a sweep enqueued ahead."""
    import torch
    nbytes = int(obe._mlib.cdll.obe_predictive_workspace_bytes(n_particles, n_settings, obe.n_channels, n_q))
    return torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=obe._device), nbytes


def _column_tiles(x, per_call):
    """Contiguous (n_setdims, <= per_call) pieces of the settings with their first column."""
    n_x = x.shape[1]
    if n_x <= per_call:
        yield 0, x
        return
    for start in range(0, n_x, per_call):
        yield start, x[:, start:start + per_call].contiguous()


def predict(obe, settings=None):
    import torch
    _device_model(obe)
    x, p, w = _inputs(obe, settings)
    n_x, n_p = x.shape[1], p.shape[1]
    mean = torch.empty((obe.n_channels, n_x), dtype=torch.float64, device=obe._device)
    var = torch.empty_like(mean)
    for start, part in _column_tiles(x, SETTINGS_PER_CALL):
        n = part.shape[1]
        d_mean = torch.empty((obe.n_channels, n), dtype=torch.float64, device=obe._device)
        d_var = torch.empty_like(d_mean)
        ws, ws_bytes = _workspace(obe, n_p, n, 0)
        obe._mlib.call("obe_predictive_moments", obe._model_struct, _ptr(part), n, n, _ptr(p), n_p, n_p, _ptr(w),
                       _ptr(d_mean), _ptr(d_var), _ptr(ws), ws_bytes, obe._stream())
        mean[:, start:start + n] = d_mean
        var[:, start:start + n] = d_var
    return mean.cpu().numpy(), torch.sqrt(torch.clamp(var, min=0.0)).cpu().numpy()


def predictive_quantile(obe, q, settings=None):
    import torch
    from . import _lib
    qs, scalar = _posterior.check_q(q)
    _device_model(obe)
    x, p, w = _inputs(obe, settings)
    n_x, n_p, n_c = x.shape[1], p.shape[1], obe.n_channels
    out = np.empty((qs.size, n_c, n_x))
    for q0 in range(0, qs.size, MAX_Q_PER_CALL):
        part_q = np.ascontiguousarray(qs[q0:q0 + MAX_Q_PER_CALL])
        for start, part in _column_tiles(x, SETTINGS_PER_CALL):
            n = part.shape[1]
            d_out = torch.empty((part_q.size, n_c, n), dtype=torch.float64, device=obe._device)
            ws, ws_bytes = _workspace(obe, n_p, n, part_q.size)
            obe._mlib.call("obe_predictive_quantiles", obe._model_struct, _ptr(part), n, n, _ptr(p), n_p, n_p, _ptr(w),
                           _lib.host_ptr(part_q), part_q.size, _ptr(d_out), _ptr(ws), ws_bytes, obe._stream())
            out[q0:q0 + part_q.size, :, start:start + n] = d_out.cpu().numpy()
    return out[0] if scalar else out


def predictive_interval(obe, level=0.95, settings=None):
    lo, hi = predictive_quantile(obe, _posterior.interval_quantiles(level), settings)
    return lo, hi
