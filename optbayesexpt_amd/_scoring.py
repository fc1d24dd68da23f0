"""Scoring a measurement against the posterior predictive, where the cloud lives: is this reading plausible?

``predict()`` and ``predictive_interval()`` summarise the model curve alone; a reading carries its noise too.  Its
density ``p(y | x, data) = sum_i w_i prod_c N(y_c; f_c(x; theta_i), sigma_c,i) / sum_i w_i`` (for the record about to
be used: the one-step model evidence) and the per-channel tail probabilities ``P(Y_c <= y_c)``, ``P(Y_c >= y_c)`` take
records x particles evaluations; they are HIP kernels (csrc/obe_predict.hip, K11) and only the ``(n_r,)`` or
``(C, n_r)`` results travel.  The argument checks are plain functions of this module (no device needed), the calls are
tiled over the records so that no workspace grows with the request; ``OptBayesExpt`` has the methods.
"""
import numpy as np
import torch

from . import _lib
from ._devcall import cloud, column_tiles, model_call, ptr as _ptr
from ._predictive import _device_model, check_settings

RECORDS_PER_CALL = 1 << 16                     # records one library call is given


# ---------------------------------------------------------------------------------------- argument checks (host)
def _numbers(value, what):
    try:
        a = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be numbers, got {value!r}") from None
    if a.ndim > 2:
        raise ValueError(f"{what} has {a.ndim} dimensions: at most (n_channels, n_records)")
    return a


def check_y_meas(y_meas, n_channels):
    """``((C, n_r) float64, single)``: a scalar or ``(n_r,)`` for one channel, ``(C,)`` for one record of a C-channel
    model, else ``(C, n_r)``; all C channels are required.  ``single``: one record given without a record axis."""
    if y_meas is None:
        raise ValueError("y_meas is required")
    a = _numbers(y_meas, "y_meas")
    single = a.ndim == 0 or (a.ndim == 1 and n_channels > 1)
    if a.ndim == 0 or (a.ndim == 1 and n_channels == 1):
        if n_channels != 1:
            raise ValueError(f"the model has {n_channels} channels: y_meas must be ({n_channels},) or "
                             f"({n_channels}, n_records)")
        a = a.reshape(1, -1)
    elif a.ndim == 1:
        if a.size != n_channels:
            raise ValueError(f"the model has {n_channels} channels, y_meas has {a.size} values")
        a = a.reshape(n_channels, 1)
    elif a.shape[0] != n_channels:
        raise ValueError(f"the model has {n_channels} channels, y_meas has {a.shape[0]} rows")
    if a.shape[1] == 0:
        raise ValueError("y_meas must hold at least one record")
    return a, single


def check_sigma(sigma, n_channels):
    """``(C, 1)`` or ``(C, n_r)`` float64 from a scalar, ``(C,)`` (for one channel also ``(n_r,)``) or ``(C, n_r)``;
    every value finite and > 0."""
    a = _numbers(sigma, "sigma")
    if a.ndim == 0:
        a = np.full((n_channels, 1), float(a))
    elif a.ndim == 1 and n_channels == 1:
        a = a.reshape(1, -1)
    elif a.ndim == 1:
        if a.size != n_channels:
            raise ValueError(f"the model has {n_channels} channels, sigma has {a.size} values")
        a = a.reshape(n_channels, 1)
    elif a.shape[0] != n_channels:
        raise ValueError(f"the model has {n_channels} channels, sigma has {a.shape[0]} rows")
    if a.shape[1] == 0:
        raise ValueError("sigma must hold at least one value")
    if not np.all(np.isfinite(a) & (a > 0.0)):
        raise ValueError("sigma must be finite and > 0")
    return a


def check_records(settings, y_meas, sigma, n_setdims, n_channels, noise_rows):
    """``(x (n_setdims, n_r), y (C, n_r), sigma (C, n_r) or None, single)``, everything broadcast to one ``n_r``.
    ``noise_rows``: the object takes sigma from its cloud (None: it does not).  ``single``: one record, given as
    ``pdf_update`` takes it (scalar settings, no record axis in ``y_meas``)."""
    if noise_rows is None and sigma is None:
        raise ValueError("sigma is required: the measurement noise of the record(s), a scalar, (C,) or (C, n_records)")
    if noise_rows is not None and sigma is not None:
        raise ValueError("this object takes sigma from its noise parameter(s), and its likelihood ignores a record's "
                         "sigma: call without sigma")
    x = check_settings(settings, n_setdims)
    y, single = check_y_meas(y_meas, n_channels)
    try:
        single = single and all(np.ndim(r) == 0 for r in settings)
    except TypeError:
        single = False
    s = None if sigma is None else check_sigma(sigma, n_channels)
    lengths = {a.shape[1] for a in (x, y, s) if a is not None} - {1}
    if len(lengths) > 1:
        raise ValueError(f"settings, y_meas and sigma do not broadcast to one number of records: {sorted(lengths)}")
    n_r = lengths.pop() if lengths else 1

    def wide(a):
        return np.ascontiguousarray(np.broadcast_to(a, (a.shape[0], n_r)))
    return wide(x), wide(y), None if s is None else wide(s), single and n_r == 1


def pvalue_from_tails(lower, upper):
    """Two-sided p-value per channel: ``2 min(lower, upper)``, clipped to 1."""
    return np.minimum(2.0 * np.minimum(lower, upper), 1.0)


# ------------------------------------------------------------------------------------------------- device calls
def _noise_rows(obe):
    rows = getattr(obe, "_noise_rows", None)
    return None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)


def _score(obe, entry, n_out, settings, y_meas, sigma):
    """The ``n_out`` device results of ``entry`` (each (rows, n_r)) for the checked records, and ``single``."""
    _device_model(obe)
    rows = _noise_rows(obe)
    n_c = obe.n_channels
    x, y, s, single = check_records(settings, y_meas, sigma, obe.allsettings.shape[0], n_c, rows)
    p, w = cloud(obe)
    n_r, n_p = x.shape[1], p.shape[1]
    dev = obe._device
    stacked = torch.from_numpy(np.vstack([x, y] + ([] if s is None else [s]))).to(dev)
    n_s = x.shape[0]
    out_rows = 1 if entry == "obe_predictive_logpdf" else n_c
    outs = [torch.empty((out_rows, n_r), dtype=torch.float64, device=dev) for _ in range(n_out)]
    for start, part in column_tiles(stacked, RECORDS_PER_CALL):
        n = part.shape[1]
        d_x, d_y = part[:n_s], part[n_s:n_s + n_c]
        d_s = None if s is None else _ptr(part[n_s + n_c:])
        d_out = [torch.empty((out_rows, n), dtype=torch.float64, device=dev) for _ in range(n_out)]
        model_call(obe, entry, "obe_predictive_score_workspace_bytes", (n_p, n, n_c),
                   _ptr(d_x), n, n, _ptr(d_y), n, d_s, n, None if rows is None else _lib.host_ptr(rows),
                   _ptr(p), n_p, n_p, _ptr(w), *[_ptr(t) for t in d_out])
        for whole, piece in zip(outs, d_out):
            whole[:, start:start + n] = piece
    return [t.cpu().numpy() for t in outs], single


def predictive_logpdf(obe, settings, y_meas, sigma=None):
    (logp,), single = _score(obe, "obe_predictive_logpdf", 1, settings, y_meas, sigma)
    return float(logp[0, 0]) if single else logp[0]


def predictive_tails(obe, settings, y_meas, sigma=None):
    """``(lower, upper)``, each ``(C, n_r)``."""
    (lower, upper), _ = _score(obe, "obe_predictive_tails", 2, settings, y_meas, sigma)
    return lower, upper


def predictive_cdf(obe, settings, y_meas, sigma=None, upper=False):
    return predictive_tails(obe, settings, y_meas, sigma)[1 if upper else 0]


def predictive_pvalue(obe, settings, y_meas, sigma=None):
    return pvalue_from_tails(*predictive_tails(obe, settings, y_meas, sigma))
