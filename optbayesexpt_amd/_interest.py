"""Design for parameters of interest: which measurement teaches us about the parameter we care about?

Every utility of the reference scores a setting by how much the model output varies there, for any reason
(obe_base.py:579-720: ``sum_c var_p / var_n``); a user who wants the line centre and treats amplitude and background as
nuisances gets readings placed where the amplitude dominates the spread.  The remedy is the covariance, over the
weighted cloud, between the model output and each parameter of interest: per setting ``S = cov(y, y)`` (C x C) and
``K = cov(theta_d, y)`` (rows x C), and from them ``G_d = k_d^T (S + diag nu)^-1 k_d`` — the variance of ``theta_d``
that the best LINEAR estimator from one reading removes (exact for a model linear in its parameters with a Gaussian
cloud, a lower bound on ``Var(E[theta_d | y])`` in general).  The blocks take settings x particles evaluations; they are
HIP kernels (csrc/obe_predict.hip, K12; the finish in csrc/obe_interest.hip) and only ``(rows, C, n_x)`` results travel.
The argument checks are plain functions of this module (no device needed), the calls are tiled over the settings
(``_predictive.SETTINGS_PER_CALL``) and over the rows (``ROWS_PER_CALL``), each with a workspace of its own;
``OptBayesExpt`` has the methods.
"""
import numpy as np
import torch

from . import _lib, _predictive
from ._devcall import column_tiles, model_call, ptr as _ptr
from ._predictive import _device_model, _inputs
from ._scoring import check_sigma

ROWS_PER_CALL = 8                              # obe_output_covariance / obe_variance_reduction: rows one call serves


# ---------------------------------------------------------------------------------------- argument checks (host)
def check_dims(dims, n_dims):
    """A tuple of distinct parameter rows in ``[0, n_dims)``, in the order given, from None (all rows), an int or a
    sequence of ints."""
    if dims is None:
        return tuple(range(n_dims))
    if isinstance(dims, (int, np.integer)) and not isinstance(dims, (bool, np.bool_)):
        rows = [dims]
    else:
        try:
            rows = list(dims)
        except TypeError:
            raise ValueError(f"dims must be None, a row index or a sequence of row indices, got {dims!r}") from None
    if not rows:
        raise ValueError("dims must name at least one parameter row")
    for r in rows:
        if isinstance(r, (bool, np.bool_)) or not isinstance(r, (int, np.integer)):
            raise ValueError(f"dims must be integer row indices, got {r!r}")
        if not 0 <= r < n_dims:
            raise ValueError(f"parameter row {r} is outside [0, {n_dims})")
    rows = tuple(int(r) for r in rows)
    if len(set(rows)) != len(rows):
        raise ValueError(f"dims names a parameter row twice: {rows}")
    return rows


def check_weights(weights, n_rows):
    """``(n_rows,)`` float64 weights of the parameters of interest: finite, >= 0, not all zero; None: 1 each."""
    if weights is None:
        return np.ones(n_rows)
    try:
        a = np.array(weights, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"weights must be numbers, got {weights!r}") from None
    if a.size != n_rows:
        raise ValueError(f"{n_rows} parameter(s) of interest, {a.size} weight(s)")
    if not np.all(np.isfinite(a) & (a >= 0.0)):
        raise ValueError("weights must be finite and >= 0")
    if not np.any(a > 0.0):
        raise ValueError("weights must not all be zero")
    return a


def noise_variance(sigma, model_noise, n_channels, n_x, n_grid, explicit):
    """The noise variance of the ``n_x`` settings of a request, ``(C, 1)`` or ``(C, n_x)`` float64: ``sigma ** 2`` if
    ``sigma`` is given (a scalar, ``(C,)`` or ``(C, n_x)``, by ``_scoring.check_sigma``), else ``model_noise()`` — the
    object's ``yvar_noise_model`` —, per channel or ``(C, n_grid)``; the latter belongs to the design grid and is
    refused with ``explicit`` settings."""
    if sigma is not None:
        s = check_sigma(sigma, n_channels)
        if s.shape[1] not in (1, n_x):
            raise ValueError(f"sigma has {s.shape[1]} values per channel for {n_x} setting(s)")
        return s * s
    nv = np.asarray(model_noise(), dtype=np.float64)
    if nv.size == 1 or nv.shape in ((n_channels,), (n_channels, 1)):
        return np.array(np.broadcast_to(nv.reshape(-1, 1), (n_channels, 1)))
    if nv.shape != (n_channels, n_grid):
        raise ValueError(f"yvar_noise_model() returned shape {nv.shape}: one value, ({n_channels},), ({n_channels}, 1) "
                         f"or ({n_channels}, {n_grid})")
    if explicit:
        raise ValueError("yvar_noise_model() returns a value per setting of the design grid: pass sigma with "
                         "settings of your own")
    return np.ascontiguousarray(nv)


def unpack_lower(packed, n_channels):
    """``(C, C, n_x)`` symmetric from the packed lower triangle ``(C (C + 1) / 2, n_x)``, row-major."""
    full = np.empty((n_channels, n_channels, packed.shape[1]))
    k = 0
    for c in range(n_channels):
        for c2 in range(c + 1):
            full[c, c2] = full[c2, c] = packed[k]
            k += 1
    return full


# ------------------------------------------------------------------------------------------------- device calls
def _blocks(obe, settings, rows):
    """Device tensors ``(mean (C, n_x), ycov (C (C + 1) / 2, n_x), xcov (n_sel, C, n_x), pvar (n_sel,))``."""
    _device_model(obe)
    x, p, w = _inputs(obe, settings)
    n_x, n_p, n_c, dev = x.shape[1], p.shape[1], obe.n_channels, obe._device
    pairs = n_c * (n_c + 1) // 2

    def new(*shape):
        return torch.empty(shape, dtype=torch.float64, device=dev)
    mean, ycov, xcov, pvar = new(n_c, n_x), new(pairs, n_x), new(len(rows), n_c, n_x), new(len(rows))
    for start, part in column_tiles(x, _predictive.SETTINGS_PER_CALL):
        n = part.shape[1]
        d_mean, d_ycov = new(n_c, n), new(pairs, n)
        for r0 in range(0, len(rows), ROWS_PER_CALL):
            tile = np.array(rows[r0:r0 + ROWS_PER_CALL], dtype=np.int32)
            d_xcov = new(tile.size, n_c, n)
            model_call(obe, "obe_output_covariance", "obe_output_covariance_workspace_bytes", (n_p, n, n_c, tile.size),
                       _ptr(part), n, n, _ptr(p), n_p, p.shape[0], n_p, _ptr(w), _lib.host_ptr(tile), tile.size,
                       _ptr(d_mean), _ptr(d_ycov) if r0 == 0 else None, _ptr(d_xcov), _ptr(pvar[r0:r0 + tile.size]))
            xcov[r0:r0 + tile.size, :, start:start + n] = d_xcov
        mean[:, start:start + n] = d_mean
        ycov[:, start:start + n] = d_ycov
    return mean, ycov, xcov, pvar


def _finish(obe, ycov, xcov, pvar, noise_var, weights=None, cost=(None, 1.0)):
    """Device ``(gain (n_sel, n_x), utility (n_x,) or None)`` from the blocks; ``weights``: form the utility too, with
    ``cost`` = (device (n_x,) or None, scalar)."""
    n_sel, n_c, n_x = xcov.shape
    dev = obe._device
    nv = torch.from_numpy(np.ascontiguousarray(noise_var)).to(dev)
    gain = torch.empty((n_sel, n_x), dtype=torch.float64, device=dev)
    utility = None if weights is None else torch.empty(n_x, dtype=torch.float64, device=dev)
    d_cost, cost_scalar = cost
    for r0 in range(0, n_sel, ROWS_PER_CALL):
        nr = min(ROWS_PER_CALL, n_sel - r0)
        a = None if weights is None else np.ascontiguousarray(weights[r0:r0 + nr], dtype=np.float64)
        obe._lib.call("obe_variance_reduction", _ptr(ycov), _ptr(xcov[r0:r0 + nr]), nr, n_c, n_x, _ptr(nv),
                      0 if nv.shape[1] == 1 else n_x, _ptr(pvar[r0:r0 + nr]),
                      None if a is None else _lib.host_ptr(a), None if d_cost is None else _ptr(d_cost),
                      float(cost_scalar), _ptr(gain[r0:r0 + nr]), None if utility is None else _ptr(utility),
                      1 if r0 else 0, obe._stream())
    return gain, utility


def output_covariance(obe, settings=None, dims=None):
    rows = check_dims(dims, obe.n_dims)
    mean, ycov, xcov, _ = _blocks(obe, settings, rows)
    return mean.cpu().numpy(), unpack_lower(ycov.cpu().numpy(), obe.n_channels), xcov.cpu().numpy()


def expected_variance_reduction(obe, settings=None, dims=None, sigma=None):
    rows = check_dims(dims, obe.n_dims)
    _device_model(obe)
    n_x = obe._n_settings if settings is None else _predictive.check_settings(settings, obe.allsettings.shape[0]).shape[1]
    nv = noise_variance(sigma, obe.yvar_noise_model, obe.n_channels, n_x, obe._n_settings, settings is not None)
    _, ycov, xcov, pvar = _blocks(obe, settings, rows)
    gain, _ = _finish(obe, ycov, xcov, pvar, nv)
    return gain.cpu().numpy()


def utility_parameter_variance(obe):
    rows, weights = obe.parameters_of_interest
    nv = noise_variance(None, obe.yvar_noise_model, obe.n_channels, obe._n_settings, obe._n_settings, False)
    _, ycov, xcov, pvar = _blocks(obe, None, rows)
    _, utility = _finish(obe, ycov, xcov, pvar, nv, weights, obe._cost_device(whole_grid=True))
    return utility.cpu().numpy()
