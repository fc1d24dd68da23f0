"""Design of a batch of measurements: which n settings, taken together, teach the most?

``opt_setting()`` answers "which one setting next"; called n times without an update in between it returns the same
setting n times.  An instrument that acquires several points per round trip (a scan table, a pulse-sequence queue,
multiplexed channels) needs n settings that are jointly informative: the second must account for what the first will
already have taught.  The quantity that needs is the covariance, over the weighted cloud, between the model output at
every setting and the output at an already chosen setting, ``X_c'c(p, x) = sum w (y_c'(p) - m_c'(p)) (y_c(x) - m_c(x)) /
sum w`` — one more settings x particles pass per pick, a HIP kernel (csrc/obe_predict.hip, K14).  The design rule is
greedy conditioning under the linear-Gaussian reading ``expected_variance_reduction()`` uses (csrc/obe_design.hip): the
output variance of every setting, conditioned on the noisy readings already planned, summed over the channels in units
of the noise and divided by the cost; the next pick is its first maximum.  That is exact for a model that is linear in
its parameters with a Gaussian cloud and an approximation otherwise, and greedy, not optimal.  The argument checks are
plain functions of this module (no device needed); ``OptBayesExpt`` has the methods.

With ``interest`` the same greedy rule designs for chosen parameter rows, the others being nuisances: the blocks of
``_interest`` — S(x) and K(x) = cov(theta_d, y(x)) — are conditioned on the planned readings by the same rows
(``obe_design_interest_step``, csrc/obe_design.hip) and every pick maximises ``utility_parameter_variance()``'s score of
what is left, ``[sum_d a_d G_d(x | picks) / V_d] / cost``.  The same caveat: exact for a model that is linear in its
parameters with a Gaussian cloud, a heuristic otherwise, and greedy.
"""
import numpy as np
import torch

from . import _interest, _lib, _predictive
from ._devcall import column_tiles, model_call, ptr as _ptr
from ._predictive import _device_model, _inputs, moments as _moments

ROWS_PER_CALL = 8                              # obe_output_cross_covariance: rows (pivots x channels) one call serves
MAX_ROWS = 128                                 # n x C of one batch: the factor store is n C C N_s doubles


# ---------------------------------------------------------------------------------------- argument checks (host)
def check_n(n, n_channels):
    """The number of picks as an int: ``1 <= n`` and ``n * C <= MAX_ROWS``."""
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)):
        raise ValueError(f"n must be an integer number of measurements, got {n!r}")
    if n < 1:
        raise ValueError(f"n must be at least 1, got {n}")
    if n * n_channels > MAX_ROWS:
        raise ValueError(f"n = {n} measurements of {n_channels} channel(s) are {n * n_channels} scalar readings: at most "
                         f"{MAX_ROWS} (the factor store holds n C C N_s doubles)")
    return int(n)


def check_noise_variance(nv):
    """The noise variance of a design: every value finite and > 0 (a reading without noise removes all variance at its
    setting and the information is infinite)."""
    nv = np.asarray(nv, dtype=np.float64)
    if not np.all(np.isfinite(nv) & (nv > 0.0)):
        raise ValueError("the noise variance of a batch design must be finite and > 0 everywhere")
    return nv


def check_points(points, n_setdims):
    """``(n_setdims, n_points)`` float64 pivot points, given as ``predict()`` takes settings."""
    return _predictive.check_settings(points, n_setdims)


def pivots_per_call(n_channels):
    return max(1, ROWS_PER_CALL // n_channels)


# ------------------------------------------------------------------------------------------------- device calls
def _cross(obe, x, pivots, p, w, mean=None):
    """Device ``(n_pivots, C, C, n_x)`` for device settings ``x`` and pivots ``(n_setdims, n_pivots)``; ``mean``: the
    ``(C, n_x)`` mean of ``obe_predictive_moments`` if the caller holds it."""
    n_x, n_p, n_c, dev = x.shape[1], p.shape[1], obe.n_channels, obe._device
    n_piv, per = pivots.shape[1], pivots_per_call(n_c)
    cross = torch.empty((n_piv, n_c, n_c, n_x), dtype=torch.float64, device=dev)
    for start, part in column_tiles(x, _predictive.SETTINGS_PER_CALL):
        n = part.shape[1]
        given = mean is not None
        d_mean = mean[:, start:start + n].contiguous() if given else torch.empty((n_c, n), dtype=torch.float64, device=dev)
        for j0 in range(0, n_piv, per):
            tile = pivots[:, j0:j0 + per].contiguous()
            nj = tile.shape[1]
            d_cross = torch.empty((nj, n_c, n_c, n), dtype=torch.float64, device=dev)
            model_call(obe, "obe_output_cross_covariance", "obe_output_cross_covariance_workspace_bytes",
                       (n_p, n, n_c, nj), _ptr(part), n, n, _ptr(tile), nj, nj, _ptr(p), n_p, n_p, _ptr(w), _ptr(d_mean),
                       1 if given or j0 else 0, _ptr(d_cross))
            cross[j0:j0 + nj, :, :, start:start + n] = d_cross
    return cross


def output_cross_covariance(obe, points, settings=None):
    _device_model(obe)
    pts = check_points(points, obe.allsettings.shape[0])
    x, p, w = _inputs(obe, settings)
    return _cross(obe, x, torch.from_numpy(pts).to(obe._device), p, w).cpu().numpy()


class _Step:
    """The state of one greedy design on the device and the ``obe_design_step`` call on it."""

    def __init__(self, obe, cvar, noise_var, cost, max_rows, distinct):
        self.obe, self.cvar, self.n_c, self.n_x = obe, cvar, cvar.shape[0], cvar.shape[1]
        dev = obe._device
        self.nv = torch.from_numpy(np.ascontiguousarray(noise_var)).to(dev)
        self.cost = cost
        self.max_rows, self.rows_done = max_rows, 0
        self.factors = torch.empty((max(max_rows, 1), self.n_c, self.n_x), dtype=torch.float64, device=dev)
        self.taken = torch.zeros(self.n_x, dtype=torch.uint8, device=dev) if distinct else None
        self.utility = torch.empty(self.n_x, dtype=torch.float64, device=dev)
        self.out = torch.zeros(3, dtype=torch.float64, device=dev)       # d_best (value, index), d_info

    def step(self, cross=None, pivot_index=0):
        """Conditions on the pivot's block ``cross (C, C, n_x)`` (None: on nothing); (the best utility left, its index,
        the information so far)."""
        d_cost, cost_scalar = self.cost
        self.obe._lib.call("obe_design_step", None if cross is None else _ptr(cross), int(pivot_index), _ptr(self.factors),
                           self.rows_done, self.max_rows, _ptr(self.cvar), self.n_c, self.n_x, _ptr(self.nv),
                           0 if self.nv.shape[1] == 1 else self.n_x, None if d_cost is None else _ptr(d_cost),
                           float(cost_scalar), None if self.taken is None else _ptr(self.taken), _ptr(self.utility),
                           _ptr(self.out), _ptr(self.out[2:]), self.obe._stream())
        if cross is not None:
            self.rows_done += self.n_c
        host = self.out.cpu().numpy()                        # the 24 bytes of a pick
        return float(host[0]), int(host.view(np.int64)[1]), float(host[2])


def plan(obe, n, sigma=None, distinct=False):
    """The greedy design: ``(report, step)`` with ``report`` as ``last_batch_design`` holds it and ``step`` the device
    state after conditioning on the first n - 1 picks (the tests read its ``cvar``)."""
    _device_model(obe)
    n_c, n_s = obe.n_channels, obe._n_settings
    n = check_n(n, n_c)
    nv = check_noise_variance(_interest.noise_variance(sigma, obe.yvar_noise_model, n_c, n_s, n_s, False))
    x, p, w = _inputs(obe, None)
    cost = obe._cost_device(whole_grid=True)
    mean, var = _moments(obe, x, p, w)
    state = _Step(obe, var, nv, cost, (n - 1) * n_c, distinct)
    indices, utility, information = np.empty(n, dtype=np.int64), np.empty(n), np.empty(n)
    pick = -1
    for j in range(n):
        if j:
            cross = _cross(obe, x, x[:, pick:pick + 1].contiguous(), p, w, mean)
            value, pick, information[j - 1] = state.step(cross[0], pick)
        else:
            value, pick, _ = state.step()
        if pick < 0:
            raise ValueError(f"opt_setting_batch: no setting with a finite utility is left for pick {j}")
        indices[j], utility[j] = pick, value
        if state.taken is not None:
            state.taken[pick] = 1
    # the information of the last reading: its own column alone (a design of one setting, the pivot itself)
    col = x[:, pick:pick + 1].contiguous()
    last = _Step(obe, state.cvar[:, pick:pick + 1].clone(),     # (a copy: the step writes its cvar)
                 nv if nv.shape[1] == 1 else np.ascontiguousarray(nv[:, pick:pick + 1]), (None, 1.0), n * n_c, False)
    last.factors[:state.rows_done] = state.factors[:state.rows_done, :, pick:pick + 1]
    last.rows_done = state.rows_done
    last.out[2:].copy_(state.out[2:])
    information[n - 1] = last.step(_cross(obe, col, col, p, w, mean[:, pick:pick + 1].contiguous())[0], 0)[2]
    return dict(indices=indices, utility=utility, information=information), state


# ------------------------------------------------------------------------ the design for parameters of interest
def check_interest(obe, interest, interest_weights):
    """None (the output-variance design) or ``(rows, weights)`` of the parameters a batch is designed for: ``interest``
    None or False: none, and weights are refused; True: the object's ``parameters_of_interest``, with
    ``interest_weights`` in place of its weights if given; an int or a sequence of ints: those rows
    (``_interest.check_dims``), weighted by ``interest_weights`` (``_interest.check_weights``; None: 1 each)."""
    if interest is None or (isinstance(interest, (bool, np.bool_)) and not interest):
        if interest_weights is not None:
            raise ValueError("interest_weights are the weights of the parameters of interest: pass interest as well")
        return None
    if isinstance(interest, (bool, np.bool_)):
        rows, weights = obe.parameters_of_interest
        if interest_weights is not None:
            weights = _interest.check_weights(interest_weights, len(rows))
        return tuple(rows), weights
    rows = _interest.check_dims(interest, obe.n_dims)
    return rows, _interest.check_weights(interest_weights, len(rows))


class _InterestStep:
    """The state of one greedy design for parameters of interest on the device — S (``ycov``, packed) and K (``xcov``)
    conditioned on the picks so far, ``pvar_left``, the factor and T stores — and the ``obe_design_interest_step`` call
    on it."""

    def __init__(self, obe, ycov, xcov, pvar, weights, noise_var, cost, max_rows, distinct):
        self.obe, self.ycov, self.xcov, self.pvar = obe, ycov, xcov, pvar
        self.n_sel, self.n_c, self.n_x = xcov.shape
        dev = obe._device

        def new(*shape):
            return torch.empty(shape, dtype=torch.float64, device=dev)
        self.pvar_left = pvar.clone()
        self.weights = np.ascontiguousarray(weights, dtype=np.float64)
        self.nv = torch.from_numpy(np.ascontiguousarray(noise_var)).to(dev)
        self.cost = cost
        self.max_rows, self.rows_done = max_rows, 0
        self.factors, self.tstore = new(max(max_rows, 1), self.n_c, self.n_x), new(max(max_rows, 1), self.n_sel)
        self.taken = torch.zeros(self.n_x, dtype=torch.uint8, device=dev) if distinct else None
        self.gain, self.utility = new(self.n_sel, self.n_x), new(self.n_x)
        self.out = torch.zeros(2, dtype=torch.float64, device=dev)       # d_best (value, index)

    def step(self, cross=None, pivot_index=0):
        """Conditions on the pivot's block ``cross (C, C, n_x)`` (None: on nothing); (the best utility left, its index,
        the ``(n_sel,)`` gains there — None if there is no such setting)."""
        d_cost, cost_scalar = self.cost
        self.obe._lib.call("obe_design_interest_step", None if cross is None else _ptr(cross), int(pivot_index),
                           _ptr(self.factors), _ptr(self.tstore), self.rows_done, self.max_rows, _ptr(self.ycov),
                           _ptr(self.xcov), self.n_sel, self.n_c, self.n_x, _ptr(self.nv),
                           0 if self.nv.shape[1] == 1 else self.n_x, _ptr(self.pvar), _ptr(self.pvar_left),
                           _lib.host_ptr(self.weights), None if d_cost is None else _ptr(d_cost), float(cost_scalar),
                           None if self.taken is None else _ptr(self.taken), _ptr(self.gain), _ptr(self.utility),
                           _ptr(self.out), self.obe._stream())
        if cross is not None:
            self.rows_done += self.n_c
        host = self.out.cpu().numpy()                        # the 16 bytes of a pick
        value, pick = float(host[0]), int(host.view(np.int64)[1])
        return value, pick, self.gain[:, pick].cpu().numpy() if pick >= 0 else None


def plan_interest(obe, n, rows, weights, sigma=None, distinct=False):
    """The greedy design for the parameter rows ``rows`` with the weights ``weights``: ``(report, step)`` with
    ``report`` as ``last_batch_design`` holds it and ``step`` the device state after conditioning on the first n - 1
    picks (the tests read it).  K12's passes once over the grid, then one cross pass per pick but the last."""
    _device_model(obe)
    n_c, n_s = obe.n_channels, obe._n_settings
    n = check_n(n, n_c)
    nv = check_noise_variance(_interest.noise_variance(sigma, obe.yvar_noise_model, n_c, n_s, n_s, False))
    x, p, w = _inputs(obe, None)
    cost = obe._cost_device(whole_grid=True)
    mean, ycov, xcov, pvar = _interest._blocks(obe, None, rows)
    state = _InterestStep(obe, ycov, xcov, pvar, weights, nv, cost, (n - 1) * n_c, distinct)
    prior = pvar.cpu().numpy()
    indices, utility, left = np.empty(n, dtype=np.int64), np.empty(n), np.empty((n, len(rows)))
    pick = -1
    for j in range(n):
        if j:
            cross = _cross(obe, x, x[:, pick:pick + 1].contiguous(), p, w, mean)
            value, pick, gain = state.step(cross[0], pick)
        else:
            value, pick, gain = state.step()
        if pick < 0:
            raise ValueError(f"opt_setting_batch: no setting with a finite utility is left for pick {j}")
        indices[j], utility[j] = pick, value
        left[j] = (left[j - 1] if j else prior) - gain
        if state.taken is not None:
            state.taken[pick] = 1
    report = dict(indices=indices, utility=utility, variance_left=left, prior_variance=prior, dims=tuple(rows),
                  weights=np.array(weights, dtype=np.float64))
    return report, state


def opt_setting_batch(obe, n, sigma=None, distinct=False, interest=None, interest_weights=None):
    _device_model(obe)
    chosen = check_interest(obe, interest, interest_weights)
    if chosen is None:
        report, _ = plan(obe, n, sigma, distinct)
    else:
        report, _ = plan_interest(obe, n, chosen[0], chosen[1], sigma, distinct)
    obe.last_batch_design = report
    grid = np.asarray(obe.allsettings)
    return tuple(np.array(grid[d, report["indices"]]) for d in range(grid.shape[0]))
