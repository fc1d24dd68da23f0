"""OptBayesExptSignalNoise — measurement noise that depends on the signal (counting noise).

The reference takes the noise of a reading as a number per channel or as an unknown constant per channel; its
``yvar_noise_model()`` (obe_base.py:542-564) names the case neither covers — noise that "depends on the measurement
value, like root(N), Poisson-like counting noise", which needs the noise model evaluated over all parameters and
averaged over the distribution — and settles for a constant.  Here the noise variance of a reading whose noise-free
value is ``y`` is, per channel,

    nu_c(y) = noise_floor_c^2 + noise_gain_c |y| + noise_relative_c^2 y^2

(a signal-independent sigma; variance per unit of signal: 1 for raw Poisson counts, 1/n for the mean of n shots; a
multiplicative noise fraction).  The likelihood takes nu at every particle's own model value, and the utilities divide
by its average over the whole weighted cloud, per setting: one more settings x particles pass that never leaves the
chip (csrc/obe_signal_noise.hip).  The coefficient checks are plain functions of this module (no device needed).
"""
import math

import numpy as np
import torch

from . import _batch, _lib, _signal
from ._ownnoise import OwnCloudPasses, check_own_records
from ._devcall import P as _P, model_call, ptr as _ptr

_FIELDS = ("noise_floor", "noise_gain", "noise_relative")
#: the public names the library sets on an object of this class only (_state.py): none, the three coefficients are
#: the library's on every class
OWN_ATTRIBUTES = frozenset()


# ---------------------------------------------------------------------------------------- argument checks (host)
def check_coefficients(noise_floor, noise_gain, noise_relative, n_channels):
    """``(C, 3)`` float64 ``{a, b, c}`` per channel, ``a = noise_floor^2, b = noise_gain, c = noise_relative^2``, as
    the library takes them.  Each argument is a scalar or ``(C,)``, finite and >= 0, and in every channel at least
    one of the three must be > 0."""
    cols = []
    for name, value in zip(_FIELDS, (noise_floor, noise_gain, noise_relative)):
        try:
            v = np.asarray(value, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number or {n_channels} numbers") from None
        if v.ndim > 1 or (v.ndim == 1 and v.size != n_channels):
            raise ValueError(f"{name} must be a scalar or have one value per channel ({n_channels}), "
                             f"got shape {v.shape}")
        v = np.broadcast_to(v, (n_channels,))
        if not np.all(np.isfinite(v) & (v >= 0.0)):
            raise ValueError(f"{name} must be finite and >= 0")
        cols.append(v)
    floor, gain, relative = cols
    dead = [c for c in range(n_channels) if not (floor[c] > 0.0 or gain[c] > 0.0 or relative[c] > 0.0)]
    if dead:
        raise ValueError(f"channel(s) {dead} have no noise at all: one of noise_floor, noise_gain and noise_relative "
                         "must be > 0 in every channel")
    return np.ascontiguousarray(np.stack([floor * floor, gain, relative * relative], axis=1))


def state_fields(obj):
    """The three coefficient arrays as a snapshot keeps them (_state.py)."""
    return {name: np.array(getattr(obj, name), dtype=np.float64) for name in _FIELDS}


def kwargs_from_state(fields):
    """The constructor's keyword arguments from ``state_fields()``'s dict."""
    return {name: np.array(fields[name], dtype=np.float64) for name in _FIELDS}


class OptBayesExptSignalNoise(OwnCloudPasses):
    """``noise_floor``, ``noise_gain``, ``noise_relative``: a scalar or one value per output channel each (public
    attributes, ``(C,)`` arrays; they may be reassigned between calls).  Needs a DeviceModel.

    ``pdf_update((setting, y_meas[, sigma]))`` ignores a record's ``sigma``; ``yvar_noise_model()`` returns the
    ``(C, n_settings)`` average of ``nu`` over the cloud, ``nu_bar_c(s) = a_c + b_c sum w |y| / W + c_c sum w y^2 / W``,
    which every ``utility_method``, ``expected_variance_reduction()`` without ``sigma`` and ``opt_setting_batch()`` use.
    ``likelihood()``: ``L_i = prod_c exp(-(y_c,i - y_meas,c)^2 / (2 nu_c(y_c,i))) / sqrt(nu_c(y_c,i))``.

    Is a reading plausible, and where will the next one fall?  ``signal_logpdf()``, ``signal_cdf()``,
    ``signal_pvalue()``, ``signal_quantile()`` and ``signal_interval()`` answer with the object's own noise: the
    predictive of a reading is the mixture of N_p Gaussians whose component i has the mean ``f_c(x; theta_i)`` and the
    variance ``nu_c(f_c(x; theta_i))``.  A particle contributes with a weight > 0 and a ``nu`` that is > 0 and finite in
    EVERY channel (the likelihood's rule: a NaN or infinite model value in any channel leaves it out of all of them).
    The summaries of the base class that take a per-record ``sigma`` (``predictive_logpdf()`` ...) raise
    ``NotImplementedError`` and point at these."""
    _PASS_SUMS = "the noise is averaged"
    _REFUSAL = ("takes a fixed sigma per record, but this object's noise depends on the signal, and a fixed sigma "
                "would contradict the object's own likelihood: signal_logpdf(), signal_cdf(), signal_pvalue(), "
                "signal_quantile() and signal_interval() score a reading and draw its band with nu at every "
                "particle's own model value (records_loglik() and pdf_update_batch() take the records without sigma)")

    def __init__(self, measurement_model, setting_values, parameter_samples, constants,
                 noise_floor=0.0, noise_gain=1.0, noise_relative=0.0, **kwargs):
        OwnCloudPasses.__init__(self, measurement_model, setting_values, parameter_samples, constants, **kwargs)
        check_coefficients(noise_floor, noise_gain, noise_relative, self.n_channels)
        for name, given in zip(_FIELDS, (noise_floor, noise_gain, noise_relative)):
            setattr(self, name, np.array(np.broadcast_to(np.asarray(given, dtype=np.float64), (self.n_channels,))))

    def _coefficients(self):
        """The ``(C, 3)`` coefficients of the attributes as they stand now."""
        return check_coefficients(self.noise_floor, self.noise_gain, self.noise_relative, self.n_channels)

    def _likelihood_device(self, y_model, measurement_record):
        """The likelihood as a device tensor, nu at every particle's own model value; a record's ``sigma`` is ignored.
        ``y_model`` None: the model is evaluated at the record's setting inside the same kernel."""
        n, yy, _ = self._record_channels(measurement_record[1], None)
        return self._likelihood_call("obe_signal_noise_likelihood", y_model, measurement_record[0],
                                     (yy, self._coefficients()), n)

    def _own_records(self, settings, y_meas):
        """The records of ``records_loglik()`` / ``pdf_update_batch()``: readings of all C channels, nu at every
        particle's own model value; ``l`` carries -R C log(2 pi) / 2, the full log density."""
        x, y, _ = check_own_records(settings, y_meas, None, None, self.allsettings.shape[0], self.n_channels)
        per_record = -0.5 * self.n_channels * math.log(2.0 * math.pi)
        return _batch.OwnRecords(self, "obe_signal_noise_records_loglik", np.vstack([x, y]), x.shape[0], False,
                                 lambda begin, end: (end - begin) * per_record, (self._coefficients(),))

    def _noise_variance(self, begin, end):
        """Device ``(C, end - begin)``: nu_bar of the settings [begin, end) of the design grid, cached until the
        particles, the weights or the coefficients change."""
        coef = self._coefficients()

        def compute():
            p, w = self._pw_tensors()
            n, n_p = end - begin, p.shape[1]
            out = torch.empty((self.n_channels, max(n, 1)), dtype=torch.float64, device=self._device)
            if n > 0:
                model_call(self, "obe_signal_noise_variance", "obe_signal_noise_workspace_bytes",
                           (n_p, n, self.n_channels), _P(self._settings_dev.data_ptr() + 8 * begin), self._n_settings, n,
                           _ptr(p), n_p, n_p, _ptr(w), _lib.host_ptr(coef), _ptr(out))
            return out

        return self._nu_bar_cached(begin, end, coef.tobytes(), compute)

    # -- nu(y)-aware scoring and reading bands (_signal.py; csrc/obe_signal_noise.hip, K21) ---------------------------
    # The coefficients are the attributes as they stand when the call starts.  A particle contributes with a weight > 0
    # and a nu > 0 and finite in every channel; the density and the tails divide by the sum of ALL positive weights, the
    # quantiles by the contributing ones.  Nothing is kept on the object.
    def signal_logpdf(self, settings, y_meas):
        """``(n_r,)`` float64, or a float for one record given as ``pdf_update`` takes it: the joint log density of each
        reading under the predictive, ``log(sum_i w_i prod_c N(y_c; f_c,i, nu_c(f_c,i)) / sum_i w_i)`` — for the record
        about to be used the one-step log evidence.  -inf where nobody contributes, NaN where sum w == 0."""
        return _signal.signal_logpdf(self, settings, y_meas)

    def signal_cdf(self, settings, y_meas, upper=False):
        """``(C, n_r)``: per channel ``P(Y_c <= y_c)`` of the reading under the predictive; ``upper=True``:
        ``P(Y_c >= y_c)``.  Both are sums of positive terms, so a far tail keeps its relative accuracy."""
        return _signal.signal_cdf(self, settings, y_meas, upper)

    def signal_pvalue(self, settings, y_meas):
        """``(C, n_r)``: the two-sided p-value per channel, ``min(2 min(lower, upper), 1)`` of ``signal_cdf()``'s tails."""
        return _signal.signal_pvalue(self, settings, y_meas)

    def signal_quantile(self, q, settings=None, max_passes=48, full_output=False):
        """``(n_q, C, n_x)`` (``(C, n_x)`` for a scalar ``q``): the y with ``P(Y_c <= y) = q`` for the next reading at
        the whole design grid (None; on a sharded object too) or at ``settings`` (points, as ``predict()`` takes them);
        levels in the open interval (0, 1).  NaN where nobody contributes.  ``max_passes`` (1..64): rows still open
        then deliver their bracket's midpoint (one ``RuntimeWarning`` counts them); ``full_output`` adds
        ``{"passes": ..., "unconverged": n}``."""
        return _signal.signal_quantile(self, q, settings, max_passes, full_output)

    def signal_interval(self, level=0.95, settings=None, max_passes=48, full_output=False):
        """``(lo, hi)``: ``signal_quantile()`` at ``(1 -+ level) / 2`` per channel and setting — the band to draw
        against measured points.  Per channel, not joint."""
        return _signal.signal_interval(self, level, settings, max_passes, full_output)


CLASS = OptBayesExptSignalNoise
