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
import numpy as np
import torch

from . import _lib
from .models import DeviceModel
from .obe_base import OptBayesExpt, _LazyState, _overridden
from .particlepdf import _P, _ptr

_FIELDS = ("noise_floor", "noise_gain", "noise_relative")


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


class OptBayesExptSignalNoise(OptBayesExpt):
    """``noise_floor``, ``noise_gain``, ``noise_relative``: a scalar or one value per output channel each (public
    attributes, ``(C,)`` arrays; they may be reassigned between calls).  Needs a DeviceModel.

    ``pdf_update((setting, y_meas[, sigma]))`` ignores a record's ``sigma``; ``yvar_noise_model()`` returns the
    ``(C, n_settings)`` average of ``nu`` over the cloud, which every ``utility_method``, ``expected_variance_reduction()``
    without ``sigma`` and ``opt_setting_batch()`` use.  The summaries that take a per-record ``sigma`` do not know
    ``nu(y)`` yet and raise ``NotImplementedError``."""

    def __init__(self, measurement_model, setting_values, parameter_samples, constants,
                 noise_floor=0.0, noise_gain=1.0, noise_relative=0.0, **kwargs):
        if not isinstance(measurement_model, DeviceModel):
            raise ValueError("OptBayesExptSignalNoise needs a DeviceModel (a built-in model, models.from_expression "
                             "or models.from_function): the noise is averaged over settings x particles on the device")
        OptBayesExpt.__init__(self, measurement_model, setting_values, parameter_samples, constants, **kwargs)
        if self._device_model is None:
            raise ValueError("OptBayesExptSignalNoise needs a DeviceModel that runs on the device")
        check_coefficients(noise_floor, noise_gain, noise_relative, self.n_channels)
        for name, given in zip(_FIELDS, (noise_floor, noise_gain, noise_relative)):
            setattr(self, name, np.array(np.broadcast_to(np.asarray(given, dtype=np.float64), (self.n_channels,))))
        self._nu_bar = {}         # settings slice -> (key, device (C, e - b)): _noise_variance()

    def _coefficients(self):
        """The ``(C, 3)`` coefficients of the attributes as they stand now."""
        return check_coefficients(self.noise_floor, self.noise_gain, self.noise_relative, self.n_channels)

    # -- likelihood: nu at every particle's own model value ---------------------------
    def _likelihood_overridden(self):
        return _overridden(self, "likelihood", OptBayesExpt, OptBayesExptSignalNoise)

    def likelihood(self, y_model, measurement_record):
        """``L_i = prod_c exp(-(y_c,i - y_meas,c)^2 / (2 nu_c(y_c,i))) / sqrt(nu_c(y_c,i))`` from ``y_model`` (C x N_p)
        on the device; a record's ``sigma`` is ignored."""
        return self._likelihood_device(y_model, measurement_record).cpu().numpy()

    def _likelihood_device(self, y_model, measurement_record):
        """The likelihood as a device tensor; ``y_model`` None: the model is evaluated at the record's setting inside
        the same kernel."""
        n, yy, _ = self._record_channels(measurement_record[1], None)
        coef = self._coefficients()
        if y_model is None:
            par = self._parameters.tensor()
            n_p = par.shape[1]
            y_args = (None, 0, _ptr(par), n_p, n_p, _lib.host_ptr(self._setting_array(measurement_record[0])))
        else:
            y_dev = self._y_to_device(y_model)
            n_p = y_dev.shape[1]
            y_args = (_ptr(y_dev), n_p, None, 0, n_p, None)
        out = torch.empty(n_p, dtype=torch.float64, device=self._device)
        self._mlib.call("obe_signal_noise_likelihood", self._model_struct, *y_args, _lib.host_ptr(yy),
                        _lib.host_ptr(coef), n, self._choke_value(), _ptr(out), self._stream())
        return out

    def _pdf_update(self, measurement_record, y_model_data):
        if self._likelihood_overridden():
            if y_model_data is None:
                y_model_data = self.eval_over_all_parameters(measurement_record[0])
            lik = self.likelihood(y_model_data, measurement_record)      # user NumPy code
        else:
            if y_model_data is None and _overridden(self, "eval_over_all_parameters", OptBayesExpt):
                y_model_data = self.eval_over_all_parameters(measurement_record[0])
            lik = self._likelihood_device(y_model_data, measurement_record)
        if lik.shape[0] != self.n_particles:
            raise ValueError("parameters and particle_weights have different lengths")
        self.bayesian_update(lik)
        self._parameters = self._particles
        if self.just_resampled:
            self.enforce_parameter_constraints()
        self._drift_after_update()
        self._sweeps.update_finished(None, self.just_resampled)
        return _LazyState(self)

    # -- noise model: nu averaged over the whole weighted cloud, per setting ------------
    def _noise_variance(self, begin, end):
        """Device ``(C, end - begin)``: nu_bar of the settings [begin, end) of the design grid, cached until the
        particles, the weights or the coefficients change."""
        coef = self._coefficients()
        key = (self._particles.version, self._weights.version, coef.tobytes())
        hit = self._nu_bar.get((begin, end))
        if hit is not None and hit[0] == key:
            return hit[1]
        p, w = self._pw_tensors()
        n, n_p = end - begin, p.shape[1]
        out = torch.empty((self.n_channels, max(n, 1)), dtype=torch.float64, device=self._device)
        if n > 0:
            # (a workspace of the call's own: the object's workspace keeps the record of a sweep enqueued ahead)
            nbytes = int(self._mlib.cdll.obe_signal_noise_workspace_bytes(n_p, n, self.n_channels))
            ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=self._device)
            self._mlib.call("obe_signal_noise_variance", self._model_struct,
                            _P(self._settings_dev.data_ptr() + 8 * begin), self._n_settings, n, _ptr(p), n_p, n_p,
                            _ptr(w), _lib.host_ptr(coef), _ptr(out), _ptr(ws), nbytes, self._stream())
        self._nu_bar ={k: v for k, v in self._nu_bar.items() if v[0] == key}
        self._nu_bar[(begin, end)] = (key, out)
        return out

    def yvar_noise_model(self):
        """``(C, n_settings)`` float64: ``nu_bar_c(s) = a_c + b_c sum w |y| / W + c_c sum w y^2 / W`` over the whole
        weighted cloud, for every setting of the design grid (on a sharded object too)."""
        return self._noise_variance(0, self._n_settings).cpu().numpy()

    def _noise_token(self):
        # (the noise variance is a pass over the cloud of its own: no sweep is enqueued ahead for this class)
        return None

    def _noise_var_device(self, values=False):
        """What a sweep takes as its noise variance: the device ``(C, n_local)`` array of this rank's settings slice."""
        if _overridden(self, "yvar_noise_model", OptBayesExptSignalNoise):
            return OptBayesExpt._noise_var_device(self)
        t = self._noise_variance(self._s_begin, self._s_end)
        return t, t.shape[1]

    # -- the summaries that take a per-record sigma -----------------------------------
    def _refuse(self, name):
        raise NotImplementedError(f"{name}() takes a fixed sigma per record, but this object's noise depends on the "
                                  "signal: these summaries do not know nu(y) yet, and a fixed sigma would contradict "
                                  "the object's own likelihood")

    def predictive_logpdf(self, settings, y_meas, sigma=None):
        self._refuse("predictive_logpdf")

    def predictive_cdf(self, settings, y_meas, sigma=None, upper=False):
        self._refuse("predictive_cdf")

    def predictive_pvalue(self, settings, y_meas, sigma=None):
        self._refuse("predictive_pvalue")

    def reading_quantile(self, q, settings=None, sigma=None, max_passes=48, full_output=False):
        self._refuse("reading_quantile")

    def reading_interval(self, level=0.95, settings=None, sigma=None, max_passes=48, full_output=False):
        self._refuse("reading_interval")

    def records_loglik(self, settings, y_meas, sigma=None):
        self._refuse("records_loglik")

    def pdf_update_batch(self, settings, y_meas, sigma=None, tempered=True, max_stages=64, on_stage=None):
        self._refuse("pdf_update_batch")
