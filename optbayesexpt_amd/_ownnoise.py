"""What OptBayesExptSignalNoise, OptBayesExptBinomial and OptBayesExptPoisson share: the likelihood and the noise
variance are the object's own passes over the cloud (csrc/obe_cloud_pass.h), not the base class's Gaussian with a given
sigma.  Each class keeps its argument checks, its ``state_fields`` / ``kwargs_from_state`` and the calls of its own
entry points; ``_state.OWN_NOISE`` lists their modules."""
import math

import numpy as np
import torch

from . import _batch, _counts, _lib
from ._scoring import _numbers, check_records
from .models import DeviceModel
from .obe_base import OptBayesExpt, _LazyState, _overridden
from ._devcall import ptr as _ptr

INFORMATION = "mutual_information"


# ---------------------------------------------------------------------------------------- argument checks (host)
def check_side(name, value, n_channels):
    """``(C, 1)`` or ``(C, n_r)`` float64 of a record's side data (``shots``, ``exposure``) from a scalar, ``(C,)``
    (for one channel also ``(n_r,)``) or ``(C, n_r)``, as ``_scoring.check_sigma`` reads a sigma; the values are the
    class's to check."""
    a = _numbers(value, name)
    if a.ndim == 0:
        a = np.full((n_channels, 1), float(a))
    elif a.ndim == 1 and n_channels == 1:
        a = a.reshape(1, -1)
    elif a.ndim == 1:
        if a.size != n_channels:
            raise ValueError(f"the model has {n_channels} channels, {name} has {a.size} values")
        a = a.reshape(n_channels, 1)
    elif a.shape[0] != n_channels:
        raise ValueError(f"the model has {n_channels} channels, {name} has {a.shape[0]} rows")
    if a.shape[1] == 0:
        raise ValueError(f"{name} must hold at least one value")
    return a


def check_own_records(settings, y_meas, name, side, n_setdims, n_channels):
    """``(x (n_setdims, n_r), readings (C, n_r), side (C, n_r) or None)``, everything broadcast to one ``n_r``:
    ``_scoring.check_records`` for the settings and the readings, ``check_side`` for ``side`` (None: the class has
    none)."""
    x, y, _, _ = check_records(settings, y_meas, None, n_setdims, n_channels, True)
    if side is None:
        return x, y, None
    b = check_side(name, side, n_channels)
    lengths = {x.shape[1], b.shape[1]} - {1}
    if len(lengths) > 1:
        raise ValueError(f"settings, y_meas and {name} do not broadcast to one number of records: {sorted(lengths)}")
    n_r = lengths.pop() if lengths else 1

    def wide(a):
        return np.ascontiguousarray(np.broadcast_to(a, (a.shape[0], n_r)))
    return wide(x), wide(y), wide(b)


def lgamma_plus_one(a):
    """``lgamma(a + 1)`` of every element (``math.lgamma``, once per distinct value): log a! of whole numbers."""
    values, inverse = np.unique(a, return_inverse=True)
    return np.array([math.lgamma(v + 1.0) for v in values])[inverse].reshape(np.shape(a))


def tile_sums(terms):
    """``constants(begin, end)`` of ``_batch.OwnRecords``: ``math.fsum`` of the (C, n_r) terms of those records."""
    return lambda begin, end: math.fsum(terms[:, begin:end].ravel().tolist())


class OwnCloudPasses(OptBayesExpt):
    """Needs a DeviceModel.  A class gives ``_PASS_SUMS`` (what its pass forms, for the constructor's refusal),
    ``_REFUSAL`` (why the summaries that take a per-record Gaussian ``sigma`` raise ``NotImplementedError``),
    ``_likelihood_device(y_model, record)`` and ``_noise_variance(begin, end)``."""
    _PASS_SUMS = _REFUSAL = None

    def __init__(self, measurement_model, setting_values, parameter_samples, constants, **kwargs):
        self._need_device_model(measurement_model)
        OptBayesExpt.__init__(self, measurement_model, setting_values, parameter_samples, constants, **kwargs)
        if self._device_model is None:
            raise ValueError(f"{self._library_name()} needs a DeviceModel that runs on the device")
        self._nu_bar = {}         # settings slice -> (key, device (C, e - b)): _nu_bar_cached()

    @classmethod
    def _library_name(cls):
        from ._state import library_class
        return library_class(cls).__name__

    @classmethod
    def _need_device_model(cls, measurement_model):
        """Before anything reads the model's channel count."""
        if not isinstance(measurement_model, DeviceModel):
            raise ValueError(f"{cls._library_name()} needs a DeviceModel (a built-in model, models.from_expression or "
                             f"models.from_function): {cls._PASS_SUMS} over settings x particles on the device")

    # -- likelihood: a kernel of the class's own ------------------------------------------
    def _likelihood_overridden(self):
        return _overridden(self, "likelihood", OptBayesExpt, OwnCloudPasses)

    def likelihood(self, y_model, measurement_record):
        """The class's likelihood (see its docstring) from ``y_model`` (C x N_p) on the device, as a NumPy array."""
        return self._likelihood_device(y_model, measurement_record).cpu().numpy()

    def _likelihood_call(self, entry, y_model, setting, host_arrays, n_lik):
        """The likelihood entry point ``entry`` as a device tensor; ``y_model`` None: the model is evaluated at
        ``setting`` inside the same kernel.  ``host_arrays``: what the entry point takes of the record, in its order."""
        if y_model is None:
            par = self._parameters.tensor()
            n_p = par.shape[1]
            y_args = (None, 0, _ptr(par), n_p, n_p, _lib.host_ptr(self._setting_array(setting)))
        else:
            y_dev = self._y_to_device(y_model)
            n_p = y_dev.shape[1]
            y_args = (_ptr(y_dev), n_p, None, 0, n_p, None)
        out = torch.empty(n_p, dtype=torch.float64, device=self._device)
        self._mlib.call(entry, self._model_struct, *y_args, *[_lib.host_ptr(a) for a in host_arrays], n_lik,
                        self._choke_value(), _ptr(out), self._stream())
        return out

    # (the likelihood — a user's override, or the device's from the model or from given model values —, then
    # bayesian_update, the constraints after a resample, the drift step and the sweep state)
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

    # -- noise model: averaged over the whole weighted cloud, per setting ----------------
    def _nu_bar_cached(self, begin, end, values, compute):
        """nu_bar of the settings [begin, end), kept until the particles, the weights or ``values`` (the bytes of what
        the class's attributes give it) change; ``compute()`` forms it on a miss."""
        key = (self._particles.version, self._weights.version, values)
        hit = self._nu_bar.get((begin, end))
        if hit is not None and hit[0] == key:
            return hit[1]
        out = compute()
        self._nu_bar = {k: v for k, v in self._nu_bar.items() if v[0] == key}
        self._nu_bar[(begin, end)] = (key, out)
        return out

    def yvar_noise_model(self):
        """``(C, n_settings)`` float64: the class's ``nu_bar_c(s)`` (see its docstring) over the whole weighted cloud,
        for every setting of the design grid (on a sharded object too)."""
        return self._noise_variance(0, self._n_settings).cpu().numpy()

    def _noise_token(self):
        # (the noise variance is a pass over the cloud of its own: no sweep is enqueued ahead for this class)
        return None

    def _noise_var_device(self, values=False):
        """What a sweep takes as its noise variance: the device ``(C, n_local)`` array of this rank's settings slice."""
        if _overridden(self, "yvar_noise_model", OwnCloudPasses):
            return OptBayesExpt._noise_var_device(self)
        t = self._noise_variance(self._s_begin, self._s_end)
        return t, t.shape[1]

    # -- the summaries that take a per-record sigma -----------------------------------
    def _refuse(self, name):
        raise NotImplementedError(f"{name}() {self._REFUSAL}")

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

    # -- a recorded data set in one call: the class's own l through the base class's engine (_batch.py) --------------
    def _batch_records(self, settings, y_meas, sigma, **side):
        """``_batch.OwnRecords`` of the checked records: a class gives ``_own_records(settings, y_meas, **side)``.  (A
        ``sigma`` never gets here: the noise is the object's own.)"""
        return self._own_records(settings, y_meas, **side)

    def _no_record_sigma(self, name, sigma):
        if sigma is not None:
            self._refuse(name)

    def records_loglik(self, settings, y_meas, sigma=None):
        """``(N_p,)`` float64: per particle the joint log density of the records under the class's own likelihood (its
        docstring), the particle-independent constant included; for every particle, whatever its weight.  NaN where a
        particle has a model value the likelihood does not take, -inf where a record is impossible for it.  ``sigma``
        must stay None.  Changes nothing of the object."""
        self._no_record_sigma("records_loglik", sigma)
        return _batch.records_loglik(self, settings, y_meas)

    def pdf_update_batch(self, settings, y_meas, sigma=None, tempered=True, max_stages=64, on_stage=None):
        """``OptBayesExpt.pdf_update_batch()`` with the class's own likelihood: the same stages, resamples, constraints
        and ``last_batch_update``; ``log_evidence`` is the log of the probability (density) of the records, constants
        included, and so comparable between models.  ``sigma`` must stay None.  No drift step is taken."""
        self._no_record_sigma("pdf_update_batch", sigma)
        return _batch.pdf_update_batch(self, settings, y_meas, None, tempered, max_stages, on_stage)


class CountReadings(OwnCloudPasses):
    """The readings are counts: ``utility_method="mutual_information"`` (the class's ``utility_information()``) next to
    the base class's names, which then work on the Gaussian approximation ``yvar_noise_model()`` gives.  A class gives
    ``_NOISE_FROM``, the attribute its noise comes from, and ``_pass(begin, end, want_information)``."""
    _PASS_SUMS = "the information is summed"
    _NOISE_FROM = None

    def __init__(self, measurement_model, setting_values, parameter_samples, constants, utility_method, **kwargs):
        base_method = "variance_approx" if utility_method == INFORMATION else utility_method
        OwnCloudPasses.__init__(self, measurement_model, setting_values, parameter_samples, constants,
                                utility_method=base_method, **kwargs)
        if utility_method == INFORMATION:
            self.utility_method = INFORMATION
            self.utility = self.utility_information

    def _per_channel(self, values):
        """``(what goes into the call, None or the device (C, 1) divisor of the rows afterwards)``: one value for all
        channels goes into the call; values per channel divide the rows afterwards (x / 1 is x)."""
        if np.all(values == values[0]):
            return float(values[0]), None
        return 1.0, torch.from_numpy(values.reshape(-1, 1)).to(self._device)

    def _noise_variance(self, begin, end):
        return self._pass(begin, end, False)[1]

    def _information_of_slice(self):
        """This rank's slice of the settings summed, the slices gathered."""
        info, _ = self._pass(self._s_begin, self._s_end, True)
        n = self._s_end - self._s_begin
        return self._gather_settings(info[:n].reshape(1, -1))[0]

    # -- what takes a Gaussian sigma per record -------------------------------------------
    def _no_sigma(self, name, sigma):
        if sigma is not None:
            raise ValueError(f"{name}(): the readings are counts, their noise is the object's own "
                             f"(yvar_noise_model(), from {self._NOISE_FROM}): leave sigma out")

    def expected_variance_reduction(self, settings=None, dims=None, sigma=None):
        self._no_sigma("expected_variance_reduction", sigma)
        return OptBayesExpt.expected_variance_reduction(self, settings, dims, None)

    def opt_setting_batch(self, n, sigma=None, distinct=False, interest=None, interest_weights=None):
        self._no_sigma("opt_setting_batch", sigma)
        return OptBayesExpt.opt_setting_batch(self, n, None, distinct, interest, interest_weights)

    # -- count-aware scoring and reading bands (_counts.py; csrc/obe_counts.hip) ----------------------------------------
    # ``side``: the class's ``_NOISE_FROM`` (``shots``, ``exposure``), which each class takes under that name; None: the
    # object's attribute.  ``P_c,i(k)``: the class's pmf of channel c at particle i (its docstring); a particle
    # contributes where its weight is > 0 and every channel's model value is one the class takes, W sums those weights,
    # and W == 0 gives NaN.  Nothing is kept on the object.
    _COUNT_LAW = None

    def count_logpmf(self, settings, counts, *, side=None):
        """``(n_r,)`` float64, or a float for one record given as ``pdf_update`` takes it: the JOINT one-step log
        evidence ``log(sum_i w_i prod_c P_c,i(k_c) / W)`` of each record, ``log C(n, k)`` / ``-log k!`` included (not
        the product of the channels' mixtures).  Records as ``records_loglik()`` takes them; counts (and shots) at most
        OBE_COUNT_MAX_OUTCOMES.  -inf where the record is impossible for every contributing particle."""
        return _counts.count_logpmf(self, settings, counts, side)

    def count_cdf(self, settings, counts, upper=False, *, side=None):
        """``(C, n_r)``: per channel ``P(K_c <= k_c)`` of the recorded count under the mixture
        ``Pbar_c(k) = sum_i w_i P_c,i(k) / W``; ``upper=True``: ``P(K_c >= k_c)``.  Both tails include k itself."""
        return _counts.count_cdf(self, settings, counts, upper, side)

    def count_pvalue(self, settings, counts, *, side=None):
        """``(C, n_r)``: the two-sided p-value per channel, ``min(2 min(lower, upper), 1)`` of ``count_cdf()``'s
        tails."""
        return _counts.count_pvalue(self, settings, counts, side)

    def count_pmf(self, settings=None, count_max=None, *, side=None):
        """``(n_x, C, count_max + 2)``: ``Pbar_c(k) = sum_i w_i P_c,i(k) / W`` for k = 0 .. ``count_max``, then the mass
        above ``count_max``, at the whole design grid (None; on a sharded object too) or at ``settings`` (points, as
        ``predict()`` takes them).  ``side``: a scalar or ``(C,)``.  ``count_max``: at most OBE_COUNT_MAX_OUTCOMES."""
        return _counts.count_pmf(self, settings, count_max, side)

    def count_quantile(self, q, settings=None, count_max=None, full_output=False, *, side=None):
        """``(n_q, C, n_x)`` float64 holding whole numbers (``(C, n_x)`` for a scalar ``q``): the smallest k with
        ``P(K_c <= k) >= q``, levels in the open interval (0, 1).  NaN where the level is not reached within
        ``count_max`` (one ``RuntimeWarning`` counts such results; ``full_output`` adds ``{"beyond": n}``)."""
        return _counts.count_quantile(self, q, settings, count_max, full_output, side)

    def count_interval(self, level=0.95, settings=None, count_max=None, full_output=False, *, side=None):
        """``(lo, hi)``: ``count_quantile()`` at ``(1 -+ level) / 2`` — the band to draw against recorded counts."""
        return _counts.count_interval(self, level, settings, count_max, full_output, side)
