"""OptBayesExptPoisson — counted events and exact information design.

A photon-counting or NV-centre experiment reads a whole number of events per reading, often a handful.  A Gaussian whose
variance follows the signal (OptBayesExptSignalNoise) puts mass on negative counts there, and its design rule is not the
information of a count.  Here the model's channel ``c`` gives a RATE ``r_c = f_c(x; theta)`` in counts per unit exposure
and a record is ``(setting, k[, t])``: ``k_c`` counted events in the exposure ``t_c``, ``lambda_c = t_c r_c``:

    likelihood   L_i = exp(sum_c [k_c log lambda_c,i - lambda_c,i - log k_c!])       (the Poisson pmf itself)
    design       U(x) = I(theta; the next reading's count censored at count_cap) / cost_estimate(),

the exact mutual information, in nats, of the outcomes ``{0, .., count_cap - 1, ">= count_cap"}`` (models of one channel):
exact for the censored reading, a lower bound of the uncensored one's, tight when the tail mass is small — which
``last_information["tail_max"]`` reports after every pass.  One settings x particles pass that never leaves the chip
(csrc/obe_poisson.hip) gives the information, the predicted histogram of the next reading (``count_distribution()``) and
``nu_bar_c(x) = sum w r_c / W / exposure_c``, the variance of the reading k / t, which ``yvar_noise_model()`` returns: the
inherited variance utilities then mean the Gaussian approximation of these counts.  The argument checks are plain
functions of this module (no device needed).
"""
import math

import numpy as np
import torch

from . import _batch, _lib, _predictive
from ._ownnoise import INFORMATION, CountReadings, check_own_records, lgamma_plus_one, tile_sums
from ._counts import Law as CountLaw
from ._devcall import P as _P, model_call, ptr as _ptr

MAX_CHANNELS = _lib.OBE_MAX_CHANNELS
CAPS = (16, 32, 64)
#: the public names the library sets on an object of this class only (_state.py)
OWN_ATTRIBUTES = frozenset(("exposure", "count_cap", "last_information"))
VARIANCE_METHODS = ("variance_approx", "variance_full", "parameter_variance", "max_min", "pseudo_utility")


# ---------------------------------------------------------------------------------------- argument checks (host)
def _values(name, value, n_channels):
    try:
        v = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number or {n_channels} numbers") from None
    if v.ndim > 1 or v.size == 0:
        raise ValueError(f"{name} must be a scalar or one value per channel, got shape {v.shape}")
    return v


def check_cap(count_cap):
    """The censoring count of the information, or ``ValueError``: 16, 32 or 64 (compile-time sizes of the kernel)."""
    if isinstance(count_cap, (bool, np.bool_)) or count_cap not in CAPS or int(count_cap) != count_cap:
        raise ValueError(f"count_cap must be one of {CAPS} (OBE_POISSON_MAX_CAP = {_lib.OBE_POISSON_MAX_CAP}), "
                         f"got {count_cap!r}")
    return int(count_cap)


def check_exposure(exposure, n_channels):
    """``(C,)`` float64 exposure per channel from a scalar or ``(C,)``: finite and > 0."""
    v = _values("exposure", exposure, n_channels)
    if v.ndim == 1 and v.size != n_channels:
        raise ValueError(f"exposure must be a scalar or have one value per channel ({n_channels}), got shape {v.shape}")
    if not np.all(np.isfinite(v)) or np.any(v <= 0):
        raise ValueError("exposure must be finite and > 0")
    return np.array(np.broadcast_to(v, (n_channels,)))


def check_record_counts(counts, exposure, n_channels):
    """``(n_lik, k, t, log k!)`` of a record: the channels that enter the likelihood (the reference's truncation of a
    record to the shorter of its values and the model's channels), their counted events, exposures and
    ``lgamma(k + 1)``, float64 arrays of ``MAX_CHANNELS``.  ``counts``: a scalar or one value per channel, whole
    numbers >= 0; ``exposure``: a scalar (for every channel) or one value per channel, finite and > 0."""
    k = np.atleast_1d(_values("the counts of a record", counts, n_channels))
    t = _values("the exposure of a record", exposure, n_channels)
    n_lik = min(n_channels, k.size, MAX_CHANNELS)
    if t.ndim == 1:
        n_lik = min(n_lik, t.size)
    k, t = k[:n_lik], np.broadcast_to(t, (n_lik,)) if t.ndim == 0 else t[:n_lik]
    if not np.all(np.isfinite(k)) or np.any(k != np.floor(k)) or np.any(k < 0):
        raise ValueError("the counts of a record must be whole numbers >= 0: the readings are counted events")
    if not np.all(np.isfinite(t)) or np.any(t <= 0):
        raise ValueError("the exposure of a record must be finite and > 0")
    kk, tt, lf = np.zeros(MAX_CHANNELS), np.ones(MAX_CHANNELS), np.zeros(MAX_CHANNELS)
    kk[:n_lik], tt[:n_lik] = k, t
    lf[:n_lik] = [math.lgamma(v + 1.0) for v in k]
    return n_lik, kk, tt, lf


def check_count_table(counts, exposure):
    """``check_record_counts``' rules for every record at once: ``counts`` (C, n_r) whole numbers >= 0, ``exposure``
    (C, n_r) finite and > 0, or ``ValueError``.  Returns ``-log k!`` per record and channel, (C, n_r): what the records
    bring that no particle changes."""
    k, t = np.asarray(counts, dtype=np.float64), np.asarray(exposure, dtype=np.float64)
    if not np.all(np.isfinite(k)) or np.any(k != np.floor(k)) or np.any(k < 0):
        raise ValueError("the counts of the records must be whole numbers >= 0: the readings are counted events")
    if not np.all(np.isfinite(t)) or np.any(t <= 0):
        raise ValueError("the exposure of the records must be finite and > 0")
    return -lgamma_plus_one(k)


def state_fields(obj):
    """What a snapshot keeps of this class besides the base class's (_state.py): ``exposure`` and ``count_cap``."""
    return {"exposure": np.array(obj.exposure, dtype=np.float64), "count_cap": int(obj.count_cap)}


def kwargs_from_state(fields):
    """The constructor's keyword arguments from ``state_fields()``'s dict."""
    return {"exposure": np.array(fields["exposure"], dtype=np.float64), "count_cap": int(fields["count_cap"])}


class OptBayesExptPoisson(CountReadings):
    """``exposure``: the exposure per reading, a scalar or one value per channel; the ``t`` of a record that brings
    none, and what ``yvar_noise_model()`` divides by: ``nu_bar_c(s) = sum w r_c / W / exposure_c``, the variance of the
    reading k / t.  ``count_cap``: 16, 32 or 64, the count the information's reading is censored at.  Both are public
    attributes and may be reassigned between calls.  Needs a DeviceModel whose outputs are rates (>= 0).

    ``utility_method``: ``"mutual_information"`` (default, models of one channel; ``utility_information()``) or any name
    the base class knows, which then works on the Gaussian approximation ``yvar_noise_model()`` gives.
    ``pdf_update((setting, k))`` or ``((setting, k, t))``; ``likelihood()``:
    ``L_i = exp(sum_c [k_c log lambda_c,i - lambda_c,i - log k_c!])``, ``lambda = t r``, 0 for a particle with a rate that
    is NaN, negative or infinite.  ``last_information`` holds ``{"cap", "tail_max"}`` of the last information pass:
    ``tail_max``, the largest mass of the outcome ">= cap" over this rank's settings, says whether ``count_cap`` is large
    enough for the rates.  ``records_loglik()`` and ``pdf_update_batch()`` take a recorded spectrum of counts at once.
    The summaries that take a per-record Gaussian ``sigma`` raise ``NotImplementedError``; for counts ask
    ``count_logpmf()``, ``count_cdf()``, ``count_pvalue()`` (is this record plausible?) and ``count_pmf()``,
    ``count_quantile()``, ``count_interval()`` (where will the next k fall?): every channel, any rate, windows up to
    OBE_COUNT_MAX_OUTCOMES, where ``count_distribution()`` serves one channel up to ``count_cap``."""
    _NOISE_FROM = "exposure"
    _REFUSAL = ("takes readings with a Gaussian sigma per record, but this object's readings are counts (k events in "
                "an exposure t): count_logpmf(), count_cdf(), count_pvalue(), count_quantile() and count_interval() "
                "score and band them (records_loglik() and pdf_update_batch() take the records without sigma)")
    DEFAULT_COUNT_MAX = 256
    _COUNT_LAW = CountLaw(_lib.OBE_COUNT_POISSON, "exposure", check_exposure, check_count_table,
                          lambda exposure: OptBayesExptPoisson.DEFAULT_COUNT_MAX, False)

    def __init__(self, measurement_model, setting_values, parameter_samples, constants, exposure=1.0, count_cap=32,
                 utility_method=INFORMATION, **kwargs):
        self._need_device_model(measurement_model)
        if utility_method == INFORMATION and measurement_model.n_channels != 1:
            raise ValueError(f"utility_method=\"{INFORMATION}\" takes a model of one channel (the joint information of "
                             f"several counted channels is not built), got {measurement_model.n_channels}; the variance "
                             f"utilities work on every channel count: {', '.join(VARIANCE_METHODS)}")
        check_exposure(exposure, measurement_model.n_channels)
        check_cap(count_cap)
        CountReadings.__init__(self, measurement_model, setting_values, parameter_samples, constants, utility_method,
                               **kwargs)
        self.exposure = exposure
        self.count_cap = count_cap
        self.last_information = None

    def _likelihood_device(self, y_model, measurement_record):
        """The likelihood as a device tensor: the counts of a record against every particle's rates.  ``y_model``
        None: the model is evaluated at the record's setting inside the same kernel."""
        given = measurement_record[2] if len(measurement_record) > 2 else None
        exposure = check_exposure(self.exposure, self.n_channels) if given is None else given
        n, kk, tt, lf = check_record_counts(measurement_record[1], exposure, self.n_channels)
        return self._likelihood_call("obe_poisson_likelihood", y_model, measurement_record[0], (kk, tt, lf), n)

    # -- a recorded data set in one call ---------------------------------------------------
    def _own_records(self, settings, y_meas, exposure=None):
        """The records of ``records_loglik()`` / ``pdf_update_batch()``: counts of all C channels and their exposures;
        ``l`` carries -sum log k!, the full log probability."""
        exposure = check_exposure(self.exposure, self.n_channels) if exposure is None else exposure
        x, k, t = check_own_records(settings, y_meas, "exposure", exposure, self.allsettings.shape[0], self.n_channels)
        neg_log_fact = check_count_table(k, t)
        return _batch.OwnRecords(self, "obe_poisson_records_loglik", np.vstack([x, k, t]), x.shape[0], True,
                                 tile_sums(neg_log_fact))

    def records_loglik(self, settings, y_meas, sigma=None, *, exposure=None):
        """``(N_p,)`` float64: ``l_i = sum_r sum_c [k log lambda - lambda - log k!]``, ``lambda = t r``, the log
        probability of the recorded counts ``y_meas`` (all C channels) per particle, whatever its weight.
        ``exposure``: None (the object's ``exposure``), a scalar, ``(C,)``, ``(C, n_r)`` or for one channel ``(n_r,)``.
        NaN where a rate is NaN, negative or infinite, -inf where a record is impossible.  ``sigma`` must stay None."""
        self._no_record_sigma("records_loglik", sigma)
        return _batch.records_loglik(self, settings, y_meas, exposure=exposure)

    def pdf_update_batch(self, settings, y_meas, sigma=None, tempered=True, max_stages=64, on_stage=None, *,
                         exposure=None):
        """``OptBayesExpt.pdf_update_batch()`` with the Poisson likelihood of the recorded counts; ``exposure`` as
        ``records_loglik()`` takes it.  ``last_batch_update["log_evidence"]`` is the log probability of the records,
        ``-log k!`` included: comparable between models of the same counts.  ``sigma`` must stay None."""
        self._no_record_sigma("pdf_update_batch", sigma)
        return _batch.pdf_update_batch(self, settings, y_meas, None, tempered, max_stages, on_stage, exposure=exposure)

    # -- count-aware scoring and reading bands: CountReadings' methods under this class's keyword ----------------------
    def count_logpmf(self, settings, counts, *, exposure=None):
        """``CountReadings.count_logpmf()``: the joint one-step log evidence of each record, ``-log k!`` included.
        ``exposure`` as ``records_loglik()`` takes it."""
        return CountReadings.count_logpmf(self, settings, counts, side=exposure)

    def count_cdf(self, settings, counts, upper=False, *, exposure=None):
        """``CountReadings.count_cdf()``: per channel P(K <= k), or P(K >= k), of the recorded counts.  ``exposure`` as
        ``records_loglik()`` takes it."""
        return CountReadings.count_cdf(self, settings, counts, upper, side=exposure)

    def count_pvalue(self, settings, counts, *, exposure=None):
        """``CountReadings.count_pvalue()``: the two-sided p-value of the recorded counts, per channel."""
        return CountReadings.count_pvalue(self, settings, counts, side=exposure)

    def count_pmf(self, settings=None, count_max=None, *, exposure=None):
        """``CountReadings.count_pmf()``: the predicted histogram of the next reading, ``(n_x, C, count_max + 2)``.
        ``count_max`` None: 256.  ``exposure``: None (the object's), a scalar or ``(C,)``."""
        return CountReadings.count_pmf(self, settings, count_max, side=exposure)

    def count_quantile(self, q, settings=None, count_max=None, full_output=False, *, exposure=None):
        """``CountReadings.count_quantile()``: the smallest k with P(K <= k) >= q, ``(n_q, C, n_x)``."""
        return CountReadings.count_quantile(self, q, settings, count_max, full_output, side=exposure)

    def count_interval(self, level=0.95, settings=None, count_max=None, full_output=False, *, exposure=None):
        """``CountReadings.count_interval()``: ``(lo, hi)``, the band the next reading's counts fall in."""
        return CountReadings.count_interval(self, level, settings, count_max, full_output, side=exposure)

    # -- one pass over settings x particles ----------------------------------------------
    def _call(self, x, ld_s, n, exposure, cost_t, cost_s, info, tail, pmf, nu):
        """obe_poisson_information on the ``n`` settings whose first column ``x`` addresses; the outputs that are not
        None are written."""
        cap = check_cap(self.count_cap)
        p, w = self._pw_tensors()
        n_p = p.shape[1]
        opt = [None if t is None else _ptr(t) for t in (info, tail, pmf, nu)]
        model_call(self, "obe_poisson_information", "obe_poisson_workspace_bytes", (n_p, n, self.n_channels, cap),
                   x, ld_s, n, _ptr(p), n_p, n_p, _ptr(w), float(exposure), cap, cost_t, float(cost_s), *opt)

    def _pass(self, begin, end, want_information):
        """Device ``(information (end - begin,) or None, nu_bar (C, end - begin))`` of the settings [begin, end) of the
        design grid.  ``nu_bar`` is cached until the particles, the weights or ``exposure`` change; the information,
        divided by a ``cost_estimate()`` that may depend on anything, is formed anew by every call that wants it, and
        leaves ``last_information`` behind."""
        exposure = check_exposure(self.exposure, self.n_channels)
        cap = check_cap(self.count_cap)
        made = {}

        def compute():
            n = end - begin
            new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self._device)      # noqa: E731
            nu = new(self.n_channels, max(n, 1))
            info, tail = (new(max(n, 1)), new(max(n, 1))) if want_information else (None, None)
            if n > 0:
                cost_t, cost_s = self._cost_device(whole_grid=True) if want_information else (None, 1.0)
                into_call, rows = self._per_channel(exposure)
                self._call(_P(self._settings_dev.data_ptr() + 8 * begin), self._n_settings, n, into_call,
                           None if cost_t is None else _P(cost_t.data_ptr() + 8 * begin), cost_s, info, tail, None, nu)
                if rows is not None:
                    nu /= rows
            if want_information:
                # (NaN where nobody contributes: such a setting says nothing about the cap)
                worst = float(torch.nan_to_num(tail[:n], nan=0.0).max().item()) if n > 0 else 0.0
                self.last_information = {"cap": cap, "tail_max": worst}
            made["info"] = info
            return nu

        if want_information:
            self._nu_bar.pop((begin, end), None)
        nu = self._nu_bar_cached(begin, end, exposure.tobytes(), compute)
        return made.get("info"), nu

    def utility_information(self):
        """``U (N_s,)`` over the design grid: the mutual information, in nats, between the parameters and the next
        reading's count censored at ``count_cap``, divided by ``cost_estimate()``; NaN where no particle contributes.
        On a sharded object every rank sums its slice of the settings and the slices are gathered.  Afterwards
        ``last_information`` holds the cap and the largest tail mass over this rank's settings."""
        if self.n_channels != 1:
            raise ValueError("utility_information() takes a model of one channel; the variance utilities work on every "
                             f"channel count: {', '.join(VARIANCE_METHODS)}")
        return self._information_of_slice()

    def count_distribution(self, settings=None):
        """``(n_settings, count_cap + 1)``: the predicted histogram of the next reading's count over the weighted cloud,
        ``Pbar_k = sum w Pois(k; exposure r) / W`` for k < ``count_cap`` and the mass of ">= count_cap" last, at the
        design grid or at ``settings`` (points, as ``predict()`` takes them).  What one draws against recorded counts,
        and what an outlier check sums a tail of.  Models of one channel."""
        if self.n_channels != 1:
            raise ValueError("count_distribution() takes a model of one channel")
        exposure = check_exposure(self.exposure, 1)
        cap = check_cap(self.count_cap)
        x, _, _ = _predictive._inputs(self, settings)
        n = x.shape[1]
        pmf = torch.empty((cap + 1, n), dtype=torch.float64, device=self._device)
        self._call(_ptr(x), n, n, exposure[0], None, 1.0, None, None, pmf, None)
        return np.ascontiguousarray(pmf.cpu().numpy().T)


CLASS = OptBayesExptPoisson
