"""OptBayesExptBinomial — yes/no outcomes and information-gain design.

Every other class of the package takes a reading as a number with Gaussian noise.  A qubit or NV-centre measurement
(Rabi, Ramsey, a resonance search by single shots) reads a click or no click, or ``k`` clicks in ``n`` shots.  Here the
model's channel ``c`` gives a success probability ``p_c = f_c(x; theta)`` and a record is ``(setting, k[, n])``:

    likelihood   L_i = exp(sum_c [k_c log p_c,i + (n_c - k_c) log1p(-p_c,i)])
    design       U(x) = [H(mean outcome distribution at x) - mean of sum_c h2(p_c)] / cost_estimate(),

the exact mutual information, in nats, between the parameters and the joint outcome of the NEXT SHOT in every channel:
no variance approximation.  (The information of a batch of n shots at one setting is not formed; the design ranks the
settings by what the next shot tells.)  One settings x particles pass that never leaves the chip
(csrc/obe_binomial.hip) gives the information and, along with it, ``nu_bar_c(x) = sum w p_c (1 - p_c) / W / shots``,
the variance of the fraction k / n, which ``yvar_noise_model()`` returns: the inherited variance utilities then mean the
Gaussian approximation of these counts.  The count checks are plain functions of this module (no device needed).
"""
import numpy as np
import torch

from . import _batch, _lib
from ._ownnoise import INFORMATION, CountReadings, check_own_records, lgamma_plus_one, tile_sums
from ._counts import Law as CountLaw
from ._devcall import P as _P, model_call, ptr as _ptr

MAX_CHANNELS = _lib.OBE_BINOMIAL_MAX_CHANNELS
#: the public names the library sets on an object of this class only (_state.py): ``shots`` is a likely name for an
#: attribute of the user's own on any other class, where it travels as it always did
OWN_ATTRIBUTES = frozenset(("shots",))


# ---------------------------------------------------------------------------------------- argument checks (host)
def _counts(name, value, n_channels):
    try:
        v = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a whole number or {n_channels} whole numbers") from None
    if v.ndim > 1 or v.size == 0:
        raise ValueError(f"{name} must be a scalar or one value per channel, got shape {v.shape}")
    if not np.all(np.isfinite(v)) or np.any(v != np.floor(v)):
        raise ValueError(f"{name} must be finite and integer-valued: the readings are counts")
    return v


def check_channels(n_channels):
    """The model's channel count, or ``ValueError``: 2^C outcome sums per lane are formed, C <= 3."""
    if not 1 <= n_channels <= MAX_CHANNELS:
        raise ValueError(f"OptBayesExptBinomial takes a model of 1..{MAX_CHANNELS} channels "
                         f"(OBE_BINOMIAL_MAX_CHANNELS), got {n_channels}")
    return n_channels


def check_shots(shots, n_channels):
    """``(C,)`` float64 shots per channel from a scalar or ``(C,)``: finite, integer-valued, >= 1."""
    v = _counts("shots", shots, n_channels)
    if v.ndim == 1 and v.size != n_channels:
        raise ValueError(f"shots must be a scalar or have one value per channel ({n_channels}), got shape {v.shape}")
    if np.any(v < 1):
        raise ValueError("shots must be >= 1")
    return np.array(np.broadcast_to(v, (n_channels,)))


def check_counts(successes, shots, n_channels):
    """``(n_lik, k, n)`` of a record: the channels that enter the likelihood (the reference's truncation of a record to
    the shorter of its values and the model's channels) and their successes and shots, float64 arrays of
    ``MAX_CHANNELS``.  ``successes``: a scalar or one value per channel; ``shots``: a scalar (for every channel) or one
    value per channel; integer-valued with 0 <= k <= n and n >= 1."""
    k = np.atleast_1d(_counts("the successes of a record", successes, n_channels))
    n = _counts("the shots of a record", shots, n_channels)
    n_lik = min(n_channels, k.size)
    if n.ndim == 1:
        n_lik = min(n_lik, n.size)
    k, n = k[:n_lik], np.broadcast_to(n, (n_lik,)) if n.ndim == 0 else n[:n_lik]
    if np.any(n < 1):
        raise ValueError("the shots of a record must be >= 1")
    if np.any(k < 0) or np.any(k > n):
        raise ValueError("the successes of a record must lie in 0..shots")
    kk, nn = np.zeros(MAX_CHANNELS), np.ones(MAX_CHANNELS)
    kk[:n_lik], nn[:n_lik] = k, n
    return n_lik, kk, nn


def check_count_table(successes, shots):
    """``check_counts``' rules for every record at once: ``successes`` and ``shots`` (C, n_r), finite and
    integer-valued with 0 <= k <= n and n >= 1, or ``ValueError``.  Returns ``log C(n, k)`` per record and channel,
    (C, n_r): what the records bring that no particle changes."""
    k, n = np.asarray(successes, dtype=np.float64), np.asarray(shots, dtype=np.float64)
    for name, v in (("the successes of the records", k), ("the shots of the records", n)):
        if not np.all(np.isfinite(v)) or np.any(v != np.floor(v)):
            raise ValueError(f"{name} must be finite and integer-valued: the readings are counts")
    if np.any(n < 1):
        raise ValueError("the shots of the records must be >= 1")
    if np.any(k < 0) or np.any(k > n):
        raise ValueError("the successes of the records must lie in 0..shots")
    return lgamma_plus_one(n) - lgamma_plus_one(k) - lgamma_plus_one(n - k)


def state_fields(obj):
    """What a snapshot keeps of this class besides the base class's (_state.py): ``shots``."""
    return {"shots": np.array(obj.shots, dtype=np.float64)}


def kwargs_from_state(fields):
    """The constructor's keyword arguments from ``state_fields()``'s dict."""
    return {"shots": np.array(fields["shots"], dtype=np.float64)}


class OptBayesExptBinomial(CountReadings):
    """``shots``: the shots per reading, a scalar or one value per channel (a public attribute; it may be reassigned
    between calls).  It is the ``n`` of a record that brings none, and what ``yvar_noise_model()`` divides by:
    ``nu_bar_c(s) = sum w p_c (1 - p_c) / W / shots_c``, the variance of the fraction k / n.  Needs a DeviceModel of at
    most 3 channels whose outputs are probabilities.

    ``utility_method``: ``"mutual_information"`` (default; ``utility_information()``: the information of the NEXT
    SHOT, whatever ``shots`` is) or any name the base class knows, which then works on the Gaussian approximation
    ``yvar_noise_model()`` gives.  ``pdf_update((setting, k))`` or ``((setting, k, n))``; ``likelihood()``:
    ``L_i = exp(sum_c [k_c log p_c,i + (n_c - k_c) log1p(-p_c,i)])``, 0 for a particle with a probability that is NaN
    or outside [0, 1].  ``records_loglik()`` and ``pdf_update_batch()`` take a recorded table of clicks at once.  The
    summaries that take a per-record Gaussian ``sigma`` raise ``NotImplementedError``; for counts ask ``count_logpmf()``,
    ``count_cdf()``, ``count_pvalue()`` (is this record plausible?) and ``count_pmf()``, ``count_quantile()``,
    ``count_interval()`` (where will the next k fall?), with ``shots`` at most OBE_COUNT_MAX_OUTCOMES."""
    _NOISE_FROM = "shots"
    _REFUSAL = ("takes readings with a Gaussian sigma per record, but this object's readings are counts (k successes "
                "in n shots): count_logpmf(), count_cdf(), count_pvalue(), count_quantile() and count_interval() "
                "score and band them (records_loglik() and pdf_update_batch() take the records without sigma)")
    _COUNT_LAW = CountLaw(_lib.OBE_COUNT_BINOMIAL, "shots", check_shots, check_count_table,
                          lambda shots: int(np.max(shots)), True)

    def __init__(self, measurement_model, setting_values, parameter_samples, constants, shots=1,
                 utility_method=INFORMATION, **kwargs):
        self._need_device_model(measurement_model)
        check_channels(measurement_model.n_channels)
        check_shots(shots, measurement_model.n_channels)
        CountReadings.__init__(self, measurement_model, setting_values, parameter_samples, constants, utility_method,
                               **kwargs)
        self.shots = shots

    def _likelihood_device(self, y_model, measurement_record):
        """The likelihood as a device tensor: the counts of a record against every particle's probabilities.
        ``y_model`` None: the model is evaluated at the record's setting inside the same kernel."""
        given = measurement_record[2] if len(measurement_record) > 2 else None
        shots = check_shots(self.shots, self.n_channels) if given is None else given
        n, kk, nn = check_counts(measurement_record[1], shots, self.n_channels)
        return self._likelihood_call("obe_binomial_likelihood", y_model, measurement_record[0], (kk, nn), n)

    # -- a recorded data set in one call ---------------------------------------------------
    def _own_records(self, settings, y_meas, shots=None):
        """The records of ``records_loglik()`` / ``pdf_update_batch()``: successes of all C channels and their shots;
        ``l`` carries sum log C(n, k), the full log probability."""
        shots = check_shots(self.shots, self.n_channels) if shots is None else shots
        x, k, n = check_own_records(settings, y_meas, "shots", shots, self.allsettings.shape[0], self.n_channels)
        log_binom = check_count_table(k, n)
        return _batch.OwnRecords(self, "obe_binomial_records_loglik", np.vstack([x, k, n]), x.shape[0], True,
                                 tile_sums(log_binom))

    def records_loglik(self, settings, y_meas, sigma=None, *, shots=None):
        """``(N_p,)`` float64: ``l_i = sum_r sum_c [k log p + (n - k) log1p(-p) + log C(n, k)]``, the log probability of
        the recorded successes ``y_meas`` (all C channels) per particle, whatever its weight.  ``shots``: None (the
        object's ``shots``), a scalar, ``(C,)``, ``(C, n_r)`` or for one channel ``(n_r,)``.  NaN where a probability
        is NaN or outside [0, 1], -inf where a record is impossible.  ``sigma`` must stay None."""
        self._no_record_sigma("records_loglik", sigma)
        return _batch.records_loglik(self, settings, y_meas, shots=shots)

    def pdf_update_batch(self, settings, y_meas, sigma=None, tempered=True, max_stages=64, on_stage=None, *, shots=None):
        """``OptBayesExpt.pdf_update_batch()`` with the binomial likelihood of the recorded successes; ``shots`` as
        ``records_loglik()`` takes it.  ``last_batch_update["log_evidence"]`` is the log probability of the records,
        binomial coefficients included.  ``sigma`` must stay None."""
        self._no_record_sigma("pdf_update_batch", sigma)
        return _batch.pdf_update_batch(self, settings, y_meas, None, tempered, max_stages, on_stage, shots=shots)

    # -- count-aware scoring and reading bands: CountReadings' methods under this class's keyword ----------------------
    def count_logpmf(self, settings, counts, *, shots=None):
        """``CountReadings.count_logpmf()``: the joint one-step log evidence of each record, ``log C(n, k)`` included.
        ``shots`` as ``records_loglik()`` takes it."""
        return CountReadings.count_logpmf(self, settings, counts, side=shots)

    def count_cdf(self, settings, counts, upper=False, *, shots=None):
        """``CountReadings.count_cdf()``: per channel P(K <= k), or P(K >= k), of the recorded successes.  ``shots`` as
        ``records_loglik()`` takes it."""
        return CountReadings.count_cdf(self, settings, counts, upper, side=shots)

    def count_pvalue(self, settings, counts, *, shots=None):
        """``CountReadings.count_pvalue()``: the two-sided p-value of the recorded successes, per channel."""
        return CountReadings.count_pvalue(self, settings, counts, side=shots)

    def count_pmf(self, settings=None, count_max=None, *, shots=None):
        """``CountReadings.count_pmf()``: the predicted histogram of the next reading, ``(n_x, C, count_max + 2)``.
        ``count_max`` None: the largest ``shots`` (nothing lies above).  ``shots``: None (the object's), a scalar or ``(C,)``."""
        return CountReadings.count_pmf(self, settings, count_max, side=shots)

    def count_quantile(self, q, settings=None, count_max=None, full_output=False, *, shots=None):
        """``CountReadings.count_quantile()``: the smallest k with P(K <= k) >= q, ``(n_q, C, n_x)``."""
        return CountReadings.count_quantile(self, q, settings, count_max, full_output, side=shots)

    def count_interval(self, level=0.95, settings=None, count_max=None, full_output=False, *, shots=None):
        """``CountReadings.count_interval()``: ``(lo, hi)``, the band the next reading's successes fall in."""
        return CountReadings.count_interval(self, level, settings, count_max, full_output, side=shots)

    # -- one pass over settings x particles: the information and the variance of a shot --
    def _pass(self, begin, end, want_information):
        """Device ``(information (end - begin,) or None, nu_bar (C, end - begin))`` of the settings [begin, end) of the
        design grid.  ``nu_bar`` is cached until the particles, the weights or ``shots`` change; the information,
        divided by a ``cost_estimate()`` that may depend on anything, is formed anew by every call that wants it."""
        shots = check_shots(self.shots, self.n_channels)
        made = {}

        def compute():
            p, w = self._pw_tensors()
            n, n_p = end - begin, p.shape[1]
            nu = torch.empty((self.n_channels, max(n, 1)), dtype=torch.float64, device=self._device)
            info = torch.empty(max(n, 1), dtype=torch.float64, device=self._device) if want_information else None
            if n > 0:
                cost_t, cost_s = self._cost_device(whole_grid=True) if want_information else (None, 1.0)
                into_call, rows = self._per_channel(shots)
                model_call(self, "obe_binomial_information", "obe_binomial_workspace_bytes", (n_p, n, self.n_channels),
                           _P(self._settings_dev.data_ptr() + 8 * begin), self._n_settings, n, _ptr(p), n_p, n_p,
                           _ptr(w), into_call, None if cost_t is None else _P(cost_t.data_ptr() + 8 * begin),
                           cost_s, None if info is None else _ptr(info), _ptr(nu))
                if rows is not None:
                    nu /= rows
            made["info"] = info
            return nu

        if want_information:
            self._nu_bar.pop((begin, end), None)
        nu = self._nu_bar_cached(begin, end, shots.tobytes(), compute)
        return made.get("info"), nu

    def utility_information(self):
        """``U (N_s,)`` over the design grid: the mutual information, in nats, between the parameters and the joint
        outcome of the next shot in every channel, divided by ``cost_estimate()``; NaN where no particle contributes.
        On a sharded object every rank sums its slice of the settings and the slices are gathered."""
        return self._information_of_slice()


CLASS = OptBayesExptBinomial
