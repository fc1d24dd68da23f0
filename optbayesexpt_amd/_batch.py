"""Assimilating a recorded data set where the cloud lives: the joint log-likelihood of many records per particle, and
the update from it in one stage or — the standard remedy for the collapse a joint update of many records causes —
in adaptively tempered stages.

``pdf_update()`` takes one reading at a time; a recorded spectrum, yesterday's scan or a second model to compare
evidences meant a loop of R calls.  Here ``records_loglik()`` forms ``l_i = sum_r log p(y_r | x_r, theta_i)`` with
records x particles evaluations that stay on the chip (csrc/obe_predict.hip, K13a; K19 for the classes of
_ownnoise.py, whose likelihood is their own: ``OptBayesExpt._batch_records()`` is the seam), and ``pdf_update_batch()``
multiplies the weights by ``exp(kappa delta (l_i - m))`` stage by stage (csrc/obe_batch.hip, K13b + the existing
``obe_bayes_update_lik``), each stage's ``delta`` the largest that keeps ``N_eff / N`` at the resample threshold, with
the reference's resample (particlepdf.py:260-310) between stages.  The argument checks and the stage search are plain
functions of this module (no device needed); ``OptBayesExpt`` has the methods.
"""
import math
import warnings

import numpy as np
import torch

from . import _lib
from ._devcall import column_tiles, model_call, ptr as _ptr
from ._scoring import _noise_rows, check_records

RECORDS_PER_CALL = 1 << 16                     # records one library call is given
TRIALS_PER_PASS = _lib._H["OBE_TEMPERED_MAX_TRIALS"]
TEMPERED_WS_BYTES = _lib._H["OBE_TEMPERED_WS_BYTES"]
SEARCH_BITS = 32                               # a stage's delta is a multiple of delta_max 2^-32: 8 passes of 16 trials
assert TRIALS_PER_PASS == 16 and SEARCH_BITS % 4 == 0


# ---------------------------------------------------------------------------------------- argument checks (host)
def check_batch_arguments(tempered, max_stages, on_stage):
    """``(tempered, max_stages)`` as a bool and an int >= 1; ``on_stage`` None or callable."""
    if not isinstance(tempered, (bool, np.bool_)):
        raise TypeError(f"tempered must be True or False, got {tempered!r}")
    if isinstance(max_stages, (bool, np.bool_)) or not isinstance(max_stages, (int, np.integer)):
        raise TypeError(f"max_stages must be an integer, got {max_stages!r}")
    if max_stages < 1:
        raise ValueError(f"max_stages must be at least 1, got {max_stages}")
    if on_stage is not None and not callable(on_stage):
        raise TypeError("on_stage must be callable: on_stage(info) is called after every stage")
    return bool(tempered), int(max_stages)


def check_choke(choke):
    """kappa, the exponent every likelihood is raised to (obe_base.py:458-459): 1 without a choke."""
    if choke is None:
        return 1.0
    kappa = float(choke)
    if not (math.isfinite(kappa) and kappa >= 0.0):
        raise ValueError(f"a batch update needs a finite choke >= 0, got {choke!r}")
    return kappa


def refuse_host_model(obe):
    if obe._device_model is None:
        raise TypeError("a batch update evaluates the model on the device: pass a device model "
                        "(models.from_function / models.from_expression turn a formula into one), not a plain "
                        "Python model_function")
    if obe._likelihood_overridden():
        raise TypeError("a batch update forms the object's own likelihood of the records on the device; this object "
                        "overrides likelihood(): loop pdf_update() instead")


# ---------------------------------------------------------------------------------------- the stage search (host)
def trial_delta(delta_max, k):
    """The grid point k of a stage's search: ``delta_max k 2^-32`` (k 2^-32 is exact, one rounding)."""
    return delta_max * (k / float(1 << SEARCH_BITS))


def search_stage(ess_fractions, delta_max, threshold):
    """The largest ``delta = delta_max k 2^-32`` (k = 1 .. 2^32) whose ``N_eff / N`` is >= ``threshold``, found by
    bisection of [0, delta_max] to 32 halvings, 16 grid points per pass: ``ess_fractions(deltas)`` returns
    ``N_eff / N`` for up to 16 values of delta at once (one pass over the cloud).  Assumes, as every bisection does,
    that ``N_eff`` falls as delta grows.  Returns ``(k, passed)``: the first pass tests delta_max itself (k = 2^32:
    the whole remainder, one stage); ``passed`` False: not even the smallest grid point (k = 1) passes — the
    caller takes it and warns."""
    step = 1 << (SEARCH_BITS - 4)
    lo = 0                                       # the largest k known to pass (0: none yet; delta = 0 changes nothing)
    first = True
    while step >= 1:
        ks = [lo + j * step for j in range(1, 17 if first else 16)]
        fractions = ess_fractions([trial_delta(delta_max, k) for k in ks])
        passing = [k for k, f in zip(ks, fractions) if f >= threshold]
        if first and passing and passing[-1] == ks[-1]:
            return ks[-1], True
        # (bisection: the passing points of a pass are its first few; the largest of them is kept)
        if passing:
            lo = max(passing)
        first = False
        step >>= 4
    return (lo, True) if lo > 0 else (1, False)


def ess_fraction(s1, s2, n_particles):
    """``N_eff / N`` of the weights ``w exp(a (l - m)) / S1``: ``S1^2 / S2 / N`` (0 when nothing is left)."""
    return (s1 * s1 / s2) / n_particles if s2 > 0.0 else 0.0


# ------------------------------------------------------------------------------------------------- device calls
class GaussianRecords:
    """The records of a request on the device and ``loglik()``, the (N_p,) device tensor of l for the object's PRESENT
    cloud: the one seam of the engine below.  ``OptBayesExpt._batch_records()`` returns what serves the object's
    likelihood; this one is the Gaussian with a sigma per record or from the cloud's noise rows (K13a), the classes of
    _ownnoise.py bring their own (``OwnRecords``)."""

    def __init__(self, obe, settings, y_meas, sigma):
        rows = _noise_rows(obe)
        x, y, s, _ = check_records(settings, y_meas, sigma, obe.allsettings.shape[0], obe.n_channels, rows)
        self.obe = obe
        #: stacked device rows [x; y; sigma]
        self.stacked = torch.from_numpy(np.vstack([x, y] + ([] if s is None else [s]))).to(obe._device)
        self.n_s, self.has_sigma = x.shape[0], s is not None

    def loglik(self):
        """Tiled by RECORDS_PER_CALL per library call (later tiles are added, in tile order); a workspace of its
        own."""
        obe, n_s = self.obe, self.n_s
        rows = None if self.has_sigma else _noise_rows(obe)
        n_c = obe.n_channels
        p = obe._parameters.tensor()                # (host edits of the cloud are uploaded here)
        n_p = p.shape[1]
        out = torch.empty(n_p, dtype=torch.float64, device=obe._device)
        for start, part in column_tiles(self.stacked, RECORDS_PER_CALL):
            n = part.shape[1]
            d_x, d_y = part[:n_s], part[n_s:n_s + n_c]
            d_s = _ptr(part[n_s + n_c:]) if self.has_sigma else None
            model_call(obe, "obe_records_loglik", "obe_records_loglik_workspace_bytes", (n_p, n, n_c),
                       _ptr(d_x), n, n, _ptr(d_y), n, d_s, n, None if rows is None else _lib.host_ptr(rows),
                       _ptr(p), n_p, n_p, 1 if start else 0, _ptr(out))
        return out


class OwnRecords:
    """The seam for a class whose likelihood is its own (_ownnoise.py): ``rows`` (n_setdims + (1 + side) C, n_r) host
    rows [x; reading; side data], ``constants(begin, end)`` the particle-independent part of the records [begin, end)
    as a host double, ``entry`` the class's ``*_records_loglik`` entry point and ``extra`` the host arrays it takes
    between the reading's stride and ``constant`` (``side_rows`` True: the side data's address and stride instead)."""

    def __init__(self, obe, entry, rows, n_setdims, side_rows, constants, extra=()):
        self.obe, self.entry, self.n_s, self.side_rows = obe, entry, n_setdims, side_rows
        self.stacked = torch.from_numpy(np.ascontiguousarray(rows)).to(obe._device)
        self.constants, self.extra = constants, tuple(extra)

    def loglik(self):
        obe, n_s, n_c = self.obe, self.n_s, self.obe.n_channels
        p = obe._parameters.tensor()                # (host edits of the cloud are uploaded here)
        n_p = p.shape[1]
        out = torch.empty(n_p, dtype=torch.float64, device=obe._device)
        for start, part in column_tiles(self.stacked, RECORDS_PER_CALL):
            n = part.shape[1]
            side = (_ptr(part[n_s + n_c:]), n) if self.side_rows else ()
            model_call(obe, self.entry, self.entry + "_workspace_bytes", (n_p, n, n_c),
                       _ptr(part[:n_s]), n, n, _ptr(part[n_s:n_s + n_c]), n, *side,
                       *[_lib.host_ptr(a) for a in self.extra], float(self.constants(start, start + n)), _ptr(p),
                       n_p, n_p, 1 if start else 0, _ptr(out))
        return out


def _records_of(obe, settings, y_meas, sigma, side):
    """What ``obe._batch_records()`` gives; the Gaussian records for whatever has no such method."""
    make = getattr(obe, "_batch_records", None)
    if make is None:
        return GaussianRecords(obe, settings, y_meas, sigma)
    return make(settings, y_meas, sigma, **side)


def records_loglik(obe, settings, y_meas, sigma=None, **side):
    refuse_host_model(obe)
    return _records_of(obe, settings, y_meas, sigma, side).loglik().cpu().numpy()


class _Sums:
    """obe_tempered_sums on one (l, weights) pair: m, sum w and per trial (S1, S2), in a workspace and a page-locked
    landing zone of the call's own."""

    def __init__(self, obe):
        self.obe, self.loglik = obe, None
        self.ws = torch.empty(TEMPERED_WS_BYTES // 8, dtype=torch.float64, device=obe._device)
        self.host = _lib.pinned_array(2 + 2 * TRIALS_PER_PASS)
        self.exponents = np.zeros(TRIALS_PER_PASS)

    def __call__(self, exponents):
        """``(m, sum w, [(S1, S2), ...])`` for up to 16 exponents."""
        obe, k = self.obe, len(exponents)
        self.exponents[:k] = exponents
        w = obe._weights.tensor()
        if w.shape[0] != self.loglik.shape[0]:
            raise ValueError("particles and particle_weights have different lengths")
        obe._lib.call("obe_tempered_sums", _ptr(self.loglik), _ptr(w), w.shape[0], _lib.host_ptr(self.exponents), k,
                      _ptr(self.ws), TEMPERED_WS_BYTES, _lib.host_ptr(self.host), obe._stream())
        h = self.host
        return float(h[0]), float(h[1]), [(float(h[2 + 2 * t]), float(h[3 + 2 * t])) for t in range(k)]


def _apply_stage(obe, loglik, exponent, shift):
    """w <- normalised(w exp(exponent (l - shift))) through obe_tempered_likelihood + obe_bayes_update_lik; returns
    sum w'^2."""
    n =loglik.shape[0]
    lik = torch.empty(n, dtype=torch.float64, device=obe._device)
    obe._lib.call("obe_tempered_likelihood", _ptr(loglik), n, float(exponent), float(shift), _ptr(lik), obe._stream())
    w = obe._weights.tensor()
    obe._unfused_update(obe._lib, "obe_bayes_update_lik", _ptr(lik), n, _ptr(w), _ptr(obe._ws), obe._ws_bytes,
                        _lib.host_ptr(obe._host_out), obe._stream())
    return float(obe._host_out[1])


def _n_eff(sum_w2):
    return 1.0 / sum_w2 if sum_w2 != 0.0 else float("inf")


def pdf_update_batch(obe, settings, y_meas, sigma=None, tempered=True, max_stages=64, on_stage=None, **side):
    from .obe_base import _LazyState
    tempered, max_stages = check_batch_arguments(tempered, max_stages, on_stage)
    refuse_host_model(obe)
    kappa = check_choke(obe.choke)
    records = _records_of(obe, settings, y_meas, sigma, side)
    # it behaves like an update: a sweep enqueued ahead reads the weights this call changes
    obe._drop_speculative_sweep()
    obe._await_host_moments()
    n_p = obe.n_particles
    threshold = float(obe.tuning_parameters["resample_threshold"])
    report = dict(stages=[], n_eff=[], resamples=0, log_evidence=None if obe.choke is not None else 0.0)
    obe.last_batch_update = report
    beta, warned = 0.0, False

    def record(delta, s1, sw, top, sum_w2):
        report["stages"].append(delta)
        report["n_eff"].append(_n_eff(sum_w2))
        if report["log_evidence"] is not None:
            with np.errstate(divide="ignore", invalid="ignore"):
                report["log_evidence"] += float(np.log(np.float64(s1) / np.float64(sw))) + delta * top

    sums = _Sums(obe)

    def stage_done(delta, beta, sum_w2):
        """The weights are the stage's: versions, the resample test's sum, the caller's look at them."""
        obe._weights.mark_device_written()
        obe._sumsq, obe._sumsq_key = sum_w2, obe._weights.version
        if on_stage is not None:
            on_stage(dict(stage=len(report["stages"]) - 1, delta=delta, beta=beta, n_eff=report["n_eff"][-1],
                          resamples=report["resamples"], log_evidence=report["log_evidence"]))

    while True:
        sums.loglik = loglik = records.loglik()       # (of the cloud as it is now)
        delta_max = 1.0 - beta
        last = not tempered
        if tempered and len(report["stages"]) + 1 >= max_stages:
            # the stage budget is spent: the whole remainder, and a warning if that breaks the threshold
            last = True
            _, _, ((s1, s2),) = sums([kappa * delta_max])
            if ess_fraction(s1, s2, n_p) < threshold:
                warnings.warn(f"pdf_update_batch: beta = {beta:.6g} after {max_stages - 1} tempered stage(s); the "
                              "remainder is applied at once (max_stages)", RuntimeWarning)
        if last:
            delta = delta_max
        else:
            def fractions(deltas):
                return [ess_fraction(s1, s2, n_p) for s1, s2 in sums([kappa * d for d in deltas])[2]]
            k, passed = search_stage(fractions, delta_max, threshold)
            last = k == 1 << SEARCH_BITS
            delta = delta_max if last else trial_delta(delta_max, k)
            if not passed and not warned:
                warned = True
                warnings.warn("pdf_update_batch: no tempering step keeps N_eff / N at the resample threshold "
                              f"({threshold}); the smallest step tested is taken", RuntimeWarning)
        top, sw, ((s1, _),) = sums([delta])       # (the evidence is that of the likelihood itself: kappa = 1)
        shift = top if math.isfinite(top) else 0.0
        sum_w2 = _apply_stage(obe, loglik, kappa * delta, shift)
        record(delta, s1, sw, shift, sum_w2)
        if last:
            break
        # a tempering stage: the resample follows whatever the resample test would say
        beta += delta
        obe.last_n_eff = report["n_eff"][-1]
        stage_done(delta, beta, sum_w2)
        obe._resample_reported()
        report["resamples"] += 1
        obe._parameters = obe._particles
        obe.enforce_parameter_constraints()
    # the last stage takes beta to exactly 1 and ends as pdf_update() does: the ordinary resample test, then the
    # constraints if it resampled
    stage_done(delta, 1.0, sum_w2)
    if obe.tuning_parameters["auto_resample"]:
        obe.resample_test()
        report["resamples"] += 1 if obe.just_resampled else 0
    obe._parameters = obe._particles
    if obe.just_resampled:
        obe.enforce_parameter_constraints()
    obe._sweeps.update_finished(None, bool(obe.just_resampled))
    return _LazyState(obe)
