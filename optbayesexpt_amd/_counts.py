"""Is this count plausible, and where will the next count fall?  Scoring and reading bands for readings that are COUNTS.

``predictive_logpdf()`` / ``predictive_cdf()`` / ``reading_quantile()`` speak of a reading with Gaussian noise.  On
``OptBayesExptBinomial`` and ``OptBayesExptPoisson`` the next reading of channel c is a whole number with the class's own
pmf per particle, ``P_c,i(k) = Binomial(k; n, p_c,i)`` or ``Poisson(k; t r_c,i)``, and the answers are probabilities and
whole numbers: the mixture ``Pbar_c(k) = sum_i w_i P_c,i(k) / W`` (``count_pmf``), its tails at a recorded count
(``count_cdf``, ``count_pvalue``), its quantiles (``count_quantile``, ``count_interval``) and the joint one-step log
evidence of a record (``count_logpmf``).  The table takes points x particles x outcomes evaluations; it and what is
read off it are HIP kernels (csrc/obe_counts.hip, K20) and only the results travel.  The argument checks are plain
functions of this module (no device needed), the calls are tiled over the points so that one call's device table stays
below ``TABLE_BYTES_PER_CALL``; ``CountReadings`` (_ownnoise.py) has the methods, each class its ``Law``.  Nothing is
kept on the object.
"""
import math
import warnings

import numpy as np
import torch

from . import _lib
from ._devcall import cloud, column_tiles, model_call, ptr as _ptr
from ._predictive import check_settings
from ._reading import check_levels
from ._scoring import pvalue_from_tails

MAX_OUTCOMES = _lib.OBE_COUNT_MAX_OUTCOMES     # the largest count_max, shots and scored count
MAX_Q_PER_CALL = _lib.OBE_COUNT_MAX_LEVELS     # obe_count_quantiles: levels one call serves
TABLE_BYTES_PER_CALL = 1 << 28                 # the device table of one call, C x (count_max + 2) x points x 8 B, at most
RECORDS_PER_CALL = 1 << 16                     # records one obe_count_logpmf call is given


class Law:
    """What a class brings: ``code`` (OBE_COUNT_BINOMIAL / OBE_COUNT_POISSON), ``name`` of its side keyword (``shots``,
    ``exposure``), ``check_grid_side(value, C)`` -> (C,) for the design grid, ``check_table(counts, side)`` -> the
    (C, n_r) per-record constants (the class's ``check_count_table``), ``default_max(side)`` -> count_max left out,
    and ``whole_side``: the side datum is itself a count (shots), bounded like one."""

    def __init__(self, code, name, check_grid_side, check_table, default_max, whole_side):
        self.code, self.name, self.check_grid_side, self.check_table = code, name, check_grid_side, check_table
        self.default_max, self.whole_side = default_max, whole_side


# ---------------------------------------------------------------------------------------- argument checks (host)
def check_count_max(count_max, default):
    """A whole number in 0..OBE_COUNT_MAX_OUTCOMES; None: ``default`` (under the same rule)."""
    if count_max is None:
        count_max = default
    if isinstance(count_max, (bool, np.bool_)) or not isinstance(count_max, (int, np.integer)):
        raise ValueError(f"count_max must be a whole number in 0..{MAX_OUTCOMES}, got {count_max!r}")
    if not 0 <= count_max <= MAX_OUTCOMES:
        raise ValueError(f"count_max must lie in 0..{MAX_OUTCOMES} (OBE_COUNT_MAX_OUTCOMES), got {count_max!r}")
    return int(count_max)


def check_bound(what, values):
    """``values`` (checked whole numbers) are at most OBE_COUNT_MAX_OUTCOMES, or ``ValueError``."""
    if np.size(values) and np.max(values) > MAX_OUTCOMES:
        raise ValueError(f"{what} must be at most {MAX_OUTCOMES} (OBE_COUNT_MAX_OUTCOMES) for the count_* methods, "
                         f"got {np.max(values):g}")


def check_scored_records(law, settings, counts, side, default_side, n_setdims, n_channels):
    """``(x (n_setdims, n_r), k (C, n_r), side (C, n_r), constants (C, n_r), single)`` of the records to score,
    everything broadcast to one ``n_r``: ``_ownnoise.check_own_records``' rules (all C channels; ``side`` a scalar,
    ``(C,)``, ``(C, n_r)`` or for one channel ``(n_r,)``; None: ``default_side``, the object's attribute), the class's
    ``check_count_table`` for the values, and OBE_COUNT_MAX_OUTCOMES for the counts (and the shots).  ``single``: one
    record, given as ``pdf_update`` takes it."""
    from ._ownnoise import check_own_records
    x, k, b = check_own_records(settings, counts, law.name, default_side if side is None else side, n_setdims,
                                n_channels)
    try:
        single = all(np.ndim(r) == 0 for r in settings) and np.ndim(counts) == (0 if n_channels == 1 else 1)
    except TypeError:
        single = False
    constants = law.check_table(k, b)
    check_bound("the counts of a scored record", k)
    if law.whole_side:
        check_bound(f"the {law.name} of a scored record", b)
    return x, k, b, constants, single and x.shape[1] == 1


def check_grid_request(law, settings, side, default_side, n_setdims, n_channels):
    """``(x (n_setdims, n_x) or None for the design grid, side (C,))``: points as ``predict()`` takes them; ``side`` a
    scalar or ``(C,)`` under the class's own rule, None: ``default_side``."""
    x = None if settings is None else check_settings(settings, n_setdims)
    b = law.check_grid_side(default_side if side is None else side, n_channels)
    if law.whole_side:
        check_bound(law.name, b)
    return x, b


def check_level(level):
    try:
        level = float(level)
    except (TypeError, ValueError):
        raise ValueError(f"level must be a number in (0, 1), got {level!r}") from None
    if not 0.0 < level < 1.0:
        raise ValueError(f"level must lie in the open interval (0, 1), got {level!r}")
    return level


def points_per_call(n_channels, count_max):
    """The points one obe_count_table call is given: its table stays below ``TABLE_BYTES_PER_CALL``."""
    return max(1, TABLE_BYTES_PER_CALL // (8 * n_channels * (count_max + 2)))


def log_factorials():
    """``lgamma(k + 1)`` for k = 0 .. OBE_COUNT_MAX_OUTCOMES + 1: obe_count_table's d_logfact, on the host."""
    return np.array([math.lgamma(k + 1.0) for k in range(MAX_OUTCOMES + 2)])


# ------------------------------------------------------------------------------------------------- device calls
_LOGFACT = {}              # device -> the table above


def _logfact(device):
    key = str(device)
    if key not in _LOGFACT:
        _LOGFACT[key] = torch.from_numpy(log_factorials()).to(device)
    return _LOGFACT[key]


def _law(obe):
    law = getattr(obe, "_COUNT_LAW", None)
    if law is None:
        raise TypeError(f"{type(obe).__name__} has no counting likelihood: the count_* methods are those of "
                        "OptBayesExptBinomial and OptBayesExptPoisson")
    return law


def _table(obe, law, part, n_s, count_max, p, w):
    """Device ``(C, count_max + 2, n)`` table of the points ``part`` = [settings (n_s rows); side (C rows)]."""
    n, n_c, n_p = part.shape[1], obe.n_channels, p.shape[1]
    pmf = torch.empty((n_c, count_max + 2, n), dtype=torch.float64, device=obe._device)
    model_call(obe, "obe_count_table", "obe_count_workspace_bytes", (n_p, n, n_c, count_max), law.code,
               _ptr(part), n, n, _ptr(part[n_s:]), n, _ptr(_logfact(obe._device)), _ptr(p), n_p, n_p, _ptr(w),
               count_max, _ptr(pmf))
    return pmf


def _grid_points(obe, law, settings, side):
    """Device [settings; side] (n_s + C, n_x) of a design-grid request, and n_s, side (C,)."""
    x, b = check_grid_request(law, settings, side, getattr(obe, law.name), obe.allsettings.shape[0], obe.n_channels)
    dev = obe._device
    x = obe._settings_dev if x is None else torch.from_numpy(x).to(dev)      # (the whole design grid, sharded or not)
    rows = torch.from_numpy(b).to(dev).reshape(-1, 1).expand(-1, x.shape[1])
    return torch.cat([x, rows]).contiguous(), x.shape[0], b


def count_pmf(obe, settings=None, count_max=None, side=None):
    law = _law(obe)
    points, n_s, b = _grid_points(obe, law, settings, side)
    count_max = check_count_max(count_max, law.default_max(b))
    p, w = cloud(obe)
    n_c = obe.n_channels
    out = np.empty((points.shape[1], n_c, count_max + 2))
    for start, part in column_tiles(points, points_per_call(n_c, count_max)):
        pmf = _table(obe, law, part, n_s, count_max, p, w)
        out[start:start + part.shape[1]] = pmf.permute(2, 0, 1).cpu().numpy()
    return out


def count_quantile(obe, q, settings=None, count_max=None, full_output=False, side=None, _stack=4):
    law = _law(obe)
    qs, scalar = check_levels(q)
    points, n_s, b = _grid_points(obe, law, settings, side)
    count_max = check_count_max(count_max, law.default_max(b))
    p, w = cloud(obe)
    n_c, n_x = obe.n_channels, points.shape[1]
    out = np.empty((qs.size, n_c, n_x))
    for start, part in column_tiles(points, points_per_call(n_c, count_max)):
        n = part.shape[1]
        pmf = _table(obe, law, part, n_s, count_max, p, w)
        for q0 in range(0, qs.size, MAX_Q_PER_CALL):
            part_q = np.ascontiguousarray(qs[q0:q0 + MAX_Q_PER_CALL])
            d_out = torch.empty((part_q.size, n_c, n), dtype=torch.float64, device=obe._device)
            obe._mlib.call("obe_count_quantiles", _ptr(pmf), n_c, count_max, n, _lib.host_ptr(part_q), part_q.size,
                           _ptr(d_out), obe._stream())
            out[q0:q0 + part_q.size, :, start:start + n] = d_out.cpu().numpy()
    beyond = np.isposinf(out)                  # (+inf: the level lies beyond count_max; NaN: nobody contributes)
    n_beyond = int(np.count_nonzero(beyond))
    out[beyond] = np.nan
    if n_beyond:
        warnings.warn(f"count_quantile: {n_beyond} of {out.size} results lie beyond count_max = {count_max} and are "
                      "NaN: raise count_max", RuntimeWarning, stacklevel=_stack)     # (the caller of the class's method)
    if scalar:
        out = out[0]
    return (out, {"beyond": n_beyond}) if full_output else out


def count_interval(obe, level=0.95, settings=None, count_max=None, full_output=False, side=None):
    level = check_level(level)
    got = count_quantile(obe, ((1.0 - level) / 2.0, (1.0 + level) / 2.0), settings, count_max, full_output, side, 5)
    if full_output:
        return got[0][0], got[0][1], got[1]
    return got[0], got[1]


def count_tails(obe, settings, counts, side=None):
    """``(lower, upper)``, each ``(C, n_r)``: P(K_c <= k_c) and P(K_c >= k_c), both with k itself."""
    law = _law(obe)
    n_c, n_s = obe.n_channels, obe.allsettings.shape[0]
    x, k, b, _, _ = check_scored_records(law, settings, counts, side, getattr(obe, law.name), n_s, n_c)
    # the window: every recorded count, and for shots all of 0..n (nothing above, then)
    count_max = int(max(k.max(), b.max() if law.whole_side else 0))
    p, w = cloud(obe)
    dev = obe._device
    stacked = torch.from_numpy(np.vstack([x, b, k])).to(dev)
    n_r = x.shape[1]
    lower, upper = np.empty((n_c, n_r)), np.empty((n_c, n_r))
    for start, part in column_tiles(stacked, points_per_call(n_c, count_max)):
        n = part.shape[1]
        pmf = _table(obe, law, part, n_s, count_max, p, w)
        d_lo = torch.empty((n_c, n), dtype=torch.float64, device=dev)
        d_up = torch.empty_like(d_lo)
        obe._mlib.call("obe_count_tails", _ptr(pmf), n_c, count_max, n, _ptr(part[n_s + n_c:]), n, _ptr(d_lo),
                       _ptr(d_up), obe._stream())
        lower[:, start:start + n] = d_lo.cpu().numpy()
        upper[:, start:start + n] = d_up.cpu().numpy()
    return lower, upper


def count_cdf(obe, settings, counts, upper=False, side=None):
    return count_tails(obe, settings, counts, side)[1 if upper else 0]


def count_pvalue(obe, settings, counts, side=None):
    return pvalue_from_tails(*count_tails(obe, settings, counts, side))


def count_logpmf(obe, settings, counts, side=None):
    law = _law(obe)
    n_c, n_s = obe.n_channels, obe.allsettings.shape[0]
    x, k, b, constants, single = check_scored_records(law, settings, counts, side, getattr(obe, law.name), n_s, n_c)
    const = np.array([math.fsum(col) for col in constants.T.tolist()]).reshape(1, -1)
    p, w = cloud(obe)
    n_r, n_p, dev = x.shape[1], p.shape[1], obe._device
    stacked = torch.from_numpy(np.vstack([x, k, b, const])).to(dev)
    out = np.empty(n_r)
    for start, part in column_tiles(stacked, RECORDS_PER_CALL):
        n = part.shape[1]
        d_out = torch.empty(n, dtype=torch.float64, device=dev)
        model_call(obe, "obe_count_logpmf", "obe_count_workspace_bytes", (n_p, n, n_c, 0), law.code,
                   _ptr(part), n, n, _ptr(part[n_s:]), n, _ptr(part[n_s + n_c:]), n, _ptr(part[n_s + 2 * n_c:]),
                   _ptr(p), n_p, n_p, _ptr(w), _ptr(d_out))
        out[start:start + n] = d_out.cpu().numpy()
    return float(out[0]) if single else out
