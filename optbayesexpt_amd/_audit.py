"""OBE_CHECK_DELIVERY=1 — an audit of how results reach the host (debug mode, host side only).

Kernels of libobe_hip deliver their few result scalars by writing page-locked host memory themselves, and the
host waits by WATCHING those words (csrc/obe_common.h: arm_host_words / wait_host_words) instead of
synchronising the stream.  That protocol is only correct if every word that is read was waited for, and three
races of rounds 4-5 were exactly violations of it (tests/test_gpu_delivery_audit.py names them).  With the mode
on, the protocol is checked by construction instead of by soak runs:

* every page-locked landing zone (``_lib.pinned_array``) is registered, one state per 8-byte word;
* a call that will deliver into a zone without waiting (the enqueue forms, ``obe_host_word(s)_arm``) marks the
  words it delivers ARMED — the table below restates, per entry point, which host words a call arms
  (include/obe_hip.h) —, a wait marks the words it covered DELIVERED (and checks that none of them still holds
  the armed bit pattern), a device synchronisation everything;
* a Python read of an ARMED word raises ``DeliveryError`` (the arrays handed out are an ndarray subclass whose
  ``__getitem__`` looks the touched words up);
* a zone that is handed back to the allocator — or re-registered at the same address — while words of it are
  ARMED is a violation too (recorded, raised by the next library call: finalisers cannot raise).

Off (the default) every hook is a no-op method of ``_NoAudit``.
"""
import bisect
import os

import numpy as np

# (_lib imports this module after it has defined these)
from ._lib import HOST_SENTINEL, OBE_SWEEP_NOWAIT, OBE_SWEEP_SPECULATIVE, PROTOTYPES, MomentLayout

try:
    _byte_bounds = np.lib.array_utils.byte_bounds          # numpy >= 2
except AttributeError:                                      # pragma: no cover
    _byte_bounds = np.byte_bounds


class DeliveryError(RuntimeError):
    """A host result word was read, or its memory released, before it had been waited for."""


class _NoAudit:
    on = False

    def wrap(self, a):
        return a

    def zone_created(self, addr, nbytes, keeper):
        pass

    def zone_released(self, keeper):
        pass

    def zone_freed(self, keeper, drained):
        pass

    def after_call(self, name, args):
        pass

    def synchronized(self):
        pass

    def raw(self, a):
        return a


class CheckedArray(np.ndarray):
    """A view of a landing zone whose element reads are checked against the zone's word states."""

    def __getitem__(self, key):
        res = np.ndarray.__getitem__(self, key)
        audit.check_read(self, key, res)
        return res


def _addr(x):
    if x is None:
        return None
    v = getattr(x, "value", x)
    return None if v is None else int(v)


def _int(x):
    return int(getattr(x, "value", x))


class _Zone:
    __slots__ = ("addr", "nbytes", "armed", "released")

    def __init__(self, addr, nbytes):
        self.addr, self.nbytes = addr, nbytes
        self.armed = np.zeros((nbytes + 7) // 8, dtype=bool)
        self.released = False


class _Audit(_NoAudit):
    on = True

    def __init__(self):
        self.starts = []          # sorted zone start addresses
        self.zones = {}           # start -> _Zone
        self.violations = []
        self.counts = dict(zones=0, armed=0, waited=0, reads=0, syncs=0)
        self.rules = {}           # entry point -> (rule, the argument positions of the parameters it reads)
        for fn, (rule, *names) in {**_RULES, **_BOUNDS_RULES, **_BATCH_RULES, **_KEEP_RULES}.items():
            params = [name for _, name in PROTOTYPES[fn][1]]
            self.rules[fn] = (rule, tuple(params.index(name) for name in names))

    # ---- zones ---------------------------------------------------------------------------------------
    def wrap(self, a):
        return a.view(CheckedArray)

    def raw(self, a):
        """The plain ndarray behind a checked view: for code that POLLS armed words on purpose."""
        return np.asarray(a).view(np.ndarray)

    def zone_created(self, addr, nbytes, keeper):
        old = self.zones.get(addr)
        if old is not None and old.armed.any():
            self.violations.append(f"landing zone at {addr:#x} handed out again while {int(old.armed.sum())} word(s) of "
                                   "its previous owner were still armed (a kernel of a dead object may write into it)")
        if old is None:
            bisect.insort(self.starts, addr)
        self.zones[addr] = _Zone(addr, nbytes)
        self.counts["zones"] += 1

    def zone_released(self, keeper):
        z = self.zones.get(keeper.data_ptr())
        if z is not None:
            z.released = True

    def zone_freed(self, keeper, drained):
        addr = keeper.data_ptr()
        z = self.zones.get(addr)
        if z is None:
            return
        if not drained and z.armed.any():
            self.violations.append(f"landing zone at {addr:#x} freed with {int(z.armed.sum())} armed word(s) and no "
                                   "device synchronisation in between")
            return                       # (stays registered: a re-use of the address is then reported as well)
        del self.zones[addr]
        self.starts.pop(bisect.bisect_left(self.starts, addr))

    def _find(self, addr):
        i = bisect.bisect_right(self.starts, addr) - 1
        if i < 0:
            return None
        z = self.zones[self.starts[i]]
        return z if addr < z.addr + z.nbytes else None

    def _mark(self, addr, n_words, armed):
        if addr is None or n_words <= 0:
            return
        z = self._find(addr)
        if z is None:
            return                       # (not one of this package's landing zones: a test's own buffer)
        w0 = (addr - z.addr) // 8
        z.armed[w0:w0 + n_words] = armed
        self.counts["armed" if armed else "waited"] += 1

    # ---- library calls -------------------------------------------------------------------------------
    def after_call(self, name, args):
        if self.violations:
            v, self.violations = self.violations, []
            raise DeliveryError("; ".join(v))
        rule = self.rules.get(name)
        if rule is not None:
            fn, positions = rule
            fn(self, *[args[i] for i in positions])

    def waited(self, addr, n_words):
        if addr is None:
            return
        words = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint64 * n_words).from_address(addr))
        if np.any(words == HOST_SENTINEL):
            raise DeliveryError(f"obe_host_words_wait returned with {int(np.sum(words == HOST_SENTINEL))} of {n_words} "
                                f"word(s) at {addr:#x} still armed")
        self._mark(addr, n_words, False)

    def synchronized(self):
        for z in self.zones.values():
            z.armed[:] = False
        self.counts["syncs"] += 1

    # ---- reads ---------------------------------------------------------------------------------------
    def check_read(self, arr, key, res):
        self.counts["reads"] += 1
        if isinstance(res, np.ndarray):
            if res.size == 0:
                return
            lo, hi = _byte_bounds(res)
        elif arr.ndim == 1 and isinstance(key, (int, np.integer)):
            lo = arr.ctypes.data + (int(key) % arr.shape[0]) * arr.strides[0]
            hi = lo + arr.itemsize
        else:
            lo, hi = _byte_bounds(arr)
        z = self._find(lo)
        if z is None:
            return
        w0, w1 = (lo - z.addr) // 8, (hi - z.addr + 7) // 8
        if z.armed[w0:w1].any():
            bad = (np.nonzero(z.armed[w0:w1])[0] + w0).tolist()
            raise DeliveryError(f"read of word(s) {bad} of the landing zone at {z.addr:#x} that were armed and have not "
                                "been waited for since (obe_host_words_wait on exactly those words, or a device "
                                "synchronisation)")


# ---- which host words a call arms / delivers (include/obe_hip.h) -----------------------------------------
# A rule gets the arguments of the parameters it names, in that order (resolved through _lib.PROTOTYPES).
def _arm(a, h_words, n_words=1):
    a._mark(_addr(h_words), _int(n_words), True)


def _wait(a, h_words, n_words=1):
    a.waited(_addr(h_words), _int(n_words))


def _update_enqueue(a, m, h_pinned_out):
    a._mark(_addr(h_pinned_out), MomentLayout(int(m.n_params)).update_len, True)


def _sweep(a, shifted, *h_results):
    nowait = bool(_int(shifted) & (OBE_SWEEP_SPECULATIVE | OBE_SWEEP_NOWAIT))
    for h in h_results:
        a._mark(_addr(h), 1, nowait)                     # (the synchronous form has waited for each of them itself)


def _resample_begin(a, n_dims, cdf_is_fresh, have_first_moments, h_f64, h_i64):
    layout = MomentLayout(_int(n_dims))
    lo = layout.first_len if _int(have_first_moments) else 0
    f64 = _addr(h_f64)
    a._mark(f64, 1, not _int(cdf_is_fresh))              # sum(w) of a CDF made by this call (a fresh one: the host's 1.0)
    a._mark(f64 + 8 * (layout.resample_k3 + lo), layout.total_len - lo, True)
    a._mark(_addr(h_i64), 2, True)


def _draw_indices(a, cdf_is_fresh, n_draws, d_idx, h_total_pinned):
    if not _int(cdf_is_fresh):
        a._mark(_addr(h_total_pinned), 1, True)          # sum(p): delivered by the call's kernels, never waited for by it
    a._mark(_addr(d_idx), _int(n_draws), True)           # the indices, when d_idx is the device view of a landing zone


def _mask_moments(a, n_dims, h_moments, h_changed):
    a._mark(_addr(h_moments), MomentLayout(_int(n_dims)).first_len, True)
    a._mark(_addr(h_changed), 1, True)


def _update_moments_delivered(a, m, h_out):
    a._mark(_addr(h_out), MomentLayout(int(m.n_params)).update_decision, False)     # (the words before the decision)


def _delivered(words):
    def rule(a, *h_results):
        for h in h_results:
            a._mark(_addr(h), words, False)
    return rule


# entry point -> (rule, the parameters it reads by their header names)
_RULES = {
    "obe_host_word_arm": (_arm, "h_pinned_word"),
    "obe_host_words_arm": (_arm, "h_pinned_words", "n_words"),
    "obe_host_word_wait": (_wait, "h_pinned_word"),
    "obe_host_words_wait": (_wait, "h_pinned_words", "n_words"),
    "obe_bayes_update_model_moments_enqueue": (_update_enqueue, "m", "h_pinned_out"),
    "obe_sweep_utility": (_sweep, "shifted", "h_best", "h_best_idx", "h_kappa"),
    "obe_resample_begin": (_resample_begin, "n_dims", "cdf_is_fresh", "have_first_moments", "h_f64", "h_i64"),
    "obe_draw_indices": (_draw_indices, "cdf_is_fresh", "n_draws", "d_idx", "h_total_pinned"),
    "obe_mask_nonpositive_moments": (_mask_moments, "n_dims", "h_moments", "h_changed"),
    "obe_mask_renorm_moments": (_mask_moments, "n_dims", "h_moments", "h_changed"),
    # synchronous forms: they wait for their own words before they return
    "obe_bayes_update_model": (_delivered(words=2), "h_out"),
    "obe_bayes_update_model_moments": (_update_moments_delivered, "m", "h_out"),
    "obe_bayes_update_lik": (_delivered(words=2), "h_out"),
    "obe_bayes_update_y": (_delivered(words=2), "h_out"),
    "obe_mask_nonpositive": (_delivered(words=1), "h_changed"),
    "obe_weight_sums": (_delivered(words=2), "h_out"),
    "obe_weight_cdf": (_delivered(words=1), "h_total"),
    "obe_utility_argmax": (_delivered(words=1), "h_best", "h_best_idx"),
    "obe_argmax": (_delivered(words=1), "h_best", "h_best_idx"),
}

# the declarative-bounds forms of the two masks (include/obe_hip.h: K6 for any rows): the words of their noise-only
# twins, under the parameter names of their own prototypes
_BOUNDS_RULES = {
    "obe_mask_bounds_moments": (_mask_moments, "n_dims", "h_first_moments", "h_count"),
    "obe_mask_bounds": (_delivered(words=1), "h_count"),
}

def _tempered_sums(a, n_trials, h_sums):
    a._mark(_addr(h_sums), 2 + 2 * _int(n_trials), False)       # (waited for before it returned, as obe_weight_sums' two)


# the sums of a tempered batch update (include/obe_hip.h: assimilating a recorded data set): obe_weight_sums' rule
# for as many words as the call has trials, under the parameter names of its own prototype
_BATCH_RULES = {
    "obe_tempered_sums": (_tempered_sums, "n_trials", "h_sums"),
}

# the sweep with a keep buffer behind its arguments (include/obe_hip.h: obe_sweep_utility_keep): obe_sweep_utility's
# rule, under the parameter names of its own prototype
_KEEP_RULES = {
    "obe_sweep_utility_keep": (_sweep, "shifted", "h_value", "h_index", "h_factor"),
}

audit = _Audit() if os.environ.get("OBE_CHECK_DELIVERY") == "1" else _NoAudit()

if audit.on and os.environ.get("OBE_AUDIT_REPORT"):
    import atexit
    import json

    def _report(path=os.environ["OBE_AUDIT_REPORT"]):
        # (appended: a test run starts several processes — ranks, tools — that all audit)
        with open(path, "a") as f:
            f.write(json.dumps(dict(audit.counts, pid=os.getpid(), pending_violations=audit.violations)) + "\n")
    atexit.register(_report)
