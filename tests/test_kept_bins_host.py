"""The host side of the kept bin grouping (include/obe_hip.h: obe_sweep_utility_keep), no GPU: the size of the keep
buffer, the binding of the new entry point, its delivery-audit rule and the key the object reuses the buffer by."""
import types

import numpy as np

from optbayesexpt_amd import _audit, _lib
from optbayesexpt_amd.obe_base import OptBayesExpt
from test_capi_symbols import _rule_effect, _w


def test_keep_buffer_size():
    lib = _lib.load()
    size = lib.cdll.obe_sweep_bins_keep_bytes
    head = 4 * (16 + 2 * (_lib.OBE_BIN_MAX + 2))              # the head and the two tables, in bytes
    previous = 0
    for n in (1, 2, 63, 64, 65, 513, 4099, 262144, 1 << 20, (1 << 30) - 1, 1 << 30):
        b = int(size(n))
        assert b % 16 == 0 and head + 4 * n <= b <= head + 4 * n + 32, n
        assert b >= previous
        previous = b
    assert size(0) == size(1) == size(-5)


def test_the_keep_entry_point_is_obe_sweep_utility_with_two_more_arguments():
    plain = _lib.PROTOTYPES["obe_sweep_utility"]
    keep = _lib.PROTOTYPES["obe_sweep_utility_keep"]
    assert keep[0] is plain[0]
    assert [t for t, _ in keep[1][:len(plain[1])]] == [t for t, _ in plain[1]]
    assert [(t, n) for t, n in keep[1][len(plain[1]):]] == [(_lib.c_void_p, "d_keep"), (_lib.c_int64, "keep_bytes")]
    assert _lib.OBE_SWEEP_BINS_KEPT == 64
    flags = [_lib.OBE_SWEEP_SHIFTED, _lib.OBE_SWEEP_SAFE, _lib.OBE_SWEEP_CELLS, _lib.OBE_SWEEP_SPECULATIVE,
             _lib.OBE_SWEEP_NOWAIT, _lib.OBE_SWEEP_BINS, _lib.OBE_SWEEP_BINS_KEPT]
    assert sum(flags) == 127 and all(f & (f - 1) == 0 for f in flags)          # seven distinct bits
    assert {"obe_sweep_utility_keep", "obe_sweep_bins_keep_bytes"} <= set(_lib.MODEL_ENTRY_POINTS)


def test_audit_rule_of_the_keep_entry_point_is_the_sweeps():
    assert set(_audit._KEEP_RULES) == {"obe_sweep_utility_keep"}
    kept = _lib.OBE_SWEEP_BINS | _lib.OBE_SWEEP_BINS_KEPT
    words = dict(h_value=_w(1), h_index=_w(2), h_factor=_w(3))
    assert _rule_effect("obe_sweep_utility_keep", shifted=kept, **words) == (set(), {1, 2, 3}, (0, 3))
    assert _rule_effect("obe_sweep_utility_keep", shifted=kept | _lib.OBE_SWEEP_SPECULATIVE, **words) \
        == ({1, 2, 3}, set(), (3, 0))
    assert _rule_effect("obe_sweep_utility_keep", shifted=kept | _lib.OBE_SWEEP_NOWAIT, h_value=_w(1), h_index=_w(2)) \
        == ({1, 2}, set(), (2, 0))


def test_the_key_follows_the_particles_the_width_and_the_count():
    from optbayesexpt_amd._sweepstate import SweepState
    fake = types.SimpleNamespace(_particles=types.SimpleNamespace(version=7), cons=np.array([0.1]), n_particles=100,
                                 tuning_parameters={"sweep_bins": "always"}, KAPPA_ENTER=1000.0, KAPPA_LEAVE=3000.0,
                                 SAFE_STREAK=3, SAFE_RETRY=64)
    fake._sweeps = SweepState(None, fake)            # (the mark and what an attempt does with it live there)
    for name in ("_bins_keep_key", "_bins_kept"):
        setattr(fake, name, types.MethodType(getattr(OptBayesExpt, name), fake))

    def _bins_kept_input(bins):
        """How a full sweep uses the keep buffer, as one of the sweep's inputs (``bins``: the plan takes them)."""
        forms = (0, 1 if bins else 0, fake._bins_keep_key())
        return fake._sweeps.attempt_for(False, True, fake.tuning_parameters, forms).inputs()["kept"]

    fake._bins_kept_input = _bins_kept_input
    assert not fake._bins_kept() and fake._bins_kept_input(True) is False and fake._bins_kept_input(False) is None
    # (set as the object sets it: a bin sweep that passed the buffer is collected with a finite kappa)
    rebuild = fake._sweeps.first_attempt(fake._sweeps.form, False, True, fake.tuning_parameters,
                                         (0, 1, fake._bins_keep_key()))
    assert rebuild.bins and rebuild.keep is False
    assert fake._sweeps.after(rebuild, 10.0, False, "never", True) is None
    assert fake._sweeps.bins_kept_for == fake._bins_keep_key()
    assert fake._bins_kept() and fake._bins_kept_input(True) is True
    fake._particles.version = 8                       # a resample, set_pdf, a write to the particles
    assert not fake._bins_kept()
    fake._particles.version = 7
    fake.cons = np.array([0.125])
    assert not fake._bins_kept()
    fake.cons = np.array([0.1])
    fake.n_particles = 101
    assert not fake._bins_kept()
    fake.n_particles = 100
    assert fake._bins_kept()
    fake.tuning_parameters["sweep_bins_keep"] = False
    assert fake._bins_kept_input(True) is None
