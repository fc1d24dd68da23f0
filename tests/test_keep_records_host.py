"""The host side of the keep buffer's records form (include/obe_hip.h: obe_sweep_bins_keep_records_bytes), no GPU: the
size function, its declaration and binding, and the flags words of the three values of
``tuning_parameters['sweep_bins_keep']``."""
import types

import numpy as np

from optbayesexpt_amd import _lib
from optbayesexpt_amd.obe_base import OptBayesExpt

DRAWS = (-5, 0, 1, 2, 63, 64, 65, 513, 4099, 262144, 1 << 20, 1 << 30)


def test_records_buffer_size():
    cdll = _lib.load().cdll
    small, large = cdll.obe_sweep_bins_keep_bytes, cdll.obe_sweep_bins_keep_records_bytes
    previous = 0
    for n in DRAWS:
        b, m = int(large(n)), max(n, 1)
        assert b % 16 == 0, n
        assert int(small(n)) + 32 * m <= b <= int(small(n)) + 32 * m + 64, (n, b)
        assert b >= previous, n
        previous = b
    assert large(0) == large(1) == large(-5)


def test_the_size_function_is_declared_exported_and_bound():
    name = "obe_sweep_bins_keep_records_bytes"
    assert name in _lib.declared_symbols()
    ret, args = _lib.PROTOTYPES[name]
    assert ret is _lib.c_int64 and args == [(_lib.c_int64, "n_draws")]
    assert _lib.PROTOTYPES[name] == _lib.PROTOTYPES["obe_sweep_bins_keep_bytes"]
    assert hasattr(_lib.load().cdll, name)
    assert name in _lib.MODEL_ENTRY_POINTS
    assert _lib.OBE_ABI_VERSION == 3                           # (a compatible addition)


def _attempts(keep):
    """(rebuilding attempt, reusing attempt) of an object with ``sweep_bins_keep = keep`` (test_kept_bins_host.py)."""
    from optbayesexpt_amd._sweepstate import SweepState
    fake = types.SimpleNamespace(_particles=types.SimpleNamespace(version=7), cons=np.array([0.1]), n_particles=100,
                                 tuning_parameters={"sweep_bins": "always"}, KAPPA_ENTER=1000.0, KAPPA_LEAVE=3000.0,
                                 SAFE_STREAK=3, SAFE_RETRY=64)
    if keep is not None:
        fake.tuning_parameters["sweep_bins_keep"] = keep
    fake._sweeps = SweepState(None, fake)
    fake._bins_keep_key = types.MethodType(OptBayesExpt._bins_keep_key, fake)
    forms = (0, 1, fake._bins_keep_key())
    first = fake._sweeps.first_attempt(fake._sweeps.form, False, True, fake.tuning_parameters, forms)
    assert fake._sweeps.after(first, 10.0, False, "never", True) is None
    return first, fake._sweeps.attempt_for(False, True, fake.tuning_parameters, forms)


def test_the_three_values_send_the_flags_words_of_before():
    bins, kept = _lib.OBE_SWEEP_BINS, _lib.OBE_SWEEP_BINS | _lib.OBE_SWEEP_BINS_KEPT
    for keep in (None, True, "grouping"):                      # (None: the default)
        first, second = _attempts(keep)
        assert first.keep is False and second.keep is True, keep
        assert (first.flags(False), second.flags(False)) == (bins, kept), keep
        assert second.flags(True) == kept | _lib.OBE_SWEEP_SPECULATIVE, keep
        assert second.inputs()["kept"] is True and first.inputs()["kept"] is False
    first, second = _attempts(False)
    assert first.keep is None and second.keep is None
    assert first.flags(False) == second.flags(False) == bins
