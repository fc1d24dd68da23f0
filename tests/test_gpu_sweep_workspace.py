"""How much of the workspace a sweep call asks for, and that it stays inside what it asked for (csrc/obe_sweep.hip:
prepare_sweep, carve_sweep_ws; csrc/obe_sweep_cells.h: CellLayout; csrc/obe_sweep_bins.h: BinLayout), for every form
and packed width of the call.

tests/golden/sweep_layout_parent.json holds, for every case below, the smallest ws_bytes the build of commit 03e02b5
("Rebuild the bin grouping in four launches; fold finalize into bin_eval") accepted, found on one MI355X by bisecting on
the refusal (tools/record_sweep_layout.py --gpu; a refusal is decided on the host and launches nothing), and the text of
that refusal.  The device buffer is always the object's whole workspace, zeroed before every call: only the size the
call is TOLD shrinks, so a carve that reached beyond what the call checked would still write inside the allocation -
and change the bits, or be seen as the refusal moving.  Asserted for every case:
  * the call is refused with the parent's error at the recorded size minus 8;
  * it is accepted at the recorded size;
  * yvar, utility, the best value, its index and kappa are then, by np.array_equal, those of the same call told the
    whole workspace; with a keep buffer, the buffer's bytes as well (a rebuild into it, then a reuse of it).
193 settings x 1 031 particles unless the case says otherwise."""
import json
import os

import numpy as np
import pytest

from test_gpu_bin_rebuild import keep_buffer, keep_bytes, sweep_call
from test_gpu_bin_sweep import prior_cloud, weights

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_layout_parent.json")
NS, N = 193, 1031
KEYS = ("yvar", "utility", "best", "idx", "kappa")


def _object(obe, model, x, cloud, cons, seed):
    o = obe.OptBayesExpt(model, (np.asarray(x, dtype=np.float64),), cloud.copy(), cons, utility_method="variance_full",
                         auto_resample=False, default_noise_std=500.0)
    o.particle_weights = weights(cloud.shape[1], seed)
    return o


def _lorentz(obe, n_settings=NS, n=N, peaks=1, expression=False):
    g = np.random.default_rng(9400 + peaks)
    cloud = prior_cloud(n, 9401)
    if peaks > 1:
        cloud = np.vstack([cloud[:1]] + [g.uniform(2, 4, (1, n)) for _ in range(peaks - 1)] + [cloud[1:]])
    if expression:
        import _expr_models
        model = _expr_models.expression_models()["lorentzian"]
    else:
        model = obe.models.lorentzian(peaks)
    return _object(obe, model, np.linspace(1.5, 4.5, n_settings), cloud, (0.1,), 9402)


def _coil(obe):
    g = np.random.default_rng(9403)
    cloud = np.array([g.uniform(0.9, 1.1, N), g.uniform(0.08, 0.12, N), g.uniform(0.9, 1.1, N), g.exponential(0.3, N)])
    return _object(obe, obe.models.coil(), np.logspace(-1, 1, NS), cloud, (), 9404)


def _draws(n_draws):
    return np.random.default_rng(9405 + n_draws).integers(0, N, n_draws).astype(np.int64)


def cases():
    """name -> (object maker, settings of the call, draws or None, flag names, with a keep buffer)"""
    return {
        "direct": (_lorentz, NS, None, (), False),
        "direct, shifted": (_lorentz, NS, None, ("OBE_SWEEP_SHIFTED",), False),
        "4100 x 1027, 8 per lane": (lambda obe: _lorentz(obe, 4100, 1027), 4100, None, (), False),
        "three peaks": (lambda obe: _lorentz(obe, peaks=3), NS, None, (), False),
        "coil, two channels": (_coil, NS, None, (), False),
        "draws 201 x 30": (lambda obe: _lorentz(obe, 201), 201, 30, (), False),
        "draws 700 x 300": (lambda obe: _lorentz(obe, 700), 700, 300, (), False),
        "cells": (_lorentz, NS, None, ("OBE_SWEEP_CELLS",), False),
        "bins": (_lorentz, NS, None, ("OBE_SWEEP_BINS",), False),
        "bins, keep buffer": (_lorentz, NS, None, ("OBE_SWEEP_BINS",), True),
        "bins and cells": (_lorentz, NS, None, ("OBE_SWEEP_BINS", "OBE_SWEEP_CELLS"), False),
        "bins, speculative": (_lorentz, NS, None, ("OBE_SWEEP_BINS", "OBE_SWEEP_SPECULATIVE"), False),
        "expression model, bins and cells": (lambda obe: _lorentz(obe, expression=True), NS, None,
                                             ("OBE_SWEEP_BINS", "OBE_SWEEP_CELLS"), False),
    }


class Call:
    """One case on the device: call(ws_bytes) with the workspace zeroed first."""

    def __init__(self, obe, case):
        import torch
        from optbayesexpt_amd import _lib
        maker, self.ns, n_draws, names, with_keep = case
        self.o = maker(obe)
        self.flags = 0
        for name in names:
            self.flags |= getattr(_lib, name)
        self.kept = _lib.OBE_SWEEP_BINS_KEPT
        self.idx = None if n_draws is None else torch.from_numpy(_draws(n_draws)).to(self.o._device)
        self.keep = keep_buffer(self.o, self.o.n_particles) if with_keep else None
        self.full = int(self.o._ws_bytes)

    def __call__(self, ws_bytes, reuse=False, refused=False, flags=None):
        self.o._ws.zero_()
        flags = self.flags if flags is None else flags
        return sweep_call(self.o, self.ns, draw_idx=self.idx, flags=flags | (self.kept if reuse else 0), keep=self.keep,
                          ws_bytes=ws_bytes, refused=refused)

    def accepted(self, ws_bytes):
        """(recording) whether the call is accepted at this size"""
        try:
            self(ws_bytes)
            return True
        except AssertionError:
            return False


def smallest_accepted(call):
    """(tools/record_sweep_layout.py) the smallest multiple of 8 bytes at which the call is accepted, and the refusal
    8 bytes below it."""
    lo, hi = 0, call.full // 8          # (refused at 8 lo, accepted at 8 hi)
    assert call.accepted(8 * hi) and not call.accepted(0)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if call.accepted(8 * mid):
            hi = mid
        else:
            lo = mid
    return {"ws_bytes": 8 * hi, "error": call(8 * hi - 8, refused=True)}


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)["smallest_workspace"]


@pytest.fixture(scope="module")
def obe(hip):
    import optbayesexpt_amd
    return optbayesexpt_amd


def same(got, want, what):
    for k in KEYS:
        assert got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k, np.flatnonzero(np.ravel(got[k] != want[k]))[:8])


CASES = list(cases())


@pytest.mark.parametrize("name", CASES)
def test_refused_below_the_parents_size_and_the_same_bits_at_it(obe, recorded, name):
    call = Call(obe, cases()[name])
    least, error = recorded[name]["ws_bytes"], recorded[name]["error"]
    assert 0 < least <= call.full
    assert call(least - 8, refused=True) == error
    if call.keep is not None:
        call.keep.zero_()
    whole = call(call.full)
    whole_keep = None if call.keep is None else keep_bytes(call.keep)
    if call.keep is not None:
        call.keep.zero_()
    same(call(least), whole, name)
    assert np.all(np.isfinite(whole["yvar"])) and np.isfinite(whole["kappa"]), name
    if call.keep is not None:
        assert np.array_equal(keep_bytes(call.keep), whole_keep), name
        again_whole = call(call.full, reuse=True)
        again = call(least, reuse=True)
        same(again, again_whole, name + ", reuse")
        same(again, whole, name + ", reuse against the rebuild")
        assert np.array_equal(keep_bytes(call.keep), whole_keep), name + ", reuse"
    if "expression" in name:
        # (a library built for one generated model has the direct form alone: the two bits change nothing)
        same(call(least, flags=0), whole, name + ", without the bits")
        assert call(least - 8, refused=True, flags=0) == error


def test_the_speculative_sweep_needs_sixteen_bytes_more(recorded):
    assert recorded["bins, speculative"]["ws_bytes"] == recorded["bins"]["ws_bytes"] + 16
    assert "OBE_WS_ABORT_WORD" in recorded["bins, speculative"]["error"]
    assert recorded["bins"]["ws_bytes"] == recorded["bins, keep buffer"]["ws_bytes"] == recorded["bins and cells"]["ws_bytes"]
    assert recorded["direct"]["ws_bytes"] < recorded["cells"]["ws_bytes"] and recorded["direct"]["ws_bytes"] < recorded["bins"]["ws_bytes"]
    assert recorded["direct"]["ws_bytes"] == recorded["direct, shifted"]["ws_bytes"] < recorded["three peaks"]["ws_bytes"]
