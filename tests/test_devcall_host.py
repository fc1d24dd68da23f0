"""The library calls of the feature modules, traced on the host: which entry points a public method calls, in which
order, with which scalars, tile boundaries, workspace sizes and null-versus-given pointers.

A fake experiment (CPU tensors, a recording library) stands in for the device; nothing is computed, so only the traces
are asserted, never the results.  The expected traces are written out from the tiling rules: 20 columns at 7 per call
are calls of 7, 7 and 6; 17 levels at 16 per call are 16 + 1; 9 rows at 8 per call are 8 + 1; 5 pivots of a 2-channel
model at 8 rows per call are 4 + 1.  The fake's workspace query returns 8 bytes times the sum of its arguments.
"""
import ctypes
import types
import warnings

import numpy as np
import pytest
import torch

from optbayesexpt_amd import _batch, _design, _interest, _posterior, _predictive, _reading, _scoring
from optbayesexpt_amd.obe_poisson import OptBayesExptPoisson

N_P, N_C, N_D, N_X = 130, 2, 9, 20
TILES = (7, 7, 6)                        # N_X columns at 7 per call
MODEL, STREAM = object(), ctypes.c_void_p(5)
CPU = torch.device("cpu")


def _seen(a):
    """What the trace keeps of one argument: 'm' the model, 's' the stream, 'p' a pointer, None a null pointer, ints
    and floats as they are."""
    if a is None:
        return None
    if a is MODEL:
        return "m"
    if a is STREAM:
        return "s"
    if isinstance(a, ctypes.c_void_p):
        return "p" if a.value else None
    if isinstance(a, (bool, np.bool_)):
        raise TypeError(f"a bool in a library call: {a!r}")
    if isinstance(a, (int, np.integer)):
        return int(a)
    if isinstance(a, float):
        return a
    raise TypeError(f"unexpected argument in a library call: {a!r}")


class Recorder:
    """``cdll.<query>_workspace_bytes(*sizes)`` and ``call(entry, *args)`` go to ``trace``; ``on_call[entry](args)``
    may write what a caller reads back and cannot take as garbage."""

    def __init__(self):
        self.trace, self.on_call, self.cdll = [], {}, self

    def __getattr__(self, name):
        if not name.endswith("_workspace_bytes"):
            raise AttributeError(name)

        def query(*sizes):
            self.trace.append((name, tuple(int(s) for s in sizes)))
            return 8 * sum(sizes)
        return query

    def call(self, entry, *args):
        self.trace.append((entry, tuple(_seen(a) for a in args)))
        if entry in self.on_call:
            self.on_call[entry](args)
        return 0


def _holder(t):
    return types.SimpleNamespace(tensor=lambda: t)


@pytest.fixture
def obe():
    """The experiment: a 2-channel model of one setting, 20 grid points, a cloud of 9 rows x 130."""
    lib = Recorder()
    return types.SimpleNamespace(
        _device_model=object(), _model_struct=MODEL, _mlib=lib, _lib=lib, _device=CPU, _stream=lambda: STREAM,
        n_channels=N_C, n_dims=N_D, allsettings=np.linspace(0.0, 1.0, N_X).reshape(1, N_X),
        _settings_dev=torch.linspace(0.0, 1.0, N_X, dtype=torch.float64).reshape(1, N_X),
        _parameters=_holder(torch.zeros((N_D, N_P), dtype=torch.float64)),
        _weights=_holder(torch.full((N_P,), 1.0 / N_P, dtype=torch.float64)))


@pytest.fixture
def seven(monkeypatch):
    for module, name in ((_predictive, "SETTINGS_PER_CALL"), (_scoring, "RECORDS_PER_CALL"),
                         (_reading, "SETTINGS_PER_CALL"), (_batch, "RECORDS_PER_CALL")):
        monkeypatch.setattr(module, name, 7)


XS = (np.linspace(0.0, 1.0, N_X),)
YS = np.zeros((N_C, N_X))
NOISE_ROWS = np.array([7, 8])


# ------------------------------------------------------------------------------------------------- _predictive
def test_predict(obe, seven):
    _predictive.predict(obe)
    expected = []
    for n in TILES:
        expected += [("obe_predictive_workspace_bytes", (N_P, n, N_C, 0)),
                     ("obe_predictive_moments", ("m", "p", n, n, "p", N_P, N_P, "p", "p", "p", "p",
                                                 8 * (N_P + n + N_C), "s"))]
    assert obe._mlib.trace == expected
    assert expected[1] == ("obe_predictive_moments", ("m", "p", 7, 7, "p", 130, 130, "p", "p", "p", "p", 1112, "s"))
    del obe._mlib.trace[:]
    _predictive.predict(obe, settings=XS)          # (points of the caller's: the same calls)
    assert obe._mlib.trace == expected


def test_predictive_quantile(obe, seven):
    _predictive.predictive_quantile(obe, np.linspace(0.0, 1.0, 17))
    expected = []
    for n_q in (16, 1):
        for n in TILES:
            expected += [("obe_predictive_workspace_bytes", (N_P, n, N_C, n_q)),
                         ("obe_predictive_quantiles", ("m", "p", n, n, "p", N_P, N_P, "p", "p", n_q, "p", "p",
                                                       8 * (N_P + n + N_C + n_q), "s"))]
    assert obe._mlib.trace == expected


# --------------------------------------------------------------------------------------------------- _scoring
def _score_calls(entry, n_out, sigma, rows):
    expected = []
    for n in TILES:
        expected += [("obe_predictive_score_workspace_bytes", (N_P, n, N_C)),
                     (entry, ("m", "p", n, n, "p", n, sigma, n, rows, "p", N_P, N_P, "p") + ("p",) * n_out
                      + ("p", 8 * (N_P + n + N_C), "s"))]
    return expected


def test_predictive_logpdf(obe, seven):
    _scoring.predictive_logpdf(obe, XS, YS, 0.5)
    assert obe._mlib.trace == _score_calls("obe_predictive_logpdf", 1, "p", None)


def test_predictive_tails(obe, seven):
    _scoring.predictive_tails(obe, XS, YS, 0.5)
    assert obe._mlib.trace == _score_calls("obe_predictive_tails", 2, "p", None)
    del obe._mlib.trace[:]
    obe._noise_rows = NOISE_ROWS
    _scoring.predictive_tails(obe, XS, YS)
    assert obe._mlib.trace == _score_calls("obe_predictive_tails", 2, None, "p")


# --------------------------------------------------------------------------------------------------- _reading
def _reading_calls(groups, sigma, rows):
    expected = []
    for n_q in groups:
        for n in TILES:
            expected += [("obe_predictive_reading_workspace_bytes", (N_P, n, N_C, n_q)),
                         ("obe_predictive_reading_quantiles",
                          ("m", "p", n, n, sigma, n, rows, "p", N_P, N_P, "p", "p", "p", n_q, 48, "p", "p", "p",
                           8 * (N_P + n + N_C + n_q), "s"))]
    return expected


def test_reading_quantile(obe, seven):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (garbage pass counts: "still open")
        _reading.reading_quantile(obe, np.linspace(0.05, 0.95, 17), sigma=0.5)
        assert obe._mlib.trace == _reading_calls((16, 1), "p", None)
        del obe._mlib.trace[:]
        obe._noise_rows = NOISE_ROWS
        _reading.reading_quantile(obe, (0.1, 0.5, 0.9), settings=XS)
        assert obe._mlib.trace == _reading_calls((3,), None, "p")


# -------------------------------------------------------------------------------------------------- _interest
def test_output_covariance(obe, seven):
    _interest.output_covariance(obe)                # all 9 rows: 8 + 1 (ROWS_PER_CALL as it is)
    assert _interest.ROWS_PER_CALL == 8
    expected = []
    for n in TILES:
        for n_r, ycov in ((8, "p"), (1, None)):
            expected += [("obe_output_covariance_workspace_bytes", (N_P, n, N_C, n_r)),
                         ("obe_output_covariance", ("m", "p", n, n, "p", N_P, N_D, N_P, "p", "p", n_r, "p", ycov, "p",
                                                    "p", "p", 8 * (N_P + n + N_C + n_r), "s"))]
    assert obe._mlib.trace == expected


# ---------------------------------------------------------------------------------------------------- _design
def test_output_cross_covariance(obe, seven):
    _design.output_cross_covariance(obe, (np.linspace(0.0, 1.0, 5),))
    assert _design.pivots_per_call(N_C) == 4
    expected = []
    for n in TILES:
        for n_j, mean_given in ((4, 0), (1, 1)):
            expected += [("obe_output_cross_covariance_workspace_bytes", (N_P, n, N_C, n_j)),
                         ("obe_output_cross_covariance", ("m", "p", n, n, "p", n_j, n_j, "p", N_P, N_P, "p", "p",
                                                          mean_given, "p", "p", 8 * (N_P + n + N_C + n_j), "s"))]
    assert obe._mlib.trace == expected


# ----------------------------------------------------------------------------------------------------- _batch
def test_gaussian_records_loglik(obe, seven):
    _batch.GaussianRecords(obe, XS, YS, 0.5).loglik()
    expected = []
    for n, accumulate in zip(TILES, (0, 1, 1)):
        expected += [("obe_records_loglik_workspace_bytes", (N_P, n, N_C)),
                     ("obe_records_loglik", ("m", "p", n, n, "p", n, "p", n, None, "p", N_P, N_P, accumulate, "p", "p",
                                             8 * (N_P + n + N_C), "s"))]
    assert obe._mlib.trace == expected


def test_own_records_loglik(obe, seven):
    def constants(begin, end):
        return 100.0 * begin + end
    rows = np.zeros((1 + 2 * N_C, N_X))
    _batch.OwnRecords(obe, "obe_binomial_records_loglik", rows, 1, True, constants).loglik()
    expected = []
    for n, accumulate, constant in zip(TILES, (0, 1, 1), (7.0, 714.0, 1420.0)):
        expected += [("obe_binomial_records_loglik_workspace_bytes", (N_P, n, N_C)),
                     ("obe_binomial_records_loglik", ("m", "p", n, n, "p", n, "p", n, constant, "p", N_P, N_P,
                                                      accumulate, "p", "p", 8 * (N_P + n + N_C), "s"))]
    assert obe._mlib.trace == expected
    del obe._mlib.trace[:]
    _batch.OwnRecords(obe, "obe_signal_noise_records_loglik", rows[:1 + N_C], 1, False, constants,
                      (np.ones((N_C, 3)),)).loglik()
    expected = []
    for n, accumulate, constant in zip(TILES, (0, 1, 1), (7.0, 714.0, 1420.0)):
        expected += [("obe_signal_noise_records_loglik_workspace_bytes", (N_P, n, N_C)),
                     ("obe_signal_noise_records_loglik", ("m", "p", n, n, "p", n, "p", constant, "p", N_P, N_P,
                                                          accumulate, "p", "p", 8 * (N_P + n + N_C), "s"))]
    assert obe._mlib.trace == expected


# ------------------------------------------------------------------------------------------------- _posterior
@pytest.fixture
def pdf():
    """A cloud of 3 rows x 130 whose ``obe_minmax_rows`` answers (0, 1) for every row: the ranges are read back."""
    lib = Recorder()

    def minmax(args):
        n = 2 * args[5]
        (ctypes.c_double * n).from_address(args[6].value)[:] = [0.0, 1.0] * args[5]
    lib.on_call["obe_minmax_rows"] = minmax
    cloud = (torch.zeros((3, N_P), dtype=torch.float64), torch.full((N_P,), 1.0 / N_P, dtype=torch.float64))
    return types.SimpleNamespace(_lib=lib, _device=CPU, _stream=lambda: STREAM, n_dims=3, n_particles=N_P,
                                 _pw_tensors=lambda: cloud)


def test_posterior_calls(pdf):
    trace = pdf._lib.trace
    _posterior.marginal_histogram(pdf, bins=4)
    assert trace == [
        ("obe_posterior_workspace_bytes", (130, 3, 0, 0)),
        ("obe_minmax_rows", ("p", 130, 3, 130, "p", 3, "p", "p", 8 * 133, "s")),
        ("obe_posterior_workspace_bytes", (130, 3, 4, 0)),
        ("obe_weighted_histogram", ("p", 130, 3, 130, "p", "p", 3, "p", 4, "p", "p", 8 * 137, "s"))]
    del trace[:]
    _posterior.marginal_histogram(pdf, dims=1, bins=4, range=(0.0, 2.0))          # (a range given: no minmax pass)
    assert trace == [
        ("obe_posterior_workspace_bytes", (130, 1, 4, 0)),
        ("obe_weighted_histogram", ("p", 130, 3, 130, "p", "p", 1, "p", 4, "p", "p", 8 * 135, "s"))]
    del trace[:]
    _posterior.joint_histogram(pdf, 0, 2, bins=(3, 5))
    assert trace == [
        ("obe_posterior_workspace_bytes", (130, 2, 0, 0)),
        ("obe_minmax_rows", ("p", 130, 3, 130, "p", 2, "p", "p", 8 * 132, "s")),
        ("obe_posterior_workspace_bytes", (130, 1, 15, 0)),
        ("obe_weighted_histogram2d", ("p", 130, 3, 130, "p", 0, 2, "p", 3, "p", 5, "p", "p", 8 * 146, "s"))]
    del trace[:]
    _posterior.quantile(pdf, np.linspace(0.0, 1.0, 17), dims=[2, 0])
    expected = []
    for n_q in (16, 1):
        expected += [("obe_posterior_workspace_bytes", (130, 2, 0, n_q)),
                     ("obe_weighted_quantiles", ("p", 130, 3, 130, "p", "p", 2, "p", n_q, "p", "p", 8 * (132 + n_q),
                                                 "s"))]
    assert trace == expected


# ------------------------------------------------------------------------------------- a pass of an own-noise class
def test_poisson_pass_call():
    """``OptBayesExptPoisson._call``: the pass workspace of the own-noise classes, on an object without a device."""
    lib = Recorder()
    o = object.__new__(OptBayesExptPoisson)
    o.__dict__.update(count_cap=32, n_channels=1, _mlib=lib, _model_struct=MODEL, _device=CPU, _stream=lambda: STREAM,
                      _particles=_holder(torch.zeros((3, N_P), dtype=torch.float64)),
                      _weights=_holder(torch.full((N_P,), 1.0 / N_P, dtype=torch.float64)))
    pmf = torch.empty((33, 6), dtype=torch.float64)
    x = ctypes.c_void_p(pmf.data_ptr())          # (any address: nothing reads it)
    o._call(x, 20, 6, 2.0, None, 1.0, None, None, pmf, None)
    assert lib.trace == [
        ("obe_poisson_workspace_bytes", (130, 6, 1, 32)),
        ("obe_poisson_information", ("m", "p", 20, 6, "p", 130, 130, "p", 2.0, 32, None, 1.0, None, None, "p", None,
                                     "p", 8 * 169, "s"))]
