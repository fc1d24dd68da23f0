"""Assimilating a recorded data set on the device (OptBayesExpt.records_loglik / pdf_update_batch; csrc/obe_predict.hip
K13a, csrc/obe_batch.hip K13b) against tests/_batch_oracle.py on the rows y = eval_over_all_parameters((x_r,)) of the
product itself, against the oracle classes' sequential updates and against the product's own record-by-record route.

Tolerances: |d l_i| <= 1e-10 max(1, B_i), B_i the sum of the absolute values of l_i's terms (each term is good to a few
eps of itself, the sums add R C eps B at worst); weights by tests/_replay.py: close_weights at 1e-10 (the exponent is
what an implementation is good to) on inputs whose every oracle weight exceeds 1e-280, asserted from the oracle first;
log evidence |d| <= 1e-10 max(1, |log Z|, sum_r |log sum t_r|).  Run to run: the same bits.  The worst error /
tolerance ratios seen are printed by test_worst_errors_are_reported."""
import copy
import importlib.util
import json
import math
import os
import pickle
import subprocess
import sys
import warnings

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _batch_models
import _batch_oracle as bo
import _expr_models
import oracle
from _replay import close_weights
from optbayesexpt_amd import _batch, _lib
from oracle import models as omodels

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _note(kind, ratio, what):
    if ratio >= WORST.get(kind, (0.0, ""))[0]:
        WORST[kind] = float(ratio), what


# ------------------------------------------------------------------------------------------------ the objects
def _model(name):
    import optbayesexpt_amd as obe
    m = obe.models
    if name == "lorentz1":
        return m.lorentzian(1), (0.1,)
    if name == "lorentz7":
        return m.lorentzian(7), (0.1,)
    if name == "coil":
        return m.coil(), ()
    if name == "rabi":
        return m.rabi(), (1.0e5, 0.3, 2.0)
    if name == "expression":
        return _expr_models.expression_models()["lorentzian"], (0.1,)
    if name == "function":
        return _expr_models.expression_models()["fn_lorentzian"], (0.1,)
    if name == "line":
        return _batch_models.expression_models()["line"], ()
    raise KeyError(name)


def _prior(name, g, n):
    if name in ("lorentz1", "function", "expression"):
        return np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    if name == "lorentz7":
        return np.vstack([g.uniform(2, 4, (7, n)), g.uniform(400, 2000, (1, n)), g.normal(500, 1000, (1, n)),
                          g.exponential(500, (1, n))])
    if name == "coil":
        return np.array([g.normal(1e-3, 1e-4, n), g.normal(10.0, 1.0, n), g.normal(1e-6, 1e-7, n)])
    if name == "rabi":
        return np.array([g.uniform(0.5, 2.0, n), g.uniform(-3.0, 3.0, n)])
    raise KeyError(name)


def _points(name, g, n_r):
    if name == "coil":
        return g.uniform(1.0e4, 6.0e4, n_r)[None, :]
    if name == "rabi":
        return np.array([g.uniform(0.0, 3.0, n_r), g.uniform(-4.0, 4.0, n_r)])
    return g.uniform(1.5, 4.5, n_r)[None, :]


def _design(name):
    if name == "rabi":
        return (np.linspace(0.0, 3.0, 5), np.linspace(-4.0, 4.0, 7))
    if name == "coil":
        return (np.linspace(1.0e4, 6.0e4, 33),)
    if name == "line":
        return (np.linspace(-1.0, 3.0, 33),)
    return (np.linspace(1.5, 4.5, 33),)


def _object(name, cloud, noise_rows=None, **kw):
    import optbayesexpt_amd as obe
    model, cons = _model(name)
    kw.setdefault("scale", False)
    if noise_rows is None:
        return obe.OptBayesExpt(model, _design(name), cloud, cons, **kw)
    return obe.OptBayesExptNoiseParameter(model, _design(name), cloud, cons, noise_parameter_index=noise_rows, **kw)


def _rows(o, x, columns=None):
    """y (n_r, C, N_p) — or the given columns of it —: the product's own model values, one record's setting at a time."""
    out = []
    for r in range(x.shape[1]):
        y = np.asarray(o.eval_over_all_parameters(tuple(float(v) for v in x[:, r]))).reshape(o.n_channels, -1)
        out.append(y if columns is None else y[:, columns])
    return np.stack(out)


def _readings(g, y, sig_rows=None):
    """Readings (C, n_r) within a few sigma of one particle's model values and, unless the object has noise rows, a
    known sigma (C, n_r) of the size of the cloud's own spread that differs per record and channel."""
    n_r, n_c, n = y.shape
    pick = n // 2
    if sig_rows is None:
        spread = np.array([[np.std(y[r, c]) for r in range(n_r)] for c in range(n_c)])
        sigma = (spread + 1e-3 * np.abs(y[:, :, pick].T) + 1e-12) * g.uniform(0.5, 2.0, (n_c, n_r))
        at = sigma
    else:
        sigma, at = None, np.abs(sig_rows[:, pick])[:, None] + 1e-12
    return y[:, :, pick].T + at * g.normal(0.0, 1.0, (n_c, n_r)), sigma


def _check_loglik(what, o, x, ym, sigma, sig_rows=None, columns=None):
    """records_loglik against the oracle on the product's own rows: NaN where the oracle has it, else within
    1e-10 max(1, B_i); the same bits from run to run.  ``columns``: the particles compared (all)."""
    got = o.records_loglik(x, ym, sigma)
    assert got.shape == (o.n_particles,) and got.dtype == np.float64
    assert_array_equal(_bits(o.records_loglik(x, ym, sigma)), _bits(got), err_msg=f"{what}: run to run")
    y = _rows(o, x, columns)
    if sig_rows is None:
        want, cond = bo.loglik(y, ym, sigma)
    else:
        want, cond = bo.loglik(y, ym, sig_rows if columns is None else sig_rows[:, columns], per_particle=True)
    mine = got if columns is None else got[columns]
    dead = np.isnan(want.astype(np.float64))
    assert_array_equal(np.isnan(mine), dead, err_msg=f"{what}: where NaN falls")
    err = np.abs((mine[~dead].astype(bo.LD) - want[~dead]).astype(np.float64))
    tol = bo.loglik_tolerance(cond[~dead])
    if err.size:
        _note("l", np.max(err / tol), what)
    assert np.all(err <= tol), f"{what}: worst error / tolerance {np.max(err / tol):.3g}"
    return got


# ------------------------------------------------------------------------- 1. l: shapes, records x particles
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_loglik_shapes_lorentzian(hip, n):
    """Both sides of the wave of 64 particles, one particle, several tiles; one record, both sides of a chunk of
    records, several chunks.  A permuted cloud gives the permuted bits."""
    for n_r in (1, 2, 63, 64, 65, 300):
        g = np.random.default_rng([n, n_r])
        cloud, x = _prior("lorentz1", g, n), _points("lorentz1", g, n_r)
        o = _object("lorentz1", cloud)
        ym, sigma = _readings(g, _rows(o, x))
        got = _check_loglik(f"lorentz1 {n} x {n_r}", o, x, ym, sigma)
        if n_r in (2, 300):
            perm = g.permutation(n)
            assert_array_equal(_bits(_object("lorentz1", cloud[:, perm]).records_loglik(x, ym, sigma)), _bits(got[perm]))


def test_loglik_one_tile_many_chunks(hip):
    g = np.random.default_rng(64)
    cloud, x = _prior("lorentz1", g, 64), _points("lorentz1", g, 5000)
    o = _object("lorentz1", cloud)
    ym, sigma = _readings(g, _rows(o, x[:, :50]))
    ym, sigma = np.resize(ym, (1, 5000)), np.resize(sigma, (1, 5000)) * 8.0
    _check_loglik("lorentz1 64 x 5000", o, x, ym, sigma)


def test_loglik_large_cloud(hip):
    """2^17 + 3 particles x 1000 records: more particle tiles than the 8192 waves a launch aims at (one chunk of
    records).  Compared on both ends of the cloud, both sides of every 2^15-th particle and a random sample."""
    n, n_r = (1 << 17) + 3, 1000
    g = np.random.default_rng(17)
    cloud, x = _prior("lorentz1", g, n), _points("lorentz1", g, n_r)
    o = _object("lorentz1", cloud)
    columns = np.unique(np.concatenate([np.arange(70), np.arange(n - 70, n), g.integers(0, n, 200)]
                                       + [np.arange(k - 2, k + 2) for k in range(1 << 15, n, 1 << 15)]))
    ym, sigma = _readings(g, _rows(o, x[:, :40], columns))
    ym, sigma = np.resize(ym, (1, n_r)), np.resize(sigma, (1, n_r)) * 4.0
    _check_loglik("lorentz1 2^17+3 x 1000", o, x, ym, sigma, columns=columns)


def test_records_tile_boundary_is_an_accumulate_chain(hip, monkeypatch):
    """RECORDS_PER_CALL records per library call: with 7, twenty records are three calls, the later ones added in
    tile order — bit for bit the accumulate chain of the entry point, and within tolerance of the oracle."""
    import torch
    g = np.random.default_rng(7)
    n, n_r = 333, 20
    cloud, x = _prior("lorentz1", g, n), _points("lorentz1", g, n_r)
    o = _object("lorentz1", cloud)
    ym, sigma = _readings(g, _rows(o, x))
    whole = o.records_loglik(x, ym, sigma)
    monkeypatch.setattr(_batch, "RECORDS_PER_CALL", 7)
    tiled = _check_loglik("tiles of 7", o, x, ym, sigma)
    dev = o._device
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    p = o._parameters.tensor()
    for start in range(0, n_r, 7):
        part = [torch.from_numpy(np.ascontiguousarray(a[:, start:start + 7])).to(dev) for a in (x, ym, sigma)]
        k = part[0].shape[1]
        nbytes = int(hip.cdll.obe_records_loglik_workspace_bytes(n, k, 1))
        ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
        o._mlib.call("obe_records_loglik", o._model_struct, part[0].data_ptr(), k, k, part[1].data_ptr(), k,
                     part[2].data_ptr(), k, None, p.data_ptr(), n, n, 1 if start else 0, out.data_ptr(), ws.data_ptr(),
                     nbytes, o._stream())
    assert_array_equal(_bits(out.cpu().numpy()), _bits(tiled))
    assert np.max(np.abs(tiled - whole)) <= 1e-10 * np.max(np.abs(whole))


# ------------------------------------------------------------------------- 2. l: models and objects
@pytest.mark.parametrize("name", ["lorentz7", "coil", "rabi", "expression", "function"])
def test_loglik_models(hip, name):
    for n, n_r in ((130, 5), (1000, 70)):
        g = np.random.default_rng([n, n_r, len(name)])
        cloud, x = _prior(name, g, n), _points(name, g, n_r)
        o = _object(name, cloud)
        ym, sigma = _readings(g, _rows(o, x))
        _check_loglik(f"{name} {n} x {n_r}", o, x, ym, sigma)


def _noise_cloud(name, g, n, x, rows):
    cloud = _prior(name, g, n)
    y = _rows(_object(name, cloud), x[:, :3])
    extra = np.ones((max(rows) + 1 - cloud.shape[0], n))
    for c, row in enumerate(rows):
        scale = np.median([np.std(y[r, c]) + 1e-3 * abs(y[r, c, 0]) + 1e-12 for r in range(y.shape[0])])
        extra[row - cloud.shape[0]] = scale * g.uniform(0.5, 2.0, n)
    return np.vstack([cloud, extra])


@pytest.mark.parametrize("name,rows", [("lorentz1", (3,)), ("coil", (4, 3))])
def test_loglik_noise_parameter_objects(hip, name, rows):
    """sigma from one and from two parameter rows; a noise row that is 0, negative or NaN marks its particle NaN."""
    g = np.random.default_rng(len(rows))
    n, n_r = 700, 65
    x = _points(name, g, n_r)
    cloud = _noise_cloud(name, g, n, x, rows)
    cloud[rows[0], [5, 64, 699]] = 0.0, -3.0, np.nan
    cloud[rows[-1], 320] = -1e-300
    o = _object(name, cloud, noise_rows=rows)
    ym, _ = _readings(g, _rows(o, x), cloud[list(rows)])
    got = _check_loglik(f"{name}, noise rows {rows}", o, x, ym, None, sig_rows=cloud[list(rows)])
    assert np.isnan(got[[5, 64, 699, 320]]).all() and np.isnan(got).sum() == 4
    with pytest.raises(ValueError, match="call without sigma"):
        o.records_loglik(x, ym, 1.0)
    with pytest.raises(ValueError, match="call without sigma"):
        o.pdf_update_batch(x, ym, 1.0)


def test_loglik_nan_falls_where_the_oracle_puts_it(hip):
    """A model output that is NaN (a NaN parameter) or +-inf (the pole of a / (x - x0) hit exactly) marks the particle;
    a record sigma <= 0 — which the method refuses — marks every particle through the C ABI."""
    import torch
    g = np.random.default_rng(9)
    n, n_r = 200, 6
    x = np.array([[0.5, 1.0, 1.5, 2.0, 2.5, 3.0]])
    cloud = np.array([g.uniform(3.5, 6.0, n), g.uniform(1.0, 2.0, n)])
    cloud[0, 17], cloud[0, 130] = 2.0, 0.5                     # x == x0: a / 0 = inf
    cloud[1, 64] = np.nan
    cloud[1, 130] = -1.5                                       # ... -inf
    o = _object_pole(cloud)
    ym, sigma = np.full((1, n_r), 0.7), np.full((1, n_r), 0.9)
    got = _check_loglik("pole", o, x, ym, sigma)
    assert np.isnan(got[[17, 64, 130]]).all() and np.isnan(got).sum() == 3
    with pytest.raises(ValueError, match="sigma must be finite and > 0"):
        o.records_loglik(x, ym, np.array([[0.9, 0.9, 0.0, 0.9, 0.9, 0.9]]))
    dev = o._device
    for bad in (0.0, -0.9, float("nan")):
        s = sigma.copy()
        s[0, 4] = bad
        d = [torch.from_numpy(a).to(dev) for a in (x, ym, s)]
        out = torch.zeros(n, dtype=torch.float64, device=dev)
        nbytes = int(o._mlib.cdll.obe_records_loglik_workspace_bytes(n, n_r, 1))
        ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
        o._mlib.call("obe_records_loglik", o._model_struct, d[0].data_ptr(), n_r, n_r, d[1].data_ptr(), n_r,
                     d[2].data_ptr(), n_r, None, o._parameters.tensor().data_ptr(), n, n, 0, out.data_ptr(),
                     ws.data_ptr(), nbytes, o._stream())
        assert np.isnan(out.cpu().numpy()).all(), bad


def _object_pole(cloud):
    import optbayesexpt_amd as obe
    return obe.OptBayesExpt(_expr_models.expression_models()["pole"], (np.linspace(0.0, 3.0, 7),), cloud, (), scale=False)


def test_host_models_are_refused(hip):
    import optbayesexpt_amd as obe
    g = np.random.default_rng(1)
    o = obe.OptBayesExpt(omodels.lorentzian, _design("lorentz1"), _prior("lorentz1", g, 50), (0.1,))
    for call in (o.records_loglik, o.pdf_update_batch):
        with pytest.raises(TypeError, match="from_function.*from_expression"):
            call((np.array([2.0, 3.0]),), np.array([1.0, 2.0]), 1.0)


# ------------------------------------------------------------------------- 3. one stage
def _one_stage_case(n=2000, n_r=40, seed=40):
    g = np.random.default_rng(seed)
    cloud, x = _prior("lorentz1", g, n), _points("lorentz1", g, n_r)
    truth = np.array([3.1, -1200.0, 50200.0])
    y = np.array([float(omodels.lorentzian((xi,), truth, (0.1,))) for xi in x[0]])
    sigma = g.uniform(1500.0, 4000.0, (1, n_r))
    return cloud, x, (y + sigma[0] * g.standard_normal(n_r))[None, :], sigma


def _oracle_sequential(cloud, x, ym, sigma, weights=None, **kw):
    """R sequential pdf_update() calls of the oracle class, auto_resample=False: the object, log sum t_r per record."""
    seq = oracle.OracleOptBayesExpt(omodels.lorentzian, _design("lorentz1"), cloud.copy(), (0.1,), auto_resample=False, **kw)
    if weights is not None:
        seq.particle_weights = weights.copy()
    logs = []
    for r in range(x.shape[1]):
        rec = ((x[0, r],), ym[0, r], sigma[0, r])
        lik = seq.likelihood(seq.eval_over_all_parameters(rec[0]), rec)
        with np.errstate(invalid="ignore"):
            logs.append(math.log(np.sum(np.nan_to_num(seq.particle_weights * lik))))
        seq.pdf_update(rec)
    return seq, np.array(logs)


@pytest.mark.parametrize("threshold", [0.999, 0.0])
def test_one_stage_is_the_sequential_updates(hip, threshold):
    """tempered=False against the oracle's and the product's own R sequential pdf_update() calls with
    auto_resample=False: the weights, the resample decision of one resample_test(), the log evidence."""
    cloud, x, ym, sigma = _one_stage_case()
    n_r = x.shape[1]
    seq, logs = _oracle_sequential(cloud, x, ym, sigma)
    assert np.min(seq.particle_weights) > 1e-280               # (the choice of inputs: CPU only)
    seq.tuning_parameters["resample_threshold"] = threshold
    decision = oracle.effective_particles(seq.particle_weights) / seq.n_particles < max(threshold, 0.1)
    assert decision == (threshold > 0.5)
    # the product, record by record: the weights and the chain of one-step evidences
    loop = _object("lorentz1", cloud, auto_resample=False)
    chain = 0.0
    for r in range(n_r):
        rec = ((x[0, r],), ym[0, r], sigma[0, r])
        chain += loop.predictive_logpdf(*rec)
        loop.pdf_update(rec)
    # the batch, without a resample: the weights
    plain = _object("lorentz1", cloud, auto_resample=False)
    plain.pdf_update_batch(x, ym, sigma, tempered=False)
    close_weights(plain.particle_weights, seq.particle_weights, 1e-10, "one stage vs the oracle's sequential run")
    close_weights(plain.particle_weights, loop.particle_weights, 1e-10, "one stage vs the product's sequential run")
    rep = plain.last_batch_update
    assert rep["stages"] == [1.0] and rep["resamples"] == 0 and len(rep["n_eff"]) == 1
    assert abs(rep["n_eff"][0] - oracle.effective_particles(seq.particle_weights)) <= 1e-8 * rep["n_eff"][0]
    want = float(np.sum(logs)) - n_r * 0.5 * math.log(2 * math.pi)
    tol = 1e-10 * max(1.0, abs(want), float(np.sum(np.abs(logs))))
    l, _ = bo.loglik(_rows(plain, x), ym, sigma)               # (the cloud did not move)
    for kind, ref in (("oracle chain", want), ("oracle stage", bo.stage_log_evidence(l, np.full(len(l), 1.0 / len(l)), 1.0)),
                      ("product chain", chain)):
        _note("log evidence", abs(rep["log_evidence"] - ref) / tol, kind)
        assert abs(rep["log_evidence"] - ref) <= tol, (kind, rep["log_evidence"], ref)
    # ... and with the resample test: the same decision
    o = _object("lorentz1", cloud, resample_threshold=threshold)
    o.rng = np.random.default_rng(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        o.pdf_update_batch(x, ym, sigma, tempered=False)
    assert bool(o.just_resampled) == decision and o.last_batch_update["resamples"] == int(decision)
    if not decision:
        assert_array_equal(_bits(o.particle_weights), _bits(plain.particle_weights))


def test_one_stage_prior_weights_and_choke(hip):
    """Zero and NaN prior weights stay zero (nan_to_num of the product, particlepdf.py:136-139); a negative one is
    carried as the record-by-record updates carry it.  choke = 0.5 against the oracle; no log evidence then."""
    cloud, x, ym, sigma = _one_stage_case(n=500, n_r=12, seed=12)
    g = np.random.default_rng(2)
    w = g.random(500)
    w[[3, 77, 400]] = 0.0
    w /= w.sum()
    seq, _ = _oracle_sequential(cloud, x, ym, sigma, weights=w)
    o = _object("lorentz1", cloud, auto_resample=False)
    o.particle_weights = w.copy()
    o.pdf_update_batch(x, ym, sigma, tempered=False)
    close_weights(o.particle_weights, seq.particle_weights, 1e-10, "given prior weights")
    assert np.all(o.particle_weights[[3, 77, 400]] == 0.0)
    w2 = w.copy()
    w2[10], w2[11] = np.nan, -1e-3
    o = _object("lorentz1", cloud, auto_resample=False)
    o.particle_weights = w2.copy()
    loop = _object("lorentz1", cloud, auto_resample=False)
    loop.particle_weights = w2.copy()
    for r in range(x.shape[1]):
        loop.pdf_update(((x[0, r],), ym[0, r], sigma[0, r]))
    o.pdf_update_batch(x, ym, sigma, tempered=False)
    assert np.all(o.particle_weights[[3, 10, 77, 400]] == 0.0) and o.particle_weights[11] < 0.0
    close_weights(o.particle_weights, loop.particle_weights, 1e-10, "NaN and negative prior weights")
    # choke
    seq, _ = _oracle_sequential(cloud, x, ym, sigma, choke=0.5)
    o = _object("lorentz1", cloud, auto_resample=False, choke=0.5)
    o.pdf_update_batch(x, ym, sigma, tempered=False)
    close_weights(o.particle_weights, seq.particle_weights, 1e-10, "choke 0.5")
    assert o.last_batch_update["log_evidence"] is None


# ------------------------------------------------------------------------- 4. the tempered run
def _tempered_case(n=5000, n_r=200, seed=5, noise=300.0):
    g = np.random.default_rng(seed)
    cloud = _prior("lorentz1", g, n)
    x = np.linspace(1.5, 4.5, n_r)[None, :]
    truth = np.array([3.1, -1200.0, 50200.0])
    y = np.array([float(omodels.lorentzian((xi,), truth, (0.1,))) for xi in x[0]])
    return cloud, x, (y + noise * g.standard_normal(n_r))[None, :], np.full((1, n_r), noise)


def test_tempered_run_stage_by_stage(hip):
    cloud, x, ym, sigma = _tempered_case()
    n = cloud.shape[1]
    o = _object("lorentz1", cloud)
    o.rng = np.random.default_rng(55)
    thr = o.tuning_parameters["resample_threshold"]
    l0, _ = bo.loglik(_rows(o, x), ym, sigma)
    assert bo.ess_fraction(l0, np.full(n, 1.0 / n), 1.0) * n < 2.0          # one stage would collapse the cloud
    snaps, after = [], []

    def on_stage(info):
        snaps.append(dict(info, cloud=o.particles.copy(), weights=o.particle_weights.copy(),
                          rng=copy.deepcopy(o.rng.bit_generator.state), flag=bool(o.just_resampled),
                          idx=None if not snaps else o.last_resample_indices_device.cpu().numpy()))

    inner = o._resample_reported

    def resample_reported():
        inner()
        after.append((o.particle_weights.copy(), bool(o.just_resampled)))
    o._resample_reported = resample_reported
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        o.pdf_update_batch(x, ym, sigma, on_stage=on_stage)
    rep = o.last_batch_update
    n_stages = len(rep["stages"])
    assert n_stages == len(snaps) >= 3 and len(after) >= n_stages - 1
    betas = [s["beta"] for s in snaps]
    assert np.all(np.diff([0.0] + betas) > 0.0) and betas[-1] == 1.0
    assert [s["delta"] for s in snaps] == rep["stages"] and [s["n_eff"] for s in snaps] == rep["n_eff"]
    log_z, beta, w_prev = 0.0, 0.0, np.full(n, 1.0 / n)
    for k, s in enumerate(snaps):
        final = k == n_stages - 1
        helper = _object("lorentz1", s["cloud"])
        l, _ = bo.loglik(_rows(helper, x), ym, sigma)
        delta, delta_max = s["delta"], 1.0 - beta
        if not final:
            assert bo.ess_fraction(l, w_prev, delta) >= thr * (1 - 1e-9), k
            assert bo.ess_fraction(l, w_prev, delta + delta_max * 2.0 ** -29) < thr * (1 + 1e-9), k
        else:
            assert delta == delta_max
        close_weights(s["weights"], bo.stage_weights(l, w_prev, delta), 1e-10, f"weights of stage {k}")
        log_z += bo.stage_log_evidence(l, w_prev, delta)
        n_eff = 1.0 / np.sum(bo.stage_weights(l, w_prev, delta).astype(bo.LD) ** 2)
        assert abs(s["n_eff"] - float(n_eff)) <= 1e-8 * float(n_eff)
        if final:
            break
        # the resample behind the stage: replayed by the oracle class from the snapshot
        weights_after, flag = after[k]
        assert flag and snaps[k + 1]["flag"]
        assert_array_equal(_bits(weights_after), _bits(np.full(n, 1.0 / n)))
        rp = oracle.OracleParticlePDF(s["cloud"].copy(), scale=False)
        rp.particle_weights = s["weights"].copy()
        rp.rng = np.random.default_rng()
        rp.rng.bit_generator.state = copy.deepcopy(s["rng"])
        cov = rp.covariance()
        rp.resample()
        assert_array_equal(snaps[k + 1]["idx"], rp.last_draw_indices, err_msg=f"resample indices, stage {k}")
        assert rp.rng.bit_generator.state == snaps[k + 1]["rng"], f"generator state after the resample of stage {k}"
        floor = 256 * 2.3e-16 * np.sqrt(np.max(np.diag(cov)))
        for d in range(cloud.shape[0]):
            assert_allclose(snaps[k + 1]["cloud"][d], rp.particles[d], rtol=1e-10, atol=floor,
                            err_msg=f"particles[{d}] after the resample of stage {k}")
        beta += delta
        w_prev = np.full(n, 1.0 / n)
    tol = 1e-8 * max(1.0, abs(log_z))          # (stage by stage on clouds that agree to 1e-10: the sum of n_stages terms)
    assert abs(rep["log_evidence"] - log_z) <= tol, (rep["log_evidence"], log_z)
    _note("tempered log evidence", abs(rep["log_evidence"] - log_z) / tol, f"{n_stages} stages")
    assert rep["resamples"] >= n_stages - 1


def test_max_stages_applies_the_remainder_and_warns(hip):
    cloud, x, ym, sigma = _tempered_case(n=1000, n_r=50, seed=6)
    o = _object("lorentz1", cloud)
    o.rng = np.random.default_rng(1)
    with pytest.warns(RuntimeWarning, match="max_stages"):
        o.pdf_update_batch(x, ym, sigma, max_stages=1)
    assert o.last_batch_update["stages"] == [1.0]
    plain = _object("lorentz1", cloud, auto_resample=False)
    plain.pdf_update_batch(x, ym, sigma, tempered=False)
    assert abs(o.last_batch_update["log_evidence"] - plain.last_batch_update["log_evidence"]) == 0.0
    o = _object("lorentz1", cloud)
    o.rng = np.random.default_rng(1)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        o.pdf_update_batch(x, ym, sigma, max_stages=2)
    assert len(o.last_batch_update["stages"]) == 2 and sum("max_stages" in str(w.message) for w in seen) == 1


# ------------------------------------------------------------------------- 5. the conjugate case
def test_tempered_posterior_on_the_conjugate_case(hip):
    """a + b x with a Gaussian prior: the tempered posterior mean within 0.2 exact posterior sd of the closed form,
    each std within 20 % (the NumPy oracle of the same algorithm stays within half of that:
    tests/test_batch_update_host.py)."""
    prior, x, y, sigma, mean, cov = bo.conjugate_case()
    sd = np.sqrt(np.diag(cov))
    o = _object("line", prior, scale=True)
    o.rng = np.random.default_rng(77)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        o.pdf_update_batch((x,), y, sigma)
    assert len(o.last_batch_update["stages"]) >= 3
    assert np.all(np.abs(o.mean() - mean) <= 0.2 * sd), (o.mean(), mean, sd)
    assert np.all(np.abs(o.std() / sd - 1.0) <= 0.2), (o.std(), sd)


# ------------------------------------------------------------------------- 6. through the classes
def test_noise_parameter_object(hip):
    g = np.random.default_rng(21)
    n, n_r = 3000, 60
    x = np.linspace(1.5, 4.5, n_r)[None, :]
    cloud = np.vstack([_prior("lorentz1", g, n), g.uniform(100.0, 1500.0, (1, n))])
    truth = np.array([3.1, -1200.0, 50200.0])
    ym = (np.array([float(omodels.lorentzian((xi,), truth, (0.1,))) for xi in x[0]]) + 500.0 * g.standard_normal(n_r))[None, :]
    # every sigma > 0: the record-by-record route of the product itself
    loop = _object("lorentz1", cloud, noise_rows=(3,), auto_resample=False)
    for r in range(n_r):
        loop.pdf_update(((x[0, r],), ym[0, r]))
    one = _object("lorentz1", cloud, noise_rows=(3,), auto_resample=False)
    one.pdf_update_batch(x, ym, tempered=False)
    live = loop.particle_weights > 1e-280
    assert live.sum() > 100
    close_weights(one.particle_weights[live], loop.particle_weights[live], 1e-10, "noise-parameter object, one stage")
    # some sigma <= 0 (a prior the constraint has not seen yet): such a particle contributes nothing, from the first
    # stage on, and the constraint behind every resample keeps it so
    cloud = cloud.copy()
    cloud[3, ::7] = g.uniform(-100.0, 0.0, cloud[3, ::7].size)
    one = _object("lorentz1", cloud, noise_rows=(3,), auto_resample=False)
    one.pdf_update_batch(x, ym, tempered=False)
    assert np.all(one.particle_weights[cloud[3] <= 0.0] == 0.0) and abs(one.particle_weights.sum() - 1.0) < 1e-12
    o = _object("lorentz1", cloud, noise_rows=(3,))
    o.rng = np.random.default_rng(4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        o.pdf_update_batch(x, ym)
    rep = o.last_batch_update
    assert len(rep["stages"]) >= 2 and math.isfinite(rep["log_evidence"]) and sum(rep["stages"]) == pytest.approx(1.0)
    assert np.all(o.particle_weights[o.particles[3] <= 0.0] == 0.0) and o.last_constraint_count >= 0
    assert abs(o.mean()[0] - 3.1) < 5 * o.std()[0] + 0.01


def test_parameter_bounds_are_enforced_after_a_stage(hip):
    cloud, x, ym, sigma = _tempered_case(n=3000, n_r=100, seed=8)
    o = _object("lorentz1", cloud)
    o.set_parameter_bounds({1: (-1500.0, -900.0)})
    o.rng = np.random.default_rng(9)
    counts = []
    inner = o.enforce_parameter_constraints

    def enforce():
        inner()
        counts.append(o.last_constraint_count)
    o.enforce_parameter_constraints = enforce
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        o.pdf_update_batch(x, ym, sigma)
    assert len(counts) >= o.last_batch_update["resamples"] >= 1 and o.last_constraint_count == counts[-1]
    outside = (o.particles[1] < -1500.0) | (o.particles[1] > -900.0)
    assert np.all(o.particle_weights[outside] == 0.0)


def _cycles(o, n, g):
    out = []
    for _ in range(n):
        xs = o.opt_setting()
        y = float(omodels.lorentzian(xs, (3.1, -1200.0, 50200.0), (0.1,))) + 500.0 * g.standard_normal()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            o.pdf_update((xs, y, 500.0))
        out.append((xs, _bits(o.particle_weights).copy(), _bits(o.particles).copy(), bool(o.just_resampled)))
    return out


def _same(a, b):
    assert len(a) == len(b)
    for (xa, wa, pa, fa), (xb, wb, pb, fb) in zip(a, b):
        assert xa == xb and fa == fb
        assert_array_equal(wa, wb)
        assert_array_equal(pa, pb)


def test_cycles_around_a_batch_update_continue_from_a_snapshot(hip, tmp_path):
    """Five opt_setting() / pdf_update() cycles, a pdf_update_batch(), five more cycles: bit for bit what a deepcopy,
    a pickle and a saved file taken right after the batch continue with — the sweep state was invalidated."""
    import optbayesexpt_amd as obe
    cloud, x, ym, sigma = _tempered_case(n=20000, n_r=30, seed=10)
    o = _object("lorentz1", cloud, utility_method="variance_full", default_noise_std=500.0)
    o.rng = np.random.default_rng(12)
    _cycles(o, 5, np.random.default_rng(1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        o.pdf_update_batch(x, ym, sigma)
    assert o.last_batch_update["stages"]
    twin = copy.deepcopy(o)
    pickled = pickle.loads(pickle.dumps(o))
    obe.save(o, str(tmp_path / "after_batch.state"))
    restored = obe.load(str(tmp_path / "after_batch.state"))
    want = _cycles(o, 5, np.random.default_rng(2))
    for other in (twin, pickled, restored):
        _same(_cycles(other, 5, np.random.default_rng(2)), want)


# ------------------------------------------------------------------------- 7. the example, the audit, the figures
def test_recorded_data_example(hip):
    spec = importlib.util.spec_from_file_location("recorded_data", os.path.join(ROOT, "examples", "recorded_data.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    true, (mean, std), (mean2, std2), report = mod.main(n_records=120, n_samples=20000, seed=3, quiet=True)
    assert np.all(np.abs(mean - np.array(true)) < 5 * std + 1e-9)
    assert np.all(np.abs(mean - mean2) < 5 * (std + std2))
    assert len(report["stages"]) >= 2 and math.isfinite(report["log_evidence"])


def test_worst_errors_are_reported(hip):
    """(runs last of the comparisons: the worst error / tolerance ratios seen by this file's checks)"""
    for kind, (ratio, what) in sorted(WORST.items()):
        print(f"worst {kind}: {ratio:.3g} of its tolerance ({what})")
    import _replay
    print(f"worst weights: {_replay.WORST.get('weights', 0.0):.3g} relative (close_weights at 1e-10 on the exponent)")
    assert WORST and "weights" in _replay.WORST


def test_a_handful_under_the_delivery_audit(hip, tmp_path):
    """Once more in a child process with OBE_CHECK_DELIVERY=1 (the pattern of tests/test_gpu_scoring.py): no armed
    host word is read, no landing zone is released with armed words."""
    assert "OBE_BATCH_AUDIT_CHILD" not in os.environ, "the audited child must not start a child of its own"
    report = tmp_path / "audit.jsonl"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"), OBE_CHECK_DELIVERY="1",
               OBE_AUDIT_REPORT=str(report), OBE_BATCH_AUDIT_CHILD="1")
    chosen = "test_one_stage or test_tempered_run or test_noise_parameter_object or test_cycles_around"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider", "-k", chosen], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "DeliveryError" not in r.stdout + r.stderr and " passed" in r.stdout and "skipped" not in r.stdout
    rows = [json.loads(line) for line in report.read_text().splitlines()]
    assert rows and not any(row["pending_violations"] for row in rows), rows
    assert sum(row["reads"] for row in rows) > 100
