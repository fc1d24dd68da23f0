"""Device-side posterior summaries (ParticlePDF.marginal_histogram / joint_histogram / quantile / median /
credible_interval; csrc/obe_posterior.hip) against NumPy and against exactly rounded sums (tests/_posterior_oracle.py).

Weights of the form integer / 2^m make every sum exact in any order, so those cases are compared with
assert_array_equal / ==; general weights are held to the fixed-point form's own error bound
4 eps mass + n_bin 2^-62 sum(w) per bin, and to the bracket property of the exact weighted CDF for quantiles."""
import importlib.util
import json
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _posterior_oracle as oracle
import _state_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = (1 << 20) + 3
QS = (0.0, 0.025, 0.25, 0.5, 0.975, 1.0)
WORST = {}


def _pdf(x, w):
    import optbayesexpt_amd as obe
    pdf = obe.ParticlePDF(x)
    pdf.particle_weights = w
    return pdf


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------- 1. exact histograms
@pytest.mark.parametrize("n_dims", [1, 3, 10, 40])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000, BIG])
def test_histograms_of_dyadic_weights_are_numpys(hip, n, n_dims):
    g = np.random.default_rng([n, n_dims])
    x, w = oracle.dyadic_cloud(g, n_dims, n)
    pdf = _pdf(x, w)
    pairs = [(0, n_dims - 1)] + ([(n_dims // 2, 0)] if n_dims > 2 and n < BIG else [])     # (np.histogram2d is slow)
    for bins in (1, 2, 64, 1000):
        mass, edges = pdf.marginal_histogram(bins=bins)
        assert mass.shape == (n_dims, bins) and edges.shape == (n_dims, bins + 1)
        assert mass.dtype == edges.dtype == np.float64
        for r in range(n_dims):
            want, want_edges = np.histogram(x[r], bins, weights=w)
            assert_array_equal(edges[r], np.histogram_bin_edges(x[r], bins), err_msg=f"edges of row {r}, {bins} bins")
            assert_array_equal(edges[r], want_edges)
            assert_array_equal(mass[r], want, err_msg=f"row {r}, {bins} bins")
        # an explicit range for every row, and a selection of rows in another order
        dims = sorted({0, n_dims - 1, n_dims // 3}, reverse=True)
        mass, edges = pdf.marginal_histogram(dims=dims, bins=bins, range=(-1.5, 0.75))
        for k, r in enumerate(dims):
            want, want_edges = np.histogram(x[r], bins, (-1.5, 0.75), weights=w)
            assert_array_equal(edges[k], want_edges)
            assert_array_equal(mass[k], want, err_msg=f"row {r}, {bins} bins, explicit range")
        for dx, dy in pairs:
            for b2 in (bins, (bins, 3)):
                mass, xe, ye = pdf.joint_histogram(dx, dy, bins=b2)
                want, wxe, wye = np.histogram2d(x[dx], x[dy], b2, weights=w)
                assert_array_equal(xe, wxe)
                assert_array_equal(ye, wye)
                assert_array_equal(mass, want, err_msg=f"rows {dx} x {dy}, bins {b2}")


# ------------------------------------------------------------------------- 2. histograms of real posteriors
def _trajectory_posterior(name, cycles):
    """The object of a golden trajectory after ``cycles`` of its recorded measurements."""
    import _replay
    import optbayesexpt_amd as obe
    fx = _replay.load_traj(name)
    model = {"lorentzian": obe.models.lorentzian(1), "multi_lorentzian_7": obe.models.lorentzian(7)}[fx["meta"]["model"]]
    o = _replay.construct(fx, obe.OptBayesExpt, obe.OptBayesExptNoiseParameter, model)
    meta = fx["meta"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for cyc in range(cycles):
            x = o.opt_setting() if meta["selection"] == "opt" else o.good_setting(meta["pickiness"])
            y = float(fx["y_meas"][cyc][0])
            o.pdf_update((x, y, meta["sigma_meas"]) if meta["cls"] == "base" else (x, y))
    return o


_C3 = {}


def _c3_posterior():
    """A c3-size cloud (2^20 x 3) after three synthetic updates without a resample: a sharply peaked posterior."""
    if not _C3:
        g = np.random.default_rng(33)
        n = 1 << 20
        x = np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
        pdf = _pdf(x, np.ones(n) / n)
        pdf.tuning_parameters["auto_resample"] = False
        for centre, width in ((3.1, 0.2), (3.07, 0.05), (3.08, 0.012)):
            pdf.bayesian_update(np.exp(-0.5 * ((x[0] - centre) / width) ** 2) * (0.5 + g.random(n)))
        _C3["pdf"], _C3["x"] = pdf, x
        _C3["w"] = np.array(pdf.particle_weights)
    return _C3["pdf"], _C3["x"], _C3["w"]


def _check_masses(what, mass, exact, count, sum_w):
    bound = oracle.mass_bound(exact, count, sum_w)
    err = np.abs(mass - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.max(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))))
    WORST[what] = max(WORST.get(what, 0.0), ratio)
    assert np.all(err <= bound), (what, ratio)


def _check_histograms(what, pdf, x, w, bins=64):
    sum_w = math.fsum(oracle.clean_weights(w))
    mass, edges = pdf.marginal_histogram(bins=bins)
    for r in range(x.shape[0]):
        assert_array_equal(edges[r], np.histogram_bin_edges(x[r], bins))
        exact, count = oracle.histogram_fsum(x[r], w, edges[r])
        _check_masses(what, mass[r], exact, count, sum_w)
    assert abs(math.fsum(mass[0]) - sum_w) <= 5 * oracle.EPS * sum_w + x.shape[1] * 2.0 ** -62 * sum_w
    # a wide explicit range puts a converged posterior into one or two bins: every lane of a wave on one address
    lo, hi = float(np.min(x[0])), float(np.max(x[0]))
    wide = (lo - 50 * (hi - lo), hi + 50 * (hi - lo))
    mass, edges = pdf.marginal_histogram(dims=0, bins=bins, range=wide)
    exact, count = oracle.histogram_fsum(x[0], w, edges[0])
    _check_masses(what, mass[0], exact, count, sum_w)
    dy = x.shape[0] - 1
    mass, xe, ye = pdf.joint_histogram(0, dy, bins=(32, 16))
    flat = oracle.histogram2d_index(x[0], x[dy], xe, ye)
    order = np.argsort(flat, kind="stable")
    fs, ws = flat[order], oracle.clean_weights(w)[order]
    a = np.searchsorted(fs, np.arange(32 * 16), "left")
    b = np.searchsorted(fs, np.arange(32 * 16), "right")
    exact = np.array([math.fsum(ws[i:j]) for i, j in zip(a, b)]).reshape(32, 16)
    _check_masses(what, mass, exact, (b - a).reshape(32, 16), sum_w)


@pytest.mark.parametrize("name,cycles", [("lorentz3_demo", 30), ("multilorentz7_noise", 20)])
def test_histograms_of_a_trajectory_posterior_stay_inside_the_fixed_point_bound(hip, name, cycles):
    o = _trajectory_posterior(name, cycles)
    _check_histograms(name, o, np.array(o.particles), np.array(o.particle_weights))
    print(f"{name}: worst |mass - fsum| / bound = {WORST[name]:.4f}")


def test_histograms_of_a_c3_size_posterior_stay_inside_the_fixed_point_bound(hip):
    pdf, x, w = _c3_posterior()
    assert 1.0 / np.sum(w ** 2) < 0.05 * w.size                     # sharply peaked
    _check_histograms("c3", pdf, x, w)
    print(f"c3-size posterior: worst |mass - fsum| / bound = {WORST['c3']:.4f}")


# -------------------------------------------------------------------------------------- 3. edge semantics
def test_bin_membership_follows_the_edges(hip):
    g = np.random.default_rng(7)
    x, w = oracle.dyadic_cloud(g, 2, 5000)
    rng_, bins = (-1.0, 2.0), 37
    edges = np.histogram_bin_edges(x[0], bins, rng_)
    x[0, 10:10 + bins + 1] = edges                                  # every edge, first and last included
    x[0, 100:104] = (np.nextafter(edges[-1], np.inf), np.nextafter(edges[0], -np.inf), np.nextafter(edges[5], -np.inf),
                     np.nextafter(edges[-1], -np.inf))
    x[0, 200:204] = (np.nan, np.inf, -np.inf, -np.nan)
    x[1, 300:303] = (np.nan, np.inf, -np.inf)
    w[10:210] = np.maximum(w[10:210], 2.0 ** -30)                   # all of them carry weight
    pdf = _pdf(x, w)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want, want_edges = np.histogram(x[0], bins, rng_, weights=w)
        want2, wxe, wye = np.histogram2d(x[0], x[1], (bins, 5), (rng_, (-30.0, 30.0)), weights=w)
    mass, got_edges = pdf.marginal_histogram(dims=0, bins=bins, range=rng_)
    assert_array_equal(got_edges[0], want_edges)
    assert_array_equal(mass[0], want)
    assert mass[0, -1] >= w[10 + bins] and mass[0, 0] >= w[10]       # x == edges[-1] and x == edges[0] are counted
    mass2, xe, ye = pdf.joint_histogram(0, 1, bins=(bins, 5), range=(rng_, (-30.0, 30.0)))
    assert_array_equal(xe, wxe)
    assert_array_equal(ye, wye)
    assert_array_equal(mass2, want2)
    # the automatic range of a row that holds a NaN or an infinity is refused as NumPy refuses it
    for dims in (0, 1, None):
        with pytest.raises(ValueError, match="not finite"):
            pdf.marginal_histogram(dims=dims)
    with pytest.raises(ValueError, match="not finite"):
        pdf.joint_histogram(0, 1)
    # NaN weights count as zero
    w_nan = w.copy()
    w_nan[::7] = np.nan
    pdf.particle_weights = w_nan
    mass, _ = pdf.marginal_histogram(dims=0, bins=bins, range=rng_)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert_array_equal(mass[0], np.histogram(x[0], bins, rng_, weights=oracle.clean_weights(w_nan))[0])


def test_constant_row_density_and_signed_zero(hip):
    g = np.random.default_rng(8)
    x, w = oracle.dyadic_cloud(g, 3, 5000)
    x[1] = 2.75                                                     # NumPy's range for it: (2.25, 3.25)
    x[2, :50] = -0.0
    x[2, 50:100] = 0.0
    pdf = _pdf(x, w)
    for bins in (1, 4, 64):
        mass, edges = pdf.marginal_histogram(bins=bins)
        for r in range(3):
            want, want_edges = np.histogram(x[r], bins, weights=w)
            assert_array_equal(edges[r], want_edges)
            assert_array_equal(mass[r], want)
        dens, edges = pdf.marginal_histogram(bins=bins, density=True)
        for r in range(3):
            assert_allclose(dens[r], np.histogram(x[r], bins, weights=w, density=True)[0], rtol=1e-15, atol=0)
        dens2, _, _ = pdf.joint_histogram(0, 2, bins=(bins, 3), density=True)
        assert_allclose(dens2, np.histogram2d(x[0], x[2], (bins, 3), weights=w, density=True)[0], rtol=1e-15, atol=0)
    # general weights too: density within 1e-15 of NumPy's arithmetic on the device's masses
    pdf3, x3, w3 = _c3_posterior()
    dens, edges = pdf3.marginal_histogram(dims=0, bins=64, density=True)
    mass, _ = pdf3.marginal_histogram(dims=0, bins=64)
    assert_allclose(dens[0], mass[0] / np.diff(edges[0]) / mass[0].sum(), rtol=1e-15, atol=0)


# ------------------------------------------------------------------------------------------- 4. quantiles
def _quantile_cloud(g, n_dims, n):
    """Rows of five kinds — plain, heavy ties, subnormals, 1e300 scales, signed zeros with duplicates — and
    particles of weight zero below and above everything else in every row."""
    x, w = oracle.dyadic_cloud(g, n_dims, n, bits=24, top=200)
    for r in range(n_dims):
        kind = r % 5
        if kind == 1:
            x[r] = np.round(x[r] / np.max(np.abs(x[r])), 1)
        elif kind == 2:
            x[r] = g.integers(-40, 41, n) * 5e-324
        elif kind == 3:
            x[r] = g.normal(size=n) * 1e300 / 8
        elif kind == 4:
            x[r] = g.choice(np.array([-3.5, -0.0, 0.0, 0.0, 1.25, 7.0]), n)
        if n >= 8:
            lo, hi = min(float(x[r].min()), -5e-324), max(float(x[r].max()), 5e-324)
            x[r, 0:3] = 2 * lo
            x[r, 3:5] = 2 * hi
    if n >= 8:
        w[0:5] = 0.0
        w[5:8] = np.maximum(w[5:8], 2.0 ** -24)
    return x, w


@pytest.mark.parametrize("n_dims,n", [(1, 1), (1, 63), (3, 64), (1, 65), (10, 5000), (40, 5000), (1, BIG), (10, BIG)])
def test_quantiles_of_dyadic_weights_are_numpys_inverted_cdf(hip, n_dims, n):
    g = np.random.default_rng([n, n_dims, 4])
    x, w = _quantile_cloud(g, n_dims, n)
    pdf = _pdf(x, w)
    got = pdf.quantile(QS)
    assert got.shape == (n_dims, len(QS)) and got.dtype == np.float64
    for r in range(n_dims):
        want = oracle.quantile_numpy(x[r], w, QS)
        assert np.all(got[r] == want), (r, got[r], want)
        assert np.all(np.isin(got[r], x[r]))                         # always a value some particle holds
    assert np.all(pdf.quantile(0.25) == got[:, 2]) and pdf.quantile(0.25).shape == (n_dims,)
    assert np.all(pdf.median() == got[:, 3]) and pdf.median().shape == (n_dims,)
    ci = pdf.credible_interval(0.95)
    assert ci.shape == (n_dims, 2)
    assert np.all(ci == pdf.quantile(((1 - 0.95) / 2, 1 - (1 - 0.95) / 2)))
    dims = [n_dims - 1, 0]
    assert np.all(pdf.quantile(QS, dims=dims) == got[dims])
    assert np.all(pdf.credible_interval(0.5, dims=0) == pdf.quantile((0.25, 0.75), dims=0))
    many = np.linspace(0, 1, 37)                                    # more q than one library call serves
    assert np.all(pdf.quantile(many, dims=0)[0] == oracle.quantile_numpy(x[0], w, many))


def test_quantile_target_is_rounded_up(hip):
    """Weights of one unit of the fixed-point scale (2^-62 beside a weight of 1): q sum(Q) = 1.5 and 2.5 must reach 2
    and 3 units — the ceil of the definition; a floor would answer one particle too early."""
    x = np.array([[1.0, 2.0, 3.0, 4.0, 5.0]])
    w = np.array([2.0 ** -62, 2.0 ** -62, 2.0 ** -62, 1.0, 0.0])
    pdf = _pdf(x[:, ::-1].copy(), w[::-1].copy())
    qs = (1.0 * 2.0 ** -62, 1.5 * 2.0 ** -62, 2.0 * 2.0 ** -62, 2.5 * 2.0 ** -62, 3.5 * 2.0 ** -62, 1.0)
    want = oracle.quantile_numpy(x[0], w, qs)
    assert want.tolist() == [1.0, 2.0, 2.0, 3.0, 4.0, 4.0]
    assert pdf.quantile(qs)[0].tolist() == want.tolist()


def _check_brackets(what, pdf, x, w):
    w = oracle.clean_weights(w)
    sum_w = math.fsum(w)
    tol = x.shape[1] * 2.0 ** -62 * sum_w + 4 * oracle.EPS * sum_w
    got = pdf.quantile(QS)
    for r in range(x.shape[0]):
        order = np.argsort(x[r], kind="stable")
        xs, ws = x[r][order], w[order]
        for q, v in zip(QS, got[r]):
            i, j = np.searchsorted(xs, v, "left"), np.searchsorted(xs, v, "right")
            assert j > i, (what, r, q, v)                            # a value some particle holds
            below, upto = math.fsum(ws[:i]), math.fsum(ws[:j])      # F(v-), F(v), exactly rounded
            assert below <= q * sum_w + tol and upto >= q * sum_w - tol, (what, r, q, v, below, upto, q * sum_w, tol)
    assert np.all(pdf.median() == got[:, 3])
    assert np.all(pdf.credible_interval(0.95) == got[:, [1, 4]])


def test_quantiles_of_general_weights_bracket_the_exact_cdf(hip):
    pdf, x, w = _c3_posterior()
    _check_brackets("c3", pdf, x, w)
    for name, cycles in (("lorentz3_demo", 30), ("multilorentz7_noise", 20)):
        o = _trajectory_posterior(name, cycles)
        _check_brackets(name, o, np.array(o.particles), np.array(o.particle_weights))


# ----------------------------------------------------------------------------------------- 5. determinism
def test_results_are_bit_identical_from_run_to_run_and_under_permutation(hip):
    """What a histogram of float64 atomics fails: the same bits twice, and the same bits for a permuted cloud."""
    g = np.random.default_rng(55)
    n = 1 << 18
    x = np.array([g.normal(3.0, 0.01, n), g.uniform(-2000, -400, n), g.normal(size=n), g.exponential(2.0, n)])
    for spread in (0.002, 5.0):                                     # converged, and broad
        w = np.exp(-0.5 * ((x[0] - 3.001) / spread) ** 2) * g.random(n)
        w /= w.sum()
        perm = g.permutation(n)
        a, b = _pdf(x, w), _pdf(x[:, perm], w[perm])
        wide = [(2.0, 4.0), (-3000.0, 0.0), (-50.0, 50.0), (0.0, 1000.0)]
        calls = [lambda p: p.marginal_histogram(bins=64, range=wide)[0],
                 lambda p: p.marginal_histogram(bins=1000)[0],
                 lambda p: p.marginal_histogram(bins=5000, dims=(0, 3))[0],
                 lambda p: p.joint_histogram(0, 1, bins=(64, 64))[0],
                 lambda p: p.joint_histogram(0, 3, bins=(100, 100), range=((2.0, 4.0), (0.0, 50.0)))[0],
                 lambda p: p.quantile(QS),
                 lambda p: p.credible_interval(0.9)]
        for k, call in enumerate(calls):
            first = call(a)
            assert_array_equal(_bits(call(a)), _bits(first), err_msg=f"call {k}: second run")
            assert_array_equal(_bits(call(b)), _bits(first), err_msg=f"call {k}: permuted cloud")


# --------------------------------------------------------------------------------------- 6. no side effects
def _summaries(o):
    d = o.n_dims
    return (o.marginal_histogram(bins=32), o.marginal_histogram(dims=0, bins=40, range=(2.0, 4.0), density=True),
            o.joint_histogram(0, d - 1, bins=(16, 8)), o.quantile((0.1, 0.9)), o.median(), o.credible_interval(0.95))


def _flags(o):
    return (o._particles.version, o._weights.version, o._particles._host_valid, o._weights._host_valid,
            o._particles._dev_valid, o._weights._dev_valid, o._mom_host_key, o._mom_dev_key, o._cdf_key, o._sumsq_key,
            json.dumps(o.rng.bit_generator.state, sort_keys=True, default=str))


def _run(case, n, watch):
    o = cases.build(case)
    picks, resampled = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for cyc in range(n):
            x = o.opt_setting()
            picks.append(int(o.last_setting_index))
            if watch:
                before = _flags(o), o.sweep_state()
                _summaries(o)
                assert (_flags(o), o.sweep_state()) == before, f"cycle {cyc}, after opt_setting"
            o.pdf_update(cases.measure(o, case, cyc, x))
            resampled.append(bool(o.just_resampled))
            if watch:
                # behind a device-side update the host copies are stale, and they stay that way
                assert not o._weights._host_valid
                before = _flags(o), o.sweep_state()
                _summaries(o)
                assert (_flags(o), o.sweep_state()) == before, f"cycle {cyc}, after pdf_update"
                assert not o._weights._host_valid
                if any(resampled) and case != "function":         # (a host-callable model reads the cloud on the host)
                    assert not o._particles._host_valid
    return o, cases.outcome(o, picks, resampled)


@pytest.mark.parametrize("case", ["lorentz_full", "noise7", "function"])
def test_a_trajectory_is_unchanged_by_summaries_between_its_cycles(hip, case):
    """30 seeded cycles with all five methods called after every opt_setting() and every pdf_update() (for
    lorentz_full with a speculative sweep in flight) against the same run without them: settings, resample flags,
    weights, cloud and generator state bit for bit."""
    from optbayesexpt_amd import _state
    watched, got = _run(case, 30, True)
    plain, want = _run(case, 30, False)
    assert got["picks"] == want["picks"] and got["resampled"] == want["resampled"]
    assert any(want["resampled"])
    assert_array_equal(_bits(got["weights"]), _bits(want["weights"]))
    assert_array_equal(_bits(got["particles"]), _bits(want["particles"]))
    np.testing.assert_equal(got["rng"], want["rng"])
    assert set(_state.snapshot(watched)) == set(_state.snapshot(plain))          # nothing added to snapshots


# ------------------------------------------------------------------------------------------- 7. breadth
@pytest.mark.parametrize("case", ["noise7", "function", "sweeper"])
def test_experiment_objects_answer_for_their_cloud(hip, case):
    """A noise-parameter object with its constraint mask applied, a host-callable model object and a sweeper: the
    summaries describe ``particles`` / ``particle_weights`` as they stand."""
    o = cases.build(case)
    cases.run(o, case, 0, 12)
    x, w = np.array(o.particles), np.array(o.particle_weights)
    if case == "noise7":
        assert np.any(w == 0.0)                                     # the constraint zeroed some weights
    _check_histograms(case, o, x, w, bins=50)
    _check_brackets(case, o, x, w)


def test_host_edits_are_uploaded_first(hip):
    g = np.random.default_rng(71)
    x, w = oracle.dyadic_cloud(g, 3, 5000)
    pdf = _pdf(x, w)
    pdf.marginal_histogram()
    pdf.particle_weights[x[0] > 0] = 0                              # in place, by host code
    w2 = np.where(x[0] > 0, 0.0, w)
    mass, _ = pdf.marginal_histogram(bins=16)
    for r in range(3):
        assert_array_equal(mass[r], np.histogram(x[r], 16, weights=w2)[0])
    assert np.all(pdf.quantile(QS, dims=1)[0] == oracle.quantile_numpy(x[1], w2, QS))
    pdf.particles[1] *= 2.0
    assert np.all(pdf.quantile(QS, dims=1)[0] == oracle.quantile_numpy(2.0 * x[1], w2, QS))
    assert_array_equal(pdf.marginal_histogram(dims=1, bins=16)[0][0], np.histogram(2.0 * x[1], 16, weights=w2)[0])
    pdf.particle_weights = w[:-1]
    with pytest.raises(ValueError, match="different lengths"):
        pdf.median()


def test_sizes_that_cannot_be_served_are_refused(hip):
    from optbayesexpt_amd import _lib, _posterior
    g = np.random.default_rng(72)
    x, w = oracle.dyadic_cloud(g, 3, 1000)
    pdf = _pdf(x, w)
    with pytest.raises(ValueError, match="bins per call"):
        pdf.marginal_histogram(bins=(1 << 24) + 1)
    with pytest.raises(ValueError, match="bins per call"):
        pdf.marginal_histogram(bins=1 << 23)                        # three rows of them
    with pytest.raises(ValueError, match="bins per call"):
        pdf.joint_histogram(0, 1, bins=(8192, 4096))
    # ... and by the library itself, before anything is launched
    import torch
    p, wt = pdf._pw_tensors()
    rows = np.arange(3, dtype=np.int32)
    buf = torch.empty(1 << 16, dtype=torch.float64, device=p.device)
    P = _posterior._ptr
    with pytest.raises(_lib.ObeHipError, match="2\\^24") as e:
        pdf._lib.call("obe_weighted_histogram", P(p), p.shape[1], 3, 1000, P(wt), _lib.host_ptr(rows), 3, P(buf),
                      (1 << 24) + 1, P(buf), P(buf), buf.numel() * 8, pdf._stream())
    assert e.value.refused_before_launch
    with pytest.raises(_lib.ObeHipError, match="quantiles per call") as e:
        pdf._lib.call("obe_weighted_quantiles", P(p), p.shape[1], 3, 1000, P(wt), _lib.host_ptr(rows), 3,
                      _lib.host_ptr(np.full(17, 0.5)), 17, P(buf), P(buf), buf.numel() * 8, pdf._stream())
    assert e.value.refused_before_launch
    # the largest marginal the LDS form serves, and the first the global form does
    for bins in (4096, 4097):
        mass, _ = pdf.marginal_histogram(bins=bins)
        for r in range(3):
            assert_array_equal(mass[r], np.histogram(x[r], bins, weights=w)[0])


# --------------------------------------------------------------------------- 8. example and delivery audit
def test_posterior_summary_example(hip):
    spec = importlib.util.spec_from_file_location("posterior_summary", os.path.join(ROOT, "examples", "posterior_summary.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        true, history = mod.main(n_measure=60, n_samples=20000, every=10, seed=3, quiet=True)
    assert [h[0] for h in history] == [10, 20, 30, 40, 50, 60]
    i, median, lo, hi, mass, edges = history[-1]
    assert lo <= median <= hi and lo - 5 * (hi - lo) <= true[0] <= hi + 5 * (hi - lo)
    assert mass.shape == (40,) and edges.shape == (41,) and abs(mass.sum() - 1.0) < 1e-6
    widths = [h[3] - h[2] for h in history]
    assert widths[-1] < widths[0]


def test_this_file_under_the_delivery_audit(hip, tmp_path):
    """Once more in a child process with OBE_CHECK_DELIVERY=1 (the pattern of tests/test_gpu_state.py): no armed
    host word is read, no landing zone is released with armed words."""
    assert "OBE_POSTERIOR_AUDIT_CHILD" not in os.environ, "the audited child must not start a child of its own"
    report = tmp_path / "audit.jsonl"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"), OBE_CHECK_DELIVERY="1",
               OBE_AUDIT_REPORT=str(report), OBE_POSTERIOR_AUDIT_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider", "-k", "not test_this_file_under_the_delivery_audit"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "DeliveryError" not in r.stdout + r.stderr and " passed" in r.stdout and "skipped" not in r.stdout
    assert "1 deselected" in r.stdout
    rows = [json.loads(line) for line in report.read_text().splitlines()]
    assert rows and not any(row["pending_violations"] for row in rows), rows
    assert sum(row["reads"] for row in rows) > 100
