"""Posterior summaries, the part that needs no device: the oracles the GPU tests compare with are pinned against
NumPy, the argument checks raise ValueError before any library call, and the new entry points refuse bad arguments
with status -1 and a message without touching a device."""
import math
import types

import numpy as np
import pytest

import _posterior_oracle as oracle
from optbayesexpt_amd import _lib, _posterior

QS = (0.0, 0.025, 0.25, 0.5, 0.975, 1.0)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------------------------------------- the oracles
@pytest.mark.parametrize("n", [1, 7, 64, 5000])
@pytest.mark.parametrize("bins", [1, 2, 64, 1000])
def test_bin_oracle_is_numpys_histogram(n, bins):
    g = np.random.default_rng(n + bins)
    x, w = oracle.dyadic_cloud(g, 2, n)
    for rng_ in (None, (-0.5, 0.75)):
        edges = np.histogram_bin_edges(x[0], bins, rng_)
        if n >= 64:
            x[0, 5:5 + min(bins, 20)] = edges[1:1 + min(bins, 20)]     # values exactly on edges, the last one included
            x[0, 3] = edges[-1]
            edges = np.histogram_bin_edges(x[0], bins, rng_)
        want, want_edges = np.histogram(x[0], bins, rng_, weights=w)
        mass, count = oracle.histogram_fsum(x[0], w, edges)
        np.testing.assert_array_equal(want_edges, edges)
        np.testing.assert_array_equal(mass, want)                       # dyadic weights: every sum is exact
        np.testing.assert_array_equal(count, np.histogram(x[0], bins, rng_)[0])
        np.testing.assert_array_equal(_posterior.bin_edges(edges[0], edges[-1], bins), edges)


def test_bin_oracle_is_numpys_histogram2d():
    g = np.random.default_rng(5)
    x, w = oracle.dyadic_cloud(g, 2, 4000)
    x[0, :3] = (np.nan, np.inf, -np.inf)
    for bins, rng_ in ((7, None), ((3, 64), ((-1.0, 1.0), (-20.0, 5.0)))):
        ok = np.isfinite(x[0])
        src = x if rng_ is not None else x[:, ok]
        ww = w if rng_ is not None else w[ok]
        want, xe, ye = np.histogram2d(src[0], src[1], bins, rng_, weights=ww)
        flat = oracle.histogram2d_index(src[0], src[1], xe, ye)
        got = np.bincount(flat[flat >= 0], weights=ww[flat >= 0], minlength=want.size).reshape(want.shape)
        np.testing.assert_array_equal(got, want)


def test_fsum_oracle_against_numpy_with_general_weights():
    g = np.random.default_rng(11)
    x = g.normal(size=20000)
    w = np.exp(-0.5 * ((x - 0.3) / 0.01) ** 2) * g.random(x.size)
    w /= w.sum()
    edges = np.histogram_bin_edges(x, 64)
    mass, count = oracle.histogram_fsum(x, w, edges)
    want = np.histogram(x, 64, weights=w)[0]
    assert count.sum() == x.size
    assert np.all(np.abs(mass - want) <= 64 * oracle.EPS * want + 1e-300)
    # the fixed-point form stays inside its bound
    Q, k = oracle.integer_weights(w)
    assert k == 62
    idx = oracle.bin_index(x, edges)
    fixed = np.zeros(64, dtype=np.uint64)
    np.add.at(fixed, idx, Q)
    err = np.abs(np.ldexp(fixed.astype(np.float64), -k) - mass)
    assert np.all(err <= oracle.mass_bound(mass, count, math.fsum(w)))


@pytest.mark.parametrize("n", [1, 7, 1000, 5000])
def test_quantile_oracle_is_numpys_inverted_cdf(n):
    g = np.random.default_rng(3 + n)
    x, w = oracle.dyadic_cloud(g, 1, n, bits=20, top=50)
    x = x[0]
    if n >= 7:
        x[::5] = x[1::5][:len(x[::5])]                 # ties
        order = np.argsort(x)
        w[order[:2]] = 0.0                             # zero-weight particles at both ends
        w[order[-2:]] = 0.0
        x[2] = -0.0
    want = oracle.quantile_numpy(x, w, QS)
    got = oracle.quantile_fixed_point(x, w, QS)
    assert np.all(got == want), (got, want)
    for q, v in zip(QS, want):                         # the bracket property, exactly
        below, upto = oracle.cdf_bracket(x, w, v)
        assert below <= q * math.fsum(w) <= upto or q == 0.0


def test_scale_exponent_keeps_normalised_weights_at_62():
    assert oracle.scale_exponent(1.0) == 62
    assert oracle.scale_exponent(1.0 + 4 * oracle.EPS) == 62 == oracle.scale_exponent(1.0 - 4 * oracle.EPS)
    assert oracle.scale_exponent(1.0 + 2.0 ** -19) == 61
    assert oracle.scale_exponent(0.4) == 63 and oracle.scale_exponent(0.5) == 63 and oracle.scale_exponent(0.51) == 62
    assert oracle.scale_exponent(3.0) == 60 and oracle.scale_exponent(0.0) == 62
    for s in (1e-300, 0.3, 1.0, 7.5, 1e300):
        assert math.ldexp(s, oracle.scale_exponent(s)) <= 2.0 ** 62 * (1 + 2.0 ** -20)


# -------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_raise_value_error():
    P = _posterior
    assert P.check_bins(1) == 1 and P.check_bins(np.int64(64)) == 64
    for bad in (0, -3, 2.5, "64", None, True, P.MAX_BINS + 1):
        with pytest.raises(ValueError):
            P.check_bins(bad)
    assert P.check_bins2(8) == (8, 8) and P.check_bins2((3, 64)) == (3, 64)
    for bad in (0, (3,), (3, 0), (1, 2, 3), "ab", (4096, 4097)):
        with pytest.raises(ValueError):
            P.check_bins2(bad)
    q, scalar = P.check_q(0.5)
    assert scalar and q.tolist() == [0.5]
    q, scalar = P.check_q([0.0, 1.0])
    assert not scalar and q.tolist() == [0.0, 1.0]
    for bad in (-1e-9, 1.0000001, float("nan"), [0.5, 2.0], [], [[0.5]], "x"):
        with pytest.raises(ValueError):
            P.check_q(bad)
    assert P.check_level(0.95) == 0.95
    assert P.interval_quantiles(0.95) == ((1 - 0.95) / 2, 1 - (1 - 0.95) / 2)
    for bad in (-0.1, 1.5, float("nan"), "wide"):
        with pytest.raises(ValueError):
            P.check_level(bad)
    assert P.check_dims(None, 3).tolist() == [0, 1, 2] and P.check_dims(None, 3).dtype == np.int32
    assert P.check_dims(2, 3).tolist() == [2] and P.check_dims((2, 0, 2), 3).tolist() == [2, 0, 2]
    for bad in (3, -1, (0, 3), [], 1.0, (0.0,)):
        with pytest.raises(ValueError):
            P.check_dims(bad, 3)
    assert P.check_range(None, 4) is None
    assert P.check_range((0, 1), 3) == [(0.0, 1.0)] * 3
    assert P.check_range(((0, 1), (2, 3)), 2) == [(0.0, 1.0), (2.0, 3.0)]
    assert P.check_range((1.5, 1.5), 1) == [(1.5, 1.5)]                  # NumPy widens it to (1, 2)
    np.testing.assert_array_equal(P.bin_edges(1.5, 1.5, 2), [1.0, 1.5, 2.0])
    for bad, n in (((1, 0), 1), ((0, np.inf), 1), ((np.nan, 1), 1), (((0, 1),), 2), ((0, 1, 2), 1), (5, 1),
                   (((0, 1), (1, 0)), 2), (("a", "b"), 1)):
        with pytest.raises(ValueError):
            P.check_range(bad, n)


def test_methods_check_their_arguments_before_any_library_call():
    """The five methods exist on ParticlePDF (so the experiment classes inherit them) and refuse bad arguments before
    they touch the cloud: driven here on an object that has no device state at all."""
    from optbayesexpt_amd import OptBayesExpt, OptBayesExptNoiseParameter, OptBayesExptSweeper, ParticlePDF
    names = ("marginal_histogram", "joint_histogram", "quantile", "median", "credible_interval")
    for cls in (OptBayesExpt, OptBayesExptNoiseParameter, OptBayesExptSweeper):
        for name in names:
            assert getattr(cls, name) is getattr(ParticlePDF, name)
    fake = types.SimpleNamespace(n_dims=3)
    calls = [lambda: ParticlePDF.marginal_histogram(fake, bins=0),
             lambda: ParticlePDF.marginal_histogram(fake, dims=3),
             lambda: ParticlePDF.marginal_histogram(fake, range=(1, 0)),
             lambda: ParticlePDF.marginal_histogram(fake, range=((0, 1), (0, 1))),
             lambda: ParticlePDF.joint_histogram(fake, 0, 3),
             lambda: ParticlePDF.joint_histogram(fake, 0, 1, bins=(4, 0)),
             lambda: ParticlePDF.joint_histogram(fake, 0, 1, range=(0, 1)),
             lambda: ParticlePDF.joint_histogram(fake, 0, 1, bins=(8192, 4096)),
             lambda: ParticlePDF.quantile(fake, 1.5),
             lambda: ParticlePDF.quantile(fake, 0.5, dims=-1),
             lambda: ParticlePDF.median(fake, dims=7),
             lambda: ParticlePDF.credible_interval(fake, level=2),
             lambda: ParticlePDF.credible_interval(fake, dims=(0, 9))]
    for call in calls:
        with pytest.raises(ValueError):
            call()


# ---------------------------------------------------------------------------- the entry points' own refusals
def test_entry_points_refuse_bad_arguments_without_a_device(lib):
    dev = 1 << 20                    # (never dereferenced: every call below is refused by its argument checks)
    rows = np.array([0, 2], dtype=np.int32)
    q = np.array([0.025, 0.975])
    n, d = 1000, 3
    c = lib.cdll
    big = 1 << 30
    assert c.obe_posterior_workspace_bytes(n, 2, 64, 0) >= 8 * 2 * 64
    assert c.obe_posterior_workspace_bytes(n, 2, 0, 2) >= 8 * 2 * 2 * 256
    assert c.obe_posterior_workspace_bytes(n, 3, 0, 0) < c.obe_posterior_workspace_bytes(n, 3, 1000, 0)
    R, Q = _lib.host_ptr(rows), _lib.host_ptr(q)

    def refused(rc, word):
        assert rc == -1 and word in lib.last_error(), (rc, lib.last_error())

    # NULL pointers
    refused(c.obe_minmax_rows(None, n, d, n, R, 2, dev, dev, big, None), "null pointer")
    refused(c.obe_minmax_rows(dev, n, d, n, None, 2, dev, dev, big, None), "null pointer")
    refused(c.obe_minmax_rows(dev, n, d, n, R, 2, None, dev, big, None), "null pointer")
    refused(c.obe_weighted_histogram(dev, n, d, n, None, R, 2, dev, 64, dev, dev, big, None), "null pointer")
    refused(c.obe_weighted_histogram(dev, n, d, n, dev, R, 2, None, 64, dev, dev, big, None), "null pointer")
    refused(c.obe_weighted_histogram(dev, n, d, n, dev, R, 2, dev, 64, dev, None, big, None), "null pointer")
    refused(c.obe_weighted_histogram2d(dev, n, d, n, dev, 0, 1, dev, 8, None, 8, dev, dev, big, None), "null pointer")
    refused(c.obe_weighted_quantiles(dev, n, d, n, dev, R, 2, None, 2, dev, dev, big, None), "null pointer")
    refused(c.obe_weighted_quantiles(None, n, d, n, dev, R, 2, Q, 2, dev, dev, big, None), "null pointer")
    # sizes
    refused(c.obe_weighted_histogram(dev, n, d, n, dev, R, 2, dev, 0, dev, dev, big, None), "n_bins < 1")
    refused(c.obe_weighted_histogram(dev, n, d, n, dev, R, 2, dev, (1 << 24) + 1, dev, dev, big, None), "2^24")
    refused(c.obe_weighted_histogram2d(dev, n, d, n, dev, 0, 1, dev, 8, dev, 0, dev, dev, big, None), "n_bins < 1")
    refused(c.obe_weighted_histogram2d(dev, n, d, n, dev, 0, 1, dev, 8192, dev, 4096, dev, dev, big, None), "2^24")
    refused(c.obe_weighted_histogram2d(dev, n, d, n, dev, 0, 3, dev, 8, dev, 8, dev, dev, big, None), "out of range")
    refused(c.obe_weighted_histogram(dev, n - 1, d, n, dev, R, 2, dev, 64, dev, dev, big, None), "cloud size")
    refused(c.obe_weighted_histogram(dev, n, d, 0, dev, R, 2, dev, 64, dev, dev, big, None), "cloud size")
    refused(c.obe_weighted_histogram(dev, n, 2, n, dev, R, 2, dev, 64, dev, dev, big, None), "out of range")
    refused(c.obe_minmax_rows(dev, n, d, n, R, 0, dev, dev, big, None), "row count")
    # q outside [0, 1], too many of them
    for bad in (-0.1, 1.5, float("nan")):
        refused(c.obe_weighted_quantiles(dev, n, d, n, dev, R, 2, _lib.host_ptr(np.array([0.5, bad])), 2, dev, dev, big,
                                         None), "outside [0, 1]")
    refused(c.obe_weighted_quantiles(dev, n, d, n, dev, R, 2, Q, 0, dev, dev, big, None), "quantiles per call")
    refused(c.obe_weighted_quantiles(dev, n, d, n, dev, R, 2, _lib.host_ptr(np.full(17, 0.5)), 17, dev, dev, big, None),
            "quantiles per call")
    # a workspace that is too small
    refused(c.obe_minmax_rows(dev, n, d, n, R, 2, dev, dev, c.obe_posterior_workspace_bytes(n, 2, 0, 0) - 1, None),
            "workspace too small")
    refused(c.obe_weighted_histogram(dev, n, d, n, dev, R, 2, dev, 64, dev, dev,
                                     c.obe_posterior_workspace_bytes(n, 2, 64, 0) - 1, None), "workspace too small")
    refused(c.obe_weighted_histogram2d(dev, n, d, n, dev, 0, 1, dev, 8, dev, 8, dev, dev,
                                       c.obe_posterior_workspace_bytes(n, 1, 64, 0) - 1, None), "workspace too small")
    refused(c.obe_weighted_quantiles(dev, n, d, n, dev, R, 2, Q, 2, dev, dev,
                                     c.obe_posterior_workspace_bytes(n, 2, 0, 2) - 1, None), "workspace too small")
    with pytest.raises(_lib.ObeHipError) as e:
        lib.call("obe_weighted_quantiles", dev, n, d, n, dev, R, 2, Q, 2, dev, dev, 0, None)
    assert e.value.refused_before_launch
