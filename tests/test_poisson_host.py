"""Counted events, the parts that need no GPU: identities of the NumPy oracle (tests/_poisson_oracle.py), the inputs of
the GPU tests, the argument checks of optbayesexpt_amd/obe_poisson.py, the state fields, and the C ABI's declarations
and refusals."""
import math
import pickle
import types

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _poisson_oracle as oracle
from optbayesexpt_amd import _lib, _state, build, obe_poisson
from optbayesexpt_amd.obe_poisson import check_cap, check_exposure, check_record_counts

NEW_ENTRY_POINTS = ("obe_poisson_likelihood", "obe_poisson_workspace_bytes", "obe_poisson_information")


def _case(kind, n):
    seed, make = {"wide": (300, oracle.lorentz_cloud), "converged": (400, oracle.converged_cloud)}[kind]
    g = np.random.default_rng(seed + n)
    cloud = make(g, n)
    return cloud, oracle.weights(g, cloud), oracle.lorentz_rates(cloud)


# ------------------------------------------------------------------------------------------- oracle identities
@pytest.mark.parametrize("cap", oracle.CAPS)
def test_information_of_a_single_particle_and_of_equal_rates_is_zero(cap):
    g = np.random.default_rng(1)
    R = g.uniform(0.5, 12.0, (7, 1))
    got = oracle.information(R, [0.3], cap=cap)
    assert np.all(got >= 0.0) and np.all(got <= 1e-14)
    R = np.repeat(R, 9, axis=1)                                          # a cloud whose particles agree
    assert np.all(oracle.information(R, np.arange(1.0, 10.0), cap=cap) <= 1e-14)


def test_information_grows_with_the_cap_and_converges():
    _, w, R = _case("wide", 257)
    by_cap = [oracle.information(R, w, 1.0, cap) for cap in oracle.CAPS]
    assert np.all(by_cap[0] <= by_cap[1] + 1e-14) and np.all(by_cap[1] <= by_cap[2] + 1e-14)
    assert np.max(np.abs(by_cap[2] - by_cap[1])) <= 1e-9                 # rates <= 12: nothing left beyond 32 counts
    assert by_cap[1].max() > 0.2
    # data processing: censoring at 16 where the counts reach 48 loses information, strictly
    low, high = oracle.information(R, w, 4.0, 16), oracle.information(R, w, 4.0, 64)
    assert np.all(low < high) and high.max() > 0.5 and low.max() < 0.8 * high.max()
    # ... and a short exposure tells little
    assert oracle.information(R, w, 0.05, 32).max() < 0.03


@pytest.mark.parametrize("cap", oracle.CAPS)
@pytest.mark.parametrize("exposure", [0.05, 1.0, 4.0])
def test_distribution_sums_to_one(cap, exposure):
    _, w, R = _case("wide", 257)
    pmf = oracle.count_distribution(R, w, exposure, cap)
    assert pmf.shape == (130, cap + 1) and np.all(pmf >= 0.0)
    assert_allclose(pmf.sum(axis=1), 1.0, rtol=0.0, atol=1e-12)


def test_likelihood_is_the_poisson_pmf():
    stats = pytest.importorskip("scipy.stats")
    g = np.random.default_rng(3)
    r = g.uniform(0.0, 40.0, (1, 500))
    for k, t in ((0, 1.0), (1, 1.0), (7, 0.5), (40, 1.0), (1000, 30.0)):
        assert_allclose(oracle.likelihood(r, [k], [t], 1), stats.poisson.pmf(k, t * r[0]), rtol=1e-11, atol=1e-300)
    # ... and the design's per-particle terms: the same pmf, formed for every outcome
    p, tau, _ = oracle._particle_terms(r[0], 32)
    assert_allclose(p, stats.poisson.pmf(np.arange(32).reshape(-1, 1), r[0]), rtol=1e-11, atol=1e-300)
    assert_allclose(tau, stats.poisson.sf(31, r[0]), rtol=0.0, atol=1e-14)
    # two channels multiply
    r2 = g.uniform(0.5, 9.0, (2, 50))
    want = stats.poisson.pmf(3, 2.0 * r2[0]) * stats.poisson.pmf(0, 0.5 * r2[1])
    assert_allclose(oracle.likelihood(r2, [3, 0], [2.0, 0.5], 2), want, rtol=1e-12)


def test_likelihood_special_cases():
    r = np.array([[0.0, -1.0, np.nan, np.inf, 1e-300, 700.0, 800.0, 2.0]])
    zero = oracle.likelihood(r, [0], [1.0], 1)
    assert_array_equal(zero[:4], [1.0, 0.0, 0.0, 0.0])                  # lambda = 0 with k = 0: the factor 1
    assert_array_equal(zero[4:], np.exp(-r[0, 4:]))                     # -lambda alone, no log
    three = oracle.likelihood(r, [3], [1.0], 1)
    assert_array_equal(three[:4], [0.0] * 4)                            # lambda = 0 with k > 0: L = 0
    assert three[4] == 0.0 and three[6] == 0.0 and 0.0 < three[5] < 1e-290
    assert_allclose(three[7], 8.0 * math.exp(-2.0) / 6.0, rtol=1e-15)
    assert_allclose(oracle.likelihood(r, [3], [1.0], 1, choke=0.5)[7], math.sqrt(three[7]), rtol=1e-15)
    # log k! keeps a large record's exponent below 0
    assert_allclose(oracle.log_likelihood(np.array([[1000.0]]), [1000], [1.0], 1), [-4.372], atol=1e-3)
    # n_lik = 1 takes the first channel alone, but a bad rate in ANY channel still excludes the particle
    r2 = np.array([[2.0, 2.0], [3.0, -3.0]])
    assert_allclose(oracle.likelihood(r2, [1, 1], [1.0, 1.0], 1), [2.0 * math.exp(-2.0), 0.0], rtol=1e-15)
    assert_array_equal(oracle.likelihood(r2, [1, 1], [1.0, 1.0], 0), [1.0, 0.0])


def test_who_contributes():
    R = np.array([[2.0, 5.0, 9.0, np.nan, 3.0, 7.0],
                  [2.0, -1.0, 9.0, 4.0, 3.0, np.inf]])
    w = np.array([1.0, 2.0, 1.0, 0.0, np.nan, 3.0])
    assert_array_equal(oracle.contributing(R, w), [[1, 1, 1, 0, 0, 1], [1, 0, 1, 0, 0, 0]])
    want0 = oracle.design(R[:1][:, [0, 1, 2, 5]], w[[0, 1, 2, 5]])
    want1 = oracle.design(R[1:][:, [0, 2]], w[[0, 2]])
    got = oracle.design(R, w)
    assert_array_equal(got[0], [want0[0][0], want1[0][0]])
    assert_array_equal(got[1], np.concatenate([want0[1], want1[1]]))
    assert_allclose(oracle.noise_variance(R, w, 4.0)[0, 1], (2.0 + 9.0) / 2.0 / 4.0, rtol=1e-15)
    assert np.all(np.isnan(oracle.information(R, np.zeros(6)))) and np.all(np.isnan(oracle.noise_variance(R, -w)))
    assert np.all(np.isnan(oracle.count_distribution(R, np.full(6, np.nan))))


# --------------------------------------------------------------------------------- the inputs of the GPU tests
@pytest.mark.parametrize("n", [257, 4097])
def test_gpu_inputs(n):
    """The figures the GPU tests lean on, from the oracle alone, and float64 against extended precision."""
    cloud, w, R = _case("wide", n)
    assert R.shape == (130, n) and 2.0 <= R.min() and R.max() <= 12.0
    info, pmf = oracle.design(R, w, 1.0, 32)
    assert 0.2 <= info.max() <= 0.3 and pmf[:, -1].max() <= 1e-8
    info16, pmf16 = oracle.design(R, w, 1.0, 16)
    assert 1e-3 <= pmf16[:, -1].max() <= 1e-2 and abs(info16.max() - info.max()) < 1e-3
    assert oracle.count_distribution(R, w, 4.0, 16)[:, -1].max() >= 0.5           # censoring bites
    want = oracle.information(R[::13], w, 1.0, 32, dtype=np.longdouble)
    assert want.dtype == np.longdouble and np.max(np.abs(want - info[::13])) <= 1e-13
    nu = oracle.noise_variance(R[::13], w, 2.0)
    assert np.max(np.abs(oracle.noise_variance(R[::13], w, 2.0, dtype=np.longdouble) - nu) / nu) <= 1e-14
    cloud, w, R = _case("converged", n)
    assert abs(np.std(cloud[0]) - 0.002) < 3e-4
    assert 1e-5 <= oracle.information(R, w, 1.0, 32).max() <= 1e-3
    # every record of the likelihood tests (k <= 1000, exposure x rate <= 1e3) has log L >= -600 on these rates
    assert oracle.log_likelihood(R[:1], [0], [50.0], 1).min() >= -600.0


# ------------------------------------------------------------------------------------------- argument checks
def test_exposure_and_cap():
    assert_array_equal(check_exposure(1, 1), [1.0])
    assert_array_equal(check_exposure(0.25, 3), [0.25] * 3)
    assert_array_equal(check_exposure([1, 64.5], 2), [1.0, 64.5])
    assert_array_equal(check_exposure(np.float64(7.0), 2), [7.0, 7.0])
    for bad in (0, -1, np.nan, np.inf, [1, 2, 3], [[1, 2]], "a", [1, 0], None, []):
        with pytest.raises(ValueError):
            check_exposure(bad, 2)
    assert [check_cap(c) for c in (16, 32, 64, np.int64(32), 64.0)] == [16, 32, 64, 32, 64]
    for bad in (0, 8, 17, 33, 128, -16, 16.5, None, "32", True, np.nan):
        with pytest.raises(ValueError, match="16, 32, 64"):
            check_cap(bad)


def test_counts_of_a_record():
    n_lik, k, t, lf = check_record_counts(3, 1.0, 1)
    assert n_lik == 1 and k[0] == 3.0 and t[0] == 1.0 and lf[0] == math.lgamma(4.0)
    assert k.dtype == t.dtype == lf.dtype == np.float64 and k.flags.c_contiguous
    assert k.size == t.size == lf.size == _lib.OBE_MAX_CHANNELS
    n_lik, k, t, lf = check_record_counts([3, 0], 0.5, 2)                 # one exposure for both channels
    assert n_lik == 2 and list(k[:2]) == [3.0, 0.0] and list(t[:2]) == [0.5, 0.5] and lf[1] == 0.0
    n_lik, k, t, lf = check_record_counts([3, 1000], [7.5, 64], 2)
    assert n_lik == 2 and list(t[:2]) == [7.5, 64.0] and lf[1] == math.lgamma(1001.0)
    assert check_record_counts(np.array([2.0]), np.array([5.0, 9.0]), 2)[0] == 1      # truncated to the shorter
    assert check_record_counts([1, 1, 1], 1, 2)[0] == 2
    for counts, exposure in ((0.5, 1), (-1, 3), (np.nan, 1), (np.inf, 1), (1, 0), (1, -2.5), (1, np.inf), (1, np.nan),
                             ("a", 1), ([[1]], 1), ([], 1), (1, [])):
        with pytest.raises(ValueError):
            check_record_counts(counts, exposure, 2)


# ----------------------------------------------------------------------------------------------------- the state
def test_state_fields_round_trip():
    for exposure, cap in ((4, 16), (np.array([0.5, 64.0]), 64)):
        obj = types.SimpleNamespace(exposure=exposure, count_cap=cap)
        fields = obe_poisson.state_fields(obj)
        assert sorted(fields) == ["count_cap", "exposure"]
        back = obe_poisson.kwargs_from_state(pickle.loads(pickle.dumps({"poisson": fields}))["poisson"])
        assert_array_equal(check_exposure(back["exposure"], 2), check_exposure(exposure, 2))
        assert back["count_cap"] == cap and type(back["count_cap"]) is int
    from optbayesexpt_amd import OptBayesExptPoisson
    assert _state.library_class(type("Mine", (OptBayesExptPoisson,), {})) is OptBayesExptPoisson
    assert _state.library_class(OptBayesExptPoisson) is OptBayesExptPoisson


def _with_attributes(cls):
    """An object of a user's subclass of ``cls`` as far as the snapshot's filter looks: its ``__dict__``."""
    o = object.__new__(type("Mine", (cls,), {}))
    o.__dict__.update(exposure=0.25, count_cap=7, utility_method="variance_approx", my_note="kept", _private=1)
    return o


def test_exposure_and_count_cap_are_the_librarys_own_on_this_class_only():
    import optbayesexpt_amd as obe
    assert not {"exposure", "count_cap"} & set(_state.LIBRARY_ATTRIBUTES)
    assert _state.user_attributes(_with_attributes(obe.OptBayesExptPoisson)) == {"my_note": "kept"}
    for cls in (obe.ParticlePDF, obe.OptBayesExpt, obe.OptBayesExptNoiseParameter, obe.OptBayesExptSignalNoise,
                obe.OptBayesExptBinomial, obe.OptBayesExptSweeper):
        assert _state.user_attributes(_with_attributes(cls)) == {"exposure": 0.25, "count_cap": 7, "my_note": "kept"}, \
            cls.__name__


def test_class_is_exported_and_checks_its_arguments_first():
    import optbayesexpt_amd as obe
    from optbayesexpt_amd import models
    assert obe.OptBayesExptPoisson is obe_poisson.OptBayesExptPoisson
    assert issubclass(obe.OptBayesExptPoisson, obe.OptBayesExpt)
    grid, cloud = (np.linspace(0, 1, 5),), np.ones((3, 8))
    with pytest.raises(ValueError, match="DeviceModel"):
        obe.OptBayesExptPoisson(lambda s, p, c: p[0] * s[0], grid, cloud, ())
    with pytest.raises(ValueError, match="exposure"):
        obe.OptBayesExptPoisson(models.lorentzian(1), grid, cloud, (0.1,), exposure=0)
    with pytest.raises(ValueError, match="count_cap"):
        obe.OptBayesExptPoisson(models.lorentzian(1), grid, cloud, (0.1,), count_cap=48)
    with pytest.raises(ValueError, match="variance_approx"):           # (names the utilities that do work)
        obe.OptBayesExptPoisson(models.coil(), grid, cloud, ())


# --------------------------------------------------------------------------------------------------- the C ABI
def test_new_entry_points_are_declared_and_served_by_plugins():
    declared = _lib.declared_symbols()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.MODEL_ENTRY_POINTS, name
        assert name in declared and name in _lib.PROTOTYPES, name
    assert set(_lib.MODEL_ENTRY_POINTS) <= set(declared)
    assert "obe_poisson.hip" in build.PLUGIN_SOURCES
    assert _lib.OBE_ABI_VERSION == 3 and _lib.OBE_POISSON_MAX_CAP == 64
    # no host result parameters: nothing for the delivery audit to rule
    for name in NEW_ENTRY_POINTS:
        for ctype, p in _lib.PROTOTYPES[name][1]:
            assert not (p.startswith("h_") and ("out" in p or "best" in p)), (name, p)
    names = [p for _, p in _lib.PROTOTYPES["obe_poisson_information"][1]]
    assert names == ["m", "d_settings", "ld_s", "n_settings", "d_particles", "ld_p", "n_particles", "d_weights",
                     "exposure", "cap", "d_cost", "cost", "d_information", "d_tail", "d_pmf", "d_noise_var", "d_ws",
                     "ws_bytes", "stream"]
    names = [p for _, p in _lib.PROTOTYPES["obe_poisson_likelihood"][1]]
    assert names == ["m", "d_y", "ld_y", "d_particles", "ld_p", "n_particles", "h_setting", "h_counts", "h_exposure",
                     "h_logfact", "n_lik_channels", "choke", "d_lik", "stream"]
    assert _lib.PROTOTYPES["obe_poisson_workspace_bytes"][0] is _lib.c_int64


def test_workspace_is_monotone_and_knows_no_cloud():
    lib = _lib.load()
    size = lib.cdll.obe_poisson_workspace_bytes
    assert size(1000, 65, 1, 32) == size(1, 65, 1, 32) == size(1 << 40, 65, 1, 32)
    assert size(1000, 65, 1, 16) >= 8 * (16 + 4) * 64 * 2                # 16 + tau + h + one rate + W, two tiles
    for n_c in (1, 2, 8):
        last = 0
        for cap in (0, 1, 16, 17, 32, 33, 64, 1000):
            for n_s in (1, 63, 64, 65, 130, 1 << 20):
                assert size(1000, n_s, n_c, cap) >= size(1000, max(n_s - 1, 1), n_c, cap) > 0
                assert n_c == 1 or size(1000, n_s, n_c, cap) > size(1000, n_s, n_c - 1, cap)
            assert size(1000, 130, n_c, cap) >= last
            last = size(1000, 130, n_c, cap)
        assert size(1000, 130, n_c, 16) < size(1000, 130, n_c, 32) < size(1000, 130, n_c, 64)


def test_bad_arguments_are_refused_before_any_launch():
    """Every bad argument: status -1 with a telling word, on a machine without a GPU too."""
    from optbayesexpt_amd import models
    lib = _lib.load()
    m = models.lorentzian(1).struct(3, (0.1,))
    coil = models.coil().struct(3, ())
    dev = 1 << 20                        # (never dereferenced: every call below is refused on its arguments)
    hp = _lib.host_ptr
    ws = lib.cdll.obe_poisson_workspace_bytes(1000, 65, 1, 32)
    nan, inf = float("nan"), float("inf")

    def information(model=m, settings=dev, ld_s=65, n_s=65, particles=dev, n_p=1000, ld_p=1000, weights=dev,
                    exposure=1.0, cap=32, info=dev, tail=dev, pmf=dev, nu=dev, d_ws=dev, ws_bytes=ws):
        return lib.cdll.obe_poisson_information(model, settings, ld_s, n_s, particles, ld_p, n_p, weights, exposure, cap,
                                                None, 1.0, info, tail, pmf, nu, d_ws, ws_bytes, None)
    for kw, word in ((dict(settings=None), "null"), (dict(particles=None), "null"), (dict(weights=None), "null"),
                     (dict(d_ws=None), "null"), (dict(info=None, tail=None, pmf=None, nu=None), "all of"),
                     (dict(model=None), "null"), (dict(n_s=0), "n_settings"), (dict(ld_s=64), "n_settings"),
                     (dict(n_p=0), "cloud"), (dict(ld_p=999), "cloud"), (dict(exposure=0.0), "exposure"),
                     (dict(exposure=nan), "exposure"), (dict(exposure=inf), "exposure"), (dict(exposure=-1.0), "exposure"),
                     (dict(cap=0), "cap"), (dict(cap=8), "cap"), (dict(cap=33), "cap"), (dict(cap=128), "cap"),
                     (dict(cap=-16), "cap"), (dict(ws_bytes=ws - 8), "workspace"), (dict(ws_bytes=0), "workspace"),
                     (dict(cap=64), "workspace"),                                   # (a larger cap needs more)
                     (dict(model=coil), "one channel"), (dict(model=coil, info=None, pmf=None), "one channel"),
                     (dict(model=coil, info=None, tail=None), "one channel"),
                     (dict(model=coil, info=None, tail=None, pmf=None), "workspace")):   # (nu alone: two channels need more)
        assert information(**kw) == -1, kw
        assert word in lib.last_error(), (kw, lib.last_error())

    one, zero = np.ones(8), np.zeros(8)
    setting = np.zeros(_lib.OBE_MAX_SETDIMS)

    def likelihood(model=m, d_y=None, ld_y=0, particles=dev, ld_p=1000, n_p=1000, x=setting, k=zero, t=one, lf=zero,
                   n_lik=1, out=dev):
        # (the host arrays live until the call has returned)
        arr = [None if a is None else np.array(a, dtype=np.float64) for a in (k, t, lf)]
        return lib.cdll.obe_poisson_likelihood(model, d_y, ld_y, particles, ld_p, n_p, None if x is None else hp(x),
                                               *[None if a is None else hp(a) for a in arr], n_lik, nan, out, None)
    for kw, word in ((dict(out=None), "null"), (dict(k=None), "null"), (dict(t=None), "null"), (dict(lf=None), "null"),
                     (dict(model=None), "null"), (dict(x=None), "h_setting"),
                     (dict(n_p=0), "n_particles"), (dict(particles=None), "no cloud"), (dict(ld_p=999), "shorter"),
                     (dict(d_y=dev, ld_y=999), "shorter"), (dict(n_lik=2), "n_lik_channels"),
                     (dict(n_lik=-1), "n_lik_channels"), (dict(model=coil, n_lik=3), "n_lik_channels"),
                     (dict(k=[0.5] + [0] * 7), "count"), (dict(k=[-1.0] + [0] * 7), "count"),
                     (dict(k=[nan] + [0] * 7), "count"), (dict(k=[inf] + [0] * 7), "count"),
                     (dict(t=[0.0] + [1] * 7), "exposure"), (dict(t=[-1.5] + [1] * 7), "exposure"),
                     (dict(t=[inf] + [1] * 7), "exposure"), (dict(t=[nan] + [1] * 7), "exposure"),
                     (dict(model=coil, n_lik=2, k=[0.0, 2.5] + [0] * 6), "count"),
                     (dict(model=coil, n_lik=2, t=[1.0, 0.0] + [1] * 6), "exposure")):
        assert likelihood(**kw) == -1, kw
        assert word in lib.last_error(), (kw, lib.last_error())
