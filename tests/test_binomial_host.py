"""Yes/no outcomes, the parts that need no GPU: identities of the NumPy oracle (tests/_binomial_oracle.py), the inputs
of the GPU tests, the count checks of optbayesexpt_amd/obe_binomial.py, the state fields, and the C ABI's declarations
and refusals."""
import pickle
import types

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _binomial_oracle as oracle
from optbayesexpt_amd import _lib, _state, build, obe_binomial
from optbayesexpt_amd.obe_binomial import check_channels, check_counts, check_shots

NEW_ENTRY_POINTS = ("obe_binomial_likelihood", "obe_binomial_workspace_bytes", "obe_binomial_information")
LOG2 = float(np.log(2.0))


# ------------------------------------------------------------------------------------------- oracle identities
def _random_case(seed, n_c, n=200, n_s=7):
    g = np.random.default_rng(seed)
    return g.uniform(0.02, 0.98, (n_s, n_c, n)), g.random(n) + 0.01


@pytest.mark.parametrize("n_c", [1, 2, 3])
def test_information_of_a_single_particle_is_zero(n_c):
    P, _ = _random_case(1, n_c, n=1)
    got = oracle.information(P, [0.3])
    assert np.all(got >= 0.0) and np.all(got <= 1e-15)
    # ... and so is that of a cloud whose particles agree
    P = np.repeat(P, 9, axis=2)
    assert np.all(oracle.information(P, np.arange(1.0, 10.0)) <= 1e-15)


@pytest.mark.parametrize("n_c", [1, 2, 3])
def test_information_of_certain_outcomes_is_the_entropy_of_the_marginal(n_c):
    """p in {0, 1}: h2 = 0 for every particle, what is left is H(Pbar)."""
    g = np.random.default_rng(2)
    P = g.integers(0, 2, (5, n_c, 40)).astype(np.float64)
    w = g.random(40)
    pbar = oracle.outcome_marginals(P, w)
    assert_allclose(pbar.sum(axis=1), 1.0, rtol=1e-14)
    assert_array_equal(oracle.information(P, w), -np.sum(oracle.xlogx(pbar), axis=1))
    # two equally likely hypotheses that one shot tells apart: one bit
    assert_allclose(oracle.information(np.array([[[0.0, 1.0]]]), [1.0, 1.0]), [LOG2], rtol=1e-15)
    # ... and in nats per unit cost
    assert_allclose(oracle.information(np.array([[[0.0, 1.0]]]), [1.0, 1.0], cost=4.0), [LOG2 / 4.0], rtol=1e-15)


@pytest.mark.parametrize("n_c", [1, 2, 3])
def test_joint_information_is_at_most_the_sum_over_the_channels(n_c):
    P, w = _random_case(3 + n_c, n_c)
    joint, per_channel = oracle.information(P, w), oracle.channel_information(P, w)
    assert per_channel.shape == (n_c, P.shape[0]) and np.all(joint > 1e-3)
    if n_c == 1:
        assert_array_equal(joint, per_channel[0])
    else:
        assert np.all(joint <= per_channel.sum(axis=0) + 1e-15)
        assert np.all(joint >= per_channel.max(axis=0) - 1e-15)          # (a further channel never takes away)
    assert np.all(joint <= n_c * LOG2)


@pytest.mark.parametrize("n_c", [1, 2, 3])
def test_information_does_not_care_which_outcome_is_called_success(n_c):
    P, w = _random_case(7 + n_c, n_c)
    assert_allclose(oracle.information(1.0 - P, w), oracle.information(P, w), rtol=0.0, atol=1e-14)
    flipped = P.copy()
    flipped[:, 0] = 1.0 - flipped[:, 0]                                 # one channel alone
    assert_allclose(oracle.information(flipped, w), oracle.information(P, w), rtol=0.0, atol=1e-14)
    assert_allclose(oracle.noise_variance(1.0 - P, w), oracle.noise_variance(P, w), rtol=1e-14)


def test_who_contributes():
    """Zero, NaN and negative weights, and at a setting a particle with a p there that is no probability."""
    P = np.array([[[0.2, 0.5, 0.9, np.nan, 0.3, 0.7]],
                  [[0.2, 1.5, 0.9, 0.4, 0.3, -1e-9]]])
    w = np.array([1.0, 2.0, 1.0, 0.0, np.nan, 3.0])
    keep = oracle.contributing(P, w)
    assert_array_equal(keep, [[1, 1, 1, 0, 0, 1], [1, 0, 1, 0, 0, 0]])
    want0 = oracle.information(P[:1][:, :, [0, 1, 2, 5]], w[[0, 1, 2, 5]])
    want1 = oracle.information(P[1:][:, :, [0, 2]], w[[0, 2]])
    assert_array_equal(oracle.information(P, w), [want0[0], want1[0]])
    assert_allclose(oracle.noise_variance(P, w, 4.0)[0, 1], (0.2 * 0.8 + 0.9 * 0.1) / 2.0 / 4.0, rtol=1e-15)
    assert np.all(np.isnan(oracle.information(P, np.zeros(6)))) and np.all(np.isnan(oracle.noise_variance(P, -w)))


def test_likelihood_closed_forms():
    p = np.array([[0.25, 0.5, 0.0, 1.0, 0.0, 1.0, -1e-9, 1.0 + 1e-9, np.nan]])
    # three successes in four shots, no binomial coefficient
    got = oracle.likelihood(p, [3.0], [4.0], 1)
    assert_allclose(got[:2], [0.25 ** 3 * 0.75, 0.5 ** 4], rtol=1e-15)
    assert_array_equal(got[2:], [0.0] * 7)
    # a count of zero skips its term: p = 0 with k = 0 and p = 1 with k = n are certain, not 0 * inf
    assert_array_equal(oracle.likelihood(p, [0.0], [4.0], 1)[[2, 4]], [1.0, 1.0])
    assert_array_equal(oracle.likelihood(p, [4.0], [4.0], 1)[[3, 5]], [1.0, 1.0])
    assert_array_equal(oracle.likelihood(p, [0.0], [4.0], 1)[[3, 6, 7, 8]], [0.0] * 4)
    assert_array_equal(oracle.log_likelihood(p, [1.0], [1.0], 1)[[2, 6, 7, 8]], [-np.inf] * 4)
    # channels multiply; n_lik = 1 takes the first alone, but a bad p in ANY channel still excludes the particle
    p2 = np.array([[0.25, 0.25], [0.5, 1.5]])
    assert_allclose(oracle.likelihood(p2, [1.0, 0.0], [1.0, 2.0], 2), [0.25 * 0.25, 0.0], rtol=1e-15)
    assert_allclose(oracle.likelihood(p2, [1.0, 0.0], [1.0, 2.0], 1), [0.25, 0.0], rtol=1e-15)
    assert_array_equal(oracle.likelihood(p2, [1.0, 0.0], [1.0, 2.0], 0), [1.0, 0.0])
    assert_allclose(oracle.likelihood(p2, [1.0, 0.0], [1.0, 2.0], 2, choke=0.5), [0.25, 0.0], rtol=1e-15)


def test_noise_variance_closed_forms():
    P = np.full((3, 1, 11), 0.25)
    w = np.random.default_rng(1).random(11)
    assert_allclose(oracle.noise_variance(P, w), np.full((1, 3), 0.1875), rtol=4e-16)
    assert_allclose(oracle.noise_variance(P, w, 4.0), np.full((1, 3), 0.1875 / 4.0), rtol=4e-16)
    P2 = np.stack([P[:, 0], 2.0 * P[:, 0]], axis=1)
    assert_allclose(oracle.noise_variance(P2, w, [1.0, 5.0]), [[0.1875] * 3, [0.05] * 3], rtol=4e-16)


# --------------------------------------------------------------------------------- the inputs of the GPU tests
def _extended_agrees(P, w):
    got = oracle.information(P, w)
    want = oracle.information(P, w, dtype=np.longdouble)
    assert want.dtype == np.longdouble
    assert np.max(np.abs(want - got)) <= 1e-14
    nu, nu_want = oracle.noise_variance(P, w), oracle.noise_variance(P, w, dtype=np.longdouble)
    assert np.max(np.abs(nu_want - nu) / nu_want) <= 1e-14
    return got


@pytest.mark.parametrize("n", oracle.N_PARTICLES)
def test_gpu_inputs_one_channel_and_converged(n):
    """What the GPU tests' tolerance leans on, from the oracle alone — every Pbar_o >= 0.01, the largest information
    >= 1e-5 (a cloud of one particle has none: the identity above) —, and float64 against extended precision."""
    for kind, make, seed in (("wide", oracle.lorentz_cloud, 300), ("converged", oracle.converged_cloud, 400)):
        g = np.random.default_rng(seed + n)
        cloud = make(g, n)
        w = oracle.weights(g, cloud)
        P = oracle.lorentz_probabilities(cloud)
        assert P.shape == (130, 1, n) and P.min() >= 0.10 and P.max() <= 0.90
        assert np.ptp(w) > 0 or n == 1
        u = _extended_agrees(P, w)
        assert oracle.outcome_marginals(P, w).min() >= 0.01
        if n > 1:
            assert u.max() >= 1e-5, (kind, u.max())
        if kind == "wide" and n >= 300:
            assert 0.05 <= u.max() <= 0.065, u.max()
        if kind == "converged" and n >= 300:
            assert abs(np.std(cloud[0]) - 0.002) < 2e-4 and 2e-5 <= u.max() <= 2e-4, u.max()


@pytest.mark.parametrize("n", [300, 4097])
def test_gpu_inputs_two_channels(n):
    g = np.random.default_rng(500 + n)
    cloud = oracle.ramsey_cloud(g, n)
    w = oracle.weights(g, cloud)
    P = oracle.ramsey_probabilities(cloud)
    assert P.shape == (65, 2, n) and P.min() >= 0.019 and P.max() <= 1.0 - 0.019
    u = _extended_agrees(P, w)
    assert oracle.outcome_marginals(P, w).min() >= 0.01
    assert 0.1 <= u.max() <= 2 * LOG2
    # |log L| <= 64 * 2 * |log 0.019| < 510 for every record of at most 64 shots in two channels
    assert 64 * 2 * abs(np.log(0.019)) < 510


# ------------------------------------------------------------------------------------------- argument checks
def test_shots_and_channels():
    assert_array_equal(check_shots(1, 1), [1.0])
    assert_array_equal(check_shots(4, 3), [4.0, 4.0, 4.0])
    assert_array_equal(check_shots([1, 64], 2), [1.0, 64.0])
    assert_array_equal(check_shots(np.float64(7.0), 2), [7.0, 7.0])
    for bad in (0, -1, 1.5, np.nan, np.inf, [1, 2, 3], [[1, 2]], "a", [1, 0], None):
        with pytest.raises(ValueError):
            check_shots(bad, 2)
    assert [check_channels(c) for c in (1, 2, 3)] == [1, 2, 3]
    for bad in (0, 4, 8):
        with pytest.raises(ValueError, match="3"):
            check_channels(bad)


def test_counts_of_a_record():
    n_lik, k, n = check_counts(1, 1, 1)
    assert n_lik == 1 and k[0] == 1.0 and n[0] == 1.0 and k.dtype == n.dtype == np.float64
    assert k.flags.c_contiguous and k.size == n.size == _lib.OBE_BINOMIAL_MAX_CHANNELS
    n_lik, k, n = check_counts([3, 0], 7, 2)                          # one n for both channels
    assert n_lik == 2 and list(k[:2]) == [3.0, 0.0] and list(n[:2]) == [7.0, 7.0]
    n_lik, k, n = check_counts([3, 64], [7, 64], 2)
    assert n_lik == 2 and list(n[:2]) == [7.0, 64.0]
    assert check_counts(np.array([2.0]), np.array([5.0, 9.0]), 2)[0] == 1          # truncated to the shorter, as a reading is
    assert check_counts([1, 1, 1], 1, 2)[0] == 2
    for successes, shots in ((0.5, 1), (2, 1), (-1, 3), (np.nan, 1), (1, 0), (1, 2.5), (1, np.inf), ([1, 5], [1, 4]),
                             ("a", 1), ([[1]], 1), (1, -3), ([], 1)):
        with pytest.raises(ValueError):
            check_counts(successes, shots, 2)


# ----------------------------------------------------------------------------------------------------- the state
def test_state_fields_round_trip():
    for shots in (4, np.array([1.0, 64.0])):
        obj = types.SimpleNamespace(shots=shots)
        fields = obe_binomial.state_fields(obj)
        assert sorted(fields) == ["shots"]
        back = obe_binomial.kwargs_from_state(pickle.loads(pickle.dumps({"binomial": fields}))["binomial"])
        assert_array_equal(check_shots(back["shots"], 2), check_shots(shots, 2))
    from optbayesexpt_amd import OptBayesExptBinomial
    assert _state.library_class(type("Mine", (OptBayesExptBinomial,), {})) is OptBayesExptBinomial
    assert _state.library_class(OptBayesExptBinomial) is OptBayesExptBinomial


def _with_attributes(cls):
    """An object of a user's subclass of ``cls`` as far as the snapshot's filter looks: its ``__dict__``."""
    o = object.__new__(type("Mine", (cls,), {}))
    o.__dict__.update(shots=1000, utility_method="variance_approx", my_note="kept", _private=1)
    return o


def test_shots_is_the_librarys_own_on_this_class_only():
    """``shots`` and ``utility_method`` of an OptBayesExptBinomial are rebuilt by its constructor and do not travel
    twice; on every other class ``shots`` is the user's own name (say, readings averaged per update) and travels in
    the snapshot's ``user`` dict, as it did before there was this class."""
    import optbayesexpt_amd as obe
    assert "utility_method" in _state.LIBRARY_ATTRIBUTES and "shots" not in _state.LIBRARY_ATTRIBUTES
    assert _state.user_attributes(_with_attributes(obe.OptBayesExptBinomial)) == {"my_note": "kept"}
    for cls in (obe.ParticlePDF, obe.OptBayesExpt, obe.OptBayesExptNoiseParameter, obe.OptBayesExptSignalNoise,
                obe.OptBayesExptSweeper):
        assert _state.user_attributes(_with_attributes(cls)) == {"shots": 1000, "my_note": "kept"}, cls.__name__


def test_a_particle_cloud_keeps_its_own_shots_through_a_snapshot():
    """The whole of ``snapshot()`` on a host-only ParticlePDF (no GPU here), and the snapshot's pickle."""
    import torch
    from optbayesexpt_amd._mirror import Mirror
    from optbayesexpt_amd.particlepdf import ParticlePDF
    o = ParticlePDF.__new__(ParticlePDF)
    o._device = torch.device("cpu")
    o._particles = Mirror(o._device, host=np.random.default_rng(2).uniform(size=(2, 20)))
    o._weights = Mirror(o._device, host=np.full(20, 0.05))
    o.n_particles, o.n_dims = 20, 2
    o._rng = np.random.default_rng(4)
    o.tuning_parameters = dict(a_param=0.98, resample_threshold=0.5, auto_resample=True, scale=True)
    o.just_resampled = False
    o._pending_total = o._mom_dev_key = o._mom_host_key = o._sumsq_key = o._sumsq = None
    o.shots = 1000
    assert pickle.loads(pickle.dumps(_state.snapshot(o)))["user"] == {"shots": 1000}


def test_class_is_exported_and_checks_its_model_first():
    import optbayesexpt_amd as obe
    from optbayesexpt_amd import models
    assert obe.OptBayesExptBinomial is obe_binomial.OptBayesExptBinomial
    assert issubclass(obe.OptBayesExptBinomial, obe.OptBayesExpt)
    grid, cloud = (np.linspace(0, 1, 5),), np.ones((3, 8))
    with pytest.raises(ValueError, match="DeviceModel"):
        obe.OptBayesExptBinomial(lambda s, p, c: p[0] * s[0], grid, cloud, ())
    with pytest.raises(ValueError, match="shots"):
        obe.OptBayesExptBinomial(models.lorentzian(1), grid, cloud, (0.1,), shots=0)
    four = models.DeviceModel.__new__(models.DeviceModel)                  # (a model of four channels, never built)
    four.n_channels = 4
    with pytest.raises(ValueError, match="OBE_BINOMIAL_MAX_CHANNELS"):
        obe.OptBayesExptBinomial(four, grid, cloud, ())


# --------------------------------------------------------------------------------------------------- the C ABI
def test_new_entry_points_are_declared_and_served_by_plugins():
    declared = _lib.declared_symbols()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.MODEL_ENTRY_POINTS, name
        assert name in declared and name in _lib.PROTOTYPES, name
    assert set(_lib.MODEL_ENTRY_POINTS) <= set(declared)
    assert "obe_binomial.hip" in build.PLUGIN_SOURCES
    assert _lib.OBE_ABI_VERSION == 3 and _lib.OBE_BINOMIAL_MAX_CHANNELS == 3
    # no host result parameters: nothing for the delivery audit to rule
    for name in NEW_ENTRY_POINTS:
        for ctype, p in _lib.PROTOTYPES[name][1]:
            assert not (p.startswith("h_") and ("out" in p or "best" in p)), (name, p)
    names = [p for _, p in _lib.PROTOTYPES["obe_binomial_information"][1]]
    assert names == ["m", "d_settings", "ld_s", "n_settings", "d_particles", "ld_p", "n_particles", "d_weights",
                     "shots", "d_cost", "cost", "d_information", "d_noise_var", "d_ws", "ws_bytes", "stream"]
    names = [p for _, p in _lib.PROTOTYPES["obe_binomial_likelihood"][1]]
    assert names == ["m", "d_y", "ld_y", "d_particles", "ld_p", "n_particles", "h_setting", "h_successes", "h_shots",
                     "n_lik_channels", "choke", "d_lik", "stream"]
    assert _lib.PROTOTYPES["obe_binomial_workspace_bytes"][0] is _lib.c_int64


def test_workspace_is_monotone_and_knows_no_cloud():
    lib = _lib.load()
    size = lib.cdll.obe_binomial_workspace_bytes
    assert size(1000, 65, 1) == size(1, 65, 1) == size(1 << 40, 65, 1)
    assert size(1000, 65, 1) >= 8 * 5 * 64 * 2                        # 2 + 1 + 1 + 1 sums per lane, two tiles
    last = 0
    for n_c in (1, 2, 3):
        for n_s in (1, 63, 64, 65, 130, 1 << 20):
            assert size(1000, n_s, n_c) >= size(1000, max(n_s - 1, 1), n_c) > 0
            assert n_c == 1 or size(1000, n_s, n_c) > size(1000, n_s, n_c - 1)
        assert size(1000, 130, n_c) > last
        last = size(1000, 130, n_c)


def test_bad_arguments_are_refused_before_any_launch():
    """Every bad argument: status -1 with a telling word, on a machine without a GPU too."""
    from optbayesexpt_amd import models
    lib = _lib.load()
    m = models.lorentzian(1).struct(3, (0.1,))
    coil = models.coil().struct(3, ())
    four = models.lorentzian(1).struct(3, (0.1,))
    four.n_channels = 4
    dev = 1 << 20                        # (never dereferenced: every call below is refused on its arguments)
    hp = _lib.host_ptr
    ws = lib.cdll.obe_binomial_workspace_bytes(1000, 65, 1)
    nan = float("nan")

    def information(model=m, settings=dev, ld_s=65, n_s=65, particles=dev, n_p=1000, ld_p=1000, weights=dev, shots=1.0,
                    info=dev, nu=dev, d_ws=dev, ws_bytes=ws):
        return lib.cdll.obe_binomial_information(model, settings, ld_s, n_s, particles, ld_p, n_p, weights, shots, None,
                                                 1.0, info, nu, d_ws, ws_bytes, None)
    for kw, word in ((dict(settings=None), "null"), (dict(particles=None), "null"), (dict(weights=None), "null"),
                     (dict(d_ws=None), "null"), (dict(info=None, nu=None), "both"), (dict(model=None), "null"),
                     (dict(n_s=0), "n_settings"), (dict(ld_s=64), "n_settings"), (dict(n_p=0), "cloud"),
                     (dict(ld_p=999), "cloud"), (dict(shots=0.0), "shots"), (dict(shots=0.5), "shots"),
                     (dict(shots=nan), "shots"), (dict(shots=float("inf")), "shots"), (dict(shots=-1.0), "shots"),
                     (dict(ws_bytes=ws - 8), "workspace"), (dict(ws_bytes=0), "workspace"),
                     (dict(model=coil, ws_bytes=ws), "workspace"),                  # (two channels need more)
                     (dict(model=four), "OBE_BINOMIAL_MAX_CHANNELS")):
        assert information(**kw) == -1, kw
        assert word in lib.last_error(), (kw, lib.last_error())

    one, zero = np.ones(3), np.zeros(3)

    setting = np.zeros(_lib.OBE_MAX_SETDIMS)

    def likelihood(model=m, d_y=None, ld_y=0, particles=dev, ld_p=1000, n_p=1000, x=setting, k=zero, n=one, n_lik=1,
                   out=dev):
        # (the two host arrays live until the call has returned)
        kk = None if k is None else np.array(k, dtype=np.float64)
        nn = None if n is None else np.array(n, dtype=np.float64)
        return lib.cdll.obe_binomial_likelihood(model, d_y, ld_y, particles, ld_p, n_p, None if x is None else hp(x),
                                                None if kk is None else hp(kk), None if nn is None else hp(nn),
                                                n_lik, nan, out, None)
    for kw, word in ((dict(out=None), "null"), (dict(k=None), "null"), (dict(n=None), "null"), (dict(model=None), "null"),
                     (dict(x=None), "h_setting"),                                  # (no setting to evaluate the model at)
                     (dict(n_p=0), "n_particles"), (dict(particles=None), "no cloud"), (dict(ld_p=999), "shorter"),
                     (dict(d_y=dev, ld_y=999), "shorter"), (dict(n_lik=2), "n_lik_channels"),
                     (dict(n_lik=-1), "n_lik_channels"), (dict(model=four), "OBE_BINOMIAL_MAX_CHANNELS"),
                     (dict(k=[0.5, 0, 0]), "count"), (dict(k=[-1.0, 0, 0]), "count"), (dict(k=[2.0, 0, 0]), "count"),
                     (dict(k=[nan, 0, 0]), "count"), (dict(n=[0.0, 1, 1]), "count"), (dict(n=[1.5, 1, 1]), "count"),
                     (dict(n=[float("inf"), 1, 1]), "count"), (dict(n=[nan, 1, 1]), "count"),
                     (dict(model=coil, n_lik=2, k=[0.0, 3.0, 0], n=[1.0, 2.0, 1]), "count")):
        assert likelihood(**kw) == -1, kw
        assert word in lib.last_error(), (kw, lib.last_error())
