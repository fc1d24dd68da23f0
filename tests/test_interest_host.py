"""Design for parameters of interest, everything that needs no GPU: the oracle of tests/_interest_oracle.py pinned
against NumPy and a closed form, the argument checks of optbayesexpt_amd/_interest.py, the entry points' refusals.
Two checks that read like host checks are in tests/test_gpu_interest.py, because both need a constructed object and the
constructor allocates on a device: the unknown-method message that lists the new name
(test_the_new_method_is_named_and_needs_a_device_model), and the snapshot with and without the new key
(test_state_carries_the_parameters_of_interest: restoring a state constructs an object)."""
import types

import numpy as np
import pytest

import _interest_oracle as oracle
from optbayesexpt_amd import _interest, _lib, models, obe_base

NAMES = ("obe_output_covariance_workspace_bytes", "obe_output_covariance", "obe_variance_reduction")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the oracle
def test_oracle_is_numpys_weighted_covariance():
    g = np.random.default_rng(1)
    n = 300
    theta = g.normal(size=(3, n)) * np.array([[1.0], [30.0], [0.01]]) + np.array([[5.0], [-200.0], [0.0]])
    y = np.vstack([theta[0] * theta[1] + theta[2], np.sin(theta[0]) + 0.1 * theta[1]])
    w = g.random(n)
    b = oracle.blocks(y, theta, w)
    full = np.cov(np.vstack([theta, y]), aweights=w, ddof=0)
    tol_S, tol_K, tol_V = oracle.tolerances(b)
    # NumPy's own sums are double: it is held to a hundredth of the bar the device is held to
    assert np.all(np.abs(b["S"] - full[3:, 3:]) <= 1e-2 * tol_S)
    assert np.all(np.abs(b["K"] - full[:3, 3:]) <= 1e-2 * tol_K)
    assert np.all(np.abs(b["V"] - np.diag(full)[:3]) <= 1e-2 * tol_V)
    assert np.all(np.abs(b["m"] - np.average(y, axis=1, weights=w)) <= 1e-12 * b["A_c"])
    assert np.all(np.abs(b["t"] - np.average(theta, axis=1, weights=w)) <= 1e-12 * b["A_d"])
    assert np.all(b["B_S"] >= np.abs(b["S"])) and np.all(b["B_K"] >= np.abs(b["K"]))
    assert np.all(b["A_c"] >= np.abs(b["m"])) and np.all(b["A_d"] >= np.abs(b["t"]))
    assert b["S"].shape == (2, 2) and b["K"].shape == (3, 2) and np.array_equal(b["S"], b["S"].T)


def test_oracle_leaves_out_what_has_no_weight():
    g = np.random.default_rng(2)
    n = 50
    theta, y, w = g.normal(size=(2, n)), g.normal(size=(1, n)), g.random(n)
    want = oracle.blocks(y, theta, w)
    w2 = np.concatenate([w, [0.0, np.nan, -1.0]])
    theta2 = np.hstack([theta, [[np.inf, np.nan, 1e300]] * 2])
    y2 = np.hstack([y, [[np.nan, np.inf, -1e300]]])
    got = oracle.blocks(y2, theta2, w2)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    # a weighted particle with a non-finite y makes the blocks non-finite
    y2[0, 3] = np.inf
    assert not np.any(np.isfinite(oracle.blocks(y2, theta2, w2)["S"]))


def test_oracle_gain_is_the_closed_form_for_a_line():
    """y = a + b x is linear in (a, b): S = J Sigma J^T and K = Sigma J^T exactly with J = (1, x) and Sigma the
    cloud's covariance, so G_d = (Sigma J)_d^2 / (J Sigma J^T + nu) whatever the cloud."""
    g = np.random.default_rng(3)
    n = 4096
    theta = np.array([g.normal(2.0, 0.5, n), g.normal(-1.0, 0.2, n)]) + 0.3 * g.normal(size=n)       # correlated
    w = g.random(n)
    sigma_theta = np.cov(theta, aweights=w, ddof=0)
    nu = 0.04
    worst = 0.0
    for x in np.linspace(-2.0, 3.0, 9):
        b = oracle.blocks((theta[0] + theta[1] * x)[None, :], theta, w)
        G, u, cond = oracle.gain(b["S"], b["K"], [nu])
        J = np.array([1.0, x])
        want = (sigma_theta @ J) ** 2 / (J @ sigma_theta @ J + nu)
        worst = max(worst, float(np.max(np.abs(G - want) / want)))
        assert cond == pytest.approx(1.0)
        assert np.all(G <= b["V"] * (1 + 1e-12))           # no estimator removes more variance than there is
    assert worst < 1e-13, worst


def test_oracle_gain_with_two_correlated_channels_is_numpys_solve():
    g = np.random.default_rng(4)
    n = 2000
    theta = g.normal(size=(3, n))
    y = np.vstack([theta[0] + 0.5 * theta[1] ** 2, theta[0] - theta[2] + 0.1 * theta[1]])
    w = g.random(n)
    b = oracle.blocks(y, theta, w)
    assert abs(b["S"][0, 1]) > 0.3 * np.sqrt(b["S"][0, 0] * b["S"][1, 1])           # the channels are correlated
    nu = np.array([0.3, 0.05])
    G, u, cond = oracle.gain(b["S"], b["K"], nu)
    full = np.cov(np.vstack([theta, y]), aweights=w, ddof=0)
    a = full[3:, 3:] + np.diag(nu)
    for d in range(3):
        k = full[d, 3:]
        want = k @ np.linalg.solve(a, k)
        assert abs(G[d] - want) <= 1e-12 * want
        assert abs(G[d] - k @ np.linalg.inv(a) @ k) <= 1e-12 * want
    assert 1.0 < cond < 1e3
    # the utility: a term with V == 0 is 0, the cost divides
    U = oracle.utility(G[:, None] * np.ones((1, 4)), np.array([b["V"][0], 0.0, b["V"][2]]), [1.0, 5.0, 2.0],
                       np.array([1.0, 2.0, 4.0, 8.0]))
    np.testing.assert_allclose(U * np.array([1.0, 2.0, 4.0, 8.0]), G[0] / b["V"][0] + 2.0 * G[2] / b["V"][2], rtol=1e-15)


# ---------------------------------------------------------------------------------------- the argument checks
def test_dims_check():
    assert _interest.check_dims(None, 3) == (0, 1, 2)
    assert _interest.check_dims(2, 3) == (2,)
    assert _interest.check_dims(np.int64(1), 3) == (1,)
    assert _interest.check_dims([2, 0], 3) == (2, 0)
    assert _interest.check_dims(np.array([1, 2]), 3) == (1, 2)
    assert _interest.check_dims(range(10), 10) == tuple(range(10))
    for bad in ([0, 0], [1, 2, 1], 3, -1, [0, 3], [], (), 1.0, [0.0], "x0", [None], True, [True], 2.5, object()):
        with pytest.raises(ValueError):
            _interest.check_dims(bad, 3)


def test_weights_check():
    np.testing.assert_array_equal(_interest.check_weights(None, 3), np.ones(3))
    np.testing.assert_array_equal(_interest.check_weights([1, 0, 0], 3), [1.0, 0.0, 0.0])
    np.testing.assert_array_equal(_interest.check_weights(2.5, 1), [2.5])
    for bad in ([1, 2], [0, 0, 0], [1, -1, 1], [1, np.nan, 1], [1, np.inf, 1], ["a", 1, 1], [[1, 2, 3], [1, 2, 3]]):
        with pytest.raises(ValueError):
            _interest.check_weights(bad, 3)


def test_noise_variance_forms():
    nv = _interest.noise_variance
    grid = 5

    def model(value):
        return lambda: value
    # sigma given: squared, (C, 1) or (C, n_x)
    np.testing.assert_array_equal(nv(2.0, None, 2, 7, grid, True), [[4.0], [4.0]])
    np.testing.assert_array_equal(nv([1.0, 3.0], None, 2, 7, grid, True), [[1.0], [9.0]])
    assert nv(np.full((2, 7), 0.5), None, 2, 7, grid, True).shape == (2, 7)
    assert nv(np.full(7, 0.5), None, 1, 7, grid, True).shape == (1, 7)
    for bad in (0.0, -1.0, np.nan, [1.0, 2.0, 3.0], np.ones((2, 6)), np.ones((3, 7)), "x"):
        with pytest.raises(ValueError):
            nv(bad, None, 2, 7, grid, True)
    # the object's noise model: per channel in any of its forms
    for value in (4.0, np.array([4.0]), np.array([[4.0]])):
        np.testing.assert_array_equal(nv(None, model(value), 2, 7, grid, True), [[4.0], [4.0]])
    np.testing.assert_array_equal(nv(None, model(np.array([[1.0], [2.0]])), 2, 7, grid, True), [[1.0], [2.0]])
    np.testing.assert_array_equal(nv(None, model(np.array([1.0, 2.0])), 2, 7, grid, False), [[1.0], [2.0]])
    # per setting of the design grid: only for the design grid
    per_setting = np.arange(10.0).reshape(2, grid) + 1.0
    np.testing.assert_array_equal(nv(None, model(per_setting), 2, grid, grid, False), per_setting)
    with pytest.raises(ValueError, match="pass sigma"):
        nv(None, model(per_setting), 2, grid, grid, True)
    with pytest.raises(ValueError, match="pass sigma"):
        nv(None, model(per_setting), 2, 7, grid, True)
    np.testing.assert_array_equal(nv(3.0, model(per_setting), 2, 7, grid, True), [[9.0], [9.0]])      # sigma decides
    with pytest.raises(ValueError, match="shape"):
        nv(None, model(np.ones((2, grid + 1))), 2, grid, grid, False)


def test_unpack_lower():
    packed = np.array([[1.0, 10.0], [2.0, 20.0], [3.0, 30.0], [4.0, 40.0], [5.0, 50.0], [6.0, 60.0]])
    full = _interest.unpack_lower(packed, 3)
    np.testing.assert_array_equal(full[:, :, 0], [[1, 2, 4], [2, 3, 5], [4, 5, 6]])
    np.testing.assert_array_equal(full[:, :, 1], 10 * full[:, :, 0])


def test_methods_check_their_arguments_before_any_library_call():
    from optbayesexpt_amd import OptBayesExpt, OptBayesExptNoiseParameter, OptBayesExptSweeper
    methods = ("output_covariance", "expected_variance_reduction", "set_parameters_of_interest",
               "parameters_of_interest", "utility_parameter_variance")
    for cls in (OptBayesExptNoiseParameter, OptBayesExptSweeper):
        for name in methods:
            assert getattr(cls, name) is getattr(OptBayesExpt, name)
    assert "parameter_variance" in obe_base.UTILITY_METHODS
    per_setting = np.ones((2, 5))
    fake = types.SimpleNamespace(_device_model=object(), allsettings=np.zeros((1, 5)), n_channels=2, n_dims=3,
                                 _n_settings=5, yvar_noise_model=lambda: per_setting, _interest=None)
    calls = [lambda: OptBayesExpt.output_covariance(fake, dims=[0, 0]),
             lambda: OptBayesExpt.output_covariance(fake, dims=3),
             lambda: OptBayesExpt.output_covariance(fake, dims=[]),
             lambda: OptBayesExpt.expected_variance_reduction(fake, dims=[1.5]),
             lambda: OptBayesExpt.expected_variance_reduction(fake, settings=(1.0, 2.0)),
             lambda: OptBayesExpt.expected_variance_reduction(fake, settings=([1.0, 2.0],), sigma=-1.0),
             lambda: OptBayesExpt.expected_variance_reduction(fake, settings=([1.0, 2.0],), sigma=np.ones((2, 3))),
             # a noise model per setting of the design grid says nothing about settings of the caller's own
             lambda: OptBayesExpt.expected_variance_reduction(fake, settings=([1.0, 2.0],)),
             lambda: OptBayesExpt.set_parameters_of_interest(fake, [0, 1], [1.0]),
             lambda: OptBayesExpt.set_parameters_of_interest(fake, [0, 1], [0.0, 0.0]),
             lambda: OptBayesExpt.set_parameters_of_interest(fake, [0, 7])]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    assert fake._interest is None
    OptBayesExpt.set_parameters_of_interest(fake, [2, 0], [1, 3])
    assert fake._interest[0] == (2, 0) and fake._interest[1].tolist() == [1.0, 3.0]
    OptBayesExpt.set_parameters_of_interest(fake, None)
    assert fake._interest[0] == (0, 1, 2) and fake._interest[1].tolist() == [1.0, 1.0, 1.0]
    host = types.SimpleNamespace(_device_model=None, n_dims=3, n_channels=1, _n_settings=5, allsettings=np.zeros((1, 5)),
                                 yvar_noise_model=lambda: 1.0, parameters_of_interest=((0,), np.ones(1)))
    for call in (lambda: OptBayesExpt.output_covariance(host), lambda: OptBayesExpt.expected_variance_reduction(host, dims=0),
                 lambda: OptBayesExpt.utility_parameter_variance(host)):
        with pytest.raises(TypeError, match="from_function.*from_expression"):
            call()


# ------------------------------------------------------------------------------------------ the entry points
def test_symbols_are_declared_exported_and_bound(lib):
    for name in NAMES:
        assert name in _lib.declared_symbols() and name in _lib.PROTOTYPES
        fn = getattr(lib.cdll, name)
        restype, params = _lib.PROTOTYPES[name]
        assert fn.restype is restype and len(fn.argtypes) == len(params)
    # the blocks depend on the model (every plugin brings them), the finish does not
    assert set(NAMES[:2]) <= set(_lib.MODEL_ENTRY_POINTS) and NAMES[2] not in _lib.MODEL_ENTRY_POINTS
    assert _lib.PROTOTYPES[NAMES[0]][0] is _lib.c_int64
    assert [p for _, p in _lib.PROTOTYPES[NAMES[1]][1]] == [
        "m", "d_settings", "ld_s", "n_settings", "d_particles", "ld_p", "n_dims", "n_particles", "d_weights", "h_rows",
        "n_rows", "d_mean", "d_ycov", "d_xcov", "d_pvar", "d_ws", "ws_bytes", "stream"]
    assert [p for _, p in _lib.PROTOTYPES[NAMES[2]][1]] == [
        "d_ycov", "d_xcov", "n_rows", "n_channels", "n_settings", "d_noise_var", "ld_noise", "d_pvar", "h_weights",
        "d_cost", "cost", "d_gain", "d_utility", "accumulate", "stream"]
    assert lib.cdll.obe_abi_version() == 3


def test_workspace_size_covers_both_passes(lib):
    size = lib.cdll.obe_output_covariance_workspace_bytes
    assert size(1, 1, 1, 1) > 0
    g = np.random.default_rng(9)
    for _ in range(2000):
        n, s = int(g.integers(1, 1 << 22)), int(g.integers(1, 1 << 17))
        c, r = int(g.integers(1, 9)), int(g.integers(1, 9))
        tiles = (s + 63) // 64
        chunks = max(1, min((n + 255) // 256, max(1, 8192 // tiles)))
        slots = max(c, c * (c + 1) // 2 + r * c)
        assert size(n, s, c, r) >= chunks * tiles * 64 * slots * 8
        assert size(n, s, c, min(r + 1, 8)) >= size(n, s, c, r)


def test_entry_points_refuse_bad_arguments_without_a_device(lib):
    dev = 1 << 20                    # (never dereferenced: every call below is refused by its argument checks)
    c = lib.cdll
    m = models.lorentzian(1).struct(3, (0.1,))
    n, s, big = 1000, 10, 1 << 30
    rows = np.array([2, 0], dtype=np.int32)
    a = np.array([1.0, 2.0])

    def refused(rc, word):
        assert rc == -1 and word in lib.last_error(), (rc, lib.last_error())

    def cov(**kw):
        args = dict(m=m, d_settings=dev, ld_s=s, n_settings=s, d_particles=dev, ld_p=n, n_dims=3, n_particles=n,
                    d_weights=dev, h_rows=_lib.host_ptr(rows), n_rows=2, d_mean=dev, d_ycov=dev, d_xcov=dev, d_pvar=dev,
                    d_ws=dev, ws_bytes=big, stream=None)
        args.update(kw)
        return c.obe_output_covariance(*args.values())

    def gain(**kw):
        args = dict(d_ycov=dev, d_xcov=dev, n_rows=2, n_channels=1, n_settings=s, d_noise_var=dev, ld_noise=0, d_pvar=dev,
                    h_weights=_lib.host_ptr(a), d_cost=None, cost=1.0, d_gain=dev, d_utility=dev, accumulate=0,
                    stream=None)
        args.update(kw)
        return c.obe_variance_reduction(*args.values())

    for name in ("m", "d_settings", "d_particles", "d_weights", "h_rows", "d_mean", "d_xcov", "d_pvar", "d_ws"):
        refused(cov(**{name: None}), "null pointer")
    for bad in (0, 9, -1):
        refused(cov(n_rows=bad), "rows per call")
    for bad in ([3, 0], [0, -1]):
        refused(cov(h_rows=_lib.host_ptr(np.array(bad, dtype=np.int32))), "row index out of range")
    refused(cov(n_dims=2), "row index out of range")
    refused(cov(n_dims=4, h_rows=_lib.host_ptr(np.array([3, 0], dtype=np.int32))), "beyond the model's parameter rows")
    refused(cov(n_settings=0), "n_settings < 1")
    refused(cov(ld_s=s - 1), "n_settings")
    refused(cov(n_particles=0), "cloud size")
    refused(cov(ld_p=n - 1), "cloud size")
    refused(cov(ws_bytes=c.obe_output_covariance_workspace_bytes(n, s, 1, 2) - 1), "workspace too small")
    bad = models.lorentzian(1).struct(3, (0.1,))
    bad.aux = 9
    refused(cov(m=bad), "aux")

    for name in ("d_ycov", "d_xcov", "d_noise_var"):
        refused(gain(**{name: None}), "null pointer")
    refused(gain(d_pvar=None), "null pointer")                  # the utility divides by it
    for bad in (0, 9):
        refused(gain(n_rows=bad), "rows per call")
    for bad in (0, 9):
        refused(gain(n_channels=bad), "channels")
    refused(gain(n_settings=0), "n_settings < 1")
    refused(gain(ld_noise=s - 1), "noise variance")
    assert gain(d_gain=None, d_utility=None) == 0               # nothing asked for: nothing launched
