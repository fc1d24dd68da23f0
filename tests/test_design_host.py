"""Design of a batch of measurements, everything that needs no GPU: the oracle of tests/_design_oracle.py pinned against
NumPy, a closed form and its own independent direct solve; the argument checks of optbayesexpt_amd/_design.py; the entry
points' declarations and refusals.  What needs a constructed object is in tests/test_gpu_design.py."""
import types

import numpy as np
import pytest

import _design_oracle as oracle
from optbayesexpt_amd import _design, _lib, build, models

NAMES = ("obe_output_cross_covariance_workspace_bytes", "obe_output_cross_covariance", "obe_design_step")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _cloud_rows(g, n_x, n_c, n):
    """y (n_x, C, N): smooth correlated rows, as a model over a cloud gives them."""
    theta = g.normal(size=(3, n))
    x = np.linspace(-1.0, 2.0, n_x)
    rows = [np.stack([theta[0] + (c + 1.0) * theta[1] * xs + np.sin(xs * theta[2] + c) for c in range(n_c)]) for xs in x]
    return np.stack(rows)


# ------------------------------------------------------------------------------------------------ the oracle
def test_blocks_are_numpys_weighted_covariance():
    g = np.random.default_rng(1)
    y = _cloud_rows(g, 5, 2, 400)
    w = g.random(400)
    b = oracle.cross_blocks(y[[3, 0]], y, w)
    assert b["X"].shape == (2, 2, 2, 5)
    flat = y.reshape(10, 400)
    cov = np.cov(flat, aweights=w, ddof=0).reshape(5, 2, 5, 2)
    for j, p in enumerate((3, 0)):
        np.testing.assert_allclose(b["X"][j], np.transpose(cov[p], (0, 2, 1)), rtol=1e-12, atol=1e-14)
    joint = oracle.Cov(y, w)
    np.testing.assert_allclose(joint.dense(), cov, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(joint.S(), np.diagonal(cov.reshape(10, 10)).reshape(5, 2).T, rtol=1e-12)
    assert np.all(joint.tol_row(2) > 0) and np.all(joint.tol_row(2) < 1e-9 * np.max(np.abs(cov)))
    for p in range(5):                                       # (the diagonal's tolerance is the block's own there)
        np.testing.assert_allclose(joint.tol_S()[:, p], np.diagonal(joint.tol_row(p)[:, :, p]), rtol=1e-12)
    # B_X bounds |X|; the tolerance has the stated form
    assert np.all(b["B_X"] >= np.abs(b["X"]))
    np.testing.assert_array_equal(oracle.cross_tolerance(b),
                                  1e-10 * b["B_X"] + 1e-20 * np.einsum("jd,sc->jdcs", b["A_p"], b["A"]))


def test_blocks_leave_out_what_has_no_weight():
    g = np.random.default_rng(2)
    y = _cloud_rows(g, 4, 1, 50)
    w = g.random(50)
    w[:5] = [0.0, np.nan, -1.0, 0.0, -0.0]
    want = oracle.cross_blocks(y[:2, :, 5:], y[:, :, 5:], w[5:])
    y2 = y.copy()
    y2[:, :, :5] = [np.inf, np.nan, -np.inf, 1e300, np.nan]
    got = oracle.cross_blocks(y2[:2], y2, w)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k])


def test_blocks_of_a_line_are_the_closed_form():
    """y = a + b x: X(p, x) = V_a + (x + p) C_ab + x p V_b."""
    g = np.random.default_rng(3)
    n = 2000
    a, b = g.normal(2.0, 0.5, n), g.normal(-1.0, 0.2, n)
    a = a + 0.4 * b
    w = g.random(n)
    x = np.linspace(-2.0, 3.0, 9)
    y = (a[None, :] + b[None, :] * x[:, None])[:, None, :]
    cov = np.cov(np.array([a, b]), aweights=w, ddof=0)
    blocks = oracle.cross_blocks(y[[1, 7]], y, w)
    for j, p in enumerate((x[1], x[7])):
        want = cov[0, 0] + (x + p) * cov[0, 1] + x * p * cov[1, 1]
        np.testing.assert_allclose(blocks["X"][j, 0, 0], want, rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("n_c", [1, 2])
@pytest.mark.parametrize("distinct", [False, True])
def test_recurrence_is_the_direct_solve_and_the_log_determinant(n_c, distinct):
    g = np.random.default_rng([4, n_c])
    n_x = 37
    y = _cloud_rows(g, n_x, n_c, 300)
    w = g.random(300)
    K = oracle.Cov(y, w)
    S = K.S()
    # per-setting noise and cost; the noise is of the size of the variance, so that a second reading of a good setting
    # is worth more than a first one of a poor setting
    nu = np.mean(S) * 0.5 * (1.0 + g.random((n_c, n_x)))
    cost = 1.0 + 0.5 * g.random(n_x)
    des = oracle.greedy(K, nu, cost, 6, distinct=distinct)
    picks = des["indices"]
    assert np.all(picks >= 0)
    assert (len(set(picks.tolist())) == 6) == distinct, picks       # without `distinct` one setting is picked twice
    for j in range(7):
        v, info, cond, _, _ = oracle.direct(K, nu, picks[:j])
        assert cond < 1e4
        if j < 6:
            np.testing.assert_allclose(des["v"][j], v, rtol=0, atol=1e-13 * np.max(S))
            np.testing.assert_allclose(des["U"][j], oracle.utility(v, nu, cost), rtol=1e-12)
        else:
            np.testing.assert_allclose(des["state"]["v"], v, rtol=0, atol=1e-13 * np.max(S))
        if j:
            np.testing.assert_allclose(des["information"][j - 1], info, rtol=1e-13, atol=1e-14)
    assert np.all(np.diff(des["information"]) > 0)
    # pick 0 is the variance utility's arg-max
    assert picks[0] == int(np.argmax(np.sum(S / nu, axis=0) / cost))
    # the conditional variance never rises and stays >= 0
    assert np.all(des["state"]["v"] <= S + 1e-15) and np.all(des["state"]["v"] > -1e-12 * np.max(S))


class _Moved:
    """A joint covariance K (n_x, C, n_x, C) given outright, with the interface direct() reads of a Cov."""

    def __init__(self, dense):
        self.dense, (self.n_x, self.n_c) = dense, dense.shape[:2]

    def row(self, p):
        return np.transpose(self.dense[int(p)], (0, 2, 1))

    def S(self):
        n = self.n_x * self.n_c
        return np.diagonal(self.dense.reshape(n, n)).reshape(self.n_x, self.n_c).T.copy()


@pytest.mark.parametrize("n_c", [1, 2])
def test_end_to_end_tolerance_covers_every_entry_moved_by_its_block_tolerance(n_c):
    """The direct solve on a joint covariance whose every entry is moved by up to its own tolerance (symmetrically)
    stays within end_to_end_tolerance of the direct solve on the unmoved one; the tolerance stays at the 1e-10 scale."""
    g = np.random.default_rng([5, n_c])
    n_x = 23
    y = _cloud_rows(g, n_x, n_c, 300)
    w = g.random(300)
    K = oracle.Cov(y, w)
    S = K.S()
    nu = np.mean(S) * 0.5 * (1.0 + g.random((n_c, n_x)))
    cost = 1.0 + 0.5 * g.random(n_x)
    picks = oracle.greedy(K, nu, cost, 5)["indices"]
    assert len(set(picks.tolist())) < 5                              # (a setting read twice is two rows of A)
    tol = np.stack([np.transpose(K.tol_row(p), (0, 2, 1)) for p in range(n_x)])
    e = g.uniform(-1.0, 1.0, (n_x * n_c, n_x * n_c))
    moved = _Moved(K.dense() + (0.5 * (e + e.T)).reshape(tol.shape) * tol)
    for j in (0, 1, 3, 5):
        state = oracle.greedy(K, nu, cost, j)["state"] if j else oracle.start(S)
        tol_v, tol_info = oracle.end_to_end_tolerance(K, nu, picks[:j], state)
        assert tol_v.shape == (n_c, n_x) and np.all(tol_v > 0) and np.all(tol_v < 1e-8 * np.max(S))
        assert 0 < tol_info < 1e-8
        v0, info0 = oracle.direct(K, nu, picks[:j])[:2]
        v1, info1 = oracle.direct(moved, nu, picks[:j])[:2]
        assert np.all(np.abs(v1 - v0) <= tol_v) and abs(info1 - info0) <= tol_info


def test_arg_max_rules():
    u = np.array([1.0, np.nan, 3.0, 3.0, np.inf, -np.inf])
    assert oracle.first_finite_maximum(u) == 2
    assert oracle.first_finite_maximum(u, taken=[0, 0, 1, 0, 0, 0]) == 3
    assert oracle.first_finite_maximum(u, taken=[0, 0, 1, 1, 0, 0]) == 0
    assert oracle.first_finite_maximum(np.array([np.nan, np.nan])) == -1
    assert oracle.first_finite_maximum(np.array([2.0]), taken=[1]) == -1
    assert oracle.margin(np.array([1.0, 2.0, np.nan])) == 0.5 and oracle.margin(np.array([1.0])) == np.inf


def test_a_reading_without_positive_finite_g_poisons_its_row_and_what_follows():
    nu = np.array([[-3.0, 1.0]])                               # (the product refuses such a noise; the kernel does not)
    state = oracle.start([[1.0, 2.0]])
    state = oracle.condition(state, np.array([[[1.0, 0.5]]]), 0, nu)
    assert np.all(np.isnan(state["v"])) and np.isnan(state["info"])


# ------------------------------------------------------------------------------------------ argument checks
def test_n_and_noise_checks():
    assert _design.check_n(1, 1) == 1 and _design.check_n(np.int64(128), 1) == 128 and _design.check_n(64, 2) == 64
    for bad in (0, -1, 1.0, True, "3", None):
        with pytest.raises(ValueError):
            _design.check_n(bad, 1)
    with pytest.raises(ValueError, match="128"):
        _design.check_n(129, 1)
    with pytest.raises(ValueError, match="128"):
        _design.check_n(65, 2)
    assert _design.check_noise_variance(np.array([[1.0], [2.0]])).shape == (2, 1)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="finite and > 0"):
            _design.check_noise_variance(np.array([[1.0, bad]]))
    assert [_design.pivots_per_call(c) for c in range(1, 9)] == [8, 4, 2, 2, 1, 1, 1, 1]
    assert _design.check_points(([1.0, 2.0, 3.0],), 1).shape == (1, 3)
    for bad in ((1.0, 2.0), ([],), np.zeros((1, 2, 2))):
        with pytest.raises(ValueError):
            _design.check_points(bad, 1)


def test_methods_check_their_arguments_before_any_library_call():
    from optbayesexpt_amd import OptBayesExpt, OptBayesExptNoiseParameter, OptBayesExptSweeper
    assert OptBayesExptNoiseParameter.opt_setting_batch is OptBayesExpt.opt_setting_batch
    assert OptBayesExptSweeper.output_cross_covariance is OptBayesExpt.output_cross_covariance
    fake = types.SimpleNamespace(_device_model=object(), allsettings=np.zeros((1, 5)), n_channels=2, n_dims=3,
                                 _n_settings=5, yvar_noise_model=lambda: np.array([1.0, 0.0]), last_batch_design=None)
    calls = [lambda: OptBayesExpt.opt_setting_batch(fake, 0),
             lambda: OptBayesExpt.opt_setting_batch(fake, 2.0),
             lambda: OptBayesExpt.opt_setting_batch(fake, 65),                     # 130 scalar readings
             lambda: OptBayesExpt.opt_setting_batch(fake, 2),                      # the model's noise is 0 in a channel
             lambda: OptBayesExpt.opt_setting_batch(fake, 2, sigma=-1.0),
             lambda: OptBayesExpt.opt_setting_batch(fake, 2, sigma=np.ones((2, 3))),
             lambda: OptBayesExpt.output_cross_covariance(fake, (1.0, 2.0)),
             lambda: OptBayesExpt.output_cross_covariance(fake, ([],))]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    assert fake.last_batch_design is None
    host = types.SimpleNamespace(_device_model=None, n_channels=1, _n_settings=5, allsettings=np.zeros((1, 5)),
                                 yvar_noise_model=lambda: 1.0)
    for call in (lambda: OptBayesExpt.opt_setting_batch(host, 2), lambda: OptBayesExpt.output_cross_covariance(host, (1.0,))):
        with pytest.raises(TypeError, match="from_function.*from_expression"):
            call()
    with pytest.raises(TypeError, match="intervals"):
        OptBayesExptSweeper.opt_setting_batch(types.SimpleNamespace(), 2)


# ------------------------------------------------------------------------------------------ the entry points
def test_symbols_are_declared_exported_and_bound(lib):
    for name in NAMES:
        assert name in _lib.declared_symbols() and name in _lib.PROTOTYPES
        fn = getattr(lib.cdll, name)
        restype, params = _lib.PROTOTYPES[name]
        assert fn.restype is restype and len(fn.argtypes) == len(params)
    # the blocks depend on the model (every plugin brings them), the step does not
    assert set(NAMES[:2]) <= set(_lib.MODEL_ENTRY_POINTS) and NAMES[2] not in _lib.MODEL_ENTRY_POINTS
    assert "obe_predict.hip" in build.PLUGIN_SOURCES and "obe_design.hip" not in build.PLUGIN_SOURCES
    assert _lib.PROTOTYPES[NAMES[0]][0] is _lib.c_int64
    assert [p for _, p in _lib.PROTOTYPES[NAMES[1]][1]] == [
        "m", "d_settings", "ld_s", "n_settings", "d_pivots", "ld_pivots", "n_pivots", "d_particles", "ld_p", "n_particles",
        "d_weights", "d_mean", "mean_given", "d_cross", "d_ws", "ws_bytes", "stream"]
    assert [p for _, p in _lib.PROTOTYPES[NAMES[2]][1]] == [
        "d_cross", "pivot_index", "d_factors", "rows_done", "max_rows", "d_cvar", "n_channels", "n_settings", "d_noise_var",
        "ld_noise", "d_cost", "cost", "d_taken", "d_utility", "d_best", "d_info", "stream"]
    # no host result: nothing for the delivery audit
    for name in NAMES:
        assert not any(p.startswith("h_") for _, p in _lib.PROTOTYPES[name][1])
    assert _lib.OBE_ABI_VERSION == 3 and lib.cdll.obe_abi_version() == 3


def test_workspace_size_covers_every_pass_and_never_shrinks(lib):
    size = lib.cdll.obe_output_cross_covariance_workspace_bytes
    assert size(1, 1, 1, 1) > 0
    g = np.random.default_rng(9)
    for _ in range(2000):
        n, s = int(g.integers(1, 1 << 22)), int(g.integers(1, 1 << 17))
        c = int(g.integers(1, 9))
        j = int(g.integers(1, 8 // c + 1))
        tiles = (s + 63) // 64
        chunks = max(1, min((n + 255) // 256, max(1, 8192 // tiles)))
        pivot_chunks = max(1, min((n + 255) // 256, 8192))
        words = n * 8 + max(chunks * tiles * 64 * j * c * c, pivot_chunks * 64 * c)
        assert size(n, s, c, j) >= words * 8
        assert size(n + 1, s, c, j) >= size(n, s, c, j) and size(n, s + 1, c, j) >= size(n, s, c, j)
        assert size(n, s, min(c + 1, 8), j) >= size(n, s, c, j) and size(n, s, c, j + 1) >= size(n, s, c, j)


def test_entry_points_refuse_bad_arguments_without_a_device(lib):
    dev = 1 << 20                    # (never dereferenced: every call below is refused by its argument checks)
    c = lib.cdll
    m = models.lorentzian(1).struct(3, (0.1,))
    n, s, big = 1000, 10, 1 << 30

    def refused(rc, word):
        assert rc == -1 and word in lib.last_error(), (rc, lib.last_error())

    def cross(**kw):
        args = dict(m=m, d_settings=dev, ld_s=s, n_settings=s, d_pivots=dev, ld_pivots=2, n_pivots=2, d_particles=dev,
                    ld_p=n, n_particles=n, d_weights=dev, d_mean=dev, mean_given=0, d_cross=dev, d_ws=dev, ws_bytes=big,
                    stream=None)
        args.update(kw)
        return c.obe_output_cross_covariance(*args.values())

    def step(**kw):
        args = dict(d_cross=dev, pivot_index=3, d_factors=dev, rows_done=2, max_rows=4, d_cvar=dev, n_channels=2,
                    n_settings=s, d_noise_var=dev, ld_noise=0, d_cost=None, cost=1.0, d_taken=None, d_utility=dev,
                    d_best=dev, d_info=dev, stream=None)
        args.update(kw)
        return c.obe_design_step(*args.values())

    for name in ("m", "d_settings", "d_pivots", "d_particles", "d_weights", "d_mean", "d_cross", "d_ws"):
        refused(cross(**{name: None}), "null pointer")
    for bad in (0, 9, -1):
        refused(cross(n_pivots=bad, ld_pivots=9), "rows (pivots x channels) per call")
    refused(cross(ld_pivots=1), "rows (pivots x channels) per call")
    coil = models.coil().struct(3, ())
    refused(cross(m=coil, n_pivots=5, ld_pivots=5), "rows (pivots x channels) per call")      # 10 rows
    refused(cross(n_settings=0), "n_settings < 1")
    refused(cross(ld_s=s - 1), "n_settings")
    refused(cross(n_particles=0), "cloud size")
    refused(cross(ld_p=n - 1), "cloud size")
    refused(cross(ws_bytes=c.obe_output_cross_covariance_workspace_bytes(n, s, 1, 2) - 1), "workspace too small")
    bad = models.lorentzian(1).struct(3, (0.1,))
    bad.aux = 9
    refused(cross(m=bad), "aux")

    for name in ("d_cvar", "d_noise_var", "d_utility", "d_best", "d_factors", "d_info"):
        refused(step(**{name: None}), "null pointer")
    for bad in (0, 9):
        refused(step(n_channels=bad), "channels")
    refused(step(n_settings=0), "n_settings < 1")
    refused(step(ld_noise=s - 1), "noise variance")
    for bad in (-1, s):
        refused(step(pivot_index=bad), "pivot index")
    refused(step(rows_done=3), "no room")
    refused(step(rows_done=-1), "no room")
