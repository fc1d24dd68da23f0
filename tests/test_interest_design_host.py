"""Design of a batch of measurements for parameters of interest, everything that needs no GPU: the argument forms of
opt_setting_batch(interest=, interest_weights=) and their refusals, the oracle of tests/_interest_design_oracle.py
against its own independent direct solve, the declaration and the refusals of obe_design_interest_step.  What needs a
constructed object is in tests/test_gpu_interest_design.py."""
import types

import numpy as np
import pytest

import _interest_design_oracle as oracle
from optbayesexpt_amd import _design, _lib, build

NAME = "obe_design_interest_step"


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _fake(**kw):
    args = dict(_device_model=object(), allsettings=np.zeros((1, 5)), n_channels=2, n_dims=3, _n_settings=5,
                yvar_noise_model=lambda: np.array([1.0, 2.0]), last_batch_design=None,
                parameters_of_interest=((2, 0), np.array([0.5, 4.0])))
    args.update(kw)
    return types.SimpleNamespace(**args)


# ------------------------------------------------------------------------------------------ argument checks
def test_forms_of_interest_and_its_weights():
    fake = _fake()
    check = _design.check_interest
    assert check(fake, None, None) is None and check(fake, False, None) is None and check(fake, np.bool_(False), None) is None
    rows, a = check(fake, True, None)                          # the object's own choice
    assert rows == (2, 0) and a.tolist() == [0.5, 4.0]
    rows, a = check(fake, np.bool_(True), [1, 0])              # ... with weights for this call only
    assert rows == (2, 0) and a.tolist() == [1.0, 0.0] and fake.parameters_of_interest[1].tolist() == [0.5, 4.0]
    rows, a = check(fake, 1, None)                             # an int is a row, True is not row 1
    assert rows == (1,) and a.tolist() == [1.0]
    rows, a = check(fake, np.int64(0), 3.0)
    assert rows == (0,) and a.tolist() == [3.0]
    rows, a = check(fake, [2, 1], (0.25, 2))
    assert rows == (2, 1) and a.tolist() == [0.25, 2.0] and a.dtype == np.float64
    rows, a = check(fake, (0, 1, 2), None)
    assert rows == (0, 1, 2) and a.tolist() == [1.0, 1.0, 1.0]


@pytest.mark.parametrize("interest,weights,word", [
    ([True], None, "integer row indices"),                     # a bool row
    ([0, True], None, "integer row indices"),
    ([1, 1], None, "twice"),                                   # a repeated row
    (3, None, "outside"),                                      # a row outside the cloud
    ([0, -1], None, "outside"),
    ([], None, "at least one"),
    (1.0, None, "row ind"),
    (None, [1.0], "pass interest"),                            # weights without interest
    (False, [1.0], "pass interest"),
    ([0, 1], [1.0], "2 parameter"),                            # the wrong length
    (True, [1.0, 2.0, 3.0], "2 parameter"),
    ([0, 1], [1.0, -1.0], ">= 0"),
    ([0, 1], [1.0, np.nan], "finite"),
    ([0, 1], [0.0, 0.0], "not all be zero"),
    (0, "a", "numbers"),
])
def test_refusals_of_interest_and_its_weights(interest, weights, word):
    from optbayesexpt_amd import OptBayesExpt
    fake = _fake()
    with pytest.raises(ValueError, match=word):
        _design.check_interest(fake, interest, weights)
    with pytest.raises(ValueError, match=word):                # ... and from the method, before any library call
        OptBayesExpt.opt_setting_batch(fake, 2, interest=interest, interest_weights=weights)
    assert fake.last_batch_design is None


def test_the_method_checks_n_and_the_noise_with_interest_as_without():
    from optbayesexpt_amd import OptBayesExpt, OptBayesExptNoiseParameter, OptBayesExptSweeper
    assert OptBayesExptNoiseParameter.opt_setting_batch is OptBayesExpt.opt_setting_batch
    calls = [lambda f: OptBayesExpt.opt_setting_batch(f, 0, interest=0),
             lambda f: OptBayesExpt.opt_setting_batch(f, 2.0, interest=True),
             lambda f: OptBayesExpt.opt_setting_batch(f, 65, interest=[0, 1]),                  # 130 scalar readings
             lambda f: OptBayesExpt.opt_setting_batch(f, 2, sigma=-1.0, interest=0),
             lambda f: OptBayesExpt.opt_setting_batch(f, 2, sigma=np.inf, interest=0),
             lambda f: OptBayesExpt.opt_setting_batch(f, 2, sigma=np.ones((2, 3)), interest=0)]
    for call in calls:
        fake = _fake()
        with pytest.raises(ValueError):
            call(fake)
        assert fake.last_batch_design is None
    zero = _fake(yvar_noise_model=lambda: np.array([1.0, 0.0]))        # the model's noise is 0 in a channel
    with pytest.raises(ValueError, match="finite and > 0"):
        OptBayesExpt.opt_setting_batch(zero, 2, interest=0)
    host = _fake(_device_model=None)
    with pytest.raises(TypeError, match="from_function.*from_expression"):
        OptBayesExpt.opt_setting_batch(host, 2, interest=0)
    for kw in (dict(interest=0), dict(interest=True, interest_weights=[1.0]), dict(interest_weights=[1.0])):
        with pytest.raises(TypeError, match="intervals"):
            OptBayesExptSweeper.opt_setting_batch(types.SimpleNamespace(), 2, **kw)


# ------------------------------------------------------------------------------------------------ the oracle
def _cloud(g, n_x, n_c, n_sel, n):
    """(y (n_x, C, N), theta (R, N), w): rows that depend on every parameter row, smoothly and not linearly."""
    theta = g.normal(size=(n_sel, n)) * np.linspace(1.0, 2.0, n_sel)[:, None]
    theta[0] += 0.4 * theta[-1]
    x = np.linspace(-1.0, 2.0, n_x)
    y = np.empty((n_x, n_c, n))
    for s, xs in enumerate(x):
        for c in range(n_c):
            lin = sum(theta[k] * np.cos((k + 1) * xs + 0.7 * c) for k in range(n_sel))
            y[s, c] = lin + 0.3 * np.sin(xs * theta[0] + c) + (c + 1.0) * xs
    return y, theta, g.random(n)


@pytest.mark.parametrize("n_c", [1, 2])
@pytest.mark.parametrize("n_sel", [1, 2, 9])
def test_recurrence_is_the_direct_solve_by_the_gain_route_and_by_the_t_route(n_c, n_sel):
    g = np.random.default_rng([6, n_c, n_sel])
    n_x, n = 31, 400
    y, theta, w = _cloud(g, n_x, n_c, n_sel, n)
    joint = oracle.Joint(y, theta, w)
    assert joint.S.shape == (n_c, n_c, n_x) and joint.K.shape == (n_sel, n_c, n_x) and joint.V.shape == (n_sel,)
    # the blocks are NumPy's weighted covariance of (theta, y)
    full = np.cov(np.vstack([theta, y.reshape(n_x * n_c, n)]), aweights=w, ddof=0)
    np.testing.assert_allclose(joint.V, np.diagonal(full)[:n_sel], rtol=1e-12)
    np.testing.assert_allclose(joint.K, np.transpose(full[:n_sel, n_sel:].reshape(n_sel, n_x, n_c), (0, 2, 1)), rtol=1e-11,
                               atol=1e-14)
    np.testing.assert_allclose(joint.S[:, :, 3], full[n_sel + 3 * n_c:n_sel + 4 * n_c, n_sel + 3 * n_c:n_sel + 4 * n_c],
                               rtol=1e-12)
    # the noise is of the size of the variance: a second reading of a good setting beats a first one of a poor setting
    nu = np.mean(np.einsum("ccs->cs", joint.S)) * 0.5 * (1.0 + g.random((n_c, n_x)))
    a = 0.5 + g.random(n_sel)
    cost = 1.0 + 0.5 * g.random(n_x)
    n_picks = 6
    des = oracle.greedy(joint, nu, a, cost, n_picks)
    picks = des["indices"]
    assert np.all(picks >= 0)
    scale = np.max(joint.V)
    # a setting read twice (two readings, two sets of rows), whether or not the greedy rule asks for it
    forced = [5, 20, 5, 11]
    state = oracle.start(joint.S, joint.K, joint.V)
    for j, p in enumerate(forced):
        state = oracle.condition(state, joint.cov.row(p), p, nu)
        left, cond, _, _ = oracle.direct(joint, nu, forced[:j + 1])
        assert cond < 1e3
        np.testing.assert_allclose(state["left"], left, rtol=0, atol=1e-12 * scale)
        G = oracle.gains(state["S"], state["K"], nu)[0]
        for x in (5, 11, 30):
            np.testing.assert_allclose(G[:, x], oracle.direct_gain(joint, nu, forced[:j + 1], x), rtol=0, atol=1e-12 * scale)
    for j in range(n_picks):
        left, cond, _, _ = oracle.direct(joint, nu, picks[:j])
        assert cond < 1e3
        np.testing.assert_allclose(des["left_T"][j], left, rtol=0, atol=1e-12 * scale)       # the T route
        if j:
            np.testing.assert_allclose(des["variance_left"][j - 1], left, rtol=0, atol=1e-12 * scale)      # the gain route
        # every gain the pick was made from is what one more reading there removes, by a solve of its own
        for x in (0, int(picks[j]), n_x - 1):
            np.testing.assert_allclose(des["G"][j][:, x], oracle.direct_gain(joint, nu, picks[:j], x), rtol=0,
                                       atol=1e-12 * scale)
        np.testing.assert_allclose(des["U"][j], oracle.utility(des["G"][j], joint.V, a, cost), rtol=1e-14)
        assert picks[j] == int(np.argmax(des["U"][j])) and des["utility"][j] == des["U"][j][picks[j]]
    np.testing.assert_allclose(des["variance_left"][-1], oracle.direct(joint, nu, picks)[0], rtol=0, atol=1e-12 * scale)
    # the gain that chose a pick is what its C rows of T remove
    T = np.array(des["state"]["T"]).reshape(n_picks - 1, n_c, n_sel)
    for j in range(n_picks - 1):
        np.testing.assert_allclose(des["G"][j][:, picks[j]], np.sum(T[j] ** 2, axis=0), rtol=0, atol=1e-12 * scale)
    # the variance left never rises, stays >= 0, and the conditioned S stays symmetric
    assert np.all(np.diff(np.vstack([joint.V, des["variance_left"]]), axis=0) <= 0) and np.all(des["variance_left"] >= 0)
    np.testing.assert_array_equal(des["state"]["S"], np.swapaxes(des["state"]["S"], 0, 1))
    # pick 0 is the single-reading design's arg-max
    G0, _, cond0 = oracle.gains(joint.S, joint.K, nu)
    assert picks[0] == int(np.argmax(oracle.utility(G0, joint.V, a, cost)))


def test_distinct_zero_variance_rows_and_a_poisoned_reading():
    g = np.random.default_rng(7)
    y, theta, w = _cloud(g, 9, 1, 2, 300)
    theta[1] = 2.5                                             # V_1 == 0: the row contributes nothing, whatever its weight
    joint = oracle.Joint(y, theta, w)
    assert joint.V[1] == 0.0
    nu = np.full((1, 9), np.mean(joint.S))
    both = oracle.greedy(joint, nu, [1.0, 7.0], 1.0, 9, distinct=True)
    alone = oracle.greedy(oracle.Joint(y, theta[:1], w), nu, [1.0], 1.0, 9, distinct=True)
    assert sorted(both["indices"].tolist()) == list(range(9))
    np.testing.assert_array_equal(both["indices"], alone["indices"])
    np.testing.assert_allclose(both["utility"], alone["utility"], rtol=1e-14)      # (a solve with one more right-hand side)
    # one more distinct pick than there are settings: none is left
    assert oracle.greedy(joint, nu, [1.0, 7.0], 1.0, 10, distinct=True)["indices"][9] == -1
    # a g that is not > 0 makes everything NaN
    bad = nu.copy()
    bad[0, 4] = -1e9
    state = oracle.condition(oracle.start(joint.S, joint.K, joint.V), joint.cov.row(4), 4, bad)
    assert np.all(np.isnan(state["S"])) and np.all(np.isnan(state["K"])) and np.all(np.isnan(state["left"]))
    # the tolerances have the stated form and scale
    state = oracle.greedy(joint, nu, [1.0, 7.0], 1.0, 4)["state"]
    tol_S, tol_K, tol_left, tol_T = oracle.recurrence_tolerance(state)
    assert tol_S.shape == (1, 1, 9) and tol_K.shape == (2, 1, 9) and tol_left.shape == (2,) and len(tol_T) == 3
    assert np.all(tol_S >= 1e-10 * np.abs(joint.S)) and np.all(tol_S < 1e-9 * np.max(joint.S))
    tol = oracle.end_to_end_tolerance(joint, nu, [4, 2, 4], state["terms_left"])
    assert tol.shape == (2,) and 0 < tol[0] < 1e-8 * joint.V[0]


# ------------------------------------------------------------------------------------------ the entry point
PARAMS = ["d_cross", "pivot_index", "d_factors", "d_tstore", "rows_done", "max_rows", "d_ycov", "d_xcov", "n_sel",
          "n_channels", "n_settings", "d_noise_var", "ld_noise", "d_pvar", "d_pvar_left", "h_weights", "d_cost", "cost",
          "d_taken", "d_gain", "d_utility", "d_best", "stream"]


def test_symbol_is_declared_exported_and_bound(lib):
    assert NAME in _lib.declared_symbols() and NAME in _lib.PROTOTYPES
    fn = getattr(lib.cdll, NAME)
    restype, params = _lib.PROTOTYPES[NAME]
    assert fn.restype is restype is _lib.c_int and len(fn.argtypes) == len(params) == len(PARAMS) == 23
    assert [p for _, p in params] == PARAMS
    # model-independent: the library serves it, no plugin does
    assert NAME not in _lib.MODEL_ENTRY_POINTS and "obe_design.hip" not in build.PLUGIN_SOURCES
    # its only host parameter is an input: nothing for the delivery audit
    from optbayesexpt_amd import _audit
    assert [p for p in PARAMS if p.startswith("h_")] == ["h_weights"] and NAME not in _audit._Audit().rules
    # additive: the ABI version stays
    assert _lib.OBE_ABI_VERSION == 3 and lib.cdll.obe_abi_version() == 3


def test_entry_point_refuses_bad_arguments_without_a_device(lib):
    dev = 1 << 20                    # (never dereferenced: every call below is refused by its argument checks)
    s = 10
    a = np.ones(3)

    def refused(rc, word):
        assert rc == -1 and NAME in lib.last_error() and word in lib.last_error(), (rc, lib.last_error())

    def step(**kw):
        args = dict(d_cross=dev, pivot_index=3, d_factors=dev, d_tstore=dev, rows_done=2, max_rows=4, d_ycov=dev, d_xcov=dev,
                    n_sel=3, n_channels=2, n_settings=s, d_noise_var=dev, ld_noise=0, d_pvar=dev, d_pvar_left=dev,
                    h_weights=_lib.host_ptr(a), d_cost=None, cost=1.0, d_taken=None, d_gain=dev, d_utility=dev, d_best=dev,
                    stream=None)
        assert list(args) == PARAMS
        args.update(kw)
        return lib.cdll.obe_design_interest_step(*args.values())

    for name in ("d_ycov", "d_xcov", "d_noise_var", "d_pvar", "d_gain", "d_utility", "d_best", "d_factors", "d_tstore",
                 "d_pvar_left"):
        refused(step(**{name: None}), "null pointer")
    for bad in (0, 9, -1):
        refused(step(n_channels=bad), "channels")
    for bad in (0, 33, -1):
        refused(step(n_sel=bad), "rows of interest")
    refused(step(n_settings=0), "n_settings < 1")
    refused(step(ld_noise=s - 1), "noise variance")
    for bad in (-1, s):
        refused(step(pivot_index=bad), "pivot index")
    refused(step(rows_done=3), "no room")
    refused(step(rows_done=-1), "no room")
    refused(step(max_rows=3), "no room")
    refused(step(n_settings=(1 << 39) + 1, pivot_index=0), "too many settings")
    refused(step(d_cross=None, n_settings=(1 << 39) + 1), "too many settings")
