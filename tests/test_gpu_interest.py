"""Design for parameters of interest on the device (OptBayesExpt.output_covariance / expected_variance_reduction /
utility_parameter_variance; csrc/obe_predict.hip K12, csrc/obe_interest.hip) against the long double oracle of
tests/_interest_oracle.py on the rows y = eval_over_all_parameters((x_s,)) of the product itself.

The blocks are held to the conditioning form of the project's 1e-10 (|dS| <= 1e-10 B_S + 1e-20 A_c A_c', |dK| <= 1e-10 B_K
+ 1e-20 A_d A_c, |dV| <= 1e-10 V + 1e-20 A_d^2), the mean to predict()'s bits, the gains to 1e-10 sum_c |u_c| |k_c| on the
device's own blocks with cond(S + diag nu) <= 1e3 asserted on the inputs.  Shapes stay below the size at which the chunk
plan of a call depends on its number of settings (clouds <= 5000: at most 20 chunks, fewer than 8192 / setting tiles), so
requests of different lengths agree bit for bit.

Measured on an MI355X (test_worst_errors_are_reported prints them), worst error / tolerance: S 1.1e-5, K 1.1e-5, V 2.7e-6,
G on the device's blocks 1.4e-5, G end to end 6.4e-6, the line's closed form 1.2e-6, U 2.9e-6; DESIGN.md section 6."""
import copy
import warnings

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _interest_oracle as oracle
import _state_cases as cases
import test_gpu_predictive as tp
from optbayesexpt_amd import _interest, _predictive, _state

pytestmark = pytest.mark.gpu
WORST = {}
_bits = tp._bits


def _note(kind, err, tol, what):
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
    worst = float(np.max(ratio)) if np.size(ratio) else 0.0
    if worst >= WORST.get(kind, (0.0, ""))[0]:
        WORST[kind] = worst, what
    assert np.all(err <= tol), f"{what}: {kind}: worst error / tolerance {worst:.3g}"


def _nu_for(S, mean):
    """A noise variance per channel that keeps cond(S + diag nu) <= 101: nu = tr S / 100 — but no smaller than 1e-12 of
    the output's own scale (a degenerate cloud: S is rounding alone there), and 1 where that is zero too."""
    nu = max(float(np.trace(S)) / 100.0, 1e-12 * float(np.sum(np.square(mean))))
    return np.full(S.shape[0], nu if nu > 0 else 1.0)


def _check(what, o, x, y, w, dims=None, gains=True):
    """output_covariance() and expected_variance_reduction() at the points x against the oracle on y (n_x, C, N_p)."""
    rows = _interest.check_dims(dims, o.n_dims)
    mean, ycov, xcov = o.output_covariance(x, dims)
    n_x, n_c = y.shape[0], y.shape[1]
    assert mean.shape == (n_c, n_x) and ycov.shape == (n_c, n_c, n_x) and xcov.shape == (len(rows), n_c, n_x)
    assert_array_equal(_bits(mean), _bits(o.predict(x)[0]), err_msg=f"{what}: the mean is predict()'s")
    assert_array_equal(_bits(ycov), _bits(np.swapaxes(ycov, 0, 1)))
    pvar = _interest._blocks(o, None if x is None else x[:, :1], rows)[3].cpu().numpy()
    theta = np.array(o.particles)[list(rows)]
    finite = []
    want = []
    for s in range(n_x):
        b = oracle.blocks(y[s], theta, w)
        want.append(b)
        if not np.all(np.isfinite(b["m"])):
            # a weighted particle with a non-finite y: the setting's blocks are non-finite
            assert not np.any(np.isfinite(np.diagonal(ycov[:, :, s]))), (what, s)
            assert not np.any(np.isfinite(xcov[:, :, s])), (what, s)
            continue
        finite.append(s)
        tol_S, tol_K, tol_V = oracle.tolerances(b)
        _note("S", np.abs(ycov[:, :, s] - b["S"]), tol_S, f"{what}, setting {s}")
        _note("K", np.abs(xcov[:, :, s] - b["K"]), tol_K, f"{what}, setting {s}")
        if s == 0:
            _note("V", np.abs(pvar - b["V"]), tol_V, what)
    if not gains or not finite:
        return mean, ycov, xcov
    # the gains: nu per setting, chosen from the device's S
    nu = np.ones((n_c, n_x))
    for s in finite:
        nu[:, s] = _nu_for(ycov[:, :, s], mean[:, s])
    sigma = np.sqrt(nu)
    nu = sigma * sigma                                   # (what the product forms from sigma)
    G = o.expected_variance_reduction(x, dims, sigma=sigma)
    assert G.shape == (len(rows), n_x)
    for s in finite:
        g_dev, u, cond = oracle.gain(ycov[:, :, s], xcov[:, :, s], nu[:, s])
        assert cond <= 1e3, (what, s, cond)
        _note("G on the device's blocks", np.abs(G[:, s] - g_dev), oracle.gain_tolerance(xcov[:, :, s], u),
              f"{what}, setting {s}")
        b = want[s]
        g_ref, u_ref, _ = oracle.gain(b["S"], b["K"], nu[:, s])
        tol_S, tol_K, _ = oracle.tolerances(b)
        _note("G end to end", np.abs(G[:, s] - g_ref), oracle.gain_tolerance_end_to_end(b["K"], u_ref, tol_S, tol_K, nu[:, s]),
              f"{what}, setting {s}")
        assert np.all(G[:, s] >= 0.0)
    return mean, ycov, xcov


# ------------------------------------------------------------------------- 1. shapes: clouds x settings
@pytest.mark.parametrize("n_x", [1, 2, 65, 1000])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_shapes_lorentzian(hip, n, n_x):
    g = np.random.default_rng([n, n_x, 12])
    cloud = tp._prior("lorentz1", g, n)
    x = tp._points("lorentz1", g, n_x)
    for kind in ("dyadic", "general", "zeros"):
        w = tp._dyadic_weights(g, n) if kind == "dyadic" else tp._general_weights(g, cloud)
        if kind == "zeros" and n > 2:
            w[g.random(n) < 0.3] = 0.0
            w[-1] = np.nan
            w[0] = 0.25
        o = tp._object("lorentz1", cloud, w)
        _check(f"lorentz1 {n} x {n_x} {kind}", o, x, tp._rows(o, x), w)


def test_a_million_particles(hip):
    g = np.random.default_rng(tp.BIG)
    cloud = tp._prior("lorentz1", g, tp.BIG)
    x = tp._points("lorentz1", g, 3)
    w = tp._general_weights(g, cloud)
    o = tp._object("lorentz1", cloud, w)
    _check("lorentz1 BIG x 3", o, x, tp._rows(o, x), w)


@pytest.mark.parametrize("name", ["lorentz7", "coil", "rabi", "expression", "function"])
def test_models(hip, name):
    for n, n_x in ((5000, 65), (257, 2)):
        g = np.random.default_rng([sum(map(ord, name)), n, 12])
        cloud = tp._prior(name, g, n)
        x = tp._points(name, g, n_x)
        w = tp._general_weights(g, cloud)
        o = tp._object(name, cloud, w)
        assert (o._mlib is not o._lib) == (name in ("expression", "function"))       # plugins serve their own model
        y = tp._rows(o, x)
        mean, ycov, xcov = _check(f"{name} {n} x {n_x}", o, x, y, w)
        if name == "coil":
            assert ycov.shape[:2] == (2, 2) and np.any(ycov[0, 1] != 0.0)              # a real 2 x 2 solve
        if name == "lorentz7":
            assert xcov.shape[0] == 10                                                  # two tiles of rows


def test_zero_weight_particles_do_not_matter_whatever_they_hold(hip):
    g = np.random.default_rng(21)
    n = 5000
    cloud = tp._prior("expression", g, n)
    w = tp._dyadic_weights(g, n)
    w[:6] = 0.0
    plain = tp._object("expression", cloud, w)
    x = np.array([[1.0, -2.0, 0.0, 0.5]])                   # a pole at x = 0: every weighted particle gives +-inf there
    want = plain.output_covariance(x)
    want_g = plain.expected_variance_reduction(x[:, :2], sigma=1.0)
    cloud2 = cloud.copy()
    cloud2[0, :6] = [np.inf, -np.inf, np.nan, 0.0, 1e300, np.nan]
    cloud2[1, :6] = [np.nan, 1e308, np.inf, np.nan, -np.inf, 0.0]
    o = tp._object("expression", cloud2, w)
    y = tp._rows(o, x)
    assert not np.all(np.isfinite(y[0, 0, :6])) and np.all(np.isfinite(y[0, 0, 6:]))
    got = o.output_covariance(x)
    for a, b in zip(got, want):
        assert_array_equal(_bits(a), _bits(b))
    assert_array_equal(_bits(o.expected_variance_reduction(x[:, :2], sigma=1.0)), _bits(want_g))
    mean, ycov, xcov = _check("pole", o, x, y, w, gains=False)
    assert np.all(np.isfinite(ycov[:, :, [0, 1, 3]])) and not np.isfinite(ycov[0, 0, 2])
    G = o.expected_variance_reduction(x, sigma=1.0)
    assert np.all(np.isfinite(G[:, [0, 1, 3]])) and np.all(np.isnan(G[:, 2]))           # no pivot > 0 there


def test_noise_parameter_object_takes_its_noise_from_the_cloud(hip):
    o = cases.build("noise7")
    cases.run(o, "noise7", 0, 12)
    w = np.array(o.particle_weights)
    assert np.any(w == 0.0)                                          # the constraint zeroed some weights
    x = np.asarray(o.allsettings)[:, ::16]
    y = tp._rows(o, x)
    _check("noise7", o, x, y, w, dims=[3, 9, 0])
    nu = np.asarray(o.yvar_noise_model()).reshape(-1)
    G = o.expected_variance_reduction(x, dims=[3, 9])
    theta = np.array(o.particles)[[3, 9]]
    for s in range(x.shape[1]):
        b = oracle.blocks(y[s], theta, w)
        g_ref, u, cond = oracle.gain(b["S"], b["K"], nu)
        tol_S, tol_K, _ = oracle.tolerances(b)
        _note("G end to end", np.abs(G[:, s] - g_ref), oracle.gain_tolerance_end_to_end(b["K"], u, tol_S, tol_K, nu),
              f"noise7, setting {s}")


def test_gain_of_a_line_is_the_closed_form(hip):
    """a + b x is linear in its parameters: G_d = (Sigma J)_d^2 / (J Sigma J^T + nu), J = (1, x), with Sigma =
    covariance() (1 - sum w^2 / (sum w)^2), the population form of the reference's unbiased one.  Sigma's own entries are held to the project's 1e-10 of their conditioning, sum w |dt_i| |dt_j| <=
    sqrt(V_i V_j); that error, propagated to first order through the closed form, is added to the end-to-end bound."""
    import optbayesexpt_amd as obe
    g = np.random.default_rng(22)
    n = 5000
    cloud = np.array([g.normal(2.0, 0.5, n), g.normal(-1.0, 0.2, n)]) + 0.3 * g.normal(size=n)
    w = tp._general_weights(g, cloud)
    model = obe.models.from_expression("a + b * x", settings=("x",), parameters=("a", "b"))
    o = obe.OptBayesExpt(model, (np.linspace(-2.0, 3.0, 9),), cloud, (), scale=False)
    o.particle_weights = w
    x = np.asarray(o.allsettings)
    y = tp._rows(o, x)
    sigma = 0.2
    G = o.expected_variance_reduction(sigma=sigma)
    # covariance() is the reference's np.cov(aweights=w): ddof = 1, sum / (W - W2 / W); the blocks divide by W
    cov = np.asarray(o.covariance()) * (1.0 - np.sum(w * w) / np.sum(w) ** 2)
    sd = np.sqrt(np.diag(cov))
    for s in range(x.shape[1]):
        J = np.array([1.0, x[0, s]])
        q, p = cov @ J, J @ cov @ J + sigma * sigma
        want = q * q / p
        b = oracle.blocks(y[s], cloud, w)
        g_ref, u, _ = oracle.gain(b["S"], b["K"], [sigma * sigma])
        tol_S, tol_K, _ = oracle.tolerances(b)
        bound_q, bound_p = sd * (sd @ np.abs(J)), (sd @ np.abs(J)) ** 2
        tol = oracle.gain_tolerance_end_to_end(b["K"], u, tol_S, tol_K, [sigma * sigma]) \
            + 1e-10 * (2.0 * np.abs(q) * bound_q / p + want * bound_p / p)
        _note("G of a line against the closed form", np.abs(G[:, s] - want), tol, f"line, setting {s}")


# ------------------------------------------------------------------------------------ 2. indexing, bit for bit
def test_indexing_is_bit_for_bit(hip, monkeypatch):
    g = np.random.default_rng(31)
    for name in ("lorentz1", "coil", "lorentz7"):
        cloud = tp._prior(name, g, 640)
        o = tp._object(name, cloud, tp._general_weights(g, cloud))
        x = tp._points(name, g, 100)
        whole = o.output_covariance(x)
        gain = o.expected_variance_reduction(x, sigma=3.0)
        # rows in the order given
        pick = [2, 0] if name != "lorentz7" else [9, 2, 0]
        some = o.output_covariance(x, dims=pick)
        assert_array_equal(_bits(some[2]), _bits(whole[2][pick]))
        assert_array_equal(_bits(some[0]), _bits(whole[0]))
        assert_array_equal(_bits(some[1]), _bits(whole[1]))
        assert_array_equal(_bits(o.expected_variance_reduction(x, dims=pick, sigma=3.0)), _bits(gain[pick]))
        assert_array_equal(_bits(o.output_covariance(x, dims=2)[2]), _bits(whole[2][2:3]))
        # the first k columns are the request of the first k points
        for k in (1, 37, 64, 65):
            for a, b in zip(o.output_covariance(x[:, :k]), whole):
                assert_array_equal(_bits(a), _bits(b[..., :k]))
            assert_array_equal(_bits(o.expected_variance_reduction(x[:, :k], sigma=3.0)), _bits(gain[:, :k]))
        # two identical calls
        for a, b in zip(o.output_covariance(x), whole):
            assert_array_equal(_bits(a), _bits(b))
        # tiled over the settings
        with monkeypatch.context() as mp:
            mp.setattr(_predictive, "SETTINGS_PER_CALL", 7)
            for a, b in zip(o.output_covariance(x), whole):
                assert_array_equal(_bits(a), _bits(b))
            assert_array_equal(_bits(o.expected_variance_reduction(x, sigma=3.0)), _bits(gain))


def test_settings_none_is_the_design_grid_and_noise_per_setting_belongs_to_it(hip):
    g = np.random.default_rng(32)
    cloud = tp._prior("rabi", g, 5000)
    o = tp._object("rabi", cloud, tp._general_weights(g, cloud))
    grid = np.asarray(o.allsettings)
    assert grid.shape == (2, 35)
    for a, b in zip(o.output_covariance(), o.output_covariance(grid)):
        assert_array_equal(_bits(a), _bits(b))
    sigma = np.linspace(0.1, 0.2, 35)[None, :]
    nv = sigma * sigma                                   # (what the product forms from sigma)
    o.yvar_noise_model = lambda: nv
    per_setting = o.expected_variance_reduction()
    assert_array_equal(_bits(per_setting), _bits(o.expected_variance_reduction(grid, sigma=sigma)))
    with pytest.raises(ValueError, match="pass sigma"):
        o.expected_variance_reduction(grid)
    o.yvar_noise_model = lambda: nv[0, 0]
    assert_array_equal(_bits(o.expected_variance_reduction()[:, 0]), _bits(per_setting[:, 0]))


# --------------------------------------------------------------------------------------------- 3. selection
def _narrowed(utility_method="parameter_variance", sigma=300.0, **kw):
    """The issue's case: the tests' Lorentzian prior with the centre known to +-0.05, 33 settings."""
    g = np.random.default_rng(41)
    cloud = tp._prior("lorentz1", g, 5000)
    cloud[0] = 3.0 + g.uniform(-0.05, 0.05, 5000)
    w = tp._general_weights(g, g.normal(size=(1, 5000)))
    o = tp._object("lorentz1", cloud, w, utility_method=utility_method, default_noise_std=sigma, **kw)
    return o, cloud, w


def _oracle_utility(o, cloud, w, rows, a, cost, nu):
    x = np.asarray(o.allsettings)
    y = tp._rows(o, x)
    G, tol = np.empty((len(rows), x.shape[1])), np.empty((len(rows), x.shape[1]))
    for s in range(x.shape[1]):
        b = oracle.blocks(y[s], cloud[list(rows)], w)
        G[:, s], u, cond = oracle.gain(b["S"], b["K"], nu)
        tol_S, tol_K, _ = oracle.tolerances(b)
        tol[:, s] = oracle.gain_tolerance_end_to_end(b["K"], u, tol_S, tol_K, nu)
    V = b["V"]
    return oracle.utility(G, V, a, cost), oracle.utility(tol, V, a, cost), G


@pytest.mark.parametrize("row", [0, 1])
def test_selection_designs_for_the_parameter_of_interest(hip, row):
    o, cloud, w = _narrowed()
    o.set_parameters_of_interest([row])
    assert o.parameters_of_interest[0] == (row,) and o.parameters_of_interest[1].tolist() == [1.0]
    want, tol, _ = _oracle_utility(o, cloud, w, [row], [1.0], 1.0, [300.0 ** 2])
    top = np.sort(want)[::-1]
    assert (top[0] - top[1]) / top[0] > 1e-6, "the arg-max must be a property of the data"
    u = o.utility()
    assert u.shape == (33,)
    _note("U", np.abs(u - want), tol, f"utility, row {row}")
    xs = o.opt_setting()
    assert o.last_setting_index == int(np.argmax(want)) and xs == (o.allsettings[0, int(np.argmax(want))],)
    if row == 0:
        # the line centre is learnt on the flank; the output-variance utility goes for the peak top, the best place
        # for the amplitude
        plain, _, _ = _narrowed("variance_full")
        plain.opt_setting()
        assert abs(xs[0] - 3.0) > 0.05 and abs(plain.allsettings[0, plain.last_setting_index] - 3.0) < abs(xs[0] - 3.0)
    picked = o.good_setting()
    assert picked[0] in o.allsettings[0] and 0 <= o.last_setting_index < 33


def test_cost_weights_and_row_tiles_of_the_utility(hip):
    o, cloud, w = _narrowed()
    nu = [300.0 ** 2]
    # weights [1, 0, 0] are dims [0]: the same G bit for bit, the same U to the tolerance
    o.set_parameters_of_interest([0])
    u0 = o.utility()
    want, tol, _ = _oracle_utility(o, cloud, w, [0], [1.0], 1.0, nu)
    o.set_parameters_of_interest(None, [1, 0, 0])
    _note("U", np.abs(o.utility() - want), tol, "weights [1, 0, 0]")
    _note("U", np.abs(o.utility() - u0), 2 * tol, "weights [1, 0, 0] against dims [0]")
    assert_array_equal(_bits(o.expected_variance_reduction(dims=None)[0]), _bits(o.expected_variance_reduction(dims=[0])[0]))
    # a scalar and a per-setting cost
    o.set_parameters_of_interest([0, 1], [1.0, 2.5])
    for cost in (4.0, np.linspace(1.0, 3.0, 33)):
        o.cost_estimate = lambda cost=cost: cost
        want, tol, _ = _oracle_utility(o, cloud, w, [0, 1], [1.0, 2.5], cost, nu)
        _note("U", np.abs(o.utility() - want), tol, f"cost {np.ndim(cost)}-d")
        top = np.sort(want)[::-1]
        assert (top[0] - top[1]) / top[0] > 1e-6
        o.opt_setting()
        assert o.last_setting_index == int(np.argmax(want))
    # ten rows: the utility accumulates over two tiles of rows
    g = np.random.default_rng(42)
    cloud7 = tp._prior("lorentz7", g, 2000)
    w7 = tp._general_weights(g, cloud7)
    o7 = tp._object("lorentz7", cloud7, w7, utility_method="parameter_variance", default_noise_std=50.0)
    a = np.linspace(0.5, 2.0, 10)
    o7.set_parameters_of_interest(None, a)
    want, tol, _ = _oracle_utility(o7, cloud7, w7, range(10), a, 1.0, [2500.0])
    _note("U", np.abs(o7.utility() - want), tol, "ten rows")
    # every parameter is of interest until told otherwise
    fresh, _, _ = _narrowed()
    assert fresh.parameters_of_interest[0] == (0, 1, 2)
    want, tol, _ = _oracle_utility(fresh, cloud, w, [0, 1, 2], [1.0, 1.0, 1.0], 1.0, nu)
    _note("U", np.abs(fresh.utility() - want), tol, "all rows")


def test_the_new_method_is_named_and_needs_a_device_model(hip):
    import optbayesexpt_amd as obe
    pars = np.random.default_rng(43).normal(size=(2, 100))
    with pytest.raises(SyntaxError, match="parameter_variance"):
        obe.OptBayesExpt(obe.models.line_ab(), (np.arange(3.0),), pars, (), utility_method="nope")
    with pytest.raises(ValueError, match="parameter_variance.*DeviceModel"):
        obe.OptBayesExpt(lambda s, p, c: p[0] + p[1] * s[0], (np.arange(3.0),), pars, (), utility_method="parameter_variance")
    host = obe.OptBayesExpt(lambda s, p, c: p[0] + p[1] * s[0], (np.arange(3.0),), pars, ())
    host.set_parameters_of_interest([1])                      # (a choice, stored; the device is asked later)
    with pytest.raises(TypeError, match="from_function.*from_expression"):
        host.output_covariance()
    # a sweeper reaches the point utility through its own selection
    o = cases.build("sweeper")
    s = obe.OptBayesExptSweeper(o.model_function, o.setting_values, np.array(o.particles), o.cons, 3, scale=False,
                                utility_method="parameter_variance")
    s.set_parameters_of_interest([0])
    pair = s.opt_setting()
    assert len(pair) == 2 and np.all(np.isfinite(s.sweep_utility()))


# ------------------------------------------------------------------------------------------------- 4. state
def test_state_carries_the_parameters_of_interest(hip, tmp_path):
    import optbayesexpt_amd as obe
    o, cloud, w = _narrowed()
    assert "parameters_of_interest" not in _state.snapshot(o)          # never set: the snapshot it always was
    o.set_parameters_of_interest([1, 0], [2.0, 0.5])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for cyc in range(3):
            xs = o.opt_setting()
            o.pdf_update((xs, 48000.0 + 100.0 * cyc, 300.0))
    snap = _state.snapshot(o)
    assert snap["parameters_of_interest"]["dims"] == (1, 0)
    path = tmp_path / "o.state"
    obe.save(o, str(path))
    loaded, copied = obe.load(str(path)), copy.deepcopy(o)
    want = o.utility()
    for other in (loaded, copied):
        assert other.utility_method == "parameter_variance"
        assert other.parameters_of_interest[0] == (1, 0) and other.parameters_of_interest[1].tolist() == [2.0, 0.5]
        assert_array_equal(_bits(other.utility()), _bits(want))
        assert other.opt_setting() == o.opt_setting()
    # a snapshot written before there were parameters of interest has no such key: it loads, all rows, 1 each
    old = {k: v for k, v in _state.snapshot(o).items() if k != "parameters_of_interest"}
    older = _state.restore(old)
    assert older.parameters_of_interest[0] == (0, 1, 2) and "parameters_of_interest" not in _state.snapshot(older)
    o.set_parameters_of_interest(None)
    assert_array_equal(_bits(older.utility()), _bits(o.utility()))


def test_nothing_of_the_object_changes(hip):
    o = cases.build("lorentz_full")
    cases.run(o, "lorentz_full", 0, 4)
    before = tp._flags(o), o.sweep_state()
    o.output_covariance()
    o.expected_variance_reduction(dims=0)
    o.utility_parameter_variance()
    assert (tp._flags(o), o.sweep_state()) == before


# ------------------------------------------------------------------------------------------------ 5. figures
def test_worst_errors_are_reported(hip):
    """(runs last: the worst error / tolerance ratios seen by this file's comparisons)"""
    for kind, (ratio, what) in sorted(WORST.items()):
        print(f"worst {kind}: {ratio:.3g} ({what})")
    assert {"S", "K", "V", "G on the device's blocks", "G end to end", "U"} <= set(WORST)
