"""Design of a batch of measurements on the device (OptBayesExpt.output_cross_covariance / opt_setting_batch;
csrc/obe_predict.hip K14, csrc/obe_design.hip) against the long double oracle of tests/_design_oracle.py on the rows
y = eval_over_all_parameters((x_s,)) of the product itself.

The blocks are held to |dX| <= 1e-10 B_X + 1e-20 A_c(x) A_c'(p), X(x, x) to output_covariance()'s S at the same
tolerance; obe_design_step alone, fed the device's own S and X, to 1e-10 of the sum of the magnitudes of its terms with
cond(K_AA + N_A) <= 1e3 asserted on the inputs; opt_setting_batch end to end to the picks of the oracle (a relative
margin > 1e-6 between the oracle's best and second-best utility asserted before every comparison) and to the direct
solve within the first-order propagation of the block tolerances (_design_oracle's docstring).  Shapes stay below the
size at which the chunk plan of a call depends on its number of settings (clouds <= 5000), so requests of different
lengths agree bit for bit.

test_worst_errors_are_reported prints the worst error / tolerance per quantity; they have not been measured on an MI355X
yet (DESIGN.md section 6 says so)."""
import copy
import importlib.util
import os
import pickle
import warnings

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _design_oracle as oracle
import _state_cases as cases
import test_gpu_predictive as tp
from optbayesexpt_amd import _design, _predictive

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}
_bits = tp._bits


def _note(kind, err, tol, what):
    err, tol = np.asarray(err, dtype=np.float64), np.asarray(tol, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
    worst = float(np.max(ratio)) if np.size(ratio) else 0.0
    print(f"{what}: {kind}: worst error / tolerance {worst:.3g}")
    if worst >= WORST.get(kind, (0.0, ""))[0]:
        WORST[kind] = worst, what
    assert np.all(err <= tol), f"{what}: {kind}: worst error / tolerance {worst:.3g}"


def _check_cross(what, o, pts, x, w, diagonal=True):
    """output_cross_covariance(pts, x) against the oracle on the product's rows; the device result."""
    y_p, y = tp._rows(o, pts), tp._rows(o, x)
    X = o.output_cross_covariance(pts, x)
    n_c = o.n_channels
    assert X.shape == (pts.shape[1], n_c, n_c, x.shape[1]) and X.dtype == np.float64
    b = oracle.cross_blocks(y_p, y, w)
    tol = oracle.cross_tolerance(b)
    finite = np.isfinite(b["X"])
    assert not np.any(np.isfinite(X[~finite])), what           # a non-finite output gives non-finite entries
    _note("X", np.abs(X - b["X"])[finite], tol[finite], what)
    if diagonal:
        # X(x, x) is S(x): the first settings as pivots against output_covariance()
        k = min(x.shape[1], _design.pivots_per_call(n_c))
        S = o.output_covariance(x[:, :k], dims=[0])[1]
        own = o.output_cross_covariance(x[:, :k], x[:, :k])
        bd = oracle.cross_blocks(y[:k], y[:k], w)
        told = oracle.cross_tolerance(bd)
        for j in range(k):
            if np.all(np.isfinite(bd["X"][j, :, :, j])):
                _note("X(x, x) against S", np.abs(own[j, :, :, j] - S[:, :, j]), told[j, :, :, j], f"{what}, setting {j}")
    return X


# ------------------------------------------------------------------------- 1. shapes: clouds x settings
@pytest.mark.parametrize("n_x", [1, 2, 65, 1000])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_shapes_lorentzian(hip, n, n_x):
    g = np.random.default_rng([n, n_x, 14])
    cloud = tp._prior("lorentz1", g, n)
    x = tp._points("lorentz1", g, n_x)
    pts = tp._points("lorentz1", g, 3)
    for kind in ("dyadic", "general", "zeros"):
        w = tp._dyadic_weights(g, n) if kind == "dyadic" else tp._general_weights(g, cloud)
        if kind == "zeros" and n > 2:
            w[g.random(n) < 0.3] = 0.0
            w[-1] = np.nan
            w[1] = -0.5
            w[0] = 0.25
        o = tp._object("lorentz1", cloud, w)
        _check_cross(f"lorentz1 {n} x {n_x} {kind}", o, pts, x, w)


def test_a_million_particles(hip):
    g = np.random.default_rng(tp.BIG + 14)
    cloud = tp._prior("lorentz1", g, tp.BIG)
    x = tp._points("lorentz1", g, 3)
    pts = tp._points("lorentz1", g, 2)
    w = tp._general_weights(g, cloud)
    o = tp._object("lorentz1", cloud, w)
    _check_cross("lorentz1 BIG x 3 x 2 pivots", o, pts, x, w)


@pytest.mark.parametrize("n_pivots", [1, 2, 3, 4, 5, 8])
def test_rows_per_call_and_padding_rows_are_not_written(hip, n_pivots):
    """The three forms of the pass (1, 4, 8 rows), straight through the C ABI into a guarded buffer."""
    import torch
    g = np.random.default_rng([n_pivots, 15])
    cloud = tp._prior("lorentz1", g, 257)
    w = tp._general_weights(g, cloud)
    o = tp._object("lorentz1", cloud, w)
    x, pts = tp._points("lorentz1", g, 65), tp._points("lorentz1", g, n_pivots)
    dx, dpts = (torch.from_numpy(a).to(o._device) for a in (x, pts))
    _, p, dw = _predictive._inputs(o, None)
    guard = 7.25
    out = torch.full((8 + 1, 65), guard, dtype=torch.float64, device=o._device)
    mean = torch.empty((1, 65), dtype=torch.float64, device=o._device)
    nbytes = int(o._mlib.cdll.obe_output_cross_covariance_workspace_bytes(257, 65, 1, n_pivots))
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=o._device)
    ptr = _predictive._ptr
    o._mlib.call("obe_output_cross_covariance", o._model_struct, ptr(dx), 65, 65, ptr(dpts), n_pivots, n_pivots, ptr(p),
                 257, 257, ptr(dw), ptr(mean), 0, ptr(out), ptr(ws), nbytes, o._stream())
    got = out.cpu().numpy()
    assert np.all(got[n_pivots:] == guard)
    assert_array_equal(_bits(got[:n_pivots]), _bits(o.output_cross_covariance(pts, x)[:, 0, 0, :]))
    assert_array_equal(_bits(mean.cpu().numpy()), _bits(o.predict(x)[0]))
    # a workspace one byte short is refused before any launch
    from optbayesexpt_amd._lib import ObeHipError
    with pytest.raises(ObeHipError, match="workspace too small") as info:
        o._mlib.call("obe_output_cross_covariance", o._model_struct, ptr(dx), 65, 65, ptr(dpts), n_pivots, n_pivots, ptr(p),
                     257, 257, ptr(dw), ptr(mean), 0, ptr(out), ptr(ws), nbytes - 1, o._stream())
    assert info.value.refused_before_launch
    _check_cross(f"{n_pivots} pivots", o, pts, x, w, diagonal=False)


@pytest.mark.parametrize("name", ["lorentz7", "coil", "rabi", "expression", "function"])
def test_models(hip, name):
    for n, n_x in ((5000, 65), (257, 2)):
        g = np.random.default_rng([sum(map(ord, name)), n, 14])
        cloud = tp._prior(name, g, n)
        x = tp._points(name, g, n_x)
        pts = tp._points(name, g, 5)
        if name == "expression":
            pts = np.where(np.abs(pts) < 0.2, 0.5, pts)         # (the pole has a test of its own)
            x = np.where(np.abs(x) < 0.2, 0.5, x)
        w = tp._general_weights(g, cloud)
        o = tp._object(name, cloud, w)
        assert (o._mlib is not o._lib) == (name in ("expression", "function"))       # plugins serve their own model
        X = _check_cross(f"{name} {n} x {n_x}", o, pts, x, w)
        if name == "coil":
            assert X.shape[1:3] == (2, 2) and np.any(X[:, 0, 1] != X[:, 1, 0])        # rows of two channels: calls of 4 + 1 pivots


def test_noise_parameter_object(hip):
    o = cases.build("noise7")
    cases.run(o, "noise7", 0, 12)
    w = np.array(o.particle_weights)
    assert np.any(w == 0.0)                                          # the constraint zeroed some weights
    x = np.asarray(o.allsettings)[:, ::16]
    _check_cross("noise7", o, x[:, [3, 9]], x, w)
    assert_array_equal(_bits(o.output_cross_covariance(x[:, [3]])[..., ::16]), _bits(o.output_cross_covariance(x[:, [3]], x)))


def test_zero_weight_particles_do_not_matter_whatever_they_hold(hip):
    g = np.random.default_rng(23)
    n = 5000
    cloud = tp._prior("expression", g, n)
    w = tp._dyadic_weights(g, n)
    w[:6] = 0.0
    plain = tp._object("expression", cloud, w)
    x = np.array([[1.0, -2.0, 0.0, 0.5]])                   # a pole at x = 0: every weighted particle gives +-inf there
    pts = np.array([[0.75, 0.0, -1.5]])
    want = plain.output_cross_covariance(pts, x)
    cloud2 = cloud.copy()
    cloud2[0, :6] = [np.inf, -np.inf, np.nan, 0.0, 1e300, np.nan]
    cloud2[1, :6] = [np.nan, 1e308, np.inf, np.nan, -np.inf, 0.0]
    o = tp._object("expression", cloud2, w)
    y = tp._rows(o, x)
    assert not np.all(np.isfinite(y[0, 0, :6])) and np.all(np.isfinite(y[0, 0, 6:]))
    got = o.output_cross_covariance(pts, x)
    assert_array_equal(_bits(got), _bits(want))
    _check_cross("pole", o, pts, x, w, diagonal=False)
    # the pole as a pivot: its rows are not finite; as a setting: its column; nothing else is affected
    assert not np.any(np.isfinite(got[1])) and not np.any(np.isfinite(got[:, :, :, 2]))
    assert np.all(np.isfinite(got[[0, 2]][..., [0, 1, 3]]))


def test_cross_covariance_of_a_line_is_the_closed_form(hip):
    """a + b x: X(p, x) = V_a + (x + p) C_ab + x p V_b with (V, C) = covariance() (1 - sum w^2 / (sum w)^2), the
    population form of the reference's unbiased one.  covariance()'s own entries are held to the project's 1e-10 of
    their conditioning, <= sqrt(V_i V_j); that error, propagated through the closed form, is added to the bound."""
    import optbayesexpt_amd as obe
    g = np.random.default_rng(24)
    n = 5000
    cloud = np.array([g.normal(2.0, 0.5, n), g.normal(-1.0, 0.2, n)]) + 0.3 * g.normal(size=n)
    w = tp._general_weights(g, cloud)
    model = obe.models.from_expression("a + b * x", settings=("x",), parameters=("a", "b"))
    o = obe.OptBayesExpt(model, (np.linspace(-2.0, 3.0, 9),), cloud, (), scale=False)
    o.particle_weights = w
    x = np.asarray(o.allsettings)
    y = tp._rows(o, x)
    pts = x[:, [1, 7, 4]]
    X = o.output_cross_covariance(pts)
    cov = np.asarray(o.covariance()) * (1.0 - np.sum(w * w) / np.sum(w) ** 2)
    sd = np.sqrt(np.diag(cov))
    b = oracle.cross_blocks(tp._rows(o, pts), y, w)
    tol = oracle.cross_tolerance(b)
    for j in range(3):
        pj, xs = pts[0, j], x[0]
        want = cov[0, 0] + (xs + pj) * cov[0, 1] + xs * pj * cov[1, 1]
        bound = sd[0] * sd[0] + np.abs(xs + pj) * sd[0] * sd[1] + np.abs(xs * pj) * sd[1] * sd[1]
        _note("X of a line against the closed form", np.abs(X[j, 0, 0] - want), tol[j, 0, 0] + 1e-10 * bound, f"line, pivot {j}")


# ------------------------------------------------------------------------------------ 2. indexing, bit for bit
def test_indexing_is_bit_for_bit(hip, monkeypatch):
    g = np.random.default_rng(33)
    for name, n_piv in (("lorentz1", 17), ("coil", 9), ("lorentz7", 9)):
        cloud = tp._prior(name, g, 640)
        o = tp._object(name, cloud, tp._general_weights(g, cloud))
        x = tp._points(name, g, 100)
        pts = tp._points(name, g, n_piv)                        # 9 and 17 pivots: more than one call
        whole = o.output_cross_covariance(pts, x)
        # two identical calls
        assert_array_equal(_bits(o.output_cross_covariance(pts, x)), _bits(whole))
        # the pivots in any order, one at a time, a prefix of them
        order = g.permutation(n_piv)
        assert_array_equal(_bits(o.output_cross_covariance(pts[:, order], x)), _bits(whole[order]))
        for j in (0, n_piv - 1):
            assert_array_equal(_bits(o.output_cross_covariance(pts[:, j:j + 1], x)), _bits(whole[j:j + 1]))
        for k in (1, 2, 3, 5, 8):
            assert_array_equal(_bits(o.output_cross_covariance(pts[:, :k], x)), _bits(whole[:k]))
        # the first k columns are the request of the first k settings
        for k in (1, 37, 64, 65):
            assert_array_equal(_bits(o.output_cross_covariance(pts, x[:, :k])), _bits(whole[..., :k]))
        # tiled over the settings
        with monkeypatch.context() as mp:
            mp.setattr(_predictive, "SETTINGS_PER_CALL", 7)
            assert_array_equal(_bits(o.output_cross_covariance(pts, x)), _bits(whole))
        # the mean given or computed
        import torch
        dx, p, w = _predictive._inputs(o, x)
        dp = torch.from_numpy(pts).to(o._device)
        mean, _ = _design._moments(o, dx, p, w)
        assert_array_equal(_bits(mean.cpu().numpy()), _bits(o.predict(x)[0]))
        assert_array_equal(_bits(_design._cross(o, dx, dp, p, w, mean).cpu().numpy()), _bits(whole))


def test_settings_none_is_the_design_grid(hip):
    g = np.random.default_rng(34)
    cloud = tp._prior("rabi", g, 5000)
    o = tp._object("rabi", cloud, tp._general_weights(g, cloud))
    grid = np.asarray(o.allsettings)
    assert grid.shape == (2, 35)
    pts = (np.array([0.5, 1.0]), np.array([-1.0, 2.0]))       # points as predict() takes settings
    assert_array_equal(_bits(o.output_cross_covariance(pts)), _bits(o.output_cross_covariance(np.array(pts), grid)))


# ------------------------------------------------------------------------------------ 3. obe_design_step alone
def _nu_for(S, mean):
    """test_gpu_interest's: a noise variance per channel nu = tr S / 100, no smaller than 1e-12 of the output's scale."""
    nu = max(float(np.sum(S)) / 100.0, 1e-12 * float(np.sum(np.square(mean))))
    return np.full(S.shape[0], nu if nu > 0 else 1.0)


@pytest.mark.parametrize("name,picks", [("lorentz1", [5, 20, 5, 11, 64]), ("coil", [47, 20, 47, 13]), ("rabi", [9, 34, 12, 20])])
@pytest.mark.parametrize("costly", [False, True])
def test_design_step_against_the_recurrence_on_the_same_inputs(hip, name, picks, costly):
    """One setting is conditioned on twice; the picks are settings of comparable variance, so that nu = tr S / 100 per
    setting keeps cond(K_AA + N_A) below 1e3 (asserted)."""
    import torch
    g = np.random.default_rng([sum(map(ord, name)), 35])
    cloud = tp._prior(name, g, 2000)
    w = tp._general_weights(g, cloud)
    o = tp._object(name, cloud, w)
    x = tp._points(name, g, 65) if name != "rabi" else np.asarray(o.allsettings)
    n_x, n_c = x.shape[1], o.n_channels
    dx, p, dw = _predictive._inputs(o, x)
    mean, var = _design._moments(o, dx, p, dw)
    S, m = var.cpu().numpy(), mean.cpu().numpy()
    nu = np.stack([_nu_for(S[:, s], m[:, s]) for s in range(n_x)], axis=1)         # per setting
    cost = 1.0 + g.random(n_x) if costly else 2.5
    d_cost = (torch.from_numpy(cost).to(o._device), 1.0) if costly else (None, 2.5)
    X = {q: o.output_cross_covariance(x[:, q:q + 1], x)[0] for q in set(picks)}     # the device's own blocks
    rows = [(q, c) for q in picks for c in range(n_c)]
    a = np.array([[X[q][c, d, r] for r, d in rows] for q, c in rows]) + np.diag([nu[c, q] for q, c in rows])
    assert np.linalg.cond(a) <= 1e3, np.linalg.cond(a)
    step = _design._Step(o, var.clone(), nu, d_cost, len(rows), False)
    want = oracle.start(S)
    value, best, info = step.step()
    u = oracle.utility(want["v"], nu, cost)
    if oracle.margin(u) > 1e-6:                              # (two of the points are the same setting)
        assert best == oracle.first_finite_maximum(u) and value == step.utility.cpu().numpy()[best]
    _note("U of the step", np.abs(step.utility.cpu().numpy() - u), 1e-10 * oracle.utility(want["terms_v"], nu, cost), name)
    assert info == 0.0
    for q in picks:
        value, best, info = step.step(torch.from_numpy(X[q]).to(o._device), q)
        want = oracle.condition(want, X[q], q, nu)
        tol_v, tol_info = oracle.recurrence_tolerance(want)
        _note("v of the step", np.abs(step.cvar.cpu().numpy() - want["v"]), tol_v, f"{name} after {q}")
        _note("info of the step", abs(info - want["info"]), tol_info, f"{name} after {q}")
        u = oracle.utility(want["v"], nu, cost)
        _note("U of the step", np.abs(step.utility.cpu().numpy() - u), oracle.utility(tol_v, nu, cost), f"{name} after {q}")
        if oracle.margin(u) > 1e-6:
            assert best == oracle.first_finite_maximum(u) and value == step.utility.cpu().numpy()[best]


def test_arg_max_rules_of_the_step(hip):
    import torch
    g = np.random.default_rng(36)
    cloud = tp._prior("lorentz1", g, 64)
    o = tp._object("lorentz1", cloud)

    def best_of(values, taken=None):
        cvar = torch.from_numpy(np.array(values, dtype=np.float64)[None, :]).to(o._device)
        step = _design._Step(o, cvar, np.ones((1, 1)), (None, 1.0), 0, taken is not None)
        if taken is not None:
            step.taken.copy_(torch.from_numpy(np.array(taken, dtype=np.uint8)))
        value, best, _ = step.step()
        assert_array_equal(step.utility.cpu().numpy(), np.array(values, dtype=np.float64))
        assert best == oracle.first_finite_maximum(values, taken)
        return value, best

    assert best_of([1.0, 3.0, 3.0, 2.0]) == (3.0, 1)                       # the first maximum
    assert best_of([np.nan, 1.0, np.nan, 2.0, 2.0]) == (2.0, 3)            # NaN is skipped (np.argmax would take it)
    assert best_of([np.inf, 1.0, -np.inf]) == (1.0, 1)                     # ... and so is an infinite utility
    value, best = best_of([np.nan, np.nan, np.nan])
    assert best == -1 and np.isnan(value)                                  # none finite
    assert best_of([5.0, 4.0, 5.0, 1.0], taken=[1, 0, 0, 0]) == (5.0, 2)   # a taken setting is never chosen
    value, best = best_of([5.0, np.nan], taken=[1, 0])
    assert best == -1
    # ties across the threads of the scan: 1000 settings, the maximum at 700 and 300
    values = np.linspace(0.0, 1.0, 1000)
    values[[700, 300]] = 2.0
    assert best_of(values) == (2.0, 300)
    values[-1] = 3.0
    assert best_of(values) == (3.0, 999)


# ------------------------------------------------------------------------------------ 4. opt_setting_batch
def _design_case(name, seed):
    """(cloud, weights) of an end-to-end case; test_gpu_predictive's priors and design grids."""
    g = np.random.default_rng([sum(map(ord, name)), seed, 37])
    cloud = tp._prior(name, g, 3000)
    if name == "lorentz1":
        cloud[0] = 3.0 + g.uniform(-0.4, 0.4, 3000)
    return cloud, tp._general_weights(g, cloud)


CASES = {
    # name: (model, seed, n, sigma per channel)
    "lorentz1": ("lorentz1", 1, 6, (2000.0,)),        # the noise is of the size of the spread: a setting is read twice
    "coil": ("coil", 1, 4, (8.0, 8.0)),
    "rabi": ("rabi", 1, 4, (2000.0,)),
    "lorentz7": ("lorentz7", 1, 4, (1500.0,)),
}


def _per_setting(n_x):
    """(factor of the noise variance (1, n_x), cost (n_x,)) of the per-setting case."""
    g = np.random.default_rng(38)
    return 1.0 + g.random((1, n_x)), 1.0 + g.random(n_x)


def _noise_prior(n=3000):
    """(cloud, weights) of the noise-parameter case: seven peaks, the noise in row 9."""
    g = np.random.default_rng(39)
    prior = np.vstack([g.uniform(2, 4, (7, n)), g.uniform(400, 2000, (1, n)), g.normal(500, 1000, (1, n)),
                       g.uniform(1000, 2000, (1, n))])
    return prior, tp._general_weights(g, prior)


def _state_after(cov, nu, cost, j, distinct):
    """The oracle's recurrence state after the first j picks."""
    return oracle.greedy(cov, nu, cost, j, distinct=distinct)["state"] if j else oracle.start(cov.S())


def _compare_design(what, o, w, n, nu, cost=1.0, repeats=None, **kw):
    """opt_setting_batch(n, **kw) against the oracle on the product's rows; (the device's report, the oracle's)."""
    grid = np.asarray(o.allsettings)
    cov = oracle.Cov(tp._rows(o, grid), w)
    want = oracle.greedy(cov, nu, cost, n, distinct=kw.get("distinct", False))
    print(f"{what}: picks {want['indices'].tolist()}, margins {np.array2string(want['margins'], precision=3)}")
    assert np.all(want["margins"] > 1e-6), "the arg-max must be a property of the data"
    before = o.last_setting_index
    xs = o.opt_setting_batch(n, **kw)
    report = o.last_batch_design
    assert o.last_setting_index == before
    assert_array_equal(report["indices"], want["indices"])
    assert report["indices"].dtype == np.int64 and set(report) == {"indices", "utility", "information"}
    assert isinstance(xs, tuple) and len(xs) == grid.shape[0]
    for d in range(grid.shape[0]):
        assert_array_equal(xs[d], grid[d, want["indices"]])
    if repeats is not None:
        assert (len(set(want["indices"].tolist())) < n) == repeats, want["indices"]
    # v (what the last pick was made from) and the information after every pick, against the direct solve
    _, state = _design.plan(o, n, kw.get("sigma"), kw.get("distinct", False))
    picks, distinct = want["indices"], kw.get("distinct", False)
    v_dir = oracle.direct(cov, nu, picks[:n - 1])[0]
    tol_v, _ = oracle.end_to_end_tolerance(cov, nu, picks[:n - 1], _state_after(cov, nu, cost, n - 1, distinct))
    _note("v end to end", np.abs(state.cvar.cpu().numpy() - v_dir), tol_v, what)
    nu_full = oracle._noise(nu, cov.n_c, cov.n_x)
    for j in range(n):
        info_dir, cond = oracle.direct(cov, nu, picks[:j + 1])[1:3]
        _, tol_info = oracle.end_to_end_tolerance(cov, nu, picks[:j + 1], _state_after(cov, nu, cost, j + 1, distinct))
        _note("information end to end", abs(report["information"][j] - info_dir), tol_info, f"{what}, pick {j}")
        tol_vj, _ = oracle.end_to_end_tolerance(cov, nu, picks[:j], _state_after(cov, nu, cost, j, distinct))
        u_dir = oracle.utility(oracle.direct(cov, nu, picks[:j])[0], nu_full, cost)[picks[j]]
        _note("U end to end", abs(report["utility"][j] - u_dir), oracle.utility(tol_vj, nu_full, cost)[picks[j]],
              f"{what}, pick {j}")
    assert np.all(np.diff(report["information"]) > 0)
    return report, want


@pytest.mark.parametrize("case", sorted(CASES))
def test_batch_design_is_the_oracles(hip, case):
    name, seed, n, sigma = CASES[case]
    cloud, w = _design_case(name, seed)
    o = tp._object(name, cloud, w)
    nu = np.square(np.array(sigma))[:, None]
    _compare_design(case, o, w, n, nu, sigma=np.array(sigma) if len(sigma) > 1 else sigma[0])
    assert o.last_batch_design["indices"].shape == (n,)


def test_repeats_distinct_noise_and_cost(hip):
    name, seed, n, sigma = CASES["lorentz1"]
    cloud, w = _design_case(name, seed)
    # the model's own noise; pick 0 is variance_full's opt_setting()
    o = tp._object(name, cloud, w, default_noise_std=sigma[0])
    nu = np.array([[sigma[0] ** 2]])
    report, want = _compare_design("repeats", o, w, n, nu, repeats=True)
    full = tp._object(name, cloud, w, utility_method="variance_full", default_noise_std=sigma[0])
    assert want["margins"][0] > 1e-6
    full.opt_setting()
    assert full.last_setting_index == report["indices"][0]
    # the call is independent of utility_method
    assert_array_equal(full.opt_setting_batch(n)[0], np.asarray(o.allsettings)[0, report["indices"]])
    # the same case with distinct=True
    report_d, _ = _compare_design("distinct", o, w, n, nu, repeats=False, distinct=True)
    assert len(set(report_d["indices"].tolist())) == n and report_d["indices"][0] == report["indices"][0]
    # per-setting noise and an overridden cost_estimate() array
    factor, cost = _per_setting(33)
    nv = nu * factor
    o.yvar_noise_model = lambda: nv
    o.cost_estimate = lambda: cost
    _compare_design("noise and cost per setting", o, w, n, nv, cost)
    # sigma given: a scalar, and per setting
    _compare_design("sigma given", o, w, 4, np.array([[1000.0 ** 2]]), cost, sigma=1000.0)
    sg = np.sqrt(nv)
    _compare_design("sigma per setting", o, w, 4, sg * sg, cost, sigma=sg)


def test_noise_parameter_design_and_refusals(hip):
    import optbayesexpt_amd as obe
    g = np.random.default_rng(40)
    prior, w = _noise_prior()
    o = obe.OptBayesExptNoiseParameter(obe.models.lorentzian(7), tp._design("lorentz7"), prior, (0.1,),
                                       noise_parameter_index=9, scale=False)
    o.particle_weights = w
    nu = np.asarray(o.yvar_noise_model()).reshape(1, 1)
    assert 1000.0 ** 2 < nu[0, 0] < 2000.0 ** 2
    _compare_design("noise parameter", o, w, 4, nu)
    # refusals
    with pytest.raises(ValueError, match="at least 1"):
        o.opt_setting_batch(0)
    with pytest.raises(ValueError, match="128"):
        o.opt_setting_batch(129)
    with pytest.raises(ValueError, match="finite and > 0"):
        o.opt_setting_batch(2, sigma=np.inf)
    host = obe.OptBayesExpt(lambda s, p, c: p[0] + p[1] * s[0], (np.arange(3.0),), g.normal(size=(2, 100)), ())
    with pytest.raises(TypeError, match="from_function.*from_expression"):
        host.opt_setting_batch(2)
    assert host.last_batch_design is None
    s = cases.build("sweeper")
    with pytest.raises(TypeError, match="intervals"):
        s.opt_setting_batch(2)
    # no finite utility left: three settings, four distinct picks
    tiny = obe.OptBayesExpt(obe.models.lorentzian(), (np.array([2.5, 3.0, 3.5]),), prior[[0, 7, 8]], (0.1,), scale=False)
    assert len(tiny.opt_setting_batch(3, sigma=100.0, distinct=True)[0]) == 3
    with pytest.raises(ValueError, match="pick 3"):
        tiny.opt_setting_batch(4, sigma=100.0, distinct=True)
    # 128 scalar readings: the limit itself runs
    assert len(tiny.opt_setting_batch(128, sigma=100.0)[0]) == 128
    assert np.all(np.diff(tiny.last_batch_design["information"]) > 0)


# ------------------------------------------------------------------------------------------------- 5. state
def test_nothing_of_the_object_changes(hip):
    o = cases.build("lorentz_full")
    cases.run(o, "lorentz_full", 0, 4)
    before = tp._flags(o), o.sweep_state(), o.last_setting_index
    o.output_cross_covariance((3.0,))
    o.opt_setting_batch(4)
    assert (tp._flags(o), o.sweep_state(), o.last_setting_index) == before


@pytest.mark.parametrize("case", ["lorentz_full", "noise7"])
def test_a_trajectory_is_the_same_with_and_without_designs(hip, case):
    """30 cycles, the sweep enqueued ahead (lorentz_full) and a noise parameter (noise7): bit-equal with and without
    opt_setting_batch(4) before every update."""
    plain = cases.build(case)
    picks, resampled = cases.run(plain, case, 0, 30)
    o = cases.build(case)
    got, flags = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for cyc in range(30):
            if case == "lorentz_full":
                o.opt_setting_batch(4)                         # (the sweep enqueued behind the last update is pending)
            x = o.opt_setting()
            got.append(int(o.last_setting_index))
            o.opt_setting_batch(4)
            assert o.last_setting_index == got[-1]
            o.pdf_update(cases.measure(o, case, cyc, x))
            flags.append(bool(o.just_resampled))
    assert got == picks and flags == resampled
    a, b = cases.outcome(plain, picks, resampled), cases.outcome(o, got, flags)
    assert_array_equal(_bits(a["particles"]), _bits(b["particles"]))
    assert_array_equal(_bits(a["weights"]), _bits(b["weights"]))
    assert a["rng"] == b["rng"]


def test_copies_and_restored_objects_design_the_same_and_carry_no_report(hip, tmp_path):
    import optbayesexpt_amd as obe
    o = cases.build("lorentz_full")
    cases.run(o, "lorentz_full", 0, 3)
    assert o.last_batch_design is None
    want = o.opt_setting_batch(5)
    report = o.last_batch_design
    assert report is not None
    path = tmp_path / "o.state"
    obe.save(o, str(path))
    for other in (copy.deepcopy(o), pickle.loads(pickle.dumps(o)), obe.load(str(path))):
        assert other.last_batch_design is None
        assert_array_equal(other.opt_setting_batch(5)[0], want[0])
        for k in report:
            assert_array_equal(_bits(other.last_batch_design[k]), _bits(report[k]))


# ----------------------------------------------------------------------------------------------- 6. example
def test_batch_design_example(hip):
    spec = importlib.util.spec_from_file_location("batch_design", os.path.join(ROOT, "examples", "batch_design.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        true, mean, std = mod.main(n_rounds=12, n_samples=20000, seed=3, quiet=True)
    assert np.all(np.abs(mean - np.array(true)) < 5 * std + 1e-9)
    assert std[0] < 0.01                                  # the peak position is pinned down


# ------------------------------------------------------------------------------------------------ 7. figures
def test_worst_errors_are_reported(hip):
    """(runs last: the worst error / tolerance ratios seen by this file's comparisons)"""
    for kind, (ratio, what) in sorted(WORST.items()):
        print(f"worst {kind}: {ratio:.3g} ({what})")
    assert {"X", "X(x, x) against S", "v of the step", "info of the step", "U of the step", "v end to end",
            "information end to end", "U end to end"} <= set(WORST)
