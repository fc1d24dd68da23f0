"""Design of a batch of measurements for parameters of interest on the device (OptBayesExpt.opt_setting_batch(interest=);
csrc/obe_design.hip: obe_design_interest_step) against the long double oracle of tests/_interest_design_oracle.py on the
rows y = eval_over_all_parameters((x_s,)) of the product itself.

obe_design_interest_step alone, fed the device's own S, K, V and X, is held after every pivot to 1e-10 of the sum of the
magnitudes of the terms of each quantity (S, K, Vleft, the T rows), its gains to 1e-10 sum_c |u_c| |k_c| on the S and K it
left, with cond(K_AA + N_A) <= 1e3 asserted on the inputs.  opt_setting_batch(n, interest=...) end to end is held to the
picks of the oracle (a relative margin > 1e-6 between the oracle's best and second-best utility asserted before every
comparison) and to the direct solve V_d - k_A^T (K_AA + N_A)^-1 k_A within the first-order propagation of the block
tolerances (_interest_design_oracle's docstring).  Clouds stay <= 5000 particles, below the size at which the chunk plan
of a call depends on its number of settings.

Measured on an MI355X (test_worst_errors_are_reported prints them), worst error / tolerance: S, K, Vleft and T of the
step 0 (the bits of the NumPy recurrence), G of the step 6.9e-6, U of the step 8.3e-6, V end to end 1.6e-6, variance_left
end to end 6.4e-7, U end to end 3.1e-7, Vleft by the T rows against the direct solve 6.2e-7 and against the gain route
1.1e-7; DESIGN.md section 6."""
import copy
import importlib.util
import os
import pickle
import warnings

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _interest_design_oracle as oracle
import _state_cases as cases
import test_gpu_predictive as tp
from optbayesexpt_amd import _design, _interest

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


# --------------------------------------------------------------------------- 1. obe_design_interest_step alone
def _step_noise(S, n_picks, per_setting, g):
    """A noise variance that keeps cond(K_AA + N_A) below 1e3 whatever the pivots: lambda_max(K_AA) <= sum of tr S over
    the n_picks pivots <= n_picks max tr S.  Per channel: nu = max tr S / 50, cond <= 1 + 50 n_picks.  Per setting:
    nu(s) = max(tr S(s), max tr S / 2) (1 + r_s / 2) / 25 with r in [0, 1): nu >= max tr S / 50, the same bound."""
    n_c, n_x = S.shape[0], S.shape[2]
    tr = np.einsum("ccs->s", S)
    top = float(np.max(tr))
    if per_setting:
        return np.array(np.broadcast_to(np.maximum(tr, top / 2) * (1.0 + 0.5 * g.random(n_x)) / 25.0, (n_c, n_x)))
    return np.full((n_c, 1), top / 50.0)


def _pivots(n_x):
    """Setting 0, the last setting and one setting conditioned on twice."""
    return {1: [0, 0], 2: [0, 1, 0]}.get(n_x, [0, n_x - 1, 20, 0, 11])


STEP_MODELS = {"lorentz1": [2, 0], "coil": [0, 2, 1], "lorentz7": [9, 0, 1, 2, 3, 4, 5, 7, 8]}      # the rows of interest


def _packed(S):
    n_c = S.shape[0]
    return np.stack([S[c, c2] for c in range(n_c) for c2 in range(c + 1)])


@pytest.mark.parametrize("per_setting", [False, True])
@pytest.mark.parametrize("n_x", [1, 2, 65, 257])
@pytest.mark.parametrize("name", sorted(STEP_MODELS))
def test_step_against_the_recurrence_on_the_same_inputs(hip, name, n_x, per_setting):
    """After every pivot: S (every packed entry), K, Vleft, the T rows, the gains, U and the best index.  per_setting:
    the noise per setting (ld_noise = n_x) and the cost a device array; else per channel and a scalar.  Rows of the
    factor and T stores beyond rows_done are compared with the pattern they were filled with."""
    import torch
    g = np.random.default_rng([sum(map(ord, name)), n_x, int(per_setting), 51])
    dims = STEP_MODELS[name]
    cloud = tp._prior(name, g, 2000)
    w = tp._general_weights(g, cloud)
    o = tp._object(name, cloud, w)
    x = tp._points(name, g, n_x)
    n_c, n_sel = o.n_channels, len(dims)
    picks = _pivots(n_x)
    _, ycov, xcov, pvar = _interest._blocks(o, x, tuple(dims))
    S, K, V = _interest.unpack_lower(ycov.cpu().numpy(), n_c), xcov.cpu().numpy(), pvar.cpu().numpy()
    nu_dev = _step_noise(S, len(picks), per_setting, g)
    nu = np.array(np.broadcast_to(nu_dev, (n_c, n_x)))
    a = 0.5 + g.random(n_sel)
    cost = 1.0 + g.random(n_x) if per_setting else 2.5
    d_cost = (torch.from_numpy(cost).to(o._device), 1.0) if per_setting else (None, 2.5)
    X = {q: o.output_cross_covariance(x[:, q:q + 1], x)[0] for q in set(picks)}     # the device's own blocks
    rows = [(q, c) for q in picks for c in range(n_c)]
    A = np.array([[X[q][c, d, r] for r, d in rows] for q, c in rows]) + np.diag([nu[c, q] for q, c in rows])
    assert np.linalg.cond(A) <= 1e3, np.linalg.cond(A)
    max_rows = len(rows) + 2
    step = _design._InterestStep(o, ycov.clone(), xcov.clone(), pvar, a, nu_dev, d_cost, max_rows, False)
    guard = 7.25
    step.factors.fill_(guard)
    step.tstore.fill_(guard)
    want = oracle.start(S, K, V)
    what = f"{name} x {n_x}"

    def compare(after):
        tol_S, tol_K, tol_left, tol_T = oracle.recurrence_tolerance(want)
        got_S, got_K = step.ycov.cpu().numpy(), step.xcov.cpu().numpy()
        _note("S of the step", np.abs(got_S - _packed(want["S"])), _packed(tol_S), f"{what} {after}")
        _note("K of the step", np.abs(got_K - want["K"]), tol_K, f"{what} {after}")
        _note("Vleft of the step", np.abs(step.pvar_left.cpu().numpy() - want["left"]), tol_left, f"{what} {after}")
        done = step.rows_done
        assert done == len(want["T"])
        if done:
            _note("T of the step", np.abs(step.tstore.cpu().numpy()[:done] - np.array(want["T"])), np.array(tol_T),
                  f"{what} {after}")
        # nothing beyond the rows of the pivots so far
        assert np.all(step.factors.cpu().numpy()[done:] == guard) and np.all(step.tstore.cpu().numpy()[done:] == guard)
        # the gains on the S and K the device left, U from them
        full = _interest.unpack_lower(got_S, n_c)
        G, u, cond = oracle.gains(full, got_K, nu)
        assert cond <= 1e3
        tol_G = 1e-10 * np.einsum("rcs,rcs->rs", np.abs(u), np.abs(got_K))
        got_G, got_U = step.gain.cpu().numpy(), step.utility.cpu().numpy()
        _note("G of the step", np.abs(got_G - G), tol_G, f"{what} {after}")
        _note("U of the step", np.abs(got_U - oracle.utility(G, V, a, cost)), oracle.utility(tol_G, V, a, cost),
              f"{what} {after}")
        return oracle.utility(oracle.gains(want["S"], want["K"], nu)[0], V, a, cost), got_U, got_G

    value, best, gain = step.step()
    u, got_U, got_G = compare("before any pivot")
    assert_array_equal(_bits(step.ycov.cpu().numpy()), _bits(ycov.cpu().numpy()))          # nothing was conditioned on
    if oracle.margin(u) > 1e-6:
        assert best == oracle.first_finite_maximum(u)
    assert value == got_U[best] and _bits(gain).tolist() == _bits(got_G[:, best]).tolist()
    for q in picks:
        value, best, gain = step.step(torch.from_numpy(X[q]).to(o._device), q)
        want = oracle.condition(want, X[q], q, nu)
        u, got_U, got_G = compare(f"after {q}")
        if oracle.margin(u) > 1e-6:
            assert best == oracle.first_finite_maximum(u)
        assert value == got_U[best] and _bits(gain).tolist() == _bits(got_G[:, best]).tolist()
    assert step.rows_done == len(rows) == max_rows - 2
    # no room for one more pivot's rows beyond max_rows: refused before any launch
    from optbayesexpt_amd._lib import ObeHipError
    step.max_rows = step.rows_done + n_c - 1
    with pytest.raises(ObeHipError, match="no room") as info:
        step.step(torch.from_numpy(X[picks[0]]).to(o._device), picks[0])
    assert info.value.refused_before_launch


def test_taken_settings_nan_columns_and_a_poisoned_pivot(hip):
    """A setting whose blocks are NaN is never chosen and stays NaN, the others are not affected; a taken setting is
    never chosen; a pivot whose g is not > 0 (a noise the product refuses, the kernel does not) makes everything NaN and
    leaves no setting to choose."""
    import torch
    g = np.random.default_rng(52)
    cloud = tp._prior("coil", g, 500)
    w = tp._general_weights(g, cloud)
    o = tp._object("coil", cloud, w)
    x = tp._points("coil", g, 65)
    _, ycov, xcov, pvar = _interest._blocks(o, x, (0, 2))
    S = _interest.unpack_lower(ycov.cpu().numpy(), 2)
    nu = _step_noise(S, 2, True, g)
    plain = _design._InterestStep(o, ycov.clone(), xcov.clone(), pvar, np.ones(2), nu, (None, 1.0), 4, False)
    _, first, _ = plain.step()
    base_U = plain.utility.cpu().numpy()
    X =o.output_cross_covariance(x[:, first:first + 1], x)[0]
    d_X = torch.from_numpy(X).to(o._device)
    _, second, _ = plain.step(d_X, first)
    assert first >= 0 and second >= 0
    # the first choice NaN in S: never chosen, before and after a pivot; the other columns keep their bits
    bad_S = ycov.clone()
    bad_S[1, first] = np.nan
    poisoned = _design._InterestStep(o, bad_S, xcov.clone(), pvar, np.ones(2), nu, (None, 1.0), 4, True)
    value, best, _ = poisoned.step()
    others = np.arange(65) != first
    assert best != first and best >= 0 and np.isnan(poisoned.utility.cpu().numpy()[first]) and np.isfinite(value)
    assert_array_equal(_bits(poisoned.utility.cpu().numpy()[others]), _bits(base_U[others]))
    poisoned.taken[best] = 1
    value2, best2, _ = poisoned.step(torch.from_numpy(o.output_cross_covariance(x[:, best:best + 1], x)[0]).to(o._device), best)
    assert best2 not in (first, best) and best2 >= 0 and np.isfinite(value2)
    assert np.all(np.isnan(poisoned.gain.cpu().numpy()[:, first])) and np.all(np.isfinite(poisoned.gain.cpu().numpy()[:, others]))
    # g <= 0 at the pivot: NaN everywhere, nothing to choose
    neg = nu.copy()
    neg[:, first] = -1e30
    broken = _design._InterestStep(o, ycov.clone(), xcov.clone(), pvar, np.ones(2), neg, (None, 1.0), 4, False)
    value, best, gain = broken.step(d_X, first)
    assert best == -1 and np.isnan(value) and gain is None
    for t in (broken.ycov, broken.xcov, broken.pvar_left, broken.utility, broken.gain, broken.tstore[:2], broken.factors[:2]):
        assert np.all(np.isnan(t.cpu().numpy()))


# ------------------------------------------------------------------------------------------------- 2. pick 0
@pytest.mark.parametrize("name,dims,weights", [("lorentz1", [0, 1], [1.0, 2.5]), ("lorentz7", None, None), ("coil", [2], None)])
def test_pick_0_is_the_single_reading_design_bit_for_bit(hip, name, dims, weights):
    """The call without a pivot launches obe_variance_reduction's kernel on the blocks utility_parameter_variance()
    forms, in the same tiles of 8 rows with the same weights: the same bits by construction (lorentz7: ten rows, two
    tiles)."""
    g = np.random.default_rng([sum(map(ord, name)), 53])
    cloud = tp._prior(name, g, 3000)
    w = tp._general_weights(g, cloud)
    sigma = {"lorentz1": 300.0, "lorentz7": 50.0, "coil": 8.0}[name]
    o = tp._object(name, cloud, w, utility_method="parameter_variance", default_noise_std=sigma)
    o.set_parameters_of_interest(dims, weights)
    cost = 1.0 + g.random(33)
    for c in (None, cost):
        if c is not None:
            o.cost_estimate = lambda c=c: c
        want = o.utility_parameter_variance()
        rows, a = o.parameters_of_interest
        report, state = _design.plan_interest(o, 1, rows, a)
        assert_array_equal(_bits(state.utility.cpu().numpy()), _bits(want))
        assert_array_equal(_bits(state.gain.cpu().numpy()), _bits(o.expected_variance_reduction(dims=rows)))
        assert state.rows_done == 0
        o.opt_setting()                                       # (the same bits: the same first maximum)
        assert report["indices"].tolist() == [o.last_setting_index] and report["utility"][0] == want[o.last_setting_index]
        xs = o.opt_setting_batch(1, interest=True)
        assert xs[0].tolist() == [np.asarray(o.allsettings)[0, o.last_setting_index]]


def test_a_batch_of_one_launches_no_cross_covariance_and_n_launches_n_minus_1(hip, monkeypatch):
    g = np.random.default_rng(54)
    cloud = tp._prior("lorentz1", g, 500)
    o = tp._object("lorentz1", cloud, tp._general_weights(g, cloud), default_noise_std=2000.0)
    calls = []
    real = o._mlib.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(o._mlib, "call", counting)
    o.opt_setting_batch(1, interest=0)
    assert calls.count("obe_output_cross_covariance") == 0 and calls.count("obe_design_interest_step") == 1
    assert calls.count("obe_output_covariance") == 1 and "obe_design_step" not in calls
    del calls[:]
    o.opt_setting_batch(5, interest=[0, 2])
    assert calls.count("obe_output_cross_covariance") == 4 and calls.count("obe_design_interest_step") == 5
    assert calls.count("obe_output_covariance") == 1 and "obe_predictive_moments" not in calls


# ------------------------------------------------------------------------------------ 3. opt_setting_batch
def _design_case(name, seed):
    """(cloud, weights) of an end-to-end case: the tests' priors (the Lorentzian's centre anywhere in [2, 4]: the ends of
    the grid are five line widths from the nearest centre, and the background's utility is not flat there)."""
    g = np.random.default_rng([sum(map(ord, name)), seed, 37])
    cloud = tp._prior(name, g, 3000)
    return cloud, tp._general_weights(g, cloud)


CASES = {
    # case: (model, seed, n, sigma per channel, interest, interest_weights)
    "x0": ("lorentz1", 2, 6, (500.0,), 0, None),
    "x0, settings read twice": ("lorentz1", 2, 6, (2000.0,), 0, None),      # the noise is of the size of the spread
    "background": ("lorentz1", 2, 6, (500.0,), 2, None),
    "x0 and amplitude": ("lorentz1", 2, 6, (500.0,), [0, 1], [1.0, 0.5]),
    "coil": ("coil", 1, 4, (8.0, 8.0), [0, 2], [1.0, 0.5]),
}
_JOINT = {}


def _joint(key, o, w, rows):
    """The oracle's blocks of a case, formed once."""
    if key not in _JOINT:
        grid = np.asarray(o.allsettings)
        _JOINT[key] = oracle.Joint(tp._rows(o, grid), np.array(o.particles)[list(rows)], w)
    return _JOINT[key]


def _compare_design(what, o, w, n, nu, rows, a, cost=1.0, key=None, **kw):
    """opt_setting_batch(n, **kw) against the oracle on the product's rows; (the device's report, the oracle's)."""
    grid = np.asarray(o.allsettings)
    joint = _joint(key or what, o, w, rows)
    distinct = kw.get("distinct", False)
    a = np.asarray(a, dtype=np.float64)
    want = oracle.greedy(joint, nu, a, cost, n, distinct=distinct)
    print(f"{what}: picks {want['indices'].tolist()}, margins {np.array2string(want['margins'], precision=3)}")
    assert np.all(want["margins"] > 1e-6), "the arg-max must be a property of the data"
    before = o.last_setting_index
    xs = o.opt_setting_batch(n, **kw)
    report = o.last_batch_design
    assert o.last_setting_index == before
    assert set(report) == {"indices", "utility", "variance_left", "prior_variance", "dims", "weights"}
    assert_array_equal(report["indices"], want["indices"])
    assert report["indices"].dtype == np.int64 and report["dims"] == tuple(rows) and report["weights"].tolist() == a.tolist()
    assert report["variance_left"].shape == (n, len(rows)) and report["prior_variance"].shape == (len(rows),)
    assert isinstance(xs, tuple) and len(xs) == grid.shape[0]
    for d in range(grid.shape[0]):
        assert_array_equal(xs[d], grid[d, want["indices"]])
    picks = want["indices"]
    nu_full = np.array(np.broadcast_to(np.asarray(nu, dtype=np.float64).reshape(joint.n_c, -1), (joint.n_c, joint.n_x)))
    _note("V end to end", np.abs(report["prior_variance"] - joint.V), joint.tol_V, what)
    # variance_left and the utility of every pick against the direct solve
    terms, step_tol, tols = joint.V.copy(), np.zeros(len(rows)), [oracle.end_to_end_tolerance(joint, nu, [], joint.V)]
    for j in range(n):
        G_pick = want["G"][j][:, picks[j]]
        terms = terms + np.abs(G_pick)
        step_tol = step_tol + want["tol_G"][j][:, picks[j]]         # the gain of pick j from S and K within their tolerances
        left, cond = oracle.direct(joint, nu, picks[:j + 1])[:2]
        assert cond <= 1e3, cond
        tols.append(oracle.end_to_end_tolerance(joint, nu, picks[:j + 1], terms) + step_tol)
        _note("variance_left end to end", np.abs(report["variance_left"][j] - left), tols[-1], f"{what}, pick {j}")
        G_dir = oracle.direct_gain(joint, nu, picks[:j], picks[j])
        cost_j = cost if np.ndim(cost) == 0 else cost[picks[j]]
        u_dir = oracle.utility(G_dir[:, None], joint.V, a, cost_j)[0]
        _note("U end to end", abs(report["utility"][j] - u_dir),
              oracle.utility_tolerance(tols[-2] + tols[-1], G_dir, joint.V, joint.tol_V, a, cost_j), f"{what}, pick {j}")
    assert np.all(np.diff(np.vstack([report["prior_variance"], report["variance_left"]]), axis=0) <= 0)
    # the two identities on the device: Vleft by the T rows after n - 1 picks against the gain route and the direct solve
    rep2, state = _design.plan_interest(o, n, tuple(rows), a, kw.get("sigma"), distinct)
    for k in ("indices", "utility", "variance_left"):
        assert_array_equal(_bits(rep2[k]), _bits(report[k]))
    assert state.rows_done == (n - 1) * joint.n_c
    if n > 1:
        by_T = state.pvar_left.cpu().numpy()
        rec = 1e-10 * want["state"]["terms_left"]
        _note("Vleft by T against the direct solve", np.abs(by_T - oracle.direct(joint, nu, picks[:n - 1])[0]),
              oracle.end_to_end_tolerance(joint, nu, picks[:n - 1], want["state"]["terms_left"]), what)
        _note("Vleft by T against the gains", np.abs(by_T - report["variance_left"][n - 2]),
              rec + 1e-10 * (terms - np.abs(want["G"][n - 1][:, picks[n - 1]])) + step_tol - want["tol_G"][n - 1][:, picks[n - 1]],
              what)
    return report, want


@pytest.mark.parametrize("case", sorted(CASES))
def test_batch_design_is_the_oracles(hip, case):
    name, seed, n, sigma, interest, weights = CASES[case]
    cloud, w = _design_case(name, seed)
    o = tp._object(name, cloud, w)
    nu = np.square(np.array(sigma))[:, None]
    rows = _interest.check_dims(interest, o.n_dims)
    a = _interest.check_weights(weights, len(rows))
    report, _ = _compare_design(case, o, w, n, nu, rows, a, key=case.partition(",")[0], sigma=np.array(sigma) if len(sigma) > 1 else sigma[0], interest=interest,
                    interest_weights=weights)
    if "twice" in case:
        assert len(set(report["indices"].tolist())) < n



def test_the_batch_for_the_centre_is_not_the_batch_for_the_background(hip):
    """x0 is learnt on the flanks of the peak, the background far from it; the output-variance design is neither."""
    name, seed, n, sigma = "lorentz1", 2, 6, 500.0
    cloud, w = _design_case(name, seed)
    o = tp._object(name, cloud, w, default_noise_std=sigma)
    nu = np.array([[sigma ** 2]])
    centre, _ = _compare_design("x0, the model's noise", o, w, n, nu, (0,), [1.0], key="x0", interest=0)
    centre = centre["indices"].copy()
    back, _ = _compare_design("background, the model's noise", o, w, n, nu, (2,), [1.0], key="background", interest=[2])
    x = np.asarray(o.allsettings)[0]
    assert set(centre.tolist()) != set(back["indices"].tolist())
    assert set(back["indices"].tolist()) == {0, 32} and np.all((x[centre] > 2.0) & (x[centre] < 4.0))
    # interest=True is the object's own choice; weights for this call only
    o.set_parameters_of_interest([0, 1], [1.0, 0.5])
    _compare_design("x0 and amplitude, the object's choice", o, w, n, nu, (0, 1), [1.0, 0.5], key="x0 and amplitude",
                              interest=True)
    o.opt_setting_batch(n, interest=True, interest_weights=[1.0, 0.0])
    assert o.last_batch_design["indices"].tolist() == centre.tolist() and o.parameters_of_interest[1].tolist() == [1.0, 0.5]
    # the call is independent of utility_method
    other = tp._object(name, cloud, w, utility_method="variance_full", default_noise_std=sigma)
    other.opt_setting_batch(n, interest=0)
    assert_array_equal(_bits(other.last_batch_design["utility"]), _bits(o_report(o, n, 0)["utility"]))


def o_report(o, n, interest, **kw):
    o.opt_setting_batch(n, interest=interest, **kw)
    return o.last_batch_design


def _per_setting(n_x):
    """(factor of the noise variance (1, n_x), cost (n_x,)) of the per-setting case."""
    g = np.random.default_rng(38)
    return 1.0 + g.random((1, n_x)), 1.0 + g.random(n_x)


def test_distinct_noise_and_cost_per_setting(hip):
    name, seed, n, sigma = "lorentz1", 2, 6, 500.0
    cloud, w = _design_case(name, seed)
    o = tp._object(name, cloud, w, default_noise_std=sigma)
    nu = np.array([[sigma ** 2]])
    plain, _ = _compare_design("background again", o, w, n, nu, (2,), [1.0], key="background", interest=2)
    assert len(set(plain["indices"].tolist())) < n
    plain = plain["indices"].copy()
    report, _ = _compare_design("distinct", o, w, n, nu, (2,), [1.0], key="background", interest=2, distinct=True)
    assert len(set(report["indices"].tolist())) == n and report["indices"][:2].tolist() == plain[:2].tolist()
    # per-setting noise and an overridden cost_estimate() array
    factor, cost = _per_setting(33)
    nv = nu * factor
    o.yvar_noise_model = lambda: nv
    o.cost_estimate = lambda: cost
    _compare_design("noise and cost per setting", o, w, n, nv, (0,), [1.0], cost, key="x0", interest=0)
    # sigma given: a scalar, and per setting
    _compare_design("sigma given", o, w, 4, np.array([[1000.0 ** 2]]), (2,), [1.0], cost, key="background", sigma=1000.0, interest=2)
    sg = np.sqrt(nv)
    _compare_design("sigma per setting", o, w, 4, sg * sg, (0, 1), [1.0, 0.5], cost, key="x0 and amplitude", sigma=sg,
                    interest=(0, 1), interest_weights=(1.0, 0.5))


def _noise_prior(n=3000):
    """(cloud, weights) of the noise-parameter case: seven peaks, the noise in row 9 (test_gpu_design's)."""
    g = np.random.default_rng(39)
    prior = np.vstack([g.uniform(2, 4, (7, n)), g.uniform(400, 2000, (1, n)), g.normal(500, 1000, (1, n)),
                       g.uniform(1000, 2000, (1, n))])
    return prior, tp._general_weights(g, prior)


def test_noise_parameter_design_and_refusals(hip):
    import optbayesexpt_amd as obe
    g = np.random.default_rng(40)
    prior, w = _noise_prior()
    o = obe.OptBayesExptNoiseParameter(obe.models.lorentzian(7), tp._design("lorentz7"), prior, (0.1,),
                                       noise_parameter_index=9, scale=False)
    o.particle_weights = w
    nu = np.asarray(o.yvar_noise_model()).reshape(1, 1)
    assert 1000.0 ** 2 < nu[0, 0] < 2000.0 ** 2
    _compare_design("noise parameter", o, w, 4, nu, (7, 8), [1.0, 1.0], interest=[7, 8])
    # refusals
    with pytest.raises(ValueError, match="at least 1"):
        o.opt_setting_batch(0, interest=0)
    with pytest.raises(ValueError, match="128"):
        o.opt_setting_batch(129, interest=0)
    with pytest.raises(ValueError, match="finite and > 0"):
        o.opt_setting_batch(2, sigma=np.inf, interest=0)
    with pytest.raises(ValueError, match="outside"):
        o.opt_setting_batch(2, interest=10)
    with pytest.raises(ValueError, match="pass interest"):
        o.opt_setting_batch(2, interest_weights=[1.0])
    host = obe.OptBayesExpt(lambda s, p, c: p[0] + p[1] * s[0], (np.arange(3.0),), g.normal(size=(2, 100)), ())
    with pytest.raises(TypeError, match="from_function.*from_expression"):
        host.opt_setting_batch(2, interest=0)
    assert host.last_batch_design is None
    s = cases.build("sweeper")
    with pytest.raises(TypeError, match="intervals"):
        s.opt_setting_batch(2, interest=0)
    # no finite utility left: three settings, four distinct picks
    tiny = obe.OptBayesExpt(obe.models.lorentzian(), (np.array([2.5, 3.0, 3.5]),), prior[[0, 7, 8]], (0.1,), scale=False)
    assert len(tiny.opt_setting_batch(3, sigma=100.0, distinct=True, interest=0)[0]) == 3
    with pytest.raises(ValueError, match="pick 3"):
        tiny.opt_setting_batch(4, sigma=100.0, distinct=True, interest=0)
    # 128 scalar readings: the limit itself runs, and the variance left never rises
    assert len(tiny.opt_setting_batch(128, sigma=100.0, interest=[0, 1])[0]) == 128
    assert np.all(np.diff(tiny.last_batch_design["variance_left"], axis=0) <= 0)
    assert np.all(tiny.last_batch_design["variance_left"][-1] > 0)


def test_a_row_without_variance_contributes_nothing(hip):
    """Weights of the form integer / 2^m and a row that is -1024 in every particle: its weighted mean is -1024 exactly,
    V_d == 0 and K_d == 0 exactly, and the design is the other row's, bit for bit, whatever weight the row has."""
    g = np.random.default_rng(55)
    cloud, _ = _design_case("lorentz1", 2)
    cloud[1] = -1024.0
    w = tp._dyadic_weights(g, 3000)
    o = tp._object("lorentz1", cloud, w, default_noise_std=500.0)
    alone = dict(o_report(o, 4, [0]))
    both = o_report(o, 4, [0, 1], interest_weights=[1.0, 7.0])
    assert both["prior_variance"][1] == 0.0 and np.all(both["variance_left"][:, 1] == 0.0)
    assert_array_equal(both["indices"], alone["indices"])
    assert_array_equal(_bits(both["utility"]), _bits(alone["utility"]))
    assert_array_equal(_bits(both["variance_left"][:, 0]), _bits(alone["variance_left"][:, 0]))
    assert np.all(np.isfinite(both["utility"])) and np.all(both["utility"] > 0)


# ------------------------------------------------------------------------------------------------- 4. state
def test_the_plain_design_is_untouched_and_nothing_of_the_object_changes(hip):
    o = cases.build("lorentz_full")
    cases.run(o, "lorentz_full", 0, 4)
    before = tp._flags(o), o.sweep_state(), o.last_setting_index
    xs = o.opt_setting_batch(4)
    plain = dict(o.last_batch_design)
    assert set(plain) == {"indices", "utility", "information"}
    o.opt_setting_batch(4, interest=0)
    assert "information" not in o.last_batch_design
    assert (tp._flags(o), o.sweep_state(), o.last_setting_index) == before
    for kw in ({}, dict(interest=None), dict(interest=False)):
        again = o.opt_setting_batch(4, **kw)
        assert_array_equal(_bits(again[0]), _bits(xs[0]))
        assert set(o.last_batch_design) == set(plain)
        for k in plain:
            assert_array_equal(_bits(o.last_batch_design[k]), _bits(plain[k]))
    # the picks feed pdf_update_batch as they are
    xs = o.opt_setting_batch(3, interest=0)
    o.pdf_update_batch(xs, np.full(3, 48000.0), cases.SIGMA)


@pytest.mark.parametrize("case", ["lorentz_full", "noise7"])
def test_a_trajectory_is_the_same_with_and_without_interest_designs(hip, case):
    """12 cycles, the sweep enqueued ahead (lorentz_full) and a noise parameter (noise7): bit-equal with and without
    opt_setting_batch(3, interest=...) before and after every opt_setting()."""
    plain = cases.build(case)
    picks, resampled = cases.run(plain, case, 0, 12)
    o = cases.build(case)
    got, flags = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for cyc in range(12):
            o.opt_setting_batch(3, interest=0)                  # (lorentz_full: the sweep enqueued behind the last update is pending)
            x = o.opt_setting()
            got.append(int(o.last_setting_index))
            o.opt_setting_batch(3, interest=[1, 0], interest_weights=[2.0, 1.0])
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
    o.set_parameters_of_interest([0, 2], [1.0, 0.25])
    assert o.last_batch_design is None
    want = o.opt_setting_batch(5, interest=True)
    report = o.last_batch_design
    assert report is not None and report["dims"] == (0, 2)
    path = tmp_path / "o.state"
    obe.save(o, str(path))
    for other in (copy.deepcopy(o), pickle.loads(pickle.dumps(o)), obe.load(str(path))):
        assert other.last_batch_design is None
        assert_array_equal(other.opt_setting_batch(5, interest=True)[0], want[0])
        assert other.last_batch_design["dims"] == report["dims"]
        for k in ("indices", "utility", "variance_left", "prior_variance", "weights"):
            assert_array_equal(_bits(other.last_batch_design[k]), _bits(report[k]))


# ----------------------------------------------------------------------------------------------- 5. example
def test_batch_design_interest_example(hip, capsys):
    spec = importlib.util.spec_from_file_location("batch_design_interest",
                                                  os.path.join(ROOT, "examples", "batch_design_interest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(n_batch=6, n_samples=3000, seed=0)
    text = capsys.readouterr().out
    assert "a batch for x0" in text and "a batch for  b" in text and "variance left / prior variance" in text
    (centre, left_c), (back, left_b) = out["x0"], out["b"]
    assert centre.shape == back.shape == (6,) and set(centre.tolist()) != set(back.tolist())
    for left in (left_c, left_b):
        assert np.all(np.diff(left) < 0) and 0 < left[-1] < left[0] < 1


# ------------------------------------------------------------------------------------------------ 6. figures
def test_worst_errors_are_reported(hip):
    """(runs last: the worst error / tolerance ratios seen by this file's comparisons)"""
    for kind, (ratio, what) in sorted(WORST.items()):
        print(f"worst {kind}: {ratio:.3g} ({what})")
    assert {"S of the step", "K of the step", "Vleft of the step", "T of the step", "G of the step", "U of the step",
            "V end to end", "variance_left end to end", "U end to end", "Vleft by T against the direct solve",
            "Vleft by T against the gains"} <= set(WORST)
