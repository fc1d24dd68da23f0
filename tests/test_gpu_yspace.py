"""The y-space kernels of the non-default utilities (max_min, pseudo_utility, full_kld_utility) at the C ABI (GPU):
obe_eval_draws, obe_yspace_add_noise, obe_yspace_maxmin, obe_yspace_variance, obe_yspace_entropy, obe_kld_utility —
each against the oracle's plain restatement (oracle.spacing_entropy & co., pinned on the CPU against scipy and a
50-digit evaluation in tests/test_oracle_golden.py) at every estimator branch and switch, ragged and grid-stride
column counts, the 8-draw load groups, degenerate columns and the limits; then through the classes at large N_DRAWS.

Tolerances are derived (tests/_replay.py: entropy_tolerance), not measured; -inf, +inf and NaN compare exactly."""
import ctypes

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _replay
from _replay import EPS, assert_entropy, assert_entropy_variance, entropy_tolerance
import oracle
from oracle import models as omodels

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
SENTINEL = -7.25                       # what output buffers are pre-filled with: no kernel result here equals it
GRID_NS = 300001                       # x 2 channels = 600 002 columns > 2048 blocks x 256 threads = 524 288
ENTROPY_DRAWS = [5, 6, 9, 10, 11, 12, 16, 30, 31, 100, 999, 1000, 1001, 1024, 2047, 2048]
REDUCE_DRAWS = [1, 2, 7, 8, 9, 15, 16, 17, 30, 257]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    import torch
    return P(torch.cuda.current_stream().cuda_stream)


def _filled(shape):
    import torch
    return torch.full(tuple(shape), SENTINEL, dtype=torch.float64, device="cuda")


def _columns(g, n, cols, ordered=True):
    """(n, cols) y-space: normal draws with a per-column scale 10^k, k in [-6, 6], on a per-column offset up to
    1e3 (spacings small against the values); column 0 already sorted, column 1 reverse-sorted if ``ordered``."""
    y = g.standard_normal((n, cols)) * 10.0 ** g.uniform(-6.0, 6.0, cols) + g.uniform(-1e3, 1e3, cols)
    if ordered:
        y[:, 0] = np.sort(y[:, 0])
        y[:, 1] = np.sort(y[:, 1])[::-1]
    return y


def _entropy(hip, y, as_variance):
    """obe_yspace_entropy on a (n, ...) host array: the output (pre-filled with SENTINEL) as a host array."""
    import torch
    n, cols = y.shape[0], y[0].size
    yd = _dev(y)
    scratch = torch.empty(n * cols, dtype=torch.float64, device="cuda")
    out = _filled(y.shape[1:])
    hip.call("obe_yspace_entropy", P(yd.data_ptr()), n, cols, as_variance, P(scratch.data_ptr()), P(out.data_ptr()),
             _stream())
    got = out.cpu().numpy()
    assert_array_equal(yd.cpu().numpy(), y)                       # the input is read only
    return got


def _check_entropy(hip, y, what, forms=(0, 1)):
    """Both forms of the kernel on y against the oracle; returns the oracle's H."""
    n = y.shape[0]
    h, scale = oracle.spacing_entropy(y, axis=0, with_log_scale=True)
    tol = entropy_tolerance(n, h, scale)
    for as_variance in forms:
        got = _entropy(hip, y, as_variance)
        if as_variance:
            worst = assert_entropy_variance(got, h, tol, f"{what}, variance form")
        else:
            worst = assert_entropy(got, h, tol, f"{what}, H")
        print(f"{what}, as_variance = {as_variance}: worst error / tolerance {worst:.3f}")
    return h


# ------------------------------------------------------------------ entropy: every estimator, switch and window
@pytest.mark.parametrize("n", ENTROPY_DRAWS)
def test_entropy_every_estimator_branch(hip, n):
    """van Es (n <= 10), Ebrahimi (n <= 1000, windows m = 3 ... 32 with their boundary terms c_i), Vasicek (n > 1000)
    and both switches, against oracle.spacing_entropy.  4099 columns (257 from n = 999 on: the insertion sort costs
    ~n^2 / 4 strided shifts per column), scales 1e-6 ... 1e6 on offsets up to 1e3 in one launch; a sorted and a
    reverse-sorted column (best and worst case of the sort) up to n = 1001.

    Both sides form the argument of every logarithm by the same IEEE operations in the same order — (n+1)/m * d,
    n * d / (c_i m), n/(2m) * d — so the arguments are bit-equal; the tolerance (_replay.entropy_tolerance) covers
    the device's log and its serial float64 sum, nothing else."""
    g = np.random.default_rng(9000 + n)
    cols = 257 if n >= 999 else 4099
    y = _columns(g, n, cols, ordered=n <= 1001)
    h = _check_entropy(hip, y, f"n = {n}, {cols} columns")
    assert np.all(np.isfinite(h))


@pytest.mark.parametrize("n", [9, 30, 1001])
def test_entropy_of_tied_draws_is_minus_infinity(hip, n):
    """Tied draws (a cloud with a few heavy particles): a zero spacing gives log 0 = -inf, H = -inf exactly and the
    variance form exactly 0.0, as scipy returns.  Columns of integers {0, 1, 2} with one value filling a whole window,
    and columns of distinct values in which exactly ONE window is tied (m + 1 copies for van Es, 2 m + 1 otherwise);
    untied neighbours in the same launch are compared as usual."""
    g = np.random.default_rng(n)
    m = int(np.floor(np.sqrt(n) + 0.5))
    run = m + 1 if n <= 10 else 2 * m + 1
    cols = 67
    y = _columns(g, n, cols, ordered=False)
    tied = np.arange(0, cols, 3)
    y[:, tied] = g.integers(0, 3, (n, tied.size)).astype(np.float64)
    y[:run, tied] = 1.0
    one = np.arange(1, cols, 3)                       # one tied window in the interior of the sorted column
    for c in one:
        order = np.argsort(y[:, c])
        lo = (n - run) // 2
        y[order[lo:lo + run], c] = y[order[lo], c]
    for c in np.concatenate([tied, one]):
        y[:, c] = g.permutation(y[:, c])
    h = _check_entropy(hip, y, f"ties, n = {n}")
    assert np.all(h[tied] == -np.inf) and np.all(h[one] == -np.inf) and np.all(np.isfinite(h[2::3]))
    assert np.all(_entropy(hip, y, 1)[np.concatenate([tied, one])] == 0.0)


@pytest.mark.parametrize("n", [9, 30, 1001])
def test_entropy_of_columns_with_nan_or_infinity(hip, n):
    """A NaN anywhere in a column gives NaN (scipy: NaN), also next to an infinity; one +inf alone gives H = +inf
    and one -inf alone H = +inf as well (an infinite spacing; scipy 1.15 returns the same) — whatever the oracle,
    pinned against scipy, returns, bit for bit.  The neighbouring columns are untouched and compared as usual."""
    g = np.random.default_rng(50 + n)
    y = _columns(g, n, 64, ordered=False)
    y[3, 5] = np.nan
    y[n - 2, 17] = np.inf
    y[0, 40], y[n - 1, 40] = np.inf, np.nan
    y[n // 2, 41] = -np.inf
    y[n - 1, 63] = np.nan
    h = _check_entropy(hip, y, f"NaN / inf, n = {n}")
    assert np.isnan(h[5]) and np.isnan(h[40]) and np.isnan(h[63]) and h[17] == np.inf and h[41] == np.inf
    assert int(np.sum(np.isfinite(h))) == 64 - 5


@pytest.mark.parametrize("n", [9, 30, 1001])
def test_entropy_at_denormal_and_1e300_scale(hip, n):
    """Spacings in the subnormal range and values of 1e300: H is finite on both (no overflow in n * d / (c_i m)
    — n * d stays below 1e304 — and no flush to zero of a subnormal spacing, which would be a tie)."""
    g = np.random.default_rng(70 + n)
    y = g.standard_normal((n, 96))
    y[:, :32] *= 5e-310
    y[:, 32:64] *= 1e300
    h = _check_entropy(hip, y, f"extreme scales, n = {n}")
    assert np.all(np.isfinite(h)) and np.all(h[:32] < -700.0) and np.all(h[32:64] > 680.0)


# ------------------------------------------------------------------ the grid-stride loop
@pytest.fixture(scope="module")
def grid_yspace():
    """(30, 2, 300 001): 600 002 columns, 76 290 of them served by the second trip of the grid-stride loop."""
    return _columns(np.random.default_rng(77), 30, 2 * GRID_NS, ordered=False).reshape(30, 2, GRID_NS)


def _second_trip_written(out, what):
    assert not np.all(out.reshape(-1)[-80000:] == SENTINEL), f"{what}: the last 80 000 columns were never written"


@pytest.mark.parametrize("n", [11, 30])
def test_entropy_beyond_one_grid(hip, grid_yspace, n):
    """600 002 columns: every column against the oracle, i.e. also the kernel's (n, row) scratch layout at a row
    of that size and the columns that only the loop's second trip reaches."""
    y = grid_yspace[:n]
    h, scale = oracle.spacing_entropy(y, axis=0, with_log_scale=True)
    got = _entropy(hip, y, 0)
    _second_trip_written(got, f"entropy, n = {n}")
    worst = assert_entropy(got, h, entropy_tolerance(n, h, scale), f"entropy of 600 002 columns, n = {n}")
    print(f"n = {n}, 600 002 columns: worst error / tolerance {worst:.3f}")


def test_reductions_noise_and_kld_beyond_one_grid(hip, grid_yspace):
    """obe_yspace_maxmin, obe_yspace_variance, obe_yspace_add_noise and obe_kld_utility on (9, 2, 300 001): every
    element, and the second trip's share of the output is not the sentinel it was filled with."""
    y = grid_yspace[:9]
    nd, c, ns = y.shape
    yd = _dev(y)
    out = _filled((c, ns))
    hip.call("obe_yspace_maxmin", P(yd.data_ptr()), nd, c * ns, P(out.data_ptr()), _stream())
    got = out.cpu().numpy()
    _second_trip_written(got, "max-min")
    assert_array_equal(got, oracle.yspace_maxmin(y))
    out = _filled((c, ns))
    hip.call("obe_yspace_variance", P(yd.data_ptr()), nd, c, ns, P(out.data_ptr()), _stream())
    got = out.cpu().numpy()
    _second_trip_written(got, "variance")
    _assert_variance(got, y, "variance of 600 002 columns")
    g = np.random.default_rng(78)
    noise = g.normal(0.0, 3.0, (nd, c))
    nz = _dev(noise)
    hip.call("obe_yspace_add_noise", P(yd.data_ptr()), nd, c, ns, P(nz.data_ptr()), _stream())
    assert_array_equal(yd.cpu().numpy(), y + noise[:, :, None])               # one IEEE add per element
    h_y, h_n = _kld_inputs(g, c, ns)
    got = _kld(hip, h_y, h_n)
    _second_trip_written(got, "KLD utility")
    _assert_kld(got, h_y, h_n, "KLD utility of 600 002 columns")


# ------------------------------------------------------------------ max-min and variance: the 8-draw load groups
def _assert_variance(got, y, what):
    """np.var(axis=0) adds the draws in order, like the kernel (same mean, same deviations; only the association of
    the squares' sum may differ).  A float64 two-pass variance of samples near `mean` is good to a few eps of
    var + eps mean^2 (the deviations y - mean are each rounded to eps |mean|): rtol 1e-13 of that."""
    ref = oracle.yspace_variance(y)
    assert got.shape == ref.shape
    tol = 1e-13 * (ref + EPS * np.mean(y, axis=0) ** 2)
    err = np.abs(got - ref)
    k = np.unravel_index(int(np.argmax(err - tol)), err.shape)
    assert np.all(err <= tol), f"{what}: column {k}: got {got[k]!r}, reference {ref[k]!r}, tolerance {tol[k]:.3g}"


@pytest.mark.parametrize("nd", REDUCE_DRAWS)
def test_maxmin_and_variance_at_every_load_group_size(hip, nd):
    """Both kernels load the draws eight at a time and repeat the last draw to fill a group (max-min from draw 1,
    the variance from draw 0): one draw, full groups, one draw more or fewer than full groups; 4099 columns.
    Max-min: exactly (max - min)^2 — a comparison rounds nothing; one draw gives 0.0."""
    g = np.random.default_rng(300 + nd)
    cols = 4099
    y = _columns(g, nd, cols)
    yd = _dev(y)
    out = _filled((cols,))
    hip.call("obe_yspace_maxmin", P(yd.data_ptr()), nd, cols, P(out.data_ptr()), _stream())
    got = out.cpu().numpy()
    assert_array_equal(got, oracle.yspace_maxmin(y))
    if nd == 1:
        assert not got.any()
    else:
        # the extremes in EVERY position of the draw axis (the last draw is the one a clamped group repeats)
        for pos in range(nd):
            y2 = y[:, :64].copy()
            y2[pos] = 1e9
            y2[(pos + 1) % nd] = -1e9
            o2 = _filled((64,))
            y2d = _dev(y2)
            hip.call("obe_yspace_maxmin", P(y2d.data_ptr()), nd, 64, P(o2.data_ptr()), _stream())
            assert_array_equal(o2.cpu().numpy(), np.full(64, 4e18))
    out = _filled((cols,))
    hip.call("obe_yspace_variance", P(yd.data_ptr()), nd, 1, cols, P(out.data_ptr()), _stream())
    got = out.cpu().numpy()
    _assert_variance(got, y, f"variance over {nd} draws")
    if nd == 1:
        assert not got.any()
    # two channels: the same numbers, (C, N_s) is one row of C * N_s columns
    y2 = np.ascontiguousarray(y[:, :cols - 1])
    out = _filled((cols - 1,))
    y2d = _dev(y2)
    hip.call("obe_yspace_variance", P(y2d.data_ptr()), nd, 2, (cols - 1) // 2, P(out.data_ptr()), _stream())
    _assert_variance(out.cpu().numpy(), y2, f"variance over {nd} draws, two channels")


def test_maxmin_leaves_the_columns_next_to_a_nan_alone(hip):
    """A NaN model output is outside the max-min kernel's declared domain: no value is asserted for that column,
    but the columns around it are exact."""
    g = np.random.default_rng(5)
    y = _columns(g, 30, 515)
    y[7, 100] = np.nan
    out = _filled((515,))
    yd = _dev(y)
    hip.call("obe_yspace_maxmin", P(yd.data_ptr()), 30, 515, P(out.data_ptr()), _stream())
    keep = np.arange(515) != 100
    assert_array_equal(out.cpu().numpy()[keep], oracle.yspace_maxmin(y[:, keep]))


# ------------------------------------------------------------------ eval_draws, add_noise, KLD with C > 1
def _kld_inputs(g, c, ns, near_zero=False):
    """Entropies as obe_kld_utility sees them: H_noise per channel and H_y = H_noise + d with |d| in 0.5 ... 30
    of either sign (or, ``near_zero``, |d| down to 1e-9: settings that tell nothing)."""
    h_n = g.normal(0.0, 3.0, c)
    d = g.uniform(0.5, 30.0, (c, ns)) if not near_zero else 10.0 ** g.uniform(-9.0, -0.4, (c, ns))
    d *= g.choice([-1.0, 1.0], (c, ns))
    return h_n[:, None] + d, h_n


def _kld(hip, h_y, h_n):
    """obe_kld_utility on host arrays h_y (C, N_s), h_n (C,): the output, pre-filled with SENTINEL."""
    c, ns = h_y.shape
    hyd, hnd, out = _dev(h_y), _dev(h_n), _filled((c, ns))
    hip.call("obe_kld_utility", P(hyd.data_ptr()), c, ns, P(hnd.data_ptr()), P(out.data_ptr()), _stream())
    return out.cpu().numpy()


def _assert_kld(got, h_y, h_n, what, exp_scale=False):
    """exp(H_y - H_n[c]) - 1 against the oracle's: relative 4 eps plus 4 eps |H_y - H_n| absolute (the difference
    and the subtraction are the same IEEE operations on both sides; the device's exp is what differs).  That bound
    is stated relative to the RESULT; where H_y - H_n is near zero the result cancels and an ulp of exp(.) ~ 1 —
    all that either side can promise — is far larger than it, so ``exp_scale`` (the near-zero case only) states
    the same 4 eps relative to exp(H_y - H_n) = result + 1 instead."""
    ref = oracle.kld_utility(h_y, h_n)
    assert got.shape == ref.shape
    d = np.abs(h_y - h_n[:, None])
    tol = 4 * EPS * (np.abs(ref) + 1.0 if exp_scale else np.abs(ref)) + 4 * EPS * d
    err = np.abs(got - ref)
    k = np.unravel_index(int(np.argmax(err / tol)), err.shape)
    assert np.all(err <= tol), f"{what}: element {k}: got {got[k]!r}, reference {ref[k]!r}, tolerance {tol[k]:.3g}"


def _model_cases(obe):
    g = np.random.default_rng(2024)
    n = 2048
    coil = np.array([g.uniform(0.9, 1.1, n), g.uniform(0.08, 0.12, n), g.uniform(0.9, 1.1, n), g.exponential(0.3, n)])
    rabi = np.array([g.uniform(1.0, 6.0, n), g.uniform(-4, 4, n)])
    return {"coil": (obe.models.coil(), omodels.coil, coil, (),
                     lambda ns: np.logspace(-1, 1, ns).reshape(1, ns) if ns > 1 else np.array([[0.7]])),
            "rabi": (obe.models.rabi(), omodels.rabi, rabi, (100000.0, 0.01, 2.0),
                     lambda ns: np.stack([g.uniform(0.02, 1.0, ns), g.uniform(-10.0, 10.0, ns)]))}


@pytest.mark.parametrize("ns", [1, 63, 4099])
@pytest.mark.parametrize("kind", ["coil", "rabi"])
def test_eval_draws_add_noise_and_kld_indexing(hip, kind, ns):
    """The (N_d, C, N_s) indexing of eval_draws_kernel, add_noise_kernel (noise[e / ns]) and kld_kernel
    (hn[e / ns]) with two channels (coil) and two setting dimensions (rabi): draw indices with repeats, particle 0
    and particle N - 1.  The y-space against the oracle's model per draw (rtol 1e-12, the bar of the exact-form
    evaluations elsewhere in the suite); the noise added exactly (one IEEE add); the KLD utility of per-channel
    entropies against exp(h_y - h_n[:, None]) - 1."""
    import optbayesexpt_amd as obe
    dm, fn, particles, cons, make_settings = _model_cases(obe)[kind]
    g = np.random.default_rng(ns)
    n = particles.shape[1]
    settings = make_settings(ns)
    nd = 41
    idx = g.integers(0, n, nd)
    idx[[0, 5, 6, 7, nd - 1]] = [0, n - 1, 17, 17, 17]
    c = dm.n_channels
    ref = np.empty((nd, c, ns))
    for d in range(nd):
        ref[d] = np.atleast_2d(fn(tuple(settings), particles[:, idx[d]], cons))
    out = _filled((nd, c, ns))
    sd, pd_, idd = _dev(settings), _dev(particles), _dev(idx.astype(np.int64))
    hip.call("obe_eval_draws", dm.struct(particles.shape[0], cons), P(sd.data_ptr()), ns, ns, P(pd_.data_ptr()), n, n,
             P(idd.data_ptr()), nd, P(out.data_ptr()), _stream())
    got = out.cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got - ref) / np.abs(ref)
    print(f"{kind}, {ns} settings: worst relative error of the y-space {err.max():.2e}")
    np.testing.assert_allclose(got, ref, rtol=1e-12)
    assert_array_equal(got[6], got[7])                                  # repeated draws: the same numbers
    noise = g.normal(0.0, 0.3, (nd, c))
    nz = _dev(noise)
    hip.call("obe_yspace_add_noise", P(out.data_ptr()), nd, c, ns, P(nz.data_ptr()), _stream())
    assert_array_equal(out.cpu().numpy(), got + noise[:, :, None])
    for near_zero in (False, True):
        h_y, h_n = _kld_inputs(g, c, ns, near_zero)
        _assert_kld(_kld(hip, h_y, h_n), h_y, h_n, f"KLD utility, {kind}, {ns} settings, near zero: {near_zero}",
                    exp_scale=near_zero)
    h_y = np.full((c, ns), -np.inf)                                      # tied draws: H_y = -inf -> utility -1
    assert_array_equal(_kld(hip, h_y, h_n), np.full((c, ns), -1.0))


# ------------------------------------------------------------------ the limits
def test_entropy_limits_at_the_abi(hip):
    """More than 2048 draws and windows with 2 m >= n (n <= 4) are refused with -1 and a message; nothing is
    launched (the output keeps what it held).  2048 draws are accepted (test_entropy_every_estimator_branch)."""
    import torch
    for n, words in [(2049, "2048"), (1, "window length"), (2, "window length"), (3, "window length"),
                     (4, "window length")]:
        y = _dev(np.random.default_rng(n).normal(size=(n, 8)))
        scratch = torch.empty(n * 8, dtype=torch.float64, device="cuda")
        out = _filled((8,))
        rc = hip.cdll.obe_yspace_entropy(P(y.data_ptr()), n, 8, 0, P(scratch.data_ptr()), P(out.data_ptr()), _stream())
        torch.cuda.synchronize()
        assert rc == -1 and words in hip.last_error(), (n, rc, hip.last_error())
        assert_array_equal(out.cpu().numpy(), np.full(8, SENTINEL))


def _lorentz_pair(obe, method, n_draws, seed=3):
    g = np.random.default_rng(seed)
    n, ns = 3000, 201
    prior = np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    sv = (np.linspace(1.5, 4.5, ns),)
    w = g.exponential(1.0, n) ** 2
    w /= w.sum()
    kw = dict(scale=False, auto_resample=False, utility_method=method, n_draws=n_draws, default_noise_std=500.0)
    a = obe.OptBayesExpt(obe.models.lorentzian(), sv, prior.copy(), (0.1,), **kw)
    b = oracle.OracleOptBayesExpt(omodels.lorentzian, sv, prior.copy(), (0.1,), **kw)
    for o in (a, b):
        o.particle_weights = w.copy()
    return a, b


def _coil_pair(obe, method, n_draws, seed=4):
    g = np.random.default_rng(seed)
    n, ns = 3000, 201
    prior = np.array([g.uniform(0.9, 1.1, n), g.uniform(0.08, 0.12, n), g.uniform(0.9, 1.1, n), g.exponential(0.3, n)])
    sv = (np.logspace(-1, 1, ns),)
    w = g.exponential(1.0, n) ** 2
    w /= w.sum()
    kw = dict(scale=False, auto_resample=False, utility_method=method, n_draws=n_draws, noise_parameter_index=(3, 3))
    a = obe.OptBayesExptNoiseParameter(obe.models.coil(), sv, prior.copy(), (), **kw)
    b = oracle.OracleOptBayesExptNoiseParameter(omodels.coil, sv, prior.copy(), (), **kw)
    for o in (a, b):
        o.particle_weights = w.copy()
    return a, b


@pytest.mark.parametrize("method", ["pseudo_utility", "full_kld_utility"])
def test_draw_counts_the_entropy_kernel_refuses_raise_before_anything_is_drawn(hip, method):
    """set_n_draws(3): scipy's ValueError, word for word (scipy >= 1.12 returns NaN with a RuntimeWarning there
    instead — seen with 1.15.3 — which is deliberately not followed: a utility of NaN at every setting would pick
    setting 0 silently).  set_n_draws(2049): a ValueError that names the 2048 limit.  Both BEFORE self.rng (or the
    module-level generator of full_kld) is touched, and the object goes on working with 30 draws."""
    import optbayesexpt_amd as obe
    import optbayesexpt_amd.obe_base as obe_base
    a, b = _lorentz_pair(obe, method, 30)
    a.rng, b.rng = np.random.default_rng(21), np.random.default_rng(21)
    obe_base.rng, b.noise_rng = np.random.default_rng(22), np.random.default_rng(22)
    state, noise_state = a.rng.bit_generator.state, obe_base.rng.bit_generator.state
    assert a.set_n_draws(3) == 3
    with pytest.raises(ValueError, match=r"Window length \(2\) must be positive and less than half the sample "
                                         r"size \(3\)\."):
        a.opt_setting()
    assert a.set_n_draws(2049) == 2049
    with pytest.raises(ValueError, match="2048"):
        a.opt_setting()
    with pytest.raises(ValueError, match="2048"):
        a.utility()
    assert a.rng.bit_generator.state == state and obe_base.rng.bit_generator.state == noise_state
    assert a.set_n_draws(30) == 30
    a.opt_setting()
    b.opt_setting()
    assert_array_equal(a.last_draw_indices, b.last_draw_indices)
    assert a.last_setting_index == b.last_setting_index
    assert a.rng.bit_generator.state == b.rng.bit_generator.state
    _replay.assert_rel(np.asarray(a.last_utility).reshape(-1), np.asarray(b.last_utility).reshape(-1), 1e-10,
                       f"{method} after the refused draw counts")


# ------------------------------------------------------------------ through the classes, large N_DRAWS
Y_RTOL = 1e-12        # what a device model's output is held to against the oracle's (test_eval_draws_... above)


def _class_reference(b, method):
    """Utility and its tolerance from the ORACLE's y-space of this call (b.last_yspace, b.last_noise) with the
    high-precision entropies.  What the device may differ by, propagated:
    * its model outputs, each within Y_RTOL |y| (full_kld: plus the noise value scaled by a noise variance that
      is itself good to 1e-12): a sample off by delta moves a spacing by 2 delta, H by 2 delta x the oracle's mean
      1 / spacing, and the span of max-min by 2 delta;
    * H itself within _replay.entropy_tolerance; exp(2H) turns tol_H into 2 tol_H relative, exp(H_y - H_n) into
      tol_Hy + tol_Hn relative to utility + 1;
    * the noise variance of the NoiseParameter class (a weighted mean over the cloud): 1e-12, the suite's bar for
      moments."""
    y = np.asarray(b.last_yspace)
    nd = y.shape[0]
    noise_var = np.asarray(b.yvar_noise_model(), dtype=np.float64).reshape(-1, 1)
    if method == "max_min":
        v = oracle.yspace_maxmin(y)
        delta = Y_RTOL * np.max(np.abs(y), axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(v > 0, 2.0 * (2.0 * delta) / np.sqrt(v), np.inf)
        ref = oracle.utility_from_yvar(v, noise_var, 1.0)
        return ref, np.sum(rel * v / noise_var, axis=0) + 1e-12 * ref
    h, scale, sens = oracle.spacing_entropy(y, axis=0, with_log_scale=True, with_sensitivity=True)
    if method == "pseudo_utility":
        tol_h = entropy_tolerance(nd, h, scale) + 2.0 * Y_RTOL * np.max(np.abs(y), axis=0) * sens
        v = oracle.entropy_variance(h)
        ref = oracle.utility_from_yvar(v, noise_var, 1.0)
        return ref, np.sum((2.0 * tol_h + 8 * EPS) * v / noise_var, axis=0) + 1e-12 * ref
    noise = np.asarray(b.last_noise)                                      # (N_d, C)
    delta = Y_RTOL * (np.max(np.abs(y - noise[:, :, None]), axis=0) + np.max(np.abs(noise), axis=0)[:, None])
    tol_hy = entropy_tolerance(nd, h, scale) + 2.0 * delta * sens
    hn, nscale = oracle.spacing_entropy(noise, axis=0, with_log_scale=True)
    tol_hn = entropy_tolerance(nd, hn, nscale) + 1e-12
    ref = oracle.kld_utility(h, hn)
    return ref, (ref + 1.0) * (tol_hy + tol_hn[:, None] + 4 * EPS * np.abs(h - hn[:, None]) + 8 * EPS)


@pytest.mark.parametrize("n_draws", [11, 200, 1001])
@pytest.mark.parametrize("method", ["pseudo_utility", "max_min", "full_kld_utility"])
@pytest.mark.parametrize("kind", ["lorentzian", "coil_noise_parameter"])
def test_classes_with_large_draw_counts(hip, kind, method, n_draws):
    """OptBayesExpt (Lorentzian) and OptBayesExptNoiseParameter (two-channel coil), 3000 particles with non-uniform
    weights, 201 settings, N_DRAWS = 11 | 200 | 1001 (Ebrahimi at its smallest window, a large one, Vasicek): the
    draw indices and the generator state equal the oracle class's, the utility agrees within the propagated
    tolerance (_class_reference), the chosen setting is the same.

    full_kld with two channels: the reference adds noisevalues[i] of shape (C,) to a (C, N_s) array, which
    broadcasts for one channel only, and its opt_setting() indexes the settings with the arg-max of the flattened
    (C, N_s) utility.  The library (and the oracle) give draw i, channel c its own noise value; utility() is
    compared there and the arg-max of the flattened array, not opt_setting()."""
    import optbayesexpt_amd as obe
    import optbayesexpt_amd.obe_base as obe_base
    a, b = (_lorentz_pair if kind == "lorentzian" else _coil_pair)(obe, method, n_draws)
    a.rng, b.rng = np.random.default_rng(n_draws), np.random.default_rng(n_draws)
    obe_base.rng, b.noise_rng = np.random.default_rng(n_draws + 2), np.random.default_rng(n_draws + 2)
    if method == "full_kld_utility" and kind != "lorentzian":
        ua, ub = np.asarray(a.utility()), np.asarray(b.utility())
        assert ua.shape == ub.shape == (2, 201)
        assert int(np.argmax(ua)) == int(np.argmax(ub))
    else:
        xa, xb = a.opt_setting(), b.opt_setting()
        assert a.last_setting_index == b.last_setting_index and xa == xb
        ua, ub = np.asarray(a.last_utility), np.asarray(b.last_utility)
    assert_array_equal(a.last_draw_indices, b.last_draw_indices)
    assert a.rng.bit_generator.state == b.rng.bit_generator.state
    assert obe_base.rng.bit_generator.state == b.noise_rng.bit_generator.state
    ref, tol = _class_reference(b, method)
    ua = ua.reshape(ref.shape)
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(tol))
    err = np.abs(ua - ref)
    k = np.unravel_index(int(np.argmax(err / tol)), err.shape)
    print(f"{kind}, {method}, {n_draws} draws: worst error / tolerance {err[k] / tol[k]:.3g} "
          f"(relative error {err[k] / abs(ref[k]):.2e}, relative tolerance {tol[k] / abs(ref[k]):.2e})")
    assert np.all(err <= tol), f"setting {k}: got {ua[k]!r}, reference {ref[k]!r}, tolerance {tol[k]:.3g}"
    # the oracle class itself (scipy's entropies) sits inside the same tolerance
    assert np.all(np.abs(ub.reshape(ref.shape) - ref) <= tol)
