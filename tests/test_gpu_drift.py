"""Parameter drift, the filter's prediction step (csrc/obe_drift.hip: drift_kernel<K, REFLECT>; ParticlePDF.drift,
OptBayesExpt.drift, set_parameter_drift).

(1) obe_drift_particles at the C ABI against tests/_drift_oracle.py, bit for bit — the contract is the chain of
operations include/obe_hip.h documents, so there is no tolerance —, with everything around the drifted rows checked
byte for byte; (2) ParticlePDF.drift() against NumPy's generator on the host and the device route of the normals;
(3) the statistics of a step and the cached moments; (4) OptBayesExpt: sweeps after a drift, per_update (also on the
signal-noise class and the sweeper), the noise-parameter class at its bound, save / load / deepcopy, a stale
``parameters`` alias; (5) examples/drifting_line.py.
tests/test_drift_host.py shows on the CPU that the inputs of (1) tell the contract from its neighbours."""
import copy
import ctypes
import functools
import math

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _drift_oracle as do

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
INF = np.inf
SENTINEL = -1.2345678901234567e123
PAD = 5                                      # ld_p = n + 5: the sentinel behind every row
MAX_BLOCKS, BLOCK = 2048, 256                # the grid cap of drift_kernel (csrc/obe_common.h: drift_blocks) x its workgroup
SECOND_TRIP = MAX_BLOCKS * BLOCK + BLOCK + 37    # one particle per thread: a second trip with a full and a ragged tile
ZIGGURAT_BODY = 3.6541528853610088           # |z| up to here: the ziggurat's body (tests/test_gpu_ziggurat.py)
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _host(a):
    return None if a is None else P(a.ctypes.data)


def _stream():
    import torch
    return P(torch.cuda.current_stream().cuda_stream)


def _padded(x, ld):
    d, n = x.shape
    padded = np.full((d, ld), SENTINEL)
    padded[:, :n] = x
    return padded


def drift_call(hip, x, rows, z, G, ld, lo=None, hi=None):
    """obe_drift_particles on a copy of ``x`` with leading dimension ``ld``: the whole (D, ld) array afterwards."""
    d, n = x.shape
    cloud, zd = _dev(_padded(x, ld)), _dev(z)
    rows, G = np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(G, dtype=np.float64)
    lo, hi = (None if b is None else np.ascontiguousarray(b, dtype=np.float64) for b in (lo, hi))
    hip.call("obe_drift_particles", P(cloud.data_ptr()), ld, d, n, _host(rows), _host(G), len(rows), P(zd.data_ptr()),
             _host(lo), _host(hi), _stream())
    return cloud.cpu().numpy()


def check_drift(hip, x, rows, z, G, want, what, lo=None, hi=None, lds=None):
    """The drifted rows are ``want``'s; the other rows and the padding columns keep their bytes."""
    n = x.shape[1]
    untouched = np.setdiff1d(np.arange(x.shape[0]), rows)
    _same(want[untouched], x[untouched], what + ": the oracle's own untouched rows")
    for ld in (n, n + PAD) if lds is None else lds:
        got = drift_call(hip, x, rows, z, G, ld, lo, hi)
        _same(got, _padded(want, ld), f"{what} ld_p={ld}")


# --------------------------------------------------------------------------------- (1) the C ABI, bit for bit
@functools.lru_cache(maxsize=None)
def general(k, n, d):
    inputs = do.general_case(k, n, d)
    want = do.drift_exact(*inputs)
    for a in inputs + (want,):
        a.setflags(write=False)
    return inputs, want


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("k", [1, 2, 3, 8, 16])
def test_general_doubles_are_the_exact_chain(hip, k, extra):
    """D = K (every row drifts) and D = K + 3 (non-adjacent rows); 1 .. 65: less than a wave, one, one particle more;
    255 .. 257: the same about a workgroup's tile — both branches of the LDS read of the normals; 1000: three full
    tiles and a ragged one."""
    for n in SIZES:
        inputs, want = general(k, n, k + extra)
        check_drift(hip, *inputs, want, f"K={k} D={k + extra} n={n}")


def test_a_wide_cloud_drifts_two_of_its_forty_rows(hip):
    for n in (257, 1000):
        inputs, want = general(2, n, 40)
        assert inputs[1].tolist() == [0, 39]
        check_drift(hip, *inputs, want, f"K=2 D=40 n={n}")


@pytest.mark.parametrize("k,d,n", [(1, 1, 1000), (3, 6, 1000), (16, 16, 1000), (2, 3, SECOND_TRIP)])
def test_on_exact_data_the_step_is_integer_arithmetic(hip, k, d, n):
    """Integers (|x| <= 2^20, |z|, |G| <= 8, G full): every order of evaluation gives NumPy's integer result.
    SECOND_TRIP: the grid is capped at 2048 workgroups of 256 threads, one particle each — 2048 * 256 + 293 particles
    take a second trip of the grid-stride loop, a full tile in workgroup 0, a ragged one in workgroup 1, none in the
    rest."""
    x, rows, z, G = do.integer_case(k, n, d)
    want = do.drift_integers(x, rows, z, G)
    check_drift(hip, x, rows, z, G, want, f"K={k} D={d} n={n} integers", lds=(n + PAD,) if n == SECOND_TRIP else None)


@pytest.mark.parametrize("k", [1, 2, 3, 8, 16])
def test_reflection_is_two_roundings_at_the_bound_crossed(hip, k):
    """An interval far narrower than the rows' spread: values pushed past lo, past hi, and most of them by more than
    the interval is wide (one reflection, no folding: they stay outside)."""
    n = 293
    x, rows, z, G = do.general_case(k, n, k + 3)
    lo, hi = do.reflection_interval(k)
    want = do.drift_exact(x, rows, z, G, lo, hi)
    plain = do.drift_exact(x, rows, z, G)
    assert np.count_nonzero(_bits(want) != _bits(plain)) >= 0.9 * k * n
    assert np.count_nonzero((want[rows] < lo[:, None]) | (want[rows] > hi[:, None])) >= 0.5 * k * n
    check_drift(hip, x, rows, z, G, want, f"K={k} reflecting", lo, hi)
    # one-sided and absent bounds
    one_sided_lo, one_sided_hi = np.where(np.arange(k) % 2 == 0, lo, -INF), np.where(np.arange(k) % 2 == 0, INF, hi)
    check_drift(hip, x, rows, z, G, do.drift_exact(x, rows, z, G, one_sided_lo, one_sided_hi), f"K={k} one-sided",
                one_sided_lo, one_sided_hi)
    check_drift(hip, x, rows, z, G, plain, f"K={k} infinite bounds", np.full(k, -INF), np.full(k, INF))


def test_reflection_of_crafted_values(hip):
    """x = 0, G = 1: v = z.  Past lo, past hi, past both by a step wider than the interval, exactly onto either bound
    (stays), inside, and NaN (left alone)."""
    z = np.array([[-0.25], [1.25], [-3.0], [5.5], [0.0], [1.0], [0.5], [np.nan]])
    want = np.array([[0.25, 0.75, 3.0, -3.5, 0.0, 1.0, 0.5, np.nan]])
    n = z.shape[0]
    x = np.zeros((2, n))
    x[1] = np.arange(n) + 0.5
    got = drift_call(hip, x, [0], z, [[1.0]], n + PAD, [0.0], [1.0])
    _same(do.reflect_two_roundings(z.T.copy(), [0.0], [1.0])[:, :-1], want[:, :-1], "the oracle on the crafted values")
    _same(got[0, :n - 1], want[0, :-1], "crafted values")
    assert np.isnan(got[0, n - 1])
    _same(got[1], _padded(x, n + PAD)[1], "the row that does not drift")
    _same(got[0, n:], np.full(PAD, SENTINEL), "the padding")
    # a NaN already in the cloud stays one, with or without bounds
    x[0, 3] = np.nan
    for bounds in ((None, None), ([0.0], [1.0])):
        got = drift_call(hip, x, [0], np.ones((n, 1)), [[1.0]], n, *bounds)
        assert np.isnan(got[0, 3]) and np.all(got[0, :3] == 1.0)


def test_refused_calls_launch_nothing(hip):
    from optbayesexpt_amd._lib import ObeHipError
    n, d = 293, 5
    x, _, z, _ = do.integer_case(3, n, d)
    ld = n + PAD
    before = _padded(x, ld)
    cloud, zd = _dev(before), _dev(z)
    rows = np.array([0, 2, 4], dtype=np.int32)
    G = np.ascontiguousarray(np.tril(np.ones((3, 3))))
    lo, hi = np.zeros(3), np.ones(3)
    big = np.arange(17, dtype=np.int32)
    good = dict(p=P(cloud.data_ptr()), ld=ld, d=d, n=n, rows=rows, G=G, k=3, z=P(zd.data_ptr()), lo=None, hi=None)

    def refused(message, **changed):
        a = dict(good, **changed)
        with pytest.raises(ObeHipError) as err:
            hip.call("obe_drift_particles", a["p"], a["ld"], a["d"], a["n"], _host(a["rows"]), _host(a["G"]), a["k"],
                     a["z"], _host(a["lo"]), _host(a["hi"]), _stream())
        assert err.value.refused_before_launch and message in hip.last_error(), hip.last_error()
        _same(cloud.cpu().numpy(), before, message + ": the cloud was written")

    def with_entry(a, i, v):
        a = np.array(a, dtype=np.float64)
        a.flat[i] = v
        return a

    refused("bad pointer", p=None)
    refused("bad pointer", rows=None)
    refused("bad pointer", G=None)
    refused("bad pointer", z=None)
    refused("bad pointer", n=0)
    refused("go together", lo=lo)
    refused("go together", hi=hi)
    refused("n_rows must be 1..16", k=0)
    refused("n_rows must be 1..16", k=17, rows=big, G=np.eye(17), d=40)
    refused("n_dims must be 1..1024", d=0)
    refused("n_dims must be 1..1024", d=1025)
    refused("row index out of range", rows=np.array([0, 2, 5], dtype=np.int32))
    refused("row index out of range", rows=np.array([-1, 2, 4], dtype=np.int32))
    refused("ascending", rows=np.array([0, 2, 2], dtype=np.int32))
    refused("ascending", rows=np.array([2, 0, 4], dtype=np.int32))
    refused("ld_p < n_particles", ld=n - 1)
    refused("factor entry not finite", G=with_entry(G, 3, np.nan))
    refused("factor entry not finite", G=with_entry(G, 8, INF))
    refused("NaN bound", lo=with_entry(lo, 1, np.nan), hi=hi)
    refused("NaN bound", lo=lo, hi=with_entry(hi, 2, np.nan))
    refused("lower > upper", lo=with_entry(lo, 0, 2.0), hi=hi)
    # ... and the good call goes through
    hip.call("obe_drift_particles", good["p"], ld, d, n, _host(rows), _host(G), 3, good["z"], None, None, _stream())
    _same(cloud.cpu().numpy(), _padded(do.drift_integers(x, rows, z, G), ld), "the call that is not refused")


# ------------------------------------------------------------------- (2) ParticlePDF.drift() against NumPy
@pytest.fixture(scope="module")
def obe(hip):
    import optbayesexpt_amd
    return optbayesexpt_amd


def _pdf_case(n, d, seed):
    g = np.random.default_rng(seed)
    return g.normal(0.0, 1.0, (d, n)) * np.arange(1, d + 1)[:, None]


Q3 = np.array([[0.04, 0.01, -0.02], [0.01, 0.09, 0.03], [-0.02, 0.03, 0.16]])


def _drifted_pdf(obe, n, device_rng, dt=0.7):
    """(object after one drift(dt), its reference generator after the same draws, x before, rows, z, G)."""
    x = _pdf_case(n, 5, 77 + n)
    o = obe.ParticlePDF(x.copy())
    if device_rng is not None:
        o.tuning_parameters["device_rng"] = device_rng
    o.rng = np.random.default_rng(4242)
    ref = np.random.default_rng(4242)
    assert o.rng.random(7).tolist() == ref.random(7).tolist()           # (not at the seed's first position)
    o.set_parameter_drift(Q3, rows=[4, 0, 2])                          # unsorted: rows 0, 2, 4 of Q3[[1, 2, 0]][:, [1, 2, 0]]
    drift = o.parameter_drift
    assert drift["rows"] == (0, 2, 4) and drift["per_update"] is False and drift["at_bounds"] == "mask"
    order = [1, 2, 0]
    _same(drift["cholesky"], np.linalg.cholesky(Q3[np.ix_(order, order)]), "the factor of the sorted covariance")
    w_before = np.array(o.particle_weights)
    assert o.drift(dt) is None
    z = ref.standard_normal((n, 3))
    G = drift["cholesky"] * math.sqrt(dt)
    _same(o.particle_weights, w_before, "the weights")
    return o, ref, x, np.array(drift["rows"]), z, G


def _same_generator(o, ref):
    assert o.rng.bit_generator.state == ref.bit_generator.state
    assert o.rng.random(5).tolist() == ref.random(5).tolist()


@pytest.mark.parametrize("n,device_rng", [(1000, None), (8192, False)])
def test_drift_with_host_normals_is_numpy_and_the_chain(obe, n, device_rng):
    """N K = 3000 < 4096 draws, and the device route switched off: rng.standard_normal((N, K)) on the host."""
    o, ref, x, rows, z, G = _drifted_pdf(obe, n, device_rng)
    _same(o.particles, do.drift_exact(x, rows, z, G), f"n={n} device_rng={device_rng}")
    _same_generator(o, ref)


def test_drift_with_device_normals_is_numpy_and_the_chain(obe):
    """N = 8192, K = 3: the generator continues on the device.  Particles whose normals all come from the ziggurat's
    body are the oracle's bits; a tail draw goes through another log1p on the device (test_device_rng_is_bitwise_numpy):
    one ulp of z through the chain, plus the roundings of the chain and of the final add."""
    n, k = 8192, 3
    o, ref, x, rows, z, G = _drifted_pdf(obe, n, None)
    _same_generator(o, ref)
    body = np.all(np.abs(z) <= ZIGGURAT_BODY, axis=1)
    assert np.count_nonzero(~body) <= 0.01 * n                          # (expected: K * 2.6e-4 of them)
    want = do.drift_exact(x, rows, z, G)
    got = np.array(o.particles)
    _same(got[:, body], want[:, body], "particles drawn from the ziggurat's body")
    untouched = np.setdiff1d(np.arange(5), rows)
    _same(got[untouched], x[untouched], "rows that do not drift")
    bound = 2.0 ** -52 * (k * (np.abs(G) @ np.abs(z[~body]).T) + np.abs(want[rows][:, ~body]))
    err = np.abs(got[rows][:, ~body] - want[rows][:, ~body])
    print(f"{np.count_nonzero(~body)} tail particles, largest error / bound {np.max(err / bound, initial=0.0):.3f}")
    assert np.all(err <= bound)


def test_drift_refusals_and_no_ops(obe):
    o = obe.ParticlePDF(_pdf_case(500, 3, 5))
    o.rng = np.random.default_rng(1)
    assert o.parameter_drift is None
    with pytest.raises(RuntimeError, match="no parameter drift"):
        o.drift()
    with pytest.raises(ValueError, match="at_bounds"):
        o.set_parameter_drift(0.1, at_bounds="fold")
    with pytest.raises(ValueError, match="rates"):
        o.set_parameter_drift(np.array([[1.0, 2.0], [2.0, 1.0]]), rows=[0, 1])
    assert o.parameter_drift is None                                    # nothing is kept of a refused call
    o.set_parameter_drift([0.1, 0.0, 0.2])
    assert o.parameter_drift["rows"] == (0, 2)
    before, state, version = np.array(o.particles), o.rng.bit_generator.state, o._particles.version
    o.drift(0.0)                                                        # dt = 0: nothing drawn, nothing moved
    assert o.rng.bit_generator.state == state and o._particles.version == version
    with pytest.raises(ValueError, match="dt"):
        o.drift(-1.0)
    _same(o.particles, before, "the cloud")
    o.drift(2.0)
    after = np.array(o.particles)
    assert np.all(after[[0, 2]] != before[[0, 2]])                      # every particle moves, whatever its weight
    _same(after[1], before[1], "the row of rate 0")
    o.set_parameter_drift(None)
    assert o.parameter_drift is None


# ------------------------------------------------------------------------------------------ (3) statistics
def test_the_step_has_covariance_dt_q_and_stales_the_moments(obe, hip):
    import torch
    from optbayesexpt_amd import _lib
    n, d, dt = 65536, 3, 0.7
    Q = np.array([[0.04, 0.015], [0.015, 0.09]])
    x = _pdf_case(n, d, 9)
    o = obe.ParticlePDF(x.copy())
    o.rng = np.random.default_rng(99)
    o.set_parameter_drift(Q, rows=[0, 2])
    mean_before, cov_before = o.mean(), o.covariance()                  # cached for the cloud before the step
    o.drift(dt)
    got = np.array(o.particles)
    step = got[[0, 2]] - x[[0, 2]]
    _same(got[1], x[1], "the row that does not drift")
    c = (step - step.mean(axis=1, keepdims=True)) @ (step - step.mean(axis=1, keepdims=True)).T / n
    want = dt * Q
    print("sample covariance / dt Q:", (c / want).tolist())
    for i in range(2):                                                  # five standard errors of a sample covariance
        assert abs(c[i, i] / want[i, i] - 1.0) <= 5.0 * math.sqrt(2.0 / n)
    assert abs(c[0, 1] - want[0, 1]) <= 5.0 * dt * math.sqrt((Q[0, 0] * Q[1, 1] + Q[0, 1] ** 2) / n)
    # mean() / covariance() after the step are obe_moments of the cloud as it is now
    cov, mean = o.covariance(), o.mean()
    layout = _lib.MomentLayout(d)
    p, w = torch.from_numpy(got).cuda(), torch.from_numpy(np.array(o.particle_weights)).cuda()
    ws = torch.empty(hip.workspace_bytes(n, 1, 1, d) // 8 + 1, dtype=torch.float64, device="cuda")
    mom_dev = torch.zeros(hip.moments_len(d), dtype=torch.float64, device="cuda")
    mom = np.zeros(hip.moments_len(d))
    hip.call("obe_moments", P(p.data_ptr()), n, d, n, P(w.data_ptr()), 1, P(mom_dev.data_ptr()), _host(mom),
             P(ws.data_ptr()), ws.numel() * 8, _stream())
    _same(mean, mom[layout.mean], "mean() after drift()")
    _same(cov, mom[layout.cov].reshape(d, d), "covariance() after drift()")
    assert not np.array_equal(mean, mean_before) and not np.array_equal(cov, cov_before)


# --------------------------------------------------------------------------- (4) OptBayesExpt integration
WIDTH, NOISE, TRUE = 0.1, 300.0, (3.0, -1000.0, 50000.0)       # (at this noise some cycles resample and some do not)
X = np.linspace(1.5, 4.5, 201)
N_P = 8192


def lorentz_prior(seed=31, n=N_P):
    g = np.random.default_rng(seed)
    return np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])


def experiment(obe, rng_seed=32, prior=None, **tuning):
    o = obe.OptBayesExpt(obe.models.lorentzian(1), (X,), lorentz_prior() if prior is None else prior, (WIDTH,),
                         scale=False, utility_method="variance_full", default_noise_std=NOISE)
    o.tuning_parameters.update(tuning)
    o.rng = np.random.default_rng(rng_seed)
    return o


def measurement(xs, k, centre=TRUE[0]):
    y = TRUE[2] + TRUE[1] / (((float(xs[0]) - centre) / WIDTH) ** 2 + 1.0)
    return y + NOISE * np.random.default_rng(1000 + k).standard_normal()


def cycle(o, k, then_drift=False):
    xs = o.opt_setting()
    o.pdf_update((xs, measurement(xs, k), NOISE))
    if then_drift:
        o.drift(1.0)
    return o.last_setting_index, bool(o.just_resampled)


def state_of(o):
    return np.array(o.particles), np.array(o.particle_weights), o.rng.bit_generator.state


def same_state(a, b, what):
    (pa, wa, ga), (pb, wb, gb) = state_of(a), state_of(b)
    _same(pa, pb, what + ": particles")
    _same(wa, wb, what + ": weights")
    assert ga == gb, what + ": generator"


@pytest.mark.parametrize("speculative", [False, True])
def test_the_sweep_after_a_drift_is_the_sweep_of_a_fresh_object(obe, speculative):
    """Bins forced, their grouping kept from sweep to sweep: the first sweep after a drift rebuilds it (kept is
    False) and gives the bits of an object built from the drifted cloud and weights — also when pdf_update() had
    enqueued the sweep of the cloud before the drift."""
    tuning = dict(sweep_bins="always", sweep_shift="never", sweep_bins_keep=True, speculative_sweep=speculative)
    o = experiment(obe, **tuning)
    o.set_parameter_drift({0: 0.02})
    k = 0
    while k < 3 or (speculative and o._sweeps.ticket is None and k < 8):
        cycle(o, k)
        k += 1
    assert o.last_sweep["bins"], o.last_sweep
    if speculative:
        assert o._sweeps.ticket is not None                             # a sweep of the present cloud is under way
    else:
        o.opt_setting()
        o.opt_setting()
        assert o.last_sweep["kept"] is True                             # the grouping of the present cloud is kept
    cloud_before = np.array(o.particles)
    resampled = o.just_resampled
    o.drift(1.0)
    assert o._sweeps.ticket is None and o.just_resampled == resampled
    cloud, w = np.array(o.particles), np.array(o.particle_weights)
    assert np.all(cloud[0] != cloud_before[0])
    _same(cloud[1:], cloud_before[1:], "the rows that do not drift")
    o.opt_setting()
    assert o.last_sweep["bins"] and o.last_sweep["kept"] is False, o.last_sweep
    fresh = experiment(obe, prior=cloud.copy(), **tuning)
    fresh.particle_weights = w
    fresh.opt_setting()
    assert fresh.last_sweep["bins"] and fresh.last_sweep["kept"] is False, fresh.last_sweep
    _same(o._utility_dev.cpu().numpy(), fresh._utility_dev.cpu().numpy(), "utility")
    assert o.last_setting_index == fresh.last_setting_index
    o.opt_setting()
    assert o.last_sweep["kept"] is True                                 # ... and the rebuilt grouping is kept again


@pytest.mark.parametrize("speculative", ["auto", True])
def test_per_update_is_pdf_update_then_drift(obe, speculative):
    a, b = experiment(obe, speculative_sweep=speculative), experiment(obe, speculative_sweep=speculative)
    a.set_parameter_drift({0: 0.02}, per_update=True)
    b.set_parameter_drift({0: 0.02})
    resamples = 0
    for k in range(6):
        ia, ra = cycle(a, k)
        assert a._sweeps.ticket is None                                 # no sweep of the cloud before the drift
        ib, rb = cycle(b, k, then_drift=True)
        assert (ia, ra) == (ib, rb), k
        same_state(a, b, f"cycle {k}")
        resamples += ra
    print(f"{resamples} of 6 cycles resampled")
    assert 0 < resamples < 6                                            # the drift behind a resample, and without one


def test_per_update_on_the_classes_with_an_update_of_their_own(obe):
    """OptBayesExptSignalNoise (its own update path) and OptBayesExptSweeper (one pdf_update() is a sweep of many
    points: ONE step behind its last point, as the generator's position shows) against pdf_update(); drift(1.0)."""
    import warnings
    import _state_cases as sc

    def signal_noise():
        o = obe.OptBayesExptSignalNoise(obe.models.lorentzian(1), (X,), lorentz_prior(), (WIDTH,), noise_floor=NOISE,
                                        noise_gain=1.0, scale=False, utility_method="variance_full")
        o.rng = np.random.default_rng(32)
        return o

    def sweep_cycle(o, k, then_drift):
        x = o.opt_setting()
        o.pdf_update(sc.measure(o, "sweeper", k, x))
        if then_drift:
            o.drift(1.0)
        return o.last_setting_index

    for name, make, one, rates in (("signal noise", signal_noise, lambda o, k, d: cycle(o, k, then_drift=d)[0], {0: 0.02}),
                                   ("sweeper", lambda: sc.build("sweeper"), sweep_cycle, {0: 0.02, 3: 5.0})):
        a, b = make(), make()
        a.set_parameter_drift(rates, per_update=True)
        b.set_parameter_drift(rates)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for k in range(4):
                assert one(a, k, False) == one(b, k, True), (name, k)
                same_state(a, b, f"{name}, cycle {k}")


def test_a_drift_that_is_set_but_never_applied_changes_nothing(obe):
    a, b = experiment(obe), experiment(obe)
    a.set_parameter_drift({0: 0.02}, per_update=False, at_bounds="reflect")
    for k in range(6):
        assert cycle(a, k) == cycle(b, k), k
        assert (a._sweeps.ticket is None) == (b._sweeps.ticket is None), k
        same_state(a, b, f"cycle {k}")
    assert a.sweep_state() == b.sweep_state()


def noise_experiment(obe, at_bounds, sigma_hi, rate):
    g = np.random.default_rng(61)
    prior = np.vstack([lorentz_prior(62), g.uniform(1.0, sigma_hi, (1, N_P))])
    o = obe.OptBayesExptNoiseParameter(obe.models.lorentzian(1), (X,), prior, (WIDTH,), noise_parameter_index=3,
                                       scale=False)
    o.tuning_parameters["device_rng"] = False                           # the normals are NumPy's own: an exact reference
    o.rng = np.random.default_rng(63)
    o.set_parameter_drift({3: rate}, at_bounds=at_bounds)
    return o, prior


def test_noise_parameter_masks_what_drifts_to_sigma_not_positive(obe):
    o, prior = noise_experiment(obe, "mask", 20.0, 10.0)
    z = np.random.default_rng(63).standard_normal((N_P, 1))
    o.drift(1.0)
    want = do.drift_exact(prior, [3], z, [[10.0]])
    bad = want[3] <= 0.0
    assert 0.05 * N_P < bad.sum() < 0.5 * N_P
    _same(o.particles, want, "the drifted cloud")
    w = np.array(o.particle_weights)
    assert_array_equal(w == 0.0, bad)
    assert o.last_constraint_count == int(bad.sum())
    assert abs(w.sum() - 1.0) < 1e-12 and np.all(w[~bad] > 0.0)


def test_noise_parameter_reflects_at_sigma_zero(obe):
    """Every step is smaller than twice sigma's distance to zero after it (there is no upper bound to cross): one
    reflection brings every particle back to sigma > 0, nothing is masked and the weights stay."""
    o, prior = noise_experiment(obe, "reflect", 20.0, 10.0)
    z = np.random.default_rng(63).standard_normal((N_P, 1))
    w_before = np.array(o.particle_weights)
    o.drift(1.0)
    plain = do.drift_exact(prior, [3], z, [[10.0]])
    want = do.drift_exact(prior, [3], z, [[10.0]], [0.0], [INF])
    crossed = plain[3] < 0.0
    assert 0.05 * N_P < crossed.sum() and np.all(want[3] > 0.0)
    _same(want[3, crossed], -plain[3, crossed], "the reflection at 0 is a change of sign")
    _same(o.particles, want, "the reflected cloud")
    assert o.last_constraint_count == 0
    _same(o.particle_weights, w_before, "the weights")
    # a user's bound joins the class's own: sigma in (0, 25]
    o, prior = noise_experiment(obe, "reflect", 20.0, 10.0)
    o.set_parameter_bounds({3: (None, 25.0)})
    o.drift(1.0)
    want = do.drift_exact(prior, [3], z, [[10.0]], [0.0], [25.0])
    _same(o.particles, want, "reflected at both ends")
    outside = (want[3] <= 0.0) | (want[3] > 25.0)
    assert o.last_constraint_count == int(outside.sum())
    assert_array_equal(np.array(o.particle_weights) == 0.0, outside)
    # 'reflect' without a bound on a drifted row is the mask's call
    o, prior = noise_experiment(obe, "reflect", 20.0, 10.0)
    o.set_parameter_drift({0: 0.02}, at_bounds="reflect")
    z = np.random.default_rng(63).standard_normal((N_P, 1))
    o.drift(1.0)
    _same(o.particles, do.drift_exact(prior, [0], z, [[0.02]]), "no bound on the drifted row")


def test_save_load_and_deepcopy_carry_the_drift(obe, tmp_path):
    o = experiment(obe)
    o.set_parameter_drift(np.array([[4e-4, 1e-3], [1e-3, 100.0]]), rows=[0, 1], per_update=True, at_bounds="reflect")
    o.set_parameter_bounds({1: (-2500.0, -100.0)})
    for k in range(2):
        cycle(o, k)
    c = copy.deepcopy(o)
    obe.save(o, str(tmp_path / "drift.state"))
    r = obe.load(str(tmp_path / "drift.state"))
    for other in (c, r):
        got, want = other.parameter_drift, o.parameter_drift
        assert got["rows"] == want["rows"] == (0, 1) and got["per_update"] is True and got["at_bounds"] == "reflect"
        _same(got["cholesky"], want["cholesky"], "the factor")
    for k in range(2, 5):
        first = cycle(o, k)
        for other, name in ((c, "deepcopy"), (r, "save / load")):
            assert cycle(other, k) == first, (name, k)
            same_state(o, other, f"{name}, cycle {k}")
    # an object without a drift writes the snapshot it always wrote
    assert "parameter_drift" not in experiment(obe).__getstate__()


def test_a_stale_parameters_alias_stays_the_alias(obe):
    o = experiment(obe)
    o.set_parameter_drift({0: 0.02})
    cloud = lorentz_prior(71)
    old = np.array(o.parameters)
    o.set_pdf(cloud.copy())
    assert o._parameters is not o._particles
    o.drift(1.0)
    assert o._parameters is not o._particles
    _same(o.parameters, old, "the alias")
    assert np.all(np.array(o.particles)[0] != cloud[0])
    _same(np.array(o.particles)[1:], cloud[1:], "the rows that do not drift")


# ------------------------------------------------------------------------------------------ (5) the example
def test_drifting_line_example_tracks_where_the_static_filter_does_not(hip):
    """The factor of 2 keeps a seed's luck from passing for tracking.  Measured on an MI355X (seed 0, 8192 particles,
    10 widths in 200 cycles): with drift 0.009976 (0.10 line widths), static 0.9102 (9.1 widths, the whole path but one
    width: it never followed)."""
    import warnings
    from test_gpu_examples import load
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with_drift, static = load("drifting_line").main(n_particles=8192, quiet=True)
    print(f"final |mean x0 - centre|: with drift {with_drift:.4g}, static {static:.4g}")
    assert 2.0 * with_drift <= static
