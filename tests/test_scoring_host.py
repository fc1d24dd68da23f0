"""Scoring a measurement against the posterior predictive, the part that needs no device: the oracle the GPU tests
compare with is pinned against SciPy and against mpmath at 50 digits, the argument checks raise before any library
call, the three entry points are declared, exported and bound, and they refuse bad arguments with status -1 and a
message without touching a device."""
import math
import types

import numpy as np
import pytest
from scipy import special, stats

import _scoring_oracle as oracle
from optbayesexpt_amd import _lib, _scoring, models

NAMES = ("obe_predictive_score_workspace_bytes", "obe_predictive_logpdf", "obe_predictive_tails")
INPUTS = ["m", "d_settings", "ld_s", "n_records", "d_y_meas", "ld_y", "d_sigma", "ld_sigma", "h_noise_rows",
          "d_particles", "ld_p", "n_particles", "d_weights"]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# -------------------------------------------------------------------------------------------------- the oracle
def _cloud(g, n, n_c, per_particle):
    y = g.normal(5.0, 2.0, (n_c, n))
    w = g.random(n)
    ym = g.normal(5.0, 2.0, n_c)
    sigma = g.uniform(0.5, 3.0, (n_c, n) if per_particle else n_c)
    return y, w, ym, sigma


@pytest.mark.parametrize("per_particle", [False, True])
@pytest.mark.parametrize("n,n_c", [(1, 1), (7, 2), (1000, 1), (5000, 3)])
def test_oracle_is_scipys_logsumexp_and_ndtr(n, n_c, per_particle):
    g = np.random.default_rng([n, n_c, per_particle])
    y, w, ym, sigma = _cloud(g, n, n_c, per_particle)
    s = np.broadcast_to(np.asarray(sigma).reshape(n_c, -1), y.shape)
    want = special.logsumexp(stats.norm.logpdf(ym[:, None], y, s).sum(axis=0), b=w) - np.log(w.sum())
    assert abs(oracle.logpdf(y, w, ym, sigma) - want) <= 1e-12 * max(1.0, abs(want))
    lower, upper = oracle.tails(y, w, ym, sigma)
    for c in range(n_c):
        lo = np.sum(w * special.ndtr((ym[c] - y[c]) / s[c])) / w.sum()
        hi = np.sum(w * special.ndtr((y[c] - ym[c]) / s[c])) / w.sum()
        assert abs(lower[c] - lo) <= 1e-12 * lo and abs(upper[c] - hi) <= 1e-12 * hi
        assert abs(lower[c] + upper[c] - 1.0) <= 1e-12


def test_oracle_exclusion_rules():
    g = np.random.default_rng(3)
    y, w, ym, sigma = _cloud(g, 50, 2, True)
    base = oracle.logpdf(y, w, ym, sigma), oracle.tails(y, w, ym, sigma)
    # particles of zero, NaN or negative weight do not count, whatever their y and sigma are
    y2 = np.concatenate([y, [[np.nan, np.inf, 1.0], [0.0, -np.inf, np.nan]]], axis=1)
    s2 = np.concatenate([sigma, [[1.0, np.nan, -1.0], [1.0, 1.0, 0.0]]], axis=1)
    w2 = np.concatenate([w, [0.0, np.nan, -2.0]])
    assert oracle.logpdf(y2, w2, ym, s2) == base[0]
    np.testing.assert_array_equal(oracle.tails(y2, w2, ym, s2), base[1])
    # weighted particles with a sigma <= 0 or NaN, or a NaN / inf y, are excluded: only sum w sees them
    y3 = np.concatenate([y, [[1.0, 2.0, 3.0, np.nan, np.inf], [1.0, 2.0, 3.0, 4.0, 5.0]]], axis=1)
    s3 = np.concatenate([sigma, [[0.0, 1.0, np.nan, 1.0, 1.0], [1.0, -1.0, 1.0, 1.0, 1.0]]], axis=1)
    w3 = np.concatenate([w, np.full(5, 0.5)])
    shift = np.log(w.sum() / w3.sum())
    assert abs(oracle.logpdf(y3, w3, ym, s3) - (base[0] + shift)) <= 1e-13
    lo3, hi3 = oracle.tails(y3, w3, ym, s3)
    ratio = w.sum() / w3.sum()
    # channel 0: the NaN y counts for neither tail, the +inf y for the upper one (the model lies above the reading);
    # channel 1: the last two particles have finite y
    extra = 0.5 * special.erfc(-(np.array([4.0, 5.0]) - ym[1]) / np.sqrt(2.0)) * 0.5
    assert abs(lo3[0] - base[1][0][0] * ratio) <= 1e-14 and abs(hi3[0] - (base[1][1][0] * ratio + 0.5 / w3.sum())) <= 1e-14
    assert abs(hi3[1] - (base[1][1][1] * ratio + extra.sum() / w3.sum())) <= 1e-14
    # nobody left: -inf and zero tails; no weight at all: NaN
    assert oracle.logpdf(y, w, ym, -sigma) == -np.inf
    np.testing.assert_array_equal(oracle.tails(y, w, ym, -sigma), np.zeros((2, 2)))
    assert np.isnan(oracle.logpdf(y, 0 * w, ym, sigma)) and np.all(np.isnan(oracle.tails(y, -w, ym, sigma)))


MP_CASES = {
    "z near 30": lambda g: (30.0 + g.normal(0.0, 0.3, (1, 40)), g.random(40), np.zeros(1), np.ones(1)),
    "z near -30, two channels": lambda g: (-60.0 + g.normal(0.0, 0.5, (2, 40)), g.random(40), np.zeros(2),
                                           np.array([2.0, 2.0])),
    "sigma 1e-150": lambda g: (1e-150 * g.normal(0.0, 2.0, (1, 30)), g.random(30), np.zeros(1), np.full(1, 1e-150)),
    "sigma 1e150": lambda g: (1e150 * g.normal(0.0, 2.0, (1, 30)), g.random(30), np.zeros(1), np.full(1, 1e150)),
    "sigma rows 1e-150 .. 1e150": lambda g: (g.normal(0.0, 1.0, (1, 31)) * 10.0 ** np.linspace(-150, 150, 31),
                                             g.random(31), np.zeros(1), 10.0 ** np.linspace(-150, 150, 31)[None, :]),
    "best particle 1e5 log-units down": lambda g: (np.sqrt(2e5) + g.random((1, 50)) * 3.0, g.random(50), np.zeros(1),
                                                   np.ones(1)),
}


@pytest.mark.parametrize("case", sorted(MP_CASES))
def test_oracle_against_mpmath_at_50_digits(case):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    y, w, ym, sigma = MP_CASES[case](np.random.default_rng(sorted(MP_CASES).index(case)))
    s = np.broadcast_to(np.asarray(sigma).reshape(y.shape[0], -1), y.shape)
    n_c, n = y.shape
    sw = mp.fsum(mp.mpf(float(v)) for v in w)
    dens, lo, hi = mp.mpf(0), [mp.mpf(0)] * n_c, [mp.mpf(0)] * n_c
    for i in range(n):
        term = mp.mpf(float(w[i]))
        for c in range(n_c):
            z = (mp.mpf(float(y[c, i])) - mp.mpf(float(ym[c]))) / mp.mpf(float(s[c, i]))
            term *= mp.exp(-z * z / 2) / (mp.mpf(float(s[c, i])) * mp.sqrt(2 * mp.pi))
            lo[c] += mp.mpf(float(w[i])) * mp.erfc(z / mp.sqrt(2)) / 2
            hi[c] += mp.mpf(float(w[i])) * mp.erfc(-z / mp.sqrt(2)) / 2
        dens += term
    want = float(mp.log(dens / sw))
    got = oracle.logpdf(y, w, ym, sigma)
    assert abs(got - want) <= 1e-13 * max(1.0, abs(want)), (got, want)
    if case == "best particle 1e5 log-units down":
        assert want < -1e5
    lower, upper = oracle.tails(y, w, ym, sigma)
    for c in range(n_c):
        for g_, w_ in ((lower[c], float(lo[c] / sw)), (upper[c], float(hi[c] / sw))):
            assert abs(g_ - w_) <= 1e-12 * w_ + 5e-324, (case, g_, w_)


# -------------------------------------------------------------------------------------------- argument checks
def test_y_meas_forms():
    S = _scoring
    for value, n_c, shape, single in ((2.5, 1, (1, 1), True), ([1.0, 2.0, 3.0], 1, (1, 3), False), ([4.0], 1, (1, 1), False),
                                      ([1.0, 2.0], 2, (2, 1), True), (np.zeros((2, 5)), 2, (2, 5), False),
                                      (np.zeros((1, 5)), 1, (1, 5), False), (np.zeros((3, 1)), 3, (3, 1), False)):
        got, one = S.check_y_meas(value, n_c)
        assert got.shape == shape and got.dtype == np.float64 and one is single
    for bad, n_c in ((2.5, 2), ([1.0, 2.0, 3.0], 2), (np.zeros((3, 4)), 2), (np.zeros((2, 0)), 2), ([], 1), (None, 1),
                     ("a", 1), (np.zeros((1, 2, 3)), 1), ([1.0], 2)):
        with pytest.raises(ValueError):
            S.check_y_meas(bad, n_c)


def test_sigma_forms():
    S = _scoring
    np.testing.assert_array_equal(S.check_sigma(0.5, 2), [[0.5], [0.5]])
    np.testing.assert_array_equal(S.check_sigma([0.5, 2.0], 2), [[0.5], [2.0]])
    np.testing.assert_array_equal(S.check_sigma([0.5, 2.0, 3.0], 1), [[0.5, 2.0, 3.0]])
    assert S.check_sigma(np.ones((2, 7)), 2).shape == (2, 7)
    for bad, n_c in ((0.0, 1), (-1.0, 1), (np.nan, 1), (np.inf, 1), ([1.0, np.nan], 2), ([1.0, 0.0], 2), ([1.0, 2.0, 3.0], 2),
                     (np.ones((3, 4)), 2), (np.ones((2, 0)), 2), ("wide", 1), (np.ones((1, 1, 1)), 1), ([], 1)):
        with pytest.raises(ValueError):
            S.check_sigma(bad, n_c)


def test_records_broadcast_to_one_length():
    S = _scoring
    x, y, s, single = S.check_records((3.0,), 1.5, 0.1, 1, 1, None)              # a record as pdf_update takes it
    assert single and x.shape == y.shape == s.shape == (1, 1)
    x, y, s, single = S.check_records((3.0,), [1.0, 2.0, 3.0], 0.1, 1, 1, None)
    assert not single and x.shape == y.shape == s.shape == (1, 3)
    np.testing.assert_array_equal(x, [[3.0, 3.0, 3.0]])
    np.testing.assert_array_equal(s, [[0.1, 0.1, 0.1]])
    x, y, s, single = S.check_records((np.arange(4.0), 2.0), [1.0, -1.0], [0.1, 0.2], 2, 2, None)
    assert not single and x.shape == (2, 4) and y.shape == s.shape == (2, 4)
    np.testing.assert_array_equal(y, [[1.0] * 4, [-1.0] * 4])
    x, y, s, single = S.check_records((1.0, 2.0), [1.0, -1.0], None, 2, 2, np.array([2, 3], dtype=np.int32))
    assert single and s is None
    assert not S.check_records(([1.0],), 1.5, 0.1, 1, 1, None)[3]                 # a record axis in the settings
    x, y, s, _ = S.check_records(np.zeros((2, 5)), np.ones((2, 5)), np.ones((2, 1)), 2, 2, None)
    assert all(a.flags.c_contiguous and a.shape == (2, 5) for a in (x, y, s))
    bad = [((3.0,), 1.5, None, 1, 1, None),                                       # sigma is required on the base class
           ((3.0,), 1.5, 0.1, 1, 1, np.zeros(1, dtype=np.int32)),                 # and refused by the noise-parameter class
           ((np.arange(3.0),), np.arange(4.0), 0.1, 1, 1, None),
           ((np.arange(4.0),), np.arange(4.0), np.ones((1, 3)), 1, 1, None),
           ((3.0, 1.0), 1.5, 0.1, 1, 1, None), (None, 1.5, 0.1, 1, 1, None),
           ((3.0,), [1.0, 2.0, 3.0], 0.1, 1, 2, None), ((3.0,), 1.5, -0.1, 1, 1, None), ((3.0,), 1.5, np.nan, 1, 1, None)]
    for args in bad:
        with pytest.raises(ValueError):
            S.check_records(*args)


def test_pvalue_definition():
    lower = np.array([[0.2, 0.5, 0.9, 1e-300, 0.0, np.nan]])
    upper = np.array([[0.8, 0.5, 0.1, 1.0, 1.0, np.nan]])
    got = _scoring.pvalue_from_tails(lower, upper)
    np.testing.assert_array_equal(got[0, :5], [0.4, 1.0, 0.2, 2e-300, 0.0])
    assert np.isnan(got[0, 5])


def test_methods_check_their_arguments_before_any_library_call():
    """The three methods exist on OptBayesExpt (the noise-parameter and sweeper classes inherit them) and refuse bad
    arguments before they touch the cloud or the library: driven here on objects that have no device state at all."""
    from optbayesexpt_amd import OptBayesExpt, OptBayesExptNoiseParameter, OptBayesExptSweeper
    methods = ("predictive_logpdf", "predictive_cdf", "predictive_pvalue")
    for cls in (OptBayesExptNoiseParameter, OptBayesExptSweeper):
        for name in methods:
            assert getattr(cls, name) is getattr(OptBayesExpt, name)
    base = types.SimpleNamespace(_device_model=object(), allsettings=np.zeros((1, 5)), n_channels=2)
    noise = types.SimpleNamespace(_device_model=object(), allsettings=np.zeros((1, 5)), n_channels=2,
                                  _noise_rows=np.array([3, 4], dtype=np.int32))
    for name in methods:
        call = getattr(OptBayesExpt, name)
        for obj, args in ((base, ((3.0,), [1.0, 2.0])),                      # no sigma on the base class
                          (base, ((3.0,), [1.0, 2.0], None)),
                          (noise, ((3.0,), [1.0, 2.0], 0.5)),                # a sigma on the noise-parameter class
                          (base, ((3.0,), 1.0, 0.5)),                        # one channel of two
                          (base, ((3.0,), [1.0, 2.0, 3.0], 0.5)),
                          (base, ((3.0, 4.0), [1.0, 2.0], 0.5)),             # two settings for a model of one
                          (base, (None, [1.0, 2.0], 0.5)),                   # there is no None form
                          (base, ((3.0,), [1.0, 2.0], 0.0)),
                          (base, ((3.0,), [1.0, 2.0], [0.5, np.nan])),
                          (base, ((np.arange(3.0),), np.zeros((2, 4)), 0.5)),
                          (noise, ((3.0,), np.zeros((3, 4))))):
            with pytest.raises(ValueError):
                call(obj, *args)
    # a host-callable model (a plain Python model_function) is refused by name, as predict() refuses it
    host = types.SimpleNamespace(_device_model=None)
    for name in methods:
        with pytest.raises(TypeError, match="from_function.*from_expression"):
            getattr(OptBayesExpt, name)(host, (3.0,), 1.0, 0.5)


# ------------------------------------------------------------------------------------------ the entry points
def test_symbols_are_declared_exported_and_bound(lib):
    for name in NAMES:
        assert name in _lib.declared_symbols() and name in _lib.PROTOTYPES and name in _lib.MODEL_ENTRY_POINTS
        fn = getattr(lib.cdll, name)
        restype, params = _lib.PROTOTYPES[name]
        assert fn.restype is restype and len(fn.argtypes) == len(params)
    assert _lib.PROTOTYPES[NAMES[0]][0] is _lib.c_int64
    assert [p for _, p in _lib.PROTOTYPES[NAMES[0]][1]] == ["n_particles", "n_records", "n_channels"]
    assert [p for _, p in _lib.PROTOTYPES[NAMES[1]][1]] == INPUTS + ["d_logpdf", "d_ws", "ws_bytes", "stream"]
    assert [p for _, p in _lib.PROTOTYPES[NAMES[2]][1]] == INPUTS + ["d_lower", "d_upper", "d_ws", "ws_bytes", "stream"]
    from optbayesexpt_amd import build
    assert "obe_predict.hip" in build.PLUGIN_SOURCES
    assert lib.cdll.obe_abi_version() == 3


def test_workspace_size_is_positive_and_does_not_shrink(lib):
    size = lib.cdll.obe_predictive_score_workspace_bytes
    assert size(1, 1, 1) > 0
    g = np.random.default_rng(8)
    for _ in range(3000):
        n, r, c = int(g.integers(1, 1 << 22)), int(g.integers(1, 1 << 18)), int(g.integers(1, 9))
        base = size(n, r, c)
        assert base > 0
        assert size(n + int(g.integers(1, 1 << 20)), r, c) >= base
        assert size(n, r + int(g.integers(1, 1 << 16)), c) >= base
        assert size(n, r, c + 1) >= base
    assert size(1 << 20, 1 << 16, 8) < 1 << 28                # per chunk, not per particle


def test_entry_points_refuse_bad_arguments_without_a_device(lib):
    dev = 1 << 20                    # (never dereferenced: every call below is refused by its argument checks)
    c = lib.cdll
    m = models.lorentzian(1).struct(4, (0.1,))
    n, r, big = 1000, 10, 1 << 30
    rows = np.array([3, 0, 0, 0, 0, 0, 0, 0], dtype=np.int32)
    R = _lib.host_ptr(rows)

    def refused(rc, word):
        assert rc == -1 and word in lib.last_error(), (rc, lib.last_error())

    def inputs(kw):
        a = dict(m=m, d_settings=dev, ld_s=r, n_records=r, d_y_meas=dev, ld_y=r, d_sigma=dev, ld_sigma=r,
                 h_noise_rows=None, d_particles=dev, ld_p=n, n_particles=n, d_weights=dev)
        assert list(a) == INPUTS
        tail = kw.pop("_tail")
        tail.update(d_ws=dev, ws_bytes=big, stream=None)
        a.update(tail)
        a.update(kw)
        return a.values()

    def logpdf(**kw):
        return c.obe_predictive_logpdf(*inputs(dict(kw, _tail=dict(d_logpdf=dev))))

    def tails(**kw):
        return c.obe_predictive_tails(*inputs(dict(kw, _tail=dict(d_lower=dev, d_upper=dev))))

    for call, outs in ((logpdf, ("d_logpdf",)), (tails, ("d_lower", "d_upper"))):
        for name in ("m", "d_settings", "d_y_meas", "d_particles", "d_weights", "d_ws") + outs:
            refused(call(**{name: None}), "null pointer")
        refused(call(d_sigma=None), "exactly one of d_sigma and h_noise_rows")              # neither
        refused(call(h_noise_rows=R), "exactly one of d_sigma and h_noise_rows")            # both
        refused(call(n_records=0), "n_settings < 1")
        refused(call(n_records=-5), "n_settings < 1")
        refused(call(ld_s=r - 1), "shorter")
        refused(call(ld_y=r - 1), "shorter than n_records")
        refused(call(ld_sigma=r - 1), "shorter than n_records")
        refused(call(n_particles=0), "cloud size")
        refused(call(ld_p=n - 1), "cloud size")
        for bad in (-1, 4, 1 << 20):
            refused(call(d_sigma=None, h_noise_rows=_lib.host_ptr(np.array([bad] * 8, dtype=np.int32))),
                    "noise row index out of range")
        refused(call(ws_bytes=c.obe_predictive_score_workspace_bytes(n, r, 1) - 1), "workspace too small")
        bad = models.lorentzian(1).struct(3, (0.1,))
        bad.aux = 9
        refused(call(m=bad), "aux")
        # two channels need twice the partial sums
        coil = models.coil().struct(3, ())
        refused(call(m=coil, ws_bytes=c.obe_predictive_score_workspace_bytes(n, r, 1)), "workspace too small")
    with pytest.raises(_lib.ObeHipError) as e:
        lib.call("obe_predictive_logpdf", m, dev, r, r, dev, r, dev, r, None, dev, n, n, dev, dev, dev, 0, None)
    assert e.value.refused_before_launch
