"""K2, the Bayes update of the particle weights, on the device (GPU) at every entry point, noise form and grid class,
against the references of tests/_update_oracle.py (pinned on the CPU by tests/test_update_oracle_host.py, which also
shows that the inputs used here tell a wrong kernel from a right one).

A. EXACT CLOUDS (weights q 2^-k, likelihoods 2^j or 0, sum q 2^j = 2^m): weights, sum t and sum w'^2 BIT FOR BIT
   through obe_bayes_update_lik, _y, _model, _model_moments, _model_moments_enqueue and _sweep (one point), at every
   edge of wave, workgroup, grid cap (768 workgroups: 196 608) and two-particle trip (65 536, 131 072); the fused
   forms' K3 block against obe_moments on the weights they left; strict sums; the special values.
B. GENERAL DOUBLES: obe_likelihood_y within likelihood_bound of the long double likelihood for 1 ... 17 channels,
   fixed sigma and noise rows, no choke / 0.6 / 1.7; the posterior through obe_bayes_update_y.
C. THE FORMS AGREE: model fused, y supplied, likelihood supplied leave the same bits; obe_eval_over_settings on the
   transposed problem returns the bits of obe_eval_over_particles.
D. THE SWEEP BATCH is the sequential replay with the resample test on the host; the enqueue form.
E. REFUSALS leave everything untouched.

No tolerance in this file is a literal: each is equality, a value of likelihood_bound / sum_t_bound, or the argument
of _replay.close_weights, the project's own bar for weights.

The harness: particles with ld = n + 5 and model outputs with ld = n + 3, NaN in the padding, both compared unchanged
after every call; a sentinel behind the weights, behind d_lik_out and behind h_out; a NaN-filled workspace of exactly
hip.workspace_bytes."""
import ctypes
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _update_oracle as uo

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD_P, PAD_Y, GUARD = 5, 3, 9
SENTINEL = -6.02214076e23
NAN = float("nan")
WEIGHT_RTOL = 1e-10            # the project's bar for particle weights (close_weights: on the exponent)
MAX_CH, MAX_SET = 8, 8         # OBE_MAX_CHANNELS, OBE_MAX_SETDIMS (include/obe_hip.h)
WORST = {}                     # what -> (worst fraction of its bound, where): test_worst_fractions_are_reported


def update_ws_bytes(d=0):
    """What an update carves from its workspace (csrc/obe_update_common.hip: update_ws_bytes): two rows of 2048
    partials, 8 scalars and, for the fused forms, 768 rows of 3 + 2 d moment partials.  Checked by the refusals."""
    return (2 * 2048 + 8 + (768 * (3 + 2 * d) if d else 0)) * 8


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _untouched(a, what):
    assert_array_equal(_bits(a), _bits(np.full(len(a), SENTINEL)), err_msg=what + ": written although it is not this call's")


def _padded(x, pad):
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    buf = np.full((x.shape[0], x.shape[1] + pad), np.nan)
    buf[:, :x.shape[1]] = x
    return buf


def _model(name, d, cons=()):
    from optbayesexpt_amd import models
    factory, args = {"line_ab": (models.line_ab, ()), "line_mb": (models.line_mb, ()),
                     "first_param": (models.first_parameter, ()), "coil": (models.coil, ()),
                     "rabi": (models.rabi, ()), "lorentz1": (models.lorentzian, (1,)),
                     "lorentz3": (models.lorentzian, (3,))}[name]
    return factory(*args).struct(d, cons)


class Dev:
    """One cloud on the device and the K2 entry points on it at the C ABI.  `particles` (rows, n) and `y`
    (channels, n) may each be None.  Every call checks its guards and that the inputs are unchanged."""

    def __init__(self, hip, n, particles=None, y=None):
        import torch
        from optbayesexpt_amd import _lib
        self.hip, self.torch, self._lib, self.n = hip, torch, _lib, n
        self.st = P(torch.cuda.current_stream().cuda_stream)
        self.p_host = self.y_host = self.p = self.y = None
        self.ld_p, self.ld_y, self.d, self.c = n + PAD_P, n + PAD_Y, 1, 1
        if particles is not None:
            self.p_host = _padded(particles, PAD_P)
            self.p = torch.from_numpy(self.p_host).cuda()
            self.d = self.p_host.shape[0]
        if y is not None:
            self.y_host = _padded(y, PAD_Y)
            self.y = torch.from_numpy(self.y_host).cuda()
            self.c = self.y_host.shape[0]
        self.ws_bytes = hip.workspace_bytes(n, 1, min(self.c, MAX_CH), min(self.d, 32))
        self.keep = []

    # -- buffers
    def weights(self, w):
        buf = np.full(self.n + GUARD, SENTINEL)
        buf[:self.n] = w
        return self.torch.from_numpy(buf).cuda()

    def workspace(self):
        return self.torch.full((-(-self.ws_bytes // 8),), NAN, dtype=self.torch.float64, device="cuda")

    def ws_ptr(self):
        self._ws = self.workspace()                            # (kept until the next call's)
        return P(self._ws.data_ptr())

    def host(self, values):
        a = np.ascontiguousarray(values)
        self.keep.append(a)
        return self._lib.host_ptr(a)

    def ptr(self, t):
        return None if t is None else P(t.data_ptr())

    def lik_args(self, prob, width=MAX_CH):
        """(h_y_meas, h_sigma, h_noise_rows, n_lik_channels, choke) of a problem dict."""
        n_lik = prob.get("n_lik", len(np.atleast_1d(prob["y_meas"])))
        ym = np.zeros(max(width, n_lik))
        ym[:n_lik] = np.atleast_1d(prob["y_meas"])[:n_lik]
        sigma = rows = None
        if prob.get("sigma") is not None:
            s = np.ones(max(width, n_lik))
            s[:n_lik] = np.atleast_1d(prob["sigma"])[:n_lik]
            sigma = self.host(s)
        if prob.get("noise_rows") is not None:
            r = np.zeros(max(width, n_lik), dtype=np.int32)
            r[:n_lik] = prob["noise_rows"][:n_lik]
            rows = self.host(r)
        choke = prob.get("choke")
        return self.host(ym), sigma, rows, n_lik, NAN if choke is None else float(choke)

    def done(self, wd, h, n_out, what):
        """(weights, h_out[:n_out]) after a call, guards and inputs checked."""
        self.torch.cuda.synchronize()
        w = wd.cpu().numpy()
        _untouched(w[self.n:], what + ": the guard behind the weights")
        _untouched(np.array(h[n_out:]), what + ": the guard behind h_out")
        self.inputs_unchanged(what)
        return w[:self.n].copy(), np.array(h[:n_out])

    def inputs_unchanged(self, what):
        if self.p is not None:
            assert_array_equal(_bits(self.p.cpu().numpy()), _bits(self.p_host), err_msg=what + ": the particles")
        if self.y is not None:
            assert_array_equal(_bits(self.y.cpu().numpy()), _bits(self.y_host), err_msg=what + ": d_y")

    def h_out(self, n_out):
        return np.full(n_out + GUARD, SENTINEL)

    # -- the entry points
    def update_lik(self, w, lik):
        wd, h = self.weights(w), self.h_out(2)
        ld = self.weights(lik)
        self.hip.call("obe_bayes_update_lik", P(ld.data_ptr()), self.n, P(wd.data_ptr()), self.ws_ptr(),
                      self.ws_bytes, self.host(h), self.st)
        assert_array_equal(_bits(ld.cpu().numpy()[:self.n]), _bits(lik), err_msg="d_lik")
        return self.done(wd, h, 2, "obe_bayes_update_lik")

    def update_y(self, w, prob):
        wd, h = self.weights(w), self.h_out(2)
        self.hip.call("obe_bayes_update_y", self.ptr(self.y), self.ld_y, self.c, self.ptr(self.p), self.ld_p, self.n,
                      P(wd.data_ptr()), *self.lik_args(prob), self.ws_ptr(), self.ws_bytes, self.host(h),
                      self.st)
        return self.done(wd, h, 2, "obe_bayes_update_y")

    def setting(self, prob):
        s = np.zeros(MAX_SET)
        v = np.atleast_1d(np.asarray(prob["setting"], dtype=np.float64))
        s[:len(v)] = v
        return self.host(s)

    def update_model(self, w, m, prob):
        wd, h = self.weights(w), self.h_out(2)
        self.hip.call("obe_bayes_update_model", m, self.ptr(self.p), self.ld_p, self.n, P(wd.data_ptr()),
                      self.setting(prob), *self.lik_args(prob), self.ws_ptr(), self.ws_bytes, self.host(h),
                      self.st)
        return self.done(wd, h, 2, "obe_bayes_update_model")

    def moments_of(self, w):
        """obe_moments(want_cov = 0) on these weights: the first-moment part of the K3 block."""
        torch = self.torch
        wd = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        out = torch.full((self.hip.moments_len(self.d) + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        self.hip.call("obe_moments", self.ptr(self.p), self.ld_p, self.d, self.n, P(wd.data_ptr()), 0, P(out.data_ptr()), None,
                      self.ws_ptr(), self.ws_bytes, self.st)
        torch.cuda.synchronize()
        return out.cpu().numpy()[:2 + 4 * self.d]

    def update_fused(self, w, m, prob, enqueue=None, ws=None, ws_bytes=None):
        """(weights, h_out[:4 + 4 d] (+ the decision word for the enqueue form), d_moments[:2 + 4 d], abort word).
        enqueue: None, or (auto_resample, threshold)."""
        torch, d = self.torch, self.d
        first = 2 + 4 * d
        n_out = 2 + first + (1 if enqueue else 0)
        wd = self.weights(w)
        mom = torch.full((self.hip.moments_len(d) + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        ws = self.workspace() if ws is None else ws
        ws_bytes = self.ws_bytes if ws_bytes is None else ws_bytes
        args = (m, self.ptr(self.p), self.ld_p, self.n, P(wd.data_ptr()), self.setting(prob), *self.lik_args(prob),
                P(mom.data_ptr()), P(ws.data_ptr()), ws_bytes)
        if enqueue:
            h = self._lib.pinned_array(n_out + GUARD)
            h[:] = SENTINEL
            self.hip.call("obe_bayes_update_model_moments_enqueue", *args, self._lib.host_ptr(h), int(enqueue[0]),
                          float(enqueue[1]), self.st)
            self.hip.call("obe_host_words_wait", self._lib.host_ptr(h), n_out, self.st)
        else:
            h = self.h_out(n_out)
            self.hip.call("obe_bayes_update_model_moments", *args, self.host(h), self.st)
        what = "obe_bayes_update_model_moments" + ("_enqueue" if enqueue else "")
        w1, out = self.done(wd, h, n_out, what)
        dev = mom.cpu().numpy()
        _untouched(dev[first:], what + ": d_moments behind the first moments")
        abort = None
        if enqueue:
            assert ws_bytes % 8 == 0
            abort = int(ws.cpu().numpy().view(np.uint32)[2 * (ws_bytes // 8 - 1)])
        return w1, out, dev[:first], abort

    def update_sweep(self, w, m, prob, settings, y_meas, auto_resample, threshold, null_settings=False):
        """`settings` (n_points, setdims) and `y_meas` (n_points, n_lik): (weights, h_out[:4])."""
        y_meas = np.atleast_2d(np.asarray(y_meas, dtype=np.float64))
        k = len(y_meas)
        hs, hy = np.zeros((k, MAX_SET)), np.zeros((k, MAX_CH))
        st = np.asarray(settings, dtype=np.float64).reshape(k, -1)
        hs[:, :st.shape[1]] = st
        hy[:, :y_meas.shape[1]] = y_meas
        wd, h = self.weights(w), self.h_out(4)
        _, sigma, rows, n_lik, choke = self.lik_args(prob)
        self.hip.call("obe_bayes_update_sweep", m, self.ptr(self.p), self.ld_p, self.n, P(wd.data_ptr()),
                      None if null_settings else self.host(hs), self.host(hy), sigma, rows, n_lik, choke, k,
                      int(auto_resample), float(threshold), self.ws_ptr(), self.ws_bytes, self.host(h),
                      self.st)
        return self.done(wd, h, 4, "obe_bayes_update_sweep")

    def likelihood_y(self, prob):
        torch = self.torch
        out = torch.full((self.n + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        n_lik = prob["n_lik"]
        self.hip.call("obe_likelihood_y", self.ptr(self.y), self.ld_y, self.c, self.ptr(self.p), self.ld_p, self.n,
                      *self.lik_args(prob, width=n_lik), P(out.data_ptr()), self.st)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        _untouched(got[self.n:], "obe_likelihood_y: the guard behind d_lik_out")
        self.inputs_unchanged("obe_likelihood_y")
        return got[:self.n].copy()

    def eval_over_particles(self, m, setting, channels):
        torch = self.torch
        out = torch.full((channels, self.ld_y), SENTINEL, dtype=torch.float64, device="cuda")
        self.hip.call("obe_eval_over_particles", m, self.ptr(self.p), self.ld_p, self.n, self.setting(dict(setting=setting)),
                      P(out.data_ptr()), self.ld_y, self.st)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for row in got:
            _untouched(row[self.n:], "obe_eval_over_particles: the padding of d_y_out")
        self.inputs_unchanged("obe_eval_over_particles")
        return got[:, :self.n].copy()


# =================================================================================== A. exact clouds, bit for bit
ALL_SIZES = uo.EXACT_SMALL + uo.EXACT_GRID
UNFUSED = ("lik", "y_rows", "y_fixed", "model_rows", "model_fixed", "sweep")
FUSED_D = {2: ("first_param", 1), 3: ("line_ab", 2), 16: ("line_ab", 9)}       # d -> (model, noise row)


def _rng(*key):
    return np.random.default_rng([17, *[int(k) for k in key]])


def _expect(cloud, shift, w, h, what):
    w1, total, w2 = cloud.posterior(shift)
    _same_bits(w, w1, what + ": weights")
    _same_bits(h[:2], [total, w2], what + ": h_out = [sum t, sum w'^2]")


def _run_unfused(hip, form, n):
    """(cloud, shift, weights, h_out) of one exact cloud through one unfused entry point."""
    fixed = form in ("y_fixed", "model_fixed")
    cloud = uo.exact_case(n, fixed)
    g = _rng(UNFUSED.index(form), n)
    if form == "lik":
        return (cloud, 0) + Dev(hip, n).update_lik(cloud.prior(), cloud.lik())
    if form in ("y_rows", "y_fixed"):
        c, n_lik = ((1, 1), (3, 2), (8, 8), (8, 5))[n % 4]
        prob = uo.exact_y_problem(g, cloud, c, n_lik, rows=not fixed)
        return (cloud, prob["shift"]) + Dev(hip, n, prob["particles"], prob["y"]).update_y(cloud.prior(), prob)
    d, row = (2, None) if fixed else (3, 2)
    prob = uo.exact_model_problem(g, cloud, "line_ab", d, row)
    dev, m = Dev(hip, n, prob["particles"]), _model("line_ab", d)
    if form == "sweep":
        w, h = dev.update_sweep(cloud.prior(), m, prob, [[prob["setting"]]], [[prob["y_meas"]]], 1, 0.5)
        assert h[3] == 1.0 and h[2] == float(uo.resample_due(h[1], n, 0.5)), "points applied, resample flag"
        return cloud, prob["shift"], w, h
    return (cloud, prob["shift"]) + dev.update_model(cloud.prior(), m, prob)


@pytest.mark.parametrize("n", ALL_SIZES)
@pytest.mark.parametrize("form", UNFUSED)
def test_exact_cloud_unfused_entry_points(hip, form, n):
    """Pass A in its three forms + normalize_kernel + fold2_kernel (the sweep: + its prologue and fold2_stop_kernel):
    one workgroup ... 768 of them and the second and third trip of the grid-stride loops."""
    cloud, shift, w, h = _run_unfused(hip, form, n)
    _expect(cloud, shift, w, h, f"{form} n={n}")


def _fused_case(hip, d, n, enqueue=None):
    model, row = FUSED_D[d]
    cloud = uo.exact_case(n)
    prob = uo.exact_model_problem(_rng(100 + d, n), cloud, model, d, row)
    dev = Dev(hip, n, prob["particles"])
    return (cloud, prob, dev) + dev.update_fused(cloud.prior(), _model(model, d), prob, enqueue)


@pytest.mark.parametrize("n", ALL_SIZES)
@pytest.mark.parametrize("d", sorted(FUSED_D))
@pytest.mark.parametrize("enqueue", [False, True])
def test_exact_cloud_fused_entry_points(hip, d, n, enqueue):
    """normalize_moments_kernel<D, FOLD = true>: the two-particle trip's second slot is live from n = 65 537 and a
    second trip starts at 131 073.  The K3 block is obe_moments(want_cov = 0) on the weights left, bit for bit."""
    threshold = 0.5
    cloud, prob, dev, w, h, mom, abort = _fused_case(hip, d, n, (1, threshold) if enqueue else None)
    what = f"fused d={d} n={n} enqueue={enqueue}"
    _expect(cloud, prob["shift"], w, h, what)
    want = dev.moments_of(w)
    _same_bits(mom, want, what + ": d_moments against obe_moments on the weights left")
    _same_bits(h[2:4 + 4 * d], want, what + ": the host block")
    if enqueue:
        due = uo.resample_due(h[1], n, threshold)
        assert h[4 + 4 * d] == float(due) and abort == int(due), what + ": the resample decision"


STRICT_FORMS = ("y_rows", "model_rows", "sweep")


@pytest.mark.parametrize("n", uo.STRICT_SIZES)
@pytest.mark.parametrize("form", STRICT_FORMS)
def test_exact_cloud_strict_sums_give_the_same_bits(hip, form, n):
    """numpy_order_sum_kernel in place of the partials' fold (obe_strict_sums): an exact cloud has one sum."""
    assert hip.cdll.obe_strict_sums(1) == 0
    try:
        cloud, shift, w, h = _run_unfused(hip, form, n)
    finally:
        assert hip.cdll.obe_strict_sums(0) == 1
    _expect(cloud, shift, w, h, f"strict {form} n={n}")


@pytest.mark.parametrize("name", sorted(uo.special_cases()))
def test_special_values(hip, name):
    """One workgroup, dyadic data: NumPy's expression of particlepdf.py:136-139 to the bit, through the likelihood
    form and the supplied-y form (sigma = 2^-j from a particle row; a dead particle 3 off with sigma 2^-6)."""
    w, j, dead, _ = uo.special_cases()[name]
    n = len(w)
    lik = uo.special_lik(j, dead)
    w1, total, w2 = uo.posterior_np(w, lik)
    got_w, got_h = Dev(hip, n).update_lik(w, lik)
    _same_bits(got_w, w1, name + " (lik): weights")
    _same_bits(got_h, [total, w2], name + " (lik): h_out")
    sig = np.where(dead, 2.0 ** -uo.J_MAX, np.ldexp(1.0, -j))
    prob = dict(y=np.where(dead, 45.0, 42.0)[None], y_meas=np.array([42.0]), particles=np.stack([np.arange(n) * 1.0, sig]),
                noise_rows=np.array([1], dtype=np.int32), sigma=None)
    got_w, got_h = Dev(hip, n, prob["particles"], prob["y"]).update_y(w, prob)
    _same_bits(got_w, w1, name + " (y): weights")
    _same_bits(got_h, [total, w2], name + " (y): h_out")
    if name == "every likelihood zero":
        assert not got_w.any() and got_h.tolist() == [0.0, 0.0]


# --- the fold without an arrival counter, in a child process
CHILD_CASES = [(d, n) for d in sorted(FUSED_D) for n in (257, 131073)]


def _child():
    """Run as a child process with OBE_CONTROL_SLOTS=0: no arrival counter, so the fused update takes
    normalize_moments_kernel<D, FOLD = false> and fold_update_moments_kernel."""
    assert os.environ.get("OBE_CONTROL_SLOTS") == "0"
    sys.path.insert(0, ROOT)
    from optbayesexpt_amd import _lib
    hip = _lib.load()
    out = {}
    for d, n in CHILD_CASES:
        cloud, prob, dev, w, h, mom, _ = _fused_case(hip, d, n)
        _expect(cloud, prob["shift"], w, h, f"FOLD = false d={d} n={n}")
        _same_bits(mom, dev.moments_of(w), "d_moments against obe_moments")
        out[f"{d},{n}"] = [hashlib.sha256(w.tobytes()).hexdigest(), h.tobytes().hex(), mom.tobytes().hex()]
    print("K2 FUSED " + json.dumps(out))


def test_fused_update_without_an_arrival_counter_leaves_the_same_bits(hip):
    env = dict(os.environ, OBE_CONTROL_SLOTS="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [s for s in r.stdout.splitlines() if s.startswith("K2 FUSED ")]
    assert len(line) == 1, r.stdout[-2000:]
    child = json.loads(line[0][len("K2 FUSED "):])
    for d, n in CHILD_CASES:
        _, _, _, w, h, mom, _ = _fused_case(hip, d, n)
        assert child[f"{d},{n}"] == [hashlib.sha256(w.tobytes()).hexdigest(), h.tobytes().hex(), mom.tobytes().hex()], \
            f"d={d} n={n}: FOLD = false against FOLD = true"


# =============================================================================== B. the likelihood on general doubles
def _record_worst(key, value, where):
    if value > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (value, where)


@functools.lru_cache(maxsize=None)
def _general_reference(case):
    p = uo.general_case(case)
    args = (p["y"], p["y_meas"], p["sig"], p["n_lik"], p["choke"])
    return p, uo.likelihood_ld(*args), uo.likelihood_bound(*args)


def _relative_u(got, ref):
    """max |got - ref| / (|ref| u) over the values whose reference is a normal float64."""
    ok = np.abs(ref) > 2.0 ** -1021
    return float((np.abs(got.astype(uo.LD) - ref)[ok] / (np.abs(ref[ok]) * uo.U)).max())


def test_libm_accuracy_measured(hip):
    """The device's exp and pow against long double on inputs that isolate them (one channel, sigma = 1, no choke:
    the likelihood IS exp(-a) with a reproduced bit for bit; sigma = 2^-j, z = 0 under a choke: it IS pow(2^j,
    choke)), in units of u = 2^-53 relative.  _update_oracle's constants must be these, rounded up, plus one."""
    import math
    p, ref, _ = _general_reference(uo.EXP_CASE)
    got = Dev(hip, uo.GENERAL_N, None, p["y"]).likelihood_y(p)
    assert np.all(got[ref < 1e-330] == 0.0) and np.count_nonzero(got) > 700
    exp_u = _relative_u(got, ref)
    pow_u = 0.0
    for case in uo.POW_CASES:
        p, ref, _ = _general_reference(case)
        pow_u = max(pow_u, _relative_u(Dev(hip, uo.GENERAL_N, p["particles"], p["y"]).likelihood_y(p), ref))
    print(f"device exp: worst {exp_u:.3f} u; device pow: worst {pow_u:.3f} u  (u = 2^-53 relative)")
    assert math.ceil(exp_u) + 1 <= uo.LIBM_EXP_ULPS <= 4, f"exp measured at {exp_u} u"
    assert math.ceil(pow_u) + 1 <= uo.LIBM_POW_ULPS <= 4, f"pow measured at {pow_u} u"


@pytest.mark.parametrize("case", [uo.EXP_CASE, *uo.POW_CASES] + uo.GENERAL_CASES, ids=str)
def test_likelihood_y_within_the_derived_bound(hip, case):
    """obe_likelihood_y: one launch up to 8 channels, groups of 8 multiplied up and choke_kernel beyond; where the
    record has at most 8 channels also the posterior through obe_bayes_update_y and, on the likelihood just
    computed, obe_bayes_update_lik — which leaves the same bits."""
    import _replay
    p, ref, bound = _general_reference(case)
    dev = Dev(hip, uo.GENERAL_N, p["particles"], p["y"])
    got = dev.likelihood_y(p)
    frac = uo.fraction_of_bound(got, ref, bound)
    worst = float(frac.max())
    key = f"likelihood, {'rows' if p['noise_rows'] is not None else 'fixed'}, choke {p['choke']}"
    print(f"{case}: worst |error| / bound {worst:.3g} (particle {int(frac.argmax())})")
    _record_worst(key, worst, str(case))
    assert worst <= 1.0, f"{case}: beyond the derived bound at particle {int(frac.argmax())}"
    if p["y"].shape[0] > MAX_CH:
        return
    w1, h = dev.update_y(p["w"], p)
    want, total = uo.posterior_ld(p["w"], ref)
    _replay.close_weights(w1, want.astype(np.float64), WEIGHT_RTOL, f"{case}: posterior through obe_bayes_update_y")
    b = uo.sum_t_bound(p["w"], ref, bound)
    err = abs(float(uo.LD(h[0]) - total))
    print(f"{case}: sum t, |error| / bound {err / b:.3g}")
    _record_worst("sum t", err / b, str(case))
    assert err <= b, f"{case}: sum t beyond its bound"
    w2, h2 = Dev(hip, uo.GENERAL_N).update_lik(p["w"], got)
    _same_bits(w2, w1, f"{case}: the likelihood form against the y form")
    _same_bits(h2, h, f"{case}: h_out, the likelihood form against the y form")


# =================================================================================================== C. the forms agree
def _model_case(name, n):
    """(model struct, particles (d, n), dict(setting, y_meas, sigma / noise_rows, choke), weights, settings (S, 261))
    of one built-in model on general doubles."""
    g = _rng(300 + sorted(MODEL_CASES).index(name), n)
    k = 261
    if name == "coil":
        p = np.stack([1e-3 * (1 + 0.1 * g.standard_normal(n)), 10 * (1 + 0.1 * g.standard_normal(n)),
                      1e-6 * (1 + 0.1 * g.standard_normal(n))])
        prob = dict(setting=[3.1e4], y_meas=[55.0, 30.0], sigma=[60.0, 45.0], choke=None)
        return _model("coil", 3), p, prob, [g.uniform(2e4, 4e4, k)]
    if name in ("lorentz1", "lorentz3_rows"):
        peaks = 1 if name == "lorentz1" else 3
        rows = [g.uniform(-2, 2, n) for _ in range(peaks)] + [g.normal(1, 0.1, n), g.normal(0, 0.1, n)]
        prob = dict(setting=[0.3], y_meas=[0.8], sigma=[0.4], choke=None)
        if peaks == 3:                                         # a noise row behind the model's, and a choke
            rows.append(0.3 + 0.2 * g.random(n))
            prob = dict(setting=[0.3], y_meas=[1.7], sigma=None, noise_rows=np.array([5], dtype=np.int32), choke=0.6)
        return _model(f"lorentz{peaks}", len(rows), (0.5,)), np.stack(rows), prob, [g.uniform(-3, 3, k)]
    if name == "rabi":
        p = np.stack([5 * (1 + 0.1 * g.standard_normal(n)), g.standard_normal(n)])
        prob = dict(setting=[0.1, 1.5], y_meas=[99800.0], sigma=[300.0], choke=1.7)
        return _model("rabi", 2, (100000.0, 0.01, 2.0)), p, prob, [g.uniform(0.01, 0.5, k), g.uniform(-3, 3, k)]
    assert name == "line_mb"
    p = np.stack([g.normal(2, 0.5, n), g.normal(-1, 0.5, n), g.normal(0, 1, n)])      # (a spare row)
    prob = dict(setting=[1.25], y_meas=[1.4], sigma=[0.7], choke=None)
    return _model("line_mb", 3), p, prob, [g.uniform(-5, 5, k)]


MODEL_CASES = {"coil": 2, "lorentz1": 1, "lorentz3_rows": 1, "rabi": 1, "line_mb": 1}         # name -> channels


@pytest.mark.parametrize("n", [777, 196609])
@pytest.mark.parametrize("name", sorted(MODEL_CASES))
def test_the_three_forms_of_pass_a_leave_the_same_bits(hip, name, n):
    """obe_bayes_update_model against obe_bayes_update_y on obe_eval_over_particles' output against
    obe_bayes_update_lik on obe_likelihood_y's output: the same likelihood_of on the same grid (csrc/obe_update.h:
    "the same update")."""
    m, particles, prob, _ = _model_case(name, n)
    c = MODEL_CASES[name]
    prob = dict(prob, n_lik=c)
    w = _rng(350, n).random(n) + 0.1
    w /= w.sum()
    dev = Dev(hip, n, particles)
    w_model, h_model = dev.update_model(w, m, prob)
    assert np.count_nonzero(w_model) > n // 2 and 0.5 < w_model.sum() < 1.5, "a posterior that keeps the cloud"
    y = dev.eval_over_particles(m, prob["setting"], c)
    dev_y = Dev(hip, n, particles, y)
    w_y, h_y = dev_y.update_y(w, prob)
    _same_bits(w_y, w_model, f"{name} n={n}: weights, y form against model form")
    _same_bits(h_y, h_model, f"{name} n={n}: h_out, y form against model form")
    lik = dev_y.likelihood_y(prob)
    w_lik, h_lik = Dev(hip, n).update_lik(w, lik)
    _same_bits(w_lik, w_model, f"{name} n={n}: weights, likelihood form against model form")
    _same_bits(h_lik, h_model, f"{name} n={n}: h_out, likelihood form against model form")


@pytest.mark.parametrize("name", sorted(MODEL_CASES))
def test_eval_over_settings_is_eval_over_particles_transposed(hip, name):
    """261 settings x 261 parameter sets: every (setting, parameters) pair once as one setting against many
    particles, once as one parameter set against many settings — the same bits; the padding of d_y_out untouched."""
    import torch
    k = 261
    m, particles, prob, settings = _model_case(name, k)
    c = MODEL_CASES[name]
    settings = np.stack(settings)
    dev = Dev(hip, k, particles)
    by_setting = np.stack([dev.eval_over_particles(m, settings[:, s], c) for s in range(k)])       # (setting, c, particle)
    sd = torch.from_numpy(_padded(settings, PAD_P)).cuda()
    out = torch.full((k, c, k + PAD_Y), SENTINEL, dtype=torch.float64, device="cuda")
    row_bytes = c * (k + PAD_Y) * 8
    for j in range(k):
        hip.call("obe_eval_over_settings", m, P(sd.data_ptr()), k + PAD_P, k, dev.host(np.ascontiguousarray(particles[:, j])),
                 P(out.data_ptr() + j * row_bytes), k + PAD_Y, dev.st)
    torch.cuda.synchronize()
    got = out.cpu().numpy()                                    # (particle, c, setting)
    _untouched(got[:, :, k:].reshape(-1), "obe_eval_over_settings: the padding of d_y_out")
    assert np.all(np.isfinite(by_setting))
    _same_bits(got[:, :, :k].transpose(2, 1, 0), by_setting, f"{name}: settings form against particles form")


# ============================================================================ D. the sweep batch is the sequential replay
SWEEP_POINTS = (-1.5, 0.9, -0.3, 0.6, 0.1, 0.3)


@functools.lru_cache(maxsize=None)
def _sweep_cloud(n):
    g = _rng(400, n)
    particles = np.stack([g.uniform(-2, 2, n), g.normal(1, 0.1, n), g.normal(0, 0.1, n)])
    y_meas = [[1.0 / (((x - 0.3) / 0.5) ** 2 + 1)] for x in SWEEP_POINTS]
    return particles, y_meas


def _replay_points(dev, m, w, sigma, y_meas, points, auto_resample, threshold):
    """obe_bayes_update_model point by point with the resample test on the host: (weights, [sum t, sum w'^2, flag,
    points applied], the N_eff / N of every point applied)."""
    trace, flag = [], 0.0
    for k in range(points):
        w, h = dev.update_model(w, m, dict(setting=[SWEEP_POINTS[k]], y_meas=y_meas[k], sigma=[sigma]))
        trace.append(1.0 / h[1] / dev.n)
        if auto_resample and uo.resample_due(h[1], dev.n, threshold):
            flag = 1.0
            break
    return w, np.array([h[0], h[1], flag, float(len(trace))]), trace


@pytest.mark.parametrize("n,strict", [(257, False), (196609, False), (257, True)])
def test_sweep_batch_is_the_sequential_replay(hip, n, strict):
    """sweep_prologue, normalize_kernel(stop) and fold2_stop_kernel against the replay: a stop after point 0, after a
    middle point (the launches behind it return at once: the sticky flag), at the last point, none; auto_resample
    off; one point; h_settings == NULL.  Both arms of resample_due: N_eff / N < threshold with thresholds above 0.1
    taken from the replay's own trace (sigma 0.4: N_eff / N falls from ~0.85 to ~0.19), and N_eff < 0.1 N with
    threshold 0 (sigma 0.1: below 0.1 from the third point on).  strict: the same with obe_strict_sums on (n = 257)."""
    particles, y_meas = _sweep_cloud(n)
    dev, m = Dev(hip, n, particles), _model("lorentz1", 3, (0.5,))
    w0 = np.full(n, 1.0 / n)
    points = len(SWEEP_POINTS)
    assert hip.cdll.obe_strict_sums(int(strict)) == 0
    try:
        _, _, trace = _replay_points(dev, m, w0, 0.4, y_meas, points, 0, 0.0)
        assert all(a > b for a, b in zip(trace, trace[1:])) and trace[-1] > 0.1 and trace[0] < 1.0, trace
        between = lambda k: 0.5 * (trace[k] + (trace[k - 1] if k else 1.0))         # a threshold that point k is the first to miss
        cases = [("a stop after point 0", 0.4, points, 1, between(0), 1, 1.0),
                 ("a stop after point 2", 0.4, points, 1, between(2), 3, 1.0),
                 ("a stop at the last point", 0.4, points, 1, between(points - 1), points, 1.0),
                 ("no stop", 0.4, points, 1, 0.5 * (trace[-1] + 0.1), points, 0.0),
                 ("auto_resample = 0", 0.4, points, 0, between(0), points, 0.0),
                 ("one point", 0.4, 1, 1, between(1), 1, 0.0),
                 ("one point that stops", 0.4, 1, 1, between(0), 1, 1.0),
                 ("threshold 0: N_eff < 0.1 N", 0.1, points, 1, 0.0, None, 1.0)]
        for what, sigma, k, auto, threshold, applied, flag in cases:
            assert threshold == 0.0 or threshold > 0.1
            want_w, want_h, tr = _replay_points(dev, m, w0, sigma, y_meas, k, auto, threshold)
            if applied is None:
                assert 2 <= want_h[3] < points and tr[-1] < 0.1 <= tr[-2], tr
            else:
                assert want_h[3] == applied and want_h[2] == flag, (what, want_h, tr)
            prob = dict(y_meas=y_meas[0], sigma=[sigma])
            got_w, got_h = dev.update_sweep(w0, m, prob, [[x] for x in SWEEP_POINTS[:k]], y_meas[:k], auto, threshold)
            _same_bits(got_h, want_h, f"n={n} {what}: h_out")
            _same_bits(got_w, want_w, f"n={n} {what}: weights")
        # h_settings == NULL is a sweep at setting 0
        prob = dict(y_meas=y_meas[0], sigma=[0.4])
        zero_w, zero_h = dev.update_sweep(w0, m, prob, [[0.0]] * 3, y_meas[:3], 0, 0.0)
        null_w, null_h = dev.update_sweep(w0, m, prob, [[9.0]] * 3, y_meas[:3], 0, 0.0, null_settings=True)
        _same_bits(null_w, zero_w, "h_settings == NULL: weights")
        _same_bits(null_h, zero_h, "h_settings == NULL: h_out")
    finally:
        assert hip.cdll.obe_strict_sums(0) == int(strict)


def test_enqueue_form_is_the_synchronous_fused_form(hip):
    """Weights and host block of obe_bayes_update_model_moments_enqueue equal the synchronous form's; word 4 + 4 D and
    OBE_WS_ABORT_WORD equal resample_due(h_out[1]) on both sides of a threshold; the refusals leave the weights alone."""
    n, d = 1000, 3
    particles, y_meas = _sweep_cloud(n)
    dev, m = Dev(hip, n, particles), _model("lorentz1", d, (0.5,))
    prob = dict(setting=[SWEEP_POINTS[0]], y_meas=y_meas[0], sigma=[0.4])
    w0 = np.full(n, 1.0 / n)
    w_sync, h_sync, mom_sync, _ = dev.update_fused(w0, m, prob)
    ratio = 1.0 / h_sync[1] / n
    assert 0.2 < ratio < 0.95
    for auto, threshold in ((1, ratio + 0.02), (1, ratio - 0.02), (0, ratio + 0.02), (1, 0.0)):
        w, h, mom, abort = dev.update_fused(w0, m, prob, (auto, threshold))
        _same_bits(w, w_sync, "enqueue: weights")
        _same_bits(h[:4 + 4 * d], h_sync, "enqueue: the host block")
        _same_bits(mom, mom_sync, "enqueue: d_moments")
        due = bool(auto) and uo.resample_due(h_sync[1], n, threshold)
        assert due == (auto == 1 and threshold > ratio)
        assert h[4 + 4 * d] == float(due) and abort == int(due), (auto, threshold)
    # the workspace an update carves: one word less is refused by the synchronous form too, exactly that is taken
    need = update_ws_bytes(d)
    ws = dev.workspace()
    w, h, _, _ = dev.update_fused(w0, m, prob, ws=ws, ws_bytes=need)
    _same_bits(w, w_sync, "a workspace of exactly update_ws_bytes")
    args = lambda wd, mom, ws_bytes, hp: (m, dev.ptr(dev.p), dev.ld_p, n, P(wd.data_ptr()), dev.setting(prob),
                                          *dev.lik_args(prob), P(mom.data_ptr()), P(ws.data_ptr()), ws_bytes, hp)
    pinned = dev._lib.pinned_array(5 + 4 * d)
    pageable = np.full(5 + 4 * d, SENTINEL)
    mom = dev.torch.full((2 + 4 * d,), SENTINEL, dtype=dev.torch.float64, device="cuda")
    for what, ws_bytes, host in (("a pageable h_out", dev.ws_bytes, pageable), ("no 16 spare bytes", need + 8, pinned),
                                 ("a short workspace", need - 8, pinned)):
        wd = dev.weights(w0)
        pinned[:] = SENTINEL
        rc = hip.cdll.obe_bayes_update_model_moments_enqueue(*args(wd, mom, ws_bytes, dev._lib.host_ptr(host)), 1, 0.5, dev.st)
        dev.torch.cuda.synchronize()
        assert rc == -1, what
        _same_bits(wd.cpu().numpy()[:n], w0, what + ": the weights are untouched")
        _untouched(mom.cpu().numpy(), what + ": d_moments")
        _untouched(host, what + ": h_out")
    wd = dev.weights(w0)
    assert hip.cdll.obe_bayes_update_model_moments(*args(wd, mom, need - 8, dev._lib.host_ptr(pageable)), dev.st) == -1
    _same_bits(wd.cpu().numpy()[:n], w0, "a short workspace, synchronous form: the weights are untouched")
    w, h, _, abort = dev.update_fused(w0, m, prob, (1, 0.0), ws=ws, ws_bytes=need + 16)
    _same_bits(w, w_sync, "16 spare bytes are enough")
    assert abort == 0


# ========================================================================================================= E. refusals
def test_refusals_leave_weights_and_outputs_untouched(hip):
    n = 300
    cloud = uo.exact_case(n)
    g = _rng(500)
    prob_y = uo.exact_y_problem(g, cloud, 3, 2, rows=True)
    prob_m = uo.exact_model_problem(g, cloud, "line_ab", 3, 2)
    dev_y = Dev(hip, n, prob_y["particles"], prob_y["y"])
    dev_m = Dev(hip, n, prob_m["particles"])
    wide = np.concatenate([prob_m["particles"], np.ones((14, n))])
    dev_17 = Dev(hip, n, wide)
    m3, m17 = _model("line_ab", 3), _model("line_ab", 17)
    w0 = cloud.prior()
    torch = dev_y.torch
    cdll = hip.cdll

    def refused(dev, what, call):
        """call(d_weights, d_ws, h_out, d_out) -> rc, with a guarded copy of everything a call could write."""
        wd = dev.weights(w0)
        h = np.full(4 + 4 * 17 + GUARD, SENTINEL)
        out = torch.full((max(n, 2 + 4 * 17) + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        ws = dev.workspace()
        rc = call(P(wd.data_ptr()), P(ws.data_ptr()), dev._lib.host_ptr(h), P(out.data_ptr()))
        torch.cuda.synchronize()
        assert rc == -1 and hip.last_error(), what
        got = wd.cpu().numpy()
        _same_bits(got[:n], w0, what + ": the weights")
        _untouched(got[n:], what + ": behind the weights")
        _untouched(h, what + ": h_out")
        _untouched(out.cpu().numpy(), what + ": the device output")
        assert np.all(np.isnan(ws.cpu().numpy())), what + ": the workspace"
        dev.inputs_unchanged(what)

    def y_call(dev, prob, n_particles=n, ws_bytes=None, null=()):
        def call(wd, ws, h, out):
            ym, sigma, rows, n_lik, choke = dev.lik_args(prob)
            return cdll.obe_bayes_update_y(dev.ptr(dev.y), dev.ld_y, dev.c, dev.ptr(dev.p), dev.ld_p, n_particles, wd,
                                           None if "y_meas" in null else ym, sigma, rows, n_lik, choke, ws,
                                           dev.ws_bytes if ws_bytes is None else ws_bytes, h, dev.st)
        return call

    def lik_y_call(dev, prob, null=()):
        def call(wd, ws, h, out):
            ym, sigma, rows, n_lik, choke = dev.lik_args(prob, width=prob["n_lik"])
            return cdll.obe_likelihood_y(dev.ptr(dev.y), dev.ld_y, dev.c, dev.ptr(dev.p), dev.ld_p, n,
                                         None if "y_meas" in null else ym, sigma, rows, n_lik, choke, out, dev.st)
        return call

    def model_call(dev, m, prob, form="model", n_particles=n, ws_bytes=None, null=()):
        def call(wd, ws, h, out):
            ym, sigma, rows, n_lik, choke = dev.lik_args(prob)
            head = (m, dev.ptr(dev.p), dev.ld_p, n_particles, wd, dev.setting(prob))
            lik = (None if "y_meas" in null else ym, sigma, rows, n_lik, choke)
            tail = (ws, dev.ws_bytes if ws_bytes is None else ws_bytes, h, dev.st)
            if form == "model":
                return cdll.obe_bayes_update_model(*head, *lik, *tail)
            if form == "fused":
                return cdll.obe_bayes_update_model_moments(*head, *lik, out, *tail)
            hy = dev.host(np.zeros((2, MAX_CH)))
            return cdll.obe_bayes_update_sweep(*head[:5], dev.host(np.zeros((2, MAX_SET))), None if "y_meas" in null else hy,
                                               *lik[1:], 2, 1, 0.5, *tail)
        return call

    prob_y = dict(prob_y, n_lik=2)
    refused(dev_y, "y: n_lik_channels > n_channels", y_call(dev_y, dict(prob_y, n_lik=4, y_meas=np.zeros(4),
                                                                        noise_rows=np.array([0, 1, 2, 3], dtype=np.int32))))
    refused(dev_y, "likelihood_y: n_lik_channels > n_channels",
            lik_y_call(dev_y, dict(prob_y, n_lik=4, y_meas=np.zeros(4), noise_rows=np.array([0, 1, 2, 3], dtype=np.int32))))
    for form in ("model", "fused", "sweep"):
        two = dict(prob_m, n_lik=2, y_meas=np.zeros(2), noise_rows=np.array([2, 2], dtype=np.int32))
        refused(dev_m, f"{form}: n_lik_channels > n_channels", model_call(dev_m, m3, two, form))
        for row in (3, -1):
            refused(dev_m, f"{form}: noise row {row} of a cloud of 3", model_call(
                dev_m, m3, dict(prob_m, noise_rows=np.array([row], dtype=np.int32)), form))
        refused(dev_m, f"{form}: NULL h_y_meas", model_call(dev_m, m3, prob_m, form, null=("y_meas",)))
        refused(dev_m, f"{form}: neither sigma nor rows", model_call(dev_m, m3, dict(prob_m, noise_rows=None), form))
        refused(dev_m, f"{form}: a short workspace", model_call(dev_m, m3, prob_m, form,
                                                                 ws_bytes=update_ws_bytes(3 if form == "fused" else 0) - 8))
        refused(dev_m, f"{form}: n_particles = 0", model_call(dev_m, m3, prob_m, form, n_particles=0))
    refused(dev_y, "y: a noise row outside any cloud", y_call(dev_y, dict(prob_y, noise_rows=np.array([0, 1024], dtype=np.int32))))
    refused(dev_y, "y: a negative noise row", y_call(dev_y, dict(prob_y, noise_rows=np.array([-1, 0], dtype=np.int32))))
    refused(dev_y, "y: NULL h_y_meas", y_call(dev_y, prob_y, null=("y_meas",)))
    refused(dev_y, "likelihood_y: NULL h_y_meas", lik_y_call(dev_y, prob_y, null=("y_meas",)))
    refused(dev_y, "y: neither sigma nor rows", y_call(dev_y, dict(prob_y, noise_rows=None)))
    refused(dev_y, "likelihood_y: neither sigma nor rows", lik_y_call(dev_y, dict(prob_y, noise_rows=None)))
    refused(dev_y, "y: a short workspace", y_call(dev_y, prob_y, ws_bytes=update_ws_bytes() - 8))
    refused(dev_y, "y: n_particles = 0", y_call(dev_y, prob_y, n_particles=0))
    refused(dev_y, "lik: a short workspace", lambda wd, ws, h, out: cdll.obe_bayes_update_lik(
        out, n, wd, ws, update_ws_bytes() - 8, h, dev_y.st))
    refused(dev_y, "lik: n_particles = 0", lambda wd, ws, h, out: cdll.obe_bayes_update_lik(
        out, 0, wd, ws, dev_y.ws_bytes, h, dev_y.st))
    refused(dev_17, "fused: n_params = 17", model_call(dev_17, m17, prob_m, "fused"))
    # ... and what was refused for its size alone is served at the size: a workspace of exactly update_ws_bytes, 17 rows unfused
    w, h = dev_17.update_model(w0, m17, prob_m)
    _expect(cloud, prob_m["shift"], w, h, "17 rows through the unfused form")
    dev_m.ws_bytes = update_ws_bytes()
    w, h = dev_m.update_model(w0, m3, prob_m)
    _expect(cloud, prob_m["shift"], w, h, "a workspace of exactly update_ws_bytes")


def test_worst_fractions_are_reported():
    """Prints the worst |error| / bound the general-double comparisons of this run measured, per noise form and choke
    (the figures of DESIGN.md's verification table)."""
    if WORST:
        print("K2 update, worst |error| / bound: " + "; ".join(f"{k} {v:.3g} ({where})" for k, (v, where) in WORST.items()))
    assert all(v <= 1.0 for v, _ in WORST.values())


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if sys.argv[1:] == ["child"]:
        _child()
