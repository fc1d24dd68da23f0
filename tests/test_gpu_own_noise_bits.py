"""The three classes whose likelihood and noise variance are passes of their own (OptBayesExptSignalNoise, -Binomial,
-Poisson; csrc/obe_signal_noise.hip, obe_binomial.hip, obe_poisson.hip) pinned to recorded bits: every output of their
C entry points at seeded inputs against tests/golden/own_noise_parent_bits.npz, np.array_equal on the uint64 view (NaN
positions must agree, NaN payloads are not compared).

The fixture was recorded on one MI355X with tools/record_own_noise_bits.py (which imports cases() and run() from this
file) from the build of commit 3fd8664, "Add OptBayesExptPoisson: counted events, exact information design": the last
commit in which each of the three files stated its own launch plan, pass scaffold and record head.  The shared forms
(csrc/obe_cloud_pass.h) perform the same operations in the same order, so they give these bits.  The file holds outputs
only; the inputs are made here from seeds.

What is recorded once and compared several times (the recorder asserts each of these equalities on the recording
build, so the fixture stays under 300 KB):
  * a pass over the first k settings of a grid gives the first k columns of the pass over the whole grid (a lane's sums
    do not depend on the other lanes): settings 1, 64 and 65 are compared with the columns of the 130-settings record;
    so is the slice [37, 101);
  * the likelihood of particle i depends on particle i alone, and on neither form (model values given, or evaluated in
    the kernel): 1, 65 and 257 particles are compared with the head of the 4 097-particle record, both forms with the
    one record.  With a choke the 4 097-particle record keeps the first 257 particles and every 16th after them
    (every workgroup of the launch sixteen times).

The shapes.  Settings 1, 64, 65, 130: one lane, a full tile, one padding tile, two tile edges.  Particles 1, 256, 257,
4 097: one chunk, the minimum-chunk edge, two chunks, seventeen chunks with a short last one.  65 536 settings x 2 100
particles (32 768 for Poisson): the grid bound decides the chunk count, 8 planned chunks of 320 of which 7 are used;
the first and the last 130 columns are kept (of the (cap + 1)-row histogram the first 130)."""
import os

import numpy as np
import pytest

import _binomial_oracle as binomial
import _poisson_oracle as poisson

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "own_noise_parent_bits.npz")
KINDS = ("signal_noise", "binomial", "poisson")
GRID, WIDTH = np.linspace(2.0, 4.0, 130), 0.1
OMEGAS, TIMES = np.linspace(1.0, 2.0, 65), poisson.TIMES
SETTINGS, PARTICLES, LIK_PARTICLES = (1, 64, 65, 130), (1, 256, 257, 4097), (1, 65, 257, 4097)
OUTPUTS = {"signal_noise": ("nu",), "binomial": ("info", "nu"), "poisson": ("info", "tail", "pmf", "nu")}
BOUND_SETTINGS = {"signal_noise": 65536, "binomial": 65536, "poisson": 32768}
BOUND_PARTICLES = 2100
# the per-call argument of the pass: {a, b, c} per channel; shots; exposure
PASS_ARG = {"signal_noise": [[0.25, 0.5, 0.01]], "binomial": 3.0, "poisson": 1.5}
COEF_TWO = [[0.01, 0.02, 0.0], [0.02, 0.0, 0.05]]
THIRD = ("0.3 + 0.4*exp(-t/T2)",)
CHOKED = np.union1d(np.arange(257), np.arange(0, 4097, 16))          # what a choked 4 097-particle record keeps
WORKSPACE_ARGS = {
    "obe_signal_noise_workspace_bytes": [(1, 1, 1), (4097, 130, 1), (7, 0, 1), (7, -5, 2), (7, 130, 0), (7, 65, 8),
                                         (1 << 20, 65536, 2), (7, 1 << 22, 1)],
    "obe_binomial_workspace_bytes": [(1, 1, 1), (4097, 130, 1), (7, 0, 1), (7, 130, 0), (7, 130, 2), (7, 130, 3),
                                     (7, 130, 4), (7, 130, 99), (1 << 20, 65536, 3), (7, 1 << 22, 1)],
    "obe_poisson_workspace_bytes": [(1, 1, 1, 16), (4097, 130, 1, 32), (7, 0, 1, 64), (7, 130, 0, 16), (7, 130, 99, 16),
                                    (7, 130, 1, 1), (7, 130, 1, 17), (7, 130, 1, 33), (7, 130, 1, 100), (7, 130, 2, 0),
                                    (1 << 20, 32768, 1, 64), (7, 1 << 22, 3, 32)],
}


# ------------------------------------------------------------------------------------------------ the inputs
def _lorentz_cloud(kind, n=4097):
    """(cloud (3, n), weights (n,)) of the one-peak Lorentzian: a probability for binomial, a rate for the others;
    the first columns of the 4 097-particle cloud, with its weights (not normalised again)."""
    g = np.random.default_rng(7100 + KINDS.index(kind))
    cloud = (binomial if kind == "binomial" else poisson).lorentz_cloud(g, 4097)
    return cloud[:, :n].copy(), poisson.weights(g, cloud)[:n].copy()


def _coil_cloud(n=129):
    """(3, n) L, R, C with both channels of the coil mostly inside [0, 1] at OMEGAS: probabilities and rates alike."""
    g = np.random.default_rng(7200)
    cloud = np.array([g.uniform(0.1, 0.4, n), g.uniform(0.2, 0.7, n), g.uniform(0.01, 0.05, n)])
    return cloud, poisson.weights(g, cloud)


def _decay_cloud(kind, n=129):
    """(3, n) a, b, T1 of poisson.DECAYS: rates, or (binomial) both channels inside [0.1, 0.7]."""
    g = np.random.default_rng(7300 + KINDS.index(kind))
    cloud = poisson.decay_cloud(g, n)
    if kind == "binomial":
        cloud = np.array([g.uniform(0.1, 0.4, n), g.uniform(0.1, 0.3, n), g.uniform(0.5, 2.0, n)])
    return cloud, poisson.weights(g, cloud)


def _model(name):
    import optbayesexpt_amd as obe
    if name == "lorentz":
        return obe.models.lorentzian(1), (WIDTH,)
    if name == "coil":
        return obe.models.coil(), ()
    if name == "decays":
        return obe.models.from_expression(poisson.DECAYS, settings=("t",), parameters=("a", "b", "T1")), ()
    if name == "ramsey3":
        return obe.models.from_expression(binomial.RAMSEY + THIRD, settings=("t",), parameters=("f", "T2")), ()
    raise KeyError(name)


def plugin_models():
    """The formula models of this file (the recorder builds their plugins ahead of the run)."""
    return [_model("decays")[0], _model("ramsey3")[0]]


def _object(kind, model, grid, cloud, w=None, **kw):
    import optbayesexpt_amd as obe
    cls = {"signal_noise": obe.OptBayesExptSignalNoise, "binomial": obe.OptBayesExptBinomial,
           "poisson": obe.OptBayesExptPoisson}[kind]
    m, cons = _model(model)
    kw.setdefault("scale", False)
    if kind == "poisson" and m.n_channels != 1:
        kw.setdefault("utility_method", "variance_approx")
    o = cls(m, (np.asarray(grid, dtype=np.float64),), cloud.copy(), cons, **kw)
    if w is not None:
        o.particle_weights = w
    return o


# ------------------------------------------------------------------------------------------------ the entry points
def _pass(kind, o, begin, end, arg, outputs=None, cap=16):
    """One call of the class's settings x cloud entry point on the settings [begin, end) of the object's grid, outputs
    pre-filled; a dict of the outputs asked for."""
    import torch
    from optbayesexpt_amd import _lib
    from optbayesexpt_amd.particlepdf import _P, _ptr
    outputs = OUTPUTS[kind] if outputs is None else outputs
    p, w = o._pw_tensors()
    n, n_p, n_c, dev = end - begin, p.shape[1], o.n_channels, o._device
    shapes = {"info": (n,), "tail": (n,), "pmf": (cap + 1, n), "nu": (n_c, n)}
    out = {k: torch.full(shapes[k], -7.0, dtype=torch.float64, device=dev) for k in outputs}
    ptr = lambda k: _ptr(out[k]) if k in out else None      # noqa: E731
    head = (o._model_struct, _P(o._settings_dev.data_ptr() + 8 * begin), o._n_settings, n, _ptr(p), n_p, n_p, _ptr(w))
    size = (n_p, n, n_c) + ((cap,) if kind == "poisson" else ())
    nbytes = int(getattr(o._mlib.cdll, f"obe_{kind}_workspace_bytes")(*size))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    if kind == "signal_noise":
        coef = np.ascontiguousarray(arg, dtype=np.float64)
        o._mlib.call("obe_signal_noise_variance", *head, _lib.host_ptr(coef), ptr("nu"), _ptr(ws), nbytes, o._stream())
    elif kind == "binomial":
        o._mlib.call("obe_binomial_information", *head, float(arg), None, 1.0, ptr("info"), ptr("nu"), _ptr(ws), nbytes,
                     o._stream())
    else:
        o._mlib.call("obe_poisson_information", *head, float(arg), cap, None, 1.0, ptr("info"), ptr("tail"), ptr("pmf"),
                     ptr("nu"), _ptr(ws), nbytes, o._stream())
    return {k: out[k].cpu().numpy() for k in outputs}


def _padded(values, fill=0.0):
    from optbayesexpt_amd import _lib
    a = np.full(_lib.OBE_MAX_CHANNELS, fill, dtype=np.float64)
    v = np.atleast_1d(np.asarray(values, dtype=np.float64))
    a[:v.size] = v
    return a


def _likelihood(kind, o, setting, record, n_lik, choke=None, given=False, coef=None):
    """One call of the class's likelihood entry point: the model evaluated in the kernel, or (given) the object's own
    model values handed in.  record: y_meas; (successes, shots); (counts, exposure)."""
    import math
    import torch
    from optbayesexpt_amd import _lib
    from optbayesexpt_amd.particlepdf import _ptr
    par = o._pw_tensors()[0]
    n_p = par.shape[1]
    x = np.zeros(_lib.OBE_MAX_SETDIMS)
    x[0] = setting
    if given:
        y = np.asarray(o.eval_over_all_parameters((setting,)), dtype=np.float64).reshape(o.n_channels, -1)
        y_dev = torch.from_numpy(np.ascontiguousarray(y)).to(o._device)
        y_args = (_ptr(y_dev), n_p, None, 0, n_p, None)
    else:
        y_args = (None, 0, _ptr(par), n_p, n_p, _lib.host_ptr(x))
    if kind == "signal_noise":
        host = [_padded(record), np.ascontiguousarray(coef, dtype=np.float64)]
    elif kind == "binomial":
        host = [_padded(record[0]), _padded(record[1], 1.0)]
    else:
        host = [_padded(record[0]), _padded(record[1], 1.0), _padded([math.lgamma(k + 1.0) for k in np.atleast_1d(record[0])])]
    out = torch.full((n_p,), -7.0, dtype=torch.float64, device=o._device)
    o._mlib.call(f"obe_{kind}_likelihood", o._model_struct, *y_args, *[_lib.host_ptr(h) for h in host], n_lik,
                 float("nan") if choke is None else float(choke), _ptr(out), o._stream())
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the cases
# name -> (function returning {output: array}, None or (the recorded case it is compared with, output -> the part of it))
_CASES = {}


def _case(name, ref=None):
    def keep(fn):
        _CASES[name] = (fn, ref)
        return fn
    return keep


def _columns(cols):
    return lambda key, a: a[..., cols]


def _pass_case(kind, n_p, n_s, begin=0):
    def fn():
        cloud, w = _lorentz_cloud(kind, n_p)
        return _pass(kind, _object(kind, "lorentz", GRID, cloud, w), begin, begin + n_s, PASS_ARG[kind])
    return fn


def _bound_case(kind):
    def fn():
        n_s = BOUND_SETTINGS[kind]
        cloud, w = _lorentz_cloud(kind, BOUND_PARTICLES)
        got = _pass(kind, _object(kind, "lorentz", np.linspace(2.0, 4.0, n_s), cloud, w), 0, n_s, PASS_ARG[kind])
        ends = np.r_[0:130, n_s - 130:n_s]
        return {k: np.ascontiguousarray(v[..., :130] if k == "pmf" else v[..., ends]) for k, v in got.items()}
    return fn


def _crafted(kind):
    """257 particles: weights with zeros, negatives and NaNs; model values NaN, below 0, above 1 (binomial), of infinite
    exposure x rate (Poisson, exposure 2)."""
    cloud, w = _lorentz_cloud(kind, 257)
    w[3::11], w[5::13], w[7::17] = 0.0, -w[5::13] - 1e-9, np.nan
    cloud[2, 4::19] = np.nan
    cloud[2, 6::23] = -20.0
    cloud[2, 8::29] = 5.0 if kind == "binomial" else 1.7e308
    return cloud, w


def _crafted_case(kind, nobody):
    def fn():
        cloud, w = _crafted(kind)
        arg = {"binomial": 3.0, "poisson": 2.0}[kind]
        return _pass(kind, _object(kind, "lorentz", GRID[:16], cloud, np.zeros(257) if nobody else w), 0, 16, arg)
    return fn


def _many_channels_case(kind, model):
    """The likelihood (a record with a zero count; all channels, and — two channels — the first alone) and the noise
    variance of a model of several channels."""
    def fn():
        grid = OMEGAS if model == "coil" else TIMES
        cloud, w = (_coil_cloud() if model == "coil" else
                    (binomial.ramsey_cloud(np.random.default_rng(7400), 129), None) if model == "ramsey3" else
                    _decay_cloud(kind))
        o = _object(kind, model, grid, cloud, w)
        n_c = o.n_channels
        record = {"signal_noise": [0.5, 0.4], "binomial": ([2, 0, 3][:n_c], [5, 3, 4][:n_c]),
                  "poisson": ([3, 0], [2.0, 1.5])}[kind]
        arg = {"signal_noise": COEF_TWO, "binomial": 2.0, "poisson": 2.0}[kind]
        out = {}
        for n_lik in range(n_c, 0, -1):
            out[f"lik{n_lik}"] = _likelihood(kind, o, float(grid[20]), record, n_lik, coef=COEF_TWO)
            assert _same(out[f"lik{n_lik}"], _likelihood(kind, o, float(grid[20]), record, n_lik, given=True, coef=COEF_TWO))
        out.update(_pass(kind, o, 0, grid.size, arg, outputs=OUTPUTS[kind] if kind == "binomial" else ("nu",)))
        return out
    return fn


RECORDS = {"signal_noise": {"plain": 6.5}, "binomial": {"plain": (2, 5)}, "poisson": {"plain": (7, 1.5)}}
ZERO_COUNTS = {"binomial": {"no_success": (0, 4), "no_failure": (4, 4)}, "poisson": {"no_event": (0, 2.0)}}


def _likelihood_case(kind, n_p, records=RECORDS):
    """Every record, both forms, without a choke and with 0.5."""
    def fn():
        cloud, _ = _lorentz_cloud(kind, n_p)
        o = _object(kind, "lorentz", GRID, cloud)
        out = {}
        for name, record in records[kind].items():
            for choke in (None, 0.5):
                key = name + ("" if choke is None else "_choked")
                out[key] = _likelihood(kind, o, 3.1, record, 1, choke, coef=PASS_ARG["signal_noise"])
                assert _same(out[key], _likelihood(kind, o, 3.1, record, 1, choke, given=True, coef=PASS_ARG["signal_noise"]))
                if choke is not None and n_p == 4097:
                    out[key] = out[key][CHOKED]
        return out
    return fn


def _head(n_p):
    def take(key, a):
        return a[CHOKED < n_p] if key.endswith("_choked") else a[:n_p]          # (CHOKED starts with 0 .. 256)
    return take


def _python_case(kind):
    """The public methods on the 4 097-particle cloud."""
    def fn():
        cloud, w = _lorentz_cloud(kind)
        kw = {"signal_noise": dict(noise_floor=0.5, noise_gain=0.5, noise_relative=0.1), "binomial": dict(shots=3),
              "poisson": dict(exposure=1.5, count_cap=16)}[kind]
        o = _object(kind, "lorentz", GRID, cloud, w, **kw)
        out = {"yvar": o.yvar_noise_model()}
        if kind != "signal_noise":
            out["information"] = o.utility_information()
        if kind == "poisson":
            out["counts"] = o.count_distribution((GRID[[5, 64, 129]],))
        record = {"signal_noise": ((3.1,), 6.5), "binomial": ((3.1,), 2, 5), "poisson": ((3.1,), 7, 1.5)}[kind]
        y = np.asarray(o.eval_over_all_parameters((3.1,))).reshape(1, -1)
        out["likelihood"] = o.likelihood(y, record)[:65]
        return out
    return fn


def _workspace_case():
    from optbayesexpt_amd import _lib
    cdll = _lib.load().cdll
    return {name: np.array([int(getattr(cdll, name)(*args)) for args in table], dtype=np.float64)
            for name, table in WORKSPACE_ARGS.items()}


for _kind in KINDS:
    for _n in PARTICLES:
        _CASES[f"{_kind}_pass_n{_n}_s130"] = (_pass_case(_kind, _n, 130), None)
        for _s in SETTINGS[:-1]:
            _CASES[f"{_kind}_pass_n{_n}_s{_s}"] = (_pass_case(_kind, _n, _s), (f"{_kind}_pass_n{_n}_s130", _columns(slice(0, _s))))
    _CASES[f"{_kind}_pass_slice_37_101"] = (_pass_case(_kind, 4097, 64, begin=37),
                                            (f"{_kind}_pass_n4097_s130", _columns(slice(37, 101))))
    _CASES[f"{_kind}_grid_bound"] = (_bound_case(_kind), None)
    _CASES[f"{_kind}_coil"] = (_many_channels_case(_kind, "coil"), None)
    _CASES[f"{_kind}_decays"] = (_many_channels_case(_kind, "decays"), None)
    for _n in LIK_PARTICLES:
        _CASES[f"{_kind}_likelihood_n{_n}"] = (_likelihood_case(_kind, _n),
                                               None if _n == 4097 else (f"{_kind}_likelihood_n4097", _head(_n)))
    _CASES[f"{_kind}_python"] = (_python_case(_kind), None)
for _kind in ("binomial", "poisson"):
    _CASES[f"{_kind}_crafted"] = (_crafted_case(_kind, False), None)
    _CASES[f"{_kind}_nobody"] = (_crafted_case(_kind, True), None)
    _CASES[f"{_kind}_likelihood_zero_counts"] = (_likelihood_case(_kind, 257, ZERO_COUNTS), None)
_CASES["binomial_three_channels"] = (_many_channels_case("binomial", "ramsey3"), None)
for _cap in (32, 64):
    def _cap_case(cap=_cap):
        cloud, w = _lorentz_cloud("poisson", 257)
        return _pass("poisson", _object("poisson", "lorentz", GRID, cloud, w), 0, 130, 1.5, ("info", "tail"), cap)
    _CASES[f"poisson_cap{_cap}"] = (_cap_case, None)


@_case("poisson_noise_var_alone")
def _cap_zero():
    cloud, w = _lorentz_cloud("poisson", 257)
    return _pass("poisson", _object("poisson", "lorentz", GRID, cloud, w), 0, 130, 1.5, ("nu",))


_CASES["workspace_bytes"] = (_workspace_case, None)


def cases():
    """The names of the cases, the recorded ones first."""
    return sorted(_CASES, key=lambda name: (_CASES[name][1] is not None, name))


def run(name):
    """{output: array} of one case from the library as built."""
    return _CASES[name][0]()


def expected(name, recorded):
    """{output: array} that run(name) must give, from the fixture's ``case:output`` entries."""
    ref = _CASES[name][1]
    if ref is None:
        return {k.split(":", 1)[1]: v for k, v in recorded.items() if k.split(":", 1)[0] == name}
    return {k: ref[1](k, v) for k, v in expected(ref[0], recorded).items()}


def _same(got, want):
    """The same bits; NaN where NaN, whatever the payload."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(got)
    return bool(np.array_equal(nan, np.isnan(want))
                and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)))


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("name", cases())
def test_outputs_have_the_recorded_bits(hip, recorded, name):
    got, want = run(name), expected(name, recorded)
    assert sorted(got) == sorted(want) and got, (name, sorted(got), sorted(want))
    for key in got:
        g, w = np.asarray(got[key], dtype=np.float64), want[key]
        assert g.shape == w.shape, (name, key, g.shape, w.shape)
        differ = np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w))).ravel())
        assert _same(g, w), (name, key, differ.size, differ[:5], g.ravel()[differ[:5]], w.ravel()[differ[:5]])
    if name.endswith("_nobody"):
        assert all(np.all(np.isnan(v)) for v in got.values())
