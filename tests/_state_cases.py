"""Experiments that tests/test_gpu_state.py copies, saves and restores, and the child-process side of it:

    python tests/_state_cases.py continue <dir> <case> ...   load <dir>/<case>.state, run CONTINUE cycles, write
                                                               <dir>/<case>.child.pkl
    python tests/_state_cases.py audit <dir>                  the deepcopy and save / load scenarios in one process
                                                               (run with OBE_CHECK_DELIVERY=1)

Every case is small; its measurements are a function of (case, cycle) alone, so any process continues it alike."""
import os
import pickle
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _fn_models  # noqa: E402
import optbayesexpt_amd as obe  # noqa: E402
from optbayesexpt_amd import models  # noqa: E402

BEFORE, CONTINUE = 10, 40
LORENTZ_TRUE = (3.0, -1000.0, 50000.0)
SIGMA = 500.0


def _lorentz_prior(g, n):
    return np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])


class Constrained(obe.OptBayesExpt):
    """A user subclass in the reference's test_zinference pattern: its own constructor keyword, extra attributes
    and a replaced enforce_parameter_constraints() in NumPy."""

    def __init__(self, *args, cost_of_changing_setting=1.0, **kwargs):
        super().__init__(*args, **kwargs)
        self.cost_of_changing_setting = cost_of_changing_setting
        self.constraint_calls = 0

    def enforce_parameter_constraints(self):
        self.constraint_calls += 1
        bad = np.argwhere(self.parameters[1] > -500.0)
        for index in bad:
            self.particle_weights[index] = 0
        self.particle_weights = self.particle_weights / np.sum(self.particle_weights)


def build(case, settings_shard=None):
    """A fresh object of ``case``, seeded (``settings_shard``: lorentz_full only)."""
    g = np.random.default_rng(sum(map(ord, case)))
    sv = (np.linspace(1.5, 4.5, 256),)
    kw = dict(utility_method="variance_full", default_noise_std=SIGMA)
    if case == "lorentz_full":
        o = obe.OptBayesExpt(models.lorentzian(), sv, _lorentz_prior(g, 16384), (0.1,), settings_shard=settings_shard,
                             **kw)
        o.tuning_parameters["speculative_sweep"] = True          # a speculative sweep is in flight after every update
    elif case == "strict4096":
        o = obe.OptBayesExpt(models.lorentzian(), sv, _lorentz_prior(g, 4096), (0.1,), **kw)
    elif case == "fused65536":
        o = obe.OptBayesExpt(models.lorentzian(), sv, _lorentz_prior(g, 65536), (0.1,), **kw)
    elif case == "noise7":                # c5's shape (7-peak Lorentzian, noise parameter row 9), small sizes
        n = 8192
        prior = np.vstack([g.uniform(2, 4, (7, n)), g.uniform(400, 2000, (1, n)), g.normal(500, 1000, (1, n)),
                           g.exponential(500, (1, n))])
        o = obe.OptBayesExptNoiseParameter(models.lorentzian(7), sv, prior, (0.1,), noise_parameter_index=9,
                                           scale=False, utility_method="variance_full")
    elif case == "sweeper":
        n = 8192
        prior = np.array([g.uniform(2, 4, n), g.uniform(400, 2000, n), g.normal(500, 1000, n), g.exponential(500, n)])
        o = obe.OptBayesExptSweeper(models.lorentzian(), (np.linspace(1.5, 4.5, 96),), prior, (0.1,), 3,
                                    scale=False, utility_method="variance_full")
    elif case == "expression":
        m = models.from_expression("b + a / (((x - x0) / d)**2 + 1)", settings=("x",), parameters=("x0", "a", "b"),
                                   constants=("d",))
        o = obe.OptBayesExpt(m, sv, _lorentz_prior(g, 16384), (0.1,), **kw)
    elif case == "function":
        o = obe.OptBayesExpt(models.from_function(_fn_models.lorentzian), sv, _lorentz_prior(g, 8192), (0.1,),
                             default_noise_std=SIGMA)                   # N_DRAWS weighted draws per sweep
    elif case == "mt19937":
        o = obe.OptBayesExpt(models.lorentzian(), sv, _lorentz_prior(g, 8192), (0.1,), default_noise_std=SIGMA)
        o.rng = np.random.Generator(np.random.MT19937(71))
        return o
    elif case == "subclass":
        o = Constrained(models.lorentzian(), sv, _lorentz_prior(g, 8192), (0.1,), cost_of_changing_setting=2.5, **kw)
    else:
        raise KeyError(case)
    o.rng = np.random.default_rng(sum(map(ord, case)) + 1)
    return o


def measure(o, case, cycle, x):
    """The record of the measurement at setting ``x`` in ``cycle``."""
    noise = np.random.default_rng([sum(map(ord, case)), cycle])
    if case == "sweeper":
        xs = o.sweep_settings[x[0]:x[1]]
        ys = o.model_function((xs,), (3.1, 1200.0, 300.0), (0.1,)) + 800.0 * noise.standard_normal(len(xs))
        return ((xs,), ys)
    if case == "noise7":
        true = (2.2, 2.5, 2.8, 3.1, 3.4, 3.7, 3.9, 1000.0, 500.0, 500.0)
        y = float(o.model_function(x, true, (0.1,))) + SIGMA * noise.standard_normal()
        return (x, y)
    y = float(o.model_function(x, LORENTZ_TRUE, (0.1,))) + SIGMA * noise.standard_normal()
    return (x, y, SIGMA)


def run(o, case, start, n, weights_log=None):
    """``n`` cycles from cycle ``start``: (setting indices, resampled flags).  The cloud is not read on the host
    in between (a host copy of it is state too: see _state.py)."""
    picks, resampled = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for cyc in range(start, start + n):
            x = o.opt_setting()
            picks.append(int(o.last_setting_index))
            o.pdf_update(measure(o, case, cyc, x))
            resampled.append(bool(o.just_resampled))
            if weights_log is not None:
                weights_log.append(np.array(o.particle_weights))
    return picks, resampled


def outcome(o, picks, resampled):
    return dict(picks=picks, resampled=resampled, particles=np.array(o.particles), weights=np.array(o.particle_weights),
                rng=o.rng.bit_generator.state)


def _continue(folder, cases):
    for case in cases:
        o = obe.load(os.path.join(folder, case + ".state"))
        res = outcome(o, *run(o, case, BEFORE, CONTINUE))
        res["user"] = {k: getattr(o, k) for k in ("cost_of_changing_setting", "constraint_calls") if hasattr(o, k)}
        res["cls"] = f"{type(o).__module__}:{type(o).__qualname__}"
        with open(os.path.join(folder, case + ".child.pkl"), "wb") as f:
            pickle.dump(res, f)


def _audit(folder):
    """The deepcopy and the save / load scenario of test_gpu_state.py, shortened, in one process."""
    import copy
    from optbayesexpt_amd._audit import audit
    assert audit.on
    case = "lorentz_full"
    o, twin = build(case), build(case)
    run(o, case, 0, BEFORE)
    run(twin, case, 0, BEFORE)
    c = copy.deepcopy(o)
    path = os.path.join(folder, "audit.state")
    obe.save(o, path)                      # (right behind the deepcopy: nothing in flight now, settled again)
    r = obe.load(path)
    got = [outcome(x, *run(x, case, BEFORE, 20)) for x in (o, c, twin, r)]
    for g in got[1:]:
        assert g["picks"] == got[0]["picks"]
        assert np.array_equal(g["particles"], got[0]["particles"]) and np.array_equal(g["weights"], got[0]["weights"])
        np.testing.assert_equal(g["rng"], got[0]["rng"])
    print("audit run ok", got[0]["picks"][:5])


if __name__ == "__main__":
    if sys.argv[1] == "continue":
        _continue(sys.argv[2], sys.argv[3:])
    elif sys.argv[1] == "audit":
        _audit(sys.argv[2])
    else:
        raise SystemExit(f"unknown mode {sys.argv[1]!r}")
