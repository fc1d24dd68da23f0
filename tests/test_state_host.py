"""Host side of save / load / pickle (no GPU): device models pickle as their recipes, snapshots of another format
version are refused, and a snapshot holds no torch tensor and no ctypes object."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import _fn_models


def _hand_tuned():
    from optbayesexpt_amd import models
    return [models.lorentzian(), models.lorentzian(7), models.line_ab(), models.line_mb(), models.first_parameter(),
            models.rabi(), models.coil()]


def _inputs(m, g):
    sets = tuple(g.uniform(1.0, 3.0, 9) for _ in range(m.n_setdims))
    pars = tuple(float(v) for v in g.uniform(0.5, 2.0, max(m.n_read, 3)))
    cons = tuple(float(v) for v in g.uniform(0.5, 2.0, m.n_consts))
    return sets, pars, cons


@pytest.mark.parametrize("k", range(7))
def test_hand_tuned_model_pickles_as_its_recipe(k):
    m = _hand_tuned()[k]
    r = pickle.loads(pickle.dumps(m))
    assert r is not m and r.spec() == m.spec() and r.spec()[0] == m.name.split("[")[0]
    assert (r.model_id, r.aux, r.n_read, r.n_setdims, r.n_channels, r.n_consts, r.safe_sweep) == \
        (m.model_id, m.aux, m.n_read, m.n_setdims, m.n_channels, m.n_consts, m.safe_sweep)
    sets, pars, cons = _inputs(m, np.random.default_rng(k))
    assert np.array_equal(np.asarray(r(sets, pars, cons)), np.asarray(m(sets, pars, cons)))


def test_lorentzian_recipe_names_its_peaks():
    from optbayesexpt_amd import models
    assert models.lorentzian(7).spec() == ("lorentzian", (7,))
    assert models.from_spec(("lorentzian", (7,))).aux == 7


def test_expression_model_pickles_as_its_recipe():
    from optbayesexpt_amd import models
    # (the expression of tests/_expr_models.py: its plugin is in the content-hash cache after build())
    m = models.from_expression("b + a / (((x - x0) / d)**2 + 1)", settings=("x",), parameters=("x0", "a", "b"),
                               constants=("d",))
    r = pickle.loads(pickle.dumps(m))
    assert r.spec() == m.spec() and r.plugin_path == m.plugin_path and r.name == m.name
    sets, pars, cons = _inputs(m, np.random.default_rng(5))
    assert np.array_equal(r(sets, pars, cons), m(sets, pars, cons))


def test_function_model_pickles_by_reference_and_is_translated_again():
    from optbayesexpt_amd import models
    m = models.from_function(_fn_models.lorentzian)
    blob = pickle.dumps(m)
    r = pickle.loads(blob)
    assert r.spec()[0] == "function" and r.spec()[1][0] is _fn_models.lorentzian
    assert r.expressions == m.expressions and r.plugin_path == m.plugin_path
    assert b"_fn_models" in blob and len(blob) < 300            # the function by reference, not by value


def test_model_without_recipe_refuses_to_pickle():
    from optbayesexpt_amd import models
    m = models.DeviceModel("handmade", models.MODEL_LINE_AB, 0, 2, 1, 1, 0, lambda s, p, c: p[0])
    with pytest.raises(TypeError, match="recipe"):
        pickle.dumps(m)


def _stub_pdf():
    """A ParticlePDF as the constructor leaves it, minus the device: host-only mirrors (no GPU here)."""
    from optbayesexpt_amd.particlepdf import ParticlePDF
    from optbayesexpt_amd._mirror import Mirror
    g = np.random.default_rng(2)
    o = ParticlePDF.__new__(ParticlePDF)
    o._device = torch.device("cpu")
    o._particles = Mirror(o._device, host=g.uniform(size=(3, 50)))
    o._weights = Mirror(o._device, host=np.full(50, 0.02))
    o.n_particles, o.n_dims = 50, 3
    o._rng = np.random.default_rng(4)
    o.tuning_parameters = dict(a_param=0.98, resample_threshold=0.5, auto_resample=True, scale=True)
    o.just_resampled = False
    o._pending_total = o._mom_dev_key = o._mom_host_key = o._sumsq_key = o._sumsq = None
    o.my_note = "kept"
    return o


def _walk(x, path="state"):
    assert not isinstance(x, torch.Tensor), path
    assert not isinstance(x, (ctypes._SimpleCData, ctypes.Structure, ctypes.Array, ctypes._Pointer)), path
    if isinstance(x, dict):
        for k, v in x.items():
            _walk(v, f"{path}[{k!r}]")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            _walk(v, f"{path}[{i}]")
    elif isinstance(x, np.ndarray):
        assert x.dtype != object, path


def test_snapshot_holds_only_host_data():
    from optbayesexpt_amd import _state
    o = _stub_pdf()
    st = _state.snapshot(o)
    _walk(st)
    assert st["format"] == _state.FORMAT_VERSION and st["cls"] == "optbayesexpt_amd.particlepdf:ParticlePDF"
    assert np.array_equal(st["particles"]["values"], o._particles._host)
    assert st["user"] == {"my_note": "kept"}
    assert isinstance(st["rng"], np.random.Generator)
    _walk(pickle.loads(pickle.dumps(st)))


@pytest.mark.parametrize("version", [None, 0, 2, "1"])
def test_other_format_version_is_refused(version):
    from optbayesexpt_amd import _state
    st = _state.snapshot(_stub_pdf())
    st["format"] = version
    with pytest.raises(ValueError, match=f"version {version!r}.*version {_state.FORMAT_VERSION}"):
        _state.restore(st)
