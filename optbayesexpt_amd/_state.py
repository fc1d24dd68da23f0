"""Snapshots of experiment objects: ``pickle``, ``copy.deepcopy``, ``save`` / ``load``.

An object of this package holds device tensors, page-locked landing zones, ctypes addresses, streams and a
sweep that may be in flight; none of that can be copied or written to a file.  Everything that decides what the
object computes next can be brought to the host exactly, though: the cloud and the weights (``Mirror``), the
NumPy ``Generator`` (authoritative on the host: ``_devrng.advance`` keeps it where numpy would be), the
constructor's arguments and a handful of counters.  ``snapshot()`` collects them into a plain dict; ``restore()``
builds a new object through its class's normal constructor (workspace sizing, plugin load,
``obe_model_validate``) and then hands it that state.  The restored object continues bit for bit where the
original stood.  The bins' kept grouping of the cloud (the buffer ``_bins_keep``; the key it was made for and the
"this cloud does not fit the bins" mark, both in ``SweepState``) is neither shared nor saved: a copy or a restored
object has no buffer and neither mark, rebuilds the grouping on its first bin sweep and gets the same bits.

Taking a snapshot first settles all work in flight (``settle()``): a speculative sweep is dropped (it is recomputed
on demand, with the same bits), the deferred check of a small draw's ``sum(w)`` runs, a constraint mask's
moments and count are waited for, and the device is drained.  Nothing else changes: the original object goes on
exactly as if no snapshot had been taken.

The snapshot of a settings-sharded object is the whole experiment (the state of its ranks is replicated); it can
be restored unsharded or as a shard of a new world of any size.
"""
import copy
import importlib

import numpy as np
import torch

from . import _drift, _lib
from ._mirror import Mirror

#: version of the snapshot layout; a snapshot of any other version is refused
FORMAT_VERSION = 1

#: public instance attributes the library sets itself: every OTHER public name in an object's ``__dict__`` is the
#: user's own (a subclass's ``cost_of_changing_setting``, a replaced hook) and travels with the snapshot as it is
LIBRARY_ATTRIBUTES = frozenset((
    # ParticlePDF
    "tuning_parameters", "n_particles", "n_dims", "just_resampled", "last_n_eff", "last_draw_indices_device",
    "last_resample_indices_device",
    # OptBayesExpt
    "model_function", "setting_values", "allsettings", "setting_indices", "cons", "choke", "N_DRAWS", "pickiness",
    "measurement_results", "last_setting_index", "n_channels", "utility_y_space", "default_noise_std",
    "utility_method", "utility", "get_setting", "last_sweep", "last_utility", "last_batch_update",
    "last_batch_design",
    # OptBayesExptNoiseParameter
    "noise_parameter_index",
    # OptBayesExptSignalNoise
    "noise_floor", "noise_gain", "noise_relative",
    # OptBayesExptSweeper
    "sweep_settings", "start_stop_subsample", "start_stop_indices", "start_stop_choice_indices", "start_stop_values",
    "cost_of_new_sweep", "last_sweep_batches",
))

#: The classes whose likelihood and noise variance are passes of their own (_ownnoise.py): (key of the snapshot,
#: module).  Each module has ``CLASS``, ``state_fields(obj)`` (what the snapshot keeps under the key),
#: ``kwargs_from_state(fields)`` (the constructor's keywords from it) and ``OWN_ATTRIBUTES``: what the library sets
#: besides LIBRARY_ATTRIBUTES on an object of that class only.
OWN_NOISE = (("signal_noise", "obe_signalnoise"), ("binomial", "obe_binomial"), ("poisson", "obe_poisson"))

_SELECTION ={"opt_setting": "optimal", "good_setting": "good", "random_setting": "random"}


def _own_noise():
    """(key, module) of OWN_NOISE, the modules imported."""
    return [(key, importlib.import_module(f"{__package__}.{name}")) for key, name in OWN_NOISE]


def _library_classes():
    from .obe_base import OptBayesExpt
    from .obe_noiseparam import OptBayesExptNoiseParameter
    from .particlepdf import ParticlePDF
    from .sweeper import OptBayesExptSweeper
    return (OptBayesExptSweeper, OptBayesExptNoiseParameter, *[m.CLASS for _, m in _own_noise()], OptBayesExpt,
            ParticlePDF)


def library_class(cls):
    """The class of this package whose constructor builds ``cls``'s objects again: the nearest one in its MRO
    (a user's subclass is rebuilt by it, and the subclass's own attributes are restored from the snapshot)."""
    known = _library_classes()
    for c in cls.__mro__:
        if c in known:
            return c
    raise TypeError(f"{cls.__name__} is not an optbayesexpt_amd class")


# ---------------------------------------------------------------------------------------------- snapshot
def settle(obj):
    """Finish or drop everything the object has in flight, so that its state can be read: the speculative sweep
    (dropped; the next request recomputes it with the same bits), an unchecked sum(w) of a small draw, a constraint
    mask's host words, then the device itself."""
    if "_sweeps" in obj.__dict__:
        obj._drop_speculative_sweep()
    obj._check_pending_total()
    obj._await_host_moments()
    if obj.__dict__.get("_constraint_pending"):
        obj.last_constraint_count            # (waits for the count's word)
    if obj._device.type == "cuda":
        torch.cuda.synchronize(obj._device)
        _lib.audit.synchronized()


def _mirror_state(m, on_device):
    """A Mirror's values and what the host knew of them.  ``on_device``: the values as a device-side clone (and the
    host copy, if one is valid, as a host copy) instead of one host array."""
    rec = dict(host_valid=bool(m._host_valid), host_born=bool(m.host_born), host=None)
    if on_device and m._dev_valid:
        rec["values"] = m._tensor.clone()
        if m._host_valid:
            rec["host"] = np.array(m._host)
    elif m._host_valid:
        rec["values"] = np.array(m._host)
    else:
        rec["values"] = m._tensor.cpu().numpy()
    return rec


def _mirror_from(device, rec):
    v = rec["values"]
    if isinstance(v, torch.Tensor):
        m = Mirror(device, tensor=v.to(device))
        if rec["host_valid"]:
            m._host, m._host_valid = np.array(rec["host"], dtype=np.float64), True
    elif rec["host_valid"]:
        m = Mirror(device, host=v)
    else:
        m = Mirror(device, tensor=torch.from_numpy(np.array(v, dtype=np.float64)).to(device))
    m.host_born = rec["host_born"]
    return m


def _model_spec(model, on_device):
    from .models import DeviceModel
    if on_device:
        return ("object", model)                 # (a copy in the same process shares the immutable model)
    if isinstance(model, DeviceModel):
        return ("device", model.spec())
    return ("host", model)                       # a host-callable model function: pickled by reference


def _model_from(spec):
    kind, what = spec
    if kind == "device":
        from .models import from_spec
        return from_spec(what)
    return what


def snapshot(obj, on_device=False):
    """The state of ``obj`` as a plain dict (see the module docstring).  Arrays are copies; the constructor's
    arguments and the user's own attributes are the object's own (``pickle`` and ``copy.deepcopy`` copy them).
    ``on_device``: the cloud, the weights and the moment block as device-side clones instead of host arrays
    (``copy.deepcopy``)."""
    from .obe_base import OptBayesExpt
    from .obe_noiseparam import OptBayesExptNoiseParameter
    from .sweeper import OptBayesExptSweeper
    settle(obj)
    cls = type(obj)
    pm, wm = obj._particles, obj._weights
    cloud = (pm.version, wm.version)
    st = dict(format=FORMAT_VERSION, cls=f"{cls.__module__}:{cls.__qualname__}",
              particles=_mirror_state(pm, on_device), weights=_mirror_state(wm, on_device),
              rng=obj._rng, tuning_parameters=obj.tuning_parameters, just_resampled=bool(obj.just_resampled))
    if "last_n_eff" in obj.__dict__:
        st["last_n_eff"] = float(obj.last_n_eff)
    # the reductions already formed for this cloud: a fresh pass would add in another order (the fused update's
    # moments are not obe_moments' bits), and the next sweep's shift and nudge read them
    dk, hk = obj._mom_dev_key, obj._mom_host_key
    mom = dict(dev=None if dk is None or dk[:2] != cloud else bool(dk[2]),
               host=None if hk is None or hk[:2] != cloud else bool(hk[2]))
    if mom["dev"] is not None:
        mom["dev_values"] = obj._moments_dev.clone() if on_device else obj._moments_dev.cpu().numpy()
    if mom["host"] is not None:
        mom["host_values"] = np.array(obj._moments_host[:])      # (a checked read under OBE_CHECK_DELIVERY)
    st["moments"] = mom
    st["sumsq"] = float(obj._sumsq) if obj._sumsq_key == wm.version and obj._sumsq is not None else None
    if obj.__dict__.get("_drift") is not None:       # (only when set: objects that never were write the snapshots they did)
        st["parameter_drift"] = _drift.copy(obj._drift)

    if isinstance(obj, OptBayesExpt):
        getter = getattr(obj.get_setting, "__name__", "opt_setting")
        st.update(model=_model_spec(obj.model_function, on_device), setting_values=obj.setting_values,
                  cons=obj.cons, N_DRAWS=obj.N_DRAWS, choke=obj.choke, pickiness=obj.pickiness,
                  default_noise_std=np.array(obj.default_noise_std), utility_method=obj.utility_method,
                  selection_method=_SELECTION.get(getter, "optimal"),
                  last_setting_index=obj.last_setting_index, measurement_results=obj.measurement_results,
                  utility_y_space=np.array(obj.utility_y_space), last_sweep=obj.__dict__.get("last_sweep"),
                  sharded_sweeps=int(obj._sharded_sweeps),
                  parameters=None if obj._parameters is pm else _mirror_state(obj._parameters, on_device),
                  parameter_bounds=obj.parameter_bounds)
        if "_changed_pinned" in obj.__dict__:
            st["constraint_count"] = obj.last_constraint_count
        if obj._interest is not None:            # (only when set: objects that never were write the snapshots they did)
            st["parameters_of_interest"] = dict(dims=obj._interest[0], weights=np.array(obj._interest[1]))
        s = obj._sweeps
        # (the counters that decide the next sweep's form and shift; versions are kept as "is it this cloud")
        st["sweeps"] = dict(safe_streak=s.safe_streak, safe_run=s.safe_run, unshifted=s.unshifted, streak=s.streak,
                            resample_rate=s.resample_rate, unavailable=s.unavailable,
                            range_hint_seen=s.range_hint_key == pm.version, updated_cloud=s.updated_cloud == cloud)
    if isinstance(obj, OptBayesExptNoiseParameter):
        st["noise_parameter_index"] = np.array(obj.noise_parameter_index)
        st["constraint_count"] = obj.last_constraint_count
    for key, module in _own_noise():
        if isinstance(obj, module.CLASS):
            st[key] = module.state_fields(obj)
    if isinstance(obj, OptBayesExptSweeper):
        st["sweeper"] = {k: getattr(obj, k) for k in ("sweep_settings", "start_stop_subsample", "start_stop_indices",
                                                      "start_stop_choice_indices", "start_stop_values",
                                                      "cost_of_new_sweep")}
        st["sweeper"]["last_sweep_batches"] = list(obj.__dict__.get("last_sweep_batches", []))
    st["user"] = user_attributes(obj)
    return st


def user_attributes(obj):
    """The public names in ``obj.__dict__`` that the library did not set on an object of this class: the user's own,
    which travel with the snapshot as they are."""
    own = LIBRARY_ATTRIBUTES.union(*[m.OWN_ATTRIBUTES for _, m in _own_noise() if isinstance(obj, m.CLASS)])
    return {k: v for k, v in obj.__dict__.items() if not k.startswith("_") and k not in own}


# ---------------------------------------------------------------------------------------------- restore
def _resolve(path):
    module, _, qualname = path.partition(":")
    target = importlib.import_module(module)
    for part in qualname.split("."):
        target = getattr(target, part)
    return target


def check_version(state):
    got = state.get("format") if isinstance(state, dict) else None
    if got != FORMAT_VERSION:
        raise ValueError(f"optbayesexpt_amd state of format version {got!r}: this package reads version "
                         f"{FORMAT_VERSION} only")


def restore(state, device=None, settings_shard=None, into=None):
    """A new object (or ``into``, an instance made by ``cls.__new__``) built from ``state``: the class's normal
    constructor on the saved arguments, then the saved state.  ``device``: where (default: the current torch
    device); ``settings_shard``: a :class:`~optbayesexpt_amd.dist.SettingsShard` of the world it becomes part of
    (collective: every rank restores the same state)."""
    from .obe_base import OptBayesExpt
    from .obe_noiseparam import OptBayesExptNoiseParameter
    from .sweeper import OptBayesExptSweeper
    check_version(state)
    cls = type(into) if into is not None else _resolve(state["cls"])
    base = library_class(cls)
    obj = into if into is not None else cls.__new__(cls)
    tp = copy.deepcopy(state["tuning_parameters"])
    prec = state["particles"]
    prior = prec["values"]
    model = _model_from(state["model"]) if "model" in state else None
    if isinstance(prior, torch.Tensor):
        # (a copy in this process: the constructor only sizes the cloud — unless a host-callable model is evaluated
        # on it for its channel count)
        from .models import DeviceModel
        prior = np.zeros(tuple(prior.shape)) if model is None or isinstance(model, DeviceModel) \
            else prior.cpu().numpy()
    pdf_kw = dict(a_param=tp["a_param"], resample_threshold=tp["resample_threshold"],
                  auto_resample=tp["auto_resample"], scale=tp["scale"], device=device)
    if not issubclass(base, OptBayesExpt):
        if settings_shard is not None:
            raise TypeError("a ParticlePDF has no settings axis to shard")
        base.__init__(obj, prior, **pdf_kw)
    else:
        args = (model, state["setting_values"], prior, state["cons"])
        kw = dict(n_draws=state["N_DRAWS"], choke=state["choke"], utility_method=state["utility_method"],
                  selection_method=state["selection_method"], pickiness=state["pickiness"],
                  default_noise_std=state["default_noise_std"], settings_shard=settings_shard, **pdf_kw)
        if base is OptBayesExptSweeper:
            base.__init__(obj, *args, state["noise_parameter_index"], **kw)
        elif base is OptBayesExptNoiseParameter:
            base.__init__(obj, *args, noise_parameter_index=state["noise_parameter_index"], **kw)
        else:
            for key, module in _own_noise():
                if base is module.CLASS:
                    kw.update(module.kwargs_from_state(state[key]))
            base.__init__(obj, *args, **kw)
    dev = obj._device

    obj.tuning_parameters = tp
    obj._particles = _mirror_from(dev, prec)
    obj._weights = _mirror_from(dev, state["weights"])
    pm, wm = obj._particles, obj._weights
    cloud = (pm.version, wm.version)
    obj.just_resampled = state["just_resampled"]
    if "last_n_eff" in state:
        obj.last_n_eff = state["last_n_eff"]
    mom = state["moments"]
    if mom["dev"] is not None:
        obj._moments_dev.copy_(torch.as_tensor(mom["dev_values"]).to(dev))
        obj._mom_dev_key = cloud + (mom["dev"],)
    if mom["host"] is not None:
        obj._moments_host[:] = mom["host_values"]
        obj._mom_host_key = cloud + (mom["host"],)
    if state["sumsq"] is not None:
        obj._sumsq, obj._sumsq_key = state["sumsq"], wm.version
    drift = state.get("parameter_drift")                 # (absent: never set, or a state written before)
    if drift is not None:
        obj._drift = dict(rows=np.array(drift["rows"], dtype=np.int32), cholesky=np.array(drift["cholesky"], dtype=np.float64),
                          per_update=bool(drift["per_update"]), at_bounds=drift["at_bounds"])

    if isinstance(obj, OptBayesExpt):
        par = state["parameters"]
        obj._parameters = pm if par is None else _mirror_from(dev, par)
        obj.last_setting_index = state["last_setting_index"]
        obj.measurement_results = copy.copy(state["measurement_results"])
        obj.utility_y_space = np.array(state["utility_y_space"])
        if state["last_sweep"] is not None:
            obj.last_sweep = dict(state["last_sweep"])
        obj._sharded_sweeps = state["sharded_sweeps"]
        sw, s = state["sweeps"], obj._sweeps
        s.safe_streak, s.safe_run, s.unshifted = sw["safe_streak"], sw["safe_run"], sw["unshifted"]
        s.streak, s.resample_rate, s.unavailable = sw["streak"], sw["resample_rate"], sw["unavailable"]
        s.range_hint_key = pm.version if sw["range_hint_seen"] else None
        s.updated_cloud = cloud if sw["updated_cloud"] else None
        # (a state written before there were bounds has none)
        obj._adopt_bounds(state.get("parameter_bounds"))
        interest = state.get("parameters_of_interest")          # (absent: never set, or a state written before)
        if interest is not None:
            obj.set_parameters_of_interest(interest["dims"], interest["weights"])
    if "constraint_count" in state:
        changed = obj._changed_pinned = _lib.pinned_array(1, np.int64)
        changed[0] = state["constraint_count"]
        obj._constraint_pending = False
    if isinstance(obj, OptBayesExptSweeper):
        for k, v in state["sweeper"].items():
            setattr(obj, k, copy.copy(v))
        obj._pairs_key = None
    for k, v in state["user"].items():
        setattr(obj, k, v)
    # last: a sharded object's replicas adopt rank 0's generator here, as at construction (_sync_rng)
    obj.rng = state["rng"]
    return obj


# ---------------------------------------------------------------------------------------------- the public forms
def deepcopy(obj, memo):
    """``copy.deepcopy``: the cloud, the weights and the moment block are cloned on the device; workspaces,
    landing zones and the sweep state are the new object's own; the (immutable) device model is shared."""
    if obj.__dict__.get("_shard") is not None:
        raise TypeError("copy.deepcopy of a settings-sharded object would need a collective that no other rank "
                        "calls: save it with optbayesexpt_amd.save() and restore it with optbayesexpt_amd.load()")
    st = snapshot(obj, on_device=True)
    keep = [st["particles"]["values"], st["weights"]["values"], st["moments"].get("dev_values")]
    if st.get("parameters"):
        keep.append(st["parameters"]["values"])
    if "model" in st:
        keep.append(st["model"][1])
    for x in keep:
        if x is not None:
            memo[id(x)] = x               # (already cloned / shared: not copied again)
    new = type(obj).__new__(type(obj))
    memo[id(obj)] = new                   # (a user attribute that refers back to the object gets the copy)
    return restore(copy.deepcopy(st, memo), device=obj._device, into=new)


def save(obj, path):
    """Write ``obj``'s state to ``path`` (a pickle of the snapshot dict)."""
    import pickle
    st = snapshot(obj)
    with open(path, "wb") as f:
        pickle.dump(st, f, protocol=pickle.HIGHEST_PROTOCOL)


def load(path, device=None, settings_shard=None):
    """The object saved at ``path``, restored on ``device`` (default: the current torch device), optionally as
    a shard of a new world (``settings_shard``, collective)."""
    import pickle
    with open(path, "rb") as f:
        st = pickle.load(f)
    return restore(st, device=device, settings_shard=settings_shard)
