"""Declarative parameter bounds, the part that needs no device: the NumPy oracle the GPU tests compare with is pinned
against the two constraint hooks it generalises, set_parameter_bounds() normalises every argument form to the same
arrays and refuses bad ones before any library call, snapshots carry the bounds, and the new entry points refuse bad
arguments with status -1 without touching a device."""
import numpy as np
import pytest

import _constraint_oracle as co
import oracle
from oracle import models as omodels
from optbayesexpt_amd import _audit, _bounds, _lib
from optbayesexpt_amd.obe_base import OptBayesExpt
from optbayesexpt_amd.obe_noiseparam import OptBayesExptNoiseParameter

INF = np.inf


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _cloud(seed, d, n):
    g = np.random.default_rng(seed)
    x = g.normal(0.1, 1.0, (d, n))
    x[:, ::17] = 0.0                  # values exactly on a bound of 0, both signs
    x[:, 5::31] = -0.0
    w = g.random(n)
    w[::13] = 0.0
    return x, w / w.sum()


# ------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("rows", [(3,), (1, 3)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_is_the_noise_parameter_hook(rows, seed):
    """sigma <= 0 on the noise rows (obe_noiseparam.py:57-79) = bounds (0, None), lower end exclusive, on those rows."""
    x, w = _cloud(seed, 4, 1500)
    model = omodels.coil if len(rows) == 2 else omodels.line_mb
    ref = oracle.OracleOptBayesExptNoiseParameter(model, (np.linspace(0.1, 1, 5),), x.copy(), (),
                                                  noise_parameter_index=rows if len(rows) > 1 else rows[0])
    ref.particle_weights = w.copy()
    ref.enforce_parameter_constraints()
    got, count = co.apply_bounds(x, w, *co.full(4, {r: (0.0, None) for r in rows}, lower_open=rows))
    np.testing.assert_array_equal(got, ref.particle_weights)
    assert count == np.count_nonzero(np.any(x[list(rows)] <= 0, axis=0)) > 0
    # nothing violates: the weights are returned as they are (no division by a sum that is not exactly 1)
    same, none = co.apply_bounds(np.abs(x) + 1.0, w, *co.full(4, {r: (0.0, None) for r in rows}, lower_open=rows))
    assert none == 0
    np.testing.assert_array_equal(same, w)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_is_the_lockin_hook(seed):
    """The lock-in demo's hook (demos/lockin/lockin_of_coil.py:115-133) in our own words: row by row, every particle
    whose value is < 0 gets weight 0; if any row had one, the weights are divided by their sum."""
    x, w = _cloud(seed, 4, 1500)
    want, any_change = w.copy(), False
    for row in x:
        below = np.flatnonzero(row < 0)
        if below.size:
            any_change = True
            for k in below:
                want[k] = 0
    if any_change:
        want = want / np.sum(want)
    got, count = co.apply_bounds(x, w, *co.full(4, {r: (0.0, None) for r in range(4)}))
    np.testing.assert_array_equal(got, want)
    assert count == np.count_nonzero(np.any(x < 0, axis=0)) > 0
    on_bound = np.any(x == 0, axis=0) & ~np.any(x < 0, axis=0)        # 0.0 and -0.0 do not violate an inclusive 0
    assert on_bound.any() and np.all((got[on_bound] > 0) == (w[on_bound] > 0))


def test_oracle_edges():
    x = np.array([[0.0, -0.0, 5e-324, -5e-324, np.nan, INF, -INF, 1.0, np.nextafter(1.0, 2), np.nextafter(1.0, 0)]])
    w = np.full(10, 0.1)
    bad = lambda *a: co.violators(x, *[np.array([v]) for v in a]).tolist()      # noqa: E731
    assert bad(0.0, INF, False, False) == [False, False, False, True, False, False, True, False, False, False]
    assert bad(0.0, INF, True, False) == [True, True, False, True, False, False, True, False, False, False]
    assert bad(-INF, 1.0, False, False) == [False] * 5 + [True, False, False, True, False]
    assert bad(-INF, 1.0, False, True) == [False] * 5 + [True, False, True, True, False]
    assert bad(1.0, 1.0, False, False) == [True] * 4 + [False, True, True, False, True, True]
    out, count = co.apply_bounds(x, w, np.array([2.0]), np.array([3.0]), np.array([False]), np.array([False]))
    assert count == 9 and out[4] == 1.0                     # (only the NaN value survives)
    out, count = co.apply_bounds(x[:, :4], w[:4], np.array([2.0]), np.array([3.0]), np.array([False]), np.array([False]))
    assert count == 4 and np.all(np.isnan(out))             # every particle violates: 0 / 0


# ------------------------------------------------------------------------------------- set_parameter_bounds
class _NoLibrary:
    """Stands where an object keeps its library: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def _bare(cls=OptBayesExpt, n_dims=4, **attrs):
    """An object of the class with just what set_parameter_bounds() may touch, and no library behind it."""
    o = object.__new__(cls)
    o.n_dims = n_dims
    o._lib = o._mlib = _NoLibrary()
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def _same(a, b):
    assert (a is None) == (b is None)
    for x, y in zip(a or (), b or ()):
        assert x.dtype == y.dtype
        np.testing.assert_array_equal(x, y)


def test_every_argument_form_normalises_to_the_same_arrays():
    want = (np.array([-INF, 0.0, 0.995, -INF]), np.array([INF, INF, 1.02, 1.0]), np.zeros(4, bool), np.zeros(4, bool))
    forms = [{1: (0.0, None), 2: (0.995, 1.02), 3: (None, 1.0)},
             {-3: (0, INF), -2: (0.995, 1.02), -1: (-INF, 1)},
             [None, (0.0, None), (0.995, 1.02), (None, 1.0)],
             ((None, None), (0, INF), [0.995, 1.02], (-INF, 1.0)),
             {1: (np.float64(0), None), 2: np.array([0.995, 1.02]), 3: (None, np.int64(1))}]
    for form in forms:
        o = _bare()
        assert o.parameter_bounds is None
        o.set_parameter_bounds(form)
        _same(o.parameter_bounds, want)
        for inc in (True, {1: True}, [True] * 4, {2: (True, True), -1: True}, [None, True, (True, True), None]):
            o.set_parameter_bounds(form, inclusive=inc)
            _same(o.parameter_bounds, want)
    # exclusive ends: only where there is a bound
    o = _bare()
    o.set_parameter_bounds(forms[0], inclusive=False)
    _same(o.parameter_bounds, want[:2] + (np.array([False, True, True, False]), np.array([False, False, True, True])))
    for inc in ({1: False, 2: (False, False), 3: False}, [True, False, False, (True, False)],
                {0: False, 1: (False, True), 2: False, -1: (True, False)}):
        o.set_parameter_bounds(forms[2], inclusive=inc)
        _same(o.parameter_bounds, want[:2] + (np.array([False, True, True, False]), np.array([False, False, True, True])))
    o.set_parameter_bounds(forms[0], inclusive={2: (True, False)})
    _same(o.parameter_bounds, want[:2] + (np.zeros(4, bool), np.array([False, False, True, False])))
    # what the library is given: the bounded rows only, bit 0 = lower end exclusive, bit 1 = upper end
    rows, lower, upper, flags = _bounds.pack(o.parameter_bounds)
    assert rows.dtype == np.int32 and flags.dtype == np.int32
    assert rows.tolist() == [1, 2, 3] and flags.tolist() == [0, 2, 0]
    assert lower.tolist() == [0.0, 0.995, -INF] and upper.tolist() == [INF, 1.02, 1.0]
    # the property hands out copies
    o.parameter_bounds[0][:] = 7.0
    assert o.parameter_bounds[0][1] == 0.0
    # cleared; bounds that bound nothing enforce nothing
    o.set_parameter_bounds(None)
    assert o.parameter_bounds is None and o._device_constraint() is None
    o.set_parameter_bounds([None] * 4)
    assert o.parameter_bounds is not None and o._device_constraint() is None
    o.set_parameter_bounds({1: (0.0, None)})
    assert o._device_constraint()[:2] == ("obe_mask_bounds", "obe_resample_particles_aos_bounded")


def test_refusals_come_before_any_library_call():
    o = _bare()
    o.set_parameter_bounds({0: (1.0, 2.0)})
    kept = o.parameter_bounds
    for bad in ({4: (0, 1)}, {-5: (0, 1)}, [(0, 1)] * 4 + [None]):
        with pytest.raises((IndexError, ValueError)) as e:
            o.set_parameter_bounds(bad)
        assert e.type is (IndexError if isinstance(bad, dict) else ValueError)
    with pytest.raises(IndexError):
        o.set_parameter_bounds({0: (0, 1)}, inclusive={7: False})
    for bad, inc in (({1: (np.nan, 1.0)}, True), ({1: (0.0, np.nan)}, True), ({1: (2.0, 1.0)}, True),
                     ({1: (1.0, 1.0)}, False), ({1: (1.0, 1.0)}, {1: (True, False)}), ({1: (1.0, 1.0)}, {1: (False, True)}),
                     ({1: 3.0}, True), ({1: (1.0, 2.0), -3: (0.0, 5.0)}, True), ([(0, 1)] * 3, True)):
        with pytest.raises(ValueError):
            o.set_parameter_bounds(bad, inclusive=inc)
    _same(o.parameter_bounds, kept)                   # a refused call leaves the bounds as they were
    o.set_parameter_bounds({1: (1.0, 1.0)})           # lower == upper, both ends inclusive: allowed
    wide = _bare(n_dims=40)
    wide.set_parameter_bounds({r: (0.0, None) for r in range(_lib.OBE_MAX_DIMS)})
    with pytest.raises(ValueError, match="OBE_MAX_DIMS"):
        wide.set_parameter_bounds({r: (0.0, None) for r in range(_lib.OBE_MAX_DIMS + 1)})
    with pytest.raises(ValueError, match="OBE_MAX_DIMS"):
        wide.set_parameter_bounds([(None, 1.0)] * 40)


def test_noise_parameter_class_intersects_with_positive_noise():
    """The user's bounds and the class's own sigma > 0 on the noise rows become one set of bounds."""
    def noise_obj(rows):
        keep = np.zeros(_lib.OBE_MAX_DIMS, dtype=np.int32)
        keep[:len(rows)] = rows
        return _bare(OptBayesExptNoiseParameter, 4, _noise_rows=keep, n_channels=len(rows), _hargs=_lib.HostArgs())
    o = noise_obj([3])
    assert o._device_constraint()[:2] == ("obe_mask_nonpositive", "obe_resample_particles_aos_masked")
    o.set_parameter_bounds({0: (None, 1.0), 1: (0.0, None)})
    _same(o.parameter_bounds, co.full(4, {0: (None, 1.0), 1: (0.0, None)}))            # as given
    _same(o._effective_bounds(o._parameter_bounds), co.full(4, {0: (None, 1.0), 1: (0.0, None), 3: (0.0, None)},
                                                            lower_open=[3]))
    assert o._device_constraint()[0] == "obe_mask_bounds" and o._bounds_call[0].tolist() == [0, 1, 3]
    assert o._bounds_call[3].tolist() == [0, 0, 1]
    for given, lo, is_open in (((-1.0, 5.0), 0.0, True), ((0.0, 5.0), 0.0, True), ((0.25, 5.0), 0.25, False),
                               ((None, 5.0), 0.0, True)):
        o.set_parameter_bounds({3: given})
        eff = o._effective_bounds(o._parameter_bounds)
        assert (eff[0][3], eff[1][3], bool(eff[2][3]), bool(eff[3][3])) == (lo, 5.0, is_open, False)
    o.set_parameter_bounds({3: (0.25, 5.0)}, inclusive=False)
    eff = o._effective_bounds(o._parameter_bounds)
    assert (eff[0][3], bool(eff[2][3]), bool(eff[3][3])) == (0.25, True, True)
    for empty in ({3: (None, 0.0)}, {3: (-2.0, -1.0)}):          # nothing is left of sigma > 0
        with pytest.raises(ValueError):
            o.set_parameter_bounds(empty)
    o.set_parameter_bounds(None)
    assert o._device_constraint()[0] == "obe_mask_nonpositive"
    two = noise_obj([2, 3])
    two.set_parameter_bounds({0: (0.0, None)})
    assert two._bounds_call[0].tolist() == [0, 2, 3] and two._bounds_call[3].tolist() == [0, 1, 1]


# ------------------------------------------------------------------------------------------------ snapshots
def test_bounds_survive_pickling_and_are_adopted_as_saved():
    """What a snapshot keeps of the bounds is the ``parameter_bounds`` tuple, and restore() hands it to
    _adopt_bounds(): pickled or deep-copied, it gives the same bounds and the same arrays for the library; None —
    what a snapshot written before there were bounds yields — clears.  (snapshot() and restore() themselves need a
    device: the round trip through live objects, and a state without the key, are in tests/test_gpu_constraints.py.)"""
    o = _bare()
    o.set_parameter_bounds({1: (0.0, None), 2: (0.995, 1.02)}, inclusive={2: (True, False)})
    saved = o.parameter_bounds
    import copy
    import pickle
    for carried in (pickle.loads(pickle.dumps(saved)), copy.deepcopy(saved)):
        new = _bare()
        new._adopt_bounds(carried)
        _same(new.parameter_bounds, saved)
        for a, b in zip(new._bounds_call[:4], o._bounds_call[:4]):
            np.testing.assert_array_equal(a, b)
    new = _bare()
    new.set_parameter_bounds({0: (0, 1)})
    new._adopt_bounds(None)
    assert new.parameter_bounds is None and new._device_constraint() is None


# ---------------------------------------------------------------------------- the entry points' own refusals
def test_entry_points_refuse_bad_arguments_without_a_device(lib):
    dev = 1 << 20                    # (never dereferenced: every call below is refused by its argument checks)
    c = lib.cdll
    n, d, big = 1000, 3, 1 << 30
    P = _lib.host_ptr
    rows, lo, hi, op = (np.array([0, 2], dtype=np.int32), np.array([0.0, -1.0]), np.array([INF, 1.0]),
                        np.array([1, 2], dtype=np.int32))
    R, LO, HI, OP = P(rows), P(lo), P(hi), P(op)
    f, m = np.eye(d), np.zeros(d)

    def refused(rc, word):
        assert rc == -1 and word in lib.last_error(), (rc, lib.last_error())

    def mask(particles=dev, ld=n, n_p=n, r=R, lower=LO, upper=HI, flags=OP, n_rows=2, w=dev, ws=dev, ws_bytes=big):
        return c.obe_mask_bounds(particles, ld, n_p, r, lower, upper, flags, n_rows, w, None, ws, ws_bytes, None)

    def mask_mom(particles=dev, ld=n, n_dims=d, n_p=n, r=R, lower=LO, upper=HI, flags=OP, n_rows=2, w=dev, mom=dev,
                 ws=dev, ws_bytes=big):
        return c.obe_mask_bounds_moments(particles, ld, n_dims, n_p, r, lower, upper, flags, n_rows, w, mom, None, None,
                                         ws, ws_bytes, None)

    def gather(aos=dev, n_dims=d, n_p=n, idx=dev, z=dev, new=dev + 8, w=dev, r=R, lower=LO, upper=HI, flags=OP, n_rows=2,
               partials=dev):
        return c.obe_resample_particles_aos_bounded(aos, n_dims, n_p, idx, z, P(f), P(m), 0.98, 0, new, n_p, w, r, lower,
                                                    upper, flags, n_rows, partials, None)

    for call, name in ((mask, "obe_mask_bounds"), (mask_mom, "obe_mask_bounds_moments")):
        refused(call(particles=None), name + ": bad pointer/size")
        refused(call(w=None), name + ": bad pointer/size")
        refused(call(n_p=0), name + ": bad pointer/size")
        refused(call(ld=n - 1), name + ": bad pointer/size")
        refused(call(ws=None), "workspace too small")
        refused(call(ws_bytes=64), "workspace too small")
    refused(mask_mom(mom=None), "bad pointer/size")
    refused(mask_mom(n_dims=0), "n_dims must be")
    refused(mask_mom(n_dims=_lib.OBE_CLOUD_MAX_DIMS + 1), "n_dims must be")
    refused(gather(aos=None), "bad pointer/size")
    refused(gather(new=dev), "bad pointer/size")                      # in place
    refused(gather(partials=None), "bad pointer/size")
    refused(gather(n_dims=_lib.OBE_FAST_DIMS + 1), "bad pointer/size")
    refused(gather(idx=None), "bad pointer/size")
    refused(gather(n_p=0), "bad pointer/size")
    many = np.zeros(_lib.OBE_MAX_DIMS + 1)
    for call in (mask, mask_mom, gather):
        for kw in (dict(r=None), dict(lower=None), dict(upper=None), dict(flags=None)):
            refused(call(**kw), "null pointer")
        refused(call(n_rows=0), "n_rows outside")
        refused(call(r=P(many.astype(np.int32)), lower=P(many), upper=P(many + 1), flags=P(many.astype(np.int32)),
                     n_rows=_lib.OBE_MAX_DIMS + 1), "n_rows outside")
        refused(call(r=P(np.array([0, -1], dtype=np.int32))), "row index out of range")
        refused(call(lower=P(np.array([0.0, np.nan]))), "NaN bound")
        refused(call(upper=P(np.array([np.nan, 1.0]))), "NaN bound")
        refused(call(lower=P(np.array([0.0, 2.0]))), "lower > upper")
    # a row must lie inside the cloud where the call knows its width
    refused(mask_mom(r=P(np.array([0, 3], dtype=np.int32))), "row index out of range")
    refused(gather(r=P(np.array([0, 3], dtype=np.int32))), "row index out of range")
    refused(mask(r=P(np.array([0, _lib.OBE_CLOUD_MAX_DIMS], dtype=np.int32))), "row index out of range")
    with pytest.raises(_lib.ObeHipError) as e:
        lib.call("obe_mask_bounds", dev, n, n, R, LO, HI, OP, 0, dev, None, dev, big, None)
    assert e.value.refused_before_launch


def test_the_delivery_audit_knows_the_new_entry_points():
    """OBE_CHECK_DELIVERY (optbayesexpt_amd/_audit.py): a call of the two entry points that deliver to the host marks
    exactly the words their noise-only twins mark — the count and the 2 + 4 D first moments armed by the _moments
    form, the count delivered by the synchronous one —, read by the parameter names of include/obe_hip.h."""
    import ctypes
    params = {fn: [name for _, name in ps] for fn, (_, ps) in _lib.PROTOTYPES.items()}
    zone = np.zeros(64)
    base = zone.ctypes.data

    def effect(fn, **values):
        assert set(values) <= set(params[fn])
        args = tuple(values.get(name) for name in params[fn])
        changed = []
        for start in (False, True):
            a = _audit._Audit()
            assert fn in a.rules
            a.zone_created(base, zone.nbytes, None)
            a.zones[base].armed[:] = start
            a.after_call(fn, args)
            changed.append(set(np.flatnonzero(a.zones[base].armed != start).tolist()))
        return changed

    def word(k):
        return ctypes.c_void_p(base + 8 * k)
    d = 3
    assert effect("obe_mask_bounds_moments", n_dims=d, h_first_moments=word(10), h_count=word(40)) == \
        [set(range(10, 10 + 2 + 4 * d)) | {40}, set()]
    assert effect("obe_mask_bounds_moments", n_dims=d, h_count=word(40)) == [{40}, set()]
    assert effect("obe_mask_bounds", h_count=word(7)) == [set(), {7}]
    for fn, (_, *names) in _audit._BOUNDS_RULES.items():
        assert set(names) <= set(params[fn]), fn
    # (the masked gather delivers nothing to the host)
    assert not [p for p in params["obe_resample_particles_aos_bounded"] if p.startswith("h_") and p not in
                ("h_factor", "h_mean", "h_rows", "h_lower", "h_upper", "h_open")]
    assert _lib.OBE_ABI_VERSION == 3
