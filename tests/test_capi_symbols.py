"""The C-ABI library (CPU-only checks, no kernel launches): it loads, exports exactly the
functions include/obe_hip.h declares with the argument counts the ctypes binding uses,
and its host-side argument validation reports errors without touching a GPU."""
import ctypes

import numpy as np
import pytest

from optbayesexpt_amd import _lib, models


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_library_exports_and_binds_every_declared_symbol(lib):
    declared = _lib.declared_symbols()
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib.cdll, name), f"{name} declared in obe_hip.h but not exported"
        restype, params = _lib.PROTOTYPES[name]
        fn = getattr(lib.cdll, name)            # (the binding HipLib applied, not just the one it computed)
        assert fn.restype is restype and len(fn.argtypes) == len(params), name
    assert lib.cdll.obe_abi_version() == _lib.OBE_ABI_VERSION == 3


def _dynamic_symbols(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_library_exports_nothing_but_the_declared_entry_points(lib):
    """`nm -D --defined-only` of libobe_hip.so == the names include/obe_hip.h declares (OBE_API), no more: the
    C++ helpers (obe::wait_host_words, obe::stream_control_words, ...), the kernels' host stubs and handle objects
    are internal (-fvisibility=hidden + the link-time export list, optbayesexpt_amd/build.py)."""
    import shutil
    if shutil.which("nm") is None:
        pytest.skip("no nm on this box")
    declared = _lib.declared_symbols()
    assert _dynamic_symbols(lib.path) == declared


def test_plugin_exports_nothing_but_the_declared_entry_points(lib):
    """... and the same for a per-model plugin library: it defines a SUBSET of the header's names (the
    model-dependent entry points + the three library queries) and nothing else, so that two plugins and the library
    in one process cannot interpose one another's internals."""
    import os
    import shutil
    from optbayesexpt_amd import build
    if shutil.which("nm") is None:
        pytest.skip("no nm on this box")
    model = None
    try:
        model = models.from_expression("b + a / (((x - x0) / d)**2 + 1)", settings=("x",),
                                       parameters=("x0", "a", "b"), constants=("d",))
    except RuntimeError:
        if os.path.exists(build.HIPCC):
            raise
        pytest.skip("plugin not prebuilt and no hipcc here")
    syms = _dynamic_symbols(model.plugin_path)
    assert set(_lib.MODEL_ENTRY_POINTS) | {"obe_abi_version", "obe_last_error", "obe_source_fingerprint"} <= set(syms)
    assert set(syms) <= set(_lib.declared_symbols()), sorted(set(syms) - set(_lib.declared_symbols()))


def _parameter_names():
    return {fn: [name for _, name in params] for fn, (_, params) in _lib.PROTOTYPES.items()}


def test_audit_rules_read_parameters_of_their_entry_points():
    """OBE_CHECK_DELIVERY's rules (optbayesexpt_amd/_audit.py) read a call's arguments by the parameter names of
    include/obe_hip.h: every name a rule reads is a parameter of its entry point, and every entry point that has a
    page-locked result parameter has a rule (or is listed as waiting for nothing new)."""
    from optbayesexpt_amd import _audit
    names = _parameter_names()
    for fn, (_, *reads) in _audit._RULES.items():
        assert set(reads) <= set(names[fn]), (fn, sorted(set(reads) - set(names[fn])))
    # every entry point with a host result parameter is covered by a rule
    host_results = ("h_out", "h_pinned_out", "h_pinned_word", "h_pinned_words", "h_best", "h_best_idx", "h_kappa", "h_f64",
                    "h_i64", "h_total", "h_total_pinned", "h_moments", "h_changed")
    unruled = {fn for fn, ps in names.items() if any(p in host_results for p in ps)} - set(_audit._RULES)
    # (these deliver by a synchronous copy or wait before they return, into memory the audit does not track as armed)
    assert unruled <= {"obe_moments", "obe_bayes_update_sweep", "obe_likelihood_y"}, sorted(unruled)


_ZONE = np.zeros(64)          # (zeros: no word holds the armed pattern, so every wait a rule records succeeds)


def _w(k):
    """Address of word k of _ZONE."""
    return ctypes.c_void_p(_ZONE.ctypes.data + 8 * k)


def _rule_effect(fn, **values):
    """(armed, delivered, marks): the words of a landing zone over _ZONE that the OBE_CHECK_DELIVERY rule of entry
    point `fn` arms and delivers after a call with these parameters (by header name; every other argument None), and
    the audit's (armed, waited) counts of that call."""
    from optbayesexpt_amd import _audit
    names = _parameter_names()[fn]
    assert set(values) <= set(names), sorted(set(values) - set(names))
    args = tuple(values.get(name) for name in names)
    base = _ZONE.ctypes.data
    changed = []
    for start in (False, True):          # all words delivered, then all armed: what the call changes
        a = _audit._Audit()
        a.zone_created(base, _ZONE.nbytes, None)
        a.zones[base].armed[:] = start
        a.after_call(fn, args)
        changed.append(set(np.flatnonzero(a.zones[base].armed != start).tolist()))
    return changed[0], changed[1], (a.counts["armed"], a.counts["waited"])


def test_audit_rules_arm_and_deliver_the_words_of_their_calls():
    """Each OBE_CHECK_DELIVERY rule (optbayesexpt_amd/_audit.py), driven on the CPU with a synthetic call: exactly
    the host words include/obe_hip.h says the call arms (left for the caller to wait for) or delivers (waited for
    before it returned), for each flag variant that changes which."""
    from optbayesexpt_amd import _audit
    d = 3                                # the K3 block of 3 rows: 2 + 4 d = 14 first-moment words, 23 in all
    m = _lib.ObeModelStruct(n_params=d)
    span = lambda k, n: set(range(k, k + n))     # noqa: E731
    cases = [
        ("obe_host_word_arm", dict(h_pinned_word=_w(5)), ({5}, set(), (1, 0))),
        ("obe_host_words_arm", dict(h_pinned_words=_w(5), n_words=4), (span(5, 4), set(), (1, 0))),
        ("obe_host_word_wait", dict(h_pinned_word=_w(5)), (set(), {5}, (0, 1))),
        ("obe_host_words_wait", dict(h_pinned_words=_w(5), n_words=4), (set(), span(5, 4), (0, 1))),
        # [sum t, sum w'^2, the 14 first moments, the resample decision]
        ("obe_bayes_update_model_moments_enqueue", dict(m=m, h_pinned_out=_w(10)), (span(10, 17), set(), (1, 0))),
        # the synchronous sweep waited for its results; the speculative and the unconditional enqueued form did not
        ("obe_sweep_utility", dict(shifted=_lib.OBE_SWEEP_SHIFTED, h_best=_w(1), h_best_idx=_w(2), h_kappa=_w(3)),
         (set(), {1, 2, 3}, (0, 3))),
        ("obe_sweep_utility", dict(shifted=_lib.OBE_SWEEP_SAFE, h_best=_w(1), h_best_idx=_w(2)),
         (set(), {1, 2}, (0, 2))),
        ("obe_sweep_utility", dict(shifted=_lib.OBE_SWEEP_SHIFTED | _lib.OBE_SWEEP_SPECULATIVE, h_best=_w(1),
                                   h_best_idx=_w(2), h_kappa=_w(3)), ({1, 2, 3}, set(), (3, 0))),
        ("obe_sweep_utility", dict(shifted=_lib.OBE_SWEEP_NOWAIT, h_best=_w(1), h_best_idx=_w(2), h_kappa=_w(3)),
         ({1, 2, 3}, set(), (3, 0))),
        # h_f64 = [sum w, the K3 block]: sum w is armed unless the CDF was fresh (the host stores 1.0), the first
        # moments unless the caller already has them; h_i64's two words always
        ("obe_resample_begin", dict(n_dims=d, cdf_is_fresh=0, have_first_moments=0, h_f64=_w(20), h_i64=_w(50)),
         ({20} | span(21, 23) | {50, 51}, set(), (3, 0))),
        ("obe_resample_begin", dict(n_dims=d, cdf_is_fresh=1, have_first_moments=0, h_f64=_w(20), h_i64=_w(50)),
         (span(21, 23) | {50, 51}, {20}, (2, 1))),
        ("obe_resample_begin", dict(n_dims=d, cdf_is_fresh=0, have_first_moments=1, h_f64=_w(20), h_i64=_w(50)),
         ({20} | span(35, 9) | {50, 51}, set(), (3, 0))),
        ("obe_resample_begin", dict(n_dims=d, cdf_is_fresh=1, have_first_moments=1, h_f64=_w(20), h_i64=_w(50)),
         (span(35, 9) | {50, 51}, {20}, (2, 1))),
        # sum(p) only when the call rebuilds the CDF; the indices when d_idx is the device view of a landing zone
        ("obe_draw_indices", dict(cdf_is_fresh=0, n_draws=4, d_idx=_w(30), h_total_pinned=_w(2)),
         ({2} | span(30, 4), set(), (2, 0))),
        ("obe_draw_indices", dict(cdf_is_fresh=1, n_draws=4, d_idx=_w(30), h_total_pinned=_w(2)),
         (span(30, 4), set(), (1, 0))),
        ("obe_draw_indices", dict(cdf_is_fresh=0, n_draws=4, d_idx=_w(30)), (span(30, 4), set(), (1, 0))),
        ("obe_draw_indices", dict(cdf_is_fresh=0, n_draws=1, d_idx=None, h_total_pinned=_w(2)), ({2}, set(), (1, 0))),
        ("obe_mask_nonpositive_moments", dict(n_dims=d, h_moments=_w(10), h_changed=_w(40)),
         (span(10, 14) | {40}, set(), (2, 0))),
        ("obe_mask_renorm_moments", dict(n_dims=d, h_moments=_w(10), h_changed=_w(40)),
         (span(10, 14) | {40}, set(), (2, 0))),
        ("obe_bayes_update_model", dict(h_out=_w(4)), (set(), {4, 5}, (0, 1))),
        # [sum t, sum w'^2, the 14 first moments]
        ("obe_bayes_update_model_moments", dict(m=m, h_out=_w(4)), (set(), span(4, 16), (0, 1))),
        ("obe_bayes_update_lik", dict(h_out=_w(4)), (set(), {4, 5}, (0, 1))),
        ("obe_bayes_update_y", dict(h_out=_w(4)), (set(), {4, 5}, (0, 1))),
        ("obe_mask_nonpositive", dict(h_changed=_w(7)), (set(), {7}, (0, 1))),
        ("obe_weight_sums", dict(h_out=_w(4)), (set(), {4, 5}, (0, 1))),
        ("obe_weight_cdf", dict(h_total=_w(7)), (set(), {7}, (0, 1))),
        ("obe_utility_argmax", dict(h_best=_w(1), h_best_idx=_w(2)), (set(), {1, 2}, (0, 2))),
        ("obe_argmax", dict(h_best=_w(1), h_best_idx=_w(2)), (set(), {1, 2}, (0, 2))),
    ]
    assert {fn for fn, _, _ in cases} == set(_audit._RULES)
    for fn, values, expect in cases:
        assert _rule_effect(fn, **values) == expect, (fn, values)
    # a wait that returns while a word still holds the armed pattern is a violation
    armed = np.array([0, _lib.HOST_SENTINEL], dtype=np.uint64)
    with pytest.raises(_audit.DeliveryError):
        _audit._Audit().after_call("obe_host_words_wait", (ctypes.c_void_p(armed.ctypes.data), 2, None))


def test_prototypes_cover_every_declaration():
    """The strict parse of the OBE_API prototypes that the binding comes from skips no declaration that the loose
    scan of the header finds."""
    assert set(_lib.PROTOTYPES) == set(_lib.declared_symbols())


def test_prototypes_refuse_a_c_type_outside_the_binding_rule(tmp_path):
    header = tmp_path / "obe_hip.h"
    header.write_text("OBE_API int obe_ok(const obe_model* m, void** out, char* name, int64_t n);\n")
    assert [t for t, _ in _lib._prototypes(str(header))["obe_ok"][1]] == [
        ctypes.POINTER(_lib.ObeModelStruct), ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]
    for c_type in ("float", "uint64_t", "unsigned int", "void"):
        header.write_text(f"OBE_API int obe_bad(const double* d_x, {c_type} v);\n")
        with pytest.raises(TypeError):
            _lib._prototypes(str(header))
    header.write_text("OBE_API float obe_bad(void);\n")
    with pytest.raises(TypeError):
        _lib._prototypes(str(header))


def test_model_struct_layout_and_validation(lib):
    assert ctypes.sizeof(_lib.ObeModelStruct) == 6 * 4 + 8 * 8
    m = models.lorentzian(1).struct(3, (0.1,))
    assert lib.cdll.obe_model_validate(m) == 0
    assert (m.n_setdims, m.n_channels) == (1, 1)
    m7 = models.lorentzian(7).struct(10, (0.1,))
    assert lib.cdll.obe_model_validate(m7) == 0
    bad = models.lorentzian(1).struct(3, (0.1,))
    bad.n_params = 2                                   # fewer rows than the model reads
    assert lib.cdll.obe_model_validate(bad) == -1
    assert "n_params" in lib.last_error()
    bad = models.lorentzian(1).struct(3, (0.1,))
    bad.aux = 9
    assert lib.cdll.obe_model_validate(bad) == -1
    bad = models.coil().struct(4, ())
    bad.n_channels = 1
    assert lib.cdll.obe_model_validate(bad) == -1
    bad.id = 99
    assert lib.cdll.obe_model_validate(bad) == -1 and "unknown model" in lib.last_error()
    with pytest.raises(ValueError):
        models.lorentzian(1).struct(3, ())             # missing constant d
    with pytest.raises(ValueError):
        models.rabi().struct(1, (1.0, 0.1, 2.0))       # too few parameter rows


def test_workspace_and_moment_sizes(lib):
    assert lib.moments_len(3) == 2 + 12 + 9
    for d in list(range(1, 17)) + [40]:
        assert _lib.MomentLayout(d).total_len == lib.moments_len(d), d
    small = lib.workspace_bytes(1000, 10, 1, 3)
    big = lib.workspace_bytes(1 << 20, 65536, 1, 3)
    assert 0 < small < big < 1 << 30
    assert lib.workspace_bytes(1 << 20, 65536, 2, 3) > big


def test_workspace_covers_every_smaller_draw_count(lib):
    """A sweep of N_DRAWS <= n draws runs in the workspace sized for n (the public N_DRAWS attribute
    can be set to anything): the size must not shrink when the draw count grows, although the
    number of particle chunks of the plan is not monotone (the chunk length is rounded up to whole
    waves after the count is chosen)."""
    g = np.random.default_rng(12)
    for _ in range(4000):
        n = int(g.integers(300, 3_000_000))
        ns = int(g.integers(1, 70_000))
        nd = int(g.integers(max(1, n // 3), n + 1))
        assert lib.workspace_bytes(nd, ns, 1, 3) <= lib.workspace_bytes(n, ns, 1, 3), (n, ns, nd)


def test_argument_errors_are_reported_not_crashed(lib):
    """NULL pointers / bad sizes come back as status -1 with a message (no launch)."""
    out = np.zeros(4)
    rc = lib.cdll.obe_weight_sums(None, 10, None, 0, _lib.host_ptr(out), None)
    assert rc == -1 and lib.last_error()
    rc = lib.cdll.obe_moments(None, 0, 3, 0, None, 0, None, None, None, 0, None)
    assert rc == -1
    rc = lib.cdll.obe_cdf_search(None, 0, None, 0, None, None, 0, None)
    assert rc == -1
    with pytest.raises(_lib.ObeHipError):
        lib.call("obe_argmax", None, 0, None, None, None, 0, None)
    dev = 1 << 20                    # (never dereferenced: a NULL generator state is the first check's refusal)
    rc = lib.cdll.obe_resample_begin(dev, 16, 3, 16, dev, None, 0, 0, 0, 1 << 16, dev, dev, dev, dev, dev, dev, 1 << 20,
                                     dev, dev, dev, None, dev, 1 << 20, None)
    assert rc == -1 and lib.last_error() == "obe_resample_begin: bad pointer/size"
    # a negative row index would make the mask kernel read in front of the cloud: refused before any launch
    rows = np.array([-1], dtype=np.int32)
    ws_bytes = lib.cdll.obe_workspace_bytes(16, 1, 1, 3)
    rc = lib.cdll.obe_mask_nonpositive(dev, 16, 16, _lib.host_ptr(rows), 1, dev, None, dev, ws_bytes, None)
    assert rc == -1 and lib.last_error() == "obe_mask_nonpositive: row index out of range"


def test_sharded_objects_decide_the_range_check_from_all_slices(lib):
    """How many sweeps (and all-gathers) an opt_setting() of a sharded object takes hangs on whether kappa can
    report "the fast form left its range", which hangs on the settings a lane owns, which hangs on the LENGTH of a
    slice: 1023 settings over two ranks are 512 + 511 settings, 2 and 1 per lane (obe_sweep_settings_per_lane_for,
    a host function).  Every rank must answer with the same figure — the largest over all slices."""
    import types
    from optbayesexpt_amd.dist import shard_bounds
    from optbayesexpt_amd.obe_base import OptBayesExpt
    per_lane = lib.cdll.obe_sweep_settings_per_lane_for
    assert (per_lane(512, 0), per_lane(511, 0)) == (2, 1)
    dm = models.lorentzian(1)
    assert dm.safe_sweep and dm.safe_sweep_min_spt == 2
    for n_settings, world in ((1023, 2), (4100, 4), (2047, 2), (65536, 8), (16384, 8), (7, 3)):
        answers = []
        for rank in range(world):
            b, e = shard_bounds(n_settings, rank, world)
            fake = types.SimpleNamespace(_s_begin=b, _s_end=e, _n_settings=n_settings, _mlib=lib, _device_model=dm,
                                         _shard=types.SimpleNamespace(rank=rank, world_size=world))
            fake._settings_per_lane = types.MethodType(OptBayesExpt._settings_per_lane, fake)
            answers.append((OptBayesExpt._settings_per_lane(fake), OptBayesExpt._sweep_needs_range_check(fake)))
        assert len(set(answers)) == 1, (n_settings, world, answers)
        lengths = [shard_bounds(n_settings, r, world) for r in range(world)]
        assert answers[0][0] == max(per_lane(e - b, 0) for b, e in lengths)
    # an unsharded object answers for its own grid
    fake = types.SimpleNamespace(_s_begin=0, _s_end=511, _n_settings=511, _mlib=lib, _device_model=dm, _shard=None)
    fake._settings_per_lane = types.MethodType(OptBayesExpt._settings_per_lane, fake)
    assert OptBayesExpt._settings_per_lane(fake) == 1 and not OptBayesExpt._sweep_needs_range_check(fake)
