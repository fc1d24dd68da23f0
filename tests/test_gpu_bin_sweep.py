"""The bin form of the one-peak Lorentzian's unshifted sweep (include/obe_hip.h: OBE_SWEEP_BINS) on the GPU: forced
with tuning_parameters['sweep_bins'] = 'always' (and 'sweep_shift' = 'never', so that the sweep is the unshifted one
the form stands in for) against the oracle at the suite's tolerance, plus the arg-max; the grouping of the draws at
every shape where a rank can go wrong; the poisoned plan and what the object does about it."""
import ctypes

import numpy as np
import pytest

from _replay import assert_rel
import oracle
from oracle import models as omodels

pytestmark = pytest.mark.gpu

RTOL = 1e-10
D = 0.1


@pytest.fixture(scope="module")
def obe(hip):
    import optbayesexpt_amd
    return optbayesexpt_amd


def prior_cloud(n, seed):
    """c3's prior.  The spread of b (1000) keeps (mean of y')^2 / var of the unshifted moments below ~10 for any
    n >= 2, so the one-pass variance is good to a few eps and the suite's 1e-10 applies as it stands."""
    g = np.random.default_rng(seed)
    return np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])


def weights(n, seed):
    w = np.random.default_rng(seed).exponential(1.0, n)
    return w / w.sum()


def make(obe, x, cloud, w, d=D, bins="always", shift="never", cells="auto"):
    o = obe.OptBayesExpt(obe.models.lorentzian(1), (np.asarray(x, dtype=np.float64),), cloud.copy(), (d,),
                         utility_method="variance_full", auto_resample=False, default_noise_std=500.0)
    o.tuning_parameters["sweep_bins"] = bins
    o.tuning_parameters["sweep_cells"] = cells
    o.tuning_parameters["sweep_shift"] = shift
    o.particle_weights = w
    return o


def oracle_yvar(x, cloud, w, d=D):
    return oracle.yvar_full_sweep(omodels.lorentzian, oracle.flatten_settings((np.asarray(x, dtype=np.float64),)), cloud,
                                  w, (d,))[0]


def check_against_oracle(o, x, cloud, w, d=D, what="", bins=True):
    ref = oracle_yvar(x, cloud, w, d)
    got = o.yvar_from_parameter_draws()[0]
    assert o.last_sweep["bins"] is bins and not o.last_sweep["shifted"], o.last_sweep
    # one particle: the reference's two-pass variance is rounding debris of (eps y)^2, the one-pass form's is
    # eps S2-sized — up to 64 eps max a^2 (b' = 0): nothing to compare relatively there
    # (tests/test_gpu_cell_sweep.py)
    floor = 64 * 2.3e-16 * float(np.max(cloud[1] ** 2)) if cloud.shape[1] == 1 else 0.0
    assert_rel(got, ref, RTOL, what, garbage_floor=floor)
    if cloud.shape[1] > 1:
        o.opt_setting()
        assert o.last_sweep["bins"] is bins
        assert o.last_setting_index == int(np.argmax(ref)), what
    return got


@pytest.mark.parametrize("ns,n", [(1, 1), (63, 2), (257, 7), (4099, 513), (63, 4099), (1, 4099), (257, 1),
                                  (4099, 4099)])
def test_ragged_shapes(obe, ns, n):
    x = np.linspace(1.5, 4.5, ns) if ns > 1 else np.array([3.1])
    cloud, w = prior_cloud(n, 100 + n), weights(n, 200 + n)
    check_against_oracle(make(obe, x, cloud, w), x, cloud, w, what=f"{ns} settings x {n} particles")


def _layouts():
    from optbayesexpt_amd import _lib
    g = np.random.default_rng(77)
    width = 2.0 / _lib.OBE_CELL_RHO_INV                 # of a bin, in x / d

    def cloud(x0):
        n = x0.size
        return np.array([x0, g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    cap = _lib.OBE_BIN_MAX
    # (x0 / d from 20 on in steps of a bin: the first and the last value decide the count, the rest fill it)
    exactly = 0.125 * (20.0 + width * np.append(g.uniform(0.0, cap - 1, 1022), [0.0, cap - 1.0]))
    one_more = 0.125 * (20.0 + width * np.append(g.uniform(0.0, cap, 1022), [0.0, float(cap)]))
    extremes = cloud(np.concatenate([[0.5], g.uniform(2, 4, 1023), [5.5]]))
    w_ext = weights(1025, 78)
    w_ext[[0, -1]] = 0.0
    w_ext /= w_ext.sum()
    return {
        "every particle in one bin": (cloud(3.0 + 0.02 * g.uniform(-1, 1, 2049)), None, D, True),
        # (the first particle is the origin; the others sit in the middle of the bins that follow)
        "every particle in a bin of its own": (cloud(3.0 + D * width * (np.arange(100) + 0.5 * (np.arange(100) > 0))),
                                               None, D, True),
        "two clusters, empty bins between": (cloud(np.concatenate([g.uniform(1.6, 1.7, 300), g.uniform(4.1, 4.3, 213)])),
                                             None, D, True),
        # d = 1/8: x0 / d and every bin edge are exact, so these x0 ARE the edges
        "x0 on bin edges": (cloud(0.125 * (16.0 + width * g.integers(0, 17, 4099))), None, 0.125, True),
        "exactly OBE_BIN_MAX bins": (cloud(exactly), None, 0.125, True),
        "one bin more than OBE_BIN_MAX": (cloud(one_more), None, 0.125, False),
        "zero-weight particles at the extremes": (extremes, w_ext, D, True),
    }


LAYOUTS = None


@pytest.mark.parametrize("layout", ["every particle in one bin", "every particle in a bin of its own",
                                    "two clusters, empty bins between", "x0 on bin edges", "exactly OBE_BIN_MAX bins",
                                    "one bin more than OBE_BIN_MAX", "zero-weight particles at the extremes"])
def test_particle_layouts(obe, layout):
    global LAYOUTS
    if LAYOUTS is None:
        LAYOUTS = _layouts()
    cloud, w, d, fits = LAYOUTS[layout]
    if w is None:
        w = weights(cloud.shape[1], 79)
    x = np.linspace(1.5, 4.5, 257) if d == D else np.linspace(2.0, 10.5, 257)
    first = check_against_oracle(make(obe, x, cloud, w, d=d), x, cloud, w, d=d, what=layout, bins=fits)
    again = make(obe, x, cloud, w, d=d).yvar_from_parameter_draws()[0]
    assert np.array_equal(first, again), layout                    # the same call twice: the same bits


@pytest.mark.parametrize("ns,n", [(257, 4099), (63, 150001)])
def test_grouping_across_block_boundaries(obe, ns, n):
    """Particles whose bins cycle with period 37 — coprime to the wavefront (64), the workgroup (256) and the unit of
    draws a wavefront groups: every unit starts in another phase, every bin has draws in every unit, and a wrong rank
    puts a record into another bin's run (or drops one), which the variance shows.  4099 particles: one trip of 64
    draws per wavefront; 150 001: two trips, the running figures carried from one to the next, and bins of four
    items."""
    g = np.random.default_rng(81)
    x0 = 2.0 + D * 0.5 * ((np.arange(n) % 37) + g.uniform(0.05, 0.95, n))
    cloud = np.array([x0, g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    w = weights(n, 82)
    x = np.linspace(1.5, 4.5, ns)
    first = check_against_oracle(make(obe, x, cloud, w), x, cloud, w, what="bins cycling with period 37")
    assert np.array_equal(first, make(obe, x, cloud, w).yvar_from_parameter_draws()[0])


def test_far_particle(obe):
    x = np.linspace(1.5, 4.5, 257)
    cloud, w = prior_cloud(513, 14), weights(513, 15)
    cloud[0, 100] = 3.0 + 1e9 * D            # |x - x0| / d = 1e9
    o = make(obe, x, cloud, w)
    got = o.yvar_from_parameter_draws()[0]
    assert np.all(np.isfinite(got)) and o.last_sweep["bins"] is False
    assert_rel(got, oracle_yvar(x, cloud, w), RTOL, "a particle 1e9 widths away")
    # the same cloud again: nothing asks for bins; a new cloud: asked again
    assert not o._bin_form_wanted() and not o._sweep_inputs(False)["bins"]
    o.yvar_from_parameter_draws()
    assert o.last_sweep["bins"] is False
    o.resample()
    assert o._bin_form_wanted() and o._sweep_inputs(False)["bins"]


def test_far_particle_launch_sequence(obe):
    """The flags word of every obe_sweep_utility_keep() call over four requests on the cloud of test_far_particle:
    what a request launches is decided from kappa alone (SweepState.after), so the sequence is the decision."""
    from optbayesexpt_amd import _lib
    x = np.linspace(1.5, 4.5, 257)
    cloud, w = prior_cloud(513, 14), weights(513, 15)
    cloud[0, 100] = 3.0 + 1e9 * D
    w[100] = 0.0              # (the bins' span counts zero-weight particles too; a resample never draws this one)
    w /= w.sum()
    o = make(obe, x, cloud, w)
    o.rng = np.random.default_rng(16)
    lib, flags = o._mlib, []
    call = lib.call

    def recording(name, *args):
        if name == "obe_sweep_utility_keep":
            flags.append(args[11])                      # (include/obe_hip.h: the `shifted` word)
        return call(name, *args)

    lib.call = recording                                # (on the instance: the class's method comes back below)
    try:
        o.yvar_from_parameter_draws()                   # the cloud does not fit the bins: repeated pair by pair
        first, flags[:] = list(flags), []
        o.yvar_from_parameter_draws()                   # nothing asks for bins again
        second, flags[:] = list(flags), []
        o.resample()                                    # a new cloud (the far particle's weight is next to nothing)
        o.yvar_from_parameter_draws()
        third, flags[:] = list(flags), []
        assert o.last_sweep["bins"] and o.last_sweep["kept"] is False, o.last_sweep
        o.yvar_from_parameter_draws()
        fourth = list(flags)
        assert o.last_sweep["bins"] and o.last_sweep["kept"] is True, o.last_sweep
    finally:
        del lib.call
    print("flags words:", first, second, third, fourth)
    assert first == [_lib.OBE_SWEEP_BINS, 0]
    assert second == [0]
    assert third == [_lib.OBE_SWEEP_BINS]
    assert fourth == [_lib.OBE_SWEEP_BINS | _lib.OBE_SWEEP_BINS_KEPT]


def c_sweep(o, flags, s_begin, n_local, draw_idx=None):
    """obe_sweep_utility on a slice of the object's settings with its own cloud: (status, yvar, kappa, best index)."""
    import torch
    from optbayesexpt_amd import _lib
    from optbayesexpt_amd.particlepdf import _ptr, _P
    p, w = o._pw_tensors()
    mom = o._moments_on_device()
    noise = torch.full((1,), 250000.0, dtype=torch.float64, device=w.device)
    yvar = torch.zeros((1, n_local), dtype=torch.float64, device=w.device)
    util = torch.zeros(n_local, dtype=torch.float64, device=w.device)
    out = _lib.pinned_array(4)
    best, idx, kappa = out[0:1], out.view(np.int64)[1:2], out[2:3]
    hp = _lib.host_ptr
    rc = o._mlib.cdll.obe_sweep_utility(o._model_struct, _P(o._settings_dev.data_ptr() + 8 * s_begin), o._n_settings,
                                        n_local, _ptr(p), p.shape[1], o.n_particles, _ptr(w),
                                        None if draw_idx is None else _ptr(draw_idx),
                                        0 if draw_idx is None else draw_idx.numel(), _ptr(mom), flags, _ptr(noise), 0,
                                        None, 1.0, _ptr(yvar), _ptr(util), hp(best), hp(idx), hp(kappa), _ptr(o._ws),
                                        o._ws_bytes, o._stream())
    torch.cuda.synchronize()
    return rc, yvar.cpu().numpy()[0], float(kappa[0]), int(idx[0])


def test_slice_at_a_settings_offset(obe):
    from optbayesexpt_amd import _lib
    x = np.linspace(1.5, 4.5, 4099)
    cloud, w = prior_cloud(513, 9), weights(513, 10)
    o = make(obe, x, cloud, w)
    lo, n_local = 1031, 1500
    rc, got, kappa, idx = c_sweep(o, _lib.OBE_SWEEP_BINS, lo, n_local)
    assert rc == 0 and np.isfinite(kappa)
    ref = oracle_yvar(x[lo:lo + n_local], cloud, w)
    assert_rel(got, ref, RTOL, "slice [1031, 2531)")
    assert idx == int(np.argmax(ref))


def test_draws_mode_above_the_one_workgroup_size(obe):
    import torch
    from optbayesexpt_amd import _lib
    x = np.linspace(1.5, 4.5, 4099)
    cloud, w = prior_cloud(5000, 11), weights(5000, 12)
    o = make(obe, x, cloud, w)
    draws = np.random.default_rng(13).integers(0, 5000, 300)
    rc, got, kappa, idx = c_sweep(o, _lib.OBE_SWEEP_BINS, 0, 4099, torch.from_numpy(draws).to(o._device))
    assert rc == 0 and np.isfinite(kappa)
    ref = oracle_yvar(x, cloud[:, draws], np.full(300, 1.0 / 300))
    assert_rel(got, ref, RTOL, "300 draws x 4099 settings")
    assert idx == int(np.argmax(ref))
    # the same call without the bit runs the direct kernel: the two forms agree to rounding, not to the bit
    rc, direct, _, _ = c_sweep(o, 0, 0, 4099, torch.from_numpy(draws).to(o._device))
    assert rc == 0 and not np.array_equal(direct, got)
    assert_rel(got, direct, RTOL, "bins vs direct, draws mode")


def test_poisoned_call(obe):
    from optbayesexpt_amd import _lib
    x = np.linspace(1.5, 4.5, 4099)
    cloud, w = prior_cloud(4099, 16), weights(4099, 17)
    cloud[0, 7] = 3.0 + 1.01 * _lib.OBE_BIN_MAX * 2.0 / _lib.OBE_CELL_RHO_INV * D        # a span beyond the cap
    o = make(obe, x, cloud, w)
    rc, got, kappa, _ = c_sweep(o, _lib.OBE_SWEEP_BINS, 0, 4099)
    assert rc == 0 and np.isnan(kappa) and np.all(np.isnan(got))


def test_high_kappa_clouds(obe):
    """The scale-0.06 and scale-0.04 clouds of test_unshifted_sweep_accuracy_below_the_kappa_threshold: bins
    against the shifted direct kernel, 2e-11 while kappa < KAPPA_LEAVE."""
    g = np.random.default_rng(123)
    n, ns = 20000, 600
    x = np.linspace(1.5, 4.5, ns)
    w = g.exponential(1.0, n)
    w /= w.sum()
    z = g.normal(size=(3, n))
    seen = []
    for scale in (0.06, 0.04):
        cloud = np.array([3.0 + 0.02 * scale * z[0], -1000.0 + 300.0 * scale * z[1], 50000.0 + 200.0 * scale * z[2]])
        shifted = make(obe, x, cloud, w, bins="never", cells="never", shift="always").yvar_from_parameter_draws()[0]
        o = make(obe, x, cloud, w)
        bins = o.yvar_from_parameter_draws()[0]
        assert o.last_sweep["bins"] and not o.last_sweep["shifted"]
        kappa = o.last_sweep["kappa"]
        seen.append(kappa)
        print(f"scale {scale}: kappa {kappa:.4g}, worst |bins / shifted - 1| = {np.max(np.abs(bins / shifted - 1)):.3g}")
        if kappa < obe.OptBayesExpt.KAPPA_LEAVE:
            assert_rel(bins, shifted, 2e-11, f"bins vs shifted direct at kappa {kappa:.3g}")
    assert any(k < obe.OptBayesExpt.KAPPA_LEAVE for k in seen), seen


def _cycles(obe, bins, n_cycles=12):
    g = np.random.default_rng(31)
    n, ns = 40000, 4200
    x = np.linspace(1.5, 4.5, ns)
    prior = np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    o = obe.OptBayesExpt(obe.models.lorentzian(1), (x,), prior, (D,), scale=False, utility_method="variance_full",
                         default_noise_std=100.0)
    o.tuning_parameters["sweep_bins"] = bins
    o.tuning_parameters["speculative_sweep"] = True
    o.rng = np.random.default_rng(32)
    sim = np.random.default_rng(33)
    o._mlib.call("obe_sweep_timing", 1, None, None)
    chosen, forms, resamples, utilities = [], [], 0, []
    for _ in range(n_cycles):
        xs = o.opt_setting()
        chosen.append(o.last_setting_index)
        forms.append(bool(o.last_sweep["bins"]))
        utilities.append(o._utility_dev.cpu().numpy().copy())
        y = float(omodels.lorentzian(xs, (3.0, -1000.0, 50000.0), (D,))) + 100.0 * sim.standard_normal()
        o.pdf_update((xs, y, 100.0))
        resamples += bool(o.just_resampled)
    o._drop_speculative_sweep()
    ms, launches = ctypes.c_double(0.0), ctypes.c_int64(0)
    o._mlib.call("obe_sweep_timing", 0, ctypes.byref(ms), ctypes.byref(launches))
    return chosen, forms, resamples, utilities, launches.value


def test_cycles_choose_the_same_settings_and_repeat_bit_for_bit(obe):
    never = _cycles(obe, "never")
    always = _cycles(obe, "always")
    again = _cycles(obe, "always")
    assert never[2] >= 1 and always[2] == never[2], (never[2], always[2])        # at least one resample
    assert not any(never[1]) and any(always[1]), always[1]
    assert always[0] == never[0]                      # the sequence of chosen indices
    assert again[0] == always[0]
    for a, b in zip(always[3], again[3]):
        assert np.array_equal(a, b)                   # two 'always' runs: the same bits
    assert always[4] == never[4] and always[4] >= 12, (always[4], never[4])      # obe_sweep_timing counts the same launches
