"""The cell form of the one-peak Lorentzian's unshifted sweep (include/obe_hip.h: OBE_SWEEP_CELLS) on the GPU:
forced with tuning_parameters['sweep_cells'] = 'always' (and 'sweep_shift' = 'never', so that the sweep is the
unshifted one the form stands in for) against the oracle at the suite's tolerance, plus the arg-max."""
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


def make(obe, x, cloud, w, d=D, cells="always", shift="never"):
    o = obe.OptBayesExpt(obe.models.lorentzian(1), (np.asarray(x, dtype=np.float64),), cloud.copy(), (d,),
                         utility_method="variance_full", auto_resample=False, default_noise_std=500.0)
    o.tuning_parameters["sweep_cells"] = cells
    o.tuning_parameters["sweep_shift"] = shift
    o.particle_weights = w
    return o


def check_against_oracle(o, x, cloud, w, d=D, what=""):
    ref = oracle.yvar_full_sweep(omodels.lorentzian, oracle.flatten_settings((np.asarray(x, dtype=np.float64),)), cloud,
                                 w, (d,))[0]
    got = o.yvar_from_parameter_draws()[0]
    assert o.last_sweep["cells"] and not o.last_sweep["shifted"], o.last_sweep
    # one particle: the reference's two-pass variance is rounding debris of (eps y)^2, the one-pass form's is
    # eps S2-sized — up to 64 eps max a^2 (b' = 0): nothing to compare relatively there
    floor = 64 * 2.3e-16 * float(np.max(cloud[1] ** 2)) if cloud.shape[1] == 1 else 0.0
    assert_rel(got, ref, RTOL, what, garbage_floor=floor)
    if cloud.shape[1] > 1:
        o.opt_setting()
        assert o.last_sweep["cells"]
        assert o.last_setting_index == int(np.argmax(ref)), what


@pytest.mark.parametrize("ns,n", [(1, 1), (63, 2), (257, 7), (4099, 513), (63, 4099), (4099, 4099), (1, 4099),
                                  (257, 1)])
def test_ragged_shapes(obe, ns, n):
    x = np.linspace(1.5, 4.5, ns) if ns > 1 else np.array([3.1])
    cloud, w = prior_cloud(n, 100 + n), weights(n, 200 + n)
    check_against_oracle(make(obe, x, cloud, w), x, cloud, w, what=f"{ns} settings x {n} particles")


SETTING_LAYOUTS = {
    # d = 1/8: x / d and every cell edge (half-width 1/4 in x / d) are exact, so these settings ARE the edges
    "on cell edges": (12.0 * 0.125 + 0.0625 * np.arange(0, 49), 0.125),
    "one setting alone in the last cell": (np.append(np.linspace(1.5, 2.0, 256), 4.49), D),
    "two clusters, empty cells between": (np.concatenate([np.linspace(1.5, 1.9, 130), np.linspace(4.0, 4.5, 127)]), D),
    "shuffled": (np.random.default_rng(5).permutation(np.linspace(1.5, 4.5, 257)), D),
}


@pytest.mark.parametrize("layout", sorted(SETTING_LAYOUTS))
def test_setting_layouts(obe, layout):
    x, d = SETTING_LAYOUTS[layout]
    cloud, w = prior_cloud(513, 7), weights(513, 8)
    check_against_oracle(make(obe, x, cloud, w, d=d), x, cloud, w, d=d, what=layout)


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
    rc, got, kappa, idx = c_sweep(o, _lib.OBE_SWEEP_CELLS, lo, n_local)
    assert rc == 0 and np.isfinite(kappa)
    ref = oracle.yvar_full_sweep(omodels.lorentzian, oracle.flatten_settings((x[lo:lo + n_local],)), cloud, w, (D,))[0]
    assert_rel(got, ref, RTOL, "slice [1031, 2531)")
    assert idx == int(np.argmax(ref))


def test_draws_mode_above_the_one_workgroup_size(obe):
    import torch
    from optbayesexpt_amd import _lib
    x = np.linspace(1.5, 4.5, 4099)
    cloud, w = prior_cloud(5000, 11), weights(5000, 12)
    o = make(obe, x, cloud, w)
    draws = np.random.default_rng(13).integers(0, 5000, 300)
    rc, got, kappa, idx = c_sweep(o, _lib.OBE_SWEEP_CELLS, 0, 4099, torch.from_numpy(draws).to(o._device))
    assert rc == 0 and np.isfinite(kappa)
    ref = oracle.yvar_full_sweep(omodels.lorentzian, oracle.flatten_settings((x,)), cloud[:, draws],
                                 np.full(300, 1.0 / 300), (D,))[0]
    assert_rel(got, ref, RTOL, "300 draws x 4099 settings")
    assert idx == int(np.argmax(ref))
    # the same call without the bit runs the direct kernel: the two forms agree to rounding, not to the bit
    rc, direct, _, _ = c_sweep(o, 0, 0, 4099, torch.from_numpy(draws).to(o._device))
    assert rc == 0 and not np.array_equal(direct, got)
    assert_rel(got, direct, RTOL, "cells vs direct, draws mode")


def test_high_kappa_clouds(obe):
    """The scale-0.06 and scale-0.04 clouds of test_unshifted_sweep_accuracy_below_the_kappa_threshold: cells
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
        shifted = make(obe, x, cloud, w, cells="never", shift="always").yvar_from_parameter_draws()[0]
        o = make(obe, x, cloud, w)
        cells = o.yvar_from_parameter_draws()[0]
        assert o.last_sweep["cells"] and not o.last_sweep["shifted"]
        kappa = o.last_sweep["kappa"]
        seen.append(kappa)
        print(f"scale {scale}: kappa {kappa:.4g}, worst |cells / shifted - 1| = {np.max(np.abs(cells / shifted - 1)):.3g}")
        if kappa < obe.OptBayesExpt.KAPPA_LEAVE:
            assert_rel(cells, shifted, 2e-11, f"cells vs shifted direct at kappa {kappa:.3g}")
    assert any(k < obe.OptBayesExpt.KAPPA_LEAVE for k in seen), seen


def test_far_particle(obe):
    x = np.linspace(1.5, 4.5, 257)
    cloud, w = prior_cloud(513, 14), weights(513, 15)
    cloud[0, 100] = 3.0 + 1e9 * D            # |x - x0| / d = 1e9
    o = make(obe, x, cloud, w)
    assert np.all(np.isfinite(o.yvar_from_parameter_draws()[0]))
    check_against_oracle(o, x, cloud, w, what="a particle 1e9 widths away")


def test_span_beyond_the_cap(obe):
    from optbayesexpt_amd import _lib
    span = _lib.OBE_CELL_MAX * 2.0 / _lib.OBE_CELL_RHO_INV * D        # the widest grid the cells cover
    x = np.linspace(0.0, 1.1 * span, 4099)
    cloud, w = prior_cloud(4099, 16), weights(4099, 17)
    cloud[0] += 1.0
    o = make(obe, x, cloud, w, cells="auto")
    rc, got, kappa, _ = c_sweep(o, _lib.OBE_SWEEP_CELLS, 0, 4099)
    assert rc == 0 and np.isnan(kappa) and np.all(np.isnan(got))
    ref = oracle.yvar_full_sweep(omodels.lorentzian, oracle.flatten_settings((x,)), cloud, w, (D,))[0]
    assert_rel(o.yvar_from_parameter_draws()[0], ref, RTOL, "'auto' on a grid beyond the cap")
    assert o.last_sweep["cells"] is False
    forced = make(obe, x, cloud, w, cells="always")         # 'always' skips the worthwhileness test only
    assert_rel(forced.yvar_from_parameter_draws()[0], ref, RTOL, "'always' on a grid beyond the cap")
    assert forced.last_sweep["cells"] is False


def _cycles(obe, cells, n_cycles=12):
    g = np.random.default_rng(31)
    n, ns = 40000, 4200
    x = np.linspace(1.5, 4.5, ns)
    prior = np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    o = obe.OptBayesExpt(obe.models.lorentzian(1), (x,), prior, (D,), scale=False, utility_method="variance_full",
                         default_noise_std=100.0)
    o.tuning_parameters["sweep_cells"] = cells
    o.tuning_parameters["speculative_sweep"] = True
    o.rng = np.random.default_rng(32)
    sim = np.random.default_rng(33)
    o._mlib.call("obe_sweep_timing", 1, None, None)
    chosen, forms, resamples, utilities = [], [], 0, []
    for _ in range(n_cycles):
        xs = o.opt_setting()
        chosen.append(o.last_setting_index)
        forms.append(bool(o.last_sweep["cells"]))
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
