"""Times the device-side parameter bounds at c5 size (524 288 particles x 10 parameters) on one GPU:

* the library calls by device events: obe_mask_bounds_moments and obe_resample_particles_aos_bounded with 1, 4 and 10
  bounded rows, next to the noise-only obe_mask_nonpositive_moments / obe_resample_particles_aos_masked (1 row);
* the whole enforce_parameter_constraints() after a resample by wall clock: bounds on the device against the same
  constraint as a NumPy hook over the host mirrors (the weights uploaded again included, as the next kernel needs them).

    python tools/time_constraints.py [n_particles] [repeats]
"""
import ctypes
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as obe                     # noqa: E402
from optbayesexpt_amd import _lib                  # noqa: E402

P = ctypes.c_void_p
D = 10


def _ptr(t):
    return P(t.data_ptr())


def _events(fn, repeats, reset):
    times = []
    for _ in range(repeats + 3):
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return np.median(times[3:]), np.min(times[3:])


def library_calls(n, repeats):
    lib = _lib.load()
    g = np.random.default_rng(0)
    x_host = g.normal(1.0, 1.0, (D, n))
    x = torch.from_numpy(x_host).cuda()
    aos = torch.from_numpy(np.ascontiguousarray(x_host.T)).cuda()
    w = torch.full((n,), 1.0 / n, dtype=torch.float64, device="cuda")
    new = torch.empty((D, n), dtype=torch.float64, device="cuda")
    idx = torch.from_numpy(g.integers(0, n, n)).cuda()
    z = torch.from_numpy(g.standard_normal(n * D)).cuda()
    factor, mean = np.ascontiguousarray(0.01 * np.eye(D)), np.ascontiguousarray(x_host.mean(axis=1))
    ws = torch.empty(lib.workspace_bytes(n, 1, 1, D) // 8 + 1, dtype=torch.float64, device="cuda")
    mom = torch.zeros(lib.moments_len(D), dtype=torch.float64, device="cuda")
    partials = torch.zeros(2 * 2048, dtype=torch.float64, device="cuda")
    h_mom, h_changed = _lib.pinned_array(2 + 4 * D), _lib.pinned_array(1, np.int64)
    st = P(torch.cuda.current_stream().cuda_stream)
    tail = (_ptr(w), _ptr(mom), _lib.host_ptr(h_mom), _lib.host_ptr(h_changed), _ptr(ws), ws.numel() * 8, st)
    gather = (_ptr(aos), D, n, _ptr(idx), _ptr(z), _lib.host_ptr(factor), _lib.host_ptr(mean), 0.98, 0, _ptr(new), n,
              _ptr(w))

    def reset():
        w.fill_(1.0 / n)
        torch.cuda.synchronize()

    print(f"library calls, {n} particles x {D} parameters, device events, median (min) of {repeats}, microseconds")
    rows1 = np.array([D - 1], dtype=np.int32)
    t = _events(lambda: lib.call("obe_mask_nonpositive_moments", _ptr(x), n, D, n, _lib.host_ptr(rows1), 1, *tail),
                repeats, reset)
    print(f"  obe_mask_nonpositive_moments         1 row : {t[0]:7.1f} ({t[1]:.1f})")
    for k in (1, 4, 10):
        rows = np.arange(D - k, D, dtype=np.int32)
        lo, hi, op = np.zeros(k), np.full(k, np.inf), np.ones(k, dtype=np.int32)
        b = (_lib.host_ptr(rows), _lib.host_ptr(lo), _lib.host_ptr(hi), _lib.host_ptr(op), k)
        t = _events(lambda: lib.call("obe_mask_bounds_moments", _ptr(x), n, D, n, *b, *tail), repeats, reset)
        hbm = 8.0 * (k + 2) * n + 8.0 * (D + 2) * n
        print(f"  obe_mask_bounds_moments             {k:2d} rows: {t[0]:7.1f} ({t[1]:.1f})   "
              f"{hbm / t[0] / 1e6:.2f} TB/s of the mask's 8(k + 2) + the moments' 8(D + 2) bytes per particle")
    t = _events(lambda: lib.call("obe_resample_particles_aos_masked", *gather, _lib.host_ptr(rows1), 1, _ptr(partials), st),
                repeats, reset)
    print(f"  obe_resample_particles_aos_masked    1 row : {t[0]:7.1f} ({t[1]:.1f})")
    t = _events(lambda: lib.call("obe_resample_particles_aos", *gather, st), repeats, reset)
    print(f"  obe_resample_particles_aos        unmasked : {t[0]:7.1f} ({t[1]:.1f})")
    for k in (1, 4, 10):
        rows = np.arange(D - k, D, dtype=np.int32)
        lo, hi, op = np.zeros(k), np.full(k, np.inf), np.ones(k, dtype=np.int32)
        b = (_lib.host_ptr(rows), _lib.host_ptr(lo), _lib.host_ptr(hi), _lib.host_ptr(op), k)
        t = _events(lambda: lib.call("obe_resample_particles_aos_bounded", *gather, *b, _ptr(partials), st), repeats, reset)
        print(f"  obe_resample_particles_aos_bounded  {k:2d} rows: {t[0]:7.1f} ({t[1]:.1f})")


class HostHook(obe.OptBayesExptNoiseParameter):
    """The same constraint as the reference's users write it: a NumPy loop over the cloud."""
    rows = ()

    def enforce_parameter_constraints(self):
        changes = False
        for r in self.rows:
            bad = np.flatnonzero(self.parameters[r] <= 0)
            if bad.size:
                changes = True
                self.particle_weights[bad] = 0
        if changes:
            self.particle_weights = self.particle_weights / np.sum(self.particle_weights)


def _spied(o):
    """The constraint's library calls of ``o`` from now on, by name."""
    used, lib = [], o._lib
    call = lib.call

    class Spy:
        def __getattr__(self, name):
            return getattr(lib, name)

        def call(self, name, *a):
            if name.startswith(("obe_mask_", "obe_resample_particles")):
                used.append(name)
            return call(name, *a)
    o._lib = Spy()
    return used


def whole_hook(n, repeats):
    """The hook as pdf_update() meets it: the cloud fresh from a resample on the device (no host copy of it), and
    ``parameters`` the alias of that cloud (obe_base.py:395)."""
    g = np.random.default_rng(1)
    prior = np.vstack([g.uniform(2, 4, (7, n)), g.uniform(0.5, 3, (1, n)), g.normal(0.5, 0.3, (1, n)),
                       g.uniform(0.05, 0.6, (1, n))])
    sv = (np.linspace(1.5, 4.5, 64),)
    sim = np.random.default_rng(3)
    for k in (1, 4, 10):
        rows = list(range(D - k, D))
        for name, cls in (("device bounds", obe.OptBayesExptNoiseParameter), ("NumPy host hook", HostHook)):
            o = cls(obe.models.lorentzian(7), sv, prior.copy(), (0.1,), noise_parameter_index=9, resample_threshold=0.999)
            o.rng = np.random.default_rng(2)
            if cls is HostHook:
                o.rows = rows
            else:
                o.set_parameter_bounds({r: (0.0, None) for r in rows}, inclusive=False)
            used = _spied(o)
            hook, counts = [], []
            for _ in range(repeats + 2):
                o.resample()
                o._parameters = o._particles              # (what pdf_update() does before it calls the hook)
                assert not o._particles._host_valid and not o._weights._host_valid
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                o.enforce_parameter_constraints()
                o._weights.tensor()                       # (the next kernel reads the weights on the device)
                if cls is not HostHook:
                    counts.append(o.last_constraint_count)               # (waits for the mask's count)
                torch.cuda.synchronize()
                hook.append((time.perf_counter() - t0) * 1e3)
                if cls is HostHook:
                    counts.append(int(np.sum(o.particle_weights == 0)))
            hook_calls = sorted(set(used) - {"obe_resample_particles", "obe_resample_particles_aos"})
            # ... and inside the cycle: pdf_update() calls that resample (the gather may apply the bounds itself)
            del used[:]
            cycle = []
            for _ in range(repeats + 2):
                x = o.opt_setting()
                y = 1.0 + 0.3 * sim.standard_normal()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                o.pdf_update((x, y))
                if cls is not HostHook:
                    o.last_constraint_count
                torch.cuda.synchronize()
                if o.just_resampled:
                    cycle.append((time.perf_counter() - t0) * 1e3)
            print(f"  {k:2d} rows  {name:16s}: hook alone {np.median(hook[2:]):8.3f} ({np.min(hook[2:]):.3f}) ms, zeroed "
                  f"{counts[-1]}, by {' + '.join(hook_calls) or 'no library call'}")
            print(f"  {'':25s}  pdf_update() with a resample {np.median(cycle[2:]):8.3f} ({np.min(cycle[2:]):.3f}) ms "
                  f"({len(cycle)} of {repeats + 2} resampled), by {' + '.join(sorted(set(used)))}")


if __name__ == "__main__":
    n_particles = int(sys.argv[1]) if len(sys.argv) > 1 else 524288
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        library_calls(n_particles, reps)
        print(f"enforce_parameter_constraints() after a resample, {n_particles} x {D}, wall clock, median (min), ms")
        whole_hook(n_particles, min(reps, 9))
