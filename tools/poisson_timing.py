"""The information pass of counted events (csrc/obe_poisson.hip) at every cap next to the binomial pass, on the one-peak
Lorentzian at 65 536 settings x 1 048 576 particles (the benchmark's largest shape).

    python tools/poisson_timing.py [--out profiles/poisson.txt] [--small]

  obe_poisson_information    d_information + d_tail + d_noise_var, what utility_information() asks for, cap 16 / 32 / 64,
                             and d_noise_var alone (the instantiation without outcome sums)
  obe_binomial_information   the yardstick: d_information + d_noise_var of a probability curve on the same grid and cloud size

Every figure is ONE library call between obe_timer_start and obe_timer_stop on the launch stream, after one warming call
of the same route; each route is read twice and both readings are printed.  "evals/s" is settings x particles over the
device time.  Rates 2 .. 12 at exposure 1: the tail mass beyond the cap is printed with every route."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import optbayesexpt_amd as obe  # noqa: E402
from optbayesexpt_amd.particlepdf import _ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poisson.txt"))
    ap.add_argument("--small", action="store_true", help="4 096 x 262 144 instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/poisson_timing.py measures on the GPU: none is visible")
    n_s, n_p = (4096, 262144) if args.small else (65536, 1048576)
    g = np.random.default_rng(5)
    dev = torch.device("cuda:0")
    grid = (np.linspace(2.0, 4.0, n_s),)
    x0 = g.uniform(2.6, 3.4, n_p)
    counts = obe.OptBayesExptPoisson(obe.models.lorentzian(1), grid, np.array([x0, g.uniform(3, 8, n_p), g.uniform(2, 4, n_p)]),
                                     (0.1,), scale=False)
    clicks = obe.OptBayesExptBinomial(obe.models.lorentzian(1), grid,
                                      np.array([x0, g.uniform(0.3, 0.6, n_p), g.uniform(0.1, 0.3, n_p)]), (0.1,), scale=False)
    w0 = g.random(n_p)
    counts.particle_weights = clicks.particle_weights = w0 / w0.sum()
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    info, tail, nu = new(n_s), new(n_s), new(1, n_s)
    timer, ms = ctypes.c_void_p(), ctypes.c_float()
    counts._lib.call("obe_timer_create", ctypes.byref(timer))

    def poisson(cap, outcomes=True):
        o = counts
        lib, st = o._mlib, o._stream()
        p, w = o._pw_tensors()
        nbytes = int(lib.cdll.obe_poisson_workspace_bytes(n_p, n_s, 1, cap))
        ws = new(nbytes // 8 + 1)
        return lambda: lib.call("obe_poisson_information", o._model_struct, _ptr(o._settings_dev), n_s, n_s, _ptr(p), n_p,
                                n_p, _ptr(w), 1.0, cap, None, 1.0, _ptr(info) if outcomes else None,
                                _ptr(tail) if outcomes else None, None, _ptr(nu), _ptr(ws), nbytes, st)

    def binomial():
        o = clicks
        lib, st = o._mlib, o._stream()
        p, w = o._pw_tensors()
        nbytes = int(lib.cdll.obe_binomial_workspace_bytes(n_p, n_s, 1))
        ws = new(nbytes // 8 + 1)
        return lambda: lib.call("obe_binomial_information", o._model_struct, _ptr(o._settings_dev), n_s, n_s, _ptr(p), n_p,
                                n_p, _ptr(w), 1.0, None, 1.0, _ptr(info), _ptr(nu), _ptr(ws), nbytes, st)

    routes = [("obe_binomial_information", binomial(), None)]
    routes += [(f"obe_poisson_information cap {cap}", poisson(cap), cap) for cap in (16, 32, 64)]
    routes += [("obe_poisson_information d_noise_var alone", poisson(32, False), None)]
    lines = [f"# tools/poisson_timing.py on {torch.cuda.get_device_name(0)}: one library call per reading, obe_timer on the "
             "launch stream, one warming call, two readings",
             "# settings x particles      route                                          ms (two readings)      evals/s   tail_max"]
    st = counts._stream()
    for what, call, cap in routes:
        call()
        torch.cuda.synchronize()
        readings = []
        for _ in range(2):
            counts._lib.call("obe_timer_start", timer, st)
            call()
            counts._lib.call("obe_timer_stop", timer, st, ctypes.byref(ms))
            readings.append(float(ms.value))
        worst = f"{float(tail.max().item()):.2e}" if cap else "-"
        lines.append(f"{n_s:6d} x {n_p:8d}         {what:44s} {readings[0]:9.2f} {readings[1]:9.2f}   "
                     f"{n_s * n_p / (min(readings) * 1e-3):9.3g}   {worst}")
        print(lines[-1], flush=True)
    counts._lib.call("obe_timer_destroy", timer)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
