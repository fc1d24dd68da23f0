"""Tracking a Lorentzian line whose centre moves during the run: the same experiment by two objects of the same seed,
one told that the centre drifts (``set_parameter_drift(..., per_update=True)``: every ``pdf_update()`` ends with a
prediction step on the device) and one that treats it as a constant, as the reference does
(demos/find_peak/sequentialLorentzian.py:88-150 is the loop; its line stands still).

The centre moves by PATH_WIDTHS line widths over PATH_CYCLES cycles at constant speed; the drifting object is given a
random walk of twice that step per cycle (standard deviation), which covers a steady motion without knowing its sign.

    python examples/drifting_line.py [n_particles] [n_cycles]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402  (same class names as the reference)

WIDTH = 0.1                              # the line's half width d
PATH_WIDTHS, PATH_CYCLES = 10.0, 200     # the centre's path: 10 widths in 200 cycles
STEP = PATH_WIDTHS * WIDTH / PATH_CYCLES
START, AMPLITUDE, BACKGROUND, NOISE = 2.5, -1000.0, 50000.0, 200.0


def lorentzian(x, x0, a, b):
    return b + a / (((x - x0) / WIDTH) ** 2 + 1.0)


def new_object(n_particles, seed, drifting):
    g = np.random.default_rng(seed)
    prior = (g.uniform(2.0, 3.0, n_particles), g.uniform(-2000.0, -400.0, n_particles),
             g.normal(BACKGROUND, 1000.0, n_particles))
    obe = optbayesexpt.OptBayesExpt(optbayesexpt.models.lorentzian(), (np.linspace(1.5, 4.5, 301),), prior, (WIDTH,))
    obe.rng = np.random.default_rng(seed + 1)
    if drifting:
        obe.set_parameter_drift({0: 2.0 * STEP}, per_update=True)       # x0 walks; a and b are constants
    return obe


def main(n_particles=8192, n_cycles=PATH_CYCLES, seed=0, quiet=False):
    """Runs both objects through ``n_cycles`` cycles of the moving line; returns ``(with drift, static)``: each
    object's final |mean x0 - centre| at the last measurement."""
    objects = [new_object(n_particles, seed, True), new_object(n_particles, seed, False)]
    noise = [np.random.default_rng(seed + 2), np.random.default_rng(seed + 2)]
    centre = START
    for k in range(n_cycles):
        centre = START + STEP * k
        for obe, g in zip(objects, noise):
            x = obe.opt_setting()
            y = lorentzian(float(x[0]), centre, AMPLITUDE, BACKGROUND) + NOISE * g.standard_normal()
            obe.pdf_update((x, y, NOISE))
    errors = tuple(abs(float(obe.mean()[0]) - centre) for obe in objects)
    if not quiet:
        for name, obe, err in zip(("with drift", "static"), objects, errors):
            print(f"{name:>10s}: x0 = {obe.mean()[0]:.4f} +/- {obe.std()[0]:.4f}; the centre is at {centre:.4f} "
                  f"(off by {err / WIDTH:.2f} widths)")
    return errors


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 8192, int(args[1]) if len(args) > 1 else PATH_CYCLES)
