"""Keeping a posterior physical with bounds instead of a hook — the lock-in measurement of a coil's impedance
(inductance L, resistance R, stray capacitance C, unknown noise sigma; the reference's demos/lockin/lockin_of_coil.py).

The reference's demo subclasses the noise-parameter class to override ``enforce_parameter_constraints()`` with a NumPy
loop that gives zero weight to every particle with a negative parameter (lockin_of_coil.py:115-133).  Such a hook
works here too, but it reads and writes the whole cloud on the host after every resample.  The same constraint as
data — R, L, C >= 0, next to the class's own sigma > 0 — stays on the device:

    coil_obe.set_parameter_bounds({0: (0, None), 1: (0, None), 2: (0, None)})

    python examples/bounded_parameters.py [n_measure] [n_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402


def main(n_measure=200, n_samples=50000, seed=0, quiet=False):
    rng = np.random.default_rng(seed)
    omega = 2 * np.pi * np.logspace(2, 6, 200)               # 100 Hz ... 1 MHz
    # priors on the scale of 1 mH, 10 Ohm, 10 uF, and a noise of 10 Ohm
    parameters = (rng.exponential(1e-3, n_samples), rng.exponential(10.0, n_samples),
                  rng.exponential(10e-6, n_samples), rng.exponential(10.0, n_samples))
    model = optbayesexpt.models.coil()
    coil_obe = optbayesexpt.OptBayesExptNoiseParameter(model, (omega,), parameters, (), scale=False,
                                                       noise_parameter_index=(3, 3))
    coil_obe.rng = np.random.default_rng(seed + 1)
    coil_obe.set_parameter_bounds({0: (0, None), 1: (0, None), 2: (0, None)})

    true_pars = tuple(rng.choice(p) for p in parameters)
    zeroed = 0
    for i in range(n_measure):
        wmeas = coil_obe.opt_setting()
        ymeasure = np.asarray(model(wmeas, true_pars, ())).reshape(-1) + true_pars[3] * rng.standard_normal(2)
        coil_obe.pdf_update((wmeas, tuple(ymeasure)))
        if coil_obe.just_resampled:
            zeroed += coil_obe.last_constraint_count
        if not quiet and i % 50 == 0:
            print(f"iteration {i:3d}")
    means, stds = coil_obe.mean(), coil_obe.std()
    if not quiet:
        for name, scale, unit, true, mean, std in zip(("L", "R", "C", "sigma"), (1e-3, 1, 1e-6, 1),
                                                      ("mH ", "Ohm", "uF ", "Ohm"), true_pars, means, stds):
            print(f"{name}: true = {true / scale:7.3f} {unit}  measured = ({mean / scale:7.3f} +/- {std / scale:7.3f}) {unit}")
        print(f"particles given zero weight by the bounds: {zeroed}")
    return true_pars, means, stds, zeroed


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:]])
