"""Design for ONE parameter: the find_peak loop (examples/find_peak.py) run twice on the same simulated experiment —
with the reference's utility (``variance_approx``: where does the model output vary most, for any reason?) and with
``utility_method="parameter_variance"`` on the line centre ``x0`` (where does a reading remove most of x0's variance?
amplitude and background are nuisances) — and the final standard deviation of x0 of both.

    python examples/parameter_of_interest.py [n_measure] [n_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402


def run(utility_method, n_measure, n_samples, seed):
    rng = np.random.default_rng(seed)
    xvals = np.linspace(1.5, 4.5, 200)
    parameters = (rng.uniform(2, 4, n_samples), rng.uniform(-2000, -400, n_samples), rng.normal(50000, 1000, n_samples))
    constants = (0.1,)
    noise_level = 500.0
    my_obe = optbayesexpt.OptBayesExpt(optbayesexpt.models.lorentzian(), (xvals,), parameters, constants, scale=False,
                                       utility_method=utility_method, default_noise_std=noise_level)
    if utility_method == "parameter_variance":
        my_obe.set_parameters_of_interest([0])              # x0; a and b are nuisances
    my_obe.rng = np.random.default_rng(seed + 1)
    optbayesexpt.obe_utils.rng = np.random.default_rng(seed + 2)
    true_pars = (rng.uniform(2.5, 3.5), rng.uniform(-2000, -400), 50000.0)
    my_sim = optbayesexpt.MeasurementSimulator(my_obe.model_function, true_pars, constants, noise_level=noise_level)
    for _ in range(n_measure):
        xmeas = my_obe.opt_setting()
        my_obe.pdf_update((xmeas, my_sim.simdata(xmeas), noise_level))
    return true_pars, my_obe.mean(), my_obe.std()


def main(n_measure=100, n_samples=50000, seed=0, quiet=False):
    out = {}
    for method in ("variance_approx", "parameter_variance"):
        true_pars, mean, std = out[method] = run(method, n_measure, n_samples, seed)
        if not quiet:
            print(f"{method:>18s}: x0 = {true_pars[0]:.4f}; measured {mean[0]:.4f} +/- {std[0]:.5f}   "
                  f"(a +/- {std[1]:.1f}, b +/- {std[2]:.1f})")
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 100, int(args[1]) if len(args) > 1 else 50000)
