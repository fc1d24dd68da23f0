"""Watching the posterior while it converges — the find-peak loop of examples/find_peak.py, printing the median, the
95 % credible interval and a 40-bin marginal of the peak position x0 every few measurements.  The reference's
demos read these from the whole cloud (demos/find_peak/seqLor_pdfevolve.py:156-163); here they are computed where the
cloud lives, and only the few result values come back — ``particles`` and ``particle_weights`` are never copied.

    python examples/posterior_summary.py [n_measure] [n_samples] [every]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402

BARS = " .:-=+*#%@"


def sparkline(mass):
    top = mass.max()
    return "".join(BARS[int(round((len(BARS) - 1) * m / top))] if top > 0 else " " for m in mass)


def main(n_measure=60, n_samples=50000, every=10, seed=0, quiet=False):
    rng = np.random.default_rng(seed)
    settings = (np.linspace(1.5, 4.5, 200),)
    parameters = (rng.uniform(2, 4, n_samples), rng.uniform(-2000, -400, n_samples), rng.normal(50000, 1000, n_samples))
    constants = (0.1,)
    my_obe = optbayesexpt.OptBayesExpt(optbayesexpt.models.lorentzian(), settings, parameters, constants, scale=False)
    my_obe.rng = np.random.default_rng(seed + 1)
    optbayesexpt.obe_utils.rng = np.random.default_rng(seed + 2)
    true_pars = (rng.uniform(2.5, 3.5), rng.uniform(-2000, -400), 50000.0)
    noise_level = 500.0
    my_sim = optbayesexpt.MeasurementSimulator(my_obe.model_function, true_pars, constants, noise_level=noise_level)

    history = []
    for i in range(1, n_measure + 1):
        xmeas = my_obe.opt_setting()
        my_obe.pdf_update((xmeas, my_sim.simdata(xmeas), noise_level))
        if i % every == 0 or i == n_measure:
            median = my_obe.median(dims=0)[0]
            lo, hi = my_obe.credible_interval(0.95, dims=0)[0]
            mass, edges = my_obe.marginal_histogram(dims=0, bins=40, range=(2.0, 4.0))
            history.append((i, median, lo, hi, mass[0], edges[0]))
            if not quiet:
                print(f"{i:4d}  x0 = {median:.4f}  95 % [{lo:.4f}, {hi:.4f}]  |{sparkline(mass[0])}|")
    if not quiet:
        print(f"true x0 = {true_pars[0]:.4f}")
    return true_pars, history


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    main(*args)
