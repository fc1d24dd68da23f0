"""The fitted curve with its uncertainty — the find-peak loop of examples/find_peak.py, printing the posterior
predictive mean, standard deviation and 95 % credible band of the model at a few settings every few measurements.
The reference's demos draw the model at the mean parameters as the "Est." curve
(demos/line_plus_noise/line_plus_noise.py:138,181), a plug-in estimate without a band; here the model is evaluated
over the whole weighted cloud where the cloud lives, and only the few result values come back.

    python examples/predictive_band.py [n_measure] [n_samples] [every]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402


def main(n_measure=60, n_samples=50000, every=20, seed=0, quiet=False):
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
    x_show = np.linspace(true_pars[0] - 0.3, true_pars[0] + 0.3, 7)          # points, not the design grid
    true_curve = np.asarray(my_obe.model_function((x_show,), true_pars, constants), dtype=np.float64)

    history = []
    for i in range(1, n_measure + 1):
        xmeas = my_obe.opt_setting()
        my_obe.pdf_update((xmeas, my_sim.simdata(xmeas), noise_level))
        if i % every == 0 or i == n_measure:
            mean, std = my_obe.predict((x_show,))
            lo, hi = my_obe.predictive_interval(0.95, (x_show,))
            history.append((i, x_show, mean[0], std[0], lo[0], hi[0]))
            if not quiet:
                print(f"after {i} measurements")
                for x, m, s, a, b, t in zip(x_show, mean[0], std[0], lo[0], hi[0], true_curve):
                    print(f"   x = {x:.3f}  y = {m:9.1f} +- {s:6.1f}  95 % [{a:9.1f}, {b:9.1f}]  true {t:9.1f}")
    if not quiet:
        whole = my_obe.predict()[1]                                           # settings=None: the whole design grid
        print(f"largest standard deviation of the curve on the design grid: {whole.max():.1f}")
    return true_curve, history


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    main(*args)
