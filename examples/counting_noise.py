"""Photon counting: the brightest setting is also the noisiest one.  An emission peak on a small background is
measured with counting noise — a reading of a noise-free value y scatters with variance nu(y) = floor^2 + gain * |y| —
by two experiments side by side on the same prior:

  signal noise   OptBayesExptSignalNoise: the likelihood takes nu at every particle's own model value, and the design
                 divides the predicted variance of a setting by nu averaged over the cloud AT THAT SETTING
  flat noise     a plain OptBayesExpt in the recipe of the reference's counting demo (demos/pipulse/pipulse.py:104,170):
                 the record carries sigma = sqrt(y_meas), taken from the noisy reading itself, and the design assumes
                 one noise level everywhere

Each draws its own readings from the same simulator.  Printed: the settings each chose (as a histogram over the distance
from the true peak, in line widths) and both posteriors' errors.

    python examples/counting_noise.py [n_measure] [n_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402

LINE_WIDTH = 0.1


def main(n_measure=60, n_samples=50000, seed=0, quiet=False):
    rng = np.random.default_rng(seed)
    model = optbayesexpt.models.lorentzian()
    settings = (np.linspace(2.0, 4.0, 201),)
    parameters = (rng.normal(3.0, 0.05, n_samples), rng.uniform(400, 2000, n_samples), rng.normal(50, 5, n_samples))
    constants = (LINE_WIDTH,)
    floor, gain = 5.0, 1.0                                   # dark counts' sigma; raw Poisson counts

    signal = optbayesexpt.OptBayesExptSignalNoise(model, settings, parameters, constants, noise_floor=floor,
                                                  noise_gain=gain, utility_method="variance_full", scale=False)
    flat = optbayesexpt.OptBayesExpt(model, settings, parameters, constants, default_noise_std=floor,
                                     utility_method="variance_full", scale=False)
    signal.rng, flat.rng = np.random.default_rng(seed + 1), np.random.default_rng(seed + 1)

    true_pars = (rng.normal(3.0, 0.03), rng.uniform(800, 1600), 50.0)

    def reading(x):
        y = float(true_pars[2] + true_pars[1] / (((x[0] - true_pars[0]) / LINE_WIDTH) ** 2 + 1.0))
        return y + np.sqrt(floor * floor + gain * abs(y)) * rng.standard_normal()

    chosen = {"signal noise": [], "flat noise": []}
    for _ in range(n_measure):
        x = signal.opt_setting()
        signal.pdf_update((x, reading(x)))
        chosen["signal noise"].append(float(x[0]))
        x = flat.opt_setting()
        y = reading(x)
        flat.pdf_update((x, y, np.sqrt(max(y, 1.0))))        # the pipulse recipe: sigma from the noisy reading
        chosen["flat noise"].append(float(x[0]))

    result = {}
    for name, obj in (("signal noise", signal), ("flat noise", flat)):
        mean, std = obj.mean(), obj.std()
        result[name] = (mean, std, np.array(chosen[name]))
        if quiet:
            continue
        print(f"--- {name}")
        away = np.abs(np.array(chosen[name]) - true_pars[0]) / LINE_WIDTH
        counts, _ = np.histogram(away, bins=[0.0, 0.25, 0.75, 1.5, 3.0, np.inf])
        print("settings chosen, by distance from the peak in line widths  [0, 1/4) [1/4, 3/4) [3/4, 3/2) [3/2, 3) beyond:",
              " ".join(f"{c:3d}" for c in counts))
        for label, t, m, s in zip(("x0", "a", "b"), true_pars, mean, std):
            print(f"{label:>3s} = {t:10.4f}; measured {m:10.4f} +/- {s:8.4f}   error {m - t:+9.4f}")
    return true_pars, result


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
