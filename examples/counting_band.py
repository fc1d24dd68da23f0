"""Photon counting, continued: the band the next reading should fall in.  The experiment of counting_noise.py — an
emission peak on a small background, a reading of a noise-free value y scattering with variance
nu(y) = floor^2 + gain * |y| — is run with OptBayesExptSignalNoise; then, at a few settings across the peak,

  signal noise   signal_interval(0.95): the band of the next reading with nu at every particle's own model value
  flat noise     the band a flat sigma = floor would give on the same posterior (a plain OptBayesExpt holding the same
                 cloud, reading_interval(0.95, sigma=floor)): right in the wings, far too narrow on the peak

are printed side by side with the p-value of one fresh reading, and the fraction of fresh simulated readings that fall
inside each band.

    python examples/counting_band.py [n_measure] [n_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402

LINE_WIDTH = 0.1


def main(n_measure=60, n_samples=50000, n_check=2000, seed=0, quiet=False):
    rng = np.random.default_rng(seed)
    model = optbayesexpt.models.lorentzian()
    settings = (np.linspace(2.0, 4.0, 201),)
    parameters = (rng.normal(3.0, 0.05, n_samples), rng.uniform(400, 2000, n_samples), rng.normal(50, 5, n_samples))
    constants = (LINE_WIDTH,)
    floor, gain = 5.0, 1.0                                   # dark counts' sigma; raw Poisson counts

    signal = optbayesexpt.OptBayesExptSignalNoise(model, settings, parameters, constants, noise_floor=floor,
                                                  noise_gain=gain, utility_method="variance_full", scale=False)
    signal.rng = np.random.default_rng(seed + 1)
    true_pars = (rng.normal(3.0, 0.03), rng.uniform(800, 1600), 50.0)

    def reading(x):
        y = true_pars[2] + true_pars[1] / (((np.asarray(x[0]) - true_pars[0]) / LINE_WIDTH) ** 2 + 1.0)
        return y + np.sqrt(floor * floor + gain * np.abs(y)) * rng.standard_normal(np.shape(y))

    for _ in range(n_measure):
        x = signal.opt_setting()
        signal.pdf_update((x, float(reading(x))))

    # the same posterior under a flat sigma = floor
    flat = optbayesexpt.OptBayesExpt(model, settings, signal.particles, constants, scale=False)
    flat.particle_weights = signal.particle_weights

    points = float(signal.mean()[0]) + LINE_WIDTH * np.array([-8.0, -2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0, 8.0])
    lo, hi = (b[0] for b in signal.signal_interval(0.95, (points,)))
    flat_lo, flat_hi = (b[0] for b in flat.reading_interval(0.95, (points,), sigma=floor))
    fresh = reading((points,))
    pvalue = signal.signal_pvalue((points,), fresh)[0]

    x_check = rng.choice(settings[0], n_check)
    y_check = reading((x_check,))
    band, flat_band = signal.signal_interval(0.95, (x_check,)), flat.reading_interval(0.95, (x_check,), sigma=floor)
    inside = {"signal noise": float(np.mean((band[0][0] <= y_check) & (y_check <= band[1][0]))),
              "flat noise": float(np.mean((flat_band[0][0] <= y_check) & (y_check <= flat_band[1][0])))}
    if not quiet:
        print("  setting   95 % band, signal noise     95 % band, flat floor     a fresh reading   its p-value")
        for k, x in enumerate(points):
            print(f"{x:9.4f}   [{lo[k]:9.1f}, {hi[k]:9.1f}]   [{flat_lo[k]:9.1f}, {flat_hi[k]:9.1f}]   {fresh[k]:13.1f}   "
                  f"{pvalue[k]:11.3f}")
        for name, fraction in inside.items():
            print(f"{name}: {100.0 * fraction:.1f} % of {n_check} fresh readings inside its 95 % band")
    return points, (lo, hi), (flat_lo, flat_hi), inside


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
