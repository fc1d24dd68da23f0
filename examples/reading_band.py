"""Where will the next reading fall? — the find-peak loop of examples/find_peak.py with the 95 % band of READINGS next to
the curve's credible band.  ``predictive_interval()`` (examples/predictive_band.py) bounds the model curve alone:
measured points scatter far outside it once the fit is good.  ``reading_interval()`` is the band to draw against the
data, noise included: the inverse of ``predictive_cdf()`` (examples/outlier_check.py), computed where the cloud lives.
Here every reading is checked against the band that was fixed BEFORE it was taken, and at the end simulated readings
all over the design grid are checked against the band of the whole grid (``settings=None``).

    python examples/reading_band.py [n_measure] [n_samples] [n_check]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402


def main(n_measure=60, n_samples=50000, n_check=400, seed=0, quiet=False):
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

    inside = []                     # was the reading inside the band fixed before it was taken?
    for i in range(1, n_measure + 1):
        xmeas = my_obe.opt_setting()
        lo, hi = my_obe.reading_interval(0.95, xmeas, noise_level)
        ymeas = my_sim.simdata(xmeas)
        inside.append(bool(lo[0, 0] <= ymeas <= hi[0, 0]))
        my_obe.pdf_update((xmeas, ymeas, noise_level))
        if not quiet and (i % 20 == 0 or i == n_measure):
            print(f"reading {i:3d} at x = {xmeas[0]:.3f}: {float(ymeas):9.1f}  95 % of readings [{lo[0, 0]:9.1f}, "
                  f"{hi[0, 0]:9.1f}]  {'inside' if inside[-1] else 'OUTSIDE'}")

    # the whole design grid: the curve's credible band, and the envelope of 95 % of the readings
    curve_lo, curve_hi = my_obe.predictive_interval(0.95)
    read_lo, read_hi = my_obe.reading_interval(0.95, sigma=noise_level)
    x_grid = settings[0]
    if not quiet:
        for k in range(0, x_grid.size, 25):
            print(f"   x = {x_grid[k]:.3f}  curve 95 % [{curve_lo[0, k]:9.1f}, {curve_hi[0, k]:9.1f}]  "
                  f"readings 95 % [{read_lo[0, k]:9.1f}, {read_hi[0, k]:9.1f}]")
    for k in rng.integers(0, x_grid.size, n_check):
        y = my_sim.simdata((x_grid[k],))
        inside.append(bool(read_lo[0, k] <= y <= read_hi[0, k]))
    fraction = float(np.mean(inside))
    if not quiet:
        print(f"{len(inside)} readings, {100.0 * fraction:.1f} % of them inside their 95 % band; the curve's own band is "
              f"{np.mean(curve_hi - curve_lo):.0f} wide on average, the readings' {np.mean(read_hi - read_lo):.0f}")
    return true_pars, fraction, len(inside), (curve_lo, curve_hi, read_lo, read_hi)


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    main(*args)
