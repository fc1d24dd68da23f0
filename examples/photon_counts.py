"""Resonance search by photon counting.  Each measurement is a COUNT of a few events in one exposure, whose rate dips on
a Lorentzian line over the setting x:  r(x) = b + a / (1 + ((x - x0) / d)^2) with a < 0, between 2 and 7 counts per
reading.  No Gaussian is fitted to a handful of counts: OptBayesExptPoisson takes the count as it is (a Poisson
likelihood) and chooses every setting by the exact information, in nats, that the next count carries about the
parameters — the reading censored at count_cap, whose tail mass last_information reports.

Every count is drawn with a seeded generator of its own, so the run can be repeated reading for reading.  Printed: the
estimate of the line's centre, depth and background, last_information, and the predicted histogram of the next reading
at the chosen setting (count_distribution()), as text.

    python examples/photon_counts.py [n_readings] [n_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402

LINE_WIDTH = 0.1


def main(n_readings=300, n_samples=20000, seed=0, quiet=False):
    rng = np.random.default_rng(seed)
    model = optbayesexpt.models.lorentzian()
    settings = (np.linspace(2.0, 4.0, 201),)
    parameters = (rng.uniform(2.6, 3.4, n_samples), rng.uniform(-6.0, -3.0, n_samples), rng.uniform(6.5, 8.0, n_samples))
    true_pars = (3.13, -5.0, 7.0)

    obe = optbayesexpt.OptBayesExptPoisson(model, settings, parameters, (LINE_WIDTH,), exposure=1.0, count_cap=32)
    obe.rng = np.random.default_rng(seed + 1)

    def count(x, reading):
        rate = true_pars[2] + true_pars[1] / (((x[0] - true_pars[0]) / LINE_WIDTH) ** 2 + 1.0)
        return int(np.random.default_rng((seed, reading)).poisson(obe.exposure * rate))      # (this reading's own generator)

    events = 0
    for reading in range(n_readings):
        x = obe.opt_setting()
        k = count(x, reading)
        obe.pdf_update((x, k))
        events += k

    mean, std = obe.mean(), obe.std()
    x = obe.opt_setting()
    histogram = obe.count_distribution((np.array([x[0]]),))[0]
    if not quiet:
        print(f"{n_readings} readings, {events} counted events")
        for label, t, m, s in zip(("x0", "a", "b"), true_pars, mean, std):
            print(f"{label:>3s} = {t:8.4f}; estimate {m:8.4f} +/- {s:7.4f}   error {m - t:+8.4f}")
        print(f"last_information = {obe.last_information}")
        print(f"the next reading at x = {x[0]:.3f}: P(k) for k = 0 .. 15, then P(k >= {obe.count_cap})")
        for k, p in enumerate(histogram[:16]):
            print(f"{k:>4d} {p:7.4f} {'#' * int(round(200 * p))}")
        print(f">={obe.count_cap:>2d} {histogram[-1]:7.1e}")
    return true_pars, mean, std, n_readings, histogram


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
