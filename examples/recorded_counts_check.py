"""Is this count plausible, and where will the next one fall?  A photon-count spectrum checked point by point.

A Lorentzian line on a background was scanned with a counter and the scan assimilated (``pdf_update_batch()``, as in
recorded_counts.py).  Today's scan of 60 points is checked against what the fit predicts: ``count_interval()`` gives
the 95 % band of the next reading at every point — whole numbers, from the mixture of Poisson laws over the cloud, not
a Gaussian around the curve —, ``count_pvalue()`` the two-sided p-value of every recorded count, and
``count_logpmf()`` the log evidence of each record.  One reading was taken with the shutter half closed; its p-value
shows.

    python examples/recorded_counts_check.py [n_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402


def main(n_samples=20000, seed=0, quiet=False):
    rng = np.random.default_rng(seed)
    width, exposure = 0.1, 4.0
    x0, a, b = 3.05, 12.0, 3.0                                 # centre, height and background, in counts per exposure

    def rate(x):
        return b + a / (((x - x0) / width) ** 2 + 1)

    # yesterday's scan, assimilated in one call
    x_old = np.linspace(2.0, 4.0, 150)
    g = np.random.default_rng(seed + 10)
    obe = optbayesexpt.OptBayesExptPoisson(
        optbayesexpt.models.lorentzian(), (np.linspace(2.0, 4.0, 201),),
        (g.uniform(2.2, 3.8, n_samples), g.uniform(2.0, 30.0, n_samples), g.uniform(0.5, 8.0, n_samples)), (width,),
        exposure=exposure, scale=False)
    obe.rng = np.random.default_rng(seed + 1)
    obe.pdf_update_batch((x_old,), rng.poisson(exposure * rate(x_old)).astype(np.float64))

    # today's scan against the band the fit predicts
    x = np.linspace(2.5, 3.6, 60)
    counts = rng.poisson(exposure * rate(x)).astype(np.float64)
    lo, hi = obe.count_interval(0.95, (x,))                    # each (C, n_x): whole numbers
    inside = int(np.count_nonzero((counts >= lo[0]) & (counts <= hi[0])))
    p = obe.count_pvalue((x,), counts)[0]

    # one more reading, taken with the shutter half closed
    x_bad = x0
    k_bad = float(rng.poisson(0.5 * exposure * rate(x_bad)))
    p_bad = float(obe.count_pvalue((x_bad,), k_bad)[0, 0])
    logp_bad, logp_good = obe.count_logpmf((x_bad,), k_bad), obe.count_logpmf((x_bad,), float(round(exposure * rate(x_bad))))

    if not quiet:
        for j in range(0, x.size, 6):
            print(f"x = {x[j]:.3f}: {counts[j]:3.0f} counts, band {lo[0, j]:3.0f} .. {hi[0, j]:3.0f}, p = {p[j]:.3f}")
        print(f"inside the 95 % band: {inside} of {x.size}")
        print(f"smallest p-value: {p.min():.4f} at x = {x[np.argmin(p)]:.3f}")
        print(f"shutter half closed at x = {x_bad:.3f}: {k_bad:.0f} counts, p = {p_bad:.2e}, "
              f"log evidence {logp_bad:.2f} against {logp_good:.2f} for the expected count")
    return inside, p, p_bad


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20000)
