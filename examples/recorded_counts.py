"""A recorded photon-count spectrum assimilated in one call, and two models compared on it.  A Lorentzian line on a
background was scanned yesterday with a counter: ``n_records`` whole numbers of events.  ``OptBayesExptPoisson``'s
``pdf_update_batch()`` takes them all at once — the joint Poisson log-likelihood of every particle in one pass over
records x particles, then adaptively tempered stages with a resample in between — and reports the log evidence of the
counts, ``-log k!`` included.  A second model, a flat rate with no line at all, gets the same counts: the difference of
the two log evidences is the log Bayes factor for the line.

    python examples/recorded_counts.py [n_records] [n_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402


def main(n_records=200, n_samples=50000, seed=0, quiet=False):
    rng = np.random.default_rng(seed)
    settings = (np.linspace(2.0, 4.0, 201),)
    width, exposure = 0.1, 1.0
    true_pars = (rng.uniform(2.8, 3.2), 12.0, 3.0)             # centre, height and background, in counts per exposure

    # yesterday's scan
    x = np.linspace(2.0, 4.0, n_records)
    x0, a, b = true_pars
    counts = rng.poisson(exposure * (b + a / (((x - x0) / width) ** 2 + 1))).astype(np.float64)

    g = np.random.default_rng(seed + 10)
    line = optbayesexpt.OptBayesExptPoisson(
        optbayesexpt.models.lorentzian(), settings,
        (g.uniform(2.2, 3.8, n_samples), g.uniform(2.0, 30.0, n_samples), g.uniform(0.5, 8.0, n_samples)), (width,),
        exposure=exposure, scale=False)
    line.rng = np.random.default_rng(seed + 1)
    stages = []
    line.pdf_update_batch((x,), counts, on_stage=stages.append)
    report = line.last_batch_update

    flat = optbayesexpt.OptBayesExptPoisson(optbayesexpt.models.first_parameter(), settings,
                                            (g.uniform(0.5, 30.0, n_samples),), (), exposure=exposure, scale=False)
    flat.rng = np.random.default_rng(seed + 2)
    flat.pdf_update_batch((x,), counts)
    flat_report = flat.last_batch_update

    if not quiet:
        for info in stages:
            print(f"stage {info['stage']:2d}: delta = {info['delta']:.6f}  beta = {info['beta']:.6f}  "
                  f"N_eff = {info['n_eff']:10.1f}")
        print(f"{len(report['stages'])} stages, {report['resamples']} resamples")
        print(f"centre = {x0:.4f}; posterior {line.mean()[0]:.4f} +/- {line.std()[0]:.4f}")
        print(f"log evidence, a line on a background: {report['log_evidence']:.3f}")
        print(f"log evidence, a flat rate:            {flat_report['log_evidence']:.3f}")
        print(f"log Bayes factor for the line:        {report['log_evidence'] - flat_report['log_evidence']:.3f}")
    return true_pars, (line.mean(), line.std()), report, flat_report


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 200, int(args[1]) if len(args) > 1 else 50000)
