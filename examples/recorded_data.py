"""A recorded spectrum assimilated in one call.  A Lorentzian line was scanned yesterday: ``n_records`` readings on a
regular grid.  ``pdf_update_batch()`` takes them all at once — the joint log-likelihood of every particle in one pass,
then adaptively tempered stages with a resample in between, because a joint update of so many readings would leave a
handful of particles — and reports the log evidence of the whole data set.  The same data fed to ``pdf_update()`` one
reading at a time ends at the same posterior (within the Monte Carlo error of two particle filters).

    python examples/recorded_data.py [n_records] [n_samples]
"""
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402


def main(n_records=200, n_samples=50000, seed=0, quiet=False):
    rng = np.random.default_rng(seed)
    model = optbayesexpt.models.lorentzian()
    settings = (np.linspace(1.5, 4.5, 200),)
    constants = (0.1,)
    true_pars = (rng.uniform(2.5, 3.5), rng.uniform(-2000, -400), 50000.0)
    noise_level = 500.0

    def fresh(s):
        g = np.random.default_rng(seed + 10)
        parameters = (g.uniform(2, 4, n_samples), g.uniform(-2000, -400, n_samples), g.normal(50000, 1000, n_samples))
        obe = optbayesexpt.OptBayesExpt(model, settings, parameters, constants, scale=False)
        obe.rng = np.random.default_rng(seed + s)
        return obe

    # yesterday's scan
    x = np.linspace(1.5, 4.5, n_records)
    x0, a, b = true_pars
    y = b + a / (((x - x0) / constants[0]) ** 2 + 1) + noise_level * rng.standard_normal(n_records)

    batch = fresh(1)
    stages = []
    batch.pdf_update_batch((x,), y, noise_level, on_stage=stages.append)
    report = batch.last_batch_update
    if not quiet:
        for info in stages:
            print(f"stage {info['stage']:2d}: delta = {info['delta']:.6f}  beta = {info['beta']:.6f}  "
                  f"N_eff = {info['n_eff']:10.1f}")
        print(f"{len(report['stages'])} stages, {report['resamples']} resamples, "
              f"log evidence of the scan = {report['log_evidence']:.3f}")

    loop = fresh(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for xi, yi in zip(x, y):
            loop.pdf_update(((xi,), yi, noise_level))

    if not quiet:
        for name, t, m, s, m2, s2 in zip(("x0", "a", "b"), true_pars, batch.mean(), batch.std(), loop.mean(), loop.std()):
            print(f"{name:>3s} = {t:10.3f}; one call {m:10.3f} +/- {s:8.3f}; record by record {m2:10.3f} +/- {s2:8.3f}")
    return true_pars, (batch.mean(), batch.std()), (loop.mean(), loop.std()), report


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 200, int(args[1]) if len(args) > 1 else 50000)
