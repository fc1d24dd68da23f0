"""Plan a batch for the parameter you care about.  ``opt_setting_batch(n)`` spends its readings where the model output
varies most, whatever parameter causes that; ``opt_setting_batch(n, interest=...)`` asks what each reading teaches about
chosen parameters, the others being nuisances, and accounts for what the readings before it will already have taught.
The same cloud is designed here for the line centre x0 alone and for the background b alone: the first batch sits on the
flanks of the peak, the second far from it.  ``last_batch_design["variance_left"]`` is the variance of each parameter of
interest that the best linear estimator leaves after the first j + 1 readings (linear-Gaussian: exact for a model that
is linear in its parameters with a Gaussian cloud, a heuristic for a Lorentzian, and greedy, not the optimal set).

    python examples/batch_design_interest.py [n_batch] [n_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402


def main(n_batch=6, n_samples=3000, seed=0, quiet=False):
    rng = np.random.default_rng(seed)
    model = optbayesexpt.models.lorentzian()
    settings = (np.linspace(1.5, 4.5, 65),)
    parameters = (rng.uniform(2, 4, n_samples), rng.uniform(-2000, -400, n_samples), rng.normal(50000, 1000, n_samples))
    obe = optbayesexpt.OptBayesExpt(model, settings, parameters, (0.1,), scale=False, default_noise_std=500.0)

    out = {}
    for name, row in (("x0", 0), ("b", 2)):
        xs = obe.opt_setting_batch(n_batch, interest=row)
        design = obe.last_batch_design
        left = design["variance_left"][:, 0] / design["prior_variance"][0]
        out[name] = design["indices"], left
        if not quiet:
            print(f"a batch for {name:>2s}: indices {design['indices'].tolist()}, x = {np.array2string(xs[0], precision=3)}")
            print(f"    variance left / prior variance after each reading: {np.array2string(left, precision=4)}")
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 6, int(args[1]) if len(args) > 1 else 3000)
