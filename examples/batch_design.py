"""Plan a batch, measure it, assimilate it.  An instrument that takes a scan table of ``n_batch`` points per round trip
asks ``opt_setting_batch()`` which points to take: the first is ``opt_setting()``'s, every further one accounts for what
the ones before it will already have taught (greedy conditioning of the model output's variance, linear-Gaussian: an
approximation for a Lorentzian, and greedy, not the optimal set).  The readings of a round go to ``pdf_update_batch()``
in one call.

    python examples/batch_design.py [n_rounds] [n_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402


def main(n_rounds=12, n_samples=50000, n_batch=8, seed=0, quiet=False):
    rng = np.random.default_rng(seed)
    model = optbayesexpt.models.lorentzian()
    settings = (np.linspace(1.5, 4.5, 200),)
    constants = (0.1,)
    true_pars = (rng.uniform(2.5, 3.5), rng.uniform(-2000, -400), 50000.0)
    noise_level = 500.0
    parameters = (rng.uniform(2, 4, n_samples), rng.uniform(-2000, -400, n_samples), rng.normal(50000, 1000, n_samples))
    obe = optbayesexpt.OptBayesExpt(model, settings, parameters, constants, scale=False, default_noise_std=noise_level)
    obe.rng = np.random.default_rng(seed + 1)

    x0, a, b = true_pars
    for rnd in range(n_rounds):
        xs = obe.opt_setting_batch(n_batch)                   # plan 8
        x = xs[0]
        y = b + a / (((x - x0) / constants[0]) ** 2 + 1) + noise_level * rng.standard_normal(n_batch)      # simulate
        obe.pdf_update_batch(xs, y, noise_level)              # assimilate
        if not quiet:
            design = obe.last_batch_design
            print(f"round {rnd:2d}: x = {np.array2string(np.sort(x), precision=3)}  "
                  f"expected information {design['information'][-1]:.2f} nats  x0 = {obe.mean()[0]:.4f} +/- {obe.std()[0]:.4f}")
    if not quiet:
        for name, t, m, s in zip(("x0", "a", "b"), true_pars, obe.mean(), obe.std()):
            print(f"{name:>3s} = {t:10.3f}; estimate {m:10.3f} +/- {s:8.3f}")
    return true_pars, obe.mean(), obe.std()


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 12, int(args[1]) if len(args) > 1 else 50000)
