"""Resonance search by single shots.  Each measurement is ONE yes/no outcome — a click or no click — whose probability
follows a Lorentzian line over the setting x:  p(x) = b + a / (1 + ((x - x0) / d)^2).  No sigma is invented for a 0/1
reading and no shots are averaged before an update: OptBayesExptBinomial takes the outcome as it is (a binomial
likelihood) and chooses every setting by the exact information, in nats, that the next shot carries about the parameters.

Every outcome is drawn with a seeded generator of its own, so the run can be repeated shot for shot.  Printed: the
estimate of the line's centre, height and background, and the number of shots used.

    python examples/binary_outcomes.py [n_shots] [n_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402

LINE_WIDTH = 0.1


def main(n_shots=400, n_samples=20000, seed=0, quiet=False):
    rng = np.random.default_rng(seed)
    model = optbayesexpt.models.lorentzian()
    settings = (np.linspace(2.0, 4.0, 201),)
    parameters = (rng.uniform(2.6, 3.4, n_samples), rng.uniform(0.3, 0.6, n_samples), rng.uniform(0.1, 0.3, n_samples))
    true_pars = (3.13, 0.5, 0.15)

    obe = optbayesexpt.OptBayesExptBinomial(model, settings, parameters, (LINE_WIDTH,), shots=1)
    obe.rng = np.random.default_rng(seed + 1)

    def click(x, shot):
        p = true_pars[2] + true_pars[1] / (((x[0] - true_pars[0]) / LINE_WIDTH) ** 2 + 1.0)
        return int(np.random.default_rng((seed, shot)).random() < p)          # (this outcome's own generator)

    clicks = 0
    for shot in range(n_shots):
        x = obe.opt_setting()
        k = click(x, shot)
        obe.pdf_update((x, k))
        clicks += k

    mean, std = obe.mean(), obe.std()
    if not quiet:
        print(f"{n_shots} single shots, {clicks} clicks")
        for label, t, m, s in zip(("x0", "a", "b"), true_pars, mean, std):
            print(f"{label:>3s} = {t:8.4f}; estimate {m:8.4f} +/- {s:7.4f}   error {m - t:+8.4f}")
    return true_pars, mean, std, n_shots


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
