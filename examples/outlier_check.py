"""Is this reading plausible?  The find-peak loop of examples/find_peak.py with every tenth reading replaced by a gross
outlier (a glitch of the instrument).  Before a reading is used, its two-sided p-value under the posterior predictive
— the model curve over the whole cloud AND the measurement noise — is printed; a reading below ``reject_below`` is set
aside instead of being fed to pdf_update().  The predictive log-density of every reading that is used, summed over
the run, is the log evidence of the model: the number to compare two candidate models with.

    python examples/outlier_check.py [n_measure] [n_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as optbayesexpt                     # noqa: E402


def main(n_measure=60, n_samples=50000, seed=0, reject_below=1e-6, quiet=False):
    rng = np.random.default_rng(seed)
    my_model_function = optbayesexpt.models.lorentzian()

    xvals = np.linspace(1.5, 4.5, 200)
    settings = (xvals,)
    x0_samples = rng.uniform(2, 4, n_samples)
    a_samples = rng.uniform(-2000, -400, n_samples)
    b_samples = rng.normal(50000, 1000, n_samples)
    parameters = (x0_samples, a_samples, b_samples)
    constants = (0.1,)

    my_obe = optbayesexpt.OptBayesExpt(my_model_function, settings, parameters, constants, scale=False)
    my_obe.rng = np.random.default_rng(seed + 1)
    optbayesexpt.obe_utils.rng = np.random.default_rng(seed + 2)

    true_pars = (rng.uniform(2.5, 3.5), rng.uniform(-2000, -400), 50000.0)
    noise_level = 500.0
    my_sim = optbayesexpt.MeasurementSimulator(my_obe.model_function, true_pars, constants, noise_level=noise_level)

    log_evidence = 0.0
    history = []                       # (reading number, it was a glitch, p-value, it was used)
    for i in range(n_measure):
        xmeas = my_obe.opt_setting()
        ymeasure = my_sim.simdata(xmeas)
        glitch = i % 10 == 9
        if glitch:
            ymeasure = ymeasure + 40.0 * noise_level * (1.0 if i % 20 == 9 else -1.0)
        record = (xmeas, ymeasure, noise_level)
        p = float(my_obe.predictive_pvalue(*record)[0, 0])
        use = p >= reject_below
        if use:
            log_evidence += my_obe.predictive_logpdf(*record)      # before the update: the one-step evidence
            my_obe.pdf_update(record)
        history.append((i, glitch, p, use))
        if not quiet:
            print(f"reading {i:3d} at x = {float(xmeas[0]):.3f}: p = {p:9.3g}  {'used' if use else 'SET ASIDE'}"
                  f"{'  (glitch)' if glitch else ''}   log evidence so far {log_evidence:.3f}")
    mean, std = my_obe.mean(), my_obe.std()
    if not quiet:
        for name, t, m, s in zip(("x0", "a", "b"), true_pars, mean, std):
            print(f"{name:>3s} = {t:10.3f}; measured {m:10.3f} +/- {s:8.3f}")
    return true_pars, mean, std, history, log_evidence


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 60, int(args[1]) if len(args) > 1 else 50000)
