"""A recorded data set assimilated in one call (pdf_update_batch(tempered=False), records_loglik) against the route that
gave the same weights before it, R sequential pdf_update() calls with auto_resample=False, at the c3 cloud
(1 048 576 x 3, Lorentzian, known sigma) and the c5 cloud (524 288 x 10, seven peaks, sigma a parameter row) for 1, 64
and 1 024 records.

    python tools/time_batch_update.py [--out profiles/batch_update.txt]

Every route is a whole call as a user makes it, between two device events after two warming calls, repeated for at
least 0.3 s; the routes of one size alternate in one process, twice, and the smaller time of each is kept.  The two
updating routes start from the same weights every time (a device-to-device copy inside the timed call, the same for
both).  Routes:
  pdf_update_batch(tempered=False)   obe_records_loglik, obe_tempered_sums, obe_tempered_likelihood,
                                     obe_bayes_update_lik: records x particles evaluations in one pass
  records_loglik                     obe_records_loglik and the (N_p,) result copied to the host
  R x pdf_update()                   the fused update of one record, R times (two passes over the cloud and a host
                                     round trip each)
"evals/s" is records x particles over the device time; "agrees" the largest difference between the weights of the two
updating routes over the largest weight."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import optbayesexpt_amd as obe  # noqa: E402
from time_predictive import build, device_clock, timed  # noqa: E402


def records(o, n_r, g):
    """n_r records near the mean curve; a known sigma grows with sqrt(n_r), so that the data set carries the same
    information at every size."""
    x = np.sort(g.uniform(1.5, 4.5, n_r))
    mean, _ = o.predict((x,))
    known = type(o) is obe.OptBayesExpt
    sigma = 500.0 * np.sqrt(n_r) * g.uniform(0.5, 2.0, n_r) if known else None
    noise = sigma if known else float(np.sqrt(np.asarray(o.yvar_noise_model()).reshape(-1)[0]))
    return x, mean[0] + noise * g.standard_normal(n_r), sigma


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_update.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_batch_update.py measures on the GPU: none is visible")
    g = np.random.default_rng(5)
    lines = [f"# tools/time_batch_update.py on {torch.cuda.get_device_name(0)}: whole calls, device events, warmed, the "
             "routes of a size in turn",
             "# size                           route                                     ms       evals/s   agrees"]
    for name, cfg in (("c3 1048576 x 3", "c3"), ("c5 524288 x 10", "c5")):
        o, _, cons = build(cfg, 1, g)
        o.tuning_parameters["auto_resample"] = False
        n_p = o.n_particles
        start = o._weights.tensor().clone()

        def restore():
            o._weights.tensor().copy_(start)
            o._weights.mark_device_written()

        for n_r in (1, 64, 1024):
            x, y, sigma = records(o, n_r, g)

            def batch():
                restore()
                o.pdf_update_batch((x,), y, sigma, tempered=False)

            def loop():
                restore()
                for r in range(n_r):
                    o.pdf_update(((x[r],), y[r]) if sigma is None else ((x[r],), y[r], sigma[r]))

            batch()
            w_batch = o._weights.tensor().clone()
            loop()
            w_loop = o._weights.tensor()
            agrees = f"{float((w_batch - w_loop).abs().max() / w_loop.max()):.1e}"
            routes = [("pdf_update_batch(tempered=False)", batch, "-"),
                      ("records_loglik", lambda: o.records_loglik((x,), y, sigma), "-"),
                      (f"{n_r} x pdf_update()", loop, agrees)]
            best = {}
            for _ in range(2):
                for what, call, _ in routes:
                    best[what] = min(best.get(what, np.inf), timed(call, device_clock))
            for what, _, agree in routes:
                ms = best[what]
                lines.append(f"{name + f', {n_r} records':30s}  {what:36s}  {ms:9.3f}  {n_r * n_p / (ms * 1e-3):10.3g}   {agree}")
                print(lines[-1], flush=True)
        del o
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
