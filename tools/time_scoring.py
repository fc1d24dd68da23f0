"""Scoring readings against the posterior predictive (predictive_logpdf, predictive_cdf) on the device against the
routes that gave the same numbers before them, at the c3 cloud (1 048 576 x 3, Lorentzian, known sigma) and the c5 cloud
(524 288 x 10, seven peaks, sigma a parameter row) for 1, 64 and 1 024 records.

    python tools/time_scoring.py [--out profiles/scoring.txt]

Every route is a whole call as a user makes it, between two device events after two warming calls, repeated for at
least 0.3 s (host route: a host clock around single runs); the routes of one size alternate in one process, twice, and
the smaller time of each is kept.  Routes:
  predictive_logpdf             obe_predictive_logpdf (one pass over the cloud, one exp per evaluation)
  predictive_cdf                obe_predictive_tails (one pass, one erfc per evaluation and channel; both tails)
  eval + likelihood + sum       per record: eval_over_all_parameters on the device, the likelihood kernel on its rows
                                (obe_likelihood_y), then log((w L).sum() / w.sum()) with torch: what there was before
  host (8 records, x n / 8)     the cloud copied to the host once, the model, scipy's logsumexp and ndtr per record, on 8
                                records; the figure is that time scaled to the full number of records
"evals/s" is records x particles over the device time."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import optbayesexpt_amd as obe  # noqa: E402
from time_predictive import build, device_clock, host_clock, timed  # noqa: E402

HOST_RECORDS = 8


def records(o, cons, n_r, g):
    """n_r records near the mean curve: points, readings and (base class) their known sigma."""
    x = np.sort(g.uniform(1.5, 4.5, n_r))
    mean, std = o.predict((x,))
    known = type(o) is obe.OptBayesExpt
    sigma = 500.0 * g.uniform(0.5, 2.0, n_r) if known else None
    noise = sigma if known else float(np.sqrt(np.asarray(o.yvar_noise_model()).reshape(-1)[0]))
    y = mean[0] + noise * g.standard_normal(n_r)
    return x, y, sigma


def composed_logpdf(o, x, y, sigma):
    w = o._weights.tensor()
    sw = w.sum()
    out = torch.empty(x.size, dtype=torch.float64, device=w.device)
    for r in range(x.size):
        rec = ((x[r],), y[r]) if sigma is None else ((x[r],), y[r], sigma[r])
        lik = o._likelihood_device(o._eval_over_all_parameters_device(rec[0]), rec)
        out[r] = torch.log((lik * w).sum() / sw)
    return out.cpu().numpy() - 0.5 * np.log(2.0 * np.pi)


def host_route(o, x, y, sigma, cons):
    from scipy import special, stats
    o._particles._host_valid = o._weights._host_valid = False       # as behind a device-side update: one copy
    p, w = np.array(o.particles), np.array(o.particle_weights)
    out = []
    for r in np.linspace(0, x.size - 1, min(HOST_RECORDS, x.size)).astype(int):
        f = np.asarray(o.model_function((x[r],), p, cons), dtype=np.float64).reshape(-1)
        s = sigma[r] if sigma is not None else p[int(o._noise_rows[0])]
        with np.errstate(all="ignore"):
            logp = special.logsumexp(stats.norm.logpdf(y[r], f, s), b=w) - np.log(w.sum())
            out.append((logp, np.sum(w * special.ndtr((y[r] - f) / s)) / w.sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scoring.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_scoring.py measures on the GPU: none is visible")
    g = np.random.default_rng(5)
    lines = [f"# tools/time_scoring.py on {torch.cuda.get_device_name(0)}: whole calls, device events, warmed, the "
             "routes of a size in turn",
             "# size                           route                                     ms       evals/s   agrees"]
    for name, cfg in (("c3 1048576 x 3", "c3"), ("c5 524288 x 10", "c5")):
        o, _, cons = build(cfg, 1, g)
        n_p = o.n_particles
        for n_r in (1, 64, 1024):
            x, y, sigma = records(o, cons, n_r, g)
            want = o.predictive_logpdf((x,), y, sigma)
            got = composed_logpdf(o, x, y, sigma)
            agrees = f"{np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))):.1e}"
            host_n = min(HOST_RECORDS, n_r)
            routes = [("predictive_logpdf", lambda: o.predictive_logpdf((x,), y, sigma), device_clock, "-"),
                      ("predictive_cdf", lambda: o.predictive_cdf((x,), y, sigma), device_clock, "-"),
                      ("eval + likelihood + sum", lambda: composed_logpdf(o, x, y, sigma), device_clock, agrees),
                      (f"host ({host_n} records, x {n_r / host_n:.4g})", lambda: host_route(o, x, y, sigma, cons),
                       host_clock, "-")]
            best = {}
            for _ in range(2):
                for what, call, clock, _ in routes:
                    ms = timed(call, clock) if clock is device_clock else timed(call, clock, 0.0, 0, 1)
                    best[what] = min(best.get(what, np.inf), ms)
            for what, call, clock, agree in routes:
                ms = best[what] * (n_r / host_n if clock is host_clock else 1.0)
                rate = f"{n_r * n_p / (ms * 1e-3):.3g}" if clock is device_clock else "-"
                lines.append(f"{name + f', {n_r} records':30s}  {what:36s}  {ms:9.3f}  {rate:>10s}   {agree}")
                print(lines[-1], flush=True)
        del o
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
