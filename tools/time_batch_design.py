"""opt_setting_batch(n) at the c3 cloud (1 048 576 x 3, Lorentzian) and the c5 cloud (524 288 x 10, seven peaks, sigma a
parameter row) for n = 1, 4 and 16, and next to it the yardstick of its cross pass: output_cross_covariance() against
output_covariance() with the same number of rows on the same cloud and settings (a cross pass is the same arithmetic
minus the S products, plus the table of the rows written once per call).

    python tools/time_batch_design.py [--out profiles/batch_design.txt]

Every route is a whole call as a user makes it, between two device events after two warming calls, repeated for at
least 0.3 s; the routes of one size alternate in one process, twice, and the smaller time of each is kept.  n picks
cost the two passes of predict() plus n - 1 cross passes over the whole grid and one over a single setting (the
information of the last reading).  "evals/s" is settings x particles x passes over the device time."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from time_predictive import build, device_clock, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_design.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_batch_design.py measures on the GPU: none is visible")
    g = np.random.default_rng(5)
    lines = [f"# tools/time_batch_design.py on {torch.cuda.get_device_name(0)}: whole calls, device events, warmed, the "
             "routes of a size in turn",
             "# size                               route                                     ms       evals/s"]
    for name, cfg in (("c3 1048576 x 3", "c3"), ("c5 524288 x 10", "c5")):
        o, _, _ = build(cfg, 1, g)
        n_p, n_s = o.n_particles, o.allsettings.shape[1]
        grid = np.asarray(o.allsettings)
        routes = []
        for n in (1, 4, 16):
            routes.append((f"opt_setting_batch({n})", lambda n=n: o.opt_setting_batch(n), n + 1))
        for r in sorted({1, min(4, o.n_dims), min(8, o.n_dims)}):
            pts = grid[:, :: max(1, n_s // r)][:, :r]
            routes.append((f"output_cross_covariance, {r} rows", lambda pts=pts: o.output_cross_covariance(pts), 2))
            routes.append((f"output_covariance, {r} rows", lambda r=r: o.output_covariance(dims=list(range(r))), 2))
        best = {}
        for _ in range(2):
            for what, call, _ in routes:
                best[what] = min(best.get(what, np.inf), timed(call, device_clock))
        for what, _, passes in routes:
            ms = best[what]
            lines.append(f"{name + f', {n_s} settings':34s}  {what:36s}  {ms:9.3f}  {passes * n_s * n_p / (ms * 1e-3):10.3g}")
            print(lines[-1], flush=True)
        del o
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
