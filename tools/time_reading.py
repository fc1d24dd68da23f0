"""The band of the next reading (reading_interval) at the sizes of tools/time_predictive.py: the c3 cloud (1 048 576 x 3,
Lorentzian, known sigma) and the c5 cloud (524 288 x 10, seven peaks, sigma from a noise row) with 1 024 settings, and
demo size, next to predictive_interval (the curve's band) on the same object.

    python tools/time_reading.py [--out FILE]          (the lines are meant for profiles/predictive.txt)

A whole call as a user makes it — the bracket pass, the budget of 48 (pass, step) pairs, the copies of the results —
between two device events after two warming calls, repeated for at least 0.3 s.  "passes": the largest and the mean
number of passes a result used; a pass whose setting tile has closed costs a launch and nothing else."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench  # noqa: E402
import optbayesexpt_amd as obe  # noqa: E402
from time_predictive import build, device_clock, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_reading.py measures on the GPU: none is visible")
    g = np.random.default_rng(5)
    lines = [f"# tools/time_reading.py on {torch.cuda.get_device_name(0)}: whole calls, device events, warmed",
             "# size                           route                                     ms   passes max / mean   still open"]
    for name, cfg, n_s in (("c3 1048576 x 3, 1024 settings", "c3", 1024), ("c5 524288 x 10, 1024 settings", "c5", 1024),
                           ("demo 5000 x 3, 201 settings", "demo", 201)):
        o, x, _ = build(cfg, n_s, g)
        sigma = (500.0 if cfg == "demo" else bench.make_workload(cfg)[4]) if type(o) is obe.OptBayesExpt else None
        _, _, info = o.reading_interval(0.95, x, sigma, full_output=True)
        used = info["passes"][info["passes"] > 0]
        ms = timed(lambda: o.reading_interval(0.95, x, sigma), device_clock)
        lines.append(f"{name:30s}  {'reading_interval(0.95)':36s}  {ms:9.3f}   {used.max():3d} / {used.mean():5.2f}"
                     f"          {info['unconverged']}")
        print(lines[-1], flush=True)
        ms = timed(lambda: o.predictive_interval(0.95, x), device_clock)
        lines.append(f"{name:30s}  {'predictive_interval(0.95)':36s}  {ms:9.3f}   -")
        print(lines[-1], flush=True)
        del o
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
