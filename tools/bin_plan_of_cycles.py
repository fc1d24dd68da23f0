"""The bins the sweeps of the benchmark's cycles actually have (developer aid): bench.py's experiment of a config,
stepped as bench.py steps it, and after the warm-up and after the last step the plan in the object's keep buffer read
back — `nbins` of the plan and how many of the bins hold draws.  Nothing is timed.

    python tools/bin_plan_of_cycles.py [c3|c2] [steps=20] [warmup=5]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch        # noqa: E402,F401
import bench        # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "c3"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 5
settings, prior, cons, true, sigma = bench.make_workload(cfg)
obe = bench.build_obe(cfg, None, settings, prior.copy(), cons)
obe.rng = np.random.default_rng(1234)
sim = np.random.default_rng(4321)


def plan():
    """(nbins, poison, occupied bins) of the head of the keep buffer: BinPlan {double origin; int nbins; unsigned
    poison}, then binstart[OBE_BIN_MAX + 2] from int 16 on (csrc/obe_sweep_bins.h: BinKeep, BinKeepLayout)."""
    keep = obe.__dict__.get("_bins_keep")
    if keep is None:
        return None
    head = keep[1][:16 + 130].cpu().numpy()
    nbins = int(head[2])
    starts = head[16:16 + nbins + 1]
    return nbins, int(head[3]), int(np.count_nonzero(np.diff(starts)))


resamples = 0
for k in range(warmup + steps):
    x = obe.opt_setting()
    y = float(np.atleast_1d(obe.model_function(x, true, cons))[0]) + sigma * sim.standard_normal()
    obe.pdf_update((x, y, sigma))
    resamples += int(obe.just_resampled)
    if k + 1 in (warmup, warmup + steps) or obe.just_resampled:
        print(f"{cfg} after step {k + 1:3d} ({'resampled' if obe.just_resampled else 'plain'}): last sweep "
              f"{obe.last_sweep.get('bins')}, plan (nbins, poison, occupied) = {plan()}", flush=True)
print(f"{cfg}: {resamples} resamples in {warmup + steps} steps")
