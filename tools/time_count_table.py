"""count_pmf(count_max=63) against count_distribution() at count_cap=64 (the output is kept in
profiles/count_table.txt): 1024 settings x 1 048 576 particles, the one-peak Lorentzian, one channel, exposure 4.  Device
events around the library calls alone (obe_count_table, obe_poisson_information with d_pmf alone; the results stay on
the device), five alternating rounds of three calls after a warm-up, medians.  Also whether the rows k < 64 of the two
are the same bits, the largest difference of the last column, and the binomial table at 63 shots on the same cloud.

    python tools/time_count_table.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as obe                              # noqa: E402
from optbayesexpt_amd import _counts                        # noqa: E402
from optbayesexpt_amd._devcall import cloud, ptr            # noqa: E402

n_p, n_s, cap = 1 << 20, 1024, 64
g = np.random.default_rng(1)
prior = np.array([g.uniform(2.6, 3.4, n_p), g.uniform(3.0, 8.0, n_p), g.uniform(2.0, 4.0, n_p)])
o = obe.OptBayesExptPoisson(obe.models.lorentzian(1), (np.linspace(2.0, 4.0, n_s),), prior, (0.1,), exposure=4.0,
                            count_cap=cap, scale=False)
dev = o._device
p, w = cloud(o)
x = o._settings_dev
law = o._COUNT_LAW
points = torch.cat([x, torch.full((1, n_s), 4.0, dtype=torch.float64, device=dev)]).contiguous()
old_pmf = torch.empty((cap + 1, n_s), dtype=torch.float64, device=dev)


def old():
    o._call(ptr(x), n_s, n_s, 4.0, None, 1.0, None, None, old_pmf, None)


def new():
    return _counts._table(o, law, points, 1, cap - 1, p, w)


def timed(f, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


for f in (old, new, old, new):
    f()
torch.cuda.synchronize()
rounds = [(timed(old, 3), timed(new, 3)) for _ in range(5)]
t_old, t_new = (float(np.median([r[k] for r in rounds])) for k in (0, 1))
new_pmf = new()

# the binomial table at 63 shots: the same Lorentzian read as a probability (a in [0.3, 0.6], b in [0.1, 0.3])
prior_b = np.array([prior[0], g.uniform(0.3, 0.6, n_p), g.uniform(0.1, 0.3, n_p)])
ob = obe.OptBayesExptBinomial(obe.models.lorentzian(1), (np.linspace(2.0, 4.0, n_s),), prior_b, (0.1,), shots=63,
                              scale=False)
pb, wb = cloud(ob)
points_b = torch.cat([ob._settings_dev, torch.full((1, n_s), 63.0, dtype=torch.float64, device=dev)]).contiguous()


def binomial():
    return _counts._table(ob, ob._COUNT_LAW, points_b, 1, 63, pb, wb)


binomial()
t_bin = float(np.median([timed(binomial, 3) for _ in range(5)]))
same_bits = bool(torch.equal(new_pmf[0, :cap].view(torch.int64), old_pmf[:cap].view(torch.int64)))
tail_diff = float((new_pmf[0, cap] - old_pmf[cap]).abs().max())
evals = n_p * n_s
out = {"count_distribution_ms": t_old, "count_pmf_ms": t_new, "ratio": t_new / t_old, "rounds": rounds,
       "rows_same_bits": same_bits, "tail_max_abs_diff": tail_diff,
       "count_pmf_outcome_sums_per_s": evals * cap / (t_new * 1e-3), "binomial_count_pmf_ms": t_bin}
print(json.dumps(out))
