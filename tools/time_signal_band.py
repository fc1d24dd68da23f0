"""signal_interval(0.95) against the base class's reading_interval(0.95, sigma=...) on the same cloud (DESIGN.md section
3, K21; the output is kept in profiles/signal_band.txt): the c3 cloud (1 048 576 particles, the one-peak Lorentzian) and
a two-level band over 1 024 settings.  The base-class call is the yardstick: per evaluation the new pass adds a square
root and a reciprocal per channel to its erfc and exp.  Device events around the library calls alone
(obe_signal_noise_reading_quantiles, obe_predictive_reading_quantiles; the results stay on the device), five alternating
rounds of two calls after a warm-up, medians; the pass counts of both calls ride along (the bands differ, so the two do
not close in the same pass everywhere).

    python tools/time_signal_band.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optbayesexpt_amd as obe                              # noqa: E402
from optbayesexpt_amd import _lib                           # noqa: E402
from optbayesexpt_amd._devcall import cloud, model_call, ptr            # noqa: E402
from optbayesexpt_amd._reading import normal_quantiles                  # noqa: E402

n_p, n_s, max_passes = 1 << 20, 1024, 48
g = np.random.default_rng(1)
prior = np.array([g.uniform(2.6, 3.4, n_p), g.uniform(400.0, 2000.0, n_p), g.uniform(40.0, 60.0, n_p)])
grid = (np.linspace(2.0, 4.0, n_s),)
floor, gain = 5.0, 1.0
signal = obe.OptBayesExptSignalNoise(obe.models.lorentzian(1), grid, prior, (0.1,), noise_floor=floor, noise_gain=gain,
                                     scale=False)
base = obe.OptBayesExpt(obe.models.lorentzian(1), grid, prior, (0.1,), scale=False)
dev = signal._device
qs = np.array([0.025, 0.975])
zs = normal_quantiles(qs)
coef = signal._coefficients()
# the yardstick's sigma: the noise at the cloud's mean curve, so that both bands have the width of the same physics
sigma = torch.from_numpy(np.sqrt(floor * floor + gain * np.abs(base.predict()[0]))).to(dev).contiguous()
out = torch.empty((2, 1, n_s), dtype=torch.float64, device=dev)
passes = torch.empty((2, 1, n_s), dtype=torch.int32, device=dev)


def new():
    p, w = cloud(signal)
    model_call(signal, "obe_signal_noise_reading_quantiles", "obe_predictive_reading_workspace_bytes", (n_p, n_s, 1, 2),
               ptr(signal._settings_dev), n_s, n_s, _lib.host_ptr(coef), ptr(p), n_p, n_p, ptr(w), _lib.host_ptr(qs),
               _lib.host_ptr(zs), 2, max_passes, ptr(out), ptr(passes))


def old():
    p, w = cloud(base)
    model_call(base, "obe_predictive_reading_quantiles", "obe_predictive_reading_workspace_bytes", (n_p, n_s, 1, 2),
               ptr(base._settings_dev), n_s, n_s, ptr(sigma), n_s, None, ptr(p), n_p, n_p, ptr(w), _lib.host_ptr(qs),
               _lib.host_ptr(zs), 2, max_passes, ptr(out), ptr(passes))


def timed(f, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def pass_counts(f):
    f()
    torch.cuda.synchronize()
    c = passes.cpu().numpy()
    return {"max": int(c.max()), "mean": float(c.mean()), "unconverged": int((c < 0).sum())}


for f in (old, new, old, new):
    f()
torch.cuda.synchronize()
rounds = [(timed(old, 2), timed(new, 2)) for _ in range(5)]
t_old, t_new = (float(np.median([r[k] for r in rounds])) for k in (0, 1))
counts_old, counts_new = pass_counts(old), pass_counts(new)
lo, hi = signal.signal_interval(0.95)
# per pass both evaluate every open (setting, particle, level): the time per enqueued pass over the whole grid
print(f"# python tools/time_signal_band.py, {torch.cuda.get_device_name(0)} (times in ms; rounds: [reading_interval, "
      "signal_interval] per round)")
print(json.dumps({"reading_interval_ms": t_old, "signal_interval_ms": t_new, "ratio": t_new / t_old, "rounds": rounds,
                  "passes_reading_interval": counts_old, "passes_signal_interval": counts_new,
                  "band_width_on_the_peak": float((hi - lo).max()), "band_width_in_the_wings": float((hi - lo).min())}))
