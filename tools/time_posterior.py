"""Posterior summaries on the device against the only route there was before them — ``particles`` and
``particle_weights`` copied to the host, then np.histogram / np.histogram2d / np.quantile — at the c3 cloud
(1 048 576 x 3) and the c5 cloud (524 288 x 10), for a freshly resampled and a sharply converged posterior.

    python tools/time_posterior.py [--out profiles/posterior_summaries.txt]

Device route: the method call as a user makes it (its kernels, the upload of the edges, the copy of the result),
between two device events around warmed-up calls repeated for at least 0.3 s.  Host route: the same answer from the
host mirrors, which a device-side update has made stale (so each repetition pays the copy of the cloud), by a host
clock around calls that end in that synchronising copy; the two routes alternate in one process.  "share" is the bytes
the algorithm must read (8 (rows + 1) per particle and pass over the cloud: the sum(w) pass, the min / max pass of an
automatic range, one histogram pass per group of rows, eight select passes of 16 bytes per row) over the device time, as a
share of 8 TB/s — a figure for the whole call, launches and copies included, not for a kernel."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import optbayesexpt_amd as obe  # noqa: E402

HBM = 8.0e12


def cloud(n, d, converged, g):
    x = g.normal(size=(d, n)) * 0.05 + np.arange(1, d + 1).reshape(d, 1)
    if converged:
        w = np.exp(-0.5 * ((x[0] - 1.003) / 0.0005) ** 2) * (0.5 + g.random(n))
        w /= w.sum()
    else:
        w = np.ones(n) / n
    pdf = obe.ParticlePDF(x)
    pdf.particle_weights = w
    pdf._pw_tensors()
    return pdf


def device_ms(call, min_seconds=0.3):
    for _ in range(3):
        call()
    reps, total = 0, 0.0
    while total < min_seconds * 1e3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            call()
        e1.record()
        e1.synchronize()
        total += e0.elapsed_time(e1)
        reps += 10
    return total / reps


def host_ms(pdf, call, reps):
    times = []
    for _ in range(reps):
        pdf._particles._host_valid = pdf._weights._host_valid = False       # as behind a device-side update
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(pdf.particles, pdf.particle_weights)
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_summaries.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_posterior.py measures on the GPU: none is visible")
    g = np.random.default_rng(5)
    lines = [f"# tools/time_posterior.py on {torch.cuda.get_device_name(0)}: device route (events around the method call) "
             "against the host route (D2H of the cloud + NumPy)",
             "# cloud            posterior  summary                      device ms  share of 8 TB/s    host ms   "
             "PCIe bytes device / host"]
    for name, n, d in (("c3 1048576 x 3", 1 << 20, 3), ("c5 524288 x 10", 1 << 19, 10)):
        for state in ("resampled", "converged"):
            pdf = cloud(n, d, state == "converged", g)
            cloud_bytes = 8 * n * (d + 1)
            # (summary, device call, host call, algorithmic bytes, result bytes that cross PCIe)
            rows_per_group = min(d, 4096 // 64)
            groups = -(-d // rows_per_group)
            work = [
                ("marginal_histogram 64 bins", lambda: pdf.marginal_histogram(bins=64),
                 lambda x, w: [np.histogram(r, 64, weights=w) for r in x],
                 8 * n + 8 * d * n + groups * 8 * n + 8 * d * n, 8 * d * (64 + 65 + 2)),
                ("joint_histogram 64 x 64", lambda: pdf.joint_histogram(0, 1, bins=64),
                 lambda x, w: np.histogram2d(x[0], x[1], 64, weights=w),
                 8 * n + 16 * n + 24 * n, 8 * (64 * 64 + 2 * 65 + 4)),
                ("credible_interval 95 %", lambda: pdf.credible_interval(0.95),
                 lambda x, w: [np.quantile(r, (0.025, 0.975), weights=w, method="inverted_cdf") for r in x],
                 8 * n + 8 * 16 * d * n, 8 * 2 * d),
            ]
            for what, dev_call, host_call, alg_bytes, pcie in work:
                t_dev, t_host = [], []
                for _ in range(2):                       # the two routes in turn
                    t_dev.append(device_ms(dev_call))
                    t_host.append(host_ms(pdf, host_call, 3))
                td, th = min(t_dev), min(t_host)
                lines.append(f"{name:16s}  {state:9s}  {what:27s}  {td:9.3f}  {alg_bytes / (td * 1e-3) / HBM:15.3f}  "
                             f"{th:9.1f}   {pcie} / {cloud_bytes}")
                print(lines[-1], flush=True)
            del pdf
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
