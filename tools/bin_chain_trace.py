"""The bin sweep's launch chain in a rocprofv3 kernel trace of bench.py (developer aid; the tables of
profiles/bin_chain.txt):

    rocprofv3 --kernel-trace --stats -d out -o t -- python3 bench.py --gpus 1 --steps 20 --warmup 5 \
        --no-other-configs --no-cpu-baseline
    python tools/bin_chain_trace.py <results.db> [label]

The kernels between the ends of the last 21 full bin_eval launches (20 cycles; a launch under 5 us is an aborted
speculative sweep): kernel time and launches per cycle, every kernel with its time per cycle, calls per cycle and mean
per call, the grouping's kernels split by whether a resample ran since the previous full sweep, and the launches of a
sweep in front of bin_moments_kernel after a resample."""
import sqlite3
import sys
from collections import defaultdict

import numpy as np

CYCLES = 20
GROUPING = ("sweep_pack_kernel", "bin_minmax_kernel", "bin_plan_kernel", "bin_group_kernel", "bin_scan_kernel",
            "bin_scatter_pack_kernel", "bin_refresh_kernel", "sweep_finalize")


def short(name):
    return name.replace("void ", "").replace("obe::", "").split("(")[0][:48]


def main(path, label):
    c = sqlite3.connect(path)
    rows = [(short(n), s, e) for n, s, e in c.execute("select name, start, end from kernels order by start")]
    full = [i for i, r in enumerate(rows) if r[0].startswith("bin_eval_kernel") and r[2] - r[1] > 5000]
    assert len(full) > CYCLES, len(full)
    first, last = full[-CYCLES - 1], full[-1]
    span = rows[first + 1:last + 1]
    per = defaultdict(list)
    for n, s, e in span:
        per[n].append((e - s) / 1e3)
    total = sum(sum(v) for v in per.values())
    print(f"{label}: kernel time {total / CYCLES:.1f} us per cycle in {len(span) / CYCLES:.1f} launches, "
          f"end to end {(rows[last][2] - rows[first][2]) / 1e3 / CYCLES:.1f} us per cycle")
    for n, v in sorted(per.items(), key=lambda kv: -sum(kv[1]))[:14]:
        print(f"  {sum(v) / CYCLES:9.2f} us/cycle  {len(v) / CYCLES:5.2f} calls/cycle  {np.mean(v):8.2f} us each  {n}")
    # the grouping's kernels of every full sweep, by whether a resample ran since the previous full sweep
    split = defaultdict(lambda: ([], []))
    chains = []
    for a, b in zip(full[-CYCLES - 1:-1], full[-CYCLES:]):
        between = rows[a + 1:b + 1]
        resampled = any(r[0].startswith("resample") for r in between)
        # the launches of the full sweep itself: everything behind the last kernel that is not the sweep's
        own = []
        for r in reversed(between[:-1]):
            if not (r[0].startswith(GROUPING) or r[0].startswith(("bin_moments_kernel", "bin_fold_kernel"))):
                break
            own.append(r)
        own.reverse()
        for n, s, e in own:
            if n.startswith(GROUPING):
                split[n][resampled].append((e - s) / 1e3)
        if resampled:
            chains.append([n for n, _, _ in own if not n.startswith(("bin_moments_kernel", "bin_fold_kernel"))])
    for n, (plain, after) in sorted(split.items()):
        cell = lambda v: f"{np.mean(v):7.2f} us x{len(v):2d}" if v else "     -       "
        print(f"  {label}: {n:48s} no resample since the last sweep {cell(plain)}   after a resample {cell(after)}")
    for chain in chains[:1]:
        print(f"  {label}: in front of bin_moments_kernel after a resample, {len(chain)} launches: " + ", ".join(chain))
    n_fin = sum(1 for r in span if r[0].startswith("sweep_finalize"))
    print(f"  {label}: sweep_finalize launches in the {CYCLES} cycles: {n_fin}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "trace")
