#!/usr/bin/env python3
"""Record the fixture of tests/test_gpu_bin_eval_lanes.py: yvar of that file's seeded calls from the library as built,
on the GPU.  Run it on the commit whose bits are to be pinned, BEFORE the kernel changes:

    python tools/record_bin_eval_lanes_bits.py tests/golden/bin_eval_lanes_parent_bits.npz

and name that commit in the test file's docstring.  Everything is swept twice; the two results must be the same bits.
OBE_VARIANT=name records from tools/_variants/libobe_hip_name.so (tools/build_variant.py) instead.

    python tools/record_bin_eval_lanes_bits.py --coefficients

needs no GPU: on the NumPy restatement of tests/test_bin_expansion_host.py it counts for how many of the 86
coefficients of a bin's row a change shows in the 257 values of the test's prior of 4 099 draws - by one ulp in the
bin nearest the middle of the settings, and by the value of the neighbouring coefficient in every bin (what a row
fed from the wrong lane would do)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(path):
    import optbayesexpt_amd as obe
    from optbayesexpt_amd import _lib
    if os.environ.get("OBE_VARIANT"):
        _lib._LIB = _lib.HipLib(os.path.join(ROOT, "tools", "_variants", f"libobe_hip_{os.environ['OBE_VARIANT']}.so"),
                                allow_variant=True)
    import test_gpu_bin_eval_lanes as t
    print("library:", _lib.load().path)
    out, again = t.record(obe), t.record(obe)
    assert out.keys() == again.keys()
    for name, v in out.items():
        assert np.array_equal(v, again[name]), name
        assert np.all(np.isfinite(v)), name
    print(f"{len(out)} arrays, {sum(v.size for v in out.values())} values")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def coefficients():
    import test_bin_expansion_host as host
    import test_gpu_bin_eval_lanes as t
    cloud, w, d = t.placement_case()
    x = t.grid(d)[t.offset_of(257):t.offset_of(257) + 257]
    fold = host.fold_items
    state = {"bin": -1, "change": None}

    def folded(parts):                       # bin_variance() folds one row per occupied bin, in bin order
        state["bin"] += 1
        row = fold(parts)
        return state["change"](row.copy(), state["bin"]) if state["change"] else row

    def run(change):
        state["bin"], state["change"] = -1, change
        return host.bin_variance(x, cloud, w, d)

    host.fold_items = folded
    try:
        base, occupied = run(None)
        tau0 = cloud[0] / d
        middle = int((np.mean(x) / d - tau0.min()) / host.WIDTH)
        assert 0 <= middle < occupied
        ncoef = 3 * host.P + 2
        ulp, ulp_all, neighbour = [], [], []
        for k in range(ncoef):
            def one_ulp(row, b, k=k):
                if b == middle:
                    row[k] = np.nextafter(row[k], np.inf)
                return row

            def from_next_lane(row, b, k=k):
                row[k] = row[(k + 1) % ncoef]
                return row

            def one_ulp_everywhere(row, b, k=k):
                row[k] = np.nextafter(row[k], np.inf)
                return row
            ulp.append(bool(np.any(run(one_ulp)[0] != base)))
            ulp_all.append(bool(np.any(run(one_ulp_everywhere)[0] != base)))
            neighbour.append(bool(np.any(run(from_next_lane)[0] != base)))
    finally:
        host.fold_items = fold
    print(f"{occupied} occupied bins, {ncoef} coefficients per row, 257 settings")
    print(f"one ulp in bin {middle}: {sum(ulp)} of {ncoef} show; silent:", [k for k in range(ncoef) if not ulp[k]])
    print(f"one ulp in every bin: {sum(ulp_all)} of {ncoef} show; silent:", [k for k in range(ncoef) if not ulp_all[k]])
    print(f"the neighbour's value in every bin: {sum(neighbour)} of {ncoef} show; silent:",
          [k for k in range(ncoef) if not neighbour[k]])


if __name__ == "__main__":
    if sys.argv[1] == "--coefficients":
        coefficients()
    else:
        main(sys.argv[1])
