#!/usr/bin/env python3
"""Record the fixture of tests/test_gpu_bin_sweep_bits.py: yvar of that file's seeded bin sweeps from the library as
built, on the GPU.  Run it on the commit whose bits are to be pinned, BEFORE the kernels change:

    python tools/record_bin_sweep_bits.py tests/golden/bin_sweep_parent_bits.npz

and name that commit in the test file's docstring.  Every case is swept twice; the two results must be the same bits."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(path):
    import optbayesexpt_amd as obe
    import test_gpu_bin_sweep_bits as t
    out = {}
    for name, (x, cloud, w) in t.cases().items():
        out[name] = t.sweep(obe, x, cloud, w)
        assert np.array_equal(out[name], t.sweep(obe, x, cloud, w)), name
        assert np.all(np.isfinite(out[name])), name
        print(f"{name}: {out[name].size} values, max {out[name].max():.17g}")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
