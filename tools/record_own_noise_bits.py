#!/usr/bin/env python3
"""Record the fixture of tests/test_gpu_own_noise_bits.py: every output of that file's seeded cases from the library as
built, on the GPU.  Run it on the commit whose bits are to be pinned, BEFORE the kernels change:

    python tools/record_own_noise_bits.py tests/golden/own_noise_parent_bits.npz

and name that commit in the test file's docstring.  Every case is run twice; the two results must be the same bits.  A
case that the test compares with a part of another case's record (fewer settings, fewer particles, a slice) is not
stored: it must give that part here.  ``--plugins`` only builds the formula models' plugins (no GPU needed)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(path):
    import test_gpu_own_noise_bits as t
    if path == "--plugins":
        print("\n".join(m.plugin_path for m in t.plugin_models()))
        return
    out = {}
    for name in t.cases():
        got, again = t.run(name), t.run(name)
        assert sorted(got) == sorted(again) and all(t._same(got[k], again[k]) for k in got), f"{name}: run to run"
        want = t.expected(name, out)
        if want:                                                   # a part of a case recorded before
            assert sorted(got) == sorted(want) and all(t._same(got[k], want[k]) for k in got), f"{name}: not that part"
            print(f"{name}: as recorded")
            continue
        for k, v in got.items():
            out[f"{name}:{k}"] = np.ascontiguousarray(v, dtype=np.float64)
        print(f"{name}: " + ", ".join(f"{k} {v.shape} {np.count_nonzero(np.isnan(v))} NaN" for k, v in got.items()))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", sum(v.size for v in out.values()), "values")


if __name__ == "__main__":
    main(sys.argv[1])
