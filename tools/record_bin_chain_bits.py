#!/usr/bin/env python3
"""Record the fixture of tests/test_gpu_bin_rebuild.py and tests/test_gpu_bin_eval_finalize.py: the outputs and keep
buffers of those files' seeded calls from the library as built, on the GPU.  Run it on the commit whose bits are to be
pinned, BEFORE the kernels change:

    python tools/record_bin_chain_bits.py tests/golden/bin_chain_parent_bits.npz

and name that commit in the docstring of test_gpu_bin_rebuild.py.  Everything is run twice; the two results must be
the same bits.  OBE_VARIANT=name records from tools/_variants/libobe_hip_name.so (tools/build_variant.py) instead."""
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
    import test_gpu_bin_eval_finalize as fin
    import test_gpu_bin_rebuild as reb
    print("library:", _lib.load().path)

    def record():
        out = reb.record(obe)
        out.update(fin.record(obe))
        return out
    out, again = record(), record()
    assert out.keys() == again.keys()
    for name, v in out.items():
        assert np.array_equal(v, again[name], equal_nan=v.dtype.kind == "f"), name
    print(f"{len(out)} arrays, {sum(v.nbytes for v in out.values())} bytes")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
