"""Record tests/golden/sweep_layout_parent.json from the library of the tree this is run in (developer aid): the
reference of tests/test_sweep_layout_host.py and tests/test_gpu_sweep_workspace.py, which import their tables and cases
from here.  Run it in a checkout of the commit the tests name, with this file and the two test files copied in:

    python tools/record_sweep_layout.py            # "host": the sizes and plans, no GPU
    python tools/record_sweep_layout.py --gpu      # and "smallest_workspace": needs one MI355X

The second part keeps what the file already holds of the first, and the other way round."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "tests", "golden", "sweep_layout_parent.json")


def main():
    from optbayesexpt_amd import _lib
    import test_sweep_layout_host as host
    data = json.load(open(OUT)) if os.path.exists(OUT) else {}
    data["host"] = host.answers(_lib.load().cdll)
    if "--gpu" in sys.argv:
        import optbayesexpt_amd as obe
        import test_gpu_sweep_workspace as gpu
        data["smallest_workspace"] = {}
        for name, case in gpu.cases().items():
            data["smallest_workspace"][name] = got = gpu.smallest_accepted(gpu.Call(obe, case))
            print(f"{name:36s} {got['ws_bytes']:10d}  {got['error']}", flush=True)
    with open(OUT, "w") as f:
        json.dump(data, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print({k: len(v) for k, v in data["host"].items()}, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
