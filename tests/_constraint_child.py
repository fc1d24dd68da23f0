"""Child process of tests/test_gpu_constraints.py: load a saved object and continue its experiment.

    python tests/_constraint_child.py <saved object> <result file>
"""
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(path, out):
    import optbayesexpt_amd as obe
    from test_gpu_constraints import _lorentz_cycles
    o = obe.load(path)
    log = _lorentz_cycles([o], 12, seed=3)
    with open(out, "wb") as f:
        pickle.dump(dict(log=log, bounds=o.parameter_bounds, w=o.particle_weights.copy(), p=o.particles.copy(),
                         count=o.last_constraint_count), f)


if __name__ == "__main__":
    main(*sys.argv[1:3])
