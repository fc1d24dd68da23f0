"""The sigma > 0 entry points (obe_mask_nonpositive, obe_mask_nonpositive_moments, obe_resample_particles_aos_masked
followed by obe_mask_renorm_moments) on fixed inputs: the cases, one runner, and the recorder of
tests/golden/constraint_parent_bits.json.

The fixture pins the bits these calls left when the library still had a sigma <= 0 kernel of its own beside the
parameter-bounds kernels.  It was written once, on an MI355X, by a build of the commit BEFORE the two were unified:

    PYTHONPATH=<a checkout of that commit, built> python -m _constraint_cases tests/golden/constraint_parent_bits.json

(run from this directory, or with it on the path).  test_gpu_constraints.py runs the same cases through run() on the
library under test and compares every item for equality.
"""
import ctypes
import hashlib
import json
import sys

import numpy as np

P = ctypes.c_void_p
INF = np.inf
SALT = (0.0, -0.0, 5e-324, -5e-324, np.nan, INF, -INF)
MASK_PARTIALS = 2 * 2048                 # 2 x kMaxBlocks doubles: {sum w, count} per workgroup of the first half

# (kind, d, n, masked rows[, scale]) — "mask": a cloud that violates now and then; "all": every particle violates (NaN
# weights, count = n); "none": nothing violates and the weights are not normalised (they must come back untouched);
# "gather": the masked gather of a resample, then the second half on its partial sums
CASES = ([("mask", d, n, rows) for d, n, rows in ((1, 1, [0]), (3, 255, [2]), (3, 256, [0, 2]), (4, 257, [3]),
                                                  (10, 4099, [8, 9]),
                                                  (17, 4099, [16]),          # beyond OBE_FAST_DIMS: the two-call route
                                                  (1, 2 ** 19 + 3, [0]))]    # beyond 2048 x 256: the grid-stride trip
         + [("all", 3, 257, [1]), ("none", 3, 5000, [0])]
         + [("gather", d, n, rows, scale) for d, n, rows in ((1, 257, [0]), (4, 4099, [3]), (10, 4099, [8, 9]),
                                                             (16, 256, [0, 15]), (2, 2 ** 19 + 3, [1]))
            for scale in (0, 1)])


def case_id(case):
    return " ".join(str(v).replace(" ", "") for v in case)


def inputs(case):
    """The arrays of one case, from a generator seeded by the case alone."""
    kind, d, n, rows = case[:4]
    g = np.random.default_rng([CASES.index(case), d, n])
    x = g.normal(0.3, 0.4, (d, n))
    mean = np.ascontiguousarray(x.mean(axis=1))             # (of the unsalted cloud: finite)
    if kind == "all":
        x[rows] = -1.0 - np.abs(x[rows])
    elif kind == "none":
        x[rows] = 1.0 + np.abs(x[rows])
    elif n >= 255:
        col = 1
        for r in rows:
            for v in SALT:
                x[r, col] = v
                col += 5
    w = g.random(n) * (g.random(n) > 0.1)                   # general values and zeros
    w[0] = 0.5
    if kind != "none":
        w /= w.sum()
    arrays = dict(x=x, w=w)
    if kind == "gather":
        arrays.update(idx=g.integers(0, n, n), z=g.standard_normal(n * d),
                      factor=np.ascontiguousarray(g.normal(0, 0.05, (d, d))), mean=mean)
    return arrays


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _hex(values):
    """Doubles as the 16 hex digits of their bits (a NaN keeps its sign and payload)."""
    return [f"{int(b):016x}" for b in np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)]


def run(lib, case):
    """One case through the entry points; everything the fixture holds about it."""
    import torch
    from optbayesexpt_amd import _lib

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def ptr(t):
        return P(t.data_ptr())

    kind, d, n, rows = case[:4]
    a = inputs(case)
    got = dict(inputs=_sha(*(a[k] for k in sorted(a))))
    rows32 = np.array(rows, dtype=np.int32)
    ws = torch.empty(lib.workspace_bytes(n, 1, 1, d) // 8 + 1, dtype=torch.float64, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)
    tail = (ptr(ws), ws.numel() * 8, st)
    first_len = _lib.MomentLayout(d).first_len

    def armed(name, x, *args):
        """A *_moments call: it arms the count and the first moments and does not wait; the wait is here."""
        mom = torch.zeros(lib.moments_len(d), dtype=torch.float64, device="cuda")
        h_mom, h_changed = _lib.pinned_array(first_len), _lib.pinned_array(1, np.int64)
        lib.call(name, ptr(x), n, d, n, *args, ptr(mom), _lib.host_ptr(h_mom), _lib.host_ptr(h_changed), *tail)
        lib.call("obe_host_words_wait", _lib.host_ptr(h_mom), first_len, st)
        lib.call("obe_host_word_wait", _lib.host_ptr(h_changed), st)
        return dict(count=int(h_changed[0]), moments_device=_hex(mom.cpu().numpy()[:first_len]),
                    moments_host=_hex(h_mom[:]))

    if kind != "gather":
        x = dev(a["x"])
        # obe_mask_nonpositive, its count into pageable and into page-locked memory
        for name, changed in (("sync_pageable", np.full(1, -1, dtype=np.int64)),
                              ("sync_pinned", _lib.pinned_array(1, np.int64))):
            w = dev(a["w"])
            lib.call("obe_mask_nonpositive", ptr(x), n, n, _lib.host_ptr(rows32), len(rows), ptr(w),
                     _lib.host_ptr(changed), *tail)
            got[name] = dict(count=int(changed[0]), weights=_sha(w.cpu().numpy()))
        w = dev(a["w"])
        got["moments"] = armed("obe_mask_nonpositive_moments", x, _lib.host_ptr(rows32), len(rows), ptr(w))
        got["moments"]["weights"] = _sha(w.cpu().numpy())
        if kind == "none":
            assert got["moments"]["weights"] == got["sync_pageable"]["weights"] == _sha(a["w"])
    else:
        aos, idx, z = dev(a["x"].T.copy()), dev(a["idx"]), dev(a["z"])
        new = torch.zeros((d, n), dtype=torch.float64, device="cuda")
        w = torch.zeros(n, dtype=torch.float64, device="cuda")
        partials = torch.zeros(MASK_PARTIALS, dtype=torch.float64, device="cuda")
        lib.call("obe_resample_particles_aos_masked", ptr(aos), d, n, ptr(idx), ptr(z), _lib.host_ptr(a["factor"]),
                 _lib.host_ptr(a["mean"]), 0.98, case[4], ptr(new), n, ptr(w), _lib.host_ptr(rows32), len(rows),
                 ptr(partials), st)
        got["gather"] = dict(cloud=_sha(new.cpu().numpy()), weights=_sha(w.cpu().numpy()),
                             partials=_sha(partials.cpu().numpy()))
        got["moments"] = armed("obe_mask_renorm_moments", new, ptr(partials), ptr(w))
        got["moments"]["weights"] = _sha(w.cpu().numpy())
    return got


def counts(got):
    return [v["count"] for v in got.values() if isinstance(v, dict) and "count" in v]


def check_condition(case, got):
    """Something is zeroed and something survives, wherever a case can have both (n = 1 cannot); the two extremes:
    everything, nothing."""
    kind, n = case[0], case[2]
    for count in counts(got):
        if kind in ("all", "none"):
            assert count == (n if kind == "all" else 0), (case, count)
        elif n > 1:
            assert 0 < count < n, (case, count)


def record(path):
    from optbayesexpt_amd import _lib
    lib = _lib.load()
    cases = {}
    for case in CASES:
        cases[case_id(case)] = got = run(lib, case)
        check_condition(case, got)
        print(case_id(case), counts(got), flush=True)
    with open(path, "w") as f:
        json.dump(dict(library=lib.cdll.obe_source_fingerprint().decode(), cases=cases), f, indent=1)
        f.write("\n")
    print("recorded by", lib.path)


if __name__ == "__main__":
    record(sys.argv[1])
