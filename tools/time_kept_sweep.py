"""The whole obe_sweep_utility_keep call on a prior cloud, rebuilding into the keep buffer and reusing it (developer
aid; the table of profiles/kept_bins.txt, profiles/bin_waves.txt and profiles/keep_records.txt).  Every call starts on a
drained stream and ends with the wait for its result; host clock, median of CALLS calls, three rounds in one process,
microseconds.  Two clouds per shape: the prior (uniform x0: 41 bins), and the prior after one measurement and one
resample, as a cycle's rebuild finds it.  The keep buffer has the records form where the library knows it
(obe_sweep_bins_keep_records_bytes), so the same file times a checkout from before it.

    python tools/time_kept_sweep.py [NSxN ...]          # default: the four shapes of the profiles

OBE_VARIANT=name times tools/_variants/libobe_hip_name.so (tools/build_variant.py) instead of the product library.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                            # noqa: E402
import optbayesexpt_amd as obe                          # noqa: E402
from optbayesexpt_amd import _lib                       # noqa: E402
from optbayesexpt_amd.particlepdf import _ptr, _P       # noqa: E402

if os.environ.get("OBE_VARIANT"):      # a library built by tools/build_variant.py instead of the product one
    _lib._LIB = _lib.HipLib(os.path.join(ROOT, "tools", "_variants", f"libobe_hip_{os.environ['OBE_VARIANT']}.so"),
                            allow_variant=True)

CALLS = 200
SHAPES = [(64, 64), (4096, 262144), (65536, 262144), (65536, 1048576)]
if os.environ.get("OBE_KEPT_SWEEP_CALLS"):
    CALLS = int(os.environ["OBE_KEPT_SWEEP_CALLS"])


def caller(ns, n, resampled=False):
    g = np.random.default_rng(5)
    cloud = np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    o = obe.OptBayesExpt(obe.models.lorentzian(1), (np.linspace(1.5, 4.5, ns),), cloud, (0.1,),
                         utility_method="variance_full", auto_resample=False, default_noise_std=500.0)
    if resampled:
        o.rng = np.random.default_rng(6)
        o.pdf_update(((3.0,), 49500.0, 500.0))
        o.resample()
    p, w = o._pw_tensors()
    mom = o._moments_on_device()
    dev = w.device
    noise = torch.full((1,), 250000.0, dtype=torch.float64, device=dev)
    yvar = torch.zeros((1, ns), dtype=torch.float64, device=dev)
    util = torch.zeros(ns, dtype=torch.float64, device=dev)
    out = _lib.pinned_array(4)
    best, idx, kappa = out[0:1], out.view(np.int64)[1:2], out[2:3]
    size = getattr(o._mlib.cdll, "obe_sweep_bins_keep_records_bytes", o._mlib.cdll.obe_sweep_bins_keep_bytes)
    keep = torch.zeros(int(size(n)) // 4, dtype=torch.int32, device=dev)
    hp = _lib.host_ptr

    def call(flags):
        rc = o._mlib.cdll.obe_sweep_utility_keep(o._model_struct, _P(o._settings_dev.data_ptr()), ns, ns, _ptr(p),
                                                 p.shape[1], n, _ptr(w), None, 0, _ptr(mom), flags, _ptr(noise), 0,
                                                 None, 1.0, _ptr(yvar), _ptr(util), hp(best), hp(idx), hp(kappa),
                                                 _ptr(o._ws), o._ws_bytes, o._stream(), _ptr(keep), keep.numel() * 4)
        torch.cuda.synchronize()
        assert rc == 0 and np.isfinite(kappa[0]), (rc, kappa[0])
    return o, call


def median_us(call, flags):
    times = []
    for _ in range(CALLS):
        t = time.perf_counter()
        call(flags)
        times.append(1e6 * (time.perf_counter() - t))
    return float(np.median(times))


def main(shapes):
    print(f"{'shape':>20}  rebuild {'':>22}|   reuse      (waves per group of settings)")
    for ns, n in shapes:
        for resampled in (False, True):
            o, call = caller(ns, n, resampled)
            for _ in range(20):
                call(_lib.OBE_SWEEP_BINS)
            rebuild = [median_us(call, _lib.OBE_SWEEP_BINS) for _ in range(3)]
            reuse = [median_us(call, _lib.OBE_SWEEP_BINS | _lib.OBE_SWEEP_BINS_KEPT) for _ in range(3)]
            waves = getattr(o._mlib.cdll, "obe_sweep_bins_eval_waves", lambda n_settings: 1)(ns)
            print(f"{ns:>8} x {n:>9}  " + " ".join(f"{t:8.2f}" for t in rebuild) + "   |  "
                  + " ".join(f"{t:8.2f}" for t in reuse) + f"      ({waves})"
                  + ("  resampled" if resampled else "  prior"), flush=True)


if __name__ == "__main__":
    main([tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]] or SHAPES)
