"""The two kernels of the signal-dependent noise model (csrc/obe_signal_noise.hip) next to their yardsticks, on the
one-peak Lorentzian at 4 096 settings x 262 144 particles and 65 536 settings x 1 048 576 particles.

    python tools/signal_noise_timing.py [--out profiles/signal_noise.txt] [--small]

  obe_signal_noise_variance     one pass over settings x particles: nu_bar of every setting
  obe_predictive_moments        the yardstick: two passes of the same geometry on the same inputs (mean, then variance)
  obe_signal_noise_likelihood   the likelihood of one record from the cloud, followed by obe_bayes_update_lik
    + obe_bayes_update_lik
  obe_bayes_update_model        the yardstick: the fused update of a fixed-sigma record at the same N

Every figure is a library call (or the pair of them) between two device events on an otherwise idle card, after two
warming calls, repeated for at least 0.3 s; the routes of one size alternate, twice, and the smaller time of each is
kept.  "evals/s" is settings x particles x passes over the device time.  The updates run on a copy of the weights that is
refreshed outside the timed window, so that every repetition multiplies the same weights."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import optbayesexpt_amd as obe  # noqa: E402
from optbayesexpt_amd import _lib  # noqa: E402
from optbayesexpt_amd.particlepdf import _ptr  # noqa: E402

COEF = np.array([[4.0e4, 0.5, 1.0e-5]])          # {a, b, c} of nu(y) = a + b |y| + c y^2


def device_clock(call, before=None):
    if before is not None:
        before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(call, before=None, min_seconds=0.3, warm=2, min_reps=3):
    for _ in range(warm):
        device_clock(call, before)
    reps, total = 0, 0.0
    while total < min_seconds * 1e3 or reps < min_reps:
        total += device_clock(call, before)
        reps += 1
    return total / reps


def routes(n_s, n_p, g):
    dev = torch.device("cuda:0")
    prior = np.array([g.uniform(2, 4, n_p), g.uniform(-2000, -400, n_p), g.normal(50000, 300, n_p)])
    o = obe.OptBayesExptSignalNoise(obe.models.lorentzian(1), (np.linspace(1.5, 4.5, n_s),), prior, (0.1,), scale=False,
                                    noise_floor=200.0, noise_gain=0.5, noise_relative=np.sqrt(1.0e-5))
    w0 = g.random(n_p)
    o.particle_weights = w0 / w0.sum()
    lib, m, st = o._mlib, o._model_struct, o._stream()
    p, w, x = o._particles.tensor(), o._weights.tensor(), o._settings_dev
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    nubar, mean, var, lik, w_work = new(1, n_s), new(1, n_s), new(1, n_s), new(n_p), new(n_p)
    nu_bytes = int(lib.cdll.obe_signal_noise_workspace_bytes(n_p, n_s, 1))
    pm_bytes = int(lib.cdll.obe_predictive_workspace_bytes(n_p, n_s, 1, 0))
    nu_ws, pm_ws = new(nu_bytes // 8 + 1), new(pm_bytes // 8 + 1)
    setting, y_meas, sigma = np.zeros(_lib.OBE_MAX_SETDIMS), np.zeros(_lib.OBE_MAX_CHANNELS), np.ones(_lib.OBE_MAX_CHANNELS)
    setting[0], y_meas[0], sigma[0] = 3.1, 49500.0, 230.0
    host_out = _lib.pinned_array(16)
    hp = _lib.host_ptr

    def variance():
        lib.call("obe_signal_noise_variance", m, _ptr(x), n_s, n_s, _ptr(p), n_p, n_p, _ptr(w), hp(COEF), _ptr(nubar),
                 _ptr(nu_ws), nu_bytes, st)

    def moments():
        lib.call("obe_predictive_moments", m, _ptr(x), n_s, n_s, _ptr(p), n_p, n_p, _ptr(w), _ptr(mean), _ptr(var),
                 _ptr(pm_ws), pm_bytes, st)

    def refresh():
        w_work.copy_(w)

    def signal_update():
        lib.call("obe_signal_noise_likelihood", m, None, 0, _ptr(p), n_p, n_p, hp(setting), hp(y_meas), hp(COEF), 1,
                 float("nan"), _ptr(lik), st)
        o._lib.call("obe_bayes_update_lik", _ptr(lik), n_p, _ptr(w_work), _ptr(o._ws), o._ws_bytes, hp(host_out), st)

    def model_update():
        lib.call("obe_bayes_update_model", m, _ptr(p), n_p, n_p, _ptr(w_work), hp(setting), hp(y_meas), hp(sigma), None, 1,
                 float("nan"), _ptr(o._ws), o._ws_bytes, hp(host_out), st)

    return o, [("obe_signal_noise_variance", variance, None, 1), ("obe_predictive_moments", moments, None, 2),
               ("obe_signal_noise_likelihood + obe_bayes_update_lik", signal_update, refresh, 0),
               ("obe_bayes_update_model", model_update, refresh, 0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signal_noise.txt"))
    ap.add_argument("--small", action="store_true", help="the smaller size only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/signal_noise_timing.py measures on the GPU: none is visible")
    g = np.random.default_rng(5)
    lines = [f"# tools/signal_noise_timing.py on {torch.cuda.get_device_name(0)}: library calls, device events, warmed, "
             "the routes of a size in turn",
             "# settings x particles      route                                                      ms       evals/s"]
    sizes = [(4096, 262144)] + ([] if args.small else [(65536, 1048576)])
    for n_s, n_p in sizes:
        o, rs = routes(n_s, n_p, g)
        best = {}
        for _ in range(2):
            for what, call, before, passes in rs:
                best[what] = min(best.get(what, np.inf), timed(call, before))
        for what, call, before, passes in rs:
            ms = best[what]
            rate = f"{n_s * n_p * passes / (ms * 1e-3):.3g}" if passes else "-"
            lines.append(f"{n_s:6d} x {n_p:8d}         {what:52s}  {ms:9.3f}  {rate:>10s}")
            print(lines[-1], flush=True)
        del o
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
