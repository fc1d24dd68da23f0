"""Posterior predictive summaries (predict, predictive_interval) on the device against the routes that gave the same
numbers before them, at the c3 cloud (1 048 576 x 3, Lorentzian) and the c5 cloud (524 288 x 10, seven peaks) with
1 024 settings, and at demo size (5 000 particles x 201 settings).

    python tools/time_predictive.py [--out profiles/predictive.txt]

Every route is a whole call as a user makes it, between two device events after two warming calls, repeated for at
least 0.3 s (host route: a host clock around single runs); the routes of one size alternate in one process, twice, and the smaller
time of each is kept.  Routes:
  predict                       obe_predictive_moments (two fused passes over the cloud)
  eval + torch reductions       per setting: eval_over_all_parameters on the device, then (w y).sum() / w.sum() and
                                the centred second moment with torch
  predictive_interval(0.95)     obe_predictive_quantiles (per tile of 64 rows: one launch for the model values, then
                                the radix select on them)
  eval + obe_weighted_quantiles the same composed from the entry points there were before: per setting
                                obe_eval_over_particles into a (64, N_p) buffer, then obe_weighted_quantiles on that
                                buffer as a cloud, tile by tile
  host (16 settings, x 64)      the cloud copied to the host once, the model and np.average / np.quantile per setting,
                                on 16 settings; the figure is that time scaled to the full number of settings
"evals/s" is settings x particles x passes over the cloud (2 for the moments, 8 select passes for the interval, 1 for
the composed routes' evaluation) over the device time."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import optbayesexpt_amd as obe  # noqa: E402
from optbayesexpt_amd import _lib, _posterior  # noqa: E402
from optbayesexpt_amd.particlepdf import _ptr  # noqa: E402

TILE = 64          # settings whose rows the composed quantile route keeps at a time: 64 x N_p doubles


def build(cfg, n_settings, g):
    """The object of a bench.py config after three updates without a resample, and n_settings points."""
    if cfg == "demo":
        n = 5000
        prior = np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
        o = obe.OptBayesExpt(obe.models.lorentzian(1), (np.linspace(1.5, 4.5, 201),), prior, (0.1,), scale=False)
        true, sigma, cons = (3.0, -1000.0, 50000.0), 500.0, (0.1,)
    else:
        settings, prior, cons, true, sigma = bench.make_workload(cfg)
        o = bench.build_obe(cfg, None, (settings[0][::64],), prior, cons)
    o.rng = np.random.default_rng(5)
    o.tuning_parameters["auto_resample"] = False
    sim = np.random.default_rng(9)
    for _ in range(3):
        x = o.opt_setting()
        y = float(o.model_function(x, true, cons)) + sigma * sim.standard_normal()
        o.pdf_update((x, y, sigma) if type(o) is obe.OptBayesExpt else (x, y))
    return o, (np.linspace(1.5, 4.5, n_settings),), cons


def timed(call, clock, min_seconds=0.3, warm=2, min_reps=2):
    for _ in range(warm):
        call()
    reps, total = 0, 0.0
    while total < min_seconds * 1e3 or reps < min_reps:
        total += clock(call)
        reps += 1
    return total / reps


def device_clock(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def host_clock(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def composed_moments(o, x):
    w = o._weights.tensor()
    sw = w.sum()
    mean = torch.empty((o.n_channels, x[0].size), dtype=torch.float64, device=w.device)
    var = torch.empty_like(mean)
    for s, xs in enumerate(x[0]):
        y = o._eval_over_all_parameters_device((xs,))
        m = (y * w).sum(dim=1) / sw
        mean[:, s] = m
        var[:, s] = ((y - m[:, None]) ** 2 * w).sum(dim=1) / sw
    return mean.cpu().numpy(), torch.sqrt(var).cpu().numpy()


def composed_interval(o, x, level=0.95):
    par, w = o._parameters.tensor(), o._weights.tensor()
    n_p = par.shape[1]
    qs = np.ascontiguousarray(_posterior.interval_quantiles(level), dtype=np.float64)
    buf = torch.empty((TILE, n_p), dtype=torch.float64, device=w.device)
    out = np.empty((x[0].size, 2))
    st = np.zeros(_lib.OBE_MAX_SETDIMS)
    for start in range(0, x[0].size, TILE):
        part = x[0][start:start + TILE]
        for r, xs in enumerate(part):
            st[0] = xs
            o._mlib.call("obe_eval_over_particles", o._model_struct, _ptr(par), n_p, n_p, _lib.host_ptr(st),
                         _lib.c_void_p(buf.data_ptr() + 8 * r * n_p), n_p, o._stream())
        rows = np.arange(part.size, dtype=np.int32)
        d_out = torch.empty((part.size, 2), dtype=torch.float64, device=w.device)
        nbytes = int(o._lib.cdll.obe_posterior_workspace_bytes(n_p, part.size, 0, 2))
        ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=w.device)
        o._lib.call("obe_weighted_quantiles", _ptr(buf), n_p, part.size, n_p, _ptr(w), _lib.host_ptr(rows), part.size,
                    _lib.host_ptr(qs), 2, _ptr(d_out), _ptr(ws), nbytes, o._stream())
        out[start:start + part.size] = d_out.cpu().numpy()
    return out[:, 0], out[:, 1]


def host_route(o, x, cons, n=16):
    o._particles._host_valid = o._weights._host_valid = False       # as behind a device-side update: one copy
    p, w = np.array(o.particles), np.array(o.particle_weights)
    out = []
    for xs in x[0][:: max(1, x[0].size // n)][:n]:
        y = np.asarray(o.model_function((xs,), p, cons), dtype=np.float64)
        m = np.average(y, weights=w)
        out.append((m, np.sqrt(np.average((y - m) ** 2, weights=w)),
                    np.quantile(y, (0.025, 0.975), weights=w, method="inverted_cdf")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictive.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_predictive.py measures on the GPU: none is visible")
    g = np.random.default_rng(5)
    lines = [f"# tools/time_predictive.py on {torch.cuda.get_device_name(0)}: whole calls, device events, warmed, the "
             "routes of a size in turn",
             "# size                           route                                     ms       evals/s   agrees"]
    for name, cfg, n_s in (("c3 1048576 x 3, 1024 settings", "c3", 1024), ("c5 524288 x 10, 1024 settings", "c5", 1024),
                           ("demo 5000 x 3, 201 settings", "demo", 201)):
        o, x, cons = build(cfg, n_s, g)
        n_p = o.n_particles
        want_m, want_s = o.predict(x)
        want_lo, want_hi = o.predictive_interval(0.95, x)
        got_m, got_s = composed_moments(o, x)
        got_lo, got_hi = composed_interval(o, x)
        agree_mom = f"{np.max(np.abs(got_m - want_m) / np.abs(want_m)):.1e} / {np.max(np.abs(got_s - want_s) / want_s):.1e}"
        agree_q = "equal" if np.array_equal(got_lo, want_lo[0]) and np.array_equal(got_hi, want_hi[0]) else "DIFFERENT"
        host_factor = n_s / min(16, n_s)
        routes = [("predict", lambda: o.predict(x), device_clock, 2, "-"),
                  ("eval + torch reductions", lambda: composed_moments(o, x), device_clock, 2, agree_mom),
                  ("predictive_interval(0.95)", lambda: o.predictive_interval(0.95, x), device_clock, 8, "-"),
                  ("eval + obe_weighted_quantiles", lambda: composed_interval(o, x), device_clock, 1, agree_q),
                  (f"host (16 settings, x {host_factor:.4g})", lambda: host_route(o, x, cons), host_clock, 0, "-")]
        best = {}
        for _ in range(2):
            for what, call, clock, passes, agrees in routes:
                ms = timed(call, clock) if clock is device_clock else timed(call, clock, 0.0, 0, 1)
                best[what] = min(best.get(what, np.inf), ms)
        for what, call, clock, passes, agrees in routes:
            ms = best[what] * (host_factor if clock is host_clock else 1.0)
            rate = f"{n_s * n_p * passes / (ms * 1e-3):.3g}" if passes else "-"
            lines.append(f"{name:30s}  {what:36s}  {ms:9.3f}  {rate:>10s}   {agrees}")
            print(lines[-1], flush=True)
        del o
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
