"""The records x particles pass of every class at one shape: obe_records_loglik (Gaussian, a sigma per record) and the
three own-noise passes (obe_signal_noise_records_loglik, obe_binomial_records_loglik, obe_poisson_records_loglik) for
262 144 particles x 4 096 records of the one-peak Lorentzian, on the same box in one process.

    python tools/time_records_loglik.py [--particles N] [--records R] [--out FILE]

Each entry point is called directly on device buffers made beforehand, once to warm up and then ``--repeats`` times
between obe_timer_start and obe_timer_stop (device events on the launch stream); the smallest time is kept.  The pass
packs its table, runs records x particles evaluations and folds the chunk partials: all three launches are inside the
timed interval.  "ratio" is the class's time over the Gaussian pass's."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import optbayesexpt_amd as obe  # noqa: E402
from optbayesexpt_amd import _lib  # noqa: E402

WIDTH = 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1 << 18)
    ap.add_argument("--records", type=int, default=1 << 12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_records_loglik.py measures on the GPU: none is visible")
    n_p, n_r = args.particles, args.records
    g = np.random.default_rng(19)
    lib = _lib.load()
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)      # noqa: E731
    x = np.sort(g.uniform(2.0, 4.0, n_r))[None, :]
    grid = (np.linspace(2.0, 4.0, 33),)
    # one cloud for all: x0, a, b with b + a / (...) in [0.1, 0.9] — a probability, a rate and a signal alike
    cloud = np.array([g.uniform(2.6, 3.4, n_p), g.uniform(0.3, 0.6, n_p), g.uniform(0.1, 0.3, n_p)])
    truth = 0.2 + 0.45 / (((x - 3.1) / WIDTH) ** 2 + 1)
    shots = np.full((1, n_r), 20.0)
    exposure = np.full((1, n_r), 10.0)
    coef = np.array([[1e-4, 1e-2, 0.0]])
    model = obe.models.lorentzian(1)
    base = obe.OptBayesExpt(model, grid, cloud, (WIDTH,), scale=False)
    p = base._parameters.tensor()
    d_x = up(x)
    out = torch.empty(n_p, dtype=torch.float64, device=dev)
    timer = ctypes.c_void_p()
    lib.call("obe_timer_create", ctypes.byref(timer))
    stream = base._stream()

    def run(entry, *middle):
        nbytes = int(getattr(lib.cdll, entry + "_workspace_bytes")(n_p, n_r, 1))
        ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)

        def call():
            base._mlib.call(entry, base._model_struct, d_x.data_ptr(), n_r, n_r, *middle, p.data_ptr(), n_p, n_p, 0,
                            out.data_ptr(), ws.data_ptr(), nbytes, stream)
        call()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(args.repeats):
            ms = ctypes.c_float(0.0)
            lib.call("obe_timer_start", timer, stream)
            call()
            lib.call("obe_timer_stop", timer, stream, ctypes.byref(ms))
            best = min(best, ms.value)
        assert bool(torch.isfinite(out).all()), entry
        return best

    d_y = up(truth + 0.05 * g.standard_normal((1, n_r)))
    d_sigma = up(np.full((1, n_r), 0.05))
    d_k = up(g.binomial(20, truth).astype(np.float64))
    d_n = up(shots)
    d_c = up(g.poisson(10.0 * truth).astype(np.float64))
    d_t = up(exposure)
    times = [
        ("obe_records_loglik", run("obe_records_loglik", d_y.data_ptr(), n_r, d_sigma.data_ptr(), n_r, None)),
        ("obe_signal_noise_records_loglik", run("obe_signal_noise_records_loglik", d_y.data_ptr(), n_r,
                                                _lib.host_ptr(coef), 0.0)),
        ("obe_binomial_records_loglik", run("obe_binomial_records_loglik", d_k.data_ptr(), n_r, d_n.data_ptr(), n_r, 0.0)),
        ("obe_poisson_records_loglik", run("obe_poisson_records_loglik", d_c.data_ptr(), n_r, d_t.data_ptr(), n_r, 0.0)),
    ]
    lib.call("obe_timer_destroy", timer)
    gauss = times[0][1]
    lines = [f"# tools/time_records_loglik.py on {torch.cuda.get_device_name(0)}: {n_p} particles x {n_r} records, one-peak "
             f"Lorentzian, the smallest of {args.repeats} timed calls after one warming call",
             "# entry point                               ms     evals/s     ratio to the Gaussian pass"]
    for name, ms in times:
        lines.append(f"{name:40s} {ms:8.3f}  {n_p * n_r / (ms * 1e-3):10.3e}  {ms / gauss:6.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
