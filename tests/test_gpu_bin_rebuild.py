"""The rebuild of the bin grouping in four launches (csrc/obe_sweep_bins.h: bin_minmax_kernel, bin_group_kernel<false>
with the plan, bin_scan_kernel, bin_group_kernel<true> as the scatter-pack; no sweep_pack_kernel) against the bits of
the six launches behind a pack that it replaces: tests/golden/bin_chain_parent_bits.npz, recorded on one MI355X with
tools/record_bin_chain_bits.py (which imports the cases from this file and from test_gpu_bin_eval_finalize.py) from the
build of commit 8ec9fbb, "Test the Bayes update bit for bit at every entry point and grid class".

Every case is one call of obe_sweep_utility_keep with a zeroed keep buffer (full mode) or of obe_sweep_utility
(without one; draws mode) on N_SETTINGS settings.  Compared with np.array_equal: yvar, utility, the best value, its
index and kappa; as bytes: the whole keep buffer - head (plan, mark, draws, d), binstart, itemstart and dest[p] of
every draw.  Of the two clouds of more than 100 000 draws the fixture holds the buffer's first 4 096 bytes and the
SHA-256 of all of it, and that is what is compared: two files of 524 KB of positions do not belong in the repository.
A poisoned cloud (129 bins, a NaN x0) gives NaN and kappa = NaN in both trees, and its buffer is compared all the same.

The draw counts are those at which the units change: 1, 63 and 65 draws (tail lanes of one wavefront, a second trip),
4 097 (65 units of 64), 131 072 (2 048 units of 64: the cap) and 131 073 (128 draws per unit, the last unit partial).
A reuse of the buffer right after each rebuild gives the rebuild's bits and leaves the buffer as it was."""
import hashlib
import os

import numpy as np
import pytest

from test_gpu_bin_sweep import make, prior_cloud, weights

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bin_chain_parent_bits.npz")
N_SETTINGS = 193
D8 = 0.125                       # x0 / d and every bin edge are exact
N = 1031                         # draws of a layout cloud
COUNTS = (1, 63, 65, 4097, 131072, 131073)
WHOLE_BUFFER_BELOW = 100000      # draws from which the fixture holds a digest of the keep buffer
HEAD_BYTES = 4096


def sweep_call(o, n_settings, s_begin=0, particles=None, n_particles=None, w=None, draw_idx=None, flags=None,
               keep=None, noise=("scalar", 250000.0), cost=None, ws_bytes=None, refused=False):
    """One obe_sweep_utility[_keep] call on settings [s_begin, s_begin + n_settings) of the object, with its moments:
    {yvar, utility, best, idx, kappa}.  particles: a (3, ld_p) device tensor in place of the object's cloud;
    noise: ("scalar", v), ("rows", array of n_settings) or ("moments", row); cost: None (1.0) or an array.
    ws_bytes: the size the call is TOLD the object's workspace has (the buffer itself is what it is); refused: the call
    must fail, and its error text is returned."""
    import torch
    from optbayesexpt_amd import _lib
    from optbayesexpt_amd.particlepdf import _ptr, _P
    p0, w0 = o._pw_tensors()
    p = p0 if particles is None else particles
    w = w0 if w is None else w
    n_particles = o.n_particles if n_particles is None else n_particles
    mom = o._moments_on_device()
    dev = w0.device
    f64 = dict(dtype=torch.float64, device=dev)
    if noise[0] == "scalar":
        noise_t, noise_ld = torch.full((o.n_channels,), noise[1], **f64), 0
    elif noise[0] == "rows":
        noise_t, noise_ld = torch.from_numpy(np.ascontiguousarray(noise[1])).to(dev), n_settings
    else:
        noise_t, noise_ld = mom, -(int(noise[1]) + 1)
    cost_t = None if cost is None else torch.from_numpy(np.ascontiguousarray(cost)).to(dev)
    yvar = torch.zeros((o.n_channels, n_settings), **f64)
    util = torch.zeros(n_settings, **f64)
    out = _lib.pinned_array(4)
    best, idx, kappa = out[0:1], out.view(np.int64)[1:2], out[2:3]
    hp = _lib.host_ptr
    flags = _lib.OBE_SWEEP_BINS if flags is None else flags
    head = (o._model_struct, _P(o._settings_dev.data_ptr() + 8 * s_begin), o._n_settings, n_settings, _ptr(p), p.shape[1],
            n_particles, _ptr(w), None if draw_idx is None else _ptr(draw_idx),
            0 if draw_idx is None else draw_idx.numel(), _ptr(mom), flags, _ptr(noise_t), noise_ld,
            None if cost_t is None else _ptr(cost_t), 1.0, _ptr(yvar), _ptr(util), hp(best), hp(idx), hp(kappa),
            _ptr(o._ws), o._ws_bytes if ws_bytes is None else ws_bytes, o._stream())
    if keep is None:
        rc = o._mlib.cdll.obe_sweep_utility(*head)
    else:
        rc = o._mlib.cdll.obe_sweep_utility_keep(*head, _ptr(keep), keep.numel() * 4)
    torch.cuda.synchronize()
    if refused:
        assert rc != 0, "the call was accepted"
        return o._mlib.last_error()
    assert rc == 0, o._mlib.last_error()
    yvar = yvar.cpu().numpy()
    return {"yvar": yvar[0] if o.n_channels == 1 else yvar, "utility": util.cpu().numpy(), "best": np.array(float(best[0])),
            "idx": np.array(int(idx[0])), "kappa": np.array(float(kappa[0]))}


def keep_buffer(o, n_draws):
    import torch
    nbytes = int(o._mlib.cdll.obe_sweep_bins_keep_bytes(n_draws))
    return torch.zeros(nbytes // 4, dtype=torch.int32, device=o._device)


def keep_bytes(keep):
    return keep.cpu().numpy().view(np.uint8)


def keep_record(raw, n_draws):
    """What the fixture holds of a keep buffer."""
    if n_draws < WHOLE_BUFFER_BELOW:
        return {"keep": raw.copy()}
    return {"keep_head": raw[:HEAD_BYTES].copy(),
            "keep_sha256": np.frombuffer(hashlib.sha256(raw.tobytes()).digest(), dtype=np.uint8).copy()}


def _cloud(g, x0):
    n = x0.size
    return np.array([x0, g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])


def clouds():
    """name -> (cloud, weights, d, x grid, what to do to the device copy, poisoned)"""
    g = np.random.default_rng(9101)
    x10, x8 = np.linspace(1.5, 4.5, N_SETTINGS), np.linspace(2.0, 10.5, N_SETTINGS)
    out = {}
    for n in COUNTS:
        out[f"{n} draws"] = (prior_cloud(n, 9200 + n % 1000), weights(n, 9300 + n % 1000), 0.1, x10, None, False)
    out["all x0 equal"] = (_cloud(g, np.full(N, 3.0)), weights(N, 9102), 0.1, x10, None, False)
    out["x0 on bin edges"] = (_cloud(g, D8 * (16.0 + 0.5 * g.integers(0, 17, N))), weights(N, 9103), D8, x8, None, False)
    span = np.append(g.uniform(0.0, 127.0, N - 2), [0.0, 128.0 - 2.0 ** -20])      # (exact in x0 and in x0 / d)
    out["128 bins"] = (_cloud(g, D8 * (20.0 + 0.5 * span)), weights(N, 9104), D8, x8, None, False)
    span = np.append(g.uniform(0.0, 127.0, N - 2), [0.0, 128.0])
    out["129 bins"] = (_cloud(g, D8 * (20.0 + 0.5 * span)), weights(N, 9105), D8, x8, None, True)
    out["one NaN x0"] = (prior_cloud(N, 9106), weights(N, 9107), 0.1, x10, "nan", True)
    w = weights(N, 9108)
    cloud = _cloud(g, np.concatenate([[0.5], g.uniform(2, 4, N - 2), [5.5]]))
    w[[0, 5, 64, 500, N - 1]] = 0.0
    out["draws of weight 0"] = (cloud, w / w.sum(), 0.1, x10, None, False)
    out["ld_p beyond the particles"] = (prior_cloud(N, 9109), weights(N, 9110), 0.1, x10, "wide", False)
    return out


def device_cloud(o, how):
    """(particles tensor or None, n_particles): the object's cloud, with particle 7's x0 NaN, or in rows 37 doubles
    longer than the cloud whose tail is NaN."""
    import torch
    if how is None:
        return None, None
    p, _ = o._pw_tensors()
    n = o.n_particles
    if how == "nan":
        q = p.clone()
        q[0, 7] = float("nan")
        return q, n
    q = torch.full((p.shape[0], n + 37), float("nan"), dtype=torch.float64, device=p.device)
    q[:, :n] = p[:, :n]
    return q, n


def run_cloud(obe, case):
    """{key: array} of one cloud: a rebuild into a keep buffer, a reuse of it, and the call without a buffer."""
    from optbayesexpt_amd import _lib
    cloud, w, d, x, how, poisoned = case
    n = cloud.shape[1]
    o = make(obe, x, cloud, w, d=d)
    p, npart = device_cloud(o, how)
    keep = keep_buffer(o, n)
    out = {}
    first = sweep_call(o, N_SETTINGS, particles=p, n_particles=npart, keep=keep)
    raw = keep_bytes(keep)
    again = sweep_call(o, N_SETTINGS, particles=p, n_particles=npart, keep=keep,
                       flags=_lib.OBE_SWEEP_BINS | _lib.OBE_SWEEP_BINS_KEPT)
    plain = sweep_call(o, N_SETTINGS, particles=p, n_particles=npart)
    for k, v in first.items():
        out[f"rebuild | {k}"] = v
        out[f"reuse | {k}"] = again[k]
        out[f"no buffer | {k}"] = plain[k]
    for k, v in keep_record(raw, n).items():
        out[f"rebuild | {k}"] = v
    for k, v in keep_record(keep_bytes(keep), n).items():
        out[f"reuse | {k}"] = v
    assert bool(np.isnan(first["kappa"])) is poisoned, (n, d, first["kappa"])
    return out


DRAWS = {"300 draws": 300, "4097 draws": 4097}


def run_draws(obe, n_draws):
    """Draws mode above the one-workgroup size: repeated indices, and indices outside the cloud (clamped)."""
    import torch
    cloud, w = prior_cloud(5000, 9111), weights(5000, 9112)
    o = make(obe, np.linspace(1.5, 4.5, N_SETTINGS), cloud, w)
    idx = np.random.default_rng(9113 + n_draws).integers(0, 5000, n_draws)
    idx[1] = idx[0]
    idx[70] = idx[0]
    idx[[2, 64, n_draws - 1]] = [-3, 5000 + 7, 2 ** 40]
    got = sweep_call(o, N_SETTINGS, draw_idx=torch.from_numpy(idx).to(o._device))
    assert np.isfinite(got["kappa"])
    return {f"draws mode | {k}": v for k, v in got.items()}


def record(obe):
    """Everything the fixture holds of this file (tools/record_bin_chain_bits.py)."""
    out = {}
    for name, case in clouds().items():
        out.update({f"{name} | {k}": v for k, v in run_cloud(obe, case).items()})
    for name, n in DRAWS.items():
        out.update({f"{name} | {k}": v for k, v in run_draws(obe, n).items()})
    return out


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def obe(hip):
    import optbayesexpt_amd
    return optbayesexpt_amd


def same_bits(got, recorded, prefix):
    assert got, prefix
    for k, v in got.items():
        want = recorded[f"{prefix} | {k}"]
        assert v.shape == want.shape and v.dtype == want.dtype, (prefix, k, v.shape, want.shape)
        differ = np.flatnonzero(np.atleast_1d(v != want))
        assert np.array_equal(v, want, equal_nan=v.dtype.kind == "f"), (prefix, k, differ.size, differ[:8])


CLOUDS = None
NAMES = [f"{n} draws" for n in COUNTS] + ["all x0 equal", "x0 on bin edges", "128 bins", "129 bins", "one NaN x0",
                                          "draws of weight 0", "ld_p beyond the particles"]


@pytest.mark.parametrize("name", NAMES)
def test_rebuild_reuse_and_no_buffer_have_the_recorded_bits(obe, recorded, name):
    global CLOUDS
    if CLOUDS is None:
        CLOUDS = clouds()
        assert list(CLOUDS) == NAMES
    got = run_cloud(obe, CLOUDS[name])
    same_bits(got, recorded, name)
    # (what the fixture says of itself: a reuse and a call without a buffer are the rebuild)
    for k in ("yvar", "utility", "best", "idx", "kappa", "keep", "keep_sha256"):
        if f"rebuild | {k}" in got:
            assert np.array_equal(got[f"rebuild | {k}"], got[f"reuse | {k}"], equal_nan=True), (name, k)
            if not k.startswith("keep"):
                assert np.array_equal(got[f"rebuild | {k}"], got[f"no buffer | {k}"], equal_nan=True), (name, k)
    if CLOUDS[name][5]:
        assert np.all(np.isnan(got["rebuild | yvar"])) and np.all(np.isnan(got["no buffer | yvar"]))


@pytest.mark.parametrize("name", list(DRAWS))
def test_draws_mode_has_the_recorded_bits(obe, recorded, name):
    same_bits(run_draws(obe, DRAWS[name]), recorded, name)
