"""The records form of the keep buffer (include/obe_hip.h: obe_sweep_bins_keep_records_bytes) at the C entry point.
A call that is told the larger size keeps the particle part of every draw's record and sqrt(w) in the buffer, in sorted
order; a later call with OBE_SWEEP_BINS_KEPT renews sqrt(w) alone (csrc/obe_sweep_bins.h: bin_refresh_kernel) and
bin_moments_kernel<true> forms the packed records from those pieces.  The same expressions on the same operands:
every comparison is np.array_equal, against a rebuild and against the same calls with a buffer of the smaller size."""
import numpy as np
import pytest

from test_gpu_bin_sweep import D, _layouts, make, prior_cloud, weights
from test_gpu_bin_rebuild import D8, device_cloud, keep_buffer, keep_bytes, sweep_call

pytestmark = pytest.mark.gpu

SHAPES = [(63, 2), (257, 7), (193, 1031), (4099, 4099), (63, 131072), (63, 131073)]       # settings x draws
RECORDS_WORD = 9                 # of the head's 16 ints: the first pad word behind plan, mark, draws, d and mismatch
MARK = 0x6b455042
RESULTS = ("yvar", "utility", "best", "idx", "kappa")


@pytest.fixture(scope="module")
def obe(hip):
    import optbayesexpt_amd
    return optbayesexpt_amd


def flags():
    from optbayesexpt_amd import _lib
    return _lib.OBE_SWEEP_BINS, _lib.OBE_SWEEP_BINS | _lib.OBE_SWEEP_BINS_KEPT


def small_bytes(o, n):
    return int(o._mlib.cdll.obe_sweep_bins_keep_bytes(n))


def records_buffer(o, n):
    import torch
    nbytes = int(o._mlib.cdll.obe_sweep_bins_keep_records_bytes(n))
    assert nbytes % 16 == 0 and nbytes >= small_bytes(o, n) + 32 * n
    return torch.zeros(nbytes // 4, dtype=torch.int32, device=o._device)


def same(a, b, what):
    for k in RESULTS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def refused(r):
    return bool(np.isnan(r["kappa"])) and bool(np.all(np.isnan(r["yvar"])))


def grid(d, ns):
    return np.linspace(1.5, 4.5, ns) if d == D else np.linspace(2.0, 10.5, ns)


def check_rebuild(obe, ns, cloud, w, d, what, how=None):
    """A rebuild into a buffer of the records form against one into a buffer of the smaller size."""
    n = cloud.shape[1]
    o = make(obe, grid(d, ns), cloud, w, d=d)
    p, npart = device_cloud(o, how)
    small, large = keep_buffer(o, n), records_buffer(o, n)
    a = sweep_call(o, ns, particles=p, n_particles=npart, keep=small)
    b = sweep_call(o, ns, particles=p, n_particles=npart, keep=large)
    same(a, b, what)
    sa = keep_bytes(small).view(np.int32)
    sb = keep_bytes(large).view(np.int32)[:sa.size]
    differ = np.flatnonzero(sa != sb)
    assert list(differ) == [RECORDS_WORD] and sa[RECORDS_WORD] == 0 and sb[RECORDS_WORD] == MARK, (what, differ[:8])
    return o, a


@pytest.mark.parametrize("ns,n", SHAPES)
def test_rebuild_into_the_records_form(obe, ns, n):
    check_rebuild(obe, ns, prior_cloud(n, 7100 + n % 1000), weights(n, 7200 + n % 1000), D, (ns, n))


LAYOUTS = None


@pytest.mark.parametrize("layout", ["every particle in one bin", "every particle in a bin of its own",
                                    "two clusters, empty bins between", "x0 on bin edges", "exactly OBE_BIN_MAX bins",
                                    "zero-weight particles at the extremes", "ld_p beyond the particles"])
def test_rebuild_into_the_records_form_at_every_layout(obe, layout):
    global LAYOUTS
    if LAYOUTS is None:
        LAYOUTS = _layouts()
    if layout == "ld_p beyond the particles":
        cloud, w, d, how = prior_cloud(1031, 7001), weights(1031, 7002), D, "wide"
    else:
        cloud, w, d, fits = LAYOUTS[layout]
        assert fits
        how = None
        if w is None:
            w = weights(cloud.shape[1], 7003)
    o, first = check_rebuild(obe, 257, cloud, w, d, layout, how)
    assert np.all(np.isfinite(first["yvar"])), layout


def weight_vectors(kind, cloud, seed):
    """w2 and w3 of one kind (normalised)."""
    n = cloud.shape[1]
    g = np.random.default_rng(seed)
    lo, hi = int(np.argmin(cloud[0])), int(np.argmax(cloud[0]))
    out = []
    for k in range(2):
        w = g.exponential(1.0, n)
        if kind == "all but one zero":
            w[:] = 0.0
            w[(n // 3 + k) % n] = 1.0
        elif kind == "zeros at both extremes" and n > 2:
            w[[lo, hi]] = 0.0
        elif kind == "subnormal entries":
            w[::3] = 1e-310 * (1 + np.arange(w[::3].size) % 7)        # (subnormal after the division by the sum too)
            w[(1 + k) % n] = 1.0
        out.append(w / w.sum())
    if kind == "subnormal entries":
        assert np.any((out[0] > 0) & (out[0] < 2.3e-308))
    return out


@pytest.mark.parametrize("kind", ["random", "all but one zero", "zeros at both extremes", "subnormal entries"])
@pytest.mark.parametrize("ns,n", SHAPES)
def test_new_weights_on_kept_records(obe, ns, n, kind):
    """Rebuild with w1; then OBE_SWEEP_BINS_KEPT with w2 and with w3 (and their moments), in both buffer sizes: each
    the result of a rebuild with those weights, and the grouping bytes stay."""
    build, kept = flags()
    cloud, w1 = prior_cloud(n, 7300 + n % 1000), weights(n, 7400 + n % 1000)
    o = make(obe, grid(D, ns), cloud, w1)
    small, large = keep_buffer(o, n), records_buffer(o, n)
    sweep_call(o, ns, keep=small)
    sweep_call(o, ns, keep=large)
    head = small.numel()
    before_small, before_large = keep_bytes(small).copy(), keep_bytes(large)[:4 * head].copy()
    for w in weight_vectors(kind, cloud, 7500 + n % 1000):
        o.particle_weights = w                                 # (the particles stay; the moments are those of w)
        fresh = sweep_call(o, ns)                              # a rebuild without a buffer
        same(sweep_call(o, ns, keep=large, flags=kept), fresh, (ns, n, kind, "records"))
        same(sweep_call(o, ns, keep=small, flags=kept), fresh, (ns, n, kind, "grouping"))
        assert not np.isnan(fresh["kappa"]), (ns, n, kind)
        assert np.array_equal(keep_bytes(small), before_small), (ns, n, kind)
        assert np.array_equal(keep_bytes(large)[:4 * head], before_large), (ns, n, kind)


# ---------------------------------------------------------------------------------------------- head and marks
X = np.linspace(1.5, 4.5, 257)


def test_a_buffer_that_was_never_filled_is_refused(obe):
    _, kept = flags()
    o = make(obe, X, prior_cloud(4099, 7601), weights(4099, 7602))
    large = records_buffer(o, 4099)
    assert refused(sweep_call(o, X.size, keep=large, flags=kept))
    assert not bool(large.any())


def test_records_that_were_never_made_take_the_checking_path(obe):
    """A rebuild that was told the smaller size leaves no records behind the grouping: a reuse that is told the
    larger size checks every draw as before, and gives the rebuild's bits."""
    build, kept = flags()
    n = 4099
    cloud = prior_cloud(n, 7603)
    o = make(obe, X, cloud, weights(n, 7604))
    large = records_buffer(o, n)
    head = small_bytes(o, n) // 4
    sweep_call(o, X.size, keep=large[:head])
    assert keep_bytes(large).view(np.int32)[RECORDS_WORD] == 0 and not bool(large[head:].any())
    for seed in (7605, 7606):
        o.particle_weights = weights(n, seed)
        same(sweep_call(o, X.size, keep=large, flags=kept), sweep_call(o, X.size), seed)
    assert keep_bytes(large).view(np.int32)[RECORDS_WORD] == 0
    # (and a particle that left its bin is still found there)
    moved = cloud.copy()
    j = int(np.argsort(cloud[0])[n // 3])
    moved[0, j] += 3 * 0.5 * D
    b = make(obe, X, moved, weights(n, 7606))
    assert refused(sweep_call(b, X.size, keep=large, flags=kept))


def test_a_buffer_made_for_other_draws_or_another_width_is_refused(obe):
    build, kept = flags()
    few = make(obe, X, prior_cloud(513, 7607), weights(513, 7608))
    many = make(obe, X, prior_cloud(4099, 7609), weights(4099, 7610))
    large = records_buffer(many, 4099)
    assert np.isfinite(sweep_call(few, X.size, keep=large)["kappa"])
    same(sweep_call(few, X.size, keep=large, flags=kept), sweep_call(few, X.size), "the cloud it was made for")
    assert refused(sweep_call(many, X.size, keep=large, flags=kept))
    x8 = np.linspace(2.0, 10.5, 257)
    cloud = prior_cloud(513, 7611)
    a, b = make(obe, x8, cloud, weights(513, 7612), d=0.1), make(obe, x8, cloud, weights(513, 7612), d=D8)
    large = records_buffer(a, 513)
    assert np.isfinite(sweep_call(a, x8.size, keep=large)["kappa"])
    assert refused(sweep_call(b, x8.size, keep=large, flags=kept))


@pytest.mark.parametrize("how", ["129 bins", "a NaN x0"])
def test_a_poisoned_cloud_stays_poisoned(obe, how):
    build, kept = flags()
    if how == "129 bins":
        cloud, _, d, fits = _layouts()["one bin more than OBE_BIN_MAX"]
        assert not fits
        o = make(obe, grid(d, 257), cloud, weights(cloud.shape[1], 7613), d=d)
        p, npart = None, None
    else:
        o = make(obe, X, prior_cloud(1031, 7614), weights(1031, 7615))
        p, npart = device_cloud(o, "nan")
    large = records_buffer(o, o.n_particles)
    assert refused(sweep_call(o, 257, particles=p, n_particles=npart, keep=large))
    assert refused(sweep_call(o, 257, particles=p, n_particles=npart, keep=large, flags=kept))


def test_a_draws_mode_call_leaves_the_buffer_alone(obe):
    import torch
    o = make(obe, X, prior_cloud(5000, 7616), weights(5000, 7617))
    idx = torch.from_numpy(np.random.default_rng(7618).integers(0, 5000, 300)).to(o._device)
    large = records_buffer(o, 300)
    got = sweep_call(o, X.size, draw_idx=idx, keep=large)
    same(got, sweep_call(o, X.size, draw_idx=idx), "draws mode")
    assert not bool(large.any())


@pytest.mark.parametrize("reuse", [False, True], ids=["rebuild", "reuse"])
def test_an_aborted_speculative_call_leaves_a_complete_buffer_as_it_was(obe, reuse):
    import torch
    from optbayesexpt_amd import _lib
    build, kept = flags()
    n = 4099
    o = make(obe, X, prior_cloud(n, 7619), weights(n, 7620))
    large = records_buffer(o, n)
    sweep_call(o, X.size, keep=large)
    before = keep_bytes(large).copy()
    assert before.view(np.int32)[RECORDS_WORD] == MARK
    o.particle_weights = weights(n, 7621)
    word = o._ws.view(torch.int32)[-2:-1]                      # OBE_WS_ABORT_WORD of the object's workspace
    word.fill_(1)
    try:
        sweep_call(o, X.size, keep=large, flags=(kept if reuse else build) | _lib.OBE_SWEEP_SPECULATIVE)
    finally:
        word.fill_(0)
    assert np.array_equal(keep_bytes(large), before)
    # (the buffer still serves: the new weights on the kept records)
    same(sweep_call(o, X.size, keep=large, flags=kept), sweep_call(o, X.size), "after the aborted call")
