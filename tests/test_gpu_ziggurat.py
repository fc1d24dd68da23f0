"""The device-side continuation of the NumPy stream (csrc/obe_rng.hip) where a random stream does not reach (GPU).

* obe_ziggurat_normal on crafted raw streams (tests/_ziggurat_oracle.py): draws of every length 1 .. 32, long
  draws across tile boundaries at every alignment, the deepest anchor search, ``offset`` > 0, buffers that are
  just long enough and just too short, and the deferred delivery of {consumed, found}.  Rectangle and wedge
  values are compared bit for bit, tail values to one ulp (libm's log1p on the host, ocml's on the device:
  rtol = 2.3e-16, as in test_device_rng_is_bitwise_numpy), ``consumed`` and the return code exactly.  Every
  stream comes from ``zo.case()``, which hands it out only after the contract of the device code (margins, draws
  <= 32 values, an anchor at least every 32 positions) has been asserted on it: nothing out of contract is fed.
* the retry paths of DeviceStream and of the pipelined resample on real PCG64 streams whose buffer is too short;
* the "segment full" branch of pcg_uniform_classify_kernel at the smallest size that takes it.
"""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _ziggurat_oracle as zo

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5            # what the output holds behind the n normals asked for
PAD = 16
TAIL_RTOL = 2.3e-16


@pytest.fixture(scope="module")
def obe(hip):
    import optbayesexpt_amd
    return optbayesexpt_amd


def _launch(hip, raw, offset, n, h_consumed):
    """obe_ziggurat_normal on a host array of raw values: (return code, device output of n + PAD values)."""
    import torch
    from optbayesexpt_amd import _devrng, _lib
    P = _lib.c_void_p
    dev = torch.device("cuda", 0)
    d_raw = torch.from_numpy(raw.view(np.int64)).to(dev)
    ws = torch.empty(int(hip.cdll.obe_ziggurat_workspace_bytes(raw.size)) // 8 + 1, dtype=torch.float64, device=dev)
    out = torch.full((n + PAD,), SENTINEL, dtype=torch.float64, device=dev)
    tables = _devrng._tables(dev)
    rc = hip.cdll.obe_ziggurat_normal(P(d_raw.data_ptr()), raw.size, offset, P(tables.data_ptr()), n, P(out.data_ptr()),
                                      _lib.host_ptr(h_consumed), P(ws.data_ptr()), ws.numel() * 8, None)
    return rc, out, (d_raw, ws)


def run_sync(hip, raw, offset, n):
    """(return code, *h_consumed, output)."""
    consumed = np.full(2, -99, dtype=np.int64)
    rc, out, _keep = _launch(hip, raw, offset, n, consumed)
    return rc, int(consumed[0]), out.cpu().numpy()


def run_deferred(hip, raw, offset, n):
    """The same call under obe_defer_host_sync(1) with a page-locked h_consumed[2]: ({consumed, found}, output) once
    the caller has synchronised."""
    import torch
    from optbayesexpt_amd import _lib
    pinned = _lib.pinned_array(2, np.int64)
    assert hip.cdll.obe_defer_host_sync(1) == 0
    try:
        rc, out, _keep = _launch(hip, raw, offset, n, pinned)
    finally:
        assert hip.cdll.obe_defer_host_sync(0) == 1
    assert rc == 0                                   # (nothing is checked inside a deferred call)
    torch.cuda.synchronize()
    return int(pinned[0]), int(pinned[1]), out.cpu().numpy()


def assert_normals(out, chain, n):
    """out[:n] are the first n normals of the oracle's chain, and nothing was written behind them."""
    vals, tail = chain[1][:n], chain[2][:n] == zo.TAIL
    assert vals.size == n
    assert_array_equal(out[:n][~tail], vals[~tail])
    assert_allclose(out[:n][tail], vals[tail], rtol=TAIL_RTOL, atol=0)
    assert_array_equal(out[n:], np.full(out.size - n, SENTINEL))


def check_accepted(hip, key, n):
    raw, tab, chain = zo.case(*key)
    first = key[3]
    rc, consumed, out = run_sync(hip, raw, first, n)
    print(f"{key} n={n}: rc={rc} consumed={consumed} oracle={int(chain[3][n - 1]) - first}")
    assert rc == 0
    assert consumed == int(chain[3][n - 1]) - first
    assert_normals(out, chain, n)


def check_refused(hip, key, n):
    raw, _, _ = zo.case(*key)
    rc, consumed, _ = run_sync(hip, raw, key[3], n)
    print(f"{key} n={n}: rc={rc} consumed={consumed}")
    assert rc == 1 and consumed == -1


# ------------------------------------------------------------------ crafted streams
@pytest.mark.parametrize("n_raw", zo.MIXED_SIZES)
@pytest.mark.parametrize("variant", range(zo.MIXED_VARIANTS))
def test_every_draw_length_and_tile_straddle(obe, hip, variant, n_raw):
    """The mixed stream (every draw length, long draws across the tile boundaries from a different alignment in
    every variant) cut after 2047, 2048, 2049 and 3 * 2048 + 5 values: all the normals that end at least 64
    values before the end, half of them, one of them; one more than all of them is refused."""
    key = ("mixed", variant, n_raw, 0)
    _, _, chain = zo.case(*key)
    n_all = zo.normals_within(chain, n_raw)
    assert n_all >= 100
    check_accepted(hip, key, n_all)
    check_accepted(hip, key, n_all // 2)
    check_accepted(hip, key, 1)
    check_refused(hip, key, n_all + 1)


@pytest.mark.parametrize("where", zo.OFFSET_NAMES)
def test_offset_inside_the_buffer(obe, hip, where):
    """``offset`` > 0: on a true start, inside a long draw (another parse: the oracle is chained from there),
    not a multiple of 8 (the staging of the lengths byte by byte), behind whole tiles, 65 before the end."""
    first = zo.mixed_offsets(0)[where]
    key = ("mixed", 0, zo.MIXED_N_RAW, first)
    _, _, chain = zo.case(*key)
    n_all = zo.normals_within(chain, zo.MIXED_N_RAW)
    assert n_all >= 1 and chain[0][0] == first
    check_accepted(hip, key, n_all)
    check_accepted(hip, key, 1)
    if n_all > 3:
        check_accepted(hip, key, n_all // 3)
    check_refused(hip, key, n_all + 1)


@pytest.mark.parametrize("first", [0, 5, zo.TILE + 3])
def test_buffer_just_long_enough_and_just_too_short(obe, hip, first):
    """Draws of one value each: n normals consume n values.  n = n_raw - offset - 64 is the most the buffer gives;
    one more, or more normals than there are values, is OBE_RNG_NEED_MORE with *h_consumed = -1."""
    key = ("ones", 7, zo.ONES_N_RAW, first)
    _, tab, _ = zo.case(*key)
    assert np.all(tab.len == 1)
    n = zo.ONES_N_RAW - first - zo.END_GUARD
    check_accepted(hip, key, n)
    check_refused(hip, key, n + 1)
    check_refused(hip, key, zo.ONES_N_RAW + 10)


def test_deferred_delivery_of_consumed_and_found(obe, hip):
    """{consumed, found} delivered by the compaction kernel itself: by the later of two workgroups (the n-th normal
    in the first tile of three), by the last workgroup alone (the n-th normal in its tile; fewer than n normals
    found), and an n-th normal that ends too close to the end.  obe_ziggurat_check on the delivered pair decides
    as the synchronous call did, and an accepted ``consumed`` is the oracle's."""
    key = ("mixed", 3, zo.DEFERRED_N_RAW, 0)
    raw, tab, chain = zo.case(*key)
    starts, ends = chain[0], chain[3]
    n_raw = zo.DEFERRED_N_RAW
    n_all = zo.normals_within(chain, n_raw)
    in_last_tile = int(np.searchsorted(starts, 2 * zo.TILE + 10)) + 1
    assert starts[in_last_tile - 1] >= 2 * zo.TILE and in_last_tile <= n_all and starts[50 - 1] < zo.TILE
    placements = {"first tile of three": (50, 0), "last tile": (in_last_tile, 0), "found < n": (starts.size + 50, 1),
                  "ends inside the last 64": (n_all + 1, 1)}
    for name, (n, want_rc) in placements.items():
        rc, sync_consumed, _ = run_sync(hip, raw, 0, n)
        consumed, found, out = run_deferred(hip, raw, 0, n)
        verdict = hip.cdll.obe_ziggurat_check(consumed, found, n, n_raw, 0)
        print(f"{name}: n={n} sync rc={rc} deferred consumed={consumed} found={found} check={verdict}")
        assert rc == want_rc and verdict == rc
        if name == "found < n":
            assert found < n
        else:
            assert found >= n
        if rc == 0:
            assert consumed == sync_consumed == int(ends[n - 1])
            assert_normals(out, chain, n)


# ------------------------------------------------------------------ retry paths, real PCG64 streams
RETRY_N_UNIFORM, RETRY_N_NORMAL = 4097, 350_005


def _assert_numpy_normals(z, zr):
    body = np.abs(zr) <= zo.ZIG_R
    assert_array_equal(z[body], zr[body])
    assert_allclose(z[~body], zr[~body], rtol=TAIL_RTOL, atol=0)


def _short_device_stream(hip, seed):
    import torch
    from optbayesexpt_amd import _devrng
    rng, ref = np.random.default_rng(seed), np.random.default_rng(seed)
    rng.random(7)
    ref.random(7)
    ds = _devrng.DeviceStream(hip, torch.device("cuda", 0), None, rng, RETRY_N_UNIFORM, RETRY_N_NORMAL)
    ds.margin = 64                    # ~2 % of 350 005 values are consumed extra: 64 cannot be enough
    ds._generate()
    assert ds.n_raw == RETRY_N_UNIFORM + RETRY_N_NORMAL + 64
    return rng, ref, ds


def test_device_stream_regenerates_a_buffer_that_was_too_short(obe, hip):
    """DeviceStream.normals() with a head-room of 64 raw values: the first attempt comes back too short (the
    margin has grown), the second delivers numpy's numbers and numpy's generator state."""
    rng, ref, ds = _short_device_stream(hip, 21)
    u_before = ds.uniforms().cpu().numpy()
    z = ds.normals().cpu().numpy()
    assert ds.margin > 64 and ds.n_raw == RETRY_N_UNIFORM + RETRY_N_NORMAL + ds.margin
    u_after = ds.uniforms().cpu().numpy()            # (from the regenerated buffer)
    want_u = ref.random(RETRY_N_UNIFORM)
    assert_array_equal(u_before, want_u)
    assert_array_equal(u_after, want_u)
    _assert_numpy_normals(z, ref.standard_normal(RETRY_N_NORMAL))
    assert rng.bit_generator.state == ref.bit_generator.state
    assert_array_equal(rng.random(5), ref.random(5))


def test_deferred_device_stream_reports_a_buffer_that_was_too_short(obe, hip):
    """normals_deferred() / finish_normals() on the same short buffer: finish_normals() returns False without
    moving the host generator, and normals() then delivers numpy's numbers from a longer buffer."""
    import torch
    rng, ref, ds = _short_device_stream(hip, 22)
    before = rng.bit_generator.state
    pinned = torch.zeros(2, dtype=torch.int64).pin_memory()
    assert hip.cdll.obe_defer_host_sync(1) == 0
    try:
        ds.normals_deferred(pinned)
    finally:
        assert hip.cdll.obe_defer_host_sync(0) == 1
    torch.cuda.synchronize()
    assert ds.finish_normals(pinned) is False
    assert ds.margin > 64 and ds.n_raw == RETRY_N_UNIFORM + RETRY_N_NORMAL + ds.margin
    assert rng.bit_generator.state == before
    z = ds.normals().cpu().numpy()
    assert_array_equal(ds.uniforms().cpu().numpy(), ref.random(RETRY_N_UNIFORM))
    _assert_numpy_normals(z, ref.standard_normal(RETRY_N_NORMAL))
    assert rng.bit_generator.state == ref.bit_generator.state


def test_pipelined_resample_falls_back_when_the_raw_buffer_is_too_short(obe, hip):
    """resample() with the smallest raw buffer obe_resample_begin accepts (head-room 4096) for a stream that
    needs more (condition below, from the oracle): the pipelined path draws the normals again from a longer
    buffer and repeats the gather — same indices, particles, weights, moments and generator state as the
    step-by-step path; the head-room has grown, and the next resample (new buffers) agrees again."""
    n, d, seed = zo.FALLBACK_N, zo.FALLBACK_D, zo.FALLBACK_SEED
    consumed = zo.numpy_consumption(seed, n, n * d)
    print(f"numpy consumes {consumed} raw values for {n * d} normals: {consumed - n * d} extra, head-room 4096 - 64")
    assert consumed > n * d + 4096 - zo.END_GUARD
    g = np.random.default_rng(123)
    prior = g.normal(0.0, 1.0, (d, n)) * np.arange(1, d + 1)[:, None]
    w1 = g.exponential(1.0, n) ** 3
    w1 /= w1.sum()
    w2 = g.exponential(1.0, n) ** 2
    w2 /= w2.sum()

    def state_of(pdf):
        return (pdf.last_resample_indices_device.cpu().numpy(), np.array(pdf.particles), np.array(pdf.particle_weights),
                pdf.mean(), pdf.covariance(), pdf.rng.bit_generator.state)

    out = {}
    for piped in (True, False):
        pdf = obe.ParticlePDF(prior.copy(), scale=True)
        pdf.tuning_parameters["pipelined_resample"] = piped
        pdf.particle_weights = w1.copy()
        pdf.rng = np.random.default_rng(seed)
        if piped:
            b = pdf._resample_buffers(n, d)
            b["margin"] = 4096
            b["n_raw"] = n + n * d + 4096
        pdf.resample()
        first = state_of(pdf)
        if piped:
            assert b["margin"] > 4096
        pdf.particle_weights = w2.copy()
        pdf.resample()
        if piped:
            again = pdf._rs_bufs
            assert again is not b and again["margin"] > 4096 and again["n_raw"] == n + n * d + again["margin"]
        out[piped] = first + state_of(pdf)
    for a, b_ in zip(out[True], out[False]):
        if isinstance(a, dict):
            assert a == b_
        else:
            assert_array_equal(a, b_)
    ref = np.random.default_rng(seed)
    ref.random(n)
    ref.standard_normal(n * d)
    assert out[True][5] == ref.bit_generator.state


# ------------------------------------------------------------------ the full slow-draw segment
# mirrored from csrc/obe_rng.hip and csrc/obe_common.h:
CLASSIFY_BLOCKS_MAX = 1024     # obe_pcg64_uniforms_classify: blocks = min<int64_t>(1024, (total + kBlock - 1) / kBlock)
CLASSIFY_BLOCK = 256           # obe_common.h: constexpr int kBlock = 256   (threads per workgroup)
SLOW_PER_BLOCK = 128           # obe_rng.hip: constexpr int kSlowPerBlock = 128   (queued draws per workgroup)


def test_classification_with_full_slow_draw_segments(obe, hip):
    """pcg_uniform_classify_kernel queues the draws that leave their rectangle, 128 per workgroup; a workgroup that
    meets more takes the wedge / tail branches in place.  At 8.1 M positions (1024 workgroups, ~117 such draws
    each) both happen — condition below: at least 5 % of the workgroups over 128 and at least 5 % under — and
    the normals are numpy's either way."""
    import torch
    from optbayesexpt_amd import _devrng, _lib
    seed, n_uniform, n_normal = 5, 65_537, 7_700_001
    n_rel = n_normal + n_normal // 24 + 4096
    total = n_uniform + n_rel
    rng, ref = np.random.default_rng(seed), np.random.default_rng(seed)
    rng.random(11)
    ref.random(11)
    # which workgroup meets which position: thread g = block * 256 + lane walks g, g + stride, ...
    probe = np.random.default_rng(seed)
    probe.random(11)
    raw = probe.bit_generator.random_raw(total)
    slow = ((raw >> np.uint64(9)) & np.uint64(zo.MASK52)) >= zo.KI_ARR[(raw & np.uint64(0xff)).astype(np.intp)]
    slow[:n_uniform] = False
    blocks = min(CLASSIFY_BLOCKS_MAX, (total + CLASSIFY_BLOCK - 1) // CLASSIFY_BLOCK)
    per_block = np.bincount((np.flatnonzero(slow) % (blocks * CLASSIFY_BLOCK)) // CLASSIFY_BLOCK, minlength=blocks)
    over, under = np.mean(per_block > SLOW_PER_BLOCK), np.mean(per_block < SLOW_PER_BLOCK)
    print(f"{total} positions, {blocks} workgroups, {per_block.mean():.1f} slow draws each: {over:.1%} over, {under:.1%} under")
    assert blocks == CLASSIFY_BLOCKS_MAX and over >= 0.05 and under >= 0.05
    del raw, slow

    st, h_state = _devrng.pcg64_state(rng)
    dev = torch.device("cuda", 0)
    u = torch.empty(n_uniform, dtype=torch.float64, device=dev)
    z = torch.empty(n_normal, dtype=torch.float64, device=dev)
    ws = torch.empty(int(hip.cdll.obe_ziggurat_workspace_bytes(n_rel)) // 8 + 1, dtype=torch.float64, device=dev)
    tables = _devrng._tables(dev)
    consumed = np.zeros(2, dtype=np.int64)
    P = _lib.c_void_p
    hip.call("obe_pcg64_uniforms_classify", _lib.host_ptr(h_state), n_uniform, n_rel, P(u.data_ptr()), P(tables.data_ptr()),
             P(ws.data_ptr()), ws.numel() * 8, None)
    hip.call("obe_ziggurat_finish", n_rel, n_normal, P(z.data_ptr()), _lib.host_ptr(consumed), P(ws.data_ptr()),
             ws.numel() * 8, None)
    assert_array_equal(u.cpu().numpy(), ref.random(n_uniform))
    _assert_numpy_normals(z.cpu().numpy(), ref.standard_normal(n_normal))
    _devrng.advance(rng, st, n_uniform + int(consumed[0]))
    assert rng.bit_generator.state == ref.bit_generator.state
