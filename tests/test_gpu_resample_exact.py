"""The gather + nudge that ends every resample (csrc/obe_resample.hip: resample_kernel<D, AOS, BOUNDS...>,
resample_wide_kernel, soa_to_aos_kernel<D>, gather_columns_kernel) at the C ABI, bit for bit, at every cloud width.

The contract is the chain of operations that include/obe_hip.h documents — an FMA chain from zero in j order, one
addition, and a scale step of three roundings — and tests/_resample_oracle.py restates it in exact arithmetic, so every
comparison in this file is ``assert_array_equal`` on the float64 BITS: there is no tolerance anywhere.  (a) general
doubles against the exact oracle, D = 1 .. 16, 17 and 33, the three plain forms; (b) in every such case padded leading
dimensions, NaN behind the old rows, a sentinel behind the new rows and the weights; (c) indices outside the cloud;
(d) large clouds — both sides of the copy-first switch, a second trip of the grid-stride loop — on integer data, where
NumPy integer arithmetic is the reference; (e) the bounded and masked gathers with bounds that are outputs of the
nudge itself; (f) obe_gather_columns; (g) the refusals.  tests/test_resample_oracle_host.py shows on the CPU that the
inputs of (a) tell the contract from a chain that rounds its products, one summed backwards, one started from the old
value and a contracted scale step."""
import ctypes
import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _resample_oracle as ro

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
INF = np.inf
A = ro.A_PARAM
SENTINEL = -1.2345678901234567e123
PAD_OLD, PAD_NEW = 5, 3                      # ld_old = n + 5 (NaN behind every old row), ld_new = n + 3 (the sentinel)
MAX_BLOCKS = 2048                            # the grid cap of the streaming kernels: d_mask_partials is 2 x this
FORMS = ("rows", "rows+ws", "aos")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()      # (the cached oracle inputs are read-only)


def _filled(shape, value=SENTINEL):
    import torch
    return torch.full(shape, value, dtype=torch.float64, device="cuda")


def _ptr(t):
    return P(t.data_ptr())


def _host(a):
    return P(a.ctypes.data)


def _stream():
    import torch
    return P(torch.cuda.current_stream().cuda_stream)


def outside_indices(idx, n):
    """A few entries of ``idx`` set to -1, n, n + 5, 2^62 and -2^62 (a copy)."""
    idx = idx.copy()
    idx[[3, n // 5, n // 2, n - 2, n - 1]] = (-1, n, n + 5, 2 ** 62, -2 ** 62)
    return idx


class Cloud:
    """One resample's inputs on the device — the old rows with ld_old = n + 5 and NaN in the padding, their (N, D)
    copy made on the host — and the calls of this file on them.  Every call checks what lies around its results: the
    padding of d_new and the element behind the weights keep the sentinel's bits."""

    def __init__(self, hip, old, idx, z, F, mean):
        self.hip = hip
        self.d, self.n = old.shape
        padded = np.full((self.d, self.n + PAD_OLD), np.nan)
        padded[:, :self.n] = old
        self.old = _dev(padded)
        self.aos = _dev(old.T) if self.d <= 16 else None
        self.idx, self.z = _dev(np.asarray(idx, dtype=np.int64)), _dev(z)
        self.F, self.mean = np.ascontiguousarray(F, dtype=np.float64), np.ascontiguousarray(mean, dtype=np.float64)

    def ws_doubles(self):
        """What the header asks of the workspace: 8 D N bytes for the (N, D) copy; F and the mean of a wide cloud."""
        return self.d * self.n if self.d <= 16 else self.d * self.d + self.d

    def _outputs(self):
        return _filled((self.d, self.n + PAD_NEW)), _filled((self.n + 1,))

    def _collect(self, new, w, what):
        new, w = new.cpu().numpy(), w.cpu().numpy()
        _same(new[:, self.n:], np.full((self.d, PAD_NEW), SENTINEL), what + ": the padding of d_new")
        _same(w[self.n:], [SENTINEL], what + ": the element behind the weights")
        return np.ascontiguousarray(new[:, :self.n]), w[:self.n].copy()

    def plain(self, form, a, scale):
        """(new (D, n), weights (n,)) of obe_resample_particles without / with a workspace, or of _aos."""
        new, w = self._outputs()
        tail = (a, scale, _ptr(new), self.n + PAD_NEW, _ptr(w))
        head = (self.d, self.n, _ptr(self.idx), _ptr(self.z), _host(self.F), _host(self.mean))
        if form == "aos":
            self.hip.call("obe_resample_particles_aos", _ptr(self.aos), *head, *tail, _stream())
        else:
            ws = _filled((self.ws_doubles(),)) if form == "rows+ws" else None
            self.hip.call("obe_resample_particles", _ptr(self.old), self.n + PAD_OLD, *head, *tail,
                          _ptr(ws) if ws is not None else None, ws.numel() * 8 if ws is not None else 0, _stream())
        return self._collect(new, w, f"D={self.d} n={self.n} {form} scale={scale}")

    def check_plain(self, want, a, scale, forms, what):
        for form in forms:
            new, w = self.plain(form, a, scale)
            _same(new, want, f"{what} {form} scale={scale}: the new cloud")
            _same(w, np.full(self.n, 1.0 / self.n), f"{what} {form} scale={scale}: weights")

    def gathered(self, name, a, scale, *bounds_args):
        """(new, weights, the weights on the device, d_mask_partials on the device) of a masked / bounded gather."""
        new, w = self._outputs()
        partials = _filled((2 * MAX_BLOCKS,))
        self.hip.call(name, _ptr(self.aos), self.d, self.n, _ptr(self.idx), _ptr(self.z), _host(self.F), _host(self.mean),
                      a, scale, _ptr(new), self.n + PAD_NEW, _ptr(w), *bounds_args, _ptr(partials), _stream())
        return self._collect(new, w, f"D={self.d} n={self.n} {name}") + (w[:self.n], partials)


# ------------------------------------------------------------------------------- the oracle, once per case
@functools.lru_cache(maxsize=None)
def general(d, n, outside=False):
    """(inputs, the oracle before its scale step) on general doubles; the scale step is three array operations."""
    old, idx, z, F, mean = ro.general_case(d, n)
    if outside:
        idx = outside_indices(idx, n)
    v = ro.unscaled_exact(old, idx, z, F)
    for x in (old, idx, z, F, mean, v):
        x.setflags(write=False)
    return (old, idx, z, F, mean), v


def expected(d, n, scale, outside=False):
    inputs, v = general(d, n, outside)
    return inputs, ro.scale_two_roundings(v, inputs[4], A) if scale else v


def forms_of(d):
    return FORMS if d <= 16 else ("rows+ws",)          # a wide cloud: only the (D, N) rows, F and the mean in the workspace


# ------------------------------------------------------------------- (a) + (b) general doubles, every width
GENERAL = [(d, 293) for d in range(1, 17)] + [(17, 293), (33, 293)] + \
          [(d, n) for d in (1, 16, 17) for n in (1, 255, 256, 257)]


@pytest.mark.parametrize("d,n", GENERAL)
def test_general_doubles_are_the_exact_chain(hip, d, n):
    """n = 293: a full tile of 256 and a ragged one of 37, both branches of the LDS read of the normals; 1, 255, 256,
    257: less than a tile, exactly one, one particle more.  The three forms give the oracle's bits, hence each
    other's."""
    for scale in (0, 1):
        inputs, want = expected(d, n, scale)
        Cloud(hip, *inputs).check_plain(want, A, scale, forms_of(d), f"D={d} n={n}")


# ------------------------------------------------------------------------------ (c) indices outside the cloud
@pytest.mark.parametrize("d", [1, 3, 16, 17])
def test_an_index_outside_the_cloud_reads_its_nearest_end(hip, d):
    n = 293
    for scale in (0, 1):
        inputs, want = expected(d, n, scale, outside=True)
        idx = inputs[1]
        assert sorted(int(i) for i in idx if i < 0 or i >= n) == sorted((-1, n, n + 5, 2 ** 62, -2 ** 62))
        # what is expected, without the oracle's own clamp: the draws below the cloud read particle 0, those above n - 1
        by_hand = list(inputs)
        by_hand[1] = np.where(idx < 0, 0, np.where(idx >= n, n - 1, idx))
        _same(want, ro.nudge_exact(*by_hand, A, scale), "the oracle's clamp")
        Cloud(hip, *inputs).check_plain(want, A, scale, ("rows", "aos") if d <= 16 else ("rows+ws",), f"D={d} outside")


# ------------------------------------------------------------------------------ (d) large clouds, exact data
SECOND_TRIP = 2048 * 256 + 256 + 37          # the grid is capped at 2048 workgroups: a full and a ragged tile, idle groups


@pytest.mark.parametrize("n", [65535, 65536, SECOND_TRIP])
@pytest.mark.parametrize("d", [2, 16, 17])
def test_large_clouds_on_exact_data_are_integer_arithmetic(hip, d, n):
    """Integers (|old| <= 2^20, |z|, |F| <= 8), a = 0.5, idx a permutation — every element of the (N, D) copy is read
    exactly once.  65 535 / 65 536: the two sides of the copy-first switch of obe_resample_particles, with and without
    the 8 D n bytes it needs; 2048 * 256 + 293: the second trip of the grid-stride loop of resample_kernel,
    soa_to_aos_kernel and resample_wide_kernel."""
    inputs = ro.integer_case(d, n)
    cloud = Cloud(hip, *inputs)
    assert cloud.ws_doubles() * 8 == (8 * d * n if d <= 16 else 8 * (d * d + d))
    for scale in (0, 1):
        want = ro.nudge_integers(*inputs, scale)
        cloud.check_plain(want, 0.5, scale, forms_of(d), f"D={d} n={n} integers")


# ------------------------------------------------------------------- (e) the bounded and the masked gather
def _abi(hip, x):
    from test_gpu_constraints import Abi
    return Abi(hip, x)


def _check_mask(hip, cloud, got, want_new, rows, lo, hi, flags, what):
    """The new cloud is the plain form's; a weight is 0.0 exactly where the oracle says violator, 1/n elsewhere; the
    count half of d_mask_partials is each workgroup's number of violators; and obe_mask_renorm_moments() on these
    partial sums leaves what obe_mask_bounds_moments() leaves for uniform weights on the same cloud, bit for bit."""
    new, w, wd, partials = got
    n = cloud.n
    _same(new, want_new, what + ": the new cloud")
    bad = ro.violators(want_new, rows, lo, hi, flags)
    assert 0 < bad.sum() < n, what
    _same(w, np.where(bad, 0.0, 1.0 / n), what + ": weights")
    nb = -(-n // 256)
    parts = partials.cpu().numpy()
    per_group = np.add.reduceat(bad.astype(np.float64), np.arange(0, n, 256))
    _same(parts[MAX_BLOCKS:MAX_BLOCKS + nb], per_group, what + ": violators per workgroup")
    assert parts[MAX_BLOCKS:MAX_BLOCKS + nb].sum() == bad.sum()
    _same(parts[nb:MAX_BLOCKS], np.full(MAX_BLOCKS - nb, SENTINEL), what + ": partial sums behind the grid")
    _same(parts[MAX_BLOCKS + nb:], np.full(MAX_BLOCKS - nb, SENTINEL), what + ": counts behind the grid")
    abi = _abi(hip, new)
    fused = abi.mask_renorm_moments(wd, partials)
    ref = abi.mask_bounds_moments(np.full(n, 1.0 / n), rows, lo, hi, flags)
    assert fused[3] == ref[3] == int(bad.sum()), what
    for a, b, item in zip(fused[:3], ref[:3], ("renormalised weights", "moments (device)", "moments (host)")):
        _same(a, b, f"{what}: {item}")
    return bad


def _bounds_args(rows, lo, hi, flags):
    keep = (np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(lo, dtype=np.float64),
            np.ascontiguousarray(hi, dtype=np.float64), np.ascontiguousarray(flags, dtype=np.int32))
    return keep, tuple(_host(a) for a in keep) + (len(keep[0]),)


@pytest.mark.parametrize("n", [293, 5000])
@pytest.mark.parametrize("d", [1, 2, 7, 16])
def test_bounds_that_are_outputs_of_the_nudge(hip, d, n):
    """Every bound is one exact output value of its row, so a particle sits ON it: with the end closed it keeps 1/n,
    with the end open it gets 0.0.  Two ends on one row; two entries for one row (nested intervals, and the same
    interval twice with one end open in each: intersect_per_row); a row bounded below only, above only."""
    inputs, want = expected(d, n, 1)
    cloud = Cloud(hip, *inputs)
    plain, _ = cloud.plain("aos", A, 1)
    _same(plain, want, "the plain form")
    r, r0 = d - 1, 0
    s, t = np.sort(want[r]), np.sort(want[r0])
    L, H, L2, H2, M = s[n // 4], s[3 * n // 4], s[n // 3], s[2 * n // 3], t[n // 2]
    assert L < L2 < H2 < H
    # (entries, flags with every end closed, flags with ends open, the values a particle sits on)
    cases = [("two ends", [r], [L], [H], [0], [3], (r, (L, H))),
             ("nested entries", [r, r], [L, L2], [H, H2], [0, 0], [3, 3], (r, (L2, H2))),
             ("one interval twice", [r, r], [L, L], [H, H], [0, 0], [1, 2], (r, (L, H))),
             ("below only", [r0], [M], [INF], [0], [1], (r0, (M,))),
             ("above only", [r0], [-INF], [M], [0], [2], (r0, (M,)))]
    for name, rows, lo, hi, closed, opened, (row, ends) in cases:
        on_bound = np.flatnonzero(np.isin(want[row], ends))
        assert on_bound.size >= len(ends)
        bad = {}
        for label, flags in (("closed", closed), ("open", opened)):
            keep, args = _bounds_args(rows, lo, hi, flags)
            got = cloud.gathered("obe_resample_particles_aos_bounded", A, 1, *args)
            bad[label] = _check_mask(hip, cloud, got, want, rows, lo, hi, np.asarray(flags), f"D={d} n={n} {name} {label}")
        assert not bad["closed"][on_bound].any() and bad["open"][on_bound].all(), name
        assert_array_equal(np.flatnonzero(bad["open"] != bad["closed"]), on_bound)


@pytest.mark.parametrize("d,n", [(2, 293), (7, 293), (16, 293), (2, 5000)])
def test_masked_gather_at_both_zeros(hip, d, n):
    """obe_resample_particles_aos_masked is the bound (0, +inf), open, on its rows: an output that is exactly 0.0 and
    one that is exactly -0.0 are both violators, and both arrive with their sign.  The chain starts from +0.0, so the
    sum before the scale step is never -0.0; after it, -0.0 needs v*a and mean*(1 - a) both -0.0.  Integer data keep
    every operation exact; a = -0.5 (the ABI takes any a) gives (+0.0)*a = -0.0 beside a mean of -0.0."""
    a = -0.5
    old, idx, z, F, mean = ro.integer_case(d, n)
    r1, r2, pa, pb = 0, d - 1, 7, n - 3
    mean[r1], mean[r2] = -0.0, 2.0
    s = F @ z.T
    old[r1, idx[pa]] = -s[r1, pa]                          # v = 0:  0*a + (-0.0)*1.5 = -0.0
    old[r2, idx[pb]] = 6.0 - s[r2, pb]                     # v = 6:  -3 + 2*1.5 = +0.0
    old[r2, idx[pa]] = -10.0 - s[r2, pa]                   # (their other bounded row is positive: 5 + 3 and 2 - 0.0,
    old[r1, idx[pb]] = -4.0 - s[r1, pb]                    # so the zero alone decides about these two particles)
    want = ro.nudge_exact(old, idx, z, F, mean, a, 1)
    assert want[r1, pa] == 0.0 and np.signbit(want[r1, pa])
    assert want[r2, pb] == 0.0 and not np.signbit(want[r2, pb])
    _same(want, (old[:, idx] + s) * a + (mean * 1.5)[:, None], "exact data: plain NumPy")
    cloud = Cloud(hip, old, idx, z, F, mean)
    rows = np.array([r1, r2], dtype=np.int32)
    got = cloud.gathered("obe_resample_particles_aos_masked", a, 1, _host(rows), 2)
    bad = _check_mask(hip, cloud, got, want, rows, [0.0, 0.0], [INF, INF], np.array([1, 1]), f"D={d} n={n} masked")
    assert bad[pa] and bad[pb]
    assert_array_equal(bad, np.any(want[[r1, r2]] <= 0.0, axis=0))
    # the bounded form with the same bound, and with it closed: the two zeros stay
    keep, args = _bounds_args(rows, [0.0, 0.0], [INF, INF], [1, 1])
    same = cloud.gathered("obe_resample_particles_aos_bounded", a, 1, *args)
    for x, y, item in zip(got[:2], same[:2], ("the new cloud", "weights")):
        _same(x, y, "masked against bounded: " + item)
    keep, args = _bounds_args(rows, [0.0, 0.0], [INF, INF], [0, 0])
    closed = cloud.gathered("obe_resample_particles_aos_bounded", a, 1, *args)
    bad0 = _check_mask(hip, cloud, closed, want, rows, [0.0, 0.0], [INF, INF], np.array([0, 0]), f"D={d} n={n} closed 0")
    assert not bad0[pa] and not bad0[pb]
    assert_array_equal(bad & ~bad0, np.min(want[[r1, r2]], axis=0) == 0.0)


# ---------------------------------------------------------------------------------- (f) obe_gather_columns
@pytest.mark.parametrize("d", [1, 3, 16, 17, 40])
def test_gather_columns_is_the_indexed_copy(hip, d):
    for n in (5, 5000):
        for nd in (1, 30, 257):
            g = np.random.default_rng(100 * d + n + nd)
            x = g.standard_normal((d, n))
            x[0, 0], x[d - 1, n - 1] = -0.0, np.nan              # bits, not values, are copied
            idx = g.integers(0, n, nd)
            if nd > 1:
                idx[:nd // 3] = idx[nd // 2]                      # repeats
                idx[-5:] = (-1, n, n + 5, 2 ** 62, -2 ** 62)
            else:
                idx[0] = n + 5
            padded = np.full((d, n + 5), SENTINEL)
            padded[:, :n] = x
            xd, ix, out = _dev(padded), _dev(idx), _filled((d, nd + 3))
            hip.call("obe_gather_columns", _ptr(xd), n + 5, d, n, _ptr(ix), nd, _ptr(out), nd + 3, _stream())
            got = out.cpu().numpy()
            what = f"D={d} n={n} draws={nd}"
            _same(got[:, :nd], x[:, ro.clamp(idx, n)], what)
            _same(got[:, nd:], np.full((d, 3), SENTINEL), what + ": the padding of d_out")


# ------------------------------------------------------------------------------------------ (g) the refusals
def test_refused_calls_launch_nothing(hip):
    from optbayesexpt_amd._lib import ObeHipError
    n = 293
    made = {}

    def refused(d, call, message):
        """``call(cloud, new, w, ws)`` must be refused before any launch: status -1, the message, untouched outputs."""
        if d not in made:
            made[d] = Cloud(hip, *ro.integer_case(max(d, 1), n))
        cloud = made[d]
        new, w = _filled((max(d, 1), n + PAD_NEW)), _filled((n + 1,))
        ws = _filled((max(d, 1) ** 2 + max(d, 1),))
        with pytest.raises(ObeHipError) as err:
            call(cloud, new, w, ws)
        assert err.value.refused_before_launch and message in hip.last_error(), hip.last_error()
        for buf in (new, w, ws):
            _same(buf.cpu().numpy(), np.full(tuple(buf.shape), SENTINEL), message + ": an output was written")

    def rows_form(d_arg, ws_bytes, in_place=False):
        def call(c, new, w, ws):
            hip.call("obe_resample_particles", _ptr(c.old), n + PAD_OLD, d_arg, n, _ptr(c.idx), _ptr(c.z), _host(c.F),
                     _host(c.mean), A, 1, _ptr(c.old) if in_place else _ptr(new), n + PAD_NEW, _ptr(w),
                     _ptr(ws) if ws_bytes else None, ws_bytes, _stream())
        return call

    def aos_form(d_arg):
        def call(c, new, w, ws):
            src = c.aos if c.aos is not None else c.old
            hip.call("obe_resample_particles_aos", _ptr(src), d_arg, n, _ptr(c.idx), _ptr(c.z), _host(c.F), _host(c.mean),
                     A, 1, _ptr(new), n + PAD_NEW, _ptr(w), _stream())
        return call

    refused(17, aos_form(17), "more than OBE_FAST_DIMS parameters")
    refused(17, rows_form(17, 0), "workspace too small")
    refused(17, rows_form(17, 8 * (17 * 17 + 17) - 8), "workspace too small")
    refused(3, rows_form(3, 0, in_place=True), "in-place gather is not supported")
    refused(0, rows_form(0, 0), "n_dims must be 1..")
    refused(0, aos_form(0), "n_dims must be 1..")
    # the old cloud of the in-place call is what it was
    c = made[3]
    _same(c.old.cpu().numpy()[:, :n], ro.integer_case(3, n)[0], "the old cloud after the refused in-place call")
