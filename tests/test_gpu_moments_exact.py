"""The K3 moment block on the device (GPU) at every parameter count, tile and grid class, against the two references of
tests/_moments_oracle.py (pinned on the CPU by tests/test_moments_oracle_host.py, which also shows that the general
inputs used here tell a wrong kernel from a right one).

EXACT CLOUDS (integer values, weights q 2^(shift - k) with sum q = 2^k): every sum is exact in any order, so the whole
block — W, W2, mean, m1, m2, std, both triangles of the covariance — is compared BIT FOR BIT with exact_block.
GENERAL DOUBLES (rows with mean / sd up to 1e6, weights over 300 decades, one heavy particle, sum w = 0.8125): every
value within block_bounds of longdouble_block; the worst measured fraction of the bound is printed per quantity.
THE PRODUCERS (obe_moments, the fused update in both fold forms, the constraint mask's second half) leave the same
bits.  No tolerance in this file is a literal: each comes from block_bounds or the assertion is equality — except the
argument of _replay.close_weights, which is the project's own bar for weights.

The harness calls obe_moments at the C ABI on a cloud with ld = n + 5 and NaN in the padding, with d_out longer than the
block and guarded by a sentinel, a NaN-filled workspace of exactly hip.workspace_bytes, and the host copy guarded too."""
import ctypes
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _moments_oracle as mo

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, GUARD = 5, 9
SENTINEL = -6.02214076e23
WEIGHT_RTOL = 1e-10            # the project's bar for particle weights (close_weights: on the exponent)
WORST = {}                     # quantity -> (worst fraction of its bound, where): test_worst_fractions_are_reported


@pytest.fixture(scope="module")
def obe(hip):
    import optbayesexpt_amd
    return optbayesexpt_amd


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b, what):
    """Bit for bit; a NaN where the other has one (fact == 0: NumPy's 0 * inf)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert_array_equal(np.isnan(a), np.isnan(b), err_msg=what + ": NaN pattern")
    ok = ~np.isnan(a)
    assert_array_equal(_bits(a)[ok], _bits(b)[ok], err_msg=what)


def _untouched(a, what):
    assert_array_equal(_bits(a), _bits(np.full(len(a), SENTINEL)), err_msg=what + ": written although it is not this call's")


class Cloud:
    """One cloud on the device, ld = n + 5 with NaN in the padding, and obe_moments on it at the C ABI."""

    def __init__(self, hip, x):
        import torch
        from optbayesexpt_amd import _lib
        self.hip, self.torch, self._lib = hip, torch, _lib
        self.d, self.n = x.shape
        self.ld = self.n + PAD
        buf = np.full((self.d, self.ld), np.nan)
        buf[:, :self.n] = x
        self.x = torch.from_numpy(buf).cuda()
        self.len = hip.moments_len(self.d)
        assert self.len == mo.block_len(self.d)
        self.ws_bytes = hip.workspace_bytes(self.n, 1, 1, self.d)
        self.st = P(torch.cuda.current_stream().cuda_stream)

    def fresh_out(self):
        return self.torch.full((self.len + GUARD,), SENTINEL, dtype=self.torch.float64, device="cuda")

    def call(self, w, want_cov, out=None, host=None):
        """(device block with its guard, host block with its guard).  `w`: NumPy weights or a device tensor; `out`: the
        d_out of an earlier call (want_cov = 2 continues it); `host`: a page-locked array to deliver into (default: a
        pageable one)."""
        torch = self.torch
        wd = w if isinstance(w, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).cuda()
        assert wd.numel() == self.n
        out = self.fresh_out() if out is None else out
        ws = torch.full((-(-self.ws_bytes // 8),), float("nan"), dtype=torch.float64, device="cuda")
        if host is None:
            host = np.full(self.len + GUARD, SENTINEL)
        self.hip.call("obe_moments", P(self.x.data_ptr()), self.ld, self.d, self.n, P(wd.data_ptr()), want_cov,
                      P(out.data_ptr()), self._lib.host_ptr(host), P(ws.data_ptr()), self.ws_bytes, self.st)
        torch.cuda.synchronize()
        dev = out.cpu().numpy()
        _untouched(dev[self.len:], "the guard behind d_out")
        _untouched(np.array(host[self.len:]), "the guard behind h_out")
        delivered = self.len if want_cov else 2 + 4 * self.d
        _same_bits(np.array(host[:delivered]), dev[:delivered], "h_out against d_out")
        return dev, np.array(host)

    def block(self, w, want_cov=1):
        return self.call(w, want_cov)[0][:self.len]


def _exact_case(seed, d, n, shift=0):
    g = np.random.default_rng(seed)
    x, q, k = mo.exact_cloud(g, d, n, shift)
    return g, x, q, k


def _check_exact(hip, x, q, k, shift, what):
    want = mo.exact_block(x, q, k, shift)
    cloud = Cloud(hip, x)
    got = cloud.block(mo.exact_weights(q, k, shift))
    sec = mo.sections(cloud.d)
    for name, sl in sec.items():
        _same_bits(got[sl], want[sl], f"{what}: {name}")
    cov = got[sec["cov"]].reshape(cloud.d, cloud.d)
    _same_bits(cov, cov.T, what + ": the two triangles")
    return cloud, want


# ------------------------------------------------------------------------------------------------ exact clouds
@pytest.mark.parametrize("d", range(1, 17))
def test_exact_cloud_every_parameter_count(hip, d):
    """NV = 2 + 2 D first moments and D (D + 1) / 2 triangle values: one partly filled reduce-scatter group (D <= 10),
    two (D = 11 ... 15: 66 ... 120 values), three (D = 16), two workgroups."""
    _, x, q, k = _exact_case(1000 + d, d, 293)
    _check_exact(hip, x, q, k, 0, f"d={d} n=293")


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, 131072 + 293])
@pytest.mark.parametrize("d", [1, 5, 11, 16])
def test_exact_cloud_every_edge_of_wave_workgroup_and_grid(hip, d, n):
    """n = 1: fact == 0, the covariance is 0 * inf = NaN as NumPy's; the rest of the block to the bit."""
    _, x, q, k = _exact_case(2000 + 17 * d + n % 1009, d, n)
    _, want = _check_exact(hip, x, q, k, 0, f"d={d} n={n}")
    assert np.all(np.isnan(want[mo.sections(d)["cov"]])) == (n == 1)


@pytest.mark.parametrize("d", [1, 5, 11, 16, 17])
def test_exact_cloud_one_hot_weight(hip, d):
    g, x, q, k = _exact_case(2500 + d, d, 1)
    x, q = mo.with_zero_weights(g, x, q, 0, 150)
    x, q = mo.with_zero_weights(g, x, q, x.shape[1], 142)
    _, want = _check_exact(hip, x, q, k, 0, f"d={d} one-hot among 293")
    sec = mo.sections(d)
    assert np.all(np.isnan(want[sec["cov"]])) and np.all(want[sec["std"]] == 0.0)


@pytest.mark.parametrize("d,n", [(4, 2 ** 21 - 1), (5, 2 ** 21), (4, 2 ** 21 + 293), (7, 2 ** 21 + 293),
                                 (8, 2 ** 21 + 293)])
def test_exact_cloud_every_grid_class(hip, obe, d, n):
    """One workgroup per CU below 2^21 particles; from there three (D <= 4), two (D <= 7) or one: 768-, 512- and 256-row
    folds, the second and third trip of fold_values_block.  (5, 2^21) once more through ParticlePDF, whose own
    workspace and K3 block serve mean() / std() / covariance() (first moments, then want_cov = 2)."""
    _, x, q, k = _exact_case(3000 + d, d, n)
    _, want = _check_exact(hip, x, q, k, 0, f"d={d} n={n}")
    if (d, n) == (5, 2 ** 21):
        sec = mo.sections(d)
        pdf = obe.ParticlePDF(x)
        pdf.particle_weights = mo.exact_weights(q, k)
        _same_bits(pdf.mean(), want[sec["mean"]], "ParticlePDF.mean()")
        _same_bits(pdf.std(), want[sec["std"]], "ParticlePDF.std()")
        _same_bits(pdf.covariance().reshape(-1), want[sec["cov"]], "ParticlePDF.covariance()")
        _same_bits(np.array(pdf._moments(True)[:len(want)]), want, "ParticlePDF's host block")


@pytest.mark.parametrize("n", [293, 65537])
@pytest.mark.parametrize("d", [17, 23, 24, 25, 32, 33, 40, 65])
def test_exact_cloud_tiles(hip, d, n):
    """8-row tiles and 8 x 8 tile pairs: short last tiles of 1 and 7 rows, full ones, a pair with both tiles short
    (the last tile with itself), nine tiles."""
    _, x, q, k = _exact_case(4000 + d, d, n)
    _check_exact(hip, x, q, k, 0, f"d={d} n={n}")


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("d", [17, 33])
def test_exact_cloud_tiles_small(hip, d, n):
    _, x, q, k = _exact_case(4500 + d + n, d, n)
    _check_exact(hip, x, q, k, 0, f"d={d} n={n}")


@pytest.mark.parametrize("d", [3, 11, 17, 40])
def test_want_cov_0_then_2_is_want_cov_1(hip, d):
    _, x, q, k = _exact_case(5000 + d, d, 293)
    w = mo.exact_weights(q, k)
    want = mo.exact_block(x, q, k)
    cloud = Cloud(hip, x)
    first = 2 + 4 * d
    out = cloud.fresh_out()
    dev, host = cloud.call(w, 0, out=out)
    _same_bits(dev[:first], want[:first], "want_cov = 0: the first moments")
    _untouched(dev[first:cloud.len], "want_cov = 0: the covariance part of d_out")
    _untouched(host[first:cloud.len], "want_cov = 0: the covariance part of h_out")
    dev2, host2 = cloud.call(w, 2, out=out)
    _same_bits(dev2[:cloud.len], want, "want_cov = 2 behind want_cov = 0")
    _same_bits(host2[:cloud.len], want, "want_cov = 2: a pageable h_out gets the whole block")
    _same_bits(dev2[:cloud.len], cloud.block(w, 1), "want_cov = 2 against want_cov = 1")


@pytest.mark.parametrize("shift", [2, -3])
@pytest.mark.parametrize("d", [3, 16, 17])
def test_exact_cloud_weights_that_do_not_sum_to_one(hip, d, shift):
    """sum w = 4 and 1 / 8: mean and covariance divide by what the weights sum to; std is the reference's
    sqrt(m2 - m1^2) whatever they sum to (NaN where that is negative, as NumPy's)."""
    _, x, q, k = _exact_case(6000 + d, d, 293, shift)
    _, want = _check_exact(hip, x, q, k, shift, f"d={d} shift={shift}")
    assert want[0] == 2.0 ** shift


@pytest.mark.parametrize("d", [3, 16, 17])
def test_exact_cloud_zero_weights(hip, d):
    """Zero weights at both ends, and a run of 300 of them from column 250 on: workgroup 1 sees nothing else."""
    g, x, q, k = _exact_case(7000 + d, d, 293)
    x, q = mo.with_zero_weights(g, x, q, 247, 300)
    x, q = mo.with_zero_weights(g, x, q, 0, 3)
    x, q = mo.with_zero_weights(g, x, q, x.shape[1], 4)
    assert x.shape[1] == 600 and not q[256:512].any() and q[0] == 0 and q[-1] == 0 and q[:256].any()
    _check_exact(hip, x, q, k, 0, f"d={d} zero weights")


@pytest.mark.parametrize("d", [3, 17, 40])
def test_page_locked_h_out_gets_the_same_bits(hip, d):
    """Page-locked h_out: the fold kernels (the tiled ones for d > 16) write the host words themselves; also with the
    wait left to the caller (obe_defer_host_sync)."""
    from optbayesexpt_amd import _lib
    _, x, q, k = _exact_case(8000 + d, d, 293)
    w = mo.exact_weights(q, k)
    want = mo.exact_block(x, q, k)
    cloud = Cloud(hip, x)
    pageable = cloud.call(w, 1)[1]
    _same_bits(pageable[:cloud.len], want, "pageable h_out")
    for deferred in (False, True):
        pinned = _lib.pinned_array(cloud.len + GUARD)
        pinned[:] = SENTINEL
        if deferred:
            assert hip.cdll.obe_defer_host_sync(1) == 0
        try:
            _, host = cloud.call(w, 1, host=pinned)
        finally:
            if deferred:
                assert hip.cdll.obe_defer_host_sync(0) == 1
        _same_bits(host, pageable, f"page-locked h_out (deferred={deferred})")


# --------------------------------------------------------------------------------------------- general doubles
@functools.lru_cache(maxsize=2)
def _general(d, n):
    x, w = mo.general_case(d, n)
    return x, w, mo.longdouble_block(x, w), mo.block_bounds(x, w, n)


def _within_bounds(got, x, w, what, ref=None, bound=None):
    """Every value of `got` (a block or its first-moment part) within block_bounds of longdouble_block; prints and
    records the worst fraction of the bound per quantity."""
    d, n = x.shape
    ref = mo.longdouble_block(x, w) if ref is None else ref
    bound = mo.block_bounds(x, w, n) if bound is None else bound
    assert np.all(np.isfinite(bound)) and np.all(bound > 0), what
    worst = mo.worst_fraction(got, ref[:len(got)], bound[:len(got)], d)
    print(f"{what}: worst |error| / bound: " + ", ".join(f"{name} {v:.3g}" for name, v in worst.items()))
    for name, v in worst.items():
        if v > WORST.get(name, (-1.0, ""))[0]:
            WORST[name] = (v, what)
    assert max(worst.values()) <= 1.0, f"{what}: beyond the derived bound: {worst}"


@pytest.mark.parametrize("d,n", mo.GENERAL_CASES)
def test_general_doubles_within_the_derived_bound(hip, d, n):
    x, w, ref, bound = _general(d, n)
    _within_bounds(Cloud(hip, x).block(w), x, w, f"obe_moments d={d} n={n}", ref, bound)


# ------------------------------------------------------------------------------------------- the producers agree
def _record(x, w):
    """A reading of row 0 half a standard deviation off its mean, with twice that as sigma: a posterior that keeps
    most of the cloud."""
    m = np.average(x[0], weights=w)
    s = float(np.sqrt(np.average((x[0] - m) ** 2, weights=w)))
    return ((0.0,), float(m + 0.5 * s), 2.0 * s)


def _update(obe, x, w, fused):
    """(weights, first-moment block, whole block after covariance()) of pdf_update() on a first_parameter model over the
    d rows of x (the model reads row 0)."""
    d = x.shape[0]
    o = obe.OptBayesExpt(obe.models.first_parameter(), (np.array([0.0]),), x.copy(), (), scale=False,
                         auto_resample=False)
    o.tuning_parameters["fused_moments"] = fused
    o.tuning_parameters["strict_sums"] = False
    o.particle_weights = w
    o.pdf_update(_record(x, w))
    key = (o._particles.version, o._weights.version)
    assert (o._mom_host_key is not None and o._mom_host_key[:2] == key) is fused
    first = np.array(o._moments(False)[:2 + 4 * d])
    weights = np.array(o.particle_weights)
    o.covariance()
    return weights, first, np.array(o._moments(True)[:mo.block_len(d)])


def _producer_input(d, n):
    x, w = mo.general_case(d, n)
    return x, w / w.sum()


@pytest.mark.parametrize("d,n", [(d, n) for n in (293, 65537, 131072 + 293) for d in range(1, 17)]
                         + [(d, 2 ** 21 + 293) for d in (4, 7, 8)])
def test_fused_update_leaves_the_bits_of_update_then_moments(obe, d, n):
    """normalize_moments_kernel<D, FOLD = true> against normalize_kernel + obe_moments: weights and K3 block bit for
    bit (131 072 + 293: the clamp of the two-particle trip's second load), the block within block_bounds of
    longdouble_block on the posterior weights, the covariance pass behind it (want_cov = 2) included."""
    import _replay
    import oracle
    x, w = _producer_input(d, n)
    fused, plain = _update(obe, x, w, True), _update(obe, x, w, False)
    for a, b, what in zip(fused, plain, ("weights", "first moments", "block with covariance")):
        _same_bits(a, b, f"d={d} n={n}: {what}, fused against unfused")
    _same_bits(fused[2][:len(fused[1])], fused[1], "the covariance pass leaves the first moments alone")
    _within_bounds(fused[2], x, fused[0], f"fused update d={d} n={n}")
    _, y, sigma = _record(x, w)
    w1 = oracle.normalized_product(w, oracle.gauss_likelihood(x[0], y, sigma))
    _replay.close_weights(fused[0], w1, WEIGHT_RTOL, f"d={d} n={n}: posterior weights")


CHILD_CASES = [(d, n) for d in (1, 5, 16) for n in (293, 65537)]


def _child():
    """Run as a child process with OBE_CONTROL_SLOTS=0: no arrival counter, so the fused update takes
    normalize_moments_kernel<D, FOLD = false> and the separate fold launch.  Prints the block's bytes."""
    assert os.environ.get("OBE_CONTROL_SLOTS") == "0"
    sys.path.insert(0, ROOT)
    import optbayesexpt_amd as obe
    out = {}
    for d, n in CHILD_CASES:
        weights, first, whole = _update(obe, *_producer_input(d, n), True)
        out[f"{d},{n}"] = [first.tobytes().hex(), whole.tobytes().hex(), hashlib.sha256(weights.tobytes()).hexdigest()]
    print("K3 BLOCKS " + json.dumps(out))


def test_fused_update_without_an_arrival_counter_leaves_the_same_bits(obe):
    env = dict(os.environ, OBE_CONTROL_SLOTS="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [s for s in r.stdout.splitlines() if s.startswith("K3 BLOCKS ")]
    assert len(line) == 1, r.stdout[-2000:]
    child = json.loads(line[0][len("K3 BLOCKS "):])
    for d, n in CHILD_CASES:
        weights, first, whole = _update(obe, *_producer_input(d, n), True)
        got = child[f"{d},{n}"]
        assert got[0] == first.tobytes().hex(), f"d={d} n={n}: first moments, FOLD = false against FOLD = true"
        assert got[1] == whole.tobytes().hex(), f"d={d} n={n}: whole block"
        assert got[2] == hashlib.sha256(weights.tobytes()).hexdigest(), f"d={d} n={n}: weights"


@pytest.mark.parametrize("d", range(1, 17))
def test_mask_with_a_bound_nobody_violates_leaves_the_bits_of_obe_moments(hip, d):
    from test_gpu_constraints import Abi
    _, x, q, k = _exact_case(9000 + d, d, 293)
    w = mo.exact_weights(q, k)
    first = 2 + 4 * d
    want = mo.exact_block(x, q, k)[:first]
    w2, mom_dev, mom_host, changed = Abi(hip, x).mask_bounds_moments(w, [d - 1], [-1000.0], [np.inf], [0])
    assert changed == 0
    _same_bits(w2, w, "the weights are untouched")
    dev, _ = Cloud(hip, x).call(w, 0)
    _same_bits(mom_dev, dev[:first], "the mask's K3 block against obe_moments(want_cov = 0)")
    _same_bits(mom_host, dev[:first], "the mask's host block")
    _same_bits(mom_dev, want, "the mask's K3 block against exact_block")


def test_worst_fractions_are_reported():
    """Prints, per quantity, the worst |error| / bound the general-double comparisons of this run measured (the
    figures of DESIGN.md's verification table)."""
    if WORST:
        print("K3 moments, worst |error| / block_bounds: "
              + "; ".join(f"{name} {v:.3g} ({where})" for name, (v, where) in WORST.items()))
    assert all(v <= 1.0 for v, _ in WORST.values())


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if sys.argv[1:] == ["child"]:
        _child()
