"""Declarative parameter bounds on the device (GPU): the three entry points against the NumPy oracle and, bit for bit,
against the noise-only calls they generalise (adapters over them, pinned by the bits recorded before they were); the
mask inside the gather against the mask behind it; the classes against the oracle classes carrying the same
constraint as a NumPy hook."""
import copy
import ctypes
import json
import os
import pickle
import subprocess
import sys
import warnings

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _constraint_cases as cc
import _constraint_oracle as co
import _replay
import oracle
from oracle import models as omodels

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
INF = np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def obe(hip):
    import optbayesexpt_amd
    return optbayesexpt_amd


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return P(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b, what):
    """Bit for bit — a NaN (a NaN or infinite particle value in a moment, 0 / 0 in a weight) where the other has one."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert_array_equal(np.isnan(a), np.isnan(b), err_msg=what + ": NaN pattern")
    ok = ~np.isnan(a)
    assert_array_equal(_bits(a)[ok], _bits(b)[ok], err_msg=what)


class Abi:
    """The calls of this file at the C ABI, on one cloud."""

    def __init__(self, hip, x):
        import torch
        from optbayesexpt_amd import _lib
        self.hip, self._lib, self.torch = hip, _lib, torch
        self.d, self.n = x.shape
        self.x = _dev(x)
        self.ws = torch.empty(hip.workspace_bytes(self.n, 1, 1, self.d) // 8 + 1, dtype=torch.float64, device="cuda")
        self.st = P(torch.cuda.current_stream().cuda_stream)
        self.first_len = _lib.MomentLayout(self.d).first_len

    def _ws(self):
        return _ptr(self.ws), self.ws.numel() * 8, self.st

    @staticmethod
    def _bounds(rows, lo, hi, flags):
        keep = (np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(lo, dtype=np.float64),
                np.ascontiguousarray(hi, dtype=np.float64), np.ascontiguousarray(flags, dtype=np.int32))
        return keep, tuple(P(a.ctypes.data) for a in keep) + (len(keep[0]),)

    def mask_bounds(self, w, rows, lo, hi, flags):
        wd, changed = _dev(w), np.full(1, -1, dtype=np.int64)
        keep, args = self._bounds(rows, lo, hi, flags)
        self.hip.call("obe_mask_bounds", _ptr(self.x), self.n, self.n, *args, _ptr(wd), P(changed.ctypes.data), *self._ws())
        return wd.cpu().numpy(), int(changed[0]), wd

    def mask_nonpositive(self, w, aux):
        ad, wd, changed = _dev(aux.reshape(1, -1)), _dev(w), np.full(1, -1, dtype=np.int64)
        rows = np.zeros(1, dtype=np.int32)
        self.hip.call("obe_mask_nonpositive", _ptr(ad), self.n, self.n, P(rows.ctypes.data), 1, _ptr(wd),
                      P(changed.ctypes.data), *self._ws())
        return wd.cpu().numpy(), int(changed[0])

    def moments(self, wd):
        mom = self.torch.zeros(self.hip.moments_len(self.d), dtype=self.torch.float64, device="cuda")
        host = np.zeros(self.hip.moments_len(self.d))
        self.hip.call("obe_moments", _ptr(self.x), self.n, self.d, self.n, _ptr(wd), 0, _ptr(mom), P(host.ctypes.data),
                      *self._ws())
        return mom.cpu().numpy()[:self.first_len], host[:self.first_len]

    def _armed_call(self, name, w, *args, partials=None):
        """One of the *_moments calls: nothing is waited for by the call, the words it arms are waited for here."""
        lib = self._lib
        wd = w if isinstance(w, self.torch.Tensor) else _dev(w)
        mom = self.torch.zeros(self.hip.moments_len(self.d), dtype=self.torch.float64, device="cuda")
        h_mom, h_changed = lib.pinned_array(self.first_len), lib.pinned_array(1, np.int64)
        head = (_ptr(self.x), self.n, self.d, self.n)
        self.hip.call(name, *head, *args, _ptr(wd), _ptr(mom), lib.host_ptr(h_mom), lib.host_ptr(h_changed), *self._ws())
        self.hip.call("obe_host_words_wait", lib.host_ptr(h_mom), self.first_len, self.st)
        self.hip.call("obe_host_word_wait", lib.host_ptr(h_changed), self.st)
        return wd.cpu().numpy(), mom.cpu().numpy()[:self.first_len], np.array(h_mom[:]), int(h_changed[0])

    def mask_bounds_moments(self, w, rows, lo, hi, flags):
        keep, args = self._bounds(rows, lo, hi, flags)
        return self._armed_call("obe_mask_bounds_moments", w, *args)

    def mask_nonpositive_moments(self, w, rows):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        return self._armed_call("obe_mask_nonpositive_moments", w, P(rows.ctypes.data), len(rows))

    def mask_renorm_moments(self, wd, partials):
        return self._armed_call("obe_mask_renorm_moments", wd, _ptr(partials))


# ------------------------------------------------------------------------------------------ 1. at the C ABI
SPECIAL = (0.0, -0.0, 5e-324, -5e-324, np.nan, INF, -INF)


def _entries(g, d, kind):
    """(rows, lower, upper, open flags) of one call.  kind: 'one' = one row, both ends inclusive; 'all' = every row
    (32 of them on a wider cloud), the ends inclusive, exclusive and absent in turn; 'dup32' = 32 entries over the
    rows of a narrower cloud (several per row: they intersect), the first of them an inclusive 0; 'point' = lower ==
    upper, inclusive; 'zero' = one row >= 0, inclusive (the lock-in hook's ``< 0``: -0.0 stays, -5e-324 goes)."""
    if kind == "zero":
        return np.array([d // 2]), np.array([0.0]), np.array([INF]), np.array([0])
    if kind == "one":
        return np.array([g.integers(d)]), np.array([-0.25]), np.array([0.5]), np.array([0])
    if kind == "point":
        return np.array([d - 1]), np.array([0.125]), np.array([0.125]), np.array([0])
    rows = np.arange(min(d, 32)) if kind == "all" else np.arange(32) % d
    k = np.arange(rows.size)
    lo = np.where(k % 3 == 2, -INF, -1.0 - 0.125 * (k % 5))
    hi = np.where(k % 4 == 3, INF, 1.0 + 0.125 * (k % 7))
    if kind == "all" and rows.size > 1:
        lo[1] = 0.0                                        # ... and a bound of 0, for the signed zeros and subnormals
    flags = ((k % 2 == 1) & np.isfinite(lo)) * 1 + ((k % 5 >= 3) & np.isfinite(hi)) * 2
    if kind == "dup32":
        lo[0], flags[0] = 0.0, flags[0] & 2                # an inclusive 0
    return rows, lo, hi, flags


def _cloud(g, base, rows, lo, hi):
    """Random values that violate now and then, and — where the cloud is large enough — values exactly on every
    bound, on its two neighbours, +-0, the smallest subnormals, NaN and +-inf in the bounded rows."""
    x = base.copy()
    d, n = x.shape
    if n >= 255:
        col = 0
        for r, a, b in zip(rows, lo, hi):
            for v in [a, np.nextafter(a, INF), np.nextafter(a, -INF), b, np.nextafter(b, INF), np.nextafter(b, -INF)] \
                    + list(SPECIAL):
                x[r, col % n] = v
                col += 3
    w = g.random(n) * (g.random(n) > 0.1)                  # general values and zeros
    w[0] = 0.5
    return x, w / w.sum()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000, 2 ** 19 + 3])
@pytest.mark.parametrize("d", [1, 3, 16, 17, 40])
def test_mask_bounds_is_the_oracle_and_the_existing_mask(hip, n, d):
    g = np.random.default_rng(1000 * d + n % 997)
    base = g.normal(0.0, 0.9, (d, n))
    for kind in ("one", "zero", "all", "point") + (("dup32",) if d < 32 else ()):
        rows, lo, hi, flags = _entries(g, d, kind)
        x, w = _cloud(g, base, rows, lo, hi)
        if kind == "zero" and n >= 255:                    # (the signed zeros stay, the negative subnormal goes)
            r = rows[0]
            special = np.isin(x[r], (0.0, 5e-324, -5e-324))
            assert_array_equal(co.violators(x[rows], lo, hi, [False], [False])[special], x[r][special] < 0)
            assert np.any(np.signbit(x[r][special]) & (x[r][special] == 0)) and np.any(x[r][special] == -5e-324)
        if kind == "point" and n > 3:
            x[d - 1, ::3] = 0.125
        # the oracle, entry by entry (the rows of the gathered cloud are the entries)
        bad = co.violators(x[rows], lo, hi, (flags & 1) != 0, (flags & 2) != 0)
        want, count = co.apply_bounds(x[rows], w, lo, hi, (flags & 1) != 0, (flags & 2) != 0)
        abi = Abi(hip, x)
        got, changed, wd = abi.mask_bounds(w, rows, lo, hi, flags)
        what = f"n={n} d={d} {kind}"
        assert changed == count == int(bad.sum()), what
        assert_array_equal(got == 0.0, want == 0.0, err_msg=what)
        # the survivors: the bits of the existing mask on a one-row cloud that is -1 where the oracle says violator
        ref, ref_changed = abi.mask_nonpositive(w, np.where(bad, -1.0, 1.0))
        assert ref_changed == count
        _same_bits(got, ref, what)
        if count == 0:
            _same_bits(got, w, what + ": nothing violates, the weights are untouched")
        elif count < n:
            np.testing.assert_allclose(got, want, rtol=1e-13, err_msg=what)        # (another order of the sum)
        # mask + first moments in two launches = the mask, then obe_moments(want_cov = 0)
        mom_dev, mom_host = abi.moments(wd)
        w2, mom2_dev, mom2_host, changed2 = abi.mask_bounds_moments(w, rows, lo, hi, flags)
        assert changed2 == count, what
        _same_bits(w2, got, what + ": weights of the _moments form")
        _same_bits(mom2_dev, mom_dev, what + ": K3 first-moment block on the device")
        _same_bits(mom2_host, mom_host, what + ": K3 first-moment block on the host")


def test_nothing_violates_leaves_the_weights_untouched(hip):
    g = np.random.default_rng(3)
    x = g.normal(0.0, 1.0, (3, 5000))
    w = g.random(5000)                                      # (not normalised: a renormalisation would show)
    abi = Abi(hip, x)
    got, changed, _ = abi.mask_bounds(w, [0, 2], [-50.0, -INF], [INF, 50.0], [1, 2])
    assert changed == 0
    _same_bits(got, w, "weights")
    w2, _, _, changed2 = abi.mask_bounds_moments(w, [0, 2], [-50.0, -INF], [INF, 50.0], [1, 2])
    assert changed2 == 0
    _same_bits(w2, w, "weights of the _moments form")


def test_every_particle_violates_gives_nan_weights(hip):
    g = np.random.default_rng(4)
    n = 257
    x = g.normal(0.0, 1.0, (3, n))
    w = np.full(n, 1.0 / n)
    abi = Abi(hip, x)
    got, changed, _ = abi.mask_bounds(w, [1], [100.0], [INF], [0])
    assert changed == n and np.all(np.isnan(got))
    w2, _, _, changed2 = abi.mask_bounds_moments(w, [1], [100.0], [INF], [0])
    assert changed2 == n and np.all(np.isnan(w2))


# ----------------------------------------------------------------------------------------- 2. new against old
@pytest.mark.parametrize("d", [4, 10])
def test_positive_noise_rows_through_the_new_entry_points_are_the_old_bits(hip, d):
    import torch
    n = 4099
    g = np.random.default_rng(d)
    x = g.normal(0.3, 0.4, (d, n))
    x[d - 1, ::50] = 0.0
    x[d - 2, 7::60] = -0.0
    w = g.random(n)
    w /= w.sum()
    abi = Abi(hip, x)
    for rows in ([d - 1], [d - 2, d - 1]):
        k = len(rows)
        old = abi.mask_nonpositive_moments(w, rows)
        new = abi.mask_bounds_moments(w, rows, [0.0] * k, [INF] * k, [1] * k)
        assert old[3] == new[3] > 0
        for a, b, what in zip(old[:3], new[:3], ("weights", "moments (device)", "moments (host)")):
            _same_bits(a, b, what)
        # the gathers: the same new cloud, weights and partial sums; then the shared second half
        idx = _dev(g.integers(0, n, n))
        z = _dev(g.standard_normal(n * d))
        aos = _dev(x.T.copy())
        factor, mean = np.ascontiguousarray(g.normal(0, 0.05, (d, d))), np.ascontiguousarray(x.mean(axis=1))
        out = []
        r32 = np.array(rows, dtype=np.int32)
        keep, bargs = Abi._bounds(rows, [0.0] * k, [INF] * k, [1] * k)
        for name, cargs in (("obe_resample_particles_aos_masked", (P(r32.ctypes.data), k)),
                            ("obe_resample_particles_aos_bounded", bargs)):
            new_x = torch.zeros((d, n), dtype=torch.float64, device="cuda")
            wd = torch.zeros(n, dtype=torch.float64, device="cuda")
            partials = torch.zeros(2 * 2048, dtype=torch.float64, device="cuda")
            hip.call(name, _ptr(aos), d, n, _ptr(idx), _ptr(z), P(factor.ctypes.data), P(mean.ctypes.data), 0.98, 1,
                     _ptr(new_x), n, _ptr(wd), *cargs, _ptr(partials), abi.st)
            gathered = Abi(hip, new_x.cpu().numpy())
            out.append((new_x.cpu().numpy(), wd.cpu().numpy().copy(), partials.cpu().numpy())
                       + gathered.mask_renorm_moments(wd, partials))
        assert out[0][6] == out[1][6] > 0
        assert out[0][6] == int(np.sum(np.any(out[0][0][rows] <= 0.0, axis=0)))
        for a, b, what in zip(out[0][:6], out[1][:6], ("new cloud", "masked weights", "partial sums", "weights",
                                                        "moments (device)", "moments (host)")):
            _same_bits(a, b, what)


@pytest.fixture(scope="module")
def parent_bits():
    with open(os.path.join(ROOT, "tests", "golden", "constraint_parent_bits.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_sigma_positive_entry_points_leave_the_parent_commits_bits(hip, parent_bits, case):
    """obe_mask_nonpositive, obe_mask_nonpositive_moments and obe_resample_particles_aos_masked (+ obe_mask_renorm_moments
    on its partial sums) are the bounds calls with (0, +inf) on their rows: the comparisons above send one
    implementation through two doors.  The independent pin is the fixture, recorded by the last commit that had a
    sigma <= 0 kernel and a row-bitmask gather of their own (tests/_constraint_cases.py): counts, first moments on the
    device and on the host, and the hashes of the weights, the new cloud and the partial sums, item by item."""
    want = parent_bits[cc.case_id(case)]
    got = cc.run(hip, case)
    assert got["inputs"] == want["inputs"], "inputs differ: the case generator no longer makes the recorded arrays"
    cc.check_condition(case, got)
    assert sorted(got) == sorted(want)
    for call in sorted(set(got) - {"inputs"}):
        assert sorted(got[call]) == sorted(want[call]), call
        for item in sorted(got[call]):
            assert got[call][item] == want[call][item], f"{cc.case_id(case)}: {call}: {item}"


def test_bounded_gather_is_the_oracle_on_any_rows(hip):
    """Bounds the old gather cannot express (an upper end, an inclusive 0, two entries for one row), D = 16 and 3:
    the zeroed particles are the oracle's on the NEW cloud, the survivors carry 1/N, the partial sums are the mask
    kernel's on that cloud."""
    import torch
    for d, n in ((16, 4099), (3, 257)):
        g = np.random.default_rng(d)
        x = g.normal(0.0, 1.0, (d, n))
        rows, lo, hi, flags = _entries(g, d, "dup32")
        idx, z, aos = _dev(g.integers(0, n, n)), _dev(g.standard_normal(n * d)), _dev(x.T.copy())
        factor, mean = np.ascontiguousarray(g.normal(0, 0.05, (d, d))), np.zeros(d)
        new_x = torch.zeros((d, n), dtype=torch.float64, device="cuda")
        wd = torch.zeros(n, dtype=torch.float64, device="cuda")
        partials = torch.zeros(2 * 2048, dtype=torch.float64, device="cuda")
        keep, bargs = Abi._bounds(rows, lo, hi, flags)
        st = P(torch.cuda.current_stream().cuda_stream)
        hip.call("obe_resample_particles_aos_bounded", _ptr(aos), d, n, _ptr(idx), _ptr(z), P(factor.ctypes.data),
                 P(mean.ctypes.data), 0.98, 0, _ptr(new_x), n, _ptr(wd), *bargs, _ptr(partials), st)
        nx, w = new_x.cpu().numpy(), wd.cpu().numpy()
        bad = co.violators(nx[rows], lo, hi, (flags & 1) != 0, (flags & 2) != 0)
        assert 0 < bad.sum() < n
        assert_array_equal(w, np.where(bad, 0.0, 1.0 / n))
        abi = Abi(hip, nx)
        got = abi.mask_renorm_moments(wd, partials)
        ref = abi.mask_bounds_moments(np.full(n, 1.0 / n), rows, lo, hi, flags)
        assert got[3] == ref[3] == int(bad.sum())
        for a, b, what in zip(got[:3], ref[:3], ("weights", "moments (device)", "moments (host)")):
            _same_bits(a, b, f"d={d}: {what}")


# ------------------------------------------------------------------------------------------ 3. gather fusion
def _spied(o, names):
    used, o_lib = [], o._lib
    call = o_lib.call

    class Spy:
        def __getattr__(self, name):
            return getattr(o_lib, name)

        def call(self, name, *a):
            if name in names:
                used.append(name)
            return call(name, *a)
    o._lib = Spy()
    return used


ROUTES = ("obe_mask_renorm_moments", "obe_mask_bounds_moments", "obe_resample_particles_aos_bounded",
          "obe_mask_nonpositive_moments", "obe_resample_particles_aos_masked")


@pytest.mark.parametrize("noise_param", [False, True])
def test_the_bounds_inside_the_gather_are_the_bounds_after_it(obe, noise_param):
    """25 cycles (variance_full) with the bounds applied by the gather of the reported resample and with
    tuning_parameters['mask_in_gather'] = False: particles, weights, moments, counts, settings, generator bit for bit;
    and with the sweep enqueued ahead (speculative_sweep True) against never (False)."""
    from test_gpu_speculative import cycles, make, same
    logs, routes = {}, {}
    for mode, flag in (("auto", True), ("auto", False), (True, True), (False, True)):
        o = make(obe, mode, n_particles=70000, n_settings=1500, noise_param=noise_param, threshold=0.9)
        o.tuning_parameters["mask_in_gather"] = flag
        o.set_parameter_bounds({0: (None, 3.5), 2: (0.4, None)}, inclusive={2: False})     # (the true b is 0.4)
        used = _spied(o, ROUTES)
        log = cycles(o, 25, between=lambda obj, c: np.array([obj.last_constraint_count], dtype=np.float64))
        logs[mode, flag], routes[mode, flag] = log, set(used)
        assert sum(e["resampled"] for e in log) >= 5 and sum(e["between"][0] > 0 for e in log) >= 3
        assert not np.any(np.isnan(log[-1]["w"]))
    def fresh(log):          # (same() takes kappa out of the entries it is given)
        return [dict(e, sweep=dict(e["sweep"])) for e in log]
    for key in (("auto", False), (True, True), (False, True)):
        same(fresh(logs["auto", True]), fresh(logs[key]))
    fused = {"obe_mask_renorm_moments", "obe_resample_particles_aos_bounded"}
    assert routes["auto", True] >= fused and routes[True, True] >= fused and routes[False, True] >= fused
    assert routes["auto", False] == {"obe_mask_bounds_moments"}
    assert not any("nonpositive" in r or r.endswith("_masked") for rs in routes.values() for r in rs)
    # outside pdf_update() nothing follows the resample: uniform weights, as the reference's resample() leaves them
    o = make(obe, False, n_particles=70000, n_settings=300, noise_param=noise_param)
    o.set_parameter_bounds({2: (0.4, None)})
    o.resample()
    w = o.particle_weights
    assert np.all(w == 1.0 / w.size)


def test_one_rank_of_a_sharded_object_applies_the_same_mask(obe):
    """A settings-sharded object's replicas each apply the bounds to their own copy of the cloud — a deterministic
    mask, no collective: one rank of a sharded object goes through the cycles of the unsharded object bit for bit,
    counts included, and its replica check stays green.  (One process: a world of one rank.)"""
    from optbayesexpt_amd.dist import SettingsShard
    from test_gpu_speculative import cycles, make, same
    logs = []
    for shard in (None, SettingsShard(0, 1)):
        o = make(obe, "auto", n_particles=70000, n_settings=1500, noise_param=True, threshold=0.9, shard=shard)
        o.tuning_parameters["replica_check_every"] = 1
        o.set_parameter_bounds({0: (None, 3.5), 2: (0.4, None)}, inclusive={2: False})
        logs.append(cycles(o, 12, between=lambda obj, c: np.array([obj.last_constraint_count], dtype=np.float64)))
        assert o.check_replicas() is True
    assert sum(e["resampled"] for e in logs[0]) >= 3 and max(e["between"][0] for e in logs[0]) > 0
    same(*logs)


def test_noise_parameter_object_without_bounds_makes_todays_calls(obe):
    from test_gpu_speculative import cycles, make
    o = make(obe, "auto", n_particles=70000, n_settings=300, noise_param=True, threshold=0.9)
    used = _spied(o, ROUTES)
    assert o.parameter_bounds is None
    log = cycles(o, 8)
    assert any(e["resampled"] for e in log)
    assert set(used) == {"obe_mask_renorm_moments", "obe_resample_particles_aos_masked"}
    base = make(obe, "auto", n_particles=70000, n_settings=300, threshold=0.9)
    used = _spied(base, ROUTES)
    log = cycles(base, 8)
    assert any(e["resampled"] for e in log) and not used and base.last_constraint_count == 0


# --------------------------------------------------------------------------- 4. trajectory against the oracle
def _coil_pair(obe, prior_seed):
    g = np.random.default_rng(prior_seed)
    n = 2048
    L, R = g.uniform(0.9, 1.1, n), g.uniform(0.0, 0.12, n)
    C, sigma = g.uniform(0.9, 1.1, n), g.exponential(0.3, n)
    prior = np.array([L, R, C, sigma])
    sv = (np.logspace(-1, 1, 60),)
    a = obe.OptBayesExptNoiseParameter(obe.models.coil(), sv, prior.copy(), (), noise_parameter_index=(3, 3), scale=False)
    b = oracle.OracleOptBayesExptNoiseParameter(omodels.coil, sv, prior.copy(), (), noise_parameter_index=(3, 3),
                                                scale=False)
    a.rng, b.rng = np.random.default_rng(101), np.random.default_rng(101)
    bounds = {0: (None, 1.0), 1: (0.0, None), 2: (0.995, 1.02)}
    a.set_parameter_bounds(bounds)
    counts = []
    co.install_hook(b, *co.full(4, {**bounds, 3: (0.0, None)}, lower_open=[3]), counts=counts)     # + sigma > 0
    return a, b, counts


def test_coil_trajectory_with_bounds_against_the_oracle(obe):
    """30 cycles of the 2-channel coil model with an unknown noise level, L <= 1, R >= 0, 0.995 <= C <= 1.02 and the
    class's sigma > 0: the oracle class carries the same mask as a NumPy hook.  Setting index, draw and resample
    indices, resample flag and constraint count exact in every cycle; weights, moments and utility to the replay
    helpers' tolerances at the coil trajectory's HIP_RTOL.  (The oracle alone, on the CPU: 10 resamples that zero
    2017, 16, 55, 24, 14, 3, 28, 1, 1, 0 particles.)"""
    rtol = _replay.HIP_RTOL["coil_2ch_noise"]
    a, b, counts = _coil_pair(obe, 1)
    meas = np.random.default_rng(201)
    true = (1.0, 0.03, 1.0, 0.3)
    zeroed = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for cyc in range(30):
            xa, xb = a.opt_setting(), b.opt_setting()
            assert_array_equal(a.last_draw_indices, b.last_draw_indices, err_msg=f"draw indices, cycle {cyc}")
            _replay.close(a._utility_dev.cpu().numpy(), np.asarray(b.last_utility).reshape(-1), rtol, f"utility, cycle {cyc}")
            assert a.last_setting_index == b.last_setting_index, f"setting index, cycle {cyc}"
            y = tuple(omodels.coil(xb, true, ()).reshape(-1) + meas.normal(0.0, 0.3, 2))
            a.pdf_update((xa, y))
            b.pdf_update((xb, y))
            assert bool(a.just_resampled) == bool(b.just_resampled), f"resample flag, cycle {cyc}"
            if b.just_resampled:
                assert_array_equal(a.last_resample_indices_device.cpu().numpy(), b.last_draw_indices,
                                   err_msg=f"resample indices, cycle {cyc}")
                assert a.last_constraint_count == counts[-1], f"constraint count, cycle {cyc}"
                zeroed.append(counts[-1])
            wa, wb = a.particle_weights, b.particle_weights
            assert_array_equal(wa == 0.0, wb == 0.0, err_msg=f"zero weights, cycle {cyc}")
            _replay.close_weights(wa, wb, rtol, f"weights, cycle {cyc}")
            mean, sd = b.mean(), b.std()
            assert np.all(np.abs(a.mean() - mean) <= rtol * (np.abs(mean) + sd)), f"mean, cycle {cyc}"
            tol = rtol * sd + 64 * 2.3e-16 * mean ** 2 / np.maximum(sd, 1e-300)
            assert np.all(np.abs(a.std() - sd) <= tol), f"std, cycle {cyc}"
    print("particles zeroed per resample:", zeroed)
    assert len(zeroed) == len(counts)
    assert sum(c > 0 for c in zeroed) >= 4 and max(zeroed) < a.n_particles


# -------------------------------------------------------------------------------- 5. smaller class-level checks
def _lorentz_pair(obe, n=5000, **kw):
    g = np.random.default_rng(17)
    prior = np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    sv = (np.linspace(1.5, 4.5, 300),)
    a = obe.OptBayesExpt(obe.models.lorentzian(), sv, prior.copy(), (0.1,), scale=False, resample_threshold=0.7, **kw)
    b = oracle.OracleOptBayesExpt(omodels.lorentzian, sv, prior.copy(), (0.1,), scale=False, resample_threshold=0.7)
    a.rng, b.rng = np.random.default_rng(1), np.random.default_rng(1)
    return a, b


LORENTZ_TRUE = (3.0, -1000.0, 50000.0)


def _lorentz_cycles(objs, n_cycles, seed=9):
    sim = np.random.default_rng(seed)
    log = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for _ in range(n_cycles):
            xs = [o.opt_setting() for o in objs]
            y = float(omodels.lorentzian(xs[0], LORENTZ_TRUE, (0.1,))) + 500.0 * sim.standard_normal()
            for o, x in zip(objs, xs):
                o.pdf_update((x, y, 500.0))
            log.append([(int(o.last_setting_index), bool(o.just_resampled)) for o in objs])
    return log


def test_base_class_with_a_bound_against_the_oracle(obe):
    """The base class, x0 >= its true value (about half of every resampled cloud violates), N = 5000."""
    a, b = _lorentz_pair(obe)
    a.set_parameter_bounds({0: (LORENTZ_TRUE[0], None)})
    counts = []
    co.install_hook(b, *co.full(3, {0: (LORENTZ_TRUE[0], None)}), counts=counts)
    seen = 0
    sim = np.random.default_rng(9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for cyc in range(25):
            xa, xb = a.opt_setting(), b.opt_setting()
            assert a.last_setting_index == b.last_setting_index, cyc
            y = float(omodels.lorentzian(xb, LORENTZ_TRUE, (0.1,))) + 500.0 * sim.standard_normal()
            a.pdf_update((xa, y, 500.0))
            b.pdf_update((xb, y, 500.0))
            assert bool(a.just_resampled) == bool(b.just_resampled), cyc
            if b.just_resampled:
                seen += 1
                assert a.last_constraint_count == counts[-1] > 0, cyc
                assert np.all(a.particles[0][a.particle_weights > 0] >= LORENTZ_TRUE[0])
            assert_array_equal(a.particle_weights == 0.0, b.particle_weights == 0.0)
            _replay.close_weights(a.particle_weights, b.particle_weights, 1e-10, f"weights, cycle {cyc}")
            assert np.all(np.abs(a.mean() - b.mean()) <= 1e-10 * (np.abs(b.mean()) + b.std())), cyc
    assert seen >= 3
    a.set_parameter_bounds(None)
    assert a.parameter_bounds is None


def test_an_overriding_hook_that_calls_super_gets_the_device_mask(obe):
    calls = []

    class Mine(obe.OptBayesExpt):
        def enforce_parameter_constraints(self):
            calls.append(self.just_resampled)
            super().enforce_parameter_constraints()

    g = np.random.default_rng(17)
    n = 5000
    prior = np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    sv = (np.linspace(1.5, 4.5, 300),)
    objs = [cls(obe.models.lorentzian(), sv, prior.copy(), (0.1,), scale=False, resample_threshold=0.7)
            for cls in (obe.OptBayesExpt, Mine)]
    for o in objs:
        o.rng = np.random.default_rng(1)
        o.set_parameter_bounds({0: (LORENTZ_TRUE[0], None)})
    log = _lorentz_cycles(objs, 20)
    assert all(x == y for x, y in log) and sum(r for (_, r), _ in log) == len(calls) >= 3
    _same_bits(objs[0].particle_weights, objs[1].particle_weights, "weights")
    _same_bits(objs[0].particles, objs[1].particles, "particles")
    assert objs[0].last_constraint_count == objs[1].last_constraint_count > 0


def test_deepcopy_and_pickle_carry_the_bounds(obe):
    a, _ = _lorentz_pair(obe)
    a.set_parameter_bounds({0: (LORENTZ_TRUE[0], None), 1: (-2500.0, 0.0)}, inclusive={1: (True, False)})
    _lorentz_cycles([a], 6)
    for b in (copy.deepcopy(a), pickle.loads(pickle.dumps(a))):
        for x, y in zip(a.parameter_bounds, b.parameter_bounds):
            assert_array_equal(x, y)
        assert b.last_constraint_count == a.last_constraint_count
        twin = copy.deepcopy(a)
        log = _lorentz_cycles([twin, b], 12, seed=3)
        assert all(x == y for x, y in log) and any(r for (_, r), _ in log)
        _same_bits(twin.particle_weights, b.particle_weights, "weights")
        _same_bits(twin.particles, b.particles, "particles")
        assert twin.last_constraint_count == b.last_constraint_count > 0


def test_saved_object_continues_in_a_fresh_process_with_its_bounds(obe, tmp_path):
    a, _ = _lorentz_pair(obe)
    a.set_parameter_bounds({0: (LORENTZ_TRUE[0], None)}, inclusive=False)
    _lorentz_cycles([a], 6)
    path = str(tmp_path / "bounded.obe")
    obe.save(a, path)
    log = _lorentz_cycles([a], 12, seed=3)
    assert any(r for ((_, r),) in log)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_constraint_child.py"), path, path + ".out"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(path + ".out", "rb") as f:
        child = pickle.load(f)
    assert child["log"] == log
    for x, y in zip(a.parameter_bounds, child["bounds"]):
        assert_array_equal(x, y)
    _same_bits(a.particle_weights, child["w"], "weights")
    _same_bits(a.particles, child["p"], "particles")
    assert a.last_constraint_count == child["count"] > 0
    # a file written before there were bounds loads with none
    from optbayesexpt_amd import _state
    st = _state.snapshot(a)
    del st["parameter_bounds"]
    assert _state.restore(st).parameter_bounds is None


def test_a_sweeper_object_with_bounds_reports_its_count(obe):
    fx = _replay.load_traj("sweeper_opt")
    ctor = dict(fx["meta"]["ctor"])
    o = obe.OptBayesExptSweeper(obe.models.lorentzian(), (fx["setval_0"],), fx["prior"].copy(), tuple(fx["cons"]), **ctor)
    o.rng = np.random.default_rng(5)
    o.set_parameter_bounds({0: (3.1, None)})
    x = fx["setval_0"]
    sim = np.random.default_rng(6)
    total, resamples = 0, 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for _ in range(6):
            pa = o.opt_setting()
            xs = x[pa[0]:pa[1]]
            ys = omodels.lorentzian((xs,), (3.1, 1200.0, 300.0), (0.1,)) + 800.0 * sim.standard_normal(len(xs))
            o.pdf_update(((xs,), ys))
            if o.just_resampled:
                resamples += 1
                total += o.last_constraint_count
                w, p = o.particle_weights, o.particles
                assert np.all(p[0][w > 0] >= 3.1) and np.all(p[o._noise_rows[0]][w > 0] > 0)
    assert total > 0


def test_the_stale_alias_takes_the_mask_alone_on_those_rows(obe):
    """set_pdf() between updates leaves ``parameters`` the OLD samples (obe_base.py:185, 395): the constraint then
    looks at those rows, as the reference's hook would, and the noise class does."""
    a, _ = _lorentz_pair(obe)
    a.set_parameter_bounds({0: (3.0, None)})
    old = a.particles.copy()
    g = np.random.default_rng(2)
    a.set_pdf(np.array([g.uniform(3.5, 4, 5000), g.uniform(-2000, -400, 5000), g.normal(50000, 1000, 5000)]))
    assert a._parameters is not a._particles
    w0 = a.particle_weights.copy()
    used = _spied(a, ("obe_mask_bounds", "obe_mask_bounds_moments"))
    a.enforce_parameter_constraints()
    want, count = co.apply_bounds(old, w0, *co.full(3, {0: (3.0, None)}))
    assert used == ["obe_mask_bounds"] and a.last_constraint_count == count > 0
    assert_array_equal(a.particle_weights == 0.0, want == 0.0)
    np.testing.assert_allclose(a.particle_weights, want, rtol=1e-13)


def test_a_cloud_wider_than_the_fused_kernels_takes_the_unfused_mask(obe):
    g = np.random.default_rng(5)
    n, d = 5000, 17
    prior = np.vstack([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n), g.normal(0, 1, (d - 3, n))])
    sv = (np.linspace(1.5, 4.5, 100),)
    a = obe.OptBayesExpt(obe.models.lorentzian(), sv, prior.copy(), (0.1,), scale=False, resample_threshold=0.7)
    a.rng = np.random.default_rng(1)
    a.set_parameter_bounds({0: (LORENTZ_TRUE[0], None), 16: (None, 0.5)})
    used = _spied(a, ROUTES + ("obe_mask_bounds",))
    seen = 0
    sim = np.random.default_rng(9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for _ in range(15):
            x = a.opt_setting()
            y = float(omodels.lorentzian(x, LORENTZ_TRUE, (0.1,))) + 500.0 * sim.standard_normal()
            a.pdf_update((x, y, 500.0))
            if a.just_resampled:
                seen += 1
                p, w = a.particles, a.particle_weights
                want, count = co.apply_bounds(p, np.full(n, 1.0 / n), *co.full(d, {0: (3.0, None), 16: (None, 0.5)}))
                assert a.last_constraint_count == count > 0
                assert_array_equal(w == 0.0, want == 0.0)
                np.testing.assert_allclose(w, want, rtol=1e-13)
                np.testing.assert_allclose(a.mean(), oracle.weighted_mean(p, w), rtol=1e-12)     # computed when asked for
    assert seen >= 2 and set(used) == {"obe_mask_bounds"}


def test_a_host_callable_model_gets_the_same_device_mask(obe):
    a, _ = _lorentz_pair(obe)
    g = np.random.default_rng(17)
    n = 5000
    prior = np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    h = obe.OptBayesExpt(omodels.lorentzian, (np.linspace(1.5, 4.5, 300),), prior, (0.1,), scale=False,
                         resample_threshold=0.7)
    h.rng = np.random.default_rng(1)
    assert h._device_model is None
    for o in (a, h):
        o.set_parameter_bounds({0: (LORENTZ_TRUE[0], None)})
    used = _spied(h, ROUTES)
    log = _lorentz_cycles([a, h], 12)
    assert all(x == y for x, y in log) and any(r for (_, r), _ in log)
    assert set(used) <= {"obe_mask_bounds_moments", "obe_mask_renorm_moments", "obe_resample_particles_aos_bounded"} and used
    assert_array_equal(a.particle_weights == 0.0, h.particle_weights == 0.0)
    assert a.last_constraint_count == h.last_constraint_count > 0


def test_the_example_script_runs(obe):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import bounded_parameters
    finally:
        sys.path.pop(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        true, means, stds, zeroed = bounded_parameters.main(n_measure=40, n_samples=20000, quiet=True)
    assert np.all(np.isfinite(means)) and np.all(means[:3] >= 0) and means[3] > 0 and zeroed >= 0
