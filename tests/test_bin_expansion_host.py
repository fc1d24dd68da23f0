"""The bin form of the one-peak Lorentzian's unshifted sweep (include/obe_hip.h: OBE_SWEEP_BINS), on the host: a
NumPy statement of the scheme of csrc/obe_models.h (LorentzBins) in the summation order of the kernels of
csrc/obe_sweep_bins.h — the draws grouped stably by bin, items of 1024 draws summed lane by lane and by a butterfly,
the items of a bin folded by 16 strided groups, each series from the highest order down, the bins in order, C1 and
C2 last — against a long-double two-pass variance, and the decisions of obe_sweep_bins_plan().  No GPU.

The clouds are those of the accuracy table of DESIGN.md ("K1 by bin expansions"): 100 000 particles with random
weights; 256 settings over 30 d (the table's 2 048 cost a minute of long-double arithmetic per cloud and meet the
same bins)."""
import numpy as np
import pytest

from optbayesexpt_amd import _lib

RHO = 1.0 / _lib.OBE_CELL_RHO_INV
P = _lib.OBE_CELL_ORDER
WIDTH = 2.0 * RHO
ITEM, LANES, GROUPS = 1024, 64, 16          # csrc/obe_sweep_bins.h: kBinChunk, kBinFoldGroups; obe_common.h: kWave


def item_sums(terms):
    """terms (n <= ITEM, m): lane l adds its draws l, l + 64, ... in order, then the butterfly over the lanes."""
    n, m = terms.shape
    padded = np.zeros((ITEM, m))
    padded[:n] = terms                          # (a draw that is not there adds an exact zero)
    trips = padded.reshape(ITEM // LANES, LANES, m)
    lanes = np.zeros((LANES, m))
    for t in trips:
        lanes = lanes + t
    o = LANES // 2
    while o:
        lanes = lanes + lanes[np.arange(LANES) ^ o]
        o //= 2
    return lanes[0]


def fold_items(parts):
    """parts (items, m): group g adds the items g, g + 16, ... in order, the groups are added in order."""
    acc = np.zeros((GROUPS, parts.shape[1]))
    for k, row in enumerate(parts):
        acc[k % GROUPS] = acc[k % GROUPS] + row
    total = acc[0]
    for g in range(1, GROUPS):
        total = total + acc[g]
    return total


def bin_variance(x, cloud, w, d):
    """The per-setting variance by bin expansions, then the unshifted one-pass formula of sweep_finalize.
    Returns (variance, number of occupied bins)."""
    x0, a, b = cloud
    tau, tau0 = x / d, x0 / d
    W = np.sum(w)
    bp = b - np.sum(w * b) / W
    origin = tau0.min()
    nbins = int(np.floor((tau0.max() - origin) * (1.0 / WIDTH))) + 1
    assert nbins <= _lib.OBE_BIN_MAX
    idx = np.minimum(((tau0 - origin) * (1.0 / WIDTH)).astype(np.int64), nbins - 1)
    order = np.argsort(idx, kind="stable")
    wa, wab2, waa = w * a, 2.0 * w * a * bp, w * a * a
    s1, s2 = np.zeros_like(tau), np.zeros_like(tau)
    C1 = C2 = 0.0
    occupied = 0
    for bin_ in range(nbins):
        sel = order[idx[order] == bin_]
        if sel.size == 0:
            continue
        occupied += 1
        tb = origin + (bin_ + 0.5) * WIDTH
        eps = tau0[sel] - tb
        assert np.all(np.abs(eps) <= RHO * (1.0 + 1e-9))
        powers = np.empty((sel.size, P))
        e = np.ones(sel.size)
        for k in range(P):
            powers[:, k] = e
            e = e * eps
        terms = np.concatenate([wa[sel, None] * powers, wab2[sel, None] * powers, waa[sel, None] * powers,
                                (w[sel] * bp[sel])[:, None], (w[sel] * bp[sel] ** 2)[:, None]], axis=1)
        parts = np.array([item_sums(terms[i:i + ITEM]) for i in range(0, sel.size, ITEM)])
        parts[:, 2 * P:3 * P] *= np.arange(1, P + 1)              # H3_k = (k + 1) M3_k, per item
        row = fold_items(parts)
        M1, M2, H3 = row[:P], row[P:2 * P], row[2 * P:3 * P]
        # r_k(s), g_k(s) by the three-term recurrences, s = tau_b - tau
        s = tb - tau
        r0 = 1.0 / (s * s + 1.0)
        B = -r0
        A = (s + s) * B
        r, g = [r0], [r0 * r0]
        Brp, Bgp = np.zeros_like(s), np.zeros_like(s)
        for k in range(P - 1):
            m_k = k * (k + 3.0) / ((k + 1.0) * (k + 2.0))
            rn, gn = A * r[k] + Brp, A * g[k] + m_k * Bgp
            Brp, Bgp = B * r[k], B * g[k]
            r.append(rn)
            g.append(gn)
        t1, t2 = np.zeros_like(s), np.zeros_like(s)
        for k in range(P - 1, -1, -1):
            t1 = M1[k] * r[k] + t1
            t2 = M2[k] * r[k] + t2
            t2 = H3[k] * g[k] + t2
        s1, s2 = s1 + t1, s2 + t2
        C1, C2 = C1 + row[3 * P], C2 + row[3 * P + 1]
    s1, s2 = s1 + C1, s2 + C2
    return (s2 - s1 * (s1 / W)) / W, occupied


def reference(x, cloud, w, d):
    """Long-double two-pass variance, and the cancellation factor kappa of the unshifted one-pass form."""
    L = np.longdouble
    x0, a, b = (v.astype(L) for v in cloud)
    w = w.astype(L)
    W = np.sum(w)
    bbar = np.sum(w * b) / W
    out, kappa = np.empty(x.size, dtype=L), np.empty(x.size)
    for i, xi in enumerate(x):
        t = (L(xi) - x0) / L(d)
        y = b + a / (t * t + 1)
        m = np.sum(w * y) / W
        out[i] = np.sum(w * (y - m) ** 2) / W
        kappa[i] = float((m - bbar) ** 2 / out[i])
    return out, kappa


def _clouds(n=100000, ns=256):
    g = np.random.default_rng(2025)
    z = g.normal(size=(3, n))
    w = g.exponential(1.0, n)
    w /= w.sum()
    x = np.linspace(1.5, 4.5, ns)

    def converged(b_spread):
        return np.array([3.0 + 0.001 * z[0], -1000.0 + 15.0 * z[1], 50000.0 + b_spread * z[2]])
    prior = np.array([g.uniform(2, 4, n), g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    narrow = np.array([3.0 + 0.05 * z[0], g.uniform(-2000, -400, n), g.normal(50000, 1000, n)])
    # d = 1/8: x0 / d and every bin edge (half-width 1/4) are exact, so these x0 ARE the edges
    edges = np.array([(16.0 + 0.5 * g.integers(0, 17, n)) * 0.125, g.uniform(-2000, -400, n),
                      g.normal(50000, 1000, n)])
    return {"c3's prior": (x, prior, w, 0.1),
            "x0 sigma 0.5 d": (x, narrow, w, 0.1),
            "converged, b-spread 0": (x, converged(0.0), w, 0.1),
            "converged, b-spread 8": (x, converged(8.0), w, 0.1),
            "x0 on the bin edges": (np.linspace(1.5, 4.5, ns), edges, w, 0.125)}


CLOUDS = _clouds()


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_bin_variance_against_long_double(name):
    """err <= min(2e-11, 1e-14 max(kappa, 4)): 2e-11 is what the unshifted direct form is held to below KAPPA_LEAVE
    (tests/test_gpu_units.py::test_unshifted_sweep_accuracy_below_the_kappa_threshold), 1e-14 kappa the one-pass
    formula's own loss.  A NumPy model with pairwise per-bin sums measured 3.9e-15 (prior), 3.3e-14 (sigma 0.5 d),
    4.0e-12 and 2.4e-12 (converged) against it."""
    x, cloud, w, d = CLOUDS[name]
    ref, kappa = reference(x, cloud, w, d)
    got, occupied = bin_variance(x, cloud, w, d)
    err = float(np.max(np.abs(got - ref) / ref))
    bound = min(2e-11, 1e-14 * max(float(kappa.max()), 4.0))
    print(f"{name}: {occupied} occupied bins, kappa max {kappa.max():.3g}, error {err:.2e}, bound {bound:.2e}")
    assert err <= bound


def test_plan_helper_decisions():
    plan = _lib.load().cdll.obe_sweep_bins_plan
    valid, worthwhile = 1, 2
    D = 0.1
    assert plan(1.5, 4.5, D, 65536, 1048576) == valid | worthwhile          # c3 (replaces the cells)
    assert plan(1.5, 4.5, D, 4096, 262144) == valid | worthwhile            # c2 (replaces the direct kernel)
    assert plan(1.5, 4.5, D, 201, 5000) == valid                            # c1
    assert plan(1.5, 4.5, D, 4099, 300) == valid                            # a sweep of 300 draws
    for d in (0.0, -D, float("nan"), float("inf")):
        assert plan(1.5, 4.5, d, 65536, 1048576) == 0
    assert plan(1.5, float("inf"), D, 65536, 1048576) == 0
    assert plan(float("nan"), 4.5, D, 65536, 1048576) == 0
