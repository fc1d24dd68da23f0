"""References for K2, the Bayes update of the particle weights (csrc/obe_update.h, obe_update.hip,
obe_update_common.hip), NumPy and the standard library only.  tests/test_update_oracle_host.py pins them on the CPU
(fractions.Fraction, mpmath at 50 digits, NumPy) and shows that the inputs of the GPU file tell a wrong kernel from a
right one; tests/test_gpu_update_exact.py compares the device with them at the C ABI.

The update (include/obe_hip.h):  L = prod_ch exp(-((y - y_meas) / s)^2 / 2) / s  [L = L^choke],
t = nan_to_num(w L),  w' = nan_to_num(t / sum t),  h_out = [sum t, sum nan_to_num(w'^2)].

(a) EXACT UPDATE CLOUDS.  Weights q 2^-k (q from _moments_oracle.exact_cloud), likelihoods 2^j (j = 0 ... 6) or 0
("dead" particles), q topped up on the live particles of the smallest j so that sum q 2^j over the live particles is
exactly 2^m.  Then t = q 2^(j - k), sum t = 2^(m - k), w' = q 2^(j - m) and sum w'^2 = sum (q 2^j)^2 2^(-2 m) are
exact in ANY order of additions (the integer sum of squares is asserted below 2^53), so weights and both sums are
defined bit for bit for every grid, every fold and the np.sum order alike.  Every entry point can realise the same
cloud: the likelihood form directly; the y and model forms with sigma = 2^-j from a particle row (or one sigma for
all), a model value equal to the reading on the live particles (z = 0, exp(-0.0) = 1) and at least 1 off with sigma
2^-6 on the dead ones (z^2 / 2 >= 2048: exp underflows to exactly 0).

(b) GENERAL DOUBLES.  likelihood_ld / posterior_ld in np.longdouble, and likelihood_bound: value by value, how far a
kernel that follows the documented arithmetic of likelihood_of may be from it.  Nothing in it is fitted; the only
numbers not derivable on paper are the accuracy of the device's exp and pow in units of u = 2^-53 RELATIVE
(a correctly rounded function has 1, a "1 ulp" function up to 2):

    measured on an MI355X (tests/test_gpu_update_exact.py::test_libm_accuracy_measured prints them):
        exp  on 777 arguments -a, a = fl(fl(z z) / 2) from 0 to 800:  worst 1.013 u
        pow  on 2^j, j = -300 ... 300, exponents 0.6 and 1.7:         worst 1.812 u
    LIBM_EXP_ULPS = LIBM_POW_ULPS = 3: each rounded up to the next integer, plus one; neither may exceed 4 (the "few ulp"
    tests/_ziggurat_oracle.py already assumes of any exp) — a larger value is a finding, not a constant to adopt.

(c) SPECIAL VALUES at one workgroup on dyadic data (order independent): the expectation is the NumPy expression of
particlepdf.py:136-139 in float64.
(d) resample_due: the resample test of csrc/obe_update.h in float64.
"""
import functools
import math

import numpy as np

import _moments_oracle as mo

LD = np.longdouble
U = 2.0 ** -53                      # unit roundoff of float64
U_REF = mo.U_REF                    # one ulp of 1.0 in long double, taken whole
TREE_DEPTH = mo.TREE_DEPTH          # additions a term of a device sum passes through, rounded up (n <= 65 536)
TINY = 2.0 ** -1074                 # the smallest subnormal: what one rounding into the subnormal range can lose
DBL_MAX = float(np.finfo(np.float64).max)
MEASURED_EXP_U = 1.013              # MI355X, see above
MEASURED_POW_U = 1.812
LIBM_EXP_ULPS = 3
LIBM_POW_ULPS = 3
assert LIBM_EXP_ULPS == math.ceil(MEASURED_EXP_U) + 1 <= 4 and LIBM_POW_ULPS == math.ceil(MEASURED_POW_U) + 1 <= 4
J_MAX = 6


# ----------------------------------------------------------------------------------------- (a) exact update clouds
class ExactCloud:
    """q, k, j, dead, m of one exact update cloud (see the module docstring) and what the update must leave."""

    def __init__(self, q, k, j, dead, m):
        self.q, self.k, self.j, self.dead, self.m = q, k, j, dead, m
        self.n = len(q)
        live = ~dead
        units = np.where(live, q << j, 0)                      # q 2^j in int64
        assert np.all(units[live] > 0), "every live particle moves sum t"
        assert int(units.sum()) == 1 << m
        self.sum_squares = sum(int(v) ** 2 for v in units.tolist())
        assert self.sum_squares < 1 << 53, "sum (q 2^j)^2 is exact in any order"
        assert int(q.max()) < 1 << 53 and int(q.min()) > 0     # q 2^-k is exact
        self.units = units

    def prior(self):
        """w = q 2^-k (not normalised: the update does not ask for that)."""
        return np.ldexp(self.q.astype(np.float64), -self.k)

    def lik(self):
        return np.where(self.dead, 0.0, np.ldexp(1.0, self.j))

    def posterior(self, shift=0):
        """(w', sum t, sum w'^2) when every likelihood carries the common factor 2^shift."""
        w1 = np.ldexp(self.units.astype(np.float64), -self.m)
        return w1, math.ldexp(1.0, self.m - self.k + shift), math.ldexp(float(self.sum_squares), -2 * self.m)


def exact_update_cloud(g, n, j_fixed=None, dead_share=0.2):
    """An ExactCloud of n particles.  j_fixed: every likelihood exponent the same (the fixed-sigma form; J_MAX so
    that the one sigma also kills the dead particles)."""
    _, q, k = mo.exact_cloud(g, 1, n)
    q = np.maximum(q, 1)                                       # (exact_cloud's centre particle may carry 0)
    j_low = 0 if j_fixed is None else int(j_fixed)
    j = g.integers(0, J_MAX + 1, size=n) if j_fixed is None else np.full(n, j_low, dtype=np.int64)
    dead = g.random(n) < dead_share
    j[dead] = J_MAX                                            # (what sigma a dead particle is given: 2^-6)
    anchor = int(g.integers(0, n))                             # at least one live particle to top up
    dead[anchor], j[anchor] = False, j_low
    live = ~dead
    s = int((q[live] << j[live]).sum())
    m = (s - 1).bit_length()
    rest = (1 << m) - s
    assert rest >= 0 and rest % (1 << j_low) == 0
    top = np.flatnonzero(live & (j == j_low))
    each, extra = divmod(rest >> j_low, len(top))              # spread over all of them, not parked on one
    q[top] += each
    q[top[:extra]] += 1
    return ExactCloud(q, k, j, dead, m)


def _deviation(g, dead):
    """0 on the live particles, an integer of magnitude 1 ... 4 on the dead ones."""
    n = len(dead)
    return np.where(dead, g.integers(1, 5, size=n) * g.choice([-1, 1], size=n), 0).astype(np.float64)


def exact_y_problem(g, cloud, n_channels, n_lik, rows):
    """The cloud as a supplied-y update: dict(y (C, n), y_meas (n_lik,), sigma (n_lik,) or None, particles (R, n) and
    noise_rows (n_lik,) or None, shift).  One channel carries sigma = 2^-j (rows: from a particle row; fixed sigma:
    the cloud's one j); the others sigma = 2^-c, c drawn per channel (rows: a constant row).  shift = sum c.  Channels
    beyond n_lik hold NaN: they must not enter."""
    n = cloud.n
    y_meas = g.integers(-1000, 1001, size=n_lik).astype(np.float64)
    y = np.full((n_channels, n), np.nan)
    y[:n_lik] = y_meas[:, None]
    ch = int(g.integers(0, n_lik))
    y[ch] += _deviation(g, cloud.dead)
    c = g.integers(0, J_MAX + 1, size=n_lik)
    c[ch] = 0
    out = dict(y=y, y_meas=y_meas, sigma=None, particles=None, noise_rows=None, shift=int(c.sum()))
    if rows:
        r = n_lik + 2
        p = g.integers(-512, 513, size=(r, n)).astype(np.float64)
        noise_rows = g.permutation(r)[:n_lik].astype(np.int32)
        for i in range(n_lik):
            p[noise_rows[i]] = np.ldexp(1.0, -cloud.j) if i == ch else math.ldexp(1.0, -int(c[i]))
        out.update(particles=p, noise_rows=noise_rows)
    else:
        assert np.all(cloud.j == cloud.j[0]), "one sigma for all: a fixed-j cloud"
        sigma = np.ldexp(1.0, -c).astype(np.float64)
        sigma[ch] = math.ldexp(1.0, -int(cloud.j[0]))
        out.update(sigma=sigma)                                # (the cloud's 2^j is already in its likelihood)
    return out


def exact_model_problem(g, cloud, model, d, noise_row):
    """The cloud as a model-fused update with a built-in model of integer arithmetic: 'line_ab' (y = p0 + p1 x) or
    'first_param' (y = p0); d rows (the model's, the noise row holding 2^-j when noise_row is not None, spare integer
    rows).  dict(particles (d, n), setting, y_meas, sigma or None, noise_rows or None, shift)."""
    n = cloud.n
    p = g.integers(-512, 513, size=(d, n)).astype(np.float64)
    y_meas = float(g.integers(-64, 65))
    xs = float(g.integers(-8, 9))
    dev = _deviation(g, cloud.dead)
    if model == "line_ab":
        p[1] = g.integers(-16, 17, size=n)
        p[0] = y_meas - p[1] * xs + dev                        # integers below 2^10: exact, and so is p0 + p1 x
        assert noise_row is None or noise_row >= 2
    else:
        assert model == "first_param" and (noise_row is None or noise_row >= 1)
        p[0] = y_meas + dev
    out = dict(particles=p, setting=xs, y_meas=y_meas, sigma=None, noise_rows=None, shift=0)
    if noise_row is None:
        assert np.all(cloud.j == cloud.j[0])
        out.update(sigma=math.ldexp(1.0, -int(cloud.j[0])))
    else:
        p[noise_row] = np.ldexp(1.0, -cloud.j)
        out["noise_rows"] = np.array([noise_row], dtype=np.int32)
    return out


# --------------------------------------------------------------------------------------------- (b) general doubles
def _sigmas(sig, n_lik, n):
    sig = np.asarray(sig, dtype=np.float64)
    return np.broadcast_to(sig[:n_lik, None] if sig.ndim == 1 else sig[:n_lik], (n_lik, n))


def exp_arguments(y, y_meas, sig, n_lik):
    """(a, s), float64 (n_lik, n): a = fl(fl(z z) / 2) with z = fl(fl(y - y_meas) / s) — the device's argument of exp,
    bit for bit (IEEE operations, no contraction on either side; the negation is exact)."""
    y = np.asarray(y, dtype=np.float64)[:n_lik]
    s = _sigmas(sig, n_lik, y.shape[1])
    ym = np.asarray(y_meas, dtype=np.float64)[:n_lik, None]
    with np.errstate(all="ignore"):
        z = (y - ym) / s
        a = (z * z) / 2.0
    return a, s


def likelihood_ld(y, y_meas, sig, n_lik, choke=None):
    """The likelihood in long double from the float64 arguments of exp: prod_ch exp(-a_ch) / s_ch, then ^choke.
    `sig`: n_lik fixed sigmas, or (n_lik, n) per-particle sigmas (the noise rows, gathered by the caller).  NaN where
    the arithmetic has one (a negative product under a choke)."""
    a, s = exp_arguments(y, y_meas, sig, n_lik)
    with np.errstate(all="ignore"):
        lik = np.prod(np.exp(-a.astype(LD)) / s.astype(LD), axis=0)
        if choke is not None:
            lik = lik ** LD(choke)
    return lik


def likelihood_bound(y, y_meas, sig, n_lik, choke=None):
    """Per particle, how far the device's likelihood may be from likelihood_ld.  Long double array (NaN where the
    reference is NaN: the device must have one there too).

    The argument a_c of exp is the device's, bit for bit (exp_arguments).  Per channel the device then forms
    fl(exp(-a_c)), fl(e / s) and fl(lk * that): relative errors LIBM_EXP_ULPS u, u and u, so with C channels
        |L^ - L| <= ((1 + (LIBM_EXP_ULPS + 2) u)^C - 1) |L|
    (a record wider than 8 channels multiplies group products: still one product rounding per channel).  A value that
    enters the subnormal range loses up to 2^-1074 absolutely at each of these roundings instead, and that error is
    then scaled by the factors still to come: at most C (LIBM_EXP_ULPS + 2) 2^-1074 max(1, max_c 1/|s_c|)
    prod_c max(1, |f_c|), f_c = exp(-a_c) / s_c.  The sum of the two is b.
    With a choke kappa > 0 the device forms pow(L^, kappa), pow good to LIBM_POW_ULPS u: x^kappa is monotone, so
        |pow(L^, kappa) - L^kappa| <= max((|L| + b)^kappa - |L|^kappa, |L|^kappa - max(|L| - b, 0)^kappa)
                                      + LIBM_POW_ULPS u (|L| + b)^kappa + LIBM_POW_ULPS 2^-1074
    — to first order kappa (b / L) + LIBM_POW_ULPS u relative, and the right statement where L underflows.
    The reference's own error (3 long double operations per channel, one power) is added as (3 C + 2) U_REF."""
    a, s = exp_arguments(y, y_meas, sig, n_lik)
    with np.errstate(all="ignore"):
        f = np.abs(np.exp(-a.astype(LD)) / s.astype(LD))
        lik = np.prod(f, axis=0)
        per = (LIBM_EXP_ULPS + 2) * U
        rel = (1 + LD(per)) ** n_lik - 1 + (3 * n_lik + 2) * U_REF
        scale = np.maximum(1, (1 / np.abs(s.astype(LD))).max(axis=0)) * np.prod(np.maximum(1, f), axis=0)
        b = rel * lik + n_lik * (LIBM_EXP_ULPS + 2) * LD(TINY) * scale
        if choke is None:
            return b
        ref = likelihood_ld(y, y_meas, sig, n_lik, choke)
        kappa = LD(choke)
        hi, mid, lo = (lik + b) ** kappa, lik ** kappa, np.maximum(lik - b, 0) ** kappa
        out = np.maximum(hi - mid, mid - lo) + (LIBM_POW_ULPS * U + 2 * U_REF) * hi + LIBM_POW_ULPS * LD(TINY)
        return np.where(np.isnan(ref), LD(np.nan), out)


def fraction_of_bound(got, ref, bound):
    """|got - ref| / bound per value (float64); 0 where they agree exactly or both are NaN, inf where only one is NaN
    or where the bound is 0 and they differ."""
    got, ref, bound = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD), np.asarray(bound, dtype=LD)
    both_nan = np.isnan(got) & np.isnan(ref)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        frac = np.where((err == 0) | both_nan, 0.0, err / bound)
        return np.where(np.isnan(frac), np.inf, frac).astype(np.float64)


def nan_to_num_ld(v):
    v = np.asarray(v, dtype=LD).copy()
    v[np.isnan(v)] = 0
    return np.clip(v, -LD(DBL_MAX), LD(DBL_MAX))


def posterior_ld(w, lik):
    """(w', sum t) in long double: t = nan_to_num(w lik), w' = nan_to_num(t / sum t)."""
    with np.errstate(all="ignore"):
        t = nan_to_num_ld(np.asarray(w, dtype=LD) * np.asarray(lik, dtype=LD))
        total = t.sum()
        return nan_to_num_ld(t / total), total


def sum_t_bound(w, lik_ref, lik_bound):
    """How far the device's sum t may be from posterior_ld's: every t_i carries its likelihood's bound times |w_i|,
    and the rounding of the product w L and of the additions it passes through — TREE_DEPTH u |t_i| (Higham 4.2; at
    most 65 536 particles: one per thread) — plus the reference's own 256 U_REF sum |t|."""
    with np.errstate(all="ignore"):
        w = np.abs(np.asarray(w, dtype=LD))
        t = np.abs(nan_to_num_ld(w * np.asarray(lik_ref, dtype=LD)))
        b = np.where(np.isnan(lik_bound), 0, lik_bound)
        return float((w * b + t * (mo._gamma(TREE_DEPTH) + 256 * U_REF)).sum())


# the general cases of tests/test_gpu_update_exact.py, section B: (channels, n_lik, rows, choke)
GENERAL_N = 777
GENERAL_CASES = [(c, n_lik, rows, choke)
                 for c in (1, 2, 8, 9, 16, 17) for n_lik in sorted({c, max(1, c - 1 - c // 4)})
                 for rows in (False, True) for choke in (None, 0.6, 1.7)]
# the case that isolates exp (one channel, sigma = 1, no choke) and the ones that isolate pow
EXP_CASE = "exp"
POW_CASES = (("pow", 0.6), ("pow", 1.7))
SPECIAL_COLUMNS = (0, 255, 256, GENERAL_N - 1)                 # z = 0 there: they carry the sum


def general_case(case, n=GENERAL_N):
    """dict(y (C, n), y_meas, sigma or None, particles / noise_rows or None, sig (what likelihood_ld takes), n_lik,
    choke, w) of one case: the same arrays wherever they are asked for.  Readings of magnitude up to 1e6, sigmas over
    four decades (rows: distinct per channel and per particle), z = (y - y_meas) / s of norm 0 ... 40 over the
    channels (exactly 0 on the SPECIAL_COLUMNS, 40 in one channel on particle 1), channels beyond n_lik holding
    values that would change the product.  Rows with >= 2 channels: particles 5 and 6 have two negative sigmas (a
    positive product of negative factors), particle 7 one (a negative product: NaN under a choke)."""
    if case == EXP_CASE:
        g = np.random.default_rng(424242)
        z = np.linspace(0.0, 40.0, n)[g.permutation(n)]
        y = (7.0 + z)[None]
        return dict(y=y, y_meas=np.array([7.0]), sigma=np.array([1.0]), particles=None, noise_rows=None,
                    sig=np.array([1.0]), n_lik=1, choke=None, w=np.ones(n))
    if isinstance(case, tuple) and case[0] == "pow":
        g = np.random.default_rng(434343)
        p = np.ldexp(1.0, g.integers(-300, 301, size=n))[None]       # sigma = 2^-j: L = 2^j exactly
        return dict(y=np.full((1, n), 3.0), y_meas=np.array([3.0]), sigma=None, particles=p,
                    noise_rows=np.array([0], dtype=np.int32), sig=p, n_lik=1, choke=case[1], w=np.ones(n))
    c, n_lik, rows, choke = case
    g = np.random.default_rng([c, n_lik, int(rows), 0 if choke is None else int(10 * choke)])
    y_meas = 10.0 ** g.uniform(0, 6, size=n_lik) * g.choice([-1, 1], size=n_lik)
    scale = 10.0 ** g.uniform(-2, 2, size=c)
    out = dict(n_lik=n_lik, choke=choke, y_meas=y_meas, sigma=None, particles=None, noise_rows=None)
    if rows:
        r = c + 2
        p = scale.mean() * (0.5 + g.random((r, n)))            # (any row read by mistake is a plausible sigma)
        noise_rows = g.permutation(r)[:n_lik].astype(np.int32)
        p[noise_rows] = scale[:n_lik, None] * (1.0 + 0.5 * g.random((n_lik, n)))
        if n_lik >= 2:
            p[noise_rows[0], 5:8] *= -1.0
            p[noise_rows[1], 5:7] *= -1.0
        sig = p[noise_rows]
        out.update(particles=p, noise_rows=noise_rows, sig=sig)
    else:
        sig = scale[:n_lik]
        out.update(sigma=sig.copy(), sig=sig)
    radius = 40.0 * g.random(n)
    radius[list(SPECIAL_COLUMNS)] = 0.0
    v = g.standard_normal((n_lik, n))
    v /= np.sqrt((v * v).sum(axis=0))
    radius[1], v[:, 1] = 40.0, 0.0
    v[0, 1] = 1.0
    y = np.empty((c, n))
    y[:n_lik] = y_meas[:, None] + radius * v * _sigmas(sig, n_lik, n)
    y[n_lik:] = 0.3 * g.standard_normal((c - n_lik, n))
    w = 10.0 ** (-12.0 * g.random(n) ** 3)
    w[5:8] = 0.0                                               # (the particles of negative sigma stay out of the posterior)
    # ... and so do the particles beyond z = 36: with up to 8 sigmas of up to 150 their likelihood can be subnormal
    # in float64, where it has lost digits that a choke below 1 then moves into a weight of ordinary size
    w[radius > 36.0] = 0.0
    out.update(y=y, w=w / w.sum())
    return out


def likelihood_mutants(case):
    """name -> likelihood (long double) of likelihood_ld with one plausible kernel mistake built in, for the mistakes
    that apply to the case.  tests/test_update_oracle_host.py requires each to leave likelihood_bound on at least one
    particle of every case it applies to."""
    p = general_case(case)
    y, ym, sig, n_lik, choke = p["y"], p["y_meas"], p["sig"], p["n_lik"], p["choke"]
    n = y.shape[1]
    a, s = exp_arguments(y, ym, sig, n_lik)
    e, sl = np.exp(-a.astype(LD)), s.astype(LD)

    def finish(lik):
        with np.errstate(all="ignore"):
            return lik if choke is None else lik ** LD(choke)

    out = {}
    with np.errstate(all="ignore"):
        out["a float32 exponent"] = finish(np.prod(np.exp(-a.astype(np.float32).astype(LD)) / sl, axis=0))
        if n_lik >= 2:
            out["sigma[0] used for every channel"] = likelihood_ld(y, ym, np.repeat(_sigmas(sig, n_lik, n)[:1], n_lik, axis=0),
                                                                   n_lik, choke)
            out["1/s omitted after channel 0"] = finish(np.prod(e, axis=0) / sl[0])
            if choke is not None and p["noise_rows"] is not None:
                out["the choke applied per channel"] = np.prod((e / sl) ** LD(choke), axis=0)
        if n_lik < y.shape[0]:
            extra = np.exp(-(y[n_lik:].astype(LD) ** 2) / 2)   # y_meas = 0, sigma = 1: what LikArgs holds beyond n_lik
            out["n_lik_channels ignored"] = finish(np.prod(e / sl, axis=0) * np.prod(extra, axis=0))
        if p["noise_rows"] is not None:
            rows = (p["noise_rows"] + 1) % p["particles"].shape[0]
            out["a noise row off by one"] = likelihood_ld(y, ym, p["particles"][rows], n_lik, choke)
    return out


# the exact clouds of tests/test_gpu_update_exact.py, section A
EXACT_SMALL = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
EXACT_GRID = (65535, 65536, 65537, 131071, 131072, 131073, 196607, 196608, 196609, 393217)
STRICT_SIZES = (257, 8193, 196609)


@functools.lru_cache(maxsize=None)
def exact_case(n, fixed=False):
    """The exact cloud of n particles (fixed: one likelihood exponent for all): the same wherever it is asked for."""
    return exact_update_cloud(np.random.default_rng(9000 + 2 * n + int(fixed)), n, J_MAX if fixed else None)


# ----------------------------------------------------------------------------------------------- (c) special values
def posterior_np(w, lik):
    """particlepdf.py:136-139 and :243-244 in float64: (w', sum t, sum nan_to_num(w'^2))."""
    with np.errstate(all="ignore"):
        t = np.nan_to_num(np.asarray(w, dtype=np.float64) * np.asarray(lik, dtype=np.float64))
        total = np.sum(t)
        w1 = np.nan_to_num(t / total)
        return w1, float(total), float(np.sum(np.nan_to_num(w1 * w1)))


def posterior_without_nan_to_num_on_t(w, lik):
    """The mutant: t = w lik as it comes."""
    with np.errstate(all="ignore"):
        t = np.asarray(w, dtype=np.float64) * np.asarray(lik, dtype=np.float64)
        total = np.sum(t)
        w1 = np.nan_to_num(t / total)
        return w1, float(total), float(np.sum(np.nan_to_num(w1 * w1)))


SPECIAL_N = 200                     # one workgroup


def special_cases():
    """name -> (w, j, dead, needs_nan_to_num): weights with the special value planted, likelihood 2^j or 0 (dead).
    The special particles are ADDED to an exact cloud at random places, so that sum t stays the power of two (or the
    DBL_MAX, the infinity, the zero) that makes every quotient and every sum exact: NumPy's order and the device's
    then give the same bits."""
    g = np.random.default_rng(5150)
    n = SPECIAL_N
    base = exact_update_cloud(g, n - 2)
    out = {}

    def planted(w_extra, j_extra, dead_extra, w=None, j=None, dead=None):
        at = np.sort(g.integers(0, n - 1, size=2))
        w = base.prior() if w is None else w
        return (np.insert(w, at, w_extra), np.insert(base.j if j is None else j, at, j_extra),
                np.insert(base.dead if dead is None else dead, at, dead_extra))

    zero = 0.0                                                 # (the second added particle, where one is enough)
    out["one NaN weight"] = planted([np.nan, zero], [3, 0], [False, True]) + (True,)
    out["w = inf with L = 0"] = planted([np.inf, zero], [2, 0], [True, True]) + (True,)
    tiny = np.ldexp(base.q.astype(np.float64), -40)
    out["one t = DBL_MAX among tiny others"] = planted([DBL_MAX, zero], [0, 0], [False, True], w=tiny,
                                                       j=np.zeros(n - 2, dtype=np.int64)) + (False,)
    out["two infinities"] = planted([np.inf, np.inf], [0, 4], [False, False]) + (False,)    # (inf / inf is 0 too)
    out["every likelihood zero"] = planted([0.25, 0.5], [1, 2], [True, True], dead=np.ones(n - 2, dtype=bool)) + (False,)
    x = math.ldexp(37.0, -base.k)
    out["a negative weight"] = planted([-x, x], [2, 2], [False, False]) + (False,)     # (sum t is unchanged)
    return out


def special_lik(j, dead):
    return np.where(dead, 0.0, np.ldexp(1.0, j))


# ------------------------------------------------------------------------------------------------ (d) resample test
def resample_due(sum_w2, n_particles, threshold):
    """csrc/obe_update.h: n_eff = 1 / sum_w2;  n_eff < 0.1 N  or  n_eff / N < threshold  — in float64."""
    with np.errstate(all="ignore"):
        n = np.float64(n_particles)
        n_eff = np.float64(1.0) / np.float64(sum_w2)
        return bool(n_eff < np.float64(0.1) * n or n_eff / n < np.float64(threshold))
