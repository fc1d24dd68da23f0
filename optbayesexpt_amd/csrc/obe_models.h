// Device model registry: the HIP counterpart of the reference's Python
// `model_function(settings, parameters, constants)` (obe_base.py:50-72).
//
// Each model provides two evaluations of the same formula:
//   eval()      — the exact NumPy operation sequence of the corresponding demo
//                 function, one correctly-rounded op at a time (no FMA contraction);
//                 used by the HBM-bound kernels (Bayes update, eval_over_*), where
//                 it costs nothing and gives reference-identical bits.
//   sweep_eval() — the flop-bound sweep form, for the SPT settings one lane owns at
//                 once: per-setting and per-particle terms are hoisted (prep_setting /
//                 pack), the SPT divisions share ONE v_rcp_f64 + Newton (Montgomery's
//                 batch inversion), and products/sums are fused.  It returns
//                 sqrt(w) * (y - offset): the weight is folded into the packed particle
//                 (one multiply per particle instead of one per evaluation) and the
//                 offset is a particle-independent constant (the mean background),
//                 which leaves the variance unchanged and removes the cancellation.
#pragma once

#include <type_traits>

#include "obe_common.h"

namespace obe {

// 1/q for the root of a batch inversion in the sweep.  v_rcp_f64 seeds 2^-24.4 relative (measured on
// gfx950, tools/microbench_fp64.hip); ONE Newton step  r (1 + e),  e = 1 - q r,  takes that to
// e^2 <= 2^-48.8 = 2e-15.  Every inverse of the batch then carries the same relative error in [-2e-15, 0]:
// the sweep's variances move by <= 4e-15 relative (1e-10 is the parity bar; the random part of the error
// averages down by a further sqrt(N) over the particles).  The step sits on the one narrow dependent chain
// of the group (product tree -> v_rcp_f64 -> correction -> back-substitution), which the wide phases of
// the neighbouring pair have to cover: dropping the third FMA of the cubically convergent form
// r (1 + e + e^2) (2^-73) shortened that chain and took 1.6 % off the c3 sweep (13.75 -> 13.52 ms on one
// box) where the issue slot alone accounts for 0.85 %.  exact_rcp below is the 1-ulp form.
__device__ __forceinline__ double fast_rcp(double q) {
    const double r = __builtin_amdgcn_rcp(q);
    const double e = fma(-q, r, 1.0);
    return fma(r, e, r);
}

// The 1-ulp form, r (1 + e + e^2), where a reciprocal is not shared (N = 1: one setting per lane, i.e. the sweeps
// of at most a few hundred settings, whose time is launch latency): with a handful of draws nothing averages the
// one-sided 2e-15 of fast_rcp down, and at kappa = (mean of y)^2 / var ~ 1e9 (a cloud of 2 particles, 10 draws:
// tools/fuzz_parity.py 300 5, case 185) it showed as 1.7e-10 in one utility value.
__device__ __forceinline__ double exact_rcp(double q) {
    const double r = __builtin_amdgcn_rcp(q);
    const double e = fma(-q, r, 1.0);
    return fma(r, fma(e, e, e), r);
}

// 1/b with IEEE behaviour at the edges (b = 0 -> inf, b = inf -> 0, NaN -> NaN): the raw
// v_rcp_f64 result is returned whenever the correction step produced a NaN.
__device__ __forceinline__ double guarded_rcp(double b) {
    const double r0 = __builtin_amdgcn_rcp(b);
    const double e = fma(-b, r0, 1.0);
    const double r = fma(r0, fma(e, e, e), r0);
    return r == r ? r : r0;
}

// ---- the inversion tree ---------------------------------------------------------------
// Montgomery's batch inversion, 1/leaf[i] for N = 1, 2, 4 or 8 leaves from ONE reciprocal of their product
// (3(N-1) multiplies + 1 rcp instead of N rcp + 4N Newton FMAs), as a balanced tree in heap order: node i has the
// children 2i and 2i + 1, the leaves are the nodes N .. 2N-1 and node 1 is the root.  Every loop is unrolled
// over constant indices, so the arrays are registers.  The batch_* helpers below are this tree with their own
// leaves, root policy (how the root reciprocal is obtained and range-checked) and scale factors.
//   products:  t[N + i] = leaf[i],  t[i] = t[2i] t[2i+1]                (t[1]: the product of all leaves)
template <int N>
__device__ __forceinline__ void tree_products(const double (&leaf)[N], double (&t)[2 * N]) {
    static_assert(N == 1 || N == 2 || N == 4 || N == 8, "inversion tree: 1, 2, 4 or 8 leaves");
#pragma unroll
    for (int i = 0; i < N; ++i) t[N + i] = leaf[i];
#pragma unroll
    for (int w = N / 2; w >= 1; w /= 2)      // level by level towards the root, each level left to right
#pragma unroll
        for (int i = w; i < 2 * w; ++i) t[i] = t[2 * i] * t[2 * i + 1];
}
//   magnitude: the sum of |leaf| in the same tree order (the range checks of the poisoned batches)
template <int N>
__device__ __forceinline__ double tree_magnitude(const double (&t)[2 * N]) {
    double m[2 * N];
#pragma unroll
    for (int i = 0; i < N; ++i) m[N + i] = fabs(t[N + i]);
#pragma unroll
    for (int w = N / 2; w >= 1; w /= 2)
#pragma unroll
        for (int i = w; i < 2 * w; ++i) m[i] = m[2 * i] + m[2 * i + 1];
    return m[1];
}
//   inverses:  u[2i] = u[i] t[2i+1],  u[2i+1] = u[i] t[2i]  from node FROM on;  r[i] = u[N + i]
template <int N, int FROM>
__device__ __forceinline__ void tree_descend(const double (&t)[2 * N], double (&u)[2 * N], double (&r)[N]) {
#pragma unroll
    for (int i = FROM; i < N; ++i) {
        u[2 * i] = u[i] * t[2 * i + 1];
        u[2 * i + 1] = u[i] * t[2 * i];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = u[N + i];
}
//   r[i] = root_inv * t[1] / leaf[i]: root_inv is the (checked, scaled) reciprocal of the root
template <int N>
__device__ __forceinline__ void tree_inverses(const double (&t)[2 * N], double root_inv, double (&r)[N]) {
    double u[2 * N];
    u[1] = root_inv;
    tree_descend<N, 1>(t, u, r);
}
//   ... with one factor per half of the leaves, r[i] = s_lo / leaf[i] (i < N/2), s_hi / leaf[i] (i >= N/2): the
//   factors enter at the top split (two multiplies) instead of once per element afterwards
template <int N>
__device__ __forceinline__ void tree_inverses2(const double (&t)[2 * N], double root_inv, double s_lo, double s_hi,
                                               double (&r)[N]) {
    static_assert(N >= 2, "two halves");
    double u[2 * N];
    u[2] = root_inv * (t[3] * s_lo);
    u[3] = root_inv * (t[2] * s_hi);
    tree_descend<N, 2>(t, u, r);
}
// the pair products q[2h] q[2h+1]: the leaves of the helpers that stop the tree one level early and let the
// caller's FMA multiply by the sibling (sibling_of):  a/q0 = (a / (q0 q1)) * q1
template <int N>
__device__ __forceinline__ void pair_products(const double (&q)[N], double* pp) {
#pragma unroll
    for (int h = 0; h < N / 2; ++h) pp[h] = q[2 * h] * q[2 * h + 1];
}

// r[j] = 1/q[j].  q >= 1 on every direct caller, so the product cannot underflow; it overflows only beyond
// q ~ 1e77.
template <int N>
__device__ __forceinline__ void batch_rcp(const double (&q)[N], double (&r)[N]) {
    if constexpr (N == 1) {
        r[0] = exact_rcp(q[0]);
    } else {
        double t[2 * N];
        tree_products<N>(q, t);
        tree_inverses<N>(t, fast_rcp(t[1]), r);
    }
}

// Two groups that share one reciprocal, each result scaled by its group's factor:
// r[j] = s_lo / q[j] (j < N/2), s_hi / q[j] (j >= N/2).
// (measured and rejected at N = 8: the Newton step applied to the two half inverses instead of the root — one slot
// more, one dependent operation less: +1.6 % at c3, profiles/r03_sweep_accuracy.txt)
template <int N>
__device__ __forceinline__ void batch_rcp_scaled2(const double (&q)[N], double s_lo, double s_hi, double (&r)[N]) {
    double t[2 * N];
    tree_products<N>(q, t);
    tree_inverses2<N>(t, fast_rcp(t[1]), s_lo, s_hi, r);
}

// Batch inversions for generated expression models, whose denominators are not known to be
// >= 1.  Straight-line code: the batch runs over the N/2 pair products and is accepted when
// their magnitudes sum to < 1e30 (no overflow, inf or NaN) and the reciprocal of the whole
// product is < 1e200 in magnitude — then every partial product inside the tree lies in
// (1e-290, 1e120): no zero, no subnormal that would lose bits.  Otherwise the root inverse is
// replaced by NaN, which poisons every result of the batch and, through the moments, the
// variance of the setting: the sweep reports kappa = NaN and the host repeats it with the
// model's sweep_eval_safe() (one guarded IEEE reciprocal per element), so a branch never
// sits in the hot loop.
__device__ __forceinline__ double poison_unless(bool ok, double v) { return ok ? v : __builtin_nan(""); }

// pair inverses ip[h] = s / (q[2h] q[2h+1]); the caller multiplies by the sibling (sibling_of)
template <int N>
__device__ __forceinline__ void batch_div_poisoned(const double (&q)[N], double s, double (&ip)[(N + 1) / 2]) {
    if constexpr (N == 1) {
        ip[0] = s * guarded_rcp(q[0]);
    } else {
        double pp[N / 2], t[N];
        pair_products<N>(q, pp);
        tree_products<N / 2>(pp, t);
        const double inv = fast_rcp(t[1]);
        tree_inverses<N / 2>(t, poison_unless(tree_magnitude<N / 2>(t) < 1e30 && fabs(inv) < 1e200, inv) * s, ip);
    }
}
template <int N>
__device__ __forceinline__ double sibling_of(const double (&q)[N], int j) {
    if constexpr (N == 1) return 1.0;
    else return q[j ^ 1];
}

// Two particles' denominators (N each, N even) through ONE inversion tree: pair inverses
// ipa[h] = sa / (qa[2h] qa[2h+1]), ipb likewise.  The range check is tighter than for one
// particle (sum of |pair products| < 1e18, total inverse < 1e150) because the root spans twice
// as many factors; every partial product then lies in (1e-276, 1e72).
template <int N>
__device__ __forceinline__ void batch_div_poisoned2(const double (&qa)[N], const double (&qb)[N], double sa, double sb,
                                                    double (&ipa)[N / 2], double (&ipb)[N / 2]) {
    double pp[N], t[2 * N], ip[N];
    pair_products<N>(qa, pp);
    pair_products<N>(qb, pp + N / 2);
    tree_products<N>(pp, t);
    const double inv = fast_rcp(t[1]);
    tree_inverses2<N>(t, poison_unless(tree_magnitude<N>(t) < 1e18 && fabs(inv) < 1e150, inv), sa, sb, ip);
#pragma unroll
    for (int h = 0; h < N / 2; ++h) {
        ipa[h] = ip[h];
        ipb[h] = ip[N / 2 + h];
    }
}
template <int N>
__device__ __forceinline__ void batch_rcp_poisoned2(const double (&qa)[N], const double (&qb)[N], double (&ra)[N],
                                                    double (&rb)[N]) {
    double ipa[N / 2], ipb[N / 2];
    batch_div_poisoned2<N>(qa, qb, 1.0, 1.0, ipa, ipb);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        ra[j] = ipa[j / 2] * qa[j ^ 1];
        rb[j] = ipb[j / 2] * qb[j ^ 1];
    }
}

// r[j] = 1 / q[j]
template <int N>
__device__ __forceinline__ void batch_rcp_poisoned(const double (&q)[N], double (&r)[N]) {
    double ip[(N + 1) / 2];
    batch_div_poisoned<N>(q, 1.0, ip);
#pragma unroll
    for (int j = 0; j < N; ++j) r[j] = ip[j / 2] * sibling_of<N>(q, j);
}

// Pair inverses ip[h] = s / (q[2h] q[2h+1]) for denominators known to be >= 1 (products of
// Lorentzian denominators): nothing can underflow, so the only range check is on the root product.
// Beyond 1e250 (where s * inv could leave the normal range) the root inverse is replaced by NaN; the
// NaN reaches the setting's variance, the sweep reports kappa = NaN and the host repeats it with the
// model's sweep_eval_safe().  An inf or NaN product fails the comparison as well.
template <int N>
__device__ __forceinline__ void batch_div_ge1(const double (&q)[N], double s, double (&ip)[(N + 1) / 2]) {
    if constexpr (N == 1) {
        ip[0] = s * exact_rcp(q[0]);
    } else {
        double pp[N / 2], t[N];
        pair_products<N>(q, pp);
        tree_products<N / 2>(pp, t);
        tree_inverses<N / 2>(t, poison_unless(t[1] < 1e250, fast_rcp(t[1])) * s, ip);
    }
}

// sum_{k in [LO, HI)} 1/q[k] as ONE fraction num/den (all q > 0, so num and den are sums and
// products of positive numbers: no cancellation).  (na/da) + (nb/db) = (na db + nb da)/(da db):
// 3 operations per combination, 2 for a leaf pair, 2 for a fraction plus a single term — 2K
// operations for K terms, against the ~3.4 a separate batched inversion costs per term.
template <int LO, int HI>
__device__ __forceinline__ void sum_of_reciprocals(const double* q, double& num, double& den) {
    if constexpr (HI - LO == 1) {
        num = 1.0;
        den = q[LO];
    } else if constexpr (HI - LO == 2) {
        num = q[LO] + q[LO + 1];
        den = q[LO] * q[LO + 1];
    } else if constexpr (HI - LO == 3) {
        const double n2 = q[LO] + q[LO + 1], d2 = q[LO] * q[LO + 1];
        num = fma(n2, q[LO + 2], d2);
        den = d2 * q[LO + 2];
    } else {
        constexpr int MID = LO + (HI - LO + 1) / 2;
        double na, da, nb, db;
        sum_of_reciprocals<LO, MID>(q, na, da);
        sum_of_reciprocals<MID, HI>(q, nb, db);
        num = fma(na, db, nb * da);
        den = da * db;
    }
}

// ---- elementary functions for the inner level of generated sweep forms ----
// The exact forms (Bayes update, eval_over_*, sweep_eval_safe, everything hoisted to the setting
// or particle level) call ocml; the inner level of the flop-bound sweep uses these: accurate to
// ~2 ulp on the ranges stated, NaN outside them — a NaN reaches the setting's variance and the
// host repeats the sweep with the safe twin (OBE_SWEEP_SAFE), as for the batched divisions.

// sin r on |r| <= pi/2 (+1 %): odd Taylor polynomial through r^21 (truncation 2e-18)
__device__ __forceinline__ double sin_poly(double r) {
    const double r2 = r * r;
    double p = 0x1.71b8ef6dcf572p-66;
    p = fma(p, r2, -0x1.2f49b46814157p-57);
    p = fma(p, r2, 0x1.952c77030ad4ap-49);
    p = fma(p, r2, -0x1.ae7f3e733b81fp-41);
    p = fma(p, r2, 0x1.6124613a86d09p-33);
    p = fma(p, r2, -0x1.ae64567f544e4p-26);
    p = fma(p, r2, 0x1.71de3a556c734p-19);
    p = fma(p, r2, -0x1.a01a01a01a01ap-13);
    p = fma(p, r2, 0x1.1111111111111p-7);
    p = fma(p, r2, -0x1.5555555555555p-3);
    return fma(r * r2, p, r);
}
// sin x = (-1)^k sin(x - k pi): two-constant Cody-Waite reduction with FMA (the product k*pi_hi is
// exact inside the FMA, so the reduced argument is good to 1e-16 absolute for |x| < 1e9)
__device__ __forceinline__ double fast_sin(double x) {
    const double k = rint(x * 0x1.45f306dc9c883p-2);
    double r = fma(-k, 0x1.921fb54442d18p+1, x);
    r = fma(-k, 0x1.1a62633145c07p-53, r);
    const double s = sin_poly(r);
    const double v = (static_cast<int>(k) & 1) ? -s : s;
    return fabs(x) < 1e9 ? v : __builtin_nan("");
}
// cos x = sin(x + pi/2)
__device__ __forceinline__ double fast_cos(double x) {
    const double k = rint(fma(x, 0x1.45f306dc9c883p-2, 0.5));
    double r = fma(-k, 0x1.921fb54442d18p+1, x) + 0x1.921fb54442d18p+0;
    r = r + fma(-k, 0x1.1a62633145c07p-53, 0x1.1a62633145c07p-54);
    const double s = sin_poly(r);
    const double v = (static_cast<int>(k) & 1) ? -s : s;
    return fabs(x) < 1e9 ? v : __builtin_nan("");
}
// 1/sqrt(a): v_rsq_f64 (~2^-23) + two Newton steps
__device__ __forceinline__ double fast_rsqrt(double a) {
    double y = __builtin_amdgcn_rsq(a);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double e = fma(-(a * y), y, 1.0);
        y = fma(y * 0.5, e, y);
    }
    return y;
}
// sqrt a = a * fast_rsqrt(a), then one correction of the root.
// 0 -> 0, negative -> NaN, +inf -> NaN (repeat with the safe twin).
__device__ __forceinline__ double fast_sqrt(double a) {
    const double y = fast_rsqrt(a);
    double s = a * y;
    s = fma(fma(-s, s, a), y * 0.5, s);
    return a == 0.0 ? 0.0 : s;
}
// hypot(a, b) with the larger magnitude scaled to [0.5, 1): no overflow / underflow of the squares
__device__ __forceinline__ double fast_hypot(double a, double b) {
    const double m = fmax(fabs(a), fabs(b));
    const int e = __builtin_amdgcn_frexp_exp(m);
    const double a1 = ldexp(a, -e), b1 = ldexp(b, -e);
    const double h = fast_sqrt(fma(a1, a1, b1 * b1));
    return m == 0.0 ? 0.0 : ldexp(h, e);
}

// ---------------------------------------------------------------------------
// y = b + sum_{k<K} a / (((x - x0_k)/d)^2 + 1)
// params: x0_0..x0_{K-1}, a, b [, anything]; const d
// demos/find_peak/sequentialLorentzian.py:53-75 (K = 1)
template <int K>
struct Lorentz {
    static constexpr int NS = 1, NC = 1, NREAD = K + 2, NCONST = 1;
    static constexpr int NXS = 1;        // prepared setting: x/d
    static constexpr int NPK = K + 2;    // packed particle: x0_k/d ..., sw*a, sw*(b - bbar)
    static constexpr int kSweepCost = K; // evaluation time relative to the one-peak model (grid planning)

    __device__ static void eval(const double* x, const ParamRef& th, const obe_model& m, double* y) {
        const double d = m.consts[0];
        const double a = th(K);
        double acc = th(K + 1);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double t = (x[0] - th(k)) / d;
            const double q = t * t + 1.0;
            acc = acc + a / q;
        }
        y[0] = acc;
    }
    __device__ static void prep_setting(const double* x, const obe_model& m, double* xs) {
        xs[0] = x[0] / m.consts[0];
    }
    __device__ static void pack(const ParamRef& th, const double* thbar, const obe_model& m, double sw,
                                double* pk) {
        const double d = m.consts[0];
#pragma unroll
        for (int k = 0; k < K; ++k) pk[k] = th(k) / d;
        pk[K] = sw * th(K);
        pk[K + 1] = sw * (th(K + 1) - thbar[K + 1]);
    }
    // K >= 3: the K peaks of one evaluation are combined into ONE fraction (sum_of_reciprocals,
    // 2K operations) and the SPT fractions of a lane share one reciprocal: a * num/den with the
    // amplitude folded into the pair inverses.  7 peaks: 35 instead of 39.6 FP64 issue slots per
    // evaluation.  The denominators are products of K factors q >= 1, so the inversion tree of 8
    // settings spans q^(8K): it is range-checked (batch_div_ge1, root < 1e250, i.e. |x - x0|/d up
    // to ~170 at K = 7) and a sweep that leaves the range is repeated with sweep_eval_safe() — the
    // peak-by-peak form, good to |x - x0|/d ~ 1e19.
    static constexpr bool kCombinePeaks = K >= 3;
    // Every K has a fast form that poisons a batch whose inversion tree leaves the double range and a SAFE twin
    // that is IEEE for any finite denominator (round 5: K = 1, 2 as well — their fast pair form used to return a
    // NaN variance beyond |x - x0|/d ~ 4e9 with nothing to repeat the sweep with):
    //   fast, K < 3 : two particles x SPT settings of one peak share one reciprocal (q^16).  No range check is
    //                 spent on it: every q >= 1, so the only failure is OVERFLOW of a product, an overflowed root
    //                 is +inf, fast_rcp(+inf) = NaN (0 * inf in its correction step) and the NaN reaches all 16
    //                 results, the setting's variance and kappa — the host repeats the sweep SAFE.  A finite root
    //                 is inverted to >= 50 bits even where 1/root is subnormal.
    //   fast, K >= 3: the combined fraction, range-checked (batch_div_ge1).
    //   SAFE, all K : the pair form per peak with a branch: a batch whose root stays below 1e250 shares its
    //                 reciprocal as before, any other is inverted element by element (guarded_rcp) — the
    //                 reference's numbers for |x - x0|/d up to sqrt(DBL_MAX) ~ 1e154, where t*t itself overflows
    //                 and NumPy, too, gets a / inf = 0.
    static constexpr bool kHasSafeEval = true;
    template <int SPT>
    __device__ __forceinline__ static void sweep_eval(const double (&xs)[SPT][NXS], const double* pk, double sw,
                                                      const obe_model& m, double (&v)[SPT][NC]) {
        if constexpr (!kCombinePeaks) {
            sweep_eval_one<SPT, false>(xs, pk, v);
        } else {
            double num[SPT], den[SPT];
#pragma unroll
            for (int j = 0; j < SPT; ++j) {
                double q[K];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double t = xs[j][0] - pk[k];
                    q[k] = fma(t, t, 1.0);
                }
                sum_of_reciprocals<0, K>(q, num[j], den[j]);
            }
            double ip[(SPT + 1) / 2];
            batch_div_ge1<SPT>(den, pk[K], ip);                       // a / (den[2h] den[2h+1])
#pragma unroll
            for (int j = 0; j < SPT; ++j) v[j][0] = fma(ip[j / 2] * sibling_of<SPT>(den, j), num[j], pk[K + 1]);
        }
    }
    // the peak-by-peak form: one batched inversion per peak (SAFE: range-guarded, see above)
    template <int SPT>
    __device__ __forceinline__ static void sweep_eval_safe(const double (&xs)[SPT][NXS], const double* pk, double,
                                                           const obe_model&, double (&v)[SPT][NC]) {
        sweep_eval_one<SPT, true>(xs, pk, v);
    }
    template <int SPT, bool GUARDED>
    __device__ __forceinline__ static void sweep_eval_one(const double (&xs)[SPT][NXS], const double* pk,
                                                          double (&v)[SPT][NC]) {
#pragma unroll
        for (int j = 0; j < SPT; ++j) v[j][0] = pk[K + 1];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double q[SPT];
#pragma unroll
            for (int j = 0; j < SPT; ++j) {
                const double t = xs[j][0] - pk[k];
                q[j] = fma(t, t, 1.0);
            }
            if constexpr (SPT == 1) {
                // (nothing shared: the IEEE-edged reciprocal in BOTH forms — a lane that owns one setting cannot
                // leave the fast form's range, which is what lets small sweeps go unchecked: models.py,
                // safe_sweep_min_spt)
                v[0][0] = fma(pk[K], guarded_rcp(q[0]), v[0][0]);
            } else {
                // Batch inversion stopped one level early: invert the SPT/2 pair products, fold
                // the amplitude into each pair inverse, and let the final multiply by the sibling
                // be the FMA that accumulates the peak:  a/q0 = (a / (q0 q1)) * q1.
                double pp[SPT / 2], ip[SPT / 2];
                double root = 1.0;
#pragma unroll
                for (int h = 0; h < SPT / 2; ++h) {
                    pp[h] = q[2 * h] * q[2 * h + 1];
                    if constexpr (GUARDED) root *= pp[h];
                }
                if (!GUARDED || root < 1e250) {
                    batch_rcp<SPT / 2>(pp, ip);
#pragma unroll
                    for (int h = 0; h < SPT / 2; ++h) {
                        const double g = pk[K] * ip[h];
                        v[2 * h][0] = fma(g, q[2 * h + 1], v[2 * h][0]);
                        v[2 * h + 1][0] = fma(g, q[2 * h], v[2 * h + 1][0]);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < SPT; ++j) v[j][0] = fma(pk[K], guarded_rcp(q[j]), v[j][0]);
                }
            }
        }
    }
    // Two particles at once: their 2*SPT/2 pair products share ONE reciprocal, and each
    // particle's amplitude enters the inversion tree at its root (2 multiplies per 16 evaluations).
    // The fast form of the peak-by-peak models (a combined fraction already spans q^(8K) per
    // particle) and, range-guarded, the form every SAFE repeat streams its particles through.
    static constexpr bool kHasPairEval = !kCombinePeaks;
    static constexpr bool kSafePairEval = true;
    template <int SPT, bool GUARDED = false>
    __device__ __forceinline__ static void sweep_eval_pair(const double (&xs)[SPT][NXS], const double* pa,
                                                           const double* pb, double (&va)[SPT][NC],
                                                           double (&vb)[SPT][NC]) {
        static_assert(SPT >= 2 && SPT <= 8, "pair evaluation batches SPT pair products");
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            va[j][0] = pa[K + 1];
            vb[j][0] = pb[K + 1];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double qa[SPT], qb[SPT], pp[SPT], ip[SPT];
#pragma unroll
            for (int j = 0; j < SPT; ++j) {
                const double ta = xs[j][0] - pa[k], tb = xs[j][0] - pb[k];
                qa[j] = fma(ta, ta, 1.0);
                qb[j] = fma(tb, tb, 1.0);
            }
            double root = 1.0;
#pragma unroll
            for (int h = 0; h < SPT / 2; ++h) {
                pp[h] = qa[2 * h] * qa[2 * h + 1];
                pp[SPT / 2 + h] = qb[2 * h] * qb[2 * h + 1];
                if constexpr (GUARDED) root *= pp[h] * pp[SPT / 2 + h];
            }
            if (!GUARDED || root < 1e250) {
                batch_rcp_scaled2<SPT>(pp, pa[K], pb[K], ip);      // ip = amplitude / pair product
#pragma unroll
                for (int h = 0; h < SPT / 2; ++h) {
                    const double ga = ip[h], gb = ip[SPT / 2 + h];
                    va[2 * h][0] = fma(ga, qa[2 * h + 1], va[2 * h][0]);
                    va[2 * h + 1][0] = fma(ga, qa[2 * h], va[2 * h + 1][0]);
                    vb[2 * h][0] = fma(gb, qb[2 * h + 1], vb[2 * h][0]);
                    vb[2 * h + 1][0] = fma(gb, qb[2 * h], vb[2 * h + 1][0]);
                }
            } else {        // (SAFE only) this lane's 16 denominators do not fit one product: one by one
#pragma unroll
                for (int j = 0; j < SPT; ++j) {
                    va[j][0] = fma(pa[K], guarded_rcp(qa[j]), va[j][0]);
                    vb[j][0] = fma(pb[K], guarded_rcp(qb[j]), vb[j][0]);
                }
            }
        }
    }
};

// ---- the one-peak Lorentzian's unshifted moments by cell expansions (OBE_SWEEP_CELLS) ----
// With tau = x/d, tau0 = x0/d, b' = b - bbar and r = 1 / ((tau - tau0)^2 + 1), the two moments of a setting are
//   S1(tau) = sum_p w (a r + b'),   S2(tau) = sum_p w (a r + b')^2 = sum_p w a^2 r^2 + 2 w a b' r + w b'^2:
// sums of rational functions of tau whose poles, tau0 +- i, are never closer than 1 to the real axis.  About the
// centre tau_c of a cell of half-width rho < 1 every particle, near or far, has a Taylor series in
// delta = tau - tau_c that converges with ratio <= rho, so the particles need not meet the settings one by one:
// per (cell, particle), with s = tau_c - tau0, q0 = s^2 + 1, B = -1/q0, A = 2 s B,
//   r_0 = 1/q0,   r_{-1} = 0,   r_{k+1} = A r_k + B r_{k-1}                                   (series of r)
//   f_0 = r_0^2,  f_{-1} = 0,   f_{k+1} = (k+2)/(k+1) A f_k + (k+3)/(k+1) B f_{k-1}           (series of r^2)
//   R_k += (w a) r_k,           H_k += (2 w a b') r_k + (w a^2) f_k
// and per setting  S1 = C1 + sum_k R_k delta^k,  S2 = C2 + sum_k H_k delta^k  (Horner), C1 = sum w b',
// C2 = sum w b'^2.  The recurrences are real and three-term: |r_k| <= 1, |f_k| <= k + 1, nothing cancels (the
// 1/(tau - z) moments of the complex form cancel by tau^2) and nothing is inverted in a batch, so there is no
// overflow range short of s^2 itself.  The code carries g_k = f_k / (k + 1), whose recurrence
//   g_{k+1} = A g_k + m_k B g_{k-1},   m_k = k (k + 3) / ((k + 1)(k + 2)),
// has one constant instead of two, and sums G_k = sum (w a^2) g_k and Q_k = sum (2 w a b') r_k apart:
// H_k = Q_k + (k + 1) G_k once per chunk.  8 FP64 issue slots per order instead of 9.
// Truncation: the neglected tail of r^2 is below (P + 1) rho^P / (1 - rho)  (P = kOrder terms); rho = 1/4, P = 28
// gives 29 * 2^-56 * 4/3 = 5e-16 ("Cell expansions").
// the two series in one place: how they start at a distance s and the step from order k to k + 1 (the cell form
// expands about a cell's centre, s = tau_c - tau0; the bin form about a bin's centre, s = tau_b - tau: the kernel
// depends on tau - tau0 alone, so the recurrences are the same)
struct LorentzSeries {
    static constexpr double m_of(int k) { return (double)k * (k + 3) / ((double)(k + 1) * (k + 2)); }
    __device__ __forceinline__ static void start(double s, double& r0, double& A, double& B) {
        r0 = exact_rcp(fma(s, s, 1.0));       // q0 >= 1
        B = -r0;
        A = (s + s) * B;
    }
    // r = r_k, g = g_k, Brp = B r_{k-1}, Bgp = B g_{k-1}  ->  the same of k + 1
    __device__ __forceinline__ static void step(int k, double A, double B, double& r, double& g, double& Brp,
                                                double& Bgp) {
        const double rn = fma(A, r, Brp), gn = fma(A, g, m_of(k) * Bgp);
        Brp = B * r;
        Bgp = B * g;
        r = rn;
        g = gn;
    }
};

struct LorentzCells : LorentzSeries {
    static constexpr int kOrder = OBE_CELL_ORDER;
    static constexpr int kMaxCells = OBE_CELL_MAX;
    static constexpr double kWidth = 2.0 / OBE_CELL_RHO_INV;         // of a cell: 2 rho
    static constexpr int kCoefs = 2 * kOrder + 2;                    // R_k, H_k, C1, C2 of one cell
    static_assert((OBE_CELL_RHO_INV & (OBE_CELL_RHO_INV - 1)) == 0 && OBE_CELL_RHO_INV >= 2, "rho: a power of 1/2");

    // centre of cell c of a plan that starts at `origin` (the same expression wherever a centre is needed)
    __device__ __forceinline__ static double centre(double origin, int c) {
        return fma((double)c + 0.5, kWidth, origin);
    }

    // running sums of one cell (one lane): three per order, and C1, C2
    struct Sums {
        double R[kOrder], Q[kOrder], G[kOrder], c1, c2;
        __device__ __forceinline__ void clear() {
#pragma unroll
            for (int k = 0; k < kOrder; ++k) R[k] = Q[k] = G[k] = 0.0;
            c1 = c2 = 0.0;
        }
        __device__ __forceinline__ double h(int k) const { return fma((double)(k + 1), G[k], Q[k]); }
    };
    // one packed particle (tau0, sw a, sw b', sw: Lorentz<1>::pack) into the sums of the cell centred at tc
    __device__ __forceinline__ static void add_particle(double tc, const double* pk, Sums& z) {
        double r0, A, B;
        start(tc - pk[0], r0, A, B);
        const double wa = pk[1] * pk[3], waa = pk[1] * pk[1], wab2 = (pk[1] + pk[1]) * pk[2];
        z.c1 = fma(pk[2], pk[3], z.c1);
        z.c2 = fma(pk[2], pk[2], z.c2);
        double r = r0, g = r0 * r0, Brp = 0.0, Bgp = 0.0;   // B r_{k-1}, B g_{k-1}
#pragma unroll
        for (int k = 0; k < kOrder; ++k) {
            z.R[k] = fma(wa, r, z.R[k]);
            z.Q[k] = fma(wab2, r, z.Q[k]);
            z.G[k] = fma(waa, g, z.G[k]);
            if (k + 1 < kOrder) step(k, A, B, r, g, Brp, Bgp);
        }
    }
    // a setting's two moments from its cell's coefficients coef[j * stride], j = 0 .. kCoefs-1 (R_k at k, H_k at
    // kOrder + k, C1, C2 last), delta = tau - centre
    __device__ __forceinline__ static void evaluate(const double* coef, int64_t stride, double delta, double& S1,
                                                    double& S2) {
        double c[kCoefs];
#pragma unroll
        for (int j = 0; j < kCoefs; ++j) c[j] = coef[j * stride];
        double p1 = c[kOrder - 1], p2 = c[2 * kOrder - 1];
#pragma unroll
        for (int k = kOrder - 2; k >= 0; --k) {
            p1 = fma(p1, delta, c[k]);
            p2 = fma(p2, delta, c[kOrder + k]);
        }
        S1 = p1 + c[2 * kOrder];
        S2 = p2 + c[2 * kOrder + 1];
    }
};

// ---- ... and by bin expansions (OBE_SWEEP_BINS): the same series with the roles exchanged ----
// r depends on tau - tau0 alone, so the particles can be summarised instead of the settings: the tau0 axis is cut
// into bins of half-width rho, and with eps = tau0 - tau_b (|eps| <= rho) and s = tau_b - tau
//   r = 1 / ((s + eps)^2 + 1) = sum_k r_k(s) eps^k,   r^2 = sum_k (k + 1) g_k(s) eps^k
// (r is even, so the sign of tau - tau0 does not matter).  Per bin, once per sweep,
//   M1_k = sum (w a) eps^k,   M2_k = sum (2 w a b') eps^k,   H3_k = (k + 1) sum (w a^2) eps^k,
// and per setting  S1 = C1 + sum_bins sum_k M1_k r_k(s),  S2 = C2 + sum_bins sum_k [M2_k r_k(s) + H3_k g_k(s)].
// The ratio, the order and the truncation bound are those of the cells; |r_k| <= 1, |g_k| <= 1.
struct LorentzBins : LorentzSeries {
    static constexpr int kOrder = OBE_CELL_ORDER;
    static constexpr int kMaxBins = OBE_BIN_MAX;
    static constexpr double kWidth = 2.0 / OBE_CELL_RHO_INV;         // of a bin: 2 rho
    static constexpr int kCoefs = 3 * kOrder + 2;                    // M1_k, M2_k, H3_k, C1, C2 of one bin
    static constexpr int kRow = (kCoefs + 1) & ~1;                   // doubles between two bins' (or items') rows

    // centre of bin b of a plan that starts at `origin` (the same expression wherever a centre is needed)
    __device__ __forceinline__ static double centre(double origin, int b) {
        return fma((double)b + 0.5, kWidth, origin);
    }
    // the bin of a packed tau0 (finite, >= origin) in a plan of nbins bins
    __device__ __forceinline__ static int bin_of(double origin, double tau0, int nbins) {
        const int b = static_cast<int>((tau0 - origin) * (1.0 / kWidth));
        return b < 0 ? 0 : (b >= nbins ? nbins - 1 : b);
    }
    // running sums of one lane's draws of one bin
    struct Sums {
        double M1[kOrder], M2[kOrder], M3[kOrder], c1, c2;
        __device__ __forceinline__ void clear() {
#pragma unroll
            for (int k = 0; k < kOrder; ++k) M1[k] = M2[k] = M3[k] = 0.0;
            c1 = c2 = 0.0;
        }
    };
    // one packed draw (tau0, sw a, sw b', sw: Lorentz<1>::pack) of the bin centred at tb
    __device__ __forceinline__ static void add_draw(double tb, const double* pk, Sums& z) {
        const double eps = pk[0] - tb;
        const double wa = pk[1] * pk[3], waa = pk[1] * pk[1], wab2 = (pk[1] + pk[1]) * pk[2];
        z.c1 = fma(pk[2], pk[3], z.c1);
        z.c2 = fma(pk[2], pk[2], z.c2);
        double e = 1.0;                                             // eps^k
#pragma unroll
        for (int k = 0; k < kOrder; ++k) {
            z.M1[k] = fma(wa, e, z.M1[k]);
            z.M2[k] = fma(wab2, e, z.M2[k]);
            z.M3[k] = fma(waa, e, z.M3[k]);
            if (k + 1 < kOrder) e *= eps;
        }
    }
    // A bin's folded row (M1_k at k, M2_k at kOrder + k, H3_k at 2 kOrder + k, C1, C2 last) is the same for the 64
    // settings of a wavefront: it lives in registers ACROSS the lanes and every use names the lane that holds the
    // coefficient, so a series step costs no memory access ("The row of a bin in the lanes").
    // Every 16-lane row of the wavefront holds a copy: register i, lane l: coefficient 16 i + (l & 15).  The use is
    // the multiply-add itself, v_fmac_f64 with the DPP source row_newbcast:j (lane j of the own 16-lane row).  The
    // registers are written by loads alone: a VGPR that a VALU instruction wrote may not be read through DPP in the
    // next two instructions, and nothing looks for that inside inline assembly.  All 64 lanes must be active.
    static constexpr int kLaneRegs = (kCoefs + 15) / 16;
    struct LaneRow { double v[kLaneRegs]; };
    __device__ __forceinline__ static void load_row(const double* __restrict__ row, int lane, LaneRow& x) {
#pragma unroll
        for (int i = 0; i < kLaneRegs; ++i) {
            const int j = 16 * i + (lane & 15);
            x.v[i] = row[j < kCoefs ? j : kCoefs - 1];            // (beyond the row: never named by a use)
        }
    }
    template <int J>   // fma(coefficient J of the row, x, t)
    __device__ __forceinline__ static double fma_coef(const LaneRow& row, double x, double t) {
        static_assert(J >= 0 && J < kCoefs, "a coefficient of the row");
        asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
            : "+v"(t) : "v"(row.v[J >> 4]), "v"(x), "n"(J & 15));
        return t;
    }
    // C1 += row[3 kOrder], C2 += row[3 kOrder + 1]: fma(c, 1, C) is c + C, rounded once
    __device__ __forceinline__ static void add_constants(const LaneRow& row, double& C1, double& C2) {
        C1 = fma_coef<3 * kOrder>(row, 1.0, C1);
        C2 = fma_coef<3 * kOrder + 1>(row, 1.0, C2);
    }
    template <int K>   // orders K, K - 1, ..., 0 of the three series
    __device__ __forceinline__ static void sum_down(const LaneRow& row, const double (&r)[kOrder],
                                                    const double (&g)[kOrder], double& t1, double& t2) {
        t1 = fma_coef<K>(row, r[K], t1);
        t2 = fma_coef<kOrder + K>(row, r[K], t2);
        t2 = fma_coef<2 * kOrder + K>(row, g[K], t2);
        if constexpr (K > 0) sum_down<K - 1>(row, r, g, t1, t2);
    }
    // one bin's share of a setting's two moments from its folded row, s = tau_b - tau: each series summed from the
    // highest order down
    __device__ __forceinline__ static void evaluate(const LaneRow& row, double s, double& t1, double& t2) {
        double r[kOrder], g[kOrder];
        double A, B, Brp = 0.0, Bgp = 0.0;
        start(s, r[0], A, B);
        g[0] = r[0] * r[0];
#pragma unroll
        for (int k = 0; k + 1 < kOrder; ++k) {
            r[k + 1] = r[k];
            g[k + 1] = g[k];
            step(k, A, B, r[k + 1], g[k + 1], Brp, Bgp);
        }
        t1 = 0.0;
        t2 = 0.0;
        sum_down<kOrder - 1>(row, r, g, t1, t2);
    }
};

// y = p0 + p1 * x        tests/test_optbayesexpt.py:11-14
struct LineAB {
    static constexpr int NS = 1, NC = 1, NREAD = 2, NXS = 1, NPK = 2, NCONST = 0;
    __device__ static void eval(const double* x, const ParamRef& th, const obe_model&, double* y) {
        const double bx = th(1) * x[0];
        y[0] = th(0) + bx;
    }
    __device__ static void prep_setting(const double* x, const obe_model&, double* xs) { xs[0] = x[0]; }
    __device__ static void pack(const ParamRef& th, const double* thbar, const obe_model&, double sw, double* pk) {
        pk[0] = sw * (th(0) - thbar[0]);
        pk[1] = sw * th(1);
    }
    template <int SPT>
    __device__ __forceinline__ static void sweep_eval(const double (&xs)[SPT][NXS], const double* pk, double,
                                                      const obe_model&, double (&v)[SPT][NC]) {
#pragma unroll
        for (int j = 0; j < SPT; ++j) v[j][0] = fma(pk[1], xs[j][0], pk[0]);
    }
};

// y = p0 * x + p1        demos/line_plus_noise/line_plus_noise.py:36-53
struct LineMB {
    static constexpr int NS = 1, NC = 1, NREAD = 2, NXS = 1, NPK = 2, NCONST = 0;
    __device__ static void eval(const double* x, const ParamRef& th, const obe_model&, double* y) {
        const double mx = th(0) * x[0];
        y[0] = mx + th(1);
    }
    __device__ static void prep_setting(const double* x, const obe_model&, double* xs) { xs[0] = x[0]; }
    __device__ static void pack(const ParamRef& th, const double* thbar, const obe_model&, double sw, double* pk) {
        pk[0] = sw * th(0);
        pk[1] = sw * (th(1) - thbar[1]);
    }
    template <int SPT>
    __device__ __forceinline__ static void sweep_eval(const double (&xs)[SPT][NXS], const double* pk, double,
                                                      const obe_model&, double (&v)[SPT][NC]) {
#pragma unroll
        for (int j = 0; j < SPT; ++j) v[j][0] = fma(pk[0], xs[j][0], pk[1]);
    }
};

// y = p0                 tests/test_zinference.py:21-26
struct FirstParam {
    static constexpr int NS = 1, NC = 1, NREAD = 1, NXS = 1, NPK = 1, NCONST = 0;
    __device__ static void eval(const double*, const ParamRef& th, const obe_model&, double* y) { y[0] = th(0); }
    __device__ static void prep_setting(const double* x, const obe_model&, double* xs) { xs[0] = x[0]; }
    __device__ static void pack(const ParamRef& th, const double* thbar, const obe_model&, double sw, double* pk) {
        pk[0] = sw * (th(0) - thbar[0]);
    }
    template <int SPT>
    __device__ __forceinline__ static void sweep_eval(const double (&)[SPT][NXS], const double* pk, double,
                                                      const obe_model&, double (&v)[SPT][NC]) {
#pragma unroll
        for (int j = 0; j < SPT; ++j) v[j][0] = pk[0];
    }
};

// Rabi oscillation counts, demos/pipulse/pipulse.py:18-49
// settings (pulsetime, delta_f); params (B1, f_center); consts (baseline, contrast, T1)
struct Rabi {
    static constexpr int NS = 2, NC = 1, NREAD = 2, NXS = 3, NPK = 3, NCONST = 3;
    static constexpr int kSweepCost = 7;   // exp, cos, hypot per evaluation (the generator's estimate for this formula)
    // the fraction removed from the baseline: y = baseline * (1 - frac)
    __device__ __forceinline__ static double frac(double tau, double df, double b1, double fc,
                                                   double contrast, double t1) {
        const double det = df - fc;
        const double rz = det / b1;
        const double zz = rz * rz;
        const double f = hypot(det, b1);
        const double e = exp(-tau / t1);
        const double arg = (6.283185307179586 * f) * tau;
        const double osc = 1.0 - cos(arg);
        const double amp = ((e * contrast) / 2.0) * osc;
        return amp / (zz + 1.0);
    }
    __device__ static void eval(const double* x, const ParamRef& th, const obe_model& m, double* y) {
        y[0] = m.consts[0] * (1.0 - frac(x[0], x[1], th(0), th(1), m.consts[1], m.consts[2]));
    }
    // Sweep form.  With f^2 = det^2 + B1^2:  1/(zz + 1) = B1^2 / f^2  and  1 - cos(2 pi f tau) =
    // 2 sin^2(pi f tau), so
    //   y - baseline = -baseline * [contrast exp(-tau/T1)] * [B1^2] * sin^2(pi f tau) / f^2
    // with the first bracket per setting and the second per particle.  One v_rsq_f64 + two
    // Newton steps give both f and 1/f^2 (no division, no hypot), and sin^2(pi x) needs no
    // quadrant logic: r = x - rint(x) is exact and sin^2(pi r) is even in r.  ~35 issue slots per
    // evaluation instead of ~150 for the literal formula (exp, hypot, cos, three IEEE divisions).
    __device__ static void prep_setting(const double* x, const obe_model& m, double* xs) {
        xs[0] = x[0];
        xs[1] = x[1];
        xs[2] = exp(-x[0] / m.consts[2]) * m.consts[1];       // contrast * exp(-tau / T1)
    }
    __device__ static void pack(const ParamRef& th, const double*, const obe_model& m, double sw, double* pk) {
        pk[0] = th(0) * th(0);                                  // B1^2
        pk[1] = th(1);                                          // f_center
        pk[2] = -(sw * m.consts[0]) * pk[0];                    // -sqrt(w) * baseline * B1^2
    }
    // sin(pi r) / r on |r| <= 1/2 as a polynomial in r^2: coefficients (-1)^k pi^(2k+1) / (2k+1)!,
    // k = 0..10; the first neglected term is 1e-17 at the edge.
    __device__ __forceinline__ static double sinpi_over_r(double r2) {
        double p = 0x1.2877020d52cf0p-31;
        p = fma(p, r2, -0x1.8a404211f9547p-26);
        p = fma(p, r2, 0x1.aaec32af93359p-21);
        p = fma(p, r2, -0x1.6fadb9f155744p-16);
        p = fma(p, r2, 0x1.e8f434d018d63p-12);
        p = fma(p, r2, -0x1.e3074fde8871fp-8);
        p = fma(p, r2, 0x1.50783487ee782p-4);
        p = fma(p, r2, -0x1.32d2cce62bd86p-1);
        p = fma(p, r2, 0x1.466bc6775aae2p+1);
        p = fma(p, r2, -0x1.4abbce625be53p+2);
        return fma(p, r2, 0x1.921fb54442d18p+1);
    }
    template <int SPT>
    __device__ __forceinline__ static void sweep_eval(const double (&xs)[SPT][NXS], const double* pk, double,
                                                      const obe_model&, double (&v)[SPT][NC]) {
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const double det = xs[j][1] - pk[1];
            const double f2 = fma(det, det, pk[0]);
            const double y = fast_rsqrt(f2);                    // 1/f
            const double x = (f2 * y) * xs[j][0];               // f * tau
            const double r = x - rint(x);
            const double s = r * sinpi_over_r(r * r);           // +- sin(pi f tau)
            v[j][0] = ((xs[j][2] * pk[2]) * (s * s)) * (y * y);
        }
    }
};

// Parallel RLC coil impedance, demos/lockin/lockin_of_coil.py:63-102
// setting w; params (L, R, C [, noise]); channels (Re Z, Im Z)
struct Coil {
    static constexpr int NS = 1, NC = 2, NREAD = 3, NXS = 2, NPK = 7, NCONST = 0;
    static constexpr int kSweepCost = 3;   // two channels, one shared complex reciprocal
    // (1 + 0j) / (c + dj) the way NumPy's complex divide loop does it (Smith's method,
    // numpy/_core/src/umath/loops.c.src, complex _divide)
    __device__ __forceinline__ static void crecip(double c, double d, double& re, double& im) {
        if (fabs(c) >= fabs(d)) {
            const double rat = d / c;
            const double scl = 1.0 / (c + d * rat);
            re = (1.0 + 0.0 * rat) * scl;
            im = (0.0 - 1.0 * rat) * scl;
        } else {
            const double rat = c / d;
            const double scl = 1.0 / (d + c * rat);
            re = (1.0 * rat + 0.0) * scl;
            im = (0.0 * rat - 1.0) * scl;
        }
    }
    __device__ __forceinline__ static void formula(double w, double L, double R, double C, double* y) {
        double y1r, y1i;
        crecip(R, w * L, y1r, y1i);
        const double yr = y1r + 0.0;
        const double yi = y1i + w * C;
        crecip(yr, yi, y[0], y[1]);
    }
    __device__ static void eval(const double* x, const ParamRef& th, const obe_model&, double* y) {
        formula(x[0], th(0), th(1), th(2), y);
    }
    // Sweep form, one reciprocal per evaluation instead of two complex divisions:
    //   Y = 1/(R + jwL) + jwC = (R - jwL)/n + jwC,  n = R^2 + w^2 L^2
    //   Z = conj(Y)/|Y|^2 = n (R - jE) / (R^2 + E^2),  E = w (C n - L)
    // The reciprocals of D = R^2 + E^2 are batched over the lane's settings; D has no fixed
    // scale (units!), so the poisoned batch + exact twin of the generated models is used.
    __device__ static void prep_setting(const double* x, const obe_model&, double* xs) {
        xs[0] = x[0];
        xs[1] = x[0] * x[0];
    }
    __device__ static void pack(const ParamRef& th, const double*, const obe_model&, double sw, double* pk) {
        const double L = th(0), R = th(1), C = th(2);
        pk[0] = L * L;
        pk[1] = R * R;
        pk[2] = C;
        pk[3] = L;
        pk[4] = sw * R;
        pk[5] = -sw;
        pk[6] = R;
    }
    template <int SPT>
    __device__ __forceinline__ static void sweep_eval(const double (&xs)[SPT][NXS], const double* pk, double,
                                                      const obe_model&, double (&v)[SPT][NC]) {
        double n[SPT], e[SPT], d[SPT], rd[SPT];
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            n[j] = fma(xs[j][1], pk[0], pk[1]);
            e[j] = xs[j][0] * fma(pk[2], n[j], -pk[3]);
            d[j] = fma(e[j], e[j], pk[1]);
        }
        batch_rcp_poisoned<SPT>(d, rd);
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const double t = n[j] * rd[j];
            v[j][0] = pk[4] * t;
            v[j][1] = (pk[5] * e[j]) * t;
        }
    }
    // the exact NumPy operation sequence: the repeat after a poisoned batch (OBE_SWEEP_SAFE)
    static constexpr bool kHasSafeEval = true;
    template <int SPT>
    __device__ __forceinline__ static void sweep_eval_safe(const double (&xs)[SPT][NXS], const double* pk, double sw,
                                                           const obe_model&, double (&v)[SPT][NC]) {
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            double y[2];
            formula(xs[j][0], pk[3], pk[6], pk[2], y);
            v[j][0] = sw * y[0];
            v[j][1] = sw * y[1];
        }
    }
};

// relative cost of one sweep evaluation (1 unless the model says otherwise): the sweep plans its grid by time
template <class M, class = void>
struct sweep_cost { static constexpr int value = 1; };
template <class M>
struct sweep_cost<M, std::void_t<decltype(M::kSweepCost)>> { static constexpr int value = M::kSweepCost; };

template <class M, class = void>
struct has_pair_eval { static constexpr bool value = false; };
template <class M>
struct has_pair_eval<M, std::enable_if_t<M::kHasPairEval>> { static constexpr bool value = true; };
// models whose SAFE sweep may run its particles two at a time through sweep_eval_pair()
template <class M, class = void>
struct safe_pair_eval { static constexpr bool value = false; };
template <class M>
struct safe_pair_eval<M, std::enable_if_t<M::kSafePairEval>> { static constexpr bool value = true; };
// models whose sweep_eval() may poison out-of-range batches bring a branchy, always-IEEE twin
template <class M, class = void>
struct has_safe_eval { static constexpr bool value = false; };
template <class M>
struct has_safe_eval<M, std::enable_if_t<M::kHasSafeEval>> { static constexpr bool value = true; };

#ifdef OBE_PLUGIN_MODEL_HEADER
// ---- plugin build -------------------------------------------------------------------
// The same kernel sources compiled once more for ONE model generated from a user's
// expression (optbayesexpt_amd/models.py: from_expression): the header defines
// obe::PluginModel with the interface of the structs above, and every entry point of the
// resulting shared library serves that model whatever m.id says.
}  // namespace obe
#include OBE_PLUGIN_MODEL_HEADER
namespace obe {
template <class F>
int dispatch_model(const obe_model&, F&& f) {
    return f(PluginModel{});
}
#else
// Host-side dispatch: f(ModelType{}) for the model named by m.id / m.aux.
template <class F>
int dispatch_model(const obe_model& m, F&& f) {
    switch (m.id) {
        case OBE_MODEL_LORENTZ:
            switch (m.aux) {
                case 1: return f(Lorentz<1>{});
                case 2: return f(Lorentz<2>{});
                case 3: return f(Lorentz<3>{});
                case 4: return f(Lorentz<4>{});
                case 5: return f(Lorentz<5>{});
                case 6: return f(Lorentz<6>{});
                case 7: return f(Lorentz<7>{});
                case 8: return f(Lorentz<8>{});
                default: return bad_arg("Lorentz: aux (number of peaks) must be 1..8");
            }
        case OBE_MODEL_LINE_AB: return f(LineAB{});
        case OBE_MODEL_LINE_MB: return f(LineMB{});
        case OBE_MODEL_FIRST_PARAM: return f(FirstParam{});
        case OBE_MODEL_RABI: return f(Rabi{});
        case OBE_MODEL_COIL: return f(Coil{});
        default: return bad_arg("unknown model id");
    }
}
#endif

}  // namespace obe
