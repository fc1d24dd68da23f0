// K20 — count-aware scoring and reading bands (OptBayesExptBinomial, OptBayesExptPoisson; extends K17/K18/K19).  The
// next reading of channel c is a whole number K_c with the class's own pmf per particle, P_c,i(k) = Binomial(k; n, p_c,i)
// or Poisson(k; t r_c,i); what a user asks of it is the mixture over the weighted cloud.
//   table      the hot path: Pbar_c(k) = sum_i w_i P_c,i(k) / W for k = 0 .. count_max, per point (a setting, or a
//              record's setting with its own n or t) and channel.  cloud_pass_kernel's geometry (obe_cloud_pass.h): one
//              wave per workgroup, lane <-> point, the particle axis streamed (the same particle for all lanes), grid =
//              point tiles x particle chunks, chunk partials folded in chunk order.  The outcomes are covered in blocks
//              of a compile-time width B (32 or 64 outcome sums per lane in registers), one launch per channel and
//              block, each folded into its rows of the table before the next one starts: the chunk partials keep the
//              size of K18's pass whatever count_max is.  Every block restarts from a log-space value of one of its
//              own outcomes, so that the table is right where e^-lambda or (1 - p)^n underflows and a recurrence's
//              error grows over one block only.  Poisson: from the block's first outcome k0,
//              exp(k0 log lambda - lambda - log k0!), then poisson_info_kernel's unrolled recurrence
//              P(k) = P(k - 1) lambda (1 / k), the factors 1 / k a table in the workspace read with wave-uniform
//              indices.  Binomial: a lane sums T(k) = Cmax p^k (1 - p)^(n - k), Cmax the block's largest C(n, k) — a
//              geometric sequence in k with the ratio p / (1 - p), which is run from its LARGE end: upwards from k0
//              for p <= 1/2, downwards from the block's last outcome <= n for p > 1/2 (a branch per lane; a wave whose
//              lanes disagree runs both).  So an underflow can only lose terms that are negligible beside the start,
//              wherever in the block the mass lies (p = 1 - 1e-12 as well as 1e-12); T(k) >= P(k), so no row that
//              matters is lost either, and the fold multiplies by C(n, k) / Cmax <= 1.  What no particle changes
//              (log k0!, log Cmax, n - k0) is formed once per lane from the caller's table of log k!.  Per evaluation
//              one exp, in Poisson blocks behind the first one log more, binomial a log1p, a division and (p > 1/2 or
//              k0 > 0) a log; per outcome 3 FP64 operations (Poisson), 2 (binomial upwards) or 4 (downwards, with the
//              selection that places the start).  lambda = 0 gives the exact point mass at 0 through the recurrence;
//              p = 0 and p = 1 have no finite ratio one way or the other: such a particle's weight is summed on its
//              own and added to the outcome 0 or n in the fold, exactly.  No atomics: the same bits from run to run.  FP64-issue bound.
//   above      the mass beyond count_max, the table's last row: max(1 - sum_k Pbar_c(k), 0) from the folded table (a
//              difference of numbers near 1: absolute accuracy), exactly 0 for a binomial point with n <= count_max.
//   tails, quantiles   light kernels on the folded table, one thread per (point, channel).
//   logpmf     the JOINT one-step log evidence of a record, log(sum_i w_i prod_c P_c,i(k_c) / W): K11's geometry (lane
//              <-> record) and its (m, S) log-sum-exp merge, the exponent being the class's record term over all
//              channels (K19's arithmetic); W per lane, since who contributes depends on the record's setting.
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>

#include "obe_cloud_pass.h"

namespace obe {
namespace {

constexpr int kCountWaves = 4096;                  // waves a pass aims at (K18's figure): chunks = this / point tiles
constexpr int kCountMax = OBE_COUNT_MAX_OUTCOMES;
constexpr int kCountNarrow = 32, kCountWide = 64;  // outcome sums per lane: the block widths
constexpr int kRecipWords = kCountMax + kCountWide + 8;        // 1 / k for every k a block's recurrence reaches
constexpr int kLogpmfSlots = 3;                    // m, S, W
constexpr double kInf = __builtin_huge_val();
constexpr double kNaN = __builtin_nan("");

constexpr int table_slots(int width) { return width + 3; }     // the outcome sums, W, the weights at p == 1 and p == 0

// The two laws, a compile-time term of the kernels below.  side: what a point brings besides its setting (shots n,
// exposure t), per channel; value: the model's p or r.
struct BinomialLaw {
    static constexpr bool kBinomial = true;
    __device__ __forceinline__ static bool side_ok(double n) { return n >= 1.0 && n <= kCountMax && n == floor(n); }
    __device__ __forceinline__ static bool value_ok(double p, double) { return p >= 0.0 && p <= 1.0; }
};
struct PoissonLaw {
    static constexpr bool kBinomial = false;
    __device__ __forceinline__ static bool side_ok(double t) { return t > 0.0 && t < kInf; }
    __device__ __forceinline__ static bool value_ok(double r, double t) { return r >= 0.0 && r * t < kInf; }
};

// recip[k] = 1 / k, correctly rounded (recip[0] is never read)
__global__ __launch_bounds__(kBlock) void count_recip_kernel(double* __restrict__ recip) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k < kRecipWords) recip[k] = k ? 1.0 / k : 0.0;
}

// log of the largest C(n, k) over the block's outcomes k0 .. min(k0 + width - 1, n): the coefficient nearest n / 2 (0 if
// k0 > n); n in 1 .. kCountMax, k0 in 0 .. kCountMax.  The table kernel and the fold form it with the same bits.
__device__ __forceinline__ double block_log_choose(const double* __restrict__ logfact, int n, int k0, int width) {
    if (k0 > n) return 0.0;
    const int last = k0 + width - 1 < n ? k0 + width - 1 : n, mid = n / 2;
    const int k = mid < k0 ? k0 : mid > last ? last : mid;
    return logfact[n] - logfact[k] - logfact[n - k];
}

// element `channel` of y[C] (channel is the same for all lanes; no run-time index into registers)
template <int C>
__device__ __forceinline__ double pick(const double (&y)[C], int channel) {
    double v = y[0];
#pragma unroll
    for (int c = 1; c < C; ++c) v = c == channel ? y[c] : v;
    return v;
}

// partials (chunk, B + 3, padded points): for the outcomes k0 .. k0 + B - 1 of channel `channel`, sums over the chunk's
// contributing particles of w P(k) (binomial: of w P(k) Cmax / C(n, k) with Cmax the block's largest coefficient; the
// fold multiplies the ratio back); then W; then (binomial) the weights of the contributing particles with p == 1 and
// with p == 0.  A particle contributes to a lane when its clean weight is > 0, the lane's side data are valid and every channel's
// value is one the law takes; one that does not is carried through the arithmetic with weight 0 and a harmless value,
// which leaves every sum's bits as they were.
template <class M, class Law, int B>
__global__ __launch_bounds__(kWave) void count_table_kernel(obe_model m, const double* __restrict__ settings,
                                                            int64_t ld_s, int64_t n_s, const double* __restrict__ side,
                                                            int64_t ld_side, const double* __restrict__ logfact,
                                                            const double* __restrict__ recip,
                                                            const double* __restrict__ particles, int64_t ld_p,
                                                            int64_t n, const double* __restrict__ w, int channel, int k0,
                                                            int64_t chunk_len, double* __restrict__ partials) {
    constexpr int C = M::NC;
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_s ? s : n_s - 1;                    // (the padding lanes repeat the last point)
    double x[M::NS], sd[C], po[B], sw = 0.0, s1 = 0.0, s0 = 0.0;
    bool lane_ok = true;
#pragma unroll
    for (int k = 0; k < M::NS; ++k) x[k] = settings[(int64_t)k * ld_s + sc];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        sd[c] = side[(int64_t)c * ld_side + sc];
        const bool ok = Law::side_ok(sd[c]);
        lane_ok = lane_ok && ok;
        sd[c] = ok ? sd[c] : 1.0;                                // (valid from here on: an index below)
    }
#pragma unroll
    for (int j = 0; j < B; ++j) po[j] = 0.0;
    // what no particle changes of the block's anchor outcomes
    const double sdc = pick<C>(sd, channel), k0d = (double)k0;
    double lc, nk = 0.0, top = 0.0;
    bool start_in = true;
    if constexpr (Law::kBinomial) {
        nk = sdc - k0d;                                          // shots beyond the block's first outcome
        start_in = nk >= 0.0;                                    // (k0 > n: the whole block is 0)
        top = nk < (double)(B - 1) ? nk : (double)(B - 1);       // the block's last outcome that is <= n, from k0
        lc = block_log_choose(logfact, (int)sdc, k0, B);         // log of the block's largest C(n, k)
    } else {
        lc = -logfact[k0];
    }
    const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    for (int64_t p = p0; p < p1; ++p) {                          // (p, w[p] and the particle are the same for all lanes)
        const double wp = clean_weight(w[p]);
        if (wp == 0.0) continue;                                 // (whatever the model gives)
        double y[C];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
        bool ok = lane_ok;
#pragma unroll
        for (int c = 0; c < C; ++c) ok = ok && Law::value_ok(y[c], sd[c]);
        const double yc = pick<C>(y, channel);
        sw += ok ? wp : 0.0;
        if constexpr (Law::kBinomial) {
            // (p == 1 and p == 0 have no finite ratio one way or the other: their point masses, at n and at 0, are
            // the particle's weight itself, summed apart and added by the fold — exactly)
            const bool one = ok && yc == 1.0, zero = ok && yc == 0.0;
            s1 += one ? wp : 0.0;
            s0 += zero ? wp : 0.0;
            const bool in = ok && !one && !zero;
            const double wl = in ? wp : 0.0, pr = in ? yc : 0.5;
            // T_j = Cmax p^(k0 + j) (1 - p)^(n - k0 - j), a geometric sequence in j with ratio p / (1 - p); it is run
            // from its LARGE end, so that an underflow only ever loses terms that are negligible beside the start
            const double lq = log1p(-pr);
            if (pr <= 0.5) {                                     // upwards from the block's first outcome
                double arg = nk * lq + lc;
                if (k0 > 0) arg += k0d * log(pr);                // (wave-uniform)
                const double t0 = exp(arg);
                double t = start_in ? t0 : 0.0;
                const double odds = pr / (1.0 - pr);             // <= 1
                po[0] = fma(wl, t, po[0]);
#pragma unroll
                for (int j = 1; j < B; ++j) {
                    t *= odds;
                    po[j] = fma(wl, t, po[j]);
                }
            } else {                                             // downwards from the block's last outcome <= n
                const double t_top = exp((k0d + top) * log(pr) + (nk - top) * lq + lc);
                const double back = (1.0 - pr) / pr;             // < 1
                double t = 0.0;                                  // (stays 0 above n, and everywhere if k0 > n)
#pragma unroll
                for (int j = B - 1; j >= 0; --j) {
                    t = top == (double)j ? t_top : t * back;
                    po[j] = fma(wl, t, po[j]);
                }
            }
        } else {
            const double wl = ok ? wp : 0.0, lam = sdc * (ok ? yc : 1.0);
            double arg = -lam;
            if (k0 > 0) arg = fma(k0d, log(lam > 0.0 ? lam : 1.0), -lam) + lc;   // (wave-uniform)
            double pk = exp(arg);
            if (k0 > 0 && lam == 0.0) pk = 0.0;
            po[0] = fma(wl, pk, po[0]);
#pragma unroll
            for (int j = 1; j < B; ++j) {                        // P(k) = P(k - 1) lambda / k
                pk *= lam * recip[k0 + j];
                po[j] = fma(wl, pk, po[j]);
            }
        }
    }
    const int64_t n_pad = (int64_t)gridDim.x * kWave;
    double* out = partials + (int64_t)blockIdx.y * table_slots(B) * n_pad + s;
#pragma unroll
    for (int j = 0; j < B; ++j) out[j * n_pad] = po[j];
    out[B * n_pad] = sw;
    out[(B + 1) * n_pad] = s1;
    out[(B + 2) * n_pad] = s0;
}

// pmf_c (count_max + 2, n_points), rows k0 .. min(k0 + width - 1, count_max) of one channel: the chunk partials added
// in chunk order (binomial: times C(n, k) / Cmax, 0 beyond n, plus the weight at p == 1 where k == n and the weight at
// p == 0 where k == 0), over W; NaN where W == 0.  blockIdx.y: the outcome within the block.
__global__ __launch_bounds__(kBlock) void count_fold_kernel(const double* __restrict__ partials, int chunks, int width,
                                                            int64_t n_pad, int64_t n_s, int binomial,
                                                            const double* __restrict__ side_c,
                                                            const double* __restrict__ logfact, int k0, int count_max,
                                                            double* __restrict__ pmf_c) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int j = blockIdx.y, k = k0 + j;
    if (s >= n_s || k > count_max) return;
    const int slots = table_slots(width);
    const double sw = chunk_order_sum(partials, chunks, slots, width, n_pad, s);
    double so = chunk_order_sum(partials, chunks, slots, j, n_pad, s);
    if (binomial) {
        const double nd = side_c[s];
        if (BinomialLaw::side_ok(nd) && k <= (int)nd) {          // C(n, k) / Cmax <= 1
            const int n = (int)nd;
            so *= exp((logfact[n] - logfact[k] - logfact[n - k]) - block_log_choose(logfact, n, k0, width));
            if (k == n) so += chunk_order_sum(partials, chunks, slots, width + 1, n_pad, s);
            if (k == 0) so += chunk_order_sum(partials, chunks, slots, width + 2, n_pad, s);
        } else {
            so = 0.0;                                            // (beyond the shots; W is 0 where n is not valid)
        }
    }
    pmf_c[(int64_t)k * n_s + s] = sw > 0.0 && sw < kInf ? so / sw : kNaN;
}

// the table's last row, the mass beyond count_max; one thread per (channel, point)
__global__ __launch_bounds__(kBlock) void count_above_kernel(double* __restrict__ pmf, int n_channels, int count_max,
                                                             int64_t n_s, int binomial, const double* __restrict__ side,
                                                             int64_t ld_side) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_s * n_channels) return;
    const int64_t c = i / n_s, s = i % n_s;
    double* col = pmf + c * (count_max + 2) * n_s + s;
    double sum = 0.0;
    for (int k = 0; k <= count_max; ++k) sum += col[(int64_t)k * n_s];
    double above = 1.0 - sum;
    if (!(above > 0.0)) above = 0.0;
    if (binomial && side[c * ld_side + s] <= (double)count_max) above = 0.0;     // (the window reaches n)
    if (sum != sum) above = kNaN;
    col[(int64_t)(count_max + 1) * n_s] = above;
}

// lower (C, n_points) = sum_{j <= k} Pbar(j), upper = sum_{j >= k} Pbar(j) + the mass above, both from the small end;
// NaN where k is not a whole number in 0 .. count_max
__global__ __launch_bounds__(kBlock) void count_tails_kernel(const double* __restrict__ pmf, int n_channels,
                                                             int count_max, int64_t n_s,
                                                             const double* __restrict__ counts, int64_t ld_k,
                                                             double* __restrict__ lower, double* __restrict__ upper) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_s * n_channels) return;
    const int64_t c = i / n_s, s = i % n_s;
    const double* col = pmf + c * (count_max + 2) * n_s + s;
    const double kd = counts[c * ld_k + s];
    double lo = kNaN, up = kNaN;
    if (kd >= 0.0 && kd <= (double)count_max && kd == floor(kd)) {
        const int k = (int)kd;
        lo = 0.0;
        for (int j = 0; j <= k; ++j) lo += col[(int64_t)j * n_s];
        up = col[(int64_t)(count_max + 1) * n_s];
        for (int j = count_max; j >= k; --j) up += col[(int64_t)j * n_s];
    }
    if (lower) lower[c * n_s + s] = lo;
    if (upper) upper[c * n_s + s] = up;
}

struct CountLevels {
    int n;
    double q[OBE_COUNT_MAX_LEVELS];
};

// quantiles (n_levels, C, n_points): the smallest k with sum_{j <= k} Pbar(j) >= q; +inf where count_max is too small
// for the level, NaN where W == 0.  Where nothing lies above the window the last outcome closes the sum: 1.
__global__ __launch_bounds__(kBlock) void count_quantiles_kernel(const double* __restrict__ pmf, int n_channels,
                                                                 int count_max, int64_t n_s, CountLevels lv,
                                                                 double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_s * n_channels) return;
    const int64_t c = i / n_s, s = i % n_s;
    const double* col = pmf + c * (count_max + 2) * n_s + s;
    const double above = col[(int64_t)(count_max + 1) * n_s];
    double found[OBE_COUNT_MAX_LEVELS];
#pragma unroll
    for (int j = 0; j < OBE_COUNT_MAX_LEVELS; ++j) found[j] = above != above ? kNaN : kInf;
    double cum = 0.0;
    for (int k = 0; k <= count_max; ++k) {
        cum += col[(int64_t)k * n_s];
        if (k == count_max && above == 0.0) cum = 1.0;
#pragma unroll
        for (int j = 0; j < OBE_COUNT_MAX_LEVELS; ++j)
            if (found[j] == kInf && cum >= lv.q[j]) found[j] = (double)k;
    }
#pragma unroll
    for (int j = 0; j < OBE_COUNT_MAX_LEVELS; ++j)
        if (j < lv.n) out[((int64_t)j * n_channels + c) * n_s + s] = found[j];
}

// (m, S) <- (m, S) + s exp(l): K11's merge (obe_predict.hip); l finite, m finite or -inf
__device__ __forceinline__ void lse_add(double& m, double& S, double l, double s) {
    const bool up = l > m;
    const double e = exp(up ? m - l : l - m);
    S = up ? S * e + s : S + s * e;
    m = up ? l : m;
}

// partials (chunk, 3, padded records): the chunk's (m, S) of sum_i w_i exp(l_i) and its W, lane <-> record;
// l_i = sum_c [k log p + (n - k) log1p(-p)] or sum_c [k log lambda - lambda], a term whose count is 0 left out (the
// record differs from lane to lane: a selection, not a branch).  An impossible record (l = -inf) adds to W alone.
template <class M, class Law>
__global__ __launch_bounds__(kWave) void count_logpmf_kernel(obe_model m, const double* __restrict__ settings,
                                                             int64_t ld_s, int64_t n_r, const double* __restrict__ counts,
                                                             int64_t ld_k, const double* __restrict__ side,
                                                             int64_t ld_side, const double* __restrict__ particles,
                                                             int64_t ld_p, int64_t n, const double* __restrict__ w,
                                                             int64_t chunk_len, double* __restrict__ partials) {
    constexpr int C = M::NC;
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_r ? s : n_r - 1;                    // (the padding lanes repeat the last record)
    double x[M::NS], kc[C], sd[C], fc[C];
    bool rec_ok = true;
#pragma unroll
    for (int k = 0; k < M::NS; ++k) x[k] = settings[(int64_t)k * ld_s + sc];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        kc[c] = counts[(int64_t)c * ld_k + sc];
        sd[c] = side[(int64_t)c * ld_side + sc];
        rec_ok = rec_ok && Law::side_ok(sd[c]) && kc[c] >= 0.0 && kc[c] < kInf && kc[c] == floor(kc[c]);
        if (Law::kBinomial) rec_ok = rec_ok && kc[c] <= sd[c];
        fc[c] = sd[c] - kc[c];                                   // (binomial: the failures)
    }
    double top = -kInf, S = 0.0, sw = 0.0;
    const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    for (int64_t p = p0; p < p1; ++p) {                          // (p, w[p] and the particle are the same for all lanes)
        const double wp = clean_weight(w[p]);
        if (wp == 0.0) continue;
        double y[C];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
        bool ok = rec_ok;
        double l = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            ok = ok && Law::value_ok(y[c], sd[c]);
            if constexpr (Law::kBinomial) {
                const double a = kc[c] * log(y[c]), b = fc[c] * log1p(-y[c]);
                l += kc[c] > 0.0 ? a : 0.0;                      // (p = 0 with k > 0: -inf)
                l += fc[c] > 0.0 ? b : 0.0;
            } else {
                const double lam = sd[c] * y[c], a = kc[c] * log(lam);
                l += kc[c] > 0.0 ? a : 0.0;                      // (lambda = 0 with k > 0: -inf)
                l -= lam;
            }
        }
        if (!ok) continue;
        sw += wp;
        if (l > -kInf) lse_add(top, S, l, wp);
    }
    const int64_t n_pad = (int64_t)gridDim.x * kWave;
    double* out = partials + (int64_t)blockIdx.y * kLogpmfSlots * n_pad + s;
    out[0] = top;
    out[n_pad] = S;
    out[2 * n_pad] = sw;
}

// logpmf (n_records,) = m + log S - log W + constant, the chunks' (m_j, S_j) merged and their W added in chunk order;
// -inf where the record is impossible for every contributing particle, NaN where W == 0
__global__ __launch_bounds__(kBlock) void count_logpmf_fold_kernel(const double* __restrict__ partials, int chunks,
                                                                   int64_t n_pad, int64_t n_r,
                                                                   const double* __restrict__ constant,
                                                                   double* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_r) return;
    double top = -kInf, S = 0.0;
    for (int j = 0; j < chunks; ++j) {
        const double mj = partials[((int64_t)j * kLogpmfSlots + 0) * n_pad + s];
        if (mj > -kInf) lse_add(top, S, mj, partials[((int64_t)j * kLogpmfSlots + 1) * n_pad + s]);
    }
    const double sw = chunk_order_sum(partials, chunks, kLogpmfSlots, 2, n_pad, s);
    double r = kNaN;
    if (sw > 0.0 && sw < kInf) r = top > -kInf ? top + log(S) - log(sw) + constant[s] : -kInf;
    out[s] = r;
}

int count_refuse(const char* who, const char* what) {
    static thread_local std::string msg;
    msg = std::string(who) + ": " + what;
    return bad_arg(msg.c_str());
}

inline bool is_law(int law) { return law == OBE_COUNT_BINOMIAL || law == OBE_COUNT_POISSON; }

// what the kernels on a folded table share of their refusals (nullptr: none)
const char* table_shape_refusal(int n_channels, int count_max, int64_t n_points) {
    if (n_channels < 1 || n_channels > OBE_MAX_CHANNELS) return "n_channels outside 1..OBE_MAX_CHANNELS";
    if (count_max < 0 || count_max > kCountMax) return "count_max outside 0..OBE_COUNT_MAX_OUTCOMES";
    if (n_points < 1) return "n_points < 1";
    if ((n_points * n_channels + kBlock - 1) / kBlock > 0x7fffffff) return "too many points for one call";
    return nullptr;
}

}  // namespace
}  // namespace obe

using namespace obe;

extern "C" {

int64_t obe_count_workspace_bytes(int64_t n_particles, int64_t n_points, int32_t n_channels, int32_t count_max) {
    (void)n_particles;                                           // (the chunks are bounded whatever the cloud,
    (void)n_channels;                                            //  a pass serves one channel
    (void)count_max;                                             //  and one block of outcomes)
    if (n_points < 1) n_points = 1;
    return (kRecipWords + cloud_pass_words(n_points, table_slots(kCountWide), kCountWaves)) * (int64_t)sizeof(double);
}

int obe_count_table(const obe_model* m, int32_t law, const double* d_settings, int64_t ld_s, int64_t n_points,
                    const double* d_side, int64_t ld_side, const double* d_logfact, const double* d_particles,
                    int64_t ld_p, int64_t n_particles, const double* d_weights, int32_t count_max, double* d_pmf,
                    void* d_ws, int64_t ws_bytes, void* stream) {
    const char* who = "obe_count_table";
    if (!m || !d_settings || !d_side || !d_logfact || !d_particles || !d_weights || !d_pmf || !d_ws)
        return count_refuse(who, "null pointer");
    if (!is_law(law)) return count_refuse(who, "law is neither OBE_COUNT_BINOMIAL nor OBE_COUNT_POISSON");
    if (count_max < 0 || count_max > kCountMax) return count_refuse(who, "count_max outside 0..OBE_COUNT_MAX_OUTCOMES");
    if (ld_side < n_points) return count_refuse(who, "a row of d_side shorter than n_points");
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    if (int rc = cloud_pass_refusal(who, n_points, ld_s, n_particles, ld_p, ws_bytes,
                                    obe_count_workspace_bytes(n_particles, n_points, mm.n_channels, count_max)))
        return rc;
    const CloudPassPlan plan = cloud_pass_plan(n_particles, n_points, kCountWaves);
    double* recip = static_cast<double*>(d_ws);
    double* partials = recip + kRecipWords;
    hipStream_t st = as_stream(stream);
    const int width = count_max < kCountNarrow ? kCountNarrow : kCountWide;
    const int binomial = law == OBE_COUNT_BINOMIAL;
    const int fold_blocks = (int)((n_points + kBlock - 1) / kBlock);
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        count_recip_kernel<<<(kRecipWords + kBlock - 1) / kBlock, kBlock, 0, st>>>(recip);
        OBE_CHECK_LAUNCH("count_recip_kernel");
        auto pass = [&](auto LawTag, auto WidthTag, int c, int k0) {
            using Law = decltype(LawTag);
            constexpr int B = decltype(WidthTag)::value;
            count_table_kernel<Model, Law, B><<<plan.grid(), kWave, 0, st>>>(
                mm, d_settings, ld_s, n_points, d_side, ld_side, d_logfact, recip, d_particles, ld_p, n_particles,
                d_weights, c, k0, plan.chunk_len, partials);
        };
        for (int c = 0; c < Model::NC; ++c) {
            double* pmf_c = d_pmf + (int64_t)c * (count_max + 2) * n_points;
            for (int k0 = 0; k0 <= count_max; k0 += width) {
                if (binomial && width == kCountNarrow) pass(BinomialLaw{}, std::integral_constant<int, kCountNarrow>{}, c, k0);
                else if (binomial) pass(BinomialLaw{}, std::integral_constant<int, kCountWide>{}, c, k0);
                else if (width == kCountNarrow) pass(PoissonLaw{}, std::integral_constant<int, kCountNarrow>{}, c, k0);
                else pass(PoissonLaw{}, std::integral_constant<int, kCountWide>{}, c, k0);
                OBE_CHECK_LAUNCH("count_table_kernel");
                const int rows = std::min(width, count_max - k0 + 1);
                count_fold_kernel<<<dim3((unsigned)fold_blocks, (unsigned)rows), kBlock, 0, st>>>(
                    partials, plan.used, width, plan.n_pad, n_points, binomial, d_side + (int64_t)c * ld_side, d_logfact,
                    k0, count_max, pmf_c);
                OBE_CHECK_LAUNCH("count_fold_kernel");
            }
        }
        count_above_kernel<<<(int)((n_points * Model::NC + kBlock - 1) / kBlock), kBlock, 0, st>>>(
            d_pmf, Model::NC, count_max, n_points, binomial, d_side, ld_side);
        OBE_CHECK_LAUNCH("count_above_kernel");
        return 0;
    });
}

int obe_count_tails(const double* d_pmf, int32_t n_channels, int32_t count_max, int64_t n_points,
                    const double* d_counts, int64_t ld_k, double* d_lower, double* d_upper, void* stream) {
    const char* who = "obe_count_tails";
    if (!d_pmf || !d_counts) return count_refuse(who, "null pointer");
    if (!d_lower && !d_upper) return count_refuse(who, "null pointer for both d_lower and d_upper");
    if (const char* what = table_shape_refusal(n_channels, count_max, n_points)) return count_refuse(who, what);
    if (ld_k < n_points) return count_refuse(who, "a row of d_counts shorter than n_points");
    count_tails_kernel<<<(int)((n_points * n_channels + kBlock - 1) / kBlock), kBlock, 0, as_stream(stream)>>>(
        d_pmf, n_channels, count_max, n_points, d_counts, ld_k, d_lower, d_upper);
    OBE_CHECK_LAUNCH("count_tails_kernel");
    return 0;
}

int obe_count_quantiles(const double* d_pmf, int32_t n_channels, int32_t count_max, int64_t n_points,
                        const double* h_levels, int32_t n_levels, double* d_quantiles, void* stream) {
    const char* who = "obe_count_quantiles";
    if (!d_pmf || !h_levels || !d_quantiles) return count_refuse(who, "null pointer");
    if (const char* what = table_shape_refusal(n_channels, count_max, n_points)) return count_refuse(who, what);
    if (n_levels < 1 || n_levels > OBE_COUNT_MAX_LEVELS)
        return count_refuse(who, "n_levels outside 1..OBE_COUNT_MAX_LEVELS");
    CountLevels lv{};
    lv.n = n_levels;
    for (int j = 0; j < OBE_COUNT_MAX_LEVELS; ++j) {
        lv.q[j] = j < n_levels ? h_levels[j] : 0.5;
        if (!(lv.q[j] > 0.0 && lv.q[j] < 1.0)) return count_refuse(who, "a level outside the open interval (0, 1)");
    }
    count_quantiles_kernel<<<(int)((n_points * n_channels + kBlock - 1) / kBlock), kBlock, 0, as_stream(stream)>>>(
        d_pmf, n_channels, count_max, n_points, lv, d_quantiles);
    OBE_CHECK_LAUNCH("count_quantiles_kernel");
    return 0;
}

int obe_count_logpmf(const obe_model* m, int32_t law, const double* d_settings, int64_t ld_s, int64_t n_records,
                     const double* d_counts, int64_t ld_k, const double* d_side, int64_t ld_side,
                     const double* d_constant, const double* d_particles, int64_t ld_p, int64_t n_particles,
                     const double* d_weights, double* d_logpmf, void* d_ws, int64_t ws_bytes, void* stream) {
    const char* who = "obe_count_logpmf";
    if (!m || !d_settings || !d_counts || !d_side || !d_constant || !d_particles || !d_weights || !d_logpmf || !d_ws)
        return count_refuse(who, "null pointer");
    if (!is_law(law)) return count_refuse(who, "law is neither OBE_COUNT_BINOMIAL nor OBE_COUNT_POISSON");
    if (ld_k < n_records || ld_side < n_records)
        return count_refuse(who, "a row of d_counts or d_side shorter than n_records");
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    if (int rc = cloud_pass_refusal(who, n_records, ld_s, n_particles, ld_p, ws_bytes,
                                    obe_count_workspace_bytes(n_particles, n_records, mm.n_channels, 0)))
        return rc;
    const CloudPassPlan plan = cloud_pass_plan(n_particles, n_records, kCountWaves);
    double* partials = static_cast<double*>(d_ws);
    hipStream_t st = as_stream(stream);
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        if (law == OBE_COUNT_BINOMIAL)
            count_logpmf_kernel<Model, BinomialLaw><<<plan.grid(), kWave, 0, st>>>(
                mm, d_settings, ld_s, n_records, d_counts, ld_k, d_side, ld_side, d_particles, ld_p, n_particles,
                d_weights, plan.chunk_len, partials);
        else
            count_logpmf_kernel<Model, PoissonLaw><<<plan.grid(), kWave, 0, st>>>(
                mm, d_settings, ld_s, n_records, d_counts, ld_k, d_side, ld_side, d_particles, ld_p, n_particles,
                d_weights, plan.chunk_len, partials);
        OBE_CHECK_LAUNCH("count_logpmf_kernel");
        count_logpmf_fold_kernel<<<(int)((n_records + kBlock - 1) / kBlock), kBlock, 0, st>>>(
            partials, plan.used, plan.n_pad, n_records, d_constant, d_logpmf);
        OBE_CHECK_LAUNCH("count_logpmf_fold_kernel");
        return 0;
    });
}

}  // extern "C"
