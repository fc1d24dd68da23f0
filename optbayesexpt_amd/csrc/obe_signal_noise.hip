// K16 — measurement noise that depends on the signal (OptBayesExptSignalNoise).  Per channel c the noise variance of a
// reading whose noise-free value is y:  nu_c(y) = a_c + b_c |y| + c_c y^2  (a floor, a variance per unit of signal —
// counting noise —, a relative part), the three coefficients host data of the call.
//   likelihood  lane <-> particle, one stream over the cloud: the factor the Bayes update multiplies the weights by,
//               L_i = prod_c exp(-(y_c,i - y_meas,c)^2 / (2 nu_c(y_c,i))) / sqrt(nu_c(y_c,i)), from the model (M::eval, the
//               bits obe_eval_over_particles writes) or from given model values.  HBM bound: reads the cloud once,
//               writes N doubles.
//   variance    nu_bar_c(s) = a_c + b_c sum w |y| / W + c_c sum w y^2 / W over the whole weighted cloud, for every
//               setting: the noise variance a sweep divides by.  cloud_pass_kernel's geometry (obe_cloud_pass.h):
//               one wave per workgroup, lane <-> setting, the particle axis streamed (the same particle for all lanes:
//               scalar loads), grid = setting tiles x particle chunks, chunk partials folded in chunk order.  ONE pass:
//               both sums are sums of non-negative terms and need no centring; W rides along.  No atomics: the same
//               bits from run to run.  FP64-issue bound, like its sibling.
//   records     K19: l_i = sum_r sum_c [-(f - y)^2 / (2 nu) - log(nu) / 2] + constant over a set of records, per particle:
//               the records x particles pass of obe_records_pass.h with NoiseRecordTerm below.  Per evaluation and
//               channel one division and one log.  FP64-issue bound.
//   scoring     K21: the predictive of a READING, a mixture of N_p Gaussians whose component i has the mean f_c(x; theta_i)
//               and the variance nu_c(f_c(x; theta_i)): its log-density and tails for recorded readings (K11's geometry,
//               lane <-> record) and its quantiles for the next one (K15's, lane <-> setting, level groups).  Four
//               kernels — logpdf, tails, bracket, pass — further down; the folds, K15's state, its init and step
//               kernels and the chunk plans see no sigma and come from obe_score_pass.h.  A particle contributes by the
//               likelihood's rule: a weight > 0 and EVERY channel's nu > 0 and finite, so a NaN or +-inf model value in
//               any channel removes it from all channels — a stated difference from K11's tails, where +-inf counts as
//               mass at infinity.  The normalisers are K11's and K15's: the density and the tails divide by the sum of
//               ALL positive weights (a left-out particle has likelihood 0: the density stays the one-step evidence),
//               the quantiles by T over the contributing particles.  FP64-issue bound.
#include "obe_cloud_pass.h"
#include "obe_records_pass.h"
#include "obe_score_pass.h"

namespace obe {
namespace {

constexpr int kNuWaves = 8192;                     // waves the pass aims at (32 per CU): chunks = this / setting tiles

constexpr int nu_slots(int n_channels) { return 2 * n_channels + 1; }      // per channel sum w |y|, sum w y^2; then W

struct NoiseCoef {
    double a[OBE_MAX_CHANNELS], b[OBE_MAX_CHANNELS], c[OBE_MAX_CHANNELS];
};

__device__ __forceinline__ double nu_of(const NoiseCoef& k, int c, double y) {
    return k.a[c] + k.b[c] * fabs(y) + k.c[c] * (y * y);
}

struct LikArg {
    LikHead head;
    double y_meas[OBE_MAX_CHANNELS];
};

// GIVEN: the model values come from y_in (C, n) rows ld_y apart; neither the cloud nor the setting is read
template <class M, bool GIVEN>
__global__ __launch_bounds__(kBlock) void signal_noise_lik_kernel(obe_model m, LikArg a, NoiseCoef k,
                                                                  const double* __restrict__ y_in, int64_t ld_y,
                                                                  const double* __restrict__ particles, int64_t ld_p,
                                                                  int64_t n, double* __restrict__ lik) {
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
        double y[M::NC];
        if (GIVEN) {
#pragma unroll
            for (int c = 0; c < M::NC; ++c) y[c] = y_in[(int64_t)c * ld_y + p];
        } else {
            M::eval(a.head.x, ParamRef{particles + p, ld_p}, m, y);
        }
        double arg = 0.0, div = 1.0;
        bool ok = true;
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            if (c < a.head.n_ch) {
                const double nu = nu_of(k, c, y[c]);
                ok = ok && nu > 0.0 && nu < kInf;                // (NaN fails)
                const double d = y[c] - a.y_meas[c];
                arg += (d * d) / (2.0 * nu);
                div *= sqrt(nu);
            }
        }
        double l = ok ? exp(-arg) / div : 0.0;
        if (a.head.use_choke) l = pow(l, a.head.choke);
        lik[p] = l;
    }
}

// K19's term (obe_records_pass.h): w0 = the reading; -(f - y)^2 / (2 nu) - log(nu) / 2 with nu at the particle's own f.
// A nu that is not > 0 or not finite (a NaN or +-inf model output lands here) fails the particle.
struct NoiseRecordTerm {
    static constexpr int kSide = 0, kMaxChannels = OBE_MAX_CHANNELS;
    using Coef = NoiseCoef;
    __device__ __forceinline__ static bool pack(double y, double, double& w0, double&) {
        w0 = y;
        return true;
    }
    __device__ __forceinline__ static void add(const Coef& k, int c, double f, double y, double, double& acc, bool& ok) {
        const double nu = nu_of(k, c, f);
        ok = ok && nu > 0.0 && nu < kInf;                        // (NaN fails)
        const double d = f - y;
        acc -= (d * d) / (2.0 * nu);
        acc -= 0.5 * log(nu);
    }
};

// a lane's sums, nu_slots(C) of them: per channel sum w |y| and sum w y^2 over the chunk, then the chunk's W
template <int C>
struct NoiseAcc {
    static constexpr int kSlots = nu_slots(C);
    double s1[C], s2[C], sw;

    __device__ __forceinline__ void add(double wp, const double (&y)[C]) {
        sw += wp;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            s1[c] = fma(wp, fabs(y[c]), s1[c]);
            s2[c] = fma(wp * y[c], y[c], s2[c]);
        }
    }
    __device__ __forceinline__ void store(double* __restrict__ out, int64_t n_pad) const {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            out[(2 * c) * n_pad] = s1[c];
            out[(2 * c + 1) * n_pad] = s2[c];
        }
        out[(2 * C) * n_pad] = sw;
    }
};

// out (C, n_settings) = a + b S1 / W + c S2 / W, the chunk partials added in chunk order; W == 0 gives NaN
__global__ __launch_bounds__(kBlock) void signal_noise_fold_kernel(const double* __restrict__ partials, int chunks,
                                                                   int n_channels, int64_t n_pad, int64_t n_s, NoiseCoef k,
                                                                   double* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_s) return;
    const int slots = nu_slots(n_channels);
    const double sw = chunk_order_sum(partials, chunks, slots, 2 * n_channels, n_pad, s);
    for (int c = 0; c < n_channels; ++c) {
        double s1 = 0.0, s2 = 0.0;
        for (int j = 0; j < chunks; ++j) {                       // (one walk for both: their loads are in flight together)
            s1 += partials[((int64_t)j * slots + 2 * c) * n_pad + s];
            s2 += partials[((int64_t)j * slots + 2 * c + 1) * n_pad + s];
        }
        out[(int64_t)c * n_s + s] = k.a[c] + k.b[c] * (s1 / sw) + k.c[c] * (s2 / sw);
    }
}

// h_noise_coef: {a, b, c} per channel of the model; each finite and >= 0, one of a channel's three > 0
int fill_noise_coef(const char* who, NoiseCoef& k, const double* h_noise_coef, int n_channels) {
    static thread_local std::string msg;
    const char* what = nullptr;
    k = NoiseCoef{};
    if (!h_noise_coef) what = "h_noise_coef is NULL";
    for (int c = 0; c < n_channels && !what; ++c) {
        const double* v = h_noise_coef + 3 * c;
        for (int j = 0; j < 3; ++j)
            if (!(v[j] >= 0.0 && v[j] < kInf)) what = "a noise coefficient is not finite and >= 0";
        if (!what && !(v[0] > 0.0 || v[1] > 0.0 || v[2] > 0.0)) what = "a channel's noise coefficients are all zero";
        k.a[c] = v[0], k.b[c] = v[1], k.c[c] = v[2];
    }
    if (!what) return 0;
    msg = std::string(who) + ": " + what;
    return bad_arg(msg.c_str());
}

// ---- K21: scoring a reading and quantiles of the next one with nu at every particle's own model value.  The kernels of
// K11 / K15 (obe_predict.hip) with the width taken from the model value just computed instead of from a row of the cloud;
// their partials have K11's / K15's layout, so obe_score_pass.h's folds, init and step kernels read them.

// nu of every channel at a particle's model values y; false: one of them is not > 0 or not finite (NaN fails) — the
// likelihood's rule, one verdict for all channels
template <class M>
__device__ __forceinline__ bool noise_of(const NoiseCoef& k, const double* y, double* nu) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < M::NC; ++c) {
        nu[c] = nu_of(k, c, y[c]);
        ok = ok && nu[c] > 0.0 && nu[c] < kInf;
    }
    return ok;
}

// partials (chunk, 2, padded records): the chunk's (m, S) of sum_i w_i exp(l_i), l_i = sum_c [-(f_c - y_c)^2 / (2 nu_c) -
// log(nu_c) / 2] — NoiseRecordTerm's arithmetic.  Lane = one record.
template <class M>
__global__ __launch_bounds__(kWave) void signal_logpdf_kernel(obe_model m, const double* __restrict__ settings, int64_t ld_s,
                                                              int64_t n_r, const double* __restrict__ y_meas, int64_t ld_y,
                                                              NoiseCoef k, const double* __restrict__ particles,
                                                              int64_t ld_p, int64_t n, const double* __restrict__ w,
                                                              int64_t chunk_len, double* __restrict__ partials) {
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_r ? s : n_r - 1;                    // (the padding lanes repeat the last record)
    double x[M::NS], ym[M::NC];
#pragma unroll
    for (int d = 0; d < M::NS; ++d) x[d] = settings[(int64_t)d * ld_s + sc];
#pragma unroll
    for (int c = 0; c < M::NC; ++c) ym[c] = y_meas[(int64_t)c * ld_y + sc];
    double top = -kInf, S = 0.0;
    const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    for (int64_t p = p0; p < p1; ++p) {                          // (p, w[p] and the particle are the same for all lanes)
        const double wp = clean_weight(w[p]);
        if (wp == 0.0) continue;
        double y[M::NC], nu[M::NC];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
        const bool ok = noise_of<M>(k, y, nu);
        double l = 0.0;
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            const double d = y[c] - ym[c];
            l -= (d * d) / (2.0 * nu[c]);
            l -= 0.5 * log(nu[c]);
        }
        if (ok && fabs(l) < kInf) lse_add(top, S, l, wp);          // (NaN and -inf contribute nothing)
    }
    const int64_t n_pad = (int64_t)gridDim.x * kWave;
    partials[((int64_t)blockIdx.y * 2 + 0) * n_pad + s] = top;
    partials[((int64_t)blockIdx.y * 2 + 1) * n_pad + s] = S;
}

// partials (chunk, 2 C, padded records): sum w P(Y_c <= y_meas_c | particle), then sum w P(Y_c >= y_meas_c | particle),
// z_c = (f_c - y_meas_c) / sqrt(nu_c).  The small one of the two is erfc(|z| / sqrt 2) / 2 itself, the large one 1 - that.
template <class M>
__global__ __launch_bounds__(kWave) void signal_tails_kernel(obe_model m, const double* __restrict__ settings, int64_t ld_s,
                                                             int64_t n_r, const double* __restrict__ y_meas, int64_t ld_y,
                                                             NoiseCoef k, const double* __restrict__ particles,
                                                             int64_t ld_p, int64_t n, const double* __restrict__ w,
                                                             int64_t chunk_len, double* __restrict__ partials) {
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_r ? s : n_r - 1;
    double x[M::NS], ym[M::NC], lo[M::NC], hi[M::NC];
#pragma unroll
    for (int d = 0; d < M::NS; ++d) x[d] = settings[(int64_t)d * ld_s + sc];
#pragma unroll
    for (int c = 0; c < M::NC; ++c) {
        ym[c] = y_meas[(int64_t)c * ld_y + sc];
        lo[c] = hi[c] = 0.0;
    }
    const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    for (int64_t p = p0; p < p1; ++p) {
        const double wp = clean_weight(w[p]);
        if (wp == 0.0) continue;
        double y[M::NC], nu[M::NC];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
        if (!noise_of<M>(k, y, nu)) continue;                    // (this lane's: the others go on)
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            const double z = (y[c] - ym[c]) * (1.0 / sqrt(nu[c]));      // > 0: the model lies above the reading
            if (z == z) {
                const double small = 0.5 * erfc(fabs(z) * kSqrtHalf), large = 1.0 - small;
                lo[c] += wp * (z > 0.0 ? small : large);
                hi[c] += wp * (z > 0.0 ? large : small);
            }
        }
    }
    const int64_t n_pad = (int64_t)gridDim.x * kWave;
#pragma unroll
    for (int c = 0; c < M::NC; ++c) {
        partials[((int64_t)blockIdx.y * 2 * M::NC + c) * n_pad + s] = lo[c];
        partials[((int64_t)blockIdx.y * 2 * M::NC + M::NC + c) * n_pad + s] = hi[c];
    }
}

// partials (chunk, C (1 + 2 n_q), padded settings): T_c, then per (level, channel) the min of f + z_lo sqrt(nu) and the
// max of f + z_hi sqrt(nu) over the contributing particles: the bracket argument holds for a width per particle.  T_c is
// the same for every channel (one verdict per particle) and is written by the first level group.
template <class M>
__global__ __launch_bounds__(kWave) void signal_bracket_kernel(obe_model m, const double* __restrict__ settings, int64_t ld_s,
                                                               int64_t n_s, NoiseCoef k,
                                                               const double* __restrict__ particles, int64_t ld_p,
                                                               int64_t n, const double* __restrict__ w, int64_t chunk_len,
                                                               ReadLevels lv, double* __restrict__ partials) {
    constexpr int G = M::NC < kReadSlots ? kReadSlots / M::NC : 1;
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_s ? s : n_s - 1;                    // (the padding lanes repeat the last setting)
    const int j0 = blockIdx.z * G;
    double x[M::NS], T = 0.0, mn[G][M::NC], mx[G][M::NC], zl[G], zh[G];
#pragma unroll
    for (int d = 0; d < M::NS; ++d) x[d] = settings[(int64_t)d * ld_s + sc];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int j = j0 + g < lv.n ? j0 + g : lv.n - 1;         // (levels beyond the call's repeat the last: not written)
        zl[g] = lv.z_lo[j];
        zh[g] = lv.z_hi[j];
#pragma unroll
        for (int c = 0; c < M::NC; ++c) mn[g][c] = kInf, mx[g][c] = -kInf;
    }
    const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    for (int64_t p = p0; p < p1; ++p) {                          // (p, w[p] and the particle are the same for all lanes)
        const double wp = clean_weight(w[p]);
        if (wp == 0.0) continue;
        double y[M::NC], nu[M::NC];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
        if (!noise_of<M>(k, y, nu)) continue;                    // (a finite nu: every f is finite too)
        T += wp;
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            const double sg = sqrt(nu[c]);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                mn[g][c] = fmin(mn[g][c], y[c] + zl[g] * sg);
                mx[g][c] = fmax(mx[g][c], y[c] + zh[g] * sg);
            }
        }
    }
    const int64_t n_pad = (int64_t)gridDim.x * kWave;
    double* out = partials + (int64_t)blockIdx.y * (M::NC * (1 + 2 * lv.n)) * n_pad + s;
#pragma unroll
    for (int c = 0; c < M::NC; ++c) {
        if (blockIdx.z == 0) out[c * n_pad] = T;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (j0 + g < lv.n) {
                out[(M::NC + ((j0 + g) * M::NC + c) * 2) * n_pad] = mn[g][c];
                out[(M::NC + ((j0 + g) * M::NC + c) * 2 + 1) * n_pad] = mx[g][c];
            }
        }
    }
}

// partials (chunk, n_q C, 2, padded settings): A and sqrt(2 pi) D = sum w exp(-z^2 / 2) / sqrt(nu) of the open rows at
// their trials.  The model, sqrt(nu) and its reciprocal are formed once per (setting, particle, channel) and shared by the
// group's levels.  A workgroup whose tile has no open row in its group returns at once: the count was written by the
// launch before.
template <class M>
__global__ __launch_bounds__(kWave) void signal_pass_kernel(obe_model m, const double* __restrict__ settings, int64_t ld_s,
                                                            int64_t n_s, NoiseCoef k, const double* __restrict__ particles,
                                                            int64_t ld_p, int64_t n, const double* __restrict__ w,
                                                            int64_t chunk_len, ReadLevels lv, ReadState st) {
    constexpr int G = M::NC < kReadSlots ? kReadSlots / M::NC : 1;
    if (st.tile_open[(int64_t)blockIdx.z * gridDim.x + blockIdx.x] == 0) return;
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_s ? s : n_s - 1;                    // (the padding lanes repeat the last setting: never open)
    const int64_t n_pad = (int64_t)gridDim.x * kWave;
    const int j0 = blockIdx.z * G;
    double x[M::NS], yt[G][M::NC], A[G][M::NC], D[G][M::NC];
    bool open[G][M::NC], up[G];
#pragma unroll
    for (int d = 0; d < M::NS; ++d) x[d] = settings[(int64_t)d * ld_s + sc];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const bool live = j0 + g < lv.n;
        up[g] = live && lv.upper[live ? j0 + g : 0] != 0;
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            const int64_t idx = ((int64_t)(live ? j0 + g : 0) * M::NC + c) * n_pad + s;
            open[g][c] = live && st.open[idx] != 0;
            yt[g][c] = open[g][c] ? st.trial[idx] : 0.0;
            A[g][c] = D[g][c] = 0.0;
        }
    }
    const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    for (int64_t p = p0; p < p1; ++p) {                          // (p, w[p] and the particle are the same for all lanes)
        const double wp = clean_weight(w[p]);
        if (wp == 0.0) continue;
        double y[M::NC], nu[M::NC];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
        if (!noise_of<M>(k, y, nu)) continue;
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            const double inv = 1.0 / sqrt(nu[c]);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (open[g][c]) {
                    const double z = (y[c] - yt[g][c]) * inv;             // > 0: the model lies above the trial
                    const double small = 0.5 * erfc(fabs(z) * kSqrtHalf), large = 1.0 - small;
                    A[g][c] += wp * ((z > 0.0) == up[g] ? large : small);
                    D[g][c] += wp * (exp(-0.5 * (z * z)) * inv);
                }
            }
        }
    }
    double* out = st.partials + (int64_t)blockIdx.y * (2 * M::NC * lv.n) * n_pad + s;
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            if (open[g][c]) {
                out[(((j0 + g) * M::NC + c) * 2) * n_pad] = A[g][c];
                out[(((j0 + g) * M::NC + c) * 2 + 1) * n_pad] = D[g][c];
            }
        }
    }
}

// What the three entry points of K21 share: everything that can refuse the call — the coefficients among it, before any
// launch —, then the launch geometry (ScorePlan, obe_score_pass.h).
struct NoiseScore : ScorePlan {
    obe_model mm;
    NoiseCoef k;
    int prepare(const char* who, const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                const double* d_y_meas, int64_t ld_y, const double* h_noise_coef, const double* d_particles, int64_t ld_p,
                int64_t n_particles, const double* d_weights, void* d_ws, int64_t ws_bytes, int n_q = 0) {      // n_q > 0: no y_meas
        static thread_local std::string msg;
        auto refuse = [&](const char* what) {
            msg = std::string(who) + ": " + what;
            return bad_arg(msg.c_str());
        };
        if (!d_y_meas && !n_q) return refuse("null pointer");
        if (int rc = check_inputs(who, m, d_settings, ld_s, n_records, d_particles, ld_p, n_particles, d_weights, d_ws))
            return rc;
        if (!n_q && ld_y < n_records) return refuse("a row of y_meas shorter than n_records");
        mm = *m;
        if (int rc = obe_model_validate(&mm)) return rc;
        if (int rc = fill_noise_coef(who, k, h_noise_coef, mm.n_channels)) return rc;
        if (const char* what = plan(n_particles, n_records, mm.n_channels, n_q, d_ws, ws_bytes)) return refuse(what);
        return 0;
    }
};

}  // namespace
}  // namespace obe

using namespace obe;

extern "C" {

int obe_signal_noise_likelihood(const obe_model* m, const double* d_y, int64_t ld_y, const double* d_particles,
                                int64_t ld_p, int64_t n_particles, const double* h_setting, const double* h_y_meas,
                                const double* h_noise_coef, int32_t n_lik_channels, double choke, double* d_lik,
                                void* stream) {
    if (!m || !h_y_meas || !d_lik || n_particles < 1) return bad_arg("obe_signal_noise_likelihood: bad pointer/size");
    if (d_y ? ld_y < n_particles : (!d_particles || ld_p < n_particles))
        return bad_arg("obe_signal_noise_likelihood: no model values and no cloud, or a row shorter than n_particles");
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    if (n_lik_channels < 0 || n_lik_channels > mm.n_channels)
        return bad_arg("obe_signal_noise_likelihood: n_lik_channels outside 0..the model's channels");
    NoiseCoef k;
    if (int rc = fill_noise_coef("obe_signal_noise_likelihood", k, h_noise_coef, mm.n_channels)) return rc;
    // (a NULL h_setting is taken: the model is then evaluated at zeros)
    LikArg a{lik_head(mm, n_lik_channels, choke, d_y ? nullptr : h_setting), {}};
    for (int c = 0; c < n_lik_channels; ++c) a.y_meas[c] = h_y_meas[c];
    hipStream_t st = as_stream(stream);
    const int nb = stream_blocks(n_particles, kBlock);
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        if (d_y)
            signal_noise_lik_kernel<Model, true><<<nb, kBlock, 0, st>>>(mm, a, k, d_y, ld_y, nullptr, 0, n_particles, d_lik);
        else
            signal_noise_lik_kernel<Model, false><<<nb, kBlock, 0, st>>>(mm, a, k, nullptr, 0, d_particles, ld_p,
                                                                         n_particles, d_lik);
        OBE_CHECK_LAUNCH("signal_noise_lik_kernel");
        return 0;
    });
}

int64_t obe_signal_noise_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels) {
    (void)n_particles;                                           // (the chunks are bounded whatever the cloud)
    if (n_settings < 1) n_settings = 1;
    if (n_channels < 1) n_channels = 1;
    return cloud_pass_words(n_settings, nu_slots(n_channels), kNuWaves) * (int64_t)sizeof(double);
}

int obe_signal_noise_variance(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                              const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                              const double* h_noise_coef, double* d_noise_var, void* d_ws, int64_t ws_bytes,
                              void* stream) {
    if (!m || !d_settings || !d_particles || !d_weights || !d_noise_var || !d_ws)
        return bad_arg("obe_signal_noise_variance: null pointer");
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    NoiseCoef k;
    if (int rc = fill_noise_coef("obe_signal_noise_variance", k, h_noise_coef, mm.n_channels)) return rc;
    if (int rc = cloud_pass_refusal("obe_signal_noise_variance", n_settings, ld_s, n_particles, ld_p, ws_bytes,
                                    obe_signal_noise_workspace_bytes(n_particles, n_settings, mm.n_channels)))
        return rc;
    const CloudPassPlan plan = cloud_pass_plan(n_particles, n_settings, kNuWaves);
    double* partials = static_cast<double*>(d_ws);
    hipStream_t st = as_stream(stream);
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        cloud_pass_kernel<Model, NoiseAcc<Model::NC>><<<plan.grid(), kWave, 0, st>>>(
            mm, d_settings, ld_s, n_settings, d_particles, ld_p, n_particles, d_weights, plan.chunk_len, partials);
        OBE_CHECK_LAUNCH("cloud_pass_kernel");
        signal_noise_fold_kernel<<<(int)((n_settings + kBlock - 1) / kBlock), kBlock, 0, st>>>(
            partials, plan.used, Model::NC, plan.n_pad, n_settings, k, d_noise_var);
        OBE_CHECK_LAUNCH("signal_noise_fold_kernel");
        return 0;
    });
}

int64_t obe_signal_noise_records_loglik_workspace_bytes(int64_t n_particles, int64_t n_records, int32_t n_channels) {
    return records_pass_bytes(n_particles, n_records, n_channels);
}

int obe_signal_noise_records_loglik(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                                    const double* d_y_meas, int64_t ld_y, const double* h_noise_coef, double constant,
                                    const double* d_particles, int64_t ld_p, int64_t n_particles, int32_t accumulate,
                                    double* d_loglik, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!m) return bad_arg("obe_signal_noise_records_loglik: null pointer");
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    NoiseCoef k;
    if (int rc = fill_noise_coef("obe_signal_noise_records_loglik", k, h_noise_coef, mm.n_channels)) return rc;
    return own_records_loglik<NoiseRecordTerm>("obe_signal_noise_records_loglik", m, d_settings, ld_s, n_records,
                                               d_y_meas, ld_y, nullptr, 0, k, constant, d_particles, ld_p, n_particles,
                                               accumulate, d_loglik, d_ws, ws_bytes, stream);
}

int obe_signal_noise_logpdf(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                            const double* d_y_meas, int64_t ld_y, const double* h_noise_coef, const double* d_particles,
                            int64_t ld_p, int64_t n_particles, const double* d_weights, double* d_logpdf, void* d_ws,
                            int64_t ws_bytes, void* stream) {
    if (!d_logpdf) return bad_arg("obe_signal_noise_logpdf: null pointer");
    NoiseScore sc;
    if (int rc = sc.prepare("obe_signal_noise_logpdf", m, d_settings, ld_s, n_records, d_y_meas, ld_y, h_noise_coef,
                            d_particles, ld_p, n_particles, d_weights, d_ws, ws_bytes))
        return rc;
    hipStream_t st = as_stream(stream);
    double* partials = reinterpret_cast<double*>(sc.ws.body);
    if (int rc = enqueue_scale(d_weights, n_particles, sc.ws, st)) return rc;
    return dispatch_model(sc.mm, [&](auto M) -> int {
        using Model = decltype(M);
        signal_logpdf_kernel<Model><<<dim3((unsigned)sc.tiles, (unsigned)sc.used), kWave, 0, st>>>(
            sc.mm, d_settings, ld_s, n_records, d_y_meas, ld_y, sc.k, d_particles, ld_p, n_particles, d_weights,
            sc.chunk_len, partials);
        OBE_CHECK_LAUNCH("signal_logpdf_kernel");
        score_logpdf_fold_kernel<<<(int)((n_records + kBlock - 1) / kBlock), kBlock, 0, st>>>(
            partials, sc.used, Model::NC, sc.tiles * kWave, n_records, sc.ws.hdr, d_logpdf);
        OBE_CHECK_LAUNCH("score_logpdf_fold_kernel");
        return 0;
    });
}

int obe_signal_noise_tails(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                           const double* d_y_meas, int64_t ld_y, const double* h_noise_coef, const double* d_particles,
                           int64_t ld_p, int64_t n_particles, const double* d_weights, double* d_lower, double* d_upper,
                           void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_lower || !d_upper) return bad_arg("obe_signal_noise_tails: null pointer");
    NoiseScore sc;
    if (int rc = sc.prepare("obe_signal_noise_tails", m, d_settings, ld_s, n_records, d_y_meas, ld_y, h_noise_coef,
                            d_particles, ld_p, n_particles, d_weights, d_ws, ws_bytes))
        return rc;
    hipStream_t st = as_stream(stream);
    double* partials = reinterpret_cast<double*>(sc.ws.body);
    if (int rc = enqueue_scale(d_weights, n_particles, sc.ws, st)) return rc;
    return dispatch_model(sc.mm, [&](auto M) -> int {
        using Model = decltype(M);
        signal_tails_kernel<Model><<<dim3((unsigned)sc.tiles, (unsigned)sc.used), kWave, 0, st>>>(
            sc.mm, d_settings, ld_s, n_records, d_y_meas, ld_y, sc.k, d_particles, ld_p, n_particles, d_weights,
            sc.chunk_len, partials);
        OBE_CHECK_LAUNCH("signal_tails_kernel");
        score_tails_fold_kernel<<<(int)((n_records + kBlock - 1) / kBlock), kBlock, 0, st>>>(
            partials, sc.used, Model::NC, sc.tiles * kWave, n_records, sc.ws.hdr, d_lower, d_upper);
        OBE_CHECK_LAUNCH("score_tails_fold_kernel");
        return 0;
    });
}

int obe_signal_noise_reading_quantiles(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                                       const double* h_noise_coef, const double* d_particles, int64_t ld_p,
                                       int64_t n_particles, const double* d_weights, const double* h_q, const double* h_z,
                                       int32_t n_q, int32_t max_passes, double* d_quantiles, int32_t* d_passes, void* d_ws,
                                       int64_t ws_bytes, void* stream) {
    const char* who = "obe_signal_noise_reading_quantiles";
    if (!d_quantiles || !d_passes) return bad_arg("obe_signal_noise_reading_quantiles: null pointer");
    ReadLevels lv;
    if (int rc = fill_read_levels(who, lv, h_q, h_z, n_q, max_passes)) return rc;
    NoiseScore sc;
    if (int rc = sc.prepare(who, m, d_settings, ld_s, n_settings, nullptr, 0, h_noise_coef, d_particles, ld_p, n_particles,
                            d_weights, d_ws, ws_bytes, n_q))
        return rc;
    hipStream_t st = as_stream(stream);
    const ReadState state = read_carve(sc.ws.body, n_settings, sc.mm.n_channels, n_q);
    return dispatch_model(sc.mm, [&](auto M) -> int {
        using Model = decltype(M);
        const int group = read_group_of(Model::NC), groups = (n_q + group - 1) / group;
        const dim3 grid((unsigned)sc.tiles, (unsigned)sc.used, (unsigned)groups);
        const dim3 fold_grid((unsigned)sc.tiles, (unsigned)groups), fold_block(kWave, (unsigned)(group * Model::NC));
        const int64_t n_pad = sc.tiles * kWave;
        signal_bracket_kernel<Model><<<grid, kWave, 0, st>>>(sc.mm, d_settings, ld_s, n_settings, sc.k, d_particles, ld_p,
                                                             n_particles, d_weights, sc.chunk_len, lv, state.partials);
        OBE_CHECK_LAUNCH("signal_bracket_kernel");
        reading_init_kernel<<<fold_grid, fold_block, 0, st>>>(sc.used, Model::NC, group, lv, n_pad, n_settings, state,
                                                              d_quantiles, d_passes);
        OBE_CHECK_LAUNCH("reading_init_kernel");
        for (int pass = 1; pass <= max_passes; ++pass) {         // a fixed budget: nothing is waited for
            signal_pass_kernel<Model><<<grid, kWave, 0, st>>>(sc.mm, d_settings, ld_s, n_settings, sc.k, d_particles, ld_p,
                                                              n_particles, d_weights, sc.chunk_len, lv, state);
            OBE_CHECK_LAUNCH("signal_pass_kernel");
            reading_step_kernel<<<fold_grid, fold_block, 0, st>>>(sc.used, Model::NC, group, lv, n_pad, n_settings, state, pass,
                                                                  max_passes, d_quantiles, d_passes);
            OBE_CHECK_LAUNCH("reading_step_kernel");
        }
        return 0;
    });
}

}  // extern "C"
