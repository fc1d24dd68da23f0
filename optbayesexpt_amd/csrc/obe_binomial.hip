// K17 — yes/no outcomes (OptBayesExptBinomial).  The model's channel c gives a success probability p_c = f_c(x; theta);
// a record holds k_c successes in n_c shots per channel.
//   likelihood   lane <-> particle, one stream over the cloud: the factor the Bayes update multiplies the weights by,
//                L_i = exp(sum_c [k_c log p_c,i + (n_c - k_c) log1p(-p_c,i)]), a term whose count is 0 skipped, from the
//                model (M::eval, the bits obe_eval_over_particles writes) or from given model values.  HBM bound.
//   information  the exact mutual information, in nats, between theta and the joint outcome of ONE shot in every
//                channel, for every setting: U = H(mean outcome distribution) - mean of sum_c h2(p_c), over the whole
//                weighted cloud.  cloud_pass_kernel's geometry (obe_cloud_pass.h): one wave per workgroup,
//                lane <-> setting, the particle axis streamed (the same particle for all lanes), grid = setting tiles x
//                particle chunks, chunk partials folded in chunk order.  Per lane 2^C outcome sums, one sum of
//                w sum_c h2, C sums of w p (1 - p) — the variance of a shot, what the Gaussian utilities divide by —
//                and W.  No atomics: the same bits from run to run.  FP64-issue bound (C log and C log1p per
//                evaluation).
//   records      K19: l_i = sum_r sum_c [k log p + (n - k) log1p(-p)] + constant over a set of records, per particle:
//                the records x particles pass of obe_records_pass.h with BinRecordTerm below.  Per evaluation and
//                channel a log and a log1p, either skipped where its count is 0.  FP64-issue bound.
#include <cmath>

#include "obe_cloud_pass.h"
#include "obe_records_pass.h"

namespace obe {
namespace {

constexpr int kInfoWaves = 8192;                   // waves the pass aims at (32 per CU): chunks = this / setting tiles
constexpr int kBinMaxCh = OBE_BINOMIAL_MAX_CHANNELS;
constexpr double kInf = __builtin_huge_val();
constexpr double kNaN = __builtin_nan("");

// 2^C outcome sums; sum w sum_c h2; per channel sum w p (1 - p); then W
constexpr int info_slots(int n_channels) { return (1 << n_channels) + 1 + n_channels + 1; }

__device__ __forceinline__ bool is_probability(double p) { return p >= 0.0 && p <= 1.0; }      // (NaN fails)

struct BinLikArg {
    LikHead head;
    double k[kBinMaxCh];       // successes
    double f[kBinMaxCh];       // failures, n - k
};

// GIVEN: the model values come from y_in (C, n) rows ld_y apart; neither the cloud nor the setting is read
template <class M, bool GIVEN>
__global__ __launch_bounds__(kBlock) void binomial_lik_kernel(obe_model m, BinLikArg a, const double* __restrict__ y_in,
                                                              int64_t ld_y, const double* __restrict__ particles,
                                                              int64_t ld_p, int64_t n, double* __restrict__ lik) {
    static_assert(M::NC <= kBinMaxCh, "refused on the host");
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
        double y[M::NC];
        if (GIVEN) {
#pragma unroll
            for (int c = 0; c < M::NC; ++c) y[c] = y_in[(int64_t)c * ld_y + p];
        } else {
            M::eval(a.head.x, ParamRef{particles + p, ld_p}, m, y);
        }
        double arg = 0.0;
        bool ok = true;
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            ok = ok && is_probability(y[c]);
            if (c < a.head.n_ch) {
                if (a.k[c] > 0.0) arg += a.k[c] * log(y[c]);               // (p = 0 with k > 0: -inf, L = 0)
                if (a.f[c] > 0.0) arg += a.f[c] * log1p(-y[c]);
            }
        }
        double l = ok ? exp(arg) : 0.0;
        if (a.head.use_choke) l = pow(l, a.head.choke);
        lik[p] = l;
    }
}

// A lane's sums, info_slots(C) of them, over the chunk's contributing particles.  A particle contributes to a lane when
// its clean weight is > 0 and every p_c of that lane's setting is in [0, 1]; one that does not is carried through the
// arithmetic with weight 0 and p = 1/2, which leaves every sum's bits as they were.
template <int C>
struct BinAcc {
    static_assert(C <= kBinMaxCh, "refused on the host");
    static constexpr int NO = 1 << C, kSlots = info_slots(C);
    double po[NO], sv[C], sh, sw;

    __device__ __forceinline__ void add(double wp, const double (&y)[C]) {
        bool ok = true;
#pragma unroll
        for (int c = 0; c < C; ++c) ok = ok && is_probability(y[c]);
        const double wl = ok ? wp : 0.0;
        double q1[C], q0[C], h = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            q1[c] = ok ? y[c] : 0.5;
            q0[c] = 1.0 - q1[c];
            if (q1[c] > 0.0) h -= q1[c] * log(q1[c]);            // (0 log 0 = 0)
            if (q0[c] > 0.0) h -= q0[c] * log1p(-q1[c]);
            sv[c] = fma(wl * q1[c], q0[c], sv[c]);
        }
        sh = fma(wl, h, sh);
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            double pr = (o & 1) ? q1[0] : q0[0];
#pragma unroll
            for (int c = 1; c < C; ++c) pr *= ((o >> c) & 1) ? q1[c] : q0[c];
            po[o] = fma(wl, pr, po[o]);
        }
        sw += wl;
    }
    __device__ __forceinline__ void store(double* __restrict__ out, int64_t n_pad) const {
#pragma unroll
        for (int o = 0; o < NO; ++o) out[o * n_pad] = po[o];
        out[NO * n_pad] = sh;
#pragma unroll
        for (int c = 0; c < C; ++c) out[(NO + 1 + c) * n_pad] = sv[c];
        out[(NO + 1 + C) * n_pad] = sw;
    }
};

// The chunk partials added in chunk order, then per setting
//   info = max(-sum_o Pbar_o log Pbar_o - S_h / W, 0) / cost,  Pbar_o = S_o / W      (NaN stays NaN; W == 0 gives NaN)
//   noise_var (C, n_settings) = S_v,c / W / shots
// either output may be absent; each is formed from the partials alone
__global__ __launch_bounds__(kBlock) void binomial_fold_kernel(const double* __restrict__ partials, int chunks,
                                                               int n_channels, int64_t n_pad, int64_t n_s, double shots,
                                                               const double* __restrict__ cost_s, double cost,
                                                               double* __restrict__ info, double* __restrict__ noise_var) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_s) return;
    const int n_out = 1 << n_channels, slots = info_slots(n_channels);
    const double sw = chunk_order_sum(partials, chunks, slots, slots - 1, n_pad, s);
    if (info) {
        double hbar = 0.0;
        for (int o = 0; o < n_out; ++o) {
            const double pb = chunk_order_sum(partials, chunks, slots, o, n_pad, s) / sw;
            if (pb > 0.0) hbar -= pb * log(pb);                  // (0 log 0 = 0)
        }
        const double sh = chunk_order_sum(partials, chunks, slots, n_out, n_pad, s);
        double u = hbar - sh / sw;
        if (u < 0.0) u = 0.0;                                    // (rounding; a NaN is kept)
        if (!(sw > 0.0 && sw < kInf)) u = kNaN;
        info[s] = u / (cost_s ? cost_s[s] : cost);
    }
    if (noise_var) {
        for (int c = 0; c < n_channels; ++c) {
            const double v = chunk_order_sum(partials, chunks, slots, n_out + 1 + c, n_pad, s);
            noise_var[(int64_t)c * n_s + s] = v / sw / shots;
        }
    }
}

// a count of a record: finite and integer-valued
__host__ __device__ inline bool is_count(double v) { return v - v == 0.0 && v == std::floor(v); }      // (inf - inf and NaN - NaN are NaN)

// K19's term (obe_records_pass.h): w0 = k, w1 = n - k, formed once per record; k log p + (n - k) log1p(-p), a term
// whose count is 0 skipped (the record is the same for all lanes: a wave-uniform branch).  p = 0 with k > 0 and p = 1
// with n - k > 0 give -inf; a p that is NaN or outside [0, 1] fails the particle.
struct BinRecordTerm {
    static constexpr int kSide = 1, kMaxChannels = kBinMaxCh;
    struct Coef {};
    __device__ __forceinline__ static bool pack(double k, double n, double& w0, double& w1) {
        w0 = k;
        w1 = n - k;
        return is_count(k) && is_count(n) && k >= 0.0 && n >= 1.0 && k <= n;
    }
    __device__ __forceinline__ static void add(const Coef&, int, double p, double k, double f, double& acc, bool& ok) {
        ok = ok && is_probability(p);
        if (k > 0.0) acc += k * log(p);
        if (f > 0.0) acc += f * log1p(-p);
    }
};

}  // namespace
}  // namespace obe

using namespace obe;

extern "C" {

int obe_binomial_likelihood(const obe_model* m, const double* d_y, int64_t ld_y, const double* d_particles,
                            int64_t ld_p, int64_t n_particles, const double* h_setting, const double* h_successes,
                            const double* h_shots, int32_t n_lik_channels, double choke, double* d_lik, void* stream) {
    if (!m || !h_successes || !h_shots || !d_lik) return bad_arg("obe_binomial_likelihood: null pointer");
    if (n_particles < 1) return bad_arg("obe_binomial_likelihood: n_particles < 1");
    if (d_y ? ld_y < n_particles : (!d_particles || ld_p < n_particles))
        return bad_arg("obe_binomial_likelihood: no model values and no cloud, or a row shorter than n_particles");
    if (!d_y && !h_setting)
        return bad_arg("obe_binomial_likelihood: null pointer for h_setting, which the model is evaluated at");
    if (m->n_channels > kBinMaxCh)
        return bad_arg("obe_binomial_likelihood: the model has more than OBE_BINOMIAL_MAX_CHANNELS channels");
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    if (n_lik_channels < 0 || n_lik_channels > mm.n_channels)
        return bad_arg("obe_binomial_likelihood: n_lik_channels outside 0..the model's channels");
    BinLikArg a{lik_head(mm, n_lik_channels, choke, d_y ? nullptr : h_setting), {}, {}};
    for (int c = 0; c < n_lik_channels; ++c) {
        const double k = h_successes[c], n = h_shots[c];
        if (!is_count(k) || !is_count(n) || k < 0.0 || n < 1.0 || k > n)
            return bad_arg("obe_binomial_likelihood: a count is not an integer with 0 <= successes <= shots, shots >= 1");
        a.k[c] = k;
        a.f[c] = n - k;
    }
    hipStream_t st = as_stream(stream);
    const int nb = stream_blocks(n_particles, kBlock);
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        if constexpr (Model::NC > kBinMaxCh) {
            return bad_arg("obe_binomial_likelihood: the model has more than OBE_BINOMIAL_MAX_CHANNELS channels");
        } else {
            if (d_y)
                binomial_lik_kernel<Model, true><<<nb, kBlock, 0, st>>>(mm, a, d_y, ld_y, nullptr, 0, n_particles, d_lik);
            else
                binomial_lik_kernel<Model, false><<<nb, kBlock, 0, st>>>(mm, a, nullptr, 0, d_particles, ld_p,
                                                                         n_particles, d_lik);
            OBE_CHECK_LAUNCH("binomial_lik_kernel");
            return 0;
        }
    });
}

int64_t obe_binomial_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels) {
    (void)n_particles;                                           // (the chunks are bounded whatever the cloud)
    if (n_settings < 1) n_settings = 1;
    if (n_channels < 1) n_channels = 1;
    if (n_channels > kBinMaxCh) n_channels = kBinMaxCh;
    return cloud_pass_words(n_settings, info_slots(n_channels), kInfoWaves) * (int64_t)sizeof(double);
}

int obe_binomial_information(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                             const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                             double shots, const double* d_cost, double cost, double* d_information,
                             double* d_noise_var, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!m || !d_settings || !d_particles || !d_weights || !d_ws)
        return bad_arg("obe_binomial_information: null pointer");
    if (!d_information && !d_noise_var)
        return bad_arg("obe_binomial_information: null pointer for both d_information and d_noise_var");
    if (!(shots >= 1.0 && shots < kInf)) return bad_arg("obe_binomial_information: shots not finite or < 1");
    if (m->n_channels > kBinMaxCh)
        return bad_arg("obe_binomial_information: the model has more than OBE_BINOMIAL_MAX_CHANNELS channels");
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    if (int rc = cloud_pass_refusal("obe_binomial_information", n_settings, ld_s, n_particles, ld_p, ws_bytes,
                                    obe_binomial_workspace_bytes(n_particles, n_settings, mm.n_channels)))
        return rc;
    const CloudPassPlan plan = cloud_pass_plan(n_particles, n_settings, kInfoWaves);
    double* partials = static_cast<double*>(d_ws);
    hipStream_t st = as_stream(stream);
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        if constexpr (Model::NC > kBinMaxCh) {
            return bad_arg("obe_binomial_information: the model has more than OBE_BINOMIAL_MAX_CHANNELS channels");
        } else {
            cloud_pass_kernel<Model, BinAcc<Model::NC>><<<plan.grid(), kWave, 0, st>>>(
                mm, d_settings, ld_s, n_settings, d_particles, ld_p, n_particles, d_weights, plan.chunk_len, partials);
            OBE_CHECK_LAUNCH("cloud_pass_kernel");
            binomial_fold_kernel<<<(int)((n_settings + kBlock - 1) / kBlock), kBlock, 0, st>>>(
                partials, plan.used, Model::NC, plan.n_pad, n_settings, shots, d_cost, cost, d_information, d_noise_var);
            OBE_CHECK_LAUNCH("binomial_fold_kernel");
            return 0;
        }
    });
}

int64_t obe_binomial_records_loglik_workspace_bytes(int64_t n_particles, int64_t n_records, int32_t n_channels) {
    return records_pass_bytes(n_particles, n_records, n_channels);
}

int obe_binomial_records_loglik(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                                const double* d_successes, int64_t ld_k, const double* d_shots, int64_t ld_n,
                                double constant, const double* d_particles, int64_t ld_p, int64_t n_particles,
                                int32_t accumulate, double* d_loglik, void* d_ws, int64_t ws_bytes, void* stream) {
    return own_records_loglik<BinRecordTerm>("obe_binomial_records_loglik", m, d_settings, ld_s, n_records, d_successes,
                                             ld_k, d_shots, ld_n, BinRecordTerm::Coef{}, constant, d_particles, ld_p,
                                             n_particles, accumulate, d_loglik, d_ws, ws_bytes, stream);
}

}  // extern "C"
