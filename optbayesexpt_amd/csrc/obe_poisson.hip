// K18 — counted events (OptBayesExptPoisson).  The model's channel c gives a rate r_c = f_c(x; theta) in counts per unit
// exposure; a record holds k_c counted events in the exposure t_c per channel, lambda_c = t_c r_c.
//   likelihood   lane <-> particle, one stream over the cloud: the factor the Bayes update multiplies the weights by,
//                L_i = exp(sum_c [k_c log lambda_c,i - lambda_c,i - log k_c!]) — the Poisson pmf itself, every exponent
//                <= 0 —, a channel whose count is 0 contributing -lambda alone, from the model (M::eval, the bits
//                obe_eval_over_particles writes) or from given model values.  HBM bound.
//   information  the exact mutual information, in nats, between theta and the next reading's count censored at CAP
//                (outcomes 0 .. CAP-1 and ">= CAP"), for every setting, over the whole weighted cloud; models of ONE
//                channel.  cloud_pass_kernel's geometry (obe_cloud_pass.h): one wave per workgroup, lane <-> setting,
//                the particle axis streamed (the same particle for all lanes), grid = setting tiles x particle chunks,
//                chunk partials folded in chunk order.  Per evaluation one exp (p_0 = e^-lambda), one log lambda, the
//                recurrence p_k = p_k-1 (lambda / k) unrolled over the compile-time CAP — CAP outcome sums per lane in
//                registers —, one log tau.  CAP = 0: the instantiation without outcome sums, for any channel count,
//                which gives sum w r_c and W alone (the noise variance of the reading k / t).  No atomics: the same bits
//                from run to run.  FP64-issue bound (5 FP64 operations per outcome and evaluation).
//   records      K19: l_i = sum_r sum_c [k log lambda - lambda] + constant over a set of records, per particle: the
//                records x particles pass of obe_records_pass.h with PoisRecordTerm below.  Per evaluation and channel
//                one log, none where the count is 0.  FP64-issue bound.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "obe_cloud_pass.h"
#include "obe_records_pass.h"

namespace obe {
namespace {

constexpr int kPoisWaves = 4096;                   // waves the pass aims at (2 .. 4 fit a SIMD): chunks = this / tiles
constexpr int kPoisMaxCap = OBE_POISSON_MAX_CAP;
constexpr double kInf = __builtin_huge_val();
constexpr double kNaN = __builtin_nan("");

// log k! for k < OBE_POISSON_MAX_CAP, correctly rounded: compile-time indices only (the unrolled recurrence), so every
// entry is an immediate of the instruction stream and nothing is looked up at run time
__device__ constexpr double kLogFact[kPoisMaxCap] = {
    0.0, 0.0, 0.6931471805599453, 1.791759469228055,
    3.1780538303479458, 4.787491742782046, 6.579251212010101, 8.525161361065415,
    10.60460290274525, 12.801827480081469, 15.104412573075516, 17.502307845873887,
    19.987214495661885, 22.552163853123425, 25.19122118273868, 27.89927138384089,
    30.671860106080672, 33.50507345013689, 36.39544520803305, 39.339884187199495,
    42.335616460753485, 45.38013889847691, 48.47118135183523, 51.60667556776438,
    54.78472939811232, 58.00360522298052, 61.261701761002, 64.55753862700634,
    67.88974313718154, 71.25703896716801, 74.65823634883016, 78.0922235533153,
    81.55795945611504, 85.05446701758152, 88.58082754219768, 92.1361756036871,
    95.7196945421432, 99.33061245478743, 102.96819861451381, 106.63176026064346,
    110.32063971475739, 114.0342117814617, 117.77188139974507, 121.53308151543864,
    125.3172711493569, 129.12393363912722, 132.95257503561632, 136.80272263732635,
    140.67392364823425, 144.5657439463449, 148.47776695177302, 152.40959258449735,
    156.3608363030788, 160.3311282166309, 164.32011226319517, 168.32744544842765,
    172.3527971391628, 176.39584840699735, 180.45629141754378, 184.53382886144948,
    188.6281734236716, 192.7390472878449, 196.86618167289, 201.00931639928152,
};

// cap outcome sums, sum w tau, sum w h (both absent at cap = 0); per channel sum w r; then W
constexpr int pois_slots(int n_channels, int cap) { return (cap ? cap + 2 : 0) + n_channels + 1; }
inline bool is_cap(int cap) { return cap == 16 || cap == 32 || cap == 64; }

// finite and >= 0 (NaN fails), and so is exposure x rate
__device__ __forceinline__ bool is_rate(double r, double t) { return r >= 0.0 && r * t < kInf; }

struct PoisLikArg {
    LikHead head;
    double k[OBE_MAX_CHANNELS];        // counted events
    double t[OBE_MAX_CHANNELS];        // exposure
    double lf[OBE_MAX_CHANNELS];       // log k!
};

// GIVEN: the model values come from y_in (C, n) rows ld_y apart; neither the cloud nor the setting is read
template <class M, bool GIVEN>
__global__ __launch_bounds__(kBlock) void poisson_lik_kernel(obe_model m, PoisLikArg a, const double* __restrict__ y_in,
                                                             int64_t ld_y, const double* __restrict__ particles,
                                                             int64_t ld_p, int64_t n, double* __restrict__ lik) {
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
            const bool in = c < a.head.n_ch;
            ok = ok && is_rate(y[c], in ? a.t[c] : 1.0);
            if (in) {
                const double lam = a.t[c] * y[c];
                if (a.k[c] > 0.0) arg += a.k[c] * log(lam);            // (lambda = 0 with k > 0: -inf, L = 0)
                arg -= lam;
                arg -= a.lf[c];
            }
        }
        double l = ok ? exp(arg) : 0.0;
        if (a.head.use_choke) l = pow(l, a.head.choke);
        lik[p] = l;
    }
}

// partials (chunk, pois_slots(C, CAP), padded settings), sums over the chunk's contributing particles.  A particle
// contributes to a lane when its clean weight is > 0 and every r_c of that lane's setting is a rate; one that does not
// is carried through the arithmetic with weight 0 and r = 1, which leaves every sum's bits as they were.
// Per evaluation and outcome k >= 1: q = lambda (1 / k) (off the chain), p_k = p_k-1 q, the outcome sum's fma, s0 += p_k
// and s2 = fma(p_k, log k!, s2): the dependent chain is ONE multiplication per outcome among five operations, so a
// single wave already keeps the FP64 pipe issuing and two particles per trip would only double the live registers.
//   sum_k p_k (k log lambda - lambda - log k!) = log lambda . lambda (s0 - p_CAP-1) - lambda s0 - s2,  k p_k = lambda p_k-1
// (cloud_pass_kernel's scaffold restated: with these sums as an Acc of that kernel the schedule holds ten more VGPRs
// at cap 32 and a wave fewer fits a SIMD — profiles/own_noise_refactor.txt)
template <class M, int CAP>
__global__ __launch_bounds__(kWave) void poisson_info_kernel(obe_model m, const double* __restrict__ settings,
                                                             int64_t ld_s, int64_t n_s,
                                                             const double* __restrict__ particles, int64_t ld_p,
                                                             int64_t n, const double* __restrict__ w, double exposure,
                                                             int64_t chunk_len, double* __restrict__ partials) {
    constexpr int C = M::NC, NP = CAP ? CAP : 1;
    static_assert(CAP == 0 || C == 1, "refused on the host");
    static_assert(CAP <= kPoisMaxCap, "the log k! table");
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_s ? s : n_s - 1;                    // (the padding lanes repeat the last setting)
    double x[M::NS], po[NP], sr[C], st = 0.0, sh = 0.0, sw = 0.0;
#pragma unroll
    for (int k = 0; k < M::NS; ++k) x[k] = settings[(int64_t)k * ld_s + sc];
#pragma unroll
    for (int k = 0; k < NP; ++k) po[k] = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) sr[c] = 0.0;
    const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    for (int64_t p = p0; p < p1; ++p) {                          // (p, w[p] and the particle are the same for all lanes)
        const double wp = clean_weight(w[p]);
        if (wp == 0.0) continue;                                 // (whatever the model gives)
        double y[C];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
        bool ok = true;
#pragma unroll
        for (int c = 0; c < C; ++c) ok = ok && is_rate(y[c], exposure);
        const double wl = ok ? wp : 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) sr[c] = fma(wl, ok ? y[c] : 1.0, sr[c]);
        sw += wl;
        if constexpr (CAP > 0) {
            const double lam = exposure * (ok ? y[0] : 1.0);
            const double ll = log(lam > 0.0 ? lam : 1.0);        // (log lambda reads as 0 at lambda = 0; no branch)
            double pk = exp(-lam), s0 = pk, s2 = 0.0;
            po[0] = fma(wl, pk, po[0]);
#pragma unroll
            for (int k = 1; k < CAP; ++k) {
                pk *= lam * (1.0 / k);
                po[k] = fma(wl, pk, po[k]);
                s0 += pk;
                s2 = fma(pk, kLogFact[k], s2);
            }
            double tau = 1.0 - s0;
            if (!(tau > 0.0)) tau = 0.0;
            double h = s2 + lam * s0 - ll * (lam * (s0 - pk));
            h -= tau * log(tau > 0.0 ? tau : 1.0);               // (0 log 0 = 0; no branch: the fmas above stay put)
            st = fma(wl, tau, st);
            sh = fma(wl, h, sh);
        }
    }
    const int64_t n_pad = (int64_t)gridDim.x * kWave;
    double* out = partials + (int64_t)blockIdx.y * pois_slots(C, CAP) * n_pad + s;
    if constexpr (CAP > 0) {
#pragma unroll
        for (int k = 0; k < CAP; ++k) out[k * n_pad] = po[k];
        out[CAP * n_pad] = st;
        out[(CAP + 1) * n_pad] = sh;
        out += (CAP + 2) * n_pad;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) out[c * n_pad] = sr[c];
    out[C * n_pad] = sw;
}

// The chunk partials added in chunk order, then per setting, with W the last slot's sum,
//   pmf (cap + 1, n_settings) = S_k / W for k < cap, then taubar = S_tau / W;  tail = taubar
//   info = max(-sum_k Pbar_k log Pbar_k - taubar log taubar - S_h / W, 0) / cost        (NaN stays NaN; W == 0 gives NaN)
//   noise_var (C, n_settings) = S_r,c / W / exposure
// any output may be absent; each is formed from the partials alone.  cap = 0: the partials hold S_r and W only.
__global__ __launch_bounds__(kBlock) void poisson_fold_kernel(const double* __restrict__ partials, int chunks,
                                                              int n_channels, int cap, int64_t n_pad, int64_t n_s,
                                                              double exposure, const double* __restrict__ cost_s,
                                                              double cost, double* __restrict__ info,
                                                              double* __restrict__ tail, double* __restrict__ pmf,
                                                              double* __restrict__ noise_var) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_s) return;
    const int slots = pois_slots(n_channels, cap);
    const double sw = chunk_order_sum(partials, chunks, slots, slots - 1, n_pad, s);
    const bool nobody = !(sw > 0.0 && sw < kInf);
    if (cap > 0 && (info || tail || pmf)) {
        double hbar = 0.0;
        for (int k = 0; k <= cap; ++k) {                         // (slot cap: tau)
            const double so = chunk_order_sum(partials, chunks, slots, k, n_pad, s);
            const double pb = nobody ? kNaN : so / sw;
            if (pb > 0.0) hbar -= pb * log(pb);                  // (0 log 0 = 0)
            if (pmf) pmf[(int64_t)k * n_s + s] = pb;
            if (tail && k == cap) tail[s] = pb;
        }
        if (info) {
            const double sh = chunk_order_sum(partials, chunks, slots, cap + 1, n_pad, s);
            double u = hbar - sh / sw;
            if (u < 0.0) u = 0.0;                                // (rounding; a NaN is kept)
            if (nobody) u = kNaN;
            info[s] = u / (cost_s ? cost_s[s] : cost);
        }
    }
    if (noise_var) {
        const int first = cap ? cap + 2 : 0;
        for (int c = 0; c < n_channels; ++c) {
            const double v = chunk_order_sum(partials, chunks, slots, first + c, n_pad, s);
            noise_var[(int64_t)c * n_s + s] = v / sw / exposure;
        }
    }
}

// a count of a record: finite, integer-valued and >= 0
__host__ __device__ inline bool is_count(double v) { return v - v == 0.0 && v == std::floor(v) && v >= 0.0; }     // (inf - inf is NaN)
__host__ __device__ inline bool is_exposure(double t) { return t > 0.0 && t < kInf; }

// K19's term (obe_records_pass.h): w0 = k, w1 = t; k log lambda - lambda with lambda = t r, a channel whose count is 0
// contributing -lambda alone (the record is the same for all lanes: a wave-uniform branch).  lambda = 0 with k > 0
// gives -inf; an r that is not a rate fails the particle.
struct PoisRecordTerm {
    static constexpr int kSide = 1, kMaxChannels = OBE_MAX_CHANNELS;
    struct Coef {};
    __device__ __forceinline__ static bool pack(double k, double t, double& w0, double& w1) {
        w0 = k;
        w1 = t;
        return is_count(k) && is_exposure(t);
    }
    __device__ __forceinline__ static void add(const Coef&, int, double r, double k, double t, double& acc, bool& ok) {
        ok = ok && is_rate(r, t);
        const double lam = t * r;
        if (k > 0.0) acc += k * log(lam);
        acc -= lam;
    }
};

}  // namespace
}  // namespace obe

using namespace obe;

extern "C" {

int obe_poisson_likelihood(const obe_model* m, const double* d_y, int64_t ld_y, const double* d_particles,
                           int64_t ld_p, int64_t n_particles, const double* h_setting, const double* h_counts,
                           const double* h_exposure, const double* h_logfact, int32_t n_lik_channels, double choke,
                           double* d_lik, void* stream) {
    if (!m || !h_counts || !h_exposure || !h_logfact || !d_lik) return bad_arg("obe_poisson_likelihood: null pointer");
    if (n_particles < 1) return bad_arg("obe_poisson_likelihood: n_particles < 1");
    if (d_y ? ld_y < n_particles : (!d_particles || ld_p < n_particles))
        return bad_arg("obe_poisson_likelihood: no model values and no cloud, or a row shorter than n_particles");
    if (!d_y && !h_setting)
        return bad_arg("obe_poisson_likelihood: null pointer for h_setting, which the model is evaluated at");
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    if (n_lik_channels < 0 || n_lik_channels > mm.n_channels || n_lik_channels > OBE_MAX_CHANNELS)
        return bad_arg("obe_poisson_likelihood: n_lik_channels outside 0..the model's channels");
    PoisLikArg a{lik_head(mm, n_lik_channels, choke, d_y ? nullptr : h_setting), {}, {}, {}};
    for (int c = 0; c < n_lik_channels; ++c) {
        if (!is_count(h_counts[c]))
            return bad_arg("obe_poisson_likelihood: a count is not a whole number >= 0");
        if (!is_exposure(h_exposure[c])) return bad_arg("obe_poisson_likelihood: an exposure is not finite and > 0");
        a.k[c] = h_counts[c];
        a.t[c] = h_exposure[c];
        a.lf[c] = h_logfact[c];
    }
    hipStream_t st = as_stream(stream);
    const int nb = stream_blocks(n_particles, kBlock);
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        if (d_y)
            poisson_lik_kernel<Model, true><<<nb, kBlock, 0, st>>>(mm, a, d_y, ld_y, nullptr, 0, n_particles, d_lik);
        else
            poisson_lik_kernel<Model, false><<<nb, kBlock, 0, st>>>(mm, a, nullptr, 0, d_particles, ld_p, n_particles,
                                                                    d_lik);
        OBE_CHECK_LAUNCH("poisson_lik_kernel");
        return 0;
    });
}

int64_t obe_poisson_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels, int32_t cap) {
    (void)n_particles;                                           // (the chunks are bounded whatever the cloud)
    if (n_settings < 1) n_settings = 1;
    n_channels = std::min(std::max(n_channels, 1), OBE_MAX_CHANNELS);
    cap = cap <= 16 ? 16 : cap <= 32 ? 32 : kPoisMaxCap;         // (the next cap there is: the size never shrinks)
    return cloud_pass_words(n_settings, pois_slots(n_channels, cap), kPoisWaves) * (int64_t)sizeof(double);
}

int obe_poisson_information(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                            const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                            double exposure, int32_t cap, const double* d_cost, double cost, double* d_information,
                            double* d_tail, double* d_pmf, double* d_noise_var, void* d_ws, int64_t ws_bytes,
                            void* stream) {
    if (!m || !d_settings || !d_particles || !d_weights || !d_ws)
        return bad_arg("obe_poisson_information: null pointer");
    const bool outcomes = d_information || d_tail || d_pmf;
    if (!outcomes && !d_noise_var)
        return bad_arg("obe_poisson_information: null pointer for all of d_information, d_tail, d_pmf and d_noise_var");
    if (!is_exposure(exposure)) return bad_arg("obe_poisson_information: exposure not finite and > 0");
    if (!is_cap(cap)) return bad_arg("obe_poisson_information: cap is not 16, 32 or 64");
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    if (outcomes && mm.n_channels != 1)
        return bad_arg("obe_poisson_information: d_information, d_tail and d_pmf take a model of one channel "
                       "(d_noise_var alone works for every channel count)");
    if (int rc = cloud_pass_refusal("obe_poisson_information", n_settings, ld_s, n_particles, ld_p, ws_bytes,
                                    obe_poisson_workspace_bytes(n_particles, n_settings, mm.n_channels, cap)))
        return rc;
    const CloudPassPlan plan = cloud_pass_plan(n_particles, n_settings, kPoisWaves);
    double* partials = static_cast<double*>(d_ws);
    hipStream_t st = as_stream(stream);
    const int run_cap = outcomes ? cap : 0;                      // (no outcome sums where nobody asks for them)
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        auto launch = [&](auto CapTag) {
            constexpr int CAP = decltype(CapTag)::value;
            poisson_info_kernel<Model, CAP><<<plan.grid(), kWave, 0, st>>>(mm, d_settings, ld_s, n_settings, d_particles, ld_p,
                                                                    n_particles, d_weights, exposure, plan.chunk_len,
                                                                    partials);
        };
        if constexpr (Model::NC == 1) {
            switch (run_cap) {
                case 16: launch(std::integral_constant<int, 16>{}); break;
                case 32: launch(std::integral_constant<int, 32>{}); break;
                case 64: launch(std::integral_constant<int, 64>{}); break;
                default: launch(std::integral_constant<int, 0>{}); break;
            }
        } else {
            if (run_cap) return bad_arg("obe_poisson_information: the outcome sums take a model of one channel");
            launch(std::integral_constant<int, 0>{});
        }
        OBE_CHECK_LAUNCH("poisson_info_kernel");
        poisson_fold_kernel<<<(int)((n_settings + kBlock - 1) / kBlock), kBlock, 0, st>>>(
            partials, plan.used, Model::NC, run_cap, plan.n_pad, n_settings, exposure, d_cost, cost, d_information, d_tail,
            d_pmf, d_noise_var);
        OBE_CHECK_LAUNCH("poisson_fold_kernel");
        return 0;
    });
}

int64_t obe_poisson_records_loglik_workspace_bytes(int64_t n_particles, int64_t n_records, int32_t n_channels) {
    return records_pass_bytes(n_particles, n_records, n_channels);
}

int obe_poisson_records_loglik(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                               const double* d_counts, int64_t ld_k, const double* d_exposure, int64_t ld_t,
                               double constant, const double* d_particles, int64_t ld_p, int64_t n_particles,
                               int32_t accumulate, double* d_loglik, void* d_ws, int64_t ws_bytes, void* stream) {
    return own_records_loglik<PoisRecordTerm>("obe_poisson_records_loglik", m, d_settings, ld_s, n_records, d_counts,
                                              ld_k, d_exposure, ld_t, PoisRecordTerm::Coef{}, constant, d_particles,
                                              ld_p, n_particles, accumulate, d_loglik, d_ws, ws_bytes, stream);
}

}  // extern "C"
