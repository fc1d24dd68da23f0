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
#include "obe_cloud_pass.h"
#include "obe_records_pass.h"

namespace obe {
namespace {

constexpr int kNuWaves = 8192;                     // waves the pass aims at (32 per CU): chunks = this / setting tiles
constexpr double kInf = __builtin_huge_val();

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

}  // extern "C"
