// K16 — measurement noise that depends on the signal (OptBayesExptSignalNoise).  Per channel c the noise variance of a
// reading whose noise-free value is y:  nu_c(y) = a_c + b_c |y| + c_c y^2  (a floor, a variance per unit of signal —
// counting noise —, a relative part), the three coefficients host data of the call.
//   likelihood  lane <-> particle, one stream over the cloud: the factor the Bayes update multiplies the weights by,
//               L_i = prod_c exp(-(y_c,i - y_meas,c)^2 / (2 nu_c(y_c,i))) / sqrt(nu_c(y_c,i)), from the model (M::eval, the
//               bits obe_eval_over_particles writes) or from given model values.  HBM bound: reads the cloud once,
//               writes N doubles.
//   variance    nu_bar_c(s) = a_c + b_c sum w |y| / W + c_c sum w y^2 / W over the whole weighted cloud, for every
//               setting: the noise variance a sweep divides by.  predict_moment_kernel's geometry (obe_predict.hip):
//               one wave per workgroup, lane <-> setting, the particle axis streamed (the same particle for all lanes:
//               scalar loads), grid = setting tiles x particle chunks, chunk partials folded in chunk order.  ONE pass:
//               both sums are sums of non-negative terms and need no centring; W rides along.  No atomics: the same
//               bits from run to run.  FP64-issue bound, like its sibling.
#include <algorithm>

#include "obe_models.h"
#include "obe_select.h"

namespace obe {
namespace {

constexpr int kNuWaves = 8192;                     // waves the pass aims at (32 per CU): chunks = this / setting tiles
constexpr int kNuMinChunk = 256;                   // particles per chunk at least
constexpr double kInf = __builtin_huge_val();

inline int64_t nu_tiles(int64_t n_settings) { return (n_settings + kWave - 1) / kWave; }
inline int nu_chunks(int64_t n_particles, int64_t n_settings) {
    const int64_t by_size = (n_particles + kNuMinChunk - 1) / kNuMinChunk;
    const int64_t by_grid = std::max<int64_t>(1, kNuWaves / nu_tiles(n_settings));
    return (int)std::max<int64_t>(1, std::min(by_size, by_grid));
}
constexpr int nu_slots(int n_channels) { return 2 * n_channels + 1; }      // per channel sum w |y|, sum w y^2; then W
// chunks x padded settings <= kNuWaves x 64 + the padded settings, whatever the cloud
inline int64_t nu_words(int64_t n_settings, int n_channels) {
    return ((int64_t)kNuWaves + nu_tiles(n_settings)) * kWave * nu_slots(n_channels);
}

struct NoiseCoef {
    double a[OBE_MAX_CHANNELS], b[OBE_MAX_CHANNELS], c[OBE_MAX_CHANNELS];
};

__device__ __forceinline__ double nu_of(const NoiseCoef& k, int c, double y) {
    return k.a[c] + k.b[c] * fabs(y) + k.c[c] * (y * y);
}

struct LikArg {
    int n_ch;          // channels entering the product
    int use_choke;
    double choke;
    double x[OBE_MAX_SETDIMS];
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
            M::eval(a.x, ParamRef{particles + p, ld_p}, m, y);
        }
        double arg = 0.0, div = 1.0;
        bool ok = true;
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            if (c < a.n_ch) {
                const double nu = nu_of(k, c, y[c]);
                ok = ok && nu > 0.0 && nu < kInf;                // (NaN fails)
                const double d = y[c] - a.y_meas[c];
                arg += (d * d) / (2.0 * nu);
                div *= sqrt(nu);
            }
        }
        double l = ok ? exp(-arg) / div : 0.0;
        if (a.use_choke) l = pow(l, a.choke);
        lik[p] = l;
    }
}

// partials (chunk, 2 C + 1, padded settings): per channel sum w |y| and sum w y^2 over the chunk, then the chunk's W
template <class M>
__global__ __launch_bounds__(kWave) void signal_noise_moment_kernel(obe_model m, const double* __restrict__ settings,
                                                                    int64_t ld_s, int64_t n_s,
                                                                    const double* __restrict__ particles, int64_t ld_p,
                                                                    int64_t n, const double* __restrict__ w,
                                                                    int64_t chunk_len, double* __restrict__ partials) {
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_s ? s : n_s - 1;                    // (the padding lanes repeat the last setting)
    double x[M::NS], s1[M::NC], s2[M::NC], sw = 0.0;
#pragma unroll
    for (int k = 0; k < M::NS; ++k) x[k] = settings[(int64_t)k * ld_s + sc];
#pragma unroll
    for (int c = 0; c < M::NC; ++c) s1[c] = s2[c] = 0.0;
    const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    for (int64_t p = p0; p < p1; ++p) {                          // (p, w[p] and the particle are the same for all lanes)
        const double wp = clean_weight(w[p]);
        if (wp == 0.0) continue;                                 // (whatever y is)
        double y[M::NC];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
        sw += wp;
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            s1[c] = fma(wp, fabs(y[c]), s1[c]);
            s2[c] = fma(wp * y[c], y[c], s2[c]);
        }
    }
    const int64_t n_pad = (int64_t)gridDim.x * kWave;
    double* out = partials + (int64_t)blockIdx.y * nu_slots(M::NC) * n_pad + s;
#pragma unroll
    for (int c = 0; c < M::NC; ++c) {
        out[(2 * c) * n_pad] = s1[c];
        out[(2 * c + 1) * n_pad] = s2[c];
    }
    out[(2 * M::NC) * n_pad] = sw;
}

// out (C, n_settings) = a + b S1 / W + c S2 / W, the chunk partials added in chunk order; W == 0 gives NaN
__global__ __launch_bounds__(kBlock) void signal_noise_fold_kernel(const double* __restrict__ partials, int chunks,
                                                                   int n_channels, int64_t n_pad, int64_t n_s, NoiseCoef k,
                                                                   double* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_s) return;
    const int slots = nu_slots(n_channels);
    double sw = 0.0;
    for (int j = 0; j < chunks; ++j) sw += partials[((int64_t)j * slots + 2 * n_channels) * n_pad + s];
    for (int c = 0; c < n_channels; ++c) {
        double s1 = 0.0, s2 = 0.0;
        for (int j = 0; j < chunks; ++j) {
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
    LikArg a{};
    a.n_ch = n_lik_channels;
    a.use_choke = choke == choke;                                // NaN: no choke
    a.choke = choke;
    for (int i = 0; i < mm.n_setdims && i < OBE_MAX_SETDIMS; ++i) a.x[i] = (h_setting && !d_y) ? h_setting[i] : 0.0;
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
    (void)n_particles;                                           // (the chunks are bounded whatever the cloud: nu_words)
    if (n_settings < 1) n_settings = 1;
    if (n_channels < 1) n_channels = 1;
    return nu_words(n_settings, n_channels) * (int64_t)sizeof(double);
}

int obe_signal_noise_variance(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                              const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                              const double* h_noise_coef, double* d_noise_var, void* d_ws, int64_t ws_bytes,
                              void* stream) {
    if (!m || !d_settings || !d_particles || !d_weights || !d_noise_var || !d_ws)
        return bad_arg("obe_signal_noise_variance: null pointer");
    if (n_settings < 1 || ld_s < n_settings)
        return bad_arg("obe_signal_noise_variance: n_settings < 1 or a row of settings shorter than that");
    if (n_particles < 1 || ld_p < n_particles) return bad_arg("obe_signal_noise_variance: bad cloud size");
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    NoiseCoef k;
    if (int rc = fill_noise_coef("obe_signal_noise_variance", k, h_noise_coef, mm.n_channels)) return rc;
    if (ws_bytes < obe_signal_noise_workspace_bytes(n_particles, n_settings, mm.n_channels))
        return bad_arg("obe_signal_noise_variance: workspace too small");
    const int64_t tiles = nu_tiles(n_settings);
    if (tiles > 0x7fffffff) return bad_arg("obe_signal_noise_variance: too many settings for one call");
    const int chunks = nu_chunks(n_particles, n_settings);
    // whole waves of particles per chunk (the count of chunks that are not empty may then be smaller)
    const int64_t chunk_len = ((n_particles + chunks - 1) / chunks + kWave - 1) / kWave * kWave;
    const int used = (int)((n_particles + chunk_len - 1) / chunk_len);
    double* partials = static_cast<double*>(d_ws);
    hipStream_t st = as_stream(stream);
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        const dim3 grid((unsigned)tiles, (unsigned)used);
        signal_noise_moment_kernel<Model><<<grid, kWave, 0, st>>>(mm, d_settings, ld_s, n_settings, d_particles, ld_p,
                                                                  n_particles, d_weights, chunk_len, partials);
        OBE_CHECK_LAUNCH("signal_noise_moment_kernel");
        signal_noise_fold_kernel<<<(int)((n_settings + kBlock - 1) / kBlock), kBlock, 0, st>>>(
            partials, used, Model::NC, tiles * kWave, n_settings, k, d_noise_var);
        OBE_CHECK_LAUNCH("signal_noise_fold_kernel");
        return 0;
    });
}

}  // extern "C"
