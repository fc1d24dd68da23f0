// K13b — the tempered update of a recorded data set, the model-independent half: from the per-particle joint
// log-likelihood l that obe_records_loglik (K13a, obe_predict.hip) left, the sums a stage's exponent is chosen from
// (obe_tempered_sums) and the factor exp(a (l - shift)) that obe_bayes_update_lik then multiplies the weights by
// (obe_tempered_likelihood).  Nothing here writes the weights.
#include <algorithm>

#include "obe_common.h"

namespace obe {
namespace {

constexpr int kTrials = OBE_TEMPERED_MAX_TRIALS;
constexpr int kTemperBlocks = 256;                 // workgroups of a pass at most: partials one fold workgroup adds
constexpr int kTemperWords = 2 + 2 * kTrials;      // m, sum w, then (S1, S2) per trial
constexpr double kInf = __builtin_huge_val();

static_assert((int64_t)(2 * kTemperWords + kTemperBlocks * kTemperWords) * 8 <= OBE_TEMPERED_WS_BYTES,
              "OBE_TEMPERED_WS_BYTES does not hold the block partials");

struct TrialExponents {
    double a[kTrials];
};

// Maximum of v over the block; valid in thread 0.  `red` = kBlock / kWave doubles of LDS.  (max is exact: any order)
__device__ __forceinline__ double block_max(double v, double* red) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, kWave));
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double s = -kInf;
    if (threadIdx.x == 0) {
        for (int i = 0; i < (int)(blockDim.x / kWave); ++i) s = fmax(s, red[i]);
    }
    return s;
}

// pass 1: per workgroup the largest finite l among the particles of weight > 0, and their sum w
__global__ __launch_bounds__(kBlock) void tempered_top_kernel(const double* __restrict__ loglik, const double* __restrict__ weights,
                                                              int64_t n, double* __restrict__ p_top,
                                                              double* __restrict__ p_sw) {
    __shared__ double red[kBlock / kWave];
    double top = -kInf, sw = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
        const double w = clean_weight(weights[p]), l = loglik[p];
        if (w == 0.0) continue;
        sw += w;
        if (fabs(l) < kInf) top = fmax(top, l);                  // (NaN fails the comparison)
    }
    const double t = block_max(top, red);
    __syncthreads();
    const double s = block_sum(sw, red);
    if (threadIdx.x == 0) {
        p_top[blockIdx.x] = t;
        p_sw[blockIdx.x] = s;
    }
}

// ... folded: head[0] = m, head[1] = sum w (the partial sums added in block order by block_sum_array)
__global__ __launch_bounds__(kBlock) void tempered_top_fold_kernel(const double* __restrict__ p_top, const double* __restrict__ p_sw,
                                                                   int nb, double* __restrict__ head) {
    __shared__ double red[kBlock / kWave];
    double top = -kInf;
    for (int i = threadIdx.x; i < nb; i += kBlock) top = fmax(top, p_top[i]);
    const double t = block_max(top, red);
    __syncthreads();
    const double s = block_sum_array(p_sw, nb, red);
    if (threadIdx.x == 0) {
        head[0] = t;
        head[1] = s;
    }
}

// pass 2: per workgroup and trial, S1 = sum w exp(a (l - m)) and S2 = sum (w exp(a (l - m)))^2; partials (2 n_trials, nb)
__global__ __launch_bounds__(kBlock) void tempered_sums_kernel(const double* __restrict__ loglik, const double* __restrict__ weights,
                                                               int64_t n, TrialExponents ex, int n_trials,
                                                               const double* __restrict__ head, double* __restrict__ partials) {
    __shared__ double red[kBlock / kWave];
    const double top = head[0];
    double s1[kTrials], s2[kTrials];
#pragma unroll
    for (int t = 0; t < kTrials; ++t) s1[t] = s2[t] = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
        const double w = clean_weight(weights[p]), l = loglik[p];
        if (w == 0.0 || !(fabs(l) < kInf)) continue;
        const double d = l - top;                                // <= 0
#pragma unroll
        for (int t = 0; t < kTrials; ++t) {
            if (t < n_trials) {
                const double v = w * exp(ex.a[t] * d);
                s1[t] += v;
                s2[t] += v * v;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < kTrials; ++t) {
        if (t < n_trials) {                                      // (n_trials is the same for all threads)
            const double a = block_sum(s1[t], red);
            __syncthreads();
            const double b = block_sum(s2[t], red);
            __syncthreads();
            if (threadIdx.x == 0) {
                partials[(int64_t)(2 * t) * gridDim.x + blockIdx.x] = a;
                partials[(int64_t)(2 * t + 1) * gridDim.x + blockIdx.x] = b;
            }
        }
    }
}

// ... folded and delivered: out (2 + 2 n_trials words, the device copy) and host_out (the device view of the caller's
// page-locked h_sums, or NULL).  Every word of the host block is watched on its own: no ordering between the stores.
__global__ __launch_bounds__(kBlock) void tempered_fold_kernel(const double* __restrict__ partials, int nb, int n_trials,
                                                               const double* __restrict__ head, double* __restrict__ out,
                                                               double* __restrict__ host_out) {
    __shared__ double red[kBlock / kWave];
    for (int k = 0; k < 2 * n_trials; ++k) {
        const double s = block_sum_array(partials + (int64_t)k * nb, nb, red);
        __syncthreads();
        if (threadIdx.x == 0) {
            out[2 + k] = s;
            if (host_out) host_out[2 + k] = s;
        }
    }
    if (threadIdx.x == 0) {
        out[0] = head[0];
        out[1] = head[1];
        if (host_out) {
            host_out[0] = head[0];
            host_out[1] = head[1];
        }
    }
}

__global__ __launch_bounds__(kBlock) void tempered_likelihood_kernel(const double* __restrict__ loglik, int64_t n, double exponent,
                                                                     double shift, double* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
        const double l = loglik[p];
        out[p] = fabs(l) < kInf ? exp(exponent * (l - shift)) : 0.0;
    }
}

}  // namespace
}  // namespace obe

using namespace obe;

extern "C" {

int obe_tempered_sums(const double* d_loglik, const double* d_weights, int64_t n_particles, const double* h_exponents,
                      int32_t n_trials, void* d_ws, int64_t ws_bytes, double* h_sums, void* stream) {
    if (!d_loglik || !d_weights || !h_exponents || !d_ws || !h_sums || n_particles <= 0)
        return bad_arg("obe_tempered_sums: bad pointer/size");
    if (n_trials < 1 || n_trials > kTrials) return bad_arg("obe_tempered_sums: 1..16 trial exponents per call");
    if (ws_bytes < OBE_TEMPERED_WS_BYTES) return bad_arg("obe_tempered_sums: workspace too small");
    TrialExponents ex{};
    for (int t = 0; t < n_trials; ++t) {
        if (!(h_exponents[t] >= 0.0 && h_exponents[t] < kInf)) return bad_arg("obe_tempered_sums: exponent not finite and >= 0");
        ex.a[t] = h_exponents[t];
    }
    hipStream_t st = as_stream(stream);
    const int nb = std::min(stream_blocks(n_particles, kBlock * 4), kTemperBlocks);
    double* head = static_cast<double*>(d_ws);                   // m, sum w
    double* out = head + kTemperWords;                           // the device copy of the results
    double* partials = out + kTemperWords;
    const int words = 2 + 2 * n_trials;
    HostWords sums(h_sums, words);
    sums.arm();
    tempered_top_kernel<<<nb, kBlock, 0, st>>>(d_loglik, d_weights, n_particles, partials, partials + nb);
    OBE_CHECK_LAUNCH("tempered_top_kernel");
    tempered_top_fold_kernel<<<1, kBlock, 0, st>>>(partials, partials + nb, nb, head);
    OBE_CHECK_LAUNCH("tempered_top_fold_kernel");
    tempered_sums_kernel<<<nb, kBlock, 0, st>>>(d_loglik, d_weights, n_particles, ex, n_trials, head, partials);
    OBE_CHECK_LAUNCH("tempered_sums_kernel");
    tempered_fold_kernel<<<1, kBlock, 0, st>>>(partials, nb, n_trials, head, out, sums.view<double>());
    OBE_CHECK_LAUNCH("tempered_fold_kernel");
    if (int rc = sums.copy(0, words, out, st)) return rc;
    return sums.wait(st);
}

int obe_tempered_likelihood(const double* d_loglik, int64_t n_particles, double exponent, double shift, double* d_lik_out,
                            void* stream) {
    if (!d_loglik || !d_lik_out || n_particles <= 0) return bad_arg("obe_tempered_likelihood: bad pointer/size");
    if (exponent != exponent || shift != shift) return bad_arg("obe_tempered_likelihood: NaN exponent or shift");
    tempered_likelihood_kernel<<<stream_blocks(n_particles, kBlock), kBlock, 0, as_stream(stream)>>>(
        d_loglik, n_particles, exponent, shift, d_lik_out);
    OBE_CHECK_LAUNCH("tempered_likelihood_kernel");
    return 0;
}

}  // extern "C"
