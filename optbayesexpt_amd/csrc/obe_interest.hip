// Design for parameters of interest, the model-independent half: from the blocks obe_output_covariance (K12,
// obe_predict.hip) left — S (C x C, packed lower triangle) and K (rows x C) per setting — the variance of each
// parameter of interest that the best linear estimator from one reading removes, G_d = k_d^T (S + diag nu)^-1 k_d, and
// the utility U = [sum_d a_d G_d / V_d] / cost.  Lane <-> setting; the C x C factor lives in registers.
#include "obe_design.h"

namespace obe {
namespace {

struct GainWeights {
    double a[kGainRows];
};

// S + diag nu = L L^T in place (packed lower triangle, row-major); false: a pivot that is not > 0 (NaN included)
template <int C>
__device__ __forceinline__ bool cholesky_packed(double (&l)[C * (C + 1) / 2]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        double piv = l[j * (j + 1) / 2 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) piv -= l[j * (j + 1) / 2 + k] * l[j * (j + 1) / 2 + k];
        ok = ok && piv > 0.0;
        const double diag = sqrt(piv);
        l[j * (j + 1) / 2 + j] = diag;
#pragma unroll
        for (int i = j + 1; i < C; ++i) {
            double v = l[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= l[i * (i + 1) / 2 + k] * l[j * (j + 1) / 2 + k];
            l[i * (i + 1) / 2 + j] = v / diag;
        }
    }
    return ok;
}

template <int C>
__global__ __launch_bounds__(kBlock) void variance_reduction_kernel(const double* __restrict__ ycov, const double* __restrict__ xcov,
                                                                    int n_rows, int64_t n_s, const double* __restrict__ noise,
                                                                    int64_t ld_noise, const double* __restrict__ pvar,
                                                                    GainWeights wts, const double* __restrict__ d_cost,
                                                                    double cost, int accumulate, double* __restrict__ gain,
                                                                    double* __restrict__ utility) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_s) return;
    double l[C * (C + 1) / 2];
#pragma unroll
    for (int k = 0; k < C * (C + 1) / 2; ++k) l[k] = ycov[(int64_t)k * n_s + s];
#pragma unroll
    for (int c = 0; c < C; ++c) l[c * (c + 1) / 2 + c] += ld_noise ? noise[(int64_t)c * ld_noise + s] : noise[c];
    const bool ok = cholesky_packed<C>(l);
    double total = 0.0;
    for (int r = 0; r < n_rows; ++r) {
        // z = L^-1 k_r, G = |z|^2 (the second solve, L^T u = z, would only serve u, which nobody reads: k . u = z . z)
        double z[C], g = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            double v = xcov[((int64_t)r * C + c) * n_s + s];
#pragma unroll
            for (int k = 0; k < c; ++k) v -= l[c * (c + 1) / 2 + k] * z[k];
            z[c] = v / l[c * (c + 1) / 2 + c];
            g += z[c] * z[c];
        }
        if (!ok) g = __builtin_nan("");
        if (gain) gain[(int64_t)r * n_s + s] = g;
        if (utility) {
            const double v = pvar[r];
            if (v != 0.0) total += wts.a[r] * g / v;
        }
    }
    if (utility) {
        const double u = total / (d_cost ? d_cost[s] : cost);
        utility[s] = accumulate ? utility[s] + u : u;
    }
}

template <int... C>
int launch_gain(int n_channels, std::integer_sequence<int, C...>, int blocks, hipStream_t st, const double* ycov,
                const double* xcov, int n_rows, int64_t n_s, const double* noise, int64_t ld_noise, const double* pvar,
                const GainWeights& wts, const double* d_cost, double cost, int accumulate, double* gain, double* utility) {
    ((n_channels == C + 1 && (variance_reduction_kernel<C + 1><<<blocks, kBlock, 0, st>>>(
                                  ycov, xcov, n_rows, n_s, noise, ld_noise, pvar, wts, d_cost, cost, accumulate, gain, utility),
                              true)) || ...);
    OBE_CHECK_LAUNCH("variance_reduction_kernel");
    return 0;
}

}  // namespace

int launch_variance_reduction(hipStream_t st, const double* d_ycov, const double* d_xcov, int n_rows, int n_channels,
                              int64_t n_settings, const double* d_noise_var, int64_t ld_noise, const double* d_pvar,
                              const double* h_weights, const double* d_cost, double cost, double* d_gain,
                              double* d_utility, int accumulate) {
    GainWeights wts;
    for (int r = 0; r < kGainRows; ++r) wts.a[r] = h_weights && r < n_rows ? h_weights[r] : 1.0;
    const int blocks = (int)((n_settings + kBlock - 1) / kBlock);
    return launch_gain(n_channels, std::make_integer_sequence<int, OBE_MAX_CHANNELS>{}, blocks, st, d_ycov, d_xcov, n_rows,
                       n_settings, d_noise_var, ld_noise, d_pvar, wts, d_cost, cost, accumulate, d_gain, d_utility);
}

}  // namespace obe

using namespace obe;

extern "C" {

int obe_variance_reduction(const double* d_ycov, const double* d_xcov, int32_t n_rows, int32_t n_channels, int64_t n_settings,
                           const double* d_noise_var, int64_t ld_noise, const double* d_pvar, const double* h_weights,
                           const double* d_cost, double cost, double* d_gain, double* d_utility, int32_t accumulate,
                           void* stream) {
    if (!d_ycov || !d_xcov || !d_noise_var || (d_utility && !d_pvar)) return bad_arg("obe_variance_reduction: null pointer");
    if (n_rows < 1 || n_rows > kGainRows) return bad_arg("obe_variance_reduction: 1..8 rows per call");
    if (n_channels < 1 || n_channels > OBE_MAX_CHANNELS) return bad_arg("obe_variance_reduction: 1..8 channels");
    if (n_settings < 1 || (ld_noise != 0 && ld_noise < n_settings))
        return bad_arg("obe_variance_reduction: n_settings < 1 or a row of the noise variance shorter than that");
    if (!d_gain && !d_utility) return 0;
    const int64_t blocks = (n_settings + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffff) return bad_arg("obe_variance_reduction: too many settings for one call");
    return launch_variance_reduction(as_stream(stream), d_ycov, d_xcov, n_rows, n_channels, n_settings, d_noise_var, ld_noise,
                                     d_pvar, h_weights, d_cost, cost, d_gain, d_utility, accumulate);
}

}  // extern "C"
