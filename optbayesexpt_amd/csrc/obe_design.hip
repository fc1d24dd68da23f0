// Design of a batch of measurements, the model-independent half: greedy conditioning of the output variance of every
// setting on the readings already planned, from the blocks obe_output_cross_covariance (K14, obe_predict.hip) left.
// A reading at the pivot p is C scalar readings, conditioned on one after the other; row m = rows_done + c':
//   a(c, x)   = X_c'c(p, x) - sum_{m' < m} L_m'(c, x) L_m'(c', p)
//   g         = a(c', p) + nu_c'(p)
//   L_m(c, x) = a(c, x) / sqrt(g),   v_c(x) -= L_m(c, x)^2,   info += log(g / nu_c'(p)) / 2
//   U(x)      = [sum_c v_c(x) / nu_c(x)] / cost(x)
// Lane <-> setting.  Row m + 1 needs L_m at the pivot's column, which belongs to another workgroup: every thread forms the
// pivot column's C x C values itself, from the inputs and the rows of earlier calls, by the same statements as its own
// column (the thread of the pivot's setting finds the same bits twice).  Nothing a launch wrote is read by that launch.
// The arg-max is a launch of its own, one workgroup, a fixed order.
//
// The design for parameters of interest (obe_design_interest_step) conditions, by the same rows L_m, the whole C x C
// block S(x) and the covariance K_dc(x) of the rows of interest with the output, and scores what is left as
// obe_variance_reduction does (obe_interest.hip's kernel, through obe_design.h):
//   b(d)      = K_dc'(p) - sum_{m' < m} T_m'(d) L_m'(c', p),   T_m(d) = b(d) / sqrt(g),   Vleft_d -= T_m(d)^2
//   S_cc''(x) -= L_m(c, x) L_m(c'', x),                        K_dc(x) -= T_m(d) L_m(c, x)
// T needs K at the pivot's column, which the grid-wide launch rewrites: a launch of one workgroup forms the T rows of the
// pick first (a thread per row of interest, from the K the earlier launches left) and the grid-wide launch reads them.
#include "obe_design.h"

namespace obe {
namespace {

constexpr double kNaN = __builtin_nan("");
constexpr double kHuge = __builtin_huge_val();

struct DesignNoise {
    const double* nu;            // (C,) with ld == 0, else (C, n_settings) with row stride ld
    int64_t ld;
    __device__ __forceinline__ double at(int c, int64_t s) const { return ld ? nu[(int64_t)c * ld + s] : nu[c]; }
};

// The rows of this pick at the column `col`: l[c'][c] = L_{m0 + c'}(c, col).  lp: the same at the pivot's column (PIVOT:
// l itself, and rs[c'] = sqrt(g) and g[c'] are formed here; a g that is not > 0 or not finite gives NaN).
template <int C, bool PIVOT>
__device__ __forceinline__ void design_column(const double* __restrict__ cross, const double* __restrict__ factors, int m0,
                                              int64_t n_s, int64_t col, int64_t p, const DesignNoise& noise,
                                              double (&lp)[C][C], double (&g)[C], double (&rs)[C], double (&l)[C][C]) {
#pragma unroll
    for (int cp = 0; cp < C; ++cp) {
        double a[C];
#pragma unroll
        for (int c = 0; c < C; ++c) a[c] = cross[((int64_t)cp * C + c) * n_s + col];
        for (int mm = 0; mm < m0; ++mm) {
            const double at_pivot = factors[((int64_t)mm * C + cp) * n_s + p];
#pragma unroll
            for (int c = 0; c < C; ++c) a[c] -= factors[((int64_t)mm * C + c) * n_s + col] * at_pivot;
        }
#pragma unroll
        for (int k = 0; k < C; ++k) {
            if (k < cp) {
#pragma unroll
                for (int c = 0; c < C; ++c) a[c] -= l[k][c] * (PIVOT ? l[k][cp] : lp[k][cp]);
            }
        }
        if (PIVOT) {
            const double gg = a[cp] + noise.at(cp, p);
            g[cp] = gg > 0.0 && gg < kHuge ? gg : kNaN;
            rs[cp] = sqrt(g[cp]);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) l[cp][c] = a[c] / rs[cp];
    }
}

// cross NULL: nothing is conditioned on, U is formed from cvar as it is.
template <int C>
__global__ __launch_bounds__(kBlock) void design_step_kernel(const double* __restrict__ cross, int64_t p,
                                                             double* __restrict__ factors, int m0,
                                                             double* __restrict__ cvar, int64_t n_s, DesignNoise noise,
                                                             const double* __restrict__ d_cost, double cost,
                                                             double* __restrict__ utility, double* __restrict__ info) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_s) return;
    double v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = cvar[(int64_t)c * n_s + s];
    if (cross) {
        double lp[C][C], l[C][C], g[C], rs[C];
        design_column<C, true>(cross, factors, m0, n_s, p, p, noise, lp, g, rs, lp);
        design_column<C, false>(cross, factors, m0, n_s, s, p, noise, lp, g, rs, l);
#pragma unroll
        for (int cp = 0; cp < C; ++cp) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                v[c] -= l[cp][c] * l[cp][c];
                factors[((int64_t)(m0 + cp) * C + c) * n_s + s] = l[cp][c];
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) cvar[(int64_t)c * n_s + s] = v[c];
        if (s == 0) {
            double add = 0.0;
#pragma unroll
            for (int cp = 0; cp < C; ++cp) add += 0.5 * log(g[cp] / noise.at(cp, p));
            *info += add;
        }
    }
    double u = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) u += v[c] / noise.at(c, s);
    utility[s] = u / (d_cost ? d_cost[s] : cost);
}

// best[0] = the largest finite utility of a setting that is not taken, best[1] (an int64) = the first index that has it;
// NaN and -1 if there is none.  One workgroup; thread t scans t, t + 256, ... upwards, the threads are folded in order.
__global__ __launch_bounds__(kBlock) void design_best_kernel(const double* __restrict__ utility, int64_t n_s,
                                                             const unsigned char* __restrict__ taken,
                                                             double* __restrict__ best) {
    __shared__ double val[kBlock];
    __shared__ int64_t idx[kBlock];
    double bv = 0.0;
    int64_t bi = -1;
    for (int64_t s = threadIdx.x; s < n_s; s += kBlock) {
        const double u = utility[s];
        if (!(fabs(u) < kHuge) || (taken && taken[s])) continue;      // (NaN fails the comparison)
        if (bi < 0 || u > bv) {
            bv = u;
            bi = s;
        }
    }
    val[threadIdx.x] = bv;
    idx[threadIdx.x] = bi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < kBlock; ++t) {
            if (idx[t] >= 0 && (bi < 0 || val[t] > bv || (val[t] == bv && idx[t] < bi))) {
                bv = val[t];
                bi = idx[t];
            }
        }
        best[0] = bi < 0 ? kNaN : bv;
        reinterpret_cast<int64_t*>(best)[1] = bi;
    }
}

template <int... C>
int launch_step(int n_channels, std::integer_sequence<int, C...>, int blocks, hipStream_t st, const double* cross, int64_t p,
                double* factors, int m0, double* cvar, int64_t n_s, const DesignNoise& noise, const double* d_cost, double cost,
                double* utility, double* info) {
    ((n_channels == C + 1 && (design_step_kernel<C + 1><<<blocks, kBlock, 0, st>>>(cross, p, factors, m0, cvar, n_s, noise,
                                                                                 d_cost, cost, utility, info),
                              true)) || ...);
    OBE_CHECK_LAUNCH("design_step_kernel");
    return 0;
}

// The T rows of this pick, tstore[m0 + c'][d], and what they remove of Vleft_d.  One workgroup, thread <-> row of
// interest; xcov holds K conditioned on the rows before m0, so that only the rows of this pick are subtracted here.
template <int C>
__global__ __launch_bounds__(kBlock) void interest_pivot_kernel(const double* __restrict__ cross, int64_t p,
                                                                const double* __restrict__ factors, int m0,
                                                                const double* __restrict__ xcov, int n_sel, int64_t n_s,
                                                                DesignNoise noise, double* __restrict__ tstore,
                                                                double* __restrict__ pvar_left) {
    const int d = threadIdx.x;
    if (d >= n_sel) return;
    double lp[C][C], g[C], rs[C], t[C];
    design_column<C, true>(cross, factors, m0, n_s, p, p, noise, lp, g, rs, lp);
    double left = pvar_left[d];
#pragma unroll
    for (int cp = 0; cp < C; ++cp) {
        double b = xcov[((int64_t)d * C + cp) * n_s + p];
#pragma unroll
        for (int k = 0; k < C; ++k) {
            if (k < cp) b -= t[k] * lp[k][cp];
        }
        t[cp] = b / rs[cp];
        left -= t[cp] * t[cp];
        tstore[(int64_t)(m0 + cp) * n_sel + d] = t[cp];
    }
    pvar_left[d] = left;
}

// Lane <-> setting: the rows of this pick as design_step_kernel forms them, then S (every packed entry) and K of its
// column.  tstore rows [m0, m0 + C): what interest_pivot_kernel left (wave-uniform reads).
template <int C>
__global__ __launch_bounds__(kBlock) void interest_condition_kernel(const double* __restrict__ cross, int64_t p,
                                                                    double* __restrict__ factors, int m0,
                                                                    const double* __restrict__ tstore, int n_sel,
                                                                    double* __restrict__ ycov, double* __restrict__ xcov,
                                                                    int64_t n_s, DesignNoise noise) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_s) return;
    double lp[C][C], l[C][C], g[C], rs[C];
    design_column<C, true>(cross, factors, m0, n_s, p, p, noise, lp, g, rs, lp);
    design_column<C, false>(cross, factors, m0, n_s, s, p, noise, lp, g, rs, l);
#pragma unroll
    for (int cp = 0; cp < C; ++cp) {
#pragma unroll
        for (int c = 0; c < C; ++c) factors[((int64_t)(m0 + cp) * C + c) * n_s + s] = l[cp][c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int c2 = 0; c2 <= c; ++c2) {
            const int64_t at = (int64_t)(c * (c + 1) / 2 + c2) * n_s + s;
            double v = ycov[at];
#pragma unroll
            for (int cp = 0; cp < C; ++cp) v -= l[cp][c] * l[cp][c2];
            ycov[at] = v;
        }
    }
    for (int d = 0; d < n_sel; ++d) {
        double t[C];
#pragma unroll
        for (int cp = 0; cp < C; ++cp) t[cp] = tstore[(int64_t)(m0 + cp) * n_sel + d];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int64_t at = ((int64_t)d * C + c) * n_s + s;
            double v = xcov[at];
#pragma unroll
            for (int cp = 0; cp < C; ++cp) v -= t[cp] * l[cp][c];
            xcov[at] = v;
        }
    }
}

template <int... C>
int launch_interest(int n_channels, std::integer_sequence<int, C...>, int blocks, hipStream_t st, const double* cross,
                    int64_t p, double* factors, int m0, double* tstore, int n_sel, double* ycov, double* xcov, int64_t n_s,
                    const DesignNoise& noise, double* pvar_left) {
    ((n_channels == C + 1 && (interest_pivot_kernel<C + 1><<<1, kBlock, 0, st>>>(cross, p, factors, m0, xcov, n_sel, n_s, noise,
                                                                               tstore, pvar_left),
                              interest_condition_kernel<C + 1><<<blocks, kBlock, 0, st>>>(cross, p, factors, m0, tstore, n_sel,
                                                                                        ycov, xcov, n_s, noise),
                              true)) || ...);
    OBE_CHECK_LAUNCH("interest_condition_kernel");
    return 0;
}

}  // namespace

int launch_design_best(hipStream_t st, const double* d_utility, int64_t n_settings, const uint8_t* d_taken, double* d_best) {
    design_best_kernel<<<1, kBlock, 0, st>>>(d_utility, n_settings, d_taken, d_best);
    OBE_CHECK_LAUNCH("design_best_kernel");
    return 0;
}

}  // namespace obe

using namespace obe;

extern "C" {

int obe_design_step(const double* d_cross, int64_t pivot_index, double* d_factors, int32_t rows_done, int32_t max_rows,
                    double* d_cvar, int32_t n_channels, int64_t n_settings, const double* d_noise_var, int64_t ld_noise,
                    const double* d_cost, double cost, const uint8_t* d_taken, double* d_utility, double* d_best,
                    double* d_info, void* stream) {
    if (!d_cvar || !d_noise_var || !d_utility || !d_best) return bad_arg("obe_design_step: null pointer");
    if (n_channels < 1 || n_channels > OBE_MAX_CHANNELS) return bad_arg("obe_design_step: 1..8 channels");
    if (n_settings < 1 || (ld_noise != 0 && ld_noise < n_settings))
        return bad_arg("obe_design_step: n_settings < 1 or a row of the noise variance shorter than that");
    if (d_cross) {
        if (!d_factors || !d_info) return bad_arg("obe_design_step: null pointer");
        if (pivot_index < 0 || pivot_index >= n_settings) return bad_arg("obe_design_step: pivot index outside the settings");
        if (rows_done < 0 || (int64_t)rows_done + n_channels > max_rows)
            return bad_arg("obe_design_step: the factor store has no room for this pivot's rows");
    }
    const int64_t blocks = (n_settings + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffff) return bad_arg("obe_design_step: too many settings for one call");
    hipStream_t st = as_stream(stream);
    const DesignNoise noise{d_noise_var, ld_noise};
    if (int rc = launch_step(n_channels, std::make_integer_sequence<int, OBE_MAX_CHANNELS>{}, (int)blocks, st, d_cross,
                             pivot_index, d_factors, rows_done, d_cvar, n_settings, noise, d_cost, cost, d_utility, d_info))
        return rc;
    return launch_design_best(st, d_utility, n_settings, d_taken, d_best);
}

int obe_design_interest_step(const double* d_cross, int64_t pivot_index, double* d_factors, double* d_tstore,
                             int32_t rows_done, int32_t max_rows, double* d_ycov, double* d_xcov, int32_t n_sel,
                             int32_t n_channels, int64_t n_settings, const double* d_noise_var, int64_t ld_noise,
                             const double* d_pvar, double* d_pvar_left, const double* h_weights, const double* d_cost,
                             double cost, const uint8_t* d_taken, double* d_gain, double* d_utility, double* d_best,
                             void* stream) {
    if (!d_ycov || !d_xcov || !d_noise_var || !d_pvar || !d_gain || !d_utility || !d_best)
        return bad_arg("obe_design_interest_step: null pointer");
    if (n_channels < 1 || n_channels > OBE_MAX_CHANNELS) return bad_arg("obe_design_interest_step: 1..8 channels");
    if (n_sel < 1 || n_sel > OBE_MAX_DIMS) return bad_arg("obe_design_interest_step: 1..OBE_MAX_DIMS rows of interest");
    if (n_settings < 1 || (ld_noise != 0 && ld_noise < n_settings))
        return bad_arg("obe_design_interest_step: n_settings < 1 or a row of the noise variance shorter than that");
    if (d_cross) {
        if (!d_factors || !d_tstore || !d_pvar_left) return bad_arg("obe_design_interest_step: null pointer");
        if (pivot_index < 0 || pivot_index >= n_settings)
            return bad_arg("obe_design_interest_step: pivot index outside the settings");
        if (rows_done < 0 || (int64_t)rows_done + n_channels > max_rows)
            return bad_arg("obe_design_interest_step: the factor and T stores have no room for this pivot's rows");
    }
    const int64_t blocks = (n_settings + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffff) return bad_arg("obe_design_interest_step: too many settings for one call");
    hipStream_t st = as_stream(stream);
    if (d_cross) {
        const DesignNoise noise{d_noise_var, ld_noise};
        if (int rc = launch_interest(n_channels, std::make_integer_sequence<int, OBE_MAX_CHANNELS>{}, (int)blocks, st, d_cross,
                                     pivot_index, d_factors, rows_done, d_tstore, n_sel, d_ycov, d_xcov, n_settings, noise,
                                     d_pvar_left))
            return rc;
    }
    // the score in obe_variance_reduction's tiles of rows, U accumulated over them as its callers accumulate it
    for (int r0 = 0; r0 < n_sel; r0 += kGainRows) {
        const int nr = n_sel - r0 < kGainRows ? n_sel - r0 : kGainRows;
        if (int rc = launch_variance_reduction(st, d_ycov, d_xcov + (int64_t)r0 * n_channels * n_settings, nr, n_channels,
                                               n_settings, d_noise_var, ld_noise, d_pvar + r0,
                                               h_weights ? h_weights + r0 : nullptr, d_cost, cost,
                                               d_gain + (int64_t)r0 * n_settings, d_utility, r0 != 0))
            return rc;
    }
    return launch_design_best(st, d_utility, n_settings, d_taken, d_best);
}

}  // extern "C"
