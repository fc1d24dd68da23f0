// K10 — posterior predictive summaries on the device: for every setting x_s and channel c the weighted mean, variance
// and quantiles of y_i = model(x_s; theta_i)[c] over the whole cloud.  The settings x particles evaluations never leave
// the chip: only the (C, n_settings) results are written.
//
// The model is evaluated with M::eval, the exact NumPy-order form, so every y is the bits obe_eval_over_particles
// writes.  NaN and negative weights count as zero, and a particle of zero weight contributes nothing whatever its y is
// (NaN and inf included).
//   moments    lane <-> setting, the particle axis streamed (the same particle for all lanes: scalar loads), grid =
//              setting tiles x particle chunks.  Two passes: sum w y, then sum w (y - mean)^2 about that mean; the
//              chunk partials are folded in chunk order.  No atomics: the same bits from run to run.
//   quantiles  the model values of a tile of (setting, channel) rows are written to the workspace once (lane <->
//              particle), then obe_posterior.hip's radix select runs on that tile as on a cloud of rows: eight
//              passes of select_pass_kernel / select_choose_kernel.  Integer sums: the same bits under any grid and
//              any permutation of the cloud.  (A fused select that recomputed the key in every pass instead of
//              loading it was built and measured: slower at both benchmark clouds)
// K11 — scoring a measurement against the posterior predictive (further down): the log-density of readings and their
// per-channel tail probabilities, noise included.  The geometry of the moments with lane <-> record.
// K15 — quantiles of the next READING (below K11): the inverse of K11's tails.  A bracket pass over the cloud, then a fixed
// budget of (iteration pass, step kernel) pairs: safeguarded Newton on the log of the tail, K11's geometry throughout.
// K12 — design for parameters of interest (below K15): per setting the covariance of the model output with itself (S)
// and with up to eight selected parameter rows (K), for obe_variance_reduction (obe_interest.hip).  The moments' two
// passes and geometry; the second pass carries C (C + 1) / 2 + R C centred products per evaluation instead of C squares.
// K14 — design of a batch of measurements (below K13a): the covariance of the model output at every setting with the
// output at up to eight "pivot" rows (a pivot point's channels), for obe_design_step (obe_design.hip).  K12's second pass
// with a table row u_r,i = w_i (y_r(pivot; theta_i) - m_r) in theta's place and without the S products.
#include <algorithm>

#include "obe_models.h"
#include "obe_records_pass.h"
#include "obe_score_pass.h"
#include "obe_select.h"

namespace obe {
namespace {

// (the header, the moment chunks and the carved workspace: obe_score_pass.h)
constexpr int kTileRows = 64;                      // (setting, channel) rows whose values are kept at a time: 64 x N_p doubles

inline int64_t tile_rows_bound(int64_t n_settings, int n_channels) { return std::min<int64_t>(n_settings * n_channels, kTileRows); }
// the tile's values, its digit histograms, prefixes, targets and results, its row list
inline int64_t select_words(int64_t n_particles, int64_t n_settings, int n_channels, int n_q) {
    const int64_t rows = tile_rows_bound(n_settings, n_channels);
    return rows * n_particles + rows * n_q * (int64_t)(kDigits + 3) + (rows + 1) / 2;
}

// ---- moments.  One wave per workgroup; lane = one setting, the chunk's particles one after the other.
// CENTRED: sum w (y - centre)^2 about centre (C, n_settings); else sum w y.
template <class M, bool CENTRED>
__global__ __launch_bounds__(kWave) void predict_moment_kernel(obe_model m, const double* __restrict__ settings,
                                                               int64_t ld_s, int64_t n_s,
                                                               const double* __restrict__ particles, int64_t ld_p,
                                                               int64_t n, const double* __restrict__ w,
                                                               int64_t chunk_len, const double* __restrict__ centre,
                                                               double* __restrict__ partials) {
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_s ? s : n_s - 1;                    // (the padding lanes repeat the last setting)
    double x[M::NS], c0[M::NC], acc[M::NC];
#pragma unroll
    for (int k = 0; k < M::NS; ++k) x[k] = settings[(int64_t)k * ld_s + sc];
#pragma unroll
    for (int c = 0; c < M::NC; ++c) {
        c0[c] = CENTRED ? centre[(int64_t)c * n_s + sc] : 0.0;
        acc[c] = 0.0;
    }
    const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    for (int64_t p = p0; p < p1; ++p) {                          // (p, w[p] and the particle are the same for all lanes)
        const double wp = clean_weight(w[p]);
        if (wp == 0.0) continue;
        double y[M::NC];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            if (CENTRED) {
                const double d = y[c] - c0[c];
                acc[c] += wp * (d * d);
            } else {
                acc[c] += wp * y[c];
            }
        }
    }
    const int64_t n_pad = (int64_t)gridDim.x * kWave;
#pragma unroll
    for (int c = 0; c < M::NC; ++c) partials[((int64_t)blockIdx.y * M::NC + c) * n_pad + s] = acc[c];
}

// out (C, n_settings) = (the chunk partials, added in chunk order) / sum w
__global__ __launch_bounds__(kBlock) void predict_fold_kernel(const double* __restrict__ partials, int chunks, int n_channels,
                                                              int64_t n_pad, int64_t n_s, const u64* __restrict__ hdr,
                                                              double* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_s) return;
    const double sw = __longlong_as_double((long long)hdr[0]);
    for (int c = 0; c < n_channels; ++c) {
        double acc = 0.0;
        for (int j = 0; j < chunks; ++j) acc += partials[((int64_t)j * n_channels + c) * n_pad + s];
        out[(int64_t)c * n_s + s] = acc / sw;
    }
}

// ---- quantiles.  Row r = setting * NC + channel.  values (rows of the tile, n): the model at the tile's settings, grid
// (particle blocks, settings of the tile).
template <class M>
__global__ __launch_bounds__(kBlock) void predict_rows_kernel(obe_model m, const double* __restrict__ settings, int64_t ld_s,
                                                              int64_t s0, const double* __restrict__ particles,
                                                              int64_t ld_p, int64_t n, double* __restrict__ values) {
    double x[M::NS];
#pragma unroll
    for (int d = 0; d < M::NS; ++d) x[d] = settings[(int64_t)d * ld_s + s0 + blockIdx.y];
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
        double y[M::NC];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
#pragma unroll
        for (int c = 0; c < M::NC; ++c) values[((int64_t)blockIdx.y * M::NC + c) * n + p] = y[c];
    }
}

__global__ void predict_row_list_kernel(int32_t* __restrict__ rows, int n) {
    if ((int)threadIdx.x < n) rows[threadIdx.x] = threadIdx.x;
}

// out (n_q, C, n_settings): the tile's results, which select_choose_kernel left row by row (rows of the tile, n_q)
__global__ __launch_bounds__(kBlock) void predict_deliver_kernel(const double* __restrict__ found, int64_t s0, int tile_settings,
                                                                 int64_t n_s, int n_channels, int n_q,
                                                                 double* __restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= tile_settings * n_channels * n_q) return;
    const int s = i % tile_settings, jc = i / tile_settings;
    const int c = jc % n_channels, j = jc / n_channels;
    out[((int64_t)j * n_channels + c) * n_s + s0 + s] = found[(s * n_channels + c) * n_q + j];
}

// ---- K11: scoring.  Lane = one record (a setting point, the reading y_meas[c], a known sigma[c]); the chunk's particles
// one after the other, particle, weight and noise rows the same for all lanes.  z_c = (y_c - y_meas_c) / sigma_c with y
// the model value.  A particle enters only with a weight > 0 and, ROWS, every noise row > 0 (NaN fails both).  The folds
// (score_logpdf_fold_kernel, score_tails_fold_kernel) and lse_add: obe_score_pass.h.
struct ScoreRows {
    int row[OBE_MAX_CHANNELS];
};

// the record's reading and, known sigma, 1 / sigma and -sum log sigma; false: a sigma of the record is not > 0
template <class M, bool ROWS>
__device__ __forceinline__ bool load_record(int64_t sc, const double* __restrict__ y_meas, int64_t ld_y,
                                            const double* __restrict__ sigma, int64_t ld_sg, double* ym, double* inv,
                                            double& neg_log) {
    bool ok = true;
    neg_log = 0.0;
#pragma unroll
    for (int c = 0; c < M::NC; ++c) {
        ym[c] = y_meas[(int64_t)c * ld_y + sc];
        if (!ROWS) {
            const double sg = sigma[(int64_t)c * ld_sg + sc];
            ok = ok && sg > 0.0;
            inv[c] = 1.0 / sg;
            neg_log -= log(sg);
        }
    }
    return ok;
}

// the particle's sigma rows (the same for all lanes); false: one of them is not > 0
template <class M>
__device__ __forceinline__ bool load_noise(const ScoreRows& rows, const double* __restrict__ particles, int64_t ld_p,
                                           int64_t p, double* inv, double& neg_log) {
    bool ok = true;
    neg_log = 0.0;
#pragma unroll
    for (int c = 0; c < M::NC; ++c) {
        const double sg = particles[(int64_t)rows.row[c] * ld_p + p];
        ok = ok && sg > 0.0;
        inv[c] = 1.0 / sg;
        neg_log -= log(sg);
    }
    return ok;
}

// partials (chunk, 2, padded records): the chunk's (m, S) of sum_i w_i exp(l_i), l_i = sum_c [-z_c^2 / 2 - log sigma_c]
template <class M, bool ROWS>
__global__ __launch_bounds__(kWave) void score_logpdf_kernel(obe_model m, const double* __restrict__ settings, int64_t ld_s,
                                                             int64_t n_r, const double* __restrict__ y_meas, int64_t ld_y,
                                                             const double* __restrict__ sigma, int64_t ld_sg,
                                                             ScoreRows rows, const double* __restrict__ particles,
                                                             int64_t ld_p, int64_t n, const double* __restrict__ w,
                                                             int64_t chunk_len, double* __restrict__ partials) {
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_r ? s : n_r - 1;                    // (the padding lanes repeat the last record)
    double x[M::NS], ym[M::NC], inv[M::NC], neg_log;
#pragma unroll
    for (int k = 0; k < M::NS; ++k) x[k] = settings[(int64_t)k * ld_s + sc];
    const bool rec_ok = load_record<M, ROWS>(sc, y_meas, ld_y, sigma, ld_sg, ym, inv, neg_log);
    double top = -kInf, S = 0.0;
    const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    for (int64_t p = p0; p < p1; ++p) {                          // (p, w[p] and the particle are the same for all lanes)
        const double wp = clean_weight(w[p]);
        if (wp == 0.0) continue;
        if (ROWS && !load_noise<M>(rows, particles, ld_p, p, inv, neg_log)) continue;
        double y[M::NC];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
        double l = neg_log;
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            const double z = (y[c] - ym[c]) * inv[c];
            l -= 0.5 * (z * z);
        }
        if (rec_ok && fabs(l) < kInf) lse_add(top, S, l, wp);      // (NaN and -inf contribute nothing)
    }
    const int64_t n_pad = (int64_t)gridDim.x * kWave;
    partials[((int64_t)blockIdx.y * 2 + 0) * n_pad + s] = top;
    partials[((int64_t)blockIdx.y * 2 + 1) * n_pad + s] = S;
}

// partials (chunk, 2 C, padded records): sum w P(Y_c <= y_meas_c | particle), then sum w P(Y_c >= y_meas_c | particle).
// The small one of the two is erfc(|z| / sqrt 2) / 2 itself, the large one 1 - that (>= 1/2: correctly rounded).
template <class M, bool ROWS>
__global__ __launch_bounds__(kWave) void score_tails_kernel(obe_model m, const double* __restrict__ settings, int64_t ld_s,
                                                            int64_t n_r, const double* __restrict__ y_meas, int64_t ld_y,
                                                            const double* __restrict__ sigma, int64_t ld_sg,
                                                            ScoreRows rows, const double* __restrict__ particles,
                                                            int64_t ld_p, int64_t n, const double* __restrict__ w,
                                                            int64_t chunk_len, double* __restrict__ partials) {
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_r ? s : n_r - 1;
    double x[M::NS], ym[M::NC], inv[M::NC], lo[M::NC], hi[M::NC], unused;
#pragma unroll
    for (int k = 0; k < M::NS; ++k) x[k] = settings[(int64_t)k * ld_s + sc];
    const bool rec_ok = load_record<M, ROWS>(sc, y_meas, ld_y, sigma, ld_sg, ym, inv, unused);
#pragma unroll
    for (int c = 0; c < M::NC; ++c) lo[c] = hi[c] = 0.0;
    const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    for (int64_t p = p0; p < p1; ++p) {
        const double wp = clean_weight(w[p]);
        if (wp == 0.0) continue;
        if (ROWS && !load_noise<M>(rows, particles, ld_p, p, inv, unused)) continue;
        double y[M::NC];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            const double z = (y[c] - ym[c]) * inv[c];            // > 0: the model lies above the reading
            if (rec_ok && z == z) {
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

// ---- K15: quantiles of the next reading, the inverse of the tails above.  For a setting, a channel c and a level q the
// y with L_c(y) = q T_c (q <= 1/2) or U_c(y) = (1 - q) T_c (q > 1/2): L, U the tails as score_tails_kernel forms them,
// T_c = sum w over the particles that contribute to the channel — weight > 0, ROWS: every noise row > 0, f_c finite (a
// stated deviation from the tails, where +-inf counts as mass at infinity: a reading cannot be infinite).  K11's
// geometry: lane = one setting, the chunk's particles one after the other, grid = setting tiles x particle chunks x level
// groups; a group is as many levels as fit kReadSlots (trial, tail, density) triples per lane with the model's channels.
//   bracket   one pass: T_c and per level the min / max over the contributing particles of f + z^-+ sigma, z^-+ the
//             level's normal quantile widened by a hair (ReadLevels): at the lower end every term of the tail is <= its
//             target, at the upper end >=, so the pair brackets the root.
//   pass      at the trial y of every open row A = L or U (the one its level solves in) and D = sum w phi(z) / sigma.
//   step      folds the chunk partials in chunk order and moves the trial by Newton's method on log A, safeguarded by the
//             bracket (midpoint when the Newton point leaves the open bracket, is not finite, or the step exceeds half
//             the previous one); keeps the number of open rows per (group, setting tile), which the next pass's
//             workgroups read before anything else.
// No atomics: the same bits from run to run.  The levels, the rows' state, the init and the step kernel and the chunk
// plan see no sigma: obe_score_pass.h.

// the sigma of the lane's setting (known sigma); false: one of them is not finite and > 0
template <class M>
__device__ __forceinline__ bool load_sigma(int64_t sc, const double* __restrict__ sigma, int64_t ld_sg, double* sg, double* inv) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < M::NC; ++c) {
        sg[c] = sigma[(int64_t)c * ld_sg + sc];
        ok = ok && sg[c] > 0.0 && sg[c] < kInf;
        inv[c] = 1.0 / sg[c];
    }
    return ok;
}

// partials (chunk, C (1 + 2 n_q), padded settings): T_c, then per (level, channel) the min of f + z_lo sigma and the max
// of f + z_hi sigma.  T_c is written by the first level group.
template <class M, bool ROWS>
__global__ __launch_bounds__(kWave) void reading_bracket_kernel(obe_model m, const double* __restrict__ settings, int64_t ld_s,
                                                                int64_t n_s, const double* __restrict__ sigma, int64_t ld_sg,
                                                                ScoreRows rows, const double* __restrict__ particles,
                                                                int64_t ld_p, int64_t n, const double* __restrict__ w,
                                                                int64_t chunk_len, ReadLevels lv,
                                                                double* __restrict__ partials) {
    constexpr int G = M::NC < kReadSlots ? kReadSlots / M::NC : 1;
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_s ? s : n_s - 1;                    // (the padding lanes repeat the last setting)
    const int j0 = blockIdx.z * G;
    double x[M::NS], sg[M::NC], inv[M::NC], T[M::NC], mn[G][M::NC], mx[G][M::NC], zl[G], zh[G];
#pragma unroll
    for (int k = 0; k < M::NS; ++k) x[k] = settings[(int64_t)k * ld_s + sc];
    bool rec_ok = true;
    if (!ROWS) rec_ok = load_sigma<M>(sc, sigma, ld_sg, sg, inv);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int j = j0 + g < lv.n ? j0 + g : lv.n - 1;         // (levels beyond the call's repeat the last: not written)
        zl[g] = lv.z_lo[j];
        zh[g] = lv.z_hi[j];
#pragma unroll
        for (int c = 0; c < M::NC; ++c) mn[g][c] = kInf, mx[g][c] = -kInf;
    }
#pragma unroll
    for (int c = 0; c < M::NC; ++c) T[c] = 0.0;
    const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    for (int64_t p = p0; p < p1; ++p) {                          // (p, w[p] and the particle are the same for all lanes)
        const double wp = clean_weight(w[p]);
        if (wp == 0.0) continue;
        if (ROWS) {
            bool ok = true;
#pragma unroll
            for (int c = 0; c < M::NC; ++c) {
                sg[c] = particles[(int64_t)rows.row[c] * ld_p + p];
                ok = ok && sg[c] > 0.0;
            }
            if (!ok) continue;
        }
        double y[M::NC];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            if (rec_ok && fabs(y[c]) < kInf) {                   // (NaN fails)
                T[c] += wp;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    mn[g][c] = fmin(mn[g][c], y[c] + zl[g] * sg[c]);
                    mx[g][c] = fmax(mx[g][c], y[c] + zh[g] * sg[c]);
                }
            }
        }
    }
    const int64_t n_pad = (int64_t)gridDim.x * kWave;
    double* out = partials + (int64_t)blockIdx.y * (M::NC * (1 + 2 * lv.n)) * n_pad + s;
#pragma unroll
    for (int c = 0; c < M::NC; ++c) {
        if (blockIdx.z == 0) out[c * n_pad] = T[c];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (j0 + g < lv.n) {
                out[(M::NC + ((j0 + g) * M::NC + c) * 2) * n_pad] = mn[g][c];
                out[(M::NC + ((j0 + g) * M::NC + c) * 2 + 1) * n_pad] = mx[g][c];
            }
        }
    }
}

// partials (chunk, n_q C, 2, padded settings): A and sqrt(2 pi) D of the open rows at their trials.  The model is
// evaluated once per (setting, particle) and shared by the group's levels.  A workgroup whose tile has no open row in
// its group returns at once: the count was written by the launch before.
template <class M, bool ROWS>
__global__ __launch_bounds__(kWave) void reading_pass_kernel(obe_model m, const double* __restrict__ settings, int64_t ld_s,
                                                             int64_t n_s, const double* __restrict__ sigma, int64_t ld_sg,
                                                             ScoreRows rows, const double* __restrict__ particles,
                                                             int64_t ld_p, int64_t n, const double* __restrict__ w,
                                                             int64_t chunk_len, ReadLevels lv, ReadState st) {
    constexpr int G = M::NC < kReadSlots ? kReadSlots / M::NC : 1;
    if (st.tile_open[(int64_t)blockIdx.z * gridDim.x + blockIdx.x] == 0) return;
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_s ? s : n_s - 1;                    // (the padding lanes repeat the last setting: never open)
    const int64_t n_pad = (int64_t)gridDim.x * kWave;
    const int j0 = blockIdx.z * G;
    double x[M::NS], sg[M::NC], inv[M::NC], yt[G][M::NC], A[G][M::NC], D[G][M::NC], unused;
    bool open[G][M::NC], up[G];
#pragma unroll
    for (int k = 0; k < M::NS; ++k) x[k] = settings[(int64_t)k * ld_s + sc];
    bool rec_ok = true;
    if (!ROWS) rec_ok = load_sigma<M>(sc, sigma, ld_sg, sg, inv);
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
        if (ROWS && !load_noise<M>(rows, particles, ld_p, p, inv, unused)) continue;
        double y[M::NC];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            const bool fin = rec_ok && fabs(y[c]) < kInf;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (open[g][c] && fin) {
                    const double z = (y[c] - yt[g][c]) * inv[c];          // > 0: the model lies above the trial
                    const double small = 0.5 * erfc(fabs(z) * kSqrtHalf), large = 1.0 - small;
                    A[g][c] += wp * ((z > 0.0) == up[g] ? large : small);
                    D[g][c] += wp * (exp(-0.5 * (z * z)) * inv[c]);
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

// What the scoring entry points and K15 share: everything that can refuse the call, then the launch geometry
// (ScorePlan, obe_score_pass.h).
struct Score : ScorePlan {
    obe_model mm;
    ScoreRows rows;
    int prepare(const char* who, const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                const double* d_y_meas, int64_t ld_y, const double* d_sigma, int64_t ld_sigma,
                const int32_t* h_noise_rows, const double* d_particles, int64_t ld_p, int64_t n_particles,
                const double* d_weights, void* d_ws, int64_t ws_bytes, int n_q = 0) {      // n_q > 0: K15, no y_meas
        static thread_local std::string msg;
        auto refuse = [&](const char* what) {
            msg = std::string(who) + ": " + what;
            return bad_arg(msg.c_str());
        };
        if (!d_y_meas && !n_q) return refuse("null pointer");
        if (int rc = check_inputs(who, m, d_settings, ld_s, n_records, d_particles, ld_p, n_particles, d_weights, d_ws))
            return rc;
        if ((d_sigma != nullptr) == (h_noise_rows != nullptr)) return refuse("exactly one of d_sigma and h_noise_rows");
        if ((!n_q && ld_y < n_records) || (d_sigma && ld_sigma < n_records))
            return refuse("a row of y_meas or sigma shorter than n_records");
        mm = *m;
        if (int rc = obe_model_validate(&mm)) return rc;
        for (int c = 0; c < OBE_MAX_CHANNELS; ++c) {
            rows.row[c] = (h_noise_rows && c < mm.n_channels) ? h_noise_rows[c] : 0;
            if (rows.row[c] && (rows.row[c] < 0 || rows.row[c] >= mm.n_params)) return refuse("noise row index out of range");
        }
        if (const char* what = plan(n_particles, n_records, mm.n_channels, n_q, d_ws, ws_bytes)) return refuse(what);
        return 0;
    }
};

// ---- K12: output-parameter covariance.  rows: the parameter rows of interest of one call, by value.
constexpr int kCovRows = 8;                        // rows one call serves (R of predict_cov_kernel: 1, 4 or 8)
constexpr int kCovStats = 2 * kCovRows;            // words: t_d (the rows' means), then V_d
constexpr int kCovRowWords = kCovStats + 2 * kCovRows * kPostPartials;      // ... and the block partials of both

struct CovRows {
    int n;
    int row[kCovRows];
};
constexpr int cov_pairs(int n_channels) { return n_channels * (n_channels + 1) / 2; }
// the chunk partials of either pass: C means, then C (C + 1) / 2 + n_rows C products
inline int64_t cov_words(int64_t n_particles, int64_t n_settings, int n_channels, int n_rows) {
    const int slots = std::max(n_channels, cov_pairs(n_channels) + n_rows * n_channels);
    return (int64_t)moment_chunks(n_particles, n_settings) * setting_tiles(n_settings) * kWave * slots;
}

// The cloud pass over the selected rows, grid (blocks, rows): partials (row, block) of sum w theta or, CENTRED, of
// sum w (theta - t)^2 about t = (the first pass's partials, added as cov_rows_fold_kernel adds them) / sum w.
template <bool CENTRED>
__global__ __launch_bounds__(kBlock) void cov_rows_partial_kernel(const double* __restrict__ particles, int64_t ld_p,
                                                                  int64_t n, const double* __restrict__ w, CovRows rows,
                                                                  const double* __restrict__ first, const u64* __restrict__ hdr,
                                                                  double* __restrict__ partials) {
    __shared__ double red[kBlock / kWave];
    const double* th = particles + (int64_t)rows.row[blockIdx.y] * ld_p;
    double t = 0.0;
    if (CENTRED) t = block_sum_array(first + (int64_t)blockIdx.y * gridDim.x, gridDim.x, red) / __longlong_as_double((long long)hdr[0]);
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const double wp = clean_weight(w[i]);
        if (wp == 0.0) continue;                                 // (whatever theta is)
        const double d = th[i] - t;
        s += CENTRED ? wp * (d * d) : wp * th[i];
    }
    __syncthreads();
    s = block_sum(s, red);
    if (threadIdx.x == 0) partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// stats[r] = t_r, stats[kCovRows + r] = pvar[r] = V_r; one workgroup per row
__global__ __launch_bounds__(kBlock) void cov_rows_fold_kernel(const double* __restrict__ first, const double* __restrict__ second,
                                                               int nb, const u64* __restrict__ hdr, double* __restrict__ stats,
                                                               double* __restrict__ pvar) {
    __shared__ double red[kBlock / kWave];
    const double sw = __longlong_as_double((long long)hdr[0]);
    const double t = block_sum_array(first + (int64_t)blockIdx.x * nb, nb, red) / sw;
    __syncthreads();
    const double v = block_sum_array(second + (int64_t)blockIdx.x * nb, nb, red) / sw;
    if (threadIdx.x == 0) {
        stats[blockIdx.x] = t;
        stats[kCovRows + blockIdx.x] = v;
        pvar[blockIdx.x] = v;
    }
}

// The second pass of the moments with every centred product: per evaluation C (C + 1) / 2 FMAs for S and R C for K.
// u_r = w (theta_r - t_r) is the same for all lanes and formed once per particle.  Rows beyond rows.n repeat row 0 and
// are not written.  partials (chunk, C (C + 1) / 2 + rows.n C, padded settings).
template <class M, int R>
__global__ __launch_bounds__(kWave) void predict_cov_kernel(obe_model m, const double* __restrict__ settings, int64_t ld_s,
                                                            int64_t n_s, const double* __restrict__ particles, int64_t ld_p,
                                                            int64_t n, const double* __restrict__ w, int64_t chunk_len,
                                                            const double* __restrict__ centre, CovRows rows,
                                                            const double* __restrict__ stats, double* __restrict__ partials) {
    constexpr int T = cov_pairs(M::NC);
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_s ? s : n_s - 1;                    // (the padding lanes repeat the last setting)
    double x[M::NS], c0[M::NC], acc_s[T], acc_k[R][M::NC], t[R];
    const double* th[R];
#pragma unroll
    for (int k = 0; k < M::NS; ++k) x[k] = settings[(int64_t)k * ld_s + sc];
#pragma unroll
    for (int c = 0; c < M::NC; ++c) c0[c] = centre[(int64_t)c * n_s + sc];
#pragma unroll
    for (int k = 0; k < T; ++k) acc_s[k] = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int rr = r < rows.n ? r : 0;
        th[r] = particles + (int64_t)rows.row[rr] * ld_p;
        t[r] = stats[rr];
#pragma unroll
        for (int c = 0; c < M::NC; ++c) acc_k[r][c] = 0.0;
    }
    const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    for (int64_t p = p0; p < p1; ++p) {                          // (p, w[p] and the particle are the same for all lanes)
        const double wp = clean_weight(w[p]);
        if (wp == 0.0) continue;
        double y[M::NC], d[M::NC], u[R];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
#pragma unroll
        for (int r = 0; r < R; ++r) u[r] = wp * (th[r][p] - t[r]);
        int k = 0;
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            d[c] = y[c] - c0[c];
            const double wd = wp * d[c];
#pragma unroll
            for (int c2 = 0; c2 <= c; ++c2) {
                acc_s[k] = fma(wd, d[c2], acc_s[k]);
                ++k;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) acc_k[r][c] = fma(u[r], d[c], acc_k[r][c]);
        }
    }
    const int64_t n_pad = (int64_t)gridDim.x * kWave;
    const int64_t slots = T + (int64_t)rows.n * M::NC;
    double* out = partials + (int64_t)blockIdx.y * slots * n_pad + s;
#pragma unroll
    for (int k = 0; k < T; ++k) out[k * n_pad] = acc_s[k];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r < rows.n) {
#pragma unroll
            for (int c = 0; c < M::NC; ++c) out[(T + r * M::NC + c) * n_pad] = acc_k[r][c];
        }
    }
}

// ycov (pairs, n_settings; NULL: not wanted), xcov (slots - pairs, n_settings) = (the chunk partials, added in chunk
// order) / sum w
__global__ __launch_bounds__(kBlock) void predict_cov_fold_kernel(const double* __restrict__ partials, int chunks, int pairs,
                                                                  int slots, int64_t n_pad, int64_t n_s,
                                                                  const u64* __restrict__ hdr, double* __restrict__ ycov,
                                                                  double* __restrict__ xcov) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_s) return;
    const double sw = __longlong_as_double((long long)hdr[0]);
    for (int k = ycov ? 0 : pairs; k < slots; ++k) {
        double acc = 0.0;
        for (int j = 0; j < chunks; ++j) acc += partials[((int64_t)j * slots + k) * n_pad + s];
        double* out = k < pairs ? ycov + (int64_t)k * n_s : xcov + (int64_t)(k - pairs) * n_s;
        out[s] = acc / sw;
    }
}

// ---- K13a: the joint log-likelihood of a set of records, per particle.  Lane = one particle, its rows in registers;
// the chunk's records one after the other from the packed table (the same record for all lanes: scalar loads).
static_assert(kRecWaves == kMomentWaves, "the records pass aims at the waves of the moments");

// words of one record of the table: the setting point, the reading and, known sigma, 1 / sigma per channel
template <class M, bool ROWS>
constexpr int rec_words() { return M::NS + M::NC + (ROWS ? 0 : M::NC); }

// table (n_records, rec_words) and chunk_log[chunk] = sum over the chunk's records and channels of log sigma (NaN if
// one of them is not > 0; ROWS: not written).  One workgroup per chunk; the block sum has a fixed order.
template <class M, bool ROWS>
__global__ __launch_bounds__(kBlock) void records_pack_kernel(const double* __restrict__ settings, int64_t ld_s, int64_t n_r,
                                                              const double* __restrict__ y_meas, int64_t ld_y,
                                                              const double* __restrict__ sigma, int64_t ld_sg,
                                                              int64_t chunk_len, double* __restrict__ table,
                                                              double* __restrict__ chunk_log) {
    __shared__ double red[kBlock / kWave];
    constexpr int W = rec_words<M, ROWS>();
    const int64_t r0 = (int64_t)blockIdx.x * chunk_len;
    const int64_t r1 = r0 + chunk_len < n_r ? r0 + chunk_len : n_r;
    double logs = 0.0;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += kBlock) {
        double* rec = table + r * W;
#pragma unroll
        for (int k = 0; k < M::NS; ++k) rec[k] = settings[(int64_t)k * ld_s + r];
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            rec[M::NS + c] = y_meas[(int64_t)c * ld_y + r];
            if (!ROWS) {
                const double sg = sigma[(int64_t)c * ld_sg + r];
                rec[M::NS + M::NC + c] = 1.0 / sg;
                logs += sg > 0.0 ? log(sg) : __builtin_nan("");
            }
        }
    }
    if (!ROWS) {
        const double s = block_sum(logs, red);
        if (threadIdx.x == 0) chunk_log[blockIdx.x] = s;
    }
}

// partials (chunk, padded particles): -q / 2 - sum log sigma over the chunk's records, q = sum_r sum_c z_rc^2 in record
// order; NaN where the particle contributes nothing
template <class M, bool ROWS>
__global__ __launch_bounds__(kWave) void records_loglik_kernel(obe_model m, const double* __restrict__ table, int64_t n_r,
                                                               int64_t chunk_len, const double* __restrict__ chunk_log,
                                                               ScoreRows rows, const double* __restrict__ particles,
                                                               int64_t ld_p, int64_t n, double* __restrict__ partials) {
    constexpr int W = rec_words<M, ROWS>();
    const int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t p = i < n ? i : n - 1;                         // (the padding lanes repeat the last particle)
    HeldParticle<M> held;
    held.load(particles, ld_p, p);
    double inv[M::NC], neg_log = 0.0;
    bool ok = true;
    if (ROWS) ok = load_noise<M>(rows, particles, ld_p, p, inv, neg_log);
    const int64_t r0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t r1 = r0 + chunk_len < n_r ? r0 + chunk_len : n_r;
    double q = 0.0;
    for (int64_t r = r0; r < r1; ++r) {                          // (r and the record are the same for all lanes)
        const double* rec = table + r * W;
        double x[M::NS], y[M::NC];
#pragma unroll
        for (int k = 0; k < M::NS; ++k) x[k] = rec[k];
        M::eval(x, held.ref(), m, y);
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            const double z = (y[c] - rec[M::NS + c]) * (ROWS ? inv[c] : rec[M::NS + M::NC + c]);
            q = fma(z, z, q);
        }
    }
    // sum log sigma: once per chunk (known sigma), R times the particle's own (noise rows)
    const double logs = ROWS ? -neg_log * (double)(r1 - r0) : chunk_log[blockIdx.y];
    double l = -0.5 * q - logs;
    if (!ok || !(q < kInf)) l = __builtin_nan("");               // (a NaN or +-inf model output leaves q NaN or +inf)
    partials[(int64_t)blockIdx.y * ((int64_t)gridDim.x * kWave) + i] = l;
}

// ---- K14: output-output covariance.  Row r = pivot j * C + channel c' of the call's pivots, R = the rows padded to 1, 4
// or 8.  table (n, R), one particle after the other: u_r = w (y_c'(p_j; theta) - m_c'(p_j)), 0 in the padding rows and
// for a particle of zero weight (never evaluated: whatever its theta is).  pivot_mean (C, n_pivots).
constexpr int kCrossRows = 8;                      // rows one call serves (R of predict_cross_kernel: 1, 4 or 8)

template <class M, int R>
__global__ __launch_bounds__(kBlock) void cross_table_kernel(obe_model m, const double* __restrict__ pivots, int64_t ld_piv,
                                                             int n_pivots, const double* __restrict__ particles, int64_t ld_p,
                                                             int64_t n, const double* __restrict__ w,
                                                             const double* __restrict__ pivot_mean, double* __restrict__ table) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        double* row = table + i * R;
        const double wp = clean_weight(w[i]);
        int filled = 0;
        if (wp != 0.0) {
            for (int j = 0; j < n_pivots; ++j) {                 // (n_pivots * NC <= R: the host checked)
                double x[M::NS], y[M::NC];
#pragma unroll
                for (int k = 0; k < M::NS; ++k) x[k] = pivots[(int64_t)k * ld_piv + j];
                M::eval(x, ParamRef{particles + i, ld_p}, m, y);
#pragma unroll
                for (int c = 0; c < M::NC; ++c) row[j * M::NC + c] = wp * (y[c] - pivot_mean[c * n_pivots + j]);
            }
            filled = n_pivots * M::NC;
        }
        for (int r = filled; r < R; ++r) row[r] = 0.0;
    }
}

// K12's second pass without S: per evaluation the exact model, C subtractions and R C FMAs.  The particle's weight and
// its table row are the same for all lanes.  Rows beyond n_rows are zero in the table and are not written.  partials
// (chunk, n_rows C, padded settings).
template <class M, int R>
__global__ __launch_bounds__(kWave) void predict_cross_kernel(obe_model m, const double* __restrict__ settings, int64_t ld_s,
                                                              int64_t n_s, const double* __restrict__ particles, int64_t ld_p,
                                                              int64_t n, const double* __restrict__ w, int64_t chunk_len,
                                                              const double* __restrict__ centre,
                                                              const double* __restrict__ table, int n_rows,
                                                              double* __restrict__ partials) {
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_s ? s : n_s - 1;                    // (the padding lanes repeat the last setting)
    double x[M::NS], c0[M::NC], acc[R][M::NC];
#pragma unroll
    for (int k = 0; k < M::NS; ++k) x[k] = settings[(int64_t)k * ld_s + sc];
#pragma unroll
    for (int c = 0; c < M::NC; ++c) c0[c] = centre[(int64_t)c * n_s + sc];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int c = 0; c < M::NC; ++c) acc[r][c] = 0.0;
    }
    const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    for (int64_t p = p0; p < p1; ++p) {                          // (p, w[p], the particle and its row: the same for all lanes)
        if (clean_weight(w[p]) == 0.0) continue;
        double y[M::NC], u[R];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
#pragma unroll
        for (int r = 0; r < R; ++r) u[r] = table[p * R + r];
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            const double d = y[c] - c0[c];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r][c] = fma(u[r], d, acc[r][c]);
        }
    }
    const int64_t n_pad = (int64_t)gridDim.x * kWave;
    double* out = partials + (int64_t)blockIdx.y * n_rows * M::NC * n_pad + s;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r < n_rows) {
#pragma unroll
            for (int c = 0; c < M::NC; ++c) out[(r * M::NC + c) * n_pad] = acc[r][c];
        }
    }
}

}  // namespace
}  // namespace obe

using namespace obe;

extern "C" {

int64_t obe_predictive_score_workspace_bytes(int64_t n_particles, int64_t n_records, int32_t n_channels) {
    (void)n_particles;                                           // (the partials are per chunk: bounded whatever the cloud)
    return score_ws_bytes(n_records, n_channels);
}

int obe_predictive_logpdf(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                          const double* d_y_meas, int64_t ld_y, const double* d_sigma, int64_t ld_sigma,
                          const int32_t* h_noise_rows, const double* d_particles, int64_t ld_p, int64_t n_particles,
                          const double* d_weights, double* d_logpdf, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_logpdf) return bad_arg("obe_predictive_logpdf: null pointer");
    Score sc;
    if (int rc = sc.prepare("obe_predictive_logpdf", m, d_settings, ld_s, n_records, d_y_meas, ld_y, d_sigma, ld_sigma,
                            h_noise_rows, d_particles, ld_p, n_particles, d_weights, d_ws, ws_bytes))
        return rc;
    hipStream_t st = as_stream(stream);
    double* partials = reinterpret_cast<double*>(sc.ws.body);
    if (int rc = enqueue_scale(d_weights, n_particles, sc.ws, st)) return rc;
    return dispatch_model(sc.mm, [&](auto M) -> int {
        using Model = decltype(M);
        const dim3 grid((unsigned)sc.tiles, (unsigned)sc.used);
        if (h_noise_rows)
            score_logpdf_kernel<Model, true><<<grid, kWave, 0, st>>>(sc.mm, d_settings, ld_s, n_records, d_y_meas, ld_y,
                                                                     nullptr, 0, sc.rows, d_particles, ld_p, n_particles,
                                                                     d_weights, sc.chunk_len, partials);
        else
            score_logpdf_kernel<Model, false><<<grid, kWave, 0, st>>>(sc.mm, d_settings, ld_s, n_records, d_y_meas, ld_y,
                                                                      d_sigma, ld_sigma, sc.rows, d_particles, ld_p,
                                                                      n_particles, d_weights, sc.chunk_len, partials);
        OBE_CHECK_LAUNCH("score_logpdf_kernel");
        score_logpdf_fold_kernel<<<(int)((n_records + kBlock - 1) / kBlock), kBlock, 0, st>>>(
            partials, sc.used, Model::NC, sc.tiles * kWave, n_records, sc.ws.hdr, d_logpdf);
        OBE_CHECK_LAUNCH("score_logpdf_fold_kernel");
        return 0;
    });
}

int obe_predictive_tails(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                         const double* d_y_meas, int64_t ld_y, const double* d_sigma, int64_t ld_sigma,
                         const int32_t* h_noise_rows, const double* d_particles, int64_t ld_p, int64_t n_particles,
                         const double* d_weights, double* d_lower, double* d_upper, void* d_ws, int64_t ws_bytes,
                         void* stream) {
    if (!d_lower || !d_upper) return bad_arg("obe_predictive_tails: null pointer");
    Score sc;
    if (int rc = sc.prepare("obe_predictive_tails", m, d_settings, ld_s, n_records, d_y_meas, ld_y, d_sigma, ld_sigma,
                            h_noise_rows, d_particles, ld_p, n_particles, d_weights, d_ws, ws_bytes))
        return rc;
    hipStream_t st = as_stream(stream);
    double* partials = reinterpret_cast<double*>(sc.ws.body);
    if (int rc = enqueue_scale(d_weights, n_particles, sc.ws, st)) return rc;
    return dispatch_model(sc.mm, [&](auto M) -> int {
        using Model = decltype(M);
        const dim3 grid((unsigned)sc.tiles, (unsigned)sc.used);
        if (h_noise_rows)
            score_tails_kernel<Model, true><<<grid, kWave, 0, st>>>(sc.mm, d_settings, ld_s, n_records, d_y_meas, ld_y,
                                                                    nullptr, 0, sc.rows, d_particles, ld_p, n_particles,
                                                                    d_weights, sc.chunk_len, partials);
        else
            score_tails_kernel<Model, false><<<grid, kWave, 0, st>>>(sc.mm, d_settings, ld_s, n_records, d_y_meas, ld_y,
                                                                     d_sigma, ld_sigma, sc.rows, d_particles, ld_p,
                                                                     n_particles, d_weights, sc.chunk_len, partials);
        OBE_CHECK_LAUNCH("score_tails_kernel");
        score_tails_fold_kernel<<<(int)((n_records + kBlock - 1) / kBlock), kBlock, 0, st>>>(
            partials, sc.used, Model::NC, sc.tiles * kWave, n_records, sc.ws.hdr, d_lower, d_upper);
        OBE_CHECK_LAUNCH("score_tails_fold_kernel");
        return 0;
    });
}

int64_t obe_predictive_reading_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels, int32_t n_q) {
    (void)n_particles;                                           // (the partials are per chunk: bounded whatever the cloud)
    return reading_ws_bytes(n_settings, n_channels, n_q);
}

int obe_predictive_reading_quantiles(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                                     const double* d_sigma, int64_t ld_sigma, const int32_t* h_noise_rows,
                                     const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                                     const double* h_q, const double* h_z, int32_t n_q, int32_t max_passes,
                                     double* d_quantiles, int32_t* d_passes, void* d_ws, int64_t ws_bytes, void* stream) {
    const char* who = "obe_predictive_reading_quantiles";
    if (!h_q || !h_z || !d_quantiles || !d_passes) return bad_arg("obe_predictive_reading_quantiles: null pointer");
    ReadLevels lv;
    if (int rc = fill_read_levels(who, lv, h_q, h_z, n_q, max_passes)) return rc;
    Score sc;
    if (int rc = sc.prepare(who, m, d_settings, ld_s, n_settings, nullptr, 0, d_sigma, ld_sigma, h_noise_rows, d_particles,
                            ld_p, n_particles, d_weights, d_ws, ws_bytes, n_q))
        return rc;
    hipStream_t st = as_stream(stream);
    const ReadState state = read_carve(sc.ws.body, n_settings, sc.mm.n_channels, n_q);
    return dispatch_model(sc.mm, [&](auto M) -> int {
        using Model = decltype(M);
        const int group = read_group_of(Model::NC), groups = (n_q + group - 1) / group;
        const dim3 grid((unsigned)sc.tiles, (unsigned)sc.used, (unsigned)groups);
        const dim3 fold_grid((unsigned)sc.tiles, (unsigned)groups), fold_block(kWave, (unsigned)(group * Model::NC));
        const int64_t n_pad = sc.tiles * kWave;
        if (h_noise_rows)
            reading_bracket_kernel<Model, true><<<grid, kWave, 0, st>>>(sc.mm, d_settings, ld_s, n_settings, nullptr, 0, sc.rows,
                                                                        d_particles, ld_p, n_particles, d_weights,
                                                                        sc.chunk_len, lv, state.partials);
        else
            reading_bracket_kernel<Model, false><<<grid, kWave, 0, st>>>(sc.mm, d_settings, ld_s, n_settings, d_sigma, ld_sigma,
                                                                         sc.rows, d_particles, ld_p, n_particles, d_weights,
                                                                         sc.chunk_len, lv, state.partials);
        OBE_CHECK_LAUNCH("reading_bracket_kernel");
        reading_init_kernel<<<fold_grid, fold_block, 0, st>>>(sc.used, Model::NC, group, lv, n_pad, n_settings, state,
                                                              d_quantiles, d_passes);
        OBE_CHECK_LAUNCH("reading_init_kernel");
        for (int pass = 1; pass <= max_passes; ++pass) {         // a fixed budget: nothing is waited for
            if (h_noise_rows)
                reading_pass_kernel<Model, true><<<grid, kWave, 0, st>>>(sc.mm, d_settings, ld_s, n_settings, nullptr, 0,
                                                                         sc.rows, d_particles, ld_p, n_particles, d_weights,
                                                                         sc.chunk_len, lv, state);
            else
                reading_pass_kernel<Model, false><<<grid, kWave, 0, st>>>(sc.mm, d_settings, ld_s, n_settings, d_sigma,
                                                                          ld_sigma, sc.rows, d_particles, ld_p, n_particles,
                                                                          d_weights, sc.chunk_len, lv, state);
            OBE_CHECK_LAUNCH("reading_pass_kernel");
            reading_step_kernel<<<fold_grid, fold_block, 0, st>>>(sc.used, Model::NC, group, lv, n_pad, n_settings, state, pass,
                                                                  max_passes, d_quantiles, d_passes);
            OBE_CHECK_LAUNCH("reading_step_kernel");
        }
        return 0;
    });
}

int64_t obe_predictive_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels, int32_t n_q) {
    if (n_settings < 1) n_settings = 1;
    if (n_channels < 1) n_channels = 1;
    if (n_q < 0) n_q = 0;
    if (n_q > kMaxQ) n_q = kMaxQ;
    if (n_particles < 1) n_particles = 1;
    const int64_t body = std::max(moment_words(n_settings, n_channels),
                                  n_q ? select_words(n_particles, n_settings, n_channels, n_q) : 0);
    return (kPredHeadWords + body) * (int64_t)sizeof(u64);
}

int obe_predictive_moments(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                           const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                           double* d_mean, double* d_var, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_mean || !d_var) return bad_arg("obe_predictive_moments: null pointer");
    if (int rc = check_inputs("obe_predictive_moments", m, d_settings, ld_s, n_settings, d_particles, ld_p, n_particles,
                              d_weights, d_ws))
        return rc;
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    if (ws_bytes < obe_predictive_workspace_bytes(n_particles, n_settings, mm.n_channels, 0))
        return bad_arg("obe_predictive_moments: workspace too small");
    hipStream_t st = as_stream(stream);
    const PredWs ws = carve(d_ws);
    const int64_t tiles = setting_tiles(n_settings);
    if (tiles > 0x7fffffff) return bad_arg("obe_predictive_moments: too many settings for one call");
    const int chunks = moment_chunks(n_particles, n_settings);
    // whole waves of particles per chunk (the count of chunks that are not empty may then be smaller)
    const int64_t chunk_len = ((n_particles + chunks - 1) / chunks + kWave - 1) / kWave * kWave;
    const int used = (int)((n_particles + chunk_len - 1) / chunk_len);
    double* partials = reinterpret_cast<double*>(ws.body);
    if (int rc = enqueue_scale(d_weights, n_particles, ws, st)) return rc;
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        const dim3 grid((unsigned)tiles, (unsigned)used);
        const int fold_blocks = (int)((n_settings + kBlock - 1) / kBlock);
        predict_moment_kernel<Model, false><<<grid, kWave, 0, st>>>(mm, d_settings, ld_s, n_settings, d_particles, ld_p,
                                                                    n_particles, d_weights, chunk_len, nullptr, partials);
        OBE_CHECK_LAUNCH("predict_moment_kernel");
        predict_fold_kernel<<<fold_blocks, kBlock, 0, st>>>(partials, used, Model::NC, tiles * kWave, n_settings, ws.hdr,
                                                            d_mean);
        OBE_CHECK_LAUNCH("predict_fold_kernel");
        predict_moment_kernel<Model, true><<<grid, kWave, 0, st>>>(mm, d_settings, ld_s, n_settings, d_particles, ld_p,
                                                                   n_particles, d_weights, chunk_len, d_mean, partials);
        OBE_CHECK_LAUNCH("predict_moment_kernel");
        predict_fold_kernel<<<fold_blocks, kBlock, 0, st>>>(partials, used, Model::NC, tiles * kWave, n_settings, ws.hdr,
                                                            d_var);
        OBE_CHECK_LAUNCH("predict_fold_kernel");
        return 0;
    });
}

int obe_predictive_quantiles(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                             const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                             const double* h_q, int32_t n_q, double* d_quantiles, void* d_ws, int64_t ws_bytes,
                             void* stream) {
    if (!h_q || !d_quantiles) return bad_arg("obe_predictive_quantiles: null pointer");
    if (n_q < 1 || n_q > kMaxQ) return bad_arg("obe_predictive_quantiles: 1..16 quantiles per call");
    for (int j = 0; j < n_q; ++j)
        if (!(h_q[j] >= 0.0 && h_q[j] <= 1.0)) return bad_arg("obe_predictive_quantiles: q outside [0, 1]");
    if (int rc = check_inputs("obe_predictive_quantiles", m, d_settings, ld_s, n_settings, d_particles, ld_p, n_particles,
                              d_weights, d_ws))
        return rc;
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    if (ws_bytes < obe_predictive_workspace_bytes(n_particles, n_settings, mm.n_channels, n_q))
        return bad_arg("obe_predictive_quantiles: workspace too small");
    const int n_c = mm.n_channels;
    const int tile_settings = (int)std::min<int64_t>(n_settings, std::max(1, kTileRows / n_c));
    const int tile_rows = tile_settings * n_c;                 // whole settings: <= tile_rows_bound()
    hipStream_t st = as_stream(stream);
    const PredWs ws = carve(d_ws);
    double* values = reinterpret_cast<double*>(ws.body);
    u64* hist = ws.body + (int64_t)tile_rows * n_particles;
    u64* prefix = hist + (int64_t)tile_rows * n_q * kDigits;
    u64* remaining = prefix + tile_rows * n_q;
    double* found = reinterpret_cast<double*>(remaining + tile_rows * n_q);
    int32_t* d_rows = reinterpret_cast<int32_t*>(found + tile_rows * n_q);
    predict_row_list_kernel<<<1, kTileRows, 0, st>>>(d_rows, tile_rows);          // the tile's rows are 0, 1, 2, ...
    OBE_CHECK_LAUNCH("predict_row_list_kernel");
    OBE_HIP_TRY(hipMemcpyAsync(ws.q, h_q, sizeof(double) * n_q, hipMemcpyHostToDevice, st));
    OBE_HIP_TRY(hipMemsetAsync(hist, 0, (size_t)tile_rows * n_q * kDigits * sizeof(u64), st));      // (handed back zeroed)
    if (int rc = enqueue_scale(d_weights, n_particles, ws, st)) return rc;
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        for (int64_t s0 = 0; s0 < n_settings; s0 += tile_settings) {
            const int ns = (int)std::min<int64_t>(tile_settings, n_settings - s0);
            const int rows = ns * n_c, slots = rows * n_q;
            predict_rows_kernel<Model><<<dim3(stream_blocks(n_particles, kBlock), ns), kBlock, 0, st>>>(
                mm, d_settings, ld_s, s0, d_particles, ld_p, n_particles, values);
            OBE_CHECK_LAUNCH("predict_rows_kernel");
            for (int pass = 0; pass < kPasses; ++pass) {
                select_pass_kernel<<<dim3(cloud_blocks(n_particles), rows), kBlock, (size_t)n_q * kDigits * sizeof(u64), st>>>(
                    values, n_particles, n_particles, d_weights, d_rows, n_q, pass, ws.hdr, prefix, hist);
                OBE_CHECK_LAUNCH("select_pass_kernel");
                select_choose_kernel<<<slots, kWave, 0, st>>>(hist, n_q, ws.q, pass, prefix, remaining, found);
                OBE_CHECK_LAUNCH("select_choose_kernel");
            }
            predict_deliver_kernel<<<(slots + kBlock - 1) / kBlock, kBlock, 0, st>>>(found, s0, ns, n_settings, n_c, n_q,
                                                                                    d_quantiles);
            OBE_CHECK_LAUNCH("predict_deliver_kernel");
        }
        return 0;
    });
}

// (records_pass_bytes, obe_records_pass.h: the table, the chunks' sum log sigma, the chunk partials)
int64_t obe_records_loglik_workspace_bytes(int64_t n_particles, int64_t n_records, int32_t n_channels) {
    return records_pass_bytes(n_particles, n_records, n_channels);
}

int obe_records_loglik(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_records,
                       const double* d_y_meas, int64_t ld_y, const double* d_sigma, int64_t ld_sigma,
                       const int32_t* h_noise_rows, const double* d_particles, int64_t ld_p, int64_t n_particles,
                       int32_t accumulate, double* d_loglik, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!m || !d_settings || !d_y_meas || !d_particles || !d_loglik || !d_ws)
        return bad_arg("obe_records_loglik: null pointer");
    if (n_records < 1 || ld_s < n_records || ld_y < n_records || (d_sigma && ld_sigma < n_records))
        return bad_arg("obe_records_loglik: n_records < 1 or a row of settings, y_meas or sigma shorter than that");
    if (n_particles < 1 || ld_p < n_particles) return bad_arg("obe_records_loglik: bad cloud size");
    if ((d_sigma != nullptr) == (h_noise_rows != nullptr))
        return bad_arg("obe_records_loglik: exactly one of d_sigma and h_noise_rows");
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    ScoreRows rows;
    for (int c = 0; c < OBE_MAX_CHANNELS; ++c) {
        rows.row[c] = (h_noise_rows && c < mm.n_channels) ? h_noise_rows[c] : 0;
        if (rows.row[c] < 0 || rows.row[c] >= mm.n_params) return bad_arg("obe_records_loglik: noise row index out of range");
    }
    if (ws_bytes < obe_records_loglik_workspace_bytes(n_particles, n_records, mm.n_channels))
        return bad_arg("obe_records_loglik: workspace too small");
    const int64_t tiles = particle_tiles(n_particles);
    if (tiles > 0x7fffffff) return bad_arg("obe_records_loglik: too many particles for one call");
    const int chunks = record_chunks(n_records, n_particles);
    const int64_t chunk_len = (n_records + chunks - 1) / chunks;
    const int used = (int)((n_records + chunk_len - 1) / chunk_len);
    hipStream_t st = as_stream(stream);
    double* table = static_cast<double*>(d_ws);
    double* chunk_log = table + n_records * rec_words_bound(mm.n_channels);
    double* partials = chunk_log + kRecWaves;
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        const dim3 grid((unsigned)tiles, (unsigned)used);
        if (h_noise_rows) {
            records_pack_kernel<Model, true><<<used, kBlock, 0, st>>>(d_settings, ld_s, n_records, d_y_meas, ld_y, nullptr, 0,
                                                                      chunk_len, table, chunk_log);
            OBE_CHECK_LAUNCH("records_pack_kernel");
            records_loglik_kernel<Model, true><<<grid, kWave, 0, st>>>(mm, table, n_records, chunk_len, chunk_log, rows,
                                                                       d_particles, ld_p, n_particles, partials);
        } else {
            records_pack_kernel<Model, false><<<used, kBlock, 0, st>>>(d_settings, ld_s, n_records, d_y_meas, ld_y, d_sigma,
                                                                       ld_sigma, chunk_len, table, chunk_log);
            OBE_CHECK_LAUNCH("records_pack_kernel");
            records_loglik_kernel<Model, false><<<grid, kWave, 0, st>>>(mm, table, n_records, chunk_len, chunk_log, rows,
                                                                        d_particles, ld_p, n_particles, partials);
        }
        OBE_CHECK_LAUNCH("records_loglik_kernel");
        records_fold_kernel<<<(int)((n_particles + kBlock - 1) / kBlock), kBlock, 0, st>>>(
            partials, used, tiles * kWave, n_particles, (double)n_records * (Model::NC * kHalfLog2Pi), accumulate != 0,
            d_loglik);
        OBE_CHECK_LAUNCH("records_fold_kernel");
        return 0;
    });
}

int64_t obe_output_covariance_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels, int32_t n_rows) {
    if (n_particles < 1) n_particles = 1;
    if (n_settings < 1) n_settings = 1;
    n_channels = std::min(std::max(n_channels, 1), OBE_MAX_CHANNELS);
    n_rows = std::min(std::max(n_rows, 1), kCovRows);
    return (kPredHeadWords + kCovRowWords + cov_words(n_particles, n_settings, n_channels, n_rows)) * (int64_t)sizeof(u64);
}

int obe_output_covariance(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                          const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                          const double* d_weights, const int32_t* h_rows, int32_t n_rows, double* d_mean, double* d_ycov,
                          double* d_xcov, double* d_pvar, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!h_rows || !d_mean || !d_xcov || !d_pvar) return bad_arg("obe_output_covariance: null pointer");
    if (n_rows < 1 || n_rows > kCovRows) return bad_arg("obe_output_covariance: 1..8 rows per call");
    CovRows rows{};
    rows.n = n_rows;
    for (int r = 0; r < n_rows; ++r) {
        if (h_rows[r] < 0 || h_rows[r] >= n_dims) return bad_arg("obe_output_covariance: row index out of range");
        rows.row[r] = h_rows[r];
    }
    if (int rc = check_inputs("obe_output_covariance", m, d_settings, ld_s, n_settings, d_particles, ld_p, n_particles,
                              d_weights, d_ws))
        return rc;
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    if (n_dims > mm.n_params) return bad_arg("obe_output_covariance: n_dims beyond the model's parameter rows");
    if (ws_bytes < obe_output_covariance_workspace_bytes(n_particles, n_settings, mm.n_channels, n_rows))
        return bad_arg("obe_output_covariance: workspace too small");
    hipStream_t st = as_stream(stream);
    const PredWs ws = carve(d_ws);
    const int64_t tiles = setting_tiles(n_settings);
    if (tiles > 0x7fffffff) return bad_arg("obe_output_covariance: too many settings for one call");
    // the chunks of obe_predictive_moments: its mean, bit for bit
    const int chunks = moment_chunks(n_particles, n_settings);
    const int64_t chunk_len = ((n_particles + chunks - 1) / chunks + kWave - 1) / kWave * kWave;
    const int used = (int)((n_particles + chunk_len - 1) / chunk_len);
    double* stats = reinterpret_cast<double*>(ws.body);
    double* row_first = stats + kCovStats;
    double* row_second = row_first + kCovRows * kPostPartials;
    double* partials = stats + kCovRowWords;
    if (int rc = enqueue_scale(d_weights, n_particles, ws, st)) return rc;
    const int nb = std::min(stream_blocks(n_particles, kBlock * 8), kPostPartials);
    cov_rows_partial_kernel<false><<<dim3(nb, n_rows), kBlock, 0, st>>>(d_particles, ld_p, n_particles, d_weights, rows,
                                                                        nullptr, ws.hdr, row_first);
    OBE_CHECK_LAUNCH("cov_rows_partial_kernel");
    cov_rows_partial_kernel<true><<<dim3(nb, n_rows), kBlock, 0, st>>>(d_particles, ld_p, n_particles, d_weights, rows,
                                                                       row_first, ws.hdr, row_second);
    OBE_CHECK_LAUNCH("cov_rows_partial_kernel");
    cov_rows_fold_kernel<<<n_rows, kBlock, 0, st>>>(row_first, row_second, nb, ws.hdr, stats, d_pvar);
    OBE_CHECK_LAUNCH("cov_rows_fold_kernel");
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        const dim3 grid((unsigned)tiles, (unsigned)used);
        const int fold_blocks = (int)((n_settings + kBlock - 1) / kBlock);
        predict_moment_kernel<Model, false><<<grid, kWave, 0, st>>>(mm, d_settings, ld_s, n_settings, d_particles, ld_p,
                                                                    n_particles, d_weights, chunk_len, nullptr, partials);
        OBE_CHECK_LAUNCH("predict_moment_kernel");
        predict_fold_kernel<<<fold_blocks, kBlock, 0, st>>>(partials, used, Model::NC, tiles * kWave, n_settings, ws.hdr,
                                                            d_mean);
        OBE_CHECK_LAUNCH("predict_fold_kernel");
        auto pass2 = [&](auto R) {
            predict_cov_kernel<Model, decltype(R)::value><<<grid, kWave, 0, st>>>(
                mm, d_settings, ld_s, n_settings, d_particles, ld_p, n_particles, d_weights, chunk_len, d_mean, rows, stats,
                partials);
        };
        if (n_rows == 1) pass2(std::integral_constant<int, 1>{});
        else if (n_rows <= 4) pass2(std::integral_constant<int, 4>{});
        else pass2(std::integral_constant<int, kCovRows>{});
        OBE_CHECK_LAUNCH("predict_cov_kernel");
        const int pairs = cov_pairs(Model::NC);
        predict_cov_fold_kernel<<<fold_blocks, kBlock, 0, st>>>(partials, used, pairs, pairs + n_rows * Model::NC,
                                                                tiles * kWave, n_settings, ws.hdr, d_ycov, d_xcov);
        OBE_CHECK_LAUNCH("predict_cov_fold_kernel");
        return 0;
    });
}

// the header, the pivots' means, the table (8 words a particle whatever R is), the chunk partials of the widest pass:
// (kMomentWaves + setting tiles) x 64 x max(C, rows C) words bound chunks x padded settings whatever the cloud
int64_t obe_output_cross_covariance_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels,
                                                    int32_t n_pivots) {
    if (n_particles < 1) n_particles = 1;
    if (n_settings < 1) n_settings = 1;
    n_channels = std::min(std::max(n_channels, 1), OBE_MAX_CHANNELS);
    n_pivots = std::min(std::max(n_pivots, 1), kCrossRows);
    const int rows = std::min(n_pivots * n_channels, kCrossRows);
    return (kPredHeadWords + kCrossRows + n_particles * kCrossRows + moment_words(n_settings, rows * n_channels))
           * (int64_t)sizeof(u64);
}

int obe_output_cross_covariance(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                                const double* d_pivots, int64_t ld_pivots, int32_t n_pivots, const double* d_particles,
                                int64_t ld_p, int64_t n_particles, const double* d_weights, double* d_mean,
                                int32_t mean_given, double* d_cross, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_pivots || !d_mean || !d_cross) return bad_arg("obe_output_cross_covariance: null pointer");
    if (int rc = check_inputs("obe_output_cross_covariance", m, d_settings, ld_s, n_settings, d_particles, ld_p, n_particles,
                              d_weights, d_ws))
        return rc;
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    if (n_pivots < 1 || ld_pivots < n_pivots || (int64_t)n_pivots * mm.n_channels > kCrossRows)
        return bad_arg("obe_output_cross_covariance: 1..8 rows (pivots x channels) per call, a row of pivots no shorter");
    if (ws_bytes < obe_output_cross_covariance_workspace_bytes(n_particles, n_settings, mm.n_channels, n_pivots))
        return bad_arg("obe_output_cross_covariance: workspace too small");
    hipStream_t st = as_stream(stream);
    const PredWs ws = carve(d_ws);
    const int64_t tiles = setting_tiles(n_settings);
    if (tiles > 0x7fffffff) return bad_arg("obe_output_cross_covariance: too many settings for one call");
    // the chunks of obe_predictive_moments: its mean, bit for bit — for the settings and, a request of their own, the pivots
    auto plan = [&](int64_t n_x, int64_t& chunk_len) {
        const int chunks = moment_chunks(n_particles, n_x);
        chunk_len = ((n_particles + chunks - 1) / chunks + kWave - 1) / kWave * kWave;
        return (int)((n_particles + chunk_len - 1) / chunk_len);
    };
    int64_t chunk_len = 0, piv_chunk_len = 0;
    const int used = plan(n_settings, chunk_len), piv_used = plan(n_pivots, piv_chunk_len);
    double* pivot_mean = reinterpret_cast<double*>(ws.body);
    double* table = pivot_mean + kCrossRows;
    double* partials = table + n_particles * kCrossRows;
    if (int rc = enqueue_scale(d_weights, n_particles, ws, st)) return rc;
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        const dim3 grid((unsigned)tiles, (unsigned)used);
        const int fold_blocks = (int)((n_settings + kBlock - 1) / kBlock);
        const int n_rows = n_pivots * Model::NC;
        predict_moment_kernel<Model, false><<<dim3(1, (unsigned)piv_used), kWave, 0, st>>>(
            mm, d_pivots, ld_pivots, n_pivots, d_particles, ld_p, n_particles, d_weights, piv_chunk_len, nullptr, partials);
        OBE_CHECK_LAUNCH("predict_moment_kernel");
        predict_fold_kernel<<<1, kBlock, 0, st>>>(partials, piv_used, Model::NC, kWave, n_pivots, ws.hdr, pivot_mean);
        OBE_CHECK_LAUNCH("predict_fold_kernel");
        if (!mean_given) {
            predict_moment_kernel<Model, false><<<grid, kWave, 0, st>>>(mm, d_settings, ld_s, n_settings, d_particles, ld_p,
                                                                        n_particles, d_weights, chunk_len, nullptr, partials);
            OBE_CHECK_LAUNCH("predict_moment_kernel");
            predict_fold_kernel<<<fold_blocks, kBlock, 0, st>>>(partials, used, Model::NC, tiles * kWave, n_settings, ws.hdr,
                                                                d_mean);
            OBE_CHECK_LAUNCH("predict_fold_kernel");
        }
        auto pass = [&](auto R) {
            constexpr int kR = decltype(R)::value;
            if constexpr (kR >= Model::NC) {                     // (a call has at least one pivot: C rows)
                cross_table_kernel<Model, kR><<<stream_blocks(n_particles, kBlock), kBlock, 0, st>>>(
                    mm, d_pivots, ld_pivots, n_pivots, d_particles, ld_p, n_particles, d_weights, pivot_mean, table);
                predict_cross_kernel<Model, kR><<<grid, kWave, 0, st>>>(mm, d_settings, ld_s, n_settings, d_particles, ld_p,
                                                                        n_particles, d_weights, chunk_len, d_mean, table,
                                                                        n_rows, partials);
            }
        };
        if (n_rows == 1) pass(std::integral_constant<int, 1>{});
        else if (n_rows <= 4) pass(std::integral_constant<int, 4>{});
        else pass(std::integral_constant<int, kCrossRows>{});
        OBE_CHECK_LAUNCH("predict_cross_kernel");
        predict_cov_fold_kernel<<<fold_blocks, kBlock, 0, st>>>(partials, used, 0, n_rows * Model::NC, tiles * kWave,
                                                                n_settings, ws.hdr, nullptr, d_cross);
        OBE_CHECK_LAUNCH("predict_cov_fold_kernel");
        return 0;
    });
}

}  // extern "C"
