// What scoring a reading (K11) and inverting its tails (K15) need whatever the noise comes from, stated once: the
// Gaussian with a known sigma or noise rows of the cloud (obe_predict.hip) and the noise variance that depends on the
// signal (obe_signal_noise.hip, K21).
//   the plans     lane <-> record or setting, the chunk's particles one after the other; grid = setting tiles x particle
//                 chunks (x level groups), chunks of whole waves of particles, at least kMomentMinChunk each; the
//                 workspace: the header with sum w (enqueue_scale), then the chunk partials and, K15, the rows' state.
//   the folds     score_logpdf_fold_kernel, score_tails_fold_kernel: the chunk partials in chunk order over sum w.
//   K15's state   ReadLevels, ReadState, reading_init_kernel (the bracket's partials into a state per row) and
//                 reading_step_kernel (safeguarded Newton on the log of the tail): they see A, D and the bracket, never
//                 a sigma.
// A noise source keeps its four passes (logpdf, tails, bracket, pass) next to its likelihood and launches these between
// them.  No atomics: the same bits from run to run.  Each source file gets its own copy of the kernels (anonymous
// namespace), as with obe_records_pass.h.
#pragma once

#include <algorithm>
#include <cmath>
#include <string>

#include "obe_models.h"
#include "obe_select.h"

namespace obe {
namespace {

constexpr int kPredHeader = 8;                     // words: [0] sum w, [1] k (scale_kernel)
constexpr int kPredHeadWords = kPredHeader + kPostPartials + kMaxQ;
constexpr int kMomentWaves = 8192;                 // waves a moments pass aims at (32 per CU): chunks = this / setting tiles
constexpr int kMomentMinChunk = 256;               // particles per chunk at least

inline int64_t setting_tiles(int64_t n_settings) { return (n_settings + kWave - 1) / kWave; }
inline int moment_chunks(int64_t n_particles, int64_t n_settings) {
    const int64_t by_size = (n_particles + kMomentMinChunk - 1) / kMomentMinChunk;
    const int64_t by_grid = std::max<int64_t>(1, kMomentWaves / setting_tiles(n_settings));
    return (int)std::max<int64_t>(1, std::min(by_size, by_grid));
}
// chunks x padded settings <= kMomentWaves x 64 + the padded settings, whatever the cloud
inline int64_t moment_words(int64_t n_settings, int n_channels) {
    return ((int64_t)kMomentWaves + setting_tiles(n_settings)) * kWave * n_channels;
}

struct PredWs {
    u64* hdr;
    double* partials;
    double* q;
    u64* body;
};
inline PredWs carve(void* d_ws) {
    u64* base = static_cast<u64*>(d_ws);
    return PredWs{base, reinterpret_cast<double*>(base + kPredHeader),
                  reinterpret_cast<double*>(base + kPredHeader + kPostPartials), base + kPredHeadWords};
}

inline int check_inputs(const char* who, const obe_model* m, const void* d_settings, int64_t ld_s, int64_t n_settings,
                        const void* d_particles, int64_t ld_p, int64_t n_particles, const void* d_weights, const void* d_ws) {
    static thread_local std::string msg;
    const char* what = nullptr;
    if (!m || !d_settings || !d_particles || !d_weights || !d_ws) what = "null pointer";
    else if (n_settings < 1 || ld_s < n_settings) what = "n_settings < 1 or a row of settings shorter than that";
    else if (n_particles < 1 || ld_p < n_particles) what = "bad cloud size";
    if (!what) return 0;
    msg = std::string(who) + ": " + what;
    return bad_arg(msg.c_str());
}

inline int enqueue_scale(const double* d_weights, int64_t n, const PredWs& ws, hipStream_t st) {
    const int nb = std::min(stream_blocks(n, kBlock * 8), kPostPartials);
    wsum_partial_kernel<<<nb, kBlock, 0, st>>>(d_weights, n, ws.partials);
    OBE_CHECK_LAUNCH("wsum_partial_kernel");
    scale_kernel<<<1, kBlock, 0, st>>>(ws.partials, nb, ws.hdr);
    OBE_CHECK_LAUNCH("scale_kernel");
    return 0;
}

// ---- K11: scoring
constexpr double kInf = __builtin_huge_val();
constexpr double kHalfLog2Pi = 0.91893853320467274178;      // log(2 pi) / 2
constexpr double kSqrtHalf = 0.70710678118654752440;

// (m, S) <- (m, S) + s exp(l): S exp(m) is the sum so far, m the largest exponent seen.  One exp; l finite, m finite or
// -inf (never +inf), so no inf - inf is formed.
__device__ __forceinline__ void lse_add(double& m, double& S, double l, double s) {
    const bool up = l > m;
    const double e = exp(up ? m - l : l - m);
    S = up ? S * e + s : S + s * e;
    m = up ? l : m;
}

// d_logpdf (n_records,) = m + log S - log sum w - (C / 2) log 2 pi, the chunks' (m_j, S_j) merged in chunk order
__global__ __launch_bounds__(kBlock) void score_logpdf_fold_kernel(const double* __restrict__ partials, int chunks,
                                                                   int n_channels, int64_t n_pad, int64_t n_r,
                                                                   const u64* __restrict__ hdr, double* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_r) return;
    const double sw = __longlong_as_double((long long)hdr[0]);
    double top = -kInf, S = 0.0;
    for (int j = 0; j < chunks; ++j) {
        const double mj = partials[((int64_t)j * 2 + 0) * n_pad + s];
        if (mj > -kInf) lse_add(top, S, mj, partials[((int64_t)j * 2 + 1) * n_pad + s]);
    }
    double r = __builtin_nan("");
    if (sw > 0.0) r = top > -kInf ? top + log(S) - log(sw) - n_channels * kHalfLog2Pi : -kInf;
    out[s] = r;
}

// d_lower, d_upper (C, n_records) = (the chunk partials, added in chunk order) / sum w
__global__ __launch_bounds__(kBlock) void score_tails_fold_kernel(const double* __restrict__ partials, int chunks,
                                                                  int n_channels, int64_t n_pad, int64_t n_r,
                                                                  const u64* __restrict__ hdr, double* __restrict__ lower,
                                                                  double* __restrict__ upper) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_r) return;
    const double sw = __longlong_as_double((long long)hdr[0]);
    for (int k = 0; k < 2 * n_channels; ++k) {
        double acc = 0.0;
        for (int j = 0; j < chunks; ++j) acc += partials[((int64_t)j * 2 * n_channels + k) * n_pad + s];
        double* out = k < n_channels ? lower : upper;
        out[(int64_t)(k % n_channels) * n_r + s] = acc / sw;
    }
}

// ---- K15: quantiles of the next reading
constexpr int kReadWaves = 4096;                   // waves a pass aims at per level group
constexpr int kReadSlots = 8;                      // (trial, A, D) triples a lane holds
constexpr double kInvSqrt2Pi = 0.39894228040143267794;
constexpr double kReadClose = 0x1p-36;             // a row closes at |A - target| <= this x target ...
constexpr double kReadUlps = 4.0;                  // ... or when its bracket is no wider than this many ulp of its larger end
constexpr double kReadHair = 1e-9;                 // z -+ kReadHair (1 + |z|): an inexact inverse normal CDF keeps the root

inline int read_group_of(int n_channels) { return n_channels < kReadSlots ? kReadSlots / n_channels : 1; }
inline int read_chunks(int64_t n_particles, int64_t n_settings) {
    const int64_t by_size = (n_particles + kMomentMinChunk - 1) / kMomentMinChunk;
    const int64_t by_grid = std::max<int64_t>(1, kReadWaves / setting_tiles(n_settings));
    return (int)std::max<int64_t>(1, std::min(by_size, by_grid));
}

// the levels of a call, by value in the kernel arguments
struct ReadLevels {
    int n;
    int upper[kMaxQ];                              // the level solves in U (q > 1/2)
    double frac[kMaxQ];                            // target / T: q or 1 - q
    double z_lo[kMaxQ], z_hi[kMaxQ];
};

// The levels from h_q and the caller's normal quantiles h_z, and the pass budget: everything of them that can refuse a
// call.  `who` in front of each refusal.
inline int fill_read_levels(const char* who, ReadLevels& lv, const double* h_q, const double* h_z, int32_t n_q, int32_t max_passes) {
    static thread_local std::string msg;
    auto refuse = [&](const char* what) {
        msg = std::string(who) + ": " + what;
        return bad_arg(msg.c_str());
    };
    if (!h_q || !h_z) return refuse("null pointer");
    if (n_q < 1 || n_q > kMaxQ) return refuse("1..16 levels per call");
    if (max_passes < 1 || max_passes > 64) return refuse("max_passes outside 1..64");
    lv = ReadLevels{};
    lv.n = n_q;
    for (int j = 0; j < n_q; ++j) {
        const double q = h_q[j], z = h_z[j];
        if (!(q > 0.0 && q < 1.0)) return refuse("q outside (0, 1)");
        if (!(std::fabs(z) < kInf)) return refuse("h_z is not finite");
        lv.upper[j] = q > 0.5;
        lv.frac[j] = q > 0.5 ? 1.0 - q : q;                      // (1 - q is exact there)
        lv.z_lo[j] = z - kReadHair * (1.0 + std::fabs(z));
        lv.z_hi[j] = z + kReadHair * (1.0 + std::fabs(z));
    }
    return 0;
}

// row = level * C + channel; every array (rows, padded settings) but tile_open (groups, setting tiles)
struct ReadState {
    double *lo, *hi, *trial, *step, *target;
    int32_t* open;
    int32_t* tile_open;
    double* partials;
};
// the state, then the chunk partials of the wider pass (the bracket's C (1 + 2 n_q) slots): chunks x padded settings <=
// (kReadWaves + setting tiles) x 64, whatever the cloud
inline int64_t read_words(int64_t n_settings, int n_channels, int n_q) {
    const int64_t tiles = setting_tiles(n_settings), cells = (int64_t)n_q * n_channels * tiles * kWave;
    return 5 * cells + (cells + 1) / 2 + (n_q * tiles + 1) / 2
           + ((int64_t)kReadWaves + tiles) * kWave * n_channels * (1 + 2 * n_q);
}
inline ReadState read_carve(u64* body, int64_t n_settings, int n_channels, int n_q) {
    const int64_t tiles = setting_tiles(n_settings), cells = (int64_t)n_q * n_channels * tiles * kWave;
    double* d = reinterpret_cast<double*>(body);
    ReadState st;
    st.lo = d, st.hi = d + cells, st.trial = d + 2 * cells, st.step = d + 3 * cells, st.target = d + 4 * cells;
    st.open = reinterpret_cast<int32_t*>(d + 5 * cells);
    st.tile_open = reinterpret_cast<int32_t*>(d + 5 * cells + (cells + 1) / 2);
    st.partials = d + 5 * cells + (cells + 1) / 2 + (n_q * tiles + 1) / 2;
    return st;
}

// ---- the workspaces: obe_predictive_score_workspace_bytes, obe_predictive_reading_workspace_bytes
inline int64_t score_ws_bytes(int64_t n_records, int32_t n_channels) {
    if (n_records < 1) n_records = 1;
    if (n_channels < 1) n_channels = 1;
    return (kPredHeadWords + moment_words(n_records, 2 * n_channels)) * (int64_t)sizeof(u64);
}
inline int64_t reading_ws_bytes(int64_t n_settings, int32_t n_channels, int32_t n_q) {
    if (n_settings < 1) n_settings = 1;
    n_channels = std::min(std::max(n_channels, 1), OBE_MAX_CHANNELS);
    n_q = std::min(std::max(n_q, 1), kMaxQ);
    return (kPredHeadWords + read_words(n_settings, n_channels, n_q)) * (int64_t)sizeof(u64);
}

// The launch geometry of a scoring (n_q == 0) or reading call and its carved workspace.
struct ScorePlan {
    PredWs ws;
    int64_t tiles, chunk_len;
    int used;
    // nullptr, or why the call is refused
    const char* plan(int64_t n_particles, int64_t n_records, int n_channels, int n_q, void* d_ws, int64_t ws_bytes) {
        const int64_t need = n_q ? reading_ws_bytes(n_records, n_channels, n_q) : score_ws_bytes(n_records, n_channels);
        if (ws_bytes < need) return "workspace too small";
        tiles = setting_tiles(n_records);
        if (tiles > 0x7fffffff) return "too many records for one call";
        const int chunks = n_q ? read_chunks(n_particles, n_records) : moment_chunks(n_particles, n_records);
        chunk_len = ((n_particles + chunks - 1) / chunks + kWave - 1) / kWave * kWave;      // whole waves of particles
        used = (int)((n_particles + chunk_len - 1) / chunk_len);
        ws = carve(d_ws);
        return nullptr;
    }
};

// the open rows of this workgroup's block: what the threads of one (64, rows of a group) workgroup found, counted wave
// by wave in thread order
__device__ __forceinline__ int count_open_rows(bool open, int* cnt) {
    const int n = __popcll(__ballot(open));
    if (threadIdx.x == 0) cnt[threadIdx.y] = n;
    __syncthreads();
    int total = 0;
    for (int k = 0; k < (int)blockDim.y; ++k) total += cnt[k];
    return total;
}

// The state of every row from the bracket's partials, folded in chunk order; workgroup (64 settings, the rows of a level
// group), grid (setting tiles, groups).  T_c == 0: NaN, 0 passes, never open.
__global__ void reading_init_kernel(int chunks, int n_channels, int group, ReadLevels lv, int64_t n_pad, int64_t n_s,
                                    ReadState st, double* __restrict__ out, int32_t* __restrict__ passes) {
    __shared__ int cnt[kReadSlots];
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int j = blockIdx.y * group + threadIdx.y / n_channels, c = threadIdx.y % n_channels;
    bool open = false;
    if (j < lv.n) {
        const int64_t slots = (int64_t)n_channels * (1 + 2 * lv.n), at = n_channels + (j * n_channels + c) * 2;
        double T = 0.0, mn = kInf, mx = -kInf;
        for (int k = 0; k < chunks; ++k) {
            const double* part = st.partials + k * slots * n_pad + s;
            T += part[c * n_pad];
            mn = fmin(mn, part[at * n_pad]);
            mx = fmax(mx, part[(at + 1) * n_pad]);
        }
        const int64_t row = (int64_t)j * n_channels + c, idx = row * n_pad + s;
        if (s < n_s) {
            if (T > 0.0) {
                const double lo = nextafter(mn, -kInf), hi = nextafter(mx, kInf);      // (the sums f + z sigma are rounded)
                st.lo[idx] = lo;
                st.hi[idx] = hi;
                st.trial[idx] = 0.5 * lo + 0.5 * hi;
                st.step[idx] = hi - lo;
                st.target[idx] = lv.frac[j] * T;
                open = true;
            } else {
                out[row * n_s + s] = __builtin_nan("");
                passes[row * n_s + s] = 0;
            }
        }
        st.open[idx] = open;
    }
    const int total = count_open_rows(open, cnt);
    if (threadIdx.x == 0 && threadIdx.y == 0) st.tile_open[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// Between two passes: the open rows' A and D folded in chunk order, then the bracket shrunk by the sign of A - target
// and the trial moved.  d_quantiles, d_passes (n_q, C, n_settings) are written when a row closes (passes = this pass)
// and, pass == max_passes, for a row still open (its bracket's midpoint, -max_passes).  The workgroup of the init kernel.
__global__ void reading_step_kernel(int chunks, int n_channels, int group, ReadLevels lv, int64_t n_pad, int64_t n_s,
                                    ReadState st, int pass, int max_passes, double* __restrict__ out,
                                    int32_t* __restrict__ passes) {
    __shared__ int cnt[kReadSlots];
    int32_t* word = st.tile_open + (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (*word == 0) return;                                      // (the whole workgroup: nothing of this tile is open)
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int j = blockIdx.y * group + threadIdx.y / n_channels, c = threadIdx.y % n_channels;
    const int64_t row = (int64_t)j * n_channels + c, idx = row * n_pad + s;
    bool open = j < lv.n && st.open[idx] != 0;
    if (open) {
        double A = 0.0, D = 0.0;
        for (int k = 0; k < chunks; ++k) {
            const double* part = st.partials + ((int64_t)k * (2 * n_channels * lv.n) + row * 2) * n_pad + s;
            A += part[0];
            D += part[n_pad];
        }
        D *= kInvSqrt2Pi;
        const bool up = lv.upper[j] != 0;
        const double y = st.trial[idx], target = st.target[idx];
        double lo = st.lo[idx], hi = st.hi[idx], result = y;
        bool done = fabs(A - target) <= kReadClose * target;
        if (!done) {
            if ((A > target) != up) hi = y;                      // L rises with y, U falls
            else lo = y;
            const double big = fmax(fabs(lo), fabs(hi)), mid = 0.5 * lo + 0.5 * hi;
            result = mid;
            done = hi - lo <= kReadUlps * (nextafter(big, kInf) - big);
            if (!done) {
                const double dy = (A / D) * log(A / target);     // Newton on log A: towards the root with the sign below
                double move = up ? dy : -dy;
                // a step below the resolution of y would leave the trial on the bracket's end it has just become, and
                // the far end where it is: two ulp in Newton's direction instead, so that the far end comes in
                const double ulp2 = 2.0 * (nextafter(fabs(y), kInf) - fabs(y));
                if (fabs(move) < ulp2) move = copysign(ulp2, move);
                double next = y + move;
                if (!(next > lo && next < hi) || !(fabs(dy) <= 0.5 * st.step[idx])) next = mid;
                st.lo[idx] = lo;
                st.hi[idx] = hi;
                st.step[idx] = fabs(next - y);
                st.trial[idx] = next;
            }
        }
        if (done || pass == max_passes) {
            out[row * n_s + s] = result;
            passes[row * n_s + s] = done ? pass : -max_passes;
            st.open[idx] = 0;
            open = false;
        }
    }
    const int total = count_open_rows(open, cnt);
    if (threadIdx.x == 0 && threadIdx.y == 0) *word = total;
}

}  // namespace
}  // namespace obe
