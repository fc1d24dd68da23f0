// What every form of the utility sweep shares (obe_sweep.hip: the direct form and the entry points; obe_sweep_cells.h,
// obe_sweep_bins.h: the two expansion forms of the one-peak Lorentzian): the arguments of a call, the pieces of the
// moment arithmetic, the finish (variance, utility, first maximum, result record) and sweep_finalize.
#pragma once
#include <atomic>
#include <cmath>
#include <cstring>

#include "obe_common.h"
#include "obe_models.h"

namespace obe {

constexpr int kSweepWaves = kBlock / kWave;   // waves of a workgroup: same settings, a quarter of the chunk each
constexpr int kFinSettings = kWave;      // settings per finalize workgroup

// one-workgroup path for reference-semantics sweeps (sweep_small_kernel): draws mode only
constexpr int64_t kSmallSweepDraws = 256, kSmallSweepEvals = 131072;
static bool one_workgroup_sweep(int64_t n_settings, int64_t n_draws) {
    return n_draws <= kSmallSweepDraws && n_settings * n_draws <= kSmallSweepEvals;
}

// packed particle: M::NPK doubles + sqrt(weight), padded to 16 bytes
template <class M>
constexpr int packed_width() { return (M::NPK + 2) & ~1; }

struct SweepPlan {     // obe_sweep.hip: plan_sweep
    int spt;           // settings per thread
    int tiles_x;       // setting tiles of 64 * spt
    int nchunks;       // particle chunks
    int64_t chunk;     // draws per chunk
    int nchunks_bound; // >= nchunks of this plan and of every plan with fewer draws (workspace sizing)
};

struct SweepArgs {
    obe_model m;
    const double* settings;
    int64_t ld_s, ns;
    const double* particles;
    int64_t ld_p;
    const double* weights;
    const int64_t* draw_idx;   // NULL: all particles, weighted
    int64_t nd;                // draws (== n_particles in full mode)
    int64_t n_particles;
    double uniform_w;          // 1/nd in draws mode
    const double* moments;     // obe_moments output: mean parameters at +2
    int64_t chunk;
    int tiles_x, nchunks;      // logical grid: setting tiles x particle chunks
    int one;                   // 1 (a run-time constant the prefetch address is built from)
    int xcd_map;               // chunks in whole groups of 8: block -> (tile, chunk) follows the XCD round robin
    double* packed;            // (nd, packed_width): written by sweep_pack_kernel, read by sweep_kernel
    double* part1;
    double* part2;
    double* cs_out;            // (C, ns): the shift each setting used (0 when unshifted)
    const unsigned* abort;     // OBE_SWEEP_SPECULATIVE: the workspace's abort word (non-zero: do nothing), else NULL
};

// A speculative sweep (enqueued behind an update whose resample decision was not waited for) does nothing
// when that update said "resample": every kernel of the call starts with this test.
__device__ __forceinline__ bool sweep_aborted(const unsigned* abort) {
    return abort && __builtin_amdgcn_readfirstlane(*abort) != 0u;
}

// the particle draw p stands for and its weight: the particle itself (full mode), or draw_idx[p] clamped to the
// cloud with the uniform weight 1/n_draws
__device__ __forceinline__ int64_t draw_source(const SweepArgs& a, int64_t p, double& w) {
    if (!a.draw_idx) {
        w = a.weights[p];
        return p;
    }
    const int64_t src = a.draw_idx[p];
    w = a.uniform_w;
    return src < 0 ? 0 : (src >= a.n_particles ? a.n_particles - 1 : src);
}

// one evaluation into the running moments of its setting and channel about the shift c_s (v = sqrt(w) * y')
template <bool SHIFT>
__device__ __forceinline__ void add_to_moments(double c_s, double sw, double v, double& s1, double& s2) {
    const double u = SHIFT ? fma(-c_s, sw, v) : v;   // sqrt(w) * (y' - c_s)
    s1 = fma(sw, u, s1);                             // sum w (y' - c_s)
    s2 = fma(u, u, s2);                              // sum w (y' - c_s)^2
}

// a wave-uniform 64-bit value, held in scalar registers
__device__ __forceinline__ int64_t wave_uniform(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(static_cast<uint64_t>(v) >> 32));
    return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}

// The sum of p[k * stride], k = 0 .. n - 1, for this lane (`live`: it has one): wavefront g of the FG sums the terms
// g, g + FG, ... (8 loads in flight), the FG sums are added in wavefront order.  Wavefront 0 holds the result.
template <int FG>
__device__ __forceinline__ double fold_in_order(const double* __restrict__ p, int n, int64_t stride, bool live,
                                                double (&acc)[FG][kWave]) {
    const int lane = threadIdx.x & (kWave - 1), grp = threadIdx.x / kWave;
    double sum = 0.0;
    if (live) {
        for (int k0 = grp; k0 < n; k0 += 8 * FG) {
            double t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + u * FG;
                t[u] = p[(int64_t)(k < n ? k : k0) * stride];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const double nx = sum + t[u];
                sum = k0 + u * FG < n ? nx : sum;
            }
        }
    }
    acc[grp][lane] = sum;
    __syncthreads();
    double t = acc[0][lane];
    if (grp == 0) {
#pragma unroll
        for (int g = 1; g < FG; ++g) t += acc[g][lane];
    }
    return t;
}

struct UtilArgs {
    const double* noise_var;
    int64_t noise_ld;     // 0: one value per channel; > 0: (C, n_settings) rows this far apart; < 0: see make_util_args
    const double* cost;   // NULL: scalar
    double cost_scalar;
    int mom_dims;         // noise_ld < 0: noise_var is a K3 block of this many parameters ...
    int mom_rows[OBE_MAX_CHANNELS];   // ... and channel c's noise variance is its m2[row] / sum w
};

// utility of setting s from its nc channel variances var[c * var_stride] (any number of channels)
__device__ __forceinline__ double utility_of(const double* var, int64_t var_stride, int nc, int64_t s,
                                             const UtilArgs& u) {
    // np.sum(var_p / var_n, axis=0) / cost   (obe_base.py:654-655)
    double acc = 0.0;
    for (int c = 0; c < nc; ++c) {
        const double nv = u.noise_ld > 0 ? u.noise_var[(int64_t)c * u.noise_ld + s]
                          : (u.noise_ld == 0 ? u.noise_var[c]
                                             : u.noise_var[2 + 2 * u.mom_dims + u.mom_rows[c]] / u.noise_var[0]);
        acc = acc + var[c * var_stride] / nv;
    }
    return acc / (u.cost ? u.cost[s] : u.cost_scalar);
}

__device__ __forceinline__ void block_argmax(Best b, double* bv, int64_t* bi) {
    __shared__ double sv[kBlock];
    __shared__ int64_t si[kBlock];
    sv[threadIdx.x] = b.v;
    si[threadIdx.x] = b.i;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            Best x{sv[threadIdx.x], si[threadIdx.x]}, y{sv[threadIdx.x + o], si[threadIdx.x + o]};
            if (better(y, x)) {
                sv[threadIdx.x] = y.v;
                si[threadIdx.x] = y.i;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        bv[blockIdx.x] = sv[0];
        bi[blockIdx.x] = si[0];
    }
}

// folds the chunk partials -> yvar, utility; per-workgroup first maximum and worst kappa (argmax_fold finishes).
// A workgroup owns 64 consecutive settings; its FG wavefronts each sum an FG-th of the chunks (coalesced
// 512-byte rows, up to 8 independent loads in flight per lane), the groups are combined in a fixed order
// through LDS.  (One thread per setting walking all chunks serially was latency-bound: 100+ us at 512
// chunks.)  FG = 16 when there are many chunks per setting — a 4096 x 262 144 sweep has 192 of them and only
// 64 finalize workgroups: 4 wavefronts with 4 loads in flight took 10.8 us for its 12.6 MB, 48 dependent
// trips per wave, 16 wavefronts take 7.9 us — FG = 4 when there are few (65 536 x 1 048 576: 40 chunks,
// 1024 workgroups, bandwidth-bound: 11.3 us with 4, 14.3 us with 16).
// Round 4, measured and not kept: argmax_fold's work done here by the last workgroup to arrive (write-through
// entries, arrival counter).  With 64-1024 workgroups the serialised tickets (~12 ns each) and the tail of
// the last workgroup cost more than the launch they save: 14.3 vs 7.9 + 4.9 us (4096 x 262 144), 27.0 vs
// 14.3 + 7.0 us (65 536 x 1 048 576), 18.1 vs 9.6 + 5.2 us (16 384 x 524 288, 10 parameters).  With the two-level
// tickets of obe_common.h: 14.6 vs 8.1 + 5.2, 18.2 vs 10.6 + 7.9, 16.4 vs 9.7 + 5.9 us — level with the two
// launches and their 1.7 us boundary, no better: the last workgroup's tail (drain, tickets, reading the
// entries past L1, the host words) costs what argmax_fold costs.
constexpr int kFinGroupsMany = 16, kFinGroupsFew = 4;      // chunk groups = wavefronts of a finalize workgroup
constexpr int kFinManyChunks = 64;
constexpr int kFinNarrow = 16;             // settings per workgroup of the narrow form (see sweep_finalize) ...
constexpr int kFinNarrowBelow = 128;       // ... used while 64 settings per workgroup would make fewer workgroups than this

// worst cancellation factor so far; a NaN (some variance is NaN) is sticky
__device__ __forceinline__ double kappa_worst(double a, double b) {
    return a != a ? a : (b != b ? b : (a > b ? a : b));
}

// One setting and channel from its moments about the shift c_s: the variance (returned), and the cancellation
// factor (mean of y')^2 / var an UNSHIFTED sweep would suffer, folded into kappa.
// (Measured alternative: chunk partials combined with TwoSum and S1*(S1/W) formed exactly
// with FMAs, plus per-tile flushing of the running sums, lowers the error of the
// unshifted variance from ~1e-15*kappa to ~2e-16*kappa — but the exact product then
// exposes the rounding of S2 itself, e.g. a non-zero variance for a single draw where
// the plain formula cancels to the reference's exact 0.  Not kept.)
__device__ __forceinline__ double variance_of_moments(double S1, double S2, double W, double c_s, double& kappa) {
    const double mu = S1 / W;
    double v = (S2 - S1 * mu) / W;
    v = v > 0.0 ? v : (v != v ? v : 0.0);          // rounding may leave -0 / tiny negatives; NaN stays NaN (np.var)
    const double m = c_s + mu;
    const double k = v != v ? v : (v > 0.0 ? (m * m) / v : (m == 0.0 ? 0.0 : INFINITY));
    kappa = kappa_worst(kappa, k);                 // a NaN variance is reported as kappa = NaN
    return v;
}

// worst kappa over the workgroup (kBlock threads), returned to every thread
__device__ __forceinline__ double block_kappa_worst(double kappa) {
    __shared__ double kred[kBlock];
    kred[threadIdx.x] = kappa;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) kred[threadIdx.x] = kappa_worst(kred[threadIdx.x], kred[threadIdx.x + o]);
        __syncthreads();
    }
    return kred[0];
}

// Where the result goes on the host, as device-visible addresses (page-locked host memory), or all
// NULL: then BestWords::read() copies it.
struct HostResult {
    double* best;
    int64_t* idx;
    double* kappa;
    double* tail = nullptr;     // the result record once more, at the END of the workspace (OBE_WS_RESULT_TAIL), or NULL
};
// (every word is armed by the host and waited for on its own: the order of the stores does not matter)
__device__ __forceinline__ void deliver(const HostResult& h, double v, int64_t i, double k) {
    if (h.tail) {       // where the update calls that reuse the head of the workspace do not reach
        h.tail[0] = v;
        reinterpret_cast<int64_t*>(h.tail)[1] = i;
        h.tail[2] = k;
        h.tail[3] = 0.0;
    }
    if (h.idx) {
        if (h.best) *h.best = v;
        if (h.kappa) *h.kappa = k;
        host_results_before_flag();
        *h.idx = i;
    } else if (h.kappa) {
        if (h.best) *h.best = v;
        host_results_before_flag();
        *h.kappa = k;
    } else if (h.best) {
        *h.best = v;
    }
}

// first maximum (np.argmax order) and worst kappa over a wavefront; valid in lane 0
__device__ __forceinline__ void wave_best(Best& b, double& kappa) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const Best y{__shfl_down(b.v, o, kWave), __shfl_down(b.i, o, kWave)};
        if (better(y, b)) b = y;
        kappa = kappa_worst(kappa, __shfl_down(kappa, o, kWave));
    }
}

// the result record of a sweep / argmax call: out_v[0] best value, [1] kappa, out_i[0] index, and the same as
// one contiguous 32-byte record {value, index bits, kappa, 0} at OBE_WS_RESULT_OFFSET (out_v + 2), so that a
// sharded caller can all-gather it straight from device memory without a host round trip
__device__ __forceinline__ void write_result_record(double* out_v, int64_t* out_i, const Best& b, double k,
                                                    const HostResult& host) {
    out_v[0] = b.v;
    out_i[0] = b.i;
    out_v[1] = k;
    out_v[2] = b.v;
    reinterpret_cast<int64_t*>(out_v)[3] = b.i;
    out_v[4] = k;
    out_v[5] = 0.0;
    deliver(host, b.v, b.i, k);
}

// WS = settings per workgroup: 64 (a wavefront per chunk group), or 16 — then a wavefront holds FOUR chunk groups
// of 16 settings each and the workgroup is a quarter as large, so that a grid of few settings still spreads over
// the chip: 2048 settings x 1024 chunks (one rank's slice of the 7-peak config, 33.5 MB of partials) was 32
// workgroups = 32 CUs, 20.4 us; 128 workgroups: see DESIGN.md K1.  Every setting's chunks are summed by the same
// FG groups in the same order either way: identical bits.
template <int FG, int WS = kFinSettings>
__global__ __launch_bounds__(FG * WS) void sweep_finalize(const double* __restrict__ part1,
                                                             const double* __restrict__ part2, int nchunks, int nc,
                                                             int64_t ns, const double* __restrict__ moments,
                                                             int full_mode, UtilArgs ua,
                                                             const double* __restrict__ cs,
                                                             double* __restrict__ yvar,
                                                             double* __restrict__ utility, double* __restrict__ bv,
                                                             int64_t* __restrict__ bi, double* __restrict__ bk,
                                                             const unsigned* abort) {
    static_assert(WS == 64 || WS == 16, "a wavefront holds one or four chunk groups");
    // (one channel's group sums at a time: OBE_MAX_CHANNELS = 8 of them would not fit the 64 KB of static LDS at
    // FG = 16, WS = 64.  Wavefront 0 turns channel c's sums into its variance before channel c + 1 overwrites them;
    // the sums themselves, their order and the arithmetic on them are what they were: the same bits.)
    __shared__ double acc1[FG][WS];
    __shared__ double acc2[FG][WS];
    if (sweep_aborted(abort)) return;
    const double W = full_mode ? moments[0] : 1.0;
    const int wlane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int lane = wlane % WS, grp = wave * (kWave / WS) + wlane / WS;      // setting within the tile, chunk group
    const int64_t s = (int64_t)blockIdx.x * WS + lane;
    double var[OBE_MAX_CHANNELS];
    double kappa = 0.0;     // worst cancellation factor of this thread's setting
    for (int c = 0; c < nc; ++c) {
        double a1 = 0.0, a2 = 0.0;
        if (s < ns) {
            int k = grp;
            // (8 loads in flight.  Round 5, measured and not kept: 16 per trip — the compiler splits them 5 + 11 with a
            // full wait in between, two round trips as before; a rank's 2048 x 1024 chunks: 12.0 us against 11.2)
            for (; k + 3 * FG < nchunks; k += 4 * FG) {
                double t1[4], t2[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t o = ((int64_t)(k + u * FG) * nc + c) * ns + s;
                    t1[u] = part1[o];
                    t2[u] = part2[o];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    a1 += t1[u];
                    a2 += t2[u];
                }
            }
            if (k < nchunks) {          // the last 1-3 chunks of this group: one batch (clamped, added selectively)
                double t1[3], t2[3];
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    const int kk = k + u * FG;
                    const int64_t o = ((int64_t)(kk < nchunks ? kk : k) * nc + c) * ns + s;
                    t1[u] = part1[o];
                    t2[u] = part2[o];
                }
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    const double n1 = a1 + t1[u], n2 = a2 + t2[u];
                    const bool ok = k + u * FG < nchunks;
                    a1 = ok ? n1 : a1;
                    a2 = ok ? n2 : a2;
                }
            }
        }
        if (c > 0) __syncthreads();          // wavefront 0 has consumed the previous channel's sums
        acc1[grp][lane] = a1;
        acc2[grp][lane] = a2;
        __syncthreads();
        if (wave == 0 && grp == 0 && s < ns) {
            a1 = 0.0;
            a2 = 0.0;
#pragma unroll
            for (int g = 0; g < FG; ++g) {
                a1 += acc1[g][lane];
                a2 += acc2[g][lane];
            }
            var[c] = variance_of_moments(a1, a2, W, cs[(int64_t)c * ns + s], kappa);
            yvar[(int64_t)c * ns + s] = var[c];
        }
    }
    if (wave != 0) return;
    Best best{-INFINITY, INT64_MAX};
    if (grp == 0 && s < ns) {
        const double u = utility_of(var, 1, nc, s, ua);
        utility[s] = u;
        best = Best{u, s};
    }
    wave_best(best, kappa);
    if (wlane == 0) {
        bv[blockIdx.x] = best.v;
        bi[blockIdx.x] = best.i;
        bk[blockIdx.x] = kappa;
    }
}

// what bin_eval_kernel finishes its settings with and where the results go; yvar = NULL: it ends with part1 / part2 /
// cs_out, and finishes nothing (obe_sweep_kernel_time)
struct BinFinish {
    UtilArgs ua;
    int full_mode;
    double* yvar;
    double* utility;
    double* bv;
    int64_t* bi;
    double* bk;
};

// OBE_SWEEP_CELLS and OBE_SWEEP_BINS are honoured where the unshifted, non-SAFE sweep_kernel<Lorentz<1>> would run
static bool expansion_applies(const obe_model& m, int flags, int64_t ns, const int64_t* d_draw_idx, int64_t n_draws) {
    return !(flags & (OBE_SWEEP_SHIFTED | OBE_SWEEP_SAFE)) && m.id == OBE_MODEL_LORENTZ && m.aux == 1
           && !(d_draw_idx && one_workgroup_sweep(ns, n_draws));
}


}  // namespace obe
