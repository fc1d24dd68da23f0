// K1 + K5 — the utility sweep: model evaluated over the settings x draws grid, reduced to
// the per-setting variance of the predicted output, then utility and argmax
// (obe_base.py:463-489 yvar_from_parameter_draws, :628-655 utility_variance,
// :733-756 opt_setting).
//
// Mapping (gfx950):
//   * lane <-> setting.  Each thread owns SPT settings in registers (prepared setting,
//     shift, and the two running moments per channel); nothing is reduced across lanes
//     inside the loop.
//   * sweep_pack_kernel packs every particle ONCE per sweep (per-particle divisions and
//     sqrt(w) hoisted out of the grid) into an AoS array in the workspace.
//   * the particle axis is streamed through the SCALAR path: a packed particle is the same
//     for all 64 lanes, so it is fetched with s_load_dwordx8 into SGPRs (one group ahead of
//     its use) and enters the FP64 instructions as their scalar operand — no LDS tile, no
//     barrier, no VGPRs for broadcast values, and each wave runs on its own.
//   * a workgroup is 4 waves that own the SAME 64*SPT settings and a quarter each of one
//     particle chunk; their moments are added in a fixed order through LDS at the end, so a
//     work item is (64*SPT settings) x (one chunk): ~5000 of them at 65 536 x 1 048 576, six
//     per resident workgroup slot (the launch is one wave of equal items, so its duration is
//     set by how evenly they finish), with partials of only n_chunks x N_s.
//   * grid = setting tiles x particle chunks, XCD-aware; chunk partial moments share one
//     shift per setting, so they simply add (finalize pass).
//   * arithmetic: FP64 VALU only (no contraction over a shared operand => no MFMA).
//     The roof is the FP64 vector rate, not HBM: compulsory traffic is
//     8(D+1)N_p + 8 S N_s bytes for N_s*N_p evaluations.
//
// Variance numerics: moments are accumulated about a per-setting shift
// c_s = model(x_s; mean parameters), so  var = (S2 - S1^2/W)/W  does not cancel
// catastrophically (np.var is two-pass; the shift plays the role of its first pass).
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "obe_common.h"
#include "obe_models.h"
#include "obe_update.h"

namespace obe {

constexpr int kSweepWaves = kBlock / kWave;   // waves of a workgroup: same settings, a quarter of the chunk each
constexpr int kMaxChunks = 1024;
constexpr int kFinMaxBlocks = 65536;     // finalize workgroups (64 settings each) the argmax partials hold
constexpr int kFinSettings = kWave;      // settings per finalize workgroup

static int64_t argmax_slots(int64_t n_settings) {
    return std::max<int64_t>(kMaxBlocks, (n_settings + kFinSettings - 1) / kFinSettings);
}

// one-workgroup path for reference-semantics sweeps (sweep_small_kernel): draws mode only
constexpr int64_t kSmallSweepDraws = 256, kSmallSweepEvals = 131072;
static bool one_workgroup_sweep(int64_t n_settings, int64_t n_draws) {
    return n_draws <= kSmallSweepDraws && n_settings * n_draws <= kSmallSweepEvals;
}

// packed particle: M::NPK doubles + sqrt(weight), padded to 16 bytes
template <class M>
constexpr int packed_width() { return (M::NPK + 2) & ~1; }
#ifdef OBE_PLUGIN_MODEL_HEADER
constexpr int kMaxPackedWidth = packed_width<PluginModel>();
#else
// every registry model: Lorentz<K> K + 2 <= n_dims, lines <= 2, Rabi 3, Coil 7
static int max_packed_width(int n_dims) { return std::max(8, (n_dims + 2) & ~1); }
#endif

struct SweepPlan {
    int spt;           // settings per thread
    int tiles_x;       // setting tiles of 64 * spt
    int nchunks;       // particle chunks
    int64_t chunk;     // draws per chunk
    int nchunks_bound; // >= nchunks of this plan and of every plan with fewer draws (workspace sizing)
};

// Tuned on MI355X at 65 536 x 1 048 576 (docs/DESIGN_rounds_1-5.md, commit 0d615a1): 8 settings per lane (one
// batched reciprocal per 8 evaluations); 768 workgroups are resident (3 per CU at <= 168 VGPRs),
// and the launch is fastest with about six work items per resident slot (4608: within 0.5 % of
// the best; 1536 is 2 % slower).  Smaller grids get fewer (down to 1536: 4 096 x 262 144 takes
// 0.27 ms with 1536 or 4608 items, 0.30 ms with 896), so that the chunk partials stay small.
// "Smaller" is measured in time, not evaluations: `cost` is the model's evaluation time relative to the one-peak
// Lorentzian (sweep_cost<M>).  One rank's 2048 x 524 288 slice of the 7-peak config is as many evaluations as
// 4096 x 262 144 of the one-peak model but runs 1.1 ms: with 1536 items (two rounds of 0.55 ms workgroups) the
// uneven tail costs 5 % — 1.145 / 1.146 ms against 1.093 / 1.083 ms with 4096 (same box, in cycles; 6144 and
// 8192 no better); the one-peak 4096 x 262 144 is indifferent (0.252 vs 0.250-0.254 ms).
static SweepPlan plan_sweep(int64_t ns, int64_t nd, int cost = 1, int max_spt = 8) {
    SweepPlan p;
    // (2048 settings: 8 per lane once there are draws enough for the 384 chunks that keep 1536 work items — one
    // rank's 2048 x 524 288 slice of the 10-parameter config: 1.118 vs 1.133 ms, 1.126 vs 1.146 ms, same box)
    p.spt = ns >= 4096 || (ns >= 2048 && nd >= 131072) ? 8 : (ns >= 1024 ? 4 : (ns >= 512 ? 2 : 1));
    // (a lane keeps 4 running values per setting and channel in registers: models with more than 4 channels get at
    // most 2 settings per lane)
    if (p.spt > max_spt) p.spt = max_spt;
    p.tiles_x = static_cast<int>((ns + (int64_t)kWave * p.spt - 1) / ((int64_t)kWave * p.spt));
    const int64_t by_work = static_cast<int64_t>((double)ns * (double)nd * (double)cost / 1.25e6);
    const int64_t target_blocks = std::max<int64_t>(1536, std::min<int64_t>(4608, by_work));
    int64_t want = (target_blocks + p.tiles_x - 1) / p.tiles_x;
    if (want > 8) want = (want + 7) / 8 * 8;          // whole groups of 8 chunks: one per XCD
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(kMaxChunks, nd / 256));   // >= 64 draws per wave
    p.nchunks = static_cast<int>(std::max<int64_t>(1, std::min(want, cap)));
    // want and cap never decrease with nd, and rounding the chunk up to whole waves below can only
    // lower the count again: this value bounds the chunks of every sweep of <= nd draws
    p.nchunks_bound = p.nchunks;
    p.chunk = (nd + p.nchunks - 1) / p.nchunks;
    p.chunk = (p.chunk + 63) / 64 * 64;
    p.nchunks = static_cast<int>((nd + p.chunk - 1) / p.chunk);
    return p;
}

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

// Every draw packed once per sweep: M::pack() (per-particle divisions, sqrt(w) folded into the
// amplitudes) and sqrt(w), one 16-byte-aligned record per draw.
template <class M>
__global__ __launch_bounds__(kBlock) void sweep_pack_kernel(SweepArgs a) {
    constexpr int NPK = M::NPK, NPKW = packed_width<M>();
    // records wider than 32 bytes leave through LDS (round 5): a thread storing its own 80-byte record makes every
    // store instruction of a wave touch 40 cache lines, 16 bytes each; staged, a workgroup's 256 records are one
    // contiguous run written lane by lane
    constexpr bool STAGED = NPKW > 4 && NPKW <= 24;          // (<= 48 KB of LDS)
    __shared__ double2 tile[STAGED ? kBlock * NPKW / 2 : 1];
    if (sweep_aborted(a.abort)) return;
    const double* __restrict__ thbar = a.moments + 2;   // weighted-mean parameters (K3 output)
    for (int64_t p0 = (int64_t)blockIdx.x * kBlock; p0 < a.nd; p0 += (int64_t)gridDim.x * kBlock) {
        const int64_t p = p0 + threadIdx.x;
        double pk[NPKW];
        if (p < a.nd) {
            double w;
            const int64_t src = draw_source(a, p, w);
            const double sw = sqrt(w);
            M::pack(ParamRef{a.particles + src, a.ld_p}, thbar, a.m, sw, pk);
            pk[NPK] = sw;
#pragma unroll
            for (int k = NPK + 1; k < NPKW; ++k) pk[k] = 0.0;
        }
        if constexpr (STAGED) {
            __syncthreads();           // the previous trip's tile has left
            if (p < a.nd) {
#pragma unroll
                for (int k = 0; k < NPKW / 2; ++k) tile[threadIdx.x * (NPKW / 2) + k] = double2{pk[2 * k], pk[2 * k + 1]};
            }
            __syncthreads();
            const int64_t run = (a.nd - p0 < kBlock ? a.nd - p0 : kBlock) * (NPKW / 2);
            double2* __restrict__ out = reinterpret_cast<double2*>(a.packed + p0 * NPKW);
            for (int64_t e = threadIdx.x; e < run; e += kBlock) out[e] = tile[e];
        } else if (p < a.nd) {
            double2* __restrict__ out = reinterpret_cast<double2*>(a.packed + p * NPKW);
#pragma unroll
            for (int k = 0; k < NPKW / 2; ++k) out[k] = double2{pk[2 * k], pk[2 * k + 1]};
        }
    }
}

// a wave-uniform 64-bit value, held in scalar registers
__device__ __forceinline__ int64_t wave_uniform(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(static_cast<uint64_t>(v) >> 32));
    return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}

// SAFE (models with kHasSafeEval only): evaluate with the model's sweep_eval_safe() — the repeat
// after a sweep whose fast, branch-free batch inversions poisoned a variance (kappa = NaN).
template <class M, int SPT, bool SHIFT, bool SAFE = false>
__global__ __launch_bounds__(kBlock) void sweep_kernel(SweepArgs a) {
    constexpr int NC = M::NC, NXS = M::NXS, NPK = M::NPK, NPKW = packed_width<M>();
    constexpr bool PAIRS = SPT >= 2 && (SAFE ? safe_pair_eval<M>::value : has_pair_eval<M>::value);
    // particles per prefetched group: two groups of packed particles live in SGPRs (~100 per wave)
    constexpr int G = PAIRS ? (NPKW <= 4 ? 4 : 2) : (NPKW <= 4 ? 4 : (NPKW <= 8 ? 2 : 1));
    __shared__ double red[kSweepWaves][NC][2][kWave];

    // XCD-aware block -> (setting tile, particle chunk) map.  Workgroup b is dispatched to
    // XCD b % 8 (observed placement; only speed depends on it): give XCD x the chunks
    // {x, x+8, ...}, so each 4 MiB L2 streams 1/8 of the cloud instead of all of it
    // (rocprofv3 FETCH_SIZE before: 8 x the cloud per launch).
    // (Only when the chunks come in whole groups of 8; a sweep of few draws has fewer chunks than
    // XCDs, and padding the map would leave most of its workgroups — and XCDs — without work.)
    int chunk_id, tile_x;
    if (a.xcd_map) {
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        chunk_id = (slot / a.tiles_x) * 8 + xcd;
        tile_x = slot % a.tiles_x;
    } else {
        chunk_id = blockIdx.x / a.tiles_x;
        tile_x = blockIdx.x % a.tiles_x;
    }
    if (chunk_id >= a.nchunks || sweep_aborted(a.abort)) return;
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;

    double xs[SPT][NXS], cs[SPT][NC], s1[SPT][NC], s2[SPT][NC];
    const double* __restrict__ thbar = a.moments + 2;   // weighted-mean parameters (K3 output)

    {   // prepared settings and the per-setting shift c_s = y'(x_s; mean parameters)
        double pkbar[NPK];
        M::pack(ParamRef{thbar, 1}, thbar, a.m, 1.0, pkbar);
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            int64_t s = ((int64_t)tile_x * SPT + j) * kWave + lane;
            if (s >= a.ns) s = a.ns - 1;
            double x[M::NS];
#pragma unroll
            for (int k = 0; k < M::NS; ++k) x[k] = a.settings[(int64_t)k * a.ld_s + s];
            M::prep_setting(x, a.m, xs[j]);
#pragma unroll
            for (int c = 0; c < NC; ++c) s1[j][c] = s2[j][c] = 0.0;
        }
        if constexpr (SAFE) M::template sweep_eval_safe<SPT>(xs, pkbar, 1.0, a.m, cs);
        else M::template sweep_eval<SPT>(xs, pkbar, 1.0, a.m, cs);
        if (!SHIFT) {
#pragma unroll
            for (int j = 0; j < SPT; ++j)
#pragma unroll
                for (int c = 0; c < NC; ++c) cs[j][c] = 0.0;
        }
    }

    // this wave's quarter of the chunk
    const int64_t c_begin = (int64_t)chunk_id * a.chunk;
    const int64_t c_end = c_begin + a.chunk < a.nd ? c_begin + a.chunk : a.nd;
    const int64_t per = ((c_end - c_begin + 4 * kSweepWaves - 1) / (4 * kSweepWaves)) * 4;
    int64_t p_begin = c_begin + wid * per;
    if (p_begin > c_end) p_begin = c_end;
    const int64_t p_end = p_begin + per < c_end ? p_begin + per : c_end;
    const int n = static_cast<int>(wave_uniform(p_end - p_begin));
    const double* __restrict__ pk = a.packed + wave_uniform(p_begin * NPKW);   // uniform address: scalar loads

    auto accumulate = [&](const double (&v)[SPT][NC], double sw) {
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
#pragma unroll
            for (int c = 0; c < NC; ++c) add_to_moments<SHIFT>(cs[j][c], sw, v[j][c], s1[j][c], s2[j][c]);
        }
    };
    auto load_group = [&](int i0, double (&g)[G][NPKW]) {
#pragma unroll
        for (int e = 0; e < G; ++e)
#pragma unroll
            for (int k = 0; k < NPKW; ++k) g[e][k] = pk[(i0 + e) * NPKW + k];
    };
    // (always_inline: with two call sites the inliner's cost model would decide, and change the SAFE kernels' code)
    auto process_one = [&](const double (&g)[NPKW]) __attribute__((always_inline)) {
        double v[SPT][NC];
        if constexpr (SAFE) M::template sweep_eval_safe<SPT>(xs, g, g[NPK], a.m, v);
        else M::template sweep_eval<SPT>(xs, g, g[NPK], a.m, v);   // sqrt(w) * y'
        accumulate(v, g[NPK]);
    };
    auto process_group = [&](const double (&g)[G][NPKW]) {
        if constexpr (PAIRS) {
#pragma unroll
            for (int e = 0; e < G; e += 2) {              // two particles share one reciprocal
                double va[SPT][NC], vb[SPT][NC];
                if constexpr (SAFE) M::template sweep_eval_pair<SPT, true>(xs, g[e], g[e + 1], va, vb);
                else M::template sweep_eval_pair<SPT>(xs, g[e], g[e + 1], va, vb);
                accumulate(va, g[e][NPK]);
                accumulate(vb, g[e + 1][NPK]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < G; ++e) process_one(g[e]);
        }
    };

    int i = 0;
    if (n >= G) {
        // software pipeline: the next group's scalar loads are in flight while this one is evaluated
        // (an L2 round trip is ~1 us; a group of the Lorentzian is 4 x 8 x 7.4 issue slots ~ 0.4 us)
        double cur[G][NPKW];
        load_group(0, cur);
        asm("" : "+s"(cur[0][0]));     // the first group has landed before the loop: no wait at the loop head,
                                       // where it would also wait for the prefetch just issued
        for (; i + G <= n; i += G) {
            double nxt[G][NPKW];
            // (a.one == 1, unknown to the optimizer: it must not fold the prefetch into the next trip's
            // own load; the last trip re-reads its own group)
            load_group(i + 2 * G <= n ? i + G * a.one : i, nxt);
            __builtin_amdgcn_sched_barrier(0);                // the loads stay ahead of the arithmetic
            process_group(cur);
#pragma unroll
            for (int e = 0; e < G; ++e)
#pragma unroll
                for (int k = 0; k < NPKW; ++k) cur[e][k] = nxt[e][k];
        }
    }
    for (; i < n; ++i) {
        double g[NPKW];
#pragma unroll
        for (int k = 0; k < NPKW; ++k) g[k] = pk[i * NPKW + k];
        process_one(g);
    }

    // (global stores only after the streaming loop: nothing may alias the packed draws before it,
    // or their loads would not be scalar)
    if (chunk_id == 0 && wid == 0) {
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const int64_t s = ((int64_t)tile_x * SPT + j) * kWave + lane;
            if (s < a.ns) {
#pragma unroll
                for (int c = 0; c < NC; ++c) a.cs_out[(int64_t)c * a.ns + s] = cs[j][c];
            }
        }
    }
    // the four waves' moments, added in wave order (fixed association); wave j % 4 writes setting j
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            red[wid][c][0][lane] = s1[j][c];
            red[wid][c][1][lane] = s2[j][c];
        }
        __syncthreads();
        const int64_t s = ((int64_t)tile_x * SPT + j) * kWave + lane;
        if (wid == (j & (kSweepWaves - 1)) && s < a.ns) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                double t1 = red[0][c][0][lane], t2 = red[0][c][1][lane];
#pragma unroll
                for (int g = 1; g < kSweepWaves; ++g) {
                    t1 += red[g][c][0][lane];
                    t2 += red[g][c][1][lane];
                }
                const int64_t o = ((int64_t)chunk_id * NC + c) * a.ns + s;
                a.part1[o] = t1;
                a.part2[o] = t2;
            }
        }
    }
}

// ---- the cell form of the one-peak Lorentzian's unshifted sweep (OBE_SWEEP_CELLS; obe_models.h: LorentzCells) ----
// Three launches in place of sweep_kernel, behind cell_plan_kernel:
//   cell_moments_kernel  lane <-> cell, the packed particles streamed through the scalar path exactly as in
//                        sweep_kernel (no cross-lane reduction); a workgroup is 4 waves that own the same 64 cells
//                        and a quarter each of one particle chunk, added in wave order through LDS: partial
//                        coefficients (chunk, coefficient, cell).
//   cell_fold_kernel     the chunks of one coefficient row summed by 16 wavefronts in a fixed order.
//   cell_eval_kernel     setting -> cell -> Horner; writes part1 / part2 as ONE chunk of sweep_kernel's layout and
//                        cs_out = 0, so that sweep_finalize, argmax_fold and the result record are what they were.
// No floating-point atomics; every sum has a fixed association, so two calls on the same inputs give the same bits.
struct CellPlan {          // written by cell_plan_kernel
    double origin;         // x/d of the left edge of cell 0: the smallest setting of the call
    int ncells;            // 0 when poisoned
    unsigned poison;       // a non-finite setting, more than kMaxCells cells, or d not finite and positive
};
struct CellChunks {
    int nchunks;
    int64_t chunk;         // particles per chunk: whole groups of 4 per wave
    int nchunks_bound;     // >= nchunks of every sweep of fewer draws (workspace sizing)
};
constexpr int kCellWaves = LorentzCells::kMaxCells / kWave;      // wavefronts of cells
constexpr int kCellMaxChunks = 512;      // x 4 waves: two per SIMD of the chip when one wavefront of cells is in use
constexpr int kCellPlanThreads = 1024;
constexpr int kCellFoldGroups = 16;
// FP64 issue slots per (cell, particle) the plan rule reckons with: 8 per order and 16 of set-up (v_rcp_f64 = 4);
// tools/count_isa.py counts 234 in cell_moments_kernel's loop at 28 orders
constexpr double kCellSlots = 8.0 * LorentzCells::kOrder + 16.0;
constexpr double kDirectSlots = 7.3125;                           // sweep_kernel<Lorentz<1>, 8, unshifted> per evaluation
constexpr int64_t kCellFullGridDraws = (int64_t)kCellMaxChunks * 64;     // draws from which every chunk exists

static CellChunks plan_cell_chunks(int64_t nd) {
    CellChunks c;
    c.nchunks_bound = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(kCellMaxChunks, nd / 64)));
    c.chunk = (nd + c.nchunks_bound - 1) / c.nchunks_bound;
    c.chunk = (c.chunk + 15) / 16 * 16;
    c.nchunks = static_cast<int>((nd + c.chunk - 1) / c.chunk);
    return c;
}
// the plan, the folded coefficients and the chunk partials of any cell sweep of AT MOST nd draws
static int64_t cell_ws_doubles(int64_t nd) {
    return 4 + (int64_t)(plan_cell_chunks(nd).nchunks_bound + 1) * LorentzCells::kCoefs * LorentzCells::kMaxCells;
}

// ---- the bin form of the same sweep (OBE_SWEEP_BINS): its plan, its sizes and where its pieces live ----
struct BinPlan {           // written by bin_group_kernel<false> (bin_plan_of)
    double origin;         // the smallest packed tau0: the left edge of bin 0
    int nbins;             // 0 when poisoned
    unsigned poison;       // a non-finite tau0, more than kMaxBins bins, or d not finite and positive
};
constexpr int kBinMinmaxBlocks = 256;
constexpr int kBinMaxUnits = 2048;        // wavefronts of the grouping passes
constexpr int kBinChunk = 1024;           // draws per item of bin_moments_kernel
constexpr int kBinFoldGroups = 16;
constexpr int kBinScanPer = kBinMaxUnits / kBlock;
// FP64 issue slots the plan rule reckons with (tools/count_isa.py): per (setting, bin) in
// bin_eval_kernel, per draw in bin_moments_kernel
constexpr double kBinEvalSlots = 8.0 * LorentzBins::kOrder + 16.0;
constexpr double kBinDrawSlots = 4.0 * LorentzBins::kOrder + 8.0;
// the pipeline's eight launches on a cloud of 64 draws and 64 settings, in lane issue slots: 80 microseconds on one
// MI355X, each sweep launched into a drained stream as a cycle does (obe_sweep_kernel_time: 78-80 us; 61 us back
// to back; DESIGN.md, "K1 by bin expansions"), at the chip's 3.9e7 FP64 lane slots per microsecond (the cell form's
// 1.57e10 lane-instructions in 0.52 ms at 0.77 of the issue rate)
constexpr double kBinFixedSlots = 80.0 * 3.9e7;

struct BinUnits {
    int nunits;
    int64_t per;           // draws per unit: whole wavefronts
};
static BinUnits plan_bin_units(int64_t nd) {
    BinUnits u;
    u.per = (nd + kBinMaxUnits - 1) / kBinMaxUnits;
    u.per = std::max<int64_t>(kWave, (u.per + kWave - 1) / kWave * kWave);
    u.nunits = static_cast<int>((nd + u.per - 1) / u.per);
    return u;
}
// Wavefronts that share a group of 64 settings in bin_eval_kernel (its instances: kBinEvalShapes), from the settings
// of the call alone.  Every instance compiles to at most 168 VGPRs: three wavefronts per SIMD, twelve per CU.  A
// workgroup is G groups x W wavefronts, always a multiple of four: the wavefronts of a workgroup are dealt to the four
// SIMDs of its CU in turn, and workgroups of two, three or six wavefronts leave SIMDs short (they measured slower than
// W = 1: profiles/bin_waves.txt), so W = 3 and 6 come as workgroups of four and two groups.  12 / (G W) whole
// workgroups fit a CU.  The rule: the largest W at which every workgroup of the launch is resident at once on the
// chip's 256 CUs, one round and no tail, which also never asks for more wavefronts than fill the SIMDs to that
// occupancy; 1 where no other instance fits: the workgroups of W = 1 (kBlock threads, four groups) then come in rounds.
// (W = 4 and W = 2 in workgroups of kBlock threads would serve 768 and 1536 groups, but within 168 VGPRs they compile
// to scratch; in workgroups of eight wavefronts they serve no more groups than W = 6 and W = 3 do.)
struct BinEvalShape {
    int waves, groups;         // W, G
};
constexpr BinEvalShape kBinEvalShapes[] = {{8, 1}, {6, 2}, {3, 4}};          // and {1, 4}
constexpr int kBinEvalWavesPerCU = 12, kChipCUs = 256;
static int plan_bin_eval_waves(int64_t ns) {
    const int64_t groups = (ns + kWave - 1) / kWave;
    for (const BinEvalShape& f : kBinEvalShapes)
        if (groups <= (int64_t)kChipCUs * f.groups * (kBinEvalWavesPerCU / (f.groups * f.waves))) return f.waves;
    return 1;
}
static int64_t bin_max_items(int64_t nd) { return (nd + kBinChunk - 1) / kBinChunk + LorentzBins::kMaxBins; }
// where the pieces live, in doubles from a 16-byte aligned base behind the packed draws
struct BinLayout {
    static constexpr int64_t kPlan = 0, kRan = 3, kStarts = 4;                           // plan; marker; 2 x 130 ints
    static constexpr int64_t kMinmax = kStarts + 132;                                   // lo, hi, bad per workgroup
    static constexpr int64_t kTotals = kMinmax + 3 * kBinMinmaxBlocks;                  // 128 ints
    static constexpr int64_t kCounts = kTotals + LorentzBins::kMaxBins / 2;             // bins x units ints
    static constexpr int64_t kCoef = kCounts + (int64_t)LorentzBins::kMaxBins * kBinMaxUnits / 2;
    static constexpr int64_t kPart = kCoef + (int64_t)LorentzBins::kMaxBins * LorentzBins::kRow;
    static int64_t sorted(int64_t nd) { return kPart + bin_max_items(nd) * LorentzBins::kRow; }
    static int64_t doubles(int64_t nd) { return sorted(nd) + 4 * nd; }
};
static_assert(BinLayout::kPart % 2 == 0 && LorentzBins::kRow % 2 == 0, "the sorted records are 16-byte aligned");
// the plan, the tables and the sorted records of any bin sweep of AT MOST nd draws
static int64_t bin_ws_doubles(int64_t nd) { return BinLayout::doubles(nd); }

// ---- the kept grouping (obe_sweep_utility_keep, OBE_SWEEP_BINS_KEPT) ----
// The workspace is scratch of every library call; what outlives a sweep lives in a buffer of the caller's: the plan,
// binstart / itemstart and the sorted position of every draw — functions of the packed tau0 = x0 / d alone.
struct BinKeep {           // head of the buffer
    BinPlan plan;
    unsigned mark;         // kBinKeepMark once the grouping behind it is complete (bin_group_kernel<true> writes it)
    int nd;                // the draws it was made for ...
    unsigned long long dbits;      // ... and the bits of d
    unsigned mismatch;     // the `call` of the last reuse that found a draw outside its kept bin
    unsigned pad[7];
};
static_assert(sizeof(BinKeep) == 64, "the head of the keep buffer is 16 ints");
constexpr unsigned kBinKeepMark = 0x6b455042u;
struct BinKeepLayout {      // in ints
    static constexpr int64_t kStarts = sizeof(BinKeep) / sizeof(int);                       // 2 x 130 ints
    static constexpr int64_t kDest = (kStarts + 2 * (LorentzBins::kMaxBins + 2) + 3) & ~(int64_t)3;
    static int64_t bytes(int64_t nd) { return ((kDest + nd) * (int64_t)sizeof(int) + 15) & ~(int64_t)15; }
};

#ifndef OBE_PLUGIN_MODEL_HEADER
__global__ __launch_bounds__(kCellPlanThreads) void cell_plan_kernel(SweepArgs a, CellPlan* __restrict__ plan) {
    constexpr int NW = kCellPlanThreads / kWave;
    __shared__ double slo[NW], shi[NW];
    __shared__ int sbad[NW];
    if (sweep_aborted(a.abort)) return;
    double lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for (int64_t s0 = threadIdx.x; s0 < a.ns; s0 += 8 * kCellPlanThreads) {
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t s = s0 + (int64_t)u * kCellPlanThreads;
            x[u] = a.settings[s < a.ns ? s : s0];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            bad |= !(fabs(x[u]) <= kDblMax);
            lo = fmin(lo, x[u]);
            hi = fmax(hi, x[u]);
        }
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_down(lo, o, kWave));
        hi = fmax(hi, __shfl_down(hi, o, kWave));
        bad |= __shfl_down(bad, o, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        slo[threadIdx.x / kWave] = lo;
        shi[threadIdx.x / kWave] = hi;
        sbad[threadIdx.x / kWave] = bad;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int g = 1; g < NW; ++g) {
        lo = fmin(lo, slo[g]);
        hi = fmax(hi, shi[g]);
        bad |= sbad[g];
    }
    const double d = a.m.consts[0];
    const double origin = lo / d, top = hi / d;             // (x / d as Lorentz::prep_setting forms it: monotone in x)
    const double n = floor((top - origin) * (1.0 / LorentzCells::kWidth)) + 1.0;
    const bool ok = !bad && d > 0.0 && d <= kDblMax && fabs(origin) <= kDblMax && fabs(top) <= kDblMax
                    && n <= (double)LorentzCells::kMaxCells;             // (a NaN fails every comparison)
    plan->origin = origin;
    plan->ncells = ok ? static_cast<int>(n) : 0;
    plan->poison = ok ? 0u : 1u;
}

__global__ __launch_bounds__(kBlock) void cell_moments_kernel(SweepArgs a, const CellPlan* __restrict__ plan,
                                                              double* __restrict__ part) {
    using LC = LorentzCells;
    constexpr int NPKW = packed_width<Lorentz<1>>(), G = 4;
    static_assert(NPKW == 4, "packed one-peak particle: tau0, sw a, sw b', sw");
    __shared__ double red[kSweepWaves][2][kWave];
    // (the wavefront of cells is the SLOW index: a grid of up to 64 cells leaves the second half of the blocks without
    // work, and workgroups are dealt round robin over the XCDs — interleaved, every other XCD would sit idle)
    const int cw = blockIdx.x / a.nchunks, chunk_id = blockIdx.x % a.nchunks;
    if (sweep_aborted(a.abort)) return;
    const int ncells = __builtin_amdgcn_readfirstlane(plan->ncells);
    if (cw * kWave >= ncells) return;                     // (poisoned: no cells at all)
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const int cell = cw * kWave + lane;                   // (< kMaxCells; beyond ncells: computed, never stored)
    const double tc = LC::centre(plan->origin, cell);

    // this wave's quarter of the chunk
    const int64_t c_begin = (int64_t)chunk_id * a.chunk;
    const int64_t c_end = c_begin + a.chunk < a.nd ? c_begin + a.chunk : a.nd;
    const int64_t per = ((c_end - c_begin + 4 * kSweepWaves - 1) / (4 * kSweepWaves)) * 4;
    int64_t p_begin = c_begin + wid * per;
    if (p_begin > c_end) p_begin = c_end;
    const int64_t p_end = p_begin + per < c_end ? p_begin + per : c_end;
    const int n = static_cast<int>(wave_uniform(p_end - p_begin));
    const double* __restrict__ pk = a.packed + wave_uniform(p_begin * NPKW);   // uniform address: scalar loads

    LC::Sums z;
    z.clear();
    auto load_group = [&](int i0, double (&g)[G][NPKW]) {
#pragma unroll
        for (int e = 0; e < G; ++e)
#pragma unroll
            for (int k = 0; k < NPKW; ++k) g[e][k] = pk[(i0 + e) * NPKW + k];
    };
    int i = 0;
    if (n >= G) {
        // the software pipeline of sweep_kernel: the next group's scalar loads are in flight while this one is expanded
        double cur[G][NPKW];
        load_group(0, cur);
        asm("" : "+s"(cur[0][0]));
        for (; i + G <= n; i += G) {
            double nxt[G][NPKW];
            load_group(i + 2 * G <= n ? i + G * a.one : i, nxt);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < G; ++e) LC::add_particle(tc, cur[e], z);
#pragma unroll
            for (int e = 0; e < G; ++e)
#pragma unroll
                for (int k = 0; k < NPKW; ++k) cur[e][k] = nxt[e][k];
        }
    }
    for (; i < n; ++i) {
        double g[NPKW];
#pragma unroll
        for (int k = 0; k < NPKW; ++k) g[k] = pk[i * NPKW + k];
        LC::add_particle(tc, g, z);
    }

    // (global stores only after the streaming loop, as in sweep_kernel)
    // the four waves' coefficients, two at a time, added in wave order; wave j % 4 writes pair j
    auto fold_pair = [&](int j, double v0, double v1, int co0, int co1) {
        __syncthreads();
        red[wid][0][lane] = v0;
        red[wid][1][lane] = v1;
        __syncthreads();
        if (wid == (j & (kSweepWaves - 1)) && cell < ncells) {
            double t0 = red[0][0][lane], t1 = red[0][1][lane];
#pragma unroll
            for (int g = 1; g < kSweepWaves; ++g) {
                t0 += red[g][0][lane];
                t1 += red[g][1][lane];
            }
            part[((int64_t)chunk_id * LC::kCoefs + co0) * LC::kMaxCells + cell] = t0;
            part[((int64_t)chunk_id * LC::kCoefs + co1) * LC::kMaxCells + cell] = t1;
        }
    };
#pragma unroll
    for (int k = 0; k < LC::kOrder; ++k) fold_pair(k, z.R[k], z.h(k), k, LC::kOrder + k);
    fold_pair(LC::kOrder, z.c1, z.c2, 2 * LC::kOrder, 2 * LC::kOrder + 1);
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

// coef[co][cell] = sum over the chunks of part[chunk][co][cell]
__global__ __launch_bounds__(kCellFoldGroups * kWave) void cell_fold_kernel(const double* __restrict__ part, int nchunks,
                                                                            const CellPlan* __restrict__ plan,
                                                                            double* __restrict__ coef,
                                                                            const unsigned* abort) {
    using LC = LorentzCells;
    __shared__ double acc[kCellFoldGroups][kWave];
    const int cw = blockIdx.x / LC::kCoefs, co = blockIdx.x % LC::kCoefs;
    if (sweep_aborted(abort)) return;
    const int ncells = __builtin_amdgcn_readfirstlane(plan->ncells);
    if (cw * kWave >= ncells) return;
    const int cell = cw * kWave + (threadIdx.x & (kWave - 1));
    const bool live = cell < ncells;
    const double t = fold_in_order<kCellFoldGroups>(part + (int64_t)co * LC::kMaxCells + cell, nchunks,
                                                    (int64_t)LC::kCoefs * LC::kMaxCells, live, acc);
    if (threadIdx.x < kWave && live) coef[(int64_t)co * LC::kMaxCells + cell] = t;
}

// `ran` (next to the plan in the workspace) receives `seq`: how obe_sweep_timing tells a speculative cell sweep that
// ran from one whose three launches returned at once (their durations are too close to tell by the clock)
__global__ __launch_bounds__(kBlock) void cell_eval_kernel(SweepArgs a, const CellPlan* __restrict__ plan,
                                                           const double* __restrict__ coef, unsigned* __restrict__ ran,
                                                           unsigned seq) {
    using LC = LorentzCells;
    if (sweep_aborted(a.abort)) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) *ran = seq;
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= a.ns) return;
    double S1 = __builtin_nan(""), S2 = __builtin_nan("");        // poisoned: kappa = NaN, the caller repeats directly
    const int ncells = plan->ncells;
    if (ncells > 0) {
        double tau;
        Lorentz<1>::prep_setting(a.settings + s, a.m, &tau);
        const double origin = plan->origin;
        int c = static_cast<int>((tau - origin) * (1.0 / LC::kWidth));
        c = c < 0 ? 0 : (c >= ncells ? ncells - 1 : c);
        LC::evaluate(coef + c, LC::kMaxCells, tau - LC::centre(origin, c), S1, S2);
    }
    a.part1[s] = S1;
    a.part2[s] = S2;
    a.cs_out[s] = 0.0;
}
// ---- the bin form of the same sweep (OBE_SWEEP_BINS; obe_models.h: LorentzBins) ----
// The particles are summarised instead of the settings.  No sweep_pack_kernel: the grouping reads the cloud itself
// (tau0 = x0 / d, the division of Lorentz<1>::pack), and a draw's record is formed once, where it is stored:
//   bin_minmax_kernel    min / max of tau0 (zero-weight draws included), one partial per workgroup.
//   bin_group_kernel<0>  every workgroup folds those partials into the plan (origin, bin count, poison word: workgroup 0
//                        stores it); a wavefront owns a contiguous unit of draws, counts them by bin (integers, no
//                        atomics) and leaves every draw's bin and its rank among the unit's draws of that bin (bin_code).
//   bin_scan_kernel      exclusive scan of the counts over the units, bin by bin, and each bin's total.
//   bin_group_kernel<1>  a draw's record goes to (start of its bin) + (draws of that bin in earlier units) + (its
//                        rank) — the order of a stable sort by bin.
//   bin_moments_kernel   lane <-> draw within one item (kBinChunk consecutive draws of ONE bin), 3 P + 2 running sums
//                        per lane, reduced over the lanes once per item (halving_reduce: a butterfly's tree).
//   bin_fold_kernel      a bin's items summed in a fixed order (fold_in_order).
//   bin_eval_kernel      lane <-> setting, a bin's row across the lanes, bins in order, one or several wavefronts per
//                        64 settings (plan_bin_eval_waves); the moments are ONE chunk, and the wavefront that holds
//                        them finishes its 64 settings as sweep_finalize would (no finalize launch: argmax_fold next).
// No floating-point atomics; every sum has a fixed association, so two calls on the same inputs give the same bits.
// With a keep buffer (obe_sweep_utility_keep) the plan, binstart and itemstart live there and bin_group_kernel<1> also
// leaves every draw's sorted position; a later call with OBE_SWEEP_BINS_KEPT runs, in place of the four grouping
// launches,
//   bin_scatter_pack_kernel   the record of draw p (bin_record), written to sorted[dest[p]]
// and then bin_moments_kernel onwards: the same records in the same places, hence the same bits.
struct BinSweepPtrs {
    BinPlan* plan;
    unsigned* ran;
    int* binstart;         // [kMaxBins + 1] first sorted draw of each bin
    int* itemstart;        // [kMaxBins + 1] first item of each bin
    BinKeep* keep;         // the caller's keep buffer (plan, binstart and itemstart point into it), or NULL
    int* dest;             // [nd] the sorted position of every draw, in the keep buffer (NULL without one)
    int* code;             // [nd] a rebuild's bin and rank of every draw (bin_code): dest, or the head of the packed draws
    int reuse;             // OBE_SWEEP_BINS_KEPT: the grouping is read from the keep buffer, not made
    int keep_nd;           // what a reused buffer must have been made for: this many draws ...
    unsigned long long keep_dbits;     // ... and this d
    unsigned call;         // this call among the process's calls with a keep buffer (never 0)
    double* minmax;
    int* totals;
    int* counts;           // [bin * kBinMaxUnits + unit]
    double* coef;
    double* part;
    double* sorted;
};

// OBE_SWEEP_BINS_KEPT: the caller's word that the buffer fits this cloud does not decide what is read through it.  Every
// kernel of a reuse first looks at the head: a complete grouping (the mark) of this many draws at this d.  (A rebuild
// reads what its own kernels have just written.)
__device__ __forceinline__ bool bin_keep_refused(const BinSweepPtrs& q) {
    if (!q.reuse) return false;
    const BinKeep* k = q.keep;
    return !(k->mark == kBinKeepMark && k->nd == q.keep_nd && k->dbits == q.keep_dbits);
}

// tau0 of draw p as the sorted record holds it: Lorentz<1>::pack's division, on the draw's own particle
__device__ __forceinline__ double bin_tau0(const SweepArgs& a, int64_t p) {
    double w;
    const int64_t src = draw_source(a, p, w);
    return a.particles[src] / a.m.consts[0];
}

// the sorted record of draw p: what sweep_pack_kernel<Lorentz<1>> makes of it
__device__ __forceinline__ void bin_record(const SweepArgs& a, int64_t p, double2& ra, double2& rb) {
    using M = Lorentz<1>;
    static_assert(packed_width<M>() == 4 && M::NPK == 3, "the sorted records are 32 bytes");
    double w, pk[4];
    const int64_t src = draw_source(a, p, w);
    const double sw = sqrt(w);
    M::pack(ParamRef{a.particles + src, a.ld_p}, a.moments + 2, a.m, sw, pk);
    ra = double2{pk[0], pk[1]};
    rb = double2{pk[2], sw};
}

// a draw between the two grouping passes of a rebuild: its bin, and its rank among its unit's draws of that bin
constexpr int kBinRankBits = 24;
static_assert((((int64_t)1 << 30) + kBinMaxUnits - 1) / kBinMaxUnits <= ((int64_t)1 << kBinRankBits)
                  && LorentzBins::kMaxBins <= (1 << (31 - kBinRankBits)),
              "a unit of a cloud of 2^30 draws (bin_form_selected) has at most 2^19 draws: rank and bin share an int");
__device__ __forceinline__ int bin_code(int bin, int rank) { return (bin << kBinRankBits) | rank; }

// (the first launch of a rebuild: with a keep buffer, no grouping stands behind its head until the scatter pass says so)
__global__ __launch_bounds__(kBlock) void bin_minmax_kernel(SweepArgs a, BinSweepPtrs q) {
    constexpr int NW = kBlock / kWave;
    __shared__ double slo[NW], shi[NW];
    __shared__ int sbad[NW];
    if (sweep_aborted(a.abort)) return;
    if (q.keep && blockIdx.x == 0 && threadIdx.x == 0) q.keep->mark = 0u;
    double* __restrict__ minmax = q.minmax;
    double lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < a.nd; p += (int64_t)gridDim.x * kBlock) {
        const double t = bin_tau0(a, p);
        bad |= !(fabs(t) <= kDblMax);
        lo = fmin(lo, t);
        hi = fmax(hi, t);
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_down(lo, o, kWave));
        hi = fmax(hi, __shfl_down(hi, o, kWave));
        bad |= __shfl_down(bad, o, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        slo[threadIdx.x / kWave] = lo;
        shi[threadIdx.x / kWave] = hi;
        sbad[threadIdx.x / kWave] = bad;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int g = 1; g < NW; ++g) {
        lo = fmin(lo, slo[g]);
        hi = fmax(hi, shi[g]);
        bad |= sbad[g];
    }
    minmax[blockIdx.x] = lo;
    minmax[kBinMinmaxBlocks + blockIdx.x] = hi;
    minmax[2 * kBinMinmaxBlocks + blockIdx.x] = bad ? 1.0 : 0.0;
}

// The plan from bin_minmax_kernel's partials, by every wavefront for itself and in every lane: at most kBinMinmaxBlocks
// of each kind, 6 KB from L2; min, max and OR are exact in any order.
__device__ __forceinline__ BinPlan bin_plan_of(const SweepArgs& a, const double* __restrict__ minmax, int nblocks) {
    const int lane = threadIdx.x & (kWave - 1);
    double lo = INFINITY, hi = -INFINITY;
    int bad = 0;
#pragma unroll
    for (int g = 0; g < kBinMinmaxBlocks / kWave; ++g) {
        const int b = g * kWave + lane;
        const bool have = b < nblocks;
        lo = fmin(lo, have ? minmax[b] : INFINITY);
        hi = fmax(hi, have ? minmax[kBinMinmaxBlocks + b] : -INFINITY);
        bad |= have ? minmax[2 * kBinMinmaxBlocks + b] != 0.0 : 0;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, o, kWave));
        hi = fmax(hi, __shfl_xor(hi, o, kWave));
        bad |= __shfl_xor(bad, o, kWave);
    }
    const double d = a.m.consts[0];
    const double n = floor((hi - lo) * (1.0 / LorentzBins::kWidth)) + 1.0;
    const bool ok = !bad && d > 0.0 && d <= kDblMax && fabs(lo) <= kDblMax && fabs(hi) <= kDblMax
                    && n <= (double)LorentzBins::kMaxBins;                // (a NaN fails every comparison)
    return BinPlan{lo, ok ? static_cast<int>(n) : 0, ok ? 0u : 1u};
}

// exclusive prefix over the lanes of a wavefront, and the wavefront's total
__device__ __forceinline__ int wave_exclusive(int v, int& total) {
    const int lane = threadIdx.x & (kWave - 1);
    int inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int up = __shfl_up(inc, o, kWave);
        inc += lane >= o ? up : 0;
    }
    total = __shfl(inc, kWave - 1, kWave);
    return inc - v;
}

// The two grouping passes of a rebuild; a wavefront owns a unit of `per` consecutive draws in both.
// SCATTER = false, the counting pass: the plan first (bin_plan_of).  Then the wavefront walks its unit in order, 64 draws
// at a time.  Lane l keeps the count of bins l and l + 64 (c0, c1); per trip the distinct bins of the 64 draws are taken
// one by one (ballot), and a draw's rank is its bin's count so far plus the number of lower lanes with the same bin.
// The counts end as the unit's, and every draw leaves its bin_code.
// SCATTER = true: lane l holds the first sorted position of (bin l, unit) and of (bin l + 64, unit); every draw's
// record (bin_record) is formed from the cloud and written at its bin's first position plus its rank.
template <bool SCATTER>
__global__ __launch_bounds__(kBlock) void bin_group_kernel(SweepArgs a, int64_t per, int nunits, int mm_blocks,
                                                           BinSweepPtrs q) {
    using LB = LorentzBins;
    if (sweep_aborted(a.abort)) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int unit = blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    BinPlan plan;
    if constexpr (SCATTER) {
        plan = *q.plan;
        // the last grouping launch: when it has ended, the keep buffer describes these draws (a poisoned plan included)
        if (q.keep && blockIdx.x == 0 && threadIdx.x == 0) {
            q.keep->nd = static_cast<int>(a.nd);
            q.keep->dbits = q.keep_dbits;
            q.keep->mismatch = 0u;
            q.keep->mark = kBinKeepMark;
        }
    } else {
        plan = bin_plan_of(a, q.minmax, mm_blocks);
        if (blockIdx.x == 0 && threadIdx.x == 0) *q.plan = plan;
    }
    const int nbins = __builtin_amdgcn_readfirstlane(plan.nbins);
    if (nbins == 0) return;
    int c0 = 0, c1 = 0;
    if constexpr (SCATTER) {
        // the bins' first positions (and first items): exclusive prefixes of the totals, by every wavefront for itself
        const int t0 = q.totals[lane], t1 = q.totals[lane + kWave];
        int sum0, sum1, isum0, isum1;
        const int e0 = wave_exclusive(t0, sum0), e1 = sum0 + wave_exclusive(t1, sum1);
        const int i0 = wave_exclusive((t0 + kBinChunk - 1) / kBinChunk, isum0);
        const int i1 = isum0 + wave_exclusive((t1 + kBinChunk - 1) / kBinChunk, isum1);
        if (unit == 0) {
            q.binstart[lane] = e0;
            q.binstart[lane + kWave] = e1;
            q.itemstart[lane] = i0;
            q.itemstart[lane + kWave] = i1;
            if (lane == 0) {
                q.binstart[LB::kMaxBins] = sum0 + sum1;
                q.itemstart[LB::kMaxBins] = isum0 + isum1;
            }
        }
        if (unit >= nunits) return;
        c0 = e0 + q.counts[lane * kBinMaxUnits + unit];
        c1 = e1 + q.counts[(lane + kWave) * kBinMaxUnits + unit];
    }
    if (unit >= nunits) return;
    const int64_t begin = (int64_t)unit * per;
    const int64_t end = begin + per < a.nd ? begin + per : a.nd;
    for (int64_t i0 = begin; i0 < end; i0 += kWave) {
        const int64_t i = i0 + lane;
        const bool live = i < end;
        if constexpr (SCATTER) {
            const int code = live ? q.code[i] : 0;
            const int bin = code >> kBinRankBits;
            // (every lane takes part in the exchange: a lane without a draw asks for bin 0)
            const int first0 = __shfl(c0, bin & (kWave - 1), kWave), first1 = __shfl(c1, bin & (kWave - 1), kWave);
            const int pos = (bin < kWave ? first0 : first1) + (code & ((1 << kBinRankBits) - 1));
            if (live && pos >= 0 && pos < a.nd) {
                double2 ra, rb;
                bin_record(a, i, ra, rb);
                double2* __restrict__ out = reinterpret_cast<double2*>(q.sorted) + 2 * (int64_t)pos;
                out[0] = ra;
                out[1] = rb;
            }
            if (q.dest && live) q.dest[i] = pos;       // (over the code this lane has just read)
        } else {
            const int bin = live ? LB::bin_of(plan.origin, bin_tau0(a, i), nbins) : -1;
            int rank = 0;
            unsigned long long todo = __ballot(live);
            while (todo) {
                const int b = __builtin_amdgcn_readlane(bin, __builtin_ctzll(todo));      // (wave-uniform)
                const unsigned long long same = __ballot(bin == b);
                const int figure = __builtin_amdgcn_readlane(b < kWave ? c0 : c1, b & (kWave - 1));
                if (bin == b) rank = figure + __popcll(same & ((1ull << lane) - 1ull));
                const int n = __popcll(same);
                if (lane == (b & (kWave - 1))) {
                    if (b < kWave) c0 += n;
                    else c1 += n;
                }
                todo &= ~same;
            }
            if (live) q.code[i] = bin_code(bin, rank);
        }
    }
    if constexpr (!SCATTER) {
        q.counts[lane * kBinMaxUnits + unit] = c0;
        q.counts[(lane + kWave) * kBinMaxUnits + unit] = c1;
    }
}

// OBE_SWEEP_BINS_KEPT, in place of the four launches above: the record of draw p (full mode), written where
// bin_group_kernel<true> put it when the keep buffer was made.  Nothing is written unless the head fits the call
// (bin_keep_refused: that is what keeps dest[p] inside `sorted`), and a draw goes nowhere unless it still belongs to
// the bin whose run holds its kept position: a tau0 that is not finite, lies outside the plan or in another bin stores
// the call's number into the head, and bin_eval_kernel answers NaN for the whole call, as for a poisoned plan.  (A
// draw that moved WITHIN its bin gives what a rebuild would: the order of a stable sort by bin does not change.)
__global__ __launch_bounds__(kBlock) void bin_scatter_pack_kernel(SweepArgs a, BinSweepPtrs q) {
    using LB = LorentzBins;
    if (sweep_aborted(a.abort)) return;
    if (bin_keep_refused(q)) return;
    const int nbins = __builtin_amdgcn_readfirstlane(q.plan->nbins);
    if (nbins <= 0 || nbins > LB::kMaxBins) return;
    const double origin = q.plan->origin;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < a.nd; p += (int64_t)gridDim.x * kBlock) {
        double2 ra, rb;
        bin_record(a, p, ra, rb);
        const int pos = q.dest[p];
        const double t = (ra.x - origin) * (1.0 / LB::kWidth);       // (bin_of's expression; a NaN fails the test)
        bool ok = t >= 0.0 && t < (double)nbins && pos >= 0 && pos < a.nd;
        if (ok) {
            const int b = LB::bin_of(origin, ra.x, nbins);
            ok = q.binstart[b] <= pos && pos < q.binstart[b + 1];
        }
        if (ok) {
            double2* __restrict__ out = reinterpret_cast<double2*>(q.sorted) + 2 * (int64_t)pos;
            out[0] = ra;
            out[1] = rb;
        } else {
            q.keep->mismatch = q.call;
        }
    }
}

// one workgroup per bin: counts[bin][unit] -> the number of the bin's draws in earlier units, and its total
__global__ __launch_bounds__(kBlock) void bin_scan_kernel(int nunits, BinSweepPtrs q, const unsigned* abort) {
    __shared__ int wsum[kBlock / kWave];
    if (sweep_aborted(abort)) return;
    const int nbins = __builtin_amdgcn_readfirstlane(q.plan->nbins);
    const int bin = blockIdx.x;
    if (nbins == 0) return;
    if (bin >= nbins) {
        if (threadIdx.x == 0) q.totals[bin] = 0;
        return;
    }
    int* __restrict__ row = q.counts + bin * kBinMaxUnits;
    int v[kBinScanPer], mine = 0;
#pragma unroll
    for (int u = 0; u < kBinScanPer; ++u) {
        const int k = threadIdx.x * kBinScanPer + u;
        v[u] = k < nunits ? row[k] : 0;
        mine += v[u];
    }
    int wtotal;
    int before = wave_exclusive(mine, wtotal);
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = wtotal;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int g = 0; g < kBlock / kWave; ++g) {
        if (g < (int)threadIdx.x / kWave) before += wsum[g];
        total += wsum[g];
    }
#pragma unroll
    for (int u = 0; u < kBinScanPer; ++u) {
        const int k = threadIdx.x * kBinScanPer + u;
        if (k < nunits) row[k] = before;
        before += v[u];
    }
    if (threadIdx.x == 0) q.totals[bin] = total;
}

// N sums per lane reduced over the 64 lanes by recursive halving: at distance DIST a lane keeps the lower or the upper
// half of its list (an odd list is padded), by its lane bit DIST, and adds its partner's copy of that half — mine +
// partner's, which is what both lanes of a pair compute for that value in a butterfly, so every value passes through
// the butterfly's tree and has its bits, in N/2 + N/4 + ... exchanges instead of 6 N.  A lane ends with two values.
template <int N, int DIST>
__device__ __forceinline__ void halving_reduce(const double (&v)[N], int lane, double (&out)[2]) {
    constexpr int H = (N + 1) / 2;
    const bool upper = (lane & DIST) != 0;
    double k[H];
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const double lo = v[i], hi = H + i < N ? v[H + i] : 0.0;
        const double mine = upper ? hi : lo, send = upper ? lo : hi;
        k[i] = mine + __shfl_xor(send, DIST, kWave);
    }
    if constexpr (DIST > 1) {
        halving_reduce<H, DIST / 2>(k, lane, out);
    } else {
        static_assert(H == 2, "64 lanes x 2 values: at most 128 sums");
        out[0] = k[0];
        out[1] = k[1];
    }
}
// which of the N sums out[e] of halving_reduce<N, 32> is on this lane; -1: padding
template <int N>
__device__ __forceinline__ int halving_index(int lane, int e) {
    int n[7];
    n[0] = N;
#pragma unroll
    for (int l = 0; l < 6; ++l) n[l + 1] = (n[l] + 1) / 2;
    int j = e;
    bool real = true;
#pragma unroll
    for (int l = 5; l >= 0; --l) {                        // level l: distance 32 >> l, lane bit 5 - l
        j += ((lane >> (5 - l)) & 1) * n[l + 1];
        real = real && j < n[l];
    }
    return real ? j : -1;
}

// one wavefront per item: kBinChunk consecutive sorted draws of one bin
__global__ __launch_bounds__(kWave) void bin_moments_kernel(BinSweepPtrs q, const unsigned* abort) {
    using LB = LorentzBins;
    if (sweep_aborted(abort)) return;
    if (bin_keep_refused(q)) return;
    const int nbins = __builtin_amdgcn_readfirstlane(q.plan->nbins);
    if (nbins == 0) return;
    const int lane = threadIdx.x, item = blockIdx.x;
    if (item >= q.itemstart[LB::kMaxBins]) return;
    // the last bin whose first item is not behind this one (an empty bin shares its first item with the next)
    const int s0 = q.itemstart[lane], s1 = q.itemstart[lane + kWave];
    const int bin = __popcll(__ballot(lane < nbins && s0 <= item)) + __popcll(__ballot(lane + kWave < nbins && s1 <= item)) - 1;
    const int first = q.binstart[bin] + (item - q.itemstart[bin]) * kBinChunk;
    const int last = q.binstart[bin + 1];
    const int end = first + kBinChunk < last ? first + kBinChunk : last;
    const double tb = LB::centre(q.plan->origin, bin);
    const double2* __restrict__ rec = reinterpret_cast<const double2*>(q.sorted);
    LB::Sums z;
    z.clear();
    // the records of the next trip are asked for before this trip's arithmetic: the wait for them sits behind it
    int i = first + lane;
    double2 ra = double2{0.0, 0.0}, rb = ra;
    if (i < end) {
        ra = rec[2 * (int64_t)i];
        rb = rec[2 * (int64_t)i + 1];
    }
    while (i < end) {
        const int in = i + kWave;
        double2 na = ra, nb = rb;
        if (in < end) {
            na = rec[2 * (int64_t)in];
            nb = rec[2 * (int64_t)in + 1];
        }
        const double pk[4] = {ra.x, ra.y, rb.x, rb.y};
        LB::add_draw(tb, pk, z);
        ra = na;
        rb = nb;
        i = in;
    }
    // the 64 lanes' sums of coefficient j (M1_k at k, M2_k at kOrder + k, M3_k at 2 kOrder + k, c1, c2), each through
    // the tree (l, l ^ 32), then ^ 16, ... ^ 1 of a butterfly, of which a lane keeps only the half it will store
    double v[LB::kCoefs], kept[2];
#pragma unroll
    for (int k = 0; k < LB::kOrder; ++k) {
        v[k] = z.M1[k];
        v[LB::kOrder + k] = z.M2[k];
        v[2 * LB::kOrder + k] = z.M3[k];
    }
    v[3 * LB::kOrder] = z.c1;
    v[3 * LB::kOrder + 1] = z.c2;
    halving_reduce<LB::kCoefs, kWave / 2>(v, lane, kept);
    double* __restrict__ out = q.part + (int64_t)item * LB::kRow;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int j = halving_index<LB::kCoefs>(lane, e);
        if (j < 0) continue;                              // (padding of an odd level)
        const bool m3 = j >= 2 * LB::kOrder && j < 3 * LB::kOrder;
        out[j] = kept[e] * (m3 ? (double)(j - 2 * LB::kOrder + 1) : 1.0);      // H3_k = (k + 1) M3_k
    }
}

// coef[bin][co] = sum over the bin's items of part[item][co]
__global__ __launch_bounds__(kBinFoldGroups * kWave) void bin_fold_kernel(BinSweepPtrs q, const unsigned* abort) {
    using LB = LorentzBins;
    __shared__ double acc[kBinFoldGroups][kWave];
    if (sweep_aborted(abort)) return;
    if (bin_keep_refused(q)) return;
    const int nbins = __builtin_amdgcn_readfirstlane(q.plan->nbins);
    const int bin = blockIdx.x >> 1, co = (blockIdx.x & 1) * kWave + (threadIdx.x & (kWave - 1));
    if (bin >= nbins) return;
    const int first = __builtin_amdgcn_readfirstlane(q.itemstart[bin]);
    const int n = __builtin_amdgcn_readfirstlane(q.itemstart[bin + 1]) - first;
    if (n == 0) return;                                   // (an empty bin: bin_eval_kernel never reads its row)
    const bool live = co < LB::kCoefs;
    const double t = fold_in_order<kBinFoldGroups>(q.part + (int64_t)first * LB::kRow + co, n, LB::kRow, live, acc);
    if (threadIdx.x < kWave && live) q.coef[(int64_t)bin * LB::kRow + co] = t;
}

#endif  // !OBE_PLUGIN_MODEL_HEADER

struct UtilArgs {
    const double* noise_var;
    int64_t noise_ld;     // 0: one value per channel; > 0: (C, n_settings) rows this far apart; < 0: see make_util_args
    const double* cost;   // NULL: scalar
    double cost_scalar;
    int mom_dims;         // noise_ld < 0: noise_var is a K3 block of this many parameters ...
    int mom_rows[OBE_MAX_CHANNELS];   // ... and channel c's noise variance is its m2[row] / sum w
};

// noise_ld < 0 (OBE_NOISE_FROM_MOMENTS): the noise variance of channel c is np.average(sigma_c^2, weights=w)
// (obe_noiseparam.py:122-136) = m2[row_c] / sum w of the K3 block d_noise_var points to — the division that
// obe_noise_var_from_moments()'s kernel does, done by the kernel that needs the value: one launch (4-5 us between
// the update and every sweep of a noise-parameter object) less, the same bits.
static int make_util_args(UtilArgs& ua, const double* d_noise_var, int64_t noise_ld, const double* d_cost, double cost_scalar,
                          int n_channels, int n_params) {
    ua = UtilArgs{d_noise_var, noise_ld, d_cost, cost_scalar, 0, {}};
    if (noise_ld >= 0) return 0;
    const int64_t code = -noise_ld - 1;
    ua.mom_dims = n_params;
    for (int c = 0; c < OBE_MAX_CHANNELS; ++c) {
        ua.mom_rows[c] = (int)((code >> (5 * c)) & 31);
        if (c < n_channels && ua.mom_rows[c] >= n_params) return bad_arg("noise rows encoded in noise_ld: out of range");
    }
    if (n_params < 1 || n_params > OBE_MAX_DIMS) return bad_arg("noise_ld < 0 needs the number of parameters");
    return 0;
}

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

#ifndef OBE_PLUGIN_MODEL_HEADER
// `ran` receives `seq`, as in cell_eval_kernel.  A bin's row is the same for the 64 settings of a wavefront, so it is
// held in registers across the lanes and named lane by lane where it is used (obe_models.h: LorentzBins::LaneRow): a
// wavefront fetches the rows of its own bins from q.coef (at most OBE_BIN_MAX rows of 688 bytes, the same lines for
// every wavefront of the chip), the row of its next occupied bin before it evaluates the current one, and the series
// sums wait for no memory.  (The rows used to come through an LDS tile: one exposed LDS round trip per series step,
// DESIGN.md.)  Two register sets take turns, so that no row register is ever copied.  The occupied bins are two
// ballots over binstart (lane <-> bin), walked lowest first.
// A workgroup holds G groups of 64 settings (lane <-> setting) and W wavefronts for each of them.
// <4, 1>: a workgroup of kBlock threads, every wavefront walks every occupied bin of its own group; no LDS, no barrier.
// W > 1: of every tile of kBinTile bins wavefront w of a group evaluates the occupied bins t = w, w + W, ... and leaves
// their t1, t2 in LDS, and behind a barrier wavefront 0 of the group adds them in bin order, as the one wavefront of
// W = 1 does: the same numbers in the same order, the same bits, and the one dependent chain per bin is walked by W
// wavefronts at once (plan_bin_eval_waves; DESIGN.md, "Several wavefronts per group of settings").  Every wavefront of
// a workgroup passes two barriers per tile of the plan, whichever bins it owns: nbins and the abort word (read once
// per workgroup where W > 1) are the same for all.  All 64 lanes stay active to the end (LaneRow).
// The bin form makes ONE chunk of moments, and the wavefront that holds S1 / S2 of a group is the group of 64 settings
// of a workgroup of sweep_finalize<kFinGroupsFew>: it finishes its own settings (BinFinish) with finalize's device
// functions on finalize's operands, and argmax_fold receives the partials finalize would have written.
constexpr int kBinTile = 16;
template <int G, int W>
__global__ __launch_bounds__(G * W * kWave, W == 1 ? 1 : 3)           // (W > 1: registers for three wavefronts per SIMD)
void bin_eval_kernel(SweepArgs a, BinSweepPtrs q, unsigned seq, BinFinish f) {
    using LB = LorentzBins;
    constexpr int kThreads = G * W * kWave;
    static_assert(W > 1 || kThreads == kBlock, "W = 1 is the workgroup of four groups");
    static_assert((G * W) % 4 == 0, "whole wavefronts for every SIMD of the CU (plan_bin_eval_waves)");
    static_assert(LB::kMaxBins <= 2 * kWave && kWave % kBinTile == 0, "two ballots name the occupied bins");
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    const int grp = wave % G, wid = wave / G;             // wavefront `wid` of group `grp`
    double* term = nullptr;                               // W > 1, the group's: t1 at [t][lane], t2 at [kBinTile + t][lane]
    if constexpr (W == 1) {
        if (sweep_aborted(a.abort)) return;
    } else {
        __shared__ double terms[G * 2 * kBinTile * kWave];
        __shared__ int stop;
        term = terms + grp * (2 * kBinTile * kWave);
        if (threadIdx.x == 0) stop = sweep_aborted(a.abort);
        __syncthreads();
        if (stop) return;
    }
    const int64_t s = ((int64_t)blockIdx.x * G + grp) * kWave + lane;
    // (a reuse whose keep buffer does not fit the call, or one of whose draws has left its kept bin: as if poisoned)
    const bool refused = bin_keep_refused(q) || (q.reuse && q.keep->mismatch == q.call);
    const int nbins = refused ? 0 : __builtin_amdgcn_readfirstlane(q.plan->nbins);
    double S1 = __builtin_nan(""), S2 = __builtin_nan("");        // poisoned: kappa = NaN, the caller repeats without the bit
    if (nbins > 0) {
        double tau;
        Lorentz<1>::prep_setting(a.settings + (s < a.ns ? s : a.ns - 1), a.m, &tau);
        const double origin = q.plan->origin;
        const double* __restrict__ coef = q.coef;
        // (the row of an empty bin was never written: it is never fetched)
        const int* __restrict__ start = q.binstart;
        const bool here0 = lane < nbins && start[lane + 1] != start[lane];
        const bool here1 = kWave + lane < nbins && start[kWave + lane + 1] != start[kWave + lane];
        const uint64_t occ0 = __ballot(here0), occ1 = __ballot(here1);            // bins 0-63, 64-127
        uint64_t own0 = occ0, own1 = occ1;                                        // ... that this wavefront evaluates
        double c1col[2] = {0.0, 0.0}, c2col[2] = {0.0, 0.0};                      // W > 1, wavefront 0: lane <-> bin
        if constexpr (W > 1) {
            uint64_t mine = 0;
            for (int t = wid; t < kBinTile; t += W) mine |= (uint64_t)1 << t;
            mine |= mine << 16;
            mine |= mine << 32;
            own0 &= mine;
            own1 &= mine;
            if (wid == 0) {
                if (here0) {
                    c1col[0] = coef[lane * LB::kRow + 3 * LB::kOrder];
                    c2col[0] = coef[lane * LB::kRow + 3 * LB::kOrder + 1];
                }
                if (here1) {
                    c1col[1] = coef[(kWave + lane) * LB::kRow + 3 * LB::kOrder];
                    c2col[1] = coef[(kWave + lane) * LB::kRow + 3 * LB::kOrder + 1];
                }
            }
        }
        auto next_bin = [&]() {                                   // the lowest bin left, or -1 (wave-uniform)
            int b = -1;
            if (own0) {
                b = __builtin_ctzll(own0);
                own0 &= own0 - 1;
            } else if (own1) {
                b = kWave + __builtin_ctzll(own1);
                own1 &= own1 - 1;
            }
            return b;
        };
        double a1 = 0.0, a2 = 0.0, C1 = 0.0, C2 = 0.0;
        int tile = 0;                                             // W > 1: the tile whose terms are being written
        auto close_tile = [&]() {
            __syncthreads();                                      // the tile's terms are in LDS
            if (wid == 0) {
                const int half = tile * kBinTile / kWave;
                const uint64_t occ = half ? occ1 : occ0;
                for (int t = 0; t < kBinTile; ++t) {
                    const int l = (tile * kBinTile + t) & (kWave - 1);
                    if (!((occ >> l) & 1)) continue;              // skipped, not added as zero
                    a1 += term[t * kWave + lane];
                    a2 += term[(kBinTile + t) * kWave + lane];
                    C1 += readlane_f64(half ? c1col[1] : c1col[0], l);
                    C2 += readlane_f64(half ? c2col[1] : c2col[0], l);
                }
            }
            __syncthreads();                                      // ... and summed: the next tile's may replace them
            ++tile;
        };
        auto evaluate = [&](const LB::LaneRow& row, int b) {
            double t1, t2;
            if constexpr (W == 1) {
                LB::evaluate(row, LB::centre(origin, b) - tau, t1, t2);
                a1 += t1;
                a2 += t2;
                LB::add_constants(row, C1, C2);
            } else {
                while (tile < b / kBinTile) close_tile();
                LB::evaluate(row, LB::centre(origin, b) - tau, t1, t2);
                term[(b % kBinTile) * kWave + lane] = t1;
                term[(kBinTile + b % kBinTile) * kWave + lane] = t2;
            }
        };
        LB::LaneRow row0, row1;
        // (behind the last bin its own row is fetched once more: a fetch under a condition would make the wait for
        // the current row a wait for every load in flight)
        int b0 = next_bin();
        if (b0 >= 0) {
            LB::load_row(coef + b0 * LB::kRow, lane, row0);
            for (;;) {
                const int b1 = next_bin();
                LB::load_row(coef + (b1 >= 0 ? b1 : b0) * LB::kRow, lane, row1);
                evaluate(row0, b0);
                if (b1 < 0) break;
                b0 = next_bin();
                LB::load_row(coef + (b0 >= 0 ? b0 : b1) * LB::kRow, lane, row0);
                evaluate(row1, b1);
                if (b0 < 0) break;
            }
        }
        if constexpr (W > 1)
            while (tile < (nbins + kBinTile - 1) / kBinTile) close_tile();
        S1 = a1 + C1;
        S2 = a2 + C2;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *q.ran = seq;
    if (W > 1 && wid != 0) return;
    if (!f.yvar) {
        if (s >= a.ns) return;
        a.part1[s] = S1;
        a.part2[s] = S2;
        a.cs_out[s] = 0.0;
        return;
    }
    // sweep_finalize's workgroup blockIdx.x * G + grp, with one chunk, one channel and the shift 0: its chain of
    // additions from 0.0 comes to 0.0 + S (a -0 becomes +0, a NaN stays)
    const int64_t group = (int64_t)blockIdx.x * G + grp;
    if (group * kWave >= a.ns) return;
    double kappa = 0.0;
    Best best{-INFINITY, INT64_MAX};
    if (s < a.ns) {
        const double var = variance_of_moments(0.0 + S1, 0.0 + S2, f.full_mode ? a.moments[0] : 1.0, 0.0, kappa);
        f.yvar[s] = var;
        const double u = utility_of(&var, 1, 1, s, f.ua);
        f.utility[s] = u;
        best = Best{u, s};
    }
    wave_best(best, kappa);
    if (lane == 0) {
        f.bv[group] = best.v;
        f.bi[group] = best.i;
        f.bk[group] = kappa;
    }
}
#endif  // !OBE_PLUGIN_MODEL_HEADER

__global__ __launch_bounds__(kBlock) void utility_kernel(const double* __restrict__ yvar, int nc, int64_t ns,
                                                         UtilArgs ua, double* __restrict__ utility,
                                                         double* __restrict__ bv, int64_t* __restrict__ bi) {
    Best best{-INFINITY, INT64_MAX};
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < ns; s += (int64_t)gridDim.x * kBlock) {
        const double u = utility_of(yvar + s, ns, nc, s, ua);      // (noise_ld >= 0 here: obe_utility_argmax)
        utility[s] = u;
        Best cand{u, s};
        if (better(cand, best)) best = cand;
    }
    block_argmax(best, bv, bi);
}

__global__ __launch_bounds__(kBlock) void argmax_kernel(const double* __restrict__ v, int64_t n,
                                                        double* __restrict__ bv, int64_t* __restrict__ bi) {
    Best best{-INFINITY, INT64_MAX};
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += (int64_t)gridDim.x * kBlock) {
        Best cand{v[s], s};
        if (better(cand, best)) best = cand;
    }
    block_argmax(best, bv, bi);
}

// one block: first-max over the block partials -> scalars {value, index (as int64 bits)}
__global__ __launch_bounds__(kBlock) void argmax_fold(const double* __restrict__ bv, const int64_t* __restrict__ bi,
                                                      int nb, const double* __restrict__ bk,
                                                      double* __restrict__ out_v,
                                                      int64_t* __restrict__ out_i, HostResult host,
                                                      const unsigned* abort = nullptr) {
    if (sweep_aborted(abort)) return;       // (the armed host words stay armed: nobody reads this result)
    Best best{-INFINITY, INT64_MAX};
    double kmax = 0.0;                  // worst cancellation factor; NaN is sticky
    // (the partials of four rounds of threads — value, index, kappa: up to 12 loads — in flight together; compared in
    // the order b, b + 256, ... of the one-at-a-time loops: the same winner.  1024 partials used to be 8 dependent
    // round trips in a one-workgroup kernel whose whole duration is latency)
    for (int base = 0; base < nb; base += 4 * kBlock) {
        double v[4], kk[4];
        int64_t ix[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = base + r * kBlock + (int)threadIdx.x, bc = b < nb ? b : nb - 1;
            v[r] = bv[bc];
            ix[r] = bi[bc];
            kk[r] = bk ? bk[bc] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = base + r * kBlock + (int)threadIdx.x;
            if (b < nb) {
                const Best cand{v[r], ix[r]};
                if (better(cand, best)) best = cand;
                kmax = kappa_worst(kmax, kk[r]);
            }
        }
    }
    block_argmax(best, out_v, out_i);   // gridDim.x == 1 -> writes element 0
    const double k = block_kappa_worst(kmax);
    if (threadIdx.x == 0) write_result_record(out_v, out_i, Best{out_v[0], out_i[0]}, k, host);
}

// Reference-semantics sweeps are tiny (201 settings x 30 draws in the demos): one workgroup
// does what sweep_kernel + sweep_finalize + argmax_fold do in three launches — the draws are
// packed into LDS once, each thread walks its settings, and the block folds utility, first
// maximum and kappa.  Same formulas and summation order as the SPT = 1, one-chunk path of the
// big kernels, hence the same bits: the arithmetic is the same functions.
template <class M, bool SAFE>
__global__ __launch_bounds__(kBlock) void sweep_small_kernel(SweepArgs a, UtilArgs ua, double* __restrict__ yvar,
                                                             double* __restrict__ utility,
                                                             double* __restrict__ out_v,
                                                             int64_t* __restrict__ out_i, HostResult host) {
    constexpr int NC = M::NC, NXS = M::NXS, NPK = M::NPK, NPKW = packed_width<M>();
    extern __shared__ __attribute__((aligned(16))) double tile[];
    const double* __restrict__ thbar = a.moments + 2;
    const int nd = static_cast<int>(a.nd);
    for (int i = threadIdx.x; i < nd; i += kBlock) {
        double w;
        const int64_t src = draw_source(a, i, w);
        const double sw = sqrt(w);
        double pk[NPK];
        M::pack(ParamRef{a.particles + src, a.ld_p}, thbar, a.m, sw, pk);
#pragma unroll
        for (int k = 0; k < NPK; ++k) tile[i * NPKW + k] = pk[k];
        tile[i * NPKW + NPK] = sw;
    }
    __syncthreads();
    double pkbar[NPK];
    M::pack(ParamRef{thbar, 1}, thbar, a.m, 1.0, pkbar);
    auto eval = [&](const double (&xs)[1][NXS], const double* pk, double sw, double (&v)[1][NC]) {
        if constexpr (SAFE) M::template sweep_eval_safe<1>(xs, pk, sw, a.m, v);
        else M::template sweep_eval<1>(xs, pk, sw, a.m, v);
    };
    const double W = 1.0;      // draws mode: uniform weights 1/nd
    Best best{-INFINITY, INT64_MAX};
    double kappa = 0.0;
    for (int64_t s = threadIdx.x; s < a.ns; s += kBlock) {
        double x[M::NS], xs[1][NXS], cs[1][NC], s1[NC], s2[NC];
#pragma unroll
        for (int k = 0; k < M::NS; ++k) x[k] = a.settings[(int64_t)k * a.ld_s + s];
        M::prep_setting(x, a.m, xs[0]);
        eval(xs, pkbar, 1.0, cs);
#pragma unroll
        for (int c = 0; c < NC; ++c) s1[c] = s2[c] = 0.0;
        for (int i = 0; i < nd; ++i) {
            double pk[NPK], v[1][NC];
#pragma unroll
            for (int k = 0; k < NPK; ++k) pk[k] = tile[i * NPKW + k];
            const double sw = tile[i * NPKW + NPK];
            eval(xs, pk, sw, v);
#pragma unroll
            for (int c = 0; c < NC; ++c) add_to_moments<true>(cs[0][c], sw, v[0][c], s1[c], s2[c]);
        }
        double var[OBE_MAX_CHANNELS];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            var[c] = variance_of_moments(s1[c], s2[c], W, cs[0][c], kappa);
            yvar[(int64_t)c * a.ns + s] = var[c];
        }
        const double u = utility_of(var, 1, NC, s, ua);
        utility[s] = u;
        const Best cand{u, s};
        if (better(cand, best)) best = cand;
    }
    block_argmax(best, out_v, out_i);       // one block: element 0
    const double k = block_kappa_worst(kappa);
    if (threadIdx.x == 0) write_result_record(out_v, out_i, Best{out_v[0], out_i[0]}, k, host);
}

// np.var(utility_y_space, axis=0): two-pass over the (small) draw axis
__global__ __launch_bounds__(kBlock) void yspace_var_kernel(const double* __restrict__ ysp, int64_t nd,
                                                            int64_t row /* C*Ns */, double* __restrict__ yvar) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < row; e += (int64_t)gridDim.x * kBlock) {
        // (eight draws' loads in flight together, added in draw order as before: one load / wait / add per draw
        // made the 30 draws of a reference-semantics cycle 60 dependent round trips)
        double sum = 0.0;
        for (int64_t d0 = 0; d0 < nd; d0 += 8) {
            double t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = ysp[(d0 + j < nd ? d0 + j : nd - 1) * row + e];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const double n = sum + t[j];
                sum = d0 + j < nd ? n : sum;
            }
        }
        const double mean = sum / (double)nd;
        double acc = 0.0;
        for (int64_t d0 = 0; d0 < nd; d0 += 8) {
            double t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = ysp[(d0 + j < nd ? d0 + j : nd - 1) * row + e];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const double dv = t[j] - mean;
                const double sq = dv * dv;
                const double n = acc + sq;
                acc = d0 + j < nd ? n : acc;
            }
        }
        yvar[e] = acc / (double)nd;
    }
}

// Optional timing of the sweep kernel inside real cycles (obe_sweep_timing): events around the
// launch on its own stream, read after the stream synchronisation the result copy needs anyway.
struct SweepTiming {
    bool on = false;
    int device = -1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double total_ms = 0.0;
    int64_t launches = 0;
    bool pending = false;      // a speculative call's events have not been read yet
    double pending_min_ms = 0.0;
    const unsigned* pending_ran = nullptr;     // a speculative CELL sweep: the marker its last kernel writes if it runs ...
    unsigned pending_seq = 0, seq = 0;         // ... and the value to find there
};
static SweepTiming g_timing;

// the time between the pair of events (both completed) joins the totals, unless it is shorter than min_ms
static void count_timed_sweep(double min_ms = 0.0) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_timing.e0, g_timing.e1) != hipSuccess) return;
    if (ms >= min_ms) {
        g_timing.total_ms += ms;
        g_timing.launches += 1;
    }
}

// A speculative call returns before its kernels have run: its pair of events is read at the next timed call
// or query.  An aborted sweep (its update resampled) is not a sweep: shorter than any kernel could sweep
// that many evaluations (half of 8e12 evaluations/s, well above this chip's rate), it is left out.
static void resolve_pending_timing() {
    if (!g_timing.pending) return;
    g_timing.pending = false;
    if (hipEventSynchronize(g_timing.e1) != hipSuccess) return;
    if (g_timing.pending_ran) {        // (the cell form: three launches that return at once are not told apart by the clock)
        unsigned ran = 0;
        const bool read = hipMemcpy(&ran, g_timing.pending_ran, sizeof ran, hipMemcpyDeviceToHost) == hipSuccess;
        if (read && ran == g_timing.pending_seq) count_timed_sweep();
        return;
    }
    count_timed_sweep(g_timing.pending_min_ms);
}

struct SweepWs {
    double* part1;
    double* part2;
    double* bv;
    int64_t* bi;
    double* out_v;
    int64_t* out_i;
    double* bk;
    double* cs;
    double* packed;
};

// what a cell sweep (OBE_SWEEP_CELLS) or a bin sweep (OBE_SWEEP_BINS) keeps behind the packed draws, with the slack
// that aligns it; a library built for one generated model has neither form
static int64_t cell_form_doubles(int64_t nd) {
#ifdef OBE_PLUGIN_MODEL_HEADER
    return 0;
#else
    return cell_ws_doubles(nd) + 2;
#endif
}
static int64_t bin_form_doubles(int64_t nd) {
#ifdef OBE_PLUGIN_MODEL_HEADER
    return 0;
#else
    return bin_ws_doubles(nd) + 2;
#endif
}
static int64_t sweep_ws_bytes(int64_t part_doubles, int64_t cs_doubles, int64_t slots, int64_t packed_doubles) {
    return (2 * part_doubles + cs_doubles + 3 * slots + 16 + packed_doubles + 2) * (int64_t)sizeof(double);
}
// ... of any sweep of ns settings, nc channels and AT MOST nd draws (obe_workspace_bytes)
static int64_t sweep_ws_bytes_bound(int64_t ns, int64_t nd, int nc, int packed_w) {
    const SweepPlan p = plan_sweep(ns, nd, 1 << 20);       // (the grid of the costliest model: the most chunks)
    // (sized by the monotone bound: the chunk count itself is not monotone in nd after the rounding
    // of the chunk length, and a sweep of N_DRAWS < n_particles draws runs in the same workspace)
    return sweep_ws_bytes((int64_t)p.nchunks_bound * nc * ns, (int64_t)nc * ns, argmax_slots(ns),
                          nd * packed_w + std::max(cell_form_doubles(nd), bin_form_doubles(nd)));
}
static int carve_sweep_ws(void* d_ws, int64_t ws_bytes, int64_t part_doubles, int64_t cs_doubles, SweepWs& w,
                          int64_t slots = kMaxBlocks, int64_t packed_doubles = 0) {
    const int64_t need = sweep_ws_bytes(part_doubles, cs_doubles, slots, packed_doubles);
    if (!d_ws || ws_bytes < need) return bad_arg("sweep workspace too small");
    double* base = static_cast<double*>(d_ws);
    w.out_v = base;                                     // [0] best value, [1] worst cancellation factor
    w.out_i = reinterpret_cast<int64_t*>(base + 8);     // [8]
    w.bv = base + 16;
    w.bi = reinterpret_cast<int64_t*>(base + 16 + slots);
    w.bk = base + 16 + 2 * slots;
    w.cs = base + 16 + 3 * slots;
    w.part1 = w.cs + cs_doubles;
    w.part2 = w.part1 + part_doubles;
    double* pk = w.part2 + part_doubles;                // 16-byte aligned records
    w.packed = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(pk) + 15) & ~uintptr_t(15));
    return 0;
}

// the copy of the result record at the end of the workspace (include/obe_hip.h: OBE_WS_RESULT_TAIL), if the
// workspace has the 48 spare bytes behind what the call itself uses
static double* result_tail(void* d_ws, int64_t ws_bytes, int64_t need_bytes) {
    if (!d_ws || ws_bytes < need_bytes + 48) return nullptr;
    return reinterpret_cast<double*>(static_cast<char*>(d_ws) + (ws_bytes & ~(int64_t)7) - 48);
}

// The caller's three result words.  The kernels deliver them only if every one that is asked for is page-locked:
// then each is armed (before any launch) and read() waits for each of them; otherwise read() copies the record.
struct BestWords {
    HostWords best, idx, kappa;
    bool by_kernel;
    BestWords(double* hb, int64_t* hi, double* hk) : best(hb, 1), idx(hi, 1), kappa(hk, 1) {
        by_kernel = !((hb && !best.view<void>()) || (hi && !idx.view<void>()) || (hk && !kappa.view<void>()));
    }
    // what the delivering kernel is given (tail: OBE_WS_RESULT_TAIL, or NULL)
    HostResult arm(double* tail) {
        if (!by_kernel) return HostResult{nullptr, nullptr, nullptr, tail};
        best.arm();
        idx.arm();
        kappa.arm();
        return HostResult{best.view<double>(), idx.view<int64_t>(), kappa.view<double>(), tail};
    }
    int read(const SweepWs& w, hipStream_t st) const {
        if (by_kernel) {       // the kernel writes them: watch every word (none asked for: nothing to wait for)
            if (int rc = idx.wait(st)) return rc;
            if (int rc = kappa.wait(st)) return rc;
            return best.wait(st);
        }
        double tmp[9];
        OBE_HIP_TRY(hipMemcpyAsync(tmp, w.out_v, 9 * sizeof(double), hipMemcpyDeviceToHost, st));
        OBE_HIP_TRY(hipStreamSynchronize(st));
        if (best.host<void>()) *best.host<double>() = tmp[0];
        if (kappa.host<void>()) *kappa.host<double>() = tmp[1];
        if (idx.host<void>()) memcpy(idx.host<void>(), &tmp[8], sizeof(int64_t));
        return 0;
    }
};

// the last launch of obe_utility_argmax / obe_argmax and the delivery of its result
static int fold_best(const SweepWs& w, int nb, const HostResult& hr, const BestWords& out, hipStream_t st) {
    argmax_fold<<<1, kBlock, 0, st>>>(w.bv, w.bi, nb, nullptr, w.out_v, w.out_i, hr);
    OBE_CHECK_LAUNCH("argmax_fold");
    return out.read(w, st);
}

template <class M, bool SHIFT, bool SAFE>
static void launch_sweep_spt(int spt, unsigned grid, const SweepArgs& a, hipStream_t st) {
    switch (spt) {
        case 8: sweep_kernel<M, 8, SHIFT, SAFE><<<grid, kBlock, 0, st>>>(a); break;
        case 4: sweep_kernel<M, 4, SHIFT, SAFE><<<grid, kBlock, 0, st>>>(a); break;
        case 2: sweep_kernel<M, 2, SHIFT, SAFE><<<grid, kBlock, 0, st>>>(a); break;
        default: sweep_kernel<M, 1, SHIFT, SAFE><<<grid, kBlock, 0, st>>>(a); break;
    }
}

// every draw packed once per sweep call
template <class M>
static int launch_pack(const SweepArgs& a, hipStream_t st) {
    sweep_pack_kernel<M><<<stream_blocks(a.nd, kBlock), kBlock, 0, st>>>(a);
    OBE_CHECK_LAUNCH("sweep_pack_kernel");
    return 0;
}

template <class M>
static int launch_sweep(const SweepPlan& p, SweepArgs& a, int flags, hipStream_t st) {
    a.tiles_x = p.tiles_x;
    a.nchunks = p.nchunks;
    a.one = 1;
    a.xcd_map = p.nchunks % 8 == 0;
    const unsigned grid = (unsigned)p.tiles_x * (unsigned)p.nchunks;
    const bool shifted = flags & OBE_SWEEP_SHIFTED;
    bool safe = false;
    if constexpr (has_safe_eval<M>::value) safe = flags & OBE_SWEEP_SAFE;
    if (safe) {
        if constexpr (has_safe_eval<M>::value) {        // always shifted: the careful variant
            launch_sweep_spt<M, true, true>(p.spt, grid, a, st);
        }
    } else if (shifted) {
        launch_sweep_spt<M, true, false>(p.spt, grid, a, st);
    } else {
        launch_sweep_spt<M, false, false>(p.spt, grid, a, st);
    }
    OBE_CHECK_LAUNCH("sweep_kernel");
    return 0;
}

// the cell form of one call: whether it is taken, and where its pieces live in the workspace
struct CellSweep {
    bool on = false;
    CellPlan* plan = nullptr;
    double* coef = nullptr;
    double* part = nullptr;
    unsigned* ran = nullptr;       // cell_eval_kernel's marker
    unsigned seq = 0;              // ... and what this call's launch writes there
    CellChunks chunks{};
};

// OBE_SWEEP_CELLS is honoured where today's unshifted, non-SAFE sweep_kernel<Lorentz<1>> would run
static bool cell_form_selected(const obe_model& m, int flags, int64_t ns, const int64_t* d_draw_idx, int64_t n_draws) {
#ifdef OBE_PLUGIN_MODEL_HEADER
    return false;
#else
    return (flags & OBE_SWEEP_CELLS) && !(flags & (OBE_SWEEP_SHIFTED | OBE_SWEEP_SAFE)) && m.id == OBE_MODEL_LORENTZ
           && m.aux == 1 && !(d_draw_idx && one_workgroup_sweep(ns, n_draws));
#endif
}

// the bin form of one call (it goes before the cell form where both bits are set)
struct BinSweep {
    bool on = false;
#ifndef OBE_PLUGIN_MODEL_HEADER
    BinSweepPtrs q{};
#endif
    unsigned* ran = nullptr;       // bin_eval_kernel's marker
    unsigned seq = 0;
    bool reuse = false;            // OBE_SWEEP_BINS_KEPT honoured: the grouping comes from the caller's keep buffer
    BinUnits units{};
    int64_t items = 0;             // items bin_moments_kernel is launched for: at least as many as any cloud makes
};
// OBE_SWEEP_BINS is honoured where the cell form would be, for clouds whose positions fit an int
static bool bin_form_selected(const obe_model& m, int flags, int64_t ns, const int64_t* d_draw_idx, int64_t n_draws,
                              int64_t nd) {
    return (flags & OBE_SWEEP_BINS) && nd <= ((int64_t)1 << 30)
           && cell_form_selected(m, flags | OBE_SWEEP_CELLS, ns, d_draw_idx, n_draws);
}

#ifndef OBE_PLUGIN_MODEL_HEADER
// once per call: the draws grouped by bin and the bins' folded rows (they depend on the cloud alone)
// (a reuse has the grouping already: bin_scatter_pack_kernel has put the records where it says)
static int launch_bin_plan(const SweepArgs& a, const BinSweep& b, hipStream_t st) {
    using LB = LorentzBins;
    if (!b.reuse) {
        const int mm_blocks = static_cast<int>(std::min<int64_t>(kBinMinmaxBlocks, (a.nd + kBlock - 1) / kBlock));
        bin_minmax_kernel<<<mm_blocks, kBlock, 0, st>>>(a, b.q);
        OBE_CHECK_LAUNCH("bin_minmax_kernel");
        const unsigned group_blocks = (unsigned)((b.units.nunits + kBlock / kWave - 1) / (kBlock / kWave));
        bin_group_kernel<false><<<group_blocks, kBlock, 0, st>>>(a, b.units.per, b.units.nunits, mm_blocks, b.q);
        OBE_CHECK_LAUNCH("bin_group_kernel<count>");
        bin_scan_kernel<<<LB::kMaxBins, kBlock, 0, st>>>(b.units.nunits, b.q, a.abort);
        OBE_CHECK_LAUNCH("bin_scan_kernel");
        bin_group_kernel<true><<<group_blocks, kBlock, 0, st>>>(a, b.units.per, b.units.nunits, mm_blocks, b.q);
        OBE_CHECK_LAUNCH("bin_group_kernel<scatter>");
    }
    bin_moments_kernel<<<(unsigned)b.items, kWave, 0, st>>>(b.q, a.abort);
    OBE_CHECK_LAUNCH("bin_moments_kernel");
    bin_fold_kernel<<<2 * LB::kMaxBins, kBinFoldGroups * kWave, 0, st>>>(b.q, a.abort);
    OBE_CHECK_LAUNCH("bin_fold_kernel");
    return 0;
}
// in place of launch_sweep and sweep_finalize (f.yvar = NULL: of launch_sweep, one chunk of moments in part1 / part2,
// cs_out = 0)
static int launch_bin_sweep(SweepPlan& p, SweepArgs& a, const BinSweep& b, const BinFinish& f, hipStream_t st) {
    p.nchunks = 1;
    const unsigned groups = (unsigned)((a.ns + kWave - 1) / kWave);
    switch (plan_bin_eval_waves(a.ns)) {             // (the shapes of kBinEvalShapes)
        case 8: bin_eval_kernel<1, 8><<<groups, 8 * kWave, 0, st>>>(a, b.q, b.seq, f); break;
        case 6: bin_eval_kernel<2, 6><<<(groups + 1) / 2, 12 * kWave, 0, st>>>(a, b.q, b.seq, f); break;
        case 3: bin_eval_kernel<4, 3><<<(groups + 3) / 4, 12 * kWave, 0, st>>>(a, b.q, b.seq, f); break;
        default: bin_eval_kernel<4, 1><<<(groups + 3) / 4, kBlock, 0, st>>>(a, b.q, b.seq, f);
    }
    OBE_CHECK_LAUNCH("bin_eval_kernel");
    return 0;
}
// a reuse's pack: every draw's record straight to its kept sorted position
static int launch_bin_scatter_pack(const SweepArgs& a, const BinSweep& b, hipStream_t st) {
    bin_scatter_pack_kernel<<<stream_blocks(a.nd, kBlock), kBlock, 0, st>>>(a, b.q);
    OBE_CHECK_LAUNCH("bin_scatter_pack_kernel");
    return 0;
}
#else
static int launch_bin_plan(const SweepArgs&, const BinSweep&, hipStream_t) { return 0; }
static int launch_bin_sweep(SweepPlan&, SweepArgs&, const BinSweep&, const BinFinish&, hipStream_t) { return 0; }
static int launch_bin_scatter_pack(const SweepArgs&, const BinSweep&, hipStream_t) { return 0; }
#endif

#ifndef OBE_PLUGIN_MODEL_HEADER
// once per call, with the pack: the cells of this call's settings
static int launch_cell_plan(const SweepArgs& a, const CellSweep& c, hipStream_t st) {
    cell_plan_kernel<<<1, kCellPlanThreads, 0, st>>>(a, c.plan);
    OBE_CHECK_LAUNCH("cell_plan_kernel");
    return 0;
}
// in place of launch_sweep: one chunk of moments in part1 / part2, cs_out = 0
static int launch_cell_sweep(SweepPlan& p, SweepArgs& a, const CellSweep& c, hipStream_t st) {
    using LC = LorentzCells;
    p.nchunks = 1;
    a.tiles_x = p.tiles_x;
    a.one = 1;
    a.xcd_map = 0;
    a.chunk = c.chunks.chunk;
    a.nchunks = c.chunks.nchunks;          // (of the expansion; sweep_finalize is told p.nchunks = 1)
    cell_moments_kernel<<<(unsigned)c.chunks.nchunks * kCellWaves, kBlock, 0, st>>>(a, c.plan, c.part);
    OBE_CHECK_LAUNCH("cell_moments_kernel");
    cell_fold_kernel<<<LC::kCoefs * kCellWaves, kCellFoldGroups * kWave, 0, st>>>(c.part, c.chunks.nchunks, c.plan, c.coef,
                                                                                 a.abort);
    OBE_CHECK_LAUNCH("cell_fold_kernel");
    cell_eval_kernel<<<(unsigned)((a.ns + kBlock - 1) / kBlock), kBlock, 0, st>>>(a, c.plan, c.coef, c.ran, c.seq);
    OBE_CHECK_LAUNCH("cell_eval_kernel");
    return 0;
}
#else
static int launch_cell_plan(const SweepArgs&, const CellSweep&, hipStream_t) { return 0; }
static int launch_cell_sweep(SweepPlan&, SweepArgs&, const CellSweep&, hipStream_t) { return 0; }
#endif

static int prepare_sweep(const obe_model* m, obe_model& mm, const double* d_settings, int64_t ld_s, int64_t ns,
                         const double* d_particles, int64_t ld_p, int64_t np, const double* d_weights,
                         const int64_t* d_draw_idx, int64_t n_draws, const double* d_moments, void* d_ws,
                         int64_t ws_bytes, SweepPlan& plan, SweepArgs& a, SweepWs& w, int64_t* ws_need = nullptr,
                         int flags = 0, CellSweep* cells = nullptr, BinSweep* bins = nullptr, void* d_keep = nullptr,
                         int64_t keep_bytes = 0) {
    if (!m || !d_settings || !d_particles || !d_moments || ns <= 0 || np <= 0) return bad_arg("sweep: bad pointer/size");
    if (!d_draw_idx && !d_weights) return bad_arg("sweep: full mode needs weights");
    mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    const int64_t nd = d_draw_idx ? n_draws : np;
    if (nd <= 0) return bad_arg("sweep: n_draws must be positive");
    int packed_w = 0, cost = 1;
    if (int rc = dispatch_model(mm, [&](auto M) -> int {
            packed_w = packed_width<decltype(M)>();
            cost = sweep_cost<decltype(M)>::value;
            return 0;
        }))
        return rc;
    plan = plan_sweep(ns, nd, cost, mm.n_channels > 4 ? 2 : 8);
    const int64_t part = (int64_t)plan.nchunks * mm.n_channels * ns;
    const bool bin_form = bins && bin_form_selected(mm, flags, ns, d_draw_idx, n_draws, nd);
    const bool cell_form = !bin_form && cells && cell_form_selected(mm, flags, ns, d_draw_idx, n_draws);
    const int64_t behind_parts = nd * packed_w + (bin_form ? bin_form_doubles(nd) : cell_form ? cell_form_doubles(nd) : 0);
    if (int rc = carve_sweep_ws(d_ws, ws_bytes, part, (int64_t)mm.n_channels * ns, w, argmax_slots(ns), behind_parts))
        return rc;
    if (ws_need) *ws_need = sweep_ws_bytes(part, (int64_t)mm.n_channels * ns, argmax_slots(ns), behind_parts);
    if (cells) {
        cells->on = cell_form;
        if (cell_form) {        // (16-byte aligned behind the packed draws: plan, folded coefficients, chunk partials)
            double* base = w.packed + nd * packed_w;
            base = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(base) + 15) & ~uintptr_t(15));
            cells->plan = reinterpret_cast<CellPlan*>(base);
            cells->ran = reinterpret_cast<unsigned*>(base + 3);
            cells->coef = base + 4;
            cells->part = cells->coef + (int64_t)LorentzCells::kCoefs * LorentzCells::kMaxCells;
            cells->chunks = plan_cell_chunks(nd);
        }
    }
    if (bins) {
        bins->on = bin_form;
#ifndef OBE_PLUGIN_MODEL_HEADER
        if (bin_form) {
            double* base = w.packed + nd * packed_w;
            base = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(base) + 15) & ~uintptr_t(15));
            using BL = BinLayout;
            BinSweepPtrs& q = bins->q;
            q.plan = reinterpret_cast<BinPlan*>(base + BL::kPlan);
            q.ran = bins->ran = reinterpret_cast<unsigned*>(base + BL::kRan);
            q.binstart = reinterpret_cast<int*>(base + BL::kStarts);
            q.itemstart = q.binstart + LorentzBins::kMaxBins + 2;
            q.minmax = base + BL::kMinmax;
            q.totals = reinterpret_cast<int*>(base + BL::kTotals);
            q.counts = reinterpret_cast<int*>(base + BL::kCounts);
            q.coef = base + BL::kCoef;
            q.part = base + BL::kPart;
            q.sorted = base + BL::sorted(nd);
            q.code = reinterpret_cast<int*>(w.packed);        // (no plain packed copy in this form: nd ints of its room)
            bins->units = plan_bin_units(nd);
            bins->items = bin_max_items(nd);
            // a keep buffer of the caller's (full sweeps only: draws are drawn anew for every call), large enough
            // for these draws: the plan and the two tables live there, and OBE_SWEEP_BINS_KEPT is honoured
            if (d_keep && !d_draw_idx && keep_bytes >= BinKeepLayout::bytes(nd)) {
                static std::atomic<unsigned> calls{0};
                int* ints = static_cast<int*>(d_keep);
                q.keep = static_cast<BinKeep*>(d_keep);
                q.plan = &q.keep->plan;
                q.binstart = ints + BinKeepLayout::kStarts;
                q.itemstart = q.binstart + LorentzBins::kMaxBins + 2;
                q.dest = ints + BinKeepLayout::kDest;
                q.code = q.dest;
                q.reuse = bins->reuse = (flags & OBE_SWEEP_BINS_KEPT) != 0;
                q.keep_nd = static_cast<int>(nd);
                memcpy(&q.keep_dbits, &mm.consts[0], sizeof q.keep_dbits);
                q.call = ++calls;
                if (q.call == 0u) q.call = ++calls;
            }
        }
#endif
    }
    a.cs_out = w.cs;
    a.packed = w.packed;
    a.m = mm;
    a.settings = d_settings;
    a.ld_s = ld_s;
    a.ns = ns;
    a.particles = d_particles;
    a.ld_p = ld_p;
    a.weights = d_weights;
    a.draw_idx = d_draw_idx;
    a.nd = nd;
    a.n_particles = np;
    a.uniform_w = 1.0 / (double)nd;
    a.moments = d_moments;
    a.chunk = plan.chunk;
    a.part1 = w.part1;
    a.part2 = w.part2;
    return 0;
}

}  // namespace obe

using namespace obe;

extern "C" {

int obe_sweep_settings_per_lane(int64_t n_settings) {
    return plan_sweep(n_settings < 1 ? 1 : n_settings, (int64_t)1 << 40).spt;      // the most any draw count gets
}

int obe_sweep_cells_plan(double x_min, double x_max, double d, int64_t n_settings, int64_t n_draws) {
    using LC = LorentzCells;
    if (!(d > 0.0 && d <= kDblMax) || !(x_min <= x_max) || !(fabs(x_min) <= kDblMax && fabs(x_max) <= kDblMax)
        || n_settings < 1 || n_draws < 1)
        return 0;
    const double lo = x_min / d, hi = x_max / d;
    if (!(fabs(lo) <= kDblMax && fabs(hi) <= kDblMax)) return 0;
    const double ncells = std::floor((hi - lo) * (1.0 / LC::kWidth)) + 1.0;       // as cell_plan_kernel counts them
    if (!(ncells <= (double)LC::kMaxCells)) return 0;
    // issue slots per particle: every lane of the cells' wavefronts expands it, against one evaluation per setting;
    // and draws enough for the whole chunk grid, without which the expansion kernel does not fill the chip
    const double cell_slots = std::ceil(ncells / kWave) * kWave * kCellSlots;
    const bool worthwhile = (double)n_settings * kDirectSlots >= OBE_CELL_MIN_GAIN * cell_slots && n_draws >= kCellFullGridDraws;
    return worthwhile ? 3 : 1;
}

int obe_sweep_bins_plan(double x_min, double x_max, double d, int64_t n_settings, int64_t n_draws) {
    if (!(d > 0.0 && d <= kDblMax) || !(x_min <= x_max) || !(fabs(x_min) <= kDblMax && fabs(x_max) <= kDblMax)
        || n_settings < 1 || n_draws < 1 || n_draws > ((int64_t)1 << 30))
        return 0;
    // the form it would replace: the cells where their plan takes them, otherwise the direct kernel
    const int cells = obe_sweep_cells_plan(x_min, x_max, d, n_settings, n_draws);
    double replaced = (double)n_settings * (double)n_draws * kDirectSlots;
    if (cells == 3) {
        const double ncells = std::floor((x_max / d - x_min / d) * (1.0 / LorentzCells::kWidth)) + 1.0;
        replaced = (double)n_draws * std::ceil(ncells / kWave) * kWave * kCellSlots;
    }
    // priced at the cap (the occupied bins are a property of the cloud, which changes): every setting meets
    // OBE_BIN_MAX bins, every draw is expanded once, and the launches of the pipeline cost what they cost on a
    // cloud of a few draws
    const double bins = (double)n_settings * OBE_BIN_MAX * kBinEvalSlots + (double)n_draws * kBinDrawSlots + kBinFixedSlots;
    return replaced >= OBE_CELL_MIN_GAIN * bins ? 3 : 1;
}

int obe_sweep_bins_eval_waves(int64_t n_settings) { return plan_bin_eval_waves(n_settings < 1 ? 1 : n_settings); }

int obe_sweep_settings_per_lane_for(int64_t n_settings, int64_t n_draws) {
    if (n_settings < 1) n_settings = 1;
    if (n_draws < 1) return obe_sweep_settings_per_lane(n_settings);
    if (one_workgroup_sweep(n_settings, n_draws)) return 1;
    return plan_sweep(n_settings, n_draws).spt;
}

int64_t obe_workspace_bytes(int64_t n_particles, int64_t n_settings, int32_t n_channels, int32_t n_dims) {
    if (n_particles < 1) n_particles = 1;
    if (n_settings < 1) n_settings = 1;
    if (n_channels < 1) n_channels = 1;
    if (n_dims < 1) n_dims = 1;
#ifdef OBE_PLUGIN_MODEL_HEADER
    const int packed_w = kMaxPackedWidth;
#else
    const int packed_w = max_packed_width(n_dims);
#endif
    // the largest of what each consumer checks against, plus room for the tails (OBE_WS_RESULT_TAIL, OBE_WS_ABORT_WORD)
    int64_t b = sweep_ws_bytes_bound(n_settings, n_particles, n_channels, packed_w);
    b = std::max(b, moments_ws_bytes(n_dims));
    b = std::max(b, update_ws_bytes(n_dims));          // (with the fused first moments; without them it is less)
    b = std::max(b, scan_ws_bytes(n_particles));
    b = std::max(b, resample_wide_ws_bytes(n_dims));
    return b + 64 * (int64_t)sizeof(double);
}

int64_t obe_sweep_bins_keep_bytes(int64_t n_draws) { return BinKeepLayout::bytes(n_draws < 1 ? 1 : n_draws); }

// obe_sweep_utility (d_keep = NULL) and obe_sweep_utility_keep
static int sweep_utility(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                         const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                         const int64_t* d_draw_idx, int64_t n_draws, const double* d_moments, int32_t shifted,
                         const double* d_noise_var, int64_t noise_ld, const double* d_cost, double cost_scalar,
                         double* d_yvar, double* d_utility, double* h_best, int64_t* h_best_idx, double* h_kappa,
                         void* d_ws, int64_t ws_bytes, void* stream, void* d_keep, int64_t keep_bytes) {
    if (!d_noise_var || !d_yvar || !d_utility) return bad_arg("obe_sweep_utility: bad output/noise pointer");
    if (d_keep && reinterpret_cast<uintptr_t>(d_keep) % 16) return bad_arg("obe_sweep_utility_keep: d_keep is not 16-byte aligned");
    obe_model mm;
    SweepPlan plan;
    SweepArgs a{};
    SweepWs w;
    int64_t sweep_ws_need = 0;
    CellSweep cells;
    BinSweep bins;
    if (int rc = prepare_sweep(m, mm, d_settings, ld_s, n_settings, d_particles, ld_p, n_particles, d_weights,
                               d_draw_idx, n_draws, d_moments, d_ws, ws_bytes, plan, a, w, &sweep_ws_need, shifted, &cells,
                               &bins, d_keep, keep_bytes))
        return rc;
    hipStream_t st = as_stream(stream);
    UtilArgs ua;
    if (int rc = make_util_args(ua, d_noise_var, noise_ld, d_cost, cost_scalar, mm.n_channels, mm.n_params)) return rc;
    const bool speculative = shifted & OBE_SWEEP_SPECULATIVE;
    const bool nowait = speculative || (shifted & OBE_SWEEP_NOWAIT);
    if (nowait) {
        if (d_draw_idx) return bad_arg("obe_sweep_utility: OBE_SWEEP_SPECULATIVE / OBE_SWEEP_NOWAIT are for full sweeps");
        if (speculative) {
            if (ws_bytes < sweep_ws_need + 16)
                return bad_arg("obe_sweep_utility: OBE_SWEEP_SPECULATIVE needs 16 spare bytes at the end of the workspace (OBE_WS_ABORT_WORD)");
            a.abort = ws_abort_word(d_ws, ws_bytes);
        }
    }
    BestWords out(h_best, h_best_idx, h_kappa);
    if (nowait && !out.by_kernel)
        return bad_arg("obe_sweep_utility: OBE_SWEEP_SPECULATIVE / OBE_SWEEP_NOWAIT need page-locked host outputs");
    const HostResult hr = out.arm(result_tail(d_ws, ws_bytes, sweep_ws_need));
    if (d_draw_idx && one_workgroup_sweep(n_settings, n_draws)) {
        int rc = dispatch_model(mm, [&](auto M) -> int {
            using Model = decltype(M);
            const size_t lds = (size_t)n_draws * packed_width<Model>() * sizeof(double);
            bool safe = false;
            if constexpr (has_safe_eval<Model>::value) safe = shifted & OBE_SWEEP_SAFE;
            if (safe) {
                if constexpr (has_safe_eval<Model>::value)
                    sweep_small_kernel<Model, true><<<1, kBlock, lds, st>>>(a, ua, d_yvar, d_utility, w.out_v, w.out_i, hr);
            } else {
                sweep_small_kernel<Model, false><<<1, kBlock, lds, st>>>(a, ua, d_yvar, d_utility, w.out_v, w.out_i, hr);
            }
            OBE_CHECK_LAUNCH("sweep_small_kernel");
            return 0;
        });
        if (rc) return rc;
        return out.read(w, st);
    }
    // (a call without host outputs — a sharded rank reads the record itself — is timed too: it waits for the
    // sweep kernel's end event instead of for the result)
    const bool timed = g_timing.on;
    if (timed) {
        resolve_pending_timing();
        int dev = 0;
        OBE_HIP_TRY(hipGetDevice(&dev));
        if (g_timing.device != dev) {
            if (g_timing.e0) (void)hipEventDestroy(g_timing.e0);
            if (g_timing.e1) (void)hipEventDestroy(g_timing.e1);
            OBE_HIP_TRY(hipEventCreate(&g_timing.e0));
            OBE_HIP_TRY(hipEventCreate(&g_timing.e1));
            g_timing.device = dev;
        }
    }
    int nb = static_cast<int>((n_settings + kFinSettings - 1) / kFinSettings);
    if (nb > kFinMaxBlocks) return bad_arg("obe_sweep_utility: more than 4 194 304 settings per call");
    const BinFinish fin{ua, d_draw_idx == nullptr, d_yvar, d_utility, w.bv, w.bi, w.bk};
    int rc = dispatch_model(mm, [&](auto M) -> int {
        // (the bin form has no plain packed copy: a rebuild of the grouping packs every draw straight to its sorted
        // position, and so does a reuse of a kept one, here)
        if (int e = !bins.on ? launch_pack<decltype(M)>(a, st) : bins.reuse ? launch_bin_scatter_pack(a, bins, st) : 0) return e;
        if (cells.on || bins.on) {
            const unsigned seq = timed && nowait ? (++g_timing.seq ? g_timing.seq : ++g_timing.seq) : 0u;      // (never 0)
            cells.seq = bins.seq = seq;
            if (cells.on)
                if (int e = launch_cell_plan(a, cells, st)) return e;
        }
        if (timed) (void)hipEventRecord(g_timing.e0, st);
        // (the bins are a function of the cloud: grouping it is part of the sweep, and of its time)
        if (bins.on)
            if (int e = launch_bin_plan(a, bins, st)) return e;
        const int e = bins.on    ? launch_bin_sweep(plan, a, bins, fin, st)
                      : cells.on ? launch_cell_sweep(plan, a, cells, st)
                                 : launch_sweep<decltype(M)>(plan, a, shifted, st);
        if (timed) (void)hipEventRecord(g_timing.e1, st);
        return e;
    });
    if (rc) return rc;
    // (FG chunk groups x WS settings per workgroup: see sweep_finalize)
    auto finalize = [&](auto FG, auto WS) {
        sweep_finalize<decltype(FG)::value, decltype(WS)::value><<<nb, decltype(FG)::value * decltype(WS)::value, 0, st>>>(
            w.part1, w.part2, plan.nchunks, mm.n_channels, n_settings, d_moments, d_draw_idx == nullptr, ua, w.cs,
            d_yvar, d_utility, w.bv, w.bi, w.bk, a.abort);
    };
    using std::integral_constant;
    if (bins.on) {
        // (bin_eval_kernel has finished its own settings: the nb partials are there)
    } else if (plan.nchunks >= kFinManyChunks && nb < kFinNarrowBelow) {
        nb = static_cast<int>((n_settings + kFinNarrow - 1) / kFinNarrow);       // (< 512: within the argmax slots)
        finalize(integral_constant<int, kFinGroupsMany>{}, integral_constant<int, kFinNarrow>{});
    } else if (plan.nchunks >= kFinManyChunks)
        finalize(integral_constant<int, kFinGroupsMany>{}, integral_constant<int, kFinSettings>{});
    else
        finalize(integral_constant<int, kFinGroupsFew>{}, integral_constant<int, kFinSettings>{});
    OBE_CHECK_LAUNCH("sweep_finalize");
    argmax_fold<<<1, kBlock, 0, st>>>(w.bv, w.bi, nb, w.bk, w.out_v, w.out_i, hr, a.abort);
    OBE_CHECK_LAUNCH("argmax_fold");
    if (nowait) {               // nobody waits here: the caller watches the armed words when it wants the result
        if (timed) {
            g_timing.pending = true;
            g_timing.pending_min_ms = 0.5 * (double)n_settings * (double)n_particles / 8e9;
            g_timing.pending_ran = bins.on ? bins.ran : cells.on ? cells.ran : nullptr;
            g_timing.pending_seq = cells.seq;
        }
        return 0;
    }
    rc = out.read(w, st);
    if (timed && !rc && !(h_best || h_best_idx || h_kappa)) rc = (int)hipEventSynchronize(g_timing.e1);
    if (timed && !rc) count_timed_sweep();    // the stream is drained: both events have completed
    return rc;
}

int obe_sweep_utility(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                      const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                      const int64_t* d_draw_idx, int64_t n_draws, const double* d_moments, int32_t shifted,
                      const double* d_noise_var, int64_t noise_ld, const double* d_cost, double cost_scalar,
                      double* d_yvar, double* d_utility, double* h_best, int64_t* h_best_idx, double* h_kappa,
                      void* d_ws, int64_t ws_bytes, void* stream) {
    return sweep_utility(m, d_settings, ld_s, n_settings, d_particles, ld_p, n_particles, d_weights, d_draw_idx, n_draws,
                         d_moments, shifted, d_noise_var, noise_ld, d_cost, cost_scalar, d_yvar, d_utility, h_best,
                         h_best_idx, h_kappa, d_ws, ws_bytes, stream, nullptr, 0);
}

int obe_sweep_utility_keep(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                           const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                           const int64_t* d_draw_idx, int64_t n_draws, const double* d_moments, int32_t shifted,
                           const double* d_noise_var, int64_t noise_ld, const double* d_cost, double cost_scalar,
                           double* d_yvar, double* d_utility, double* h_value, int64_t* h_index, double* h_factor,
                           void* d_ws, int64_t ws_bytes, void* stream, void* d_keep, int64_t keep_bytes) {
    return sweep_utility(m, d_settings, ld_s, n_settings, d_particles, ld_p, n_particles, d_weights, d_draw_idx, n_draws,
                         d_moments, shifted, d_noise_var, noise_ld, d_cost, cost_scalar, d_yvar, d_utility, h_value,
                         h_index, h_factor, d_ws, ws_bytes, stream, d_keep, keep_bytes);
}

int obe_sweep_timing(int32_t enable, double* h_total_ms, int64_t* h_launches) {
    resolve_pending_timing();
    if (h_total_ms) *h_total_ms = g_timing.total_ms;
    if (h_launches) *h_launches = g_timing.launches;
    if (enable >= 0) {
        g_timing.on = enable != 0;
        g_timing.total_ms = 0.0;
        g_timing.launches = 0;
    }
    return 0;
}

int obe_sweep_kernel_time(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                          const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                          const double* d_moments, int32_t shifted, void* d_ws, int64_t ws_bytes, int32_t iters,
                          float* h_ms_avg, void* stream) {
    if (!h_ms_avg || iters == 0) return bad_arg("obe_sweep_kernel_time: bad arguments");
    obe_model mm;
    SweepPlan plan;
    SweepArgs a{};
    SweepWs w;
    CellSweep cells;
    BinSweep bins;
    if (int rc = prepare_sweep(m, mm, d_settings, ld_s, n_settings, d_particles, ld_p, n_particles, d_weights,
                               nullptr, 0, d_moments, d_ws, ws_bytes, plan, a, w, nullptr, shifted, &cells, &bins))
        return rc;
    hipStream_t st = as_stream(stream);
    hipEvent_t e0, e1;
    OBE_HIP_TRY(hipEventCreate(&e0));
    OBE_HIP_TRY(hipEventCreate(&e1));
    auto sweep_once = [&]() -> int {
        // (the bins are a function of the cloud, and a new cloud means a new sweep: the whole pipeline is the sweep —
        // the rebuild's, whatever a caller of obe_sweep_utility_keep may have kept)
        if (bins.on) {
            if (int e = launch_bin_plan(a, bins, st)) return e;
            return launch_bin_sweep(plan, a, bins, BinFinish{}, st);
        }
        if (cells.on) return launch_cell_sweep(plan, a, cells, st);
        return dispatch_model(mm, [&](auto M) -> int { return launch_sweep<decltype(M)>(plan, a, shifted, st); });
    };
    int rc = bins.on ? 0 : dispatch_model(mm, [&](auto M) -> int { return launch_pack<decltype(M)>(a, st); });
    if (!rc && cells.on) rc = launch_cell_plan(a, cells, st);
    if (rc) {
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        return rc;
    }
    if (iters < 0) {
        // isolated launches, as a measurement cycle issues them: the stream is drained before each
        // one, so neither the previous launch's tail nor its clocks carry over
        double total = 0.0;
        for (int i = 0; i < -iters && !rc; ++i) {
            hipError_t e = hipStreamSynchronize(st);
            (void)hipEventRecord(e0, st);
            rc = sweep_once();
            (void)hipEventRecord(e1, st);
            if (e == hipSuccess) e = hipEventSynchronize(e1);
            float ms = 0.f;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
            if (e != hipSuccess && !rc) rc = fail(e, "sweep timing");
            total += ms;
        }
        *h_ms_avg = (float)(total / (double)(-iters));
    } else {
        rc = sweep_once();   // warm
        if (!rc) {
            (void)hipEventRecord(e0, st);
            for (int i = 0; i < iters && !rc; ++i)
                rc = sweep_once();
            (void)hipEventRecord(e1, st);
            hipError_t e = hipEventSynchronize(e1);
            float ms = 0.f;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
            if (e != hipSuccess) rc = fail(e, "sweep timing");
            *h_ms_avg = ms / (float)iters;
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

int obe_yspace_variance(const double* d_yspace, int64_t n_draws, int32_t n_channels, int64_t n_settings,
                        double* d_yvar, void* stream) {
    if (!d_yspace || !d_yvar || n_draws <= 0 || n_channels < 1 || n_settings <= 0)
        return bad_arg("obe_yspace_variance: bad pointer/size");
    const int64_t row = (int64_t)n_channels * n_settings;
    yspace_var_kernel<<<stream_blocks(row, kBlock), kBlock, 0, as_stream(stream)>>>(d_yspace, n_draws, row, d_yvar);
    OBE_CHECK_LAUNCH("yspace_var_kernel");
    return 0;
}

int obe_utility_argmax(const double* d_yvar, int32_t n_channels, int64_t n_settings, const double* d_noise_var,
                       int64_t noise_ld, const double* d_cost, double cost_scalar, double* d_utility,
                       double* h_best, int64_t* h_best_idx, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_yvar || !d_noise_var || !d_utility || n_settings <= 0 || n_channels < 1)
        return bad_arg("obe_utility_argmax: bad pointer/size");
    SweepWs w;
    if (int rc = carve_sweep_ws(d_ws, ws_bytes, 0, 0, w)) return rc;
    hipStream_t st = as_stream(stream);
    if (noise_ld < 0) return bad_arg("obe_utility_argmax: noise_ld < 0 (noise variance from a K3 block) is for obe_sweep_utility");
    UtilArgs ua;
    if (int rc = make_util_args(ua, d_noise_var, noise_ld, d_cost, cost_scalar, 0, 0)) return rc;
    const int nb = stream_blocks(n_settings, kBlock);
    BestWords out(h_best, h_best_idx, nullptr);
    const HostResult hr = out.arm(result_tail(d_ws, ws_bytes, sweep_ws_bytes(0, 0, kMaxBlocks, 0)));
    utility_kernel<<<nb, kBlock, 0, st>>>(d_yvar, n_channels, n_settings, ua, d_utility, w.bv, w.bi);
    OBE_CHECK_LAUNCH("utility_kernel");
    return fold_best(w, nb, hr, out, st);
}

int obe_argmax(const double* d_v, int64_t n, double* h_best, int64_t* h_best_idx, void* d_ws, int64_t ws_bytes,
               void* stream) {
    if (!d_v || n <= 0) return bad_arg("obe_argmax: bad pointer/size");
    SweepWs w;
    if (int rc = carve_sweep_ws(d_ws, ws_bytes, 0, 0, w)) return rc;
    hipStream_t st = as_stream(stream);
    const int nb = stream_blocks(n, kBlock);
    BestWords out(h_best, h_best_idx, nullptr);
    const HostResult hr = out.arm(result_tail(d_ws, ws_bytes, sweep_ws_bytes(0, 0, kMaxBlocks, 0)));
    argmax_kernel<<<nb, kBlock, 0, st>>>(d_v, n, w.bv, w.bi);
    OBE_CHECK_LAUNCH("argmax_kernel");
    return fold_best(w, nb, hr, out, st);
}

}  // extern "C"
