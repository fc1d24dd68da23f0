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
// This file: the plan, the pack, the direct kernels, the workspace, the timing and the entry points.  What every form
// shares is in obe_sweep_common.h; the two expansion forms of the one-peak Lorentzian (kernels and host half) are in
// obe_sweep_cells.h and obe_sweep_bins.h.
//
// Variance numerics: moments are accumulated about a per-setting shift
// c_s = model(x_s; mean parameters), so  var = (S2 - S1^2/W)/W  does not cancel
// catastrophically (np.var is two-pass; the shift plays the role of its first pass).
#include <cstdlib>

#include "obe_update.h"
#include "obe_sweep_common.h"
#include "obe_sweep_cells.h"
#include "obe_sweep_bins.h"

namespace obe {

constexpr int kMaxChunks = 1024;
constexpr int kFinMaxBlocks = 65536;     // finalize workgroups (64 settings each) the argmax partials hold

static int64_t argmax_slots(int64_t n_settings) {
    return std::max<int64_t>(kMaxBlocks, (n_settings + kFinSettings - 1) / kFinSettings);
}

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
    const unsigned* pending_ran = nullptr;     // a speculative cell or bin sweep: the marker its last kernel writes if it runs ...
    unsigned pending_seq = 0, seq = 0;         // ... and the value to find there
    unsigned* met_abort = nullptr;             // page-locked: the abort word as a speculative direct sweep met it
    bool pending_met_abort = false;
};
static SweepTiming g_timing;

// the time between the pair of events (both completed) joins the totals
static void count_timed_sweep() {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_timing.e0, g_timing.e1) != hipSuccess) return;
    g_timing.total_ms += ms;
    g_timing.launches += 1;
}

// A speculative call returns before its kernels have run: its pair of events is read at the next timed call
// or query.  An aborted sweep (its update resampled) is not a sweep, and the clock does not tell: the span of
// launches that return at once is mostly the host's, and now and then as long as a small sweep.  An expansion
// form's last kernel leaves a marker if it runs; the direct form's abort word is copied ahead of the sweep, on
// its stream, before a later update can write it again.
static void resolve_pending_timing() {
    if (!g_timing.pending) return;
    g_timing.pending = false;
    if (hipEventSynchronize(g_timing.e1) != hipSuccess) return;
    if (g_timing.pending_ran) {
        unsigned ran = 0;
        const bool read = hipMemcpy(&ran, g_timing.pending_ran, sizeof ran, hipMemcpyDeviceToHost) == hipSuccess;
        if (read && ran == g_timing.pending_seq) count_timed_sweep();
        return;
    }
    if (!g_timing.pending_met_abort || *static_cast<volatile unsigned*>(g_timing.met_abort) == 0u) count_timed_sweep();
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

// what a sweep call was given (obe_sweep_utility_keep; obe_sweep_kernel_time: full mode, no keep buffer)
struct SweepInputs {
    const obe_model* m;
    const double* d_settings;
    int64_t ld_s, ns;
    const double* d_particles;
    int64_t ld_p, np;
    const double* d_weights;
    const int64_t* d_draw_idx;
    int64_t n_draws;
    const double* d_moments;
    int flags;
    void* d_ws;
    int64_t ws_bytes;
    void* d_keep;
    int64_t keep_bytes;
};

// The one place where a library built for ONE generated model differs: the packed width is that model's, and its sweep
// has the direct form alone.  The library has the one-peak Lorentzian, whose unshifted sweep may take an expansion
// form: the bins before the cells where both are asked for.
#ifdef OBE_PLUGIN_MODEL_HEADER
static int max_packed_width(int) { return packed_width<PluginModel>(); }
struct SweepForms { static constexpr bool kAny = false; };
#else
// every registry model: Lorentz<K> K + 2 <= n_dims, lines <= 2, Rabi 3, Coil 7
static int max_packed_width(int n_dims) { return std::max(8, (n_dims + 2) & ~1); }
struct SweepForms {
    static constexpr bool kAny = true;
    // a form's room lies behind the packed draws from a 16-byte aligned base: what the alignment may cost
    static constexpr int64_t kSlack = 2;
    BinForm bins;
    CellForm cells;
    // the most a form keeps behind the packed draws in any sweep of AT MOST nd draws
    static int64_t doubles_bound(int64_t nd) { return kSlack + std::max(CellLayout::doubles(nd), BinLayout::doubles(nd)); }
    // which form this call takes, and what it keeps behind the packed draws (0: the direct form)
    int64_t select(const obe_model& m, const SweepInputs& in, int64_t nd) {
        bins.on = BinForm::selected(m, in.flags, in.ns, in.d_draw_idx, in.n_draws, nd);
        cells.on = !bins.on && CellForm::selected(m, in.flags, in.ns, in.d_draw_idx, in.n_draws);
        return bins.on ? kSlack + BinLayout::doubles(nd) : cells.on ? kSlack + CellLayout::doubles(nd) : 0;
    }
    void carve(double* packed_end, double* packed, const obe_model& m, const SweepInputs& in, int64_t nd) {
        double* base = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(packed_end) + 15) & ~uintptr_t(15));
        if (bins.on) bins.carve(base, packed, nd, m, in.flags, in.d_draw_idx, in.d_keep, in.keep_bytes);
        else if (cells.on) cells.carve(base);
    }
    // the marker the form's last kernel writes (NULL: the direct form)
    const unsigned* ran() const { return bins.on ? bins.q.ran : cells.on ? cells.ran : nullptr; }
};
#endif

// the bytes of the workspace a sweep uses, and those of any sweep of ns settings, nc channels and AT MOST nd draws
// (obe_workspace_bytes)
static int64_t sweep_ws_bytes(int64_t part_doubles, int64_t cs_doubles, int64_t slots, int64_t packed_doubles) {
    return (2 * part_doubles + cs_doubles + 3 * slots + 16 + packed_doubles + 2) * (int64_t)sizeof(double);
}
template <class F = SweepForms>
static int64_t sweep_ws_bytes_bound(int64_t ns, int64_t nd, int nc, int packed_w) {
    const SweepPlan p = plan_sweep(ns, nd, 1 << 20);       // (the grid of the costliest model: the most chunks)
    int64_t behind_parts = nd * packed_w;
    if constexpr (F::kAny) behind_parts += F::doubles_bound(nd);
    // (sized by the monotone bound: the chunk count itself is not monotone in nd after the rounding
    // of the chunk length, and a sweep of N_DRAWS < n_particles draws runs in the same workspace)
    return sweep_ws_bytes((int64_t)p.nchunks_bound * nc * ns, (int64_t)nc * ns, argmax_slots(ns), behind_parts);
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

// one sweep call on the host: its plan, its kernel arguments, its workspace and the form it takes
struct SweepCall {
    obe_model mm;
    SweepPlan plan;
    SweepArgs a{};
    SweepWs w;
    int64_t ws_need = 0;           // the bytes of the workspace the call uses
    SweepForms forms;
    bool finishes_itself = false;  // the bin form, given a BinFinish: yvar, utility and the argmax partials are the sweep's
    // how obe_sweep_timing tells a speculative expansion sweep that ran from one whose launches returned at once (their
    // durations are too close to tell by the clock): the form's last kernel writes `seq` to `ran` (NULL: the direct form)
    const unsigned* ran = nullptr;
    unsigned seq = 0;
};

// (templates over the call, so that what names a form is compiled only where there are forms: SweepForms::kAny)
template <class C>
static int prepare_sweep(const SweepInputs& in, C& c) {
    using F = decltype(c.forms);
    if (!in.m || !in.d_settings || !in.d_particles || !in.d_moments || in.ns <= 0 || in.np <= 0)
        return bad_arg("sweep: bad pointer/size");
    if (!in.d_draw_idx && !in.d_weights) return bad_arg("sweep: full mode needs weights");
    obe_model& mm = c.mm;
    mm = *in.m;
    if (int rc = obe_model_validate(&mm)) return rc;
    const int64_t ns = in.ns, nd = in.d_draw_idx ? in.n_draws : in.np;
    if (nd <= 0) return bad_arg("sweep: n_draws must be positive");
    int packed_w = 0, cost = 1;
    if (int rc = dispatch_model(mm, [&](auto M) -> int {
            packed_w = packed_width<decltype(M)>();
            cost = sweep_cost<decltype(M)>::value;
            return 0;
        }))
        return rc;
    c.plan = plan_sweep(ns, nd, cost, mm.n_channels > 4 ? 2 : 8);
    const int64_t part = (int64_t)c.plan.nchunks * mm.n_channels * ns, cs = (int64_t)mm.n_channels * ns;
    int64_t behind_parts = nd * packed_w;
    if constexpr (F::kAny) behind_parts += c.forms.select(mm, in, nd);
    if (int rc = carve_sweep_ws(in.d_ws, in.ws_bytes, part, cs, c.w, argmax_slots(ns), behind_parts)) return rc;
    c.ws_need = sweep_ws_bytes(part, cs, argmax_slots(ns), behind_parts);
    if constexpr (F::kAny) {
        c.forms.carve(c.w.packed + nd * packed_w, c.w.packed, mm, in, nd);
        c.ran = c.forms.ran();
        c.finishes_itself = c.forms.bins.on;
    }
    SweepArgs& a = c.a;
    a.cs_out = c.w.cs;
    a.packed = c.w.packed;
    a.m = mm;
    a.settings = in.d_settings;
    a.ld_s = in.ld_s;
    a.ns = ns;
    a.particles = in.d_particles;
    a.ld_p = in.ld_p;
    a.weights = in.d_weights;
    a.draw_idx = in.d_draw_idx;
    a.nd = nd;
    a.n_particles = in.np;
    a.uniform_w = 1.0 / (double)nd;
    a.moments = in.d_moments;
    a.chunk = c.plan.chunk;
    a.part1 = c.w.part1;
    a.part2 = c.w.part2;
    return 0;
}

// The launches of a call, for whichever form is on.  Before the sweep, once per call: every draw packed, or what the
// form has in its place, and what it derives from the settings.
template <class M, class C>
static int before_sweep(const C& c, hipStream_t st) {
    if constexpr (decltype(c.forms)::kAny) {
        if (c.forms.bins.on) return c.forms.bins.before(c.a, st);       // (the bin form has no plain packed copy)
        if (int e = launch_pack<M>(c.a, st)) return e;
        return c.forms.cells.on ? c.forms.cells.before(c.a, st) : 0;
    } else
        return launch_pack<M>(c.a, st);
}
// The sweep: what obe_sweep_timing and obe_sweep_kernel_time time.  It leaves the chunk moments in part1 / part2 and the
// shifts in cs; a form that finishes itself (c.finishes_itself) does so where fin.yvar is given.
template <class M, class C>
static int run_sweep(C& c, int flags, const BinFinish& fin, hipStream_t st) {
    if constexpr (decltype(c.forms)::kAny) {
        if (c.forms.bins.on) return c.forms.bins.sweep(c.plan, c.a, c.seq, fin, st);
        if (c.forms.cells.on) return c.forms.cells.sweep(c.plan, c.a, c.seq, st);
    }
    return launch_sweep<M>(c.plan, c.a, flags, st);
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
    const int packed_w = max_packed_width(n_dims);
    // the largest of what each consumer checks against, plus room for the tails (OBE_WS_RESULT_TAIL, OBE_WS_ABORT_WORD)
    int64_t b = sweep_ws_bytes_bound(n_settings, n_particles, n_channels, packed_w);
    b = std::max(b, moments_ws_bytes(n_dims));
    b = std::max(b, update_ws_bytes(n_dims));          // (with the fused first moments; without them it is less)
    b = std::max(b, scan_ws_bytes(n_particles));
    b = std::max(b, resample_wide_ws_bytes(n_dims));
    return b + 64 * (int64_t)sizeof(double);
}

int64_t obe_sweep_bins_keep_bytes(int64_t n_draws) { return BinKeepLayout::bytes(n_draws < 1 ? 1 : n_draws); }
int64_t obe_sweep_bins_keep_records_bytes(int64_t n_draws) {
    return BinKeepLayout::records_bytes(n_draws < 1 ? 1 : n_draws);
}

int obe_sweep_utility(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                      const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                      const int64_t* d_draw_idx, int64_t n_draws, const double* d_moments, int32_t shifted,
                      const double* d_noise_var, int64_t noise_ld, const double* d_cost, double cost_scalar,
                      double* d_yvar, double* d_utility, double* h_best, int64_t* h_best_idx, double* h_kappa,
                      void* d_ws, int64_t ws_bytes, void* stream) {
    return obe_sweep_utility_keep(m, d_settings, ld_s, n_settings, d_particles, ld_p, n_particles, d_weights, d_draw_idx,
                                  n_draws, d_moments, shifted, d_noise_var, noise_ld, d_cost, cost_scalar, d_yvar, d_utility,
                                  h_best, h_best_idx, h_kappa, d_ws, ws_bytes, stream, nullptr, 0);
}

// (the error texts name obe_sweep_utility, with or without a keep buffer)
int obe_sweep_utility_keep(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                           const double* d_particles, int64_t ld_p, int64_t n_particles, const double* d_weights,
                           const int64_t* d_draw_idx, int64_t n_draws, const double* d_moments, int32_t shifted,
                           const double* d_noise_var, int64_t noise_ld, const double* d_cost, double cost_scalar,
                           double* d_yvar, double* d_utility, double* h_best, int64_t* h_best_idx, double* h_kappa,
                           void* d_ws, int64_t ws_bytes, void* stream, void* d_keep, int64_t keep_bytes) {
    if (!d_noise_var || !d_yvar || !d_utility) return bad_arg("obe_sweep_utility: bad output/noise pointer");
    if (d_keep && reinterpret_cast<uintptr_t>(d_keep) % 16) return bad_arg("obe_sweep_utility_keep: d_keep is not 16-byte aligned");
    SweepCall c;
    if (int rc = prepare_sweep(SweepInputs{m, d_settings, ld_s, n_settings, d_particles, ld_p, n_particles, d_weights,
                                           d_draw_idx, n_draws, d_moments, shifted, d_ws, ws_bytes, d_keep, keep_bytes}, c))
        return rc;
    const obe_model& mm = c.mm;
    SweepPlan& plan = c.plan;
    SweepArgs& a = c.a;
    const SweepWs& w = c.w;
    hipStream_t st = as_stream(stream);
    UtilArgs ua;
    if (int rc = make_util_args(ua, d_noise_var, noise_ld, d_cost, cost_scalar, mm.n_channels, mm.n_params)) return rc;
    const bool speculative = shifted & OBE_SWEEP_SPECULATIVE;
    const bool nowait = speculative || (shifted & OBE_SWEEP_NOWAIT);
    if (nowait) {
        if (d_draw_idx) return bad_arg("obe_sweep_utility: OBE_SWEEP_SPECULATIVE / OBE_SWEEP_NOWAIT are for full sweeps");
        if (speculative) {
            if (ws_bytes < c.ws_need + 16)
                return bad_arg("obe_sweep_utility: OBE_SWEEP_SPECULATIVE needs 16 spare bytes at the end of the workspace (OBE_WS_ABORT_WORD)");
            a.abort = ws_abort_word(d_ws, ws_bytes);
        }
    }
    BestWords out(h_best, h_best_idx, h_kappa);
    if (nowait && !out.by_kernel)
        return bad_arg("obe_sweep_utility: OBE_SWEEP_SPECULATIVE / OBE_SWEEP_NOWAIT need page-locked host outputs");
    const HostResult hr = out.arm(result_tail(d_ws, ws_bytes, c.ws_need));
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
            if (!g_timing.met_abort) OBE_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&g_timing.met_abort), sizeof(unsigned)));
            g_timing.device = dev;
        }
    }
    int nb = static_cast<int>((n_settings + kFinSettings - 1) / kFinSettings);
    if (nb > kFinMaxBlocks) return bad_arg("obe_sweep_utility: more than 4 194 304 settings per call");
    const BinFinish fin{ua, d_draw_idx == nullptr, d_yvar, d_utility, w.bv, w.bi, w.bk};
    if (c.ran && timed && nowait) c.seq = ++g_timing.seq ? g_timing.seq : ++g_timing.seq;      // (never 0)
    const bool copy_abort = timed && a.abort && !c.ran;        // (resolve_pending_timing)
    int rc = dispatch_model(mm, [&](auto M) -> int {
        if (int e = before_sweep<decltype(M)>(c, st)) return e;
        if (copy_abort) OBE_HIP_TRY(hipMemcpyAsync(g_timing.met_abort, a.abort, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        if (timed) (void)hipEventRecord(g_timing.e0, st);
        const int e = run_sweep<decltype(M)>(c, shifted, fin, st);
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
    if (c.finishes_itself) {
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
            g_timing.pending_met_abort = copy_abort;
            g_timing.pending_ran = c.ran;
            g_timing.pending_seq = c.seq;
        }
        return 0;
    }
    rc = out.read(w, st);
    if (timed && !rc && !(h_best || h_best_idx || h_kappa)) rc = (int)hipEventSynchronize(g_timing.e1);
    if (timed && !rc) count_timed_sweep();    // the stream is drained: both events have completed
    return rc;
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
    // (full mode and no keep buffer.  The bins are a function of the cloud, and a new cloud means a new sweep: the whole
    // pipeline is the sweep — the rebuild's, whatever a caller of obe_sweep_utility_keep may have kept)
    SweepCall c;
    if (int rc = prepare_sweep(SweepInputs{m, d_settings, ld_s, n_settings, d_particles, ld_p, n_particles, d_weights,
                                           nullptr, 0, d_moments, shifted, d_ws, ws_bytes, nullptr, 0}, c))
        return rc;
    hipStream_t st = as_stream(stream);
    hipEvent_t e0, e1;
    OBE_HIP_TRY(hipEventCreate(&e0));
    OBE_HIP_TRY(hipEventCreate(&e1));
    // (BinFinish{}: the sweep alone — a form that could finish its settings ends with part1 / part2 instead)
    auto sweep_once = [&]() -> int {
        return dispatch_model(c.mm, [&](auto M) -> int { return run_sweep<decltype(M)>(c, shifted, BinFinish{}, st); });
    };
    int rc = dispatch_model(c.mm, [&](auto M) -> int { return before_sweep<decltype(M)>(c, st); });
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
