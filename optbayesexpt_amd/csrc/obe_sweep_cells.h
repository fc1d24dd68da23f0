// The cell form of the utility sweep (OBE_SWEEP_CELLS): its constants and workspace layout, its kernels, and CellForm,
// the host half of one call.  The first part is plain host code and serves every build (obe_sweep_cells_plan answers
// from it whatever the model); the kernels and CellForm exist where the library has the one-peak Lorentzian.
#pragma once
#include "obe_sweep_common.h"

namespace obe {

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
// where the pieces live, in doubles from a 16-byte aligned base behind the packed draws (SweepForms::carve), for any
// cell sweep of AT MOST nd draws
struct CellLayout {
    static constexpr int64_t kPlan = 0, kRan = 3, kCoef = 4;                 // plan; marker; folded coefficients
    static constexpr int64_t kPart = kCoef + (int64_t)LorentzCells::kCoefs * LorentzCells::kMaxCells;     // chunk partials
    static int64_t doubles(int64_t nd) {
        return kPart + (int64_t)plan_cell_chunks(nd).nchunks_bound * LorentzCells::kCoefs * LorentzCells::kMaxCells;
    }
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

// the cell form of one call: whether it is taken, where its pieces live in the workspace, and its launches
struct CellForm {
    bool on = false;
    CellPlan* plan = nullptr;
    double* coef = nullptr;
    double* part = nullptr;
    unsigned* ran = nullptr;       // cell_eval_kernel's marker

    static bool selected(const obe_model& m, int flags, int64_t ns, const int64_t* d_draw_idx, int64_t n_draws) {
        return (flags & OBE_SWEEP_CELLS) && expansion_applies(m, flags, ns, d_draw_idx, n_draws);
    }
    void carve(double* base) {
        plan = reinterpret_cast<CellPlan*>(base + CellLayout::kPlan);
        ran = reinterpret_cast<unsigned*>(base + CellLayout::kRan);
        coef = base + CellLayout::kCoef;
        part = base + CellLayout::kPart;
    }
    // once per call, behind the pack: the cells of this call's settings
    int before(const SweepArgs& a, hipStream_t st) const {
        cell_plan_kernel<<<1, kCellPlanThreads, 0, st>>>(a, plan);
        OBE_CHECK_LAUNCH("cell_plan_kernel");
        return 0;
    }
    // in place of sweep_kernel: one chunk of moments in part1 / part2, cs_out = 0
    int sweep(SweepPlan& p, SweepArgs& a, unsigned seq, hipStream_t st) const {
        using LC = LorentzCells;
        const CellChunks chunks = plan_cell_chunks(a.nd);
        p.nchunks = 1;
        a.tiles_x = p.tiles_x;
        a.one = 1;
        a.xcd_map = 0;
        a.chunk = chunks.chunk;
        a.nchunks = chunks.nchunks;          // (of the expansion; sweep_finalize is told p.nchunks = 1)
        cell_moments_kernel<<<(unsigned)chunks.nchunks * kCellWaves, kBlock, 0, st>>>(a, plan, part);
        OBE_CHECK_LAUNCH("cell_moments_kernel");
        cell_fold_kernel<<<LC::kCoefs * kCellWaves, kCellFoldGroups * kWave, 0, st>>>(part, chunks.nchunks, plan, coef, a.abort);
        OBE_CHECK_LAUNCH("cell_fold_kernel");
        cell_eval_kernel<<<(unsigned)((a.ns + kBlock - 1) / kBlock), kBlock, 0, st>>>(a, plan, coef, ran, seq);
        OBE_CHECK_LAUNCH("cell_eval_kernel");
        return 0;
    }
};
#endif  // the kernels and the host half

}  // namespace obe
