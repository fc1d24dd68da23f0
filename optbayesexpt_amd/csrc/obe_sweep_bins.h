// The bin form of the utility sweep (OBE_SWEEP_BINS, and the kept grouping of obe_sweep_utility_keep): its constants,
// workspace and keep-buffer layout, its kernels, and BinForm, the host half of one call.  The first part is plain host
// code and serves every build (obe_sweep_bins_plan, obe_sweep_bins_eval_waves, obe_sweep_bins_keep_bytes and
// obe_sweep_bins_keep_records_bytes answer from it whatever the model); the kernels and BinForm exist where the library
// has the one-peak Lorentzian.
#pragma once
#include "obe_sweep_common.h"

namespace obe {

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

// ---- the kept grouping (obe_sweep_utility_keep, OBE_SWEEP_BINS_KEPT) ----
// The workspace is scratch of every library call; what outlives a sweep lives in a buffer of the caller's: the plan,
// binstart / itemstart and the sorted position of every draw — functions of the packed tau0 = x0 / d alone.
struct BinKeep {           // head of the buffer
    BinPlan plan;
    unsigned mark;         // kBinKeepMark once the grouping behind it is complete (bin_group_kernel<true> writes it)
    int nd;                // the draws it was made for ...
    unsigned long long dbits;      // ... and the bits of d
    unsigned mismatch;     // the `call` of the last reuse that found a draw outside its kept bin
    unsigned records;      // kBinKeepMark once the records behind the grouping are complete too (BinKeepLayout)
    unsigned pad[6];
};
static_assert(sizeof(BinKeep) == 64, "the head of the keep buffer is 16 ints");
constexpr unsigned kBinKeepMark = 0x6b455042u;
struct BinKeepLayout {      // in ints
    static constexpr int64_t kStarts = sizeof(BinKeep) / sizeof(int);                       // 2 x 130 ints
    static constexpr int64_t kDest = (kStarts + 2 * (LorentzBins::kMaxBins + 2) + 3) & ~(int64_t)3;
    static int64_t bytes(int64_t nd) { return ((kDest + nd) * (int64_t)sizeof(int) + 15) & ~(int64_t)15; }
    // The records form (obe_sweep_bins_keep_records_bytes): behind the grouping, each piece 16-byte aligned, the
    // particle part of every draw in sorted order, {x0 / d, a, b}, and a dense array of sqrt(w) in the same order: the
    // only piece a sweep of the same particles with other weights has to write (it shares no line with the records
    // but the one at the seam).
    static constexpr int64_t kRecord = 3;                                                  // doubles per draw
    static int64_t records_at(int64_t nd) { return bytes(nd); }                            // in bytes
    static int64_t sw_at(int64_t nd) { return records_at(nd) + ((kRecord * 8 * nd + 15) & ~(int64_t)15); }
    static int64_t records_bytes(int64_t nd) { return sw_at(nd) + ((8 * nd + 15) & ~(int64_t)15); }
};

#ifndef OBE_PLUGIN_MODEL_HEADER
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
// and then bin_moments_kernel onwards: the same records in the same places, hence the same bits.  With a keep buffer
// of the records form (BinKeepLayout::records_bytes) the particle part of every record and sqrt(w) live in the buffer
// too, in sorted order; such a later call runs
//   bin_refresh_kernel        sqrt(w) of draw p, written to sw[dest[p]]
// and bin_moments_kernel<true> forms every packed record from those pieces.
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

// The records form of the keep buffer (a call whose keep_bytes reaches BinKeepLayout::records_bytes): where a rebuild
// leaves the particle part of every draw and sqrt(w), and where bin_moments_kernel<true> reads them; rec == NULL
// otherwise, and the packed records go through the workspace's `sorted`.
struct BinRecords {
    double* rec;           // [nd][kRecord] x0 / d, a, b in sorted order
    double* sw;            // [nd] sqrt(w) in sorted order
    const double* bbar;    // the mean of b: element K + 1 of the mean parameters in d_moments
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
__device__ __forceinline__ double bin_x0(const SweepArgs& a, int64_t p) {
    double w;
    const int64_t src = draw_source(a, p, w);
    return a.particles[src];
}
__device__ __forceinline__ double bin_tau0(const SweepArgs& a, int64_t p) { return bin_x0(a, p) / a.m.consts[0]; }

// The packed record of a draw from its particle part {x0 / d, a, b}, sqrt(w) and the mean of b: the expressions of
// Lorentz<1>::pack behind its division, stated once for the record that is stored (bin_record) and the one that
// bin_moments_kernel<true> forms from the kept particle part.  (-ffp-contract=off: the same bits in either place.)
__device__ __forceinline__ void bin_pk(double tau0, double amp, double b, double bbar, double sw, double (&pk)[4]) {
    pk[0] = tau0;
    pk[1] = sw * amp;
    pk[2] = sw * (b - bbar);
    pk[3] = sw;
}
// the particle part of draw p and sqrt of its weight
__device__ __forceinline__ void bin_particle(const SweepArgs& a, int64_t p, double (&part)[3], double& sw) {
    using M = Lorentz<1>;
    static_assert(packed_width<M>() == 4 && M::NPK == 3, "the sorted records are 32 bytes");
    double w;
    const int64_t src = draw_source(a, p, w);
    sw = sqrt(w);
    part[0] = a.particles[src] / a.m.consts[0];               // (Lorentz<1>::pack's division)
    part[1] = a.particles[src + a.ld_p];
    part[2] = a.particles[src + 2 * a.ld_p];
}
// the sorted record of draw p: what sweep_pack_kernel<Lorentz<1>> makes of it
__device__ __forceinline__ void bin_record(const SweepArgs& a, int64_t p, double2& ra, double2& rb) {
    double part[3], sw, pk[4];
    bin_particle(a, p, part, sw);
    bin_pk(part[0], part[1], part[2], a.moments[4], sw, pk);
    ra = double2{pk[0], pk[1]};
    rb = double2{pk[2], pk[3]};
}

// the records form: the particle part of draw p and sqrt(w) to their sorted position `pos` in the keep buffer
__device__ __forceinline__ void bin_store_particle(const SweepArgs& a, int64_t p, int pos, const BinRecords& r) {
    double part[3], sw;
    bin_particle(a, p, part, sw);
    double* __restrict__ out = r.rec + BinKeepLayout::kRecord * (int64_t)pos;
    out[0] = part[0];
    out[1] = part[1];
    out[2] = part[2];
    r.sw[pos] = sw;
}

// a draw between the two grouping passes of a rebuild: its bin, and its rank among its unit's draws of that bin
constexpr int kBinRankBits = 24;
static_assert((((int64_t)1 << 30) + kBinMaxUnits - 1) / kBinMaxUnits <= ((int64_t)1 << kBinRankBits)
                  && LorentzBins::kMaxBins <= (1 << (31 - kBinRankBits)),
              "a unit of a cloud of 2^30 draws (BinForm::selected) has at most 2^19 draws: rank and bin share an int");
__device__ __forceinline__ int bin_code(int bin, int rank) { return (bin << kBinRankBits) | rank; }
constexpr int kBinIndexBits = 7;
constexpr int kBinGroupAhead = 8;         // trips of the counting pass whose loads are in flight together
static_assert(LorentzBins::kMaxBins == 1 << kBinIndexBits, "a bin index is matched bit by bit (bin_group_kernel<false>)");

// (the first launch of a rebuild: with a keep buffer, no grouping stands behind its head until the scatter pass says so)
__global__ __launch_bounds__(kBlock) void bin_minmax_kernel(SweepArgs a, BinSweepPtrs q) {
    constexpr int NW = kBlock / kWave;
    __shared__ double slo[NW], shi[NW];
    __shared__ int sbad[NW];
    if (sweep_aborted(a.abort)) return;
    if (q.keep && blockIdx.x == 0 && threadIdx.x == 0) {
        q.keep->mark = 0u;
        q.keep->records = 0u;
    }
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
// at a time.  The unit's count of every bin is a table in LDS; per trip every lane finds the lanes that hold its own bin
// (kBinIndexBits ballots, whatever the number of distinct bins among the 64 draws), and a draw's rank is its bin's count
// so far plus the number of lower lanes with the same bin; the lowest of them adds their number to the count.
// The counts end as the unit's, and every draw leaves its bin_code.
// SCATTER = true: lane l holds the first sorted position of (bin l, unit) and of (bin l + 64, unit); every draw's
// record (bin_record) is formed from the cloud and written at its bin's first position plus its rank.
// RECORDS (with SCATTER, a keep buffer of the records form): in place of the packed record in the workspace, the
// draw's particle part and sqrt(w) go to the keep buffer (BinRecords), and the head says that they are complete.
template <bool SCATTER, bool RECORDS = false>
__global__ __launch_bounds__(kBlock) void bin_group_kernel(SweepArgs a, int64_t per, int nunits, int mm_blocks,
                                                           BinSweepPtrs q, BinRecords r) {
    using LB = LorentzBins;
    static_assert(SCATTER || !RECORDS, "the counting pass stores no record");
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
            if constexpr (RECORDS) q.keep->records = kBinKeepMark;
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
    if constexpr (SCATTER) {
        for (int64_t i0 = begin; i0 < end; i0 += kWave) {
            const int64_t i = i0 + lane;
            const bool live = i < end;
            const int code = live ? q.code[i] : 0;
            const int bin = code >> kBinRankBits;
            // (every lane takes part in the exchange: a lane without a draw asks for bin 0)
            const int first0 = __shfl(c0, bin & (kWave - 1), kWave), first1 = __shfl(c1, bin & (kWave - 1), kWave);
            const int pos = (bin < kWave ? first0 : first1) + (code & ((1 << kBinRankBits) - 1));
            if (live && pos >= 0 && pos < a.nd) {
                if constexpr (RECORDS) {
                    bin_store_particle(a, i, pos, r);
                } else {
                    double2 ra, rb;
                    bin_record(a, i, ra, rb);
                    double2* __restrict__ out = reinterpret_cast<double2*>(q.sorted) + 2 * (int64_t)pos;
                    out[0] = ra;
                    out[1] = rb;
                }
            }
            if (q.dest && live) q.dest[i] = pos;       // (over the code this lane has just read)
        }
    } else {
        // the unit's count of every bin so far: a table of the wavefront's own (same-wavefront LDS accesses execute in
        // order; the fence keeps the compiler from moving one trip's read above the trip before's stores)
        __shared__ int tally[kBlock / kWave][LB::kMaxBins];
        int* count = tally[threadIdx.x / kWave];
        count[lane] = 0;
        count[lane + kWave] = 0;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const double d = a.m.consts[0];
        const unsigned long long below = (1ull << lane) - 1ull;
        // One trip: the 64 draws from i0 on, lane <-> draw, x0 the lane's own.
        auto trip = [&](int64_t i0, double x0) {
            const int64_t i = i0 + lane;
            const bool live = i < end;
            const int bin = live ? LB::bin_of(plan.origin, x0 / d, nbins) : -1;        // (bin_tau0's division)
            // the live lanes that hold this lane's bin: one ballot per bit of a bin index, kept where the lane's own
            // bit agrees.  (A lane without a draw has every bit set and is in the ballots of the set bits; the live
            // lanes drop it with the first mask, and it matches nobody itself.)
            unsigned long long same = __ballot(live);
#pragma unroll
            for (int k = 0; k < kBinIndexBits; ++k) {
                const bool bit = (bin >> k) & 1;
                const unsigned long long have = __ballot(bit);
                same &= bit ? have : ~have;
            }
            if (!live) same = 0ull;
            const int sofar = live ? count[bin] : 0;
            // (one leader per bin and trip: no two lanes store to one word)
            if (live && (same & below) == 0ull) count[bin] = sofar + __popcll(same);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            if (live) q.code[i] = bin_code(bin, sofar + __popcll(same & below));
        };
        // The x0 of kBinGroupAhead trips are asked for together, before the first of them is matched: a unit of a
        // cloud of 2^20 draws is eight trips, and a trip's arithmetic is short against one round trip to memory.  A lane
        // without a draw asks for the unit's last one (a load under a condition would be waited for where it stands).
        for (int64_t i0 = begin; i0 < end; i0 += kBinGroupAhead * kWave) {
            double x0[kBinGroupAhead];
#pragma unroll
            for (int k = 0; k < kBinGroupAhead; ++k) {
                const int64_t i = i0 + k * kWave + lane;
                x0[k] = bin_x0(a, i < end ? i : end - 1);
            }
#pragma unroll
            for (int k = 0; k < kBinGroupAhead; ++k)
                if (i0 + k * kWave < end) trip(i0 + k * kWave, x0[k]);
        }
        q.counts[lane * kBinMaxUnits + unit] = count[lane];
        q.counts[(lane + kWave) * kBinMaxUnits + unit] = count[lane + kWave];
    }
}

// OBE_SWEEP_BINS_KEPT, in place of the four launches above: the record of draw p (full mode), written where
// bin_group_kernel<true> put it when the keep buffer was made.  Nothing is written unless the head fits the call
// (bin_keep_refused: that is what keeps dest[p] inside `sorted`), and a draw goes nowhere unless it still belongs to
// the bin whose run holds its kept position: a tau0 that is not finite, lies outside the plan or in another bin stores
// the call's number into the head, and bin_eval_kernel answers NaN for the whole call, as for a poisoned plan.  (A
// draw that moved WITHIN its bin gives what a rebuild would: the order of a stable sort by bin does not change.)
// (RECORDS: the verified draw's particle part and sqrt(w) go to the keep buffer's records instead)
template <bool RECORDS>
__device__ __forceinline__ void bin_scatter_pack_draw(const SweepArgs& a, const BinSweepPtrs& q, const BinRecords& r,
                                                      double origin, int nbins, int64_t p) {
    using LB = LorentzBins;
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
        if constexpr (RECORDS) {
            bin_store_particle(a, p, pos, r);
        } else {
            double2* __restrict__ out = reinterpret_cast<double2*>(q.sorted) + 2 * (int64_t)pos;
            out[0] = ra;
            out[1] = rb;
        }
    } else {
        q.keep->mismatch = q.call;
    }
}
__global__ __launch_bounds__(kBlock) void bin_scatter_pack_kernel(SweepArgs a, BinSweepPtrs q) {
    using LB = LorentzBins;
    if (sweep_aborted(a.abort)) return;
    if (bin_keep_refused(q)) return;
    const int nbins = __builtin_amdgcn_readfirstlane(q.plan->nbins);
    if (nbins <= 0 || nbins > LB::kMaxBins) return;
    const double origin = q.plan->origin;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < a.nd; p += (int64_t)gridDim.x * kBlock)
        bin_scatter_pack_draw<false>(a, q, BinRecords{}, origin, nbins, p);
}

// OBE_SWEEP_BINS_KEPT with a keep buffer of the records form, in place of bin_scatter_pack_kernel: the particles have
// not changed (the caller's word, as for d_moments), so of a draw's record only sqrt(w) is new, and it goes to
// sw[dest[p]]: no particle is read, nothing is divided and no bin is checked.  What is written through still rests on
// the head alone (bin_keep_refused, and the library wrote dest itself: 0 <= dest[p] < nd is checked all the same).
// A buffer whose grouping is complete but whose records are not (its last rebuild was told the smaller size) takes the
// verifying path of bin_scatter_pack_kernel, into the records.  A workgroup owns `per` consecutive draws: the draws of
// one bin in it are neighbours in sw, and a line of sw is not split over the L2s of several XCDs more than it must.
__global__ __launch_bounds__(kBlock) void bin_refresh_kernel(SweepArgs a, BinSweepPtrs q, BinRecords r, int64_t per) {
    using LB = LorentzBins;
    if (sweep_aborted(a.abort)) return;
    if (bin_keep_refused(q)) return;
    const int nbins = __builtin_amdgcn_readfirstlane(q.plan->nbins);
    if (nbins <= 0 || nbins > LB::kMaxBins) return;
    const int64_t begin = (int64_t)blockIdx.x * per;
    const int64_t end = begin + per < a.nd ? begin + per : a.nd;
    if (q.keep->records == kBinKeepMark) {
        const double* __restrict__ w = a.weights;
        const int* __restrict__ dest = q.dest;
        for (int64_t p = begin + threadIdx.x; p < end; p += kBlock) {
            const int pos = dest[p];
            if (pos >= 0 && pos < a.nd) r.sw[pos] = sqrt(w[p]);
        }
    } else {
        const double origin = q.plan->origin;
        for (int64_t p = begin + threadIdx.x; p < end; p += kBlock) bin_scatter_pack_draw<true>(a, q, r, origin, nbins, p);
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

// one wavefront per item: kBinChunk consecutive sorted draws of one bin.  RECORDS: the keep buffer's records form
// (BinRecords) in place of the packed records of `sorted`: a draw's packed record is formed here, from its kept particle
// part, sqrt(w) and the mean of b (bin_pk: the stored record's expressions on its operands, hence its bits).
template <bool RECORDS>
__global__ __launch_bounds__(kWave) void bin_moments_kernel(BinSweepPtrs q, const unsigned* abort, BinRecords r) {
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
    LB::Sums z;
    z.clear();
    if constexpr (!RECORDS) {
        const double2* __restrict__ rec = reinterpret_cast<const double2*>(q.sorted);
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
    } else {
        // the same draws in the same order, lane by lane, the next trip's pieces asked for before this trip's arithmetic
        const double bbar = *r.bbar;
        const double* __restrict__ rec = r.rec;
        const double* __restrict__ rsw = r.sw;
        constexpr int64_t R = BinKeepLayout::kRecord;
        int i = first + lane;
        double tau0 = 0.0, amp = 0.0, b = 0.0, sw = 0.0;
        if (i < end) {
            tau0 = rec[R * i];
            amp = rec[R * i + 1];
            b = rec[R * i + 2];
            sw = rsw[i];
        }
        while (i < end) {
            const int in = i + kWave;
            double ntau0 = tau0, namp = amp, nb = b, nsw = sw;
            if (in < end) {
                ntau0 = rec[R * in];
                namp = rec[R * in + 1];
                nb = rec[R * in + 2];
                nsw = rsw[in];
            }
            double pk[4];
            bin_pk(tau0, amp, b, bbar, sw, pk);
            LB::add_draw(tb, pk, z);
            tau0 = ntau0;
            amp = namp;
            b = nb;
            sw = nsw;
            i = in;
        }
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

// the bin form of one call (it goes before the cell form where both bits are set): whether it is taken, where its
// pieces live in the workspace and in the caller's keep buffer, and its launches
struct BinForm {
    bool on = false;
    BinSweepPtrs q{};              // (q.ran: bin_eval_kernel's marker; q.reuse: OBE_SWEEP_BINS_KEPT honoured)
    BinRecords r{};                // (r.rec: the keep buffer has the records form)

    // OBE_SWEEP_BINS is honoured where the cell form would be, for clouds whose positions fit an int
    static bool selected(const obe_model& m, int flags, int64_t ns, const int64_t* d_draw_idx, int64_t n_draws,
                         int64_t nd) {
        return (flags & OBE_SWEEP_BINS) && nd <= ((int64_t)1 << 30) && expansion_applies(m, flags, ns, d_draw_idx, n_draws);
    }
    // packed: the room of the packed draws (no plain packed copy in this form: a rebuild keeps nd ints there)
    void carve(double* base, double* packed, int64_t nd, const obe_model& m, int flags, const int64_t* d_draw_idx,
               void* d_keep, int64_t keep_bytes) {
        using BL = BinLayout;
        q.plan = reinterpret_cast<BinPlan*>(base + BL::kPlan);
        q.ran = reinterpret_cast<unsigned*>(base + BL::kRan);
        q.binstart = reinterpret_cast<int*>(base + BL::kStarts);
        q.itemstart = q.binstart + LorentzBins::kMaxBins + 2;
        q.minmax = base + BL::kMinmax;
        q.totals = reinterpret_cast<int*>(base + BL::kTotals);
        q.counts = reinterpret_cast<int*>(base + BL::kCounts);
        q.coef = base + BL::kCoef;
        q.part = base + BL::kPart;
        q.sorted = base + BL::sorted(nd);
        q.code = reinterpret_cast<int*>(packed);
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
            q.reuse = (flags & OBE_SWEEP_BINS_KEPT) != 0;
            q.keep_nd = static_cast<int>(nd);
            memcpy(&q.keep_dbits, &m.consts[0], sizeof q.keep_dbits);
            q.call = ++calls;
            if (q.call == 0u) q.call = ++calls;
            // ... and large enough for the records form too: the draws' records live there, not in `sorted`
            if (keep_bytes >= BinKeepLayout::records_bytes(nd)) {
                char* bytes = static_cast<char*>(d_keep);
                r.rec = reinterpret_cast<double*>(bytes + BinKeepLayout::records_at(nd));
                r.sw = reinterpret_cast<double*>(bytes + BinKeepLayout::sw_at(nd));
            }
        }
    }
    // in place of the pack.  A rebuild of the grouping packs every draw straight to its sorted position, as part of
    // the sweep; a reuse of a kept one does so here: bin_scatter_pack_kernel puts the records where the buffer says,
    // or, where the buffer holds the records themselves, bin_refresh_kernel renews their sqrt(w)
    int before(const SweepArgs& a, hipStream_t st) const {
        if (!q.reuse) return 0;
        if (r.rec) {
            // (a workgroup's run of draws: those of its four wavefronts in the grouping passes)
            const int64_t per = plan_bin_units(a.nd).per * (kBlock / kWave);
            bin_refresh_kernel<<<(unsigned)((a.nd + per - 1) / per), kBlock, 0, st>>>(a, q, r, per);
            OBE_CHECK_LAUNCH("bin_refresh_kernel");
            return 0;
        }
        bin_scatter_pack_kernel<<<stream_blocks(a.nd, kBlock), kBlock, 0, st>>>(a, q);
        OBE_CHECK_LAUNCH("bin_scatter_pack_kernel");
        return 0;
    }
    // in place of sweep_kernel and sweep_finalize (f.yvar = NULL: of sweep_kernel, one chunk of moments in part1 / part2,
    // cs_out = 0).  The bins are a function of the cloud: grouping it is part of the sweep, and of its time; then the
    // bins' folded rows, and the settings.
    int sweep(SweepPlan& p, const SweepArgs& a, unsigned seq, const BinFinish& f, hipStream_t st) const {
        using LB = LorentzBins;
        if (!q.reuse) {
            const BinUnits units = plan_bin_units(a.nd);
            const int mm_blocks = static_cast<int>(std::min<int64_t>(kBinMinmaxBlocks, (a.nd + kBlock - 1) / kBlock));
            bin_minmax_kernel<<<mm_blocks, kBlock, 0, st>>>(a, q);
            OBE_CHECK_LAUNCH("bin_minmax_kernel");
            const unsigned group_blocks = (unsigned)((units.nunits + kBlock / kWave - 1) / (kBlock / kWave));
            bin_group_kernel<false><<<group_blocks, kBlock, 0, st>>>(a, units.per, units.nunits, mm_blocks, q, r);
            OBE_CHECK_LAUNCH("bin_group_kernel<count>");
            bin_scan_kernel<<<LB::kMaxBins, kBlock, 0, st>>>(units.nunits, q, a.abort);
            OBE_CHECK_LAUNCH("bin_scan_kernel");
            if (r.rec)
                bin_group_kernel<true, true><<<group_blocks, kBlock, 0, st>>>(a, units.per, units.nunits, mm_blocks, q, r);
            else
                bin_group_kernel<true><<<group_blocks, kBlock, 0, st>>>(a, units.per, units.nunits, mm_blocks, q, r);
            OBE_CHECK_LAUNCH("bin_group_kernel<scatter>");
        }
        // (one wavefront per item: at least as many as any cloud makes)
        if (r.rec) {
            BinRecords rr = r;
            rr.bbar = a.moments + 4;          // (Lorentz<1>::pack's thbar[K + 1] of thbar = d_moments + 2)
            bin_moments_kernel<true><<<(unsigned)bin_max_items(a.nd), kWave, 0, st>>>(q, a.abort, rr);
        } else {
            bin_moments_kernel<false><<<(unsigned)bin_max_items(a.nd), kWave, 0, st>>>(q, a.abort, r);
        }
        OBE_CHECK_LAUNCH("bin_moments_kernel");
        bin_fold_kernel<<<2 * LB::kMaxBins, kBinFoldGroups * kWave, 0, st>>>(q, a.abort);
        OBE_CHECK_LAUNCH("bin_fold_kernel");
        p.nchunks = 1;
        const unsigned groups = (unsigned)((a.ns + kWave - 1) / kWave);
        switch (plan_bin_eval_waves(a.ns)) {             // (the shapes of kBinEvalShapes)
            case 8: bin_eval_kernel<1, 8><<<groups, 8 * kWave, 0, st>>>(a, q, seq, f); break;
            case 6: bin_eval_kernel<2, 6><<<(groups + 1) / 2, 12 * kWave, 0, st>>>(a, q, seq, f); break;
            case 3: bin_eval_kernel<4, 3><<<(groups + 3) / 4, 12 * kWave, 0, st>>>(a, q, seq, f); break;
            default: bin_eval_kernel<4, 1><<<(groups + 3) / 4, kBlock, 0, st>>>(a, q, seq, f);
        }
        OBE_CHECK_LAUNCH("bin_eval_kernel");
        return 0;
    }
};
#endif  // the kernels and the host half

}  // namespace obe
