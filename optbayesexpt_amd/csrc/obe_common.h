// Shared device helpers for libobe_hip (gfx950 only).
//
// Build flags matter here: the library is compiled with -ffp-contract=off so that the
// parity-critical streams (Bayes update, moments, resample) perform exactly the
// NumPy sequence of correctly-rounded operations, while the flop-bound sweep kernel
// asks for its FMAs explicitly with fma().
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <type_traits>
#include <utility>

#include "../../include/obe_hip.h"

namespace obe {

constexpr int kWave = 64;          // CDNA wavefront
constexpr int kBlock = 256;        // 4 waves: one per SIMD of a CU
constexpr int kMaxBlocks = 2048;   // 256 CUs x 8: grid cap for streaming kernels
constexpr int kFastDims = OBE_FAST_DIMS;   // cloud kernels are templated on the row count up to here, tiled beyond
constexpr double kDblMax = 1.7976931348623157e308;

void set_error(const std::string& msg);
bool defer_host_sync();    // obe_defer_host_sync: host results are copied asynchronously, the caller synchronises
int fail(hipError_t e, const char* what);
int bad_arg(const char* what);

// Host-side dispatch on the width of the cloud: f(std::integral_constant<int, D>{}) for D == n_dims in
// [LO, kFastDims], the widths the cloud kernels are instantiated for; any other width is refused with `refusal`.
static_assert(OBE_FAST_DIMS == 16, "edit with OBE_FAST_DIMS the five refusals that say \"1..16\": obe_bayes_update_model_moments, "
                                   "obe_mask_renorm_moments, obe_resample_begin, obe_resample_particles, obe_drift_particles");
template <int LO, class F, int... I>
int dispatch_dims_from(int n_dims, const char* refusal, F&& f, std::integer_sequence<int, I...>) {
    int rc = 0;
    const bool found = ((n_dims == LO + I && ((rc = f(std::integral_constant<int, LO + I>{})), true)) || ...);
    return found ? rc : bad_arg(refusal);
}
template <int LO = 1, class F>
int dispatch_dims(int n_dims, const char* refusal, F&& f) {
    return dispatch_dims_from<LO>(n_dims, refusal, f, std::make_integer_sequence<int, kFastDims - LO + 1>{});
}

#define OBE_HIP_TRY(expr)                                   \
    do {                                                    \
        hipError_t e_ = (expr);                             \
        if (e_ != hipSuccess) return ::obe::fail(e_, #expr); \
    } while (0)

#define OBE_CHECK_LAUNCH(name)                                  \
    do {                                                        \
        hipError_t e_ = hipGetLastError();                      \
        if (e_ != hipSuccess) return ::obe::fail(e_, name);     \
    } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Device-visible address of page-locked host memory (hipHostMalloc / hipHostRegister: what torch's
// pin_memory() gives), or nullptr for pageable memory.  A kernel that delivers a few scalars to the
// host writes them there itself: the blit kernel of a tiny hipMemcpyAsync costs a launch (~5-10 us of
// latency per result on an otherwise short call).
inline void* device_view_of_host(const void* h) {
    if (!h) return nullptr;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, h) != hipSuccess) {
        (void)hipGetLastError();           // pageable memory is "invalid value" to some runtimes: not an error here
        return nullptr;
    }
    return attr.type == hipMemoryTypeHost ? attr.devicePointer : nullptr;
}

// Results that a call's LAST kernel writes straight into the caller's page-locked memory are waited for
// by watching that memory, not by hipStreamSynchronize: the host arms one designated word with a bit pattern
// no result can have (a NaN payload / an impossible index), the kernel stores its results, fences at system
// scope and stores that word last, and the host spins until it changes.  On MI355X the round trip of a
// short kernel is 5.9 us this way against 11.1 us through the stream's completion signal
// (tools/microbench_sync.hip) — a cycle of the reference-sized workloads has two of them.  A kernel that
// never delivers (a fault) ends the spin after kHostWaitSpinUs and the stream is synchronised, which
// reports the error; later work on the stream is ordered behind the kernel as usual.
constexpr uint64_t kHostSentinel = 0x7ff8c0dec0dec0deULL;
constexpr double kHostWaitSpinUs = 400.0;        // (longer kernels: the stream's own wait; its 5 us no longer matter)
inline void arm_host_word(void* h_word) { *reinterpret_cast<volatile uint64_t*>(h_word) = kHostSentinel; }
int wait_host_word(const void* h_word, hipStream_t st);      // obe_capi.hip
// Round 4: results of more than one word are waited for WORD BY WORD — every word of the block is armed and
// the host spins until none carries the pattern any more.  An 8-byte store arrives whole, so that needs no
// ordering between the stores at all.  The earlier form (arm one word, store it last behind a system-scope
// fence) was not safe for blocks that span several 128-byte lines: about once in 3000 resamples the host saw
// the watched word while the covariance entries of ANOTHER line still held the previous resample's values
// (per-thread fences, an explicit s_waitcnt after the fence and delivery by a single wave did not close it;
// found by tools/fuzz_parity.py's sweeper recipes, pinned down with tools/diag_host_delivery.py).
inline void arm_host_words(void* h_words, int64_t n) {
    volatile uint64_t* p = reinterpret_cast<volatile uint64_t*>(h_words);
    for (int64_t i = 0; i < n; ++i) p[i] = kHostSentinel;
}
int wait_host_words(const void* h_words, int64_t n, hipStream_t st);      // obe_capi.hip

// n result words of the caller's (h_words NULL: the caller wants none), and the one statement of how they reach the
// host.  The call hands view() — the device view, NULL for pageable memory — to the kernel that delivers, arm()s the
// words once nothing can refuse it any more and BEFORE its first launch, and after its last launch wait()s: by
// watching the armed words, or — pageable memory, or a call that may not arm (obe_moments) — by the stream's own wait.
// A call that does not wait by design (the update's enqueue form, OBE_SWEEP_NOWAIT, ...) stops after arm(): the
// caller watches.  copy() is the pageable route, from the device copy of the results; a no-op where kernels deliver.
class HostWords {
  public:
    HostWords(void* h_words, int64_t n) : host_(h_words), dev_(device_view_of_host(h_words)), n_(n) {}
    template <class T> T* host() const { return static_cast<T*>(host_); }
    template <class T> T* view() const { return static_cast<T*>(dev_); }
    void arm() {
        if (dev_) arm_host_words(host_, n_);
        armed_ = dev_ != nullptr;
    }
    int copy(int64_t first, int64_t count, const void* d_src, hipStream_t st) const {
        if (!host_ || dev_) return 0;
        OBE_HIP_TRY(hipMemcpyAsync(host<uint64_t>() + first, d_src, count * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        return 0;
    }
    int wait(hipStream_t st) const {
        if (!host_) return 0;
        if (armed_) return wait_host_words(host_, n_, st);
        OBE_HIP_TRY(hipStreamSynchronize(st));
        return 0;
    }

  private:
    void* host_;
    void* dev_;
    int64_t n_;
    bool armed_ = false;
};
// device side: everything stored to the host before this call is visible there before what follows
// (the explicit wait restates the one that belongs behind the fence's L2 write-back: ROCm 7.2's compiler drops
// it when its scoreboard says this wave has nothing outstanding, and the flag store that follows can then
// overtake the write-back of the results — cdna_hip_programming.md, Guideline 16 pitfall 12; seen here as a
// host copy of the covariance with entries of the previous resample, about once in 3000 resamples)
__device__ __forceinline__ void host_results_before_flag() {
    __threadfence_system();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- "the last workgroup to arrive folds": arrival counter + write-through partials ----
// Zeroed device words owned by the library, one slot per (device, stream) (obe_capi.hip); nullptr: none
// (allocation failed, or OBE_CONTROL_SLOTS=0).  A full table hands the least recently used slot on — after a
// device synchronisation, so that no kernel of its previous owner is still counting in it.
unsigned* stream_control_words(hipStream_t st);

// A second stream (and three events) that belongs to a caller's stream: two independent kernel chains of one
// call run side by side (obe_resample.hip: the random-number chain next to the CDF / search / covariance
// chain) and are joined again with events before the call's results are consumed on the caller's stream.
// Created on first use per (device, stream), never destroyed.  false: none available — one stream does both.
struct SideStream {
    hipStream_t stream;
    hipEvent_t entry, mid, done;
    hipStream_t stream2;         // a third chain (round 5: the covariance + the (N, D) copy of a resample)
    hipEvent_t done2;
};
bool side_stream_of(hipStream_t st, SideStream* out);      // obe_capi.hip

// A block partial that another workgroup of the same launch will read: written through to memory
// (a relaxed agent-scope atomic store lowers to `global_store ... sc1`), so publishing needs no release
// fence — an agent-scope release writes back every dirty line of the XCD's L2, i.e. the weights the
// kernel has just written (MI355X_MICROARCH.md, inter-workgroup visibility: publish-large).
__device__ __forceinline__ void store_published(double* p, double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ... and read back past this CU's L1 (sc1 load): stands in for an agent-scope acquire
__device__ __forceinline__ double load_published_f64(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p),
                                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// Call after every thread of the workgroup has issued its store_published() calls.  Returns true in
// EVERY thread of the workgroup that arrived last: by then all workgroups' published values are in
// memory; read them with load_published_f64() (ACQUIRE = false) or, after the agent-scope acquire this
// function then performs, with plain loads.
// Two levels of arrival counters: the workgroups b with b % 8 == g share counter g (its own 128-byte line),
// the last one of each group takes a ticket on the top counter.  256 tickets on ONE word cost ~4.3 us of
// serialised device-scope atomics (measured: the update's normalisation pass took 22.7 / 26.5 / 31.1 us with
// 256 / 512 / 768 workgroups); 8 x 32 on separate lines run side by side: 21.3 us (16 x 16: 21.7 us).  Every counter wraps to zero with
// its last arrival (atomicInc), ready for the next launch on the stream.  `flag` = one int of LDS.
constexpr int kArriveGroups = 8;
constexpr int kArriveStride = 32;                       // words between two counters: one 128-byte line each
constexpr int kControlSlotWords = kArriveStride * (kArriveGroups + 1);
// The resample decision that the enqueue form of the fused update leaves on the device (1: this update is
// followed by a resample) for the kernels of a sweep enqueued behind it (obe_sweep.hip: OBE_SWEEP_SPECULATIVE),
// which then do nothing.  It lives in the CALLER's memory — the last 8-byte word of the workspace both calls
// are given (include/obe_hip.h: OBE_WS_ABORT_WORD) — so the pair is tied by the object that owns the workspace,
// not by the stream: another object's (or thread's) update on the same stream cannot change it.  Both forms
// refuse a workspace without 16 spare bytes behind what their kernels use.
inline unsigned* ws_abort_word(void* d_ws, int64_t ws_bytes) {
    return reinterpret_cast<unsigned*>(static_cast<char*>(d_ws) + (ws_bytes & ~(int64_t)7) - 8);
}
template <bool ACQUIRE = true>
__device__ __forceinline__ bool arrive_last(unsigned* counter, int* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wave drains its write-through stores
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned g = blockIdx.x & (kArriveGroups - 1);
        const unsigned in_group = (gridDim.x - g + kArriveGroups - 1) / kArriveGroups;
        const unsigned groups = gridDim.x < (unsigned)kArriveGroups ? gridDim.x : (unsigned)kArriveGroups;
        int last = atomicInc(counter + g * kArriveStride, in_group - 1) == in_group - 1;          // device scope
        if (last) last = atomicInc(counter + kArriveGroups * kArriveStride, groups - 1) == groups - 1;
        if (ACQUIRE && last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");    // drop this CU's stale lines
        *flag = last;
    }
    __syncthreads();
    return *flag != 0;
}

inline int stream_blocks(int64_t n, int per_block) {
    int64_t b = (n + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > kMaxBlocks) b = kMaxBlocks;
    return static_cast<int>(b);
}
// obe_drift_particles: one particle per thread, at most kMaxBlocks workgroups of kBlock — a cloud of more than
// kMaxBlocks * kBlock = 524 288 particles takes further trips of the kernel's grid-stride loop
inline int drift_blocks(int64_t n_particles) { return stream_blocks(n_particles, kBlock); }

// ---- what the calls of obe_resample.hip need of the caller's workspace (they check against these; so does
// obe_workspace_bytes, next to moments_ws_bytes of obe_moments.h, update_ws_bytes of obe_update.h and the sweep's own)
constexpr int kScanItems = 8;                         // contiguous weights per thread
constexpr int kScanTile = kBlock * kScanItems;        // 2048 weights per block
// obe_weight_cdf / obe_cumsum / obe_draw_indices: 8 scalars, the block sums and (a CDF of weights) the block minima
inline int64_t scan_ws_bytes(int64_t n) {
    const int64_t nb = (n + kScanTile - 1) / kScanTile;
    return (2 * nb + 8) * (int64_t)sizeof(double);
}
// obe_resample_particles beyond OBE_FAST_DIMS: the D x D factor and the mean travel through the workspace
inline int64_t resample_wide_ws_bytes(int n_dims) {
    return ((int64_t)n_dims * n_dims + n_dims) * (int64_t)sizeof(double);
}

// a particle weight as every sum over the cloud takes it
__device__ __forceinline__ double clean_weight(double w) { return w > 0.0 ? w : 0.0; }      // NaN, negative -> 0

// np.nan_to_num defaults: NaN -> 0, +inf -> DBL_MAX, -inf -> -DBL_MAX
__device__ __forceinline__ double nan_to_num(double v) {
    if (v != v) return 0.0;
    if (v > kDblMax) return kDblMax;
    if (v < -kDblMax) return -kDblMax;
    return v;
}

// ---- declarative parameter bounds (OptBayesExpt.set_parameter_bounds; the constraint hooks of obe_noiseparam.py:57-79
// and demos/lockin/lockin_of_coil.py:115-133).  "This value violates its bound", stated once for mask_bounds_kernel
// (obe_update_common.hip) and the bounded gather (obe_resample.hip).  open: bit 0 = the lower bound itself violates
// (v <= lo instead of v < lo), bit 1 = the upper one; an absent end is -inf / +inf, inclusive.  Every comparison is
// false for a NaN value: it violates nothing, as in the reference's idioms.
__device__ __forceinline__ bool outside_bounds(double v, double lo, double hi, int open) {
    const bool below = (open & 1) ? v <= lo : v < lo;
    const bool above = (open & 2) ? v >= hi : v > hi;
    return below || above;
}

// the bounded rows of a call, by value in the kernel arguments (as RowsArg)
struct BoundsArg {
    int n;
    int rows[OBE_MAX_DIMS];
    double lo[OBE_MAX_DIMS], hi[OBE_MAX_DIMS];
    unsigned char open[OBE_MAX_DIMS];
};
// 0, or the refusal (-1): a NULL array, n_rows outside 1..OBE_MAX_DIMS, a row outside [0, n_dims_limit) — the kernels
// index the cloud with these —, a NaN bound, lower > upper
inline int make_bounds_arg(BoundsArg& ba, const int32_t* h_rows, const double* h_lower, const double* h_upper,
                           const int32_t* h_open, int n_rows, int n_dims_limit) {
    if (!h_rows || !h_lower || !h_upper || !h_open) return bad_arg("parameter bounds: null pointer");
    if (n_rows < 1 || n_rows > OBE_MAX_DIMS) return bad_arg("parameter bounds: n_rows outside 1..OBE_MAX_DIMS");
    ba = BoundsArg{};
    ba.n = n_rows;
    for (int k = 0; k < n_rows; ++k) {
        if (h_rows[k] < 0 || h_rows[k] >= n_dims_limit) return bad_arg("parameter bounds: row index out of range");
        if (h_lower[k] != h_lower[k] || h_upper[k] != h_upper[k]) return bad_arg("parameter bounds: NaN bound");
        if (h_lower[k] > h_upper[k]) return bad_arg("parameter bounds: lower > upper");
        ba.rows[k] = h_rows[k];
        ba.lo[k] = h_lower[k];
        ba.hi[k] = h_upper[k];
        // (an infinite end is an absent one: nothing is excluded there, whatever its flag says)
        const int lower_open = h_lower[k] > -INFINITY ? h_open[k] & 1 : 0;
        const int upper_open = h_upper[k] < INFINITY ? h_open[k] & 2 : 0;
        ba.open[k] = (unsigned char)(lower_open | upper_open);
    }
    return 0;
}

// lane `lane` (wave-uniform) of x, the same value in every lane
__device__ __forceinline__ double readlane_f64(double x, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

// ---- reductions: wave shuffle, then 4 partials through LDS; fixed order => deterministic
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
    return v;   // lane 0 holds the sum
}

// Sum of v over the block; valid in thread 0.  `red` = kBlock/kWave doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
        for (int i = 0; i < (int)(blockDim.x / kWave); ++i) s += red[i];
    }
    return s;
}

// Sum over the block, result broadcast to every thread.
__device__ __forceinline__ double block_sum_all(double v, double* red) {
    double s = block_sum(v, red);
    __syncthreads();
    if (threadIdx.x == 0) red[0] = s;
    __syncthreads();
    return red[0];
}

// Deterministic sum of a small device array by one block (every thread gets it).
// (four elements per thread and trip, their loads issued together and added in the order i, i + nt, ... of the
// one-at-a-time loop — the same bits: the 768 partial sums of the update's first pass used to be three dependent
// round trips at the start of EVERY workgroup of its second pass)
// (nt_part: the threads that take part, the first nt_part of the workgroup — a workgroup of more threads than kBlock
// that must reproduce the sum a kBlock-thread workgroup forms, e.g. the total the unfused normalisation divides by:
// the other threads contribute +0.0 behind everybody else's partial sums, which changes nothing)
__device__ __forceinline__ double block_sum_array(const double* a, int n, double* red, int nt_part = 0) {
    double v = 0.0;
    const int nt = nt_part > 0 ? nt_part : (int)blockDim.x;
    const bool part = (int)threadIdx.x < nt;
    for (int base = 0; base < n; base += 4 * nt) {
        double x[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = base + r * nt + (int)threadIdx.x;
            x[r] = a[i < n ? i : n - 1];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = base + r * nt + (int)threadIdx.x;
            const double t = v + x[r];
            v = i < n && part ? t : v;
        }
    }
    return block_sum_all(v, red);
}

// Exclusive scan, in place, of a short array (block sums of a reduce-then-scan) by ONE
// workgroup: each thread owns a contiguous segment, the segment totals are scanned through
// LDS in thread order.  Fixed association => deterministic.  Returns the grand total in
// every thread.  `lds` = blockDim.x elements of T.
template <class T>
__device__ __forceinline__ T block_exclusive_scan_inplace(T* __restrict__ data, int64_t n, T* lds) {
    const int t = threadIdx.x, nt = blockDim.x;
    const int64_t per = (n + nt - 1) / nt;
    const int64_t b = (int64_t)t * per, e = b + per < n ? b + per : n;
    T sum = T(0);
    for (int64_t i = b; i < e; ++i) sum = sum + data[i];
    lds[t] = sum;
    __syncthreads();
    if (t == 0) {
        // <= 256 serial adds.  Eight LDS reads are issued together and then added one after the other — the same
        // left-to-right sum: read / wait / add / write per element made this loop ~100 cycles per element, 11 us
        // of a 13 us kernel for the 256 block sums of a 524 288-particle CDF (rocprofv3 trace, round 5).
        T run = T(0);
        int k = 0;
        for (; k + 8 <= nt; k += 8) {
            T s[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = lds[k + j];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                lds[k + j] = run;
                run = run + s[j];
            }
        }
        for (; k < nt; ++k) {
            const T s = lds[k];
            lds[k] = run;
            run = run + s;
        }
        lds[nt] = run;
    }
    __syncthreads();
    T run = lds[t];
    for (int64_t i = b; i < e; ++i) {
        const T s = data[i];
        data[i] = run;
        run = run + s;
    }
    return lds[nt];
}

// Strided view of one particle's parameters: th(i) = particles[i*ld + p].
struct ParamRef {
    const double* base;
    int64_t ld;
    __device__ __forceinline__ double operator()(int i) const { return base[(int64_t)i * ld]; }
};

// (value, index) with np.argmax ordering: NaN beats everything, then larger value,
// ties -> lower index.
struct Best {
    double v;
    int64_t i;
};
__device__ __forceinline__ bool better(const Best& a, const Best& b) {
    const bool an = a.v != a.v, bn = b.v != b.v;
    if (an != bn) return an;
    if (an && bn) return a.i < b.i;
    if (a.v != b.v) return a.v > b.v;
    return a.i < b.i;
}

}  // namespace obe
