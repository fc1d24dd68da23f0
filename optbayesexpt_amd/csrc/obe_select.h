// The fixed-point weight, the order-preserving sort key and the radix-select pieces that the posterior summaries
// (obe_posterior.hip) and the posterior predictive summaries (obe_predict.hip) share.  Each source file gets its own
// copy of the kernels (anonymous namespace): a plugin library links obe_predict.hip without obe_posterior.hip.
#pragma once

#include <algorithm>

#include "obe_common.h"

namespace obe {
namespace {

typedef unsigned long long u64;

constexpr int kPostPartials = 1024;       // workgroups of the sum(w) pass (and slots for their partial sums)
constexpr int kMaxQ = 16;                 // quantiles per call (one digit histogram of 2 KiB each in LDS)
constexpr int kDigits = 256;              // radix select: 8 passes of 8 bits over the 64-bit key
constexpr int kPasses = 8;
constexpr int kAggregateFrom = 8;         // lanes of a wave that must share a bin before they are summed in registers

__device__ __forceinline__ u64 weight_q(double w, int k) {
    const double v = rint(ldexp(clean_weight(w), k));
    return v < 9.2e18 ? (u64)v : (u64)9200000000000000000ull;
}

// np.sort's order as an unsigned key: -0.0 == 0.0, every NaN last
__device__ __forceinline__ u64 sort_key(double x) {
    if (x != x) return ~(u64)0;
    u64 b = (u64)__double_as_longlong(x);
    if ((b << 1) == 0) b = 0;
    return (b >> 63) ? ~b : (b | ((u64)1 << 63));
}
__device__ __forceinline__ double key_value(u64 key) {
    const u64 b = (key >> 63) ? (key & ~((u64)1 << 63)) : ~key;
    return __longlong_as_double((long long)b);
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// hist[bin] += q for the active lanes.  EVERY lane of the wave calls it (shuffles inside).  A converged posterior puts
// all 64 lanes on one bin — and a radix-select pass over its leading digits always does —, which as 64 atomics on one
// address would be served one after the other: while at least kAggregateFrom of the lanes still to add share the bin
// of the first of them, that group is summed in registers and added once (at most four groups, then the rest singly).
template <class P>
__device__ __forceinline__ void wave_add(P hist, int bin, u64 q, bool active) {
    active = active && q != 0;
    u64 todo = __ballot(active);
    const int lane = threadIdx.x & (kWave - 1);
    for (int r = 0; r < 4 && todo; ++r) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lb = __shfl(bin, leader, kWave);
        const bool mine = active && bin == lb;
        const u64 same = __ballot(mine);
        if (__popcll(same) < kAggregateFrom) break;
        const u64 total = wave_sum_u64(mine ? q : 0);
        if (lane == leader) atomicAdd(&hist[lb], total);
        active = active && !mine;
        todo &= ~same;
    }
    if (active) atomicAdd(&hist[bin], q);
}

// ---- sum(w) in a fixed order, then the exponent
__global__ __launch_bounds__(kBlock) void wsum_partial_kernel(const double* __restrict__ w, int64_t n,
                                                              double* __restrict__ partials) {
    __shared__ double red[kBlock / kWave];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        s += clean_weight(w[i]);
    s = block_sum(s, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// k = 62 - e, e the smallest integer with sum(w) <= 2^e (1 + 2^-20): sum(Q) <= 2^62 (1 + 2^-20) + N / 2 < 2^63.  (The
// margin keeps a sum that is 1 to a few ulp, on either side, at k = 62.)
__global__ __launch_bounds__(kBlock) void scale_kernel(const double* __restrict__ partials, int nb, u64* __restrict__ hdr) {
    __shared__ double red[kBlock / kWave];
    const double s = block_sum_array(partials, nb, red);
    if (threadIdx.x == 0) {
        int e = 0;
        if (s > 0.0 && s <= kDblMax) {
            int ex;
            const double m = frexp(s, &ex);              // s = m 2^ex, 0.5 <= m < 1
            e = m <= 0.5 * (1.0 + 9.5367431640625e-07) ? ex - 1 : ex;
        }
        hdr[0] = (u64)__double_as_longlong(s);
        hdr[1] = (u64)(long long)(62 - e);
    }
}

inline int cloud_blocks(int64_t n) { return std::min(stream_blocks(n, kBlock * 4), 1024); }

// ---- quantiles: radix select on the sort key.  Pass t histograms digit t (from the top) of the keys that carry the
// digits chosen so far, once per requested q; grid (cloud chunks, rows), LDS = n_q x 256 bins.
__global__ __launch_bounds__(kBlock) void select_pass_kernel(const double* __restrict__ p, int64_t ld, int64_t n,
                                                             const double* __restrict__ w,
                                                             const int32_t* __restrict__ rows, int n_q, int pass,
                                                             const u64* __restrict__ hdr, const u64* __restrict__ prefix,
                                                             u64* __restrict__ hist) {
    extern __shared__ u64 lds[];
    __shared__ u64 pfx[kMaxQ];
    const int row = blockIdx.y;
    for (int j = threadIdx.x; j < n_q * kDigits; j += kBlock) lds[j] = 0;
    if ((int)threadIdx.x < n_q) pfx[threadIdx.x] = pass ? prefix[row * n_q + threadIdx.x] : 0;
    __syncthreads();
    const int k = (int)(long long)hdr[1];
    const int shift = 64 - 8 * (pass + 1);
    const double* x = p + (int64_t)rows[row] * ld;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += stride) {
        const int64_t i = base + threadIdx.x;
        const u64 q = i < n ? weight_q(w[i], k) : 0;
        u64 key = 0;
        if (q != 0) key = sort_key(x[i]);
        const int digit = (int)((key >> shift) & (kDigits - 1));
        const u64 high = pass ? key >> (shift + 8) : 0;
        for (int j = 0; j < n_q; ++j) wave_add(lds + j * kDigits, digit, q, high == pfx[j]);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < n_q * kDigits; j += kBlock) {
        const u64 v = lds[j];
        if (v) atomicAdd(&hist[(int64_t)row * n_q * kDigits + j], v);
    }
}


// Between two passes, one wave per (row, q): the smallest digit at which the cumulative sum reaches what is still
// wanted.  Pass 0 sees every particle, so its histogram's total is sum(Q), and the target is set there:
// max(1, ceil(q sum Q)) — at least 1, because np.quantile's inverted CDF starts at the first particle of non-zero
// cumulative weight.  Each lane owns four consecutive digits; their sums are scanned across the wave, the first lane
// whose inclusive sum reaches the target looks among its four.  The histogram is handed back zeroed.  The last pass
// writes the value.
__global__ __launch_bounds__(kWave) void select_choose_kernel(u64* __restrict__ hist, int n_q, const double* __restrict__ qs,
                                                              int pass, u64* __restrict__ prefix,
                                                              u64* __restrict__ remaining, double* __restrict__ out) {
    static_assert(kDigits == 4 * kWave, "four digits per lane");
    const int s = blockIdx.x, lane = threadIdx.x;
    u64* h = hist + (int64_t)s * kDigits + 4 * lane;
    u64 c[4], mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = h[j];
        h[j] = 0;
        mine += c[j];
    }
    u64 upto = mine;                                       // inclusive scan over the lanes
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const u64 t = __shfl_up(upto, o, kWave);
        if (lane >= o) upto += t;
    }
    const u64 total = __shfl(upto, kWave - 1, kWave);
    u64 want;
    if (pass == 0) {
        const double t = ceil(qs[s % n_q] * (double)total);
        want = t < 9.2e18 ? (u64)t : total;
        if (want > total) want = total;
        if (want < 1) want = 1;
    } else {
        want = remaining[s];
    }
    const u64 reached = __ballot(upto >= want);
    const int owner = reached ? __ffsll((long long)reached) - 1 : kWave - 1;      // (nobody: sum(Q) == 0, digit 255)
    if (lane != owner) return;
    u64 below = upto - mine;
    int digit = kDigits - 1;
    if (reached) {
#pragma unroll
        for (int j = 3; j >= 0; --j) {                     // the smallest j that reaches: scanned from the top down
            u64 b = upto - mine;
            for (int i = 0; i < j; ++i) b += c[i];
            if (b + c[j] >= want) {
                digit = 4 * lane + j;
                below = b;
            }
        }
    }
    const u64 chosen = ((pass ? prefix[s] : 0) << 8) | (u64)digit;
    prefix[s] = chosen;
    remaining[s] = want > below ? want - below : 0;
    if (pass == kPasses - 1) out[s] = key_value(chosen);
}

}  // namespace
}  // namespace obe
