// Posterior summaries on the device: per-row min / max, weighted marginal and joint histograms, weighted quantiles.
//
// Every weight enters as the integer Q_i = rint(w_i * 2^k), 2^k a power of two chosen from sum(w) so that sum(Q) < 2^63
// (k = 62 for normalised weights).  Bins and cumulative sums are unsigned 64-bit integers, added with integer atomics
// (LDS per workgroup, then global): integer addition is associative, so masses and quantiles are the same bits from
// run to run, under any launch geometry and under any permutation of the cloud.
// NaN and negative weights count as zero.  Nothing here reads or writes anything but the caller's buffers.
#include <algorithm>

#include "obe_select.h"

namespace obe {
namespace {

constexpr int kPostHeader = 8;            // words: [0] sum w, [1] k, rest spare
constexpr int kLdsBins = 4096;            // 64-bit bins one workgroup keeps in LDS: 32 KiB
constexpr int64_t kMaxBins = (int64_t)1 << 24;      // per row / per joint histogram

// ---- workspace: header, partial sums, the row list, the q list, then the body of the call
struct PostWs {
    u64* hdr;
    double* partials;
    int32_t* rows;
    double* q;
    u64* body;
};
inline int64_t head_words(int64_t n_rows) { return kPostHeader + kPostPartials + (n_rows + 1) / 2 + kMaxQ; }
inline PostWs carve(void* d_ws, int64_t n_rows) {
    u64* base = static_cast<u64*>(d_ws);
    PostWs w;
    w.hdr = base;
    w.partials = reinterpret_cast<double*>(base + kPostHeader);
    w.rows = reinterpret_cast<int32_t*>(base + kPostHeader + kPostPartials);
    w.q = reinterpret_cast<double*>(base + kPostHeader + kPostPartials + (n_rows + 1) / 2);
    w.body = base + head_words(n_rows);
    return w;
}
inline int minmax_blocks(int64_t n) { return std::min(stream_blocks(n, kBlock * 8), 512); }

__device__ __forceinline__ u64 wave_min_u64(u64 v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const u64 t = __shfl_xor(v, o, kWave);
        v = t < v ? t : v;
    }
    return v;
}
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const u64 t = __shfl_xor(v, o, kWave);
        v = t > v ? t : v;
    }
    return v;
}

// The bin of x by the edges alone: edges[k] <= x < edges[k + 1], x == edges[nb] in the last bin, -1 outside / NaN.
// NumPy's index guess, checked against the edge array; a guess that is off is replaced by a binary search.
__device__ __forceinline__ int find_bin(double x, const double* __restrict__ e, int nb) {
    const double first = e[0], last = e[nb];
    if (!(x >= first && x <= last)) return -1;
    const double g = (x - first) * (double)nb / (last - first);
    int k = g >= (double)(nb - 1) ? nb - 1 : (g > 0.0 ? (int)g : 0);
    if (e[k] <= x && (k == nb - 1 || x < e[k + 1])) return k;
    int lo = 0, hi = nb - 1;                    // the largest k with e[k] <= x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (e[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- min / max per row: integer min / max of the sort keys (exact, any order)
__global__ __launch_bounds__(kBlock) void minmax_kernel(const double* __restrict__ p, int64_t ld, int64_t n,
                                                        const int32_t* __restrict__ rows, u64* __restrict__ keys) {
    __shared__ u64 s_min, s_max;
    if (threadIdx.x == 0) {
        s_min = ~(u64)0;
        s_max = 0;
    }
    __syncthreads();
    const double* x = p + (int64_t)rows[blockIdx.y] * ld;
    u64 mn = ~(u64)0, mx = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const u64 key = sort_key(x[i]);
        mn = key < mn ? key : mn;
        mx = key > mx ? key : mx;
    }
    mn = wave_min_u64(mn);
    mx = wave_max_u64(mx);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        atomicMin(&s_min, mn);
        atomicMax(&s_max, mx);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(&keys[2 * blockIdx.y], s_min);
        atomicMax(&keys[2 * blockIdx.y + 1], s_max);
    }
}

__global__ void minmax_init_kernel(u64* __restrict__ keys, int n_rows) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_rows) {
        keys[2 * r] = ~(u64)0;
        keys[2 * r + 1] = 0;
    }
}

// a NaN anywhere in the row makes both NaN (np.min / np.max propagate it)
__global__ void minmax_finish_kernel(const u64* __restrict__ keys, int n_rows, double* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_rows) {
        const double mx = key_value(keys[2 * r + 1]);
        out[2 * r] = mx != mx ? mx : key_value(keys[2 * r]);
        out[2 * r + 1] = mx;
    }
}

// ---- marginal histograms: grid (cloud chunks, row groups); LDS = rows of the group x bins, or none (global atomics)
template <bool LDS>
__global__ __launch_bounds__(kBlock) void hist_kernel(const double* __restrict__ p, int64_t ld, int64_t n,
                                                      const double* __restrict__ w, const int32_t* __restrict__ rows,
                                                      int n_rows, int rows_per_group, const double* __restrict__ edges,
                                                      int nb, const u64* __restrict__ hdr, u64* __restrict__ counts) {
    extern __shared__ u64 lds[];
    const int r0 = blockIdx.y * rows_per_group;
    const int r1 = r0 + rows_per_group < n_rows ? r0 + rows_per_group : n_rows;
    if (LDS) {
        for (int j = threadIdx.x; j < (r1 - r0) * nb; j += kBlock) lds[j] = 0;
        __syncthreads();
    }
    const int k = (int)(long long)hdr[1];
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += stride) {      // (uniform trip count per wave)
        const int64_t i = base + threadIdx.x;
        const u64 q = i < n ? weight_q(w[i], k) : 0;
        for (int r = r0; r < r1; ++r) {
            int bin = -1;
            if (q != 0) bin = find_bin(p[(int64_t)rows[r] * ld + i], edges + (int64_t)r * (nb + 1), nb);
            if (LDS) wave_add(lds + (r - r0) * nb, bin, q, bin >= 0);
            else wave_add(counts + (int64_t)r * nb, bin, q, bin >= 0);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int j = threadIdx.x; j < (r1 - r0) * nb; j += kBlock) {
            const u64 v = lds[j];
            if (v) atomicAdd(&counts[(int64_t)r0 * nb + j], v);
        }
    }
}

template <bool LDS>
__global__ __launch_bounds__(kBlock) void hist2d_kernel(const double* __restrict__ px, const double* __restrict__ py,
                                                        int64_t n, const double* __restrict__ w,
                                                        const double* __restrict__ xedges, int nbx,
                                                        const double* __restrict__ yedges, int nby,
                                                        const u64* __restrict__ hdr, u64* __restrict__ counts) {
    extern __shared__ u64 lds[];
    const int total = nbx * nby;
    if (LDS) {
        for (int j = threadIdx.x; j < total; j += kBlock) lds[j] = 0;
        __syncthreads();
    }
    const int k = (int)(long long)hdr[1];
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += stride) {
        const int64_t i = base + threadIdx.x;
        const u64 q = i < n ? weight_q(w[i], k) : 0;
        int bin = -1;
        if (q != 0) {
            const int bx = find_bin(px[i], xedges, nbx);
            const int by = bx >= 0 ? find_bin(py[i], yedges, nby) : -1;
            if (by >= 0) bin = bx * nby + by;
        }
        if (LDS) wave_add(lds, bin, q, bin >= 0);
        else wave_add(counts, bin, q, bin >= 0);
    }
    if (LDS) {
        __syncthreads();
        for (int j = threadIdx.x; j < total; j += kBlock) {
            const u64 v = lds[j];
            if (v) atomicAdd(&counts[j], v);
        }
    }
}

// mass = Q_bin 2^-k
__global__ __launch_bounds__(kBlock) void mass_kernel(const u64* __restrict__ counts, int64_t n, const u64* __restrict__ hdr,
                                                      double* __restrict__ mass) {
    const int k = (int)(long long)hdr[1];
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (int64_t)gridDim.x * kBlock)
        mass[j] = ldexp((double)counts[j], -k);
}

// ---- host side
int check_cloud(const char* who, const void* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                const int32_t* h_rows, int32_t n_rows, const void* d_ws) {
    static thread_local std::string msg;
    const char* what = nullptr;
    if (!d_particles || !h_rows || !d_ws) what = "null pointer";
    else if (n_particles < 1 || ld_p < n_particles) what = "bad cloud size";
    else if (n_dims < 1 || n_dims > OBE_CLOUD_MAX_DIMS || n_rows < 1 || n_rows > OBE_CLOUD_MAX_DIMS) what = "bad row count";
    else
        for (int r = 0; r < n_rows; ++r)
            if (h_rows[r] < 0 || h_rows[r] >= n_dims) what = "row index out of range";
    if (!what) return 0;
    msg = std::string(who) + ": " + what;
    return bad_arg(msg.c_str());
}

int enqueue_scale(const double* d_weights, int64_t n, const PostWs& ws, hipStream_t st) {
    const int nb = std::min(stream_blocks(n, kBlock * 8), kPostPartials);
    wsum_partial_kernel<<<nb, kBlock, 0, st>>>(d_weights, n, ws.partials);
    OBE_CHECK_LAUNCH("wsum_partial_kernel");
    scale_kernel<<<1, kBlock, 0, st>>>(ws.partials, nb, ws.hdr);
    OBE_CHECK_LAUNCH("scale_kernel");
    return 0;
}

}  // namespace
}  // namespace obe

using namespace obe;

extern "C" {

int64_t obe_posterior_workspace_bytes(int64_t n_particles, int32_t n_rows, int64_t n_bins, int32_t n_q) {
    (void)n_particles;
    if (n_rows < 1) n_rows = 1;
    if (n_bins < 0) n_bins = 0;
    if (n_q < 0) n_q = 0;
    if (n_q > kMaxQ) n_q = kMaxQ;
    int64_t body = 2 * (int64_t)n_rows;                                       // obe_minmax_rows
    body = std::max(body, (int64_t)n_rows * n_bins);                          // histogram counts
    body = std::max(body, (int64_t)n_rows * n_q * (kDigits + 2));             // digit histograms, prefixes, targets
    return (head_words(n_rows) + body) * (int64_t)sizeof(u64);
}

int obe_minmax_rows(const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles, const int32_t* h_rows,
                    int32_t n_rows, double* d_minmax, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_minmax) return bad_arg("obe_minmax_rows: null pointer");
    if (int rc = check_cloud("obe_minmax_rows", d_particles, ld_p, n_dims, n_particles, h_rows, n_rows, d_ws)) return rc;
    if (ws_bytes < obe_posterior_workspace_bytes(n_particles, n_rows, 0, 0)) return bad_arg("obe_minmax_rows: workspace too small");
    hipStream_t st = as_stream(stream);
    const PostWs ws = carve(d_ws, n_rows);
    OBE_HIP_TRY(hipMemcpyAsync(ws.rows, h_rows, sizeof(int32_t) * n_rows, hipMemcpyHostToDevice, st));
    minmax_init_kernel<<<(n_rows + kBlock - 1) / kBlock, kBlock, 0, st>>>(ws.body, n_rows);
    OBE_CHECK_LAUNCH("minmax_init_kernel");
    minmax_kernel<<<dim3(minmax_blocks(n_particles), n_rows), kBlock, 0, st>>>(d_particles, ld_p, n_particles, ws.rows, ws.body);
    OBE_CHECK_LAUNCH("minmax_kernel");
    minmax_finish_kernel<<<(n_rows + kBlock - 1) / kBlock, kBlock, 0, st>>>(ws.body, n_rows, d_minmax);
    OBE_CHECK_LAUNCH("minmax_finish_kernel");
    return 0;
}

int obe_weighted_histogram(const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                           const double* d_weights, const int32_t* h_rows, int32_t n_rows, const double* d_edges,
                           int64_t n_bins, double* d_mass, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_weights || !d_edges || !d_mass) return bad_arg("obe_weighted_histogram: null pointer");
    if (n_bins < 1) return bad_arg("obe_weighted_histogram: n_bins < 1");
    if (n_bins > kMaxBins) return bad_arg("obe_weighted_histogram: more than 2^24 bins per row");
    if (int rc = check_cloud("obe_weighted_histogram", d_particles, ld_p, n_dims, n_particles, h_rows, n_rows, d_ws)) return rc;
    if (ws_bytes < obe_posterior_workspace_bytes(n_particles, n_rows, n_bins, 0))
        return bad_arg("obe_weighted_histogram: workspace too small");
    hipStream_t st = as_stream(stream);
    const PostWs ws = carve(d_ws, n_rows);
    const int64_t total = (int64_t)n_rows * n_bins;
    const int nb = (int)n_bins;
    OBE_HIP_TRY(hipMemcpyAsync(ws.rows, h_rows, sizeof(int32_t) * n_rows, hipMemcpyHostToDevice, st));
    OBE_HIP_TRY(hipMemsetAsync(ws.body, 0, total * sizeof(u64), st));
    if (int rc = enqueue_scale(d_weights, n_particles, ws, st)) return rc;
    if (nb <= kLdsBins) {
        const int per_group = std::min((int)n_rows, kLdsBins / nb);
        const int groups = (n_rows + per_group - 1) / per_group;
        hist_kernel<true><<<dim3(cloud_blocks(n_particles), groups), kBlock, (size_t)per_group * nb * sizeof(u64), st>>>(
            d_particles, ld_p, n_particles, d_weights, ws.rows, n_rows, per_group, d_edges, nb, ws.hdr, ws.body);
    } else {
        const int per_group = std::min((int)n_rows, 8);
        const int groups = (n_rows + per_group - 1) / per_group;
        hist_kernel<false><<<dim3(cloud_blocks(n_particles), groups), kBlock, 0, st>>>(
            d_particles, ld_p, n_particles, d_weights, ws.rows, n_rows, per_group, d_edges, nb, ws.hdr, ws.body);
    }
    OBE_CHECK_LAUNCH("hist_kernel");
    mass_kernel<<<stream_blocks(total, kBlock), kBlock, 0, st>>>(ws.body, total, ws.hdr, d_mass);
    OBE_CHECK_LAUNCH("mass_kernel");
    return 0;
}

int obe_weighted_histogram2d(const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                             const double* d_weights, int32_t row_x, int32_t row_y, const double* d_xedges,
                             int64_t n_bins_x, const double* d_yedges, int64_t n_bins_y, double* d_mass, void* d_ws,
                             int64_t ws_bytes, void* stream) {
    if (!d_weights || !d_xedges || !d_yedges || !d_mass) return bad_arg("obe_weighted_histogram2d: null pointer");
    if (n_bins_x < 1 || n_bins_y < 1) return bad_arg("obe_weighted_histogram2d: n_bins < 1");
    if (n_bins_x > kMaxBins || n_bins_y > kMaxBins || n_bins_x * n_bins_y > kMaxBins)
        return bad_arg("obe_weighted_histogram2d: more than 2^24 bins");
    const int32_t rows[2] = {row_x, row_y};
    if (int rc = check_cloud("obe_weighted_histogram2d", d_particles, ld_p, n_dims, n_particles, rows, 2, d_ws)) return rc;
    const int64_t total = n_bins_x * n_bins_y;
    if (ws_bytes < obe_posterior_workspace_bytes(n_particles, 1, total, 0))
        return bad_arg("obe_weighted_histogram2d: workspace too small");
    hipStream_t st = as_stream(stream);
    const PostWs ws = carve(d_ws, 1);
    const double* px = d_particles + (int64_t)row_x * ld_p;
    const double* py = d_particles + (int64_t)row_y * ld_p;
    OBE_HIP_TRY(hipMemsetAsync(ws.body, 0, total * sizeof(u64), st));
    if (int rc = enqueue_scale(d_weights, n_particles, ws, st)) return rc;
    if (total <= kLdsBins)
        hist2d_kernel<true><<<cloud_blocks(n_particles), kBlock, (size_t)total * sizeof(u64), st>>>(
            px, py, n_particles, d_weights, d_xedges, (int)n_bins_x, d_yedges, (int)n_bins_y, ws.hdr, ws.body);
    else
        hist2d_kernel<false><<<cloud_blocks(n_particles), kBlock, 0, st>>>(
            px, py, n_particles, d_weights, d_xedges, (int)n_bins_x, d_yedges, (int)n_bins_y, ws.hdr, ws.body);
    OBE_CHECK_LAUNCH("hist2d_kernel");
    mass_kernel<<<stream_blocks(total, kBlock), kBlock, 0, st>>>(ws.body, total, ws.hdr, d_mass);
    OBE_CHECK_LAUNCH("mass_kernel");
    return 0;
}

int obe_weighted_quantiles(const double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles,
                           const double* d_weights, const int32_t* h_rows, int32_t n_rows, const double* h_q, int32_t n_q,
                           double* d_quantiles, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_weights || !h_q || !d_quantiles) return bad_arg("obe_weighted_quantiles: null pointer");
    if (n_q < 1 || n_q > kMaxQ) return bad_arg("obe_weighted_quantiles: 1..16 quantiles per call");
    for (int j = 0; j < n_q; ++j)
        if (!(h_q[j] >= 0.0 && h_q[j] <= 1.0)) return bad_arg("obe_weighted_quantiles: q outside [0, 1]");
    if (int rc = check_cloud("obe_weighted_quantiles", d_particles, ld_p, n_dims, n_particles, h_rows, n_rows, d_ws)) return rc;
    if (ws_bytes < obe_posterior_workspace_bytes(n_particles, n_rows, 0, n_q))
        return bad_arg("obe_weighted_quantiles: workspace too small");
    hipStream_t st = as_stream(stream);
    const PostWs ws = carve(d_ws, n_rows);
    const int64_t slots = (int64_t)n_rows * n_q;
    u64* hist = ws.body;
    u64* prefix = hist + slots * kDigits;
    u64* remaining = prefix + slots;
    OBE_HIP_TRY(hipMemcpyAsync(ws.rows, h_rows, sizeof(int32_t) * n_rows, hipMemcpyHostToDevice, st));
    OBE_HIP_TRY(hipMemcpyAsync(ws.q, h_q, sizeof(double) * n_q, hipMemcpyHostToDevice, st));
    OBE_HIP_TRY(hipMemsetAsync(hist, 0, slots * kDigits * sizeof(u64), st));
    if (int rc = enqueue_scale(d_weights, n_particles, ws, st)) return rc;
    for (int pass = 0; pass < kPasses; ++pass) {
        select_pass_kernel<<<dim3(cloud_blocks(n_particles), n_rows), kBlock, (size_t)n_q * kDigits * sizeof(u64), st>>>(
            d_particles, ld_p, n_particles, d_weights, ws.rows, n_q, pass, ws.hdr, prefix, hist);
        OBE_CHECK_LAUNCH("select_pass_kernel");
        select_choose_kernel<<<(int)slots, kWave, 0, st>>>(hist, n_q, ws.q, pass, prefix, remaining, d_quantiles);
        OBE_CHECK_LAUNCH("select_choose_kernel");
    }
    return 0;
}

}  // extern "C"
