// Parameter drift — the prediction step of the particle filter (extension: the reference's parameters are constants,
// its cloud moves only in the nudge of a resample, particlepdf.py:296-305).  K chosen rows of the (D, N) cloud do one
// step of a Gaussian random walk, in place:
//
//   x[rows[k], p] += sum_j z[p, j] G[k, j]        z (N, K) standard normals, G = sqrt(dt) L, L L^T = Q  (host)
//
// the same "cloud + normals x factor" as the nudge of resample_kernel (obe_resample.hip) without its gather: 8 K bytes
// of normals and 16 K bytes of cloud per particle, every access lane-contiguous.  Model-independent (no plugin source).
#include <cmath>

#include "obe_common.h"

namespace obe {

struct DriftArgs {
    double factor[kFastDims * kFastDims];   // G row-major (K x K)
    double lo[kFastDims], hi[kFastDims];    // REFLECT only: the interval of drifted row k (-inf / +inf: no bound)
    int rows[kFastDims];
};

// One reflection, no folding: a value that is still outside afterwards is the caller's mask's business.  Each
// operation is rounded on its own (the library is built with -ffp-contract=off); every comparison is false for NaN.
__device__ __forceinline__ double reflect_once(double v, double lo, double hi) {
    if (v < lo) {
        const double over = lo - v;
        v = lo + over;
    } else if (v > hi) {
        const double over = v - hi;
        v = hi - over;
    }
    return v;
}

// One thread per particle.  K is a template parameter so that the z row and the K drifted values live in registers,
// the K x K factor is read as wave-uniform kernel arguments and both loops unroll.  Rows that are not drifted are
// never addressed.
template <int K, bool REFLECT>
__global__ __launch_bounds__(kBlock) void drift_kernel(DriftArgs da, double* __restrict__ x, int64_t ld, int64_t n,
                                                       const double* __restrict__ z) {
    // the (N, K) row-major normals of a workgroup's 256 particles are one contiguous run: read it lane-contiguously
    // into LDS (a thread reading its own row makes every load touch 64 lines — resample_kernel).  In LDS a particle's
    // row starts every ROW doubles: the row reads below are 8-byte reads, 32 lanes to a group, the bank pair of a
    // double its index mod 32 — a stride of K doubles puts the lanes of a group on 32 / gcd(K, 32) of the bank pairs
    // (two, at K = 16), an odd stride on all of them, so an even K is padded by one double.
    constexpr int ROW = K | 1;
    auto slot = [](int e) { return (e / K) * ROW + e % K; };      // element e of the (256, K) tile
    __shared__ double zs[kBlock * ROW];
    for (int64_t p0 = (int64_t)blockIdx.x * kBlock; p0 < n; p0 += (int64_t)gridDim.x * kBlock) {
        const int64_t p = p0 + threadIdx.x;
        const int64_t run = (n - p0 < kBlock ? n - p0 : kBlock) * K;
        __syncthreads();       // the previous trip's rows have been consumed
        if (run == (int64_t)kBlock * K) {
            double t[K];       // a full tile: the K loads of a thread in flight together
#pragma unroll
            for (int j = 0; j < K; ++j) t[j] = z[p0 * K + threadIdx.x + j * kBlock];
#pragma unroll
            for (int j = 0; j < K; ++j) zs[slot(threadIdx.x + j * kBlock)] = t[j];
        } else {
            for (int64_t e = threadIdx.x; e < run; e += kBlock) zs[slot((int)e)] = z[p0 * K + e];
        }
        __syncthreads();
        if (p >= n) continue;
        double zr[K], x0[K];
#pragma unroll
        for (int j = 0; j < K; ++j) zr[j] = zs[threadIdx.x * ROW + j];
#pragma unroll
        for (int k = 0; k < K; ++k) x0[k] = x[(int64_t)da.rows[k] * ld + p];      // K independent loads in flight
#pragma unroll
        for (int k = 0; k < K; ++k) {
            // (z @ G.T)[p, k]: FMA chain from zero in j order, all K terms — the contract (include/obe_hip.h)
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j) s = fma(zr[j], da.factor[k * K + j], s);
            double v = x0[k] + s;
            if constexpr (REFLECT) v = reflect_once(v, da.lo[k], da.hi[k]);
            x[(int64_t)da.rows[k] * ld + p] = v;
        }
    }
}

}  // namespace obe

using namespace obe;

extern "C" {

int obe_drift_particles(double* d_particles, int64_t ld_p, int32_t n_dims, int64_t n_particles, const int32_t* h_rows,
                        const double* h_factor, int32_t n_rows, const double* d_normals, const double* h_lower,
                        const double* h_upper, void* stream) {
    if (!d_particles || !h_rows || !h_factor || !d_normals || n_particles <= 0)
        return bad_arg("obe_drift_particles: bad pointer/size");
    if (n_dims < 1 || n_dims > OBE_CLOUD_MAX_DIMS) return bad_arg("obe_drift_particles: n_dims must be 1..1024");
    if (n_rows < 1 || n_rows > kFastDims) return bad_arg("obe_drift_particles: n_rows must be 1..16 (OBE_FAST_DIMS)");
    if (ld_p < n_particles) return bad_arg("obe_drift_particles: ld_p < n_particles");
    if ((h_lower == nullptr) != (h_upper == nullptr))
        return bad_arg("obe_drift_particles: h_lower and h_upper go together (both, or both NULL)");
    DriftArgs da{};
    for (int k = 0; k < n_rows; ++k) {
        if (h_rows[k] < 0 || h_rows[k] >= n_dims) return bad_arg("obe_drift_particles: row index out of range");
        if (k > 0 && h_rows[k] <= h_rows[k - 1])
            return bad_arg("obe_drift_particles: rows must be ascending, each named once");
        da.rows[k] = h_rows[k];
    }
    for (int i = 0; i < n_rows * n_rows; ++i) {
        if (!std::isfinite(h_factor[i])) return bad_arg("obe_drift_particles: factor entry not finite");
        da.factor[i] = h_factor[i];
    }
    const bool reflect = h_lower != nullptr;
    for (int k = 0; reflect && k < n_rows; ++k) {
        if (h_lower[k] != h_lower[k] || h_upper[k] != h_upper[k]) return bad_arg("obe_drift_particles: NaN bound");
        if (h_lower[k] > h_upper[k]) return bad_arg("obe_drift_particles: lower > upper");
        da.lo[k] = h_lower[k];
        da.hi[k] = h_upper[k];
    }
    hipStream_t st = as_stream(stream);
    const int blocks = drift_blocks(n_particles);
    return dispatch_dims(n_rows, "obe_drift_particles: n_rows must be 1..16 (OBE_FAST_DIMS)", [&](auto K) -> int {
        constexpr int k = decltype(K)::value;
        if (reflect) drift_kernel<k, true><<<blocks, kBlock, 0, st>>>(da, d_particles, ld_p, n_particles, d_normals);
        else drift_kernel<k, false><<<blocks, kBlock, 0, st>>>(da, d_particles, ld_p, n_particles, d_normals);
        OBE_CHECK_LAUNCH("drift_kernel");
        return 0;
    });
}

}  // extern "C"
