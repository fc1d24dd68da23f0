// The records x particles pass, stated once: the joint log-likelihood of a set of records, per particle, for the
// Gaussian with a given sigma (K13a, obe_predict.hip) and for the classes whose likelihood is their own
// (obe_signal_noise.hip, obe_binomial.hip, obe_poisson.hip).
//   the plan      lane <-> particle, its M::NREAD rows held in registers (HeldParticle); the records are packed once per
//                 call into a table that is read with wave-uniform indices; grid = particle tiles x record chunks, at
//                 least kRecMinChunk records per chunk; the chunk partials are folded in chunk order
//                 (records_fold_kernel).  No atomics: the same bits from run to run, and a permuted cloud gives the
//                 permuted bits.
//   K13a          keeps its own pack and pass kernels (sum log sigma per chunk, noise rows of the cloud) and takes the
//                 plan, HeldParticle and the fold from here: the launches of obe_records_loglik are what they were.
//   the own-noise classes   share ONE pack kernel and ONE pass kernel, own_records_pack_kernel and own_records_kernel;
//                 a class gives its per-record term as a functor (Term, below) next to its likelihood kernel.
// Functor against restated scaffold (obe_cloud_pass.h records ten VGPRs lost to a functor in the information pass): here
// the compiler's report is the same either way.  A lane of this pass carries ONE running sum and a flag besides the
// held rows and Term::add is inlined into the channel loop: each class's pass restated by hand (scaffold and term in
// one kernel body) reports, for every built-in model, the VGPRs, SGPRs and occupancy of the functor's instantiation
// — one exception, the binomial term on FirstParam, 39 VGPRs against 35, eight waves per SIMD both — and 0 bytes of
// scratch throughout.  So the scaffold is stated once.
// Each source file gets its own copy of the kernels (anonymous namespace), as with obe_cloud_pass.h.
#pragma once

#include <algorithm>

#include "obe_models.h"

namespace obe {
namespace {

constexpr int kRecWaves = 8192;                    // waves a pass aims at (32 per CU): chunks = this / particle tiles
constexpr int kRecMinChunk = 32;                   // records per chunk at least

inline int rec_words_bound(int n_channels) { return OBE_MAX_SETDIMS + 2 * n_channels; }

inline int64_t particle_tiles(int64_t n_particles) { return (n_particles + kWave - 1) / kWave; }
inline int record_chunks(int64_t n_records, int64_t n_particles) {
    const int64_t by_size = (n_records + kRecMinChunk - 1) / kRecMinChunk;
    const int64_t by_grid = std::max<int64_t>(1, kRecWaves / particle_tiles(n_particles));
    return (int)std::max<int64_t>(1, std::min(by_size, by_grid));
}

// the table, one word per chunk (K13a: the chunk's sum log sigma; the own-noise classes: 0, or NaN where a record of
// the chunk cannot be one), the chunk partials: chunks x padded particles <= kRecWaves x 64 + the padded particles,
// whatever the number of records
inline int64_t records_pass_bytes(int64_t n_particles, int64_t n_records, int32_t n_channels) {
    if (n_particles < 1) n_particles = 1;
    if (n_records < 1) n_records = 1;
    n_channels = std::min(std::max(n_channels, 1), OBE_MAX_CHANNELS);
    return (n_records * rec_words_bound(n_channels) + kRecWaves
            + ((int64_t)kRecWaves + particle_tiles(n_particles)) * kWave) * (int64_t)sizeof(double);
}

// A particle's rows held in registers behind the interface of ParamRef: M::eval reads th(i) with constant i
template <class M>
struct HeldParticle {
    double v[M::NREAD];
    __device__ __forceinline__ void load(const double* __restrict__ particles, int64_t ld_p, int64_t p) {
#pragma unroll
        for (int k = 0; k < M::NREAD; ++k) v[k] = particles[(int64_t)k * ld_p + p];
    }
    __device__ __forceinline__ ParamRef ref() const { return ParamRef{v, 1}; }
};

// d_loglik (n,) [+]= (the chunk partials, added in chunk order) - constant
__global__ __launch_bounds__(kBlock) void records_fold_kernel(const double* __restrict__ partials, int chunks, int64_t n_pad,
                                                              int64_t n, double constant, int accumulate,
                                                              double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
    for (int j = 0; j < chunks; ++j) acc += partials[(int64_t)j * n_pad + i];
    acc -= constant;
    out[i] = accumulate ? out[i] + acc : acc;
}

// ---- the own-noise classes.  Term, a class's per-record term:
//   kSide                   rows of side data a record brings besides the reading (0 or 1)
//   Coef                    what the whole call brings, by value in the kernel arguments
//   pack(a, b, w0, w1)      a channel's reading a and side datum b (0.0 at kSide == 0) into the table's words w0 and,
//                           kSide == 1, w1; false: these cannot be a record
//   add(coef, c, f, w0, w1, acc, ok)   channel c of a record with the model value f: acc += the term, ok &= the
//                           particle's value is one the class takes.  w0 and w1 are the same for all lanes.
// A record of the table: the setting point (M::NS), w0 per channel and, kSide == 1, w1 per channel.
template <class M, class Term>
constexpr int own_rec_words() { return M::NS + (1 + Term::kSide) * M::NC; }

// table (n_records, own_rec_words) and chunk_mark[chunk] = 0, or NaN if a record of the chunk cannot be one.  One
// workgroup per chunk; the block sum has a fixed order.
template <class M, class Term>
__global__ __launch_bounds__(kBlock) void own_records_pack_kernel(const double* __restrict__ settings, int64_t ld_s,
                                                                  int64_t n_r, const double* __restrict__ reading,
                                                                  int64_t ld_a, const double* __restrict__ side,
                                                                  int64_t ld_b, int64_t chunk_len,
                                                                  double* __restrict__ table,
                                                                  double* __restrict__ chunk_mark) {
    __shared__ double red[kBlock / kWave];
    constexpr int W = own_rec_words<M, Term>();
    const int64_t r0 = (int64_t)blockIdx.x * chunk_len;
    const int64_t r1 = r0 + chunk_len < n_r ? r0 + chunk_len : n_r;
    double mark = 0.0;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += kBlock) {
        double* rec = table + r * W;
#pragma unroll
        for (int k = 0; k < M::NS; ++k) rec[k] = settings[(int64_t)k * ld_s + r];
#pragma unroll
        for (int c = 0; c < M::NC; ++c) {
            const double a = reading[(int64_t)c * ld_a + r];
            const double b = Term::kSide ? side[(int64_t)c * ld_b + r] : 0.0;
            double w0, w1 = 0.0;
            if (!Term::pack(a, b, w0, w1)) mark = __builtin_nan("");
            rec[M::NS + c] = w0;
            if (Term::kSide) rec[M::NS + M::NC + c] = w1;
        }
    }
    const double s = block_sum(mark, red);
    if (threadIdx.x == 0) chunk_mark[blockIdx.x] = s;
}

// partials (chunk, padded particles): the sum of the class's terms over the chunk's records and channels, in record
// order, for EVERY particle; NaN where the particle has a value the class does not take, or the chunk a marked record
template <class M, class Term>
__global__ __launch_bounds__(kWave) void own_records_kernel(obe_model m, const double* __restrict__ table, int64_t n_r,
                                                            int64_t chunk_len, const double* __restrict__ chunk_mark,
                                                            typename Term::Coef coef,
                                                            const double* __restrict__ particles, int64_t ld_p,
                                                            int64_t n, double* __restrict__ partials) {
    constexpr int W = own_rec_words<M, Term>();
    const int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t p = i < n ? i : n - 1;                         // (the padding lanes repeat the last particle)
    HeldParticle<M> held;
    held.load(particles, ld_p, p);
    const int64_t r0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t r1 = r0 + chunk_len < n_r ? r0 + chunk_len : n_r;
    double acc = 0.0;
    bool ok = true;
    for (int64_t r = r0; r < r1; ++r) {                          // (r and the record are the same for all lanes)
        const double* rec = table + r * W;
        double x[M::NS], y[M::NC];
#pragma unroll
        for (int k = 0; k < M::NS; ++k) x[k] = rec[k];
        M::eval(x, held.ref(), m, y);
#pragma unroll
        for (int c = 0; c < M::NC; ++c)
            Term::add(coef, c, y[c], rec[M::NS + c], Term::kSide ? rec[M::NS + M::NC + c] : 0.0, acc, ok);
    }
    double l = acc + chunk_mark[blockIdx.y];
    if (!ok) l = __builtin_nan("");
    partials[(int64_t)blockIdx.y * ((int64_t)gridDim.x * kWave) + i] = l;
}

// Everything that can refuse a call of an own-noise class's records entry point, then its launches.  `who` in front
// of each refusal; Term::kMaxChannels: the widest model the class takes.
template <class Term>
int own_records_loglik(const char* who, const obe_model* m, const double* d_settings, int64_t ld_s,
                       int64_t n_records, const double* d_reading, int64_t ld_a, const double* d_side, int64_t ld_b,
                       const typename Term::Coef& coef, double constant, const double* d_particles, int64_t ld_p,
                       int64_t n_particles, int32_t accumulate, double* d_loglik, void* d_ws, int64_t ws_bytes,
                       void* stream) {
    static thread_local std::string msg;
    auto refuse = [&](const char* what) {
        msg = std::string(who) + ": " + what;
        return bad_arg(msg.c_str());
    };
    if (!m || !d_settings || !d_reading || (Term::kSide && !d_side) || !d_particles || !d_loglik || !d_ws)
        return refuse("null pointer");
    if (n_records < 1 || ld_s < n_records || ld_a < n_records || (Term::kSide && ld_b < n_records))
        return refuse("n_records < 1 or a row of the records shorter than that");
    if (n_particles < 1 || ld_p < n_particles) return refuse("bad cloud size");
    if (!(constant - constant == 0.0)) return refuse("constant is not finite");
    if (m->n_channels > Term::kMaxChannels) return refuse("the model has more channels than this likelihood takes");
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    if (ws_bytes < records_pass_bytes(n_particles, n_records, mm.n_channels)) return refuse("workspace too small");
    const int64_t tiles = particle_tiles(n_particles);
    if (tiles > 0x7fffffff) return refuse("too many particles for one call");
    const int chunks = record_chunks(n_records, n_particles);
    const int64_t chunk_len = (n_records + chunks - 1) / chunks;
    const int used = (int)((n_records + chunk_len - 1) / chunk_len);
    hipStream_t st = as_stream(stream);
    double* table = static_cast<double*>(d_ws);
    double* chunk_mark = table + n_records * rec_words_bound(mm.n_channels);
    double* partials = chunk_mark + kRecWaves;
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        if constexpr (Model::NC > Term::kMaxChannels) {
            return refuse("the model has more channels than this likelihood takes");
        } else {
            own_records_pack_kernel<Model, Term><<<used, kBlock, 0, st>>>(d_settings, ld_s, n_records, d_reading, ld_a,
                                                                         d_side, ld_b, chunk_len, table, chunk_mark);
            OBE_CHECK_LAUNCH("own_records_pack_kernel");
            own_records_kernel<Model, Term><<<dim3((unsigned)tiles, (unsigned)used), kWave, 0, st>>>(
                mm, table, n_records, chunk_len, chunk_mark, coef, d_particles, ld_p, n_particles, partials);
            OBE_CHECK_LAUNCH("own_records_kernel");
            records_fold_kernel<<<(int)((n_particles + kBlock - 1) / kBlock), kBlock, 0, st>>>(
                partials, used, tiles * kWave, n_particles, -constant, accumulate != 0, d_loglik);
            OBE_CHECK_LAUNCH("records_fold_kernel");
            return 0;
        }
    });
}

}  // namespace
}  // namespace obe
