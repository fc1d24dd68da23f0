// What the classes whose likelihood and noise variance are passes of their own share (obe_signal_noise.hip,
// obe_binomial.hip, obe_poisson.hip), stated once.
//   the pass        "lane <-> setting, particle chunks streamed, partials folded in chunk order": one wave per
//                   workgroup, the particle axis streamed (the same particle for all lanes: scalar loads), grid =
//                   setting tiles x particle chunks; what a lane sums is its class's Acc.  No atomics: the same bits
//                   from run to run.
//   the likelihood  what every record brings (channels, choke, setting) and how it is filled; the kernels themselves
//                   stay with their classes.
// Each source file gets its own copy of the kernels (anonymous namespace), as with obe_select.h.
#pragma once

#include <algorithm>

#include "obe_models.h"

namespace obe {
namespace {

constexpr int kPassMinChunk = 256;                 // particles per chunk at least

// ---- the launch plan of a pass.  waves: what the pass aims at; chunks = waves / setting tiles, at least one
struct CloudPassPlan {
    int64_t tiles;         // of kWave settings
    int64_t chunk_len;     // particles per chunk
    int used;              // chunks that are not empty: the grid's second dimension
    int64_t n_pad;         // padded settings, tiles x kWave
    dim3 grid() const { return dim3((unsigned)tiles, (unsigned)used); }
};
inline int64_t cloud_pass_tiles(int64_t n_settings) { return (n_settings + kWave - 1) / kWave; }
inline CloudPassPlan cloud_pass_plan(int64_t n_particles, int64_t n_settings, int waves) {
    CloudPassPlan plan;
    plan.tiles = cloud_pass_tiles(n_settings);
    const int64_t by_size = (n_particles + kPassMinChunk - 1) / kPassMinChunk;
    const int64_t by_grid = std::max<int64_t>(1, waves / plan.tiles);
    const int chunks = (int)std::max<int64_t>(1, std::min(by_size, by_grid));
    // whole waves of particles per chunk (the count of chunks that are not empty may then be smaller)
    plan.chunk_len = ((n_particles + chunks - 1) / chunks + kWave - 1) / kWave * kWave;
    plan.used = (int)((n_particles + plan.chunk_len - 1) / plan.chunk_len);
    plan.n_pad = plan.tiles * kWave;
    return plan;
}
// chunks x padded settings <= waves x 64 + the padded settings, whatever the cloud
inline int64_t cloud_pass_words(int64_t n_settings, int slots, int waves) {
    return ((int64_t)waves + cloud_pass_tiles(n_settings)) * kWave * slots;
}

// The refusals every entry point of a pass shares, `who` in front of each (0: none)
inline int cloud_pass_refusal(const char* who, int64_t n_settings, int64_t ld_s, int64_t n_particles, int64_t ld_p,
                              int64_t ws_bytes, int64_t ws_needed) {
    static thread_local std::string msg;
    const char* what = nullptr;
    if (n_settings < 1 || ld_s < n_settings) what = "n_settings < 1 or a row of settings shorter than that";
    else if (n_particles < 1 || ld_p < n_particles) what = "bad cloud size";
    else if (ws_bytes < ws_needed) what = "workspace too small";
    else if (cloud_pass_tiles(n_settings) > 0x7fffffff) what = "too many settings for one call";
    if (!what) return 0;
    msg = std::string(who) + ": " + what;
    return bad_arg(msg.c_str());
}

// partials (chunk, Acc::kSlots, padded settings): a lane's sums over the chunk's particles of weight > 0.
// Acc: the lane's sums, all zero when value-initialised — add(wp, y) for a particle of clean weight wp > 0 and model
// values y[M::NC], store(out, n_pad) with slot k at out[k * n_pad].
template <class M, class Acc>
__global__ __launch_bounds__(kWave) void cloud_pass_kernel(obe_model m, const double* __restrict__ settings,
                                                           int64_t ld_s, int64_t n_s,
                                                           const double* __restrict__ particles, int64_t ld_p,
                                                           int64_t n, const double* __restrict__ w, int64_t chunk_len,
                                                           double* __restrict__ partials) {
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const int64_t sc = s < n_s ? s : n_s - 1;                    // (the padding lanes repeat the last setting)
    double x[M::NS];
#pragma unroll
    for (int k = 0; k < M::NS; ++k) x[k] = settings[(int64_t)k * ld_s + sc];
    Acc acc{};
    const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
    const int64_t p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    for (int64_t p = p0; p < p1; ++p) {                          // (p, w[p] and the particle are the same for all lanes)
        const double wp = clean_weight(w[p]);
        if (wp == 0.0) continue;                                 // (whatever the model gives)
        double y[M::NC];
        M::eval(x, ParamRef{particles + p, ld_p}, m, y);
        acc.add(wp, y);
    }
    const int64_t n_pad = (int64_t)gridDim.x * kWave;
    acc.store(partials + (int64_t)blockIdx.y * Acc::kSlots * n_pad + s, n_pad);
}

// slot `slot` of setting s summed over the chunks, in chunk order (what the fold kernels start from)
__device__ __forceinline__ double chunk_order_sum(const double* __restrict__ partials, int chunks, int slots, int slot,
                                                  int64_t n_pad, int64_t s) {
    double sum = 0.0;
    for (int j = 0; j < chunks; ++j) sum += partials[((int64_t)j * slots + slot) * n_pad + s];
    return sum;
}

// ---- the likelihood of a record: what every record brings, the first member of each class's kernel argument (the
// kernels stay with their classes: their arithmetic moved into a function of a shared kernel costs registers)
struct LikHead {
    int n_ch;          // channels entering the product
    int use_choke;
    double choke;
    double x[OBE_MAX_SETDIMS];
};
// h_setting NULL: the model is evaluated at zeros (or not at all: given model values)
inline LikHead lik_head(const obe_model& mm, int n_lik_channels, double choke, const double* h_setting) {
    LikHead a{};
    a.n_ch = n_lik_channels;
    a.use_choke = choke == choke;                                // NaN: no choke
    a.choke = choke;
    for (int i = 0; i < mm.n_setdims && i < OBE_MAX_SETDIMS; ++i) a.x[i] = h_setting ? h_setting[i] : 0.0;
    return a;
}

}  // namespace
}  // namespace obe
