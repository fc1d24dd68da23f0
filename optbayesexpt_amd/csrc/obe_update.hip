// K2 — Bayes update of the particle weights, plus the model-evaluation wrappers and
// the OptBayesExptNoiseParameter constraint mask.  All HBM-bound streams:
//   pass A  read (D+1) rows, write t = nan_to_num(w * L), block partial sums of t
//   pass B  read t, write w' = nan_to_num(t / sum t), block partial sums of w'^2
//   pass C  one block folds the partials into two scalars
// Algorithmic traffic per particle: 8(D_read + 1) + 8 (A) + 16 (B) bytes.
// Reductions are fixed-order (no float atomics) so results are run-to-run identical.
// Measured alternative (round 1): folding the partials inside pass A / pass B by the last
// workgroup to arrive (atomicInc ticket) removes pass C and the per-block re-fold of pass B,
// but 2048 same-address device-scope atomics cost ~12 ns each across the 8 XCDs and an
// agent-scope release fence per workgroup writes back the 8 MB of weights just dirtied:
// 62-89 us per update instead of 21.7 us.  Separate launches win at this size.
// Also measured: all three passes in ONE workgroup for demo-size clouds (bit-identical by
// replaying the virtual workgroups' shuffle trees): 18 us per point at 5 000 particles and
// 100 us at 50 000 (one CU's bandwidth) against 15 us for the three launches at any size up to
// 1M — the launches are ~5 us each and already the floor; not kept.
#include "obe_models.h"
#include "obe_update.h"

namespace obe {

// pass A, model fused
// (round 4, measured and not kept: issuing the loads of 6 particles per thread together before their ~170
// dependent FP64 instructions each — 23.2 vs 23.0 us per update at 1 M particles, 17.4 vs 15.7 at 262 144:
// three waves per SIMD already hide the latency; t stored with __builtin_nontemporal_store so that the kernel
// boundary has less to write back: 21.8 vs 21.8-22.6 us at 1 M particles, 47.1 vs 50.2 us with 10 parameters)
template <class M>
__global__ __launch_bounds__(kBlock) void update_model_kernel(
    obe_model m, SettingArg st, LikArgs la, const double* __restrict__ particles, int64_t ld,
    int64_t n, double* __restrict__ weights, double* __restrict__ partials, SweepCtl ctl) {
    __shared__ double red[kBlock / kWave];
    if (sweep_prologue(ctl, red)) return;
    __syncthreads();
    double acc = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
        double y[M::NC];
        M::eval(st.x, ParamRef{particles + p, ld}, m, y);
        const double t = nan_to_num(weights[p] * likelihood_of(y, la, particles, ld, p));
        weights[p] = t;
        acc += t;
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// (round 5, measured and not kept: both passes in one launch behind a grid barrier — profiles/r05_update_moments.txt)

template <class M>
__global__ __launch_bounds__(kBlock) void eval_particles_kernel(obe_model m, SettingArg st,
                                                                const double* __restrict__ particles, int64_t ld,
                                                                int64_t n, double* __restrict__ out, int64_t ld_y) {
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
        double y[M::NC];
        M::eval(st.x, ParamRef{particles + p, ld}, m, y);
#pragma unroll
        for (int c = 0; c < M::NC; ++c) out[(int64_t)c * ld_y + p] = y[c];
    }
}

struct ParamArg {
    double th[OBE_MAX_DIMS];
};

template <class M>
__global__ __launch_bounds__(kBlock) void eval_settings_kernel(obe_model m, ParamArg pa,
                                                               const double* __restrict__ settings, int64_t ld_s,
                                                               int64_t n, double* __restrict__ out, int64_t ld_y) {
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += (int64_t)gridDim.x * kBlock) {
        double x[M::NS], y[M::NC];
#pragma unroll
        for (int k = 0; k < M::NS; ++k) x[k] = settings[(int64_t)k * ld_s + s];
        M::eval(x, ParamRef{pa.th, 1}, m, y);
#pragma unroll
        for (int c = 0; c < M::NC; ++c) out[(int64_t)c * ld_y + s] = y[c];
    }
}

// What the three model-update entry points share: prepare() = everything that can refuse the call, then pass A.
// Pass A multiplies the weights by the likelihood in place: a refusal after it would leave them half updated, and a
// caller that then falls back to another form would apply the likelihood twice — so prepare() comes before any launch.
struct ModelUpdate {
    obe_model mm;
    LikArgs la;
    UpdateWs w;
    int nb;
    // (with_moments: the partials of the fused first moments are carved too — mm.n_params of them, 1..OBE_FAST_DIMS)
    int prepare(const obe_model* m, const double* h_y_meas, const double* h_sigma, const int32_t* h_noise_rows,
                int32_t n_lik_channels, double choke, int64_t n_particles, void* d_ws, int64_t ws_bytes, bool with_moments) {
        mm = *m;
        if (int rc = obe_model_validate(&mm)) return rc;
        if (n_lik_channels > mm.n_channels) return bad_arg("n_lik_channels exceeds model channels");
        if (with_moments && (mm.n_params < 1 || mm.n_params > kFastDims))
            return bad_arg("obe_bayes_update_model_moments: n_params must be 1..16 (OBE_FAST_DIMS)");
        if (int rc = fill_lik_args(la, h_y_meas, h_sigma, h_noise_rows, n_lik_channels, choke, mm.n_params)) return rc;
        if (int rc = carve_update_ws(d_ws, ws_bytes, w, with_moments ? mm.n_params : 0)) return rc;
        nb = update_blocks(n_particles);
        return 0;
    }
    // h_setting: this point's setting, mm.n_setdims values (NULL: zeros)
    int pass_a(const double* h_setting, const double* d_particles, int64_t ld_p, int64_t n_particles, double* d_weights,
               const SweepCtl& ctl, hipStream_t st) const {
        SettingArg sa{};
        for (int k = 0; k < mm.n_setdims; ++k) sa.x[k] = h_setting ? h_setting[k] : 0.0;
        return dispatch_model(mm, [&](auto M) -> int {
            using Model = decltype(M);
            update_model_kernel<Model><<<nb, kBlock, 0, st>>>(mm, sa, la, d_particles, ld_p, n_particles, d_weights, w.pa,
                                                              ctl);
            OBE_CHECK_LAUNCH("update_model_kernel");
            return 0;
        });
    }
};

}  // namespace obe

using namespace obe;

extern "C" {

int obe_bayes_update_model(const obe_model* m, const double* d_particles, int64_t ld_p, int64_t n_particles,
                           double* d_weights, const double* h_setting, const double* h_y_meas,
                           const double* h_sigma, const int32_t* h_noise_rows, int32_t n_lik_channels,
                           double choke, void* d_ws, int64_t ws_bytes, double* h_out, void* stream) {
    if (!m || !d_particles || !d_weights || n_particles <= 0) return bad_arg("obe_bayes_update_model: bad pointer/size");
    ModelUpdate u;
    if (int rc = u.prepare(m, h_y_meas, h_sigma, h_noise_rows, n_lik_channels, choke, n_particles, d_ws, ws_bytes, false))
        return rc;
    hipStream_t st = as_stream(stream);
    if (int rc = u.pass_a(h_setting, d_particles, ld_p, n_particles, d_weights, SweepCtl{}, st)) return rc;
    return finish_update(u.w, u.nb, n_particles, d_weights, h_out, st);
}

static int update_model_moments(const obe_model* m, const double* d_particles, int64_t ld_p, int64_t n_particles,
                                double* d_weights, const double* h_setting, const double* h_y_meas,
                                const double* h_sigma, const int32_t* h_noise_rows, int32_t n_lik_channels,
                                double choke, double* d_moments, void* d_ws, int64_t ws_bytes, double* h_out,
                                void* stream, bool enqueue_only, int32_t auto_resample, double resample_threshold) {
    if (!m || !d_particles || !d_weights || !d_moments || n_particles <= 0)
        return bad_arg("obe_bayes_update_model_moments: bad pointer/size");
    ModelUpdate u;
    if (int rc = u.prepare(m, h_y_meas, h_sigma, h_noise_rows, n_lik_channels, choke, n_particles, d_ws, ws_bytes, true))
        return rc;
    const int d = u.mm.n_params;
    hipStream_t st = as_stream(stream);
    // [0] sum t, [1] sum w'^2, [2..) the K3 block's first moments, (enqueue form) the resample decision
    HostWords out(h_out, 2 + 2 + 4 * (int64_t)d + (enqueue_only ? 1 : 0));
    double* hv = out.view<double>();
    if (enqueue_only && !hv) return bad_arg("obe_bayes_update_model_moments_enqueue: h_out must be page-locked");
    // the fold rides in the normalisation launch (its last workgroup to arrive) unless there is no counter for this stream
    unsigned* counter = stream_control_words(st);
    if (enqueue_only && !counter) return bad_arg("obe_bayes_update_model_moments_enqueue: no control words for this stream");
    if (enqueue_only && ws_bytes < update_ws_bytes(d) + 16)
        return bad_arg("obe_bayes_update_model_moments_enqueue: the workspace needs 16 spare bytes at its end (OBE_WS_ABORT_WORD)");
    out.arm();      // every word of the result block is watched
    const UpdateFold fold{counter, u.w.scalars, d_moments, hv, enqueue_only ? ws_abort_word(d_ws, ws_bytes) : nullptr,
                          (double)n_particles, resample_threshold, auto_resample};
    if (int rc = u.pass_a(h_setting, d_particles, ld_p, n_particles, d_weights, SweepCtl{}, st)) return rc;
    if (int rc = launch_normalize_moments(d, u.w, u.nb, d_particles, ld_p, n_particles, d_weights, fold, st)) return rc;
    if (enqueue_only) return 0;      // armed, not waited for: the caller watches
    if (int rc = out.copy(0, 2, u.w.scalars, st)) return rc;
    if (int rc = out.copy(2, 2 + 4 * (int64_t)d, d_moments, st)) return rc;
    return out.wait(st);
}

int obe_bayes_update_model_moments(const obe_model* m, const double* d_particles, int64_t ld_p, int64_t n_particles,
                                   double* d_weights, const double* h_setting, const double* h_y_meas,
                                   const double* h_sigma, const int32_t* h_noise_rows, int32_t n_lik_channels,
                                   double choke, double* d_moments, void* d_ws, int64_t ws_bytes, double* h_out,
                                   void* stream) {
    return update_model_moments(m, d_particles, ld_p, n_particles, d_weights, h_setting, h_y_meas, h_sigma,
                                h_noise_rows, n_lik_channels, choke, d_moments, d_ws, ws_bytes, h_out, stream, false, 0,
                                0.0);
}

int obe_bayes_update_model_moments_enqueue(const obe_model* m, const double* d_particles, int64_t ld_p,
                                           int64_t n_particles, double* d_weights, const double* h_setting,
                                           const double* h_y_meas, const double* h_sigma,
                                           const int32_t* h_noise_rows, int32_t n_lik_channels, double choke,
                                           double* d_moments, void* d_ws, int64_t ws_bytes, double* h_pinned_out,
                                           int32_t auto_resample, double resample_threshold, void* stream) {
    if (!h_pinned_out) return bad_arg("obe_bayes_update_model_moments_enqueue: h_pinned_out is NULL");
    return update_model_moments(m, d_particles, ld_p, n_particles, d_weights, h_setting, h_y_meas, h_sigma,
                                h_noise_rows, n_lik_channels, choke, d_moments, d_ws, ws_bytes, h_pinned_out, stream,
                                true, auto_resample, resample_threshold);
}

int obe_bayes_update_sweep(const obe_model* m, const double* d_particles, int64_t ld_p, int64_t n_particles,
                           double* d_weights, const double* h_settings, const double* h_y_meas,
                           const double* h_sigma, const int32_t* h_noise_rows, int32_t n_lik_channels,
                           double choke, int64_t n_points, int32_t auto_resample, double resample_threshold,
                           void* d_ws, int64_t ws_bytes, double* h_out, void* stream) {
    if (!m || !d_particles || !d_weights || n_particles <= 0 || n_points <= 0 || !h_y_meas || !h_out)
        return bad_arg("obe_bayes_update_sweep: bad pointer/size");
    ModelUpdate u;
    if (int rc = u.prepare(m, h_y_meas, h_sigma, h_noise_rows, n_lik_channels, choke, n_particles, d_ws, ws_bytes, false))
        return rc;
    hipStream_t st = as_stream(stream);
    if (int rc = launch_sweep_reset(u.w, st)) return rc;
    // (obe_strict_sums: every point's sum t and sum w'^2 in np.sum's order, as the point-by-point calls form them)
    const bool strict = strict_sums_on();
    const int nfold = strict ? 1 : u.nb;
    for (int64_t k = 0; k < n_points; ++k) {
        // (the points differ in their measurement and setting only: what could refuse was checked with point 0's)
        for (int c = 0; c < u.la.n_ch; ++c) u.la.y_meas[c] = h_y_meas[k * OBE_MAX_CHANNELS + c];
        const SweepCtl ctl{u.w.scalars, u.w.pa, u.w.pb, nfold, (int)k, auto_resample, resample_threshold, (double)n_particles};
        if (int rc = u.pass_a(h_settings ? h_settings + k * OBE_MAX_SETDIMS : nullptr, d_particles, ld_p, n_particles,
                              d_weights, ctl, st))
            return rc;
        if (int rc = launch_sweep_point_tail(u.w, u.nb, nfold, n_particles, d_weights, strict, st)) return rc;
    }
    if (int rc = launch_sweep_end(u.w, nfold, n_particles, auto_resample, resample_threshold, (int)n_points, st)) return rc;
    OBE_HIP_TRY(hipMemcpyAsync(h_out, u.w.scalars, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    OBE_HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int obe_eval_over_particles(const obe_model* m, const double* d_particles, int64_t ld_p, int64_t n_particles,
                            const double* h_setting, double* d_y_out, int64_t ld_y, void* stream) {
    if (!m || !d_particles || !d_y_out || n_particles <= 0) return bad_arg("obe_eval_over_particles: bad pointer/size");
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    SettingArg sa{};
    for (int k = 0; k < mm.n_setdims; ++k) sa.x[k] = h_setting ? h_setting[k] : 0.0;
    hipStream_t st = as_stream(stream);
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        eval_particles_kernel<Model><<<stream_blocks(n_particles, kBlock), kBlock, 0, st>>>(
            mm, sa, d_particles, ld_p, n_particles, d_y_out, ld_y);
        OBE_CHECK_LAUNCH("eval_particles_kernel");
        return 0;
    });
}

int obe_eval_over_settings(const obe_model* m, const double* d_settings, int64_t ld_s, int64_t n_settings,
                           const double* h_params, double* d_y_out, int64_t ld_y, void* stream) {
    if (!m || !d_settings || !d_y_out || !h_params || n_settings <= 0) return bad_arg("obe_eval_over_settings: bad pointer/size");
    obe_model mm = *m;
    if (int rc = obe_model_validate(&mm)) return rc;
    ParamArg pa{};
    for (int i = 0; i < mm.n_params && i < OBE_MAX_DIMS; ++i) pa.th[i] = h_params[i];
    hipStream_t st = as_stream(stream);
    return dispatch_model(mm, [&](auto M) -> int {
        using Model = decltype(M);
        eval_settings_kernel<Model><<<stream_blocks(n_settings, kBlock), kBlock, 0, st>>>(
            mm, pa, d_settings, ld_s, n_settings, d_y_out, ld_y);
        OBE_CHECK_LAUNCH("eval_settings_kernel");
        return 0;
    });
}

}  // extern "C"
